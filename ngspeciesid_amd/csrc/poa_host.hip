// poa_host.hip - host drivers over the POA tile engine: the depth-tiled hierarchy and ngsid_poa_consensus (a13,a14); the polisher (polish_host.hip) runs
// its windows through run_hierarchy.  Mirrors oracle/ngsid_oracle_poa.c: run_hierarchy / ongsid_poa_consensus.
#include "poa_host.h"
#include <chrono>
#include <algorithm>
#include <memory>

namespace {

// weight of every base of a sequence that stands for w reads (capped like the tile consensuses of the upper levels)
__host__ __device__ inline int32_t poa_base_weight(uint64_t w) { return w > (1u << 20) ? (1 << 20) : w < 1 ? 1 : (int32_t)w; }

// A tile output as a sequence of the next level (oracle run_hierarchy): cw = the weight of the reads it stands for.  In a window (bb >= 0, wlen = its backbone length)
// a tile consensus is a layer like the reads it stands for, with span[0..1] = its first and last backbone position: global only if it spans the window with 1 % slack
// (racon).  wlen is a reference so that the device reads it only for a window.
__host__ __device__ inline PSeq poa_tile_pseq(const uint8_t* s, uint64_t cw, int32_t len, int mode, int bb, const int32_t& wlen, const int32_t* span)
{
    PSeq S; S.s = s; S.q = nullptr; S.len = len; S.uw = poa_base_weight(cw); S.cw = (uint32_t)(cw > 0xffffffffull ? 0xffffffffull : cw); S.mode = mode; S.a0 = 0; S.a1 = -1;
    if (bb >= 0) {
        const int offset = (int)(0.01 * (double)wlen), begin = span[0], end = span[1];
        if (end >= begin) { S.a0 = begin; S.a1 = end; S.mode = (begin < offset && end > wlen - offset) ? NGSID_POA_GLOBAL : NGSID_POA_SEMI; }
    }
    return S;
}

__global__ void k_make_pseq_reads(const uint8_t* seq, const uint8_t* qual, const uint64_t* off, uint64_t n, int mode, const uint32_t* weight, PSeq* out)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    PSeq S; S.s = seq + off[i]; S.q = qual ? qual + off[i] : nullptr; S.len = (int32_t)(off[i + 1] - off[i]); S.uw = 1; S.cw = 1; S.mode = mode; S.a0 = 0; S.a1 = -1;
    if (weight) {        // a sequence that stands for weight[i] reads (ngsid_poa_consensus_weighted): unit weights of that size, like the tile consensuses of the upper levels
        const uint32_t wv = weight[i]; S.q = nullptr; S.cw = wv; S.uw = poa_base_weight(wv);
    }
    out[i] = S;
}

// Tile lists of a level: the sequences of every unfinished unit in tiles of hp.D (poa_ntiles), unit after unit.  The host arrays are kept across levels and
// calls (a million entries per level; fresh allocations would page-fault every time).
struct TileLists {
    PinVec<uint32_t> job_off, seq_idx, job_unit; PinVec<int32_t> job_bb; PinVec<uint8_t> job_final /* tiles that end their unit (trim 3) */;
    uint32_t maxD, maxn; int maxbb; bool any_nobb;      // largest tile, largest unit, longest backbone (0 if none), a unit without a backbone
    uint32_t njobs() const { return (uint32_t)job_unit.size(); }
};
// unit_rec != null: per unit its sequence count | first tile | tile count (3 x units.size() entries).  Units without sequences are marked done.
void build_tiles(TileLists& T, std::vector<Unit>& units, const std::vector<int>& bb_len, int D, uint32_t* unit_rec)
{
    T.job_off.assign(1, 0); T.seq_idx.clear(); T.job_unit.clear(); T.job_bb.clear(); T.job_final.clear();
    T.maxD = 0; T.maxn = 0; T.maxbb = 0; T.any_nobb = false;
    { size_t tot = 0; for (const Unit& U : units) if (!U.done) tot += U.seqs.size(); T.seq_idx.reserve(tot); }
    const size_t nu = units.size();
    for (size_t u = 0; u < nu; ++u) {
        Unit& U = units[u];
        const uint32_t ncur = U.done ? 0u : (uint32_t)U.seqs.size(), job0 = T.njobs();
        if (ncur == 0) U.done = true;
        else {
            const uint32_t Dl = D > 0 ? (uint32_t)D : ncur, nt = poa_ntiles(ncur, Dl), base = (uint32_t)T.seq_idx.size();
            T.seq_idx.insert(T.seq_idx.end(), U.seqs.begin(), U.seqs.end());          // the unit's sequences in one block copy: its tiles are consecutive slices of it
            for (uint32_t t = 0; t < nt; ++t) {
                const uint32_t a = t * Dl, b = t + 1 == nt ? ncur : a + Dl;
                T.job_off.push_back(base + b); T.job_bb.push_back(U.bb); T.job_unit.push_back((uint32_t)u); T.job_final.push_back(nt == 1 ? 1 : 0);
                T.maxD = std::max(T.maxD, b - a);
            }
            if (U.bb >= 0) T.maxbb = std::max(T.maxbb, bb_len[U.bb]); else T.any_nobb = true;
            T.maxn = std::max(T.maxn, ncur);
        }
        if (unit_rec) { unit_rec[u] = ncur; unit_rec[nu + u] = job0; unit_rec[2 * nu + u] = T.njobs() - job0; }
    }
}
// the tile lists to the level buffers B (job_final with trim 3; job_unit for the device-driven levels)
int32_t upload_tiles(ngsid_ctx* ctx, const TileLists& T, ngsid_ctx::PoaLevelBufs& B, bool final_, bool unit)
{
    HIPCHK(ctx, B.job_off.reserve(T.job_off.size())); HIPCHK(ctx, B.seq_idx.reserve(T.seq_idx.size())); HIPCHK(ctx, B.job_bb.reserve(T.job_bb.size()));
    HIPCHK(ctx, hipMemcpyAsync(B.job_off.p, T.job_off.data(), 4 * T.job_off.size(), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(B.seq_idx.p, T.seq_idx.data(), 4 * T.seq_idx.size(), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(B.job_bb.p, T.job_bb.data(), 4 * T.job_bb.size(), hipMemcpyHostToDevice, ctx->stream));
    if (final_) { HIPCHK(ctx, B.job_final.reserve(T.job_final.size())); HIPCHK(ctx, hipMemcpyAsync(B.job_final.p, T.job_final.data(), T.job_final.size(), hipMemcpyHostToDevice, ctx->stream)); }
    if (unit) { HIPCHK(ctx, B.job_unit.reserve(T.job_unit.size())); HIPCHK(ctx, hipMemcpyAsync(B.job_unit.p, T.job_unit.data(), 4 * T.job_unit.size(), hipMemcpyHostToDevice, ctx->stream)); }
    return NGSID_OK;
}

// Launch geometry: graph capacity by the oracle rule for the longest first sequence or backbone L0 (at least the longest member Lm + 1, a multiple of 8), Lm rounded up to 16
PoaPlan poa_plan(const HierParams& hp, int L0, uint32_t Lm, bool sub)
{
    long long capV = (long long)L0 * (hp.node_cap > 0 ? hp.node_cap : 28) / 16; capV = std::max<long long>(capV, L0 + 64); capV = std::max<long long>(capV, (long long)Lm + 1);
    capV = (capV + 7) & ~7ll;
    PoaPlan P{};
    P.Vcap = (int)capV; P.Ecap = (int)(3 * capV / 2); P.Lmax = (int)((std::max<uint32_t>(Lm, 1) + 15) & ~15u);
    P.band0 = hp.band <= 64 ? 64 : (hp.band <= 128 ? 128 : 256); P.sub = sub;
    return P;
}

// the job set of a level's tiles in the level buffers ctx->poa_lv[level & 1]; flags: dropped, slot_overflow.  The caller says which tiles a launch runs (nrun, job_list, nrun_dev).
PoaJobSet level_jobs(ngsid_ctx* ctx, const HierParams& hp, const PoaPlan& P, int level, int slots, const PSeq* seqs, const PSeq* bbs, const uint32_t* seq_idx, uint32_t njobs, uint32_t* flags)
{
    const ngsid_ctx::PoaLevelBufs& B = ctx->poa_lv[level & 1];
    PoaJobSet J{};
    J.seqs = seqs; J.bbs = bbs; J.seq_idx = seq_idx; J.job_off = B.job_off.p; J.job_bb = B.job_bb.p; J.njobs = njobs;
    J.m = hp.m; J.n = hp.n; J.g = hp.g; J.Vcap = P.Vcap; J.Ecap = P.Ecap; J.Lmax = P.Lmax; J.D = slots; J.node_cap = hp.node_cap;
    J.trim_tiles = (hp.trim_tiles & 1) | ((level > 0 && (hp.trim_tiles & 1)) ? 2 : 0); J.job_final = (hp.trim_tiles & 4) ? B.job_final.p : nullptr;
    J.out = B.out.p; J.out_len = B.out_len.p; J.out_cw = B.out_cw.p; J.out_n = B.out_n.p; J.out_cov = (hp.want_cov || hp.trim_tiles) ? B.out_cov.p : nullptr; J.out_span = B.out_span.p;
    J.dropped = flags; J.slot_overflow = flags + 1;
    return J;
}

// Runs all units to completion.  level0: device PSeq array (nseq0 entries) whose max length is maxlen0;
// bbs: device backbone PSeqs (may be null), maxbb = longest backbone.
int32_t run_hierarchy_host(ngsid_ctx* ctx, const PSeq* d_level0, uint32_t maxlen0, const PSeq* d_bbs, const std::vector<int>& bb_len,
                           std::vector<Unit>& units, const HierParams& hp)
{
    const PSeq* cur = d_level0; uint32_t cur_maxlen = maxlen0;
    int slots_cap = 0;
    HostTimer ht(ctx->stream, "hierarchy");
    if (ctx->poa_ctr.n < 1) HIPCHK(ctx, ctx->poa_ctr.alloc(16));
    for (int level = 0;; ++level) {
        // ---- jobs of this level
        static thread_local TileLists T;
        build_tiles(T, units, bb_len, hp.D, nullptr);
        const uint32_t njobs = T.njobs(), maxD = T.maxD;
        if (njobs == 0) break;
        if (level == 0) ht.mark("L0 host job lists");
        // capacity (LDS sizing): the largest per-job capacity the oracle rule can produce; without a backbone the first member sets L0 (<= the longest member)
        PoaPlan plan = poa_plan(hp, std::max({1, T.maxbb, T.any_nobb ? (int)cur_maxlen : 0}), cur_maxlen, hp.sub && level == 0);
        { int32_t rc = poa_prepare(ctx, plan, njobs, hp.m, hp.g); if (rc) return rc; }
        const int capV = plan.Vcap;
        ngsid_ctx::PoaLevelBufs* Lv = &ctx->poa_lv[level & 1];      // level L+1 reads what level L wrote: two alternating, grow-only buffer sets
        DevBuf<uint32_t>& d_flags = Lv->flags;
        { int32_t rc = upload_tiles(ctx, T, *Lv, hp.trim_tiles & 4, false); if (rc) return rc; }
        HIPCHK(ctx, d_flags.reserve(4));
        int slots = slots_cap ? slots_cap : (int)std::min<uint32_t>(maxD, (uint32_t)std::max<long long>(1, ngsid_opt(ctx, "poa_out_slots", 4)));
        static thread_local PinVec<uint32_t> h_out_n; static thread_local PinVec<int32_t> h_out_len, h_out_span; static thread_local PinVec<uint64_t> h_out_cw;
        const bool need_cov = hp.want_cov || hp.trim_tiles;
        auto launch = [&](const PoaJobSet& J, int bw, bool redo) -> int32_t {
            HIPCHK(ctx, hipMemsetAsync(ctx->poa_ctr.p, 0, sizeof(uint32_t), ctx->stream));      // the work queue of every launch starts at its first tile
            return poa_launch(ctx, plan, J, bw, redo, ctx->poa_ctr.p, plan.sub);
        };
        for (;;) {      // retry with more output slots if a tile had to split more often than `slots`
            HIPCHK(ctx, Lv->out.reserve((size_t)njobs * slots * capV)); HIPCHK(ctx, Lv->out_len.reserve((size_t)njobs * slots)); HIPCHK(ctx, Lv->out_cw.reserve((size_t)njobs * slots)); HIPCHK(ctx, Lv->out_n.reserve(njobs)); HIPCHK(ctx, Lv->out_span.reserve((size_t)njobs * slots * 2));
            if (need_cov) HIPCHK(ctx, Lv->out_cov.reserve((size_t)njobs * slots * capV));
            HIPCHK(ctx, hipMemsetAsync(d_flags.p, 0, 16, ctx->stream));
            PoaJobSet J = level_jobs(ctx, hp, plan, level, slots, cur, d_bbs, Lv->seq_idx.p, njobs, d_flags.p);
            J.nrun = njobs;
            DevBuf<unsigned long long> d_ph; static const bool want_ph = getenv("NGSID_POA_PHASES") != nullptr;
            if (want_ph) { HIPCHK(ctx, d_ph.alloc(24 * 256)); HIPCHK(ctx, hipMemsetAsync(d_ph.p, 0, 192 * 256, ctx->stream)); J.phase_cycles = d_ph.p; J.phase_detail = atoi(getenv("NGSID_POA_PHASES")) >= 2; }
            if (level == 0) ht.mark("L0 alloc + upload");
            int32_t rc = launch(J, plan.band0, false); if (rc) return rc;
            if (level == 0) ht.mark("L0 kernel");
            uint32_t h_flags[4];
            h_out_n.resize(njobs); h_out_len.resize((size_t)njobs * slots); h_out_cw.resize((size_t)njobs * slots); h_out_span.resize((size_t)njobs * slots * 2);
            auto download = [&]() -> int32_t {
                HIPCHK(ctx, hipMemcpyAsync(h_flags, d_flags.p, 16, hipMemcpyDeviceToHost, ctx->stream));
                HIPCHK(ctx, hipMemcpyAsync(h_out_n.data(), Lv->out_n.p, 4ull * njobs, hipMemcpyDeviceToHost, ctx->stream));
                HIPCHK(ctx, hipMemcpyAsync(h_out_len.data(), Lv->out_len.p, 4ull * njobs * slots, hipMemcpyDeviceToHost, ctx->stream));
                HIPCHK(ctx, hipMemcpyAsync(h_out_cw.data(), Lv->out_cw.p, 8ull * njobs * slots, hipMemcpyDeviceToHost, ctx->stream));
                HIPCHK(ctx, hipMemcpyAsync(h_out_span.data(), Lv->out_span.p, 8ull * njobs * slots, hipMemcpyDeviceToHost, ctx->stream));
                HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
                return NGSID_OK;
            };
            rc = download(); if (rc) return rc;
            // band-edge check (oracle run_tile): tiles in which a traceback touched a clipped edge of its band run again, whole, with twice the band
            for (int bw = plan.band0; bw < 256 && !h_flags[1] && !h_flags[2];) {
                static thread_local PinVec<uint32_t> redo; redo.clear();
                for (uint32_t j = 0; j < njobs; ++j) if (h_out_n[j] & 0x80000000u) redo.push_back(j);
                if (redo.empty()) break;
                bw *= 2;
                HIPCHK(ctx, Lv->job_list.reserve(redo.size()));
                HIPCHK(ctx, hipMemcpyAsync(Lv->job_list.p, redo.data(), 4 * redo.size(), hipMemcpyHostToDevice, ctx->stream));
                J.job_list = Lv->job_list.p; J.nrun = (uint32_t)redo.size();
                rc = launch(J, bw, true); if (rc) return rc;
                rc = download(); if (rc) return rc;
                ctx->poa_redo_tiles += redo.size();
            }
            for (uint32_t j = 0; j < njobs; ++j) h_out_n[j] &= 0x7fffffffu;
            if (want_ph) { std::vector<unsigned long long> hs(24 * 256); HIPCHK(ctx, hipMemcpy(hs.data(), d_ph.p, 192 * 256, hipMemcpyDeviceToHost)); unsigned long long h[24] = {0}; for (int s_ = 0; s_ < 256; ++s_) for (int k_ = 0; k_ < 24; ++k_) h[k_] += hs[s_ * 24 + k_]; fprintf(stderr, "[ngsid poa phases, Mcycles] jobs %u prepass %.1f forward %.1f traceback %.1f update %.1f emit %.1f | rows %llu non-chain %llu | sums: bestv %llu bestpk %llu nnew %llu alnsum %llu outlen %llu | tb iters %llu reloads %llu reload Mcycles %.1f | emit backtrack %.1f | row kinds: tight %llu in %llu runs, chain %llu, near %llu, generic %llu | update: A %.1f S+D %.1f N %.1f\n", njobs, h[0] / 1e6, h[1] / 1e6, h[2] / 1e6, h[3] / 1e6, h[4] / 1e6, h[5], h[6], h[8], h[9], h[10], h[11], h[12], h[7], h[13], h[14] / 1e6, h[15] / 1e6, h[16], h[17], h[18], h[19], h[20], h[21] / 1e6, h[22] / 1e6, h[23] / 1e6); }
            if (h_flags[2]) NGSID_FAIL(ctx, NGSID_ERR_HIP, "internal: POA tile kernel loop guard tripped (code %u)", h_flags[2]);
            if (!h_flags[1]) break;
            if (slots >= (int)maxD) NGSID_FAIL(ctx, NGSID_ERR_HIP, "internal: POA output slot overflow at full depth");
            slots = (int)std::min<uint32_t>(maxD, (uint32_t)slots * 4); slots_cap = slots;
        }
        if (level == 0) ht.mark("L0 download");
        // ---- distribute outputs to units
        std::vector<std::vector<uint32_t>> outs(units.size());         // flat slot indices (job*slots + s) in job order
        for (uint32_t j = 0; j < njobs; ++j) for (uint32_t s = 0; s < h_out_n[j]; ++s) outs[T.job_unit[j]].push_back(j * (uint32_t)slots + s);
        static thread_local PinVec<PSeq> next; uint32_t next_maxlen = 0;
        { size_t tot = 0; for (uint32_t j = 0; j < njobs; ++j) tot += h_out_n[j]; next.clear(); next.reserve(tot); }
        for (size_t u = 0; u < units.size(); ++u) {
            Unit& U = units[u]; if (U.done) continue;
            const std::vector<uint32_t>& O = outs[u];
            const size_t ncur = U.seqs.size();
            int pick = -1;
            if (O.empty()) { U.done = true; continue; }
            if (O.size() == 1) pick = 0;
            else if (O.size() >= ncur) { pick = 0; for (size_t i = 1; i < O.size(); ++i) if (h_out_cw[O[i]] > h_out_cw[O[pick]]) pick = (int)i; }
            if (pick >= 0) {
                const uint32_t sl = O[pick]; const int len = h_out_len[sl];
                U.result.resize(len);
                if (len) HIPCHK(ctx, hipMemcpy(&U.result[0], Lv->out.p + (size_t)sl * capV, len, hipMemcpyDeviceToHost));
                if (hp.want_cov) { U.cov.resize(len); if (len) HIPCHK(ctx, hipMemcpy(U.cov.data(), Lv->out_cov.p + (size_t)sl * capV, 4ull * len, hipMemcpyDeviceToHost)); }
                U.has_result = true; U.done = true; continue;
            }
            U.seqs.clear();
            for (uint32_t sl : O) {
                const PSeq S = poa_tile_pseq(Lv->out.p + (size_t)sl * capV, h_out_cw[sl], h_out_len[sl], hp.upper_mode, U.bb, U.bb >= 0 ? bb_len[U.bb] : 0, &h_out_span[2 * (size_t)sl]);
                U.seqs.push_back((uint32_t)next.size()); next.push_back(S); next_maxlen = std::max<uint32_t>(next_maxlen, (uint32_t)S.len);
            }
        }
        if (level == 0) ht.mark("L0 distribute"); else { char lb[48]; snprintf(lb, sizeof lb, "level %d (%u tiles)", level, njobs); ht.mark(lb); }
        if (next.empty()) break;
        HIPCHK(ctx, Lv->seqs.reserve(sizeof(PSeq) * next.size()));
        HIPCHK(ctx, hipMemcpyAsync(Lv->seqs.p, next.data(), sizeof(PSeq) * next.size(), hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        cur = (const PSeq*)Lv->seqs.p; cur_maxlen = next_maxlen;
    }
    ht.mark("levels >= 1");
    return NGSID_OK;
}


// ------------------------------------------------------------------------------------------------------------------------------------
// Device-driven hierarchy (round 3).  The host-driven loop above synchronises after every level (flags, output counts, lengths, weights and
// spans come back, the host builds the next level's sequence / tile lists and uploads them): 4 - 5 ms of idle GPU per polishing iteration at
// 1 M reads, and the top levels are a string of millisecond launches with a round trip in between.  Here the level bookkeeping runs in small
// kernels on the same stream - band-edge redo lists, per-unit output scan, next-level sequence descriptors, next-level tile lists, results
// of finished units copied to an arena - and the tile kernels read their tile count from device memory.  The host enqueues all levels of a
// hierarchy at once and synchronises ONCE.  Same results as the host-driven loop (tests run both: ngsid_ctx_option "poa_host_levels").
// Anything the fixed launch geometry cannot hold (a tile with more outputs than `slots`, a tile consensus much longer than the longest input,
// more upper-level tiles than planned) sets a flag and the call is repeated by the host-driven loop.
enum { C_NJOBS = 0 /* 2 words: level parity */, C_NSEQ = 2, C_OVERFLOW = 3, C_RES_USED = 4, C_REDO_TOTAL = 5, C_FLAGS = 8 /* dropped, slot_overflow (2 words) */, C_REDO = 16 /* + 2 * level + stage */, C_MAXLV = 48, C_WORK = C_REDO + 2 * C_MAXLV /* + 3 * level + instance */, C_WORDS = C_WORK + 3 * C_MAXLV };

struct HierDev {
    uint32_t U; int D, slots, capV, upper_mode, want_cov, Lmax, keep_final; uint32_t cap_jobs[2];
    const int32_t* unit_bb; const int32_t* unit_wlen;
    uint32_t* unit_ncur; uint32_t* unit_job0[2]; uint32_t* unit_njobs[2]; uint32_t* unit_seq0; int32_t* unit_pick; uint32_t* unit_tmp /* njobs_next, nseq_next, res_len of this level: 3 U */;
    uint32_t* res_off; int32_t* res_len; uint8_t* res; uint32_t* res_cov;
    uint32_t* ctrl;
};
struct LevelDev { PSeq* seqs; uint8_t* out; int32_t* out_len; int32_t* out_span; uint64_t* out_cw; uint32_t* out_n; uint32_t* out_cov; uint32_t* job_off; int32_t* job_bb; uint32_t* job_unit; uint32_t* job_pos; uint32_t* job_list; uint8_t* job_final; };

// tiles whose traceback touched a clipped band edge (bit 31 of out_n) -> list for the launch with twice the band
__global__ __launch_bounds__(256) void k_poa_redo_list(const uint32_t* __restrict__ out_n, const uint32_t* __restrict__ njobs, uint32_t* __restrict__ list, uint32_t* __restrict__ cnt, uint32_t* __restrict__ total)
{
    const uint32_t n = *njobs; const int lane = threadIdx.x & 63;
    for (uint32_t j0 = blockIdx.x * blockDim.x; j0 < n; j0 += gridDim.x * blockDim.x) {
        const uint32_t j = j0 + threadIdx.x;
        const bool f = j < n && (out_n[j] & 0x80000000u);
        const unsigned long long m = __ballot(f);
        if (!m) continue;
        const int leader = __ffsll((long long)m) - 1;
        uint32_t base = 0; if (lane == leader) { base = atomicAdd(cnt, (uint32_t)__popcll(m)); atomicAdd(total, (uint32_t)__popcll(m)); }
        base = __shfl(base, leader);
        if (f) list[base + __popcll(m & ((1ull << lane) - 1))] = j;
    }
}

__device__ __forceinline__ uint32_t block_excl_scan_256(uint32_t v, uint32_t* sm /* 8 words */, uint32_t& total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t y = __shfl_up(x, d); if (lane >= d) x += y; }
    __syncthreads();
    if (lane == 63) sm[w] = x;
    __syncthreads();
    uint32_t off = 0; for (int k = 0; k < w; ++k) off += sm[k];
    total = sm[0] + sm[1] + sm[2] + sm[3];
    return off + x - v;
}

// one workgroup per unit: output count of the level, position of every tile's outputs among them, fate of the unit
//   pick: -3 = was finished before, -2 = goes on, -1 = finishes without a result, >= 0 = finishes with the output in that slot
__global__ __launch_bounds__(256) void k_poa_unit_scan(HierDev H, LevelDev Lv, int par)
{
    __shared__ uint32_t sm[8]; __shared__ unsigned long long best_s[4]; __shared__ uint32_t one_slot;
    const uint32_t u = blockIdx.x; if (u >= H.U || H.ctrl[C_OVERFLOW]) return;
    const uint32_t j0 = H.unit_job0[par][u], nj = H.unit_njobs[par][u];
    uint32_t* tmp = H.unit_tmp + 3ull * u;
    if (nj == 0) {        // finished at an earlier level, or empty from the start
        if (threadIdx.x == 0) { if (H.unit_pick[u] == -2) H.unit_pick[u] = -1; else if (H.unit_pick[u] >= 0 || H.unit_pick[u] == -1) H.unit_pick[u] = -3; tmp[0] = 0; tmp[1] = 0; tmp[2] = 0; }
        return;
    }
    if (threadIdx.x == 0) one_slot = 0xffffffffu;
    __syncthreads();
    uint32_t running = 0;
    for (uint32_t b = 0; b < nj; b += 256) {
        const uint32_t x = b + threadIdx.x; const uint32_t j = j0 + x;
        const uint32_t c = x < nj ? (Lv.out_n[j] & 0x7fffffffu) : 0u;
        uint32_t tot; const uint32_t ex = block_excl_scan_256(c, sm, tot);
        if (x < nj) Lv.job_pos[j] = running + ex;
        if (c) one_slot = j * (uint32_t)H.slots;                  // only read when the unit has exactly one output
        running += tot;
        __syncthreads();
    }
    const uint32_t T = running, ncur = H.unit_ncur[u];
    int pick = -2;
    if (T == 0) pick = -1;
    else if (T == 1) { __syncthreads(); pick = (int)one_slot; }
    else if (T >= ncur) {        // no reduction: the output that stands for most reads wins, the first of them on ties (host loop: strictly greater replaces)
        unsigned long long best = 0ull;      // (cw + 1 capped to 40 bits) << 24 | (0xFFFFFF - order): larger weight first, then the earlier output
        uint32_t bslot = 0;
        for (uint32_t x = threadIdx.x; x < nj; x += 256) {
            const uint32_t j = j0 + x; const uint32_t c = Lv.out_n[j] & 0x7fffffffu; const uint32_t pos = Lv.job_pos[j];
            for (uint32_t sidx = 0; sidx < c; ++sidx) {
                unsigned long long cw = Lv.out_cw[(size_t)j * H.slots + sidx]; if (cw > 0xFFFFFFFFFEull) cw = 0xFFFFFFFFFEull;
                const unsigned long long key = ((cw + 1) << 24) | (unsigned long long)(0xFFFFFFu - ((pos + sidx) & 0xFFFFFFu));
                if (key > best) { best = key; bslot = j * (uint32_t)H.slots + sidx; }
            }
        }
        // block arg-max (keys are unique: the order is part of the key)
        unsigned long long kb = best; uint32_t sb = bslot;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { const unsigned long long ok = __shfl_xor(kb, d); const uint32_t os = __shfl_xor(sb, d); if (ok > kb) { kb = ok; sb = os; } }
        if ((threadIdx.x & 63) == 0) { best_s[threadIdx.x >> 6] = kb; sm[4 + (threadIdx.x >> 6)] = sb; }
        __syncthreads();
        unsigned long long kk = 0ull; uint32_t ss = 0; for (int k = 0; k < 4; ++k) if (best_s[k] > kk) { kk = best_s[k]; ss = sm[4 + k]; }
        pick = (int)ss;
    }
    if (threadIdx.x == 0) {
        H.unit_pick[u] = pick;
        if (pick == -2) { H.unit_ncur[u] = T; tmp[0] = H.D > 0 ? poa_ntiles(T, (uint32_t)H.D) : 1u; tmp[1] = T; tmp[2] = 0; }
        else { tmp[0] = 0; tmp[1] = 0; tmp[2] = pick >= 0 ? (uint32_t)Lv.out_len[pick] : 0u; }
    }
}

// one workgroup: prefix sums over the units -> first tile / first sequence of every unit at the next level, arena offsets of the results
__global__ __launch_bounds__(1024) void k_poa_unit_offsets(HierDev H, int par)
{
    __shared__ uint32_t wsum[3][16]; __shared__ uint32_t carry[3];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (H.ctrl[C_OVERFLOW]) { if (threadIdx.x == 0) H.ctrl[C_NJOBS + (par ^ 1)] = 0; return; }
    if (threadIdx.x < 3) carry[threadIdx.x] = threadIdx.x == 2 ? H.ctrl[C_RES_USED] : 0u;
    __syncthreads();
    for (uint32_t b = 0; b < H.U; b += 1024) {
        const uint32_t u = b + threadIdx.x; uint32_t v[3] = {0, 0, 0};
        if (u < H.U) { v[0] = H.unit_tmp[3ull * u]; v[1] = H.unit_tmp[3ull * u + 1]; v[2] = H.unit_tmp[3ull * u + 2]; }
        uint32_t x[3] = {v[0], v[1], v[2]};
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) for (int k = 0; k < 3; ++k) { const uint32_t y = __shfl_up(x[k], d); if (lane >= d) x[k] += y; }
        if (lane == 63) for (int k = 0; k < 3; ++k) wsum[k][w] = x[k];
        __syncthreads();
        uint32_t off[3], tot[3];
        for (int k = 0; k < 3; ++k) { off[k] = carry[k]; for (int q = 0; q < w; ++q) off[k] += wsum[k][q]; tot[k] = 0; for (int q = 0; q < 16; ++q) tot[k] += wsum[k][q]; }
        if (u < H.U) {
            H.unit_job0[par ^ 1][u] = off[0] + x[0] - v[0]; H.unit_njobs[par ^ 1][u] = v[0];
            H.unit_seq0[u] = off[1] + x[1] - v[1];
            if (H.unit_pick[u] >= 0) H.res_off[u] = off[2] + x[2] - v[2];
        }
        __syncthreads();
        if (threadIdx.x < 3) carry[threadIdx.x] += tot[threadIdx.x];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const uint32_t nj = carry[0], ns = carry[1];
        H.unit_job0[par ^ 1][H.U] = nj;
        H.ctrl[C_RES_USED] = carry[2];
        bool ovf = nj > H.cap_jobs[par ^ 1] || ns > H.cap_jobs[par] * (uint32_t)H.slots || H.ctrl[C_OVERFLOW] != 0 || H.ctrl[C_FLAGS + 1] != 0 || H.ctrl[C_FLAGS + 2] != 0;
        if (ovf) H.ctrl[C_OVERFLOW] = 1;
        H.ctrl[C_NJOBS + (par ^ 1)] = ovf ? 0u : nj; H.ctrl[C_NSEQ] = ns;
    }
}

// one wave per tile of the level: its outputs become sequences of the next level (units that go on) or the unit's result (copied to the arena)
__global__ __launch_bounds__(256) void k_poa_fill_next(HierDev H, LevelDev Lv, int par)
{
    const int lane = threadIdx.x & 63;
    const uint32_t njobs = H.ctrl[C_NJOBS + par];
    if (H.ctrl[C_OVERFLOW]) return;
    for (uint32_t j = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); j < njobs; j += gridDim.x * (blockDim.x >> 6)) {
    const uint32_t u = Lv.job_unit[j]; const int pick = H.unit_pick[u];
    const uint32_t n = Lv.out_n[j] & 0x7fffffffu;
    if (pick == -2) {
        if ((uint32_t)lane < n) {
            const size_t sl = (size_t)j * H.slots + lane;
            const PSeq S = poa_tile_pseq(Lv.out + sl * (size_t)H.capV, Lv.out_cw[sl], Lv.out_len[sl], H.upper_mode, H.unit_bb[u], H.unit_wlen[u], Lv.out_span + 2 * sl);
            if (S.len > H.Lmax) atomicExch(&H.ctrl[C_OVERFLOW], 1u);       // longer than the launch geometry was planned for: the host-driven loop takes over
            Lv.seqs[H.unit_seq0[u] + Lv.job_pos[j] + (uint32_t)lane] = S;
        }
    } else if (pick >= 0 && (uint32_t)pick / (uint32_t)H.slots == j) {
        const int len = Lv.out_len[pick]; const uint8_t* src = Lv.out + (size_t)pick * H.capV; uint8_t* dst = H.res + H.res_off[u];
        for (int x = lane; x < len; x += 64) dst[x] = src[x];
        if (H.want_cov) { const uint32_t* cs = Lv.out_cov + (size_t)pick * H.capV; uint32_t* cd = H.res_cov + H.res_off[u]; for (int x = lane; x < len; x += 64) cd[x] = cs[x]; }
        if (lane == 0) H.res_len[u] = len;
    }
    }
}

// tile lists of the next level: tile t of a unit takes its sequences [t D, (t + 1) D)
__global__ __launch_bounds__(256) void k_poa_fill_jobs(HierDev H, LevelDev Nx, int par /* of the level just done */)
{
    const uint32_t nj = H.ctrl[C_NJOBS + (par ^ 1)];
    if (H.ctrl[C_OVERFLOW]) return;
    const uint32_t* j0 = H.unit_job0[par ^ 1];
    for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < nj; t += gridDim.x * blockDim.x) {
    uint32_t lo = 0, hi = H.U;                 // last unit whose first tile is <= t (units without tiles share the first tile of their successor and come before it)
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (j0[mid] <= t) lo = mid; else hi = mid; }
    const uint32_t u = lo, tl = t - j0[u];
    const uint32_t T = H.unit_ncur[u]; const uint32_t Dl = H.D > 0 ? (uint32_t)H.D : T;
    Nx.job_off[t] = H.unit_seq0[u] + tl * Dl; Nx.job_bb[t] = H.unit_bb[u]; Nx.job_unit[t] = u;
    if (H.keep_final) Nx.job_final[t] = H.unit_njobs[par ^ 1][u] == 1 ? 1 : 0;            // (trim 3: the tile that ends its unit)
    if (t == nj - 1) Nx.job_off[nj] = H.ctrl[C_NSEQ];
    }
}


// returns NGSID_OK with *done = true when the device-driven hierarchy ran to completion; *done = false: nothing was changed, use the host-driven loop
int32_t run_hierarchy_dev(ngsid_ctx* ctx, const PSeq* d_level0, uint32_t maxlen0, const PSeq* d_bbs, const std::vector<int>& bb_len,
                          std::vector<Unit>& units, const HierParams& hp, bool* done)
{
    *done = false;
    static const bool want_ph = getenv("NGSID_POA_PHASES") != nullptr;       // the phase counters are read per level by the host-driven loop
    if (want_ph || ngsid_opt(ctx, "poa_host_levels", 0) || units.empty()) return NGSID_OK;
    const uint32_t U = (uint32_t)units.size();
    HostTimer ht(ctx->stream, "hierarchy (device levels)");
    // ---- level-0 tile lists (as in the host-driven loop) + per-unit records
    static thread_local TileLists T; static thread_local PinVec<uint32_t> u_u32; static thread_local PinVec<int32_t> u_i32;
    u_u32.assign(3ull * U, 0); u_i32.assign(3ull * U, 0);        // ncur | job0 | njobs   and   bb | wlen | pick
    build_tiles(T, units, bb_len, hp.D, u_u32.data());
    for (uint32_t u = 0; u < U; ++u) { const int bb = units[u].bb; u_i32[u] = bb; u_i32[U + u] = bb >= 0 ? bb_len[bb] : 0; u_i32[2ull * U + u] = -2; }
    const uint32_t njobs0 = T.njobs(), maxD = T.maxD; const uint64_t maxn = T.maxn;
    if (njobs0 == 0) return NGSID_OK;
    // ---- one launch geometry for all levels: members of the upper levels are tile consensus sequences, planned for up to 5/4 of the longest input
    const int Lb = std::max<int>((int)maxlen0, T.maxbb), Lb2 = Lb + Lb / 4 + 16;
    PoaPlan plan = poa_plan(hp, std::max(T.maxbb, T.any_nobb ? Lb2 : 1), (uint32_t)Lb2, hp.sub);
    if (poa_check_limits(nullptr, plan, hp.m, hp.g)) return NGSID_OK;      // the host loop reports what is wrong (or fits where this margin does not)
    const int band0 = plan.band0; const long long capV = plan.Vcap;
    const int slots = (int)std::min<uint32_t>(maxD, (uint32_t)std::max<long long>(1, ngsid_opt(ctx, "poa_out_slots", 4)));      // output slots per tile of the first attempt (a tile that closes its graph more often falls back to the host-driven loop, which retries with more)
    // levels the LARGEST unit needs when every tile returns one consensus (the tile counts of poa_ntiles, level by level).  Round 6: exactly that many are enqueued before the first
    // synchronisation (it used to be two more - an off-by-one and a spare - i.e. 2 x 9 empty dispatches per hierarchy); a tile that closes its graph early and returns two
    // sequences can make a unit need one level more: the loop below then enqueues three more after looking at the counters.
    int levels_est = 0; { uint64_t n = maxn; const uint32_t Dd = hp.D > 0 ? (uint32_t)hp.D : (uint32_t)std::min<uint64_t>(maxn, 0xffffffffull); while (n > 1 && levels_est < C_MAXLV - 4) { n = poa_ntiles((uint32_t)n, std::max<uint32_t>(Dd, 2u)); ++levels_est; } }
    levels_est = std::min(std::max(levels_est, 1), C_MAXLV - 2);
    uint32_t cap[2]; cap[0] = njobs0;
    { const uint64_t e1 = hp.D > 0 ? (njobs0 + (uint64_t)hp.D - 1) / (uint64_t)hp.D * (uint64_t)slots + U : U; cap[1] = (uint32_t)std::min<uint64_t>(njobs0, e1 + e1 / 4 + 1024); }
    { int32_t rc = poa_prepare(ctx, plan, njobs0, hp.m, hp.g); if (rc) return rc; }
    // ---- buffers
    const bool need_cov = hp.want_cov || hp.trim_tiles;
    LevelDev L[2];
    for (int q = 0; q < 2; ++q) {
        ngsid_ctx::PoaLevelBufs* B = &ctx->poa_lv[q]; const size_t ns = (size_t)cap[q] * slots;
        HIPCHK(ctx, B->out.reserve(ns * capV)); HIPCHK(ctx, B->out_len.reserve(ns)); HIPCHK(ctx, B->out_cw.reserve(ns)); HIPCHK(ctx, B->out_span.reserve(ns * 2)); HIPCHK(ctx, B->out_n.reserve(cap[q]));
        if (need_cov) HIPCHK(ctx, B->out_cov.reserve(ns * capV));
        HIPCHK(ctx, B->seqs.reserve(sizeof(PSeq) * ns)); HIPCHK(ctx, B->job_off.reserve((size_t)cap[q] + 1)); HIPCHK(ctx, B->job_bb.reserve(cap[q])); HIPCHK(ctx, B->job_list.reserve(cap[q]));
        HIPCHK(ctx, B->job_unit.reserve(cap[q])); HIPCHK(ctx, B->job_pos.reserve(cap[q])); HIPCHK(ctx, B->job_final.reserve(cap[q]));
        L[q] = LevelDev{(PSeq*)B->seqs.p, B->out.p, B->out_len.p, B->out_span.p, B->out_cw.p, B->out_n.p, need_cov ? B->out_cov.p : nullptr, B->job_off.p, B->job_bb.p, B->job_unit.p, B->job_pos.p, B->job_list.p, B->job_final.p};
    }
    DevBuf<uint32_t> d_u32, d_ctrl, d_res_off, d_res_cov; DevBuf<int32_t> d_i32, d_res_len; DevBuf<uint8_t> d_res;
    HIPCHK(ctx, d_u32.alloc(9ull * U + 4)); HIPCHK(ctx, d_i32.alloc(3ull * U)); HIPCHK(ctx, d_ctrl.alloc(C_WORDS)); HIPCHK(ctx, d_res_off.alloc(U)); HIPCHK(ctx, d_res_len.alloc(U));
    HIPCHK(ctx, d_res.alloc((size_t)U * capV)); if (hp.want_cov) HIPCHK(ctx, d_res_cov.alloc((size_t)U * capV));
    HierDev H{};
    H.U = U; H.D = hp.D; H.slots = slots; H.capV = (int)capV; H.upper_mode = hp.upper_mode; H.want_cov = hp.want_cov ? 1 : 0; H.Lmax = plan.Lmax; H.keep_final = (hp.trim_tiles & 4) ? 1 : 0; H.cap_jobs[0] = cap[0]; H.cap_jobs[1] = cap[1];
    H.unit_bb = d_i32.p; H.unit_wlen = d_i32.p + U; H.unit_pick = d_i32.p + 2ull * U;
    H.unit_ncur = d_u32.p; H.unit_job0[0] = d_u32.p + U; H.unit_njobs[0] = d_u32.p + 2ull * U + 1; H.unit_job0[1] = d_u32.p + 3ull * U + 1; H.unit_njobs[1] = d_u32.p + 4ull * U + 2; H.unit_seq0 = d_u32.p + 5ull * U + 2; H.unit_tmp = d_u32.p + 6ull * U + 2;
    H.res_off = d_res_off.p; H.res_len = d_res_len.p; H.res = d_res.p; H.res_cov = hp.want_cov ? d_res_cov.p : nullptr; H.ctrl = d_ctrl.p;
    HIPCHK(ctx, hipMemsetAsync(d_ctrl.p, 0, sizeof(uint32_t) * C_WORDS, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(d_res_len.p, 0xff, sizeof(int32_t) * U, ctx->stream));                                    // -1 = no result
    HIPCHK(ctx, hipMemcpyAsync(H.unit_ncur, u_u32.data(), 4ull * U, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(H.unit_job0[0], u_u32.data() + U, 4ull * U, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(H.unit_njobs[0], u_u32.data() + 2ull * U, 4ull * U, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_i32.p, u_i32.data(), 12ull * U, hipMemcpyHostToDevice, ctx->stream));
    { int32_t rc = upload_tiles(ctx, T, ctx->poa_lv[0], hp.trim_tiles & 4, true); if (rc) return rc; }       // (within the sizes reserved above: the pointers in L stay valid)
    static thread_local PinVec<uint32_t> h_nj; h_nj.assign(1, njobs0);
    HIPCHK(ctx, hipMemcpyAsync(d_ctrl.p + C_NJOBS, h_nj.data(), 4, hipMemcpyHostToDevice, ctx->stream));
    ht.mark("L0 lists + upload");
    static thread_local PinVec<uint32_t> h_ctrl; h_ctrl.resize(C_WORDS);
    int level = 0;
    for (;;) {
        const int batch_end = std::min(C_MAXLV - 1, level + (level == 0 ? levels_est : 3));
        for (; level < batch_end; ++level) {
            const int par = level & 1; LevelDev& Lv = L[par]; LevelDev& Nx = L[par ^ 1];
            PoaJobSet J = level_jobs(ctx, hp, plan, level, slots, level == 0 ? d_level0 : (const PSeq*)Nx.seqs, d_bbs, level == 0 ? ctx->poa_lv[0].seq_idx.p : nullptr, cap[par], d_ctrl.p + C_FLAGS);
            J.nrun_dev = d_ctrl.p + C_NJOBS + par;
            int32_t rc = poa_launch(ctx, plan, J, band0, false, d_ctrl.p + C_WORK + 3 * level, hp.sub && level == 0); if (rc) return rc;
            int stage = 0;
            for (int bw = band0 * 2; bw <= 256; bw *= 2, ++stage) {          // band-edge check (oracle run_tile): flagged tiles run again, whole, with twice the band
                uint32_t* cnt = d_ctrl.p + C_REDO + 2 * level + stage;
                hipLaunchKernelGGL(k_poa_redo_list, dim3(std::min<uint32_t>((cap[par] + 255) / 256, 1024u)), dim3(256), 0, ctx->stream, Lv.out_n, d_ctrl.p + C_NJOBS + par, Lv.job_list, cnt, d_ctrl.p + C_REDO_TOTAL);
                PoaJobSet R = J; R.job_list = Lv.job_list; R.nrun_dev = cnt;
                rc = poa_launch(ctx, plan, R, bw, true, d_ctrl.p + C_WORK + 3 * level + 1 + stage, hp.sub && level == 0); if (rc) return rc;
            }
            hipLaunchKernelGGL(k_poa_unit_scan, dim3(U), dim3(256), 0, ctx->stream, H, Lv, par);
            hipLaunchKernelGGL(k_poa_unit_offsets, dim3(1), dim3(1024), 0, ctx->stream, H, par);
            hipLaunchKernelGGL(k_poa_fill_next, dim3(std::min<uint32_t>((cap[par] + 3) / 4, 4096u)), dim3(256), 0, ctx->stream, H, Lv, par);
            hipLaunchKernelGGL(k_poa_fill_jobs, dim3(std::min<uint32_t>((cap[par ^ 1] + 255) / 256, 1024u)), dim3(256), 0, ctx->stream, H, Nx, par);
            HIPCHK(ctx, hipGetLastError());
        }
        HIPCHK(ctx, hipMemcpyAsync(h_ctrl.data(), d_ctrl.p, 4 * C_WORDS, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        if (h_ctrl[C_FLAGS + 2]) NGSID_FAIL(ctx, NGSID_ERR_HIP, "internal: POA tile kernel loop guard tripped (code %u)", h_ctrl[C_FLAGS + 2]);
        if (h_ctrl[C_OVERFLOW] || h_ctrl[C_FLAGS + 1]) { ht.mark("gave up (geometry): host-driven loop"); return NGSID_OK; }
        if (h_ctrl[C_NJOBS + (level & 1)] == 0) break;                        // every unit has finished
        if (level >= C_MAXLV - 1) return NGSID_OK;
    }
    ctx->poa_redo_tiles += h_ctrl[C_REDO_TOTAL];
    ht.mark("levels");
    // ---- results
    static thread_local PinVec<int32_t> h_len; static thread_local PinVec<uint32_t> h_off, h_cov; static thread_local PinVec<uint8_t> h_res;
    h_len.resize(U); h_off.resize(U); const size_t used = h_ctrl[C_RES_USED];
    HIPCHK(ctx, hipMemcpyAsync(h_len.data(), d_res_len.p, 4ull * U, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(h_off.data(), d_res_off.p, 4ull * U, hipMemcpyDeviceToHost, ctx->stream));
    h_res.resize(used + 1); if (used) HIPCHK(ctx, hipMemcpyAsync(h_res.data(), d_res.p, used, hipMemcpyDeviceToHost, ctx->stream));
    if (hp.want_cov) { h_cov.resize(used + 1); if (used) HIPCHK(ctx, hipMemcpyAsync(h_cov.data(), d_res_cov.p, 4 * used, hipMemcpyDeviceToHost, ctx->stream)); }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (uint32_t u = 0; u < U; ++u) {
        Unit& Un = units[u]; if (Un.done) continue;
        Un.done = true; Un.seqs.clear();
        if (h_len[u] < 0) continue;
        const int len = h_len[u];
        Un.result.assign((const char*)h_res.data() + h_off[u], (size_t)len);
        if (hp.want_cov) Un.cov.assign(h_cov.data() + h_off[u], h_cov.data() + h_off[u] + len);
        Un.has_result = true;
    }
    ht.mark("results");
    *done = true;
    return NGSID_OK;
}

static int32_t run_hierarchy_batch(ngsid_ctx* ctx, const PSeq* d_level0, uint32_t maxlen0, const PSeq* d_bbs, const std::vector<int>& bb_len,
                                   std::vector<Unit>& units, const HierParams& hp)
{
    bool done = false;
    int32_t rc = run_hierarchy_dev(ctx, d_level0, maxlen0, d_bbs, bb_len, units, hp, &done);
    if (rc || done) return rc;
    return run_hierarchy_host(ctx, d_level0, maxlen0, d_bbs, bb_len, units, hp);
}

}  // namespace

// Round 5: the level buffers of a hierarchy are sized by its level-0 tiles (output slots x graph capacity bytes per tile, + 4 bytes per base of
// coverage when tiles are trimmed: 17.6 KB per tile of a 500-base polishing window), i.e. by the number of READS of the call - 107 GB for the two windows of 10 M
// 750-base reads.  Units (clusters / windows) are independent hierarchies, so the call is cut into batches of whole units under a byte budget the context derives
// from the HBM that is free NOW (a third of it, divided by the live contexts of the process, at most 48 GB, at least 1 GB; "poa_level_budget_mb" sets it for tests).  Results cannot depend on the batching: a
// unit's hierarchy never sees another unit, and the launch geometry a batch plans for (graph capacity, slots) only decides whether the device-driven levels or
// the host-driven loop run it (tests run one batch per unit against one batch for all).  A single unit larger than the budget still runs alone: the footprint is
// bounded by max(budget, largest unit), not by the call.
int32_t run_hierarchy(ngsid_ctx* ctx, const PSeq* d_level0, uint32_t maxlen0, const PSeq* d_bbs, const std::vector<int>& bb_len,
                      std::vector<Unit>& units, const HierParams& hp)
{
    if (hp.single_below > 0) {
        // round 6 (ngsid_poa_params_t.single_below, oracle run_unit): the units the caller marked (fewer sequences than the threshold) run as ONE graph in the given order, as
        // hierarchies of their own - with room for NGSID_POA_SINGLE_NODE_CAP / 16 times the first sequence where the unit's longest sequence has at most NGSID_POA_SINGLE_MAXLEN
        // bases (launch geometry for that class only), with the caller's capacity otherwise; the others are tiled at depth D exactly as before.  A call without such units
        // takes the unchanged path.
        HierParams hb = hp; hb.single_below = 0;
        for (int cls = 0; cls < 2; ++cls) {
            std::vector<size_t> pick; uint32_t mx = 0;
            for (size_t u = 0; u < units.size(); ++u) if (!units[u].done && units[u].single_maxlen > 0 && (units[u].single_maxlen <= NGSID_POA_SINGLE_MAXLEN) == (cls == 0)) { pick.push_back(u); mx = std::max(mx, units[u].single_maxlen); }
            if (pick.empty()) continue;
            HierParams hs = hb; hs.D = 0; if (cls == 0) hs.node_cap = NGSID_POA_SINGLE_NODE_CAP;
            std::vector<Unit> sub; sub.reserve(pick.size());
            for (size_t u : pick) sub.push_back(std::move(units[u]));
            const int32_t rc = run_hierarchy(ctx, d_level0, std::min(maxlen0, mx), d_bbs, bb_len, sub, hs);
            for (size_t x = 0; x < pick.size(); ++x) { units[pick[x]] = std::move(sub[x]); units[pick[x]].done = true; }
            if (rc) return rc;
        }
        bool any = false; for (const Unit& U : units) any = any || !U.done;
        if (!any) return NGSID_OK;
        return run_hierarchy(ctx, d_level0, maxlen0, d_bbs, bb_len, units, hb);      // the large units (the others are done: every loop below skips them)
    }
    size_t own = 0; for (auto& L : ctx->poa_lv) own += L.out.abytes + L.out_cov.abytes + L.seqs.abytes;       // grow-only buffers of this context that the call will reuse
    const long long mb = ngsid_opt(ctx, "poa_level_budget_mb", 0);
    const size_t budget = mb > 0 ? (size_t)mb << 20 : ngsid_mem_share(3, (size_t)1 << 30, (size_t)48 << 30, (size_t)16 << 30, own);      // (contexts of one process share the device: eight virtual ranks each take a 24th)
    // bytes per level-0 tile: both ping-pong level buffers (the second holds ~slots / D of the first + 25 %), as run_hierarchy_dev sizes them
    int maxbb = 0; for (const Unit& U : units) if (!U.done && U.bb >= 0) maxbb = std::max(maxbb, bb_len[U.bb]);
    const int Lb = std::max<int>((int)maxlen0, maxbb), Lb2 = Lb + Lb / 4 + 16;
    long long capV = (long long)Lb2 * (hp.node_cap > 0 ? hp.node_cap : 28) / 16; capV = std::max<long long>(capV, Lb2 + 64);
    const long long slots = std::max<long long>(1, ngsid_opt(ctx, "poa_out_slots", 4));
    const bool need_cov = hp.want_cov || hp.trim_tiles;
    const double per_tile = (double)slots * ((double)capV * (need_cov ? 5.0 : 1.0) + 64.0) * (hp.D > 0 ? 1.0 + 1.25 * (double)slots / (double)hp.D : 1.0) + 32.0;
    // batches of consecutive units
    std::vector<std::pair<size_t, size_t>> batches; size_t b0 = 0; double acc = 0;
    for (size_t u = 0; u < units.size(); ++u) {
        const uint32_t ncur = units[u].done ? 0u : (uint32_t)units[u].seqs.size();
        const double need = ncur ? per_tile * (double)poa_ntiles(ncur, hp.D > 0 ? (uint32_t)hp.D : ncur) : 0.0;
        if (u > b0 && acc + need > (double)budget) { batches.push_back({b0, u}); b0 = u; acc = 0; }
        acc += need;
    }
    batches.push_back({b0, units.size()});
    if (batches.size() == 1) return run_hierarchy_batch(ctx, d_level0, maxlen0, d_bbs, bb_len, units, hp);
    for (auto& bt : batches) {
        std::vector<Unit> sub; sub.reserve(bt.second - bt.first);
        for (size_t u = bt.first; u < bt.second; ++u) sub.push_back(std::move(units[u]));
        const int32_t rc = run_hierarchy_batch(ctx, d_level0, maxlen0, d_bbs, bb_len, sub, hp);
        for (size_t u = bt.first; u < bt.second; ++u) units[u] = std::move(sub[u - bt.first]);
        if (rc) return rc;
    }
    return NGSID_OK;
}

// ---------------------------------------------------------------------------------------------- (a13,a14)
static int32_t poa_consensus_impl(ngsid_ctx* ctx, const ngsid_reads_t* reads, const uint32_t* read_order, const uint64_t* grp_off, uint64_t n_groups,
                                  const ngsid_poa_params_t* prm, uint64_t* cons_off, uint8_t* cons, uint64_t cons_cap, uint64_t* needed, uint32_t* cov, const uint32_t* weight = nullptr);

// (8e step 3) the merge of per-shard partial consensuses: sequence i stands for weight[i] reads (host array, one entry per read of `reads`; 0 counts as 1).
// Qualities are ignored: every base of sequence i weighs weight[i] (capped at 2^20 per base like the tile consensuses of the hierarchy's upper levels).
extern "C" int32_t ngsid_poa_consensus_weighted(ngsid_ctx* ctx, const ngsid_reads_t* reads, const uint32_t* read_order, const uint64_t* grp_off, uint64_t n_groups,
                                                const ngsid_poa_params_t* prm, const uint32_t* weight, uint64_t* cons_off, uint8_t* cons, uint64_t cons_cap, uint64_t* needed)
{
    if (ctx && !weight) NGSID_FAIL(ctx, NGSID_ERR_ARG, "null weight array");
    return poa_consensus_impl(ctx, reads, read_order, grp_off, n_groups, prm, cons_off, cons, cons_cap, needed, nullptr, weight);
}

extern "C" int32_t ngsid_poa_consensus(ngsid_ctx* ctx, const ngsid_reads_t* reads, const uint32_t* read_order, const uint64_t* grp_off, uint64_t n_groups,
                                       const ngsid_poa_params_t* prm, uint64_t* cons_off, uint8_t* cons, uint64_t cons_cap, uint64_t* needed)
{
    ApiClock api_clock_(ctx, "poa_consensus");
    return poa_consensus_impl(ctx, reads, read_order, grp_off, n_groups, prm, cons_off, cons, cons_cap, needed, nullptr);
}

// same, plus the per-base coverage of the consensus (boundary 8b: "consensus bytes, len, per-base coverage")
extern "C" int32_t ngsid_poa_consensus_cov(ngsid_ctx* ctx, const ngsid_reads_t* reads, const uint32_t* read_order, const uint64_t* grp_off, uint64_t n_groups,
                                           const ngsid_poa_params_t* prm, uint64_t* cons_off, uint8_t* cons, uint32_t* cov, uint64_t cons_cap, uint64_t* needed)
{
    if (ctx && !cov) NGSID_FAIL(ctx, NGSID_ERR_ARG, "null coverage buffer");
    return poa_consensus_impl(ctx, reads, read_order, grp_off, n_groups, prm, cons_off, cons, cons_cap, needed, cov);
}

static int32_t poa_consensus_impl(ngsid_ctx* ctx, const ngsid_reads_t* reads, const uint32_t* read_order, const uint64_t* grp_off, uint64_t n_groups,
                                  const ngsid_poa_params_t* prm, uint64_t* cons_off, uint8_t* cons, uint64_t cons_cap, uint64_t* needed, uint32_t* cov, const uint32_t* weight)
{
    if (!ctx) return NGSID_ERR_ARG;
    if (!reads || !grp_off || !prm || !cons_off) NGSID_FAIL(ctx, NGSID_ERR_ARG, "null argument");
    HostTimer htc(ctx->stream, "consensus");
    DevReads RD; int32_t rc = ngsid_upload_reads(ctx, reads, &RD, false); if (rc) return rc;
    htc.mark("upload");
    NGSID_TRY(ngsid_check_lists(ctx, read_order, grp_off, n_groups, RD.n));
    htc.mark("checks");
    DevBuf<PSeq> d_seqs; HIPCHK(ctx, d_seqs.alloc(RD.n));
    DevBuf<uint32_t> d_weight; if (weight && RD.n) NGSID_TRY(dev_put(ctx, d_weight, weight, RD.n));
    if (RD.n) hipLaunchKernelGGL(k_make_pseq_reads, dim3(NGSID_GRID(ctx, (RD.n + 255) / 256, 256, "k_make_pseq_reads")), dim3(256), 0, ctx->stream, RD.seq, RD.qual, RD.off, RD.n, prm->mode, weight ? d_weight.p : (const uint32_t*)nullptr, d_seqs.p);
    HIPCHK(ctx, hipGetLastError());
    std::vector<Unit> units(n_groups);
    for (uint64_t g = 0; g < n_groups; ++g) {
        if (read_order) units[g].seqs.assign(read_order + grp_off[g], read_order + grp_off[g + 1]);
        else { units[g].seqs.resize(grp_off[g + 1] - grp_off[g]); for (uint64_t r = grp_off[g]; r < grp_off[g + 1]; ++r) units[g].seqs[r - grp_off[g]] = (uint32_t)r; }
    }
    HierParams hp{prm->match, prm->mismatch, prm->gap, prm->band > 0 ? prm->band : (RD.maxlen <= NGSID_POA_BAND64_MAXLEN ? 64 : 128), prm->node_cap, prm->tile_depth, prm->mode, cov != nullptr, prm->trim > 0 ? 1 : 0};
    hp.single_below = prm->single_below > 0 ? prm->single_below : 0;
    if (hp.single_below > 0) for (Unit& U : units) if (!U.seqs.empty() && U.seqs.size() < (size_t)hp.single_below) { uint32_t mx = 1; for (uint32_t r : U.seqs) mx = std::max<uint32_t>(mx, (uint32_t)(RD.h_off[r + 1] - RD.h_off[r])); U.single_maxlen = mx; }
    std::vector<int> nobb;
    htc.mark("units");
    rc = run_hierarchy(ctx, d_seqs.p, RD.maxlen, nullptr, nobb, units, hp); if (rc) return rc;
    htc.mark("hierarchy");
    rc = ngsid_pack_strings(ctx, "consensus", n_groups, [&](size_t g) -> const std::string& { return units[g].result; }, cons_off, cons, cons_cap, needed);
    if (cov && cons) for (uint64_t g = 0; g < n_groups && cons_off[g + 1] <= cons_cap; ++g) {      // the coverage of every consensus that fitted (zeros where the hierarchy returned none)
        const uint64_t a = cons_off[g], len = cons_off[g + 1] - a;
        if (units[g].cov.size() == len && len) memcpy(cov + a, units[g].cov.data(), 4 * len); else std::fill(cov + a, cov + a + len, 0u);
    }
    return rc;
}
