// k_errprof.hip - ngsid_error_profile (include/ngsid_errprof.h): per group and strand, what the centre's letters became in the reads, how long insertions and deletions are,
// how errors depend on the homopolymer a base sits in, and how often a base of reported quality q was right.
//
// The store pass is ngsid_hp_runs' (ngsid_rec_walk with positions, k_support.hip); this is its fifth consumer and the first that asks about the READS.  PROFILE (k_errprof): a
// workgroup takes a slice of ONE group's pairs of the chunk (an items list, as k_hp_runs), each of its four waves walks whole rows, 64 centre positions a step (as k_cigar_walk:
// class, flag and centre byte of the position before come from the lane below, for lane 0 carried from the step before).  Nine columns in ten are '=': their 4 PAIR and 8 HPCTX
// cells are lane-private registers per strand, added with selects and reduced across the wave once per slice.  The '=' column of qtab is an LDS table in EP_QREP copies,
// [strand][q][lane & 15]: lanes that meet on a quality meet on different banks and on different words.  Everything else ('X', 'D', 'I', their lengths, letters and qualities)
// is rare and goes to LDS with atomics.  A 'D' run is found with one ballot; the run open at the end of a step is carried as a length.  An 'I' run sits between two match
// positions (include/ngsid_cigar.h): the lane BEHIND it reads both read positions, so the run behind position 64 j + 63 is the business of lane 0 of step j + 1.
// Every non-zero counter goes to global memory with ONE 64-bit atomicAdd per (workgroup, counter).  Integer adds commute: the result does not depend on slices, waves or chunks.
#include "k_support.h"
#include "../../include/ngsid_errprof.h"
#include <algorithm>

typedef unsigned long long u64;

#define EP_WAVES 4              // rows in flight per workgroup (one wave each)
#define EP_THREADS (64 * EP_WAVES)
#define EP_SLICE 1024           // pairs per workgroup
#define EP_QREP 16              // copies of the '=' column of qtab in LDS
#define EP_NC NGSID_ERRPROF_NCOUNT
#define EP_NQ NGSID_ERRPROF_NQ

__device__ __forceinline__ uint32_t ep_q(uint8_t byte) { const int q = (int)byte - 33; return (uint32_t)min(max(q, 0), EP_NQ - 1); }
__device__ __forceinline__ uint32_t ep_len(uint32_t l) { return min(l, (uint32_t)NGSID_ERRPROF_MAXLEN) - 1u; }

template <bool QT>
__global__ __launch_bounds__(EP_THREADS)
void k_errprof(const uint32_t* __restrict__ rec, uint32_t stride, const uint16_t* __restrict__ pos /* [pair][stride * 8] */, const int32_t* __restrict__ span,
               const uint32_t* __restrict__ pair_read, const uint8_t* __restrict__ pair_strand /* both: pairs of this chunk */, const uint8_t* __restrict__ oseq,
               const uint8_t* __restrict__ oqual, const uint64_t* __restrict__ read_off, const uint32_t* __restrict__ items /* [n][3]: group, first pair, end pair (pairs of this chunk) */,
               const uint8_t* __restrict__ cen_ctx /* per centre position: min(run length, 8) | letter code << 4 */, const uint64_t* __restrict__ cen_off,
               u64* __restrict__ counts, u64* __restrict__ qtab)
{
    __shared__ uint32_t cnt[2 * EP_NC];                                              // [strand][counter]: the rare classes, and the hot ones once per wave
    __shared__ uint32_t qeq[QT ? 2 * EP_NQ * EP_QREP : 1];                           // [strand][q][copy]
    __shared__ uint32_t qxi[QT ? 2 * EP_NQ * 2 : 1];                                 // [strand][q][X, I]
    const uint32_t g = items[blockIdx.x * 3], p0 = items[blockIdx.x * 3 + 1], p1 = items[blockIdx.x * 3 + 2];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    for (uint32_t i = tid; i < 2 * EP_NC; i += EP_THREADS) cnt[i] = 0;
    if (QT) {
        for (uint32_t i = tid; i < 2 * EP_NQ * EP_QREP; i += EP_THREADS) qeq[i] = 0;
        for (uint32_t i = tid; i < 2 * EP_NQ * 2; i += EP_THREADS) qxi[i] = 0;
    }
    __syncthreads();
    const int m = (int)(cen_off[g + 1] - cen_off[g]);
    const uint8_t* cx = cen_ctx + cen_off[g];
    uint32_t e0[4] = {0, 0, 0, 0}, e1[4] = {0, 0, 0, 0}, h0[8] = {0, 0, 0, 0, 0, 0, 0, 0}, h1[8] = {0, 0, 0, 0, 0, 0, 0, 0};      // '=' by centre letter, '=' by run length: strand 0, strand 1
    for (uint32_t p = p0 + wave; p < p1; p += EP_WAVES) {                              // (p, and with it everything read per pair, is wave-uniform)
        const int qb = span[(u64)p * 4], qe = span[(u64)p * 4 + 1], tb = span[(u64)p * 4 + 2], te = span[(u64)p * 4 + 3];
        const uint32_t rd = pair_read[p];
        const u64 rb = read_off[rd]; const int L = (int)(read_off[rd + 1] - rb);
        if (tb < 0 || te < tb || te >= m || (uint32_t)te >= stride * 8u || qb < 0 || qe < qb || qe >= L) continue;      // no counted column (all -1); anything else a path cannot be keeps the loads inside the row
        const uint32_t s = pair_strand[p] ? 1u : 0u;
        uint32_t* const C = cnt + s * EP_NC;
        if (lane == 0) atomicAdd(C + NGSID_ERRPROF_READS, 1u);
        const uint32_t* row = rec + (u64)p * stride; const uint16_t* prow = pos + (u64)p * stride * 8;
        const uint8_t* rs = oseq + rb; const uint8_t* rq = QT ? oqual + rb : nullptr;
        uint32_t carry_del = 0, carry_flag = 0, carry_ctx = 0, d_open = 0;             // of the last position of the step before: a 'D'? its flag, its centre byte; length of the 'D' run that reaches it
        for (int base = tb & ~63; base <= te; base += 64) {
            const int b = base + (int)lane;
            const bool valid = b >= tb && b <= te;
            const uint32_t nib = valid ? (row[b >> 3] >> ((b & 7) * 4)) & 15u : 0u, code = nib & 7u, flag = nib >> 3;
            const uint32_t ctx = valid ? cx[b] : 0u, cc = ctx >> 4, rl = (ctx & 15u) - 1u;      // letter code of the centre base (4: outside ACGT), run length - 1
            const bool is_eq = valid && code == NGSID_REC_EQ, is_del = valid && code == NGSID_REC_DEL, is_x = valid && code >= NGSID_REC_SUB && code <= NGSID_REC_OTHER;
            uint32_t pd = __shfl_up((uint32_t)is_del, 1), pf = __shfl_up(flag, 1), pctx = __shfl_up(ctx, 1);
            if (lane == 0) { pd = carry_del; pf = carry_flag; pctx = carry_ctx; }
            const bool insb = valid && b > tb && pf && !pd && !is_del;                 // an 'I' run between the position before and this one: both are match positions
            // ---- '=': registers (and the replicated quality table)
            const uint32_t hot = is_eq && cc < 4u;
            if (s) {
#pragma unroll
                for (uint32_t c = 0; c < 4; ++c) e1[c] += hot & (uint32_t)(cc == c);
#pragma unroll
                for (uint32_t r = 0; r < 8; ++r) h1[r] += hot & (uint32_t)(rl == r);
            } else {
#pragma unroll
                for (uint32_t c = 0; c < 4; ++c) e0[c] += hot & (uint32_t)(cc == c);
#pragma unroll
                for (uint32_t r = 0; r < 8; ++r) h0[r] += hot & (uint32_t)(rl == r);
            }
            if (QT && (is_eq || is_x)) {
                const int x = prow[b];
                if (x < L) {                                                           // always true for a path of the aligner
                    const uint32_t q = ep_q(rq[x]);
                    if (is_eq) atomicAdd(&qeq[(s * EP_NQ + q) * EP_QREP + (lane & (EP_QREP - 1))], 1u);
                    else atomicAdd(&qxi[(s * EP_NQ + q) * 2], 1u);
                }
            }
            // ---- 'X' and 'D': LDS atomics
            if (is_x || is_del) {
                const uint32_t o = is_del ? 5u : code - NGSID_REC_SUB;                 // 0 .. 3 the read's letter, 4 outside ACGT, 5 deleted
                if (cc < 4u) { atomicAdd(C + NGSID_ERRPROF_PAIR + cc * 6u + o, 1u); atomicAdd(C + NGSID_ERRPROF_HPCTX + rl * 4u + (is_del ? 2u : 1u), 1u); }
                else atomicAdd(C + NGSID_ERRPROF_CEN_OTHER, 1u);
            }
            // ---- the 'D' runs that end in this step (the one that reaches lane 63 is carried)
            const u64 D = __ballot(is_del);
            if (d_open && !(D & 1ull) && lane == 0) atomicAdd(C + NGSID_ERRPROF_DEL_LEN + ep_len(d_open), 1u);      // the carried run ended on lane 63 of the step before
            if (is_del && lane < 63u && !((D >> (lane + 1u)) & 1ull)) {
                const u64 gap = ~D & ((1ull << lane) - 1ull);                          // positions below this one that are no 'D'
                const uint32_t len = gap ? lane - (uint32_t)(63 - __clzll((long long)gap)) : lane + 1u + d_open;
                atomicAdd(C + NGSID_ERRPROF_DEL_LEN + ep_len(len), 1u);
            }
            if ((D >> 63) & 1ull) d_open = ~D ? (uint32_t)__clzll((long long)~D) : d_open + 64u; else d_open = 0;
            // ---- the 'I' run in front of this position
            if (insb) {
                const int qa = prow[b - 1], qz = prow[b];
                if (qa + 1 < qz && qz < L) {                                           // always true for a path of the aligner: keeps the loads inside the read
                    atomicAdd(C + NGSID_ERRPROF_INS_LEN + ep_len((uint32_t)(qz - qa - 1)), 1u);
                    if ((pctx >> 4) < 4u && (pctx & 15u)) atomicAdd(C + NGSID_ERRPROF_HPCTX + ((pctx & 15u) - 1u) * 4u + 3u, 1u);
                    for (int i = qa + 1; i < qz; ++i) {
                        atomicAdd(C + NGSID_ERRPROF_INS_LETTER + (uint32_t)ngsid_bcode(rs[i]), 1u);
                        if (QT) atomicAdd(&qxi[(s * EP_NQ + ep_q(rq[i])) * 2 + 1], 1u);
                    }
                }
            }
            const int v1 = min(te - base, 63);                                         // the last valid lane of the step
            carry_del = __shfl((uint32_t)is_del, v1); carry_flag = __shfl(flag, v1); carry_ctx = __shfl(ctx, v1);
        }
        if (d_open && lane == 0) atomicAdd(C + NGSID_ERRPROF_DEL_LEN + ep_len(d_open), 1u);      // (a path ends on a match column: never taken)
    }
    // ---- the hot counters: one reduction per wave and counter
#pragma unroll
    for (int k = 0; k < 24; ++k) {
        uint32_t v = k < 4 ? e0[k] : k < 8 ? e1[k - 4] : k < 16 ? h0[k - 8] : h1[k - 16];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
        const uint32_t at = k < 4 ? NGSID_ERRPROF_PAIR + k * 7 : k < 8 ? EP_NC + NGSID_ERRPROF_PAIR + (k - 4) * 7 : k < 16 ? NGSID_ERRPROF_HPCTX + (k - 8) * 4 : EP_NC + NGSID_ERRPROF_HPCTX + (k - 16) * 4;
        if (lane == 0 && v) atomicAdd(cnt + at, v);
    }
    __syncthreads();
    for (uint32_t i = tid; i < 2 * EP_NC; i += EP_THREADS) { const uint32_t v = cnt[i]; if (v) atomicAdd(counts + (u64)g * 2 * EP_NC + i, (u64)v); }
    if (QT) {
        for (uint32_t i = tid; i < 2 * EP_NQ; i += EP_THREADS) {
            uint32_t v = 0;
#pragma unroll
            for (int r = 0; r < EP_QREP; ++r) v += qeq[i * EP_QREP + r];
            u64* out = qtab + ((u64)g * 2 * EP_NQ + i) * NGSID_ERRPROF_NK;
            if (v) atomicAdd(out, (u64)v);
            if (qxi[i * 2]) atomicAdd(out + 1, (u64)qxi[i * 2]);
            if (qxi[i * 2 + 1]) atomicAdd(out + 2, (u64)qxi[i * 2 + 1]);
        }
    }
}

static inline uint32_t ep_host_code(uint8_t c) { switch (c) { case 'A': case 'a': return 0; case 'C': case 'c': return 1; case 'G': case 'g': return 2; case 'T': case 't': return 3; default: return 4; } }

extern "C" int32_t ngsid_error_profile(ngsid_ctx* ctx, const ngsid_reads_t* centres, const ngsid_reads_t* reads, const uint32_t* read_order,
                                       const uint64_t* grp_off, uint64_t n_groups, const ngsid_support_params_t* prm,
                                       uint64_t* counts, uint64_t* qtab, int8_t* strand)
{
    ApiClock api_clock_(ctx, "error_profile");
    if (!ctx) return NGSID_ERR_ARG;
    if (!counts) NGSID_FAIL(ctx, NGSID_ERR_ARG, "null counts");
    const uint32_t G = (uint32_t)n_groups;
    const size_t NCNT = (size_t)G * 2 * EP_NC, NQT = (size_t)G * 2 * EP_NQ * NGSID_ERRPROF_NK;
    DevBuf<u64> d_counts, d_qtab; DevBuf<uint32_t> d_items; DevBuf<uint8_t> d_pair_strand, d_ctx;
    std::vector<uint8_t> cen_ctx, pair_strand; std::vector<uint32_t> items; bool started = false, with_q = false;
    auto init = [&](const RecPlan& P) -> int32_t {
        memset(counts, 0, sizeof(uint64_t) * NCNT);
        if (qtab) memset(qtab, 0, sizeof(uint64_t) * NQT);
        cen_ctx.resize(P.total);
        for (uint32_t g = 0; g < P.G; ++g) {                                           // per centre position: the length of the maximal run of equal bytes that holds it, and its letter
            const uint8_t* C = P.bseq + P.boff[g]; const uint64_t m = P.boff[g + 1] - P.boff[g];
            for (uint64_t a = 0; a < m; ) {
                uint64_t b = a + 1; while (b < m && C[b] == C[a]) ++b;
                const uint8_t v = (uint8_t)(std::min<uint64_t>(b - a, NGSID_ERRPROF_MAXRUN) | (ep_host_code(C[a]) << 4));
                for (uint64_t i = a; i < b; ++i) cen_ctx[P.boff[g] + i] = v;
                a = b;
            }
        }
        return NGSID_OK;
    };
    auto start = [&](const RecPlan& P) -> int32_t {
        with_q = qtab && P.d_oqual;                                                    // a read set without qualities: qtab stays zero
        NGSID_TRY(dev_put(ctx, d_ctx, cen_ctx.data(), cen_ctx.size()));
        pair_strand.resize(P.NP);
        for (uint64_t p = 0; p < P.NP; ++p) pair_strand[p] = P.h_orient[P.pair_read[p]] ? 1 : 0;
        NGSID_TRY(dev_put(ctx, d_pair_strand, pair_strand.data(), pair_strand.size()));
        HIPCHK(ctx, d_counts.alloc(NCNT)); HIPCHK(ctx, hipMemsetAsync(d_counts.p, 0, sizeof(u64) * NCNT, ctx->stream));
        if (with_q) { HIPCHK(ctx, d_qtab.alloc(NQT)); HIPCHK(ctx, hipMemsetAsync(d_qtab.p, 0, sizeof(u64) * NQT, ctx->stream)); }
        started = true; return NGSID_OK;
    };
    auto chunk = [&](const RecPlan& P, const RecChunk& C) -> int32_t {
        items.clear();
        for (uint32_t g = 0; g < P.G; ++g) {
            const uint64_t a = std::max(P.gbeg[g], C.c0), e = std::min(P.gbeg[g + 1], C.c1);
            if (P.boff[g + 1] == P.boff[g]) continue;
            for (uint64_t s = a; s < e; s += EP_SLICE) { items.push_back(g); items.push_back((uint32_t)(s - C.c0)); items.push_back((uint32_t)(std::min(e, s + EP_SLICE) - C.c0)); }
        }
        if (items.empty()) return NGSID_OK;
        HIPCHK(ctx, d_items.reserve(items.size()));
        HIPCHK(ctx, hipMemcpyAsync(d_items.p, items.data(), 4 * items.size(), hipMemcpyHostToDevice, ctx->stream));
        const unsigned grid = NGSID_GRID(ctx, items.size() / 3, EP_THREADS, "k_errprof");
        { ProfScope ps_(ctx, "k_errprof");
          if (with_q) hipLaunchKernelGGL(k_errprof<true>, dim3(grid), dim3(EP_THREADS), 0, ctx->stream, C.rec, P.stride, C.pos, C.span, P.d_pair_read + C.c0, d_pair_strand.p + C.c0, P.d_oseq,
                                         P.d_oqual, P.d_read_off, d_items.p, d_ctx.p, P.d_cen_off, d_counts.p, d_qtab.p);
          else hipLaunchKernelGGL(k_errprof<false>, dim3(grid), dim3(EP_THREADS), 0, ctx->stream, C.rec, P.stride, C.pos, C.span, P.d_pair_read + C.c0, d_pair_strand.p + C.c0, P.d_oseq,
                                  (const uint8_t*)nullptr, P.d_read_off, d_items.p, d_ctx.p, P.d_cen_off, d_counts.p, (u64*)nullptr); }
        HIPCHK(ctx, hipGetLastError());
        return NGSID_OK;
    };
    int32_t rc = ngsid_rec_walk(ctx, centres, reads, read_order, grp_off, n_groups, prm, strand, init, start, chunk, true); if (rc) return rc;
    if (!started) return NGSID_OK;
    NGSID_TRY(dev_get(ctx, (u64*)counts, d_counts.p, NCNT));
    if (with_q) NGSID_TRY(dev_get(ctx, (u64*)qtab, d_qtab.p, NQT));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return NGSID_OK;
}
