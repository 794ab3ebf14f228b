// polish_host.hip - ngsid_polish (a16,a17): strands and oriented reads, the grouped-reads front end, and the iteration driver (PolishRun) over the read -> backbone
// aligners, k_layers, the unit lists (polish_units.h) and the POA hierarchy (poa_host.h).  Mirrors oracle/ngsid_oracle_poa.c: ongsid_polish.
#include "poa_host.h"
#include "polish_units.h"

namespace {

__global__ __launch_bounds__(256)
void k_strand(const uint64_t* __restrict__ mzoff /* compact CSR offsets of the reads' minimizers */, const uint32_t* __restrict__ mzcnt, const uint32_t* __restrict__ hlen, const uint64_t* __restrict__ mzcode, int k,
              const uint32_t* __restrict__ rgroup, const uint64_t* __restrict__ bcodes, const uint64_t* __restrict__ boff /* 2G+1: fw lists then rc lists */, uint32_t G,
              uint64_t n, uint8_t* __restrict__ orient)
{
    const int lane = threadIdx.x & 63;
    const uint64_t r = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (r >= n) return;
    const uint32_t g = rgroup[r];
    if (g == 0xffffffffu) { if (lane == 0) orient[r] = 255; return; }        // read belongs to no group
    const uint32_t M = hlen[r] >= (uint32_t)k ? mzcnt[r] : 0;
    const uint64_t* cf = bcodes + boff[g]; const uint32_t nf = (uint32_t)(boff[g + 1] - boff[g]);
    const uint64_t* cr = bcodes + boff[G + g]; const uint32_t nr = (uint32_t)(boff[G + g + 1] - boff[G + g]);
    int a = 0, b = 0;
    for (uint32_t x = lane; x < M; x += 64) {
        const uint64_t code = mzcode[mzoff[r] + x];
        uint32_t lo = 0, hi = nf; while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (cf[mid] < code) lo = mid + 1; else hi = mid; }
        a += (lo < nf && cf[lo] == code);
        lo = 0; hi = nr; while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (cr[mid] < code) lo = mid + 1; else hi = mid; }
        b += (lo < nr && cr[lo] == code);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { a += __shfl_xor(a, d); b += __shfl_xor(b, d); }
    if (lane == 0) orient[r] = (a == 0 && b == 0) ? 255 : (b > a ? 1 : 0);
}

// Polishing windows of a backbone of Bl bases: W bases each; a last window shorter than W/10 is merged into the one before it.  (racon keeps it:
// only layers of at least 0.02 W bases enter a window, so a 7-base tail window is built from the reads that carry INSERTIONS there and the
// consensus gains bases - seen on 5 007-base amplicons.)  Window w covers [w * W, w == nwin - 1 ? Bl : (w + 1) * W).
__host__ __device__ __forceinline__ int polish_nwin(int Bl, int W) { const int raw = Bl <= W ? 1 : (Bl + W - 1) / W; const int tail = Bl - (raw - 1) * W; return (raw >= 2 && tail < W / 10) ? raw - 1 : raw; }
__host__ __device__ __forceinline__ int polish_wlen(int Bl, int W, int w) { return w == polish_nwin(Bl, W) - 1 ? Bl - w * W : W; }

__device__ __forceinline__ uint8_t comp_base(uint8_t c) { switch (c) { case 'A': return 'T'; case 'C': return 'G'; case 'G': return 'C'; case 'T': return 'A'; default: return 'N'; } }

__global__ void k_orient(const uint8_t* __restrict__ seq, const uint8_t* __restrict__ qual, const uint64_t* __restrict__ off, uint64_t n,
                         const uint8_t* __restrict__ orient, uint8_t* __restrict__ oseq, uint8_t* __restrict__ oqual)
{
    const uint64_t r = blockIdx.x;
    if (r >= n) return;
    const uint64_t b = off[r]; const int len = (int)(off[r + 1] - b); const bool rc = orient[r] == 1;
    for (int i = threadIdx.x; i < len; i += blockDim.x) {
        if (rc) { oseq[b + i] = comp_base(seq[b + len - 1 - i]); if (qual) oqual[b + i] = qual[b + len - 1 - i]; }
        else { oseq[b + i] = seq[b + i]; if (qual) oqual[b + i] = qual[b + i]; }
    }
}

// one wave per (pair, window): validity filters of racon's window assignment + the PSeq of the layer (oracle ongsid_polish);
// the lanes share the mean-quality sum over the layer's bases (coalesced), everything else is wave-uniform
__global__ __launch_bounds__(256) void k_layers(const uint8_t* __restrict__ oseq, const uint8_t* __restrict__ oqual, const uint64_t* __restrict__ off,
                         const uint32_t* __restrict__ pair_read, const uint32_t* __restrict__ pair_group, uint64_t npairs, int nwinmax,
                         const int32_t* __restrict__ bp, const int32_t* __restrict__ span, const int32_t* __restrict__ blen /* per group */,
                         int W, double qthr, double ethr, int sub /* NGSID_ALN_SUBGRAPH: a layer that does not span its window gets POA_MODE_SUBGRAPH */,
                         PSeq* __restrict__ lay, uint16_t* __restrict__ valid /* 0 = no layer, else 1 + its first window position */, int* __restrict__ maxlen_out)
{
    const int lane = threadIdx.x & 63;
    const uint64_t t = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (t >= npairs * (uint64_t)nwinmax) return;
    const uint64_t p = t / nwinmax; const int wdx = (int)(t % nwinmax);
    if (lane == 0) valid[t] = 0;
    const int qb = span[p * 4 + 0], qe = span[p * 4 + 1], tb = span[p * 4 + 2], te = span[p * 4 + 3];
    if (qb < 0) return;
    const int qs = qe - qb + 1, ts = te - tb + 1; const int mn = qs < ts ? qs : ts, mx = qs < ts ? ts : qs;
    if (1.0 - (double)mn / (double)mx > ethr) return;
    const int Bl = blen[pair_group[p]]; const int nw = polish_nwin(Bl, W);
    if (wdx >= nw) return;
    const int32_t* b = bp + (p * (uint64_t)nwinmax + wdx) * 4;
    int qf = b[0], ql = b[1], tf = b[2], tl = b[3];
    if (wdx == nw - 1 && wdx + 1 < nwinmax && (Bl + W - 1) / W > nw) {       // merged tail window: the aligner's break points of the two raw windows are joined
        const int32_t* b2 = b + 4;
        if (b2[0] >= 0) { if (qf < 0) { qf = b2[0]; tf = b2[2]; } ql = b2[1]; tl = b2[3]; }
    }
    if (qf < 0) return;
    const int len = ql - qf + 1; if ((double)len < 0.02 * (double)W) return;
    const uint32_t read = pair_read[p]; const uint64_t rb = off[read];
    if (oqual) {
        long long sq = 0;
        for (int x = qf + lane; x <= ql; x += 64) sq += (long long)oqual[rb + x] - 33;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) sq += __shfl_xor(sq, d);
        if ((double)sq / (double)len < qthr) return;
    }
    const int ws = wdx * W; const int wlen = polish_wlen(Bl, W, wdx);
    const int begin = tf - ws, end = tl - ws; const int offset = (int)(0.01 * (double)wlen);
    PSeq S; S.s = oseq + rb + qf; S.q = oqual ? oqual + rb + qf : nullptr; S.len = len; S.uw = 1; S.cw = 1; S.a0 = begin; S.a1 = end;
    S.mode = (begin < offset && end > wlen - offset) ? NGSID_POA_GLOBAL : (sub ? POA_MODE_SUBGRAPH : NGSID_POA_SEMI);
    if (lane == 0) { lay[t] = S; valid[t] = (uint16_t)((begin < 0 ? 0 : (begin > 65533 ? 65533 : begin)) + 1); if (len > __atomic_load_n(maxlen_out, __ATOMIC_RELAXED)) atomicMax(maxlen_out, len); }      // (millions of atomics on one word would serialise)
}

std::string revcomp(const std::string& s) { std::string r(s.size(), 'N'); for (size_t i = 0; i < s.size(); ++i) { char c = s[s.size() - 1 - i]; r[i] = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : 'N'; } return r; }

}  // namespace

// First stage of ngsid_polish, shared with ngsid_consensus_support (k_support.hip): the strand of every read against the backbone B[g] of its group h_rgroup[r] (h_orient: 0 forward,
// 1 reverse complement, 255 = in no group or no shared minimizer) and the oriented copies of the reads in ctx->pol_oseq / pol_oqual (k_orient, in flight on the stream at return).
int32_t ngsid_polish_orient(ngsid_ctx* ctx, const DevReads& RD, const std::vector<std::string>& B, const std::vector<uint32_t>& h_rgroup, int k, int w, OrientBufs& S, PinVec<uint8_t>& h_orient)
{
    const uint64_t N = RD.n; const uint32_t G = (uint32_t)B.size(); int32_t rc;
    // ---- strand detection (replaces minimap2's strand call): shared HPC minimizers with the initial backbone, fw vs rc
    DevBuf<uint64_t>& mzcode = ctx->pol_mzcode; DevBuf<uint32_t>& mzcnt = ctx->mzc_cnt; DevBuf<uint32_t>& hlen = ctx->mzc_hlen; DevBuf<uint32_t>& d_rgroup = S.d_rgroup; DevBuf<double>& herr = S.herr; DevBuf<double>& rawerr = S.rawerr; DevBuf<uint8_t>& d_orient = S.d_orient;
    HIPCHK(ctx, mzcnt.reserve(N)); HIPCHK(ctx, hlen.reserve(N));
    NGSID_TRY(dev_put(ctx, d_rgroup, h_rgroup.data(), N)); HIPCHK(ctx, d_orient.alloc(N));
    const int sk = std::min(k, 21), sw = std::max(w, sk);       // strand detection only needs SOME minimizer scheme: one-word codes, comparable between the two launches
    {   // the clustering call that preceded this one left the minimizers of the same reads in the context (same bases, offsets, k, w): reuse them
        bool hit = false;
        if (ctx->mzc.valid && ctx->mzc.n == N && ctx->mzc.total == RD.total && ctx->mzc.k == sk && ctx->mzc.w == sw) {
            unsigned long long fp = 0; rc = ngsid_reads_fingerprint(ctx, RD, &fp); if (rc) return rc;
            hit = fp == ctx->mzc.fp;
        }
        if (!hit) {
            ctx->mzc.valid = false;
            HIPCHK(ctx, herr.alloc(N)); HIPCHK(ctx, rawerr.alloc(N));
            static thread_local PinVec<uint32_t> h_c, h_l; h_c.resize(N); h_l.resize(N); long long bad = -1;
            rc = ngsid_minimizers_csr(ctx, RD, sk, sw, ngsid_ctx_mz(ctx), mzcnt.p, hlen.p, herr.p, rawerr.p, h_c.data(), h_l.data(), &bad); if (rc) return rc;
            if (bad >= 0) NGSID_FAIL(ctx, NGSID_ERR_ALPHABET, "base outside ACGTN in a read (read %lld)", bad);       // (the cache stays invalid: ADVICE r4)
            if (N >= 1024) { unsigned long long fp = 0; rc = ngsid_reads_fingerprint(ctx, RD, &fp); if (rc) return rc; ctx->mzc.n = N; ctx->mzc.total = RD.total; ctx->mzc.k = sk; ctx->mzc.w = sw; ctx->mzc.fp = fp; ctx->mzc.valid = true; }
        }
    }
    {
        // backbone fw + rc minimizers through the same kernel (a CSR of their own), then sorted on the host (a handful of short lists)
        std::vector<std::string> two; for (uint32_t g = 0; g < G; ++g) two.push_back(B[g]); for (uint32_t g = 0; g < G; ++g) two.push_back(revcomp(B[g]));
        std::vector<uint64_t> toff(2 * G + 1, 0); std::string cat; for (size_t i = 0; i < two.size(); ++i) { cat += two[i]; toff[i + 1] = cat.size(); }
        ngsid_reads_t br{(const uint8_t*)cat.data(), nullptr, toff.data(), 2ull * G, NGSID_MEM_HOST, 0};
        DevReads BR; rc = ngsid_upload_reads(ctx, &br, &BR, false); if (rc) return rc;
        SketchBufs K; long long bad;
        rc = ngsid_sketch(ctx, BR, sk, sw, K, &bad); if (rc) return rc;
        if (bad >= 0) NGSID_FAIL(ctx, NGSID_ERR_ALPHABET, "base outside ACGTN in a backbone");
        const PinVec<uint64_t>& hmo = K.h_off; const uint64_t btot = hmo[2 * G];
        std::vector<uint64_t> hc(btot + 1);
        NGSID_TRY(dev_get(ctx, hc.data(), K.code.p, btot));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        std::vector<uint64_t> lists, loff(2 * G + 1, 0);
        for (uint32_t i = 0; i < 2 * G; ++i) {
            const uint32_t c = K.h_hlen[i] >= (uint32_t)sk ? K.h_cnt[i] : 0;
            std::vector<uint64_t> v(hc.begin() + hmo[i], hc.begin() + hmo[i] + c); std::sort(v.begin(), v.end());
            lists.insert(lists.end(), v.begin(), v.end()); loff[i + 1] = lists.size();
        }
        DevBuf<uint64_t> d_lists, d_loff; NGSID_TRY(dev_put(ctx, d_lists, lists.data(), lists.size())); NGSID_TRY(dev_put(ctx, d_loff, loff.data(), loff.size()));
        { ProfScope ps_(ctx, "k_strand"); hipLaunchKernelGGL(k_strand, dim3(NGSID_GRID(ctx, (N + 3) / 4, 256, "k_strand")), dim3(256), 0, ctx->stream, ctx->mz_off.p, mzcnt.p, hlen.p, mzcode.p, sk, d_rgroup.p, d_lists.p, d_loff.p, G, N, d_orient.p); }
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    h_orient.resize(N);
    NGSID_TRY(dev_get(ctx, h_orient.data(), d_orient.p, N)); HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    // ---- oriented copies of the reads
    DevBuf<uint8_t>& oseq = ctx->pol_oseq; DevBuf<uint8_t>& oqual = ctx->pol_oqual; HIPCHK(ctx, oseq.reserve(RD.total + 16)); if (RD.qual) HIPCHK(ctx, oqual.reserve(RD.total + 16));
    { ProfScope ps_(ctx, "k_orient"); hipLaunchKernelGGL(k_orient, dim3(NGSID_GRID(ctx, N, 128, "k_orient")), dim3(128), 0, ctx->stream, RD.seq, RD.qual, RD.off, N, d_orient.p, oseq.p, RD.qual ? oqual.p : nullptr); }
    HIPCHK(ctx, hipGetLastError());
    return NGSID_OK;
}

// The grouped-reads front end (ngsid_host.h), first half: argument and list checks, the reads on the device, the centres on the host
int32_t ngsid_groups_open(ngsid_ctx* ctx, const ngsid_reads_t* centres, const ngsid_reads_t* reads, const uint32_t* read_order, const uint64_t* grp_off, uint64_t n_groups, GroupedReads& S)
{
    if (!centres || !reads || !grp_off) NGSID_FAIL(ctx, NGSID_ERR_ARG, "null argument");
    if (centres->n != n_groups) NGSID_FAIL(ctx, NGSID_ERR_ARG, "one centre (backbone) per group expected");
    NGSID_TRY(ngsid_upload_reads(ctx, reads, &S.RD, false));
    NGSID_TRY(ngsid_check_lists(ctx, read_order, grp_off, n_groups, S.RD.n));
    const uint32_t G = (uint32_t)n_groups; S.G = G; S.N = S.RD.n; S.NL = grp_off[n_groups];
    S.boff.assign(G + 1, 0); S.B.resize(G);
    if (G) {
        if (centres->mem == NGSID_MEM_DEVICE) {
            HIPCHK(ctx, hipMemcpy(S.boff.data(), centres->off, 8 * (G + 1), hipMemcpyDeviceToHost)); S.bseq.resize(S.boff[G] + 1);
            if (S.boff[G]) HIPCHK(ctx, hipMemcpy(S.bseq.data(), centres->seq, S.boff[G], hipMemcpyDeviceToHost));
        } else { memcpy(S.boff.data(), centres->off, 8 * (G + 1)); S.bseq.assign(centres->seq, centres->seq + S.boff[G]); S.bseq.push_back(0); }
    }
    for (uint32_t g = 0; g < G; ++g) { S.B[g].assign((const char*)S.bseq.data() + S.boff[g], (size_t)(S.boff[g + 1] - S.boff[g])); S.maxb = std::max<uint32_t>(S.maxb, (uint32_t)S.B[g].size()); }
    return NGSID_OK;
}

// ... second half: the read -> group map, strands and oriented copies, the pairs in list order (group by group)
int32_t ngsid_groups_pairs(ngsid_ctx* ctx, const uint32_t* read_order, const uint64_t* grp_off, int k, int w, GroupedReads& S, int8_t* strand)
{
    static thread_local PinVec<uint8_t> h_orient; static thread_local PinVec<uint32_t> pair_read, pair_group, pair_x;
    S.h_orient = &h_orient; S.pair_read = &pair_read; S.pair_group = &pair_group; S.pair_x = &pair_x; pair_read.clear(); pair_group.clear(); pair_x.clear();
    const uint32_t G = S.G; const OffView& off = S.RD.h_off;
    S.h_rgroup.assign(S.N, 0xffffffffu); S.gbases.assign(G, 0);
    for (uint32_t g = 0; g < G; ++g) {
        uint64_t tot = 0;
        for (uint64_t x = grp_off[g]; x < grp_off[g + 1]; ++x) {
            const uint64_t r = read_order ? read_order[x] : x;
            if (S.h_rgroup[r] != 0xffffffffu) NGSID_FAIL(ctx, NGSID_ERR_ARG, "read %llu is listed twice (groups %u and %u): strand and layers are kept per read, list every read under one centre (backbone)", (unsigned long long)r, S.h_rgroup[r], g);
            S.h_rgroup[r] = g; tot += off[r + 1] - off[r];
        }
        S.gbases[g] = tot;
    }
    NGSID_TRY(ngsid_polish_orient(ctx, S.RD, S.B, S.h_rgroup, k, w, S.ob, h_orient));
    S.gbeg.assign(G + 1, 0);
    for (uint32_t g = 0; g < G; ++g) {
        for (uint64_t x = grp_off[g]; x < grp_off[g + 1]; ++x) {
            const uint64_t r = read_order ? read_order[x] : x;
            if (h_orient[r] == 255) continue;
            pair_read.push_back((uint32_t)r); pair_group.push_back(g); pair_x.push_back((uint32_t)x); if (strand) strand[x] = (int8_t)h_orient[r];
        }
        S.gbeg[g + 1] = pair_read.size();
    }
    S.NP = pair_read.size();
    return NGSID_OK;
}

namespace {

struct PolishTrace { std::vector<std::string> seq; std::vector<uint64_t> used; int32_t* aln = nullptr; };      // seq, used: [it * G + g], the backbones after every iteration; aln (ngsid_polish_trace_aln): [(it * n_listed + x) * 6 ...] = the read -> backbone alignment of listed read x in iteration it

// The alignment records of iteration `it` (NL x 6 from aln + it * NL * 6) start as the previous iteration's - a stable group has the same backbone and the same reads: the
// same alignments - and as -1 (not aligned: no PAF line) in iteration 0; the pairs aligned in the iteration then overwrite theirs
static void open_aln_records(int32_t* aln, size_t it, uint64_t NL) { int32_t* A = aln + it * NL * 6; if (it == 0) std::fill(A, A + NL * 6, -1); else memcpy(A, A - NL * 6, sizeof(int32_t) * NL * 6); }

// What one call of ngsid_polish* owns, and the steps of its iterations (polish_impl calls them in order).  Iter is what one iteration builds: made at its start and destroyed
// at its end (a DevBuf's destructor waits for the stream).
struct PolishRun {
    ngsid_ctx* ctx; const ngsid_polish_params_t* prm; PolishTrace* trace; const bool want_aln; const int W; HostTimer ht;
    GroupedReads S; uint64_t NP = 0; int iters_done = 0;      // S.B: the current backbones (tiny, rebuilt on the host after every iteration); NP: pairs still aligned (S.pair_*, S.gbeg)
    std::vector<uint8_t> tgs, stable; std::vector<uint64_t> used;      // per group: the TGS window type (mean read length above 1000); stop_when_stable: the last iteration returned the backbone unchanged; reads with a layer in the last iteration that ran it
    DevBuf<int> flag; DevBuf<int32_t> d_dist; DevBuf<uint32_t> d_pair_read, d_pair_group; DevBuf<int32_t> d_open, d_span, d_blen;      // (declared in the order open() fills them: they go back to the block cache in reverse)
    PinVec<int32_t> *h_span = nullptr, *h_dist = nullptr; PinVec<uint16_t>* h_valid = nullptr;      // the thread's pinned host mirrors (open)
    struct Iter {
        std::vector<uint64_t> boff; std::string cat; std::vector<int32_t> blen; int nwinmax = 1; uint32_t maxb = 0; DevReads BB; int max_layer = 1, aln_mode = 0;      // the backbones of the iteration, its longest layer, its aligner
        std::vector<Unit> units; std::vector<std::pair<uint32_t, int>> unit_gw; std::vector<size_t> nlayers;      // units = (group, window) with their layers; nlayers: before the under-two rule
        std::vector<PSeq> bbs; std::vector<int> bb_len; DevBuf<PSeq> d_bbs;                                         // the windows of the units that run
    };
    PolishRun(ngsid_ctx* c, const ngsid_polish_params_t* p, PolishTrace* t) : ctx(c), prm(p), trace(t), want_aln(t && t->aln), W(p->window > 0 ? p->window : 500), ht(c->stream, "polish") {}
    bool finished() const { return S.N == 0 || S.G == 0 || std::find(stable.begin(), stable.end(), 0) == stable.end(); }      // nothing listed, or every group stable
    int32_t open(const ngsid_reads_t* backbones, const ngsid_reads_t* reads, const uint32_t* read_order, const uint64_t* grp_off, uint64_t n_groups)      // the reads, then (unless nothing is listed) strands and pairs (usable reads that belong to a group), fixed over the iterations; the window type of every group
    {
        NGSID_TRY(ngsid_groups_open(ctx, backbones, reads, read_order, grp_off, n_groups, S));
        const uint32_t G = S.G; used.assign(G, 0); stable.assign(G, 0); tgs.assign(G, 0);
        ht.mark("upload + checks");
        if (S.N == 0 || G == 0) return NGSID_OK;
        HIPCHK(ctx, flag.alloc(1)); NGSID_TRY(ngsid_groups_pairs(ctx, read_order, grp_off, prm->k, prm->w, S));
        for (uint32_t g = 0; g < G; ++g) { const uint64_t ns = grp_off[g + 1] - grp_off[g]; tgs[g] = ns > 0 && ((double)S.gbases[g] / (double)ns) > 1000.0; }
        ht.mark("group map + minimizers + strand + orient");
        static thread_local PinVec<int32_t> v_span, v_dist; static thread_local PinVec<uint16_t> v_valid; h_span = &v_span; h_dist = &v_dist; h_valid = &v_valid; NP = S.NP;
        if (want_aln) { HIPCHK(ctx, d_dist.alloc(NP + 1)); v_span.resize(NP * 4 + 4); v_dist.resize(NP + 1); }
        NGSID_TRY(dev_put(ctx, d_pair_read, S.pair_read->data(), NP)); NGSID_TRY(dev_put(ctx, d_pair_group, S.pair_group->data(), NP)); HIPCHK(ctx, d_open.alloc(NP)); HIPCHK(ctx, d_span.alloc(NP * 4)); HIPCHK(ctx, d_blen.alloc(G));
        if (NP) HIPCHK(ctx, hipMemsetD32Async((hipDeviceptr_t)d_open.p, prm->aln_open, NP, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        ht.mark("orient + pairs");
        return NGSID_OK;
    }
    int32_t drop_stable_pairs(int it)      // stop_when_stable: the pairs of the stable groups go (their reads would be aligned and stacked into exactly the same windows again); the others keep their order
    {
        if (!prm->stop_when_stable || it == 0) return NGSID_OK;
        PinVec<uint32_t> &pair_read = *S.pair_read, &pair_group = *S.pair_group, &pair_pos = *S.pair_x; size_t keep = 0;
        for (size_t p = 0; p < NP; ++p) if (!stable[pair_group[p]]) { pair_read[keep] = pair_read[p]; pair_group[keep] = pair_group[p]; pair_pos[keep] = pair_pos[p]; ++keep; }
        if (keep == NP) return NGSID_OK;
        pair_read.resize(keep); pair_group.resize(keep); pair_pos.resize(keep); NP = keep;
        S.gbeg.assign(S.G + 1, 0); for (size_t p = 0; p < NP; ++p) S.gbeg[pair_group[p] + 1]++; for (uint32_t g = 0; g < S.G; ++g) S.gbeg[g + 1] += S.gbeg[g];
        if (NP) { HIPCHK(ctx, hipMemcpyAsync(d_pair_read.p, pair_read.data(), 4 * NP, hipMemcpyHostToDevice, ctx->stream)); HIPCHK(ctx, hipMemcpyAsync(d_pair_group.p, pair_group.data(), 4 * NP, hipMemcpyHostToDevice, ctx->stream)); HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); }
        return NGSID_OK;
    }
    int32_t upload_backbones(Iter& I)      // the current backbones on the device; the counts and the layer-length flag of the iteration cleared
    {
        const uint32_t G = S.G; const std::vector<std::string>& B = S.B; I.boff.assign(G + 1, 0); I.blen.resize(G);
        for (uint32_t g = 0; g < G; ++g) { I.cat += B[g]; I.boff[g + 1] = I.cat.size(); I.blen[g] = (int32_t)B[g].size(); I.nwinmax = std::max(I.nwinmax, (int)((B[g].size() + W - 1) / W)); I.maxb = std::max<uint32_t>(I.maxb, (uint32_t)B[g].size()); }
        ngsid_reads_t br{(const uint8_t*)I.cat.data(), nullptr, I.boff.data(), G, NGSID_MEM_HOST, 0};
        NGSID_TRY(ngsid_upload_reads(ctx, &br, &I.BB, false));
        HIPCHK(ctx, hipMemcpyAsync(d_blen.p, I.blen.data(), 4 * G, hipMemcpyHostToDevice, ctx->stream));
        for (uint32_t g = 0; g < G; ++g) if (!stable[g]) used[g] = 0;
        HIPCHK(ctx, hipMemsetAsync(flag.p, 0, sizeof(int), ctx->stream));
        return NGSID_OK;
    }
    int32_t align_and_layers(Iter& I)      // every pair against its backbone (break points per raw window, spans), the layers of every (pair, window) with their validity; the host has them at return
    {
        if (!NP) return NGSID_OK;
        const DevReads& RD = S.RD; const int nwinmax = I.nwinmax; const uint64_t T = NP * (uint64_t)nwinmax; int32_t rc;
        DevBuf<int32_t>& d_bp = ctx->pol_bp; DevBuf<uint8_t>& d_lay_raw = ctx->pol_lay; DevBuf<uint16_t>& d_valid = ctx->pol_valid;
        HIPCHK(ctx, d_bp.reserve(T * 4)); HIPCHK(ctx, d_lay_raw.reserve(sizeof(PSeq) * T)); HIPCHK(ctx, d_valid.reserve(T));
        AlignJob J{};
        J.qseq = ctx->pol_oseq.p; J.qoff = RD.off; J.tseq = I.BB.seq; J.toff = I.BB.off; J.qidx = d_pair_read.p; J.tidx = d_pair_group.p; J.npairs = NP;
        J.match = prm->aln_match; J.mismatch = prm->aln_mismatch; J.ext = prm->aln_ext; J.k = 1; J.open = d_open.p; J.match_id = nullptr;
        J.score = nullptr; J.ncols = nullptr; J.nmatch = nullptr; J.region = nullptr; J.bp = d_bp.p; J.bp_windows = nwinmax; J.window = W; J.span = d_span.p;
        int aln_mode = prm->aln_mode & ~NGSID_ALN_SUBGRAPH; if (aln_mode == 2) aln_mode = 1;      // (the sub-graph flag is a rule of the window layers, not of this aligner)
        if (aln_mode == 3) { aln_mode = 1; J.clip = 1; }          // edit distance + overlap-span clipping (include/ngsid.h)
        if (aln_mode == 1) rc = ngsid_launch_ed_align(ctx, J, RD.maxlen, I.maxb, want_aln ? d_dist.p : nullptr);          // unit-cost, bit-parallel (k_ed_align.hip)
        else rc = ngsid_launch_align(ctx, J, RD.maxlen, I.maxb, prm->aln_open);
        if (rc) return rc; I.aln_mode = aln_mode;
        { ProfScope ps_(ctx, "k_layers"); hipLaunchKernelGGL(k_layers, dim3(NGSID_GRID(ctx, (T + 3) / 4, 256, "k_layers")), dim3(256), 0, ctx->stream, ctx->pol_oseq.p, RD.qual ? ctx->pol_oqual.p : nullptr, RD.off, d_pair_read.p, d_pair_group.p, NP, nwinmax,
                           d_bp.p, d_span.p, d_blen.p, W, prm->quality_threshold, prm->error_threshold, (prm->aln_mode & NGSID_ALN_SUBGRAPH) ? 1 : 0, (PSeq*)d_lay_raw.p, d_valid.p, flag.p); }
        HIPCHK(ctx, hipGetLastError()); h_valid->resize(T);
        HIPCHK(ctx, hipMemcpyAsync(&I.max_layer, flag.p, 4, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(h_valid->data(), d_valid.p, 2 * T, hipMemcpyDeviceToHost, ctx->stream));
        if (want_aln) { HIPCHK(ctx, hipMemcpyAsync(h_span->data(), d_span.p, 16 * NP, hipMemcpyDeviceToHost, ctx->stream)); if (aln_mode == 1) HIPCHK(ctx, hipMemcpyAsync(h_dist->data(), d_dist.p, 4 * NP, hipMemcpyDeviceToHost, ctx->stream)); }
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        return NGSID_OK;
    }
    void record_alignments(const Iter& I, int it)      // ngsid_polish_trace_aln: the PAF records of the iteration, fresh ones for the pairs just aligned (the read's interval on its ORIGINAL strand)
    {
        if (!want_aln) return; open_aln_records(trace->aln, it, S.NL);
        int32_t* A = trace->aln + (size_t)it * S.NL * 6; const PinVec<int32_t>& sp = *h_span;
        for (uint64_t p = 0; p < NP; ++p) {
            int32_t* a = A + (size_t)(*S.pair_x)[p] * 6; const uint32_t r = (*S.pair_read)[p]; const int32_t ql = (int32_t)(S.RD.h_off[r + 1] - S.RD.h_off[r]);
            const int32_t qf = sp[p * 4], qe = sp[p * 4 + 1], tf = sp[p * 4 + 2], te = sp[p * 4 + 3];
            if (qf < 0) { for (int c = 0; c < 6; ++c) a[c] = -1; continue; }
            const bool rcs = (*S.h_orient)[r] == 1;
            a[0] = rcs ? 1 : 0; a[1] = rcs ? ql - 1 - qe : qf; a[2] = rcs ? ql - qf : qe + 1; a[3] = tf; a[4] = te + 1; a[5] = I.aln_mode == 1 ? (*h_dist)[p] : -1;
        }
    }
    void window_units(Iter& I)      // units = the (group, window)s of the groups that still run, with their layers as racon adds them; used = the reads of a group with a layer
    {
        const uint32_t G = S.G; std::vector<uint32_t> nwin(G, 0);
        for (uint32_t g = 0; g < G; ++g) { if (stable[g]) continue; nwin[g] = (uint32_t)polish_nwin((int)S.B[g].size(), W); for (uint32_t wdx = 0; wdx < nwin[g]; ++wdx) I.unit_gw.push_back({g, (int)wdx}); }
        const unsigned forced = (unsigned)ngsid_opt(ctx, "polish_unit_threads", 0);      // (ngsid_ctx_option takes 0 .. 16; 65 536 and 16 are carried over from the two fillers this builder replaced, not measured again)
        const unsigned threads = forced ? forced : NP < 65536 ? 1u : std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
        std::vector<std::vector<uint32_t>> lists; std::vector<uint64_t> with_layer;
        polish_build_units(h_valid->data(), I.nwinmax, S.gbeg, I.unit_gw, nwin, threads, lists, with_layer);
        I.units.resize(lists.size()); for (size_t u = 0; u < lists.size(); ++u) I.units[u].seqs = std::move(lists[u]);
        for (uint32_t g = 0; g < G; ++g) if (!stable[g]) used[g] = with_layer[g];
    }
    int32_t unit_backbones(Iter& I)      // the windows of the units that run (racon: fewer than 3 sequences incl. the backbone -> the window stays), and which of them run as ONE graph
    {
        std::vector<Unit>& units = I.units; I.nlayers.resize(units.size());
        for (size_t u = 0; u < units.size(); ++u) {
            I.nlayers[u] = units[u].seqs.size();
            if (units[u].seqs.size() < 2) { units[u].seqs.clear(); units[u].done = true; continue; }
            const uint32_t g = I.unit_gw[u].first; const int ws = I.unit_gw[u].second * W; const int wlen = polish_wlen((int)S.B[g].size(), W, I.unit_gw[u].second);
            PSeq P; P.s = I.BB.seq + I.boff[g] + ws; P.q = nullptr; P.len = wlen; P.uw = 0; P.cw = 0; P.mode = NGSID_POA_GLOBAL; P.a0 = 0; P.a1 = -1;
            units[u].bb = (int)I.bbs.size(); I.bbs.push_back(P); I.bb_len.push_back(wlen);
        }
        NGSID_TRY(dev_put(ctx, I.d_bbs, I.bbs.data(), I.bbs.size()));
        if (prm->single_below > 0) for (Unit& U : units) {       // windows with few layers: ONE graph; the longest sequence that can enter it = the longest READ behind its layers, or the window
            if (U.done || U.seqs.size() >= (size_t)prm->single_below) continue;
            uint32_t mx = (uint32_t)std::max(1, I.bb_len[U.bb]); for (uint32_t id : U.seqs) { const uint32_t r = (*S.pair_read)[id / (uint32_t)I.nwinmax]; mx = std::max<uint32_t>(mx, (uint32_t)(S.RD.h_off[r + 1] - S.RD.h_off[r])); }
            U.single_maxlen = mx;
        }
        return NGSID_OK;
    }
    int32_t hierarchy(Iter& I)
    {
        bool any_tgs = prm->trim == 2; for (uint32_t g = 0; g < S.G; ++g) any_tgs = any_tgs || (tgs[g] && prm->trim);
        HierParams hp{prm->match, prm->mismatch, prm->gap, prm->band > 0 ? prm->band : (S.RD.maxlen <= NGSID_POA_BAND64_MAXLEN ? 64 : 128), prm->node_cap, prm->tile_depth, NGSID_POA_GLOBAL, any_tgs, (prm->trim >= 2 ? 1 : 0) | (prm->trim == 3 ? 4 : 0)};      // trim_tiles: 1 = trim tile consensuses, 4 = except the tile that ends a unit (trim 3)
        hp.single_below = prm->single_below > 0 ? prm->single_below : 0; hp.sub = (prm->aln_mode & NGSID_ALN_SUBGRAPH) != 0;
        return run_hierarchy(ctx, (const PSeq*)ctx->pol_lay.p, (uint32_t)std::max(I.max_layer, 1), I.d_bbs.p, I.bb_len, I.units, hp);
    }
    void stitch_backbones(const Iter& I)      // new backbones: window consensuses (coverage-trimmed where the rule says so; the old window where there is none) end to end; unchanged ones become stable
    {
        const uint32_t G = S.G; std::vector<std::string>& B = S.B; std::vector<std::string> NB(G);
        for (size_t u = 0; u < I.units.size(); ++u) {
            const Unit& U = I.units[u]; const uint32_t g = I.unit_gw[u].first; const int ws = I.unit_gw[u].second * W; const int wlen = polish_wlen((int)B[g].size(), W, I.unit_gw[u].second);
            std::string c = U.has_result ? U.result : std::string();
            if (!c.empty() && prm->trim && (tgs[g] || prm->trim == 2) && U.cov.size() == c.size()) {      // trim 3: racon's window rule (TGS only) with trimmed tiles
                const uint32_t avg = (uint32_t)(I.nlayers[u] / 2); int b = 0, e = (int)c.size() - 1;
                for (; b < (int)c.size(); ++b) if (U.cov[b] >= avg) break; for (; e >= 0; --e) if (U.cov[e] >= avg) break;
                if (b < e) c = c.substr(b, e - b + 1);
            }
            NB[g] += c.empty() ? B[g].substr(ws, wlen) : c;
        }
        for (uint32_t g = 0; g < G; ++g) { if (stable[g]) NB[g] = B[g]; else if (prm->stop_when_stable && NB[g] == B[g]) stable[g] = 1; }
        B.swap(NB); ++iters_done;
        if (trace) for (uint32_t g = 0; g < G; ++g) { trace->seq.push_back(B[g]); trace->used.push_back(used[g]); }
    }
    int32_t finish(uint64_t* out_off, uint8_t* out, uint64_t out_cap, uint64_t* needed, uint64_t* n_used)      // the iterations that did not run (nothing listed, every group stable) return what the last one did; the backbones behind their offsets
    {
        if (trace) for (int it = iters_done; it < prm->iters; ++it) {
            if (want_aln) open_aln_records(trace->aln, it, S.NL);
            for (uint32_t g = 0; g < S.G; ++g) { trace->seq.push_back(S.B[g]); trace->used.push_back(used[g]); }
        }
        if (n_used) std::copy(used.begin(), used.end(), n_used);
        return ngsid_pack_strings(ctx, "output", S.G, [&](size_t g) -> const std::string& { return S.B[g]; }, out_off, out, out_cap, needed, trace != nullptr);      // (ngsid_polish_trace hands no buffer in: it returns the trace's strings)
    }
};

static int32_t polish_impl(ngsid_ctx* ctx, const ngsid_reads_t* backbones, const ngsid_reads_t* reads, const uint32_t* read_order,
                           const uint64_t* grp_off, uint64_t n_groups, const ngsid_polish_params_t* prm,
                           uint64_t* out_off, uint8_t* out, uint64_t out_cap, uint64_t* needed, uint64_t* n_used, PolishTrace* trace)
{
    if (!ctx) return NGSID_ERR_ARG;
    if (!prm || !out_off) NGSID_FAIL(ctx, NGSID_ERR_ARG, "null argument");
    PolishRun run(ctx, prm, trace);
    NGSID_TRY(run.open(backbones, reads, read_order, grp_off, n_groups));
    for (int it = 0; it < prm->iters && !run.finished(); ++it) {
        NGSID_TRY(run.drop_stable_pairs(it));
        PolishRun::Iter I;
        NGSID_TRY(run.upload_backbones(I));
        NGSID_TRY(run.align_and_layers(I));
        run.record_alignments(I, it);
        run.ht.mark("align + layers + valid copy");
        run.window_units(I);
        NGSID_TRY(run.unit_backbones(I));
        run.ht.mark("unit lists");
        NGSID_TRY(run.hierarchy(I));
        run.ht.mark("hierarchy");
        run.stitch_backbones(I);
    }
    return run.finish(out_off, out, out_cap, needed, n_used);
}

}  // namespace

extern "C" int32_t ngsid_polish(ngsid_ctx* ctx, const ngsid_reads_t* backbones, const ngsid_reads_t* reads, const uint32_t* read_order,
                                const uint64_t* grp_off, uint64_t n_groups, const ngsid_polish_params_t* prm,
                                uint64_t* out_off, uint8_t* out, uint64_t out_cap, uint64_t* needed, uint64_t* n_used)
{
    ApiClock api_clock_(ctx, "polish");
    return polish_impl(ctx, backbones, reads, read_order, grp_off, n_groups, prm, out_off, out, out_cap, needed, n_used, nullptr);
}

static int32_t polish_trace_impl(ngsid_ctx* ctx, const ngsid_reads_t* backbones, const ngsid_reads_t* reads, const uint32_t* read_order,
                                 const uint64_t* grp_off, uint64_t n_groups, const ngsid_polish_params_t* prm,
                                 uint64_t* it_off, uint8_t* it_out, uint64_t it_cap, uint64_t* needed, uint64_t* it_used, int32_t* it_aln)
{
    if (!ctx) return NGSID_ERR_ARG;
    if (!prm || !it_off || prm->iters < 1) NGSID_FAIL(ctx, NGSID_ERR_ARG, "ngsid_polish_trace: null argument or iters < 1");
    PolishTrace tr; tr.aln = it_aln; std::vector<uint64_t> ooff(n_groups + 1, 0); uint64_t need1 = 0;
    const int32_t rc = polish_impl(ctx, backbones, reads, read_order, grp_off, n_groups, prm, ooff.data(), nullptr, 0, &need1, nullptr, &tr);
    if (rc != NGSID_OK) return rc;                                        // (with a trace the inner call copies nothing out and checks no capacity: ADVICE r4)
    if (tr.seq.size() != (size_t)prm->iters * n_groups || tr.used.size() != tr.seq.size()) NGSID_FAIL(ctx, NGSID_ERR_HIP, "internal: polish trace holds %zu entries for %d x %llu", tr.seq.size(), (int)prm->iters, (unsigned long long)n_groups);
    if (it_used) std::copy(tr.used.begin(), tr.used.end(), it_used);
    return ngsid_pack_strings(ctx, "trace", tr.seq.size(), [&](size_t x) -> const std::string& { return tr.seq[x]; }, it_off, it_out, it_cap, needed);
}
extern "C" int32_t ngsid_polish_trace(ngsid_ctx* ctx, const ngsid_reads_t* backbones, const ngsid_reads_t* reads, const uint32_t* read_order,
                                      const uint64_t* grp_off, uint64_t n_groups, const ngsid_polish_params_t* prm,
                                      uint64_t* it_off, uint8_t* it_out, uint64_t it_cap, uint64_t* needed, uint64_t* it_used)
{
    ApiClock api_clock_(ctx, "polish_trace");
    return polish_trace_impl(ctx, backbones, reads, read_order, grp_off, n_groups, prm, it_off, it_out, it_cap, needed, it_used, nullptr);
}
// (a17, boundary 8b(1)) ngsid_polish_trace + what minimap2 leaves in read_alignments_it_{i}.paf (consensus.py:112-121): the read -> backbone alignment of every LISTED read in
// every iteration, it_aln[(it * n_listed + x) * 6 ...] = {strand (0 +, 1 -, -1 = not aligned: no PAF line), q_begin, q_end, t_begin, t_end, edit distance}, PAF coordinates
// (0-based, end exclusive, the query interval on the read's ORIGINAL strand); n_listed = grp_off[n_groups].
extern "C" int32_t ngsid_polish_trace_aln(ngsid_ctx* ctx, const ngsid_reads_t* backbones, const ngsid_reads_t* reads, const uint32_t* read_order,
                                          const uint64_t* grp_off, uint64_t n_groups, const ngsid_polish_params_t* prm,
                                          uint64_t* it_off, uint8_t* it_out, uint64_t it_cap, uint64_t* needed, uint64_t* it_used, int32_t* it_aln)
{
    ApiClock api_clock_(ctx, "polish_trace");
    if (ctx && !it_aln) NGSID_FAIL(ctx, NGSID_ERR_ARG, "ngsid_polish_trace_aln: null alignment buffer");
    return polish_trace_impl(ctx, backbones, reads, read_order, grp_off, n_groups, prm, it_off, it_out, it_cap, needed, it_used, it_aln);
}
