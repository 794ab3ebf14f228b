// k_align.hip - (a10,a15) batched semi-global affine alignment WITH traceback, one 64-lane wave per pair.
//
// Replaces parasail.sg_trace_scan_16/32 + cigar_to_seq + the k-column identity windows of
// cluster.py:130-169, and the identity count of consensus.py:129-145.  Also produces racon-style window
// break points for the polisher (replaces the edlib NW walk of racon's overlap.cpp).
//
// Mapping to CDNA4: lane l owns RPL consecutive query rows; the wave sweeps target columns as a systolic
// anti-diagonal (lane l works on column tau-l at step tau), the row-boundary (H,F) pair moves to the next
// lane with one cross-lane shift per step, H/E of the lane's rows live in VGPRs, the target is staged in
// LDS.  Every step each lane emits 4 traceback bits per cell (2 H-source, 1 E-extend, 1 F-extend) packed
// in one 64-bit word -> a fully coalesced 512 B store per wave per step.  The traceback then walks the
// words backwards and folds the k-column window statistic on the fly in a 64-bit shift register
// (the window count is symmetric under path reversal), so no CIGAR or gapped strings ever exist in HBM.
// Integer work throughout (int32 scores); bound by VALU issue, not by HBM: ~0.5 KB of traceback per
// DP step versus ~300 VALU ops.
// This file also holds the host side of all three aligners (this int32 kernel, k_sg_align16 of k_align16.hip, k_sg_align16p of
// k_align16p.hip): the query-length class table, the launch plans, and ngsid_launch_align, which decides which kernel a pair gets.
#include "k_align_common.h"
#include <algorithm>
#include <type_traits>

#define NEGINF (-(1 << 29))

template <int RPL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 4)))
void k_sg_align(AlignJob J, uint64_t* __restrict__ tb, uint64_t tb_words_per_wave, int32_t* __restrict__ bnd, uint32_t bnd_stride, uint32_t lds_per_wave, uint32_t* __restrict__ work_ctr)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63;
    const int wib = threadIdx.x >> 6;
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + wib;
    uint8_t* tgt = smem + (size_t)wib * lds_per_wave;                 // raw target, raw query, 4 KB traceback block
    const uint32_t seq_lds = (lds_per_wave - 4096) / 2;
    uint8_t* qry = tgt + seq_lds;
    uint64_t* tbblk = (uint64_t*)(tgt + 2 * (size_t)seq_lds);
    uint64_t* mytb = tb + wave * tb_words_per_wave;
    int32_t* mybnd = bnd + wave * (uint64_t)bnd_stride * 2;
    const int STRIP = 64 * RPL;

    for (;;) {
        // persistent waves pull pairs from a queue: the grid is sized to what is resident, so there is no tail of idle SIMDs
        uint32_t pq = 0; if (lane == 0) pq = atomicAdd(work_ctr, 1u);
        const uint64_t px = (uint32_t)__builtin_amdgcn_readfirstlane((int)pq);
        if (px >= (J.npairs_dev ? (uint64_t)*J.npairs_dev : J.npairs)) break;
        const uint64_t p = J.pair_list ? (uint64_t)J.pair_list[px] : px;       // (round 5: the long-pair class of a partitioned batch comes as an index list with its count on the device)
        const uint32_t qi = J.qidx[p], ti = J.tidx[p];
        const uint8_t* q = J.qseq + J.qoff[qi]; const int n = (int)(J.qoff[qi + 1] - J.qoff[qi]);
        const uint8_t* t = J.tseq + J.toff[ti]; const int m = (int)(J.toff[ti + 1] - J.toff[ti]);
        const int gopen = J.open[p], gext = J.ext, smatch = J.match, smis = J.mismatch;
        if (n <= 0 || m <= 0) { sg_degenerate(J, p, n, m, lane); continue; }
        for (int x = lane; x < m; x += 64) tgt[x] = t[x];
        for (int x = lane; x < n; x += 64) qry[x] = q[x];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();

        const int steps = m + 63;
        const int nstrips = (n + STRIP - 1) / STRIP;
        int bestRowV = NEGINF, bestRowJ = 0;       // last query row (ascending column, first maximum)
        int bestColV = NEGINF, bestColI = 0x7fffffff;   // last target column (ascending row, strictly larger only)

        for (int sidx = 0; sidx < nstrips; ++sidx) {
            const int i0 = sidx * STRIP + lane * RPL;
            int qc[RPL], hl[RPL], e[RPL];
#pragma unroll
            for (int r = 0; r < RPL; ++r) { qc[r] = (i0 + r < n) ? ngsid_bcode(qry[i0 + r]) : 4; hl[r] = 0; e[r] = NEGINF; }
            const int rlast = (n - 1) - i0;            // row n-1 lives in this lane iff 0 <= rlast < RPL
            int hdiag_top = 0;                         // H[i0-1][j-1]
            int send_h = 0, send_f = NEGINF;
            uint64_t* stb = mytb + (uint64_t)sidx * steps * 64;
            for (int tau = 0; tau < steps; ++tau) {
                const int j = tau - lane;
                // lane l-1 -> lane l in one DPP move (wave_shr:1), no LDS crossbar round trip
                int hup = __builtin_amdgcn_update_dpp(0, send_h, 0x138, 0xf, 0xf, false), fup = __builtin_amdgcn_update_dpp(0, send_f, 0x138, 0xf, 0xf, false);
                if (lane == 0) {
                    if (sidx == 0) { hup = 0; fup = NEGINF; }
                    else if (j >= 0 && j < m) {
                        hup = __hip_atomic_load(&mybnd[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        fup = __hip_atomic_load(&mybnd[bnd_stride + j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                }
                if (j >= 0 && j < m) {
                    const int tc = ngsid_bcode(tgt[j]);
                    int hd = hdiag_top, hu = hup, f = fup;
                    uint64_t word = 0;
#pragma unroll
                    for (int r = 0; r < RPL; ++r) {
                        const int e_ext = e[r] - gext, e_opn = hl[r] - gopen;
                        const int ebit = e_ext >= e_opn; const int E = ebit ? e_ext : e_opn;
                        const int f_ext = f - gext, f_opn = hu - gopen;
                        const int fbit = f_ext >= f_opn; const int F = fbit ? f_ext : f_opn;
                        const int a = qc[r];
                        const int sc = ((a | tc) > 3) ? 0 : (a == tc ? smatch : smis);
                        const int d = hd + sc;
                        int h, src;
                        if (d >= E && d >= F) { h = d; src = 0; } else if (E >= F) { h = E; src = 1; } else { h = F; src = 2; }
                        word |= (uint64_t)(src | (ebit << 2) | (fbit << 3)) << (4 * r);
                        hd = hl[r]; hl[r] = h; e[r] = E; hu = h; f = F;
                    }
                    hdiag_top = hup;
                    send_h = hu; send_f = f;
                    stb[(uint64_t)tau * 64 + lane] = word;
                    // lane 63 hands the strip's bottom row to the next strip through HBM.  In-place is safe: lane 0 of
                    // this strip consumed bnd[j] 63 steps ago.  Agent-scope relaxed accesses keep the hand-off out of L1.
                    if (lane == 63 && sidx + 1 < nstrips) {
                        __hip_atomic_store(&mybnd[j], hu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        __hip_atomic_store(&mybnd[bnd_stride + j], f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                    if (rlast >= 0 && rlast < RPL) {
                        int v = hl[0];
#pragma unroll
                        for (int r = 1; r < RPL; ++r) if (r == rlast) v = hl[r];
                        if (v > bestRowV) { bestRowV = v; bestRowJ = j; }
                    }
                    if (j == m - 1) {
#pragma unroll
                        for (int r = 0; r < RPL; ++r) if (i0 + r < n && hl[r] > bestColV) { bestColV = hl[r]; bestColI = i0 + r; }
                    }
                }
            }
            if (nstrips > 1) { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent"); __builtin_amdgcn_s_waitcnt(0); }
        }
        // ---- end cell (in the last row exactly one lane, the owner of row n-1 in the last strip, holds a value)
        int ei, ej, best;
        sg_end_cell(bestRowV, bestRowJ, bestColV, bestColI, n, m, ei, ej, best);

        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_s_waitcnt(0);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");

        // ---- traceback: executed uniformly by the whole wave; traceback words are pulled 64 steps x 8 lanes (4 KB) at a time
        //      into LDS (one HBM round trip per ~64 path steps instead of one per step), sequences are read from LDS.
        //      The bookkeeping is that of the int16 kernels (k_align_common.h); this walk alone also writes the alignment columns.
        sg_bp_clear(J, p, lane);
        {
            SgWindows w(J.k, J.match_id ? J.match_id[p] : J.k);
            uint8_t* opp = J.ops ? J.ops + J.ops_off[p] : nullptr; int oc = 0;      // optional: the alignment columns themselves, in traceback (reverse) order
            if (opp && lane == 0) { for (int x = n - 1; x > ei; --x) opp[oc++] = 2; for (int x = m - 1; x > ej; --x) opp[oc++] = 3; }
            w.end_gaps((n - 1 - ei) + (m - 1 - ej));       // trailing end gaps (walked first)
            int i = ei, j = ej, state = 0;
            int q_end = -1, t_end = -1, q_beg = -1, t_beg = -1;
            int cw = -1, w_qf = 0, w_ql = 0, w_tf = 0, w_tl = 0;
            int32_t* bpp = J.bp ? J.bp + p * (uint64_t)J.bp_windows * 4 : nullptr;
            int blk_s = -1, blk_g = -1, blk_hi = -1;       // loaded block: strip, 8-lane group, highest step
            // (every round of the walk takes at least one step or reloads a block once per 64 steps: the bound is never reached; it turns a corrupted traceback word into a wrong
            // result the parity tests catch instead of a wave that never ends)
            for (int guard = 4 * (n + m) + 512; i >= 0 && j >= 0 && guard > 0; --guard) {
                const int sidx = i / STRIP; const int il = i - sidx * STRIP; const int l = il / RPL; const int r = il - l * RPL;
                const int tau = j + l; const int grp = l >> 3;
                if (sidx != blk_s || grp != blk_g || tau > blk_hi || tau < blk_hi - 63) {
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    blk_s = sidx; blk_g = grp; blk_hi = tau;
                    const int tt = tau - lane;
                    if (tt >= 0) {
                        const uint4* src = (const uint4*)(mytb + ((uint64_t)sidx * steps + (uint64_t)tt) * 64 + grp * 8);
                        ngsid_v4u* dstp = (ngsid_v4u*)(tbblk + lane * 8);
                        // nt loads are served by L2: this wave rewrites the same scratch addresses for every pair, an L1 line may be stale
                        dstp[0] = ngsid_load16_l2(src + 0); dstp[1] = ngsid_load16_l2(src + 1); dstp[2] = ngsid_load16_l2(src + 2); dstp[3] = ngsid_load16_l2(src + 3);
                    }
                    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
                    __builtin_amdgcn_wave_barrier();
                }
                const uint64_t word = tbblk[(blk_hi - tau) * 8 + (l & 7)];
                const int v = (int)((word >> (4 * r)) & 15);
                int bit = 0, emit = 1;
                if (state == 0) {
                    const int src = v & 3;
                    if (src == 0) {
                        bit = (qry[i] == tgt[j]);
                        if (opp && lane == 0) opp[oc++] = bit ? 0 : 1;
                        if (q_end < 0) { q_end = i; t_end = j; }
                        q_beg = i; t_beg = j;
                        if (bpp) {
                            const int wn = j / J.window;
                            if (wn != cw) { if (lane == 0 && cw >= 0 && cw < J.bp_windows) { bpp[cw * 4 + 0] = w_qf; bpp[cw * 4 + 1] = w_ql; bpp[cw * 4 + 2] = w_tf; bpp[cw * 4 + 3] = w_tl; } cw = wn; w_ql = i; w_tl = j; }
                            w_qf = i; w_tf = j;
                        }
                        --i; --j;
                    } else { state = src; emit = 0; }
                } else if (state == 1) { if (opp && lane == 0) opp[oc++] = 3; if (!((v >> 2) & 1)) state = 0; --j; }
                else { if (opp && lane == 0) opp[oc++] = 2; if (!((v >> 3) & 1)) state = 0; --i; }
                if (emit) w.push(bit);
            }
            if (lane == 0 && bpp && cw >= 0 && cw < J.bp_windows) { bpp[cw * 4 + 0] = w_qf; bpp[cw * 4 + 1] = w_ql; bpp[cw * 4 + 2] = w_tf; bpp[cw * 4 + 3] = w_tl; }
            if (opp && lane == 0) { for (int x = i; x >= 0; --x) opp[oc++] = 2; for (int x = j; x >= 0; --x) opp[oc++] = 3; }
            w.end_gaps((i + 1) + (j + 1));                 // leading end gaps
            sg_store(J, p, lane, best, w.cols, w.nm, w.windows(), q_beg, q_end, t_beg, t_end);
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// ======== host side of the three aligners: plans, launches and the routing of pairs to kernels

// Persistent waves of a launch: as many as are resident at once (occupancy x CUs; wpb waves and lds bytes per block), no more than there are work items or
// than the traceback scratch budget holds (tb_bytes per wave), at least one block
static int32_t plan_waves(ngsid_ctx* ctx, const void* kernel, int wpb, size_t lds, uint64_t items, uint64_t tb_bytes, uint64_t* nwaves)
{
    int occ = 0;
    HIPCHK(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kernel, 64 * wpb, lds));
    if (occ < 1) occ = 1;
    const uint64_t want = std::max<uint64_t>(1, std::min<uint64_t>({items, ctx->scratch_budget / (tb_bytes + 1), (uint64_t)occ * ctx->n_cu * wpb}));
    *nwaves = (want + wpb - 1) / wpb * wpb;
    return NGSID_OK;
}

// One-pair kernels (k_sg_align, k_sg_align16): a lane owns `rows` query rows of a strip, a strip takes m + skew steps.  Per wave: the traceback words of all
// strips of a pair, the strip-boundary row (H, F) of bnd_stride entries each, and in LDS both sequences and a 4 KB traceback block
struct StripPlan { uint64_t words, nwaves; uint32_t lds_per_wave, bnd_stride; int wpb; };
static int32_t plan_strips(ngsid_ctx* ctx, const void* kernel, int rows, int skew, uint64_t npairs, uint32_t max_qlen, uint32_t max_tlen, StripPlan* L)
{
    const uint64_t strip = 64ull * rows, nstrips = (max_qlen + strip - 1) / strip;
    L->words = (nstrips ? nstrips : 1) * ((uint64_t)max_tlen + skew) * 64;
    const uint32_t seq_lds = ((max_tlen > max_qlen ? max_tlen : max_qlen) + 15u) & ~15u;
    L->lds_per_wave = 2 * seq_lds + 4096;
    L->bnd_stride = (max_tlen + 15u) & ~15u;
    int wpb = 4;
    while (wpb > 1 && (uint64_t)wpb * L->lds_per_wave > 40 * 1024) wpb >>= 1;
    L->wpb = wpb;
    const size_t lds = (size_t)wpb * L->lds_per_wave;
    if (lds > 160 * 1024) NGSID_FAIL(ctx, NGSID_ERR_TOO_LONG, "aligner needs %zu bytes of LDS per wave", lds);
    if (lds > 64 * 1024) HIPCHK(ctx, hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));   // reads above 30 k bases: both sequences of a pair in LDS are more than the default limit
    return plan_waves(ctx, kernel, wpb, lds, npairs, L->words * 8, &L->nwaves);
}

template <int RPL>
static int32_t launch_rpl(ngsid_ctx* ctx, const AlignJob& job, uint32_t max_qlen, uint32_t max_tlen, bool long_class = false)
{
    // long_class: the pairs above the int16 lengths of a partitioned batch - own scratch (the class launches of the same call are still running on theirs), own queue counter
    DevBuf<uint64_t>& TB = long_class ? ctx->tb_long : ctx->tb; DevBuf<int32_t>& BND = long_class ? ctx->bnd_long : ctx->bnd;
    const uint32_t ctr_slot = long_class ? 6u : 0u;
    StripPlan L; int32_t rc = plan_strips(ctx, (const void*)k_sg_align<RPL>, RPL, 63, job.npairs, max_qlen, max_tlen, &L); if (rc) return rc;
    if (ctx->aln_ctr.n < 16) HIPCHK(ctx, ctx->aln_ctr.alloc(16));
    HIPCHK(ctx, hipMemsetAsync(ctx->aln_ctr.p + ctr_slot, 0, sizeof(uint32_t), ctx->stream));
    if (TB.n < L.nwaves * L.words) HIPCHK(ctx, TB.alloc(L.nwaves * L.words));
    if (BND.n < L.nwaves * 2ull * L.bnd_stride) HIPCHK(ctx, BND.alloc(L.nwaves * 2ull * L.bnd_stride));
    { ProfScope ps_(ctx, "k_sg_align"); hipLaunchKernelGGL((k_sg_align<RPL>), dim3((unsigned)(L.nwaves / L.wpb)), dim3(64 * L.wpb), (size_t)L.wpb * L.lds_per_wave, ctx->stream,
                       job, TB.p, L.words, BND.p, L.bnd_stride, L.lds_per_wave, ctx->aln_ctr.p + ctr_slot); }
    HIPCHK(ctx, hipGetLastError());
    return NGSID_OK;
}

template <int RP>
static int32_t plan16(ngsid_ctx* ctx, uint64_t npairs, uint32_t max_qlen, uint32_t max_tlen, StripPlan* L)
{
    return plan_strips(ctx, (const void*)k_sg_align16<RP>, 2 * RP, 127, npairs, max_qlen, max_tlen, L);
}
// k_sg_align16<RP> on stream st: work-queue counter ctr (zeroed by the caller), scratch tb / bnd as planned by plan16
template <int RP>
static int32_t launch16(ngsid_ctx* ctx, const AlignJob& job, const StripPlan& L, hipStream_t st, uint32_t* ctr, uint64_t* tb, int32_t* bnd)
{
    { ProfScope ps_(ctx, st == ctx->stream ? "k_sg_align" : "k_sg_align_side", st);      // side-stream launches overlap the main one: timed under their own name
      hipLaunchKernelGGL((k_sg_align16<RP>), dim3((unsigned)(L.nwaves / L.wpb)), dim3(64 * L.wpb), (size_t)L.wpb * L.lds_per_wave, st,
                         job, tb, L.words, bnd, L.bnd_stride, L.lds_per_wave, ctr); }
    HIPCHK(ctx, hipGetLastError());
    return NGSID_OK;
}

// Paired kernel k_sg_align16p<R>: one wave per work item of two pairs, both traceback halves in one scratch slice (words_half words each); in LDS two targets,
// two queries and a 4 KB traceback block
struct PairedPlan { uint64_t words_half, nwaves; uint32_t seq_lds; size_t lds; };
template <int R, bool SKEW>
static int32_t plan16p(ngsid_ctx* ctx, uint64_t npairs, uint32_t max_tlen, PairedPlan* L)
{
    L->seq_lds = (std::max<uint32_t>(max_tlen, 64u * R) + 15u) & ~15u;
    L->lds = 4 * (size_t)L->seq_lds + 4096;
    L->words_half = ((uint64_t)max_tlen + 63) * 64;
    return plan_waves(ctx, (const void*)k_sg_align16p<R, SKEW>, 1, L->lds, (npairs + 1) / 2, 2 * L->words_half * 8, &L->nwaves);
}

// ---- binning of one length class by (n - 1) mod R for the paired kernel.  `list` / `count` = the class list of k_pair_classes (queries of 513 - 896 bases: n >= 1).
__global__ __launch_bounds__(256)
void k_pair_bins(AlignJob J, const uint32_t* __restrict__ list, const uint32_t* __restrict__ count, int R, uint8_t* __restrict__ bin_of, uint32_t* __restrict__ bin_cnt /* [PBINS] */)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int bin = -1;
    if (k < *count) {
        const uint64_t p = list[k]; const uint32_t qi = J.qidx[p];
        const int n = (int)(J.qoff[qi + 1] - J.qoff[qi]);
        bin = n >= 1 ? (n - 1) % R : 0;
        bin_of[k] = (uint8_t)bin;
    }
    for (int b = 0; b < PBINS; ++b) {                     // one atomic per wave and bin
        const unsigned long long mk = __ballot(bin == b);
        if (mk && lane == (int)__builtin_ctzll(mk)) atomicAdd(&bin_cnt[b], (uint32_t)__popcll(mk));
    }
}
__global__ void k_bin_offsets(const uint32_t* __restrict__ bin_cnt, uint32_t* __restrict__ bin_off, uint32_t* __restrict__ item_off, uint32_t* __restrict__ cursor)
{
    if (threadIdx.x != 0) return;
    uint32_t a = 0, it = 0;
    for (int b = 0; b < PBINS; ++b) { bin_off[b] = a; item_off[b] = it; cursor[b] = 0; a += bin_cnt[b]; it += (bin_cnt[b] + 1) / 2; }
    bin_off[PBINS] = a; item_off[PBINS] = it;
}
__global__ __launch_bounds__(256)
void k_bin_scatter(const uint32_t* __restrict__ list, const uint32_t* __restrict__ count, const uint8_t* __restrict__ bin_of, const uint32_t* __restrict__ bin_off, uint32_t* __restrict__ cursor, uint32_t* __restrict__ sorted)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int bin = k < *count ? (int)bin_of[k] : -1;
    for (int b = 0; b < PBINS; ++b) {
        const unsigned long long mk = __ballot(bin == b);
        if (!mk) continue;
        const int leader = (int)__builtin_ctzll(mk);
        uint32_t base = 0; if (lane == leader) base = atomicAdd(&cursor[b], (uint32_t)__popcll(mk));
        base = __shfl(base, leader);
        if (bin == b) sorted[bin_off[b] + base + __popcll(mk & ((1ull << lane) - 1))] = list[k];
    }
}

// length class `cls` of a partitioned batch (class lists of ngsid_partition_pairs) through the paired kernel on stream st; tb = this launch's slice of the
// traceback scratch (plan16p).  SKEW: the instance with the skewed gap frame (the caller has checked ngsid_align16p_skew_exact)
template <int R, bool SKEW>
static int32_t launch16p(ngsid_ctx* ctx, const AlignJob& job, int cls, uint32_t max_tlen, hipStream_t st, uint64_t* tb)
{
    const uint64_t n = job.npairs;
    const size_t ints = 4 * PBINS + 8;                     // the class launches of a call run concurrently: one slice of the binning scratch each
    if (ctx->aln_pint.n < 4 * ints) HIPCHK(ctx, ctx->aln_pint.alloc(4 * ints));
    if (ctx->aln_psorted.n < 4 * n) HIPCHK(ctx, ctx->aln_psorted.reserve(4 * n));
    if (ctx->aln_pbin.n < 4 * n) HIPCHK(ctx, ctx->aln_pbin.reserve(4 * n));
    uint32_t* ibase = ctx->aln_pint.p + cls * ints; uint32_t* sorted = ctx->aln_psorted.p + (size_t)cls * n; uint8_t* bin_of = ctx->aln_pbin.p + (size_t)cls * n;
    const uint32_t* list = ctx->aln_cls.p + (size_t)cls * n; const uint32_t* count = ctx->aln_ctr.p + 8 + cls;
    uint32_t* bin_cnt = ibase, *bin_off = ibase + PBINS, *item_off = bin_off + PBINS + 1, *cursor = item_off + PBINS + 1, *wctr = cursor + PBINS;
    HIPCHK(ctx, hipMemsetAsync(ibase, 0, (size_t)(4 * PBINS + 8) * sizeof(uint32_t), st));
    const unsigned nb = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(k_pair_bins, dim3(nb), dim3(256), 0, st, job, list, count, R, bin_of, bin_cnt);
    hipLaunchKernelGGL(k_bin_offsets, dim3(1), dim3(64), 0, st, (const uint32_t*)bin_cnt, bin_off, item_off, cursor);
    hipLaunchKernelGGL(k_bin_scatter, dim3(nb), dim3(256), 0, st, list, count, (const uint8_t*)bin_of, (const uint32_t*)bin_off, cursor, sorted);
    HIPCHK(ctx, hipGetLastError());
    PairedPlan L; int32_t rc = plan16p<R, SKEW>(ctx, n, max_tlen, &L); if (rc) return rc;
    HIPCHK(ctx, hipFuncSetAttribute((const void*)k_sg_align16p<R, SKEW>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.lds));
    { ProfScope ps_(ctx, st == ctx->stream ? "k_sg_align" : "k_sg_align_side", st);
      hipLaunchKernelGGL((k_sg_align16p<R, SKEW>), dim3((unsigned)L.nwaves), dim3(64), L.lds, st, job, (const uint32_t*)sorted, (const uint32_t*)bin_off, (const uint32_t*)item_off, tb, L.words_half, L.seq_lds, wctr); }
    HIPCHK(ctx, hipGetLastError());
    return NGSID_OK;
}

// ---- routing

// Query-length classes of a partitioned batch: every pair runs in the instance with the fewest idle rows (a lane owns 2 RP rows of k_sg_align16; 750-base
// reads with a few 800-base ones would otherwise all run with RP = 7).  Per class: the largest query, the instance of k_sg_align16, that of the paired kernel
// k_sg_align16p (single strip, queries of up to 64 R bases; 0: none) and the side stream of its launch (-1: the context's stream, for the class of the ONT
// amplicon lengths).  The pairs above NGSID_ALIGN16_MAXLEN, if any, form list NCLS (the int32 kernel takes them).
#define NCLS 5
struct AlignClass { uint32_t bound; int rp, r, side; };
constexpr AlignClass kAlignClass[NCLS] = {{256, 2, 4, 0}, {512, 4, 8, 1}, {768, 6, 12, -1}, {896, 7, 14, 2}, {0xffffffffu, 8, 0, 3}};

// f(std::integral_constant<int, c>{}): class c as a compile-time constant, for the kernel instances of kAlignClass[c]
template <class F>
static int32_t with_class(int c, F&& f)
{
    switch (c) {
        case 0: return f(std::integral_constant<int, 0>{});
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        default: return f(std::integral_constant<int, 4>{});
    }
}

// pairs -> per-class index lists (order inside a class is irrelevant: results are written by pair index)
__global__ __launch_bounds__(256)
void k_pair_classes(AlignJob J, uint32_t* __restrict__ lists, uint32_t* __restrict__ counts, uint32_t long_len)
{
    // long_len > 0: pairs with a query or a target above it form class NCLS
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int cls = -1;
    if (p < J.npairs) {
        const uint32_t qi = J.qidx[p]; const uint32_t ql = (uint32_t)(J.qoff[qi + 1] - J.qoff[qi]); cls = 0; while (ql > kAlignClass[cls].bound) ++cls;
        if (long_len) { const uint32_t ti = J.tidx[p]; const uint32_t tl = (uint32_t)(J.toff[ti + 1] - J.toff[ti]); if (ql > long_len || tl > long_len) cls = NCLS; }
    }
#pragma unroll
    for (int c = 0; c < NCLS + 1; ++c) {                      // one atomic per wave and class
        const unsigned long long m = __ballot(cls == c);
        if (!m) continue;
        const int leader = __ffsll((long long)m) - 1;
        uint32_t base = 0; if (lane == leader) base = atomicAdd(&counts[c], (uint32_t)__popcll(m));
        base = __shfl(base, leader);
        if (cls == c) lists[(size_t)c * J.npairs + base + __popcll(m & ((1ull << lane) - 1))] = (uint32_t)p;
    }
}

// pairs -> NCLS + 1 index lists in ctx->aln_cls (class c at offset c * npairs), counts in ctx->aln_ctr[8 + c]; all 16 counters are zeroed first
int32_t ngsid_partition_pairs(ngsid_ctx* ctx, const AlignJob& job, uint32_t long_len)
{
    const uint64_t n = job.npairs;
    if (ctx->aln_ctr.n < 16) HIPCHK(ctx, ctx->aln_ctr.alloc(16));
    if (ctx->aln_cls.n < (size_t)(NCLS + 1) * n) HIPCHK(ctx, ctx->aln_cls.reserve((size_t)(NCLS + 1) * n));
    HIPCHK(ctx, hipMemsetAsync(ctx->aln_ctr.p, 0, 16 * sizeof(uint32_t), ctx->stream));
    hipLaunchKernelGGL(k_pair_classes, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, job, ctx->aln_cls.p, ctx->aln_ctr.p + 8, long_len);
    HIPCHK(ctx, hipGetLastError());
    return NGSID_OK;
}

// A partitioned batch: one launch per length class that has pairs, the classes of up to 896 bases through the paired kernel unless
// ngsid_ctx_option("align_paired", 0); the paired kernel in its skewed-frame instances where they are exact for this call (ngsid_align16p_skew_exact) unless
// ngsid_ctx_option("align_skew", 0).  long_len > 0: max_qlen / max_tlen are clamped to it, the longer pairs land in list NCLS for the caller.
static int32_t launch_classes(ngsid_ctx* ctx, const AlignJob& job, uint32_t max_qlen, uint32_t max_tlen, int max_open, uint32_t min_qlen, uint32_t long_len)
{
    const uint64_t n = job.npairs;
    { int32_t rc = ngsid_partition_pairs(ctx, job, long_len); if (rc) return rc; }
    // The class launches run CONCURRENTLY (the big class on the context's stream, the others on side streams): a class with a few hundred
    // pairs costs the latency of one pair, which would otherwise be paid once per class and call.  Every launch has its own scratch slice.
    { int32_t rc = ngsid_side_streams(ctx); if (rc) return rc; }
    const bool paired = ngsid_opt(ctx, "align_paired", 1) != 0;
    const bool skew = ngsid_opt(ctx, "align_skew", 1) != 0 && ngsid_align16p_skew_exact(job, max_qlen, max_tlen, max_open);
    bool used[NCLS]; uint64_t tbo[NCLS + 1] = {0}, bo[NCLS + 1] = {0};
    for (int c = 0; c < NCLS; ++c) {
        used[c] = (c == 0 || max_qlen > kAlignClass[c - 1].bound) && min_qlen <= std::min(max_qlen, kAlignClass[c].bound);
        uint64_t words = 0, bwords = 0;
        if (used[c]) {
            int32_t rc = with_class(c, [&](auto C) -> int32_t {
                constexpr AlignClass K = kAlignClass[decltype(C)::value];
                if constexpr (K.r > 0) {
                    if (paired) { PairedPlan P; int32_t r = skew ? plan16p<K.r, true>(ctx, n, max_tlen, &P) : plan16p<K.r, false>(ctx, n, max_tlen, &P); words = P.nwaves * 2 * P.words_half; return r; }
                }
                StripPlan L; int32_t r = plan16<K.rp>(ctx, n, std::min(max_qlen, K.bound), max_tlen, &L); words = L.nwaves * L.words; bwords = L.nwaves * 2ull * L.bnd_stride; return r;
            });
            if (rc) return rc;
        }
        tbo[c + 1] = tbo[c] + words; bo[c + 1] = bo[c] + bwords;
    }
    // scratch is grow-only and sized for all launches of a call BEFORE the first one (a reallocation frees memory that an earlier, still running launch uses)
    if (ctx->tb.n < tbo[NCLS]) HIPCHK(ctx, ctx->tb.reserve(tbo[NCLS]));
    if (ctx->bnd.n < bo[NCLS]) HIPCHK(ctx, ctx->bnd.reserve(bo[NCLS]));
    HIPCHK(ctx, hipEventRecord(ctx->ev_fork, ctx->stream));
    for (int i = 0; i < 4; ++i) HIPCHK(ctx, hipStreamWaitEvent(ctx->side[i], ctx->ev_fork, 0));
    for (int on_main = 0; on_main < 2; ++on_main)            // the side-stream classes first, the one on the context's stream last
        for (int c = 0; c < NCLS; ++c) {
            if (!used[c] || (kAlignClass[c].side < 0) != (on_main == 1)) continue;
            const hipStream_t st = kAlignClass[c].side < 0 ? ctx->stream : ctx->side[kAlignClass[c].side];
            int32_t rc = with_class(c, [&](auto C) -> int32_t {
                constexpr AlignClass K = kAlignClass[decltype(C)::value];
                if constexpr (K.r > 0) {
                    if (paired) return skew ? launch16p<K.r, true>(ctx, job, c, max_tlen, st, ctx->tb.p + tbo[c]) : launch16p<K.r, false>(ctx, job, c, max_tlen, st, ctx->tb.p + tbo[c]);
                }
                AlignJob jc = job; jc.pair_list = ctx->aln_cls.p + (size_t)c * n; jc.npairs_dev = ctx->aln_ctr.p + 8 + c;
                StripPlan L; int32_t r = plan16<K.rp>(ctx, n, std::min(max_qlen, K.bound), max_tlen, &L); if (r) return r;
                return launch16<K.rp>(ctx, jc, L, st, ctx->aln_ctr.p + 1 + c, ctx->tb.p + tbo[c], ctx->bnd.p + bo[c]);   // (counters zeroed by ngsid_partition_pairs)
            });
            if (rc) return rc;
        }
    for (int i = 0; i < 4; ++i) { HIPCHK(ctx, hipEventRecord(ctx->ev_join[i], ctx->side[i])); HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_join[i], 0)); }
    return NGSID_OK;
}

// the 16-bit path is exact when every score fits comfortably in int16 (see the range argument in DESIGN.md)
bool ngsid_align16_applicable(const AlignJob& job, uint32_t max_qlen, uint32_t max_tlen, int max_open)
{
    return max_qlen <= NGSID_ALIGN16_MAXLEN && max_tlen <= NGSID_ALIGN16_MAXLEN && job.match >= 0 && job.match <= 4 && job.mismatch <= 0 && job.mismatch >= -8 &&
           job.ext >= 0 && job.ext <= 4 && max_open >= 0 && max_open <= 16;
}

// The skewed-frame instances of the paired kernel (k_align16p.hip) are exact while no difference of two values of a DP cell leaves int16.  The frame adds up to
// (n + m) ext to a value, so the bound depends on the lengths of THIS call: the longest query that reaches the paired kernel (its classes end at 896 bases) and the
// longest target.  With ext <= 1 it holds for everything ngsid_align16_applicable accepts; a call it does not hold for runs the plain instances.
bool ngsid_align16p_skew_exact(const AlignJob& job, uint32_t max_qlen, uint32_t max_tlen, int max_open)
{
    uint32_t qmax = 0;
    for (int c = 0; c < NCLS; ++c) if (kAlignClass[c].r > 0) qmax = std::max(qmax, kAlignClass[c].bound);
    return ngsid_align16_applicable(job, max_qlen, max_tlen, max_open) &&
           sg16p_flag_span(job.match, job.ext, max_open, std::min(max_qlen, qmax), max_tlen, true) < 32768;
}

// measurement (profiling on): DP cells of the call = sum of n x m over its pairs, one atomic per workgroup
__global__ __launch_bounds__(256) void k_align_cells(AlignJob J, unsigned long long* __restrict__ stat)
{
    const uint64_t np = J.npairs_dev ? (uint64_t)*J.npairs_dev : J.npairs;
    unsigned long long c = 0;
    for (uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x; x < np; x += (uint64_t)gridDim.x * 256) {
        const uint64_t p = J.pair_list ? J.pair_list[x] : x; const uint32_t qi = J.qidx[p], ti = J.tidx[p];
        c += (unsigned long long)(J.qoff[qi + 1] - J.qoff[qi]) * (unsigned long long)(J.toff[ti + 1] - J.toff[ti]);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d);
    __shared__ unsigned long long part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(stat, part[0] + part[1] + part[2] + part[3]);
}

int32_t ngsid_launch_align(ngsid_ctx* ctx, const AlignJob& job, uint32_t max_qlen, uint32_t max_tlen, int max_open, uint32_t min_qlen)
{
    if (job.npairs == 0) return NGSID_OK;
    if (ctx->prof && ctx->stat.p && !job.bp) { hipLaunchKernelGGL(k_align_cells, dim3((unsigned)std::min<uint64_t>(1024, (job.npairs + 255) / 256)), dim3(256), 0, ctx->stream, job, ctx->stat.p + 1); HIPCHK(ctx, hipGetLastError()); }
    if (job.npairs > 0xf0000000ull) NGSID_FAIL(ctx, NGSID_ERR_ARG, "more than 2^32 pairs in one aligner call");
    if (max_tlen > NGSID_MAX_READ_LEN || max_qlen > NGSID_MAX_READ_LEN) NGSID_FAIL(ctx, NGSID_ERR_TOO_LONG, "sequence longer than %d in aligner", NGSID_MAX_READ_LEN);
    if (job.k > 64) NGSID_FAIL(ctx, NGSID_ERR_ARG, "window k > 64 unsupported");
    if (!job.ops && !ngsid_opt(ctx, "align32", 0)) {      // packed int16 kernels (bit-identical)
        // Round 5 (reads up to 65 535 bases): a large batch with a few long sequences keeps its short pairs in the int16 instances - the pairs with a query or a
        // target above NGSID_ALIGN16_MAXLEN become a class of their own that runs in int32, after the others (without this one 40 kb read among the
        // representatives would send a million 750-base pairs through the int32 kernel at one wave per CU)
        const uint32_t q16 = std::min<uint32_t>(max_qlen, NGSID_ALIGN16_MAXLEN), t16 = std::min<uint32_t>(max_tlen, NGSID_ALIGN16_MAXLEN);
        const bool has_long = max_qlen > q16 || max_tlen > t16;
        if (ngsid_align16_applicable(job, q16, t16, max_open)) {
            if (job.npairs >= 4096 && q16 > 256 && !job.pair_list && !ngsid_opt(ctx, "align_noclass", 0)) {
                int32_t rc = launch_classes(ctx, job, q16, t16, max_open, min_qlen, has_long ? NGSID_ALIGN16_MAXLEN : 0);
                if (rc || !has_long) return rc;
                AlignJob jl = job; jl.pair_list = ctx->aln_cls.p + (size_t)NCLS * job.npairs; jl.npairs_dev = ctx->aln_ctr.p + 8 + NCLS;
                return launch_rpl<16>(ctx, jl, max_qlen, max_tlen, true);
            }
            if (!has_long) {      // one launch on the context's stream, in the instance of the longest query's class
                int c = 0; while (max_qlen > kAlignClass[c].bound) ++c;
                return with_class(c, [&](auto C) -> int32_t {
                    constexpr int RP = kAlignClass[decltype(C)::value].rp;
                    StripPlan L; int32_t rc = plan16<RP>(ctx, job.npairs, max_qlen, max_tlen, &L); if (rc) return rc;
                    if (ctx->aln_ctr.n < 16) HIPCHK(ctx, ctx->aln_ctr.alloc(16));
                    HIPCHK(ctx, hipMemsetAsync(ctx->aln_ctr.p, 0, sizeof(uint32_t), ctx->stream));
                    if (ctx->tb.n < L.nwaves * L.words) HIPCHK(ctx, ctx->tb.alloc(L.nwaves * L.words));
                    if (ctx->bnd.n < L.nwaves * 2ull * L.bnd_stride) HIPCHK(ctx, ctx->bnd.alloc(L.nwaves * 2ull * L.bnd_stride));
                    return launch16<RP>(ctx, job, L, ctx->stream, ctx->aln_ctr.p, ctx->tb.p, ctx->bnd.p);
                });
            }
        }
    }
    if (max_qlen <= 256) return launch_rpl<4>(ctx, job, max_qlen, max_tlen);
    if (max_qlen <= 512) return launch_rpl<8>(ctx, job, max_qlen, max_tlen);
    if (max_qlen <= 768) return launch_rpl<12>(ctx, job, max_qlen, max_tlen);
    if (max_qlen <= 832) return launch_rpl<13>(ctx, job, max_qlen, max_tlen);     // tight fit: fewer idle lanes and rows per step
    if (max_qlen <= 896) return launch_rpl<14>(ctx, job, max_qlen, max_tlen);
    return launch_rpl<16>(ctx, job, max_qlen, max_tlen);
}
