// k_demux.hip - ngsid_demux_locate (include/ngsid_demux.h): the infix location of every sample tag in both end windows of every read, and the best tag per (read, side).
//
// The search is ngsid_host_infix_locate (host_io.hip) for tags of at most 64 bases: ONE 64-bit Myers / Hyyro column per tag, free start in the window, the same
// 64-bit expressions as the host function, so every score of the last row is the host's.
//
// Lane mapping.  One tag per lane.  Tp = the tag count rounded up to a power of two (64 when T >= 64); a wave holds G = 64 / Tp read-sides (a read-side = one end
// window of one read; G is capped at 32 for windows above 128 bases to bound the LDS), lane = g * Tp + slot.  With T > 64 the tag list is walked in passes of 64
// (tag = pass * 64 + lane) and every lane keeps the two best keys of its own tags; the lanes of a read-side are reduced once, after the last pass.
// LDS per workgroup (4 waves): the match masks of the current pass, [5 window letters A C G T N][64 slots] x 8 B = 2 560 B - the window letter of a step is uniform
// within a read-side, so the 64-bit read is conflict-free for G = 1 -, and the windows of the wave's read-sides as letter codes (side 1 reverse-complemented while
// staging), 4 x G x W bytes (at most 32 KB).  Registers: Pv, Mv, Eq (3 x 2), score / best / end, two keys.
// The start of the WINNING tag only is computed, by the reversed pass of the host function (reversed tag = bit-reversed masks, reversed window prefix read backwards
// from `end`, anchored): all lanes of the read-side run it redundantly, which costs one more pass per read-side.
#include "ngsid_host.h"
#include "../../include/ngsid_demux.h"
#include <algorithm>

typedef unsigned long long u64;

#define DMX_WAVES 4
#define DMX_THREADS (DMX_WAVES * 64)
#define DMX_NOHIT 0x7fffffffu
// key of a hit: ed (6 bits) | tag (12 bits) | end (8 bits): ordered by (ed, tag)
#define DMX_KEY(ed, tag, end) (((uint32_t)(ed) << 20) | ((uint32_t)(tag) << 8) | (uint32_t)(end))

static_assert(NGSID_DEMUX_MAX_TAG_LEN == 64 && NGSID_DEMUX_MAX_WINDOW <= 256 && NGSID_DEMUX_MAX_TAGS <= 4096, "key layout and one-word columns");

// any base outside upper-case ACGTN in seq[0, len) sets *flag
__global__ __launch_bounds__(256)
void k_demux_alphabet(const uint8_t* __restrict__ seq, u64 len, uint32_t* __restrict__ flag)
{
    uint32_t bad = 0;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += (u64)gridDim.x * blockDim.x) {
        const uint8_t c = seq[i];
        bad |= !(c == 'A' || c == 'C' || c == 'G' || c == 'T' || c == 'N');
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1u);
}

__device__ __forceinline__ uint32_t dmx_code(uint8_t c, int complement)
{
    uint32_t k = c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u;
    return (complement && k < 4u) ? 3u - k : k;
}

__global__ __launch_bounds__(DMX_THREADS)
void k_demux_locate(const uint8_t* __restrict__ seq, const uint64_t* __restrict__ off, u64 r0, u64 nrs /* read-sides of this launch */,
                    const u64* __restrict__ peq /* [npass][5][64] */, const int32_t* __restrict__ tlen /* [npass * 64], 0 = no tag */,
                    int T, int logTp, int G, int npass, int W, int Wpad, int max_ed,
                    int32_t* __restrict__ hits /* [nrs][5] */, int16_t* __restrict__ ed_all, int16_t* __restrict__ end_all /* [nrs][T] or null */)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t dmx_lds[];
    u64* s_peq = (u64*)dmx_lds;
    uint8_t* s_win = dmx_lds + 5 * 64 * sizeof(u64) + (size_t)(threadIdx.x >> 6) * G * Wpad;      // this wave's windows
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int Tp = 1 << logTp, g = lane >> logTp, slot = lane & (Tp - 1);
    const bool in_group = g < G;
    const uint8_t* my_win = s_win + (size_t)(in_group ? g : 0) * Wpad;
    const u64 per_batch = (u64)DMX_WAVES * G, nbatch = (nrs + per_batch - 1) / per_batch;
    if (npass == 1) {
        for (int i = threadIdx.x; i < 5 * 64; i += DMX_THREADS) s_peq[i] = peq[i];
        __syncthreads();
    }
    for (u64 b = blockIdx.x; b < nbatch; b += gridDim.x) {
        const u64 base = (b * DMX_WAVES + wave) * G;
        // ---- the windows of this wave's read-sides, as letter codes
        for (int gi = 0; gi < G; ++gi) {
            const u64 rsid = base + gi;
            if (rsid >= nrs) break;
            const u64 a = off[r0 + (rsid >> 1)], L = off[r0 + (rsid >> 1) + 1] - a;
            const int side = (int)(rsid & 1), wl = (int)min((u64)W, L);
            for (int j = lane; j < Wpad; j += 64)
                s_win[(size_t)gi * Wpad + j] = (uint8_t)(j < wl ? dmx_code(side ? seq[a + L - 1 - j] : seq[a + j], side) : 4u);
        }
        const u64 my_rs = base + (u64)g;
        const bool have_rs = in_group && my_rs < nrs;
        int wl = 0;
        if (have_rs) { const u64 a = off[r0 + (my_rs >> 1)], L = off[r0 + (my_rs >> 1) + 1] - a; wl = (int)min((u64)W, L); }
        int wmax = wl;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) wmax = max(wmax, __shfl_xor(wmax, d));
        __syncthreads();
        uint32_t k1 = DMX_NOHIT, k2 = DMX_NOHIT;
        for (int pass = 0; pass < npass; ++pass) {
            if (npass > 1) {
                __syncthreads();
                for (int i = threadIdx.x; i < 5 * 64; i += DMX_THREADS) s_peq[i] = peq[(size_t)pass * 5 * 64 + i];
                __syncthreads();
            }
            const int tag = pass * 64 + slot;
            const int m = have_rs ? tlen[tag] : 0;
            const u64 top = 1ull << ((m > 0 ? m : 1) - 1);
            u64 Pv = ~0ull, Mv = 0;
            int score = m, best = m, e = -1;
            for (int j0 = 0; j0 < wmax; j0 += 4) {
                const uint32_t wd = *(const uint32_t*)(my_win + j0);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const uint32_t c = (wd >> (8 * q)) & 0xffu;
                    const u64 Eq = s_peq[c * 64 + slot];
                    const u64 Xv = Eq | Mv;
                    const u64 Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
                    u64 Ph = Mv | ~(Xh | Pv), Mh = Pv & Xh;
                    score += (Ph & top) ? 1 : 0; score -= (Mh & top) ? 1 : 0;
                    Ph <<= 1; Mh <<= 1;
                    Pv = Mh | ~(Xv | Ph); Mv = Ph & Xv;
                    if (j0 + q < wl && score < best) { best = score; e = j0 + q; }
                }
            }
            const bool hit = m > 0 && e >= 0 && best <= max_ed;
            if (m > 0) {
                if (ed_all) ed_all[my_rs * (u64)T + tag] = (int16_t)(hit ? best : -1);
                if (end_all) end_all[my_rs * (u64)T + tag] = (int16_t)(hit ? e : -1);
            }
            const uint32_t key = hit ? DMX_KEY(best, tag, e) : DMX_NOHIT;
            if (key < k1) { k2 = k1; k1 = key; } else if (key < k2) k2 = key;
        }
        // ---- the two best keys of the read-side (keys are distinct: the tag is part of them)
        for (int d = Tp >> 1; d >= 1; d >>= 1) {
            const uint32_t o1 = __shfl_xor(k1, d), o2 = __shfl_xor(k2, d);
            const uint32_t lo = min(k1, o1), hi = max(k1, o1);
            k2 = min(hi, min(k2, o2)); k1 = lo;
        }
        // ---- start of the winner: reversed tag against the reversed window prefix [0, end], anchored at `end`; the LAST column with the same distance
        const bool won = have_rs && k1 != DMX_NOHIT;
        const int bed = (int)(k1 >> 20), wtag = (int)((k1 >> 8) & 0xfffu), e = won ? (int)(k1 & 0xffu) : -1;
        int emax = e;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) emax = max(emax, __shfl_xor(emax, d));
        int start = -1;
        if (emax >= 0) {
            const int m = won ? tlen[wtag] : 1;
            u64 rq[5];
#pragma unroll
            for (int c = 0; c < 5; ++c) rq[c] = won ? __brevll(peq[((size_t)(wtag >> 6) * 5 + c) * 64 + (wtag & 63)]) >> (64 - m) : 0ull;
            const u64 top = 1ull << (m - 1);
            u64 Pv = ~0ull, Mv = 0;
            int score = m, jl = -1;
            for (int j = 0; j <= emax; ++j) {
                const uint32_t c = my_win[max(e - j, 0)];
                const u64 Eq = c == 0 ? rq[0] : c == 1 ? rq[1] : c == 2 ? rq[2] : c == 3 ? rq[3] : rq[4];
                const u64 Xv = Eq | Mv;
                const u64 Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
                u64 Ph = Mv | ~(Xh | Pv), Mh = Pv & Xh;
                score += (Ph & top) ? 1 : 0; score -= (Mh & top) ? 1 : 0;
                Ph = (Ph << 1) | 1ull; Mh <<= 1;
                Pv = Mh | ~(Xv | Ph); Mv = Ph & Xv;
                if (j <= e && score == bed) jl = j;
            }
            if (won) start = jl >= 0 ? e - jl : e + 1;
        }
        if (have_rs && slot == 0) {
            int32_t* h = hits + my_rs * NGSID_DEMUX_NFIELD;
            h[0] = won ? wtag : -1; h[1] = won ? bed : -1; h[2] = start; h[3] = e; h[4] = k2 != DMX_NOHIT ? (int32_t)(k2 >> 20) : -1;
        }
    }
}

int32_t ngsid_alphabet_scan(ngsid_ctx* ctx, const DevReads& R, uint32_t* d_flag, const char* prof_name)
{
    const uint64_t b0 = R.n ? R.h_off[0] : 0, nbases = R.n ? R.h_off[R.n] - b0 : 0;
    if (!nbases) return NGSID_OK;
    const auto launch = [&] { hipLaunchKernelGGL(k_demux_alphabet, dim3((unsigned)std::min<uint64_t>((nbases + 255) / 256, (uint64_t)ctx->n_cu * 16)), dim3(256), 0, ctx->stream, R.seq + b0, (u64)nbases, d_flag); };
    if (prof_name) { ProfScope ps_(ctx, prof_name); launch(); } else launch();
    HIPCHK(ctx, hipGetLastError());
    return NGSID_OK;
}

bool ngsid_iupac_eq(uint8_t a, uint8_t b, int iupac);      // host_io.hip: the equality rule of ngsid_host_infix_locate

extern "C" int32_t ngsid_demux_locate(ngsid_ctx* ctx, const ngsid_reads_t* reads, const ngsid_reads_t* tags, const ngsid_demux_params_t* prm,
                                      int32_t* hits, int16_t* ed_all, int16_t* end_all)
{
    ApiClock api_clock_(ctx, "demux_locate");
    if (!ctx) return NGSID_ERR_ARG;
    if (!reads || !tags || !prm) NGSID_FAIL(ctx, NGSID_ERR_ARG, "null argument");
    if (prm->window < 1 || prm->window > NGSID_DEMUX_MAX_WINDOW) NGSID_FAIL(ctx, NGSID_ERR_ARG, "ngsid_demux_params_t.window must be 1 .. %d", NGSID_DEMUX_MAX_WINDOW);
    if (prm->max_ed < 0) NGSID_FAIL(ctx, NGSID_ERR_ARG, "ngsid_demux_params_t.max_ed must not be negative");
    if (tags->mem != NGSID_MEM_HOST) NGSID_FAIL(ctx, NGSID_ERR_ARG, "the tags are a host read set");
    if (tags->n == 0 || tags->n > NGSID_DEMUX_MAX_TAGS) NGSID_FAIL(ctx, NGSID_ERR_ARG, "1 .. %d tags expected", NGSID_DEMUX_MAX_TAGS);
    if (!tags->off || !tags->seq) NGSID_FAIL(ctx, NGSID_ERR_ARG, "null tag set");
    const int T = (int)tags->n, npass = (T + 63) / 64;
    for (int t = 0; t < T; ++t) {
        if (tags->off[t + 1] <= tags->off[t]) NGSID_FAIL(ctx, NGSID_ERR_ARG, "tag %d is empty", t);
        if (tags->off[t + 1] - tags->off[t] > NGSID_DEMUX_MAX_TAG_LEN) NGSID_FAIL(ctx, NGSID_ERR_TOO_LONG, "tag %d is longer than %d", t, NGSID_DEMUX_MAX_TAG_LEN);
    }
    DevReads RD; int32_t rc = ngsid_upload_reads(ctx, reads, &RD, false); if (rc) return rc;
    const uint64_t N = RD.n;
    if (N == 0) return NGSID_OK;
    if (!hits) NGSID_FAIL(ctx, NGSID_ERR_ARG, "null hits");
    // ---- match masks per (tag, window letter), laid out as the kernel stages them
    std::vector<u64> h_peq((size_t)npass * 5 * 64, 0); std::vector<int32_t> h_tlen((size_t)npass * 64, 0);
    for (int t = 0; t < T; ++t) {
        const uint8_t* q = tags->seq + tags->off[t]; const int m = (int)(tags->off[t + 1] - tags->off[t]);
        h_tlen[t] = m;
        for (int c = 0; c < 5; ++c) { u64 v = 0; for (int i = 0; i < m; ++i) if (ngsid_iupac_eq(q[i], (uint8_t)"ACGTN"[c], prm->iupac)) v |= 1ull << i; h_peq[((size_t)(t >> 6) * 5 + c) * 64 + (t & 63)] = v; }
    }
    DevBuf<u64> d_peq; DevBuf<int32_t> d_tlen, d_hits; DevBuf<uint32_t> d_flag; DevBuf<int16_t> d_ed, d_end;
    NGSID_TRY(dev_put(ctx, d_peq, h_peq.data(), h_peq.size())); NGSID_TRY(dev_put(ctx, d_tlen, h_tlen.data(), h_tlen.size())); HIPCHK(ctx, d_hits.alloc(N * 2 * NGSID_DEMUX_NFIELD)); HIPCHK(ctx, d_flag.alloc(1));
    HIPCHK(ctx, hipMemsetAsync(d_flag.p, 0, sizeof(uint32_t), ctx->stream));
    NGSID_TRY(ngsid_alphabet_scan(ctx, RD, d_flag.p));
    // ---- lane mapping
    const int W = prm->window, Wpad = (W + 3) & ~3;
    int logTp = 0; while ((1 << logTp) < std::min(T, 64)) ++logTp;
    const int G = std::min(64 >> logTp, Wpad > 128 ? 32 : 64);
    const size_t lds = 5 * 64 * sizeof(u64) + (size_t)DMX_WAVES * G * Wpad;
    // ---- chunks of reads: with the [n][2][T] matrices under a share of the free device memory, else one launch
    const int nmat = (ed_all ? 1 : 0) + (end_all ? 1 : 0);
    uint64_t rows = N;
    const long long opt = ngsid_opt(ctx, "demux_chunk_reads", 0);
    if (opt > 0) rows = std::min<uint64_t>(N, (uint64_t)opt);
    else if (nmat) rows = std::min<uint64_t>(N, std::max<uint64_t>(1024, ngsid_mem_share(4, (size_t)64 << 20, (size_t)2 << 30, (size_t)4 << 30) / ((size_t)2 * T * sizeof(int16_t) * nmat)));
    if (ed_all) HIPCHK(ctx, d_ed.alloc(rows * 2 * T));
    if (end_all) HIPCHK(ctx, d_end.alloc(rows * 2 * T));
    for (uint64_t c0 = 0; c0 < N; c0 += rows) {
        const uint64_t c1 = std::min(N, c0 + rows), nrs = (c1 - c0) * 2;
        const uint64_t nbatch = (nrs + (uint64_t)DMX_WAVES * G - 1) / ((uint64_t)DMX_WAVES * G);
        { ProfScope ps_(ctx, "k_demux_locate");
          hipLaunchKernelGGL(k_demux_locate, dim3((unsigned)std::min<uint64_t>(nbatch, (uint64_t)ctx->n_cu * 8)), dim3(DMX_THREADS), lds, ctx->stream,
                             RD.seq, RD.off, (u64)c0, (u64)nrs, d_peq.p, d_tlen.p, T, logTp, G, npass, W, Wpad, prm->max_ed,
                             d_hits.p + c0 * 2 * NGSID_DEMUX_NFIELD, ed_all ? d_ed.p : nullptr, end_all ? d_end.p : nullptr); }
        HIPCHK(ctx, hipGetLastError());
        if (ed_all) NGSID_TRY(dev_get(ctx, ed_all + c0 * 2 * T, d_ed.p, nrs * T));
        if (end_all) NGSID_TRY(dev_get(ctx, end_all + c0 * 2 * T, d_end.p, nrs * T));
        if (nmat) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));          // the next chunk writes the same two buffers
    }
    uint32_t bad = 0;
    NGSID_TRY(dev_get(ctx, hits, d_hits.p, N * 2 * NGSID_DEMUX_NFIELD)); NGSID_TRY(dev_get(ctx, &bad, d_flag.p, 1));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (bad) NGSID_FAIL(ctx, NGSID_ERR_ALPHABET, "a read base outside upper-case ACGTN");
    return NGSID_OK;
}
