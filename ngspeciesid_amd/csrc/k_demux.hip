// k_demux.hip - ngsid_demux_locate (include/ngsid_demux.h): the infix location of every sample tag in both end windows of every read, and the best tag per (read, side).
//
// The column, the match masks, the lane map and the LDS layout are those of k_demux_common.h; the text of a lane is a read-side = one end window of one read.  What is this kernel's:
//   - the windows of the wave's read-sides are staged whole, as letter codes (side 1 reverse-complemented while staging), 4 x G x W bytes; G is capped at 32 for windows above
//     128 bases to bound them at 32 KB;
//   - every lane keeps the two best keys of its own tags over the passes; the lanes of a read-side are reduced once, after the last pass;
//   - the start of the WINNING tag only is computed, by the reversed pass of the host function (reversed tag = bit-reversed masks, reversed window prefix read backwards
//     from `end`, anchored): all lanes of the read-side run it redundantly, which costs one more pass per read-side.
// Registers: Pv, Mv, Eq (3 x 2), score / best / end, two keys.
#include "k_demux_common.h"

#define DMX_NOHIT 0x7fffffffu
// key of a hit: ed (6 bits) | tag (12 bits) | end (8 bits): ordered by (ed, tag)
#define DMX_KEY(ed, tag, end) (((uint32_t)(ed) << 20) | ((uint32_t)(tag) << 8) | (uint32_t)(end))

static_assert(NGSID_DEMUX_MAX_WINDOW <= 256 && NGSID_DEMUX_MAX_TAGS <= 4096, "key layout");

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

__global__ __launch_bounds__(DMX_THREADS)
void k_demux_locate(const uint8_t* __restrict__ seq, const uint64_t* __restrict__ off, u64 r0, u64 nrs /* read-sides of this launch */,
                    const u64* __restrict__ peq /* [npass][5][64] */, const int32_t* __restrict__ tlen /* [npass * 64], 0 = no tag */,
                    int T, int logTp, int G, int npass, int W, int Wpad, int max_ed,
                    int32_t* __restrict__ hits /* [nrs][5] */, int16_t* __restrict__ ed_all, int16_t* __restrict__ end_all /* [nrs][T] or null */)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t dmx_lds[];
    u64* s_peq = (u64*)dmx_lds;
    uint8_t* s_win = dmx_lds + DMX_PEQ_BYTES + (size_t)(threadIdx.x >> 6) * G * Wpad;      // this wave's windows
    const DmxLanes ln = dmx_lanes(logTp, G);
    const int lane = ln.lane, slot = ln.slot;
    const uint8_t* my_win = s_win + (size_t)(ln.in_group ? ln.g : 0) * Wpad;
    const u64 nbatch = dmx_nbatch(nrs, G);
    dmx_peq_preload(s_peq, peq, npass);
    for (u64 b = blockIdx.x; b < nbatch; b += gridDim.x) {
        const u64 base = (b * DMX_WAVES + ln.wave) * G;
        // ---- the windows of this wave's read-sides, as letter codes
        for (int gi = 0; gi < G; ++gi) {
            const u64 rsid = base + gi;
            if (rsid >= nrs) break;
            const u64 a = off[r0 + (rsid >> 1)], L = off[r0 + (rsid >> 1) + 1] - a;
            const int side = (int)(rsid & 1), wl = (int)min((u64)W, L);
            for (int j = lane; j < Wpad; j += 64)
                s_win[(size_t)gi * Wpad + j] = (uint8_t)(j < wl ? dmx_code(side ? seq[a + L - 1 - j] : seq[a + j], side) : 4u);
        }
        const u64 my_rs = base + (u64)ln.g;
        const bool have_rs = ln.in_group && my_rs < nrs;
        int wl = 0;
        if (have_rs) { const u64 a = off[r0 + (my_rs >> 1)], L = off[r0 + (my_rs >> 1) + 1] - a; wl = (int)min((u64)W, L); }
        const int wmax = dmx_wave_max(wl);
        __syncthreads();
        uint32_t k1 = DMX_NOHIT, k2 = DMX_NOHIT;
        for (int pass = 0; pass < npass; ++pass) {
            dmx_peq_reload(s_peq, peq, npass, pass);
            const int tag = pass * 64 + slot;
            const int m = have_rs ? tlen[tag] : 0;
            const int top = (m > 0 ? m : 1) - 1;
            DmxColumn col = {~0ull, 0, m};
            int best = m, e = -1;
            for (int j0 = 0; j0 < wmax; j0 += 4) {
                const uint32_t wd = *(const uint32_t*)(my_win + j0);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const uint32_t c = (wd >> (8 * q)) & 0xffu;
                    col = dmx_step<false>(col, s_peq[c * 64 + slot], top);
                    if (j0 + q < wl && col.score < best) { best = col.score; e = j0 + q; }
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
        for (int d = ln.Tp >> 1; d >= 1; d >>= 1) {
            const uint32_t o1 = __shfl_xor(k1, d), o2 = __shfl_xor(k2, d);
            const uint32_t lo = min(k1, o1), hi = max(k1, o1);
            k2 = min(hi, min(k2, o2)); k1 = lo;
        }
        // ---- start of the winner: reversed tag against the reversed window prefix [0, end], anchored at `end`; the LAST column with the same distance
        const bool won = have_rs && k1 != DMX_NOHIT;
        const int bed = (int)(k1 >> 20), wtag = (int)((k1 >> 8) & 0xfffu), e = won ? (int)(k1 & 0xffu) : -1;
        const int emax = dmx_wave_max(e);
        int start = -1;
        if (emax >= 0) {
            const int m = won ? tlen[wtag] : 1;
            u64 rq[5];
#pragma unroll
            for (int c = 0; c < 5; ++c) rq[c] = won ? __brevll(peq[((size_t)(wtag >> 6) * 5 + c) * 64 + (wtag & 63)]) >> (64 - m) : 0ull;
            const int top = m - 1;
            DmxColumn col = {~0ull, 0, m};
            int jl = -1;
            for (int j = 0; j <= emax; ++j) {
                const uint32_t c = my_win[max(e - j, 0)];
                col = dmx_step<true>(col, c == 0 ? rq[0] : c == 1 ? rq[1] : c == 2 ? rq[2] : c == 3 ? rq[3] : rq[4], top);
                if (j <= e && col.score == bed) jl = j;
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

extern "C" int32_t ngsid_demux_locate(ngsid_ctx* ctx, const ngsid_reads_t* reads, const ngsid_reads_t* tags, const ngsid_demux_params_t* prm,
                                      int32_t* hits, int16_t* ed_all, int16_t* end_all)
{
    ApiClock api_clock_(ctx, "demux_locate");
    if (!ctx) return NGSID_ERR_ARG;
    if (!reads || !tags || !prm) NGSID_FAIL(ctx, NGSID_ERR_ARG, "null argument");
    if (prm->window < 1 || prm->window > NGSID_DEMUX_MAX_WINDOW) NGSID_FAIL(ctx, NGSID_ERR_ARG, "ngsid_demux_params_t.window must be 1 .. %d", NGSID_DEMUX_MAX_WINDOW);
    if (prm->max_ed < 0) NGSID_FAIL(ctx, NGSID_ERR_ARG, "ngsid_demux_params_t.max_ed must not be negative");
    DmxPatterns P;
    NGSID_TRY(dmx_patterns(ctx, tags, NGSID_DEMUX_MAX_TAGS, prm->iupac, "tag", "tags", P));
    const int T = P.n;
    DevReads RD; int32_t rc = ngsid_upload_reads(ctx, reads, &RD, false); if (rc) return rc;
    const uint64_t N = RD.n;
    if (N == 0) return NGSID_OK;
    if (!hits) NGSID_FAIL(ctx, NGSID_ERR_ARG, "null hits");
    DevBuf<int32_t> d_hits; DevBuf<uint32_t> d_flag; DevBuf<int16_t> d_ed, d_end;
    HIPCHK(ctx, d_hits.alloc(N * 2 * NGSID_DEMUX_NFIELD)); HIPCHK(ctx, d_flag.alloc(1));
    HIPCHK(ctx, hipMemsetAsync(d_flag.p, 0, sizeof(uint32_t), ctx->stream));
    NGSID_TRY(ngsid_alphabet_scan(ctx, RD, d_flag.p));
    // ---- lane mapping
    const int W = prm->window, Wpad = (W + 3) & ~3;
    const int G = std::min(64 >> P.logTp, Wpad > 128 ? 32 : 64);
    const size_t lds = DMX_PEQ_BYTES + (size_t)DMX_WAVES * G * Wpad;
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
        { ProfScope ps_(ctx, "k_demux_locate");
          hipLaunchKernelGGL(k_demux_locate, dim3((unsigned)std::min<uint64_t>(dmx_nbatch(nrs, G), (uint64_t)ctx->n_cu * 8)), dim3(DMX_THREADS), lds, ctx->stream,
                             RD.seq, RD.off, (u64)c0, (u64)nrs, P.d_peq.p, P.d_len.p, T, P.logTp, G, P.npass, W, Wpad, prm->max_ed,
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
