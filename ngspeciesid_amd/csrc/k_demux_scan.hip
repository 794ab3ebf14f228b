// k_demux_scan.hip - ngsid_demux_scan (include/ngsid_demux.h): every place in the WHOLE read where a pattern occurs within max_ed edits, one hit per run of qualifying
// last-row scores.
//
// The column is that of k_demux_locate (k_demux.hip): ONE 64-bit Myers / Hyyro word per pattern and lane, free start, the 64-bit expressions of ngsid_host_infix_locate, so
// every s[j] is the host's.  What differs:
//   - the read is streamed: its letter codes pass through the LDS in staging chunks of DSC_CHUNK letters; Pv, Mv and the score are carried from chunk to chunk;
//   - every lane keeps the state of its open run (run_best = DSC_NORUN when none is open, run_end) and appends one record when the run closes, or at L;
//   - there is no best-two reduction and no reversed pass.
// Lane mapping.  One pattern per lane.  Tp = the pattern count rounded up to a power of two (64 when P >= 64); a wave holds G = 64 / Tp reads, lane = g * Tp + slot, and runs
// to the longest of them: a lane whose read has ended sees only non-qualifying columns, so its open run closes at its own L and no later column reports.  With P > 64 the
// pattern list is walked in passes of 64 and the read is streamed once per pass.
// LDS per workgroup (4 waves): the match masks of the current pass, [5 letters A C G T N][64 slots] x 8 B = 2 560 B, and 4 x G x DSC_CHUNK bytes of letter codes (at most 32 KB).
// The staging area is private to a wave (a wave's LDS instructions execute in order), the masks are shared by the workgroup.
// Records go through ONE append counter into a found buffer; the counter runs on when the buffer is full, so the host learns the count and repeats the reads in smaller
// chunks (the rule of k_near_tiles).  The host brings the records into (read, end, pattern) order.
#include "ngsid_host.h"
#include "../../include/ngsid_demux.h"
#include <algorithm>

typedef unsigned long long u64;

#define DSC_WAVES 4
#define DSC_THREADS (DSC_WAVES * 64)
#define DSC_CHUNK 128                   // letters of a read staged at a time (tests/test_gpu_demux_scan.py places read lengths around its multiples)
#define DSC_NORUN 0x7fffffff

static_assert(NGSID_DEMUX_MAX_TAG_LEN == 64 && DSC_CHUNK % 4 == 0, "one-word columns, staging in 32-bit words");

struct DscRec { uint32_t read; int32_t pattern, end, ed; };      // read = index within the launch's chunk

__device__ __forceinline__ uint32_t dsc_code(uint8_t c) { return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u; }
__device__ __forceinline__ void dsc_wave_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_wave_barrier(); }

__device__ __forceinline__ void dsc_emit(DscRec* __restrict__ found, u64 limit, unsigned long long* __restrict__ ctr, uint32_t read, int pattern, int end, int ed)
{
    const u64 at = atomicAdd(ctr, 1ull);
    if (at < limit) { DscRec r; r.read = read; r.pattern = pattern; r.end = end; r.ed = ed; found[at] = r; }
}

__global__ __launch_bounds__(DSC_THREADS)
void k_demux_scan(const uint8_t* __restrict__ seq, const uint64_t* __restrict__ off, u64 r0, u64 nr /* reads of this launch */,
                  const u64* __restrict__ peq /* [npass][5][64] */, const int32_t* __restrict__ plen /* [npass * 64], 0 = no pattern */,
                  int logTp, int G, int npass, int max_ed, DscRec* __restrict__ found, u64 limit, unsigned long long* __restrict__ ctr)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t dsc_lds[];
    u64* s_peq = (u64*)dsc_lds;
    uint8_t* s_win = dsc_lds + 5 * 64 * sizeof(u64) + (size_t)(threadIdx.x >> 6) * G * DSC_CHUNK;      // this wave's staging area
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int Tp = 1 << logTp, g = lane >> logTp, slot = lane & (Tp - 1);
    const bool in_group = g < G;
    const uint8_t* my_win = s_win + (size_t)(in_group ? g : 0) * DSC_CHUNK;
    const u64 per_batch = (u64)DSC_WAVES * G, nbatch = (nr + per_batch - 1) / per_batch;
    const int words = G * (DSC_CHUNK / 4);                       // 32-bit words of a staged chunk, all reads of the wave
    if (npass == 1) {
        for (int i = threadIdx.x; i < 5 * 64; i += DSC_THREADS) s_peq[i] = peq[i];
        __syncthreads();
    }
    for (u64 b = blockIdx.x; b < nbatch; b += gridDim.x) {
        const u64 base = (b * DSC_WAVES + wave) * G;
        const u64 my_r = base + (u64)g;
        const bool have_r = in_group && my_r < nr;
        int L = 0;
        if (have_r) L = (int)(off[r0 + my_r + 1] - off[r0 + my_r]);
        int Lmax = L;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) Lmax = max(Lmax, __shfl_xor(Lmax, d));
        for (int pass = 0; pass < npass; ++pass) {
            if (npass > 1) {
                __syncthreads();
                for (int i = threadIdx.x; i < 5 * 64; i += DSC_THREADS) s_peq[i] = peq[(size_t)pass * 5 * 64 + i];
                __syncthreads();
            }
            const int pattern = pass * 64 + slot;
            const int m = have_r ? plen[pattern] : 0;
            const int myL = m > 0 ? L : 0;                        // a lane without a pattern or a read has no qualifying column
            const int k = min(max_ed, m - 1);
            const u64 top = 1ull << ((m > 0 ? m : 1) - 1);
            u64 Pv = ~0ull, Mv = 0;
            int score = m, run_best = DSC_NORUN, run_end = 0;
            for (int c0 = 0; c0 < Lmax; c0 += DSC_CHUNK) {
                const int cn = min(DSC_CHUNK, (Lmax - c0 + 3) & ~3);      // columns of this chunk, a multiple of 4
                // ---- stage letters [c0, c0 + cn) of the wave's reads, four per lane and step (past a read's end: N)
                dsc_wave_sync();                                  // the previous chunk has been read
                for (int w = lane; w < words; w += 64) {
                    const int gi = w / (DSC_CHUNK / 4), j = (w % (DSC_CHUNK / 4)) * 4;
                    const u64 rid = base + (u64)gi;
                    if (j >= cn) continue;
                    uint32_t wd = 0x04040404u;                    // a group without a read still indexes the masks with what it finds here
                    if (rid < nr) {
                        const u64 a = off[r0 + rid]; const int Lg = (int)(off[r0 + rid + 1] - a);
                        wd = 0;
#pragma unroll
                        for (int q = 0; q < 4; ++q) wd |= (c0 + j + q < Lg ? dsc_code(seq[a + (u64)(c0 + j + q)]) : 4u) << (8 * q);
                    }
                    *(uint32_t*)(s_win + (size_t)gi * DSC_CHUNK + j) = wd;
                }
                dsc_wave_sync();
                for (int j0 = 0; j0 < cn; j0 += 4) {
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
                        const int j = c0 + j0 + q;
                        if (j < myL && score <= k) {
                            if (score < run_best) { run_best = score; run_end = j; }
                        } else if (run_best != DSC_NORUN) {
                            dsc_emit(found, limit, ctr, (uint32_t)my_r, pattern, run_end, run_best);
                            run_best = DSC_NORUN;
                        }
                    }
                }
            }
            if (run_best != DSC_NORUN) dsc_emit(found, limit, ctr, (uint32_t)my_r, pattern, run_end, run_best);      // a run open at the last base of the longest read
        }
    }
}

bool ngsid_iupac_eq(uint8_t a, uint8_t b, int iupac);      // host_io.hip: the equality rule of ngsid_host_infix_locate

extern "C" int32_t ngsid_demux_scan(ngsid_ctx* ctx, const ngsid_reads_t* reads, const ngsid_reads_t* patterns, const ngsid_demux_scan_params_t* prm,
                                    uint64_t* hit_off, int32_t* hit, uint64_t cap, uint64_t* needed)
{
    ApiClock api_clock_(ctx, "demux_scan");
    if (!ctx) return NGSID_ERR_ARG;
    if (!reads || !patterns || !prm || !needed || (cap && (!hit_off || !hit))) NGSID_FAIL(ctx, NGSID_ERR_ARG, "null argument");
    *needed = 0;
    if (prm->max_ed < 0) NGSID_FAIL(ctx, NGSID_ERR_ARG, "ngsid_demux_scan_params_t.max_ed must not be negative");
    if (patterns->mem != NGSID_MEM_HOST) NGSID_FAIL(ctx, NGSID_ERR_ARG, "the patterns are a host read set");
    if (patterns->n == 0 || patterns->n > 2 * NGSID_DEMUX_MAX_TAGS) NGSID_FAIL(ctx, NGSID_ERR_ARG, "1 .. %d patterns expected", 2 * NGSID_DEMUX_MAX_TAGS);
    if (!patterns->off || !patterns->seq) NGSID_FAIL(ctx, NGSID_ERR_ARG, "null pattern set");
    const int P = (int)patterns->n, npass = (P + 63) / 64;
    for (int t = 0; t < P; ++t) {
        if (patterns->off[t + 1] <= patterns->off[t]) NGSID_FAIL(ctx, NGSID_ERR_ARG, "pattern %d is empty", t);
        if (patterns->off[t + 1] - patterns->off[t] > NGSID_DEMUX_MAX_TAG_LEN) NGSID_FAIL(ctx, NGSID_ERR_TOO_LONG, "pattern %d is longer than %d", t, NGSID_DEMUX_MAX_TAG_LEN);
    }
    DevReads RD; int32_t rc = ngsid_upload_reads(ctx, reads, &RD, false); if (rc) return rc;
    const uint64_t N = RD.n;
    if (RD.maxlen > NGSID_MAX_READ_LEN) NGSID_FAIL(ctx, NGSID_ERR_TOO_LONG, "a read is longer than %d", NGSID_MAX_READ_LEN);
    if (N == 0) { if (hit_off) hit_off[0] = 0; return NGSID_OK; }
    // ---- match masks per (pattern, read letter), laid out as the kernel stages them
    std::vector<u64> h_peq((size_t)npass * 5 * 64, 0); std::vector<int32_t> h_plen((size_t)npass * 64, 0);
    for (int t = 0; t < P; ++t) {
        const uint8_t* q = patterns->seq + patterns->off[t]; const int m = (int)(patterns->off[t + 1] - patterns->off[t]);
        h_plen[t] = m;
        for (int c = 0; c < 5; ++c) { u64 v = 0; for (int i = 0; i < m; ++i) if (ngsid_iupac_eq(q[i], (uint8_t)"ACGTN"[c], prm->iupac)) v |= 1ull << i; h_peq[((size_t)(t >> 6) * 5 + c) * 64 + (t & 63)] = v; }
    }
    DevBuf<u64> d_peq; DevBuf<int32_t> d_plen; DevBuf<uint32_t> d_flag; DevBuf<unsigned long long> d_ctr; DevBuf<DscRec> d_found;
    NGSID_TRY(dev_put(ctx, d_peq, h_peq.data(), h_peq.size())); NGSID_TRY(dev_put(ctx, d_plen, h_plen.data(), h_plen.size())); HIPCHK(ctx, d_flag.alloc(1)); HIPCHK(ctx, d_ctr.alloc(1));
    HIPCHK(ctx, hipMemsetAsync(d_flag.p, 0, sizeof(uint32_t), ctx->stream));
    NGSID_TRY(ngsid_alphabet_scan(ctx, RD, d_flag.p));
    uint32_t bad = 0;
    NGSID_TRY(dev_get(ctx, &bad, d_flag.p, 1));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (bad) NGSID_FAIL(ctx, NGSID_ERR_ALPHABET, "a read base outside upper-case ACGTN");
    // ---- lane mapping
    int logTp = 0; while ((1 << logTp) < std::min(P, 64)) ++logTp;
    const int G = 64 >> logTp;
    const size_t lds = 5 * 64 * sizeof(u64) + (size_t)DSC_WAVES * G * DSC_CHUNK;
    // ---- the found buffer: cap records, or what a share of the free device memory holds; reads in chunks, the same reads in smaller chunks when a launch finds more
    const uint64_t F = std::min<uint64_t>(cap, ngsid_mem_share(4, (size_t)64 << 20, (size_t)4 << 30, (size_t)4 << 30) / sizeof(DscRec));
    if (F) HIPCHK(ctx, d_found.alloc(F));
    const long long opt = ngsid_opt(ctx, "demux_scan_chunk_reads", 0);
    const uint64_t max_rows = (uint64_t)1 << 31;                  // the record's read index is 32 bits wide
    bool fill = cap > 0;
    std::vector<DscRec> recs; std::vector<size_t> launch_at; std::vector<uint64_t> launch_r0;      // records of all launches; where a launch's records begin, and its first read
    uint64_t total = 0, rows_now = std::min<uint64_t>(opt > 0 ? (uint64_t)opt : N, max_rows);
    for (uint64_t c0 = 0; c0 < N; ) {
        const uint64_t c1 = std::min(N, c0 + rows_now), nr = c1 - c0;
        const uint64_t nbatch = (nr + (uint64_t)DSC_WAVES * G - 1) / ((uint64_t)DSC_WAVES * G);
        const uint64_t limit = fill ? std::min(F, cap - total) : 0;
        HIPCHK(ctx, hipMemsetAsync(d_ctr.p, 0, sizeof(unsigned long long), ctx->stream));
        { ProfScope ps_(ctx, "k_demux_scan");
          hipLaunchKernelGGL(k_demux_scan, dim3((unsigned)std::min<uint64_t>(nbatch, (uint64_t)ctx->n_cu * 8)), dim3(DSC_THREADS), lds, ctx->stream,
                             RD.seq, RD.off, (u64)c0, (u64)nr, d_peq.p, d_plen.p, logTp, G, npass, prm->max_ed, d_found.p, (u64)limit, d_ctr.p); }
        HIPCHK(ctx, hipGetLastError());
        unsigned long long c = 0;
        NGSID_TRY(dev_get(ctx, &c, d_ctr.p, 1));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        if (fill && c > limit) {
            if (limit == cap - total) fill = false;               // more hits than the caller has room for: count on
            else if (nr > 1) { rows_now = nr / 2; continue; }     // more than the found buffer holds: the same reads in smaller chunks
            else NGSID_FAIL(ctx, NGSID_ERR_HIP, "one read has %llu hits: beyond the found buffer the free device memory allows", c);
        }
        if (fill && c) {
            const size_t at = recs.size();
            recs.resize(at + c); launch_at.push_back(at); launch_r0.push_back(c0);
            NGSID_TRY(dev_get(ctx, recs.data() + at, d_found.p, (size_t)c));
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        }
        total += c;
        c0 = c1;
    }
    *needed = total;
    if (total > cap) NGSID_FAIL(ctx, NGSID_ERR_CAPACITY, "%llu hits, room for %llu", (unsigned long long)total, (unsigned long long)cap);
    if (!hit_off) return NGSID_OK;                                // the count call of a read set without a hit
    // ---- ascending (read, end, pattern): a counting sort by read, then the few hits of each read by (end, pattern); the triples are distinct
    for (uint64_t r = 0; r <= N; ++r) hit_off[r] = 0;
    for (size_t l = 0; l < launch_at.size(); ++l)
        for (size_t x = launch_at[l]; x < (l + 1 < launch_at.size() ? launch_at[l + 1] : recs.size()); ++x) hit_off[launch_r0[l] + recs[x].read + 1] += 1;
    for (uint64_t r = 0; r < N; ++r) hit_off[r + 1] += hit_off[r];
    std::vector<uint64_t> fill_at(hit_off, hit_off + N);
    std::vector<DscRec> sorted(total);
    for (size_t l = 0; l < launch_at.size(); ++l)
        for (size_t x = launch_at[l]; x < (l + 1 < launch_at.size() ? launch_at[l + 1] : recs.size()); ++x) sorted[fill_at[launch_r0[l] + recs[x].read]++] = recs[x];
    for (uint64_t r = 0; r < N; ++r)
        std::sort(sorted.begin() + hit_off[r], sorted.begin() + hit_off[r + 1], [](const DscRec& x, const DscRec& y) { return x.end != y.end ? x.end < y.end : x.pattern < y.pattern; });
    for (uint64_t h = 0; h < total; ++h) {
        hit[h * NGSID_DEMUX_SCAN_NFIELD + 0] = sorted[h].pattern; hit[h * NGSID_DEMUX_SCAN_NFIELD + 1] = sorted[h].end; hit[h * NGSID_DEMUX_SCAN_NFIELD + 2] = sorted[h].ed;
    }
    return NGSID_OK;
}
