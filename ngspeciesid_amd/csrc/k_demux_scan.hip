// k_demux_scan.hip - ngsid_demux_scan (include/ngsid_demux.h): every place in the WHOLE read where a pattern occurs within max_ed edits, one hit per run of qualifying
// last-row scores.
//
// The column, the match masks, the lane map and the LDS layout are those of k_demux_common.h; the text of a lane is a whole read, G = 64 / Tp.  What is this kernel's:
//   - the read is streamed: its letter codes pass through the LDS in staging chunks of DSC_CHUNK letters (4 x G x DSC_CHUNK bytes, private to a wave: a wave's LDS
//     instructions execute in order); Pv, Mv and the score are carried from chunk to chunk, and with more than 64 patterns the read is streamed once per pass;
//   - a wave runs to the longest of its reads: a lane whose read has ended sees only non-qualifying columns, so its open run closes at its own L and no later column reports;
//   - every lane keeps the state of its open run (run_best = DSC_NORUN when none is open, run_end) and appends one record when the run closes, or at L;
//   - there is no best-two reduction and no reversed pass.
// Records go through ONE append counter into a found buffer; the counter runs on when the buffer is full, so the host learns the count and repeats the reads in smaller
// chunks (ngsid_found_loop, ngsid_host.h).  The host brings the records into (read, end, pattern) order.
#include "k_demux_common.h"

#define DSC_CHUNK 128                   // letters of a read staged at a time (tests/test_gpu_demux_scan.py places read lengths around its multiples)
#define DSC_NORUN 0x7fffffff

static_assert(DSC_CHUNK % 4 == 0, "staging in 32-bit words");

struct DscRec { uint32_t read; int32_t pattern, end, ed; };      // read = index within the launch's chunk

__device__ __forceinline__ void dsc_wave_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_wave_barrier(); }

__device__ __forceinline__ void dsc_emit(DscRec* __restrict__ found, u64 limit, unsigned long long* __restrict__ ctr, uint32_t read, int pattern, int end, int ed)
{
    unsigned long long at;
    if (ngsid_found_slot(ctr, limit, &at)) { DscRec r; r.read = read; r.pattern = pattern; r.end = end; r.ed = ed; found[at] = r; }
}

__global__ __launch_bounds__(DMX_THREADS)
void k_demux_scan(const uint8_t* __restrict__ seq, const uint64_t* __restrict__ off, u64 r0, u64 nr /* reads of this launch */,
                  const u64* __restrict__ peq /* [npass][5][64] */, const int32_t* __restrict__ plen /* [npass * 64], 0 = no pattern */,
                  int logTp, int G, int npass, int max_ed, DscRec* __restrict__ found, u64 limit, unsigned long long* __restrict__ ctr)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t dsc_lds[];
    u64* s_peq = (u64*)dsc_lds;
    uint8_t* s_win = dsc_lds + DMX_PEQ_BYTES + (size_t)(threadIdx.x >> 6) * G * DSC_CHUNK;      // this wave's staging area
    const DmxLanes ln = dmx_lanes(logTp, G);
    const int lane = ln.lane, slot = ln.slot;
    const uint8_t* my_win = s_win + (size_t)(ln.in_group ? ln.g : 0) * DSC_CHUNK;
    const u64 nbatch = dmx_nbatch(nr, G);
    const int words = G * (DSC_CHUNK / 4);                       // 32-bit words of a staged chunk, all reads of the wave
    dmx_peq_preload(s_peq, peq, npass);
    for (u64 b = blockIdx.x; b < nbatch; b += gridDim.x) {
        const u64 base = (b * DMX_WAVES + ln.wave) * G;
        const u64 my_r = base + (u64)ln.g;
        const bool have_r = ln.in_group && my_r < nr;
        int L = 0;
        if (have_r) L = (int)(off[r0 + my_r + 1] - off[r0 + my_r]);
        const int Lmax = dmx_wave_max(L);
        for (int pass = 0; pass < npass; ++pass) {
            dmx_peq_reload(s_peq, peq, npass, pass);
            const int pattern = pass * 64 + slot;
            const int m = have_r ? plen[pattern] : 0;
            const int myL = m > 0 ? L : 0;                        // a lane without a pattern or a read has no qualifying column
            const int k = min(max_ed, m - 1);
            const int top = (m > 0 ? m : 1) - 1;
            DmxColumn col = {~0ull, 0, m};
            int run_best = DSC_NORUN, run_end = 0;
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
                        for (int q = 0; q < 4; ++q) wd |= (c0 + j + q < Lg ? ngsid_base_code(seq[a + (u64)(c0 + j + q)]) : 4u) << (8 * q);
                    }
                    *(uint32_t*)(s_win + (size_t)gi * DSC_CHUNK + j) = wd;
                }
                dsc_wave_sync();
                for (int j0 = 0; j0 < cn; j0 += 4) {
                    const uint32_t wd = *(const uint32_t*)(my_win + j0);
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const uint32_t c = (wd >> (8 * q)) & 0xffu;
                        col = dmx_step<false>(col, s_peq[c * 64 + slot], top);
                        const int j = c0 + j0 + q;
                        if (j < myL && col.score <= k) {
                            if (col.score < run_best) { run_best = col.score; run_end = j; }
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

extern "C" int32_t ngsid_demux_scan(ngsid_ctx* ctx, const ngsid_reads_t* reads, const ngsid_reads_t* patterns, const ngsid_demux_scan_params_t* prm,
                                    uint64_t* hit_off, int32_t* hit, uint64_t cap, uint64_t* needed)
{
    ApiClock api_clock_(ctx, "demux_scan");
    if (!ctx) return NGSID_ERR_ARG;
    if (!reads || !patterns || !prm || !needed || (cap && (!hit_off || !hit))) NGSID_FAIL(ctx, NGSID_ERR_ARG, "null argument");
    *needed = 0;
    if (prm->max_ed < 0) NGSID_FAIL(ctx, NGSID_ERR_ARG, "ngsid_demux_scan_params_t.max_ed must not be negative");
    DmxPatterns P;
    NGSID_TRY(dmx_patterns(ctx, patterns, 2 * NGSID_DEMUX_MAX_TAGS, prm->iupac, "pattern", "patterns", P));
    DevReads RD; int32_t rc = ngsid_upload_reads(ctx, reads, &RD, false); if (rc) return rc;
    const uint64_t N = RD.n;
    if (RD.maxlen > NGSID_MAX_READ_LEN) NGSID_FAIL(ctx, NGSID_ERR_TOO_LONG, "a read is longer than %d", NGSID_MAX_READ_LEN);
    if (N == 0) { if (hit_off) hit_off[0] = 0; return NGSID_OK; }
    NGSID_TRY(ngsid_alphabet_check(ctx, RD, nullptr, nullptr, "a read base outside upper-case ACGTN"));
    DevBuf<unsigned long long> d_ctr; DevBuf<DscRec> d_found;
    HIPCHK(ctx, d_ctr.alloc(1));
    // ---- lane mapping
    const int G = 64 >> P.logTp;
    const size_t lds = DMX_PEQ_BYTES + (size_t)DMX_WAVES * G * DSC_CHUNK;
    // ---- the found buffer: cap records, or what a share of the free device memory holds; reads in chunks, the same reads in smaller chunks when a launch finds more
    const uint64_t F = std::min<uint64_t>(cap, ngsid_mem_share(4, (size_t)64 << 20, (size_t)4 << 30, (size_t)4 << 30) / sizeof(DscRec));
    if (F) HIPCHK(ctx, d_found.alloc(F));
    const long long opt = ngsid_opt(ctx, "demux_scan_chunk_reads", 0);
    const uint64_t max_rows = (uint64_t)1 << 31;                  // the record's read index is 32 bits wide
    std::vector<DscRec> recs; std::vector<size_t> launch_at; std::vector<uint64_t> launch_r0;      // records of all launches; where a launch's records begin, and its first read
    const auto launch = [&](uint64_t c0, uint64_t& c1, uint64_t limit, bool&) -> int32_t {
        HIPCHK(ctx, hipMemsetAsync(d_ctr.p, 0, sizeof(unsigned long long), ctx->stream));
        ProfScope ps_(ctx, "k_demux_scan");
        hipLaunchKernelGGL(k_demux_scan, dim3((unsigned)std::min<uint64_t>(dmx_nbatch(c1 - c0, G), (uint64_t)ctx->n_cu * 8)), dim3(DMX_THREADS), lds, ctx->stream,
                           RD.seq, RD.off, (u64)c0, (u64)(c1 - c0), P.d_peq.p, P.d_len.p, P.logTp, G, P.npass, prm->max_ed, d_found.p, (u64)limit, d_ctr.p);
        return NGSID_OK;
    };
    const auto fetch = [&](uint64_t c0, size_t c) -> int32_t {
        const size_t at = recs.size();
        recs.resize(at + c); launch_at.push_back(at); launch_r0.push_back(c0);
        return dev_get(ctx, recs.data() + at, d_found.p, c);
    };
    uint64_t total = 0;
    NGSID_TRY(ngsid_found_loop(ctx, N, std::min<uint64_t>(opt > 0 ? (uint64_t)opt : N, max_rows), F, cap, d_ctr.p, launch, fetch, "read", "hits", &total));
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
