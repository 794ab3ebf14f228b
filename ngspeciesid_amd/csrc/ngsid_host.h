// ngsid_host.h - host-side plumbing the entry points share: transfers, the launch bound, the memory budget, list checks, the grouped-reads front end, pair batches, sketch scratch,
// the alphabet check, the IUPAC equality and the letter code (k_demux_common.h, k_near.hip), the found-list emit, pair key and loop (k_demux_scan.hip, k_near.hip, k_umi.hip)
#pragma once
#include "ngsid_internal.h"
#include <algorithm>

#define NGSID_TRY(call) do { const int32_t rc_ = (call); if (rc_) return rc_; } while (0)

// ---- transfers on ctx->stream (asynchronous: the caller synchronises before the host side is read or reused)
template <typename T> static inline int32_t dev_put(ngsid_ctx* ctx, DevBuf<T>& d, const T* h, size_t n)      // allocates n entries and fills them from the host
{
    HIPCHK(ctx, d.alloc(n));
    if (n) HIPCHK(ctx, hipMemcpyAsync(d.p, h, sizeof(T) * n, hipMemcpyHostToDevice, ctx->stream));
    return NGSID_OK;
}
template <typename T> static inline int32_t dev_get(ngsid_ctx* ctx, T* h, const T* d, size_t n)
{
    if (n) HIPCHK(ctx, hipMemcpyAsync(h, d, sizeof(T) * n, hipMemcpyDeviceToHost, ctx->stream));
    return NGSID_OK;
}

// ---- the launch bound: HIP takes no grid with gridDim.x * blockDim.x >= 2^32 (hipModuleLaunchKernel, hip_runtime_api.h) - a larger one is not refused but runs in part.
// A launch whose workgroup count grows with the input either chunks by ngsid_max_blocks or passes the count through NGSID_GRID; grids clamped to a multiple of n_cu need neither.
#define NGSID_MAX_GRID_ITEMS 0x100000000ull
static inline uint64_t ngsid_max_blocks(unsigned threads) { return (NGSID_MAX_GRID_ITEMS - 1) / threads; }
static inline int32_t ngsid_grid(ngsid_ctx* ctx, uint64_t blocks, unsigned threads, const char* kernel, unsigned* grid)
{
    if (blocks > ngsid_max_blocks(threads)) NGSID_FAIL(ctx, NGSID_ERR_ARG, "%s: %llu workgroups of %u exceed the 2^32 - 1 work-items of a launch", kernel, (unsigned long long)blocks, threads);
    *grid = (unsigned)blocks;
    return NGSID_OK;
}
// the checked workgroup count as an expression (for a dim3): returns NGSID_ERR_ARG from the calling function where ngsid_grid refuses, never truncates
#define NGSID_GRID(ctx, blocks, threads, kernel) ({ unsigned grid_ = 0; NGSID_TRY(ngsid_grid((ctx), (uint64_t)(blocks), (threads), (kernel), &grid_)); grid_; })

// ---- the byte budget of a chunked call: the 1 / divisor share of the device memory that is free now (+ what the allocator's cache and the caller's own grow-only
// buffers hold: both are reused), divided among the live contexts of the process, clamped to [floor, ceiling]
static inline size_t ngsid_mem_share(size_t divisor, size_t floor, size_t ceiling, size_t free_if_unknown, size_t own_bytes = 0)
{
    size_t freeb = 0, totalb = 0; if (hipMemGetInfo(&freeb, &totalb) != hipSuccess) freeb = free_if_unknown;
    return std::min(std::max((freeb + own_bytes + ngsid_pool_cached_bytes()) / (divisor * (size_t)ngsid_pool_contexts()), floor), ceiling);
}

// ---- read lists of a grouped call: reads read_order[grp_off[g] .. grp_off[g + 1]) (or the range itself without read_order) are group g
static inline int32_t ngsid_check_lists(ngsid_ctx* ctx, const uint32_t* read_order, const uint64_t* grp_off, uint64_t n_groups, uint64_t n_reads)
{
    const uint64_t NL = grp_off[n_groups];
    if (!read_order && NL > n_reads) NGSID_FAIL(ctx, NGSID_ERR_ARG, "group offsets exceed the read set");
    if (read_order) for (uint64_t x = 0; x < NL; ++x) if (read_order[x] >= n_reads) NGSID_FAIL(ctx, NGSID_ERR_ARG, "read_order[%llu] out of range", (unsigned long long)x);
    return NGSID_OK;
}

// ---- grouped-reads front end (polish_host.hip) of ngsid_polish* and of the support walk (k_support.hip): reads listed under one centre (backbone) per group.
// ngsid_groups_open: argument and list checks, the reads on the device, the centres on the host.  The caller validates and clears its own outputs, returns early where
// nothing is listed (N == 0 || G == 0), then ngsid_groups_pairs: the read -> group map (one pass over the lists; a read listed twice is an error), strands and oriented
// copies (ngsid_polish_orient), the pairs = listed reads with a strand, in list order.  The pair vectors are pinned and belong to the calling thread: valid until its next call.
struct GroupedReads {
    DevReads RD; uint64_t N = 0, NL = 0, NP = 0; uint32_t G = 0, maxb = 0;      // reads of the set, listed reads, pairs, groups, longest centre
    std::vector<uint64_t> boff; std::vector<uint8_t> bseq; std::vector<std::string> B;      // the centres: host offsets, bytes (+ one 0), strings
    std::vector<uint32_t> h_rgroup; std::vector<uint64_t> gbases;                           // group of every read (0xffffffff: none), bases listed per group
    OrientBufs ob; PinVec<uint8_t>* h_orient = nullptr;                                     // per read 0 forward, 1 reverse complement, 255 no strand; oriented copies in ctx->pol_oseq / pol_oqual
    PinVec<uint32_t> *pair_read = nullptr, *pair_group = nullptr, *pair_x = nullptr;        // per pair: read, group, position of the read in the caller's list
    std::vector<uint64_t> gbeg;                                                             // pairs [gbeg[g], gbeg[g + 1]) are group g's
};
int32_t ngsid_groups_open(ngsid_ctx* ctx, const ngsid_reads_t* centres, const ngsid_reads_t* reads, const uint32_t* read_order, const uint64_t* grp_off, uint64_t n_groups, GroupedReads& S);
int32_t ngsid_groups_pairs(ngsid_ctx* ctx, const uint32_t* read_order, const uint64_t* grp_off, int k, int w, GroupedReads& S, int8_t* strand = nullptr);      // strand: [NL], written for the pairs

// ---- pair batches of the aligner entry points: both read sets on the device, the index lists checked and uploaded, the longest query and target of the batch
struct PairBatch { DevReads Q, T; DevBuf<uint32_t> dq, dt; uint32_t mq = 0, mt = 0; };
static inline int32_t ngsid_pair_batch(ngsid_ctx* ctx, const ngsid_reads_t* queries, const ngsid_reads_t* targets, const uint32_t* q_idx, const uint32_t* t_idx, uint64_t n_pairs, PairBatch& B)
{
    if (!queries || !targets || (n_pairs && (!q_idx || !t_idx))) NGSID_FAIL(ctx, NGSID_ERR_ARG, "null argument");
    NGSID_TRY(ngsid_upload_reads(ctx, queries, &B.Q, false)); NGSID_TRY(ngsid_upload_reads(ctx, targets, &B.T, false));
    for (uint64_t p = 0; p < n_pairs; ++p) {
        if (q_idx[p] >= B.Q.n || t_idx[p] >= B.T.n) NGSID_FAIL(ctx, NGSID_ERR_ARG, "pair %llu out of range", (unsigned long long)p);
        B.mq = std::max<uint32_t>(B.mq, (uint32_t)(B.Q.h_off[q_idx[p] + 1] - B.Q.h_off[q_idx[p]]));
        B.mt = std::max<uint32_t>(B.mt, (uint32_t)(B.T.h_off[t_idx[p] + 1] - B.T.h_off[t_idx[p]]));
    }
    if (n_pairs) { NGSID_TRY(dev_put(ctx, B.dq, q_idx, n_pairs)); NGSID_TRY(dev_put(ctx, B.dt, t_idx, n_pairs)); }
    return NGSID_OK;
}
static inline int ngsid_max_open(const int32_t* open, uint64_t n)      // bound of the gap-open costs for ngsid_launch_align (a negative one: no bound)
{
    int mo = 0; for (uint64_t p = 0; p < n; ++p) { if (open[p] < 0) return 1 << 20; mo = std::max(mo, (int)open[p]); }
    return mo;
}

// ---- the temporaries of one ngsid_minimizers_csr call: the CSR, the per-read device arrays and their host mirrors
struct SketchBufs { DevBuf<uint64_t> code, off; DevBuf<uint32_t> pos, cnt, hlen; DevBuf<double> herr, rawerr; PinVec<uint64_t> h_off; PinVec<uint32_t> h_cnt, h_hlen; };
static inline int32_t ngsid_sketch(ngsid_ctx* ctx, const DevReads& R, int k, int w, SketchBufs& S, long long* bad)      // *bad: a read with a base outside ACGTN, or -1
{
    const uint64_t n = R.n; S.h_cnt.resize(n); S.h_hlen.resize(n); *bad = -1;
    HIPCHK(ctx, S.cnt.alloc(n)); HIPCHK(ctx, S.hlen.alloc(n)); HIPCHK(ctx, S.herr.alloc(n)); HIPCHK(ctx, S.rawerr.alloc(n));
    return ngsid_minimizers_csr(ctx, R, k, w, MzOut{&S.code, &S.pos, &S.off, &S.h_off}, S.cnt.p, S.hlen.p, S.herr.p, S.rawerr.p, S.h_cnt.data(), S.h_hlen.data(), bad);
}

// ---- k_demux.hip: enqueues the scan of R's bases; *d_flag (cleared by the caller) becomes non-zero when one is outside upper-case ACGTN.  The caller reads the flag
// (ngsid_demux_locate does, together with its hits); everyone else calls ngsid_alphabet_check: the flag, the scan of A and of B (or null), the read, the synchronisation,
// NGSID_ERR_ALPHABET with `message`.  prof_name: the profiling line of the scans, or null
int32_t ngsid_alphabet_scan(ngsid_ctx* ctx, const DevReads& R, uint32_t* d_flag, const char* prof_name = nullptr);
static inline int32_t ngsid_alphabet_check(ngsid_ctx* ctx, const DevReads& A, const DevReads* B, const char* prof_name, const char* message)
{
    DevBuf<uint32_t> d_flag; HIPCHK(ctx, d_flag.alloc(1));
    HIPCHK(ctx, hipMemsetAsync(d_flag.p, 0, sizeof(uint32_t), ctx->stream));
    NGSID_TRY(ngsid_alphabet_scan(ctx, A, d_flag.p, prof_name)); if (B) NGSID_TRY(ngsid_alphabet_scan(ctx, *B, d_flag.p, prof_name));
    uint32_t bad = 0;
    NGSID_TRY(dev_get(ctx, &bad, d_flag.p, 1));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (bad) NGSID_FAIL(ctx, NGSID_ERR_ALPHABET, "%s", message);
    return NGSID_OK;
}
bool ngsid_iupac_eq(uint8_t a, uint8_t b, int iupac);      // host_io.hip: the equality rule of ngsid_host_infix_locate
// the letter code of the demultiplexer and near-pairs kernels: A C G T -> 0 .. 3, anything else (N) -> 4
__device__ __forceinline__ uint32_t ngsid_base_code(uint8_t c) { return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u; }

// ---- found lists (ngsid_demux_scan, ngsid_near_pairs*, ngsid_umi_pairs): a kernel appends its records to a found buffer through ONE counter.  ngsid_found_slot takes
// the next slot and tells whether it lies inside the buffer; the counter runs on past `limit`, so a launch always yields its count, whatever it could store.
__device__ __forceinline__ bool ngsid_found_slot(unsigned long long* ctr, uint64_t limit, unsigned long long* slot) { *slot = atomicAdd(ctr, 1ull); return *slot < limit; }
// the key of a found pair of sequences: (smaller index << 32) | larger index, so that ascending keys are ascending (i, j)
__device__ __forceinline__ uint64_t ngsid_pair_key(uint32_t x, uint32_t y) { return ((uint64_t)min(x, y) << 32) | max(x, y); }
static inline void ngsid_pair_unkey(uint64_t key, uint32_t* i, uint32_t* j) { *i = (uint32_t)(key >> 32); *j = (uint32_t)key; }

// the found-buffer loop of ngsid_demux_scan and ngsid_near_pairs*: rows [0, N) in chunks of rows_first, every launch appending its records to a found buffer of F
// records.  launch(a, b, limit, launched) clears the counter (*d_ctr) and enqueues rows [a, b) (it may lower b, or clear `launched` when the rows hold nothing to launch);
// fetch(a, c) enqueues the copy of the c records of the launch that began at row a.
// -> *total: the records of all rows.  Filling stops (and counting goes on) exactly when total exceeds cap.
// ngsid_umi_pairs is not a user: its two producers (the join and the short path) feed ONE device-resident list that a device sort orders, so nothing is fetched per launch
// and a launch has no count of its own to act on - its chunk loops only bound the tile list and the launch.
template <typename Launch, typename Fetch>
static inline int32_t ngsid_found_loop(ngsid_ctx* ctx, uint64_t N, uint64_t rows_first, uint64_t F, uint64_t cap, unsigned long long* d_ctr, Launch launch, Fetch fetch,
                                       const char* row_noun, const char* record_noun, uint64_t* total_out)
{
    bool fill = cap > 0;
    uint64_t total = 0, rows_now = rows_first;
    for (uint64_t a = 0; a < N; ) {
        uint64_t b = std::min(N, a + rows_now);
        const uint64_t limit = fill ? std::min(F, cap - total) : 0;
        bool launched = true;
        NGSID_TRY(launch(a, b, limit, launched));
        if (!launched) { a = b; continue; }
        HIPCHK(ctx, hipGetLastError());
        unsigned long long c = 0;
        NGSID_TRY(dev_get(ctx, &c, d_ctr, 1));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        if (fill && c > limit) {
            if (limit == cap - total) fill = false;                     // more records than the caller has room for: count on
            else if (b - a > 1) { rows_now = (b - a) / 2; continue; }   // more than the found buffer holds: the same rows in smaller chunks
            else NGSID_FAIL(ctx, NGSID_ERR_HIP, "one %s has %llu %s: beyond the found buffer the free device memory allows", row_noun, c, record_noun);
        }
        if (fill && c) { NGSID_TRY(fetch(a, (size_t)c)); HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); }
        total += c;
        a = b;
    }
    *total_out = total;
    return NGSID_OK;
}
