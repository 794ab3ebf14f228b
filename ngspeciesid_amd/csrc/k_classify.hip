// k_classify.hip - ngsid_refdb_build / ngsid_classify_search (include/ngsid_classify.h): for every (query, strand, reference) the number of distinct minimizer
// codes they share, and per query the best top_k references.
//
// Library (built once): the references are sketched by k_hpc_minimizers (k <= 21: one-word codes, comparable between calls), every minimizer becomes a (code, ref)
// pair - the compact CSR lists them in ascending ref order -, ONE stable radix sort by code leaves the refs ascending within a code, adjacent duplicates are dropped
// (a code that occurs twice in a reference), and three arrays stay on the device: the sorted distinct codes, their posting offsets, the postings (uint32 refs).
//
// Search.  The queries are doubled on the device (forward, reverse complement) and sketched in one minimizer call; a segmented radix sort + k_classify_uniq leave the
// sorted distinct codes of every (query, strand).
// k_classify_count: one workgroup per (query, strand) of a chunk and a dense uint32 count row [n_refs] of its own.  One WAVE per query code: the code is found in the
//   library's code array by binary search (uniform in the wave), the 64 lanes stride through its posting list and atomicAdd the row; the refs within a list are
//   distinct, so only the lists of the four waves meet in a counter.  (The other form - the whole workgroup walks one list at a time with plain read-modify-write
//   stores and a barrier between lists - was measured against this one and dropped: DESIGN.md section 5, profiles/classify_count_forms.txt.)
// k_classify_topk: one workgroup per query, each of its four waves owns a contiguous quarter of the references (a multiple of 64: the "block boundary" of the selection).
//   1. histogram of the merged counts (max of the two strand rows, strand 0 on a tie) that reach min_shared, in LDS: they are bounded by the query's code count; one
//      level of 4 096 bins, or two levels of 8 bits for queries with 4 096 or more codes;  2. the threshold t with #(count > t) < top_k <= #(count >= t);  3. every
//      reference above t goes to the survivor list, the waves count their references at t;  4. the lowest-indexed references at t fill the list: a wave knows its rank
//      base from the waves before it and ranks its own by ballot;  5. the at most 64 survivors are ordered by (shared descending, ref ascending) by rank counting.
//   Integer LDS atomics build the histogram and hand out the slots of step 3; neither decides an order: the histogram is a sum and the slots are sorted in step 5.
#include "ngsid_host.h"
#include "../../include/ngsid_classify.h"
#include <hipcub/hipcub.hpp>
#include <algorithm>

typedef uint64_t u64;

#define CLS_WAVES 4
#define CLS_THREADS (CLS_WAVES * 64)
#define CLS_HIST 4096

static_assert(NGSID_CLASSIFY_MAX_TOPK == 64, "survivor list and rank sort are sized for 64");

struct ngsid_refdb {
    ngsid_ctx* ctx = nullptr;
    int k = 0, w = 0;
    uint64_t n_refs = 0, n_postings = 0, n_codes = 0;
    DevBuf<uint64_t> codes;          // [n_codes] sorted, distinct
    DevBuf<uint32_t> post_off;       // [n_codes + 1]
    DevBuf<uint32_t> post;           // [n_postings] reference indices, ascending within a code
};

namespace {

// ---- build
__global__ __launch_bounds__(64)
void k_classify_pairs(const uint64_t* __restrict__ moff, u64 n, uint32_t* __restrict__ ref)
{
    const u64 r = blockIdx.x; if (r >= n) return;
    const u64 a = moff[r], b = moff[r + 1];
    for (u64 i = a + threadIdx.x; i < b; i += 64) ref[i] = (uint32_t)r;
}

// fp: first of its (code, ref) pair; fc: first of its code
__global__ __launch_bounds__(256)
void k_classify_flags(const u64* __restrict__ scode, const uint32_t* __restrict__ sref, u64 M, uint32_t* __restrict__ fp, uint32_t* __restrict__ fc)
{
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x; if (i >= M) return;
    const bool nc = i == 0 || scode[i] != scode[i - 1];
    fc[i] = nc ? 1u : 0u; fp[i] = (nc || sref[i] != sref[i - 1]) ? 1u : 0u;
}

// rp / rc: inclusive sums of fp / fc
__global__ __launch_bounds__(256)
void k_classify_scatter(const u64* __restrict__ scode, const uint32_t* __restrict__ sref, const uint32_t* __restrict__ fp, const uint32_t* __restrict__ fc,
                        const uint32_t* __restrict__ rp, const uint32_t* __restrict__ rc, u64 M, u64* __restrict__ codes, uint32_t* __restrict__ post_off, uint32_t* __restrict__ post)
{
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x; if (i >= M) return;
    if (fp[i]) post[rp[i] - 1] = sref[i];
    if (fc[i]) { codes[rc[i] - 1] = scode[i]; post_off[rc[i] - 1] = rp[i] - 1; }
    if (i == M - 1) post_off[rc[i]] = rp[i];
}

// ---- search
__device__ __forceinline__ uint8_t cls_comp(uint8_t c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : c; }

// sequence 2 q = query q, sequence 2 q + 1 = its reverse complement (N stays N; a letter outside the alphabet stays what it is and is reported by the encoder)
__global__ __launch_bounds__(256)
void k_classify_revcomp(const uint8_t* __restrict__ seq, const uint64_t* __restrict__ off, u64 n, const uint64_t* __restrict__ doff, uint8_t* __restrict__ out)
{
    const u64 q = blockIdx.x; if (q >= n) return;
    const u64 a = off[q], L = off[q + 1] - a, f = doff[2 * q], r = doff[2 * q + 1];
    for (u64 j = threadIdx.x; j < L; j += 256) { out[f + j] = seq[a + j]; out[r + j] = cls_comp(seq[a + L - 1 - j]); }
}

// one wave per (query, strand): the distinct codes of its sorted list, written at the list's own offset; ucnt = how many
__global__ __launch_bounds__(64)
void k_classify_uniq(const u64* __restrict__ sorted, const uint64_t* __restrict__ moff, u64 nseg, u64* __restrict__ ucodes, uint32_t* __restrict__ ucnt)
{
    const u64 seg = blockIdx.x; if (seg >= nseg) return;
    const int lane = threadIdx.x;
    const u64 a = moff[seg], m = moff[seg + 1] - a;
    uint32_t outn = 0;
    for (u64 c0 = 0; c0 < m; c0 += 64) {
        const u64 i = c0 + lane; const bool in = i < m;
        const u64 code = in ? sorted[a + i] : 0;
        const bool isnew = in && (i == 0 || sorted[a + i - 1] != code);
        const u64 mask = __ballot(isnew);
        if (isnew) ucodes[a + outn + __popcll(mask & ((1ull << lane) - 1))] = code;
        outn += (uint32_t)__popcll(mask);
    }
    if (lane == 0) ucnt[seg] = outn;
}

// index of `code` in the sorted distinct codes, or n_lib
__device__ __forceinline__ uint32_t cls_find(const u64* __restrict__ lib_codes, uint32_t n_lib, u64 code)
{
    uint32_t lo = 0, hi = n_lib;
    while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (lib_codes[mid] < code) lo = mid + 1; else hi = mid; }
    return (lo < n_lib && lib_codes[lo] == code) ? lo : n_lib;
}

__global__ __launch_bounds__(CLS_THREADS)
void k_classify_count(const u64* __restrict__ ucodes, const uint64_t* __restrict__ moff, const uint32_t* __restrict__ ucnt, u64 seg0,
                      const u64* __restrict__ lib_codes, uint32_t n_lib, const uint32_t* __restrict__ post_off, const uint32_t* __restrict__ post,
                      uint32_t n_refs, uint32_t* cnt /* [gridDim.x][n_refs], zeroed */)
{
    const u64 seg = seg0 + blockIdx.x;
    const u64* qc = ucodes + moff[seg];
    const uint32_t m = ucnt[seg];
    uint32_t* row = cnt + (size_t)blockIdx.x * n_refs;
    if (n_lib == 0) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t i = wave; i < m; i += CLS_WAVES) {
        const uint32_t j = cls_find(lib_codes, n_lib, qc[i]);
        if (j == n_lib) continue;
        const uint32_t a = post_off[j], b = post_off[j + 1];
        for (uint32_t p = a + lane; p < b; p += 64) atomicAdd(&row[post[p]], 1u);
    }
}

__global__ __launch_bounds__(CLS_THREADS)
void k_classify_topk(const uint32_t* __restrict__ cnt /* [gridDim.x][2][n_refs] */, uint32_t n_refs, u64 q0, const uint32_t* __restrict__ ucnt,
                     int top_k, int min_shared, int32_t* __restrict__ cand_ref, int32_t* __restrict__ cand_shared, int8_t* __restrict__ cand_strand)
{
    __shared__ uint32_t hist[CLS_HIST];
    __shared__ uint32_t s_t, s_above, s_need, s_n, s_hi;
    __shared__ uint32_t s_ties[CLS_WAVES];
    __shared__ u64 s_key[NGSID_CLASSIFY_MAX_TOPK];
    __shared__ uint8_t s_str[NGSID_CLASSIFY_MAX_TOPK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u64 q = q0 + blockIdx.x;
    const uint32_t* r0 = cnt + (size_t)blockIdx.x * 2 * n_refs; const uint32_t* r1 = r0 + n_refs;
    int32_t* o_ref = cand_ref + q * (u64)top_k; int32_t* o_sh = cand_shared + q * (u64)top_k; int8_t* o_st = cand_strand + q * (u64)top_k;
    for (int i = tid; i < top_k; i += CLS_THREADS) { o_ref[i] = -1; o_sh[i] = -1; o_st[i] = -1; }
    const uint32_t bound = max(ucnt[2 * q], ucnt[2 * q + 1]);                     // no count of this query exceeds its code count
    const uint32_t ms = (uint32_t)min_shared, K = (uint32_t)top_k;
    if (bound < ms) return;                                                       // (uniform)
    const uint32_t segw = (((n_refs + CLS_WAVES - 1) / CLS_WAVES) + 63u) & ~63u;  // references per wave, a multiple of 64
    const u64 lo64 = (u64)wave * segw;
    const uint32_t lo = (uint32_t)min<u64>(lo64, n_refs), hi = (uint32_t)min<u64>(lo64 + segw, n_refs);
    // histogram of the bins bin(c) of the merged counts c >= min_shared with (c >> pshift) == prefix
    auto hist_pass = [&](uint32_t nbins, int shift, uint32_t mask, int pshift, uint32_t prefix) {
        for (uint32_t i = tid; i < nbins; i += CLS_THREADS) hist[i] = 0;
        __syncthreads();
        for (uint32_t r = lo + lane; r < hi; r += 64) {
            const uint32_t c = max(r0[r], r1[r]);
            if (c >= ms && (c >> pshift) == prefix) atomicAdd(&hist[(c >> shift) & mask], 1u);
        }
        __syncthreads();
    };
    // ---- 1, 2: the threshold.  (t, above, need): every reference with c > t survives (above of them), and the `need` lowest-indexed ones with c == t
    const bool two = bound >= CLS_HIST;
    const uint32_t nb1 = two ? (bound >> 8) + 1 : bound + 1;                      // bound <= NGSID_MAX_READ_LEN = 65 535: at most 256 bins on the first level
    hist_pass(nb1, two ? 8 : 0, CLS_HIST - 1, 31, 0u);
    if (tid == 0) {
        uint32_t total = 0;
        for (uint32_t b = 0; b < nb1; ++b) total += hist[b];
        s_n = 0;
        if (total <= K) { s_t = ms - 1; s_above = total; s_need = 0; s_hi = 0xffffffffu; }         // every candidate survives
        else {
            uint32_t cum = 0, b = nb1 - 1;
            while (cum + hist[b] < K) { cum += hist[b]; --b; }                    // (total > K: stops at some b >= 0)
            s_t = b; s_above = cum; s_need = K - cum; s_hi = b;
        }
    }
    __syncthreads();
    if (two && s_hi != 0xffffffffu) {                                            // second level: the low 8 bits of the counts in bin s_hi
        const uint32_t H = s_hi, above_h = s_above;
        __syncthreads();
        hist_pass(256, 0, 255, 8, H);
        if (tid == 0) {
            uint32_t cum = above_h, b = 255;
            while (cum + hist[b] < K) { cum += hist[b]; --b; }
            s_t = (H << 8) | b; s_above = cum; s_need = K - cum;
        }
        __syncthreads();
    }
    const uint32_t t = s_t, above = s_above, need = s_need;
    // ---- 3: survivors above t (any slot: they are ordered below), ties per wave
    uint32_t ties = 0;
    for (uint32_t rb = lo; rb < hi; rb += 64) {
        const uint32_t r = rb + lane; const bool in = r < hi;
        const uint32_t c0 = in ? r0[r] : 0u, c1 = in ? r1[r] : 0u, c = max(c0, c1);
        if (in && c > t) { const uint32_t s = atomicAdd(&s_n, 1u); s_key[s] = ((u64)(0xffffffffu - c) << 32) | r; s_str[s] = c1 > c0 ? 1 : 0; }
        ties += (uint32_t)__popcll(__ballot(in && c == t && c >= ms));
    }
    if (lane == 0) s_ties[wave] = ties;
    __syncthreads();
    // ---- 4: the lowest-indexed references at t
    if (need) {
        uint32_t base = 0;
        for (int x = 0; x < wave; ++x) base += s_ties[x];
        for (uint32_t rb = lo; rb < hi && base < need; rb += 64) {
            const uint32_t r = rb + lane; const bool in = r < hi;
            const uint32_t c0 = in ? r0[r] : 0u, c1 = in ? r1[r] : 0u, c = max(c0, c1);
            const bool tie = in && c == t;
            const u64 mask = __ballot(tie);
            const uint32_t rank = base + (uint32_t)__popcll(mask & ((1ull << lane) - 1));
            if (tie && rank < need) { s_key[above + rank] = ((u64)(0xffffffffu - c) << 32) | r; s_str[above + rank] = c1 > c0 ? 1 : 0; }
            base += (uint32_t)__popcll(mask);
        }
    }
    __syncthreads();
    // ---- 5: order by (shared descending, ref ascending): keys are distinct
    const uint32_t ns = above + need;
    if ((uint32_t)tid < ns) {
        const u64 key = s_key[tid];
        uint32_t rank = 0;
        for (uint32_t j = 0; j < ns; ++j) rank += s_key[j] < key ? 1u : 0u;
        o_ref[rank] = (int32_t)(uint32_t)(key & 0xffffffffu); o_sh[rank] = (int32_t)(0xffffffffu - (uint32_t)(key >> 32)); o_st[rank] = (int8_t)s_str[tid];
    }
}

}  // namespace

void ngsid_refdb_release_all(ngsid_ctx* ctx)
{
    for (ngsid_refdb* db : ctx->refdbs) delete db;
    ctx->refdbs.clear();
}

static int32_t cls_check_kw(ngsid_ctx* ctx, int k, int w)
{
    if (k < 1 || k > 21 || w < k || w > 255) NGSID_FAIL(ctx, NGSID_ERR_ARG, "k must be in [1,21] (one-word codes, comparable between calls) and k <= w <= 255 (k=%d w=%d)", k, w);
    return NGSID_OK;
}

extern "C" int32_t ngsid_refdb_build(ngsid_ctx* ctx, const ngsid_reads_t* refs, const ngsid_refdb_params_t* prm, ngsid_refdb** out)
{
    ApiClock api_clock_(ctx, "refdb_build");
    if (!ctx) return NGSID_ERR_ARG;
    if (!refs || !prm || !out) NGSID_FAIL(ctx, NGSID_ERR_ARG, "null argument");
    *out = nullptr;
    int32_t rc = cls_check_kw(ctx, prm->k, prm->w); if (rc) return rc;
    if (refs->mem != NGSID_MEM_HOST) NGSID_FAIL(ctx, NGSID_ERR_ARG, "the references are a host read set");
    if (refs->n == 0 || refs->n > NGSID_CLASSIFY_MAX_REFS) NGSID_FAIL(ctx, NGSID_ERR_ARG, "1 .. %u references expected", NGSID_CLASSIFY_MAX_REFS);
    ngsid_reads_t noq = *refs; noq.qual = nullptr;                       // qualities never influence a code
    DevReads R; rc = ngsid_upload_reads(ctx, &noq, &R, false); if (rc) return rc;
    const uint64_t n = R.n;
    SketchBufs K; long long bad;
    rc = ngsid_sketch(ctx, R, prm->k, prm->w, K, &bad); if (rc) return rc;
    DevBuf<uint64_t> &ccode = K.code, &coff = K.off; DevBuf<uint32_t>& cpos = K.pos; const PinVec<uint64_t>& hmoff = K.h_off;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (bad >= 0) NGSID_FAIL(ctx, NGSID_ERR_ALPHABET, "reference %lld: base outside upper-case ACGTN", bad);
    const uint64_t M = hmoff[n];
    if (M >= 0x7fffffffull) NGSID_FAIL(ctx, NGSID_ERR_TOO_LONG, "the references hold %llu minimizers: a library is limited to 2^31 - 1", (unsigned long long)M);
    std::unique_ptr<ngsid_refdb> db(new ngsid_refdb());
    db->ctx = ctx; db->k = prm->k; db->w = prm->w; db->n_refs = n;
    uint32_t h_np = 0, h_nc = 0;
    if (M == 0) {
        HIPCHK(ctx, db->codes.alloc(1)); HIPCHK(ctx, db->post.alloc(1)); HIPCHK(ctx, db->post_off.alloc(1));
        HIPCHK(ctx, hipMemsetAsync(db->post_off.p, 0, sizeof(uint32_t), ctx->stream));
    } else {
        DevBuf<uint64_t> scode; DevBuf<uint32_t> ref, sref, fp, fc, rp, rcs; DevBuf<unsigned char> tmp;
        HIPCHK(ctx, scode.alloc(M)); HIPCHK(ctx, ref.alloc(M)); HIPCHK(ctx, sref.alloc(M));
        { ProfScope ps_(ctx, "k_classify_pairs");
          hipLaunchKernelGGL(k_classify_pairs, dim3(NGSID_GRID(ctx, n, 64, "k_classify_pairs")), dim3(64), 0, ctx->stream, coff.p, (u64)n, ref.p); }
        HIPCHK(ctx, hipGetLastError());
        size_t tb = 0;
        HIPCHK(ctx, hipcub::DeviceRadixSort::SortPairs(nullptr, tb, ccode.p, scode.p, ref.p, sref.p, (int)M, 0, 3 * prm->k, ctx->stream));
        HIPCHK(ctx, tmp.alloc(tb));
        { ProfScope ps_(ctx, "hipcub_classify_sort");
          HIPCHK(ctx, hipcub::DeviceRadixSort::SortPairs(tmp.p, tb, ccode.p, scode.p, ref.p, sref.p, (int)M, 0, 3 * prm->k, ctx->stream)); }      // stable: refs stay ascending within a code
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        ccode.release(); cpos.release(); ref.release();
        HIPCHK(ctx, fp.alloc(M)); HIPCHK(ctx, fc.alloc(M)); HIPCHK(ctx, rp.alloc(M)); HIPCHK(ctx, rcs.alloc(M));
        const unsigned gb = (unsigned)((M + 255) / 256);
        { ProfScope ps_(ctx, "k_classify_flags");
          hipLaunchKernelGGL(k_classify_flags, dim3(gb), dim3(256), 0, ctx->stream, scode.p, sref.p, (u64)M, fp.p, fc.p); }
        HIPCHK(ctx, hipGetLastError());
        size_t tb2 = 0;
        HIPCHK(ctx, hipcub::DeviceScan::InclusiveSum(nullptr, tb2, fp.p, rp.p, (int)M, ctx->stream));
        if (tb2 > tb) { HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); HIPCHK(ctx, tmp.alloc(tb2)); tb = tb2; }
        HIPCHK(ctx, hipcub::DeviceScan::InclusiveSum(tmp.p, tb2, fp.p, rp.p, (int)M, ctx->stream));
        HIPCHK(ctx, hipcub::DeviceScan::InclusiveSum(tmp.p, tb2, fc.p, rcs.p, (int)M, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(&h_np, rp.p + (M - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(&h_nc, rcs.p + (M - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        HIPCHK(ctx, db->codes.alloc(h_nc)); HIPCHK(ctx, db->post_off.alloc((size_t)h_nc + 1)); HIPCHK(ctx, db->post.alloc(h_np));
        { ProfScope ps_(ctx, "k_classify_scatter");
          hipLaunchKernelGGL(k_classify_scatter, dim3(gb), dim3(256), 0, ctx->stream, scode.p, sref.p, fp.p, fc.p, rp.p, rcs.p, (u64)M, db->codes.p, db->post_off.p, db->post.p); }
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    db->n_postings = h_np; db->n_codes = h_nc;
    ctx->refdbs.push_back(db.get());
    *out = db.release();
    return NGSID_OK;
}

extern "C" int32_t ngsid_refdb_info(const ngsid_refdb* db, uint64_t* n_refs, uint64_t* n_postings, uint64_t* n_codes, uint64_t* device_bytes)
{
    if (!db) return NGSID_ERR_ARG;
    if (n_refs) *n_refs = db->n_refs;
    if (n_postings) *n_postings = db->n_postings;
    if (n_codes) *n_codes = db->n_codes;
    if (device_bytes) *device_bytes = (uint64_t)db->codes.abytes + db->post_off.abytes + db->post.abytes;
    return NGSID_OK;
}

extern "C" int32_t ngsid_refdb_release(ngsid_ctx* ctx, ngsid_refdb* db)
{
    ApiClock api_clock_(ctx, "refdb_release");
    if (!ctx) return NGSID_ERR_ARG;
    if (!db) return NGSID_OK;
    auto it = std::find(ctx->refdbs.begin(), ctx->refdbs.end(), db);
    if (it == ctx->refdbs.end()) NGSID_FAIL(ctx, NGSID_ERR_ARG, "this reference library does not belong to the context (or was released already)");
    ctx->refdbs.erase(it);
    delete db;
    return NGSID_OK;
}

extern "C" int32_t ngsid_classify_search(ngsid_ctx* ctx, const ngsid_refdb* db, const ngsid_reads_t* queries, const ngsid_classify_params_t* prm,
                                         int32_t* cand_ref, int32_t* cand_shared, int8_t* cand_strand, int32_t* n_codes)
{
    ApiClock api_clock_(ctx, "classify_search");
    if (!ctx) return NGSID_ERR_ARG;
    if (!db || !queries || !prm) NGSID_FAIL(ctx, NGSID_ERR_ARG, "null argument");
    if (std::find(ctx->refdbs.begin(), ctx->refdbs.end(), db) == ctx->refdbs.end()) NGSID_FAIL(ctx, NGSID_ERR_ARG, "this reference library does not belong to the context (or was released already)");
    if (prm->top_k < 1 || prm->top_k > NGSID_CLASSIFY_MAX_TOPK) NGSID_FAIL(ctx, NGSID_ERR_ARG, "ngsid_classify_params_t.top_k must be 1 .. %d", NGSID_CLASSIFY_MAX_TOPK);
    if (prm->min_shared < 1) NGSID_FAIL(ctx, NGSID_ERR_ARG, "ngsid_classify_params_t.min_shared must be at least 1");
    DevReads RD; int32_t rc = ngsid_upload_reads(ctx, queries, &RD, false); if (rc) return rc;
    const uint64_t N = RD.n;
    if (N == 0) return NGSID_OK;
    if (!cand_ref || !cand_shared || !cand_strand) NGSID_FAIL(ctx, NGSID_ERR_ARG, "null output");
    if (N > 0x3fffffffull) NGSID_FAIL(ctx, NGSID_ERR_ARG, "more than 2^30 queries in one call");
    if (RD.maxlen > NGSID_MAX_READ_LEN) NGSID_FAIL(ctx, NGSID_ERR_TOO_LONG, "query of %u bases exceeds NGSID_MAX_READ_LEN=%d", RD.maxlen, NGSID_MAX_READ_LEN);
    const int top_k = prm->top_k;
    // ---- both strands of every query as one read set
    const uint64_t b0 = RD.h_off[0], T = RD.h_off[N] - b0;
    DevReads D2; D2.n = 2 * N; D2.total = 2 * T; D2.maxlen = RD.maxlen; D2.minlen = RD.minlen; D2.h_off.resize(2 * N + 1);
    for (uint64_t q = 0; q < N; ++q) { const uint64_t a = RD.h_off[q] - b0, L = RD.h_off[q + 1] - RD.h_off[q]; D2.h_off[2 * q] = 2 * a; D2.h_off[2 * q + 1] = 2 * a + L; }
    D2.h_off[2 * N] = 2 * T;
    HIPCHK(ctx, D2.own_seq.alloc(2 * T + 16)); NGSID_TRY(dev_put(ctx, D2.own_off, D2.h_off.data(), 2 * N + 1));
    { ProfScope ps_(ctx, "k_classify_revcomp");
      hipLaunchKernelGGL(k_classify_revcomp, dim3(NGSID_GRID(ctx, N, 256, "k_classify_revcomp")), dim3(256), 0, ctx->stream, RD.seq, RD.off, (u64)N, D2.own_off.p, D2.own_seq.p); }
    HIPCHK(ctx, hipGetLastError());
    D2.seq = D2.own_seq.p; D2.off = D2.own_off.p; D2.qual = nullptr;
    // ---- their sketches: sorted distinct codes per (query, strand)
    const uint64_t S = 2 * N;
    DevBuf<uint64_t> scode, ucode; DevBuf<uint32_t> ucnt; SketchBufs K; long long bad;
    rc = ngsid_sketch(ctx, D2, db->k, db->w, K, &bad); if (rc) return rc;
    DevBuf<uint64_t> &ccode = K.code, &coff = K.off; const PinVec<uint64_t>& hmoff = K.h_off;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (bad >= 0) NGSID_FAIL(ctx, NGSID_ERR_ALPHABET, "query %lld: base outside upper-case ACGTN", bad / 2);
    const uint64_t M = hmoff[S];
    if (M >= 0x7fffffffull) NGSID_FAIL(ctx, NGSID_ERR_TOO_LONG, "the queries hold %llu minimizers: a call is limited to 2^31 - 1", (unsigned long long)M);
    HIPCHK(ctx, scode.alloc(M)); HIPCHK(ctx, ucode.alloc(M)); HIPCHK(ctx, ucnt.alloc(S));
    if (M) {
        DevBuf<unsigned char> tmp; size_t tb = 0;
        HIPCHK(ctx, hipcub::DeviceSegmentedRadixSort::SortKeys(nullptr, tb, ccode.p, scode.p, (int)M, (int)S, coff.p, coff.p + 1, 0, 3 * db->k, ctx->stream));
        HIPCHK(ctx, tmp.alloc(tb));
        { ProfScope ps_(ctx, "hipcub_classify_sort");
          HIPCHK(ctx, hipcub::DeviceSegmentedRadixSort::SortKeys(tmp.p, tb, ccode.p, scode.p, (int)M, (int)S, coff.p, coff.p + 1, 0, 3 * db->k, ctx->stream)); }
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));          // (tmp goes out of scope)
    }
    { ProfScope ps_(ctx, "k_classify_uniq");
      hipLaunchKernelGGL(k_classify_uniq, dim3(NGSID_GRID(ctx, S, 64, "k_classify_uniq")), dim3(64), 0, ctx->stream, scode.p, coff.p, (u64)S, ucode.p, ucnt.p); }
    HIPCHK(ctx, hipGetLastError());
    // ---- chunks of queries: two count rows each, under a share of the free device memory
    const uint32_t n_refs = (uint32_t)db->n_refs;
    const size_t row_bytes = (size_t)2 * n_refs * sizeof(uint32_t);
    uint64_t chunk = N;
    const long long opt = ngsid_opt(ctx, "classify_chunk_queries", 0);
    if (opt > 0) chunk = std::min<uint64_t>(N, (uint64_t)opt);
    else chunk = std::min<uint64_t>(N, std::max<uint64_t>(1, ngsid_mem_share(4, (size_t)64 << 20, (size_t)16 << 30, (size_t)4 << 30) / row_bytes));
    HIPCHK(ctx, ctx->cls_cnt.reserve((size_t)chunk * 2 * n_refs));
    DevBuf<int32_t> d_ref, d_sh; DevBuf<int8_t> d_st;
    HIPCHK(ctx, d_ref.alloc(N * top_k)); HIPCHK(ctx, d_sh.alloc(N * top_k)); HIPCHK(ctx, d_st.alloc(N * top_k));
    for (uint64_t c0 = 0; c0 < N; c0 += chunk) {
        const uint64_t nq = std::min(N, c0 + chunk) - c0;
        HIPCHK(ctx, hipMemsetAsync(ctx->cls_cnt.p, 0, nq * row_bytes, ctx->stream));
        { ProfScope ps_(ctx, "k_classify_count");
          hipLaunchKernelGGL(k_classify_count, dim3(NGSID_GRID(ctx, 2 * nq, CLS_THREADS, "k_classify_count")), dim3(CLS_THREADS), 0, ctx->stream, ucode.p, coff.p, ucnt.p, (u64)(2 * c0),
                             db->codes.p, (uint32_t)db->n_codes, db->post_off.p, db->post.p, n_refs, ctx->cls_cnt.p); }
        HIPCHK(ctx, hipGetLastError());
        { ProfScope ps_(ctx, "k_classify_topk");
          hipLaunchKernelGGL(k_classify_topk, dim3(NGSID_GRID(ctx, nq, CLS_THREADS, "k_classify_topk")), dim3(CLS_THREADS), 0, ctx->stream, ctx->cls_cnt.p, n_refs, (u64)c0, ucnt.p, top_k, prm->min_shared, d_ref.p, d_sh.p, d_st.p); }
        HIPCHK(ctx, hipGetLastError());
    }
    NGSID_TRY(dev_get(ctx, cand_ref, d_ref.p, N * top_k)); NGSID_TRY(dev_get(ctx, cand_shared, d_sh.p, N * top_k)); NGSID_TRY(dev_get(ctx, cand_strand, d_st.p, N * top_k));
    if (n_codes) NGSID_TRY(dev_get(ctx, (uint32_t*)n_codes, ucnt.p, S));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return NGSID_OK;
}
