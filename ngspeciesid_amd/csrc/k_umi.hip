// k_umi.hip - ngsid_umi_pairs / ngsid_umi_centroids (include/ngsid_umi.h): which sequences of up to 64 letters lie within d <= 8 edits of each other, by a seeded search
// instead of the all-pairs tiles of k_near.hip, and the greedy centroid pass over the pair list.
//
// The rule (d = max_dist, g = seed_len).  A sequence is seedable when it has at least (d + 1) g letters; its seeds are the segments [j g, (j + 1) g), j = 0 .. d.  If
// ed(A, B) <= d and A is seedable, one of the d + 1 disjoint seeds of A carries no edit, and the indels in front of it shift it by at most d: seed j of A occurs exactly
// in B at position j g + s, |s| <= d.  (tests/test_umi_seed_model_cpu.py runs the rule, the keys and the dedupe rule below on Python ints against brute force.)
//
// k_umi_keys: one lane per sequence.  Its letters become three bit planes (bit p of plane k = bit k of the code of letter p, A C G T N = 0 .. 4: N is a letter like any
//   other) and go, with the length, to a 32-byte record; every seedable sequence writes its d + 1 index entries (key, sequence), key = j << 48 | the g bits of plane 2
//   << 32 | plane 1 << 16 | plane 0 - three bits per letter in 48 bits, four bits of j -, a sequence that is not seedable writes d + 1 entries of a key no query forms.
//   ONE stable hipcub radix sort over the 52 key bits leaves the sequence numbers ascending within a key.
// k_umi_ranges: one lane per (query B, q), q = j (2 d + 1) + s + d: the key of B's substring at j g + s (none where it would leave B), its entries with a sequence number
//   below B's (the index side of a pair is always the smaller index: within a key those entries are a prefix) -> first entry, count, tiles of 64.  The first entry by
//   a binary search over every 64th key (k_umi_sample: a table that stays in the caches) and then between two samples, the end of the prefix by galloping from there.
//   An inclusive sum over the tiles of the chunk and k_umi_tiles (every entry writes its number into the tiles it owns) make the work list.
// k_umi_join: one WAVE per tile = 64 candidates A of one (B, q), read from the tile list - a bucket of thousands (a deep bin of identical
//   sequences) is spread over as many waves as it has tiles, no wave walks a bucket alone.  B, j, s and the planes of B are wave-uniform (scalar registers); a lane loads
//   the 32-byte record of its A.  First-witness rule, in registers: the pair is verified in this tile only if no q' < q is a witness too (seed j' of A equal to B's
//   substring at j' g + s', three shifted xors under the seed mask per q'); every pair therefore goes through the column exactly once, whatever matches.
//   Verification: one 64-bit Myers / Hyyro column per text letter, B the pattern (Eq from the planes, as in k_near.hip: ~((B0 ^ T0) | (B1 ^ T1) | (B2 ^ T2)) under B's
//   length mask, T the 0 / -1 masks of A's letter), global distance (the horizontal delta shifted in at row 0 is +1), the value tracked on the diagonal of (m, n) -
//   it never decreases, so a lane leaves at d + 1.  No LDS, no traceback.  A found pair is appended through one counter; the records are ordered by one more radix sort.
// k_umi_short: the pairs whose smaller-index member x is not seedable (short sequences, a seed_len too large for the set): x against every y > x whose length is within d
//   of x's - the set is ordered by length on the host -, the same column.  Together the two paths see every pair i < j exactly once: the join where i is seedable, the
//   short path where it is not.
// Considered and not built: one wave per query B that walks all of B's buckets itself (B's planes stay resident and no tile list is needed, but one wave serialises a
//   bucket of thousands, and the lanes of a bucket of three idle just the same) - DESIGN.md section 5.
#include "ngsid_host.h"
#include "../../include/ngsid_umi.h"
#include <hipcub/hipcub.hpp>
#include <numeric>

typedef uint64_t u64;

static_assert(NGSID_UMI_MAX_LEN == 64, "one 64-bit word per letter plane and per Myers column");
static_assert(NGSID_UMI_MAX_DIST + 1 < 15, "four bits of the key hold the seed number, 15 marks an entry no query matches");

namespace {

#define UMI_NOKEY ((15ull << 48) | 0xffffffffffffull)      // the key of an entry that is not a seed
#define UMI_KEY_BITS 52
#define UMI_NSTAT 64                    // candidate counters of a profiled call ...
#define UMI_STAT_STRIDE 16              // ... 128 bytes apart, behind the counter of the found pairs

struct __attribute__((aligned(32))) UmiPack { u64 p0, p1, p2, len; };

// the key of the g letters at pos of the planes (gm = the low g bits), seed number j
__device__ __forceinline__ u64 umi_key(u64 p0, u64 p1, u64 p2, int pos, int j, u64 gm)
{
    return ((u64)j << 48) | (((p2 >> pos) & gm) << 32) | (((p1 >> pos) & gm) << 16) | ((p0 >> pos) & gm);
}

__global__ __launch_bounds__(256)
void k_umi_keys(const uint8_t* __restrict__ seq, const uint64_t* __restrict__ off, u64 n, int d, int g, UmiPack* __restrict__ pack, u64* __restrict__ key, uint32_t* __restrict__ val)
{
    const u64 s = (u64)blockIdx.x * 256 + threadIdx.x;
    if (s >= n) return;
    const u64 a = off[s];
    const int L = (int)min((u64)NGSID_UMI_MAX_LEN, off[s + 1] - a);      // (the host refuses longer sequences before the launch)
    u64 p0 = 0, p1 = 0, p2 = 0;
    for (int i = 0; i < L; ++i) {
        const u64 c = ngsid_base_code(seq[a + i]);
        p0 |= (c & 1) << i; p1 |= ((c >> 1) & 1) << i; p2 |= ((c >> 2) & 1) << i;
    }
    UmiPack P; P.p0 = p0; P.p1 = p1; P.p2 = p2; P.len = (u64)L;
    pack[s] = P;
    const bool seedable = L >= (d + 1) * g;
    const u64 gm = (1ull << g) - 1;
    for (int j = 0; j <= d; ++j) {
        const u64 e = s * (u64)(d + 1) + j;
        key[e] = seedable ? umi_key(p0, p1, p2, j * g, j, gm) : UMI_NOKEY;
        val[e] = (uint32_t)s;
    }
}

// every 64th key of the sorted index: the first level of the lookup (a table that stays in the caches)
__global__ __launch_bounds__(256)
void k_umi_sample(const u64* __restrict__ skey, uint32_t S, u64* __restrict__ samp)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < S) samp[i] = skey[(u64)i * 64];
}

// entry idx of the chunk = (query b0 + idx / Q, q = idx % Q): lo = its first index entry, cnt = how many of the key's entries belong to a smaller sequence, tile = cnt in 64s.
// The first entry with the key: a binary search in the samples (S = ceil(M / 64) of them), then in the 63 keys between two samples.  The end of the prefix of smaller
// sequences: galloping from the first entry (most buckets hold a few entries of one cache line), then a binary search in the last step
__global__ __launch_bounds__(256)
void k_umi_ranges(const UmiPack* __restrict__ pack, const u64* __restrict__ skey, const uint32_t* __restrict__ sval, uint32_t M, const u64* __restrict__ samp, uint32_t S,
                  u64 b0, uint32_t nidx, int d, int g, uint32_t* __restrict__ lo_out, uint32_t* __restrict__ cnt_out, u64* __restrict__ tile)
{
    const uint32_t idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= nidx) return;
    const int W = 2 * d + 1, Q = (d + 1) * W;
    const u64 b = b0 + idx / Q;
    const int q = (int)(idx % Q), j = q / W, s = q % W - d, pos = j * g + s;
    const UmiPack P = pack[b];
    uint32_t first = 0, cnt = 0;
    if (pos >= 0 && pos + g <= (int)P.len) {
        const u64 K = umi_key(P.p0, P.p1, P.p2, pos, j, (1ull << g) - 1);
        uint32_t lo = 0, hi = S;                                     // the first sample >= K
        while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (samp[mid] < K) lo = mid + 1; else hi = mid; }
        if (lo > 0) {                                                // skey[64 (lo - 1)] < K, and skey[64 lo] >= K where it exists: the first entry >= K lies in between
            uint32_t a = (lo - 1) * 64 + 1, e = min((u64)lo * 64, (u64)M);
            while (a < e) { const uint32_t mid = a + ((e - a) >> 1); if (skey[mid] < K) a = mid + 1; else e = mid; }
            first = a;
        }
        const auto mine = [&](uint32_t e) { return skey[e] == K && (u64)sval[e] < b; };      // (e >= first: its key is at least K)
        if (first < M && mine(first)) {
            uint32_t p = first, step = 1, end = M;                   // mine(p) holds; end: an entry that is not mine, or M
            while (true) { const u64 nx = (u64)p + step; if (nx >= M) break; if (mine((uint32_t)nx)) { p = (uint32_t)nx; step <<= 1; } else { end = (uint32_t)nx; break; } }
            uint32_t a = p + 1;
            while (a < end) { const uint32_t mid = a + ((end - a) >> 1); if (mine(mid)) a = mid + 1; else end = mid; }
            cnt = a - first;
        }
    }
    lo_out[idx] = first; cnt_out[idx] = cnt; tile[idx] = ((u64)cnt + 63) >> 6;
}

// B (m letters) the pattern, A (n letters) the text -> ed(A, B) if it is <= d, else -1
__device__ __forceinline__ int umi_column_ed(u64 B0, u64 B1, u64 B2, int m, u64 A0, u64 A1, u64 A2, int n, int d)
{
    const int dl = m - n;
    int val = dl < 0 ? -dl : dl;
    if (val > d) return -1;
    if (m == 0 || n == 0) return val;
    const u64 mm = m == 64 ? ~0ull : (1ull << m) - 1;
    u64 Pv = ~0ull, Mv = 0;
    for (int c = 0; c < n; ++c) {
        const u64 T0 = (u64)0 - ((A0 >> c) & 1), T1 = (u64)0 - ((A1 >> c) & 1), T2 = (u64)0 - ((A2 >> c) & 1);
        const u64 Eq = ~((B0 ^ T0) | (B1 ^ T1) | (B2 ^ T2)) & mm;
        const u64 D0 = (((Eq & Pv) + Pv) ^ Pv) | Eq | Mv;
        u64 Ph = Mv | ~(D0 | Pv);
        u64 Mh = Pv & D0;
        const int row = c + 1 + dl;                                  // the row of the diagonal of (m, n) in this column: 1 .. m once it has entered the matrix
        if (row >= 1) val += 1 - (int)((D0 >> (row - 1)) & 1);
        if (val > d) return -1;
        Ph = (Ph << 1) | 1; Mh <<= 1;
        Pv = Mh | ~(D0 | Ph);
        Mv = Ph & D0;
    }
    return val;
}

__device__ __forceinline__ void umi_emit(uint32_t x, uint32_t y, int dist, u64* __restrict__ fkey, uint8_t* __restrict__ fdist, u64 limit, unsigned long long* ctr)
{
    unsigned long long slot;
    if (ngsid_found_slot(ctr, limit, &slot)) { fkey[slot] = ngsid_pair_key(x, y); fdist[slot] = (uint8_t)dist; }
}

// the tile list of the chunk: entry idx owns the tiles tsum[idx] - tiles(idx) .. tsum[idx] - 1 (tsum = inclusive sums of the tiles) and writes its number into each
__global__ __launch_bounds__(256)
void k_umi_tiles(const u64* __restrict__ tsum, const uint32_t* __restrict__ rcnt, uint32_t nidx, uint32_t* __restrict__ tidx)
{
    const uint32_t idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= nidx) return;
    const u64 nt = ((u64)rcnt[idx] + 63) >> 6, base = tsum[idx] - nt;
    for (u64 t = 0; t < nt; ++t) tidx[base + t] = idx;
}

// tile T of the chunk belongs to the entry idx = tidx[T]: candidates 64 t .. 64 t + 63 of its range, t = T - (tsum[idx] - tiles(idx)).
// ctr[0]: found pairs; while profiling (count != 0) the pairs that went through the column are counted in UMI_NSTAT counters a cache line apart behind it - one
// counter that every wave of the launch adds to made k_umi_join 294 ms instead of 46 ms at a million keys (profiles/umi.txt), so an unprofiled call counts nothing
__global__ __launch_bounds__(256)
void k_umi_join(const UmiPack* __restrict__ pack, const uint32_t* __restrict__ sval, const u64* __restrict__ tsum, const uint32_t* __restrict__ tidx, const uint32_t* __restrict__ rlo,
                const uint32_t* __restrict__ rcnt, u64 b0, u64 ntiles, int d, int g, u64* __restrict__ fkey, uint8_t* __restrict__ fdist, u64 limit, unsigned long long* ctr, int count)
{
    const int lane = threadIdx.x & 63;
    const u64 Tl = (u64)blockIdx.x * 4 + (threadIdx.x >> 6);
    const u64 T = ((u64)(uint32_t)__builtin_amdgcn_readfirstlane((int)(Tl >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)Tl);
    if (T >= ntiles) return;
    const uint32_t idx = tidx[T], cnt = rcnt[idx];
    const u64 t = T - (tsum[idx] - (((u64)cnt + 63) >> 6));
    const int S = 2 * d + 1, Q = (d + 1) * S;
    const u64 b = b0 + idx / Q;
    const int q = (int)(idx % Q);
    const u64 e = 64 * t + lane;
    if (e >= cnt) return;
    const uint32_t a = sval[(u64)rlo[idx] + e];
    const UmiPack PB = pack[b], PA = pack[a];
    const int m = (int)PB.len, n = (int)PA.len;
    // first witness: an earlier (j', s') at which seed j' of A equals B's substring verifies the pair in its own tile
    const u64 gm = (1ull << g) - 1;
    bool first = true;
    for (int q2 = 0; q2 < q; ++q2) {
        const int j2 = q2 / S, pos2 = j2 * g + q2 % S - d;
        if (pos2 < 0 || pos2 + g > m) continue;
        const int ja = j2 * g;
        const u64 x = ((PA.p0 >> ja) ^ (PB.p0 >> pos2)) | ((PA.p1 >> ja) ^ (PB.p1 >> pos2)) | ((PA.p2 >> ja) ^ (PB.p2 >> pos2));
        if ((x & gm) == 0) first = false;
    }
    if (!first) return;
    const int dl = m - n;
    if (dl > d || -dl > d) return;
    if (count) atomicAdd(ctr + UMI_STAT_STRIDE * (1 + (blockIdx.x & (UMI_NSTAT - 1))), 1ull);
    const int dist = umi_column_ed(PB.p0, PB.p1, PB.p2, m, PA.p0, PA.p1, PA.p2, n, d);
    if (dist >= 0) umi_emit(a, (uint32_t)b, dist, fkey, fdist, limit, ctr);
}

// row r of the launch = the sequence x = ns[r0 + r], not seedable: against order[p], p in lstart[max(m - d, 0)] .. lstart[min(m + d, 64) + 1] - 1 (the set ordered by
// length, lstart[L] = the first position of length L), every y > x of them; the block's threads and the blocks along y stride through the range
__global__ __launch_bounds__(256)
void k_umi_short(const UmiPack* __restrict__ pack, const uint32_t* __restrict__ ns, const uint32_t* __restrict__ order, const uint32_t* __restrict__ lstart, u64 r0, int d,
                 u64* __restrict__ fkey, uint8_t* __restrict__ fdist, u64 limit, unsigned long long* ctr, int count)
{
    const uint32_t x = ns[r0 + blockIdx.x];
    const UmiPack PB = pack[x];
    const int m = (int)PB.len;
    const uint32_t pa = lstart[max(m - d, 0)], pb = lstart[min(m + d, NGSID_UMI_MAX_LEN) + 1];
    for (u64 p = (u64)pa + (u64)blockIdx.y * 256 + threadIdx.x; p < pb; p += (u64)256 * gridDim.y) {
        const uint32_t y = order[p];
        if (y <= x) continue;
        const UmiPack PA = pack[y];
        if (count) atomicAdd(ctr + UMI_STAT_STRIDE * (1 + ((blockIdx.x + blockIdx.y) & (UMI_NSTAT - 1))), 1ull);
        const int dist = umi_column_ed(PB.p0, PB.p1, PB.p2, m, PA.p0, PA.p1, PA.p2, (int)PA.len, d);
        if (dist >= 0) umi_emit(x, y, dist, fkey, fdist, limit, ctr);
    }
}

// stable radix sort of (key, value) pairs on the context's stream, the temporary storage in ctx->umi_tmp
template <typename V>
int32_t umi_sort(ngsid_ctx* ctx, const u64* kin, u64* kout, const V* vin, V* vout, uint64_t n, int bits, const char* prof_name)
{
    size_t tb = 0;
    HIPCHK(ctx, hipcub::DeviceRadixSort::SortPairs(nullptr, tb, kin, kout, vin, vout, (int)n, 0, bits, ctx->stream));
    HIPCHK(ctx, ctx->umi_tmp.reserve(tb));
    ProfScope ps_(ctx, prof_name);
    HIPCHK(ctx, hipcub::DeviceRadixSort::SortPairs(ctx->umi_tmp.p, tb, kin, kout, vin, vout, (int)n, 0, bits, ctx->stream));
    return NGSID_OK;
}

int32_t umi_pairs_run(ngsid_ctx* ctx, const ngsid_reads_t* seqs, const ngsid_umi_params_t* prm, uint32_t* pair_i, uint32_t* pair_j, uint8_t* dist, uint64_t cap, uint64_t* n_found, uint64_t* needed)
{
    if (!seqs || !prm || !n_found || !needed || (cap && (!pair_i || !pair_j || !dist))) NGSID_FAIL(ctx, NGSID_ERR_ARG, "null argument");
    *n_found = 0; *needed = 0;
    const int d = prm->max_dist, g = prm->seed_len;
    if (d < 0 || d > NGSID_UMI_MAX_DIST) NGSID_FAIL(ctx, NGSID_ERR_ARG, "ngsid_umi_params_t.max_dist %d outside 0 .. NGSID_UMI_MAX_DIST=%d", d, NGSID_UMI_MAX_DIST);
    if (g < 4 || g > 16) NGSID_FAIL(ctx, NGSID_ERR_ARG, "ngsid_umi_params_t.seed_len %d outside 4 .. 16", g);
    DevReads R;
    NGSID_TRY(ngsid_upload_reads(ctx, seqs, &R, false));
    const uint64_t N = R.n;
    if (R.maxlen > NGSID_UMI_MAX_LEN) NGSID_FAIL(ctx, NGSID_ERR_TOO_LONG, "a sequence of %u letters exceeds NGSID_UMI_MAX_LEN=%d", R.maxlen, NGSID_UMI_MAX_LEN);
    if (N * (uint64_t)(d + 1) >= 0x7fffffffull) NGSID_FAIL(ctx, NGSID_ERR_ARG, "%llu sequences x %d seeds: the index is limited to 2^31 - 1 entries", (unsigned long long)N, d + 1);
    NGSID_TRY(ngsid_alphabet_check(ctx, R, nullptr, "k_umi_check", "a sequence holds a letter outside upper-case ACGTN"));
    if (N < 2) return NGSID_OK;
    // ---- host side of the split: which sequences are seedable, the set ordered by length
    auto len = [&](uint64_t s) { return (uint32_t)(R.h_off[s + 1] - R.h_off[s]); };
    const uint32_t need = (uint32_t)((d + 1) * g);
    PinVec<uint32_t> ns, order(N), lstart(NGSID_UMI_MAX_LEN + 2, 0);
    for (uint64_t s = 0; s < N; ++s) { if (len(s) < need) ns.push_back((uint32_t)s); lstart[len(s) + 1] += 1; }
    for (int L = 0; L <= NGSID_UMI_MAX_LEN; ++L) lstart[L + 1] += lstart[L];
    { std::vector<uint32_t> at(lstart.begin(), lstart.end() - 1); for (uint64_t s = 0; s < N; ++s) order[at[len(s)]++] = (uint32_t)s; }
    const bool any_seedable = ns.size() < N;
    // ---- planes and index
    const uint64_t M = N * (uint64_t)(d + 1);
    HIPCHK(ctx, ctx->umi_pack.reserve(4 * N)); HIPCHK(ctx, ctx->umi_key.reserve(M)); HIPCHK(ctx, ctx->umi_val.reserve(M));
    HIPCHK(ctx, ctx->umi_skey.reserve(M)); HIPCHK(ctx, ctx->umi_sval.reserve(M));
    UmiPack* pack = (UmiPack*)ctx->umi_pack.p;
    { ProfScope ps_(ctx, "k_umi_keys");
      hipLaunchKernelGGL(k_umi_keys, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, ctx->stream, R.seq, R.off, (u64)N, d, g, pack, ctx->umi_key.p, ctx->umi_val.p); }
    HIPCHK(ctx, hipGetLastError());
    if (any_seedable) NGSID_TRY(umi_sort<uint32_t>(ctx, ctx->umi_key.p, ctx->umi_skey.p, ctx->umi_val.p, ctx->umi_sval.p, M, UMI_KEY_BITS, "k_umi_sort"));      // stable: sequences ascending within a key
    DevBuf<uint64_t> d_samp;
    const uint32_t S = (uint32_t)((M + 63) / 64);
    if (any_seedable) {
        HIPCHK(ctx, d_samp.alloc(S));
        ProfScope ps_(ctx, "k_umi_sort");
        hipLaunchKernelGGL(k_umi_sample, dim3((S + 255) / 256), dim3(256), 0, ctx->stream, ctx->umi_skey.p, S, d_samp.p);
        HIPCHK(ctx, hipGetLastError());
    }
    // ---- the found buffer and the counters
    const uint64_t F = std::min<uint64_t>(cap, 0x7fffffffull);
    if (F) { HIPCHK(ctx, ctx->umi_found.reserve(F)); HIPCHK(ctx, ctx->umi_dist.reserve(F)); }
    const size_t nctr = (size_t)UMI_STAT_STRIDE * (UMI_NSTAT + 1);
    DevBuf<unsigned long long> d_ctr; HIPCHK(ctx, d_ctr.alloc(nctr));
    HIPCHK(ctx, hipMemsetAsync(d_ctr.p, 0, nctr * sizeof(unsigned long long), ctx->stream));
    const int count = ctx->prof ? 1 : 0;
    const long long opt = ngsid_opt(ctx, "umi_chunk_seqs", 0), opt_tiles = ngsid_opt(ctx, "umi_max_tiles", 0);
    const int Q = (d + 1) * (2 * d + 1);
    // the tiles of a join chunk: what the tile list is allowed to hold (1 GiB) and what a launch holds, four tiles per workgroup; above max_tiles the queries are split
    const uint64_t launch_tiles = std::min<uint64_t>((uint64_t)1 << 28, 4 * ngsid_max_blocks(256));
    const uint64_t max_tiles = opt_tiles > 0 ? std::min<uint64_t>((uint64_t)opt_tiles, launch_tiles) : launch_tiles;
    // ---- join: queries 1 .. N - 1 in chunks (query 0 has no smaller index)
    if (any_seedable) {
        uint64_t rows = opt > 0 ? (uint64_t)opt : std::max<uint64_t>(1, ((uint64_t)8 << 20) / Q);
        for (uint64_t b0 = 1; b0 < N; ) {
            const uint64_t b1 = std::min(N, b0 + rows);
            const uint32_t nidx = (uint32_t)((b1 - b0) * Q);
            HIPCHK(ctx, ctx->umi_lo.reserve(nidx)); HIPCHK(ctx, ctx->umi_cnt.reserve(nidx)); HIPCHK(ctx, ctx->umi_tile.reserve(nidx)); HIPCHK(ctx, ctx->umi_tsum.reserve(nidx));
            size_t tb = 0;
            HIPCHK(ctx, hipcub::DeviceScan::InclusiveSum(nullptr, tb, ctx->umi_tile.p, ctx->umi_tsum.p, (int)nidx, ctx->stream));
            HIPCHK(ctx, ctx->umi_tmp.reserve(tb));
            uint64_t nt = 0;
            { ProfScope ps_(ctx, "k_umi_ranges");
              hipLaunchKernelGGL(k_umi_ranges, dim3((nidx + 255) / 256), dim3(256), 0, ctx->stream, pack, ctx->umi_skey.p, ctx->umi_sval.p, (uint32_t)M, d_samp.p, S, (u64)b0, nidx, d, g,
                                 ctx->umi_lo.p, ctx->umi_cnt.p, ctx->umi_tile.p);
              HIPCHK(ctx, hipGetLastError());
              HIPCHK(ctx, hipcub::DeviceScan::InclusiveSum(ctx->umi_tmp.p, tb, ctx->umi_tile.p, ctx->umi_tsum.p, (int)nidx, ctx->stream)); }
            NGSID_TRY(dev_get(ctx, &nt, ctx->umi_tsum.p + (nidx - 1), 1));
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
            if (nt > launch_tiles && b1 - b0 == 1) NGSID_FAIL(ctx, NGSID_ERR_ARG, "one sequence has %llu candidate tiles: beyond a launch", (unsigned long long)nt);
            if (nt > max_tiles && b1 - b0 > 1) { rows = (b1 - b0) / 2; continue; }      // the same queries in smaller chunks
            if (nt) {
                HIPCHK(ctx, ctx->umi_tidx.reserve(nt));
                ProfScope ps_(ctx, "k_umi_join");
                hipLaunchKernelGGL(k_umi_tiles, dim3((nidx + 255) / 256), dim3(256), 0, ctx->stream, ctx->umi_tsum.p, ctx->umi_cnt.p, nidx, ctx->umi_tidx.p);
                hipLaunchKernelGGL(k_umi_join, dim3((unsigned)((nt + 3) / 4)), dim3(256), 0, ctx->stream, pack, ctx->umi_sval.p, ctx->umi_tsum.p, ctx->umi_tidx.p, ctx->umi_lo.p, ctx->umi_cnt.p,
                                   (u64)b0, (u64)nt, d, g, ctx->umi_found.p, ctx->umi_dist.p, (u64)F, d_ctr.p, count);
            }
            HIPCHK(ctx, hipGetLastError());
            b0 = b1;
        }
    }
    // ---- short path: the sequences that are not seedable against the longer-indexed ones of a near length
    if (!ns.empty()) {
        DevBuf<uint32_t> d_ns, d_order, d_lstart;
        NGSID_TRY(dev_put(ctx, d_ns, ns.data(), ns.size())); NGSID_TRY(dev_put(ctx, d_order, order.data(), N)); NGSID_TRY(dev_put(ctx, d_lstart, lstart.data(), lstart.size()));
        uint32_t widest = 0;                                            // the largest range of a row
        for (int L = 0; L <= NGSID_UMI_MAX_LEN; ++L) widest = std::max(widest, lstart[std::min(L + d, NGSID_UMI_MAX_LEN) + 1] - lstart[std::max(L - d, 0)]);
        const unsigned ny = (unsigned)std::min<uint64_t>(std::max<uint64_t>(((uint64_t)widest + 255) / 256, 1), 64);
        const uint64_t rows = std::min<uint64_t>(opt > 0 ? (uint64_t)opt : (uint64_t)1 << 24, ngsid_max_blocks(256));
        for (uint64_t r0 = 0; r0 < ns.size(); r0 += rows) {
            ProfScope ps_(ctx, "k_umi_short");
            hipLaunchKernelGGL(k_umi_short, dim3((unsigned)std::min<uint64_t>(rows, ns.size() - r0), ny), dim3(256), 0, ctx->stream, pack, d_ns.p, d_order.p, d_lstart.p, (u64)r0, d,
                               ctx->umi_found.p, ctx->umi_dist.p, (u64)F, d_ctr.p, count);
            HIPCHK(ctx, hipGetLastError());
        }
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));                 // (the host vectors and device lists of this scope)
    }
    std::vector<unsigned long long> h_ctr(nctr, 0);
    NGSID_TRY(dev_get(ctx, h_ctr.data(), d_ctr.p, nctr));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    const uint64_t total = h_ctr[0];
    if (count) { uint64_t c = 0; for (int k = 1; k <= UMI_NSTAT; ++k) c += h_ctr[(size_t)UMI_STAT_STRIDE * k]; ctx->prof_acc["umi_candidates"].second += c; }
    *needed = total;
    if (total > cap) NGSID_FAIL(ctx, NGSID_ERR_CAPACITY, "%llu UMI pairs, room for %llu", (unsigned long long)total, (unsigned long long)cap);
    if (total > F) NGSID_FAIL(ctx, NGSID_ERR_ARG, "%llu UMI pairs: a call is limited to 2^31 - 1", (unsigned long long)total);
    if (total == 0) return NGSID_OK;
    // ---- ascending (i, j): the keys are distinct
    HIPCHK(ctx, ctx->umi_sfound.reserve(total)); HIPCHK(ctx, ctx->umi_sdist.reserve(total));
    NGSID_TRY(umi_sort<uint8_t>(ctx, ctx->umi_found.p, ctx->umi_sfound.p, ctx->umi_dist.p, ctx->umi_sdist.p, total, 64, "k_umi_order"));
    PinVec<uint64_t> keys(total);
    NGSID_TRY(dev_get(ctx, keys.data(), ctx->umi_sfound.p, total)); NGSID_TRY(dev_get(ctx, dist, ctx->umi_sdist.p, total));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (uint64_t k = 0; k < total; ++k) ngsid_pair_unkey(keys[k], pair_i + k, pair_j + k);
    *n_found = total;
    return NGSID_OK;
}

}  // namespace

extern "C" int32_t ngsid_umi_pairs(ngsid_ctx* ctx, const ngsid_reads_t* seqs, const ngsid_umi_params_t* prm, uint32_t* pair_i, uint32_t* pair_j, uint8_t* dist,
                                   uint64_t cap, uint64_t* n_found, uint64_t* needed)
{
    ApiClock api_clock_(ctx, "umi_pairs");
    if (!ctx) return NGSID_ERR_ARG;
    return umi_pairs_run(ctx, seqs, prm, pair_i, pair_j, dist, cap, n_found, needed);
}

extern "C" int32_t ngsid_umi_centroids(const uint32_t* pair_i, const uint32_t* pair_j, uint64_t n_pairs, const uint32_t* order, uint32_t n, int32_t* bin_of, uint32_t* centroid, uint32_t* n_bins)
{
    if (!n_bins || (n && (!order || !bin_of || !centroid)) || (n_pairs && (!pair_i || !pair_j))) return NGSID_ERR_ARG;
    *n_bins = 0;
    if (n > 0x7fffffffu) return NGSID_ERR_ARG;
    try {
        std::vector<uint8_t> seen(n, 0);
        for (uint32_t k = 0; k < n; ++k) { if (order[k] >= n || seen[order[k]]) return NGSID_ERR_ARG; seen[order[k]] = 1; }
        // CSR adjacency, both directions
        std::vector<uint64_t> adj_off((size_t)n + 1, 0);
        for (uint64_t p = 0; p < n_pairs; ++p) {
            if (pair_i[p] >= n || pair_j[p] >= n || pair_i[p] == pair_j[p]) return NGSID_ERR_ARG;
            adj_off[(size_t)pair_i[p] + 1] += 1; adj_off[(size_t)pair_j[p] + 1] += 1;
        }
        for (uint32_t x = 0; x < n; ++x) adj_off[(size_t)x + 1] += adj_off[x];
        std::vector<uint32_t> adj(2 * n_pairs);
        { std::vector<uint64_t> at(adj_off.begin(), adj_off.end() - 1);
          for (uint64_t p = 0; p < n_pairs; ++p) { adj[at[pair_i[p]]++] = pair_j[p]; adj[at[pair_j[p]]++] = pair_i[p]; } }
        // one pass in `order`: founded[y] = the bin y founded, or -1
        std::vector<int32_t> founded(n, -1);
        uint32_t nb = 0;
        for (uint32_t k = 0; k < n; ++k) {
            const uint32_t x = order[k];
            int32_t best = -1;
            for (uint64_t e = adj_off[x]; e < adj_off[(size_t)x + 1]; ++e) { const int32_t f = founded[adj[e]]; if (f >= 0 && (best < 0 || f < best)) best = f; }
            if (best < 0) { best = (int32_t)nb; founded[x] = best; centroid[nb++] = x; }
            bin_of[x] = best;
        }
        *n_bins = nb;
    } catch (const std::bad_alloc&) { return NGSID_ERR_ARG; }
    return NGSID_OK;
}
