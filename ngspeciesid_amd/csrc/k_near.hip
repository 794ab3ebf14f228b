// k_near.hip - ngsid_ed_within_batch / ngsid_near_pairs and their wide twins (include/ngsid_near.h): the unit-cost edit distance of pairs that are at most max_dist edits
// apart, on both strands, for listed pairs and for all pairs of a set.  max_dist <= 31 with the plain calls, <= 255 with the wide ones.
//
// One pair per lane, W band words per lane, W = 1, 2, 4 or 8, the smallest that holds max_dist: the diagonal-band form of Myers' bit-vector recurrence (Hyyro 2003) on a
// band of B = 64 W bits, H = B / 2 - 1 = 32 W - 1.  In column c (1-based) of the DP matrix of a pattern (rows) against a text (columns), bit r of the band is row
// c - H + r (word j holds bits 64 j .. 64 j + 63), so a diagonal keeps its bit from column to column and the cell (m, n) sits at bit H - (n - m).  VP / VN hold the
// vertical deltas of the column before, already aligned to the rows of the column that is computed: the band slides one row per column by the one shift D0 >> 1, which
// takes its top bit from the next word.  Row c + H + 1 was outside the band one column earlier; its delta is taken as +1 (the top bit of VP's top word), which can only
// raise a value.  Rows <= 0 are virtual rows that match nothing and hold D[i][c] = c (VP = VN = 0 there: VP starts as ones from bit H up), rows behind the pattern's end
// match nothing.  The sum (Eq & VP) + VP carries from word to word.  Every band value is the cost of a real alignment, so it is >= the full DP's, and equal to it where
// that is <= H: a path of cost <= H stays within H diagonals of the main one.  That is why a band of W words is exact up to 32 W - 1 edits (31, 63, 127, 255).
// The value on the diagonal of (m, n) is tracked from column 0 on (start max(m - n, 0), + 1 wherever D0 has a zero there).  Its bit lies in word (H - (n - m)) >> 6,
// which differs from lane to lane: the word is picked by a compare / select chain over the W words, never by indexing the register array (that would send the band to
// scratch); at W = 1 the chain is empty.  Values never decrease along a diagonal, so a lane leaves the loop as soon as the tracked value exceeds its bound: pairs with
// |n - m| above it never enter, unrelated pairs leave after a few dozen columns, a wave stops when its last lane has.  The reverse strand runs after the forward one with
// the bound forward - 1 (a tie goes to forward), not at all behind a forward 0.
//
// No LDS and no traceback.  k_near_pack turns a sequence into bit planes of its letters' codes (A C G T N = 0 .. 4, 7 outside the sequence: equals nothing), one layout
// per role.  Pattern planes: three planes, base p at bit p + 255, padded once for the widest band, so that the window of column c + 1 of a W-word band starts at bit
// c + 32 (8 - W), a whole number of words in, and one layout serves every W.  Text planes: three planes TEXT (base p at bit p) and three TEXT_RC (the complement of base
// len - 1 - p at bit p: rc(b) is never materialised).  The three planes of a kind are interleaved word by word (word w of plane k at 3 w + k), so what a lane loads
// for a block of 32 columns is contiguous.  A call packs only what it reads.  A lane keeps 2 W + 1 pattern words per plane in registers, slides them by one word per
// 32 columns and loads the word that enters, and the next text word, one block ahead.  Per column the windows are v_alignbit_b32 of two neighbouring words: unlike a
// 64-bit shift it takes any two registers, so a word that is the high half of one window and the low half of the next is not copied into a register pair of its own
// (W = 8, before the planes were interleaved: 151 instead of 241 VGPRs).  The text letter is three 0 / -1 masks, and Eq = ~((W0 ^ T0) | (W1 ^ T1) | (W2 ^ T2)): N by the planes, not by a branch.
// W = 1 has a column loop of its own inside near_band_ed (the same planes, records and kernels): with the general loop k_near_tiles<1> and k_near_within<1> measured
// 2 - 3 % slower than with it.  tests/variants_band_model.py runs both loops on Python ints, word for word, for every W.
//
// k_near_within<W>: lane = listed pair (pattern = query, text = target).
// k_near_tiles<W>: the set sorted by length on the host; wave = tile = sequence x (sorted position) against 64 of the sequences behind it; the tiles of x end at hi[x],
//   the last sequence at most max_dist bases longer: the length bound removes whole tiles, and the lanes of a wave see lengths within max_dist of each other.  The text is
//   x, the shorter one, the same for every lane: its words and masks are wave-uniform, and every lane has the same number of columns.  A lane that finds a pair appends
//   (min, max of the caller's indices | a 16-bit record: distance | strand << 15) through one counter; the host sorts what came back.
#include "ngsid_host.h"
#include "../../include/ngsid_near.h"
#include <numeric>

typedef uint64_t u64;

#define NEAR_WMAX 8                     // the widest band in words: the pattern planes carry 32 * NEAR_WMAX - 1 pad bits
static_assert(NGSID_NEAR_MAX_DIST == 32 * 1 - 1, "the band of near_band_ed<1> holds 31 edits");
static_assert(NGSID_NEAR_WIDE_MAX_DIST == 32 * NEAR_WMAX - 1, "the widest band of near_band_ed holds 32 W - 1 edits");

namespace {

#define NEAR_PATTERN 0                  // the two kinds of planes near_pack writes
#define NEAR_TEXT 1

// words per pattern plane of a sequence of len bases: its bits, the eight pad words in front, and what a lane reads beyond the window's first word for a text up to
// 32 W - 1 bases longer: 2 W words of the window and the word loaded one block ahead (the farthest read is word ((len + 31) >> 5) + 2 W + 8, see near_band_ed)
__host__ __device__ __forceinline__ int near_nwp(int len) { return ((len + 31) >> 5) + 3 * NEAR_WMAX + 2; }
// words per text plane: its bits and the word loaded one block ahead (the farthest read is word ((len - 1) >> 5) + 1 = (len + 31) >> 5; a text of no bases is not read)
__host__ __device__ __forceinline__ int near_nwt(int len) { return ((len + 31) >> 5) + 1; }

// word w of the three planes at base (plane k at base[3 w + k]): bit t holds the code of base p = 32 w + t - shift of seq (L bases), with rc the complement of base L - 1 - p
__device__ __forceinline__ void near_pack_word(const uint8_t* __restrict__ seq, int L, int w, int shift, bool rc, uint32_t* __restrict__ base)
{
    uint32_t b0 = 0, b1 = 0, b2 = 0;
    for (int t = 0; t < 32; ++t) {
        const int p = 32 * w + t - shift;
        int c = 7;
        if (p >= 0 && p < L) {
            c = (int)ngsid_base_code(seq[rc ? L - 1 - p : p]);
            if (rc && c < 4) c = 3 - c;
        }
        b0 |= (uint32_t)(c & 1) << t; b1 |= (uint32_t)((c >> 1) & 1) << t; b2 |= (uint32_t)((c >> 2) & 1) << t;
    }
    base[3 * w] = b0; base[3 * w + 1] = b1; base[3 * w + 2] = b2;
}

// planes of sequence s, nw words each, the three planes of a kind interleaved word by word.  NEAR_PATTERN: woff[s] * 3 words in.  NEAR_TEXT: woff[s] * 6 words in, TEXT
// first, TEXT_RC 3 * nw words behind it
__global__ __launch_bounds__(64)
void k_near_pack(const uint8_t* __restrict__ seq, const uint64_t* __restrict__ off, const uint64_t* __restrict__ woff, u64 s0, int kind, uint32_t* __restrict__ planes)
{
    const u64 s = s0 + blockIdx.x;
    const u64 a = off[s];
    const int L = (int)(off[s + 1] - a);
    if (kind == NEAR_PATTERN) {
        const int nw = near_nwp(L);
        for (int w = threadIdx.x; w < nw; w += 64) near_pack_word(seq + a, L, w, 32 * NEAR_WMAX - 1, false, planes + woff[s] * 3);
    } else {
        const int nw = near_nwt(L);
        uint32_t* base = planes + woff[s] * 6;
        for (int w = threadIdx.x; w < nw; w += 64) { near_pack_word(seq + a, L, w, 0, false, base); near_pack_word(seq + a, L, w, 0, true, base + (size_t)3 * nw); }
    }
}

// bits s .. s + 31 of hi:lo, s = 0 .. 31: as one v_lshrrev_b64 of the register pair (near_funnel), as one v_alignbit_b32 of any two registers (near_align)
__device__ __forceinline__ uint32_t near_funnel(uint32_t hi, uint32_t lo, int s) { return (uint32_t)((((u64)hi << 32) | lo) >> s); }
__device__ __forceinline__ uint32_t near_align(uint32_t hi, uint32_t lo, int s) { return __builtin_amdgcn_alignbit(hi, lo, (uint32_t)s); }

// pat: the pattern planes of a sequence of m bases (word i of plane k at pat[3 i + k]), txt: the TEXT or the TEXT_RC planes of one of n bases -> their edit distance if it is
// <= K <= 32 W - 1, else -1.  Reads pattern words up to (8 - W) + ((n - 1) >> 5) + 2 W + 1 <= ((m + 31) >> 5) + 2 W + 8 < near_nwp(m) (n <= m + 32 W - 1 behind
// the length test) and text words up to ((n - 1) >> 5) + 1 < near_nwt(n); W = 1 one word less of each.  Every array is indexed by unrolled constants only: the band
// lives in registers.
template <int W>
__device__ __forceinline__ int near_band_ed(const uint32_t* __restrict__ pat, const uint32_t* __restrict__ txt, int m, int n, int K)
{
    constexpr int H = 32 * W - 1, NA = 2 * W + 1;
    const int d = n - m;
    int val = d < 0 ? -d : 0;
    if (val > K || d > K) return -1;
    if (n == 0) return val;
    if constexpr (W == 1) {
        // one word: the same recurrence without the carry, the shift across words and the select chain.  The three pattern words and the text word of a block are
        // loaded at its start, nothing ahead: most pairs are dead within two blocks.  The windows are 64-bit shifts of register pairs; with three words per plane
        // there is nothing for v_alignbit_b32 to save.  On the same planes the loop below, instantiated for W = 1, ran 2 % (k_near_tiles) and 3 % (k_near_within) slower
        const int sb = H - d;
        u64 VP = ~0ull << H, VN = 0;
        pat += 3 * (NEAR_WMAX - 1);
        for (int c0 = 0; c0 < n; c0 += 32) {
            const int w = c0 >> 5;
            const uint32_t a0 = pat[3 * w], a1 = pat[3 * w + 3], a2 = pat[3 * w + 6];
            const uint32_t b0 = pat[3 * w + 1], b1 = pat[3 * w + 4], b2 = pat[3 * w + 7];
            const uint32_t c_0 = pat[3 * w + 2], c_1 = pat[3 * w + 5], c_2 = pat[3 * w + 8];
            const uint32_t t0 = txt[3 * w], t1 = txt[3 * w + 1], t2 = txt[3 * w + 2];
            const int ce = min(32, n - c0);
            for (int s = 0; s < ce; ++s) {
                const u64 W0 = ((u64)near_funnel(a2, a1, s) << 32) | near_funnel(a1, a0, s);
                const u64 W1 = ((u64)near_funnel(b2, b1, s) << 32) | near_funnel(b1, b0, s);
                const u64 W2 = ((u64)near_funnel(c_2, c_1, s) << 32) | near_funnel(c_1, c_0, s);
                const u64 T0 = (u64)0 - ((t0 >> s) & 1u), T1 = (u64)0 - ((t1 >> s) & 1u), T2 = (u64)0 - ((t2 >> s) & 1u);
                const u64 Eq = ~((W0 ^ T0) | (W1 ^ T1) | (W2 ^ T2));
                const u64 D0 = (((Eq & VP) + VP) ^ VP) | Eq | VN;
                const u64 HP = VN | ~(D0 | VP);
                const u64 HN = D0 & VP;
                const u64 D0s = D0 >> 1;
                VP = HN | ~(D0s | HP) | (1ull << 63);
                VN = D0s & HP;
                val += 1 - (int)((D0 >> sb) & 1u);
                if (val > K) return -1;
            }
        }
        return val;
    }
    const int sb = H - d, sw = sb >> 6, sbit = sb & 63;
    u64 VP[W], VN[W];
#pragma unroll
    for (int j = 0; j < W; ++j) { VP[j] = j < (H >> 6) ? 0ull : j == (H >> 6) ? ~0ull << (H & 63) : ~0ull; VN[j] = 0; }
    pat += 3 * (NEAR_WMAX - W);
    uint32_t a[3][NA], t[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int i = 0; i < NA; ++i) a[k][i] = pat[3 * i + k];
        t[k] = txt[k];
    }
    for (int c0 = 0; c0 < n; c0 += 32) {
        const int w = c0 >> 5;
        uint32_t nx[3], tn[3];                                       // the words of the next block, loaded one block ahead
#pragma unroll
        for (int k = 0; k < 3; ++k) { nx[k] = pat[3 * (w + NA) + k]; tn[k] = txt[3 * (w + 1) + k]; }
        const int ce = min(32, n - c0);
        for (int s = 0; s < ce; ++s) {
            const uint32_t T0 = 0u - ((t[0] >> s) & 1u), T1 = 0u - ((t[1] >> s) & 1u), T2 = 0u - ((t[2] >> s) & 1u);
            u64 D0[W];
            unsigned long long cy = 0;
#pragma unroll
            for (int j = 0; j < W; ++j) {
                const uint32_t nlo = (near_align(a[0][2 * j + 1], a[0][2 * j], s) ^ T0) | (near_align(a[1][2 * j + 1], a[1][2 * j], s) ^ T1) | (near_align(a[2][2 * j + 1], a[2][2 * j], s) ^ T2);
                const uint32_t nhi = (near_align(a[0][2 * j + 2], a[0][2 * j + 1], s) ^ T0) | (near_align(a[1][2 * j + 2], a[1][2 * j + 1], s) ^ T1) | (near_align(a[2][2 * j + 2], a[2][2 * j + 1], s) ^ T2);
                const u64 Eq = ~(((u64)nhi << 32) | nlo);
                const u64 S = __builtin_addcll(Eq & VP[j], VP[j], cy, &cy);      // the carry runs from word j to word j + 1
                D0[j] = (S ^ VP[j]) | Eq | VN[j];
            }
#pragma unroll
            for (int j = 0; j < W; ++j) {
                const u64 HP = VN[j] | ~(D0[j] | VP[j]);
                const u64 HN = D0[j] & VP[j];
                const u64 D0s = j + 1 < W ? (D0[j] >> 1) | (D0[j + 1] << 63) : D0[j] >> 1;
                VP[j] = HN | ~(D0s | HP) | (j == W - 1 ? 1ull << 63 : 0ull);
                VN[j] = D0s & HP;
            }
            u64 tr = D0[0];
#pragma unroll
            for (int j = 1; j < W; ++j) tr = sw == j ? D0[j] : tr;
            val += 1 - (int)((tr >> sbit) & 1u);
            if (val > K) return -1;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
#pragma unroll
            for (int i = 0; i + 1 < NA; ++i) a[k][i] = a[k][i + 1];
            a[k][NA - 1] = nx[k]; t[k] = tn[k];
        }
    }
    return val;
}

// pat: the pattern planes, txt6: the six text planes.  Forward, then the reverse strand below the forward result -> the distance or -1; *strand = 1 iff the reverse
// strand is strictly closer
template <int W>
__device__ __forceinline__ int near_both(const uint32_t* __restrict__ pat, const uint32_t* __restrict__ txt6, int nwt, int m, int n, int K, bool both, int* strand)
{
    int best = near_band_ed<W>(pat, txt6, m, n, K);
    *strand = 0;
    if (both && best != 0) {
        const int r = near_band_ed<W>(pat, txt6 + (size_t)3 * nwt, m, n, best < 0 ? K : best - 1);
        if (r >= 0) { best = r; *strand = 1; }
    }
    return best;
}

// qwoff / qpl: the pattern planes of the queries, twoff / tpl: the text planes of the targets
template <int W>
__global__ __launch_bounds__(256)
void k_near_within(const uint64_t* __restrict__ qoff, const uint64_t* __restrict__ qwoff, const uint32_t* __restrict__ qpl, const uint64_t* __restrict__ toff, const uint64_t* __restrict__ twoff,
                   const uint32_t* __restrict__ tpl, const uint32_t* __restrict__ qidx, const uint32_t* __restrict__ tidx, u64 p0, u64 p1, int K, int both,
                   int32_t* __restrict__ dist, uint8_t* __restrict__ strand)
{
    const u64 p = p0 + (u64)blockIdx.x * 256 + threadIdx.x;
    if (p >= p1) return;
    const uint32_t q = qidx[p], t = tidx[p];
    const int m = (int)(qoff[q + 1] - qoff[q]), n = (int)(toff[t + 1] - toff[t]);
    int st = 0;
    const int best = near_both<W>(qpl + qwoff[q] * 3, tpl + twoff[t] * 6, near_nwt(n), m, n, K, both != 0, &st);
    dist[p] = best;
    strand[p] = (uint8_t)st;
}

// rows x = xa .. xa + nrows - 1 (sorted positions); tile T of the launch belongs to the row r with toff[r] <= T < toff[r + 1] and covers y = x + 1 + 64 (T - toff[r]) + lane.
// pwoff / ppl: the pattern planes of the set, twoff / tpl: its text planes; a found pair's record is distance | strand << 15
template <int W>
__global__ __launch_bounds__(256)
void k_near_tiles(const uint64_t* __restrict__ off, const uint64_t* __restrict__ pwoff, const uint32_t* __restrict__ ppl, const uint64_t* __restrict__ twoff, const uint32_t* __restrict__ tpl,
                  const uint32_t* __restrict__ order, const uint32_t* __restrict__ hi, const uint64_t* __restrict__ toff, uint32_t xa, uint32_t nrows, u64 ntiles, int K, int both,
                  u64* __restrict__ key, uint16_t* __restrict__ ds, u64 limit, unsigned long long* counter)
{
    const int lane = threadIdx.x & 63;
    const u64 Tl = (u64)blockIdx.x * 4 + (threadIdx.x >> 6);
    const u64 T = ((u64)(uint32_t)__builtin_amdgcn_readfirstlane((int)(Tl >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)Tl);
    if (T >= ntiles) return;
    uint32_t lo = 0, up = nrows;                                   // the last r with toff[r] <= T
    while (up - lo > 1) { const uint32_t mid = lo + (up - lo) / 2; if (toff[mid] <= T) lo = mid; else up = mid; }
    const uint32_t x = xa + lo;
    const u64 y64 = (u64)x + 1 + (T - toff[lo]) * 64 + lane;
    if (y64 > hi[x]) return;
    const uint32_t y = (uint32_t)y64, ox = order[x], oy = order[y];
    const int n = (int)(off[ox + 1] - off[ox]), m = (int)(off[oy + 1] - off[oy]);
    int st = 0;
    const int best = near_both<W>(ppl + pwoff[oy] * 3, tpl + twoff[ox] * 6, near_nwt(n), m, n, K, both != 0, &st);
    if (best < 0) return;
    unsigned long long slot;
    if (ngsid_found_slot(counter, limit, &slot)) { key[slot] = ngsid_pair_key(ox, oy); ds[slot] = (uint16_t)(best | (st << 15)); }
}

// the planes of one kind (NEAR_PATTERN or NEAR_TEXT) of every sequence of R in `buf` (grow-only), the word offsets on the device
int32_t near_pack(ngsid_ctx* ctx, const DevReads& R, int kind, DevBuf<uint32_t>& buf, DevBuf<uint64_t>& d_woff)
{
    PinVec<uint64_t> woff(R.n + 1);
    woff[0] = 0;
    for (uint64_t s = 0; s < R.n; ++s) { const int len = (int)(R.h_off[s + 1] - R.h_off[s]); woff[s + 1] = woff[s] + (uint64_t)(kind == NEAR_PATTERN ? near_nwp(len) : near_nwt(len)); }
    HIPCHK(ctx, buf.reserve(woff[R.n] * (kind == NEAR_PATTERN ? 3 : 6)));
    NGSID_TRY(dev_put(ctx, d_woff, woff.data(), R.n + 1));
    ProfScope ps_(ctx, "k_near_pack");
    for (uint64_t s0 = 0; s0 < R.n; s0 += ngsid_max_blocks(64)) {
        hipLaunchKernelGGL(k_near_pack, dim3((unsigned)std::min<uint64_t>(R.n - s0, ngsid_max_blocks(64))), dim3(64), 0, ctx->stream, R.seq, R.off, d_woff.p, (u64)s0, kind, buf.p);
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));                  // (woff is a host vector of this scope)
    return NGSID_OK;
}

// the checks the entry points share: max_dist (limit = NGSID_NEAR_MAX_DIST or NGSID_NEAR_WIDE_MAX_DIST), the length bound, the alphabet
int32_t near_check(ngsid_ctx* ctx, int32_t max_dist, int32_t limit, const DevReads* A, const DevReads* B)
{
    if (max_dist < 0 || max_dist > limit) NGSID_FAIL(ctx, NGSID_ERR_ARG, "max_dist %d outside 0 .. %s=%d", max_dist, limit == NGSID_NEAR_MAX_DIST ? "NGSID_NEAR_MAX_DIST" : "NGSID_NEAR_WIDE_MAX_DIST", limit);
    const uint32_t maxlen = std::max(A->maxlen, B ? B->maxlen : 0u);
    if (maxlen > NGSID_MAX_CONSENSUS_LEN) NGSID_FAIL(ctx, NGSID_ERR_TOO_LONG, "a sequence of %u bases exceeds NGSID_MAX_CONSENSUS_LEN=%d", maxlen, NGSID_MAX_CONSENSUS_LEN);
    if (A->n >= 0x100000000ull || (B && B->n >= 0x100000000ull)) NGSID_FAIL(ctx, NGSID_ERR_ARG, "a set is limited to 2^32 - 1 sequences");
    return ngsid_alphabet_check(ctx, *A, B, "k_near_check", "a sequence holds a base outside upper-case ACGTN");
}

// the band words of a call: the smallest instance that holds max_dist
int near_width(int32_t max_dist) { return max_dist <= NGSID_NEAR_MAX_DIST ? 1 : max_dist <= 63 ? 2 : max_dist <= 127 ? 4 : 8; }

// launches the instance KERN<W> of k_near_within or k_near_tiles, W = near_width(max_dist), under the profiling line KERN (W = 1) or KERN_wide
#define NEAR_LAUNCH(KERN, W, GRID, ...) do { \
        ProfScope ps_(ctx, (W) == 1 ? #KERN : #KERN "_wide"); \
        if ((W) == 1) hipLaunchKernelGGL((KERN<1>), GRID, dim3(256), 0, ctx->stream, __VA_ARGS__); \
        else if ((W) == 2) hipLaunchKernelGGL((KERN<2>), GRID, dim3(256), 0, ctx->stream, __VA_ARGS__); \
        else if ((W) == 4) hipLaunchKernelGGL((KERN<4>), GRID, dim3(256), 0, ctx->stream, __VA_ARGS__); \
        else hipLaunchKernelGGL((KERN<8>), GRID, dim3(256), 0, ctx->stream, __VA_ARGS__); \
    } while (0)

// ngsid_ed_within_batch (limit = NGSID_NEAR_MAX_DIST) and ngsid_ed_within_wide_batch (limit = NGSID_NEAR_WIDE_MAX_DIST) behind their argument checks
int32_t near_within_run(ngsid_ctx* ctx, const ngsid_reads_t* queries, const ngsid_reads_t* targets, const uint32_t* q_idx, const uint32_t* t_idx, uint64_t n_pairs,
                        int32_t max_dist, int32_t limit, uint32_t flags, int32_t* dist, uint8_t* strand)
{
    if (n_pairs && !dist) NGSID_FAIL(ctx, NGSID_ERR_ARG, "null output");
    PairBatch B;
    NGSID_TRY(ngsid_pair_batch(ctx, queries, targets, q_idx, t_idx, n_pairs, B));
    NGSID_TRY(near_check(ctx, max_dist, limit, &B.Q, &B.T));
    if (n_pairs == 0) return NGSID_OK;
    const int W = near_width(max_dist);
    DevBuf<uint64_t> d_qw, d_tw; DevBuf<int32_t> d_dist; DevBuf<uint8_t> d_strand;
    NGSID_TRY(near_pack(ctx, B.Q, NEAR_PATTERN, ctx->near_pat, d_qw));
    NGSID_TRY(near_pack(ctx, B.T, NEAR_TEXT, ctx->near_txt, d_tw));
    HIPCHK(ctx, d_dist.alloc(n_pairs)); HIPCHK(ctx, d_strand.alloc(n_pairs));
    const long long opt = ngsid_opt(ctx, "near_chunk_pairs", 0);
    const uint64_t chunk = opt > 0 ? (uint64_t)opt : (uint64_t)1 << 30;
    for (uint64_t p0 = 0; p0 < n_pairs; p0 += chunk) {
        const uint64_t p1 = std::min(n_pairs, p0 + chunk);
        NEAR_LAUNCH(k_near_within, W, dim3(NGSID_GRID(ctx, (p1 - p0 + 255) / 256, 256, "k_near_within")), B.Q.off, d_qw.p, ctx->near_pat.p, B.T.off, d_tw.p, ctx->near_txt.p,
                    B.dq.p, B.dt.p, (u64)p0, (u64)p1, (int)max_dist, (int)(flags & NGSID_NEAR_BOTH_STRANDS), d_dist.p, d_strand.p);
        HIPCHK(ctx, hipGetLastError());
    }
    NGSID_TRY(dev_get(ctx, dist, d_dist.p, n_pairs));
    if (strand) NGSID_TRY(dev_get(ctx, strand, d_strand.p, n_pairs));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return NGSID_OK;
}

// ngsid_near_pairs (dist_limit = NGSID_NEAR_MAX_DIST) and ngsid_near_pairs_wide (dist_limit = NGSID_NEAR_WIDE_MAX_DIST) behind the context check
int32_t near_pairs_run(ngsid_ctx* ctx, const ngsid_reads_t* seqs, int32_t max_dist, int32_t dist_limit, uint32_t flags, uint32_t* pair_i, uint32_t* pair_j, uint8_t* dist, uint8_t* strand,
                       uint64_t cap, uint64_t* n_found, uint64_t* needed)
{
    if (!seqs || !n_found || !needed || (cap && (!pair_i || !pair_j || !dist || !strand))) NGSID_FAIL(ctx, NGSID_ERR_ARG, "null argument");
    *n_found = 0; *needed = 0;
    DevReads R;
    NGSID_TRY(ngsid_upload_reads(ctx, seqs, &R, false));
    NGSID_TRY(near_check(ctx, max_dist, dist_limit, &R, nullptr));
    const uint64_t N = R.n;
    if (N < 2) return NGSID_OK;
    const int W = near_width(max_dist);
    // ---- sorted by (length, index); hi[x] = the last sorted position whose sequence is at most max_dist bases longer than x's; 64 candidates per tile
    auto len = [&](uint32_t s) { return (uint32_t)(R.h_off[(size_t)s + 1] - R.h_off[s]); };
    PinVec<uint32_t> order(N), hi(N);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return len(a) < len(b); });
    std::vector<uint64_t> tiles(N + 1, 0);
    for (uint64_t x = 0, y = 0; x < N; ++x) {
        if (y < x) y = x;
        while (y + 1 < N && len(order[y + 1]) - len(order[x]) <= (uint32_t)max_dist) ++y;
        hi[x] = (uint32_t)y;
        tiles[x + 1] = tiles[x] + (y - x + 63) / 64;
    }
    DevBuf<uint64_t> d_pwoff, d_twoff, d_toff; DevBuf<uint32_t> d_order, d_hi; DevBuf<unsigned long long> d_ctr;
    NGSID_TRY(near_pack(ctx, R, NEAR_PATTERN, ctx->near_pat, d_pwoff));
    NGSID_TRY(near_pack(ctx, R, NEAR_TEXT, ctx->near_txt, d_twoff));
    NGSID_TRY(dev_put(ctx, d_order, order.data(), N)); NGSID_TRY(dev_put(ctx, d_hi, hi.data(), N));
    HIPCHK(ctx, d_ctr.alloc(1));
    // ---- the found buffer: cap entries, or what a share of the free device memory holds; rows in chunks
    const uint64_t F = std::min<uint64_t>(cap, ngsid_mem_share(4, (size_t)64 << 20, (size_t)16 << 30, (size_t)4 << 30, ctx->near_key.abytes + ctx->near_ds.abytes) / (8 + sizeof(uint16_t)));
    if (F) { HIPCHK(ctx, ctx->near_key.reserve(F)); HIPCHK(ctx, ctx->near_ds.reserve(F)); }
    const long long opt = ngsid_opt(ctx, "near_chunk_seqs", 0), opt_tiles = ngsid_opt(ctx, "near_max_tiles", 0);
    const uint64_t launch_tiles = 4 * ngsid_max_blocks(256);          // what a launch holds: four tiles per workgroup
    const uint64_t max_tiles = opt_tiles > 0 ? std::min<uint64_t>((uint64_t)opt_tiles, launch_tiles) : launch_tiles;      // above: the rows are split
    std::vector<uint64_t> keys; std::vector<uint16_t> dss;
    PinVec<uint64_t> h_toff;
    const auto launch = [&](uint64_t xa, uint64_t& xb, uint64_t limit, bool& launched) -> int32_t {
        while (xb - xa > 1 && tiles[xb] - tiles[xa] > max_tiles) xb = xa + (xb - xa) / 2;
        const uint64_t nt = tiles[xb] - tiles[xa];
        if (nt == 0) { launched = false; return NGSID_OK; }
        if (nt > launch_tiles) NGSID_FAIL(ctx, NGSID_ERR_ARG, "one sequence has %llu candidate tiles: beyond a launch", (unsigned long long)nt);
        h_toff.resize(xb - xa + 1);
        for (uint64_t r = 0; r <= xb - xa; ++r) h_toff[r] = tiles[xa + r] - tiles[xa];
        NGSID_TRY(dev_put(ctx, d_toff, h_toff.data(), xb - xa + 1));
        HIPCHK(ctx, hipMemsetAsync(d_ctr.p, 0, sizeof(unsigned long long), ctx->stream));
        NEAR_LAUNCH(k_near_tiles, W, dim3((unsigned)((nt + 3) / 4)), R.off, d_pwoff.p, ctx->near_pat.p, d_twoff.p, ctx->near_txt.p, d_order.p, d_hi.p, d_toff.p, (uint32_t)xa, (uint32_t)(xb - xa), (u64)nt,
                    (int)max_dist, (int)(flags & NGSID_NEAR_BOTH_STRANDS), ctx->near_key.p, ctx->near_ds.p, (u64)limit, d_ctr.p);
        return NGSID_OK;
    };
    const auto fetch = [&](uint64_t, size_t c) -> int32_t {
        const size_t at = keys.size();
        keys.resize(at + c); dss.resize(at + c);
        NGSID_TRY(dev_get(ctx, keys.data() + at, ctx->near_key.p, c));
        return dev_get(ctx, dss.data() + at, ctx->near_ds.p, c);
    };
    uint64_t total = 0;
    NGSID_TRY(ngsid_found_loop(ctx, N, opt > 0 ? (uint64_t)opt : N, F, cap, d_ctr.p, launch, fetch, "sequence", "near neighbours", &total));
    *needed = total;
    if (total > cap) NGSID_FAIL(ctx, NGSID_ERR_CAPACITY, "%llu near pairs, room for %llu", (unsigned long long)total, (unsigned long long)cap);
    // ---- ascending (i, j): the keys are distinct
    std::vector<uint64_t> perm(total);
    std::iota(perm.begin(), perm.end(), (uint64_t)0);
    std::sort(perm.begin(), perm.end(), [&](uint64_t a, uint64_t b) { return keys[a] < keys[b]; });
    for (uint64_t k = 0; k < total; ++k) {
        const uint16_t v = dss[perm[k]];
        ngsid_pair_unkey(keys[perm[k]], pair_i + k, pair_j + k); dist[k] = (uint8_t)(v & 0x7fffu); strand[k] = (uint8_t)(v >> 15);
    }
    *n_found = total;
    return NGSID_OK;
}

}  // namespace

extern "C" int32_t ngsid_ed_within_batch(ngsid_ctx* ctx, const ngsid_reads_t* queries, const ngsid_reads_t* targets, const uint32_t* q_idx, const uint32_t* t_idx, uint64_t n_pairs,
                                         int32_t max_dist, uint32_t flags, int32_t* dist, uint8_t* strand)
{
    ApiClock api_clock_(ctx, "ed_within_batch");
    if (!ctx) return NGSID_ERR_ARG;
    return near_within_run(ctx, queries, targets, q_idx, t_idx, n_pairs, max_dist, NGSID_NEAR_MAX_DIST, flags, dist, strand);
}

extern "C" int32_t ngsid_ed_within_wide_batch(ngsid_ctx* ctx, const ngsid_reads_t* queries, const ngsid_reads_t* targets, const uint32_t* q_idx, const uint32_t* t_idx, uint64_t n_pairs,
                                              int32_t max_dist, uint32_t flags, int32_t* dist, uint8_t* strand)
{
    ApiClock api_clock_(ctx, "ed_within_wide_batch");
    if (!ctx) return NGSID_ERR_ARG;
    return near_within_run(ctx, queries, targets, q_idx, t_idx, n_pairs, max_dist, NGSID_NEAR_WIDE_MAX_DIST, flags, dist, strand);
}

extern "C" int32_t ngsid_near_pairs(ngsid_ctx* ctx, const ngsid_reads_t* seqs, int32_t max_dist, uint32_t flags, uint32_t* pair_i, uint32_t* pair_j, uint8_t* dist, uint8_t* strand,
                                    uint64_t cap, uint64_t* n_found, uint64_t* needed)
{
    ApiClock api_clock_(ctx, "near_pairs");
    if (!ctx) return NGSID_ERR_ARG;
    return near_pairs_run(ctx, seqs, max_dist, NGSID_NEAR_MAX_DIST, flags, pair_i, pair_j, dist, strand, cap, n_found, needed);
}

extern "C" int32_t ngsid_near_pairs_wide(ngsid_ctx* ctx, const ngsid_reads_t* seqs, int32_t max_dist, uint32_t flags, uint32_t* pair_i, uint32_t* pair_j, uint8_t* dist, uint8_t* strand,
                                         uint64_t cap, uint64_t* n_found, uint64_t* needed)
{
    ApiClock api_clock_(ctx, "near_pairs_wide");
    if (!ctx) return NGSID_ERR_ARG;
    return near_pairs_run(ctx, seqs, max_dist, NGSID_NEAR_WIDE_MAX_DIST, flags, pair_i, pair_j, dist, strand, cap, n_found, needed);
}
