// k_recruit.hip - ngsid_recruit (include/ngsid_recruit.h): every read of a group located inside every consensus strand of that group, the two nearest consensuses per
// read reduced in registers.
//
// The recurrence is ngsid_host_infix_locate's (host_io.hip, myers_last_row with a free start) for patterns of up to 2 048 letters: Hyyro's block form, W = ceil(m / 64)
// 64-bit words per lane, the horizontal delta of block b handed to block b + 1 (the carry of the addition is NOT), the score followed at row m - 1 of the last block, the same
// 64-bit expressions as the host function, so every score of the last row is the host's.
// Lane mapping.  One read per lane.  The host cuts the reads of a chunk into waves of up to 64 consecutive reads of ONE group (RcWave); a wave walks that group's
// consensuses, forward strand then reverse complement, all lanes stepping the same pattern: the word count and the bound are wave-uniform, the only divergence is the read
// length - a wave runs to its longest read and a lane past its own L takes no minimum (as k_demux_scan).  Each lane keeps its best two (D, index), the strand and end of the
// best; one store of six ints per read, no cross-lane reduction, no found list.
// Instances.  Pv[W] and Mv[W] live in registers, so the block loop is unrolled at compile time: one instance per word count of RC_INSTANCES; a wave runs in the smallest
// instance that holds the longest consensus of its group, and a shorter pattern skips the blocks it has not got behind a wave-uniform branch.
// Match words (the first route of the two that were weighed): the [5 letters][W] table of the current pattern strand, built on the host, copied into a
// wave-private LDS slice; the address of a column's word depends on the lane's letter alone, so at most five distinct addresses are read per word.
// Letters: the wave's reads pass through the LDS in staging chunks of RC_CHUNK letters as codes (ngsid_base_code), rows RC_STRIDE bytes apart so that the 64 lanes' reads of
// their own row fall into different banks.
// LDS per workgroup (4 waves): 4 x 5 x W x 8 B of match words (at most 5 120 B) + 4 x 64 x RC_STRIDE = 33 792 B of letter codes.  A wave's LDS instructions execute in
// order, and nothing is shared between waves: no workgroup barrier.
#include "ngsid_host.h"
#include "../../include/ngsid_recruit.h"
#include <algorithm>

typedef unsigned long long u64;

#define RC_WAVES 4
#define RC_THREADS (RC_WAVES * 64)
#define RC_CHUNK 128                    // letters of a read staged at a time (tests/test_gpu_recruit.py places read lengths around its multiples)
#define RC_STRIDE (RC_CHUNK + 4)        // bytes between the rows of two lanes: 33 dwords, so lane l's dword j sits in bank (l + j) % 32
#define RC_NONE 0x7fffffff
#define RC_MAX_W (NGSID_RECRUIT_MAX_LEN / 64)
#define RC_CUT_DEFAULT 1                // what option "recruit_cutoff" = 0 (unset) means: 1 = the cut-off instances (profiles/recruit.txt), 0 = the plain ones

static_assert(RC_CHUNK % 4 == 0, "staging in 32-bit words");
static_assert(NGSID_RECRUIT_MAX_LEN % 64 == 0 && RC_MAX_W == 32, "the widest instance holds the longest consensus");

struct RcWave { u64 r0; uint32_t nr, group; };                  // reads r0 .. r0 + nr - 1 (nr <= 64) of `group`
struct RcCons { int32_t m, k; u64 peq; };                       // letters, k_c, first match word of the forward strand: [2 strands][5 letters][W] behind it

// the wave's LDS writes are done and visible to its lanes before any lane goes on (a wave's LDS instructions execute in order; the fence makes the compiler wait for them)
__device__ __forceinline__ void rc_wave_sync() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); }
__device__ __forceinline__ int rc_wave_max(int v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d));
    return v;
}

// one text letter through blocks 0 .. nb - 1 of a column of Wp <= W blocks (the plain kernel: nb = Wp).  eq: the lane's row of the match words ([Wp], in the LDS); top: bit of
// row m - 1 in the last block.  -> the horizontal delta at the last row of block nb - 1: with nb = Wp the change of the score of row m - 1
template <int W>
__device__ __forceinline__ int rc_column(u64 (&Pv)[W], u64 (&Mv)[W], const u64* __restrict__ eq, int nb, int Wp, int top)
{
    u64 hp = 0, hm = 0;                                         // the horizontal delta entering the block: +1, -1 or neither (row 0: free start in the read)
#pragma unroll
    for (int b = 0; b < W; ++b) {
        if (b < nb) {                                           // wave-uniform
            const u64 Eq = eq[b];
            const int tb = b == Wp - 1 ? top : 63;
            const u64 Xv = Eq | Mv[b];
            const u64 Eq2 = Eq | hm;
            const u64 Xh = (((Eq2 & Pv[b]) + Pv[b]) ^ Pv[b]) | Eq2;
            u64 Ph = Mv[b] | ~(Xh | Pv[b]), Mh = Pv[b] & Xh;
            const u64 op = (Ph >> tb) & 1ull, om = (Mh >> tb) & 1ull;
            Ph = (Ph << 1) | hp; Mh = (Mh << 1) | hm;
            Pv[b] = Mh | ~(Xv | Ph); Mv[b] = Ph & Xv;
            hp = op; hm = om;
        }
    }
    return (int)hp - (int)hm;
}

// ---- the cut-off (CUT instances): edlib's last-active-block rule, made uniform over the wave.  Only blocks 0 .. B are stepped; `score` is then the value at the last row
// of block B.  Before a column block B + 1 enters - as all +1 vertical deltas, an upper bound of what it holds - when SOME live lane has score <= k; one block per column is
// enough, because a cell of block B + 2 can be <= k in a column only if the last row of block B + 1 was <= k in the column before.  After a column block B leaves - one block per column - when EVERY
// lane that sees another column has score - (rows of B - 1) > k: no cell of the block can be <= k.  Every cell whose true value is <= k lies in a stepped block and is exact
// there, values above k are upper bounds, so the hit, its distance and its end are those of the plain column (tests/recruit_block_model.py pins the rule on the CPU).
// (block B is picked out of the register arrays by selects over the unrolled b: an assignment behind `if (b == B)` makes hipcc index the arrays in scratch memory)
template <int W>
__device__ __forceinline__ void rc_block_enter(u64 (&Pv)[W], u64 (&Mv)[W], int B)
{
#pragma unroll
    for (int b = 1; b < W; ++b) { Pv[b] = b == B ? ~0ull : Pv[b]; Mv[b] = b == B ? 0ull : Mv[b]; }
}
// the sum of the vertical deltas of block B over its `rows` rows: what the score falls by when the block leaves
template <int W>
__device__ __forceinline__ int rc_block_rise(const u64 (&Pv)[W], const u64 (&Mv)[W], int B, int rows)
{
    u64 pv = 0, mv = 0;
#pragma unroll
    for (int b = 1; b < W; ++b) { pv = b == B ? Pv[b] : pv; mv = b == B ? Mv[b] : mv; }
    const u64 mask = rows == 64 ? ~0ull : (1ull << rows) - 1ull;
    return __popcll(pv & mask) - __popcll(mv & mask);
}

template <int W, bool CUT>
__global__ __launch_bounds__(RC_THREADS)
void k_recruit(const uint8_t* __restrict__ seq, const uint64_t* __restrict__ off, const RcWave* __restrict__ waves, uint32_t nwaves,
               const uint64_t* __restrict__ cons_off /* [n_groups + 1] */, const RcCons* __restrict__ cons, const u64* __restrict__ peq, int nstrand,
               u64 chunk_r0, int32_t* __restrict__ hits /* [reads of the chunk][6] */, unsigned long long* __restrict__ stat /* block steps of all waves, or null */)
{
    __shared__ __attribute__((aligned(16))) u64 s_peq_all[RC_WAVES][5 * W];
    __shared__ __attribute__((aligned(16))) uint8_t s_win_all[RC_WAVES][64 * RC_STRIDE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t wi = blockIdx.x * RC_WAVES + wave;
    if (wi >= nwaves) return;                                   // (no workgroup barrier below)
    u64* s_peq = s_peq_all[wave];
    uint8_t* s_win = s_win_all[wave];
    const uint8_t* my_win = s_win + lane * RC_STRIDE;
    const RcWave wv = waves[wi];
    const bool have = (uint32_t)lane < wv.nr;
    const u64 my_r = wv.r0 + (u64)lane;
    u64 a = 0; int L = 0;
    if (have) { a = off[my_r]; L = (int)(off[my_r + 1] - a); }
    const int Lmax = rc_wave_max(L);
    const uint32_t a_lo = (uint32_t)a, a_hi = (uint32_t)(a >> 32);
    int d1 = RC_NONE, c1 = -1, s1 = 0, e1 = -1, d2 = RC_NONE, c2 = -1;
    unsigned long long steps = 0;                               // block steps of this wave (one per block and column; wave-uniform), counted while profiling
    const u64 cb =cons_off[wv.group], ce = cons_off[wv.group + 1];
    for (u64 c = cb; c < ce; ++c) {
        const RcCons cn_ = cons[c];
        const int m = cn_.m, k = cn_.k;
        const int Wp = (m + 63) >> 6, top = (m - 1) & 63;
        int dbest = RC_NONE, ebest = -1, sbest = 0;
        for (int s = 0; s < nstrand; ++s) {
            // ---- this strand's match words into the wave's slice
            rc_wave_sync();                                     // the previous strand's columns have been read
            for (int i = lane; i < 5 * Wp; i += 64) s_peq[i] = peq[cn_.peq + (u64)s * 5 * Wp + i];
            u64 Pv[W], Mv[W];
#pragma unroll
            for (int b = 0; b < W; ++b) { Pv[b] = ~0ull; Mv[b] = 0; }
            int B = CUT ? 0 : Wp - 1;                           // the last block that is stepped (wave-uniform); `score` is the value at its last row
            int score = CUT ? min(m, 64) : m, d = RC_NONE, e = -1;
            for (int c0 = 0; c0 < Lmax; c0 += RC_CHUNK) {
                const int cn = min(RC_CHUNK, (Lmax - c0 + 3) & ~3);      // columns of this chunk, a multiple of 4
                // ---- stage letters [c0, c0 + cn) of the wave's reads, four per lane and step (past a read's end: N)
                rc_wave_sync();                                 // the previous chunk has been read
                for (int w = lane; w < 64 * (RC_CHUNK / 4); w += 64) {
                    const int gi = w / (RC_CHUNK / 4), j = (w % (RC_CHUNK / 4)) * 4;
                    const u64 ag = ((u64)__shfl(a_hi, gi) << 32) | __shfl(a_lo, gi);
                    const int Lg = __shfl(L, gi);
                    if (j >= cn) continue;
                    uint32_t wd = 0;
#pragma unroll
                    for (int q = 0; q < 4; ++q) wd |= (c0 + j + q < Lg ? ngsid_base_code(seq[ag + (u64)(c0 + j + q)]) : 4u) << (8 * q);
                    *(uint32_t*)(s_win + gi * RC_STRIDE + j) = wd;
                }
                rc_wave_sync();
                for (int j0 = 0; j0 < cn; j0 += 4) {
                    const uint32_t wd = *(const uint32_t*)(my_win + j0);
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const uint32_t code = (wd >> (8 * q)) & 0xffu;
                        const int j = c0 + j0 + q;
                        if (CUT && B < Wp - 1 && __any(j < L && score <= k)) {
                            ++B; rc_block_enter<W>(Pv, Mv, B); score += B == Wp - 1 ? top + 1 : 64;
                        }
                        score += rc_column<W>(Pv, Mv, s_peq + code * Wp, B + 1, Wp, top);
                        if (stat) steps += (unsigned)(B + 1);
                        if (j < L && B == Wp - 1 && score < d) { d = score; e = j; }      // the smallest j that attains the minimum (row m - 1 is known where the last block is stepped)
                        if (CUT && B > 0) {
                            const int rows = B == Wp - 1 ? top + 1 : 64;
                            if (!__any(j + 1 < L && score - (rows - 1) <= k)) { score -= rc_block_rise<W>(Pv, Mv, B, rows); --B; }
                        }
                    }
                }
            }
            if (d <= k && d < dbest) { dbest = d; ebest = e; sbest = s; }  // a tie goes to forward
        }
        if (dbest != RC_NONE) {                                 // consensuses come in ascending index: on equal D the earlier one stays in front
            if (dbest < d1) { d2 = d1; c2 = c1; d1 = dbest; c1 = (int)c; s1 = sbest; e1 = ebest; }
            else if (dbest < d2) { d2 = dbest; c2 = (int)c; }
        }
    }
    if (have) {
        int32_t* h = hits + (my_r - chunk_r0) * NGSID_RECRUIT_NFIELD;
        h[0] = c1; h[1] = c1 < 0 ? -1 : d1; h[2] = s1; h[3] = e1; h[4] = c2; h[5] = c2 < 0 ? -1 : d2;
    }
    if (stat && lane == 0) atomicAdd(stat, steps);
}

// ---- the instances: the word counts the block loop is unrolled for (DESIGN.md section 5 has their register counts)
static const int RC_INSTANCES[] = {1, 2, 4, 8, 12, 16, 24, 32};
#define RC_NINST ((int)(sizeof(RC_INSTANCES) / sizeof(RC_INSTANCES[0])))
static inline int rc_instance(int words) { int x = 0; while (RC_INSTANCES[x] < words) ++x; return x; }

template <int W>
static void rc_launch(ngsid_ctx* ctx, bool cut, unsigned grid, const DevReads& RD, const RcWave* waves, uint32_t nwaves, const uint64_t* cons_off, const RcCons* cons, const u64* peq,
                      int nstrand, u64 chunk_r0, int32_t* hits, unsigned long long* stat)
{
    if constexpr (W > 1) {                                      // one block has nothing to cut off
        if (cut) { hipLaunchKernelGGL((k_recruit<W, true>), dim3(grid), dim3(RC_THREADS), 0, ctx->stream, RD.seq, RD.off, waves, nwaves, cons_off, cons, peq, nstrand, chunk_r0, hits, stat); return; }
    }
    hipLaunchKernelGGL((k_recruit<W, false>), dim3(grid), dim3(RC_THREADS), 0, ctx->stream, RD.seq, RD.off, waves, nwaves, cons_off, cons, peq, nstrand, chunk_r0, hits, stat);
}

static inline uint8_t rc_complement(uint8_t c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : c; }

extern "C" int32_t ngsid_recruit(ngsid_ctx* ctx, const ngsid_reads_t* reads, const uint64_t* read_off, const ngsid_reads_t* cons, const uint64_t* cons_off, uint64_t n_groups,
                                 const int32_t* max_ed, uint32_t flags, int32_t* hits)
{
    ApiClock api_clock_(ctx, "recruit");
    if (!ctx) return NGSID_ERR_ARG;
    if (!reads || !cons || !read_off || !cons_off) NGSID_FAIL(ctx, NGSID_ERR_ARG, "null argument");
    if (cons->mem != NGSID_MEM_HOST) NGSID_FAIL(ctx, NGSID_ERR_ARG, "the consensuses are a host read set");
    const uint64_t N = reads->n, NC = cons->n;
    if ((N && !hits) || (NC && (!max_ed || !cons->off || !cons->seq))) NGSID_FAIL(ctx, NGSID_ERR_ARG, "null array");
    if (NC >= ((uint64_t)1 << 31) || n_groups >= ((uint64_t)1 << 32)) NGSID_FAIL(ctx, NGSID_ERR_ARG, "2^31 or more consensuses, or 2^32 or more groups");
    // ---- the two offset lists cover their sets, group by group
    if (read_off[0] != 0 || cons_off[0] != 0 || read_off[n_groups] != N || cons_off[n_groups] != NC) NGSID_FAIL(ctx, NGSID_ERR_ARG, "read_off / cons_off do not cover the read set / the consensus set");
    for (uint64_t g = 0; g < n_groups; ++g)
        if (read_off[g + 1] < read_off[g] || cons_off[g + 1] < cons_off[g] || read_off[g + 1] > N || cons_off[g + 1] > NC) NGSID_FAIL(ctx, NGSID_ERR_ARG, "group %llu: offsets not monotone", (unsigned long long)g);
    // ---- the consensuses: lengths, bounds, letters; the match words of both strands
    std::vector<RcCons> h_cons(NC); std::vector<u64> h_peq;
    const int nstrand = (flags & NGSID_RECRUIT_BOTH_STRANDS) ? 2 : 1;
    for (uint64_t c = 0; c < NC; ++c) {
        if (cons->off[c + 1] <= cons->off[c]) NGSID_FAIL(ctx, NGSID_ERR_ARG, "consensus %llu is empty", (unsigned long long)c);
        if (cons->off[c + 1] - cons->off[c] > NGSID_RECRUIT_MAX_LEN) NGSID_FAIL(ctx, NGSID_ERR_TOO_LONG, "consensus %llu is longer than %d", (unsigned long long)c, NGSID_RECRUIT_MAX_LEN);
        if (max_ed[c] < 0) NGSID_FAIL(ctx, NGSID_ERR_ARG, "max_ed[%llu] must not be negative", (unsigned long long)c);
    }
    for (uint64_t c = 0; c < NC; ++c) {
        const uint8_t* p = cons->seq + cons->off[c]; const int m = (int)(cons->off[c + 1] - cons->off[c]); const int Wp = (m + 63) / 64;
        for (int i = 0; i < m; ++i) if (!memchr("ACGTN", p[i], 5)) NGSID_FAIL(ctx, NGSID_ERR_ALPHABET, "a consensus base outside upper-case ACGTN");
        h_cons[c].m = m; h_cons[c].k = std::min<int32_t>(max_ed[c], m - 1); h_cons[c].peq = h_peq.size();
        h_peq.resize(h_peq.size() + (size_t)2 * 5 * Wp, 0);
        u64* fw = h_peq.data() + h_cons[c].peq; u64* rv = fw + 5 * Wp;
        for (int i = 0; i < m; ++i) {
            const uint8_t f = p[i], r = rc_complement(p[m - 1 - i]);
            fw[(size_t)(strchr("ACGTN", f) - "ACGTN") * Wp + i / 64] |= 1ull << (i & 63);
            rv[(size_t)(strchr("ACGTN", r) - "ACGTN") * Wp + i / 64] |= 1ull << (i & 63);
        }
    }
    DevReads RD; int32_t rc = ngsid_upload_reads(ctx, reads, &RD, false); if (rc) return rc;
    if (RD.maxlen > NGSID_MAX_READ_LEN) NGSID_FAIL(ctx, NGSID_ERR_TOO_LONG, "a read is longer than %d", NGSID_MAX_READ_LEN);
    if (N == 0) return NGSID_OK;
    NGSID_TRY(ngsid_alphabet_check(ctx, RD, nullptr, nullptr, "a read base outside upper-case ACGTN"));
    // ---- the instance of every group: the smallest that holds its longest consensus (a group without one: the narrowest)
    std::vector<uint8_t> g_inst(n_groups, 0);
    for (uint64_t g = 0; g < n_groups; ++g) {
        int words = 1; for (uint64_t c = cons_off[g]; c < cons_off[g + 1]; ++c) words = std::max(words, (h_cons[c].m + 63) / 64);
        g_inst[g] = (uint8_t)rc_instance(words);
    }
    DevBuf<RcCons> d_cons; DevBuf<u64> d_peq; DevBuf<uint64_t> d_coff; DevBuf<RcWave> d_waves; DevBuf<int32_t> d_hits;
    NGSID_TRY(dev_put(ctx, d_cons, h_cons.data(), h_cons.size())); NGSID_TRY(dev_put(ctx, d_peq, h_peq.data(), h_peq.size())); NGSID_TRY(dev_put(ctx, d_coff, cons_off, n_groups + 1));
    // ---- reads in chunks: six ints of results and (at worst, one read per wave) one wave record per read on the device
    const long long opt = ngsid_opt(ctx, "recruit_chunk_reads", 0);
    const long long cut_opt = ngsid_opt(ctx, "recruit_cutoff", 0);              // 0 the library's choice, 1 the plain instances, 2 the ones with the last-active-block rule: the same results
    const bool cut = cut_opt == 0 ? RC_CUT_DEFAULT != 0 : cut_opt == 2;
    DevBuf<unsigned long long> d_stat;                          // block steps of the call's launches, while profiling is on (else null)
    if (ctx->prof) { HIPCHK(ctx, d_stat.alloc(1)); HIPCHK(ctx, hipMemsetAsync(d_stat.p, 0, sizeof(unsigned long long), ctx->stream)); }
    const size_t per_read = NGSID_RECRUIT_NFIELD * sizeof(int32_t) + sizeof(RcWave);
    uint64_t chunk = opt > 0 ? (uint64_t)opt : ngsid_mem_share(4, (size_t)64 << 20, (size_t)4 << 30, (size_t)4 << 30) / per_read;
    chunk = std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(chunk, N), ngsid_max_blocks(RC_THREADS)));      // a wave holds a read at least: never more workgroups than reads
    HIPCHK(ctx, d_hits.alloc(chunk * NGSID_RECRUIT_NFIELD)); HIPCHK(ctx, d_waves.alloc(chunk));
    std::vector<RcWave> h_waves[RC_NINST], flat;
    uint64_t g = 0;
    for (uint64_t r0 = 0; r0 < N; r0 += chunk) {
        const uint64_t r1 = std::min(N, r0 + chunk);
        for (auto& v : h_waves) v.clear();
        while (g < n_groups && read_off[g + 1] <= r0) ++g;
        for (uint64_t gg = g; gg < n_groups && read_off[gg] < r1; ++gg)
            for (uint64_t x = std::max(r0, read_off[gg]), y = std::min(r1, read_off[gg + 1]); x < y; x += 64)
                h_waves[g_inst[gg]].push_back(RcWave{x, (uint32_t)std::min<uint64_t>(64, y - x), (uint32_t)gg});
        flat.clear(); for (auto& v : h_waves) flat.insert(flat.end(), v.begin(), v.end());
        HIPCHK(ctx, hipMemcpyAsync(d_waves.p, flat.data(), flat.size() * sizeof(RcWave), hipMemcpyHostToDevice, ctx->stream));
        size_t at = 0;
        for (int x = 0; x < RC_NINST; ++x) {
            const uint32_t nw = (uint32_t)h_waves[x].size(); if (!nw) continue;
            const unsigned grid = NGSID_GRID(ctx, (nw + RC_WAVES - 1) / RC_WAVES, RC_THREADS, "k_recruit");
            ProfScope ps_(ctx, "k_recruit");
            const RcWave* wl = d_waves.p + at;
            switch (RC_INSTANCES[x]) {
                case 1:  rc_launch<1>(ctx, cut, grid, RD, wl, nw, d_coff.p, d_cons.p, d_peq.p, nstrand, r0, d_hits.p, d_stat.p); break;
                case 2:  rc_launch<2>(ctx, cut, grid, RD, wl, nw, d_coff.p, d_cons.p, d_peq.p, nstrand, r0, d_hits.p, d_stat.p); break;
                case 4:  rc_launch<4>(ctx, cut, grid, RD, wl, nw, d_coff.p, d_cons.p, d_peq.p, nstrand, r0, d_hits.p, d_stat.p); break;
                case 8:  rc_launch<8>(ctx, cut, grid, RD, wl, nw, d_coff.p, d_cons.p, d_peq.p, nstrand, r0, d_hits.p, d_stat.p); break;
                case 12: rc_launch<12>(ctx, cut, grid, RD, wl, nw, d_coff.p, d_cons.p, d_peq.p, nstrand, r0, d_hits.p, d_stat.p); break;
                case 16: rc_launch<16>(ctx, cut, grid, RD, wl, nw, d_coff.p, d_cons.p, d_peq.p, nstrand, r0, d_hits.p, d_stat.p); break;
                case 24: rc_launch<24>(ctx, cut, grid, RD, wl, nw, d_coff.p, d_cons.p, d_peq.p, nstrand, r0, d_hits.p, d_stat.p); break;
                default: rc_launch<32>(ctx, cut, grid, RD, wl, nw, d_coff.p, d_cons.p, d_peq.p, nstrand, r0, d_hits.p, d_stat.p); break;
            }
            at += nw;
        }
        HIPCHK(ctx, hipGetLastError());
        NGSID_TRY(dev_get(ctx, hits + r0 * NGSID_RECRUIT_NFIELD, d_hits.p, (size_t)(r1 - r0) * NGSID_RECRUIT_NFIELD));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));         // the wave records and the result buffer are reused by the next chunk
    }
    if (d_stat.p) {                                             // profiling line recruit_block_steps: the count field holds the block steps
        unsigned long long steps = 0;
        NGSID_TRY(dev_get(ctx, &steps, d_stat.p, 1)); HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        ctx->prof_acc["recruit_block_steps"].second += steps;
    }
    return NGSID_OK;
}
