// k_align16p.hip - the packed-int16 semi-global aligner with TWO PAIRS PER WAVE (round 3).
//
// Same DP, same tie-breaks, same outputs as k_sg_align16 / k_sg_align / the oracle; different packing.  k_sg_align16 puts two row halves of ONE pair
// in the two 16-bit halves of a register, one column apart, which costs a systolic skew of two columns per lane (m + 127 steps).  Here the low halves
// belong to pair 0 and the high halves to pair 1 of a work item: both work on the same column, the skew is one column per lane (max(m0, m1) + 63
// steps), a lane owns R consecutive query rows of each pair (single strip: n <= 64 R), and the per-step overhead (letters, masks, DPP hand-off, the
// store) is paid once for two pairs.  About 11 % fewer VALU instructions per pair in a loop that runs at the VALU issue rate.
// The capture of the last query row is a compile-time choice of the register (as in k_sg_align16), so the two pairs of an item must agree in
// (n - 1) mod R: the launcher bins the pairs of a length class by that residue (k_pair_bins / k_bin_offsets / k_bin_scatter in k_align.hip) and an item is
// two consecutive entries of a bin (the last item of a bin may hold one pair).  Results are written by pair index, so the pairing does not show.
// The traceback walk and its bookkeeping are shared with k_sg_align16 (k_align_common.h); the launches and the routing are in k_align.hip.
#include "k_align_common.h"
#include <type_traits>

// The traceback flags of this kernel are SIGN bits of packed 16-bit differences (d - h, E - mx, e_ext - E, f_ext - F): exact only while no difference wraps.  The
// largest magnitude is a cell at the "minus infinity" NEG16 (less one extension) against the largest score a pair of this kernel can reach - the bounds of
// ngsid_align16_applicable (match <= 4, ext <= 4, open <= 16) with queries of at most 896 bases (the single-strip classes): ADVICE r4.
// The row state is g = h - open rather than h (one subtraction per cell instead of the two of e_opn / f_opn).  The bound holds unchanged in that frame: the four
// differences are the same numbers as before (e_opn = g_left, f_opn = g_up, d = g_diag + (score + open)); the one new value g = h - open stays above NEG16 - ext
// (an h is at least -open - ext * 4000, a gap along a whole target of the int16 range); the diagonal constant match + open is at most 20.
static_assert(sg16p_flag_span(4 /* match */, 4 /* ext */, 16 /* open */, 896 /* query rows */, NGSID_ALIGN16_MAXLEN, false) < 32768, "packed sign-bit flags of k_sg_align16p would wrap");
//
// The SKEW instances keep every value of cell (i, j) in the frame X^ = X + (i + j) ext (the column skew k_poa.hip uses for its in-row gap chain, here in both gap
// directions), with the row state g' = H - open + ext:
//     E^(i, j) = max(E^(i, j-1), g'^(i, j-1))        F^(i, j) = max(F^(i-1, j), g'^(i-1, j))        (no "- ext": the frame of the neighbour is one ext behind)
//     d^ = g'^(i-1, j-1) + (score + open + ext)      h^ = max(d^, E^, F^)                           g'^ = h^ - (open - ext)
// All candidates of a cell carry the same skew, so every maximum, every tie-break and the four flag differences (d^ - h^, E^ - mx^, E^left - E^, F^up - F^) are the
// numbers of the plain frame: the traceback words do not change.  The frame is undone where values of different cells meet (the maxima over the last row and the
// last column) and where one leaves the kernel (best).
// Range.  The real values of the frame lie in [-2 open - ext + mismatch, match min(n, m) + (n + m) ext]: below, H(i, j) >= -open - min(i, j) ext (a gap from the nearer border),
// which the skew lifts to >= -open; above, H <= match min(n, m) and the skew of the last cell plus the ext of g' is at most (n + m) ext.  The one value outside is the
// "minus infinity" NEG16 of E in column -1 and of F in row -1, which the frame neither lifts nor (without the "- ext") lowers.  So every same-cell difference, one
// against NEG16 included, is below -(NEG16) + ext + open + match min(n, m) + (n + m + 1) ext = sg16p_flag_span(..., true), and must stay below 2^15: with ext = 1 that
// holds for every length of the paired classes (static_assert below); a call with a larger ext and long targets runs the plain instances (the host decides per call,
// from its own maximum lengths: ngsid_align16p_skew_exact in k_align.hip).
// In the NOWILD SKEW instances the score of a row is one byte permute: a lane's target letter is fixed for a step, so the step builds per pair a table of four bytes,
// byte c = score + open + ext of query letter c against that target letter, and row r selects byte q_r (pair 0: low half) and byte 4 + q_r (pair 1: high half) with
// zero high bytes.  It needs 0 <= mismatch + open + ext and match + open + ext <= 255; an item that does not satisfy it runs the instance with the select (mad form).
static_assert(sg16p_flag_span(4, 1, 16, 896, NGSID_ALIGN16_MAXLEN, true) < 32768, "the skewed frame of k_sg_align16p must hold every paired length with ext = 1");
// (inline asm: the masks and selectors live in SGPRs - gfx9 VOP3 takes no literal)
__device__ __forceinline__ int pp_bfi(int mask_s, int a, int b) { int d; asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(d) : "s"(mask_s), "v"(a), "v"(b)); return d; }        // (a & mask) | (b & ~mask)
// byte permute of {a : b} (b = bytes 0..3); selectors 8..11 give 0xFF or 0x00 by the sign of bits 15, 31, 47, 63 = of the halves b.lo, b.hi, a.lo, a.hi
__device__ __forceinline__ int pp_perm(int a, int b, int sel_s) { int d; asm("v_perm_b32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "s"(sel_s)); return d; }
__device__ __forceinline__ int pp_permv(int a, int b, int sel_v) { int d; asm("v_perm_b32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(sel_v)); return d; }          // per-lane selector
// 0xFFFF / 0 by the sign of each half (the shift count comes packed from an SGPR: an inline constant would reach the low half only)
__device__ __forceinline__ int pk_ashr15_i16(int a) { int d; asm("v_pk_ashrrev_i16 %0, %1, %2" : "=v"(d) : "s"(0x000F000F), "v"(a)); return d; }
__device__ __forceinline__ int pp_sel(int mask, int a, int b) { return (a & mask) | (b & ~mask); }      // per bit: mask ? a : b (one v_bfi)

// traceback layout: the word of cell (i, j) is at step j + l, lane l = i / R (one strip); row r = i % R is bit r % 8 of the four flag bytes of the 32-bit half r / 8,
// flags complemented
template <int R>
struct Planes {
    const uint64_t* tb;
    __device__ SgCell at(int i, int j) const { const int l = i / R; return SgCell{l >> 3, j + l, l & 7, i - l * R}; }
    __device__ const uint64_t* block(int grp, int tt) const { return tb + (uint64_t)tt * 64 + grp * 8; }
    __device__ int flags(uint64_t word, int r) const {
        const unsigned x = (unsigned)(word >> (32 * (r >> 3) + (r & 7)));
        return (int)(~(x & 1u) & 1u) | (int)(~(x >> 7) & 2u) | (int)(~(x >> 14) & 4u) | (int)(~(x >> 21) & 8u);
    }
};

// (the SKEW instances name the occupancy of the plain ones as their minimum: left to itself the scheduler spends registers up to the next occupancy step)
template <int R, bool SKEW>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(SKEW ? (R <= 8 ? 4 : 3) : 2, 4)))
void k_sg_align16p(AlignJob J, const uint32_t* __restrict__ sorted, const uint32_t* __restrict__ bin_off /* [PBINS + 1] pairs */, const uint32_t* __restrict__ item_off /* [PBINS + 1] items */,
                   uint64_t* __restrict__ tb, uint64_t tb_words_per_wave /* per half */, uint32_t seq_lds, uint32_t* __restrict__ work_ctr)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x;
    uint8_t* tgt0 = smem; uint8_t* tgt1 = tgt0 + seq_lds; uint8_t* qry0 = tgt1 + seq_lds; uint8_t* qry1 = qry0 + seq_lds;
    uint64_t* tbblk = (uint64_t*)(smem + 4 * (size_t)seq_lds);            // traceback block: 64 steps x 8 lanes
    uint64_t* mytb0 = tb + (uint64_t)blockIdx.x * tb_words_per_wave * 2; uint64_t* mytb1 = mytb0 + tb_words_per_wave;
    constexpr int NA = 2 * ((R + 7) / 8);                                 // flag accumulators: two per group of 8 rows, one (flag, pair) plane per byte
    const uint32_t nitems = item_off[PBINS];

    for (;;) {
        uint32_t pq = 0; if (lane == 0) pq = atomicAdd(work_ctr, 1u);
        const uint32_t kq = (uint32_t)__builtin_amdgcn_readfirstlane((int)pq);
        if (kq >= nitems) break;
        int bin = 0;
        while (bin + 1 < PBINS && item_off[bin + 1] <= kq) ++bin;        // (<= 32 scalar loads; the items of a wave come in bin order)
        const uint32_t ib = kq - item_off[bin], b0 = bin_off[bin], cntb = bin_off[bin + 1] - b0;
        const bool have1 = 2 * ib + 1 < cntb;
        const uint64_t p0 = sorted[b0 + 2 * ib], p1 = have1 ? sorted[b0 + 2 * ib + 1] : p0;
        const uint32_t qi0 = J.qidx[p0], ti0 = J.tidx[p0], qi1 = J.qidx[p1], ti1 = J.tidx[p1];
        const uint8_t* q0 = J.qseq + J.qoff[qi0]; const uint8_t* t0 = J.tseq + J.toff[ti0];
        const uint8_t* q1 = J.qseq + J.qoff[qi1]; const uint8_t* t1 = J.tseq + J.toff[ti1];
        int n0 = sgpr((int)(J.qoff[qi0 + 1] - J.qoff[qi0])), m0 = sgpr((int)(J.toff[ti0 + 1] - J.toff[ti0]));
        int n1 = sgpr((int)(J.qoff[qi1 + 1] - J.qoff[qi1])), m1 = sgpr((int)(J.toff[ti1 + 1] - J.toff[ti1]));
        if (!have1) { n1 = 0; m1 = 0; }                                   // single pair: the high halves stay inactive
        // an empty target or an empty query (class 0 holds queries from 0 bases up): the outputs of k_sg_align16 for that case, the half takes no part in the DP
        const bool deg0 = m0 <= 0 || n0 <= 0, deg1 = have1 && (m1 <= 0 || n1 <= 0);
        if (deg0) sg_degenerate(J, p0, n0, m0, lane);
        if (deg1) sg_degenerate(J, p1, n1, m1, lane);
        const int own_p = ((n0 > 0 ? n0 : 1) - 1) % R;                    // == (n1 - 1) % R: same bin
        if (deg0) { n0 = 0; m0 = 0; }
        if (deg1) { n1 = 0; m1 = 0; }
        if (deg0 && (deg1 || !have1)) continue;
        // letters outside ACGT (bits 0x7C of the permuted byte) score 0 against everything: two mask operations per cell that an item without such letters - nearly
        // every item - does not need (NOWILD instances of the step loop below; same results by construction)
        unsigned wild = 0;
        for (int x = lane; x < m0; x += 64) { const uint8_t v = perm_letter(t0[x]); tgt0[x] = v; wild |= v; }
        for (int x = lane; x < n0; x += 64) { const uint8_t v = perm_letter(q0[x]); qry0[x] = v; wild |= v; }
        for (int x = lane; x < m1; x += 64) { const uint8_t v = perm_letter(t1[x]); tgt1[x] = v; wild |= v; }
        for (int x = lane; x < n1; x += 64) { const uint8_t v = perm_letter(q1[x]); qry1[x] = v; wild |= v; }
        const bool nowild = __ballot((wild & 0x7Cu) != 0) == 0;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();

        // SKEW: ext and the lane's first row are made values of THIS item (the empty asm hides where they come from).  As kernel invariants, the per-row frame
        // offsets (i0 + r) ext are hoisted out of the item loop and hold R registers for the whole kernel - the difference between 3 and 2 waves per SIMD at R = 12
        int ext = J.ext; if constexpr (SKEW) asm volatile("" : "+s"(ext));
        const int open0 = sgpr(J.open[p0]), open1 = sgpr(J.open[p1]), skx = SKEW ? ext : 0;
        const int NOPEN2 = sgpr(PK(-open0, -open1)), EXT2 = sgpr(PK(ext, ext));
        const int dk0 = open0 + skx, dk1 = open1 + skx;                      // the diagonal adds back what the row state lacks: g_diag + score + open (SKEW: + ext)
        const int DIAG2 = sgpr(PK(dk0, dk1)), GSUB2 = sgpr(PK(open0 - skx, open1 - skx));   // score 0 on the diagonal (wildcards); h -> row state
        const int MATCHO2 = PK(J.match + dk0, J.match + dk1), NDIFF2 = sgpr(PK(J.mismatch - J.match, J.mismatch - J.match));
        const int ONE2 = sgpr(0x00010001);
        // SKEW, permute score table: byte c of the table of a target letter t is the diagonal constant of query letter c; XX = mismatch in all four bytes, MX turns byte t into match
        const bool tbl_ok = SKEW && J.mismatch + dk0 >= 0 && J.mismatch + dk1 >= 0 && J.match + dk0 <= 255 && J.match + dk1 <= 255;
        const int XX0 = sgpr((J.mismatch + dk0) * 0x01010101), XX1 = sgpr((J.mismatch + dk1) * 0x01010101), MX0 = sgpr((J.match + dk0) ^ (J.mismatch + dk0)), MX1 = sgpr((J.match + dk1) ^ (J.mismatch + dk1));
        // (the v_perm selectors and the row masks of the flag planes are constants for the "s" operands of the asm: s_mov, which the compiler can rematerialise)
        constexpr int SGN = 0x0B0A0908;                                   // v_perm: the signs of b.lo, b.hi, a.lo, a.hi as 0x00 / 0xFF bytes
        constexpr int SEL0 = 0x06040200, SEL1 = 0x07050301;               // v_perm: the pair 0 / pair 1 bytes of the two accumulators of a row group
        const int mmax = m0 > m1 ? m0 : m1;
        const int steps = mmax + 63;
        const int own_lane0 = n0 > 0 ? (n0 - 1) / R : -1, own_lane1 = n1 > 0 ? (n1 - 1) / R : -1;
        int bestRowV0 = -(1 << 29), bestRowJ0 = 0, bestRowV1 = -(1 << 29), bestRowJ1 = 0;
        int hl2[R], e2[R], qc2[R], nwq2[R];                                // hl2 = g = H - open of the last column (column -1: H = 0; SKEW: g' = -open + ext in the frame of cell (i, -1))
        int i0 = lane * R; if constexpr (SKEW) asm volatile("" : "+v"(i0));
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = i0 + r;
            const int ca = i < n0 ? qry0[i] : 0x7C, cb = i < n1 ? qry1[i] : 0x7C;
            // (SKEW: a wildcard is the SIGN of the letter's half instead of a mask register per row - the wildcard instance pays one shift per row for R registers less;
            // the flag makes such a letter differ from every target letter, which the wildcard select overrides)
            if constexpr (SKEW) { qc2[r] = PK((ca & 3) | ((ca & 0x7C) ? 0x8000 : 0), (cb & 3) | ((cb & 0x7C) ? 0x8000 : 0)); nwq2[r] = 0; }
            else { qc2[r] = PK(ca & 3, cb & 3); nwq2[r] = PK((ca & 0x7C) ? 0 : 0xffff, (cb & 0x7C) ? 0 : 0xffff); }
            hl2[r] = SKEW ? PK(i * ext - open0, i * ext - open1) : NOPEN2; e2[r] = PK(NEG16, NEG16);
        }

        auto forward = [&](auto OPc, auto NWc) {
            constexpr int OWN_P = decltype(OPc)::value; constexpr bool NOWILD = decltype(NWc)::value;
            constexpr bool TABLE = SKEW && NOWILD;                        // (a SKEW item the table cannot hold runs the !NOWILD instance: see the switch below)
            int hdiag2 = SKEW ? PK((i0 - 1) * ext - open0, (i0 - 1) * ext - open1) : NOPEN2;      // g[i0-1][j-1], both pairs (SKEW: cell (i0 - 1, -1))
            if constexpr (TABLE) {
#pragma unroll
                for (int r = 0; r < R; ++r) qc2[r] += 0x0C040C00;         // v_perm selectors of the row: byte q of pair 0's table, zero, byte 4 + q = of pair 1's table, zero
            }
            int send_h = NOPEN2, send_f = PK(NEG16, NEG16);               // bottom row (g, F) of this lane for the next one
            int keyRow0 = (int)0x80000000u, keyRow1 = (int)0x80000000u; const int jinv0 = 0xFFFF + lane;      // steady steps: packed (last-row g, -column) maxima
            // The steps in which EVERY lane stands inside both targets (tau - lane in [0, min(m0, m1)) for all 64 lanes: 63 <= tau < min(m0, m1), 84 % of the steps of a 750-base
            // pair) need none of the range masks: their own instance of the step (STEADY) drops the mask selects of the state (one per row, three per step) and the range tests.
            auto step = [&](int tau, auto STc) {
                constexpr bool STEADY = decltype(STc)::value;
                const int j = tau - lane;
                // lane 0 has no source lane: the shift leaves it the `old` operand - -open for g (H = 0 in row -1 of the matrix), minus infinity for F (no select needed)
                // (SKEW: row -1 stands in the frame of cell (-1, j), j = tau for lane 0)
                const int top2 = SKEW ? PK(tau * ext - open0, tau * ext - open1) : NOPEN2;
                const int hup = __builtin_amdgcn_update_dpp(top2, send_h, 0x138, 0xf, 0xf, false), fup = __builtin_amdgcn_update_dpp(PK(NEG16, NEG16), send_f, 0x138, 0xf, 0xf, false);
                const bool a0 = STEADY || (j >= 0 && j < m0), a1 = STEADY || (j >= 0 && j < m1);      // STEADY: every lane stands inside both targets
                const int l0 = tgt0[STEADY ? j : (a0 ? j : 0)], l1 = tgt1[STEADY ? j : (a1 ? j : 0)];
                const int tc2 = TABLE ? 0 : PK(l0 & 3, l1 & 3);
                int tb0 = 0, tb1 = 0; if constexpr (TABLE) { tb0 = XX0 ^ (MX0 << ((l0 << 3) & 31)); tb1 = XX1 ^ (MX1 << ((l1 << 3) & 31)); }     // (letter & 3) * 8: the shift keeps five bits
                int nwt2 = 0; if constexpr (!NOWILD) nwt2 = PK((a0 && !(l0 & 0x7C)) ? 0xffff : 0, (a1 && !(l1 & 0x7C)) ? 0xffff : 0);
                const int am2 = STEADY ? -1 : PK(a0 ? 0xffff : 0, a1 ? 0xffff : 0);
                int hu2 = hup, f2 = fup, hd2 = hdiag2;
                int acc[NA], cap2 = 0;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    // the row state is g = H - open: the gap opens of E and F are the g of the left and of the upper cell, and the diagonal adds open back
                    // (SKEW: the extension candidates are the E of the left and the F of the upper cell as they are - their frame is one ext behind)
                    const int e_ext = SKEW ? e2[r] : pk_sub_i16_s(e2[r], EXT2); const int E = pk_max_i16(e_ext, hl2[r]);
                    const int f_ext = SKEW ? f2 : pk_sub_i16_s(f2, EXT2); const int F = pk_max_i16(f_ext, hu2);
                    int sc;
                    if constexpr (TABLE) sc = pp_permv(tb1, tb0, qc2[r]);                          // match / mismatch + open + ext from the step's tables
                    else {
                        const int z = pk_min_u16_s(qc2[r] ^ tc2, ONE2);                            // 1 = letters differ
                        sc = pk_mad_i16_sv(z, NDIFF2, MATCHO2);                                    // match / mismatch + open ...
                    }
                    if constexpr (!NOWILD) { const int nw = SKEW ? (~pk_ashr15_i16(qc2[r]) & nwt2) : (nwq2[r] & nwt2); sc = pp_sel(nw, sc, DIAG2); }   // ... / 0 + open for wildcards (and for columns outside the target, whose cells nothing reads)
                    const int d = pk_add_i16(hd2, sc);
                    const int mx = pk_max_i16(E, F); const int h = pk_max_i16(d, mx);
                    const int g = pk_sub_i16_s(h, GSUB2);
                    // COMPLEMENT flags (1 = "not equal"): 0 h!=d, 1 mx!=E (F>E), 2 E!=e_ext (opened), 3 F!=f_ext (opened)
                    // each flag is the SIGN of a packed difference (smaller - larger: negative iff they differ).  One v_perm turns the four signs of two differences into
                    // 0x00 / 0xFF bytes (flag 0 pair 0, flag 0 pair 1, flag 1 pair 0, flag 1 pair 1; flags 2 / 3 alike) and one bit-field insert keeps bit r & 7 of each:
                    // accumulator 2 (r >> 3) holds flags 0 / 1 of the rows of group r >> 3 as four bit planes of 8 rows, accumulator 2 (r >> 3) + 1 flags 2 / 3
                    const int s0 = pk_sub_i16(d, h), s1 = pk_sub_i16(E, mx), s2 = pk_sub_i16(e_ext, E), s3 = pk_sub_i16(f_ext, F);
                    const int pa = pp_perm(s1, s0, SGN), pb = pp_perm(s3, s2, SGN);
                    int& a01 = acc[2 * (r >> 3)]; int& a23 = acc[2 * (r >> 3) + 1];
                    if ((r & 7) == 0) { a01 = pa & 0x01010101; a23 = pb & 0x01010101; }                     // first row of a group: no zeroing
                    else { a01 = pp_bfi(0x01010101 << (r & 7), pa, a01); a23 = pp_bfi(0x01010101 << (r & 7), pb, a23); }
                    hd2 = hl2[r];
                    hl2[r] = STEADY ? g : pp_sel(am2, g, hl2[r]);
                    // not masked in the plain frame (see k_align16.hip: before a lane's first column E only relaxes to -open, after its last it is not used).  SKEW: without the
                    // "- ext" a relaxed E would EQUAL the open candidate of column 0 and turn its "opened" flag: E stays at minus infinity until the lane's first column
                    e2[r] = (SKEW && !STEADY) ? pp_sel(am2, E, e2[r]) : E;
                    hu2 = g; f2 = F;
                    if (r == OWN_P) cap2 = g;
                }
                // traceback words: bits [32 k, 32 k + 32) = row group k, byte f of the group = flag f (complement), bit b of the byte = row 8 k + b; pair 0 takes the
                // even bytes of the group's two accumulators, pair 1 the odd ones
                unsigned long long w0 = 0, w1 = 0;
#pragma unroll
                for (int k = 0; k < NA / 2; ++k) {
                    w0 |= (unsigned long long)(unsigned)pp_perm(acc[2 * k + 1], acc[2 * k], SEL0) << (32 * k);
                    w1 |= (unsigned long long)(unsigned)pp_perm(acc[2 * k + 1], acc[2 * k], SEL1) << (32 * k);
                }
                mytb0[(uint64_t)tau * 64 + lane] = w0;
                mytb1[(uint64_t)tau * 64 + lane] = w1;
                if (STEADY) { hdiag2 = hup; send_h = hu2; send_f = f2; }
                else { hdiag2 = pp_sel(am2, hup, hdiag2); send_h = pp_sel(am2, hu2, send_h); send_f = pp_sel(am2, f2, send_f); }
                // SKEW: the columns of the last row are compared without the part of the frame that moves with the step (tau ext; the rest, (n - 1 - lane) ext, is the same
                // for all columns of the owner lane and is taken off after the loop)
                if constexpr (SKEW) cap2 = pk_sub_i16_s(cap2, sgpr(PK(tau * ext, tau * ext)));
                if (STEADY) {
                    // last query row, first maximum over the columns, as ONE signed maximum per pair of (value << 16 | 0xFFFF - column): equal values keep the larger low
                    // half = the smaller column.  Every lane runs it, only the lane that owns the last row is read (merged into bestRow* after the steady steps).
                    const int jinv = jinv0 - tau;
                    keyRow0 = max(keyRow0, (int)(((unsigned)cap2 << 16) | (unsigned)jinv));
                    keyRow1 = max(keyRow1, (int)(((unsigned)cap2 & 0xFFFF0000u) | (unsigned)jinv));
                } else {   // last query row: first maximum over the columns (of g: the same order as H within a pair)
                    const int v0 = LO16(cap2), v1 = HI16(cap2);
                    const bool b0_ = a0 && lane == own_lane0 && v0 > bestRowV0; bestRowV0 = b0_ ? v0 : bestRowV0; bestRowJ0 = b0_ ? j : bestRowJ0;
                    const bool b1_ = a1 && lane == own_lane1 && v1 > bestRowV1; bestRowV1 = b1_ ? v1 : bestRowV1; bestRowJ1 = b1_ ? j : bestRowJ1;
                }
            };
            const int mmin = m0 < m1 ? m0 : m1;
            const int st_lo = 63 < steps ? 63 : steps, st_hi = mmin > st_lo ? (mmin < steps ? mmin : steps) : st_lo;
            int tau = 0;
            for (; tau < st_lo; ++tau) step(tau, std::false_type{});
            // two steps per iteration: the state a step leaves (one register per row: the new g of the row, while the old one is still the diagonal input of the row below)
            // is consumed by the second step in place, instead of being copied back into the loop's registers after every step (~38 v_mov per step of ~340 instructions)
            for (; tau + 1 < st_hi; tau += 2) { step(tau, std::true_type{}); step(tau + 1, std::true_type{}); }
            for (; tau < st_hi; ++tau) step(tau, std::true_type{});
            if (st_hi > st_lo) {      // the steady steps' maxima join the running ones (their columns lie between those of the ramp-up and of the ramp-down steps)
                const int v0 = keyRow0 >> 16, v1 = keyRow1 >> 16;
                if (lane == own_lane0 && v0 > bestRowV0) { bestRowV0 = v0; bestRowJ0 = 0xFFFF - (keyRow0 & 0xFFFF); }
                if (lane == own_lane1 && v1 > bestRowV1) { bestRowV1 = v1; bestRowJ1 = 0xFFFF - (keyRow1 & 0xFFFF); }
            }
            for (; tau < steps; ++tau) step(tau, std::false_type{});
        };
        switch (own_p) {
#define PCASE(k) case k: if (SKEW ? (nowild && tbl_ok) : nowild) forward(std::integral_constant<int, (R > k ? k : 0)>{}, std::true_type{}); else forward(std::integral_constant<int, (R > k ? k : 0)>{}, std::false_type{}); break;
            PCASE(0) PCASE(1) PCASE(2) PCASE(3) PCASE(4) PCASE(5) PCASE(6) PCASE(7) PCASE(8) PCASE(9) PCASE(10) PCASE(11) PCASE(12) PCASE(13) PCASE(14)
#undef PCASE
            default: if (SKEW ? (nowild && tbl_ok) : nowild) forward(std::integral_constant<int, (R > 15 ? 15 : 0)>{}, std::true_type{}); else forward(std::integral_constant<int, (R > 15 ? 15 : 0)>{}, std::false_type{}); break;
        }
        bestRowV0 += open0 - skx * (n0 - own_lane0); bestRowV1 += open1 - skx * (n1 - own_lane1);      // g -> H (SKEW: g' = H - open + ext, plus the (n - 1 - lane) ext of the frame)
        // last target column of each pair: the state holds g[i][m-1] = H[i][m-1] - open for every row
        int bestColV0 = -(1 << 29), bestColI0 = 0x7fffffff, bestColV1 = -(1 << 29), bestColI1 = 0x7fffffff;
        if constexpr (SKEW) { i0 = lane * R; asm volatile("" : "+v"(i0)); }      // (not kept across the step loops: see above)
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = i0 + r; const int v0 = LO16(hl2[r]) + open0 - skx * (i + m0), v1 = HI16(hl2[r]) + open1 - skx * (i + m1);     // (SKEW: g' of cell (i, m - 1) -> H)
            if (i < n0 && v0 > bestColV0) { bestColV0 = v0; bestColI0 = i; }
            if (i < n1 && v1 > bestColV1) { bestColV1 = v1; bestColI1 = i; }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_s_waitcnt(0);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");

        const AlignJob* Jt = sg_cold_job();
        for (int half = 0; half < 2; ++half) {
            const uint64_t p = half ? p1 : p0; const int n = half ? n1 : n0, m = half ? m1 : m0;
            if (n <= 0) continue;                          // no second pair / degenerate pair (handled above)
            // end cell: the code of sg_end_cell, written out - through the helper the compiler gives R = 4 / 8 one or two more VGPRs (R = 8: one wave less per SIMD)
            int rowV = half ? bestRowV1 : bestRowV0, rowJ = half ? bestRowJ1 : bestRowJ0;
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) { int ov = __shfl_xor(rowV, d), oj = __shfl_xor(rowJ, d); if (ov > rowV) { rowV = ov; rowJ = oj; } }
            int colV = half ? bestColV1 : bestColV0, colI = half ? bestColI1 : bestColI0;
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) { int ov = __shfl_xor(colV, d), oi = __shfl_xor(colI, d); if (ov > colV || (ov == colV && oi < colI)) { colV = ov; colI = oi; } }
            int ei = n - 1, ej = rowJ, best = rowV;
            if (colV > best) { best = colV; ei = colI; ej = m - 1; }
            ei = sgpr(ei); ej = sgpr(ej); best = sgpr(best);
            sg_walk(Jt, Planes<R>{half ? mytb1 : mytb0}, tbblk, half ? qry1 : qry0, half ? tgt1 : tgt0, p, n, m, ei, ej, best, lane);
            __builtin_amdgcn_wave_barrier();
        }
    }
}

template __global__ void k_sg_align16p<4, false>(AlignJob, const uint32_t*, const uint32_t*, const uint32_t*, uint64_t*, uint64_t, uint32_t, uint32_t*);
template __global__ void k_sg_align16p<4, true>(AlignJob, const uint32_t*, const uint32_t*, const uint32_t*, uint64_t*, uint64_t, uint32_t, uint32_t*);
template __global__ void k_sg_align16p<8, false>(AlignJob, const uint32_t*, const uint32_t*, const uint32_t*, uint64_t*, uint64_t, uint32_t, uint32_t*);
template __global__ void k_sg_align16p<8, true>(AlignJob, const uint32_t*, const uint32_t*, const uint32_t*, uint64_t*, uint64_t, uint32_t, uint32_t*);
template __global__ void k_sg_align16p<12, false>(AlignJob, const uint32_t*, const uint32_t*, const uint32_t*, uint64_t*, uint64_t, uint32_t, uint32_t*);
template __global__ void k_sg_align16p<12, true>(AlignJob, const uint32_t*, const uint32_t*, const uint32_t*, uint64_t*, uint64_t, uint32_t, uint32_t*);
template __global__ void k_sg_align16p<14, false>(AlignJob, const uint32_t*, const uint32_t*, const uint32_t*, uint64_t*, uint64_t, uint32_t, uint32_t*);
template __global__ void k_sg_align16p<14, true>(AlignJob, const uint32_t*, const uint32_t*, const uint32_t*, uint64_t*, uint64_t, uint32_t, uint32_t*);
