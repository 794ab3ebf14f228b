// k_align_common.h - device code shared by the semi-global affine aligners (k_align.hip, k_align16.hip, k_align16p.hip):
// the packed 16-bit helpers of the two int16 kernels, the traceback bookkeeping of all three (k-column windows, end gaps, result store, end cell, empty pairs)
// and the wave-parallel traceback walk of the int16 kernels.  The host side (plans, launches, routing) is in k_align.hip.
#pragma once
#include "ngsid_internal.h"

// the int16 kernels (launched from k_align.hip; the instances are instantiated in their own files)
template <int RP> __global__ void k_sg_align16(AlignJob J, uint64_t* tb, uint64_t tb_words_per_wave, int32_t* bnd, uint32_t bnd_stride, uint32_t lds_per_wave, uint32_t* work_ctr);
#define PBINS 32          // bins of one length class of the paired kernel: residues (n - 1) mod R, R <= 16 (the rest unused)
template <int R, bool SKEW> __global__ void k_sg_align16p(AlignJob J, const uint32_t* sorted, const uint32_t* bin_off, const uint32_t* item_off, uint64_t* tb, uint64_t tb_words_per_wave, uint32_t seq_lds, uint32_t* work_ctr);

// ---- packed 16-bit helpers
#define NEG16 (-20000)
// Paired kernel: bound on the magnitude of a difference of two values of one DP cell, the "minus infinity" NEG16 included (its traceback flags are sign bits of such
// differences, so the bound must stay below 2^15).  skew: the instances that keep cell (i, j) in the frame X + (i + j) ext, which lifts the largest value by the frame
// of the last cell (derivation at the top of k_align16p.hip).  Shared by the kernel's static_asserts and the host's choice of the instance.
constexpr long long sg16p_flag_span(int match, int ext, int open, long long qlen, long long tlen, bool skew)
{
    return -(long long)(NEG16) + ext + open + match * (qlen < tlen ? qlen : tlen) + (skew ? (qlen + tlen + 1) * ext : 0);
}
// Packed 16-bit VALU ops through inline asm: with plain vector types the compiler "simplifies" the flag arithmetic back into
// per-half compares + selects (no packed compare exists), which costs more than the 32-bit kernel.
#define PKOP2(name, mnem) __device__ __forceinline__ int name(int a, int b) { int d; asm(mnem " %0, %1, %2" : "=v"(d) : "v"(a), "v"(b)); return d; }
PKOP2(pk_sub_i16, "v_pk_sub_i16")
PKOP2(pk_add_i16, "v_pk_add_i16")
PKOP2(pk_max_i16, "v_pk_max_i16")
PKOP2(pk_sub_u16, "v_pk_sub_u16")
// second operand wave-uniform (lives in an SGPR: one constant-bus read per instruction is allowed on gfx9)
#define PKOP2S(name, mnem) __device__ __forceinline__ int name(int a, int b) { int d; asm(mnem " %0, %1, %2" : "=v"(d) : "v"(a), "s"(b)); return d; }
PKOP2S(pk_sub_i16_s, "v_pk_sub_i16")
PKOP2S(pk_min_u16_s, "v_pk_min_u16")
__device__ __forceinline__ int pk_mad_i16_sv(int a, int b_s, int c) { int d; asm("v_pk_mad_i16 %0, %1, %2, %3" : "=v"(d) : "v"(a), "s"(b_s), "v"(c)); return d; }
__device__ __forceinline__ int sgpr(int x) { return __builtin_amdgcn_readfirstlane(x); }
// Staged letters are stored through a byte PERMUTATION that sends A,C,G,T to 0..3 and a,c,g,t to 0x80..0x83 (and those eight
// byte values back to the letters), so raw-character equality is preserved and the DP loop decodes with two ANDs.
__device__ __forceinline__ uint8_t perm_letter(uint8_t c) {
    const int b = ngsid_bcode(c);
    if (b < 4) return (uint8_t)(b | ((c & 0x20) ? 0x80 : 0));
    if ((c & 0x7C) == 0) { const int x = c & 3; const int up = x == 0 ? 'A' : x == 1 ? 'C' : x == 2 ? 'G' : 'T'; return (uint8_t)((c & 0x80) ? (up | 0x20) : up); }
    return c;
}
__device__ __forceinline__ int PK(int lo, int hi) { return (lo & 0xffff) | (hi << 16); }
__device__ __forceinline__ int LO16(int x) { return (int)(short)(x & 0xffff); }
__device__ __forceinline__ int HI16(int x) { return x >> 16; }

// ---- traceback bookkeeping (all three kernels)

// break points of a pair: every record -1 (none) until the walk fills it in
__device__ __forceinline__ void sg_bp_clear(const AlignJob& J, uint64_t p, int lane)
{
    if (J.bp) for (int x = lane; x < J.bp_windows * 4; x += 64) J.bp[p * (uint64_t)J.bp_windows * 4 + x] = -1;
}

__device__ __forceinline__ void sg_store(const AlignJob& J, uint64_t p, int lane, int score, int cols, int nm, int region, int q_beg, int q_end, int t_beg, int t_end)
{
    if (lane == 0) {
        if (J.score) J.score[p] = score;
        if (J.ncols) J.ncols[p] = cols;
        if (J.nmatch) J.nmatch[p] = nm;
        if (J.region) J.region[p] = region;
        if (J.span) { J.span[p * 4 + 0] = q_beg; J.span[p * 4 + 1] = q_end; J.span[p * 4 + 2] = t_beg; J.span[p * 4 + 3] = t_end; }
    }
}

// an empty query or target: n + m gap columns, no DP
__device__ __forceinline__ void sg_degenerate(const AlignJob& J, uint64_t p, int n, int m, int lane)
{
    if (lane == 0) {
        const int cols = n + m; const int mid = J.match_id ? J.match_id[p] : J.k;
        sg_store(J, p, lane, 0, cols, 0, (cols <= J.k) ? (0 >= mid) : ((0 >= mid) ? cols - J.k + 1 : 0), 0, 0, 0, 0);
    }
    sg_bp_clear(J, p, lane);
}

// k-column identity windows (cluster.py:130-169), folded on the fly while the traceback walks the path backwards (the window count is symmetric under
// path reversal): the match bits of the last K columns in a 64-bit shift register, region = windows with at least mid matches
struct SgWindows {
    int K, mid; uint64_t kmask; uint64_t win = 0; int cols = 0, nm = 0, region = 0;
    __device__ SgWindows(int K_, int mid_) : K(K_), mid(mid_), kmask((K_ >= 64) ? ~0ull : ((1ull << K_) - 1)) {}
    __device__ void push(int bit) { win = (win << 1) | (uint64_t)bit; nm += bit; ++cols; if (cols >= K) region += ((int)__popcll(win & kmask) >= mid); }
    __device__ void end_gaps(int z) {
        const int zl = z < K ? z : K;             // after K zeros the window is all zero
        for (int x = 0; x < zl; ++x) { win <<= 1; ++cols; if (cols >= K) region += ((int)__popcll(win & kmask) >= mid); }
        if (z > zl) { region += (0 >= mid) ? (z - zl) : 0; cols += z - zl; }
    }
    __device__ int windows() const { return cols < K ? ((nm >= mid) ? 1 : 0) : region; }      // a single, shorter window (cluster.py:148-154)
};

// end cell: first maximum over the last row (lowest column), then a strictly larger one over the last column (lowest row); the lanes hold partial maxima
__device__ __forceinline__ void sg_end_cell(int rowV, int rowJ, int colV, int colI, int n, int m, int& ei, int& ej, int& best)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { int ov = __shfl_xor(rowV, d), oj = __shfl_xor(rowJ, d); if (ov > rowV) { rowV = ov; rowJ = oj; } }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { int ov = __shfl_xor(colV, d), oi = __shfl_xor(colI, d); if (ov > colV || (ov == colV && oi < colI)) { colV = ov; colI = oi; } }
    ei = n - 1; ej = rowJ; best = rowV;
    if (colV > best) { best = colV; ei = colI; ej = m - 1; }
}

// The fields of the job description that only the traceback needs are read from the kernel-argument segment (the AlignJob is the first argument),
// through a pointer the compiler cannot see through: kept in SGPRs across the step loops they pushed loop-invariant exec masks into VGPR lanes
// (18 v_readlane reloads per DP step of k_sg_align16, 8 % of its VALU work).  Call it after the step loops.
__device__ __forceinline__ const AlignJob* sg_cold_job()
{
    const AlignJob* Jt = (const AlignJob*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(Jt));
    return Jt;
}

// ---- wave-parallel traceback walk of the int16 kernels, from the end cell (ei, ej), uniform over the wave.  Traceback words are pulled 64 steps x 8 lanes
// (4 KB) at a time into LDS (tbblk): one HBM round trip per ~64 path steps.  The layout policy Lay says where the word of a cell lives and how its flags are packed:
//   Lay::at(i, j)         -> SgCell of cell (i, j)
//   Lay::block(key, tt)   -> the 8 words of step tt of block `key` in HBM
//   Lay::flags(word, sub) -> the cell's flags: bit0 diagonal, bit1 E >= F, bit2 E extends, bit3 F extends
struct SgCell { int key, tau, col, sub; };      // block key (strip and group of 8 lanes), step, lane in the group, position in the word
template <class Lay>
__device__ __forceinline__ void sg_walk(const AlignJob* Jt, const Lay& L, uint64_t* tbblk, const uint8_t* qry, const uint8_t* tgt, uint64_t p, int n, int m, int ei, int ej, int best, int lane)
{
    sg_bp_clear(*Jt, p, lane);
    const int K = Jt->k; SgWindows w(K, Jt->match_id ? Jt->match_id[p] : K);
    w.end_gaps((n - 1 - ei) + (m - 1 - ej));     // trailing end gaps (walked first)
    int i = ei, j = ej, state = 0;
    int q_end = -1, t_end = -1, q_beg = -1, t_beg = -1;
    // polishing-window break points: per window of target columns {first query row, last query row, first column, last column} of the diagonal cells
    int cw = -1, w_qf = 0, w_ql = 0, w_tf = 0, w_tl = 0;
    int32_t* bpp = Jt->bp ? Jt->bp + p * (uint64_t)Jt->bp_windows * 4 : nullptr;
    int blk_key = -1, blk_hi = -1;
    // polishing window of the current column, tracked incrementally (no divisions in the loop): [ws, ws + window), index wsn
    int wsn = bpp ? j / Jt->window : 0, ws = bpp ? wsn * Jt->window : 0;
    // (every round of the walk takes at least one step or reloads a block once per 64 steps: the bound is never reached; it turns a corrupted traceback word into a wrong
    // result the parity tests catch instead of a wave that never ends)
    for (int guard = 4 * (n + m) + 512; i >= 0 && j >= 0 && guard > 0; --guard) {
        if (bpp) while (j < ws) { ws -= Jt->window; --wsn; }
        {   // make sure the block of traceback words around the current cell is in LDS (64 steps x one group of 8 lanes)
            const SgCell c = L.at(i, j);
            if (c.key != blk_key || c.tau > blk_hi || c.tau < blk_hi - 63) {
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                blk_key = c.key; blk_hi = c.tau;
                const int tt = c.tau - lane;
                if (tt >= 0) {
                    const uint4* src = (const uint4*)L.block(c.key, tt);
                    ngsid_v4u* dstp = (ngsid_v4u*)(tbblk + lane * 8);
                    // nt loads are served by L2: this wave rewrites the same scratch addresses for every pair, an L1 line may be stale
                    dstp[0] = ngsid_load16_l2(src + 0); dstp[1] = ngsid_load16_l2(src + 1); dstp[2] = ngsid_load16_l2(src + 2); dstp[3] = ngsid_load16_l2(src + 3);
                }
                asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_wave_barrier();
            }
        }
        // lane k decodes the cell k diagonal steps back; in state 0 the wave takes the whole leading run of diagonal moves at once
        // (most of an alignment of similar sequences), then the first other cell is handled by the serial state machine below
        const int ik = i - lane, jk = j - lane;
        bool inb = false; int vk = 0;
        if (ik >= 0 && jk >= 0) {
            const SgCell c = L.at(ik, jk);
            if (c.key == blk_key && c.tau <= blk_hi && c.tau >= blk_hi - 63) { vk = L.flags(tbblk[(blk_hi - c.tau) * 8 + c.col], c.sub); inb = true; }
        }
        int run = 0;
        if (state == 0) {
            const bool good = inb && (vk & 1) && jk >= ws;          // a run never crosses a polishing-window boundary
            const unsigned long long gm = __ballot(good);
            run = (~gm) ? __builtin_ctzll(~gm) : 64;
        }
        if (run > 0) {
            const unsigned long long mb = __ballot(ik >= 0 && jk >= 0 && qry[ik >= 0 ? ik : 0] == tgt[jk >= 0 ? jk : 0]);      // match bit of step k
            const unsigned long long rmask = run == 64 ? ~0ull : ((1ull << run) - 1);
            // window after step k: the k+1 new bits enter in step order (step 0 ends up highest)
            const uint64_t wk = (lane == 63 ? 0ull : (w.win << (lane + 1))) | (__brevll(mb) >> (63 - lane));
            const bool cnt = (w.cols + lane + 1 >= w.K) && ((int)__popcll(wk & w.kmask) >= w.mid);
            w.region += (int)__popcll(__ballot(cnt) & rmask);
            w.nm += (int)__popcll(mb & rmask);
            { const int last = run - 1; const unsigned lo_ = __builtin_amdgcn_readlane((unsigned)wk, last), hi_ = __builtin_amdgcn_readlane((unsigned)(wk >> 32), last); w.win = ((uint64_t)hi_ << 32) | lo_; }
            w.cols += run;
            if (q_end < 0) { q_end = i; t_end = j; }
            q_beg = i - run + 1; t_beg = j - run + 1;
            if (bpp) {
                if (wsn != cw) { if (lane == 0 && cw >= 0 && cw < Jt->bp_windows) { bpp[cw * 4 + 0] = w_qf; bpp[cw * 4 + 1] = w_ql; bpp[cw * 4 + 2] = w_tf; bpp[cw * 4 + 3] = w_tl; } cw = wsn; w_ql = i; w_tl = j; }
                w_qf = i - run + 1; w_tf = j - run + 1;
            }
            i -= run; j -= run;
            if (i < 0 || j < 0) break;
            if (bpp) while (j < ws) { ws -= Jt->window; --wsn; }
        }
        if (run == 64 || !((__ballot(inb) >> run) & 1)) continue;     // next cell outside the loaded block: go round (reloads)
        const int v = __builtin_amdgcn_readlane(vk, run);
        int bit = 0, emit = 1;
        if (state == 0) {
            if (v & 1) {                                       // (a diagonal move the run could not take: window boundary)
                bit = (qry[i] == tgt[j]);
                if (q_end < 0) { q_end = i; t_end = j; }
                q_beg = i; t_beg = j;
                if (bpp) {
                    if (wsn != cw) { if (lane == 0 && cw >= 0 && cw < Jt->bp_windows) { bpp[cw * 4 + 0] = w_qf; bpp[cw * 4 + 1] = w_ql; bpp[cw * 4 + 2] = w_tf; bpp[cw * 4 + 3] = w_tl; } cw = wsn; w_ql = i; w_tl = j; }
                    w_qf = i; w_tf = j;
                }
                --i; --j;
            } else { state = (v & 2) ? 1 : 2; emit = 0; }
        } else if (state == 1) { if (!((v >> 2) & 1)) state = 0; --j; }
        else { if (!((v >> 3) & 1)) state = 0; --i; }
        if (emit) w.push(bit);
    }
    if (lane == 0 && bpp && cw >= 0 && cw < Jt->bp_windows) { bpp[cw * 4 + 0] = w_qf; bpp[cw * 4 + 1] = w_ql; bpp[cw * 4 + 2] = w_tf; bpp[cw * 4 + 3] = w_tl; }
    w.end_gaps((i + 1) + (j + 1));                     // leading end gaps
    sg_store(*Jt, p, lane, best, w.cols, w.nm, w.windows(), q_beg, q_end, t_beg, t_end);
}
