// k_align16.hip - packed-int16 variant of the semi-global affine aligner (k_align.hip) for sequences <= 4000 bases.
//
// Same DP, same tie-breaks, same outputs (bit-identical to k_sg_align and to the oracle); different mapping:
// a lane owns 2*RP consecutive query rows split in two halves A (rows i0..i0+RP-1) and B (rows i0+RP..i0+2RP-1).
// Register p holds row p of A in its low 16 bits and row p of B in its high 16 bits, and the two halves work one
// column apart (A on column j, B on column j-1), which makes the two 16-bit lanes of every register independent
// cells: all max/add/sub are v_pk_*_i16 (two cells per VALU op).  Traceback flags are derived without compares
// (flag = 1 - min(u16(max - candidate), 1)) and collected in packed accumulators; per step a lane still emits one
// 8-byte word (4 bits per cell, A cells in the low dword, B cells in the high dword).
// The systolic skew is two columns per lane: steps = m + 127 per strip.
// The traceback walk and its bookkeeping are shared with k_sg_align16p (k_align_common.h); the launches and the routing are in k_align.hip.
#include "k_align_common.h"
#include <type_traits>
// traceback layout: the word of cell (i, j) is at strip i / (128 RP), step j + 2 l + h, lane l (h: half B); the cell's nibble sits in the dword of its half,
// accumulator 0 (rows 0 .. C0-1 of the half) in the low 16 bits and accumulator 1 in the high ones, the first row of each in the highest nibble, flags complemented
template <int RP>
struct Nibbles {
    static constexpr int RPL = 2 * RP, STRIP = 64 * RPL, C0 = RP < 4 ? RP : 4, C1 = RP - C0;
    const uint64_t* tb; int steps;
    __device__ SgCell at(int i, int j) const {
        const int sidx = i / STRIP; const int il = i - sidx * STRIP; const int l = il / RPL; const int rr = il - l * RPL;
        return SgCell{sidx * 8 + (l >> 3), j + 2 * l + rr / RP, l & 7, rr};
    }
    __device__ const uint64_t* block(int key, int tt) const { return tb + ((uint64_t)(key >> 3) * steps + (uint64_t)tt) * 64 + (key & 7) * 8; }
    __device__ int flags(uint64_t word, int rr) const {
        const int half = rr / RP, r = rr - half * RP;
        const unsigned w32 = half ? (unsigned)(word >> 32) : (unsigned)word;
        const int sh = r < C0 ? 4 * (C0 - 1 - r) : 16 + 4 * (C1 - 1 - (r - C0));
        return (int)((~(w32 >> sh)) & 15);
    }
};

template <int RP>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 8)))
void k_sg_align16(AlignJob J, uint64_t* __restrict__ tb, uint64_t tb_words_per_wave, int32_t* __restrict__ bnd, uint32_t bnd_stride, uint32_t lds_per_wave, uint32_t* __restrict__ work_ctr)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63;
    const int wib = threadIdx.x >> 6;
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + wib;
    uint8_t* tgt = smem + (size_t)wib * lds_per_wave;
    const uint32_t seq_lds = (lds_per_wave - 4096) / 2;
    uint8_t* qry = tgt + seq_lds;
    uint64_t* tbblk = (uint64_t*)(tgt + 2 * (size_t)seq_lds);
    uint64_t* mytb = tb + wave * tb_words_per_wave;
    int32_t* mybnd = bnd + wave * (uint64_t)bnd_stride * 2;
    constexpr int RPL = 2 * RP;
    constexpr int STRIP = 64 * RPL;
    constexpr int C0 = RP < 4 ? RP : 4;            // pairs collected in accumulator 0
    constexpr int C1 = RP - C0;                     // pairs collected in accumulator 1

    for (;;) {
        // persistent waves pull pairs from a queue: the grid is sized to what is resident, so there is no tail of idle SIMDs
        uint32_t pq = 0; if (lane == 0) pq = atomicAdd(work_ctr, 1u);
        const uint32_t kq = (uint32_t)__builtin_amdgcn_readfirstlane((int)pq);
        if (kq >= (J.npairs_dev ? *J.npairs_dev : (uint32_t)J.npairs)) break;
        const uint64_t p = J.pair_list ? J.pair_list[kq] : kq;
        const uint32_t qi = J.qidx[p], ti = J.tidx[p];
        const uint8_t* q = J.qseq + J.qoff[qi]; const int n = sgpr((int)(J.qoff[qi + 1] - J.qoff[qi]));     // wave-uniform by construction
        const uint8_t* t = J.tseq + J.toff[ti]; const int m = sgpr((int)(J.toff[ti + 1] - J.toff[ti]));
        if (n <= 0 || m <= 0) { sg_degenerate(J, p, n, m, lane); continue; }
        for (int x = lane; x < m; x += 64) tgt[x] = perm_letter(t[x]);
        for (int x = lane; x < n; x += 64) qry[x] = perm_letter(q[x]);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();

        const int OPEN2 = sgpr(PK(J.open[p], J.open[p])), EXT2 = sgpr(PK(J.ext, J.ext));
        const int MATCH2 = PK(J.match, J.match), NDIFF2 = sgpr(PK(J.mismatch - J.match, J.mismatch - J.match));
        const int ONE2 = sgpr(0x00010001);
        const int steps = m + 127;
        const int nstrips = (n + STRIP - 1) / STRIP;
        // owner of the last query row (wave-uniform)
        const int own_il = (n - 1) % STRIP, own_lane = own_il / RPL, own_rr = own_il % RPL, own_half = own_rr / RP, own_p = own_rr % RP;
        int bestRowV = -(1 << 29), bestRowJ = 0;
        int bestColV = -(1 << 29), bestColI = 0x7fffffff;

        // The strip loop is instantiated once per register pair that can hold the LAST query row (wave-uniform own_p): the capture of that row's
        // cell is then a compile-time choice instead of RP selects per step.
        auto strips = [&](auto OPc) {
        constexpr int OWN_P = decltype(OPc)::value;
        for (int sidx = 0; sidx < nstrips; ++sidx) {
            const int i0 = sidx * STRIP + lane * RPL;
            int qc2[RP], nwq2[RP], hl2[RP], e2[RP];
#pragma unroll
            for (int r = 0; r < RP; ++r) {
                const int ia = i0 + r, ib = i0 + RP + r;
                const int ca = ia < n ? qry[ia] : 0x7C, cb = ib < n ? qry[ib] : 0x7C;
                qc2[r] = PK(ca & 3, cb & 3); nwq2[r] = PK((ca & 0x7C) ? 0 : 0xffff, (cb & 0x7C) ? 0 : 0xffff);
                hl2[r] = 0; e2[r] = PK(NEG16, NEG16);
            }
            int hdiagA = 0;                              // H[i0-1][jA-1]
            int aBot_h1 = 0, aBot_h2 = 0, aBot_f1 = NEG16; // A's bottom row at columns jA-1 (H,F) and jA-2 (H)
            int send_h = 0, send_f = NEG16;               // B's bottom row for the next lane
            const bool last_strip = sidx + 1 == nstrips;
            uint64_t* stb = mytb + (uint64_t)sidx * steps * 64;
            int tc2 = 0, nwt2 = 0, am2 = 0;              // target letter / not-wildcard mask / active mask: low half = A now, high half = A one step ago = B now
            for (int tau = 0; tau < steps; ++tau) {
                const int jA = tau - 2 * lane, jB = jA - 1;
                int hupA = __builtin_amdgcn_update_dpp(0, send_h, 0x138, 0xf, 0xf, false), fupA = __builtin_amdgcn_update_dpp(0, send_f, 0x138, 0xf, 0xf, false);
                const bool actA = jA >= 0 && jA < m;
                const bool actB = am2 & 1;                // A was active one step ago <=> column jB is inside the matrix
                if (lane == 0) {
                    if (sidx == 0) { hupA = 0; fupA = NEG16; }
                    else if (actA) { hupA = __hip_atomic_load(&mybnd[jA], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); fupA = __hip_atomic_load(&mybnd[bnd_stride + jA], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
                }
                // no early exit and no branches on activity: inactive halves are masked out of the state updates
                const int pA = tgt[actA ? jA : 0];
                tc2 = (tc2 << 16) | (pA & 3);
                nwt2 = (nwt2 << 16) | ((actA && !(pA & 0x7C)) ? 0xffff : 0);
                am2 = (am2 << 16) | (actA ? 0xffff : 0);
                int hu2 = PK(hupA, aBot_h1), f2 = PK(fupA, aBot_f1), hd2 = PK(hdiagA, aBot_h2);
                int acc0 = 0, acc1 = 0, cap2 = 0;
#pragma unroll
                for (int r = 0; r < RP; ++r) {
                    const int e_ext = pk_sub_i16_s(e2[r], EXT2), e_opn = pk_sub_i16_s(hl2[r], OPEN2); const int E = pk_max_i16(e_ext, e_opn);
                    const int f_ext = pk_sub_i16_s(f2, EXT2), f_opn = pk_sub_i16_s(hu2, OPEN2); const int F = pk_max_i16(f_ext, f_opn);
                    const int z = pk_min_u16_s(qc2[r] ^ tc2, ONE2);                                // 1 = letters differ
                    const int sc = pk_mad_i16_sv(z, NDIFF2, MATCH2) & nwq2[r] & nwt2;              // match / mismatch / 0 for wildcards
                    const int d = pk_add_i16(hd2, sc);
                    const int m1 = pk_max_i16(E, F); const int h = pk_max_i16(d, m1);
                    // COMPLEMENT flags (1 = "not equal"): bit0 h!=d, bit1 m1!=E (i.e. F>E), bit2 E!=e_ext (opened), bit3 F!=f_ext (opened).
                    // Every half holds 0/1, so plain 32-bit shifts by <= 3 stay inside their half.
                    int c = pk_min_u16_s(pk_sub_u16(h, d), ONE2);
                    c |= pk_min_u16_s(pk_sub_u16(m1, E), ONE2) << 1;
                    c |= pk_min_u16_s(pk_sub_u16(E, e_ext), ONE2) << 2;
                    c |= pk_min_u16_s(pk_sub_u16(F, f_ext), ONE2) << 3;
                    if (r < C0) acc0 = (acc0 << 4) | c; else acc1 = (acc1 << 4) | c;                // never crosses a 16-bit half: <= 4 nibbles each
                    hd2 = hl2[r];
                    hl2[r] = (h & am2) | (hl2[r] & ~am2);
                    e2[r] = E;       // not masked: before a lane's first column E only relaxes to H - open = -open (what the first real column computes from
                                     // the boundary anyway: same value, same 'opened' flag), after its last column E is not used again
                    hu2 = h; f2 = F;
                    if (r == OWN_P) cap2 = h;
                }
                // traceback word: A cells low dword, B cells high dword (complement nibbles); words of inactive steps are never read
                const unsigned wA = ((unsigned)acc0 & 0xffffu) | ((unsigned)acc1 << 16), wB = ((unsigned)acc0 >> 16) | ((unsigned)acc1 & 0xffff0000u);
                stb[(uint64_t)tau * 64 + lane] = (uint64_t)wA | ((uint64_t)wB << 32);
                const int botA_h = LO16(hu2), botA_f = LO16(f2), botB_h = HI16(hu2), botB_f = HI16(f2);
                aBot_h2 = actA ? aBot_h1 : aBot_h2; aBot_h1 = actA ? botA_h : aBot_h1; aBot_f1 = actA ? botA_f : aBot_f1; hdiagA = actA ? hupA : hdiagA;
                send_h = actB ? botB_h : send_h; send_f = actB ? botB_f : send_f;
                if (!last_strip) {
                    if (actB && lane == 63) {
                        __hip_atomic_store(&mybnd[jB], botB_h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        __hip_atomic_store(&mybnd[bnd_stride + jB], botB_f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                } else {
                    const int v = own_half ? HI16(cap2) : LO16(cap2); const bool act = (own_half ? actB : actA) && lane == own_lane; const int jj = own_half ? jB : jA;
                    const bool better = act && v > bestRowV;
                    bestRowV = better ? v : bestRowV; bestRowJ = better ? jj : bestRowJ;
                }
            }
            // last target column: the state now holds H[i][m-1] for every row of the strip
#pragma unroll
            for (int r = 0; r < RP; ++r) { const int ia = i0 + r; const int v = LO16(hl2[r]); if (ia < n && v > bestColV) { bestColV = v; bestColI = ia; } }
#pragma unroll
            for (int r = 0; r < RP; ++r) { const int ib = i0 + RP + r; const int v = HI16(hl2[r]); if (ib < n && v > bestColV) { bestColV = v; bestColI = ib; } }
            if (nstrips > 1) { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent"); __builtin_amdgcn_s_waitcnt(0); }
        }
        };
        switch (own_p) {
            case 0: strips(std::integral_constant<int, 0>{}); break;
            case 1: strips(std::integral_constant<int, (RP > 1 ? 1 : 0)>{}); break;
            case 2: strips(std::integral_constant<int, (RP > 2 ? 2 : 0)>{}); break;
            case 3: strips(std::integral_constant<int, (RP > 3 ? 3 : 0)>{}); break;
            case 4: strips(std::integral_constant<int, (RP > 4 ? 4 : 0)>{}); break;
            case 5: strips(std::integral_constant<int, (RP > 5 ? 5 : 0)>{}); break;
            case 6: strips(std::integral_constant<int, (RP > 6 ? 6 : 0)>{}); break;
            default: strips(std::integral_constant<int, (RP > 7 ? 7 : 0)>{}); break;
        }
        int ei, ej, best;
        sg_end_cell(bestRowV, bestRowJ, bestColV, bestColI, n, m, ei, ej, best);

        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_s_waitcnt(0);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");

        sg_walk(sg_cold_job(), Nibbles<RP>{mytb, steps}, tbblk, qry, tgt, p, n, m, ei, ej, best, lane);
        __builtin_amdgcn_wave_barrier();
    }
}

template __global__ void k_sg_align16<2>(AlignJob, uint64_t*, uint64_t, int32_t*, uint32_t, uint32_t, uint32_t*);
template __global__ void k_sg_align16<4>(AlignJob, uint64_t*, uint64_t, int32_t*, uint32_t, uint32_t, uint32_t*);
template __global__ void k_sg_align16<6>(AlignJob, uint64_t*, uint64_t, int32_t*, uint32_t, uint32_t, uint32_t*);
template __global__ void k_sg_align16<7>(AlignJob, uint64_t*, uint64_t, int32_t*, uint32_t, uint32_t, uint32_t*);
template __global__ void k_sg_align16<8>(AlignJob, uint64_t*, uint64_t, int32_t*, uint32_t, uint32_t, uint32_t*);
