// k_chimera.hip - ngsid_chimera_model (include/ngsid_chimera.h): for every (query, parent) pair the best cost of every query prefix and of every query suffix
// against the parent, and per query the best one-parent and the best two-parent model.
//
// k_chimera_profile: persistent waves (one per workgroup) pull PAIRS from a counter.  The two directions of a pair - (q, p) and (reversed q, reversed p) - have the same
//   rectangle, so they run as the low and the high half of one packed uint16 DP: every v_pk_* op computes one cell of each (what the two-halves-one-column-apart packing
//   of k_align16 buys, without its skew: no half waits for the other).  The query is staged in LDS as one 16-bit entry per column (forward letter | reversed letter << 8;
//   queries above NGSID_CHIMERA_LDS_QUERY bases are read through the caches instead); the parent's letters are read once per strip, straight into the registers of the lane
//   that owns the rows.  Systolic: lane l owns the R = NGSID_CHIMERA_ROWS consecutive parent rows jb + l R + 1 .. jb + (l + 1) R of the strip and works one query column
//   behind lane l - 1.  A lane hands to its successor, by one DPP shift each, the bottom cell of its column AND the running minimum of that column over all rows above
//   (row 0 and the earlier strips included); the successor folds its own rows in.  No reduction across lanes per column: the lane that owns the strip's last parent row
//   holds min over j of D[j][i] when it finishes column i and stores F[i] (low half) and B[n - i] (high half).
//   Rows behind the parent's end need no mask: they hold a letter (0xFF) that equals nothing, and a parent extended by letters that match nothing cannot be closer to
//   any query prefix than the parent itself (drop the extra letters from an alignment: every one of them cost 1 as a deletion or as a substitution, which becomes an
//   insertion of the same cost), so their cells never lower the minimum.
//   Parents above one strip (64 R rows) run in further strips: a global boundary array per wave carries the bottom row and the running minimum per column (in place:
//   column i is read 63 steps before it is rewritten); it is read 64 columns at a time, one block ahead.  No traceback is kept.  Values stay below
//   NGSID_MAX_CONSENSUS_LEN + 64 R < 2^16.
// k_chimera_reduce: one wave per query, lanes over the positions i.  At each i one pass over the query's pairs keeps, for F and for B, the best (value, pair) by
//   (value, pair index) and the best pair whose gid differs from the best's ("second").  The two-parent minimum at i, tie rules included, is among the four
//   combinations {F best, F second} x {B best, B second} with different gids:
//     1. if gid(F best) != gid(B best), that pair has the smallest value of either term and the smallest index attaining each: it is the answer;
//     2. else g = their common gid; an admissible (a, b) has gid(a) != g - then F_a >= F second, B_b >= B best, and (F second, B best) is admissible with the smallest
//        indices attaining both bounds - or gid(a) == g, so gid(b) != g - then F_a >= F best, B_b >= B second, likewise for (F best, B second);
//     3. the smallest (value, a, b) over the two classes is therefore the smallest over those candidates, all of which are admissible.
//   The lanes keep their smallest (value, i), a butterfly picks the wave's; a second pass over the winning pair's two profiles gives bp_hi.
#include "ngsid_host.h"
#include "../../include/ngsid_chimera.h"
#include <algorithm>

typedef uint64_t u64;

#define CHM_R NGSID_CHIMERA_ROWS
#define CHM_STRIP NGSID_CHIMERA_STRIP
#define CHM_QCAP NGSID_CHIMERA_LDS_QUERY
#define CHM_INF 0x7fffffff

static_assert(NGSID_MAX_CONSENSUS_LEN + CHM_STRIP < 65536, "cell values (at most max(column, row) of a padded strip) must fit uint16");
static_assert(NGSID_CHIMERA_NFIELD == 7, "k_chimera_reduce writes seven fields");

namespace {

// packed uint16 ops through inline asm (k_align_common.h: plain vector types are turned back into per-half code)
#define CHM_PK2(name, mnem) __device__ __forceinline__ int name(int a, int b) { int d; asm(mnem " %0, %1, %2" : "=v"(d) : "v"(a), "v"(b)); return d; }
#define CHM_PK2S(name, mnem) __device__ __forceinline__ int name(int a, int b) { int d; asm(mnem " %0, %1, %2" : "=v"(d) : "v"(a), "s"(b)); return d; }
CHM_PK2(chm_add, "v_pk_add_u16")
CHM_PK2(chm_min, "v_pk_min_u16")
CHM_PK2S(chm_add_s, "v_pk_add_u16")
CHM_PK2S(chm_min_s, "v_pk_min_u16")
__device__ __forceinline__ int chm_pk(int x) { return (x & 0xffff) | (x << 16); }
__device__ __forceinline__ int chm_shr1(int x) { return __builtin_amdgcn_update_dpp(0, x, 0x138, 0xf, 0xf, false); }      // lane l receives lane l - 1's value

__global__ __launch_bounds__(64)
void k_chimera_profile(const uint8_t* __restrict__ qseq, const uint64_t* __restrict__ qoff, const uint8_t* __restrict__ pseq, const uint64_t* __restrict__ poff,
                       const uint32_t* __restrict__ pair_q, const uint32_t* __restrict__ pair_parent, const uint64_t* __restrict__ prof_off, u64 v0, uint32_t npairs,
                       uint16_t* __restrict__ prof, uint32_t* bnd, uint32_t bnd_stride, uint32_t* work_ctr)
{
    __shared__ uint16_t qs[CHM_QCAP];
    const int lane = threadIdx.x;
    uint32_t* bot = bnd + (size_t)blockIdx.x * 2 * bnd_stride;       // bottom row of the strip before, per column
    uint32_t* bmn = bot + bnd_stride;                                 // running column minimum down to that row
    const int ONE2 = __builtin_amdgcn_readfirstlane(0x00010001);
    for (;;) {
        uint32_t pq = 0; if (lane == 0) pq = atomicAdd(work_ctr, 1u);
        const uint32_t k = (uint32_t)__builtin_amdgcn_readfirstlane((int)pq);
        if (k >= npairs) break;
        const uint32_t qi = pair_q[k], pi = pair_parent[k];
        const uint8_t* q = qseq + qoff[qi]; const int n = __builtin_amdgcn_readfirstlane((int)(qoff[qi + 1] - qoff[qi]));
        const uint8_t* p = pseq + poff[pi]; const int m = __builtin_amdgcn_readfirstlane((int)(poff[pi + 1] - poff[pi]));
        uint16_t* F = prof + (prof_off[k] - v0); uint16_t* B = F + (n + 1);
        if (lane == 0) { F[0] = 0; B[n] = 0; }                         // column 0: D[j][0] = j
        if (m == 0) {                                                   // ed(q[0:i], "") = i
            for (int i = lane + 1; i <= n; i += 64) { F[i] = (uint16_t)i; B[n - i] = (uint16_t)i; }
            continue;
        }
        const bool ldsq = n <= CHM_QCAP;
        __syncthreads();                                                // (one wave: orders the LDS reads of the pair before against these writes)
        if (ldsq) for (int x = lane; x < n; x += 64) qs[x] = (uint16_t)(q[x] | ((uint32_t)q[n - 1 - x] << 8));
        __syncthreads();
        // letters of column i (1-based): forward letter in the low half, reversed letter in the high half
        auto letters = [&](int i) -> int {
            if (i < 1 || i > n) return 0;
            const uint32_t v = ldsq ? (uint32_t)qs[i - 1] : ((uint32_t)q[i - 1] | ((uint32_t)q[n - i] << 8));
            return (int)((v & 0xffu) | ((v & 0xff00u) << 8));
        };
        const int nstrips = (m + CHM_STRIP - 1) / CHM_STRIP;
        for (int s = 0; s < nstrips; ++s) {
            const int jb = s * CHM_STRIP, row0 = jb + lane * CHM_R;    // this lane: rows row0 + 1 .. row0 + R
            const int rows_here = min(m - jb, CHM_STRIP);
            const int wl = (rows_here - 1) / CHM_R;                    // the lane that owns the strip's last parent row (uniform)
            const bool last = s + 1 == nstrips;
            int pc[CHM_R], prev[CHM_R];
#pragma unroll
            for (int r = 0; r < CHM_R; ++r) {
                const int j = row0 + 1 + r;
                const int cf = j <= m ? p[j - 1] : 0xFF, cr = j <= m ? p[m - j] : 0xFF;
                pc[r] = cf | (cr << 16); prev[r] = chm_pk(j);
            }
            int top_prev = chm_pk(row0);                               // D[row0][column - 1]
            int out_b = 0, out_m = 0;                                  // what the next lane takes: bottom cell and running minimum of the column just finished
            int cur_b = 0, cur_m = 0, nxt_b = 0, nxt_m = 0;            // boundary columns (t & ~63) + 1 + lane, and the block after
            if (s > 0 && 1 + lane <= n) {
                nxt_b = (int)__hip_atomic_load(&bot[1 + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                nxt_m = (int)__hip_atomic_load(&bmn[1 + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            int qn = letters(1 - lane);
            const int steps = n + wl;
            for (int t = 0; t < steps; ++t) {
                const int i = t - lane + 1;                            // this lane's column
                int top = chm_shr1(out_b), rmin = chm_shr1(out_m);
                if (s == 0) { if (lane == 0) { top = chm_pk(i); rmin = top; } }      // row 0: D[0][i] = i
                else {
                    if ((t & 63) == 0) {
                        cur_b = nxt_b; cur_m = nxt_m;
                        const int col = t + 65 + lane;
                        if (col <= n) {
                            nxt_b = (int)__hip_atomic_load(&bot[col], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            nxt_m = (int)__hip_atomic_load(&bmn[col], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        }
                    }
                    const int tb = __builtin_amdgcn_readlane(cur_b, t & 63), tm = __builtin_amdgcn_readlane(cur_m, t & 63);
                    if (lane == 0) { top = tb; rmin = tm; }
                }
                const int qc = qn;
                qn = letters(i + 1);
                if (i >= 1 && i <= n) {
                    int diag = top_prev, up = top;
#pragma unroll
                    for (int r = 0; r < CHM_R; ++r) {
                        const int ne = chm_min_s(pc[r] ^ qc, ONE2);                                  // 1 = letters differ
                        const int d = chm_min(chm_add(diag, ne), chm_add_s(chm_min(up, prev[r]), ONE2));
                        diag = prev[r]; prev[r] = d; up = d;
                        rmin = chm_min(rmin, d);
                    }
                    top_prev = top; out_b = up; out_m = rmin;
                    if (lane == wl) {
                        if (last) { F[i] = (uint16_t)(rmin & 0xffff); B[n - i] = (uint16_t)((uint32_t)rmin >> 16); }
                        else { __hip_atomic_store(&bot[i], (uint32_t)up, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); __hip_atomic_store(&bmn[i], (uint32_t)rmin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
                    }
                }
            }
        }
    }
}

// best (value, pair) by (value, pair index) and the best pair of another gid; pairs arrive in ascending index order
struct ChmTop {
    int v1 = CHM_INF, k1 = -1, g1 = 0, v2 = CHM_INF, k2 = -1, g2 = 0;
    __device__ __forceinline__ void add(int v, int k, int g) {
        if (v < v1) { if (g != g1 || k1 < 0) { v2 = v1; k2 = k1; g2 = g1; } v1 = v; k1 = k; g1 = g; }
        else if (g != g1 && v < v2) { v2 = v; k2 = k; g2 = g; }
    }
};

__global__ __launch_bounds__(64)
void k_chimera_reduce(const uint64_t* __restrict__ qoff, u64 q0, const uint64_t* __restrict__ pair_off, u64 pair0, const uint64_t* __restrict__ prof_off, u64 v0,
                      const int32_t* __restrict__ gid, const uint16_t* __restrict__ prof, int32_t* __restrict__ fields)
{
    const int lane = threadIdx.x;
    const u64 q = q0 + blockIdx.x;
    const u64 a0 = pair_off[q];
    const int P = (int)(pair_off[q + 1] - a0);
    const int n = (int)(qoff[q + 1] - qoff[q]);
    int32_t* o = fields + q * NGSID_CHIMERA_NFIELD;
    if (P == 0) { if (lane < NGSID_CHIMERA_NFIELD) o[lane] = -1; return; }
    const size_t blk = 2 * ((size_t)n + 1);
    const uint16_t* base = prof + (prof_off[a0 - pair0] - v0);                // the query's blocks are contiguous
    const int32_t* g = gid + (a0 - pair0);
    int bc = CHM_INF, bi = CHM_INF, ba = -1, bb = -1;
    for (int i = lane; i <= n; i += 64) {
        ChmTop f, b;
        for (int k = 0; k < P; ++k) {
            const int gk = g[k];
            f.add(base[(size_t)k * blk + i], k, gk);
            b.add(base[(size_t)k * blk + (n + 1) + i], k, gk);
        }
        if (i == n) { o[0] = f.k1; o[1] = f.v1; }
        int cv = CHM_INF, ca = -1, cb = -1;
        auto cand = [&](int fv, int fk, int fg, int bv, int bk, int bg) {
            if (fk < 0 || bk < 0 || fg == bg) return;
            const int v = fv + bv;
            if (v < cv || (v == cv && (fk < ca || (fk == ca && bk < cb)))) { cv = v; ca = fk; cb = bk; }
        };
        cand(f.v1, f.k1, f.g1, b.v1, b.k1, b.g1); cand(f.v1, f.k1, f.g1, b.v2, b.k2, b.g2);
        cand(f.v2, f.k2, f.g2, b.v1, b.k1, b.g1); cand(f.v2, f.k2, f.g2, b.v2, b.k2, b.g2);
        if (cv < bc) { bc = cv; bi = i; ba = ca; bb = cb; }              // (i ascending within a lane)
    }
    for (int d = 32; d >= 1; d >>= 1) {
        const int oc = __shfl_xor(bc, d), oi = __shfl_xor(bi, d), oa = __shfl_xor(ba, d), ob = __shfl_xor(bb, d);
        if (oc < bc || (oc == bc && oi < bi)) { bc = oc; bi = oi; ba = oa; bb = ob; }
    }
    if (bc == CHM_INF) { if (lane >= 2 && lane < NGSID_CHIMERA_NFIELD) o[lane] = -1; return; }      // one gid only (uniform)
    const uint16_t* Fa = base + (size_t)ba * blk; const uint16_t* Bb = base + (size_t)bb * blk + (n + 1);
    int hi = -1;
    for (int i = lane; i <= n; i += 64) if ((int)Fa[i] + (int)Bb[i] == bc) hi = i;
    for (int d = 32; d >= 1; d >>= 1) hi = max(hi, __shfl_xor(hi, d));
    if (lane == 0) { o[2] = bc; o[3] = ba; o[4] = bb; o[5] = bi; o[6] = hi; }
}

}  // namespace

extern "C" int32_t ngsid_chimera_model(ngsid_ctx* ctx, const ngsid_reads_t* queries, const ngsid_reads_t* parents,
                                       const uint64_t* pair_off, const uint32_t* pair_parent, const int32_t* pair_gid, int32_t* fields, uint16_t* profiles)
{
    ApiClock api_clock_(ctx, "chimera_model");
    if (!ctx) return NGSID_ERR_ARG;
    if (!queries || !parents || !pair_off) NGSID_FAIL(ctx, NGSID_ERR_ARG, "null argument");
    DevReads Q, Pr;
    int32_t rc = ngsid_upload_reads(ctx, queries, &Q, false); if (rc) return rc;
    rc = ngsid_upload_reads(ctx, parents, &Pr, false); if (rc) return rc;
    const uint64_t N = Q.n;
    // ---- the CSR
    if (pair_off[0] != 0) NGSID_FAIL(ctx, NGSID_ERR_ARG, "pair_off[0] must be 0");
    for (uint64_t q = 0; q < N; ++q) if (pair_off[q + 1] < pair_off[q]) NGSID_FAIL(ctx, NGSID_ERR_ARG, "pair_off decreases at query %llu", (unsigned long long)q);
    const uint64_t NP = pair_off[N];
    if (NP >= 0x80000000ull) NGSID_FAIL(ctx, NGSID_ERR_ARG, "%llu pairs: a call is limited to 2^31 - 1", (unsigned long long)NP);
    if (NP && !pair_parent) NGSID_FAIL(ctx, NGSID_ERR_ARG, "null pair_parent");
    for (uint64_t k = 0; k < NP; ++k) if (pair_parent[k] >= Pr.n) NGSID_FAIL(ctx, NGSID_ERR_ARG, "pair %llu: parent %u out of range (%llu parents)", (unsigned long long)k, pair_parent[k], (unsigned long long)Pr.n);
    if (Q.maxlen > NGSID_MAX_CONSENSUS_LEN || Pr.maxlen > NGSID_MAX_CONSENSUS_LEN)
        NGSID_FAIL(ctx, NGSID_ERR_TOO_LONG, "a sequence of %u bases exceeds NGSID_MAX_CONSENSUS_LEN=%d", std::max(Q.maxlen, Pr.maxlen), NGSID_MAX_CONSENSUS_LEN);
    NGSID_TRY(ngsid_alphabet_check(ctx, Q, &Pr, "k_chimera_check", "a query or a parent holds a base outside upper-case ACGTN"));
    if (N == 0) return NGSID_OK;
    if (!fields) NGSID_FAIL(ctx, NGSID_ERR_ARG, "null output");
    // ---- per pair: its query, its gid, where its block starts (in uint16 values, from the first pair of the call)
    PinVec<uint32_t> h_pq(NP); PinVec<int32_t> h_gid(NP); PinVec<uint64_t> h_po(NP + 1);
    std::vector<uint64_t> qbytes(N);
    uint64_t run = 0;
    for (uint64_t q = 0; q < N; ++q) {
        const uint64_t blk = 2 * (Q.h_off[q + 1] - Q.h_off[q] + 1);
        for (uint64_t k = pair_off[q]; k < pair_off[q + 1]; ++k) { h_pq[k] = (uint32_t)q; h_gid[k] = pair_gid ? pair_gid[k] : (int32_t)pair_parent[k]; h_po[k] = run; run += blk; }
        qbytes[q] = blk * (pair_off[q + 1] - pair_off[q]) * sizeof(uint16_t);
    }
    h_po[NP] = run;
    // ---- chunks of queries under a share of the free device memory
    std::vector<uint64_t> cuts{0};
    const long long opt = ngsid_opt(ctx, "chimera_chunk_queries", 0);
    if (opt > 0) { for (uint64_t c = (uint64_t)opt; c < N; c += (uint64_t)opt) cuts.push_back(c); }
    else {
        const size_t budget = ngsid_mem_share(4, (size_t)64 << 20, (size_t)16 << 30, (size_t)4 << 30);
        uint64_t acc = 0;
        for (uint64_t q = 0; q < N; ++q) { if (acc && acc + qbytes[q] > budget) { cuts.push_back(q); acc = 0; } acc += qbytes[q]; }
    }
    cuts.push_back(N);
    uint64_t chunk_vals = 1;
    for (size_t c = 0; c + 1 < cuts.size(); ++c) chunk_vals = std::max<uint64_t>(chunk_vals, h_po[pair_off[cuts[c + 1]]] - h_po[pair_off[cuts[c]]]);
    HIPCHK(ctx, ctx->chm_prof.reserve(chunk_vals));
    const bool strips = Pr.maxlen > CHM_STRIP;
    const uint32_t bnd_stride = strips ? ((Q.maxlen + 1 + 63u) & ~63u) : 0;
    const unsigned max_grid = (unsigned)ctx->n_cu * (strips ? 8u : 32u);
    HIPCHK(ctx, ctx->chm_bnd.reserve(strips ? (size_t)max_grid * 2 * bnd_stride : 1));
    DevBuf<uint32_t> d_pq, d_pp, d_ctr; DevBuf<int32_t> d_gid, d_fields; DevBuf<uint64_t> d_po, d_poff;
    NGSID_TRY(dev_put(ctx, d_pq, h_pq.data(), NP)); NGSID_TRY(dev_put(ctx, d_pp, pair_parent, NP)); NGSID_TRY(dev_put(ctx, d_gid, h_gid.data(), NP));
    NGSID_TRY(dev_put(ctx, d_po, h_po.data(), NP + 1)); NGSID_TRY(dev_put(ctx, d_poff, pair_off, N + 1));
    HIPCHK(ctx, d_ctr.alloc(cuts.size())); HIPCHK(ctx, d_fields.alloc(N * NGSID_CHIMERA_NFIELD));
    HIPCHK(ctx, hipMemsetAsync(d_ctr.p, 0, sizeof(uint32_t) * cuts.size(), ctx->stream));
    for (size_t c = 0; c + 1 < cuts.size(); ++c) {
        const uint64_t qa = cuts[c], qb = cuts[c + 1], ka = pair_off[qa], kb = pair_off[qb], v0 = h_po[ka], nv = h_po[kb] - v0;
        uint16_t* prof = ctx->chm_prof.p;                                 // the chunk's blocks start at value v0 of the call
        if (kb > ka) {
            const unsigned grid = (unsigned)std::min<uint64_t>(kb - ka, max_grid);
            ProfScope ps_(ctx, "k_chimera_profile");
            hipLaunchKernelGGL(k_chimera_profile, dim3(grid), dim3(64), 0, ctx->stream, Q.seq, Q.off, Pr.seq, Pr.off, d_pq.p + ka, d_pp.p + ka, d_po.p + ka, (u64)v0, (uint32_t)(kb - ka),
                               prof, ctx->chm_bnd.p, bnd_stride, d_ctr.p + c);
            HIPCHK(ctx, hipGetLastError());
        }
        { ProfScope ps_(ctx, "k_chimera_reduce");
          hipLaunchKernelGGL(k_chimera_reduce, dim3(NGSID_GRID(ctx, qb - qa, 64, "k_chimera_reduce")), dim3(64), 0, ctx->stream, Q.off, (u64)qa, d_poff.p, (u64)ka, d_po.p + ka, (u64)v0, d_gid.p + ka, prof, d_fields.p); }
        HIPCHK(ctx, hipGetLastError());
        if (profiles) NGSID_TRY(dev_get(ctx, profiles + v0, ctx->chm_prof.p, nv));
        if (c + 2 < cuts.size()) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));      // the next chunk rewrites the scratch
    }
    NGSID_TRY(dev_get(ctx, fields, d_fields.p, N * NGSID_CHIMERA_NFIELD));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return NGSID_OK;
}
