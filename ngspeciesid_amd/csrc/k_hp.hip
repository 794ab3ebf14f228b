// k_hp.hip - ngsid_hp_runs (include/ngsid_hp.h): per listed homopolymer run of every centre and per strand, the histogram of the run's length in the reads.
//
// The store pass is ngsid_consensus_support's (ngsid_rec_walk, k_support.hip) with its second output: beside the nibble per (read, centre position) the read index of every
// '=' / 'X' column, so "the read has one more A here" can be told from "the read has a G the centre lacks".  RUNS (k_hp_runs) has the shape of k_support_sum: a workgroup takes a
// slice of ONE group's pairs of the chunk, its lanes are the listed runs of the group in tiles of 256, the span and the strand of a pair are uniform loads.  A lane reads the two
// flank nibbles of its run, the two read positions behind them and the read bases in between.  Its 2 x 17 counters are indexed by what it finds, so they live in LDS, one private
// column per thread laid out [counter][thread] (consecutive lanes on consecutive addresses, no two lanes share one - as k_phase_pairs); uint16 holds a slice of 1 024 pairs.  Every
// non-zero counter goes to global memory with ONE atomicAdd per (workgroup, run).  Integer adds commute: the result does not depend on slices, tiles or chunks.
#include "k_support.h"
#include "../../include/ngsid_hp.h"
#include <algorithm>

typedef uint64_t u64;

#define HP_TILE 256             // listed runs per workgroup (= threads)
#define HP_SLICE 1024           // pairs per workgroup: a uint16 counter cannot overflow
#define HP_NCOUNT (2 * NGSID_HP_NBUCKET)

__global__ __launch_bounds__(HP_TILE)
void k_hp_runs(const uint32_t* __restrict__ rec, uint32_t stride, const uint16_t* __restrict__ pos /* [pair][stride * 8] */, const int32_t* __restrict__ span,
               const uint32_t* __restrict__ pair_read, const uint8_t* __restrict__ pair_strand /* both: pairs of this chunk */, const uint8_t* __restrict__ oseq,
               const u64* __restrict__ read_off, const uint32_t* __restrict__ items /* [n][3]: group, first pair, end pair (pairs of this chunk) */,
               const u64* __restrict__ run_off, const uint32_t* __restrict__ run_start, const uint32_t* __restrict__ run_end, const uint8_t* __restrict__ cen_seq,
               const u64* __restrict__ cen_off, uint32_t* __restrict__ hist)
{
    __shared__ uint16_t cnt[HP_NCOUNT * HP_TILE];                                  // [counter][thread]
    const uint32_t g = items[blockIdx.x * 3], p0 = items[blockIdx.x * 3 + 1], p1 = items[blockIdx.x * 3 + 2];
    const uint32_t tid = threadIdx.x;
    const u64 r = (u64)blockIdx.y * HP_TILE + tid;
    if (r >= run_off[g + 1] - run_off[g]) return;                                  // (no barrier below: every thread owns its column)
    const int m = (int)(cen_off[g + 1] - cen_off[g]);
    const int a = (int)run_start[run_off[g] + r], b = (int)run_end[run_off[g] + r];
    const int c = ngsid_bcode(cen_seq[cen_off[g] + (u64)a]);
    if (a < 1 || b > m - 1 || c >= 4) return;                                      // the first and the last run are never spanned; a run of N collects nothing
#pragma unroll
    for (int k = 0; k < HP_NCOUNT; ++k) cnt[k * HP_TILE + tid] = 0;
    const int wa = (a - 1) >> 3, sa = ((a - 1) & 7) * 4, wb = b >> 3, sb = (b & 7) * 4;
    for (uint32_t p = p0; p < p1; ++p) {
        const int tb = span[(u64)p * 4 + 2], te = span[(u64)p * 4 + 3];            // (uniform; tb = te = -1: no counted column)
        if (a - 1 < tb || b > te) continue;                                          // not spanned
        const uint32_t* row = rec + (u64)p * stride;
        const uint32_t na = (row[wa] >> sa) & 7u, nb = (row[wb] >> sb) & 7u;
        uint32_t bucket = NGSID_HP_OTHER;
        if (na == NGSID_REC_EQ && nb == NGSID_REC_EQ) {
            const uint16_t* prow = pos + (u64)p * stride * 8;
            const int qa = prow[a - 1], qb = prow[b];
            const uint32_t rd = pair_read[p];
            const uint8_t* q = oseq + read_off[rd]; const int n = (int)(read_off[rd + 1] - read_off[rd]);
            if (qa < qb && qb < n) {                                                 // always true for a path of the aligner: keeps the loads inside the read whatever the cells hold
                bool same = true;
                for (int i = qa + 1; i < qb; ++i) same &= ngsid_bcode(q[i]) == c;
                if (same) bucket = (uint32_t)min(qb - qa - 1, 15);
            }
        }
        cnt[((uint32_t)pair_strand[p] * NGSID_HP_NBUCKET + bucket) * HP_TILE + tid] += 1;
    }
    uint32_t* out = hist + (run_off[g] + r) * HP_NCOUNT;
#pragma unroll
    for (int k = 0; k < HP_NCOUNT; ++k) { const uint32_t v = cnt[k * HP_TILE + tid]; if (v) atomicAdd(out + k, v); }
}

extern "C" int32_t ngsid_hp_runs(ngsid_ctx* ctx, const ngsid_reads_t* centres, const ngsid_reads_t* reads, const uint32_t* read_order,
                                 const uint64_t* grp_off, uint64_t n_groups, const ngsid_support_params_t* prm,
                                 const uint64_t* run_off, const uint32_t* run_start, uint32_t* hist, int8_t* strand)
{
    ApiClock api_clock_(ctx, "hp_runs");
    if (!ctx) return NGSID_ERR_ARG;
    if (!run_off) NGSID_FAIL(ctx, NGSID_ERR_ARG, "null argument");
    const uint32_t G = (uint32_t)n_groups;
    DevBuf<u64> d_run_off; DevBuf<uint32_t> d_run_start, d_run_end, d_hist, d_items; DevBuf<uint8_t> d_pair_strand;
    std::vector<uint32_t> run_end, items; std::vector<uint8_t> pair_strand; bool started = false; u64 max_runs = 0;
    auto init = [&](const RecPlan& P) -> int32_t {
        for (uint32_t g = 0; g < G; ++g) if (run_off[g + 1] < run_off[g]) NGSID_FAIL(ctx, NGSID_ERR_ARG, "run_off descends at group %u", g);
        const u64 NR = run_off[G] - run_off[0];
        if (run_off[0] != 0) NGSID_FAIL(ctx, NGSID_ERR_ARG, "run_off[0] must be 0");
        if (NR && (!run_start || !hist)) NGSID_FAIL(ctx, NGSID_ERR_ARG, "null run_start or hist");
        run_end.resize(NR);
        for (uint32_t g = 0; g < G; ++g) {
            const u64 m = P.boff[g + 1] - P.boff[g]; const uint8_t* C = P.bseq + P.boff[g];
            max_runs = std::max(max_runs, run_off[g + 1] - run_off[g]);
            for (u64 i = run_off[g]; i < run_off[g + 1]; ++i) {
                const u64 a = run_start[i];
                if (a >= m) NGSID_FAIL(ctx, NGSID_ERR_ARG, "run %u of group %u lies beyond its centre of %llu bases", run_start[i], g, (unsigned long long)m);
                if (i > run_off[g] && run_start[i] <= run_start[i - 1]) NGSID_FAIL(ctx, NGSID_ERR_ARG, "the runs of group %u are not strictly ascending", g);
                if (a > 0 && C[a - 1] == C[a]) NGSID_FAIL(ctx, NGSID_ERR_ARG, "position %u of group %u is not the first base of a run", run_start[i], g);
                u64 b = a + 1; while (b < m && C[b] == C[a]) ++b;
                run_end[i] = (uint32_t)b;
            }
        }
        if (NR) memset(hist, 0, sizeof(uint32_t) * HP_NCOUNT * NR);
        return NGSID_OK;
    };
    auto start = [&](const RecPlan& P) -> int32_t {
        if (run_end.empty()) return NGSID_OK;                                      // no run anywhere: the strands are the whole result
        int32_t rc;
        if ((rc = dev_put(ctx, d_run_off, run_off, (size_t)G + 1)) || (rc = dev_put(ctx, d_run_start, run_start, run_end.size())) ||
            (rc = dev_put(ctx, d_run_end, run_end.data(), run_end.size()))) return rc;
        pair_strand.resize(P.NP);
        for (u64 p = 0; p < P.NP; ++p) pair_strand[p] = P.h_orient[P.pair_read[p]] ? 1 : 0;
        NGSID_TRY(dev_put(ctx, d_pair_strand, pair_strand.data(), pair_strand.size()));
        HIPCHK(ctx, d_hist.alloc(run_end.size() * HP_NCOUNT));
        HIPCHK(ctx, hipMemsetAsync(d_hist.p, 0, sizeof(uint32_t) * HP_NCOUNT * run_end.size(), ctx->stream));
        started = true; return NGSID_OK;
    };
    auto chunk = [&](const RecPlan& P, const RecChunk& C) -> int32_t {
        if (!started) return NGSID_OK;
        items.clear();
        for (uint32_t g = 0; g < P.G; ++g) {
            const uint64_t a = std::max(P.gbeg[g], C.c0), e = std::min(P.gbeg[g + 1], C.c1);
            if (run_off[g + 1] == run_off[g]) continue;
            for (uint64_t s = a; s < e; s += HP_SLICE) { items.push_back(g); items.push_back((uint32_t)(s - C.c0)); items.push_back((uint32_t)(std::min(e, s + HP_SLICE) - C.c0)); }
        }
        if (items.empty()) return NGSID_OK;
        HIPCHK(ctx, d_items.reserve(items.size()));
        HIPCHK(ctx, hipMemcpyAsync(d_items.p, items.data(), 4 * items.size(), hipMemcpyHostToDevice, ctx->stream));
        { ProfScope ps_(ctx, "k_hp_runs");
          hipLaunchKernelGGL(k_hp_runs, dim3(NGSID_GRID(ctx, items.size() / 3, HP_TILE, "k_hp_runs"), (unsigned)((max_runs + HP_TILE - 1) / HP_TILE)), dim3(HP_TILE), 0, ctx->stream,
                             C.rec, P.stride, C.pos, C.span, P.d_pair_read + C.c0, d_pair_strand.p + C.c0, P.d_oseq, P.d_read_off, d_items.p,
                             d_run_off.p, d_run_start.p, d_run_end.p, P.d_cen_seq, P.d_cen_off, d_hist.p); }
        HIPCHK(ctx, hipGetLastError());
        return NGSID_OK;
    };
    int32_t rc = ngsid_rec_walk(ctx, centres, reads, read_order, grp_off, n_groups, prm, strand, init, start, chunk, true); if (rc) return rc;
    if (!started) return NGSID_OK;
    NGSID_TRY(dev_get(ctx, hist, d_hist.p, run_end.size() * HP_NCOUNT));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return NGSID_OK;
}
