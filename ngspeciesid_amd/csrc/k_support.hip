// k_support.hip - ngsid_consensus_support (include/ngsid_support.h): per base of every centre, how many reads agree, disagree (and with what), delete or insert.
//
// Two passes.  STORE: the polisher's edit-distance aligner with the path recorded (k_ed_align<.., REC>, k_ed_align.hip) writes one nibble per (read, centre position) into
// a [read][centre position] matrix - 0.5 B per cell, a dword store per lane and 8 columns.  SUM (k_support_sum, below): lanes over centre positions (8 lanes share a dword,
// 256 lanes read 128 consecutive bytes of a row), a workgroup takes a slice of ONE group's reads, keeps the eight counters of its position in registers and adds them once
// per (workgroup, position) with atomicAdd on uint32.  The traceback itself never touches the counters: its 64 lanes walk 64 reads of the same centre in near lockstep, so
// every step would be 64 atomics on one address.  Integer adds commute: the result does not depend on the schedule.
#include "k_support.h"

typedef unsigned long long u64;

#define SUPPORT_TILE 256        // centre positions per workgroup (= threads)
#define SUPPORT_SLICE 1024      // reads per workgroup

__global__ __launch_bounds__(SUPPORT_TILE)
void k_support_sum(const uint32_t* __restrict__ rec, uint32_t stride, const int32_t* __restrict__ span /* per pair {q_begin, q_end, t_begin, t_end}, -1 = no counted column */,
                   const uint32_t* __restrict__ items /* [n][3]: group, first pair, end pair (pairs of this chunk) */, const uint64_t* __restrict__ cen_off,
                   uint32_t* __restrict__ counts, u64* __restrict__ n_used)
{
    const uint32_t g = items[blockIdx.x * 3], p0 = items[blockIdx.x * 3 + 1], p1 = items[blockIdx.x * 3 + 2];
    if (blockIdx.y == 0) {              // reads of the slice that counted at least one column
        unsigned used = 0;
        for (uint32_t p = p0 + threadIdx.x; p < p1; p += SUPPORT_TILE) used += span[(u64)p * 4 + 2] >= 0;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) used += __shfl_xor(used, d);
        if ((threadIdx.x & 63) == 0 && used) atomicAdd(n_used + g, (u64)used);
    }
    const int m = (int)(cen_off[g + 1] - cen_off[g]);
    const int b = (int)(blockIdx.y * SUPPORT_TILE + threadIdx.x);
    if (b >= m) return;
    const uint32_t* col = rec + (b >> 3); const int sh = (b & 7) * 4;
    uint32_t depth = 0, agree = 0, sa = 0, sc = 0, sg = 0, st = 0, del = 0, ins = 0;
#pragma unroll 4
    for (uint32_t p = p0; p < p1; ++p) {
        const int tb = span[(u64)p * 4 + 2], te = span[(u64)p * 4 + 3];          // (uniform: one scalar load per read)
        if (b < tb || b > te) continue;                                            // outside the counted columns of this read (tb = te = -1: none)
        const uint32_t nib = (col[(u64)p * stride] >> sh) & 15u, code = nib & 7u;
        depth += code != 0; agree += code == NGSID_REC_EQ;
        sa += code == NGSID_REC_SUB; sc += code == NGSID_REC_SUB + 1; sg += code == NGSID_REC_SUB + 2; st += code == NGSID_REC_SUB + 3;
        del += code == NGSID_REC_DEL;
        ins += (nib >> 3) & (uint32_t)(b < te);                                    // a run behind the LAST counted column is not counted
    }
    uint32_t* out = counts + (cen_off[g] + (u64)b) * NGSID_SUPPORT_NCOUNT;
    if (depth) atomicAdd(out + NGSID_SUPPORT_DEPTH, depth);
    if (agree) atomicAdd(out + NGSID_SUPPORT_AGREE, agree);
    if (sa) atomicAdd(out + NGSID_SUPPORT_SUB_A, sa);
    if (sc) atomicAdd(out + NGSID_SUPPORT_SUB_A + 1, sc);
    if (sg) atomicAdd(out + NGSID_SUPPORT_SUB_A + 2, sg);
    if (st) atomicAdd(out + NGSID_SUPPORT_SUB_A + 3, st);
    if (del) atomicAdd(out + NGSID_SUPPORT_DEL, del);
    if (ins) atomicAdd(out + NGSID_SUPPORT_INS, ins);
}

// The store pass and its bookkeeping, shared with ngsid_phase_genotypes (k_phase.hip): argument checks, strands, pairs in list order, the path matrix chunk by chunk.
// `init` runs once the centres are on the host (P.G, P.total, P.maxb, P.boff: validate and clear the caller's outputs); `start` once before the first chunk, when there is
// at least one pair (everything else of P is set: device allocations of the consumer); `chunk` after the store pass of every chunk, followed by a stream synchronisation.
int32_t ngsid_rec_walk(ngsid_ctx* ctx, const ngsid_reads_t* centres, const ngsid_reads_t* reads, const uint32_t* read_order, const uint64_t* grp_off, uint64_t n_groups,
                       const ngsid_support_params_t* prm, int8_t* strand, const std::function<int32_t(const RecPlan&)>& init,
                       const std::function<int32_t(const RecPlan&)>& start, const std::function<int32_t(const RecPlan&, const RecChunk&)>& chunk, bool want_pos)
{
    if (!prm) NGSID_FAIL(ctx, NGSID_ERR_ARG, "null argument");
    if (prm->clip != 0 && prm->clip != 1) NGSID_FAIL(ctx, NGSID_ERR_ARG, "ngsid_support_params_t.clip must be 0 or 1");
    GroupedReads S; NGSID_TRY(ngsid_groups_open(ctx, centres, reads, read_order, grp_off, n_groups, S));
    const DevReads& RD = S.RD; const uint32_t G = S.G, maxb = S.maxb; const uint64_t total = S.boff[G];
    RecPlan P; P.G = G; P.boff = S.boff; P.total = total; P.maxb = maxb; P.bseq = S.bseq.data();
    int32_t rc = init(P); if (rc) return rc;
    if (strand) for (uint64_t x = 0; x < S.NL; ++x) strand[x] = -1;
    if (maxb > NGSID_MAX_CONSENSUS_LEN) NGSID_FAIL(ctx, NGSID_ERR_TOO_LONG, "centre longer than %d", NGSID_MAX_CONSENSUS_LEN);
    if (S.N == 0 || G == 0 || S.NL == 0) return NGSID_OK;
    NGSID_TRY(ngsid_groups_pairs(ctx, read_order, grp_off, prm->k, prm->w, S, strand));
    const uint64_t NP = S.NP; P.NP = NP; P.gbeg = S.gbeg;
    if (NP == 0 || total == 0) { HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); return NGSID_OK; }
    P.pair_x = S.pair_x->data(); P.pair_group = S.pair_group->data(); P.pair_read = S.pair_read->data(); P.h_orient = S.h_orient->data();
    DevBuf<uint32_t> d_pair_read, d_pair_group, d_rec; DevBuf<int32_t> d_span; DevBuf<uint16_t> d_pos;
    NGSID_TRY(dev_put(ctx, d_pair_read, S.pair_read->data(), NP)); NGSID_TRY(dev_put(ctx, d_pair_group, S.pair_group->data(), NP));
    ngsid_reads_t br{S.bseq.data(), nullptr, S.boff.data(), G, NGSID_MEM_HOST, 0};
    DevReads BB; rc = ngsid_upload_reads(ctx, &br, &BB, false); if (rc) return rc;
    // ---- chunks of pairs under the byte budget of the path matrix (the share of the free device memory the POA batches take; option "support_budget_mb")
    const uint32_t stride = ((maxb + 63u) & ~63u) / 8;                    // dwords per row
    P.stride = stride; P.d_cen_seq = BB.seq; P.d_cen_off = BB.off; P.d_pair_group = d_pair_group.p;
    P.d_oseq = ctx->pol_oseq.p; P.d_oqual = RD.qual ? ctx->pol_oqual.p : nullptr; P.d_read_off = RD.off; P.d_pair_read = d_pair_read.p;
    rc = start(P); if (rc) return rc;
    const long long mb = ngsid_opt(ctx, "support_budget_mb", 0);
    const size_t budget = mb > 0 ? (size_t)mb << 20 : ngsid_mem_share(3, (size_t)256 << 20, (size_t)16 << 30, (size_t)16 << 30);
    const uint64_t rows = std::min<uint64_t>(NP, std::max<uint64_t>(64, budget / ((size_t)stride * (want_pos ? 20 : 4))));      // a row: 4 bits per position, and 2 bytes with the positions
    HIPCHK(ctx, d_rec.alloc(rows * stride)); HIPCHK(ctx, d_span.alloc(rows * 4));
    if (want_pos) HIPCHK(ctx, d_pos.alloc(rows * stride * 8));
    for (uint64_t c0 = 0; c0 < NP; c0 += rows) {
        const uint64_t c1 = std::min(NP, c0 + rows);
        AlignJob J{};
        J.qseq = ctx->pol_oseq.p; J.qoff = RD.off; J.tseq = BB.seq; J.toff = BB.off; J.qidx = d_pair_read.p + c0; J.tidx = d_pair_group.p + c0; J.npairs = c1 - c0;
        J.span = d_span.p; J.clip = prm->clip;
        rc = ngsid_launch_ed_align_rec(ctx, J, RD.maxlen, maxb, d_rec.p, stride, d_pos.p); if (rc) return rc;
        rc = chunk(P, RecChunk{d_rec.p, d_span.p, c0, c1, d_pos.p}); if (rc) return rc;
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));          // the consumer's host lists are pageable and refilled by the next chunk
    }
    return NGSID_OK;
}

extern "C" int32_t ngsid_consensus_support(ngsid_ctx* ctx, const ngsid_reads_t* centres, const ngsid_reads_t* reads, const uint32_t* read_order,
                                           const uint64_t* grp_off, uint64_t n_groups, const ngsid_support_params_t* prm,
                                           uint32_t* counts, uint64_t* n_used, int8_t* strand)
{
    ApiClock api_clock_(ctx, "consensus_support");
    if (!ctx) return NGSID_ERR_ARG;
    DevBuf<uint32_t> d_counts, d_items; DevBuf<u64> d_used; std::vector<uint32_t> items; bool started = false;
    auto init = [&](const RecPlan& P) -> int32_t {
        if (P.total && !counts) NGSID_FAIL(ctx, NGSID_ERR_ARG, "null counts");
        if (counts) memset(counts, 0, sizeof(uint32_t) * NGSID_SUPPORT_NCOUNT * P.total);
        if (n_used) for (uint32_t g = 0; g < P.G; ++g) n_used[g] = 0;
        return NGSID_OK;
    };
    auto start = [&](const RecPlan& P) -> int32_t {
        HIPCHK(ctx, d_counts.alloc(P.total * NGSID_SUPPORT_NCOUNT)); HIPCHK(ctx, d_used.alloc(P.G));
        HIPCHK(ctx, hipMemsetAsync(d_counts.p, 0, sizeof(uint32_t) * NGSID_SUPPORT_NCOUNT * P.total, ctx->stream));
        HIPCHK(ctx, hipMemsetAsync(d_used.p, 0, sizeof(u64) * P.G, ctx->stream));
        started = true; return NGSID_OK;
    };
    auto chunk = [&](const RecPlan& P, const RecChunk& C) -> int32_t {
        items.clear();
        for (uint32_t g = 0; g < P.G; ++g) {
            const uint64_t a = std::max(P.gbeg[g], C.c0), e = std::min(P.gbeg[g + 1], C.c1);
            if (P.boff[g + 1] == P.boff[g]) continue;
            for (uint64_t s = a; s < e; s += SUPPORT_SLICE) { items.push_back(g); items.push_back((uint32_t)(s - C.c0)); items.push_back((uint32_t)(std::min(e, s + SUPPORT_SLICE) - C.c0)); }
        }
        if (items.empty()) return NGSID_OK;
        HIPCHK(ctx, d_items.reserve(items.size()));
        HIPCHK(ctx, hipMemcpyAsync(d_items.p, items.data(), 4 * items.size(), hipMemcpyHostToDevice, ctx->stream));
        { ProfScope ps_(ctx, "k_support_sum");
          hipLaunchKernelGGL(k_support_sum, dim3(NGSID_GRID(ctx, items.size() / 3, SUPPORT_TILE, "k_support_sum"), (P.maxb + SUPPORT_TILE - 1) / SUPPORT_TILE), dim3(SUPPORT_TILE), 0, ctx->stream,
                             C.rec, P.stride, C.span, d_items.p, P.d_cen_off, d_counts.p, d_used.p); }
        HIPCHK(ctx, hipGetLastError());
        return NGSID_OK;
    };
    int32_t rc = ngsid_rec_walk(ctx, centres, reads, read_order, grp_off, n_groups, prm, strand, init, start, chunk); if (rc) return rc;
    if (!started) return NGSID_OK;
    const uint32_t G = (uint32_t)n_groups; const uint64_t total = d_counts.n / NGSID_SUPPORT_NCOUNT;
    std::vector<u64> h_used(G);
    NGSID_TRY(dev_get(ctx, counts, d_counts.p, NGSID_SUPPORT_NCOUNT * total)); NGSID_TRY(dev_get(ctx, h_used.data(), d_used.p, G));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (n_used) for (uint32_t g = 0; g < G; ++g) n_used[g] = h_used[g];
    return NGSID_OK;
}
