// k_cigar.hip - ngsid_read_cigars (include/ngsid_cigar.h): the alignment of every listed read to its centre as run-length-encoded BAM operations.
//
// The store pass is ngsid_hp_runs' (ngsid_rec_walk with positions, k_support.hip).  WALK (k_cigar_walk) gives ONE WAVE to a pair: its lanes are 64 consecutive centre
// positions of an aligned step, a lane reads the nibble of its position and gets class and insertion flag of the position before it from the lane below (lane 0: from
// lane 63 of the step before, carried wave-uniform).  "An op starts here" is one ballot: the bits below a lane count the ops in front of its own, the next set bit gives
// the run's length; the run still open at the end of a step is carried (index, length) and written by lane 0 when a later step closes it.  An insertion sits between two
// match positions (include/ngsid_cigar.h: never next to a 'D'), its length is the difference of their read positions - pos is read there and nowhere else.  No LDS, no
// atomics.  The walk runs twice: COUNT (ops per pair), a host scan over the chunk's pairs, EMIT (the ops at their offsets, t / q span and nm per pair).
#include "k_support.h"
#include "../../include/ngsid_cigar.h"
#include <algorithm>

typedef uint64_t u64;

#define CIGAR_WAVES 4           // pairs per workgroup (one wave each)

__device__ __forceinline__ uint32_t cigar_op(uint32_t cls, bool merge) { return cls == 2 ? NGSID_CIGAR_OP_D : cls == 1 ? NGSID_CIGAR_OP_X : merge ? NGSID_CIGAR_OP_M : NGSID_CIGAR_OP_EQ; }

template <bool EMIT>
__global__ __launch_bounds__(64 * CIGAR_WAVES)
void k_cigar_walk(const uint32_t* __restrict__ rec, uint32_t stride, const uint16_t* __restrict__ pos /* [pair][stride * 8] */, const int32_t* __restrict__ span,
                  const uint32_t* __restrict__ pair_read /* pairs of this chunk */, const u64* __restrict__ read_off, uint32_t npairs, uint32_t merge,
                  uint32_t* __restrict__ cnt /* [pair]: written by COUNT, the bound of a pair's writes in EMIT */, const u64* __restrict__ off /* EMIT: first op of every pair */,
                  uint32_t* __restrict__ ops, int32_t* __restrict__ aln /* EMIT: [pair][5] */)
{
    const uint32_t lane = threadIdx.x & 63u;
    const u64 p = (u64)blockIdx.x * CIGAR_WAVES + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (p >= npairs) return;                                                           // (wave-uniform, no barrier below)
    const int qb = span[p * 4], qe = span[p * 4 + 1], tb = span[p * 4 + 2], te = span[p * 4 + 3];
    const uint32_t rd = pair_read[p];
    const int L = (int)(read_off[rd + 1] - read_off[rd]);
    if (tb < 0 || te < tb || (uint32_t)te >= stride * 8u || qb < 0 || qe < qb || qe >= L) {      // no counted column (all -1); anything else a path cannot be keeps the loads inside the row
        if (EMIT) { if (lane < NGSID_CIGAR_NFIELD) aln[p * NGSID_CIGAR_NFIELD + lane] = -1; }
        else if (lane == 0) cnt[p] = 0;
        return;
    }
    const uint32_t* row = rec + p * stride; const uint16_t* prow = pos + p * stride * 8;
    uint32_t* out = nullptr; uint32_t room = 0;
    if (EMIT) { out = ops + off[p]; room = cnt[p]; }
    auto put = [&](uint32_t i, uint32_t len, uint32_t op) { if (EMIT && i < room) out[i] = (len << 4) | op; };
    uint32_t nops = qb > 0;                                                          // ops in front of the current step
    if (lane == 0 && qb > 0) put(0, (uint32_t)qb, NGSID_CIGAR_OP_S);
    uint32_t open_idx = 0, open_len = 0; bool have_open = false;                      // the run that reaches the end of the step before (its class: carry_cls)
    uint32_t carry_cls = 0, carry_flag = 0, n_x = 0, n_d = 0;
    for (int base = tb & ~63; base <= te; base += 64) {
        const int b = base + (int)lane;
        const bool valid = b >= tb && b <= te;
        const uint32_t nib = valid ? (row[b >> 3] >> ((b & 7) * 4)) & 15u : 0u, code = nib & 7u, flag = nib >> 3;
        const uint32_t cls = code == NGSID_REC_DEL ? 2u : (merge || code == NGSID_REC_EQ) ? 0u : 1u;
        uint32_t pc = __shfl_up(cls, 1), pf = __shfl_up(flag, 1);
        if (lane == 0) { pc = carry_cls; pf = carry_flag; }
        const bool insb = valid && b > tb && pf && pc != 2u && cls != 2u;              // an 'I' run between the position before and this one: both are match positions
        const bool start = valid && (b == tb || cls != pc || insb);
        const u64 S = __ballot(start), I = __ballot(insb), V = __ballot(valid);        // V: one contiguous range of lanes, never empty
        n_x += (uint32_t)__popcll(__ballot(valid && code != NGSID_REC_EQ && code != NGSID_REC_DEL));
        n_d += (uint32_t)__popcll(__ballot(valid && code == NGSID_REC_DEL));
        const int v0 = __ffsll((long long)V) - 1, v1 = 63 - __clzll((long long)V);
        const u64 below = (1ull << lane) - 1;
        const uint32_t my = nops + (uint32_t)__popcll(S & below) + (uint32_t)__popcll(I & below);      // index of the first op made at this position
        if (EMIT && insb) put(my, (uint32_t)((int)prow[b] - (int)prow[b - 1] - 1) & 0xfffffffu, NGSID_CIGAR_OP_I);
        if (have_open) open_len += (uint32_t)((S ? __ffsll((long long)S) - 1 : v1 + 1) - v0);
        if (S) {
            if (have_open && lane == 0) put(open_idx, open_len, cigar_op(carry_cls, merge));
            if (start) {
                const u64 above = S & ((~0ull << lane) << 1);
                if (above) put(my + insb, (uint32_t)(__ffsll((long long)above) - 1) - lane, cigar_op(cls, merge));
            }
            const int last = 63 - __clzll((long long)S);                               // the last run of the step stays open
            open_idx = nops + (uint32_t)__popcll(S & ((1ull << last) - 1)) + (uint32_t)__popcll(I & ((2ull << last) - 1));
            open_len = (uint32_t)(v1 - last + 1); have_open = true;
        }
        nops += (uint32_t)__popcll(S) + (uint32_t)__popcll(I);
        carry_cls = __shfl(cls, v1); carry_flag = __shfl(flag, v1);
    }
    const int tail = L - 1 - qe;
    if (lane == 0) {
        put(open_idx, open_len, cigar_op(carry_cls, merge));
        if (tail > 0) put(nops, (uint32_t)tail, NGSID_CIGAR_OP_S);
    }
    nops += tail > 0;
    if (!EMIT) { if (lane == 0) cnt[p] = nops; return; }
    if (lane == 0) {
        int32_t* a = aln + p * NGSID_CIGAR_NFIELD;
        a[0] = tb; a[1] = te; a[2] = qb; a[3] = qe;
        a[4] = (int32_t)(n_x + n_d) + (qe - qb + 1) - ((te - tb + 1) - (int32_t)n_d);      // 'I' columns = read letters of the span - its match columns
    }
}

extern "C" int32_t ngsid_read_cigars(ngsid_ctx* ctx, const ngsid_reads_t* centres, const ngsid_reads_t* reads, const uint32_t* read_order,
                                     const uint64_t* grp_off, uint64_t n_groups, const ngsid_support_params_t* prm, uint32_t flags,
                                     int8_t* strand, int32_t* aln, uint64_t* op_off, uint32_t* ops, uint64_t cap, uint64_t* needed)
{
    ApiClock api_clock_(ctx, "read_cigars");
    if (!ctx) return NGSID_ERR_ARG;
    if (!needed) NGSID_FAIL(ctx, NGSID_ERR_ARG, "null argument");
    if (flags & ~NGSID_CIGAR_MERGE_M) NGSID_FAIL(ctx, NGSID_ERR_ARG, "unknown flags %u", flags);
    *needed = 0;
    const bool count_only = !aln && !op_off && !ops;
    if (count_only && cap) NGSID_FAIL(ctx, NGSID_ERR_ARG, "a count call has cap 0");
    if (!count_only && (!aln || !op_off || (cap && !ops))) NGSID_FAIL(ctx, NGSID_ERR_ARG, "null aln, op_off or ops");
    DevBuf<uint32_t> d_cnt, d_ops; DevBuf<u64> d_off; DevBuf<int32_t> d_aln;
    std::vector<uint32_t> h_cnt; std::vector<u64> h_off; std::vector<int32_t> h_aln;
    u64 total = 0, NL = 0; bool fill = !count_only;
    auto init = [&](const RecPlan& P) -> int32_t {
        NL = grp_off[n_groups];
        if (!count_only) {
            for (u64 x = 0; x < NL * NGSID_CIGAR_NFIELD; ++x) aln[x] = -1;
            for (u64 x = 0; x <= NL; ++x) op_off[x] = 0;
        }
        return NGSID_OK;
    };
    auto start = [&](const RecPlan&) -> int32_t { return NGSID_OK; };
    auto chunk = [&](const RecPlan& P, const RecChunk& C) -> int32_t {
        const uint32_t n = (uint32_t)(C.c1 - C.c0);
        const unsigned grid = NGSID_GRID(ctx, ((u64)n + CIGAR_WAVES - 1) / CIGAR_WAVES, 64 * CIGAR_WAVES, "k_cigar_walk");
        HIPCHK(ctx, d_cnt.reserve(n)); h_cnt.resize(n);
        { ProfScope ps_(ctx, "k_cigar_count");
          hipLaunchKernelGGL(k_cigar_walk<false>, dim3(grid), dim3(64 * CIGAR_WAVES), 0, ctx->stream, C.rec, P.stride, C.pos, C.span, P.d_pair_read + C.c0, P.d_read_off,
                             n, flags & NGSID_CIGAR_MERGE_M, d_cnt.p, (const u64*)nullptr, (uint32_t*)nullptr, (int32_t*)nullptr); }
        HIPCHK(ctx, hipGetLastError());
        NGSID_TRY(dev_get(ctx, h_cnt.data(), d_cnt.p, n));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        h_off.resize(n); u64 sum = 0;
        for (uint32_t i = 0; i < n; ++i) { h_off[i] = sum; sum += h_cnt[i]; }
        const u64 base = total; total += sum;
        if (!fill) return NGSID_OK;
        if (total > cap) { fill = false; return NGSID_OK; }                           // more ops than the caller has room for: count on
        for (uint32_t i = 0; i < n; ++i) op_off[P.pair_x[C.c0 + i] + 1] = h_cnt[i];  // (counts: summed over the listed reads behind the last chunk)
        HIPCHK(ctx, d_off.reserve(n)); HIPCHK(ctx, d_ops.reserve(sum)); HIPCHK(ctx, d_aln.reserve((size_t)n * NGSID_CIGAR_NFIELD)); h_aln.resize((size_t)n * NGSID_CIGAR_NFIELD);
        HIPCHK(ctx, hipMemcpyAsync(d_off.p, h_off.data(), sizeof(u64) * n, hipMemcpyHostToDevice, ctx->stream));
        { ProfScope ps_(ctx, "k_cigar_emit");
          hipLaunchKernelGGL(k_cigar_walk<true>, dim3(grid), dim3(64 * CIGAR_WAVES), 0, ctx->stream, C.rec, P.stride, C.pos, C.span, P.d_pair_read + C.c0, P.d_read_off,
                             n, flags & NGSID_CIGAR_MERGE_M, d_cnt.p, (const u64*)d_off.p, d_ops.p, d_aln.p); }
        HIPCHK(ctx, hipGetLastError());
        NGSID_TRY(dev_get(ctx, ops + base, d_ops.p, sum)); NGSID_TRY(dev_get(ctx, h_aln.data(), d_aln.p, (size_t)n * NGSID_CIGAR_NFIELD));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        for (uint32_t i = 0; i < n; ++i) memcpy(aln + (size_t)P.pair_x[C.c0 + i] * NGSID_CIGAR_NFIELD, h_aln.data() + (size_t)i * NGSID_CIGAR_NFIELD, sizeof(int32_t) * NGSID_CIGAR_NFIELD);
        return NGSID_OK;
    };
    int32_t rc = ngsid_rec_walk(ctx, centres, reads, read_order, grp_off, n_groups, prm, strand, init, start, chunk, true); if (rc) return rc;
    *needed = total;
    if (total > cap) NGSID_FAIL(ctx, NGSID_ERR_CAPACITY, "%llu ops, room for %llu", (unsigned long long)total, (unsigned long long)cap);
    if (!count_only) for (u64 x = 0; x < NL; ++x) op_off[x + 1] += op_off[x];
    return NGSID_OK;
}
