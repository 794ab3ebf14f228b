// k_phase.hip - include/ngsid_phase.h: read x site genotypes from the path matrix of the support call, pair tables of the sites, nearest haplotype of every read.
//
// GATHER (k_phase_gather): the store pass is ngsid_consensus_support's (ngsid_rec_walk, k_support.hip); instead of summing the [read][centre position] nibble matrix over the
// reads, a lane takes one (read, site), reads the ONE dword that holds the site's nibble and writes the code as a byte - the lanes of a read write consecutive bytes of its row.
// PAIRS (k_phase_pairs): 64 * 63 / 2 * 25 counters of a group are 201 KB, so a workgroup takes 64 site pairs and a slice of the reads of ONE group: lane = site pair, the four
// waves take every fourth read, and every thread counts into its OWN column of 25 LDS counters ([counter][thread]: consecutive lanes hit consecutive banks, no two lanes share
// an address - the alleles of a site are skewed, so a shared 25-counter histogram per pair would serialise 64 reads on the major / major counter).  The four columns of a pair
// are summed after a barrier and every non-zero counter goes to global memory with ONE atomicAdd per workgroup - never one per read.
// ASSIGN (k_phase_assign): one lane per read, the haplotypes of the group in LDS (broadcast reads), 16 distances in registers.
#include "k_support.h"
#include "../../include/ngsid_phase.h"
#include <algorithm>

typedef uint64_t u64;

#define PHASE_THREADS 256
#define PHASE_PAIRS 64          // site pairs per workgroup (= lanes of a wave)
#define PHASE_SLICE 4096        // reads per workgroup of k_phase_pairs
#define PHASE_CELLS 25          // 5 x 5 codes

__global__ __launch_bounds__(PHASE_THREADS)
void k_phase_gather(const uint32_t* __restrict__ rec, uint32_t stride, const int32_t* __restrict__ span, const uint32_t* __restrict__ pair_group, const uint32_t* __restrict__ pair_x,
                    u64 npairs, int lp_shift /* lanes per pair = 1 << lp_shift >= the largest site count */, const u64* __restrict__ site_off, const uint32_t* __restrict__ site_pos,
                    const u64* __restrict__ geno_off, const uint8_t* __restrict__ cen_seq, const u64* __restrict__ cen_off, uint8_t* __restrict__ geno)
{
    const u64 t = (u64)blockIdx.x * PHASE_THREADS + threadIdx.x, p = t >> lp_shift;
    const uint32_t s = (uint32_t)(t & ((1u << lp_shift) - 1u));
    if (p >= npairs) return;
    const uint32_t g = pair_group[p];
    const uint32_t S = (uint32_t)(site_off[g + 1] - site_off[g]);
    if (s >= S) return;
    const int pos = (int)site_pos[site_off[g] + s];
    const int tb = span[p * 4 + 2], te = span[p * 4 + 3];                        // tb = te = -1: no counted column
    uint32_t code = NGSID_GENO_NONE;
    if (pos >= tb && pos <= te) {
        const uint32_t nib = (rec[p * stride + ((uint32_t)pos >> 3)] >> ((pos & 7) * 4)) & 7u;
        if (nib == NGSID_REC_EQ) code = (uint32_t)ngsid_bcode(cen_seq[cen_off[g] + (u64)pos]);
        else if (nib >= NGSID_REC_SUB && nib < NGSID_REC_SUB + 4) code = nib - NGSID_REC_SUB;
        else if (nib == NGSID_REC_OTHER) code = NGSID_GENO_OTHER;
        else if (nib == NGSID_REC_DEL) code = NGSID_GENO_DEL;
    }
    geno[geno_off[g] + (u64)pair_x[p] * S + s] = (uint8_t)code;
}

// pair number k of the S * (S - 1) / 2 pairs s < t in row-major order -> (s, t)
__device__ __forceinline__ void phase_pair(uint32_t k, uint32_t S, uint32_t& s, uint32_t& t)
{
    s = 0;
    while (k >= S - 1 - s) { k -= S - 1 - s; ++s; }
    t = s + 1 + k;
}

__global__ __launch_bounds__(PHASE_THREADS)
void k_phase_pairs(const uint8_t* __restrict__ geno, const u64* __restrict__ geno_off, const u64* __restrict__ site_off, const u64* __restrict__ tab_off,
                   const uint32_t* __restrict__ items /* [n][4]: group, first site pair, first read, end read (reads within the group) */, uint32_t* __restrict__ tables)
{
    __shared__ uint32_t hist[PHASE_CELLS * PHASE_THREADS];                       // [counter][thread]
    const uint32_t g = items[blockIdx.x * 4], k0 = items[blockIdx.x * 4 + 1], r0 = items[blockIdx.x * 4 + 2], r1 = items[blockIdx.x * 4 + 3];
    const uint32_t S = (uint32_t)(site_off[g + 1] - site_off[g]), npair = S * (S - 1) / 2;
    const uint32_t tid = threadIdx.x, lane = tid & (PHASE_PAIRS - 1), wave = tid / PHASE_PAIRS;
#pragma unroll
    for (int c = 0; c < PHASE_CELLS; ++c) hist[c * PHASE_THREADS + tid] = 0;
    if (k0 + lane < npair) {
        uint32_t s, t; phase_pair(k0 + lane, S, s, t);
        const uint8_t* rows = geno + geno_off[g];
        for (uint32_t r = r0 + wave; r < r1; r += PHASE_THREADS / PHASE_PAIRS) {
            const uint32_t a = rows[(u64)r * S + s], b = rows[(u64)r * S + t];   // (the 64 lanes of a wave read bytes of ONE row of at most 64 bytes)
            if (a <= NGSID_GENO_DEL && b <= NGSID_GENO_DEL) atomicAdd(&hist[(a * 5 + b) * PHASE_THREADS + tid], 1u);      // own column: an LDS add without return, no conflict
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < PHASE_CELLS * PHASE_PAIRS; i += PHASE_THREADS) {
        const uint32_t pp = i & (PHASE_PAIRS - 1), c = i / PHASE_PAIRS;
        if (k0 + pp >= npair) continue;
        uint32_t sum = 0;
#pragma unroll
        for (int w = 0; w < PHASE_THREADS / PHASE_PAIRS; ++w) sum += hist[c * PHASE_THREADS + w * PHASE_PAIRS + pp];
        if (!sum) continue;
        uint32_t s, t; phase_pair(k0 + pp, S, s, t);
        atomicAdd(tables + tab_off[g] + ((u64)s * S + t) * PHASE_CELLS + c, sum);
    }
}

__global__ __launch_bounds__(PHASE_THREADS)
void k_phase_assign(const uint8_t* __restrict__ geno, const u64* __restrict__ geno_off, const u64* __restrict__ grp_off, const u64* __restrict__ site_off,
                    const u64* __restrict__ hap_off, const u64* __restrict__ hal_off, const uint8_t* __restrict__ hap_alleles,
                    const uint32_t* __restrict__ items /* [n][2]: group, first read (within the group) */, int8_t* __restrict__ best, uint8_t* __restrict__ dist, uint8_t* __restrict__ dist2)
{
    __shared__ uint8_t hap[NGSID_PHASE_MAX_HAPS * NGSID_PHASE_MAX_SITES];
    const uint32_t g = items[blockIdx.x * 2], r = items[blockIdx.x * 2 + 1] + threadIdx.x;
    const uint32_t S = (uint32_t)(site_off[g + 1] - site_off[g]), H = (uint32_t)(hap_off[g + 1] - hap_off[g]), R = (uint32_t)(grp_off[g + 1] - grp_off[g]);
    for (uint32_t i = threadIdx.x; i < H * S; i += PHASE_THREADS) hap[(i / S) * NGSID_PHASE_MAX_SITES + i % S] = hap_alleles[hal_off[g] + i];
    __syncthreads();
    if (r >= R) return;
    const uint8_t* row = geno + geno_off[g] + (u64)r * S;
    uint32_t d[NGSID_PHASE_MAX_HAPS]; bool any = false;
#pragma unroll
    for (int h = 0; h < NGSID_PHASE_MAX_HAPS; ++h) d[h] = 0;
    for (uint32_t s = 0; s < S; ++s) {
        const uint32_t c = row[s];
        if (c > NGSID_GENO_DEL) continue;
        any = true;
#pragma unroll
        for (int h = 0; h < NGSID_PHASE_MAX_HAPS; ++h) {
            const uint32_t a = hap[h * NGSID_PHASE_MAX_SITES + s];             // (rows h >= H hold whatever LDS held: masked below)
            d[h] += (uint32_t)((uint32_t)h < H && a != NGSID_HAP_ANY && a != c);
        }
    }
    int b = -1; uint32_t d1 = 255, d2 = 255;
    if (any) {
#pragma unroll
        for (int h = 0; h < NGSID_PHASE_MAX_HAPS; ++h) {
            if ((uint32_t)h >= H) continue;
            if (b < 0 || d[h] < d1) { d2 = b < 0 ? 255u : d1; d1 = d[h]; b = h; }
            else if (d[h] < d2) d2 = d[h];
        }
    }
    const u64 x = grp_off[g] + r;
    best[x] = (int8_t)b; dist[x] = (uint8_t)d1; dist2[x] = (uint8_t)d2;
}

// block offsets of a call: genotype rows, tables, checks of the site counts
static int32_t phase_layout(ngsid_ctx* ctx, const u64* grp_off, const u64* site_off, uint32_t G, std::vector<u64>& geno_off, uint32_t* max_s)
{
    geno_off.assign(G + 1, 0); *max_s = 0;
    for (uint32_t g = 0; g < G; ++g) {
        if (grp_off[g + 1] < grp_off[g] || site_off[g + 1] < site_off[g]) NGSID_FAIL(ctx, NGSID_ERR_ARG, "offsets of group %u descend", g);
        const u64 S = site_off[g + 1] - site_off[g];
        if (S > NGSID_PHASE_MAX_SITES) NGSID_FAIL(ctx, NGSID_ERR_ARG, "group %u has %llu sites: at most %d", g, (unsigned long long)S, NGSID_PHASE_MAX_SITES);
        if (grp_off[g + 1] - grp_off[g] > 0xffffffffull) NGSID_FAIL(ctx, NGSID_ERR_ARG, "group %u has more than 2^32 reads", g);
        geno_off[g + 1] = geno_off[g] + (grp_off[g + 1] - grp_off[g]) * S; *max_s = std::max(*max_s, (uint32_t)S);
    }
    return NGSID_OK;
}

extern "C" int32_t ngsid_phase_genotypes(ngsid_ctx* ctx, const ngsid_reads_t* centres, const ngsid_reads_t* reads, const uint32_t* read_order,
                                         const uint64_t* grp_off, uint64_t n_groups, const ngsid_support_params_t* prm,
                                         const uint64_t* site_off, const uint32_t* site_pos, uint8_t* geno, int8_t* strand)
{
    ApiClock api_clock_(ctx, "phase_genotypes");
    if (!ctx) return NGSID_ERR_ARG;
    if (!grp_off || !site_off) NGSID_FAIL(ctx, NGSID_ERR_ARG, "null argument");
    const uint32_t G = (uint32_t)n_groups;
    std::vector<u64> geno_off; uint32_t max_s = 0;
    DevBuf<u64> d_site_off, d_geno_off; DevBuf<uint32_t> d_site_pos, d_pair_x; DevBuf<uint8_t> d_geno; std::vector<uint32_t> pair_x; bool started = false; int lp_shift = 0;
    auto init = [&](const RecPlan& P) -> int32_t {
        int32_t rc = phase_layout(ctx, grp_off, site_off, G, geno_off, &max_s); if (rc) return rc;
        if (site_off[G] && !site_pos) NGSID_FAIL(ctx, NGSID_ERR_ARG, "null site_pos");
        if (geno_off[G] && !geno) NGSID_FAIL(ctx, NGSID_ERR_ARG, "null geno");
        for (uint32_t g = 0; g < G; ++g) for (u64 i = site_off[g]; i < site_off[g + 1]; ++i) {
            if (site_pos[i] >= P.boff[g + 1] - P.boff[g]) NGSID_FAIL(ctx, NGSID_ERR_ARG, "site %u of group %u lies beyond its centre of %llu bases", site_pos[i], g, (unsigned long long)(P.boff[g + 1] - P.boff[g]));
            if (i > site_off[g] && site_pos[i] <= site_pos[i - 1]) NGSID_FAIL(ctx, NGSID_ERR_ARG, "the sites of group %u are not strictly ascending", g);
        }
        if (geno_off[G]) memset(geno, NGSID_GENO_NONE, geno_off[G]);
        return NGSID_OK;
    };
    auto start = [&](const RecPlan& P) -> int32_t {
        if (!geno_off[G]) return NGSID_OK;                                        // no site anywhere: the strands are the whole result
        int32_t rc;
        if ((rc = dev_put(ctx, d_site_off, site_off, (size_t)G + 1)) || (rc = dev_put(ctx, d_geno_off, geno_off.data(), (size_t)G + 1)) ||
            (rc = dev_put(ctx, d_site_pos, site_pos, (size_t)site_off[G]))) return rc;
        pair_x.resize(P.NP);                                                      // position of every pair's read in the list of its group
        for (u64 p = 0; p < P.NP; ++p) pair_x[p] = (uint32_t)(P.pair_x[p] - grp_off[P.pair_group[p]]);
        NGSID_TRY(dev_put(ctx, d_pair_x, pair_x.data(), pair_x.size()));
        HIPCHK(ctx, d_geno.alloc(geno_off[G]));
        HIPCHK(ctx, hipMemsetAsync(d_geno.p, NGSID_GENO_NONE, geno_off[G], ctx->stream));
        while ((1u << lp_shift) < max_s) ++lp_shift;
        started = true; return NGSID_OK;
    };
    auto chunk = [&](const RecPlan& P, const RecChunk& C) -> int32_t {
        if (!started) return NGSID_OK;
        const u64 np = C.c1 - C.c0, blocks = ((np << lp_shift) + PHASE_THREADS - 1) / PHASE_THREADS;
        { ProfScope ps_(ctx, "k_phase_gather");
          hipLaunchKernelGGL(k_phase_gather, dim3(NGSID_GRID(ctx, blocks, PHASE_THREADS, "k_phase_gather")), dim3(PHASE_THREADS), 0, ctx->stream, C.rec, P.stride, C.span, P.d_pair_group + C.c0, d_pair_x.p + C.c0, np, lp_shift,
                             d_site_off.p, d_site_pos.p, d_geno_off.p, P.d_cen_seq, P.d_cen_off, d_geno.p); }
        HIPCHK(ctx, hipGetLastError());
        return NGSID_OK;
    };
    int32_t rc = ngsid_rec_walk(ctx, centres, reads, read_order, grp_off, n_groups, prm, strand, init, start, chunk); if (rc) return rc;
    if (!started) return NGSID_OK;
    NGSID_TRY(dev_get(ctx, geno, d_geno.p, geno_off[G]));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return NGSID_OK;
}

extern "C" int32_t ngsid_phase_pair_tables(ngsid_ctx* ctx, const uint8_t* geno, const uint64_t* grp_off, const uint64_t* site_off, uint64_t n_groups, uint32_t* tables)
{
    ApiClock api_clock_(ctx, "phase_pair_tables");
    if (!ctx) return NGSID_ERR_ARG;
    if (!grp_off || !site_off) NGSID_FAIL(ctx, NGSID_ERR_ARG, "null argument");
    const uint32_t G = (uint32_t)n_groups;
    std::vector<u64> geno_off; uint32_t max_s = 0;
    int32_t rc = phase_layout(ctx, grp_off, site_off, G, geno_off, &max_s); if (rc) return rc;
    std::vector<u64> tab_off(G + 1, 0);
    for (uint32_t g = 0; g < G; ++g) { const u64 S = site_off[g + 1] - site_off[g]; tab_off[g + 1] = tab_off[g] + S * S * PHASE_CELLS; }
    if ((geno_off[G] && !geno) || (tab_off[G] && !tables)) NGSID_FAIL(ctx, NGSID_ERR_ARG, "null argument");
    if (tab_off[G]) memset(tables, 0, sizeof(uint32_t) * tab_off[G]);
    std::vector<uint32_t> items;
    for (uint32_t g = 0; g < G; ++g) {
        const uint32_t S = (uint32_t)(site_off[g + 1] - site_off[g]), npair = S * (S - 1) / 2; const u64 R = grp_off[g + 1] - grp_off[g];
        if (S < 2) continue;
        for (uint32_t k = 0; k < npair; k += PHASE_PAIRS) for (u64 r = 0; r < R; r += PHASE_SLICE) { items.push_back(g); items.push_back(k); items.push_back((uint32_t)r); items.push_back((uint32_t)std::min<u64>(R, r + PHASE_SLICE)); }
    }
    if (items.empty()) return NGSID_OK;
    DevBuf<uint8_t> d_geno; DevBuf<u64> d_geno_off, d_site_off, d_tab_off; DevBuf<uint32_t> d_items, d_tables;
    if ((rc = dev_put(ctx, d_geno, geno, (size_t)geno_off[G])) || (rc = dev_put(ctx, d_geno_off, geno_off.data(), (size_t)G + 1)) || (rc = dev_put(ctx, d_site_off, site_off, (size_t)G + 1)) ||
        (rc = dev_put(ctx, d_tab_off, tab_off.data(), (size_t)G + 1)) || (rc = dev_put(ctx, d_items, items.data(), items.size()))) return rc;
    HIPCHK(ctx, d_tables.alloc(tab_off[G]));
    HIPCHK(ctx, hipMemsetAsync(d_tables.p, 0, sizeof(uint32_t) * tab_off[G], ctx->stream));
    { ProfScope ps_(ctx, "k_phase_pairs");
      hipLaunchKernelGGL(k_phase_pairs, dim3(NGSID_GRID(ctx, items.size() / 4, PHASE_THREADS, "k_phase_pairs")), dim3(PHASE_THREADS), 0, ctx->stream, d_geno.p, d_geno_off.p, d_site_off.p, d_tab_off.p, d_items.p, d_tables.p); }
    HIPCHK(ctx, hipGetLastError());
    NGSID_TRY(dev_get(ctx, tables, d_tables.p, tab_off[G]));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return NGSID_OK;
}

extern "C" int32_t ngsid_phase_assign(ngsid_ctx* ctx, const uint8_t* geno, const uint64_t* grp_off, const uint64_t* site_off, uint64_t n_groups,
                                      const uint64_t* hap_off, const uint8_t* hap_alleles, int8_t* best, uint8_t* dist, uint8_t* dist2)
{
    ApiClock api_clock_(ctx, "phase_assign");
    if (!ctx) return NGSID_ERR_ARG;
    if (!grp_off || !site_off || !hap_off) NGSID_FAIL(ctx, NGSID_ERR_ARG, "null argument");
    const uint32_t G = (uint32_t)n_groups;
    std::vector<u64> geno_off; uint32_t max_s = 0;
    int32_t rc = phase_layout(ctx, grp_off, site_off, G, geno_off, &max_s); if (rc) return rc;
    std::vector<u64> hal_off(G + 1, 0);
    for (uint32_t g = 0; g < G; ++g) {
        if (hap_off[g + 1] < hap_off[g]) NGSID_FAIL(ctx, NGSID_ERR_ARG, "hap_off descends at group %u", g);
        const u64 H = hap_off[g + 1] - hap_off[g];
        if (H > NGSID_PHASE_MAX_HAPS) NGSID_FAIL(ctx, NGSID_ERR_ARG, "group %u has %llu haplotypes: at most %d", g, (unsigned long long)H, NGSID_PHASE_MAX_HAPS);
        hal_off[g + 1] = hal_off[g] + H * (site_off[g + 1] - site_off[g]);
    }
    const u64 NL = grp_off[G];
    if ((geno_off[G] && !geno) || (hal_off[G] && !hap_alleles) || (NL && (!best || !dist || !dist2))) NGSID_FAIL(ctx, NGSID_ERR_ARG, "null argument");
    if (NL) { memset(best, 0xff, NL); memset(dist, 0xff, NL); memset(dist2, 0xff, NL); }
    std::vector<uint32_t> items;
    for (uint32_t g = 0; g < G; ++g) {
        if (hap_off[g + 1] == hap_off[g] || site_off[g + 1] == site_off[g]) continue;          // no haplotype, or no site: -1 / 255 / 255
        for (u64 r = 0; r < grp_off[g + 1] - grp_off[g]; r += PHASE_THREADS) { items.push_back(g); items.push_back((uint32_t)r); }
    }
    if (items.empty()) return NGSID_OK;
    DevBuf<uint8_t> d_geno, d_hal, d_dist, d_dist2; DevBuf<int8_t> d_best; DevBuf<u64> d_geno_off, d_grp_off, d_site_off, d_hap_off, d_hal_off; DevBuf<uint32_t> d_items;
    if ((rc = dev_put(ctx, d_geno, geno, (size_t)geno_off[G])) || (rc = dev_put(ctx, d_geno_off, geno_off.data(), (size_t)G + 1)) || (rc = dev_put(ctx, d_grp_off, grp_off, (size_t)G + 1)) ||
        (rc = dev_put(ctx, d_site_off, site_off, (size_t)G + 1)) || (rc = dev_put(ctx, d_hap_off, hap_off, (size_t)G + 1)) || (rc = dev_put(ctx, d_hal_off, hal_off.data(), (size_t)G + 1)) ||
        (rc = dev_put(ctx, d_hal, hap_alleles, (size_t)hal_off[G])) || (rc = dev_put(ctx, d_items, items.data(), items.size()))) return rc;
    HIPCHK(ctx, d_best.alloc(NL)); HIPCHK(ctx, d_dist.alloc(NL)); HIPCHK(ctx, d_dist2.alloc(NL));
    HIPCHK(ctx, hipMemsetAsync(d_best.p, 0xff, NL, ctx->stream)); HIPCHK(ctx, hipMemsetAsync(d_dist.p, 0xff, NL, ctx->stream)); HIPCHK(ctx, hipMemsetAsync(d_dist2.p, 0xff, NL, ctx->stream));
    { ProfScope ps_(ctx, "k_phase_assign");
      hipLaunchKernelGGL(k_phase_assign, dim3(NGSID_GRID(ctx, items.size() / 2, PHASE_THREADS, "k_phase_assign")), dim3(PHASE_THREADS), 0, ctx->stream, d_geno.p, d_geno_off.p, d_grp_off.p, d_site_off.p, d_hap_off.p, d_hal_off.p, d_hal.p,
                         d_items.p, d_best.p, d_dist.p, d_dist2.p); }
    HIPCHK(ctx, hipGetLastError());
    NGSID_TRY(dev_get(ctx, best, d_best.p, NL)); NGSID_TRY(dev_get(ctx, dist, d_dist.p, NL)); NGSID_TRY(dev_get(ctx, dist2, d_dist2.p, NL));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return NGSID_OK;
}
