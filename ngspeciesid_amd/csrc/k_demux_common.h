// k_demux_common.h - what k_demux_locate (k_demux.hip) and k_demux_scan (k_demux_scan.hip) share: the column, the match masks and their staging, the lane map, and the
// host function that checks and uploads a tag / pattern set.
//
// The column is ngsid_host_infix_locate's (host_io.hip) for patterns of at most 64 letters: ONE 64-bit Myers / Hyyro word per pattern and lane, free start in the text, the
// same 64-bit expressions as the host function, so every score of the last row is the host's.  dmx_step is the only place in the device code where they stand.
// Lane mapping.  One pattern per lane.  Tp = the pattern count rounded up to a power of two (64 when there are 64 or more); a wave holds G <= 64 / Tp texts (read-sides for
// locate, reads for scan), lane = g * Tp + slot; a lane with g >= G (G capped by the kernel's LDS) belongs to no group.  A batch is the DMX_WAVES x G texts of one workgroup.
// Above 64 patterns the list is walked in passes of 64 (pattern = pass * 64 + slot).
// LDS per workgroup (4 waves): the match masks of the current pass, [5 text letters A C G T N][64 slots] x 8 B = 2 560 B, shared by the workgroup - the text letter of a step
// is uniform within a group, so the 64-bit read is conflict-free for G = 1 - and behind them DMX_WAVES x G x (bytes per text) of letter codes, private to each wave (at most 32 KB).
#pragma once
#include "ngsid_host.h"
#include "../../include/ngsid_demux.h"
#include <algorithm>

typedef unsigned long long u64;

#define DMX_WAVES 4
#define DMX_THREADS (DMX_WAVES * 64)
#define DMX_PEQ_WORDS (5 * 64)                              // the masks of one pass: [5 letters][64 slots]
#define DMX_PEQ_BYTES (DMX_PEQ_WORDS * sizeof(u64))         // 2 560 B in front of the letter codes

static_assert(NGSID_DEMUX_MAX_TAG_LEN == 64, "one-word columns");

// letter code of the reverse-complemented text: A <-> T, C <-> G, N stays
__device__ __forceinline__ uint32_t dmx_code(uint8_t c, int complement)
{
    const uint32_t k = ngsid_base_code(c);
    return (complement && k < 4u) ? 3u - k : k;
}

// ---- the column of a pattern of m letters: starts as { ones, 0, m }
struct DmxColumn { u64 Pv, Mv; int score; };

// one text letter (Eq = the pattern's match mask for it; top = m - 1, the bit of the last row) -> the column behind it.  ANCHORED: the alignment starts at the first letter
// of the text (row 0 rises by one per column), else anywhere.  The state goes in and out by value and top is the bit's index, not its mask: with the state behind a reference
// or the mask tested, hipcc adds a v_min per column to k_demux_locate and two VGPRs (profiles/demux_common_isa.txt)
template <bool ANCHORED>
__device__ __forceinline__ DmxColumn dmx_step(DmxColumn s, u64 Eq, int top)
{
    u64 &Pv = s.Pv, &Mv = s.Mv;
    const u64 Xv = Eq | Mv;
    const u64 Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
    u64 Ph = Mv | ~(Xh | Pv), Mh = Pv & Xh;
    s.score += (int)((Ph >> top) & 1); s.score -= (int)((Mh >> top) & 1);
    Ph = ANCHORED ? (Ph << 1) | 1ull : Ph << 1; Mh <<= 1;
    Pv = Mh | ~(Xv | Ph); Mv = Ph & Xv;
    return s;
}

// ---- the masks in the LDS: a one-pass list is staged once, in front of the batch loop (dmx_peq_preload); a longer one per pass, between two workgroup barriers (dmx_peq_reload)
__device__ __forceinline__ void dmx_peq_load(u64* s_peq, const u64* peq /* [npass][5][64] */, int pass)
{
    peq += (size_t)pass * DMX_PEQ_WORDS;
    for (int i = threadIdx.x; i < DMX_PEQ_WORDS; i += DMX_THREADS) s_peq[i] = peq[i];
}
__device__ __forceinline__ void dmx_peq_preload(u64* s_peq, const u64* peq, int npass) { if (npass == 1) { dmx_peq_load(s_peq, peq, 0); __syncthreads(); } }
__device__ __forceinline__ void dmx_peq_reload(u64* s_peq, const u64* peq, int npass, int pass) { if (npass > 1) { __syncthreads(); dmx_peq_load(s_peq, peq, pass); __syncthreads(); } }

// ---- the lane map
struct DmxLanes { int lane, wave, Tp, g, slot; bool in_group; };
__device__ __forceinline__ DmxLanes dmx_lanes(int logTp, int G)
{
    DmxLanes m;
    m.lane = threadIdx.x & 63; m.wave = threadIdx.x >> 6;
    m.Tp = 1 << logTp; m.g = m.lane >> logTp; m.slot = m.lane & (m.Tp - 1);
    m.in_group = m.g < G;
    return m;
}
__host__ __device__ __forceinline__ u64 dmx_nbatch(u64 ntext, int G) { const u64 per_batch = (u64)DMX_WAVES * G; return (ntext + per_batch - 1) / per_batch; }
__device__ __forceinline__ int dmx_wave_max(int v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d));
    return v;
}

// ---- host: the tag / pattern set of a call, checked (a host read set of 1 .. max_n entries, none empty, none longer than NGSID_DEMUX_MAX_TAG_LEN; noun / nouns name it in
// the messages) and on the device: the match masks per (pattern, text letter) by ngsid_iupac_eq, laid out as the kernels stage them, and the lengths [npass * 64], 0 = no pattern
struct DmxPatterns { DevBuf<u64> d_peq; DevBuf<int32_t> d_len; int n = 0, npass = 0, logTp = 0; std::vector<u64> h_peq; std::vector<int32_t> h_len; };      // h_*: the source of the asynchronous copies
static inline int32_t dmx_patterns(ngsid_ctx* ctx, const ngsid_reads_t* set, int max_n, int iupac, const char* noun, const char* nouns, DmxPatterns& P)
{
    if (set->mem != NGSID_MEM_HOST) NGSID_FAIL(ctx, NGSID_ERR_ARG, "the %s are a host read set", nouns);
    if (set->n == 0 || set->n > (uint64_t)max_n) NGSID_FAIL(ctx, NGSID_ERR_ARG, "1 .. %d %s expected", max_n, nouns);
    if (!set->off || !set->seq) NGSID_FAIL(ctx, NGSID_ERR_ARG, "null %s set", noun);
    P.n = (int)set->n; P.npass = (P.n + 63) / 64;
    while ((1 << P.logTp) < std::min(P.n, 64)) ++P.logTp;
    P.h_peq.assign((size_t)P.npass * DMX_PEQ_WORDS, 0); P.h_len.assign((size_t)P.npass * 64, 0);
    for (int t = 0; t < P.n; ++t) {
        if (set->off[t + 1] <= set->off[t]) NGSID_FAIL(ctx, NGSID_ERR_ARG, "%s %d is empty", noun, t);
        if (set->off[t + 1] - set->off[t] > NGSID_DEMUX_MAX_TAG_LEN) NGSID_FAIL(ctx, NGSID_ERR_TOO_LONG, "%s %d is longer than %d", noun, t, NGSID_DEMUX_MAX_TAG_LEN);
        const uint8_t* q = set->seq + set->off[t]; const int m = (int)(set->off[t + 1] - set->off[t]);
        P.h_len[t] = m;
        for (int c = 0; c < 5; ++c) { u64 v = 0; for (int i = 0; i < m; ++i) if (ngsid_iupac_eq(q[i], (uint8_t)"ACGTN"[c], iupac)) v |= 1ull << i; P.h_peq[((size_t)(t >> 6) * 5 + c) * 64 + (t & 63)] = v; }
    }
    NGSID_TRY(dev_put(ctx, P.d_peq, P.h_peq.data(), P.h_peq.size())); NGSID_TRY(dev_put(ctx, P.d_len, P.h_len.data(), P.h_len.size()));
    return NGSID_OK;
}
