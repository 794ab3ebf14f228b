/* ngsid_demux.h - sample tags of pooled reads located on the device, on top of include/ngsid.h.
 *
 * Additive: ngsid_abi_version() stays 2.  The call has no twin in the CPU oracle - its definition is restated by the tests from the host locator
 * (tests/demux_reference.py: windows and reverse complements in numpy, every (window, tag) pair through ngsid_host_infix_locate / ongsid_host_infix_locate,
 * the reduction in numpy).  The library returns integers only; which read goes to which sample is policy and lives in the binding layer
 * (ngspeciesid_amd/demux.py). */
#ifndef NGSID_DEMUX_H
#define NGSID_DEMUX_H
#include "ngsid.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int32_t window;    /* 1 .. NGSID_DEMUX_MAX_WINDOW: bases of a read end that are searched */
    int32_t max_ed;    /* >= 0: a tag further than this from every infix of the window is not a hit */
    int32_t iupac;     /* != 0: the IUPAC equalities of ngsid_host_infix_locate (symmetric, not transitive; N and X = any of ACGT) */
} ngsid_demux_params_t;

#define NGSID_DEMUX_MAX_TAG_LEN 64
#define NGSID_DEMUX_MAX_WINDOW 256
#define NGSID_DEMUX_MAX_TAGS 4096
#define NGSID_DEMUX_NFIELD 5       /* tag, ed, start, end, ed2 */

/* For every read, both sides and every tag: the infix location of the tag in the side's window; per (read, side) the best tag.
 *
 * Side 0 window = read[0 : min(window, L)].  Side 1 window = the first min(window, L) bases of the reverse complement of the read (N stays N); side 1
 * positions are in reverse-complement coordinates, so on either side the tag sits at the head and the inner cut is end + 1.
 * Location of tag t in window w = exactly ngsid_host_infix_locate(t, len, w, wlen, max_ed, iupac): unit costs, window ends free; ed = the smallest
 * distance (only a value below the tag length counts), end = the first window position at which an alignment with that distance ends, start = the
 * smallest start of such an alignment; all -1 without a hit within max_ed, or when the window is empty.
 *
 * reads: upper-case ACGTN (NGSID_ERR_ALPHABET otherwise), host- or device-resident.  tags: a host read set (qual ignored) of 1 .. NGSID_DEMUX_MAX_TAGS
 * sequences of 1 .. NGSID_DEMUX_MAX_TAG_LEN upper-case letters.
 *
 * hits[(r * 2 + side) * 5 + f] (int32):  f = 0 tag = index of the smallest ed, on equal ed the smallest index, -1 if no tag hits; 1, 2, 3 = ed, start, end of
 * that tag; 4 ed2 = the smallest ed among the OTHER tags that hit, -1 if none does (a tie for the best gives ed2 == ed).
 * ed_all / end_all (each may be NULL; int16 [n][2][T]): ed and end of every tag.  With them the call runs in chunks of reads under a share of the free
 * device memory (option "demux_chunk_reads" fixes the chunk); results never depend on the chunking.
 * Empty read sets, reads of length 0 or 1 and T = 1 are legal.
 *
 * One 64-bit Myers / Hyyro column per tag and lane (k_demux.hip).  Profiling line (ngsid_profile_read): k_demux_locate.
 * Errors: NGSID_ERR_ARG (window or max_ed out of range, no tag, an empty tag, too many tags), NGSID_ERR_TOO_LONG (a tag above 64 bases),
 * NGSID_ERR_ALPHABET, NGSID_ERR_HIP. */
int32_t ngsid_demux_locate(ngsid_ctx* ctx, const ngsid_reads_t* reads, const ngsid_reads_t* tags, const ngsid_demux_params_t* prm,
                           int32_t* hits, int16_t* ed_all, int16_t* end_all);

typedef struct {
    int32_t max_ed;    /* >= 0: a position whose last-row score is above min(max_ed, pattern length - 1) belongs to no run */
    int32_t iupac;     /* != 0: the IUPAC equalities of ngsid_host_infix_locate */
} ngsid_demux_scan_params_t;

#define NGSID_DEMUX_SCAN_NFIELD 3  /* pattern, end, ed */

/* For every read and every pattern: every place in the WHOLE read where the pattern occurs within max_ed edits.
 *
 * Pattern p of m letters against read x of L letters, unit costs, equality as in ngsid_demux_locate (bytes, or the IUPAC rule with iupac != 0):
 *   D[0][j] = 0 (j = 0 .. L), D[i][0] = i, D[i][j] = min(D[i-1][j-1] + [p[i-1] != x[j-1]], D[i-1][j] + 1, D[i][j-1] + 1);
 *   s[j] = D[m][j+1] (j = 0 .. L-1): the smallest distance of p to an infix of x that ends at j;  k = min(max_ed, m - 1).
 * A run is a maximal interval of consecutive positions j with s[j] <= k.  Every run yields exactly one hit: ed = the minimum of s over the run, end = the smallest j
 * of the run with s[j] == ed.  A run still open at the last base is closed there.  A pattern may have several hits in a read; positions are in the read's own forward
 * coordinates, and the call knows nothing of strands: reverse complements are patterns of their own.
 * Where a (read, pattern) pair has a hit, its hit with the smallest (ed, end) has the ed and end of ngsid_host_infix_locate(p, m, x, L, max_ed, iupac, ...).
 *
 * reads: upper-case ACGTN (NGSID_ERR_ALPHABET otherwise), host- or device-resident, each up to NGSID_MAX_READ_LEN.  patterns: a host read set (qual ignored) of
 * 1 .. 2 * NGSID_DEMUX_MAX_TAGS sequences of 1 .. NGSID_DEMUX_MAX_TAG_LEN upper-case letters.
 *
 * CSR result: the hits of read r are hit[hit_off[r] .. hit_off[r + 1]), hit[h * 3 + f] (int32): f = 0 pattern, 1 end, 2 ed; within a read in ascending (end, pattern)
 * order.  hit_off holds n + 1 entries, hit has room for cap hits.  *needed = the number of hits, always.  cap = 0 with hit_off = hit = NULL asks for the count.
 * More hits than cap: NGSID_ERR_CAPACITY, and neither array is written.
 * Empty read sets, reads of length 0 and a single pattern are legal.  The reads run in chunks under a share of the free device memory (option
 * "demux_scan_chunk_reads" fixes the chunk); results never depend on the chunking.
 *
 * One 64-bit Myers / Hyyro column per pattern and lane, the read streamed through it (k_demux_scan.hip).  Profiling line (ngsid_profile_read): k_demux_scan.
 * Errors: NGSID_ERR_ARG (max_ed negative, no pattern, an empty pattern, too many patterns, a missing array), NGSID_ERR_TOO_LONG (a pattern above 64 letters),
 * NGSID_ERR_ALPHABET, NGSID_ERR_CAPACITY, NGSID_ERR_HIP. */
int32_t ngsid_demux_scan(ngsid_ctx* ctx, const ngsid_reads_t* reads, const ngsid_reads_t* patterns, const ngsid_demux_scan_params_t* prm,
                         uint64_t* hit_off, int32_t* hit, uint64_t cap, uint64_t* needed);

#ifdef __cplusplus
}
#endif
#endif
