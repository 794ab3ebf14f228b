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

#ifdef __cplusplus
}
#endif
#endif
