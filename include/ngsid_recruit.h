/* ngsid_recruit.h - every read of a sample located inside every final consensus of that sample, on both strands, and the two nearest consensuses per read reduced on
 * the device, on top of include/ngsid.h.
 *
 * Additive: ngsid_abi_version() stays 2.  The call has no twin in the CPU oracle - its definition is restated by the tests (tests/recruit_reference.py: the row-wise
 * table in numpy, anchored to ngsid_host_infix_locate / ongsid_host_infix_locate pair by pair).  The library returns integers only; which read counts for which
 * consensus (identity threshold, margin, the recount) is policy and lives in the binding layer (ngspeciesid_amd/recruit.py). */
#ifndef NGSID_RECRUIT_H
#define NGSID_RECRUIT_H
#include "ngsid.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NGSID_RECRUIT_MAX_LEN 2048     /* letters per consensus (32 band-free 64-bit words per lane) */
#define NGSID_RECRUIT_NFIELD  6        /* cons, ed, strand, end, cons2, ed2 */
#define NGSID_RECRUIT_BOTH_STRANDS 1u  /* flags: also compare the reverse complement of every consensus */

/* Definition.
 *
 * Equality and reverse complement.  Letters are upper-case ACGTN.  Two letters are equal iff their bytes are equal (the iupac = 0 rule of ngsid_host_infix_locate:
 * N equals only N).  rc = reverse complement; the reverse complement of N is N.
 *
 * Distance of one consensus strand to one read.  Pattern p (a consensus, or its reverse complement) of m letters, read x of L letters, the recurrence of
 * ngsid_demux_scan with unit costs:
 *   D[0][j] = 0 (j = 0 .. L), D[i][0] = i, D[i][j] = min(D[i-1][j-1] + [p[i-1] != x[j-1]], D[i-1][j] + 1, D[i][j-1] + 1);
 *   s[j] = D[m][j+1] (j = 0 .. L-1);  d(p, x) = min over j of s[j];  end = the smallest j attaining it, in the read's own forward coordinates on both strands;
 *   k_c = min(max_ed[c], m - 1).  The pair is a hit iff L > 0 and d <= k_c.
 * This is exactly the ed and end of ngsid_host_infix_locate(p, m, x, L, k_c, 0, ...): the pattern end to end, the read's ends free.
 *
 * Per read and consensus c of the read's group.  D(c) = min(d(c, x), d(rc(c), x)) over the strands that hit; strand = 0 if the forward strand attains the minimum
 * (a tie goes to forward, and a consensus equal to its own reverse complement is strand 0), else 1.  Without NGSID_RECRUIT_BOTH_STRANDS only the forward strand is
 * compared.
 *
 * Per read.  cons = the consensus with the smallest (D, index) among those that hit, an index into the call's consensus set; ed, strand and end are those of cons.
 * cons2 and ed2 = the smallest (D, index) among the OTHER consensuses that hit - the other strand of cons is not another consensus; an exact tie gives ed2 == ed.
 * Every field is -1 where there is nothing, except strand, which is 0.
 *
 * Arguments.  reads: host- or device-resident (qual ignored), each up to NGSID_MAX_READ_LEN letters.  Group g holds reads read_off[g] .. read_off[g + 1] - 1 and
 * consensuses cons_off[g] .. cons_off[g + 1] - 1; read_off[0] = cons_off[0] = 0, read_off[n_groups] = reads->n, cons_off[n_groups] = cons->n, both non-decreasing.
 * cons: a host read set (qual ignored) of sequences of 1 .. NGSID_RECRUIT_MAX_LEN letters.  max_ed[c] >= 0 per consensus.
 * hits[r * 6 + f] (int32): f = 0 cons, 1 ed, 2 strand, 3 end, 4 cons2, 5 ed2.
 *
 * Legal: no reads, groups with no read, groups with no consensus (all six fields of their reads are "nothing"), a group with one consensus, reads of length 0 and 1,
 * reads shorter than the consensus, identical consensuses in a group (the smaller index is cons, the other cons2 with ed2 == ed).
 *
 * The reads run in chunks under a share of the free device memory (option "recruit_chunk_reads" fixes the chunk); results never depend on the chunking.
 *
 * One lane per read, a wave of 64 consecutive reads of one group against that group's consensus strands one after the other; the column is Hyyro's block form of the
 * Myers recurrence, ceil(m / 64) words per lane held in registers (k_recruit.hip).  Profiling line (ngsid_profile_read): k_recruit.
 * Errors: NGSID_ERR_ARG (an empty consensus, a negative max_ed, offsets that are not monotone or do not cover the sets, a null array, a device-resident consensus
 * set), NGSID_ERR_TOO_LONG (a consensus above NGSID_RECRUIT_MAX_LEN, a read above NGSID_MAX_READ_LEN), NGSID_ERR_ALPHABET (anything but upper-case ACGTN in a read or
 * a consensus), NGSID_ERR_HIP.  With NGSID_ERR_ARG, NGSID_ERR_TOO_LONG and NGSID_ERR_ALPHABET hits is not written. */
int32_t ngsid_recruit(ngsid_ctx* ctx, const ngsid_reads_t* reads, const uint64_t* read_off /* [n_groups + 1] */,
                      const ngsid_reads_t* cons, const uint64_t* cons_off /* [n_groups + 1] */, uint64_t n_groups,
                      const int32_t* max_ed /* [cons->n] */, uint32_t flags, int32_t* hits /* [reads->n][6] */);

#ifdef __cplusplus
}
#endif
#endif
