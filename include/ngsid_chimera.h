/* ngsid_chimera.h - the two-parent (PCR chimera) model of a set of sequences against candidate parents, on top of include/ngsid.h.
 *
 * Additive: ngsid_abi_version() stays 2.  The call has no twin in the CPU oracle - its definition is restated by the tests in numpy
 * (tests/chimera_reference.py).  The library returns integers only; which parents are offered to a query (abundance skew, both strands) and which
 * result is called a chimera (gain, model distance, position of the breakpoint) is policy and lives in the binding layer (ngspeciesid_amd/chimera.py). */
#ifndef NGSID_CHIMERA_H
#define NGSID_CHIMERA_H
#include "ngsid.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NGSID_CHIMERA_NFIELD 7          /* one_pair, one_cost, two_cost, pair_a, pair_b, bp_lo, bp_hi */
#define NGSID_CHIMERA_ROWS   12         /* R: parent rows a lane of k_chimera_profile owns */
#define NGSID_CHIMERA_STRIP  (64 * NGSID_CHIMERA_ROWS)      /* parent rows one pass of a wave covers; longer parents run in further strips */
#define NGSID_CHIMERA_LDS_QUERY 2048    /* queries up to this many bases are staged in LDS, longer ones are read through the caches */

/* Definition.  Sequences are upper-case ACGTN; two letters are equal iff the bytes are equal (N equals only N).  ed = unit-cost edit distance.
 * For a query q of length n and a parent p of length m:
 *   F_p[i] = min over 0 <= j <= m of ed(q[0:i], p[0:j])      i = 0 .. n     (F_p[0] = 0)
 *   B_p[i] = min over 0 <= j <= m of ed(q[i:n], p[j:m])      i = 0 .. n     (B_p[n] = 0)
 * (B_p is F of the reversed strings, read backwards.)
 *
 * The pairs are a CSR: pair_off[n_queries + 1] (ascending, pair_off[0] = 0), pair_parent[n_pairs] (an index into `parents`), pair_gid[n_pairs] (int32; NULL: the
 * gid of a pair is its parent index).  The pairs of a query are numbered 0 .. P-1 in row order.
 *   one-parent model: one_cost = min over k of F_k[n]; one_pair = the smallest k that attains it.
 *   two-parent model: two_cost = min of F_a[i] + B_b[i] over 0 <= i <= n and over pairs a, b with gid[a] != gid[b];
 *     bp_lo            = the smallest i at which some admissible (a, b) attains two_cost;
 *     (pair_a, pair_b) = the lexicographically smallest admissible pair that attains it at bp_lo;
 *     bp_hi            = the largest i with F_pair_a[i] + B_pair_b[i] == two_cost.
 *   i = n is admissible (B[n] = 0), so with two or more gids two_cost <= one_cost: the gain one_cost - two_cost is >= 0.
 * fields[q][0 .. 7) = one_pair, one_cost, two_cost, pair_a, pair_b, bp_lo, bp_hi.  A query without a pair has all seven -1; a query whose pairs share one gid
 * has the last five -1.
 * Legal: empty query sets, sequences of length 0 (the formulas hold as they stand), identical parents (the smaller pair index wins), a parent equal to the query.
 * Bounds: every sequence has at most NGSID_MAX_CONSENSUS_LEN bases (so every cost fits uint16); n_pairs < 2^31.
 *
 * profiles (uint16, may be NULL): the blocks of the pairs follow each other in pair order; the block of pair k of a query of n bases is F_k[0 .. n] followed by
 * B_k[0 .. n], 2 (n + 1) values.  With it a wrong result can be pinned on the DP kernel or on the reduction.
 * The profiles live in grow-only context scratch (returned by option "release_scratch"); the queries run in chunks sized from a share of the free device memory
 * (option "chimera_chunk_queries" fixes the queries per chunk).  Results never depend on it.
 *
 * queries / parents are host- or device-resident read sets (qual ignored); the pair arrays are host arrays.
 * Profiling lines (ngsid_profile_read): k_chimera_check, k_chimera_profile, k_chimera_reduce.
 * Errors: NGSID_ERR_ARG (null argument, pair_off not starting at 0 or decreasing, a parent index out of range, 2^31 or more pairs), NGSID_ERR_ALPHABET (anything
 * but upper-case ACGTN), NGSID_ERR_TOO_LONG (a sequence above NGSID_MAX_CONSENSUS_LEN), NGSID_ERR_HIP. */
int32_t ngsid_chimera_model(ngsid_ctx* ctx, const ngsid_reads_t* queries, const ngsid_reads_t* parents,
                            const uint64_t* pair_off /* [n_queries + 1] */, const uint32_t* pair_parent /* [n_pairs] */, const int32_t* pair_gid /* [n_pairs], may be NULL */,
                            int32_t* fields /* [n_queries][NGSID_CHIMERA_NFIELD] */, uint16_t* profiles /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif
