/* ngsid_near.h - which sequences lie within a few edits of each other, on either strand: a banded unit-cost edit distance for listed pairs and for all pairs of a set,
 * on top of include/ngsid.h.
 *
 * Additive: ngsid_abi_version() stays 2.  The calls have no twin in the CPU oracle - their definition is restated by the tests in numpy (tests/variants_reference.py).
 * The library returns integers only; what a variant is (the identity threshold per pair, abundance-ordered centroids, the tables) is policy and lives in the binding
 * layer (ngspeciesid_amd/variants.py). */
#ifndef NGSID_NEAR_H
#define NGSID_NEAR_H
#include "ngsid.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NGSID_NEAR_MAX_DIST 31          /* largest max_dist: the band of k_near is one 64-bit word per lane, rows c - 31 .. c + 32 of column c */
#define NGSID_NEAR_WIDE_MAX_DIST 255 /* largest max_dist of the wide calls: up to eight band words per lane, a band of W words holds 32 W - 1 edits */
#define NGSID_NEAR_BOTH_STRANDS 1u      /* flags: also compare against the reverse complement */

/* Definition.  Sequences are upper-case ACGTN; two letters are equal iff the bytes are equal (N equals only N).  ed = unit-cost global edit distance (both sequences
 * end to end).  rc = reverse complement, the complement of N is N.
 *   with NGSID_NEAR_BOTH_STRANDS: D(a, b) = min(ed(a, b), ed(a, rc(b))); strand = 0 if ed(a, b) attains the minimum (a tie goes to forward), else 1;
 *   without:                      D(a, b) = ed(a, b), strand = 0.
 * (ed(a, rc(b)) = ed(rc(a), b): D is symmetric.)
 * Legal: empty sets, one sequence, sequences of length 0 (ed("", x) = |x|), identical sequences (distance 0), a sequence equal to its own reverse complement (strand 0).
 * Bounds: every sequence has at most NGSID_MAX_CONSENSUS_LEN bases; fewer than 2^32 sequences per set; 0 <= max_dist <= NGSID_NEAR_MAX_DIST.
 * Read sets are host- or device-resident (qual ignored); every other array is a host array.
 * Scratch (grow-only, in the context; returned by option "release_scratch"): the letter planes a call reads - pattern planes of the queries (three bits per base and
 * 78 words per sequence, padded for the widest band of the wide calls) and text planes of the targets (six bits per base: both strands), both kinds for the set of
 * ngsid_near_pairs - and the found pairs (ten bytes each).  Work runs in chunks: option "near_chunk_pairs" fixes the listed pairs per launch of ngsid_ed_within_batch, option "near_chunk_seqs" the sequences
 * (rows of the pair triangle) per launch of ngsid_near_pairs; by default the chunks are sized from the launch limits and from a share of the free device memory.
 * Results never depend on it.
 * Profiling lines (ngsid_profile_read): k_near_check, k_near_pack, k_near_within, k_near_tiles.
 * Errors: NGSID_ERR_ARG (null argument, max_dist outside 0 .. 31, an index out of range, 2^32 or more sequences), NGSID_ERR_ALPHABET (anything but upper-case ACGTN),
 * NGSID_ERR_TOO_LONG (a sequence above NGSID_MAX_CONSENSUS_LEN), NGSID_ERR_CAPACITY (ngsid_near_pairs: more pairs than cap), NGSID_ERR_HIP. */

/* Listed pairs: dist[p] = D(queries[q_idx[p]], targets[t_idx[p]]) if that is <= max_dist, else -1; strand[p] (may be NULL) by the rule above, 0 where dist[p] is -1. */
int32_t ngsid_ed_within_batch(ngsid_ctx* ctx, const ngsid_reads_t* queries, const ngsid_reads_t* targets,
                              const uint32_t* q_idx /* [n_pairs] */, const uint32_t* t_idx /* [n_pairs] */, uint64_t n_pairs,
                              int32_t max_dist, uint32_t flags, int32_t* dist /* [n_pairs] */, uint8_t* strand /* [n_pairs], may be NULL */);

/* All pairs: every i < j of seqs with D(s_i, s_j) <= max_dist, in ascending (i, j) order, in the caller's numbering: pair_i, pair_j, dist, strand [*n_found].
 * *needed = the number of such pairs, always.  More pairs than cap: NGSID_ERR_CAPACITY, *n_found = 0, nothing written (cap = 0 with NULL arrays asks for the count).
 * The candidate pairs are enumerated on the device (the set sorted by length, tiles of one sequence against 64 of the next longer ones; tiles beyond a length
 * difference of max_dist do not exist); only the found pairs come back. */
int32_t ngsid_near_pairs(ngsid_ctx* ctx, const ngsid_reads_t* seqs, int32_t max_dist, uint32_t flags,
                         uint32_t* pair_i, uint32_t* pair_j, uint8_t* dist, uint8_t* strand /* [cap] each */, uint64_t cap, uint64_t* n_found, uint64_t* needed);

/* The wide calls: the two calls above, word for word - D, the strand and tie rule, N, empty sequences, the ascending (i, j) order, the cap / needed protocol, the options
 * and the error codes - with the range 0 <= max_dist <= NGSID_NEAR_WIDE_MAX_DIST.  The band is 2, 4 or 8 words per lane, the smallest that holds max_dist (63, 127,
 * 255 edits); for max_dist <= NGSID_NEAR_MAX_DIST they run the one-word instance, as the calls above do, and return exactly what those return.  Scratch: the
 * same planes and records.  Profiling lines above NGSID_NEAR_MAX_DIST: k_near_within_wide, k_near_tiles_wide; k_near_check and k_near_pack are shared. */
int32_t ngsid_ed_within_wide_batch(ngsid_ctx* ctx, const ngsid_reads_t* queries, const ngsid_reads_t* targets,
                                   const uint32_t* q_idx /* [n_pairs] */, const uint32_t* t_idx /* [n_pairs] */, uint64_t n_pairs,
                                   int32_t max_dist, uint32_t flags, int32_t* dist /* [n_pairs] */, uint8_t* strand /* [n_pairs], may be NULL */);
int32_t ngsid_near_pairs_wide(ngsid_ctx* ctx, const ngsid_reads_t* seqs, int32_t max_dist, uint32_t flags,
                              uint32_t* pair_i, uint32_t* pair_j, uint8_t* dist, uint8_t* strand /* [cap] each */, uint64_t cap, uint64_t* n_found, uint64_t* needed);

#ifdef __cplusplus
}
#endif
#endif
