/* ngsid_umi.h - which short sequences (UMI keys) lie within a few edits of each other, at the scale of a run: a seeded search by the pigeonhole rule instead of
 * the all-pairs enumeration of ngsid_near_pairs, and the abundance-ordered centroid pass over the pair list; on top of include/ngsid.h.
 *
 * Additive: ngsid_abi_version() stays 2.  The calls have no twin in the CPU oracle - their definition is restated by the tests (tests/umi_reference.py).
 * The library returns integers only; what a UMI is (the flanks, the key of a read, the order of the centroids, the bins and their consensus) is policy and lives
 * in the binding layer (ngspeciesid_amd/umi.py). */
#ifndef NGSID_UMI_H
#define NGSID_UMI_H
#include "ngsid.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NGSID_UMI_MAX_LEN   64   /* letters per sequence: one 64-bit Myers word */
#define NGSID_UMI_MAX_DIST   8

typedef struct {
    int32_t max_dist;            /* 0 .. NGSID_UMI_MAX_DIST */
    int32_t seed_len;            /* 4 .. 16: letters per seed; it never changes the result, only the work */
} ngsid_umi_params_t;

/* Every i < j of seqs with ed(s_i, s_j) <= max_dist, in ascending (i, j) order: pair_i, pair_j, dist [*n_found].  The definition is that of
 * ngsid_near_pairs(seqs, max_dist, flags = 0) (include/ngsid_near.h), word for word: unit-cost global edit distance, equality by bytes (N equals only N), *needed = the
 * number of such pairs, always; more pairs than cap: NGSID_ERR_CAPACITY, *n_found = 0, nothing written (cap = 0 with NULL arrays asks for the count).
 * Input letters are upper-case ACGTN, lengths 0 .. NGSID_UMI_MAX_LEN.  Legal: empty sets, one sequence, sequences of length 0, identical sequences, any mixture of
 * lengths.  The result never depends on seed_len or on the chunking.
 *
 * The rule.  d = max_dist, g = seed_len.  A sequence is seedable when it has at least (d + 1) g letters; its seeds are the segments [j g, (j + 1) g), j = 0 .. d.  If
 * ed(A, B) <= d and A is seedable, some seed j of A occurs exactly in B at position j g + s with |s| <= d.  Every seedable sequence enters a sorted index with its
 * d + 1 seeds; every sequence B looks its substrings at j g + s up, entries of a smaller sequence index only, and each candidate pair is verified once, at its
 * first (j, s) in ascending j (2 d + 1) + s + d order, by one 64-bit Myers column.  Pairs whose smaller-index member is not seedable are compared directly, within
 * the length difference d.
 * Bounds: n (d + 1) < 2^31 sequences x seeds; at most 2^31 - 1 found pairs per call.
 * Read sets are host- or device-resident (qual ignored); every other array is a host array.
 * Scratch (grow-only, in the context; returned by option "release_scratch"): 32 bytes per sequence (three letter planes and the length), 24 bytes per seed (the
 * index and its sort buffers), 24 bytes per (query, substring) and 4 bytes per tile of 64 candidates of a chunk, and 18 bytes per found pair.  Queries run in chunks: option "umi_chunk_seqs" fixes the
 * sequences per chunk.
 * Profiling lines (ngsid_profile_read): k_umi_check (the alphabet scan), k_umi_keys, k_umi_sort (the index and its samples), k_umi_ranges (ranges and tile sums), k_umi_join (tile list and the join itself),
 * k_umi_short, k_umi_order (the found pairs into ascending order); umi_candidates (a count, not a kernel: the pairs that went through the Myers column).
 * Errors: NGSID_ERR_ARG (null argument, max_dist or seed_len out of range, too many sequences), NGSID_ERR_ALPHABET (anything but upper-case ACGTN),
 * NGSID_ERR_TOO_LONG (a sequence of more than NGSID_UMI_MAX_LEN letters), NGSID_ERR_CAPACITY, NGSID_ERR_HIP. */
int32_t ngsid_umi_pairs(ngsid_ctx* ctx, const ngsid_reads_t* seqs, const ngsid_umi_params_t* prm,
                        uint32_t* pair_i, uint32_t* pair_j, uint8_t* dist /* [cap] each */, uint64_t cap, uint64_t* n_found, uint64_t* needed);

/* Greedy centroid pass over a pair list (a host function, no context): the nodes 0 .. n - 1 are walked in `order` (a permutation); a node joins the earliest-founded
 * centroid it shares a listed pair with, otherwise it founds a bin.  bin_of[x] = the bin of node x, centroid[b] = the node that founded bin b (founding order),
 * *n_bins = the number of bins.  The pairs are unordered (i, j) with i != j, in any order; a pair listed twice counts once.  One pass over a CSR adjacency.
 * Errors: NGSID_ERR_ARG (null argument, an index out of range, i == j, order not a permutation). */
int32_t ngsid_umi_centroids(const uint32_t* pair_i, const uint32_t* pair_j, uint64_t n_pairs, const uint32_t* order /* [n] */, uint32_t n,
                            int32_t* bin_of /* [n] */, uint32_t* centroid /* [n], first *n_bins used */, uint32_t* n_bins);

#ifdef __cplusplus
}
#endif
#endif
