/* ngsid_classify.h - consensus sequences searched against a reference library by shared minimizers, on top of include/ngsid.h.
 *
 * Additive: ngsid_abi_version() stays 2.  The calls have no twin in the CPU oracle - their definition is restated by the tests from the minimizer call
 * (tests/classify_reference.py: codes from ngsid_hpc_minimizers / ongsid_hpc_minimizers, reverse complements in numpy, Python sets, the reduction and the
 * order in numpy).  The library returns integers only; which candidate names a consensus - the verification alignment, identity, coverage, thresholds - is
 * policy and lives in the binding layer (ngspeciesid_amd/classify.py). */
#ifndef NGSID_CLASSIFY_H
#define NGSID_CLASSIFY_H
#include "ngsid.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ngsid_refdb ngsid_refdb;      /* opaque; owned by the ctx it was built in (ngsid_destroy releases what the caller did not) */

typedef struct {
    int32_t k, w;          /* 1 <= k <= 21, k <= w <= 255 as in ngsid_hpc_minimizers; codes of k > 21 are not comparable between calls: NGSID_ERR_ARG */
} ngsid_refdb_params_t;

typedef struct {
    int32_t top_k;         /* 1 .. NGSID_CLASSIFY_MAX_TOPK: candidates kept per query */
    int32_t min_shared;    /* >= 1: a reference that shares fewer minimizers is no candidate */
} ngsid_classify_params_t;

#define NGSID_CLASSIFY_MAX_TOPK 64
#define NGSID_CLASSIFY_MAX_REFS (1u << 24)

/* Definition.
 *   S(x)            = the set of DISTINCT minimizer codes ngsid_hpc_minimizers(x, k, w) returns for sequence x (homopolymer-compressed, 3 bits per base,
 *                     order preserving).  Qualities never influence a code.
 *   q_0 = q, q_1    = the reverse complement of q (N stays N).
 *   shared(q, s, r) = |S(q_s) & S(r)|: a code that occurs at several positions of a sequence counts once.
 *   shared(q, r)    = max over s of shared(q, s, r); strand(q, r) = the s that attains it, 0 on a tie.
 *   r is a candidate of q when shared(q, r) >= min_shared.  The candidates of q are ordered by (shared descending, r ascending); the first top_k of them fill
 *   cand_ref / cand_shared / cand_strand [q][0 .. top_k), the rest of the row is -1 / -1 / -1.
 *   n_codes[q][s]   = |S(q_s)| (may be NULL).
 * Legal: empty query sets, queries or references without a minimizer (shorter than k after compression), top_k above the number of references, identical
 * references (the smaller index comes first).
 *
 * ngsid_refdb_build: refs is a HOST read set (qual ignored) of 1 .. NGSID_CLASSIFY_MAX_REFS sequences.  The library keeps on the device: the sorted distinct
 *   codes of all references, their posting offsets, and the postings (uint32 reference indices, ascending within a code); *out is valid until
 *   ngsid_refdb_release or ngsid_destroy of ctx, and is searched through ctx only.
 * ngsid_refdb_info: sizes of the library (any pointer may be NULL); device_bytes = what the three arrays hold on the device.
 * ngsid_classify_search: queries are host- or device-resident.  Count rows ([query][strand][n_refs] uint32) live in grow-only context scratch (returned by option
 *   "release_scratch"); the queries run in chunks sized from a share of the free device memory (option "classify_chunk_queries" fixes the chunk).  Results never depend on it.
 *
 * Profiling lines (ngsid_profile_read): k_classify_pairs, k_classify_flags, k_classify_scatter (build); k_classify_revcomp, k_classify_uniq, k_classify_count,
 * k_classify_topk (search); k_hpc_minimizers and hipcub_classify_sort for the sketches and the sorts.
 * Errors: NGSID_ERR_ARG (parameters out of range, no reference, more than NGSID_CLASSIFY_MAX_REFS references, a library of another context),
 * NGSID_ERR_ALPHABET (anything but upper-case ACGTN), NGSID_ERR_TOO_LONG (a sequence above NGSID_MAX_READ_LEN; a library of 2^31 or more minimizers),
 * NGSID_ERR_HIP. */
int32_t ngsid_refdb_build(ngsid_ctx* ctx, const ngsid_reads_t* refs, const ngsid_refdb_params_t* prm, ngsid_refdb** out);
int32_t ngsid_refdb_info(const ngsid_refdb* db, uint64_t* n_refs, uint64_t* n_postings, uint64_t* n_codes, uint64_t* device_bytes);
int32_t ngsid_refdb_release(ngsid_ctx* ctx, ngsid_refdb* db);
int32_t ngsid_classify_search(ngsid_ctx* ctx, const ngsid_refdb* db, const ngsid_reads_t* queries, const ngsid_classify_params_t* prm,
                              int32_t* cand_ref, int32_t* cand_shared, int8_t* cand_strand /* each [n_queries][top_k] */,
                              int32_t* n_codes /* [n_queries][2], may be NULL */);

#ifdef __cplusplus
}
#endif
#endif
