/* ngsid_support.h - per-base read support of a consensus sequence, on top of include/ngsid.h.
 *
 * Additive: ngsid_abi_version() stays 2.  The call has no twin in the CPU oracle - its definition is restated from the oracle's parts by the tests
 * (tests/support_reference.py: strands of ongsid_polish_trace_aln, alignment columns of ongsid_i_ed_ops, counting in numpy).  The columns and strands those parts give are also pinned, without the
 * oracle, by tests/columns_reference.py (from tests/ed_reference.py and the strand rule of tests/polish_reference.py; tests/test_gpu_rec_reference.py).  The library returns integers
 * only; the quality formula lives in the binding layer (consensus.support_phred). */
#ifndef NGSID_SUPPORT_H
#define NGSID_SUPPORT_H
#include "ngsid.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int32_t k, w;      /* minimizer scheme of the strand detection: the polisher's rule (HPC minimizers of at most 21 bases, window max(w, k)) */
    int32_t clip;      /* 0 = the counted columns of a read run from its first to its last '=' / 'X' column; 1 = from its first to its last run of at least
                          15 '=' columns (the rule of ngsid_polish_params_t.aln_mode 3: reads whose ends are known to overhang the centre) */
} ngsid_support_params_t;

#define NGSID_SUPPORT_DEPTH 0      /* counted columns '=', 'X' or 'D' at the base */
#define NGSID_SUPPORT_AGREE 1      /* '=' */
#define NGSID_SUPPORT_SUB_A 2      /* 'X' whose read base is A; 3 = C, 4 = G, 5 = T.  An 'X' with a read base outside ACGT raises the depth only */
#define NGSID_SUPPORT_DEL   6      /* 'D': the read has no base here */
#define NGSID_SUPPORT_INS   7      /* reads with a run of 'I' columns directly behind the column of this base (once per run) */
#define NGSID_SUPPORT_NCOUNT 8

/* How many reads agree, disagree (and with what), delete or insert at every base of every centre.
 *
 * centres: one sequence per group (qual ignored).  Reads are grouped like in ngsid_polish: the listed reads [grp_off[g], grp_off[g+1]) (read_order[x], or x itself when
 * read_order is NULL) belong to group g, and a read may be listed under ONE group only (NGSID_ERR_ARG otherwise).
 *
 * Per listed read against the centre C of its group: the strand is the polisher's (shared minimizer codes of the read with C against rc(C); none shared: the read
 * contributes nothing) and equals it_aln[..][0] of ngsid_polish_trace_aln with iters = 1; the read, reverse-complemented on strand 1, is aligned with the rules of
 * aln_mode 1 (unit costs, the read end to end, centre ends free, end column = leftmost minimum of the last row, traceback prefers diagonal, then read-only, then
 * centre-only; letters match only if both are ACGT in any case and equal).  The counted columns are those of prm->clip; a read without one contributes nothing.
 * There is no racon -e / -q filtering: every oriented read counts.
 *
 * counts[(cen_off + b) * 8 + c] (uint32, cen_off = centres->off[g]; centres->off[n_groups] * 8 entries): counter c (NGSID_SUPPORT_*) of base b of group g;
 * depth >= agree + sub_* + del.  n_used[g] (may be NULL) = reads of the group that counted at least one column.  strand[x] (may be NULL) = strand of listed read x:
 * 0, 1 or -1.  Empty groups, one-read groups and groups where no read shares a minimizer with the centre are legal (all zeros).
 *
 * The alignments are those of the polisher's bit-parallel aligner with the path recorded (4 bits per cell of a [read][centre position] matrix, in chunks under a
 * share of the free device memory); the counters are summed from that matrix with integer adds, so the result is bit-reproducible.  Profiling lines
 * (ngsid_profile_read): k_ed_align_rec (alignment + path), k_support_sum.
 * Errors: NGSID_ERR_ARG, NGSID_ERR_ALPHABET (base outside ACGTN), NGSID_ERR_TOO_LONG (a read or centre above NGSID_MAX_CONSENSUS_LEN), NGSID_ERR_HIP. */
int32_t ngsid_consensus_support(ngsid_ctx* ctx, const ngsid_reads_t* centres, const ngsid_reads_t* reads, const uint32_t* read_order,
                                const uint64_t* grp_off, uint64_t n_groups, const ngsid_support_params_t* prm,
                                uint32_t* counts, uint64_t* n_used, int8_t* strand);

#ifdef __cplusplus
}
#endif
#endif
