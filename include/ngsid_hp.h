/* ngsid_hp.h - per homopolymer run of a consensus sequence, how long that run is in every read, on top of include/ngsid_support.h.
 *
 * Additive: ngsid_abi_version() stays 2.  The call has no twin in the CPU oracle - its definition is restated from the oracle's parts by the tests
 * (tests/hp_reference.py: strands and alignment columns as tests/support_reference.py, read positions by cumulative sums, counting in numpy).  The columns and strands those parts give are also pinned, without the
 * oracle, by tests/columns_reference.py (from tests/ed_reference.py and the strand rule of tests/polish_reference.py; tests/test_gpu_rec_reference.py).  The library
 * returns integers only; which length is called from a histogram is policy and lives in the binding layer (ngspeciesid_amd/hp.py). */
#ifndef NGSID_HP_H
#define NGSID_HP_H
#include "ngsid_support.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NGSID_HP_NBUCKET 17        /* buckets 0 - 14: the read's run has exactly that many bases; 15: 15 or more */
#define NGSID_HP_OTHER   16        /* the read spans the run but gives no length: a flank that is not '=', or a foreign letter between the flanks */

/* The length histogram of every listed homopolymer run of every centre, per strand.
 *
 * centres, reads, read_order, grp_off, n_groups, prm, strand: exactly those of ngsid_consensus_support - the same grouped reads, the same strand rule, the same
 * alignment (the rules of aln_mode 1) and the same counted columns (prm->clip).
 *
 * run_start[run_off[g] .. run_off[g + 1]) are the listed runs of group g: strictly ascending positions of its centre C, each the FIRST base of a maximal run of
 * equal bytes (pos == 0 || C[pos - 1] != C[pos]).  A position inside a run, at or beyond the centre length, or a list that does not ascend: NGSID_ERR_ARG.
 * There is no cap on the number of runs; an empty list is legal.
 *
 * Listed run [a, b) of a centre of m bases (letter c = C[a]; b = the first position behind a whose byte differs, or m), one oriented read with a strand >= 0 and
 * at least one counted column, counted target span [t_begin, t_end]:
 *   - the read SPANS the run when a >= 1, b <= m - 1 and t_begin <= a - 1, b <= t_end; a read that does not span the run adds nothing (so the first and the last
 *     run of a centre never collect anything);
 *   - when the columns of the centre positions a - 1 and b are both '=' columns, at read positions qa and qb: l = qb - qa - 1; when every read base in (qa, qb)
 *     equals c (c one of ACGT, any case) the read adds 1 to bucket min(l, 15) - l = 0: the read has no base of the run -, otherwise 1 to NGSID_HP_OTHER;
 *   - a spanning read with a flank that is not '=' adds 1 to NGSID_HP_OTHER;
 *   - a run whose letter is outside ACGT collects nothing.
 * The two '=' flanks carry letters other than c, so the bases between them are the read's whole run wherever the aligner put its gaps.
 *
 * hist[((run_off[g] + r) * 2 + s) * NGSID_HP_NBUCKET + bucket] (uint32; run_off[n_groups] * 2 * 17 entries): reads of strand s in that bucket of listed run r of
 * group g.  strand[x] (may be NULL) as in ngsid_consensus_support.  Empty groups, groups without runs and reads without a strand are legal (all zeros).
 *
 * The store pass is the support call's with a second output, the read position of every '=' / 'X' column (2 bytes per cell beside the 4 bits of the path, both
 * under the same chunk budget); the histograms are integer sums, so the result is bit-reproducible and does not depend on the chunks.  Profiling lines
 * (ngsid_profile_read): k_ed_align_rec (alignment + path + positions), k_hp_runs.
 * Errors: those of ngsid_consensus_support, and NGSID_ERR_ARG for the lists as above. */
int32_t ngsid_hp_runs(ngsid_ctx* ctx, const ngsid_reads_t* centres, const ngsid_reads_t* reads, const uint32_t* read_order,
                      const uint64_t* grp_off, uint64_t n_groups, const ngsid_support_params_t* prm,
                      const uint64_t* run_off, const uint32_t* run_start, uint32_t* hist, int8_t* strand);

#ifdef __cplusplus
}
#endif
#endif
