/* ngsid_errprof.h - the error profile of the reads of every group against the group's centre, and how often a base of reported quality q was right, on top of
 * include/ngsid_support.h.
 *
 * Additive: ngsid_abi_version() stays 2.  The call has no twin in the CPU oracle - its definition is restated from the oracle's parts by the tests
 * (tests/errprof_reference.py: strands and alignment columns as tests/support_reference.py, counted columns as tests/cigar_reference.py, the tables in numpy).  The columns and strands those parts give are also pinned, without the
 * oracle, by tests/columns_reference.py (from tests/ed_reference.py and the strand rule of tests/polish_reference.py; tests/test_gpu_rec_reference.py).
 * The library returns integer sums only; rates, shares, the empirical Phred of a quality bin and every sentence about what the tables mean are policy and live in
 * the binding layer (ngspeciesid_amd/errprof.py).  NB the centre is made of the same reads: an error the majority of a group shares is invisible here, and a true
 * minority variant counts as an error. */
#ifndef NGSID_ERRPROF_H
#define NGSID_ERRPROF_H
#include "ngsid_support.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NGSID_ERRPROF_NCOUNT     96      /* entries of counts per (group, strand) */
#define NGSID_ERRPROF_PAIR        0      /* + c * 6 + o: centre letter c (A C G T = 0 .. 3) became o: 0 .. 3 the read letter A C G T, 4 a read letter outside ACGT, 5 deleted */
#define NGSID_ERRPROF_INS_LETTER 24      /* + l: letters of the 'I' columns, A C G T, other */
#define NGSID_ERRPROF_CEN_OTHER  29      /* 'X' and 'D' columns whose centre letter is outside ACGT */
#define NGSID_ERRPROF_READS      30      /* reads with at least one counted column (entry 31 is always 0) */
#define NGSID_ERRPROF_INS_LEN    32      /* + min(l, 16) - 1: maximal runs of 'I' columns of length l */
#define NGSID_ERRPROF_DEL_LEN    48      /* + min(l, 16) - 1: maximal runs of 'D' columns of length l */
#define NGSID_ERRPROF_HPCTX      64      /* + (min(r, 8) - 1) * 4 + k: columns by the length r of the centre run they sit in; k: 0 '=', 1 'X', 2 'D', 3 an 'I' run follows */
#define NGSID_ERRPROF_MAXLEN     16      /* the last bucket of INS_LEN and DEL_LEN: that length or more */
#define NGSID_ERRPROF_MAXRUN      8      /* the last row of HPCTX: a centre run of that length or more */
#define NGSID_ERRPROF_NQ         94      /* reported qualities 0 .. 93 */
#define NGSID_ERRPROF_NK          3      /* per quality: bases in '=' columns, in 'X' columns, in 'I' columns */

/* The error tables of every group, per strand.
 *
 * centres, reads, read_order, grp_off, n_groups, prm, strand: exactly those of ngsid_consensus_support - the same grouped reads, the same strand rule, the same
 * alignment (the rules of aln_mode 1), the same counted columns (prm->clip) and the same errors.
 *
 * Take one listed read with a strand and the forward column list of the ORIENTED read against its centre ('=', 'X', 'I' read only, 'D' centre only).  Its counted
 * columns are x0 .. x1 (the first and the last '=' / 'X' column; with prm->clip the first column of the first and the last column of the last run of 15 '=').
 * Everything below is counted over these columns only; a run of 'I' behind the last counted column lies outside them and is never counted.
 *
 * counts[(g * 2 + s) * NGSID_ERRPROF_NCOUNT + i] (uint64), group g, strand s:
 *   PAIR[c * 6 + o]      '=', 'X' and 'D' columns whose centre letter is c (any case); o = the read letter (4: outside ACGT) or 5 = deleted.  PAIR[c][c] are the '=' columns.
 *   INS_LETTER[l]        letters of the 'I' columns
 *   CEN_OTHER            'X' and 'D' columns whose centre letter is outside ACGT
 *   READS                reads with at least one counted column
 *   INS_LEN, DEL_LEN     maximal runs of 'I' / of 'D' columns by length l, index min(l, 16) - 1
 *   HPCTX[(min(r, 8) - 1) * 4 + k]   per '=' / 'X' / 'D' column of a centre base of ACGT, r = the length of the maximal run of equal BYTES of the centre that holds
 *                        the base; k = 0 '=', 1 'X', 2 'D'; k = 3 is counted IN ADDITION when a run of 'I' columns directly follows the column.  A base of a centre
 *                        run outside ACGT adds nothing.
 * qtab[((g * 2 + s) * NGSID_ERRPROF_NQ + q) * NGSID_ERRPROF_NK + k] (uint64; may be NULL: the table and its cost are skipped): read bases of reported quality
 * q = clamp(byte - 33, 0, 93) in an '=' (k = 0), an 'X' (k = 1) or an 'I' (k = 2) column.  The quality byte is the ORIENTED read's: on strand 1 oriented position i
 * holds byte L - 1 - i of the read as it was handed in.  A read set without qualities is legal and gives an all-zero qtab.
 *
 * A caller may rely on (same lists, same prm; DEPTH, AGREE, DEL, INS, n_used of ngsid_consensus_support, nm of ngsid_read_cigars; sums over strands and positions):
 *   - sum PAIR + CEN_OTHER = sum DEPTH;   sum PAIR[c][c] = sum AGREE;   sum PAIR[c][5] + the 'D' part of CEN_OTHER = sum DEL;
 *   - sum INS_LEN = sum INS;   sum HPCTX over k = 0, 1, 2 = sum PAIR;
 *   - 'X' columns + sum INS_LETTER + 'D' columns = sum nm;   READS = n_used;
 *   - with qualities: sum qtab[.., 0] = sum PAIR[c][c], sum qtab[.., 2] = sum INS_LETTER.
 *
 * Both outputs are cleared by the call.  Empty groups, one-read groups, reads without a strand, a centre of length 0 and no reads at all are legal (zeros).  The store
 * pass is the one of ngsid_hp_runs (path nibbles and read positions, chunks under the same budget); the tables are integer sums, so the result is bit-reproducible
 * and does not depend on chunks, slices or launch shapes.  Profiling lines (ngsid_profile_read): k_ed_align_rec, k_errprof.
 * Errors: those of ngsid_consensus_support, and NGSID_ERR_ARG for null counts. */
int32_t ngsid_error_profile(ngsid_ctx* ctx, const ngsid_reads_t* centres, const ngsid_reads_t* reads, const uint32_t* read_order,
                            const uint64_t* grp_off, uint64_t n_groups, const ngsid_support_params_t* prm,
                            uint64_t* counts, uint64_t* qtab, int8_t* strand);

#ifdef __cplusplus
}
#endif
#endif
