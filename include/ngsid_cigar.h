/* ngsid_cigar.h - the alignment of every read to the centre of its group as a run-length-encoded list of BAM operations, on top of include/ngsid_support.h.
 *
 * Additive: ngsid_abi_version() stays 2.  The call has no twin in the CPU oracle - its definition is restated from the oracle's parts by the tests
 * (tests/cigar_reference.py: strands and alignment columns as tests/support_reference.py, run lengths in numpy).  The columns and strands those parts give are also pinned, without the
 * oracle, by tests/columns_reference.py (from tests/ed_reference.py and the strand rule of tests/polish_reference.py; tests/test_gpu_rec_reference.py).  The library returns integers only; the text
 * of a CIGAR is made by the record writer (ngsid_host_write_sam, include/ngsid.h) and which reads are listed under which centre is policy (ngspeciesid_amd/sam.py). */
#ifndef NGSID_CIGAR_H
#define NGSID_CIGAR_H
#include "ngsid_support.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NGSID_CIGAR_NFIELD  5        /* per listed read: t_begin, t_end, q_begin, q_end, nm */
#define NGSID_CIGAR_MERGE_M 1u       /* flags: '=' and 'X' both become 'M' (op 0) and neighbouring runs merge */
/* an entry of ops: length << 4 | op, the op codes of BAM */
#define NGSID_CIGAR_OP_M  0u
#define NGSID_CIGAR_OP_I  1u
#define NGSID_CIGAR_OP_D  2u
#define NGSID_CIGAR_OP_S  4u
#define NGSID_CIGAR_OP_EQ 7u
#define NGSID_CIGAR_OP_X  8u

/* The alignment of every listed read against the centre of its group.
 *
 * centres, reads, read_order, grp_off, n_groups, prm, strand: exactly those of ngsid_consensus_support - the same grouped reads, the same strand rule, the same
 * alignment (the rules of aln_mode 1) and the same counted columns (prm->clip).  flags: 0 or NGSID_CIGAR_MERGE_M.
 *
 * Take the forward column list of the oriented read of L letters against its centre ('=', 'X', 'I' read only, 'D' centre only).  t_begin, t_end, q_begin, q_end are
 * the centre and read positions of the first and the last counted column (inclusive, in the ORIENTED read's coordinates), nm the number of 'X', 'I' and 'D'
 * columns among the counted ones.  The read's ops are: S q_begin when non-zero; the run-length encoding of the counted columns ('=' 7, 'X' 8, 'I' 1, 'D' 2; with
 * NGSID_CIGAR_MERGE_M '=' and 'X' are both 0); S (L - 1 - q_end) when non-zero.  A listed read without a strand or without a counted column has no ops and -1 in
 * all five fields.
 *
 * aln [n_listed][NGSID_CIGAR_NFIELD] int32.  ops: the ops of the listed reads one behind the other in listed order, op_off [n_listed + 1]:
 * ops[op_off[x] .. op_off[x + 1]) are those of listed read x.  A caller may rely on:
 *   - the lengths of the ops that consume the read (M, =, X, I, S) sum to L;
 *   - the lengths of the ops that consume the centre (M, =, X, D) sum to t_end - t_begin + 1;
 *   - the first and the last op that is not S are match ops (M, =, X);
 *   - neighbouring ops differ;
 *   - an I run never touches a D run (next to each other they cost two edits where one X costs one: no minimum-cost path holds the pair).  This holds for the
 *     counted columns, which are all a caller sees.  Outside them the free centre ends are centre-only columns that cost nothing: read letters in front of the
 *     first match column follow the free prefix directly (they are soft-clipped here), and those behind the last one are followed by the free suffix.
 *
 * Capacity: *needed is always the total number of ops.  cap = 0 with null aln, op_off and ops is the count call (NGSID_ERR_CAPACITY whenever there is an op,
 * NGSID_OK otherwise).  A fill call with fewer than *needed entries of room returns NGSID_ERR_CAPACITY; the call streams chunk by chunk, so on that error the
 * contents of aln, op_off and ops are UNSPECIFIED (strand is complete).  The count call repeats the whole store pass: a caller that knows a bound passes it as cap.
 * 2 * nm + 3 bounds the ops of one read.
 *
 * Empty groups, one-read groups, groups where no read shares a minimizer with the centre, a centre of length 0 and no reads at all are legal.
 * The store pass is the one of ngsid_hp_runs (path nibbles and read positions, chunks under the same budget); a wave walks one row and finds run starts, indices
 * and lengths with ballots, so the result is bit-reproducible and does not depend on the chunks.  Profiling lines (ngsid_profile_read): k_ed_align_rec,
 * k_cigar_count, k_cigar_emit.
 * Errors: those of ngsid_consensus_support, NGSID_ERR_ARG for unknown flags or missing outputs, and NGSID_ERR_CAPACITY. */
int32_t ngsid_read_cigars(ngsid_ctx* ctx, const ngsid_reads_t* centres, const ngsid_reads_t* reads, const uint32_t* read_order,
                          const uint64_t* grp_off, uint64_t n_groups, const ngsid_support_params_t* prm, uint32_t flags,
                          int8_t* strand, int32_t* aln, uint64_t* op_off, uint32_t* ops, uint64_t cap, uint64_t* needed);

#ifdef __cplusplus
}
#endif
#endif
