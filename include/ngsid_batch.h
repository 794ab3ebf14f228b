/* ngsid_batch.h - multi-sample (batch) entry points of libngsid_hip.so, on top of include/ngsid.h.
 *
 * Additive: ngsid_abi_version() stays 2.  These calls have no twin in the CPU oracle - their definition is "the call of ngsid.h, once per
 * sample" (the binding layer falls back to exactly that loop when the bound library lacks the symbol). */
#ifndef NGSID_BATCH_H
#define NGSID_BATCH_H
#include "ngsid.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Greedy clustering of several independent read sets ("segments": one demultiplexed sample each) in ONE pass.
 *
 * reads [seg_off[s], seg_off[s+1]) are segment s; seg_off has n_segments + 1 entries, seg_off[0] = 0, seg_off[n_segments] = reads->n, non-decreasing.
 * The outputs restricted to segment s are exactly what ngsid_cluster_greedy returns for that segment's reads alone (same order, the acc_rank slice,
 * prev_batch = known_err = NULL), with rep_of_read holding indices into the WHOLE set: a read never joins a representative of another segment, however
 * similar.  counters (may be NULL) = [n_segments][4], the four counters of ngsid_cluster_greedy per segment.  Empty segments, one-read segments and
 * segments whose reads are all shorter than k are legal.  There are no merge rounds (no prev_batch).
 *
 * Isolation is part of the index key: the segment number sits in the bits of the 64-bit minimizer code that the k-mer leaves free (64 - 3k for k <= 21;
 * 64 - bit length of the call's minimizer count for k >= 22, whose codes are dense ranks).  More segments than those bits can number -> NGSID_ERR_ARG
 * (k = 13: 2^25, k = 15: 2^19, k = 21: 2).  The tagged codes live in the context's minimizer store; the context's minimizer cache is left invalid, so
 * no later call (ngsid_polish's strand detection) mistakes them for plain codes.
 *
 * Context option "cluster_seg_order": 0 (default) = items interleaved (rank within segment, then segment), 1 = segments end to end.  Same results.
 * Errors: those of ngsid_cluster_greedy + NGSID_ERR_ARG for a malformed seg_off or too many segments. */
int32_t ngsid_cluster_greedy_segmented(ngsid_ctx* ctx, const ngsid_reads_t* reads, const ngsid_cluster_params_t* prm, const uint32_t* acc_rank,
                                       const uint64_t* seg_off, uint64_t n_segments,
                                       int32_t* rep_of_read, double* hpc_err_out, uint8_t* status_out, uint64_t* counters);

#ifdef __cplusplus
}
#endif
#endif
