/* ngsid_phase.h - the device half of splitting a cluster into haplotypes by linked variant sites, on top of include/ngsid_support.h.
 *
 * Additive: ngsid_abi_version() stays 2.  Three calls: the allele of every read at chosen centre positions (read x site genotypes), the 5 x 5 co-occurrence table of every
 * pair of sites, and the assignment of every read to the nearest of a set of haplotypes.  Which positions are sites, which sites are linked and which allele strings are
 * haplotypes is policy and lives in the binding layer (ngspeciesid_amd/phase.py); the library returns integers only.  The calls have no twin in the CPU oracle - their
 * definition is restated from the oracle's parts by the tests (tests/phase_reference.py).  The columns and strands those parts give are also pinned, without the
 * oracle, by tests/columns_reference.py (from tests/ed_reference.py and the strand rule of tests/polish_reference.py; tests/test_gpu_rec_reference.py).
 *
 * The genotype matrix crosses the boundary as a HOST array in both directions (at most 64 B per listed read). */
#ifndef NGSID_PHASE_H
#define NGSID_PHASE_H
#include "ngsid_support.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NGSID_PHASE_MAX_SITES 64     /* sites per group */
#define NGSID_PHASE_MAX_HAPS  16     /* haplotypes per group */

#define NGSID_GENO_DEL   4           /* 0-3: A C G T */
#define NGSID_GENO_OTHER 5           /* an 'X' column whose read base is outside ACGT */
#define NGSID_GENO_NONE  7           /* the site is outside the read's counted columns, or the read contributes nothing */
#define NGSID_HAP_ANY    255         /* hap_alleles: matches every code */

/* The allele of every listed read at the sites of its group.
 *
 * centres, reads, read_order, grp_off, n_groups, prm, strand: exactly as in ngsid_consensus_support - the same strand rule, the same alignment, the same counted columns
 * (prm->clip).  site_pos[site_off[g] .. site_off[g+1]) are strictly ascending positions of centre g: S_g of them, at most NGSID_PHASE_MAX_SITES, zero is legal.
 *
 * geno (uint8): the block of group g starts at sum over h < g of R_h * S_h (R_h = grp_off[h+1] - grp_off[h]) and is row-major [listed read][site].  Codes: 0-3 = the read's
 * base A / C / G / T at that centre base ('=' column: the centre's base; 'X' column with a read base in ACGT: that base), NGSID_GENO_DEL = 'D' column, NGSID_GENO_OTHER = 'X'
 * column with a read base outside ACGT, NGSID_GENO_NONE = not counted (the position lies outside the read's counted columns; strand -1; no counted column).  Read-only ('I')
 * columns are not genotyped.  Per site, the histogram of the codes of a group equals the counters of ngsid_consensus_support at that base (depth = codes <= 5).
 *
 * The alignments and the path matrix are those of ngsid_consensus_support (same routing, band retries and chunks under "support_budget_mb"); k_phase_gather reads the nibble of
 * every (read, site) from the matrix, masked with the span the aligner returns.  Profiling lines: k_ed_align_rec, k_phase_gather.
 * Errors: those of ngsid_consensus_support; NGSID_ERR_ARG also for more than NGSID_PHASE_MAX_SITES sites in a group, a site list that is not strictly ascending and a site
 * at or beyond the length of its centre. */
int32_t ngsid_phase_genotypes(ngsid_ctx* ctx, const ngsid_reads_t* centres, const ngsid_reads_t* reads, const uint32_t* read_order,
                              const uint64_t* grp_off, uint64_t n_groups, const ngsid_support_params_t* prm,
                              const uint64_t* site_off, const uint32_t* site_pos, uint8_t* geno, int8_t* strand);

/* Co-occurrence of alleles between every two sites of a group.
 *
 * geno, grp_off, site_off: as returned by / given to ngsid_phase_genotypes (host).  tables (uint32): the block of group g starts at sum over h < g of 25 * S_h * S_h and is
 * [S_g][S_g][5][5]: tables[s][t][a][b], s < t, = listed reads of g with code a at site s and code b at site t, both <= NGSID_GENO_DEL.  Entries with s >= t are zero.
 *
 * k_phase_pairs: a workgroup owns 64 site pairs and a slice of the reads of ONE group, counts in LDS (a private column of 25 counters per thread: no two lanes share an
 * address) and adds every non-zero counter to global memory once.  Integer adds only: bit-reproducible, independent of the slicing.
 * Errors: NGSID_ERR_ARG (null argument, more than NGSID_PHASE_MAX_SITES sites in a group), NGSID_ERR_HIP. */
int32_t ngsid_phase_pair_tables(ngsid_ctx* ctx, const uint8_t* geno, const uint64_t* grp_off, const uint64_t* site_off, uint64_t n_groups, uint32_t* tables);

/* Nearest haplotype of every listed read.
 *
 * Haplotypes hap_off[g] .. hap_off[g+1] belong to group g (H_g of them, at most NGSID_PHASE_MAX_HAPS, zero is legal).  hap_alleles (uint8): the block of group g starts at
 * sum over h < g of H_h * S_h and is row-major [haplotype][site]; values 0 - NGSID_GENO_DEL, or NGSID_HAP_ANY.
 *
 * Per listed read x: dist(h) = sites where the read's code is <= NGSID_GENO_DEL, the haplotype's value is not NGSID_HAP_ANY, and the two differ.  best[x] (int8) = the
 * haplotype of its group (0 .. H_g - 1) with the smallest distance, the lowest on ties; dist[x] (uint8) = that distance; dist2[x] (uint8) = the smallest distance over the
 * OTHER haplotypes, 255 when there is none.  A read without a site of code <= NGSID_GENO_DEL, and every read of a group without haplotypes: best -1, dist 255, dist2 255.
 *
 * k_phase_assign: one lane per read, the haplotypes of the group in LDS.
 * Errors: NGSID_ERR_ARG (null argument, more than NGSID_PHASE_MAX_SITES sites or NGSID_PHASE_MAX_HAPS haplotypes in a group, hap_off not ascending), NGSID_ERR_HIP. */
int32_t ngsid_phase_assign(ngsid_ctx* ctx, const uint8_t* geno, const uint64_t* grp_off, const uint64_t* site_off, uint64_t n_groups,
                           const uint64_t* hap_off, const uint8_t* hap_alleles, int8_t* best, uint8_t* dist, uint8_t* dist2);

#ifdef __cplusplus
}
#endif
#endif
