// k_support.h - the store pass of ngsid_consensus_support (k_support.hip), shared with ngsid_phase_genotypes (k_phase.hip)
#pragma once
#include "ngsid_host.h"
#include "../../include/ngsid_support.h"
#include <functional>

struct RecPlan {
    const uint8_t* d_oseq = nullptr; const uint64_t* d_read_off = nullptr; const uint32_t* d_pair_read = nullptr;      // device: the oriented reads, their offsets, the read of every pair
    uint32_t G = 0, maxb = 0, stride = 0;            // groups, longest centre, dwords per row of the path matrix
    uint64_t total = 0, NP = 0;                      // bases of all centres, pairs (= listed reads with a strand)
    std::vector<uint64_t> boff;                      // host offsets of the centres
    std::vector<uint64_t> gbeg;                      // pairs [gbeg[g], gbeg[g + 1]) are group g's, in list order
    const uint32_t* pair_x = nullptr; const uint32_t* pair_group = nullptr;      // host: position of every pair's read in the caller's list, its group
    const uint32_t* d_pair_group = nullptr;          // device: group of every pair
    const uint8_t* d_cen_seq = nullptr; const uint64_t* d_cen_off = nullptr;      // device: the centres
    const uint8_t* bseq = nullptr;                   // host: the bytes of the centres (boff)
    const uint8_t* h_orient = nullptr; const uint32_t* pair_read = nullptr;      // host: strand of every READ (0, 1, 255 = none), read of every pair
    const uint8_t* d_oqual = nullptr;                // device: the oriented qualities (as d_oseq), null when the read set came without qualities
};
struct RecChunk { const uint32_t* rec; const int32_t* span; uint64_t c0, c1; const uint16_t* pos; };   // path matrix and spans {q_begin, q_end, t_begin, t_end} of the pairs [c0, c1), row 0 = pair c0;
                                                                                  // pos (want_pos only, else null): read index of every '=' / 'X' column, [pair][stride * 8] uint16
int32_t ngsid_rec_walk(ngsid_ctx* ctx, const ngsid_reads_t* centres, const ngsid_reads_t* reads, const uint32_t* read_order, const uint64_t* grp_off, uint64_t n_groups,
                       const ngsid_support_params_t* prm, int8_t* strand, const std::function<int32_t(const RecPlan&)>& init,
                       const std::function<int32_t(const RecPlan&)>& start, const std::function<int32_t(const RecPlan&, const RecChunk&)>& chunk, bool want_pos = false);
