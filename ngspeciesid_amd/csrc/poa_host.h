// poa_host.h - what the polisher (polish_host.hip) takes from the hierarchy driver (poa_host.hip): units, hierarchy parameters, run_hierarchy, the output packing
#pragma once
#include "ngsid_host.h"
#include "k_poa.h"

struct Unit {                       // one consensus problem: a cluster (spoa stage) or a backbone window (polish)
    std::vector<uint32_t> seqs;     // indices into the CURRENT level's PSeq array, in order
    int bb = -1;                    // backbone index (into the bbs array) or -1
    bool done = false;
    uint32_t single_maxlen = 0;     // round 6 (single_below): set (> 0) by the caller for a unit that runs as ONE graph = the longest sequence that can enter it (reads of its members / layers, its backbone)
    std::string result; std::vector<uint32_t> cov; bool has_result = false;
};

struct HierParams { int m, n, g, band, node_cap, D, upper_mode; bool want_cov; int trim_tiles; int single_below = 0; bool sub = false; };      // single_below: ngsid_poa_params_t.single_below (units the caller marked with single_maxlen); sub: level 0 may hold POA_MODE_SUBGRAPH layers (the sub-graph tile instances run it)

// Runs all units to completion.  level0: device PSeq array whose max length is maxlen0; bbs: device backbone PSeqs (may be null) of the lengths bb_len.
int32_t run_hierarchy(ngsid_ctx* ctx, const PSeq* d_level0, uint32_t maxlen0, const PSeq* d_bbs, const std::vector<int>& bb_len, std::vector<Unit>& units, const HierParams& hp);

// The strings str(0) .. str(n - 1) behind offsets: off[0 .. n], their bytes in out where they fit (offsets_only: none are copied and none are missed), *needed = their sum.
// Some did not fit (or out is null): NGSID_ERR_CAPACITY "<what> buffer too small: need <sum> bytes".
template <typename Str>
static inline int32_t ngsid_pack_strings(ngsid_ctx* ctx, const char* what, size_t n, Str str, uint64_t* off, uint8_t* out, uint64_t cap, uint64_t* needed, bool offsets_only = false)
{
    uint64_t total = 0; bool ovf = false; off[0] = 0;
    for (size_t x = 0; x < n; ++x) {
        const std::string& s = str(x);
        if (offsets_only) {} else if (out && total + s.size() <= cap) memcpy(out + total, s.data(), s.size()); else if (s.size()) ovf = true;
        total += s.size(); off[x + 1] = total;
    }
    if (needed) *needed = total;
    if (ovf) NGSID_FAIL(ctx, NGSID_ERR_CAPACITY, "%s buffer too small: need %llu bytes", what, (unsigned long long)total);
    return NGSID_OK;
}
