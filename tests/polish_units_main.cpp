// polish_units_main.cpp - polish_build_units (csrc/polish_units.h) alone, against a per-pair loop over random validity maps, with 1, 2, 3 and 16 threads.
// Stand-alone: tests/test_polish_units_cpu.py compiles and runs it; it also is the program to build with a host sanitizer.  Exit status 0 = no difference.
#include "polish_units.h"
#include <cstdio>
#include <random>

// one pass over the pairs, every layer appended to the list of its (group, window) and the lists then ordered by window position, ties in read order
static void naive_units(const std::vector<uint16_t>& valid, int nwinmax, const std::vector<uint32_t>& pair_group, const std::vector<std::pair<uint32_t, int>>& unit_gw,
                        const std::vector<uint32_t>& nwin, std::vector<std::vector<uint32_t>>& lists, std::vector<uint64_t>& used)
{
    const size_t G = nwin.size(); std::vector<size_t> ubase(G, 0);
    lists.assign(unit_gw.size(), {}); used.assign(G, 0);
    for (size_t u = unit_gw.size(); u-- > 0;) ubase[unit_gw[u].first] = u;      // (the units of a group are consecutive: its first)
    for (size_t p = 0; p < pair_group.size(); ++p) {
        const uint32_t g = pair_group[p]; bool any = false;
        for (uint32_t w = 0; w < nwin[g]; ++w) if (valid[p * nwinmax + w]) { lists[ubase[g] + w].push_back((uint32_t)(p * nwinmax + w)); any = true; }
        used[g] += any;
    }
    for (std::vector<uint32_t>& v : lists) std::stable_sort(v.begin(), v.end(), [&](uint32_t a, uint32_t b) { return valid[a] < valid[b]; });
}

int main()
{
    std::mt19937_64 rng(20240607); int bad = 0; size_t layers = 0, unsorted = 0;
    auto below = [&](uint64_t n) { return (uint64_t)(rng() % n); };
    for (int trial = 0; trial < 300 && !bad; ++trial) {
        const uint32_t G = 1 + (uint32_t)below(40); const int nwinmax = 6 + (int)below(3);
        const uint64_t key_range = trial % 3 == 0 ? 3 : trial % 3 == 1 ? 40 : 65534;      // window positions: many ties, some, hardly any
        const unsigned p_layer = 1 + (unsigned)below(100);                                // per cent of (pair, window) slots with a layer
        std::vector<uint32_t> nwin(G), pair_group; std::vector<uint64_t> gbeg(G + 1, 0); std::vector<std::pair<uint32_t, int>> unit_gw;
        for (uint32_t g = 0; g < G; ++g) {
            const bool stable = below(5) == 0, empty = below(6) == 0;
            nwin[g] = stable ? 0 : 1 + (uint32_t)below(5);
            for (uint32_t w = 0; w < nwin[g]; ++w) unit_gw.push_back({g, (int)w});
            const uint64_t np = empty ? 0 : below(301);
            pair_group.insert(pair_group.end(), np, g); gbeg[g + 1] = pair_group.size();
        }
        std::vector<uint16_t> valid(pair_group.size() * nwinmax + 1);
        for (size_t p = 0; p < pair_group.size(); ++p) for (int w = 0; w < nwinmax; ++w)
            valid[p * nwinmax + w] = (uint32_t)w >= nwin[pair_group[p]] ? (uint16_t)below(65535)          // past the group's windows: anything (k_layers leaves 0, nothing may read it)
                                     : below(100) < p_layer ? (uint16_t)(1 + below(key_range)) : 0;
        std::vector<std::vector<uint32_t>> want, got; std::vector<uint64_t> want_used, got_used;
        naive_units(valid, nwinmax, pair_group, unit_gw, nwin, want, want_used);
        for (const std::vector<uint32_t>& v : want) { layers += v.size(); for (size_t x = 1; x < v.size(); ++x) if (v[x] < v[x - 1]) { ++unsorted; break; } }
        for (unsigned threads : {1u, 2u, 3u, 16u}) {
            polish_build_units(valid.data(), nwinmax, gbeg, unit_gw, nwin, threads, got, got_used);
            if (got != want || got_used != want_used) { fprintf(stderr, "trial %d, %u threads: %s differ (%u groups, %zu units, %zu pairs)\n", trial, threads, got != want ? "lists" : "counts", G, unit_gw.size(), pair_group.size()); ++bad; }
        }
    }
    if (!layers || !unsorted) { fprintf(stderr, "the cases hold no layer, or no list that the order changes\n"); ++bad; }
    printf("polish_units: %s (%zu layers, %zu lists reordered)\n", bad ? "FAILED" : "ok", layers, unsorted);
    return bad ? 1 : 0;
}
