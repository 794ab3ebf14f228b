// polish_units.h - the unit lists of one polishing iteration (polish_host.hip window_units; tests/polish_units_main.cpp runs it alone): plain C++, no HIP, no context.
#pragma once
#include <cstdint>
#include <vector>
#include <utility>
#include <thread>
#include <atomic>
#include <algorithm>

// racon adds the layers of a window in the order of their first window position (src/window.cpp: rank sorted by positions_.first); ties keep the read order
// (stable): counting sort of the layer ids v on valid[id] (= 1 + that position).  tmpv, cnt: the caller's scratch.
static inline void polish_order_unit(const uint16_t* valid, std::vector<uint32_t>& v, std::vector<uint32_t>& tmpv, std::vector<uint32_t>& cnt)
{
    if (v.size() < 2) return;
    uint32_t kmax = 0; bool sorted = true;
    for (size_t x = 0; x < v.size(); ++x) { const uint32_t kx = valid[v[x]]; kmax = std::max(kmax, kx); if (x && valid[v[x - 1]] > kx) sorted = false; }
    if (sorted) return;
    cnt.assign((size_t)kmax + 2, 0);
    for (uint32_t id : v) cnt[valid[id] + 1]++;
    for (size_t k = 1; k < cnt.size(); ++k) cnt[k] += cnt[k - 1];
    tmpv.resize(v.size());
    for (uint32_t id : v) tmpv[cnt[valid[id]]++] = id;
    std::copy(tmpv.begin(), tmpv.end(), v.begin());
}

// valid[p * nwinmax + w] != 0: pair p has a layer in window w of its group (k_layers); pairs [gbeg[g], gbeg[g + 1]) are group g's, in read order.
// -> lists[u] = the layer ids p * nwinmax + w of unit u = (group, window) unit_gw[u], ordered as racon adds them; used[g] = the pairs of group g with a layer in one of
// its nwin[g] windows (0 windows: a group without units).  One task per unit and one per group, handed out by one counter to `threads` threads (1: inline, none spawned).
static inline void polish_build_units(const uint16_t* valid, int nwinmax, const std::vector<uint64_t>& gbeg, const std::vector<std::pair<uint32_t, int>>& unit_gw,
                                      const std::vector<uint32_t>& nwin, unsigned threads, std::vector<std::vector<uint32_t>>& lists, std::vector<uint64_t>& used)
{
    const size_t nu = unit_gw.size(), ntask = nu + nwin.size(); const uint64_t nwm = (uint64_t)nwinmax;
    lists.assign(nu, {}); used.assign(nwin.size(), 0); std::atomic<size_t> next_task{0};
    auto worker = [&]() {
        std::vector<uint32_t> tmpv, cnt;
        for (;;) {
            const size_t t = next_task.fetch_add(1); if (t >= ntask) break;
            if (t < nu) {        // lists sized for the worst case, filled through a raw cursor, trimmed afterwards
                const uint32_t g = unit_gw[t].first, wdx = (uint32_t)unit_gw[t].second;
                std::vector<uint32_t>& v = lists[t]; v.resize(gbeg[g + 1] - gbeg[g]); uint32_t* c = v.data();
                for (uint64_t p = gbeg[g]; p < gbeg[g + 1]; ++p) { *c = (uint32_t)(p * nwm + wdx); c += valid[p * nwm + wdx] != 0; }
                v.resize((size_t)(c - v.data())); polish_order_unit(valid, v, tmpv, cnt);
            } else {
                const size_t g = t - nu; uint64_t u = 0;
                for (uint64_t p = gbeg[g]; p < gbeg[g + 1]; ++p) { const uint16_t* hv = valid + p * nwm; uint32_t any = 0; for (uint32_t wdx = 0; wdx < nwin[g]; ++wdx) any |= hv[wdx] != 0; u += any; }
                used[g] = u;
            }
        }
    };
    std::vector<std::thread> th; for (unsigned x = 1; x < threads; ++x) th.emplace_back(worker);
    worker(); for (std::thread& t : th) t.join();
}
