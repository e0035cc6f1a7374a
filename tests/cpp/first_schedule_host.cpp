// Runs the first fused launch's hand-out rule (csrc/wfpt_first_schedule.h) on the host, as bounce_kernel<kBounceFirst> applies it
// (tests/test_first_schedule_host.py; built with AddressSanitizer + UBSan there): over item counts around the multiples of the grid,
// three grids and every share of the sweep, the static items of all workgroups plus the dynamic range cover [0, n_items) exactly once,
// every workgroup's items ascend, and share 0 leaves nothing static. No GPU code is linked.
#include "wfpt_first_schedule.h"
#include <cstdint>
#include <cstdio>
#include <vector>

using namespace wfpt;

static_assert(first_n_static(259200u, 1024u, 0u, 1u) == 0u, "share 0: every item by ticket");
static_assert(first_n_static(259200u, 1024u, 1u, 1u) == 253u * 1024u, "share 1: every whole round");
static_assert(first_n_static(259200u, 1024u, 15u, 16u) == 237u * 1024u, "floor(15/16 * 259200 / 1024) = 237 rounds");
static_assert(first_static_item(5u, 3u, 1024u) == 3077u && first_dynamic_item(2048u, 7u) == 2055u, "");

// One launch as the kernel runs it: a workgroup holds `item`, knows the next one while first_next_is_static says so, and otherwise draws
// grid + counter++ (its own index was its first ticket). `order` picks which workgroup finishes its item next, so that tickets are drawn in
// an order unlike the workgroups' own.
static int launch(uint32_t n_items, uint32_t grid, uint32_t num, uint32_t den, uint32_t order) {
    const uint32_t n_static = first_n_static(n_items, grid, num, den);
    if (num == 0 && n_static != 0) return 1;
    if (n_static > n_items || n_static % grid != 0) return 2;
    if (static_cast<uint64_t>(n_static / grid) != static_cast<uint64_t>(n_items) * num / (static_cast<uint64_t>(den) * grid)) return 3;
    const uint32_t rounds = first_static_rounds(n_static, grid);
    std::vector<uint32_t> taken(n_items, 0), item(grid), last(grid, 0), count(grid, 0);
    std::vector<char> running(grid, 0);
    uint32_t counter = 0, left = 0; // Control::ticket
    for (uint32_t b = 0; b < grid; ++b) {
        item[b] = b; // = first_static_item(b, 0, grid), or ticket b of the dynamic range when there is no static round
        if (rounds == 0 && first_dynamic_item(n_static, b) != b) return 4;
        running[b] = item[b] < n_items;
        left += running[b];
    }
    uint32_t pick = order % grid;
    while (left) {
        while (!running[pick]) pick = (pick + 1) % grid;
        const uint32_t b = pick, it = item[b];
        if (it >= n_items) return 5;
        taken[it] += 1;
        if (count[b] && it <= last[b]) return 6; // a workgroup's items ascend
        if (count[b] < rounds && it != first_static_item(b, count[b], grid)) return 7;
        if (count[b] >= rounds && it < n_static) return 8;
        last[b] = it;
        count[b] += 1;
        if (first_next_is_static(it, n_static)) {
            if (count[b] > rounds) return 9; // only the static rounds go without a ticket ...
            item[b] = it + grid;             // ... the last of them leads to the workgroup's own ticket
            if (count[b] == rounds && item[b] != first_dynamic_item(n_static, b)) return 10;
        } else {
            if (count[b] <= rounds) return 11;
            item[b] = first_dynamic_item(n_static, grid + counter++);
        }
        if (item[b] >= n_items) { running[b] = 0; left -= 1; }
        pick = (pick + 1 + order * 7u) % grid;
    }
    for (uint32_t i = 0; i < n_items; ++i)
        if (taken[i] != 1) return 12;
    for (uint32_t b = 0; b < grid; ++b)
        if (count[b] < rounds) return 13;
    // every workgroup draws one ticket it cannot use, as before: the counter ends at dynamic items - first tickets used + workgroups that drew
    return 0;
}

int main() {
    const uint32_t shares[11][2] = {{0, 1}, {1, 2}, {3, 4}, {7, 8}, {15, 16}, {1, 1}, {1, 16}, {1, 8}, {1, 4}, {3, 8}, {5, 8}}; // (the sweep, and the points added between 0 and 3/4)
    uint32_t runs = 0;
    for (uint32_t grid : {1u, 7u, 1024u}) {
        const uint32_t counts[9] = {0u, 1u, grid - 1u, grid, grid + 1u, 2u * grid - 1u, 2u * grid, 2u * grid + 1u, 259200u};
        for (uint32_t n_items : counts)
            for (const auto &s : shares)
                for (uint32_t order : {0u, 1u, 5u}) {
                    if (int r = launch(n_items, grid, s[0], s[1], order)) {
                        std::printf("n_items %u grid %u share %u/%u order %u: check %d failed\n", n_items, grid, s[0], s[1], order, r);
                        return r;
                    }
                    runs += 1;
                }
    }
    // the largest launch a context can make (65535 segments, 64 samples in flight): the products stay exact
    if (first_n_static(65535u * 64u, 1024u, 15u, 16u) != 1024u * 3839u) return 20;
    if (first_n_static(0xffffffffu, 1u, 1u, 1u) != 0xffffffffu || first_n_static(5u, 0u, 1u, 1u) != 0u) return 21;
    std::printf("%u launches\nok\n", runs);
    return 0;
}
