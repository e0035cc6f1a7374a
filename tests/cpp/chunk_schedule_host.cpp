// Runs the fused launches' chunked hand-out (csrc/wfpt_ticket_chunks.h) on the host, as bounce_kernel applies it behind the first
// launch's static range (csrc/wfpt_first_schedule.h) or, with no static range, over a middle launch's tickets
// (tests/test_chunk_schedule_host.py; built with AddressSanitizer + UBSan there). Over three grids, dynamic ranges around every edge of
// the layout, chunk lengths 1 .. 16, 0 / 1 / 4 tail rounds, static shares 0 and 1/2 and three orders in which the workgroups finish:
// every item is taken exactly once, a workgroup's items ascend, "follows" is true exactly inside a chunk (checked against a count of
// what is left of the chunk, which the kernel does not keep), the draws that find something number n_body + singles, chunk length 1 is
// first_dynamic_item draw for draw, and the 32-bit products are exact at the largest launch. No GPU code is linked.
#include "wfpt_first_schedule.h"
#include "wfpt_ticket_chunks.h"
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

using namespace wfpt;

static_assert(chunk_tail(259200u, 1024u, 4u) == 4096u && chunk_body(259200u, 1024u, 8u, 4u) == 255104u, "the frame bench.py times: 31 888 chunks of 8");
static_assert(chunk_draws(259200u, 255104u, 8u) == 31888u + 4096u, "and 4096 singles");
static_assert(chunk_draw_position(31887u, 259200u, 255104u, 8u) == 255096u && chunk_draw_position(31888u, 259200u, 255104u, 8u) == 255104u, "");
static_assert(chunk_draw_position(35983u, 259200u, 255104u, 8u) == 259199u && chunk_draw_position(35984u, 259200u, 255104u, 8u) == 259200u, "");
static_assert(chunk_follows(255102u, 255104u, 8u) && !chunk_follows(255103u, 255104u, 8u) && !chunk_follows(255104u, 255104u, 8u), "");
static_assert(chunk_body(5u, 1024u, 8u, 4u) == 0u && chunk_body(100u, 7u, 16u, 0u) == 96u && chunk_body(0u, 7u, 16u, 0u) == 0u, "");

struct Group {
    uint32_t item = 0, last = 0, count = 0, left = 0; // left: positions of the current chunk still to come (the kernel keeps no such count)
    bool running = false;
};

// One launch as the kernel runs it. A workgroup holds `item`; while the item lies in the static range the next one is item + grid (the
// last static round leads to the workgroup's own draw, its index); inside a chunk it is item + 1; otherwise the workgroup has drawn
// grid + counter++ at the start of the item. `order` picks which workgroup finishes its item next.
static int launch(uint32_t n_items, uint32_t grid, uint32_t num, uint32_t den, uint32_t chunk, uint32_t tail_rounds, uint32_t order) {
    const uint32_t n_static = first_n_static(n_items, grid, num, den);
    const uint32_t d = n_items - n_static, body = chunk_body(d, grid, chunk, tail_rounds), n_body = body / chunk;
    if (body > d || body % chunk != 0u) return 1;
    if (d - body < chunk_tail(d, grid, tail_rounds) || d - body >= chunk_tail(d, grid, tail_rounds) + chunk) return 2; // the tail and less than one chunk
    if (chunk == 1u && body != d - chunk_tail(d, grid, tail_rounds)) return 3;
    std::vector<uint8_t> taken(n_items, 0);
    std::vector<Group> g(grid);
    uint32_t counter = 0, left = 0, found = 0; // Control::ticket; workgroups running; draws that found something
    // what draw u gives: an item, or n_items for "nothing left"
    auto draw = [&](uint32_t b, uint32_t u) -> uint32_t {
        const uint32_t p = chunk_draw_position(u, d, body, chunk);
        if (p > d) return 0xffffffffu;
        if (chunk == 1u) { // today's rule: position = draw
            const uint32_t was = first_dynamic_item(n_static, u);
            if (p < d ? n_static + p != was : was < n_items) return 0xffffffffu;
        }
        if (p < d) {
            found += 1;
            if (u < n_body ? p != chunk * u : p != body + (u - n_body)) return 0xffffffffu;
            g[b].left = u < n_body ? chunk - 1u : 0u;
        }
        return n_static + p;
    };
    for (uint32_t b = 0; b < grid; ++b) {
        g[b].item = b;
        if (n_static == 0u && (g[b].item = draw(b, b)) == 0xffffffffu) return 4;
        g[b].running = g[b].item < n_items;
        left += g[b].running;
    }
    uint32_t pick = order % grid;
    while (left) {
        while (!g[pick].running) pick = (pick + 1) % grid;
        Group &w = g[pick];
        const uint32_t b = pick, it = w.item;
        if (it >= n_items || taken[it]) return 5;
        taken[it] = 1;
        if (w.count && it <= w.last) return 6; // a workgroup's items ascend
        w.last = it;
        w.count += 1;
        const bool in_static = first_next_is_static(it, n_static);
        const bool follows = !in_static && chunk_follows(it - n_static, body, chunk);
        if (!in_static && follows != (w.left > 0u)) return 7; // true exactly inside a chunk
        uint32_t drawn = 0;
        if (!in_static && !follows) drawn = grid + counter++; // issued at the start of the item, one item ahead
        if (in_static) {
            w.item = it + grid;
            if (w.item >= n_static) {
                if (w.item - n_static != b) return 8;
                if ((w.item = draw(b, b)) == 0xffffffffu) return 9;
            }
        } else if (follows) {
            w.item = it + 1u;
            w.left -= 1u;
        } else if ((w.item = draw(b, drawn)) == 0xffffffffu) return 10;
        if (w.item >= n_items) {
            if (w.item != n_items) return 11;
            w.running = false;
            left -= 1;
        }
        pick = (pick + 1 + order * 7u) % grid;
    }
    for (uint32_t i = 0; i < n_items; ++i)
        if (taken[i] != 1) return 12;
    if (found != chunk_draws(d, body, chunk) || found != n_body + (d - body)) return 13;
    return 0;
}

// the header's 32-bit arithmetic against the same in 64 bits
static int exact(uint32_t d, uint32_t grid, uint32_t chunk, uint32_t tail_rounds) {
    const uint64_t tail = std::min<uint64_t>(d, static_cast<uint64_t>(grid) * tail_rounds), body = chunk * ((d - tail) / chunk), n_body = body / chunk;
    if (chunk_tail(d, grid, tail_rounds) != tail || chunk_body(d, grid, chunk, tail_rounds) != body) return 30;
    const uint64_t draws = n_body + (d - body);
    if (chunk_draws(d, static_cast<uint32_t>(body), chunk) != draws) return 31;
    const uint64_t us[8] = {0u, 1u, n_body ? n_body - 1u : 0u, n_body, n_body + 1u, draws ? draws - 1u : 0u, draws, draws + 2u * grid};
    for (uint64_t u : us) {
        if (u > 0xffffffffu) continue;
        const uint64_t want = u < n_body ? chunk * u : (u < draws ? body + (u - n_body) : d);
        if (chunk_draw_position(static_cast<uint32_t>(u), d, static_cast<uint32_t>(body), chunk) != want) return 32;
    }
    return 0;
}

int main() {
    uint32_t runs = 0;
    for (uint32_t grid : {1u, 7u, 1024u})
        for (uint32_t chunk : {1u, 2u, 4u, 8u, 16u})
            for (uint32_t tail_rounds : {0u, 1u, 4u}) {
                const uint32_t gt = grid * tail_rounds, gtc = grid * (tail_rounds + chunk);
                std::vector<uint32_t> ds = {0u, 1u, 2u, chunk - 1u, chunk, chunk + 1u, gt ? gt - 1u : 0u, gt, gt + 1u, gt + chunk - 1u, gt + chunk, gt + chunk + 1u,
                                            gtc - 1u, gtc, gtc + 1u, 259200u, 65535u * 64u};
                for (uint32_t d : ds) {
                    if (int r = exact(d, grid, chunk, tail_rounds)) return r;
                    // share 0: the range is the launch. Share 1/2: the same range behind max(d / grid, 1) static rounds where the share
                    // allows exactly that (d >= grid), and the launch of d items with whatever range the share leaves it
                    std::vector<uint32_t> launches[2] = {{d}, {d}};
                    if (d >= grid && d / grid * grid + static_cast<uint64_t>(d) <= 0xffffffffu) launches[1].push_back(d / grid * grid + d);
                    for (uint32_t share = 0; share < 2; ++share)
                        for (uint32_t n_items : launches[share])
                            for (uint32_t order : {0u, 1u, 5u}) {
                                if (int r = launch(n_items, grid, share, 2u, chunk, tail_rounds, order)) {
                                    std::printf("n_items %u grid %u share %u/2 chunk %u tail rounds %u order %u: check %d failed\n", n_items, grid, share, chunk,
                                                tail_rounds, order, r);
                                    return r;
                                }
                                runs += 1;
                            }
                }
            }
    // a range and a grid at the end of 32 bits
    if (int r = exact(0xffffffffu, 0xffffffffu, 16u, 4u)) return r;
    if (int r = exact(0xffffffffu, 1024u, 16u, 4u)) return r;
    if (int r = exact(0xffffffffu, 1u, 1u, 0u)) return r;
    std::printf("%u launches\nok\n", runs);
    return 0;
}
