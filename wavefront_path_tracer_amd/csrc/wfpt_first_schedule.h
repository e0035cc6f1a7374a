// wfpt_first_schedule.h -- how the first fused launch (bounce_kernel<kBounceFirst>, wfpt_kernels.hip) hands its work items to its
// workgroups, shared by the kernel and a host test (tests/cpp/first_schedule_host.cpp). Internal.
//
// The items of the first launch -- 512 ray slots of one sample each -- are all known before the launch and cost nearly the same, so a
// workgroup needs no counter to know most of its items. The launch's n_items are split in two ranges:
//   * static, [0, n_static): n_static = G * floor(share * n_items / G) with G = gridDim.x. Workgroup b takes b, b + G, b + 2G, ... below
//     n_static: no atomic, no exchange through LDS, and the next item depends on nothing loaded.
//   * dynamic, [n_static, n_items): handed out by Control::ticket as every fused launch hands out its items: workgroup b holds ticket b
//     from the start and draws G + atomicAdd(ticket, 1) from then on, one item ahead; ticket t is item n_static + t. The tail of the
//     launch stays balanced by whoever is free.
// A workgroup's items ascend: its static items, then n_static + b, then what it draws (all larger).
// share = WFPT_FIRST_STATIC_SHARE_NUM / WFPT_FIRST_STATIC_SHARE_DEN; 0 is the launch as it was up to round 6.
// Since round 9 a ticket of the dynamic range buys a chunk of items (wfpt_ticket_chunks.h: ticket -> position, item = n_static + position;
// with a chunk length of 1 the position is the ticket, as described here), and share 0 ships.
#pragma once
#include <stdint.h>

#if defined(__HIP__)
#define WFPT_FS_FN __host__ __device__ constexpr
#else
#define WFPT_FS_FN constexpr
#endif

namespace wfpt {

// items of the static range: whole rounds of `grid` items (0 for an empty grid or share 0; never more than n_items for share <= 1)
WFPT_FS_FN uint32_t first_n_static(uint32_t n_items, uint32_t grid, uint32_t share_num, uint32_t share_den) {
    return grid == 0u || share_den == 0u
               ? 0u
               : grid * static_cast<uint32_t>(static_cast<uint64_t>(n_items) * share_num / (static_cast<uint64_t>(share_den) * grid));
}
// static rounds of every workgroup
WFPT_FS_FN uint32_t first_static_rounds(uint32_t n_static, uint32_t grid) { return grid == 0u ? 0u : n_static / grid; }
// the k-th static item of workgroup `block` (k < first_static_rounds)
WFPT_FS_FN uint32_t first_static_item(uint32_t block, uint32_t k, uint32_t grid) { return block + k * grid; }
// the item of dynamic ticket t (a workgroup's own index is its first ticket; drawn ones are grid + the counter's value); >= n_items: none left
WFPT_FS_FN uint32_t first_dynamic_item(uint32_t n_static, uint32_t ticket) { return n_static + ticket; }
// does the workgroup that runs `item` know its next item without a ticket? (block + k * grid < n_static exactly for k < rounds, as block < grid)
WFPT_FS_FN bool first_next_is_static(uint32_t item, uint32_t n_static) { return item < n_static; }

} // namespace wfpt
