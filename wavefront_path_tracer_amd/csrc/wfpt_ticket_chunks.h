// wfpt_ticket_chunks.h -- what one draw from Control::ticket buys in the fused launches (bounce_kernel, wfpt_kernels.hip; DESIGN.md
// section 4, round 9), shared by the kernel and a host test (tests/cpp/chunk_schedule_host.cpp). Internal.
//
// A launch hands a dynamic range of D positions to its G workgroups by one counter: workgroup b holds draw b from the start and draws
// G + atomicAdd(ticket, 1) from then on, one item ahead. One returning atomic per position saturates the counter's word (the first launch:
// 87 draws per us), so most draws buy a chunk of C consecutive positions, and the positions of a chunk follow one another with no atomic,
// no exchange through LDS and nothing loaded between two items. The end of the range goes out singly, so that whoever is free still evens
// out the tail. With tail = min(D, G * T) and body = C * floor((D - tail) / C):
//   * draw u < n_body = body / C           is the positions [C * u, C * u + C);
//   * draw n_body <= u < n_body + D - body is the single position body + (u - n_body);
//   * any larger draw finds nothing left (chunk_draw_position returns D).
// Position p is followed by p + 1 without a draw exactly when p < body and p % C != C - 1: a function of p alone (a mask for a power of
// two), so a workgroup keeps no count of what is left of its chunk. The draw for what comes after a chunk is issued at the start of the
// chunk's last position. A workgroup's positions ascend. C = 1 is one position per draw: position = draw, body = D - tail, nothing follows.
#pragma once
#include <stdint.h>

#if defined(__HIP__)
#define WFPT_TC_FN __host__ __device__ constexpr
#else
#define WFPT_TC_FN constexpr
#endif

namespace wfpt {

// positions at the end of the range that are drawn one at a time: `tail_rounds` per workgroup
WFPT_TC_FN uint32_t chunk_tail(uint32_t d, uint32_t grid, uint32_t tail_rounds) {
    const uint64_t t = static_cast<uint64_t>(grid) * tail_rounds;
    return t < d ? static_cast<uint32_t>(t) : d;
}
// positions handed out as whole chunks of `chunk` (>= 1): [0, body)
WFPT_TC_FN uint32_t chunk_body(uint32_t d, uint32_t grid, uint32_t chunk, uint32_t tail_rounds) {
    return chunk * ((d - chunk_tail(d, grid, tail_rounds)) / chunk);
}
// draws that find something: the chunks of the body and the singles behind it
WFPT_TC_FN uint32_t chunk_draws(uint32_t d, uint32_t body, uint32_t chunk) { return body / chunk + (d - body); }
// the first (or only) position of draw u; d: nothing left. (chunk * u < body and body + (u - n_body) < d where they are formed.)
WFPT_TC_FN uint32_t chunk_draw_position(uint32_t u, uint32_t d, uint32_t body, uint32_t chunk) {
    const uint32_t n_body = body / chunk;
    return u < n_body ? chunk * u : (u - n_body < d - body ? body + (u - n_body) : d);
}
// is position p followed by p + 1 without a draw?
WFPT_TC_FN bool chunk_follows(uint32_t p, uint32_t body, uint32_t chunk) { return p < body && p % chunk != chunk - 1u; }

} // namespace wfpt
