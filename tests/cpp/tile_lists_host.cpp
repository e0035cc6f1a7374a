// Drives the host twin of the tile-list builder (wfpt_tile_lists_host, wfpt_host.cpp; csrc/wfpt_tile_lists.h) under AddressSanitizer +
// UBSan (tests/test_tile_lists_host.py): the book scene under the book camera with and without its lens, the five-sphere scene under the
// head-on camera, whole and partial tiles, band-sharded contexts, cameras the bound does not cover. No GPU code is linked.
#include "wfpt.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

// (centre | left_first), (half-extent | prim_count) per node, the half-extent grown by 2^-17 of the scene's extent: what
// wfpt_debug_nodes_ch computes, near enough for a run that looks for memory errors
static std::vector<float> boxes_of(const std::vector<wfpt_bvh_node> &nodes) {
    float extent = 0.0f;
    for (size_t i = 0; i < nodes.size(); ++i)
        for (int ax = 0; ax < 3 && i != 1; ++ax) extent = std::fmax(extent, std::fmax(std::fabs(nodes[i].aabb_min[ax]), std::fabs(nodes[i].aabb_max[ax])));
    std::vector<float> ch(8 * nodes.size());
    for (size_t i = 0; i < nodes.size(); ++i) {
        for (int ax = 0; ax < 3; ++ax) {
            ch[8 * i + ax] = 0.5f * (nodes[i].aabb_min[ax] + nodes[i].aabb_max[ax]);
            ch[8 * i + 4 + ax] = 0.5f * (nodes[i].aabb_max[ax] - nodes[i].aabb_min[ax]) + std::ldexp(extent, -17);
        }
        std::memcpy(&ch[8 * i + 3], &nodes[i].left_first, 4);
        std::memcpy(&ch[8 * i + 7], &nodes[i].prim_count, 4);
    }
    return ch;
}

static int run(const std::vector<wfpt_bvh_node> &nodes, const float from[3], const float at[3], float vfov_deg, float defocus_deg, uint32_t w,
               uint32_t h, uint32_t rank, uint32_t world, bool break_view) {
    float pitch, yaw, view[16], ip[16];
    wfpt_gpu_camera cam;
    wfpt_camera_new(from, at, &pitch, &yaw);
    wfpt_view_transform(from, pitch, yaw, view);
    wfpt_p_inv(wfpt_to_radians(vfov_deg), static_cast<float>(w) / static_cast<float>(h), 0.1f, 100.0f, ip);
    wfpt_gpu_camera_new(from, pitch, yaw, wfpt_to_radians(defocus_deg), 10.0f, &cam);
    if (break_view) view[3] = 0.5f; // not affine: every tile must say "no list"
    const uint32_t gx = (w + 7) / 8, bands = (h + 7) / 8, gy = bands > rank ? (bands - rank + world - 1) / world : 0;
    const std::vector<float> ch = boxes_of(nodes);
    std::vector<uint32_t> rec(static_cast<size_t>(gx) * gy * WFPT_TILE_LIST_CAP + 1, 0xdeadbeefu);
    if (wfpt_tile_lists_host(ch.data(), static_cast<uint32_t>(nodes.size()), &cam, ip, view, w, h, rank, world, rec.data(), gx * gy) != WFPT_OK) return 1;
    if (rec.back() != 0xdeadbeefu) return 2;
    uint32_t none = 0, longest = 0;
    for (uint32_t t = 0; t < gx * gy; ++t) {
        const uint32_t *r = &rec[static_cast<size_t>(t) * WFPT_TILE_LIST_CAP];
        uint32_t n = 0;
        if (r[0] == WFPT_TILE_NO_LIST) { none += 1; continue; }
        while (n < WFPT_TILE_LIST_CAP && r[n] != 0) ++n;
        longest = n > longest ? n : longest;
    }
    if (break_view && none != gx * gy) return 3;
    std::printf("%ux%u rank %u/%u defocus %.1f: %u tiles, %u without a list, longest %u\n", w, h, rank, world, defocus_deg, gx * gy, none, longest);
    // a tile count that does not match is refused
    if (wfpt_tile_lists_host(ch.data(), static_cast<uint32_t>(nodes.size()), &cam, ip, view, w, h, rank, world, rec.data(), gx * gy + 1) != WFPT_ERR_INVALID_ARGUMENT) return 4;
    return 0;
}

int main() {
    std::vector<wfpt_sphere> sp(512);
    std::vector<wfpt_material> mt(512);
    const float book[3] = {13, 2, 3}, origin[3] = {0, 0, 0}, front[3] = {0, 0, 1}, back[3] = {0, 0, -1};
    {
        const uint32_t n = wfpt_scene_book_one_final(1, sp.data(), mt.data(), 512);
        std::vector<wfpt_bvh_node> nodes(2 * n);
        uint32_t nn = 0;
        if (wfpt_build_bvh(sp.data(), n, nodes.data(), 2 * n, &nn) != 0) return 10;
        nodes.resize(nn);
        for (float defocus : {0.6f, 0.0f})
            for (uint32_t wh : {128u << 16 | 72u, 64u << 16 | 40u, 60u << 16 | 44u, 1u << 16 | 1u, 400u << 16 | 225u})
                if (int r = run(nodes, book, origin, 20.0f, defocus, wh >> 16, wh & 0xffffu, 0, 1, false)) return r;
        if (int r = run(nodes, book, origin, 20.0f, 0.6f, 128, 72, 1, 3, false)) return r;
        if (int r = run(nodes, book, origin, 20.0f, 0.6f, 128, 72, 7, 8, false)) return r;
        if (int r = run(nodes, book, origin, 20.0f, 0.6f, 64, 40, 0, 1, true)) return r;
    }
    {
        const uint32_t n = wfpt_scene_new(sp.data(), mt.data());
        std::vector<wfpt_bvh_node> nodes(2 * n);
        uint32_t nn = 0;
        if (wfpt_build_bvh(sp.data(), n, nodes.data(), 2 * n, &nn) != 0) return 11;
        nodes.resize(nn);
        if (int r = run(nodes, front, back, 90.0f, 0.0f, 64, 64, 0, 1, false)) return r;
    }
    std::puts("ok");
    return 0;
}
