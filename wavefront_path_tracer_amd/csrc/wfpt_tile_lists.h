// wfpt_tile_lists.h -- the bundle test behind the first launch's per-tile candidate lists, shared by the
// device builder (tile_lists_kernel, wfpt_kernels.hip) and its host twin (wfpt_tile_lists_host, wfpt_host.cpp). Internal.
//
// A wave of the first fused launch is one 8x8 pixel tile of one sample: its 64 primary rays leave one lens through one small patch of the
// focus plane, sample after sample, for as long as the camera stands. Which leaves of the tree such a bundle can touch is a fact about the
// tile, not about the sample: the table holds, per tile, every leaf whose margin-grown box (SceneDev::nodes_ch) the bundle can reach, and
// the first launch tests those leaves' primitives instead of walking the tree from the root (trace_tile_list, wfpt_kernels.hip).
//
// The test may say "maybe" freely and never "no" for a box some ray of the tile can reach. The bound (all in world space):
//   * Pixel range. primary_ray jitters a pixel by rng_next_in_unit_disk, one pixel either side, so the tile's rays pass the rectangle
//     [x0 - 1, x0 + 8] x [y0 - 1, y0 + 8] of pixel coordinates; it is taken kPixelPad wider.
//   * Pinhole bound. primary_ray's direction is view * G with G = pp (pinhole) or G = (focus_distance / pp.z) * pp (thin lens: the point
//     of the focus plane), pp = inv_proj * ndc / w. pp is P / w with P and w affine in the pixel coordinates, so wherever w (and, with a
//     lens, pp.z) keeps one sign over the rectangle -- checked at its corners; both are affine -- every G is a positive combination of the
//     four corner values W_k, computed here with primary_ray's own operations. The rays of a pinhole camera therefore lie in the pyramid
//     A + cone(W_0 .. W_3), A = the camera position.
//   * Thin-lens bound. A ray leaves A + L, L = view * (l, 0), |l| <= R = defocus_radius, towards A + W: its point at fraction u >= 0 of the
//     way is A + u W + (1 - u) L. With n an inward unit normal of a side plane of the pyramid, n . (x - A) = u n . W + (1 - u) n . L
//     >= -|1 - u| |L|: the bundle lies in the pyramid dilated by |L| max(1, u - 1), |L| <= R * s with s the largest singular value of
//     view's first two columns (s^2 <= max(|c0|^2, |c1|^2) + |c0 . c1|; 1 for a rigid view). With f the unit normal of the lens plane
//     (c0 x c1, so f . L = 0), f . (x - A) = u f . W: u <= depth / min_k f . W_k, taken at the box's far depth, and a box wholly behind
//     the lens plane is out of reach.
//   * Slop. What the device computes differs from this by rounding: the pixel coordinates, ndc and the two matrix products of primary_ray
//     carry relative errors of a few 2^-24 each (under 16 * 2^-24 on the direction for a matrix whose terms do not cancel), a direction
//     that much off moves a point at distance D by D * 2^-20, and the plane distances below are sums of six products of magnitude at most
//     |c - A|, |A| + |c| and |h|, each rounded to 2^-24. kSlop = 2^-18 of the sum of those magnitudes (and of R s) covers both four times
//     over; the unit normals' own error (2^-22 of their length) scales the same sums. kPixelPad = 1/16 pixel keeps the sixteenth of a
//     pixel beyond it for the jitter's own rounding (|off| <= 1 + 2^-22).
// A camera the bound does not cover (a view that is not affine, a w or pp.z that changes sign or vanishes, a value that is not finite, an
// image wider or higher than 2^14) gives "no list" for the tile, and so does a tile with more than kTileListCap candidates.
//
// Every operation is written out (one IEEE f32 operation per step, fma where named; build with -ffp-contract=off), so the host twin and
// the device builder produce the same bits.
#pragma once
#include <stdint.h>

#include "wfpt.h"

#if defined(__HIP__)
#define WFPT_TL_FN __host__ __device__ inline
#else
#define WFPT_TL_FN inline
#endif

namespace wfpt {

// One 64-byte record per local tile: up to kTileListCap leaf words (left_first | prim_count << 16, never 0: a leaf holds a primitive) in
// ascending node order, the rest 0. word[0] = kTileNoList: no list, the wave walks the tree.
constexpr uint32_t kTileListCap = 16;
constexpr uint32_t kTileNoList = 0xffffffffu;
constexpr float kTilePixelPad = 0.0625f;
constexpr float kTileSlop = 3.8146973e-6f; // 2^-18

struct TileBundle {
    float ax, ay, az;    // apex A
    float n[4][3];       // inward unit normals of the side planes
    float fx, fy, fz;    // unit normal of the lens plane, towards the scene
    float rw;            // bound on |L| (0 for a pinhole camera)
    float inv_df;        // 1 / min_k f . W_k
    float a1;            // |A|_1
    uint32_t ok;         // 0: the camera is not covered, no list
};

WFPT_TL_FN bool tl_finite(float v) { return __builtin_fabsf(v) < 1e30f; } // false for NaN too

// The bundle of the tile whose first pixel is (x0, y0). inv_proj, view: column-major, as CameraDev holds them.
WFPT_TL_FN TileBundle tile_bundle(const wfpt_gpu_camera &cam, const float *inv_proj, const float *view, uint32_t x0, uint32_t y0, uint32_t width,
                                  uint32_t height) {
    TileBundle b;
    b.ok = 0u;
    const bool lens = cam.defocus_radius > 0.0f;
    const float fw = static_cast<float>(width), fh = static_cast<float>(height);
    const float px[2] = {(static_cast<float>(x0) - 1.0f) - kTilePixelPad, (static_cast<float>(x0) + 8.0f) + kTilePixelPad};
    const float py[2] = {(static_cast<float>(y0) - 1.0f) - kTilePixelPad, (static_cast<float>(y0) + 8.0f) + kTilePixelPad};
    float w[4][3];
    bool ok = width <= 16384u && height <= 16384u && view[3] == 0.0f && view[7] == 0.0f && view[11] == 0.0f && view[15] == 1.0f;
    float sign_w = 0.0f, sign_z = 0.0f;
    for (int k = 0; k < 4; ++k) { // corners in order around the rectangle
        const float cx = px[(k == 1 || k == 2) ? 1 : 0], cy = py[k >= 2 ? 1 : 0];
        float ndc_x = cx / fw; // gr:66-67
        float ndc_y = 1.0f - cy / fh;
        ndc_x = 2.0f * ndc_x - 1.0f;
        ndc_y = 2.0f * ndc_y - 1.0f;
        const float qx = ((inv_proj[0] * ndc_x + inv_proj[4] * ndc_y) + inv_proj[8] * 1.0f) + inv_proj[12] * 1.0f; // gr:68 (mat_mul)
        const float qy = ((inv_proj[1] * ndc_x + inv_proj[5] * ndc_y) + inv_proj[9] * 1.0f) + inv_proj[13] * 1.0f;
        const float qz = ((inv_proj[2] * ndc_x + inv_proj[6] * ndc_y) + inv_proj[10] * 1.0f) + inv_proj[14] * 1.0f;
        const float qw = ((inv_proj[3] * ndc_x + inv_proj[7] * ndc_y) + inv_proj[11] * 1.0f) + inv_proj[15] * 1.0f;
        float gx = qx / qw, gy = qy / qw, gz = qz / qw; // gr:69
        ok = ok && tl_finite(gx) && tl_finite(gy) && tl_finite(gz) && qw != 0.0f && (k == 0 || (qw > 0.0f) == (sign_w > 0.0f));
        sign_w = k == 0 ? qw : sign_w;
        if (lens) { // gr:80-81 with the lens point at the centre
            ok = ok && gz != 0.0f && (k == 0 || (gz > 0.0f) == (sign_z > 0.0f));
            sign_z = k == 0 ? gz : sign_z;
            const float tf = cam.focus_distance / gz;
            gx = tf * gx;
            gy = tf * gy;
            gz = tf * gz;
        }
        w[k][0] = ((view[0] * gx + view[4] * gy) + view[8] * gz) + view[12] * 0.0f; // gr:84
        w[k][1] = ((view[1] * gx + view[5] * gy) + view[9] * gz) + view[13] * 0.0f;
        w[k][2] = ((view[2] * gx + view[6] * gy) + view[10] * gz) + view[14] * 0.0f;
        ok = ok && tl_finite(w[k][0]) && tl_finite(w[k][1]) && tl_finite(w[k][2]);
    }
    // the apex: the lens centre view * (0, 0, 0, 1), or the camera position of a pinhole camera (gr:71)
    b.ax = lens ? view[12] : cam.position[0];
    b.ay = lens ? view[13] : cam.position[1];
    b.az = lens ? view[14] : cam.position[2];
    b.a1 = (__builtin_fabsf(b.ax) + __builtin_fabsf(b.ay)) + __builtin_fabsf(b.az);
    ok = ok && tl_finite(b.a1);
    // the lens plane's normal c0 x c1 and the reach of a lens point
    const float c0x = view[0], c0y = view[1], c0z = view[2], c1x = view[4], c1y = view[5], c1z = view[6];
    float fx = c0y * c1z - c0z * c1y, fy = c0z * c1x - c0x * c1z, fz = c0x * c1y - c0y * c1x;
    const float fl = __builtin_sqrtf((fx * fx + fy * fy) + fz * fz);
    ok = ok && fl > 0.0f && tl_finite(fl);
    float inv = 1.0f / fl;
    if (((fx * w[0][0] + fy * w[0][1]) + fz * w[0][2]) < 0.0f) inv = -inv;
    fx = fx * inv;
    fy = fy * inv;
    fz = fz * inv;
    b.fx = fx; b.fy = fy; b.fz = fz;
    float df = 1e30f;
    for (int k = 0; k < 4; ++k) {
        const float d = (fx * w[k][0] + fy * w[k][1]) + fz * w[k][2];
        df = d < df ? d : df;
    }
    ok = ok && df > 0.0f;
    b.inv_df = 1.0f / df;
    if (lens) {
        const float n0 = (c0x * c0x + c0y * c0y) + c0z * c0z, n1 = (c1x * c1x + c1y * c1y) + c1z * c1z;
        const float s2 = (n0 > n1 ? n0 : n1) + __builtin_fabsf((c0x * c1x + c0y * c1y) + c0z * c1z);
        b.rw = (cam.defocus_radius * __builtin_sqrtf(s2)) * 1.000001f;
        ok = ok && tl_finite(b.rw);
    } else {
        b.rw = 0.0f;
    }
    for (int k = 0; k < 4; ++k) { // side plane through A, W_k and W_k+1, its normal towards W_k+2
        const float *u = w[k], *v = w[(k + 1) & 3], *t = w[(k + 2) & 3];
        float nx = u[1] * v[2] - u[2] * v[1], ny = u[2] * v[0] - u[0] * v[2], nz = u[0] * v[1] - u[1] * v[0];
        const float nl = __builtin_sqrtf((nx * nx + ny * ny) + nz * nz);
        ok = ok && nl > 0.0f && tl_finite(nl);
        float ninv = 1.0f / nl;
        if (((nx * t[0] + ny * t[1]) + nz * t[2]) < 0.0f) ninv = -ninv;
        b.n[k][0] = nx * ninv;
        b.n[k][1] = ny * ninv;
        b.n[k][2] = nz * ninv;
        ok = ok && tl_finite(b.n[k][0]) && tl_finite(b.n[k][1]) && tl_finite(b.n[k][2]);
    }
    b.ok = ok ? 1u : 0u;
    return b;
}

// Can a ray of bundle b (b.ok != 0) reach the box of centre c and half-extent h? "false" only when it cannot.
WFPT_TL_FN bool tile_bundle_reaches(const TileBundle &b, float cx, float cy, float cz, float hx, float hy, float hz) {
    const float dx = cx - b.ax, dy = cy - b.ay, dz = cz - b.az;
    const float mag = ((((__builtin_fabsf(dx) + __builtin_fabsf(dy)) + __builtin_fabsf(dz)) + ((hx + hy) + hz)) + b.a1) +
                      ((((__builtin_fabsf(cx) + __builtin_fabsf(cy)) + __builtin_fabsf(cz))) + b.rw);
    const float slop = kTileSlop * mag;
    if (!(mag < 1e30f)) return true; // a box that is not finite: maybe
    // the far depth of the box over the lens plane
    const float depth = ((b.fx * dx + b.fy * dy) + b.fz * dz) + ((__builtin_fabsf(b.fx) * hx + __builtin_fabsf(b.fy) * hy) + __builtin_fabsf(b.fz) * hz);
    if (depth + slop < 0.0f) return false;
    const float u1 = (depth + slop) * b.inv_df - 1.0f; // u - 1 at the far depth, rounded by less than the slop's share of it ...
    const float rho = b.rw * ((u1 > 1.0f ? u1 : 1.0f) * 1.000001f) + slop; // ... which the factor pays for
    bool reach = true;
    for (int k = 0; k < 4; ++k) {
        const float nx = b.n[k][0], ny = b.n[k][1], nz = b.n[k][2];
        const float s = ((nx * dx + ny * dy) + nz * dz) + ((__builtin_fabsf(nx) * hx + __builtin_fabsf(ny) * hy) + __builtin_fabsf(nz) * hz);
        reach = reach && !(s + rho < 0.0f);
    }
    return reach;
}

// The first pixel of local tile `tile` (generate_rays' numbering, gr:42-57: gx tiles per row, the rows of tiles this context's bands)
WFPT_TL_FN void tile_origin(uint32_t tile, uint32_t gx, uint32_t rank, uint32_t world, uint32_t &x0, uint32_t &y0) {
    const uint32_t wx = tile % gx, wy = tile / gx;
    x0 = wx * 8u;
    y0 = (wy * world + rank) * 8u;
}

// nodes_ch's node i as a candidate: its leaf word, 0 when node i is no leaf (or the pad slot, bvh.rs:160-161), kTileNoList for a leaf the
// word cannot name (a scene in LDS holds fewer than 2^16 primitives, so there is none: the builders then write no list at all)
WFPT_TL_FN uint32_t tile_leaf_word(uint32_t i, uint32_t left_first, uint32_t prim_count) {
    if (i == 1u || prim_count == 0u) return 0u;
    if (prim_count >= 0xffffu || left_first > 0xffffu) return kTileNoList;
    return left_first | (prim_count << 16);
}

} // namespace wfpt
