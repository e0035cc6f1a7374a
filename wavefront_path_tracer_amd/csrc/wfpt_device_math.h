// wfpt_device_math.h -- gfx950 device arithmetic for the wavefront kernels.
//
// The WGSL built-ins the reference's shaders call (sqrt, sin, cos, pow, min, max, normalize, dot,
// f32(u32)) have backend-defined precision, so the build fixes one definition of each, made only of
// IEEE-754 binary32 add/sub/mul/div/sqrt/fma and integer bit operations in a fixed order:
//   * hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt gives correctly rounded `/` and sqrt;
//   * this translation unit is compiled with -ffp-contract=off, the only fused operations are the
//     explicit __builtin_fmaf calls below (v_fma_f32);
//   * fp32 denormals are not flushed on gfx950 (and no result below is ever denormal).
// The CPU oracle carries its own independent statement of the same definitions; the GPU tests compare
// the two bit for bit (wfpt_selftest_math).
//
// Citations: gr = gpu_wavefront_pt/shaders/generate_rays.wgsl, sh = .../shade.wgsl.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wfpt {

__device__ __forceinline__ float fma_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__host__ __device__ __forceinline__ float sqrt_(float x) { return __builtin_sqrtf(x); }
// minNum / maxNum (v_min_f32 / v_max_f32): a NaN operand yields the other operand
__device__ __forceinline__ float min_(float a, float b) { return __builtin_fminf(a, b); }
__device__ __forceinline__ float max_(float a, float b) { return __builtin_fmaxf(a, b); }

// ---------------- integer RNG (gr:138-181, identical in sh:228-266) ----------------
__device__ __forceinline__ uint32_t jenkins_hash(uint32_t x) { // gr:173-181
    x += x << 10;
    x ^= x >> 6;
    x += x << 3;
    x ^= x >> 11;
    x += x << 15;
    return x;
}
__device__ __forceinline__ uint32_t init_rng(uint32_t px, uint32_t py, uint32_t res_x, uint32_t frame) { // gr:138-141
    return jenkins_hash((px + py * res_x) ^ jenkins_hash(frame));
}
__device__ __forceinline__ uint32_t rng_next_int(uint32_t &state) { // gr:146-153, PCG-RXS-M-XS-32
    const uint32_t s = state * 747796405u + 2891336453u;
    state = s;
    const uint32_t word = ((s >> ((s >> 28) + 4u)) ^ s) * 277803737u;
    return (word >> 22) ^ word;
}
__device__ __forceinline__ float u32_to_unit_float(uint32_t x) { // gr:133-136: f32(x) * 2^-32, RTNE
    return static_cast<float>(x) * 2.3283064365387e-10f;
}
__device__ __forceinline__ float rng_next_float(uint32_t &state) { return u32_to_unit_float(rng_next_int(state)); }
// gr:155-171: the skip-ahead as written (only the final `delta == 1` step accumulates)
__device__ __forceinline__ uint32_t advance(uint32_t state, uint32_t advance_by) {
    uint32_t acc_mult = 1u, acc_plus = 0u, cur_mult = 747796405u, cur_plus = 2891336453u;
    for (uint32_t delta = advance_by; delta > 0; delta >>= 1) {
        if (delta == 1) {
            acc_mult *= cur_mult;
            acc_plus = acc_plus * cur_mult + cur_plus;
        }
        cur_plus = (cur_mult + 1u) * cur_plus;
        cur_mult *= cur_mult;
    }
    return state * acc_mult + acc_plus;
}

// ---------------- sin / cos ----------------
// Quadrant reduction k = rint(x * 2/pi), r = x - k*pi/2 with pi/2 split in three (Cody-Waite, fma),
// Cephes single-precision polynomials on [-pi/4, pi/4].
__device__ __forceinline__ void sincos_(float x, float &sin_out, float &cos_out) {
    const float k = __builtin_rintf(x * 0.63661975f);
    float r = fma_(-k, 1.5703125f, x);
    r = fma_(-k, 4.837512969970703125e-4f, r);
    r = fma_(-k, 7.54978995489188216e-8f, r);
    const float z = r * r;
    float ps = fma_(z, -1.9515295891e-4f, 8.3321608736e-3f);
    ps = fma_(z, ps, -1.6666654611e-1f);
    const float s = fma_(r * z, ps, r);
    float pc = fma_(z, 2.443315711809948e-5f, -1.388731625493765e-3f);
    pc = fma_(z, pc, 4.166664568298827e-2f);
    const float c = fma_(z * z, pc, fma_(z, -0.5f, 1.0f));
    const int q = static_cast<int>(k) & 3;
    float sq = (q & 1) ? c : s;
    float cq = (q & 1) ? s : c;
    sq = (q & 2) ? -sq : sq;
    cq = ((q + 1) & 2) ? -cq : cq;
    sin_out = sq;
    cos_out = cq;
}

// ---------------- pow(x, y) = exp2(y * log2(x)) ----------------
__device__ __forceinline__ float log2_pos(float x) { // normal x > 0
    const uint32_t bits = __float_as_uint(x);
    int e = static_cast<int>(bits >> 23) - 127;
    float m = __uint_as_float((bits & 0x007fffffu) | 0x3f800000u);
    if (m > 1.41421356f) { m = m * 0.5f; e += 1; }
    const float f = m - 1.0f;
    const float z = f * f;
    float p = fma_(f, 7.0376836292e-2f, -1.1514610310e-1f);
    p = fma_(f, p, 1.1676998740e-1f);
    p = fma_(f, p, -1.2420140846e-1f);
    p = fma_(f, p, 1.4249322787e-1f);
    p = fma_(f, p, -1.6668057665e-1f);
    p = fma_(f, p, 2.0000714765e-1f);
    p = fma_(f, p, -2.4999993993e-1f);
    p = fma_(f, p, 3.3333331174e-1f);
    const float ln_m = fma_(f * z, p, fma_(z, -0.5f, f));
    return fma_(ln_m, 1.44269504f, static_cast<float>(e));
}
__device__ __forceinline__ float exp2_(float x) {
    if (x != x) return x;
    if (x < -125.0f) return 0.0f;
    if (x > 127.0f) return __uint_as_float(0x7f800000u);
    const float n = __builtin_rintf(x);
    const float g = x - n;
    float p = fma_(g, 1.535336188319500e-4f, 1.339887440266574e-3f);
    p = fma_(g, p, 9.618437357674640e-3f);
    p = fma_(g, p, 5.550332471162809e-2f);
    p = fma_(g, p, 2.402264791363012e-1f);
    p = fma_(g, p, 6.931472028550421e-1f);
    p = fma_(g, p, 1.0f);
    return p * __uint_as_float(static_cast<uint32_t>(static_cast<int>(n) + 127) << 23);
}
__device__ __forceinline__ float pow_(float x, float y) { // sh:120 (y = 0.33333), sh:161 (y = 5)
    if (x == 0.0f) return 0.0f;
    if (!(x > 0.0f)) return __uint_as_float(0x7fc00000u);
    return exp2_(y * log2_pos(x));
}

// ---------------- small vectors: fixed association order, no contraction ----------------
struct float3_ { float x, y, z; };
__host__ __device__ __forceinline__ float dot3(float3_ a, float3_ b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
// WGSL normalize(v): the built-in's accuracy is that of v / length(v) (2.5 ULP per component); the definition fixed here since round 4
// is v * (1 / length(v)): one IEEE division and three products instead of three divisions (a correctly rounded division is ~11
// instructions, most of them half rate), at most 1.5 ULP from the quotient form. Rounds 1-3 divided each component.
__host__ __device__ __forceinline__ float3_ normalize3(float3_ a) {
    const float inv = 1.0f / sqrt_(dot3(a, a));
    return {a.x * inv, a.y * inv, a.z * inv};
}

// ---------------- environment map (WFPT_FLAG_ENVIRONMENT; include/wfpt.h "Environment map") ----------------
// Only IEEE f32 add / sub / mul / div / sqrt, comparisons, selects and floor, no fma: numpy float32 restates every step bit for bit
// (tests/environment_ref.py).
//
// atan2_(y, x): a Cephes atanf (Moshier) polynomial on a reduced ratio of lo = min(|x|, |y|) and hi = max(|x|, |y|), then the octant and
// quadrant fix-ups. Constants that are not floats are carried as hi + lo pairs:
//   t = lo / hi (0 when hi == 0);  r = t, base = 0            when t <= tan(pi/8)
//                                  r = (2 lo - hi) / (2 hi + lo), base = atan(1/2)   otherwise (the ratio's exact difference form of
//                                  (t - 1/2) / (1 + t/2): 2 lo - hi is exact there, so r carries two roundings, not four)
//   z = r r;  p = (((c3 z - c2) z + c1) z - c0) z;  a = base_hi + (base_lo + (p r + r))    (a = p r + r when base = 0)
//   |y| > |x|:  a <- pi/2_hi + (pi/2_lo - a);    x < 0:  a <- pi_hi + (pi_lo - a);    y < 0:  a <- -a
// The signs are read by comparisons, so a zero of either sign counts as positive: atan2_(+-0, +-0) = 0, atan2_(+-0, x < 0) = pi,
// atan2_(+-0, x > 0) = 0, atan2_(y > 0, +-0) = pi/2, atan2_(y < 0, +-0) = -pi/2. Finite inputs below 2^126 in magnitude are within 2 ulp of
// the true atan2 (1.8 measured; tests/test_environment_host.py).
__host__ __device__ __forceinline__ float atan2_(float y, float x) {
    const float ax = __builtin_fabsf(x), ay = __builtin_fabsf(y);
    const float hi = ax > ay ? ax : ay, lo = ax > ay ? ay : ax;
    const float t = hi > 0.0f ? lo / hi : 0.0f;
    const bool big = t > 0.41421356f;
    const float r = big ? (2.0f * lo - hi) / (2.0f * hi + lo) : t;
    const float z = r * r;
    const float p = (((8.05374449538e-2f * z - 1.38776856032e-1f) * z + 1.99777106478e-1f) * z - 3.33329491539e-1f) * z;
    float a = p * r + r;
    if (big) a = 4.636476040e-01f + (5.012158688e-09f + a);
    if (ay > ax) a = 1.570796371e+00f + (-4.371138829e-08f - a);
    if (x < 0.0f) a = 3.141592741e+00f + (-8.742277657e-08f - a);
    return y < 0.0f ? -a : a;
}

// The map's value in direction d (not necessarily unit length): a w x h equirectangular map of float4 texels (rgb, unused), row 0 = +y,
// column w/2 faces -z, `rotation` in turns added to u, bilinear with texel centres at half-integers, columns wrapping and rows clamped.
//   n = normalize3(d);  phi = atan2_(n.x, -n.z);  theta = atan2_(sqrt(n.x n.x + n.z n.z), n.y)
//   u = phi / 2pi + (0.5 + rotation), u <- u - floor(u);  v = theta / pi
//   x = u w - 0.5, x0 = floor(x), fx = x - x0 (the same for y); column x0 mod w and x0 + 1 mod w, rows clamp(y0), clamp(y0 + 1)
//   c = (((t00 (1-fx)(1-fy) + t10 fx (1-fy)) + t01 (1-fx) fy) + t11 fx fy) * intensity      (each weight one product)
// x0 and y0 are clamped to the map (as floats) before they become indices, so no direction reads outside the map. A zero, NaN or infinite
// direction normalises to NaN components; atan2_'s comparisons are all false for them, so phi = theta = 0 and the lookup is the ordinary one at
// u = 0.5 + rotation, v = 0. A direction whose squared length underflows normalises to +-inf components; atan2_ then divides inf by inf, x0 and
// y0 are NaN, fmax(NaN, -1) = -1 and fmax(NaN, 0) = 0 pick columns w - 1 and 0 of row 0, and the NaN weights make the result NaN.
__host__ __device__ __forceinline__ float3_ env_lookup(const float4 *tex, uint32_t w, uint32_t h, float intensity, float rotation, float dx,
                                                       float dy, float dz) {
    const float3_ n = normalize3({dx, dy, dz});
    const float phi = atan2_(n.x, -n.z);
    const float theta = atan2_(sqrt_(n.x * n.x + n.z * n.z), n.y);
    float u = phi * 0.15915494f + (0.5f + rotation);
    u = u - __builtin_floorf(u);
    const float v = theta * 0.31830988f;
    const float fw = static_cast<float>(w), fh = static_cast<float>(h);
    const float x = u * fw - 0.5f, y = v * fh - 0.5f;
    const float x0 = __builtin_floorf(x), y0 = __builtin_floorf(y);
    const float fx = x - x0, fy = y - y0;
    const int i0 = static_cast<int>(__builtin_fminf(__builtin_fmaxf(x0, -1.0f), fw - 1.0f)); // -1 .. w-1
    const uint32_t c0 = i0 < 0 ? w - 1u : static_cast<uint32_t>(i0);
    const uint32_t c1 = static_cast<uint32_t>(i0 + 1) >= w ? 0u : static_cast<uint32_t>(i0 + 1);
    const size_t r0 = static_cast<size_t>(__builtin_fminf(__builtin_fmaxf(y0, 0.0f), fh - 1.0f)) * w;
    const size_t r1 = static_cast<size_t>(__builtin_fminf(__builtin_fmaxf(y0 + 1.0f, 0.0f), fh - 1.0f)) * w;
    const float4 t00 = tex[r0 + c0], t10 = tex[r0 + c1], t01 = tex[r1 + c0], t11 = tex[r1 + c1];
    const float gx = 1.0f - fx, gy = 1.0f - fy;
    const float w00 = gx * gy, w10 = fx * gy, w01 = gx * fy, w11 = fx * fy;
    return {(((t00.x * w00 + t10.x * w10) + t01.x * w01) + t11.x * w11) * intensity,
            (((t00.y * w00 + t10.y * w10) + t01.y * w01) + t11.y * w11) * intensity,
            (((t00.z * w00 + t10.z * w10) + t01.z * w01) + t11.z * w11) * intensity};
}

// ---------------- surface textures (WFPT_FLAG_TEXTURES; include/wfpt.h "Textures") ----------------
// The same rules as the environment map: IEEE f32 add / sub / mul / div / sqrt, comparisons, selects and floor, no fma; restated bit for bit
// by tests/texture_ref.py.
//
// A texture as the kernels see it: w x h float4 texels (rgb, 0), row 0 = the top (v = 1), the UV transform and the filter.
struct TexDev {
    const float4 *texels;
    uint32_t w, h;
    float scale_u, scale_v, offset_u, offset_v;
    uint32_t filter; // WFPT_TEXTURE_BILINEAR 0, WFPT_TEXTURE_NEAREST 1
    uint32_t _pad;
};

// (u, v) of the point with unit outward normal n on a sphere (Shirley book 2's get_sphere_uv, v = 0 at the -y pole)
__host__ __device__ __forceinline__ void sphere_uv(float3_ n, float &u, float &v) {
    u = atan2_(-n.z, n.x) * 0.15915494f + 0.5f;
    v = atan2_(sqrt_(n.x * n.x + n.z * n.z), -n.y) * 0.31830988f;
}

// The barycentrics b0, b1, b2 of point p on the triangle (v0, e1, e2), from the normal equations; b1 = b2 = 0 unless den > 0. One text
// for triangle_uv and shading_normal (a macro: each user is compiled from these statements, in this order)
#define WFPT_TRIANGLE_BARYCENTRICS(p, v0, e1, e2)                                                                          \
    const float3_ w = {p.x - v0.x, p.y - v0.y, p.z - v0.z};                                                                \
    const float d00 = dot3(e1, e1), d01 = dot3(e1, e2), d11 = dot3(e2, e2), d20 = dot3(w, e1), d21 = dot3(w, e2);          \
    const float den = d00 * d11 - d01 * d01;                                                                               \
    float b1 = 0.0f, b2 = 0.0f;                                                                                            \
    if (den > 0.0f) {                                                                                                      \
        const float inv = 1.0f / den;                                                                                      \
        b1 = (d11 * d20 - d01 * d21) * inv;                                                                                \
        b2 = (d00 * d21 - d01 * d20) * inv;                                                                                \
    }                                                                                                                      \
    const float b0 = (1.0f - b1) - b2

// (u, v) of point p on the triangle (v0, e1, e2) with corner UVs uv[0..5] = u0 v0 u1 v1 u2 v2: barycentrics from the normal equations
__host__ __device__ __forceinline__ void triangle_uv(float3_ p, float3_ v0, float3_ e1, float3_ e2, const float *uv, float &u, float &v) {
    WFPT_TRIANGLE_BARYCENTRICS(p, v0, e1, e2);
    u = (uv[0] * b0 + uv[2] * b1) + uv[4] * b2;
    v = (uv[1] * b0 + uv[3] * b1) + uv[5] * b2;
}

// ---------------- shading normals (WFPT_FLAG_SHADING_NORMALS; include/wfpt.h "Shading normals") ----------------
// The same rules as the textures: IEEE f32 add / sub / mul / div / sqrt and comparisons, no fma; restated bit for bit by
// tests/shading_normals_ref.py. The normal shade scatters about at point p of the triangle (v0, e1, e2) with stored normal ng and corner
// normals n0, n1, n2: the corner normals weighed by triangle_uv's barycentrics and normalised, or ng where that has no length (zero, NaN
// or infinite) or leaves ng's hemisphere. Returns true where it fell back to ng.
__host__ __device__ __forceinline__ bool shading_normal(float3_ p, float3_ v0, float3_ e1, float3_ e2, float3_ ng, float3_ n0, float3_ n1,
                                                        float3_ n2, float3_ &ns) {
    WFPT_TRIANGLE_BARYCENTRICS(p, v0, e1, e2);
    const float3_ m = {(n0.x * b0 + n1.x * b1) + n2.x * b2, (n0.y * b0 + n1.y * b1) + n2.y * b2, (n0.z * b0 + n1.z * b1) + n2.z * b2};
    const float l2 = dot3(m, m);
    const float il = 1.0f / sqrt_(l2); // normalize3's own expressions
    ns = {m.x * il, m.y * il, m.z * il};
    const bool keep = l2 > 0.0f && l2 < __builtin_inff() && dot3(ns, ng) > 0.0f; // (a NaN fails each)
    if (!keep) ns = ng;
    return !keep;
}

// ---------------- normal maps (WFPT_FLAG_NORMAL_MAPS; include/wfpt.h "Normal maps") ----------------
// Steps B-F of the header in its operation order, the same rules again (no fma); restated bit for bit by tests/normal_map_ref.py. The
// normal a mapped hit scatters about: the texel c (rgb = 0.5 + 0.5 * the tangent-space normal) at strength s, carried into the world by
// the frame (t, bt, ns) -- t the direction of dP/du of the triangle (e1, e2) with corner UVs uv[0..5], made orthogonal to the shading
// normal ns, bt = +-cross(ns, t) on dP/dv's side. Never flipped against the stored normal ng. Returns the header's probe code: 0 mapped,
// 1 identity (ns bit for bit), 2 no tangent frame (ns), 3 rejected (ns).
__host__ __device__ __forceinline__ uint32_t mapped_normal(float3_ ng, float3_ ns, float3_ e1, float3_ e2, const float *uv, float3_ c, float s,
                                                           float3_ &n) {
    n = ns;
    // B. the tangent-space normal
    const float x = (2.0f * c.x - 1.0f) * s, y = (2.0f * c.y - 1.0f) * s, z = 2.0f * c.z - 1.0f;
    if (x == 0.0f && y == 0.0f) return 1u;
    // C. dP/du and dP/dv up to |det|
    const float du1 = uv[2] - uv[0], dv1 = uv[3] - uv[1], du2 = uv[4] - uv[0], dv2 = uv[5] - uv[1];
    const float det = du1 * dv2 - du2 * dv1;
    if (!(det > 0.0f) && !(det < 0.0f)) return 2u; // (zero or NaN)
    const float sg = det > 0.0f ? 1.0f : -1.0f;
    const float3_ T = {(e1.x * dv2 - e2.x * dv1) * sg, (e1.y * dv2 - e2.y * dv1) * sg, (e1.z * dv2 - e2.z * dv1) * sg};
    const float3_ Bt = {(e2.x * du1 - e1.x * du2) * sg, (e2.y * du1 - e1.y * du2) * sg, (e2.z * du1 - e1.z * du2) * sg};
    // D. Gram-Schmidt against ns
    const float k = dot3(ns, T);
    const float3_ tt = {T.x - ns.x * k, T.y - ns.y * k, T.z - ns.z * k};
    const float l2 = dot3(tt, tt);
    if (!(l2 > 0.0f) || !(l2 < __builtin_inff())) return 2u;
    const float il = 1.0f / sqrt_(l2);
    const float3_ t = {tt.x * il, tt.y * il, tt.z * il};
    // E. the bitangent, on Bt's side (mirrored UVs keep their handedness)
    float3_ bt = {ns.y * t.z - ns.z * t.y, ns.z * t.x - ns.x * t.z, ns.x * t.y - ns.y * t.x};
    if (dot3(bt, Bt) < 0.0f) bt = {-bt.x, -bt.y, -bt.z};
    // F. into the world
    const float3_ m = {(t.x * x + bt.x * y) + ns.x * z, (t.y * x + bt.y * y) + ns.y * z, (t.z * x + bt.z * y) + ns.z * z};
    const float l2m = dot3(m, m);
    const float ilm = 1.0f / sqrt_(l2m);
    const float3_ nm = {m.x * ilm, m.y * ilm, m.z * ilm};
    if (!(l2m > 0.0f && l2m < __builtin_inff() && dot3(nm, ng) > 0.0f)) return 3u;
    n = nm;
    return 0u;
}

// ---------------- roughness maps (WFPT_FLAG_ROUGHNESS_MAPS; include/wfpt.h "Roughness maps") ----------------
// Steps R3-R4 of the header in its operation order, the same rules again (no fma, min as minNum); restated bit for bit by
// tests/roughness_map_ref.py. The GGX alpha a mapped hit is sampled with: the material's alpha_m scaled by channel `channel` (0, 1, 2 = r,
// g, b) of the texel c, clamped at 1 and, where remap is WFPT_ROUGHNESS_SQUARED (1), squared. r: the factor.
__host__ __device__ __forceinline__ float hit_roughness(float alpha_m, float3_ c, uint32_t channel, uint32_t remap, float &r) {
    r = __builtin_fminf(channel == 0u ? c.x : channel == 1u ? c.y : c.z, 1.0f);
    if (remap == 1u) r = r * r;
    return alpha_m * r;
}

// index of a texel coordinate c0 (floor of a float, expected in -1 .. n-1) and of c0 + 1, both wrapped into 0 .. n-1; NaN reads index n-1
__host__ __device__ __forceinline__ void wrap_pair(float c0, float fn, uint32_t n, uint32_t &i0, uint32_t &i1) {
    const int k = static_cast<int>(__builtin_fminf(__builtin_fmaxf(c0, -1.0f), fn - 1.0f)); // -1 .. n-1
    i0 = k < 0 ? n - 1u : static_cast<uint32_t>(k);
    i1 = static_cast<uint32_t>(k + 1) >= n ? 0u : static_cast<uint32_t>(k + 1);
}

// The texture's value at (u, v): u' = u * scale + offset, wrapped into [0, 1] by u' - floor(u'), the same for v'; then
//   bilinear: x = u' w - 0.5, y = (1 - v') h - 0.5, texel centres at half-integers, columns and rows wrapping, weights combined in
//             env_lookup's order ((t00 w00 + t10 w10) + t01 w01) + t11 w11
//   nearest:  column min(floor(u' w), w - 1), row min(floor((1 - v') h), h - 1)
__host__ __device__ __forceinline__ float3_ tex_lookup(const TexDev &t, float u, float v) {
    float uu = u * t.scale_u + t.offset_u, vv = v * t.scale_v + t.offset_v;
    uu = uu - __builtin_floorf(uu);
    vv = vv - __builtin_floorf(vv);
    const float fw = static_cast<float>(t.w), fh = static_cast<float>(t.h);
    const float ry = 1.0f - vv;
    if (t.filter == 1u) { // WFPT_TEXTURE_NEAREST
        const uint32_t cx = static_cast<uint32_t>(__builtin_fminf(__builtin_fmaxf(__builtin_floorf(uu * fw), 0.0f), fw - 1.0f));
        const uint32_t cy = static_cast<uint32_t>(__builtin_fminf(__builtin_fmaxf(__builtin_floorf(ry * fh), 0.0f), fh - 1.0f));
        const float4 c = t.texels[static_cast<size_t>(cy) * t.w + cx];
        return {c.x, c.y, c.z};
    }
    const float x = uu * fw - 0.5f, y = ry * fh - 0.5f;
    const float x0 = __builtin_floorf(x), y0 = __builtin_floorf(y);
    const float fx = x - x0, fy = y - y0;
    uint32_t c0, c1, r0, r1;
    wrap_pair(x0, fw, t.w, c0, c1);
    wrap_pair(y0, fh, t.h, r0, r1);
    const size_t o0 = static_cast<size_t>(r0) * t.w, o1 = static_cast<size_t>(r1) * t.w;
    const float4 t00 = t.texels[o0 + c0], t10 = t.texels[o0 + c1], t01 = t.texels[o1 + c0], t11 = t.texels[o1 + c1];
    const float gx = 1.0f - fx, gy = 1.0f - fy;
    const float w00 = gx * gy, w10 = fx * gy, w01 = gx * fy, w11 = fx * fy;
    return {((t00.x * w00 + t10.x * w10) + t01.x * w01) + t11.x * w11, ((t00.y * w00 + t10.y * w10) + t01.y * w01) + t11.y * w11,
            ((t00.z * w00 + t10.z * w10) + t01.z * w01) + t11.z * w11};
}

} // namespace wfpt
