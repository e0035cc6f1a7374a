/*
 * wfpt.h -- C ABI of the MI355X-native wavefront path-tracing kernel chain
 *           generate_rays -> extend -> shade -> miss_kernel -> accumulate.
 *
 * Drop-in boundary for ONE path of rchiaramo/wavefront_path_tracer @ 2024_10_08: the kernel-stage API
 * `Kernel::new / Kernel::run / Kernel::get_timing` (gpu_wavefront_pt/src/kernel.rs:26-146) together with the
 * buffers and the wavefront loop `PathTracer::new / run` owns (gpu_wavefront_pt/src/path_tracer.rs:43-371).
 * Everything here is `extern "C"`, plain pointers and sizes; struct layouts are byte-identical to the
 * `#[repr(C)]` structs of `wavefront_common` that the reference uploads with bytemuck::cast_slice
 * (path_tracer.rs:120-156), so a Rust `-sys` shim can pass them through unchanged.
 *
 * Conventions: functions returning `int` return WFPT_OK (0) or a negative wfpt_status and never throw;
 * `wfpt_last_error` gives the message. A context is bound to one HIP device and one stream; it is not
 * thread-safe, independent contexts may be used from different threads/processes (one per GPU).
 * Calls are asynchronous on the context's stream unless they read data back.
 *
 * All citations are relative to the reference root.
 */
#ifndef WFPT_H
#define WFPT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ data model (wavefront_common) */

/* wavefront_common/src/sphere.rs:3-11 == extend.wgsl:10-15. center.w is 1.0 (sphere.rs:18-20).
 * radius may be 0 or negative; wfpt_create accepts both and the kernels do what the reference's text does. extend.wgsl:193 squares the radius
 * and shade.wgsl:93 normalises p - centre without dividing by it, so a negative radius is the sphere of |radius| with an OUTWARD normal (not
 * Shirley's hollow sphere); its box (sphere.rs:23-24) is inverted, which the slab test reads like the proper box but which does not widen the
 * boxes of its ancestors, so the sphere is only seen where those cover it anyway (e.g. inside another sphere). A sphere of radius 0 is hit
 * only where the discriminant rounds to exactly 0. Materials are not validated either: any fuzz, albedo and refraction index, non-finite ones
 * included, go through scatter() as the shader text has them (tests/test_gpu_shade_edges.py). */
typedef struct wfpt_sphere {
    float center[4];
    float radius;
    uint32_t material_idx;
    uint32_t material_type;
    uint32_t _buffer;
} wfpt_sphere;

/* wavefront_common/src/material.rs:12-20 == shade.wgsl:19-24. 0 Lambertian, 1 Metal, 2 Dielectric. */
typedef struct wfpt_material {
    float albedo[4];
    float fuzz;
    float refract_index;
    uint32_t material_type;
    uint32_t _buffer;
} wfpt_material;

/* wavefront_common/src/bvh.rs:38-45 == extend.wgsl:3-8. prim_count > 0: leaf, left_first = first
 * sphere; else left_first = left child and right child = left_first + 1. nodes[1] is a pad (bvh.rs:160). */
typedef struct wfpt_bvh_node {
    float aabb_min[3];
    uint32_t left_first;
    float aabb_max[3];
    uint32_t prim_count;
} wfpt_bvh_node;

/* BUILD EXTENSION -- the reference intersects spheres only (extend.wgsl:185-210; "other geometric shapes" and
 * OBJ loading are future items, README.md:22-26). A triangle is a vertex and two edge vectors; the hit test
 * is Moeller-Trumbore with extend.wgsl's (t_min, t_nearest) window, the shading normal is
 * normalize(cross(e1, e2)) (never flipped), HitPayload.sphere_idx carries the triangle index. 48 B. */
typedef struct wfpt_triangle {
    float v0[3];
    uint32_t material_idx;
    float e1[3];
    uint32_t material_type;
    float e2[3];
    uint32_t _pad;          /* WFPT_FLAG_TEXTURES: the triangle's row in the context's UV table (wfpt_set_triangle_uvs); 0 otherwise. The
                               BVH builders move a triangle whole, so the row follows it when they reorder. */
} wfpt_triangle;

/* wavefront_common/src/camera_controller.rs:161-185 == generate_rays.wgsl:13-19 */
typedef struct wfpt_gpu_camera {
    float position[4];
    float pitch;
    float yaw;
    float defocus_radius;
    float focus_distance;
} wfpt_gpu_camera;

/* wavefront_common/src/gpu_structs.rs:5-12 == generate_rays.wgsl:21-26 */
typedef struct wfpt_frame_buffer {
    uint32_t width;
    uint32_t height;
    uint32_t frame;
    uint32_t sample_number;
} wfpt_frame_buffer;

/* extend.wgsl:17-22: the reference's device Ray. Used only by the read-back functions; on the device
 * rays live in SoA planes. */
typedef struct wfpt_ray {
    float origin[4];
    float direction[4];
    float inv_direction[3];
    uint32_t pixel_idx;
} wfpt_ray;

/* extend.wgsl:24-29 */
typedef struct wfpt_hit_payload {
    float t;
    uint32_t ray_idx;
    uint32_t sphere_idx;
    uint32_t mat_type;
} wfpt_hit_payload;

/* Compile-time layout checks: these are the byte layouts the reference uploads with bytemuck::cast_slice
 * (path_tracer.rs:120-156) and declares in WGSL (extend.wgsl:3-29, shade.wgsl:19-24, generate_rays.wgsl:13-26). */
#if defined(__cplusplus)
#define WFPT_LAYOUT_ASSERT(cond, msg) static_assert(cond, msg)
#else
#define WFPT_LAYOUT_ASSERT(cond, msg) _Static_assert(cond, msg)
#endif
WFPT_LAYOUT_ASSERT(sizeof(wfpt_sphere) == 32 && offsetof(wfpt_sphere, radius) == 16 && offsetof(wfpt_sphere, material_idx) == 20 &&
                       offsetof(wfpt_sphere, material_type) == 24,
                   "Sphere: sphere.rs:3-11, 32 bytes");
WFPT_LAYOUT_ASSERT(sizeof(wfpt_material) == 32 && offsetof(wfpt_material, fuzz) == 16 && offsetof(wfpt_material, refract_index) == 20 &&
                       offsetof(wfpt_material, material_type) == 24,
                   "Material: material.rs:12-20, 32 bytes");
WFPT_LAYOUT_ASSERT(sizeof(wfpt_bvh_node) == 32 && offsetof(wfpt_bvh_node, left_first) == 12 && offsetof(wfpt_bvh_node, aabb_max) == 16 &&
                       offsetof(wfpt_bvh_node, prim_count) == 28,
                   "BVHNode: bvh.rs:38-45, 32 bytes");
WFPT_LAYOUT_ASSERT(sizeof(wfpt_triangle) == 48 && offsetof(wfpt_triangle, e1) == 16 && offsetof(wfpt_triangle, e2) == 32,
                   "wfpt_triangle: three 16-byte rows");
WFPT_LAYOUT_ASSERT(sizeof(wfpt_gpu_camera) == 32 && offsetof(wfpt_gpu_camera, pitch) == 16 && offsetof(wfpt_gpu_camera, yaw) == 20 &&
                       offsetof(wfpt_gpu_camera, defocus_radius) == 24 && offsetof(wfpt_gpu_camera, focus_distance) == 28,
                   "GPUCamera: camera_controller.rs:161-185, 32 bytes");
WFPT_LAYOUT_ASSERT(sizeof(wfpt_frame_buffer) == 16 && offsetof(wfpt_frame_buffer, frame) == 8 && offsetof(wfpt_frame_buffer, sample_number) == 12,
                   "GPUFrameBuffer: gpu_structs.rs:5-12, 16 bytes");
WFPT_LAYOUT_ASSERT(sizeof(wfpt_ray) == 48 && offsetof(wfpt_ray, direction) == 16 && offsetof(wfpt_ray, inv_direction) == 32 &&
                       offsetof(wfpt_ray, pixel_idx) == 44,
                   "Ray: extend.wgsl:17-22, 48 bytes");
WFPT_LAYOUT_ASSERT(sizeof(wfpt_hit_payload) == 16 && offsetof(wfpt_hit_payload, ray_idx) == 4 && offsetof(wfpt_hit_payload, sphere_idx) == 8 &&
                       offsetof(wfpt_hit_payload, mat_type) == 12,
                   "HitPayload: extend.wgsl:24-29, 16 bytes");

/* ------------------------------------------------------------------ enums */

typedef enum wfpt_status {
    WFPT_OK = 0,
    WFPT_ERR_INVALID_ARGUMENT = -1,
    WFPT_ERR_HIP = -2,          /* a HIP runtime call failed; message holds hipGetErrorString */
    WFPT_ERR_OUT_OF_MEMORY = -3,
    WFPT_ERR_UNSUPPORTED = -4,  /* e.g. BVH deeper than the traversal supports */
    WFPT_ERR_NO_DEVICE = -5     /* no gfx950 device visible: there is NO CPU fallback */
} wfpt_status;

/* Stage names are the reference's shader basenames (kernel.rs:32; call sites path_tracer.rs:162,167,175,
 * 180,185). wfpt_stage_from_name maps the strings. The three per-material stages implement the
 * reference's README to-do "split shade into by-material shade kernels" (README.md:19). */
typedef enum wfpt_stage {
    WFPT_STAGE_GENERATE_RAYS = 0, /* "generate_rays" */
    WFPT_STAGE_EXTEND = 1,        /* "extend"        */
    WFPT_STAGE_SHADE = 2,         /* "shade"         */
    WFPT_STAGE_MISS = 3,          /* "miss_kernel"   */
    WFPT_STAGE_ACCUMULATE = 4,    /* "accumulate"    */
    WFPT_STAGE_SHADE_LAMBERTIAN = 5,
    WFPT_STAGE_SHADE_METAL = 6,
    WFPT_STAGE_SHADE_DIELECTRIC = 7,
    WFPT_STAGE_SCAN = 8, /* internal helper launched with extend (queue positions + loop control); only
                            appears in wfpt_render_sample_timed's per-stage times */
    /* The device-resident loop's fused launches (not dispatchable through wfpt_kernel_run; they appear in the
     * per-stage times of wfpt_render_timed). One launch per wavefront: */
    WFPT_STAGE_BOUNCE_FIRST = 9,  /* "bounce_first": generate_rays + extend of wavefront 0 */
    WFPT_STAGE_BOUNCE = 10,       /* "bounce": shade of wavefront b-1 + extend of wavefront b + miss_kernel of b-1 */
    WFPT_STAGE_BOUNCE_LAST = 11,  /* "bounce_last": shade + miss_kernel of the last wavefront */
    WFPT_STAGE_COMPACT = 12,      /* "compact": scenes beyond LDS only -- dense per-ray results into the queues */
    WFPT_STAGE_COUNT = 13
} wfpt_stage;

/* How shade keys its RNG (shade.wgsl:72 uses the dispatch's global_invocation_id):
 *  DISPATCH: exactly that, with every atomicAdd resolved in ascending thread index (stable queues).
 *            One legal execution of the reference; the default.
 *  PIXEL:    keyed by the ray's own pixel (x = pixel_idx % W, y = pixel_idx / W). Deviates from
 *            shade.wgsl:72, but makes the image independent of queue order, which tile sharding across
 *            GPUs and the per-material split need to be bit-identical to a single-queue render. */
typedef enum wfpt_rng_mode { WFPT_RNG_DISPATCH = 0, WFPT_RNG_PIXEL = 1 } wfpt_rng_mode;

enum {
    WFPT_FLAG_SPLIT_SHADE = 1u << 0, /* fused loop runs the three per-material shade stages */
    WFPT_FLAG_NO_GRAPH = 1u << 1,    /* fused loop launches kernels directly instead of replaying a hipGraph */
    WFPT_FLAG_UNFUSED = 1u << 2,     /* device-resident loop runs the stage kernels one by one (extend, scan, shade,
                                        miss_kernel per wavefront) instead of one fused bounce launch per wavefront.
                                        Same images bit for bit; WFPT_FLAG_SPLIT_SHADE implies it. */
    WFPT_FLAG_BINARY_BVH = 1u << 3,  /* scenes too large for LDS: walk the caller's binary tree as it is instead of the
                                        four-wide collapse built at wfpt_create (same hits; for comparisons) */
    WFPT_FLAG_NO_REFILL = 1u << 4,   /* scenes too large for LDS: lanes keep their ray until the whole 512-ray segment is
                                        done (the fused bounce kernel) instead of taking new rays as they finish */
    WFPT_FLAG_NO_LDS_SCENE = 1u << 5, /* treat the scene as too large for LDS even if it fits (experiments, tests of the
                                        HBM-resident traversal on small scenes) */
    WFPT_FLAG_EXACT_TRAVERSAL = 1u << 6, /* trace_ray / hit_bvh_node exactly as extend.wgsl:72-183 writes them: slab planes
                                        (b - o) * inv with min / max per axis, a missed box reports 1e30 (so the reference's
                                        `1e30 > 1e30` descent into doubly-missed pairs happens), the binary tree walked as it
                                        is. Default (flag clear): the same walk with a CONSERVATIVE box test (boxes grown by
                                        more than the test's rounding error) -- same hits, fewer instructions; the library
                                        falls back to the exact test by itself when a camera or an injected ray lies outside
                                        the range that bound covers. Same images bit for bit; for bisecting and proofs. */
    WFPT_FLAG_NO_BINNING = 1u << 7,  /* keep the hit queue in thread order (a work item of the fused loop = 512 consecutive hits). This
                                        is the default in both RNG modes since the end of round 5 (rounds 4-5 binned contexts of at
                                        least 3/4 Mpixel in WFPT_RNG_PIXEL by default); the flag is accepted and wins over
                                        WFPT_FLAG_BINNING. */
    WFPT_FLAG_BINNING = 1u << 8,     /* WFPT_RNG_PIXEL, scenes in LDS: the class-binned loop -- every segment's hits stored sorted by cost
                                        class (the dominant primitive | lambertian | metal | dielectric), a work item = 512 hits of ONE
                                        class: 32.8 instead of 29.0 of 64 lanes per vector instruction, and level with the thread-ordered
                                        loop end to end at 1920x1080 (behind it on smaller slabs), hence opt-in. Same images bit for bit. With
                                        WFPT_RNG_DISPATCH wfpt_create refuses the flag (WFPT_ERR_INVALID_ARGUMENT): shade.wgsl:72 keys
                                        its RNG on the dispatch's thread index, i.e. on the order of the hit queue, which this loop
                                        gives up. (Round 4 carried that order through the binning -- thread indices in the records, a hit
                                        flag per ray, a rank table per wavefront -- measured it 5.8 % slower than the thread-ordered loop
                                        and round 5 removed it; so was the two-chain experiment, WFPT_FLAG_TWO_CHAINS, bit 9:
                                        profiles/r04_rejected_experiments.txt.) */
    /* bit 9 is retired (WFPT_FLAG_TWO_CHAINS, above) and stays unused */
    WFPT_FLAG_AOV = 1u << 10,        /* first-hit feature buffers (AOVs) for denoisers, see "AOVs" below: every sample wfpt_render* renders
                                        also traces its primary ray once more (aov_kernel) and adds the first hit's albedo, normal and
                                        depth to per-pixel sums. Without the flag nothing is allocated or launched. */
    WFPT_FLAG_DENOISE = 1u << 11,    /* the on-device denoiser, see "Denoiser" below: implies WFPT_FLAG_AOV, and every rendered batch also adds
                                        each sample's luminance and its square to per-pixel moments (accumulate_moments_kernel in place
                                        of accumulate_kernel). Without the flag nothing is allocated or launched. */
    WFPT_FLAG_ENVIRONMENT = 1u << 12 /* misses lit by an HDR environment map, see "Environment map" below: the miss queues carry the full
                                        direction (two more planes). Without a map set the context renders the gradient sky, bit for bit;
                                        without the flag nothing is allocated or launched. */,
    WFPT_FLAG_TEXTURES = 1u << 13    /* image textures on spheres and triangle meshes, see "Textures" below: up to WFPT_MAX_TEXTURES slots, a
                                        material bound to a slot multiplies the throughput of its hits by the texture as well as by its
                                        albedo. With nothing bound the context renders bit for bit as without the flag, and launches the
                                        same kernels. */,
    WFPT_FLAG_EMISSION = 1u << 14    /* emissive materials, see "Emission" below: a material given a non-zero emission colour lights the scene
                                        and ends the paths that hit it. With no emitter set the context renders bit for bit as without the
                                        flag, and launches the same kernels. */,
    WFPT_FLAG_NEE = 1u << 15         /* next-event estimation, see "Next-event estimation" below: every diffuse hit sends one shadow ray to a
                                        sampled point of an emitter. Needs WFPT_FLAG_EMISSION. With no emitter set the context renders bit
                                        for bit as without the flag, and launches the same kernels. */,
    WFPT_FLAG_ENV_NEE = 1u << 16     /* the environment map as one more light of the connect pass, sampled in proportion to its radiance, see
                                        "Environment next-event estimation" below. Needs WFPT_FLAG_ENVIRONMENT, WFPT_FLAG_EMISSION and
                                        WFPT_FLAG_NEE. With no map set (or a black one) the context renders bit for bit as without the
                                        flag, and launches the same kernels. */,
    WFPT_FLAG_MIS = 1u << 17         /* multiple importance sampling, see "Multiple importance sampling" below: the emitter hits of
                                        scattered rays and the shadow rays of the connect pass are both kept, weighed by the balance
                                        heuristic. Needs WFPT_FLAG_EMISSION and WFPT_FLAG_NEE, refused with WFPT_FLAG_ENV_NEE. With no emitter
                                        set the context renders bit for bit as without the flag, and launches the same kernels. */,
    WFPT_FLAG_ENV_MIS = 1u << 18,    /* multiple importance sampling between the environment map and the scatter, see "Environment multiple
                                        importance sampling" below: the map's connect samples and the misses of scattered rays are both
                                        kept, weighed by the balance heuristic, and so are the emitters' samples and hits. Needs
                                        WFPT_FLAG_ENVIRONMENT, WFPT_FLAG_EMISSION, WFPT_FLAG_NEE and WFPT_FLAG_ENV_NEE, refused with
                                        WFPT_FLAG_MIS. With no map set (or a black one) the context renders bit for bit as without the
                                        flag, and launches the same kernels. */
    WFPT_FLAG_NO_TILE_LISTS = 1u << 19 /* the first fused launch walks the tree for every tile instead of testing its tile's candidate list,
                                        see "Tile lists" below (A/B runs and tests; the results are the same bits either way) */,
    WFPT_FLAG_RETIRE = 1u << 20      /* path termination, see "Path termination" below: a path whose throughput is zero is retired at
                                        once, and from wavefront roulette_start on Russian roulette retires or re-weights the others.
                                        Refused with WFPT_FLAG_BINNING; combines freely with every other flag. */,
    WFPT_FLAG_ADAPTIVE = 1u << 21    /* adaptive sampling, see "Adaptive sampling" below: a per-pixel active mask that generate_rays and
                                        accumulate obey, per-pixel sample counts and luminance moments, and a device pass that turns the
                                        moments into the next mask. Refused with WFPT_FLAG_AOV, WFPT_FLAG_DENOISE and WFPT_FLAG_BINNING;
                                        combines freely with every other flag. Without the flag nothing is allocated or launched. */,
    WFPT_FLAG_LIGHT_POWER = 1u << 22 /* the connect pass selects its light in proportion to the lights' power (luminance times area), see
                                        "Light selection by power" below. Needs WFPT_FLAG_EMISSION and WFPT_FLAG_NEE, refused with
                                        WFPT_FLAG_ENV_NEE (and so WFPT_FLAG_ENV_MIS). With no emitter set, and with one light, the context
                                        renders bit for bit as without the flag. */,
    WFPT_FLAG_ANALYTIC_LIGHTS = 1u << 23 /* point, spot and directional lights for the connect pass, see "Analytic lights" below. Needs
                                        WFPT_FLAG_EMISSION and WFPT_FLAG_NEE, refused with WFPT_FLAG_ENV_NEE, WFPT_FLAG_ENV_MIS and
                                        WFPT_FLAG_LIGHT_POWER. With no analytic light set the context renders bit for bit as without the
                                        flag, and launches the same kernels. */
};

#define WFPT_INACTIVE_PIXEL 0xffffffffu

typedef struct wfpt_params {
    uint32_t width;          /* viewport (RenderParameters::viewport_size, parameters.rs:43-45) */
    uint32_t height;
    uint32_t max_pixels;     /* buffer capacity, the reference's max_window_size (path_tracer.rs:44); 0 = width*height */
    uint32_t max_wavefronts; /* path_tracer.rs:323: 50 */
    uint32_t miss_floor;     /* path_tracer.rs:332: loop exits before shading when misses < 128 */
    uint32_t rng_mode;       /* wfpt_rng_mode */
    uint32_t flags;          /* WFPT_FLAG_* */
    uint32_t tile_rank;      /* pixel-tile sharding: this context owns the 8-pixel-high bands k with */
    uint32_t tile_world;     /*   k % tile_world == tile_rank; 0 or 1 = whole image */
    int32_t device;          /* HIP device ordinal */
    uint32_t batch;          /* samples kept in flight per launch by wfpt_render (1..128, 1..64 for the stage-by-stage
                                loop; 0 = 16; larger values are clamped). Results are bit-identical for every value:
                                samples are independent and accumulate in order. */
} wfpt_params;

typedef struct wfpt_ctx wfpt_ctx;

/* ------------------------------------------------------------------ host-side data model helpers
 * (no GPU needed). They restate wavefront_common so a host without the Rust crate can build inputs. */

/* scene.rs:12-46: 5 spheres, 5 materials; arrays need capacity 5. Returns the count. */
uint32_t wfpt_scene_new(wfpt_sphere *spheres, wfpt_material *materials);
/* scene.rs:48-107 with a SEEDED generator (the reference's thread_rng is unseeded): PCG32 stream 54,
 * f32 = top 24 bits * 2^-24, same distributions and draw order. Returns the count (<= 488), or 0 if
 * capacity is too small. */
uint32_t wfpt_scene_book_one_final(uint64_t seed, wfpt_sphere *spheres, wfpt_material *materials, uint32_t capacity);
/* bvh.rs:147-210 (4096-bin SAH): reorders `spheres` in place, writes at most 2*n nodes. */
int wfpt_build_bvh(wfpt_sphere *spheres, uint32_t n_spheres, wfpt_bvh_node *nodes, uint32_t node_capacity,
                   uint32_t *n_nodes);
/* Build extension: the same builder over triangles (bin key = centroid v0 + (e1 + e2)/3) with a caller-chosen
 * number of bins per axis (bvh.rs:4's 4096 is O(10^10) work for a million primitives). Reorders in place. */
int wfpt_build_bvh_triangles(wfpt_triangle *triangles, uint32_t n_triangles, wfpt_bvh_node *nodes,
                             uint32_t node_capacity, uint32_t *n_nodes, uint32_t n_bins);
/* Build extension: the same two builders ON THE DEVICE (csrc/wfpt_bvh_build.hip). Same
 * arguments, same results byte for byte -- node array in bvh.rs's depth-first numbering, primitives reordered in
 * place -- so either can feed wfpt_create / wfpt_create_mesh. `device` is the HIP device ordinal; `device_ms`
 * (may be NULL) receives the time between the first and the last build kernel (host<->device copies of the
 * inputs / outputs excluded). WFPT_ERR_NO_DEVICE without a GPU: there is no silent fall back to the host builder. */
int wfpt_build_bvh_device(wfpt_sphere *spheres, uint32_t n_spheres, wfpt_bvh_node *nodes, uint32_t node_capacity,
                          uint32_t *n_nodes, int device, float *device_ms);
int wfpt_build_bvh_triangles_device(wfpt_triangle *triangles, uint32_t n_triangles, wfpt_bvh_node *nodes,
                                    uint32_t node_capacity, uint32_t *n_nodes, uint32_t n_bins, int device,
                                    float *device_ms);
/* Build extension (README.md:25 "start loading in obj files"): reads the `v` and `f` records of a
 * Wavefront OBJ file into wfpt_triangle (v0, e1 = v1 - v0, e2 = v2 - v0), fan-triangulating polygons; `f` entries may
 * be `i`, `i/t`, `i//n` or `i/t/n`, 1-based or negative (relative). Every triangle gets `material_idx` /
 * `material_type`. With triangles == NULL it only counts. Returns WFPT_OK and the count in *n_triangles;
 * WFPT_ERR_INVALID_ARGUMENT for an unreadable file, a bad index or too small a capacity. */
int wfpt_load_obj(const char *path, wfpt_triangle *triangles, uint32_t capacity, uint32_t *n_triangles,
                  uint32_t material_idx, uint32_t material_type);
/* wfpt_load_obj plus texture coordinates (WFPT_FLAG_TEXTURES): also reads `vt u v [w]` records, and writes triangle i of the file (in file
 * order, after fan triangulation) with _pad = i and row i of uv6 (6 floats: u0 v0 u1 v1 u2 v2) from its corners' `t` indices (1-based or
 * negative); corners without one get (0, 0). uv6 holds `capacity` rows; both NULL only counts. */
int wfpt_load_obj_uv(const char *path, wfpt_triangle *triangles, float *uv6, uint32_t capacity, uint32_t *n_triangles,
                     uint32_t material_idx, uint32_t material_type);
/* BASELINE config 5: seeded triangle soup -- centres U[-10,10]^3, edges U[-0.05,0.05]^3, material i % 3 over
 * {Lambertian 0.7, Metal 0.8 fuzz 0.1, Dielectric 1.5}. Writes n triangles and 3 materials; returns 3. */
uint32_t wfpt_scene_random_mesh(uint64_t seed, uint32_t n_triangles, wfpt_triangle *triangles, wfpt_material *materials);
/* camera.rs:11-24 */
void wfpt_camera_new(const float look_from[3], const float look_at[3], float *pitch, float *yaw);
/* camera.rs:41-69: world-from-camera, 16 floats column-major (columns right, up, dir, position) */
void wfpt_view_transform(const float position[3], float pitch, float yaw, float view[16]);
/* projection_matrix.rs:21-37: inverse projection, 16 floats column-major */
void wfpt_p_inv(float vfov_rad, float aspect_ratio, float z_near, float z_far, float p_inv[16]);
/* camera_controller.rs:173-185 */
void wfpt_gpu_camera_new(const float position[3], float pitch, float yaw, float defocus_angle_rad,
                         float focus_distance, wfpt_gpu_camera *out);
/* f32::to_radians */
float wfpt_to_radians(float degrees);
/* camera_controller.rs:125-158 (CameraController::update_camera): moves the camera by the pressed-key amounts
 * {forward, backward, right, left, up, down} and the pending mouse rotation {horizontal, vertical} over dt seconds,
 * clamps the pitch to +-(pi - 0.001), and zeroes `rotate` like the reference does. */
void wfpt_camera_controller_update(float position[3], float *pitch, float *yaw, const float amounts[6],
                                   float rotate[2], float speed, float sensitivity, float dt);
/* path_tracer.rs:282-289. The reference panics for x <= 64; this returns (1,1) there. */
void wfpt_workgroup_size_64(uint32_t x, uint32_t *gx, uint32_t *gy);
/* kernel.rs:32: shader basename -> stage; -1 if unknown */
int wfpt_stage_from_name(const char *name);
const char *wfpt_stage_name(int stage);

/* ------------------------------------------------------------------ context: PathTracer::new (path_tracer.rs:43-217) */

int wfpt_device_count(void);
/* Copies every input; no pointer is retained. Returns NULL on failure (wfpt_last_error(NULL)). */
wfpt_ctx *wfpt_create(const wfpt_params *params,
                      const wfpt_sphere *spheres, uint32_t n_spheres,
                      const wfpt_material *materials, uint32_t n_materials,
                      const wfpt_bvh_node *nodes, uint32_t n_nodes,
                      const wfpt_gpu_camera *camera, const float inv_proj[16], const float view[16]);
/* Same context over a triangle mesh (build extension). Scenes whose BVH does not fit a CU's LDS are traversed
 * from HBM / Infinity Cache by a second extend variant. */
wfpt_ctx *wfpt_create_mesh(const wfpt_params *params,
                           const wfpt_triangle *triangles, uint32_t n_triangles,
                           const wfpt_material *materials, uint32_t n_materials,
                           const wfpt_bvh_node *nodes, uint32_t n_nodes,
                           const wfpt_gpu_camera *camera, const float inv_proj[16], const float view[16]);
void wfpt_destroy(wfpt_ctx *ctx);
const char *wfpt_last_error(const wfpt_ctx *ctx);

/* Dynamic scenes (the reference builds its scene once, in PathTracer::new, path_tracer.rs:117-128):
 * replaces the scene of a live context. `spheres` / `triangles` are reordered in place by the BVH build, as
 * BVHTree::build_bvh_tree does (bvh.rs:182); the BVH is rebuilt on the context's device by wfpt_build_bvh_device /
 * wfpt_build_bvh_triangles_device (byte-identical to bvh.rs:147-210; n_bins = 0 means 32), the traversal's derived data
 * re-derived, and the accumulation and the frame counter reset like update_buffers does for a parameter change
 * (path_tracer.rs:240-277). The primitive count and kind may change; queues and images keep their size. The context is
 * unchanged if the arguments are refused; a HIP failure half way leaves it without a scene (only wfpt_destroy is safe). */
int wfpt_update_scene(wfpt_ctx *ctx, wfpt_sphere *spheres, uint32_t n_spheres, const wfpt_material *materials, uint32_t n_materials);
int wfpt_update_scene_mesh(wfpt_ctx *ctx, wfpt_triangle *triangles, uint32_t n_triangles, const wfpt_material *materials,
                           uint32_t n_materials, uint32_t n_bins);

/* Image chunking on one GPU (the reference's to-do "split rendering of image into chunks so that the buffers aren't so
 * big", README.md:20): renders n_samples of the whole frame as `chunks` band-interleaved slabs, one context after the
 * other (chunk k holds the 8-row bands j with j % chunks == k, so every device buffer is sized for 1/chunks of the
 * frame), and writes the accumulated frame (3 floats per pixel, row-major, width * height pixels) to host memory at
 * `rgb`. params->tile_rank / tile_world / max_pixels are ignored. With chunks > 1 params->rng_mode must be
 * WFPT_RNG_PIXEL (the dispatch-keyed RNG of shade.wgsl:72 depends on a ray's queue position, hence on the cut); the
 * frame is then bit-identical to the unchunked WFPT_RNG_PIXEL render as long as the loop-exit test of path_tracer.rs:332
 * (`misses < miss_floor`), which every chunk applies to its OWN miss count, fires in no chunk before it would for the
 * whole frame -- with miss_floor = 0 (wavefront limit only) it never does and the image is independent of the cut.
 * The same holds for contexts sharded with tile_rank / tile_world across GPUs. Blocking. */
int wfpt_render_chunked(const wfpt_params *params,
                        const wfpt_sphere *spheres, uint32_t n_spheres,
                        const wfpt_material *materials, uint32_t n_materials,
                        const wfpt_bvh_node *nodes, uint32_t n_nodes,
                        const wfpt_gpu_camera *camera, const float inv_proj[16], const float view[16],
                        uint32_t n_samples, uint32_t chunks, float *rgb);
int wfpt_render_chunked_mesh(const wfpt_params *params,
                             const wfpt_triangle *triangles, uint32_t n_triangles,
                             const wfpt_material *materials, uint32_t n_materials,
                             const wfpt_bvh_node *nodes, uint32_t n_nodes,
                             const wfpt_gpu_camera *camera, const float inv_proj[16], const float view[16],
                             uint32_t n_samples, uint32_t chunks, float *rgb);

/* frame_buffer.queue_for_gpu (path_tracer.rs:296-297, 366-367). The uniform set here is what the STAGE API
 * (wfpt_kernel_run) reads. The device-resident loop (wfpt_render_sample / wfpt_render) owns the frame uniform like
 * PathTracer::run does (path_tracer.rs:293-297): its next call overwrites it with {width, height,
 * wfpt_frame() + 1, sample_number 0}, whatever was set here. */
int wfpt_set_frame(wfpt_ctx *ctx, const wfpt_frame_buffer *frame);
/* update_buffers (path_tracer.rs:240-277): new camera / matrices / viewport; zeroes the accumulated image
 * and resets progress exactly as the reference does on any parameter change. */
int wfpt_update_render_parameters(wfpt_ctx *ctx, uint32_t width, uint32_t height, const wfpt_gpu_camera *camera,
                                  const float inv_proj[16], const float view[16]);
/* counter_buffer protocol (path_tracer.rs:313-316, 335-336, 352; extend.wgsl:41):
 * [0] miss count, [1] hit count, [2] rays in for extend / extension rays out of shade, [3..15] unused. */
int wfpt_set_counters(wfpt_ctx *ctx, const uint32_t counters[16]);
int wfpt_read_counters(wfpt_ctx *ctx, uint32_t counters[16]); /* blocking, like wgpu_state.rs:132-147 */
int wfpt_reset_image(wfpt_ctx *ctx);       /* image <- 1.0 (path_tracer.rs:305-306) */
int wfpt_reset_accumulated(wfpt_ctx *ctx); /* accumulated <- 0 (path_tracer.rs:248-250) */
/* RenderProgress::reset (parameters.rs:92-95) + the accumulation clear above: the next sample is frame 1 again. What
 * update_buffers does after a change (path_tracer.rs:248-250, 276) without re-uploading camera or matrices. */
int wfpt_reset_progress(wfpt_ctx *ctx);
int wfpt_clear_ray_queues(wfpt_ctx *ctx);  /* path_tracer.rs:309-310 */
/* copy_buffer_to_buffer(extension_ray_buffer -> ray_buffer) (path_tracer.rs:348, wgpu_state.rs:115-130)
 * done as a pointer swap. */
int wfpt_swap_ray_queues(wfpt_ctx *ctx);

/* Kernel::run((gx, gy)) (kernel.rs:107-140): gx*gy workgroups of 64 threads, thread index linearised as
 * in the shaders (workgroup_index*64 + local_index). Semantics per stage follow the WGSL entry points:
 *   generate_rays: width = 8*gx, height = 8*gy, one ray per thread (generate_rays.wgsl:42-91)
 *   extend:        threads idx < counters[2] trace; counters[1] += hits, counters[0] += misses (extend.wgsl:47-70)
 *   shade:         threads idx < counters[1]; counters[2] += rays emitted (shade.wgsl:56-156)
 *   miss_kernel:   threads idx < counters[0] (miss_kernel.wgsl:13-38)
 *   accumulate:    threads idx < pixel count (accumulate.wgsl:4-17; the reference has no guard)
 * counters[0] and [1] must be zero when extend runs and counters[2] zero when shade runs, as the
 * reference's host guarantees (path_tracer.rs:335-336, 352). */
int wfpt_kernel_run(wfpt_ctx *ctx, int stage, uint32_t gx, uint32_t gy);
/* Kernel::get_timing (kernel.rs:142-146, query_gpu.rs:26-43): blocks, returns the running mean (us) of
 * the last <= 10 timed dispatches of that stage; 0 if it never ran. */
float wfpt_kernel_timing_us(wfpt_ctx *ctx, int stage);

/* wfpt_render_sample: PathTracer::run for one sample (path_tracer.rs:291-368) with the whole wavefront loop resident on the
 * device: frame += 1, image <- 1, generate, up to max_wavefronts x (extend, shade, miss) with the
 * `misses < miss_floor` exit evaluated on the device, accumulate. No host synchronisation. Sizes that
 * are not multiples of 8 use true-size semantics: out-of-image lanes emit inactive rays. */
/* Which loop wfpt_render enqueues for this context, as decided at wfpt_create / wfpt_update_scene from the flags, the RNG mode, the size
 * of the slab and the scene (hosts and benchmarks label their figures with this instead of re-deriving the library's gates):
 *   WFPT_LOOP_STAGES        the stage kernels one by one (WFPT_FLAG_UNFUSED / WFPT_FLAG_SPLIT_SHADE, or more than 65535 queue segments)
 *   WFPT_LOOP_FUSED         one fused bounce launch per wavefront, hit queue in the reference's thread order (bounce_kernel)
 *   WFPT_LOOP_FUSED_BINNED  the same with the hit queue binned by cost class (WFPT_RNG_PIXEL, scenes in LDS; bounce_binned_kernel)
 *   WFPT_LOOP_REFILL        scenes beyond LDS: four-wide traversal with dynamic lane refill (refill_kernel)
 * Returns the kind, or a negative status. */
typedef enum wfpt_loop_kind { WFPT_LOOP_STAGES = 0, WFPT_LOOP_FUSED = 1, WFPT_LOOP_FUSED_BINNED = 2, WFPT_LOOP_REFILL = 3 } wfpt_loop_kind;
int wfpt_loop_kind_of(const wfpt_ctx *ctx);
int wfpt_render_sample(wfpt_ctx *ctx);
int wfpt_render(wfpt_ctx *ctx, uint32_t n_samples);
int wfpt_synchronize(wfpt_ctx *ctx);
uint32_t wfpt_frame(const wfpt_ctx *ctx);               /* RenderProgress.frame */
/* RNG frame offset of the device-resident loop (wfpt_render*, default 0): the frame uniform it writes becomes
 * {width, height, wfpt_frame() + 1 + offset, 0} (uint32 wrap-around), so the samples after a reset continue the random streams of
 * earlier epochs instead of replaying frames 1, 2, ... (a temporal blend of repeated streams gains nothing). wfpt_frame()
 * keeps its meaning. Setting it takes effect at the next rendered batch; no reset, camera change or scene change clears it. The stage
 * API (wfpt_set_frame / wfpt_kernel_run, PathTracer.run) sets the frame itself and ignores the offset, as does wfpt_render_chunked*. */
int wfpt_set_frame_offset(wfpt_ctx *ctx, uint32_t offset);
uint32_t wfpt_frame_offset(const wfpt_ctx *ctx);
uint32_t wfpt_accumulated_samples(const wfpt_ctx *ctx); /* RenderProgress.accumulated_samples */
float wfpt_progress(const wfpt_ctx *ctx, uint32_t spp); /* PathTracer::progress (path_tracer.rs:219-221) */
/* Same loop with hipEvent pairs around every stage launch; adds the elapsed milliseconds per stage
 * into stage_ms[WFPT_STAGE_COUNT] (+= , caller zeroes) and counts launches in stage_launches (may be
 * NULL). Blocks until the sample is done. */
int wfpt_render_sample_timed(wfpt_ctx *ctx, float *stage_ms, uint32_t *stage_launches);
/* n_samples with the same batching as wfpt_render, timed per launch the same way. */
int wfpt_render_timed(wfpt_ctx *ctx, uint32_t n_samples, float *stage_ms, uint32_t *stage_launches);

/* ------------------------------------------------------------------ AOVs (WFPT_FLAG_AOV): first-hit feature buffers
 * On a context created with WFPT_FLAG_AOV every sample rendered by wfpt_render, wfpt_render_sample, wfpt_render_timed and
 * wfpt_render_sample_timed -- whatever the loop (fused, stage kernels, split shade, binned, refill), primitive kind, RNG mode or
 * sharding -- also adds to per-pixel AOV sums. Sample k's primary ray is exactly the ray its beauty pass traces (same primary_ray,
 * frame number, sample_number and true-size padding), traced with the same traversal the first extend would use, so t and the
 * primitive are the first extend's, bit for bit. Per sample and pixel:
 *   hit:  albedo = the material albedo (rgb) of the primitive hit; normal = the normal shade scatters about (spheres:
 *         normalize3(p - centre), p = o + t d as shade computes it; triangles: the stored normalize(cross(e1, e2))); depth = t (primary
 *         directions are unit length, so t is the distance); hits += 1.
 *   miss: albedo = miss_kernel's sky colour for the direction (a = 0.5 (dy + 1), (1 - a) * 1 + a * (0.5, 0.7, 1.0)); normal = 0.
 * Sums are added in ascending sample order, so every batch size and loop kind gives the same bits. Read-back resolves them with one
 * IEEE f32 division each; n = wfpt_accumulated_samples:
 *   WFPT_AOV_ALBEDO       sum / n                                3 floats per pixel
 *   WFPT_AOV_NORMAL       sum / n (not renormalised)             3 floats per pixel
 *   WFPT_AOV_DEPTH        sum of t / hits, 0 where hits == 0     1 float per pixel
 *   WFPT_AOV_COVERAGE     hits / n                               1 float per pixel
 *   WFPT_AOV_PRIM_ID      primitive of the first sample since the last reset, 0xffffffff on a miss    1 u32 per pixel
 *   WFPT_AOV_MATERIAL_ID  that sample's material_idx, 0xffffffff on a miss                           1 u32 per pixel
 * With n == 0 the float AOVs read 0 and the ids 0xffffffff. Pixels are row-major like wfpt_read_accumulated; a sharded context holds
 * its own bands. Whatever zeroes `accumulated` (wfpt_reset_accumulated, wfpt_reset_progress, a camera / size / scene change) zeroes the
 * sums too. Out of scope: the stage API (wfpt_kernel_run), wfpt_render_chunked*, a gather of AOVs, and specular chains (only the first
 * hit counts, as stored, for metal and dielectric too). On a context without the flag, or with an unknown `which`, these functions
 * return WFPT_ERR_INVALID_ARGUMENT. */
typedef enum wfpt_aov {
    WFPT_AOV_ALBEDO = 0,
    WFPT_AOV_NORMAL = 1,
    WFPT_AOV_DEPTH = 2,
    WFPT_AOV_COVERAGE = 3,
    WFPT_AOV_PRIM_ID = 4,
    WFPT_AOV_MATERIAL_ID = 5,
    WFPT_AOV_COUNT = 6
} wfpt_aov;
/* components per pixel of an AOV (3 or 1), 0 for an unknown one */
int wfpt_aov_channels(int which);
/* the resolved AOV, wfpt_aov_channels(which) * n_pixels elements of 4 bytes (float, or uint32_t for the ids); n_elems may be less (blocking) */
int wfpt_read_aov(wfpt_ctx *ctx, int which, void *out, size_t n_elems);
/* the same values resolved on the device (aov_resolve_kernel, the same bits as wfpt_read_aov) into a caller's device buffer of n_bytes
 * (at most the whole AOV); ordered on the context's stream, returns when they are written */
int wfpt_copy_aov_to_device(wfpt_ctx *ctx, int which, void *device_ptr, size_t n_bytes);
/* time of the AOV launches of every timed render since wfpt_create (hipEvent pairs, not part of stage_ms) and their count; either
 * pointer may be NULL */
int wfpt_aov_timing_ms(wfpt_ctx *ctx, float *ms_total, uint32_t *launches);

/* ------------------------------------------------------------------ Denoiser (WFPT_FLAG_DENOISE): edge-avoiding a-trous wavelet filter
 * A context created with WFPT_FLAG_DENOISE keeps the AOVs above (the flag implies WFPT_FLAG_AOV: wfpt_read_aov and wfpt_aov_timing_ms work
 * on it) and two more per-pixel sums over the samples k that wfpt_render* adds to `accumulated`: S1 = sum of L_k and S2 = sum of L_k * L_k,
 * L_k = (0.2126 r + 0.7152 g) + 0.0722 b of the value sample k adds, in ascending sample order (the same bits for every batch size and
 * loop kind). They are reset with the AOV sums, and out of scope in the same places (stage API, wfpt_render_chunked*).
 * wfpt_read_variance resolves them, n = wfpt_accumulated_samples, with one IEEE f32 division each in this order:
 *   mu = S1 / n;  v = max(0, S2 / n - mu * mu) / n        the variance of the n-sample mean's luminance, 0 where n == 0
 * wfpt_denoise filters the mean colour c = accumulated / n with the spatial part of SVGF (Schied et al. 2017) on Dammertz et al. 2010:
 *   prepare     guides per pixel from the read-back values: the normalised normal, depth, albedo, the depth gradient (per axis the
 *               smaller step to an existing neighbour) and v; for n < 4, v is the population variance of L(c) over the 7x7 window
 *   pass i      (i < iterations) a 5x5 a-trous tap set at step 2^i, taps outside the image skipped; the weight of tap q for pixel p is
 *               h(dx) h(dy) exp(-|L_p - L_q| / (sigma_luminance sqrt(g3(v)_p) + 1e-10) - |z_p - z_q| / (sigma_depth |grad z_p| 2^i |(dx, dy)| + 1e-3)
 *                                 - |A_p - A_q|^2 / sigma_albedo^2) * max(0, dot(N_p, N_q))^sigma_normal
 *               (the normal term is 1 where both normals are 0 and 0 where one is), h = (1, 4, 6, 4, 1) / 16, g3 = 3x3 binomial blur of
 *               v; c' = sum w c_q / sum w, v' = sum w^2 v_q / (sum w)^2
 * The result is the last pass's c, a mean colour (not a sum): 3 floats per pixel, stride 12, row-major. No atomics and a fixed order
 * of every sum: repeated calls, every batch size and every loop kind give the same bits. A call reads the sums and writes only its own
 * buffers (allocated on the first call): the next render continues as if it had not happened. With n == 0 the outputs are 0.
 * WFPT_ERR_INVALID_ARGUMENT without the flag, for a bad parameter or too large a size; WFPT_ERR_UNSUPPORTED from the two denoise calls on
 * a band-sharded context (tile_world > 1: the filter needs the other ranks' bands). */
typedef struct wfpt_denoise_params {
    uint32_t iterations;      /* a-trous passes, 0..8; 0 = c = accumulated / n unfiltered */
    float sigma_luminance;    /* each sigma > 0 and finite */
    float sigma_normal;
    float sigma_depth;
    float sigma_albedo;
    uint32_t _reserved[3];    /* must be 0 */
} wfpt_denoise_params;
WFPT_LAYOUT_ASSERT(sizeof(wfpt_denoise_params) == 32 && offsetof(wfpt_denoise_params, sigma_luminance) == 4 &&
                       offsetof(wfpt_denoise_params, sigma_normal) == 8 && offsetof(wfpt_denoise_params, sigma_depth) == 12 &&
                       offsetof(wfpt_denoise_params, sigma_albedo) == 16 && offsetof(wfpt_denoise_params, _reserved) == 20,
                   "wfpt_denoise_params: 32 bytes");
/* iterations 5, sigma_luminance 4, sigma_normal 128, sigma_depth 1 (SVGF's), sigma_albedo 0.5 (tuned: DESIGN.md 9c); _reserved zeroed */
void wfpt_denoise_params_default(wfpt_denoise_params *p);
/* the denoised mean colour, 3 * n_pixels floats at most (blocking) */
int wfpt_denoise(wfpt_ctx *ctx, const wfpt_denoise_params *p, float *rgb, size_t n_floats);
/* the same bits written into a caller's device buffer of n_bytes (at most 12 * n_pixels); returns when they are written */
int wfpt_denoise_to_device(wfpt_ctx *ctx, const wfpt_denoise_params *p, void *device_ptr, size_t n_bytes);
/* the per-pixel variance v above, n_pixels floats at most (blocking); a sharded context holds its own bands */
int wfpt_read_variance(wfpt_ctx *ctx, float *out, size_t n_elems);
/* time of the last denoise call's launches (a hipEvent pair around them) and the number of calls since wfpt_create; either pointer may
 * be NULL */
int wfpt_denoise_timing_ms(wfpt_ctx *ctx, float *ms_last, uint32_t *calls);

/* ------------------------------------------------------------------ Temporal denoiser (WFPT_FLAG_DENOISE): reprojected history
 * wfpt_denoise_temporal is wfpt_denoise with temporal_prepare_kernel in place of prepare: it carries the samples of earlier camera poses
 * into the current one (the temporal part of SVGF, Schied et al. 2017), then runs the same a-trous passes. Any WFPT_FLAG_DENOISE context.
 * Epochs: an epoch is the span between two resets of the accumulation (every camera change, wfpt_reset_progress, wfpt_reset_accumulated).
 * The context keeps two history slots, live and sealed (allocated by the first call): per pixel the blended colour c and history length L,
 * the per-sample moments (m1, m2), the guides (normalised normal and depth as prepare makes them, coverage, material id), plus the epoch
 * and the camera (position, view, inv_proj, viewport) they were written under. A call first seals: when the live slot was written in
 * another epoch, live and sealed swap. Then, n = wfpt_accumulated_samples, S / S1 / S2 the sums, per pixel p = (x, y):
 *   ray         the centre ray of primary_ray (jitter (0, 0), no lens) from the camera position o; X = (o + z d, 1) where coverage > 0
 *               (a hit), else the direction (d, 0)
 *   project     q = M X, M = inverse(inv_proj_s) inverse(view_s) of the sealed camera (double on the host, rounded to f32); q.w <= 0: no
 *               history; else x' = ((q.x / q.w + 1) 0.5) W, y' = (1 - (q.y / q.w + 1) 0.5) H (pixel centres at integers),
 *               z' = |X - o_s| for hits (0 for misses)
 *   taps        (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1), x0 = floor(x'), bilinear weights; a tap inside the image is accepted when
 *               for a hit: its coverage > 0, the same material id, |z_t - z'| <= depth_tolerance z' and dot(N_p, N_t) >= normal_cos;
 *               for a miss: its coverage is 0. Wsum = sum of the accepted weights in tap order
 *   no history (no projection, Wsum < 0.01 or history_cap == 0): prepare's outputs, bit for bit; the slot gets c = S / n, L = n and the
 *               moments (S1 / n, S2 / n)
 *   history     H = sum w value_t / Wsum over the accepted taps for c, m1, m2 and L; h = min(H_L, history_cap), L = h + n;
 *               c = (h H_c + S) / L, m1 = (h H_m1 + S1) / L, m2 = (h H_m2 + S2) / L, v = max(0, m2 - m1 m1) / L (for L < 4 prepare's
 *               7x7 variance times n / L instead)
 * (c, v) is pass 0's input. Each call is a pure function of the sealed slot, the sums and the parameters: repeated calls give the same
 * bits, and it changes nothing a render, wfpt_denoise or the AOV read-backs see. The next call has no history after wfpt_reset_history,
 * wfpt_update_scene* (there are no object motion vectors), a viewport size change, and on the first call. With n == 0 the call writes
 * zeros and leaves both slots untouched. WFPT_ERR_INVALID_ARGUMENT without the flag, for a bad parameter or too large a size;
 * WFPT_ERR_UNSUPPORTED on a band-sharded context. Out of scope: object motion, the stage API, wfpt_render_chunked*. */
typedef struct wfpt_temporal_params {
    wfpt_denoise_params spatial;  /* the a-trous passes, checked as wfpt_denoise checks them */
    float history_cap;            /* >= 0, finite: samples of history a pixel may carry; 0 = none (the call equals wfpt_denoise) */
    float depth_tolerance;        /* > 0, finite, relative */
    float normal_cos;             /* in [-1, 1] */
    uint32_t _reserved[5];        /* must be 0 */
} wfpt_temporal_params;
WFPT_LAYOUT_ASSERT(sizeof(wfpt_temporal_params) == 64 && offsetof(wfpt_temporal_params, history_cap) == 32 &&
                       offsetof(wfpt_temporal_params, depth_tolerance) == 36 && offsetof(wfpt_temporal_params, normal_cos) == 40 &&
                       offsetof(wfpt_temporal_params, _reserved) == 44,
                   "wfpt_temporal_params: 64 bytes");
/* spatial = wfpt_denoise_params_default, history_cap 32 (chosen by a sweep: DESIGN.md 9d), depth_tolerance 0.05, normal_cos 0.9 */
void wfpt_temporal_params_default(wfpt_temporal_params *p);
/* the denoised mean colour, 3 * n_pixels floats at most (blocking) */
int wfpt_denoise_temporal(wfpt_ctx *ctx, const wfpt_temporal_params *p, float *rgb, size_t n_floats);
/* the same bits written into a caller's device buffer of n_bytes (at most 12 * n_pixels); returns when they are written */
int wfpt_denoise_temporal_to_device(wfpt_ctx *ctx, const wfpt_temporal_params *p, void *device_ptr, size_t n_bytes);
/* per-pixel state of the last temporal call (channels per pixel in the comment) */
typedef enum wfpt_temporal_out {
    WFPT_TEMPORAL_COLOR = 0,   /* 3: c before the passes */
    WFPT_TEMPORAL_MOMENTS = 1, /* 2: (m1, m2) */
    WFPT_TEMPORAL_LENGTH = 2,  /* 1: L */
    WFPT_TEMPORAL_MOTION = 3   /* 3: (x', y', z'); (-1e30, -1e30, 0) where there was no projection */
} wfpt_temporal_out;
/* channels * n_pixels floats at most (blocking); WFPT_ERR_INVALID_ARGUMENT when no call has run since the history was dropped */
int wfpt_read_temporal(wfpt_ctx *ctx, int which, float *out, size_t n_elems);
/* drops both history slots: the next temporal call has no history */
int wfpt_reset_history(wfpt_ctx *ctx);
/* time of the last temporal call's launches and the number of calls since wfpt_create; either pointer may be NULL */
int wfpt_temporal_timing_ms(wfpt_ctx *ctx, float *ms_last, uint32_t *calls);

/* ------------------------------------------------------------------ Environment map (WFPT_FLAG_ENVIRONMENT): image-based lighting of misses
 * With a map set, every miss that miss_kernel would colour with the gradient sky (image[pixel] *= sky(d)) is multiplied by the map's value
 * in its direction d instead, per channel: thr.r * c.r, thr.g * c.g, thr.b * c.b. The lookup (wfpt_device_math.h env_lookup), IEEE f32
 * add / sub / mul / div / sqrt, comparisons and floor only, no fma:
 *   n = normalize3(d);  phi = atan2_(n.x, -n.z);  theta = atan2_(sqrt(n.x n.x + n.z n.z), n.y)
 *   u = phi / 2pi + (0.5 + rotation), u <- u - floor(u);  v = theta / pi      (row 0 of the map = +y, column w/2 faces -z)
 *   x = u w - 0.5, x0 = floor(x), fx = x - x0 (the same for y); columns wrap modulo w, rows clamp to [0, h - 1]
 *   c = (((t00 (1-fx)(1-fy) + t10 fx (1-fy)) + t01 (1-fx) fy) + t11 fx fy) * intensity
 * atan2_ is the library's own (Cephes atanf with a fixed operation order, within 2 ulp; wfpt_selftest_math op 8). A context with
 * WFPT_FLAG_AOV adds the map's value of the primary direction to the albedo sum of a primary miss, in place of the sky colour.
 * wfpt_set_environment and wfpt_clear_environment act like a scene update: the accumulation and the frame counter restart, the temporal
 * history is dropped, and so are the captured graphs. wfpt_update_scene* and viewport changes keep the map. A refused call leaves the
 * context as it was, its map included. WFPT_ERR_INVALID_ARGUMENT without the flag and for a bad size, texel or parameter; WFPT_ERR_UNSUPPORTED
 * while wfpt_loop_kind_of reports WFPT_LOOP_FUSED_BINNED (the opt-in class-binned loop measures level with the default one and is not
 * extended: WFPT_FLAG_BINNING contexts keep the gradient sky). Out of scope: wfpt_render_chunked* (the flag is masked off there). Importance
 * sampling of the map by shadow rays: WFPT_FLAG_ENV_NEE ("Environment next-event estimation" below). */
typedef struct wfpt_environment_params {
    float intensity;        /* >= 0, finite: multiplies every texel */
    float rotation;         /* in [0, 1): turns added to u (the map turns about +y) */
    uint32_t _reserved[6];  /* must be 0 */
} wfpt_environment_params;
WFPT_LAYOUT_ASSERT(sizeof(wfpt_environment_params) == 32 && offsetof(wfpt_environment_params, rotation) == 4 &&
                       offsetof(wfpt_environment_params, _reserved) == 8,
                   "wfpt_environment_params: 32 bytes");
/* intensity 1, rotation 0, _reserved zeroed */
void wfpt_environment_params_default(wfpt_environment_params *p);
/* rgb: h rows of w texels, 3 floats each (row-major, row 0 = up), finite and >= 0; 1 <= w <= 16384, 1 <= h <= 8192. Stored on the device
 * as float4 texels; replaces any earlier map. p may be NULL (the defaults). Blocking. */
int wfpt_set_environment(wfpt_ctx *ctx, const float *rgb, uint32_t w, uint32_t h, const wfpt_environment_params *p);
/* back to the gradient sky */
int wfpt_clear_environment(wfpt_ctx *ctx);
/* the lookup above on the device for n caller directions (xyz, 3 floats each) into rgb_out (3 floats each); WFPT_ERR_INVALID_ARGUMENT when
 * no map is set. Blocking. */
int wfpt_sample_environment(wfpt_ctx *ctx, const float *dirs, size_t n, float *rgb_out);

/* ------------------------------------------------------------------ Textures (WFPT_FLAG_TEXTURES): image textures on surfaces
 * A context created with WFPT_FLAG_TEXTURES holds WFPT_MAX_TEXTURES texture slots, and a material can be bound to a slot. Every hit on a
 * primitive whose material is bound is shaded, for every material type, with
 *   thr <- (thr * tex) * albedo      per channel, two IEEE f32 multiplies (unbound materials: thr <- thr * albedo, as without the flag)
 * where tex is the texture's value at the hit's UV (wfpt_device_math.h, IEEE f32 operations only, no fma):
 *   spheres:   n = normalize3(p - centre);  u = atan2_(-n.z, n.x) / 2pi + 0.5;  v = atan2_(sqrt(n.x n.x + n.z n.z), -n.y) / pi
 *   triangles: w = p - v0; d00 = e1.e1, d01 = e1.e2, d11 = e2.e2, d20 = w.e1, d21 = w.e2; den = d00 d11 - d01 d01;
 *              b1 = b2 = 0 unless den > 0, else b1 = (d11 d20 - d01 d21) / den, b2 = (d00 d21 - d01 d20) / den (one reciprocal, two products);
 *              b0 = (1 - b1) - b2;  uv = (uv0 b0 + uv1 b1) + uv2 b2 with the corner UVs of the triangle's row (_pad) of the UV table,
 *              (0, 0) at every corner when no table is set
 *   lookup:    u' = u scale.u + offset.u, u' <- u' - floor(u') (the same for v'): both axes repeat; row 0 of the image is the top (v' = 1)
 *              bilinear: x = u' w - 0.5, y = (1 - v') h - 0.5, texel centres at half-integers, columns wrap modulo w and rows modulo h,
 *                        ((t00 w00 + t10 w10) + t01 w01) + t11 w11 with w00 = (1-fx)(1-fy), w10 = fx (1-fy), w01 = (1-fx) fy, w11 = fx fy
 *              nearest:  column min(floor(u' w), w - 1), row min(floor((1 - v') h), h - 1)
 * Textures change no scattering, RNG, traversal, miss or exit decision. With WFPT_FLAG_AOV a primary hit adds tex * albedo to the albedo sum.
 * wfpt_set_texture, wfpt_clear_texture, wfpt_bind_texture and wfpt_set_triangle_uvs act like wfpt_set_environment: the accumulation and the
 * frame counter restart, the temporal history and the captured graphs are dropped. wfpt_update_scene* and viewport changes keep the slots,
 * the bindings and the UV table. A refused call leaves the context as it was. WFPT_ERR_INVALID_ARGUMENT without the flag, for a slot out of
 * range, a binding to an empty slot, a bad size, texel or parameter, a UV that is not finite, and a triangle whose row is >= the rows of a set
 * UV table (checked by wfpt_set_triangle_uvs and wfpt_update_scene_mesh); WFPT_ERR_UNSUPPORTED for a call that would texture a
 * WFPT_LOOP_FUSED_BINNED context (a context with a binding never runs the class-binned loop). wfpt_render_chunked* masks the flag off.
 * Out of scope: mip-mapping, normal / bump / roughness maps, per-vertex normals, .mtl files. */
#define WFPT_MAX_TEXTURES 64u
typedef enum wfpt_texture_filter { WFPT_TEXTURE_BILINEAR = 0, WFPT_TEXTURE_NEAREST = 1 } wfpt_texture_filter;
typedef struct wfpt_texture_params {
    float scale[2];            /* finite; default (1, 1) */
    float offset[2];           /* finite; default (0, 0) */
    uint32_t filter;           /* a wfpt_texture_filter: WFPT_TEXTURE_BILINEAR (default) or WFPT_TEXTURE_NEAREST */
    uint32_t _reserved[3];     /* must be 0 */
} wfpt_texture_params;
WFPT_LAYOUT_ASSERT(sizeof(wfpt_texture_params) == 32 && offsetof(wfpt_texture_params, offset) == 8 &&
                       offsetof(wfpt_texture_params, filter) == 16 && offsetof(wfpt_texture_params, _reserved) == 20,
                   "wfpt_texture_params: 32 bytes");
/* scale (1, 1), offset (0, 0), bilinear, _reserved zeroed */
void wfpt_texture_params_default(wfpt_texture_params *p);
/* rgb: h rows of w texels, 3 floats each (linear, row-major, row 0 = the top), finite and >= 0; 1 <= w, h <= 16384. Stored on the device as
 * float4 texels in slot `slot`, replacing what it held (its bindings stay). p may be NULL (the defaults). Blocking. */
int wfpt_set_texture(wfpt_ctx *ctx, uint32_t slot, const float *rgb, uint32_t w, uint32_t h, const wfpt_texture_params *p);
/* empties the slot and unbinds the materials bound to it */
int wfpt_clear_texture(wfpt_ctx *ctx, uint32_t slot);
/* binds material material_idx (< the scene's materials) to slot (which must hold a texture); slot -1 unbinds */
int wfpt_bind_texture(wfpt_ctx *ctx, uint32_t material_idx, int32_t slot);
/* the UV table: n_rows rows of u0 v0 u1 v1 u2 v2 (finite), row r for the triangles whose _pad is r; NULL / 0 clears it */
int wfpt_set_triangle_uvs(wfpt_ctx *ctx, const float *uv6, uint32_t n_rows);
/* the lookup above on the device for n caller UVs (2 floats each) into rgb_out (3 floats each); the slot must hold a texture. Blocking. */
int wfpt_sample_texture(wfpt_ctx *ctx, uint32_t slot, const float *uv, size_t n, float *rgb_out);
/* the texture launches of every timed render since wfpt_create (not a wfpt_stage: WFPT_STAGE_COUNT stays as it is) */
int wfpt_texture_timing_ms(wfpt_ctx *ctx, float *ms_total, uint32_t *launches);

/* ------------------------------------------------------------------ Emission (WFPT_FLAG_EMISSION): materials that light the scene
 * A context created with WFPT_FLAG_EMISSION holds one emission colour per material, all zero at creation. A material with a non-zero colour
 * is an emitter -- Shirley's diffuse_light: it emits and does not scatter.
 * The per-sample image holds the path throughput thr per pixel: 1 when the primary ray is generated, times the albedo at every hit, times
 * the sky (or the environment map) at a miss. A context with an emitter keeps a second per-sample plane `emitted` of the same shape, 0
 * wherever the image is set to 1. Before every shade step of every loop, an emission pass visits the hits that step will shade; for each hit
 * on an emitter of colour e, per channel, with IEEE f32 operations and no fma:
 *   emitted[pixel] <- emitted[pixel] + thr * e      (one multiply, one add)
 *   thr            <- +0.0                          (the path is dead)
 * Shade then runs unchanged: it scatters the dead path, which keeps travelling with zero throughput and adds +0 wherever it ends (0 * e = +0
 * at another emitter). With WFPT_FLAG_TEXTURES the emission pass runs after the texture pass of the same step, so an emitter's bound texture
 * modulates its light: emitted += (thr * tex) * e.
 * Accumulation adds image_k + emitted_k per sample, in ascending sample order: one f32 add per channel for the sample's value, then the add
 * into `accumulated`; every batch size and loop gives the same bits. On a WFPT_FLAG_DENOISE context the luminance moments take L of that
 * same value. The AOVs are unchanged: a primary hit on an emitter adds its material albedo (times its texture) to the albedo sum.
 * What does not change:
 *   - the loop exit `misses < miss_floor`: a closed room lit by emitters alone has no misses, so it needs miss_floor = 0 to be traced at all;
 *   - dead paths stay in the queues: they cost their bounces until they miss or max_wavefronts ends them (DESIGN.md 9g has the price);
 *   - without WFPT_FLAG_NEE ("Next-event estimation" below) there are no shadow rays: emitters are found by path hits only.
 * With no emitter set, a flagged context launches exactly the kernels a context without the flag launches and renders the same bits; the
 * second plane is allocated with the first emitter.
 * wfpt_set_emission and wfpt_clear_emission act like wfpt_bind_texture: the accumulation and the frame counter restart, the temporal
 * history and the captured graphs are dropped. wfpt_update_scene* keeps the colours of the material indices below the new material count;
 * the colours of indices at or beyond it are dropped (a later scene with more materials finds them zero). Viewport changes keep everything.
 * A refused call leaves the context as it was. WFPT_ERR_INVALID_ARGUMENT without the flag, for a material index out of range and for a
 * colour that is not finite or is negative; WFPT_ERR_UNSUPPORTED for a set or clear on a WFPT_LOOP_FUSED_BINNED context (a context with an
 * emitter never runs the class-binned loop). wfpt_render_chunked* masks the flag off. wfpt_read_image returns thr alone. */
/* rgb: finite and >= 0; all zeros makes the material an ordinary one again */
int wfpt_set_emission(wfpt_ctx *ctx, uint32_t material_idx, const float rgb[3]);
int wfpt_get_emission(wfpt_ctx *ctx, uint32_t material_idx, float rgb[3]);
/* every material's colour back to zero */
int wfpt_clear_emission(wfpt_ctx *ctx);
/* the emission launches of every timed render since wfpt_create -- the passes and the zeroing of the second plane at the start of each
 * batch (not a wfpt_stage: WFPT_STAGE_COUNT stays as it is) */
int wfpt_emission_timing_ms(wfpt_ctx *ctx, float *ms_total, uint32_t *launches);

/* ------------------------------------------------------------------ Next-event estimation (WFPT_FLAG_NEE): shadow rays to the emitters
 * wfpt_create* accepts WFPT_FLAG_NEE only together with WFPT_FLAG_EMISSION (WFPT_ERR_INVALID_ARGUMENT otherwise). A flagged context with
 * an emitter keeps a light list: the indices of all primitives whose material emits, in the order the device holds the primitives,
 * resolved wherever the emission table is (wfpt_set_emission, wfpt_clear_emission, wfpt_update_scene*). Before every shade step of every
 * loop the passes run in the order texture, emission, connect, shade. Each pixel has a connected flag, 0 wherever the image is set to 1.
 * The connect pass visits the hits the step will shade. For hit h of wavefront b (b = 0 for the primary hits; the stage API counts the
 * extend stages since the last generate_rays stage):
 *  1. The hit is diffuse when its material class is Lambertian (mat_type 0 or above 2) and its material does not emit. A diffuse hit sets
 *     the pixel's flag to 1 and goes on; every other hit (metal, dielectric, emitter) clears it to 0 and does nothing else.
 *  2. Three draws u0 u1 u2 from a stream of the pass's own, keyed by the pixel in both RNG modes (shade's stream is not touched):
 *       s = init_rng((x, y), (W, H), frame) = jenkins_hash((x + y W) ^ jenkins_hash(frame)), frame the sample's frame (no advance by
 *       sample_number);  s <- jenkins_hash(s ^ (0x9E3779B9 * (b + 1)))  (u32 arithmetic);  then three rng_next_float(s).
 *  3. With n_l lights, nf = f32(n_l): light i = min(floor(u0 * nf), n_l - 1), its primitive's material emits e. A point q on it, uniform by
 *     area, its normal nl and its area A. All operations are IEEE f32 add, sub, mul, div, sqrt in the order written, no fma; sin and cos
 *     are the library's own (wfpt_selftest_math), pi = 3.1415927f, 2 pi and 4 pi its exact doubles:
 *       sphere (c, radius):  ra = |radius|;  z = 1 - 2 u1;  r = sqrt(max(0, 1 - z z));  phi = (2 pi) u2;
 *                            q = c + ra * (r cos phi, r sin phi, z)   (per component: the product in the parentheses, times ra, plus c);
 *                            nl = (q - c) / ra   (three divisions);  A = (4 pi) * (ra ra)
 *       triangle (v0, e1, e2):  su = sqrt(u1);  b1 = 1 - su;  b2 = u2 su;  q = (v0 + b1 e1) + b2 e2;
 *                            nl = the stored normalize(cross(e1, e2));  cr = cross(e1, e2), each component one difference of two products
 *                            (e1.y e2.z - e1.z e2.y, ...);  A = 0.5 * sqrt((cr.x cr.x + cr.y cr.y) + cr.z cr.z)
 *     Lights emit from both sides.
 *  4. p = o + t d as shade computes it (shade.wgsl:91), n the normal shade scatters about (never flipped):
 *       v = q - p;  dist2 = (v.x v.x + v.y v.y) + v.z v.z;  dist = sqrt(dist2);  w = v / dist   (three divisions);
 *       cos_s = (n.x w.x + n.y w.y) + n.z w.z;  cos_l = |(nl.x w.x + nl.y w.y) + nl.z w.z|
 *     The sample contributes only if A > 0, dist2 > 0, cos_s > 0 and cos_l > 0 (a NaN fails each test). Then the ray (p, w) is traced with
 *     the context's own traversal (t_min = 0.001, extend.wgsl:90); the sample is occluded iff the closest hit has t < dist * 0.999.
 *  5. An unoccluded sample adds, per channel, emitted[pixel] += ((thr * albedo) * e_q) * G with
 *       G = (((cos_s * cos_l) * A) * nf) / (pi * dist2)
 *     thr the pixel's throughput after the texture and emission passes of this step, albedo the one shade will multiply in, e_q = e, or
 *     e * tex per channel where the light's material is bound to a texture (the texture pass's lookup at q).
 * The emission pass of such a context still leaves thr = +0 at a hit on an emitter, but adds thr * e only where the pixel's connected flag
 * is 0: at primary hits and after a metal or dielectric bounce. After a diffuse bounce the connect pass has already counted that light
 * (next-event estimation without multiple importance sampling; with it: WFPT_FLAG_MIS, "Multiple importance sampling" below).
 * Shade, the tracing kernels, miss, the loop exit, the AOVs, accumulation (image + emitted in sample order) and the luminance moments are
 * unchanged, and dead paths keep travelling. Every batch size, loop, RNG mode's queue order and band sharding gives the same connect
 * samples: the stream is keyed by the pixel.
 * With no emitter set a flagged context launches exactly the kernels a context without the flag launches and renders the same bits. A
 * context with the flag and an emitter never runs the class-binned loop (set and clear on such a context are refused, see "Emission");
 * wfpt_render_chunked* masks the flag off. The calls below return WFPT_ERR_INVALID_ARGUMENT on a context without the flag.
 * (Light selection by power: WFPT_FLAG_LIGHT_POWER, "Light selection by power" below. Lights without a surface -- point, spot, directional:
 * WFPT_FLAG_ANALYTIC_LIGHTS, "Analytic lights" below.)
 * Not done: multiple importance sampling, cone sampling of sphere lights, a light BVH, retiring fully
 * shadowed paths (dead ones: WFPT_FLAG_RETIRE), contact shadows thinner than the 0.001 / 0.1 % windows. (Importance sampling of the environment map: WFPT_FLAG_ENV_NEE.) */
/* the number of emitting primitives (the light list's length), 0 with none; negative: a wfpt_status */
int wfpt_nee_light_count(wfpt_ctx *ctx);
/* the connect launches of every timed render since wfpt_create (not a wfpt_stage: WFPT_STAGE_COUNT stays as it is) */
int wfpt_nee_timing_ms(wfpt_ctx *ctx, float *ms_total, uint32_t *launches);
/* Steps 3 and 4 for n caller-supplied receivers on the device. in9: n rows of (p.xyz, n.xyz, u0, u1, u2); out8: n rows of (q.xyz, the
 * light's primitive index as a float, the unoccluded factor e_q * G per channel -- 0 where the sample contributes nothing --, 1.0 if the
 * sample is occluded and 0.0 otherwise). WFPT_ERR_INVALID_ARGUMENT while no primitive emits. */
int wfpt_sample_lights(wfpt_ctx *ctx, const float *in9, size_t n, float *out8);

/* ------------------------------------------------------------------ Environment next-event estimation (WFPT_FLAG_ENV_NEE)
 * wfpt_create* accepts WFPT_FLAG_ENV_NEE only together with WFPT_FLAG_ENVIRONMENT, WFPT_FLAG_EMISSION and WFPT_FLAG_NEE
 * (WFPT_ERR_INVALID_ARGUMENT otherwise). On such a context the map is one of the lights the connect pass can pick, sampled in proportion
 * to its radiance; its sample lands in the `emitted` plane, under the same connected flag (emitted.w).
 *
 * The sampling distribution is built by wfpt_set_environment and dropped by wfpt_clear_environment; wfpt_update_scene* and viewport
 * changes keep it. It is made of integers, so every build order gives the same tables. For a map of w x h texels (r, g, b):
 *   L(x, y)  = (0.2126 r + 0.7152 g) + 0.0722 b of the stored texel (f32, the luminance moments' order; `intensity` is not applied)
 *   Lm(x, y) = the maximum of L over columns x - 1, x, x + 1 (modulo w) and rows y - 1, y, y + 1 (clamped to [0, h - 1]): the texels the
 *              bilinear taps of a lookup inside texel (x, y) can reach, so a direction with radiance never has probability zero
 *   s_y      = the sine the library's sincos gives for pi * ((f32(y) + 0.5) / f32(h))
 *   f = Lm * s_y;  M = the maximum of f over the map
 *   k(x, y)  = u32(ceil((f / M) * 65535.0)), in [0, 65535], and 1 where f > 0 and the quotient underflows to 0
 *   row[y][x] = the inclusive prefix sum of k along row y (u32);  marg[y] = the inclusive prefix sum of the row totals (u64)
 *   total = marg[h - 1]
 * If M is not a finite number above 0 (a black map) there is no distribution, and for this flag the context behaves as with no map.
 *
 * With a distribution the context connects even with no emitter: the `emitted` plane and the connect launches exist from
 * wfpt_set_environment on. Steps 1 and 2 of "Next-event estimation" are unchanged (u0 u1 u2 as there). Then, with p the effective share
 * -- 1 when the light list is empty, the context's environment share (wfpt_set_environment_share, default 0.5) otherwise:
 *   p = 1:            the environment branch, without a comparison (a draw of exactly 1.0 never reaches an empty light list)
 *   p < 1, u0 >= p:   the emitter branch: q = 1 - p;  steps 3-5 with u0' = (u0 - p) / q in place of u0, and the value step 5 adds is
 *                     divided by q as its last operation: emitted += (((thr * albedo) * e_q) * G) / q
 *   p < 1, u0 < p:    the environment branch
 * The environment branch draws two more floats u3 u4 from the same stream (only this branch draws them). All operations are IEEE f32 in
 * the order written, no fma, f64 only where said; pi = 3.1415927f, 2 pi its exact double, 2 pi^2 = 19.739209f:
 *   row:      T = u64(floor(f64(u1) * f64(total))), at most total - 1;  y = the first row with marg[y] > T
 *   column:   R = row[y][w - 1];  C = u32(floor(f64(u2) * f64(R))), at most R - 1;  x = the first column with row[y][x] > C
 *             (a NaN or negative product of a caller's row selects 0);  k = row[y][x] - row[y][x - 1] (row[y][-1] = 0), > 0 by construction
 *   direction: u = (f32(x) + u3) / f32(w);  v = (f32(y) + u4) / f32(h);  theta = pi * v;  phi = (2 pi) * ((u - 0.5) - rotation);
 *             (st, ct) = sincos(theta);  (sp, cp) = sincos(phi);  wdir = (st * sp, ct, -(st * cp))
 *             -- the inverse of the lookup's phi = atan2(n.x, -n.z), theta = atan2(hypot(n.x, n.z), n.y), u = phi / 2 pi + 0.5 + rotation
 *   probability: P = f32(k) / f32(total) (u64 -> f32 rounds to nearest even);  pdf = ((P * f32(w)) * f32(h)) / ((2 pi^2) * st)
 *             cos_s = (n.x wdir.x + n.y wdir.y) + n.z wdir.z;  e = the map's lookup in direction wdir, with intensity and rotation
 * The sample contributes only if st > 0, cos_s > 0 and pdf > 0 (a NaN fails each test). Then the ray (p_hit, wdir) is traced with the
 * context's own traversal (t_min = 0.001); it is occluded iff the walk reports any hit. An unoccluded sample adds, per channel,
 *   emitted[pixel] += ((thr * albedo) * e) * Genv,   Genv = (cos_s / pi) / (pdf * p)
 * Either branch sets the pixel's connected flag to 1, as a diffuse hit does without this flag; metal, dielectric and emitter hits clear
 * it. The miss pass leaves thr = +0 where the pixel's connected flag is 1 -- the connect pass of the bounce before has already counted
 * the map -- and multiplies by the map where it is 0: primary misses and misses after a metal or dielectric bounce. The emission pass
 * gates emitter hits by the same flag, as before. AOVs, shade, the tracing kernels, the loop exit, accumulation and the moments are
 * untouched. Such a context never runs the class-binned loop while a map is set; wfpt_render_chunked* masks the flag off.
 * With no map set, or a black one, a flagged context launches exactly the kernels a context with the three other flags launches and
 * renders the same bits, with and without emitters. The calls below return WFPT_ERR_INVALID_ARGUMENT on a context without the flag; the
 * connect launches stay under wfpt_nee_timing_ms.
 * (Multiple importance sampling between the map and the scatter: WFPT_FLAG_ENV_MIS, "Environment multiple importance sampling" below.)
 * Not done: a distribution that accounts for the receiver's normal or for
 * visibility, a coarser importance grid or an alias table for very large maps, the class-binned loop and wfpt_render_chunked*. (Object
 * lights selected by power: WFPT_FLAG_LIGHT_POWER, refused together with this flag: the emitter branch beside the map's share selects
 * uniformly.) */
/* the environment share: finite, in (0, 1]. Acts like wfpt_set_emission: the accumulation restarts, the graphs and the history are dropped */
int wfpt_set_environment_share(wfpt_ctx *ctx, float share);
float wfpt_environment_share(const wfpt_ctx *ctx); /* 0 on a context without the flag */
/* the tables of the map's distribution: row_wh w * h words (row-major), marg_h h words; either may be NULL. WFPT_ERR_INVALID_ARGUMENT
 * while no map with a distribution is set */
int wfpt_read_environment_distribution(wfpt_ctx *ctx, uint32_t *row_wh, uint64_t *marg_h);
/* The environment branch with p = 1 for n caller-supplied receivers on the device. in10: n rows of (p.xyz, n.xyz, u1, u2, u3, u4); out8: n
 * rows of (wdir.xyz, f32(y * w + x), e * Genv per channel -- 0 where the sample contributes nothing --, 1.0 if the sample is occluded and
 * 0.0 otherwise). WFPT_ERR_INVALID_ARGUMENT while no map with a distribution is set */
int wfpt_sample_environment_light(wfpt_ctx *ctx, const float *in10, size_t n, float *out8);

/* ------------------------------------------------------------------ Multiple importance sampling (WFPT_FLAG_MIS)
 * wfpt_create* accepts WFPT_FLAG_MIS only together with WFPT_FLAG_EMISSION and WFPT_FLAG_NEE, and refuses it together with
 * WFPT_FLAG_ENV_NEE (WFPT_ERR_INVALID_ARGUMENT either way). The flag combines the two strategies that can find an emitter after a diffuse
 * bounce -- shade's cosine-distributed Lambertian scatter and the connect pass's area sampling of the light list -- by the balance
 * heuristic. No ray is added: the emitter hit of a scattered ray, which "Next-event estimation" drops, gets the weight wb, and the shadow
 * ray's sample, which it takes whole, gets the complementary wl.
 *
 * The identity the weights rest on: shade's Lambertian scatter (shade.wgsl:102-108) is d = n + r with r a normalised point of the unit
 * sphere and d NOT normalised, a cosine distribution about the unflipped n with solid-angle density cos / pi. As |n| = |r| = 1,
 * |d|^2 = 2 (1 + n.r), so the cosine of d against n is |d| / 2: the density of the scatter that produced a ray is (0.5 |d|) / pi, from
 * the ray's own direction, without the previous normal. Two caveats: n and r are unit vectors only to rounding, so 0.5 |d| and n.d / |d|
 * differ by rounding (DESIGN.md 9j measures it); and the scatter's `length < 0.001` fallback d = n gives 0.5 where the cosine is 1, an
 * event of probability of order 1e-9 that is accepted.
 *
 * On a flagged context with an emitter the step order stays texture, emission, connect, shade; the stream, the draws, the light choice,
 * the point, the occlusion test and the connected flag of "Next-event estimation" are unchanged. All operations are IEEE f32 in the order
 * written, no fma, pi = 3.1415927f. Two things change:
 *  1. Connect pass, step 5. For an unoccluded contributing sample
 *       pb = cos_s / pi;  pl = dist2 / ((cos_l * A) * nf);  wl = pl / (pl + pb)
 *       emitted[pixel] += (((thr * albedo) * e_q) * G) * wl
 *     At every diffuse hit, contributing or not, the pass also writes the hit point p (as shade computes it) into a per-sample,
 *     per-pixel float4 plane `origin`, as (p.x, p.y, p.z, 0). The plane has the shape of `emitted`, is allocated with the first emitter
 *     and kept, and costs 16 bytes per pixel per sample in flight. It is never zeroed: it is read only where the connected flag is 1.
 *  2. Emission pass. At a hit on an emitter whose pixel's connected flag is 0, emitted += thr * e as before (primary hits, hits after
 *     metal or glass). Where the flag is 1, with d the hit's ray direction (not normalised), o the pixel's `origin` entry and ph the hit
 *     point as shade computes it:
 *       v = ph - o;  dist2 = (v.x v.x + v.y v.y) + v.z v.z;  dist = sqrt(dist2);  w = v / dist   (three divisions)
 *       nl, A = the hit primitive's, as step 3 of "Next-event estimation" computes them with q = ph
 *               (sphere: nl = (ph - c) / ra, A = (4 pi) * (ra ra);  triangle: the stored normal and the cross-product area)
 *       cos_l = |(nl.x w.x + nl.y w.y) + nl.z w.z|;  len = sqrt((d.x d.x + d.y d.y) + d.z d.z);  pb = (0.5 * len) / pi
 *       wb = 1 and pl = 0                                     if A > 0, dist2 > 0 or cos_l > 0 fails (a NaN fails each test)
 *       pl = dist2 / ((cos_l * A) * nf);  wb = pb / (pb + pl)   otherwise
 *       emitted[pixel] += (thr * e) * wb   per channel (thr already holds the texture where the texture pass applied);  thr <- +0
 *     wb = 1 on a failed condition because the connect pass can never produce that sample. o equals the origin of the ray that made the
 *     hit bit for bit (extension_ray.origin = p): a loop that still holds the ray queue may read it there instead; the shipped kernels
 *     read the plane in every loop.
 * Every batch size, loop, RNG mode and band sharding gives the same weights: they depend on the path alone.
 * With no emitter set a flagged context launches exactly the kernels a context without the flag launches and renders the same bits. A
 * flagged context with an emitter never runs the class-binned loop (see "Emission"); wfpt_render_chunked* masks the flag off. The
 * launches are booked under wfpt_emission_timing_ms and wfpt_nee_timing_ms. The calls below are blocking and return
 * WFPT_ERR_INVALID_ARGUMENT on a context without the flag and while no primitive emits.
 * (Weighing the environment map against the scatter: WFPT_FLAG_ENV_MIS, a flag of its own below; WFPT_FLAG_ENV_NEE stays refused here.)
 * (Light selection by power: WFPT_FLAG_LIGHT_POWER, "Light selection by power" below, which restates pl with the selected light's weight.)
 * (Analytic lights: WFPT_FLAG_ANALYTIC_LIGHTS, "Analytic lights" below: their samples are not weighed, and nf counts them.)
 * Not done: the power heuristic, cone sampling of
 * sphere lights, MIS for fuzzy metal, the class-binned loop and wfpt_render_chunked*. */
/* Steps 3 to 5 with the weight for n caller-supplied receivers on the device. in9: as wfpt_sample_lights; out12: n rows of (q.xyz, the
 * light's primitive index as a float, ((e_q * G) * wl) per channel, 1.0 if the sample is occluded and 0.0 otherwise, pl, pb, wl, 0) --
 * the three channels and pl, pb, wl are 0 where the sample contributes nothing. */
int wfpt_sample_lights_mis(wfpt_ctx *ctx, const float *in9, size_t n, float *out12);
/* The emission pass's weight for n caller-supplied hits on the device. in8: n rows of (o.xyz, d.xyz, t, the primitive index as the float
 * of its integer value), with ph = o + t d per component; out4: n rows of (pl, pb, wb, cos_l). A primitive that does not emit or is out
 * of range (a NaN included) gives (0, pb, 1, 0). */
int wfpt_mis_hit_weight(wfpt_ctx *ctx, const float *in8, size_t n, float *out4);

/* ------------------------------------------------------------------ Light selection by power (WFPT_FLAG_LIGHT_POWER)
 * wfpt_create* accepts WFPT_FLAG_LIGHT_POWER only together with WFPT_FLAG_EMISSION and WFPT_FLAG_NEE, and refuses it together with
 * WFPT_FLAG_ENV_NEE, and therefore WFPT_FLAG_ENV_MIS (WFPT_ERR_INVALID_ARGUMENT either way). It combines freely with WFPT_FLAG_MIS,
 * WFPT_FLAG_TEXTURES, WFPT_FLAG_ENVIRONMENT, WFPT_FLAG_RETIRE, WFPT_FLAG_ADAPTIVE, WFPT_FLAG_AOV, WFPT_FLAG_DENOISE, every loop the emitters
 * run in, both RNG modes and band sharding. "Next-event estimation" picks light i = floor(u0 * n_l) uniformly and weighs the sample by
 * nf = f32(n_l): a bright lamp among 63 dim ones is sampled 1/64 of the time with weight 64, and a light of no area draws its share of
 * shadow rays for nothing. A flagged context picks light i with a probability proportional to its power, luminance times area.
 *
 * The distribution belongs to the light list and is rebuilt wherever the list is (wfpt_set_emission, wfpt_clear_emission,
 * wfpt_update_scene*); viewport changes keep it; texture bindings do not enter it. It is made of integers, so every build order gives the
 * same tables. For light i of the list (primitive lights[i], its material's colour e), all f32, no fma:
 *       A_i = the area exactly as step 3 of "Next-event estimation" computes it
 *             (sphere: (4 pi) * (ra ra);  triangle: 0.5 * sqrt((cr.x cr.x + cr.y cr.y) + cr.z cr.z))
 *       L_i = (0.2126 e.r + 0.7152 e.g) + 0.0722 e.b   (the denoiser's luminance, in its order);  f_i = L_i * A_i
 *       M = the maximum of the f_i that are > 0
 *       k_i = u32(ceil((f_i / M) * 65535.0)) where f_i > 0, and 1 where that quotient underflows to 0;  k_i = 0 where f_i > 0 fails (a NaN
 *             included): such a light is never selected
 *       cdf[i] = k_0 + ... + k_i  (u64);  total = cdf[n_l - 1];  prim_k[primitive] = k_i for the lights, 0 for every other primitive
 * If M is not a finite number above 0 (no f_i > 0, or one overflows) there is no distribution, and the context behaves, for this flag, as
 * a context without it: the same kernels, the same bits. The tables cost 8 bytes per light and 4 per primitive.
 *
 * With a distribution, steps 1, 2 and 4 of "Next-event estimation" are unchanged: the stream, the three draws, the point on the light from
 * u1 u2, the occlusion window and the connected flag. What changes:
 *  - Step 3, the selection.  T = u64(floor(f64(u0) * f64(total))), at most total - 1; a NaN or negative product selects 0.  i = the first
 *    index with cdf[i] > T (a binary search; lights with k = 0 are never chosen).  k = cdf[i] - cdf[i - 1]  (cdf[-1] = 0).
 *    nfi = f32(total) / f32(k): the two conversions round to nearest even, then one division.
 *  - Steps 3 and 5, the weight. nfi stands wherever nf stood:  G = (((cos_s * cos_l) * A) * nfi) / (pi * dist2).
 *  - WFPT_FLAG_MIS, connect pass:  pl = dist2 / ((cos_l * A) * nfi);  pb and wl as before.
 *  - WFPT_FLAG_MIS, emission pass, where the connected flag is 1:  k = prim_k[hit primitive];  wb = 1 and pl = 0 if k == 0 or one of the
 *    existing conditions fails;  otherwise nfi = f32(total) / f32(k),  pl = dist2 / ((cos_l * A) * nfi),  wb = pb / (pb + pl).
 * wfpt_sample_lights, wfpt_sample_lights_mis and wfpt_mis_hit_weight on such a context follow this section and keep their row layouts. The
 * connect launches stay under wfpt_nee_timing_ms, the emission launches under wfpt_emission_timing_ms.
 * Consequences:
 *  - No emitter. With no emitter set a flagged context launches the kernels of the unflagged one and renders the same bits.
 *  - One light. With exactly one light total = k = 65535, nfi = 1.0f = nf and the selection is trivial: the images and every sampler row are
 *    bit-identical to the unflagged context's.
 *  - Several equal lights. Nothing of the kind is promised: the f64 selection and the f32 one round differently at the boundaries.
 * wfpt_render_chunked* masks the flag off, as it does its prerequisites.
 * Not done: the emitter branch of WFPT_FLAG_ENV_NEE / WFPT_FLAG_ENV_MIS contexts (the flag is refused there), an alias table, power that
 * accounts for a light's texture, a light BVH (selection that knows the receiver). */
/* The light list and its distribution: light_prims and cdf get wfpt_nee_light_count entries each; either may be NULL. Blocking.
 * WFPT_ERR_INVALID_ARGUMENT on a context without the flag and while the list has no distribution. */
int wfpt_read_light_distribution(wfpt_ctx *ctx, uint32_t *light_prims, uint64_t *cdf);

/* ------------------------------------------------------------------ Analytic lights (WFPT_FLAG_ANALYTIC_LIGHTS)
 * Lights without a surface: point lights, spot lights and directional lights (a sun). No ray can hit them, so they are reached by the
 * connect pass alone. wfpt_create* accepts WFPT_FLAG_ANALYTIC_LIGHTS only together with WFPT_FLAG_EMISSION and WFPT_FLAG_NEE, and refuses
 * it together with WFPT_FLAG_ENV_NEE, WFPT_FLAG_ENV_MIS and WFPT_FLAG_LIGHT_POWER (WFPT_ERR_INVALID_ARGUMENT either way). It combines
 * freely with WFPT_FLAG_MIS, WFPT_FLAG_TEXTURES, WFPT_FLAG_ENVIRONMENT, WFPT_FLAG_RETIRE, WFPT_FLAG_ADAPTIVE, WFPT_FLAG_AOV,
 * WFPT_FLAG_DENOISE, every loop the emitters run in, both RNG modes and band sharding.
 *
 * wfpt_set_lights replaces the context's analytic lights (NULL / 0: none) and acts like wfpt_set_emission: the accumulation and the frame
 * counter restart, the temporal history and the captured graphs are dropped; wfpt_update_scene* and viewport changes keep the lights; a
 * refused call leaves the context as it was; WFPT_ERR_UNSUPPORTED on a context that runs WFPT_LOOP_FUSED_BINNED (a context that holds an
 * analytic light never runs that loop); wfpt_render_chunked* masks the flag off. WFPT_ERR_INVALID_ARGUMENT: a context without the flag,
 * n > WFPT_MAX_LIGHTS, n > 0 with a NULL array, an unknown type, a position that is not finite (point, spot), a colour that is not
 * finite or is negative, a direction (spot, directional) that is not finite or has length 0 -- or whose squared length overflows or
 * underflows to 0 in f32 --, a spot that does not satisfy -1 <= cos_outer < cos_inner <= 1 (a NaN fails it). The fields a type does not
 * read (a directional light's position, a point light's direction, the cosines of both) are stored as given and never looked at.
 * The direction of a spot or directional light is normalised once, at the call, on the host, in IEEE f32:
 *       len = sqrt((x x + y y) + z z);  direction <- (x / len, y / len, z / len)
 * and the normalised direction is what is stored, what wfpt_get_lights returns and what every formula below reads. A colour of -0 is
 * stored as +0. On the device the lights are three 16-byte rows each, wfpt_light's own layout.
 *
 * Semantics. n_l: the length of the emitter list of "Next-event estimation"; n_a: the number of analytic lights; N = n_l + n_a;
 * Nf = f32(N). Wherever the sections above say "a context with an emitter" a flagged context reads "with N > 0": the connect pass runs,
 * and the `emitted` plane, the connected flag and (WFPT_FLAG_MIS) the `origin` plane exist, from the first call that makes N > 0 -- a
 * scene lit by a sun alone, with no emissive material, is the main case. The emission pass runs while a material emits, as before.
 * With n_a = 0 a flagged context launches exactly the kernels of the unflagged context and renders the same bits; with N = 0 those of a
 * context without any of the flags.
 * Steps 1, 2 and 4 of "Next-event estimation" are unchanged: the stream, the three draws (u1 and u2 are drawn and not used by an analytic
 * light), the connected flag. All operations are IEEE f32 in the order written, no fma, pi = 3.1415927f. What changes:
 *  - Selection.  i = min(u32(min(max(floor(u0 * Nf), 0), Nf)), N - 1)  (a NaN or negative u0 of a caller's row selects 0).  i < n_l picks
 *    emitter lights[i]: everything as today with Nf wherever nf stood -- in G, and under WFPT_FLAG_MIS in pl of the connect pass and of
 *    the emission pass. Otherwise the pass picks analytic light j = i - n_l, in the order of the array wfpt_set_lights took.
 *  - Point and spot light (position c, stored axis a, colour e):
 *       v = c - p;  dist2 = (v.x v.x + v.y v.y) + v.z v.z;  dist = sqrt(dist2);  w = v / dist   (three divisions)
 *       cos_s = (n.x w.x + n.y w.y) + n.z w.z
 *       point:  fall = 1
 *       spot:   cd = -((a.x w.x + a.y w.y) + a.z w.z);  s = (cd - cos_outer) / (cos_inner - cos_outer);
 *               s <- s where s > 0, else 0 (a NaN gives 0);  s <- s where s < 1, else 1;  fall = (s s) * (3 - 2 s)
 *       G = ((cos_s * fall) * Nf) / (pi * dist2)
 *    The sample contributes only if dist2 > 0, cos_s > 0 and fall > 0 (a NaN fails each test). The ray (p, w) is traced as in step 4; the
 *    sample is occluded iff the closest hit has t < dist * 0.999, the emitters' window.
 *  - Directional light (stored axis a, the way the light travels; colour e, the irradiance on a surface that faces it):
 *       w = -a;  cos_s as above;  G = (cos_s * Nf) / pi
 *    The sample contributes only if cos_s > 0. The ray (p, w) is traced as the environment branch of "Environment next-event estimation"
 *    traces its ray (t_min = 0.001, no far end); the sample is occluded iff the walk reports any hit.
 *  - Contribution.  emitted[pixel] += ((thr * albedo) * e) * G per channel, as step 5. No texture applies to an analytic light.
 *  - WFPT_FLAG_MIS. The scatter can never produce an analytic light's sample, so it has wl = 1 and its contribution is not weighed (the
 *    value above is added as it stands). The `origin` plane and the connected flag are written as for any diffuse hit. The emission pass
 *    never sees an analytic light: it only reads Nf in nf's place. (After a diffuse bounce an emitter hit is therefore weighed against a
 *    connect pass that picks that emitter with probability 1 / N.)
 *  - Samplers. wfpt_sample_lights and wfpt_sample_lights_mis keep their row layouts and work while N > 0, n_l = 0 included. For analytic
 *    light j the primitive column holds -(1 + j) as a float; q is the light's position for point and spot lights and w for a directional
 *    one; the MIS row reports pl = 0, pb = cos_s / pi and wl = 1 where the sample contributes, zeros elsewhere. wfpt_mis_hit_weight uses
 *    Nf (and still needs an emitter).
 * Shade, the tracing kernels, miss, the loop exit, the AOVs, accumulation and the moments are untouched. The connect launches stay under
 * wfpt_nee_timing_ms.
 * Not done: the flag together with WFPT_FLAG_ENV_NEE, with WFPT_FLAG_ENV_MIS, and with WFPT_FLAG_LIGHT_POWER (refused: the map's share and
 * the power distribution both select among emitters only); area-less lights with a radius (soft shadows), IES profiles, selection that
 * knows the receiver, the class-binned loop and wfpt_render_chunked*. */
typedef enum wfpt_light_type { WFPT_LIGHT_POINT = 0, WFPT_LIGHT_SPOT = 1, WFPT_LIGHT_DIRECTIONAL = 2 } wfpt_light_type;
typedef struct wfpt_light {      /* 48 bytes, three 16-byte rows */
    float position[3];  uint32_t type;        /* a wfpt_light_type */
    float direction[3]; float cos_inner;      /* direction: the way the light travels (spot axis, sun direction) */
    float colour[3];    float cos_outer;      /* point / spot: radiant intensity; directional: irradiance on a facing surface */
} wfpt_light;
WFPT_LAYOUT_ASSERT(sizeof(wfpt_light) == 48 && offsetof(wfpt_light, direction) == 16 &&
                       offsetof(wfpt_light, cos_inner) == 28 && offsetof(wfpt_light, colour) == 32 && offsetof(wfpt_light, cos_outer) == 44,
                   "wfpt_light layout");
#define WFPT_MAX_LIGHTS 1024u
/* lights: n entries, copied; NULL / 0 clears */
int wfpt_set_lights(wfpt_ctx *ctx, const wfpt_light *lights, uint32_t n);
/* the lights as stored (directions normalised): up to `capacity` entries into out (may be NULL with capacity 0), the count into *n (may be NULL) */
int wfpt_get_lights(wfpt_ctx *ctx, wfpt_light *out, uint32_t capacity, uint32_t *n);
/* the number of analytic lights, 0 with none; negative: a wfpt_status */
int wfpt_analytic_light_count(wfpt_ctx *ctx);

/* ------------------------------------------------------------------ Environment multiple importance sampling (WFPT_FLAG_ENV_MIS)
 * wfpt_create* accepts WFPT_FLAG_ENV_MIS only together with WFPT_FLAG_ENVIRONMENT, WFPT_FLAG_EMISSION, WFPT_FLAG_NEE and
 * WFPT_FLAG_ENV_NEE, and refuses it together with WFPT_FLAG_MIS (WFPT_ERR_INVALID_ARGUMENT either way; WFPT_FLAG_MIS stays refused with
 * WFPT_FLAG_ENV_NEE, which is why this is a bit of its own). "Environment next-event estimation" takes all light of the map after a
 * diffuse bounce from the one shadow ray and zeroes the scattered ray's miss, although that ray is traced anyway. This flag keeps both
 * and weighs them by the balance heuristic, and does the same for the emitters (as "Multiple importance sampling" does without a map).
 * No ray is added. The scatter's density comes from the identity of "Multiple importance sampling": the miss queue of a
 * WFPT_FLAG_ENVIRONMENT context carries the un-normalised direction d, and (0.5 |d|) / pi is the density of the scatter that made it.
 *
 * The flag acts only while the map has a sampling distribution. With no map set, or a black one, a flagged context launches exactly the
 * kernels the same context without the flag launches and renders the same bits, with and without emitters. While a distribution exists
 * the step order stays texture, emission, connect, shade, then miss; the stream, the draws u0..u4, the branch choice, the selections,
 * the direction, the occlusion tests and the connected flag of "Next-event estimation" and "Environment next-event estimation" are
 * unchanged. All operations are IEEE f32 in the order written, no fma, pi = 3.1415927f, 2 pi^2 = 19.739209f; p is the effective share (1
 * with an empty light list), q = 1 - p. Four things change:
 *  1. Connect pass, environment branch. For a contributing, unoccluded sample
 *       pe = pdf * p;  pb = cos_s / pi;  we = pe / (pe + pb)
 *       emitted[pixel] += (((thr * albedo) * e) * Genv) * we
 *  2. Connect pass, emitter branch (only when p < 1). With pl and pb as step 1 of "Multiple importance sampling" computes them
 *       plq = pl * q;  wl = plq / (plq + pb)
 *       emitted[pixel] += ((((thr * albedo) * e_q) * G) / q) * wl
 *     At every diffuse hit, in either branch, contributing or not, the pass writes the hit point into the `origin` plane as described
 *     there. On a flagged context the plane is allocated wherever `emitted` is: with the first emitter or the first map that has a
 *     distribution, whichever comes first.
 *  3. Emission pass. Where the pixel's connected flag is 0 nothing changes. Where it is 1, step 2 of "Multiple importance sampling" with
 *     plq = pl * q in place of pl: wb = pb / (pb + plq), and wb = 1 on a failed condition. (With p = 1 and emitters, a share the caller
 *     set, plq = 0 and the hit counts whole: the connect pass never samples an emitter then.)
 *  4. Miss pass. Where the pixel's connected flag is 0: thr *= c, as before. Where it is 1, with d the miss queue's direction:
 *       len = sqrt((d.x d.x + d.y d.y) + d.z d.z);  pb = (0.5 * len) / pi
 *       n, phi, theta, u (after its wrap), v: exactly the values the map's lookup forms for d ("Environment map")
 *       st = sqrt(n.x n.x + n.z n.z)   (the value the lookup hands to atan2)
 *       xt = min(u32(floor(u * f32(w))), w - 1);  yt = min(u32(floor(v * f32(h))), h - 1)   (a NaN u or v selects 0)
 *       k = row[yt][xt] - row[yt][xt - 1]   (row[yt][-1] = 0);  P = f32(k) / f32(total)
 *       pdf = ((P * f32(w)) * f32(h)) / ((2 pi^2) * st);  pe = pdf * p
 *       wb = 1 and pe = 0           if st > 0 or pdf > 0 fails (a NaN fails each test)
 *       wb = pb / (pb + pe)         otherwise
 *       thr <- (thr * c) * wb       per channel, c the lookup's value as before
 *     The two sides take pb from different expressions (cos_s / pi in connect, the length in the miss) and the miss finds its texel from
 *     a rounded direction, so we + wb is 1 to rounding, not exactly (DESIGN.md 9l measures it), and a direction within a few ulp of a
 *     texel edge may find the neighbouring texel's k.
 * Every batch size, loop, RNG mode and band sharding gives the same weights: they depend on the path alone. A change of the map, the
 * share or the emitters drops the captured graphs as before. wfpt_render_chunked* masks the flag off. The launches are booked under
 * wfpt_emission_timing_ms, wfpt_nee_timing_ms and the miss stage. The calls below are blocking, use the context's effective share p, and
 * return WFPT_ERR_INVALID_ARGUMENT on a context without the flag, while no map with a distribution is set, and for a NULL pointer with
 * n > 0.
 * Not done: the power heuristic, a distribution aware of the receiver's normal, MIS for fuzzy metal, the class-binned loop,
 * wfpt_render_chunked*, the samplers of WFPT_FLAG_MIS (wfpt_sample_lights_mis, wfpt_mis_hit_weight) on a context
 * with this flag. */
/* The environment branch with its weight for n caller-supplied receivers on the device. in10: as wfpt_sample_environment_light; out12: n
 * rows of (wdir.xyz, f32(y * w + x), ((e * Genv) * we) per channel, 1.0 if the sample is occluded and 0.0 otherwise, pe, pb, we, 0) --
 * the three channels and pe, pb, we are 0 where the sample contributes nothing. */
int wfpt_sample_environment_light_mis(wfpt_ctx *ctx, const float *in10, size_t n, float *out12);
/* The miss pass's weight for n caller-supplied directions on the device. dirs3: n rows of an un-normalised direction; out4: n rows of
 * (pe, pb, wb, f32(yt * w + xt)). */
int wfpt_env_mis_miss_weight(wfpt_ctx *ctx, const float *dirs3, size_t n, float *out4);

/* ------------------------------------------------------------------ Path termination (WFPT_FLAG_RETIRE)
 * Without this flag no path ends before it misses or max_wavefronts ends it: a path that hit an emitter (thr = +0, "Emission") is
 * scattered, traced, connected and shaded on, and a closed room rendered with miss_floor = 0 runs every path to max_wavefronts.
 * wfpt_create* refuses the flag together with WFPT_FLAG_BINNING (WFPT_ERR_INVALID_ARGUMENT): such a context never runs the class-binned
 * loop. wfpt_render_chunked* masks the flag off, as the other feature flags. It combines freely with every other flag.
 *
 * A flagged context holds a wfpt_termination_params (defaults: roulette_start = 3, q_min = 0.05; roulette_start = 0xffffffff means no
 * roulette; q_min must be finite and in (0, 1]; _reserved must be 0). The termination step sits at the end of the shade step of
 * wavefront b (b = 0 for the primary hits; the stage API counts the extend stages since the last generate_rays stage, as the connect pass
 * does). The step order stays texture, emission, connect, shade. Shade forms t' = thr * albedo as before, the same bits, and then:
 *  1. The step applies only if b + 1 < max_wavefronts: the last shade of a loop emits nothing that is ever traced and stays as it is.
 *  2. Dead. If t'.x == 0 && t'.y == 0 && t'.z == 0 the hit is retired and thr <- t' as before (a -0 counts as zero; a NaN channel makes
 *     the test false).
 *  3. Roulette. Otherwise, if roulette_start != 0xffffffff and b >= roulette_start:
 *       m = t'.x;  if (t'.y > m) m = t'.y;  if (t'.z > m) m = t'.z
 *       q = m;  if (!(q >= q_min)) q = q_min          (a NaN m gives q_min)
 *       if q >= 1: the hit survives untouched and nothing is drawn. Otherwise one u is drawn from a stream of the step's own, keyed
 *       by the pixel in both RNG modes, with `frame` the sample's frame as the connect pass takes it:
 *         s = jenkins_hash(pixel_idx ^ jenkins_hash(frame));  s <- jenkins_hash(s ^ (0x85EBCA6Bu * (b + 1)));  u = rng_next_float(s)
 *       if u < q: the hit survives with thr <- t' / q (three IEEE f32 divisions); otherwise it is retired with thr <- (+0, +0, +0).
 *       thr.w stays as it is.
 *  4. A retired hit emits an INACTIVE extension ray: the next extend neither hits nor misses with it. It still occupies its slot:
 *     rays_in of the bounce table, counters[2] and n_in count slots as before, and the retired paths show up as rays_in - hits -
 *     misses. Shade's own RNG, the scatter, and the hit order and thread index of the surviving hits (shade's key under
 *     WFPT_RNG_DISPATCH) are those of a queue with gaps, exactly as for the padding rays of an image whose size is no multiple of 8.
 *     A survivor's scatter is unchanged; a retired hit's extension ray holds no direction anyone may rely on.
 * What does not change: the loop exit `misses < miss_floor` is untouched -- it now sees fewer misses in later wavefronts, so a flagged
 * context may leave the loop a wavefront earlier than an unflagged one; emission, connect, miss, the AOVs, accumulation, the moments and
 * the denoisers. The connected flag and the `origin` plane of a retired path are never read again. With the flag clear every context
 * launches the kernels it launched before.
 * wfpt_set_termination drops the captured graphs and restarts the accumulation, like wfpt_set_emission. The calls below return
 * WFPT_ERR_INVALID_ARGUMENT on a context without the flag or for a bad parameter; a refused call leaves the context as it was.
 * Not done: retiring fully shadowed paths, the class-binned loop and wfpt_render_chunked*. */
typedef struct wfpt_termination_params {
    uint32_t roulette_start; /* first wavefront b whose shade step plays roulette; 0xffffffff = never */
    float q_min;             /* the survival probability's floor, in (0, 1] */
    uint32_t _reserved[6];   /* must be 0 */
} wfpt_termination_params;
WFPT_LAYOUT_ASSERT(sizeof(wfpt_termination_params) == 32, "wfpt_termination_params is 32 bytes");
void wfpt_termination_params_default(wfpt_termination_params *p);
int wfpt_set_termination(wfpt_ctx *ctx, const wfpt_termination_params *p);
int wfpt_get_termination(wfpt_ctx *ctx, wfpt_termination_params *p);
/* Steps 2 and 3 (without the test of step 1) for n caller-supplied hits on the device, blocking. thr3: n rows of t'; pixel_idx: n
 * pixels; frame, b: the sample's frame and the wavefront. out8: n rows of (q, u, verdict, 0, thr'.rgb, 0) -- verdict 0 = retired dead,
 * 1 = retired by roulette, 2 = survives; q and u are 0 where nothing is drawn. */
int wfpt_sample_termination(wfpt_ctx *ctx, const float *thr3, const uint32_t *pixel_idx, uint32_t frame, uint32_t b, size_t n, float *out8);

/* ------------------------------------------------------------------ Adaptive sampling (WFPT_FLAG_ADAPTIVE)
 * Without this flag every sample goes to every pixel. A flagged context keeps, beside `accumulated`:
 *   mask    one uint64_t per 8x8 tile of the context's slab, indexed by generate_rays' tile index (slot >> 6: tiles row-major, a sharded
 *           context's own bands); bit ly * 8 + lx set = the pixel is active; bits of lanes outside the image are always clear. Allocated
 *           once at wfpt_create: the captured graphs hold its address and stay valid while its contents change.
 *   count   one uint32_t per pixel: the samples added to that pixel.
 *   S1, S2  the luminance moments of "Denoiser" (the same planes, the same L_k), allocated here on their own.
 * Whatever zeroes `accumulated` (wfpt_reset_accumulated, wfpt_reset_progress, a camera / size / scene change) zeroes count and the moments
 * and sets the mask to every pixel inside the image. wfpt_accumulated_samples keeps its meaning: the sample passes rendered.
 * wfpt_create* refuses the flag (WFPT_ERR_INVALID_ARGUMENT) together with WFPT_FLAG_AOV, WFPT_FLAG_DENOISE -- the AOV sums, the denoiser's
 * prepare and the temporal blend divide by one n for the whole image -- and WFPT_FLAG_BINNING; wfpt_render_chunked* refuses it. It
 * combines freely with every other flag, both RNG modes, spheres and meshes, scenes in LDS and beyond, and tile_world > 1.
 *
 * Rendering (wfpt_render, wfpt_render_sample, both timed calls; every loop kind). In generate_rays a lane whose bit is clear does what a
 * lane outside the image does: no primary ray is computed, its slot holds an inactive ray (the dense array's inactive marker in the
 * refill loop), and the pixel's image slice is not reset. Slots are NOT compacted: the launch's slot count, n_in, the work items and the
 * bounce table's rays_in are those of the unmasked frame, so the order of the hits -- shade's RNG key under WFPT_RNG_DISPATCH -- is that of
 * the same queue with gaps, as for the padding rays of an odd-sized image. The masked pixels show up as rays_in - hits - misses in row 0.
 * A wave (one tile) whose word is 0 computes no ray, reads no candidate list and walks nothing. Accumulate passes over a pixel whose bit
 * is clear before it loads anything of it -- `accumulated` and the moments stay -- and an active pixel adds the batch's samples in
 * ascending order as before, and count += the batch's samples. The mask is constant during a call: every batch size gives the same bits.
 * The loop exit `misses < miss_floor` is untouched and counts the misses of the ACTIVE pixels: under a mask whose primary rays rarely miss
 * (a region of ground, a few hard pixels left by the update) it ends a sample's loop earlier than it would for the whole frame -- before the
 * first shade, where fewer than miss_floor primary rays miss. Create the context with miss_floor = 0 where that matters.
 * The stage API (wfpt_kernel_run) ignores the mask and the counts, as it ignores the AOVs. wfpt_gather_accumulated* still gathers sums;
 * a gather of counts is out of scope. wfpt_read_accumulated still returns sums; wfpt_read_variance works on a flagged context with the
 * pixel's own n, and wfpt_save_ppm / _png / _pfm write the mean (wfpt_read_mean).
 *
 * wfpt_adaptive_update computes the next mask from the moments on the device, one wave per tile, one lane per pixel, on the context's
 * stream outside the captured graphs; it blocks only when n_active is not NULL, which then receives the number of set bits. For pixel i
 * with n = count[i], nf = (float)n, each line one IEEE f32 operation in this order:
 *   mu  = S1 / nf
 *   v   = max(0, S2 / nf - mu * mu) / nf           (wfpt_read_variance's formula with the pixel's own n; max(0, d) is d < 0 ? 0 : d)
 *   tol = threshold * (mu + luminance_floor)
 *   unconverged = !(n >= min_samples && v <= tol * tol)        (a NaN anywhere, and n == 0, leave the pixel unconverged)
 * A lane outside the image is neither unconverged nor under the maximum. Then, on the tile's 64-bit words:
 *   U = ballot(unconverged);  with dilate != 0, U is dilated by one pixel INSIDE THE TILE: H = U | ((U << 1) & ~col0) | ((U >> 1) & ~col7)
 *   (col0 = 0x0101010101010101, col7 = 0x8080808080808080), D = H | (H << 8) | (H >> 8)
 *   word = D & ballot(max_samples == 0 || n < max_samples) & ballot(inside the image)
 * The dilation is clipped to the tile on purpose: the update of a band-sharded context then equals the unsharded one bit for bit (no
 * rank needs another's moments), at the price of a converged pixel on a tile's edge not being kept alive by its neighbour across it.
 * wfpt_set_adaptive refuses (WFPT_ERR_INVALID_ARGUMENT, the context as it was) a threshold or luminance_floor that is not finite and
 * positive, min_samples < 2, a non-zero max_samples below min_samples and non-zero reserved words. A successful call neither resets the
 * accumulation nor drops the graphs: the parameters are arguments of the update kernel only.
 * Every call below returns WFPT_ERR_INVALID_ARGUMENT on a context without the flag. */
typedef struct wfpt_adaptive_params {
    uint32_t min_samples;    /* a pixel is never converged before it holds this many samples; >= 2 */
    uint32_t max_samples;    /* a pixel that holds this many samples is switched off; 0 = no maximum */
    float threshold;         /* relative tolerance of the mean's standard deviation; finite, > 0 */
    float luminance_floor;   /* added to the mean before the tolerance is formed (dark pixels); finite, > 0 */
    uint32_t dilate;         /* non-zero: the unconverged pixels keep their neighbours inside the tile alive */
    uint32_t _reserved[3];   /* must be 0 */
} wfpt_adaptive_params;
WFPT_LAYOUT_ASSERT(sizeof(wfpt_adaptive_params) == 32 && offsetof(wfpt_adaptive_params, max_samples) == 4 &&
                       offsetof(wfpt_adaptive_params, threshold) == 8 && offsetof(wfpt_adaptive_params, luminance_floor) == 12 &&
                       offsetof(wfpt_adaptive_params, dilate) == 16 && offsetof(wfpt_adaptive_params, _reserved) == 20,
                   "wfpt_adaptive_params: 32 bytes");
/* min_samples 16, max_samples 0, threshold 0.05, luminance_floor 0.01, dilate 1; _reserved zeroed */
void wfpt_adaptive_params_default(wfpt_adaptive_params *p);
int wfpt_set_adaptive(wfpt_ctx *ctx, const wfpt_adaptive_params *p);
int wfpt_get_adaptive(wfpt_ctx *ctx, wfpt_adaptive_params *p);
/* A caller's mask (region rendering): one byte per pixel, row-major like wfpt_read_accumulated, non-zero = active; n_pixels must be
 * wfpt_n_pixels. Bytes of a sharded slab's rows beyond the image are ignored. Blocking. wfpt_read_active_mask is the inverse (0 / 1). */
int wfpt_set_active_mask(wfpt_ctx *ctx, const uint8_t *mask, size_t n_pixels);
int wfpt_read_active_mask(wfpt_ctx *ctx, uint8_t *mask, size_t n_pixels);
int wfpt_adaptive_update(wfpt_ctx *ctx, uint32_t *n_active);
/* the per-pixel sample counts, n <= wfpt_n_pixels (blocking) */
int wfpt_read_sample_counts(wfpt_ctx *ctx, uint32_t *out, size_t n);
/* accumulated / (float)count, one IEEE f32 division per channel, 0 where the count is 0: 3 floats per pixel, stride 12 (blocking) */
int wfpt_read_mean(wfpt_ctx *ctx, float *rgb, size_t n_floats);
/* the same bits from a resolve kernel (mean_resolve_kernel) into a caller's device buffer of n_bytes (at most the whole image); ordered on
 * the context's stream, returns when they are written */
int wfpt_copy_mean_to_device(wfpt_ctx *ctx, void *device_ptr, size_t n_bytes);
/* The convenience loop, a host loop over the two public calls and nothing more: wfpt_render(interval) then wfpt_adaptive_update, until
 * no pixel is active or max_passes sample passes are done (the last wfpt_render takes what is left of them). interval >= 1. n_active
 * (may be NULL) receives the set bits of the last update. */
int wfpt_render_adaptive(wfpt_ctx *ctx, uint32_t max_passes, uint32_t interval, uint32_t *n_active);

/* ------------------------------------------------------------------ read-back (blocking) */

uint32_t wfpt_n_pixels(const wfpt_ctx *ctx);  /* pixels held by this context (whole 8-row bands when sharded) */
uint32_t wfpt_ray_capacity(const wfpt_ctx *ctx);
/* accumulated_image_buffer / image_buffer: 3 floats per pixel, stride 12, row-major (accumulate.wgsl:1-2) */
int wfpt_read_accumulated(wfpt_ctx *ctx, float *rgb, size_t n_floats);
int wfpt_read_image(wfpt_ctx *ctx, float *rgb, size_t n_floats);
/* device-to-device copy of the accumulated slab on the context's stream (for a RCCL gather) */
int wfpt_copy_accumulated_to_device(wfpt_ctx *ctx, void *device_ptr, size_t n_bytes);
/* ------------------------------------------------------------------ multi-GPU: RCCL gather of the band-sharded frame
 * BUILD-SIDE ADDITION (the reference is single-GPU). One process (or thread) per GPU creates a context
 * with tile_rank = r, tile_world = R: it renders the 8-row bands k with k % R == r, with no exchange inside the
 * bounce loop. The only collective is this gather of the accumulated slabs to rank 0 over xGMI:
 *   rank 0:    wfpt_comm_unique_id(id);  ... hand the 128 bytes to every rank by any means (MPI, a file, a socket) ...
 *   all ranks: wfpt_comm_init(ctx, id, r, R);                      (collective: ncclCommInitRank on the context's device)
 *   all ranks: wfpt_render(ctx, spp); wfpt_gather_accumulated(ctx); (asynchronous, ordered on the context's stream)
 *   rank 0:    wfpt_read_gathered(ctx, rgb, 3 * width * height);    (blocking; the assembled frame, row-major)
 * RCCL (librccl.so) is opened at run time; without it these calls return WFPT_ERR_UNSUPPORTED and nothing else in the
 * library depends on it. In the pixel-keyed RNG mode the gathered frame is bit-identical to a single-GPU render. */
#define WFPT_COMM_UNIQUE_ID_BYTES 128
int wfpt_comm_unique_id(void *id128);
int wfpt_comm_init(wfpt_ctx *ctx, const void *id128, int rank, int world);
int wfpt_gather_accumulated(wfpt_ctx *ctx);
/* The same gather bracketed by two events on the context's stream; blocks until it is done and returns its duration on this rank
 * (BASELINE.md section 3's "gather time"). What the stream did before -- renders still in flight -- is waited for first, so the figure
 * is the gather's own time when every rank calls it idle, after a barrier. */
int wfpt_gather_accumulated_timed(wfpt_ctx *ctx, float *ms);
int wfpt_read_gathered(wfpt_ctx *ctx, float *rgb, size_t n_floats);
int wfpt_comm_destroy(wfpt_ctx *ctx); /* also done by wfpt_destroy */

/* Queues in the reference's own layouts and in its (ascending-thread-index) order. */
int wfpt_read_rays(wfpt_ctx *ctx, wfpt_ray *rays, uint32_t n);
int wfpt_read_extension_rays(wfpt_ctx *ctx, wfpt_ray *rays, uint32_t n);
int wfpt_read_hits(wfpt_ctx *ctx, wfpt_hit_payload *hits, uint32_t n);
int wfpt_read_misses(wfpt_ctx *ctx, uint32_t *ray_indices, uint32_t n);
/* test/bench input injection: overwrite the first n rays of the current ray queue */
int wfpt_write_rays(wfpt_ctx *ctx, const wfpt_ray *rays, uint32_t n);
/* Per-bounce table of the last fused sample: rows of (rays_in, hits, misses, shaded). */
int wfpt_read_bounce_table(wfpt_ctx *ctx, uint32_t *rows4, uint32_t max_rows, uint32_t *n_rows);
/* Totals since creation over fused samples: [0] rays traced by extend, [1] hits, [2] misses. */
int wfpt_read_totals(wfpt_ctx *ctx, uint64_t totals[3]);
/* The same per wavefront: rows of (rays traced, hits, misses) summed over every fused sample since creation, one row
 * per wavefront 0 .. max_wavefronts-1 (what a bench needs to price each launch of the loop in bytes). */
int wfpt_read_wavefront_totals(wfpt_ctx *ctx, uint64_t *rows3, uint32_t max_rows, uint32_t *n_rows);
/* hipDeviceProp_t facts a report needs: CU count, memory clock (kHz) and bus width (bits), memory size. Any output
 * pointer may be NULL. Double-data-rate peak bandwidth = 2 * clock * width / 8. */
int wfpt_device_info(int device, uint32_t *compute_units, uint32_t *memory_clock_khz, uint32_t *memory_bus_width_bits,
                     uint64_t *total_memory_bytes);
/* display_shader.wgsl:50-52 tone map, sqrt(acc / n_samples) -> 8-bit RGB (host side, for image dumps) */
void wfpt_tonemap_rgb8(const float *accumulated, uint32_t n_pixels, uint32_t n_samples, uint8_t *rgb);

/* Image output, the step right after the path (the reference presents through a fullscreen pass, display.rs:112-150,
 * display_shader.wgsl:44-55; here the frame goes to a file). Both read the accumulated image of this context and
 * divide by wfpt_accumulated_samples. Rows are written top to bottom as stored (pixel_idx = x + y*width).
 *   wfpt_save_ppm: binary P6, 8-bit, sqrt(acc / n) exactly like display_shader.wgsl:50-52.
 *   wfpt_save_pfm: binary PF, linear f32 acc / n (PFM stores rows bottom-up, so rows are flipped on write).
 *   (wfpt_save_png below.) Contexts created with tile sharding hold only their own bands and are refused. */
int wfpt_save_ppm(wfpt_ctx *ctx, const char *path);
int wfpt_save_pfm(wfpt_ctx *ctx, const char *path);
/*   wfpt_save_png: the same 8-bit image as wfpt_save_ppm as a PNG (rows in deflate "stored" blocks: no compression library).
 *   wfpt_write_png_rgb8: the writer itself, for any width x height RGB8 buffer (e.g. wfpt_tonemap_rgb8 of a gathered frame). */
int wfpt_save_png(wfpt_ctx *ctx, const char *path);
int wfpt_write_png_rgb8(const char *path, const uint8_t *rgb, uint32_t width, uint32_t height);

/* ------------------------------------------------------------------ diagnostics */
/* Runs the device math primitives over arrays (op: 0 sqrt(a), 1 a/b, 2 sin(a), 3 cos(a), 4 pow(a,b),
 * 5 f32(u32 bits of a)*2^-32, 6 min(a,b), 7 max(a,b), 8 atan2_(a, b)); used by the parity tests to prove the device
 * arithmetic matches the oracle's bit for bit. */
int wfpt_selftest_math(int device, int op, const float *a, const float *b, float *out, size_t n);
/* Workgroups of the extend kernel that fit one CU when each declares `lds_bytes` of dynamic LDS (occupancy query;
 * negative status on error). Diagnostic for sizing the LDS-resident scene. */
int wfpt_debug_extend_blocks_per_cu(int device, uint32_t lds_bytes);
/* Diagnostic builds only (-DWFPT_STAMPS=1): per-phase shader-cycle sums of the middle bounce launches; zeros otherwise. */
int wfpt_debug_read_stamps(wfpt_ctx *ctx, uint64_t out[16], int reset);
/* ... and of the refill traversal's launches (scenes beyond LDS): which = 1 the first launch, 2 the middle launches (0: the call above);
 * which = 3: the first fused launch of an LDS-resident scene */
int wfpt_debug_read_stamps_ex(wfpt_ctx *ctx, int which, uint64_t out[16], int reset);
/* Host-side check of the four-wide quantised tree the device walks for scenes beyond LDS (no GPU needed): collapses
 * `nodes` and verifies that every quantised child box encloses the binary node's box and that the two trees have the
 * same leaves. counts = {four-wide nodes, depth, leaf children, inner children}. */
int wfpt_debug_bvh4(const wfpt_bvh_node *nodes, uint32_t n_nodes, uint32_t counts[4]);
/* ------------------------------------------------------------------ Tile lists
 * A wave of the first fused launch traces the 64 primary rays of one 8x8 pixel tile: one lens, one small patch of the focus plane, the
 * same for every sample while the camera stands. WFPT_LOOP_FUSED contexts whose scene lies in LDS and is walked by the default
 * (conservative) traversal therefore keep, per tile, the list of every leaf whose margin-grown box a ray of the tile can reach -- one
 * 64-byte record: WFPT_TILE_LIST_CAP words `left_first | prim_count << 16` in ascending node order, the rest 0; word 0 =
 * WFPT_TILE_NO_LIST where the tile has more candidates or the camera is one the bound does not cover -- and the first launch tests the
 * listed leaves' primitives instead of walking the tree from the root (no list: it walks, as every other context does). The results are
 * bit for bit those of the walk (a superset of what the reference tests, the verdict on the final hit's leaf, the
 * hand-over to the reference's own walk). wfpt_create, wfpt_update_render_parameters and every change of the scene leave every tile
 * without a list; the table is built on the device before the SECOND batch rendered since (a camera that moves before every frame never
 * pays for a table it would use once). WFPT_FLAG_NO_TILE_LISTS turns it off.
 *   wfpt_tile_lists_host: the same table computed on the host (no GPU needed), record for record. nodes_ch: 8 floats per node as
 *     wfpt_debug_nodes_ch writes them; n_tiles = ceil(width / 8) * (the 8-row bands k with k % tile_world == tile_rank).
 *   wfpt_debug_nodes_ch: the margin-grown (centre | left_first), (half-extent | prim_count) boxes a context of this tree and camera
 *     walks; WFPT_ERR_UNSUPPORTED where a box is not finite (such a context walks the reference's boxes and keeps no lists).
 *   wfpt_debug_read_tile_lists: the context's table (blocking; builds it at once if it is not built). *n_tiles: in, the records `records`
 *     holds; out, the context's tiles -- 0 when the context keeps no lists, and nothing is written then (nor with records == NULL: the
 *     count alone).
 *   wfpt_tile_lists_timing_ms: the device time of the last build and the builds since wfpt_create (blocking). */
#define WFPT_TILE_LIST_CAP 16u
#define WFPT_TILE_NO_LIST 0xffffffffu
int wfpt_tile_lists_host(const float *nodes_ch, uint32_t n_nodes, const wfpt_gpu_camera *camera, const float inv_proj[16], const float view[16],
                         uint32_t width, uint32_t height, uint32_t tile_rank, uint32_t tile_world, uint32_t *records, uint32_t n_tiles);
int wfpt_debug_nodes_ch(const wfpt_bvh_node *nodes, uint32_t n_nodes, const wfpt_gpu_camera *camera, float *nodes_ch);
int wfpt_debug_read_tile_lists(wfpt_ctx *ctx, uint32_t *records, uint32_t *n_tiles);
int wfpt_tile_lists_timing_ms(wfpt_ctx *ctx, float *ms_last, uint32_t *builds);
/* Static facts about the built library, e.g. "gfx950;chunk=512;..." */
const char *wfpt_build_info(void);

#ifdef __cplusplus
}
#endif
#endif /* WFPT_H */
