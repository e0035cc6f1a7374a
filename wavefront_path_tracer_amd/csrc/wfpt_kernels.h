// wfpt_kernels.h -- device-side data layout and kernel launchers shared by wfpt_kernels.hip (kernels)
// and wfpt_api.hip (context, C ABI). Internal; the public surface is include/wfpt.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "wfpt.h"
#include "wfpt_bvh4.h"
#include "wfpt_device_math.h"
#include "wfpt_first_schedule.h"
#include "wfpt_ticket_chunks.h"
#include "wfpt_tile_lists.h"

namespace wfpt {

// A ray queue is cut into segments of kChunk consecutive slots. One extend workgroup traces one
// segment at a time and leaves that segment's hits and misses compacted (stable) at the front of the
// matching segment of the hit / miss queues; a one-workgroup scan then turns the per-segment counts
// into global queue positions. See DESIGN.md "Queues".
#ifndef WFPT_CHUNK
#define WFPT_CHUNK 512 // rays per queue segment = threads of an extend workgroup (tuning builds: 256 / 512 / 1024)
#endif
constexpr int kChunk = WFPT_CHUNK;
constexpr int kExtendThreads = kChunk;
constexpr int kExtendWaves = kExtendThreads / 64;
#ifndef WFPT_CONSUMER_THREADS
#define WFPT_CONSUMER_THREADS 256
#endif
constexpr int kConsumerThreads = WFPT_CONSUMER_THREADS;
constexpr int kScanThreads = 1024;
constexpr int kMaxRows = 64;       // per-bounce table rows kept on the device
constexpr int kMaxTrailDepth = 63; // traversal keeps one pending bit per tree level in a u64
constexpr int kMaxBatch = 128;     // samples kept in flight by one launch of the device-resident loop (fused bounce launches)
constexpr int kClsMax = 8;         // cost classes of the class-binned fused loop (Control::cls_n)
constexpr int kMaxBatchClassic = 64; // ... by the stage kernels one by one (WFPT_FLAG_UNFUSED / WFPT_FLAG_SPLIT_SHADE): their LDS tables are per sample

// SoA ray queue: 28 B per ray (origin, direction, pixel); inverse direction is recomputed. The seven planes of a
// slice sit `cap` elements apart behind one base pointer (3 SGPRs per queue in a kernel instead of 14).
// An element count that fits 32 bits but is used in 64-bit address arithmetic: kept as ONE scalar register in the kernels' argument
// blocks (a size_t costs two, and the fused kernels spill scalar registers to vector lanes), widened where it is used.
struct Stride32 {
    uint32_t v;
    __host__ __device__ operator size_t() const { return v; }
    __host__ __device__ Stride32 &operator=(size_t x) { v = static_cast<uint32_t>(x); return *this; }
};

struct RayQueue {
    float *base;
    uint32_t cap;
    __host__ __device__ float *ox() const { return base; }
    __host__ __device__ float *oy() const { return base + cap; }
    __host__ __device__ float *oz() const { return base + 2u * static_cast<size_t>(cap); }
    __host__ __device__ float *dx() const { return base + 3u * static_cast<size_t>(cap); }
    __host__ __device__ float *dy() const { return base + 4u * static_cast<size_t>(cap); }
    __host__ __device__ float *dz() const { return base + 5u * static_cast<size_t>(cap); }
    __host__ __device__ uint32_t *pixel() const { return reinterpret_cast<uint32_t *>(base + 6u * static_cast<size_t>(cap)); }
};

// Hit queue (12 B per hit: t, primitive, ray index) and miss queue (12 B per miss: ray index, direction.y, pixel),
// segment-compacted. Three planes `plane` elements apart behind one base pointer each.
struct HitQueue {
    uint32_t *base;
    Stride32 plane; // elements between planes (= samples in flight * capacity)
    __host__ __device__ float *t() const { return reinterpret_cast<float *>(base); }
    __host__ __device__ uint32_t *prim() const { return base + static_cast<size_t>(plane); }
    __host__ __device__ uint32_t *ridx() const { return base + 2u * static_cast<size_t>(plane); }
};
// WFPT_FLAG_ENVIRONMENT contexts allocate two more planes, direction.x and direction.z (the map is looked up in the full direction); the
// environment variants of the kernels write and read them, the others never touch them.
struct MissQueue {
    uint32_t *base;
    Stride32 plane;
    __host__ __device__ uint32_t *ridx() const { return base; }
    __host__ __device__ float *dy() const { return reinterpret_cast<float *>(base + static_cast<size_t>(plane)); }
    __host__ __device__ uint32_t *pixel() const { return base + 2u * static_cast<size_t>(plane); }
    __host__ __device__ float *dx() const { return reinterpret_cast<float *>(base + 3u * static_cast<size_t>(plane)); }
    __host__ __device__ float *dz() const { return reinterpret_cast<float *>(base + 4u * static_cast<size_t>(plane)); }
};
constexpr uint32_t kMissPlanes = 3, kMissPlanesEnv = 5;

// The environment map a miss is lit by (WFPT_FLAG_ENVIRONMENT, include/wfpt.h "Environment map"): w x h float4 texels (rgb, 0), row 0 = +y.
// Passed by value as the last argument of the environment variants of the kernels (a captured graph bakes it in: setting a map drops them).
struct EnvDev {
    const float4 *texels;
    uint32_t w, h;
    float intensity, rotation;
};

// Surface textures (WFPT_FLAG_TEXTURES, include/wfpt.h "Textures"), as the texture pass and the AOV kernel read them: the per-primitive table
// the host resolves from the bindings, the scene and the UV table -- {texture slot or kNoTexture, UV row} -- the WFPT_MAX_TEXTURES
// descriptors (TexDev, wfpt_device_math.h) and the UV rows (u0 v0 u1 v1 u2 v2; null = (0, 0) at every corner). Passed by value (a captured
// graph bakes it in: every change drops the graphs).
constexpr uint32_t kNoTexture = 0xffffffffu;
struct TexScene {
    const uint2 *prim_tex;
    const TexDev *tex;
    const float *uv6;
};

// Device-resident control block. `counters` is the reference's counter_buffer (extend.wgsl:41).
struct Control {
    uint32_t counters[16];
    wfpt_frame_buffer frame;
    uint32_t n_in;       // rays the next fused extend traces
    uint32_t seg_n;      // rays the last extend traced (segments the consumers walk)
    uint32_t hits;       // totals of the last extend
    uint32_t misses;
    uint32_t shade_n;    // fused loop: hits to shade (0 once the loop has exited)
    uint32_t miss_n;     // fused loop: misses to shade
    uint32_t shade_gx;   // x extent of workgroup_size_64(hits): the dispatch shape shade.wgsl:72 keys its RNG on
    uint32_t done;       // fused loop exited (path_tracer.rs:332)
    uint32_t ticket;     // extend's dynamic segment ticket
    uint32_t bounce;     // rows written this sample
    uint32_t samples;    // fused samples accumulated
    uint32_t _pad;
    // class-binned fused loop (bounce_binned_kernel): hits of the last extend per cost class (0 once the loop has
    // exited), the segments that extend wrote, and the segments the next one will write (= its hit work items)
    uint32_t cls_n[kClsMax];
    uint32_t n_segs, next_segs, _pad2[2];
    uint32_t rows[kMaxRows][4]; // (rays_in, hits, misses, shaded) per bounce of the current sample
    unsigned long long totals[4]; // rays traced, hits, misses, samples
    unsigned long long wave_totals[kMaxRows][3]; // per wavefront, over all fused samples: rays traced, hits, misses
};

// What shade needs to know about a primitive, merged into one 48-byte record (three float4) so that one
// gather replaces the reference's dependent sphere -> material look-ups (shade.wgsl:80-84):
// v = sphere centre, or for a triangle its unit normal normalize(cross(e1, e2)) (computed once on the host
// with the same operation order the oracle uses per hit).
struct ShadeRec {
    float v[3];
    float fuzz;
    float albedo[3];
    float refract_index;
    uint32_t mat_type;
    uint32_t cost_class; // class-binned loop: 0 = the scene's dominant primitive, 1 + material class otherwise (upload_scene)
    uint32_t _pad[2];
};

struct SceneDev {
    const wfpt_bvh_node *nodes;   // reference layout, 32 B
    const float4 *prim_geom;      // spheres: (cx, cy, cz, r), 16 B each; triangles: the wfpt_triangle array, 3 x 16 B each
    const uint16_t *pair_parent;  // LDS variant: parent node of the sibling pair (2k, 2k+1); padded to 8 entries
    const uint32_t *pair_parent32; // HBM variant: same table, 32-bit
    const wfpt_sphere *spheres;   // reference layout (shade reads material_idx / material_type)
    const wfpt_triangle *triangles;
    const wfpt_material *materials;
    const float4 *shade_rec;      // ShadeRec per primitive, as 3 x float4
    uint32_t n_nodes, n_spheres, n_materials; // n_spheres = primitive count
    uint32_t prim_kind;           // 0 spheres (the reference), 1 triangles (build extension)
    uint32_t lds_scene;           // 1: nodes + primitives + parents are staged in LDS by extend
    uint32_t lds_bytes;           // dynamic LDS the extend kernel needs for this scene
    uint32_t depth;               // levels below the root (validated <= kMaxTrailDepth)
    // HBM-resident scenes: the binary tree collapsed into four-wide nodes (64-byte quantised nodes); null = walk
    // the binary tree. Stack entries beyond the LDS column spill to `stack_spill`, entry k of global thread g at
    // [k * spill_stride + g].
    const float4 *nodes4;
    uint32_t tile_n;              // nodes4[0 .. tile_n) = the top of the tree (breadth-first numbering), staged in LDS by refill_kernel
    uint32_t *stack_spill;
    uint32_t spill_stride;
    // LDS-resident scenes, default traversal: every node as (centre.xyz | left_first), (half-extent.xyz | prim_count), the
    // half-extent grown by more than the box test's rounding error (trace_ray_conservative); staged instead of `nodes`
    const float4 *nodes_ch;
    float safe_c[3], safe_r2; // free walks: origins within sqrt(safe_r2) of safe_c are covered by the margin's bound (far_origin)
    uint32_t exact; // 1: WFPT_FLAG_EXACT_TRAVERSAL (or a fallback to it): the reference's box test and 1e30 miss value
    uint32_t root_leaf; // the root is a leaf: its box is never tested (ex:84), so neither is it by the leaf-box test of the free walks
};

constexpr uint32_t kStack4Lds = 8;  // stack entries of the four-wide traversal kept in LDS per lane (0.3 % of the pushes go deeper: they spill)
constexpr uint32_t kTileNodesMax = 341; // four-wide nodes staged in LDS by the refill traversal: five full levels (1 + 4 + 16 + 64 + 256), 21.8 KB

struct CameraDev {
    wfpt_gpu_camera cam;
    float inv_proj[16];
    float view[16];
};

struct Tiling {
    uint32_t rank, world; // this context owns 8-row bands k with k % world == rank
};

// Sample batching. One launch serves `n` independent samples (frames f0, f0+1, ...): every per-sample
// buffer is an array of `n` identically laid out slices, `*_stride` elements apart. Sample s keeps its
// own queues, counts and Control block, so results are exactly those of n sequential samples.
struct Batch {
    uint32_t n;            // samples in this launch (1 for the stage API)
    uint32_t ctl_stride;   // u32 words between Control blocks
    Stride32 ray_stride;   // floats between ray-queue slices (7 * capacity)
    Stride32 queue_stride; // elements between hit / miss queue slices (capacity)
    Stride32 chunk_stride; // elements between per-segment count arrays
    Stride32 image_stride; // floats between image slices (a slice holds one float4 per pixel)
};

struct GenerateArgs {
    Batch batch;
    RayQueue q;
    float *image;            // reset to 1 when reset_image != 0
    Control *ctl;            // frame uniform; fused loop: n_in <- rays generated
    const CameraDev *camera;
    uint32_t gx, gy;         // dispatch (gy counts this rank's bands)
    uint32_t true_size;      // 0: width/height = 8*gx, 8*gy (generate_rays.wgsl:55-56); 1: from the frame uniform
    uint32_t reset_image;
    uint32_t set_n_in;       // fused loop: ctl->n_in = gx*gy*64 (pt:313-316)
    uint32_t capacity;
    Tiling tile;
};

struct ExtendArgs {
    Batch batch;
    RayQueue q;
    HitQueue hq;
    MissQueue mq;         // payload: direction.y and pixel of the missing ray, so miss_kernel needs no gather
    uint32_t *chunk_hits, *chunk_miss;
    // Beside the reference's hit queue (t, primitive, ray index: what wfpt_read_hits returns) extend leaves the path record the fused loop
    // carries -- (hit point | pixel), (incoming direction | primitive), two float4 at the hit's slot -- so that shade STREAMS 32 bytes per hit
    // instead of gathering seven planes of the ray queue through the ray index (round 5; null = not written)
    float4 *rec_out;
    Control *ctl;
    const uint32_t *n_in; // rays to trace = min(*n_in, limit)
    uint32_t limit;
    uint32_t has_inactive; // ray queue may hold WFPT_INACTIVE_PIXEL padding rays
    // per-material partition of each segment's hits (README.md:19 "split shade into by-material shade kernels"):
    // list m of segment c holds, ascending, the in-segment ranks of its hits with material_type m
    uint32_t partition;
    uint16_t *mat_list;      // [3][batch][capacity]
    uint32_t *chunk_mat;     // [3][batch][segments]
    size_t mat_list_mstride; // elements between materials
    size_t chunk_mat_mstride;
    SceneDev scene;
};

struct ScanArgs {
    Batch batch;
    const uint32_t *chunk_hits, *chunk_miss;
    uint32_t *chunk_hit_base, *chunk_miss_base;
    Control *ctl;
    const uint32_t *n_in;
    uint32_t limit;
    uint32_t *first_seg; // fused bounce kernel: first_seg[s] = segment that holds hit 512*s (may be null)
    uint32_t fused;      // 1: drive the device-resident loop; 0: stage API (counters protocol only)
    uint32_t miss_floor;
    uint32_t bounce;
};

// ---- fused bounce kernel of the device-resident loop (DESIGN.md "The loop"): one launch per wavefront does
//   shade(hit of wavefront b-1) -> extend(the extension ray, straight from registers) -> compaction,
// plus miss_kernel for wavefront b-1's misses. The wavefront's queue IS the hit queue: a *path record* is the hit
// (point, incoming direction, primitive, pixel), 32 B as two float4, segment-compacted like the hit queue.
constexpr int kBounceFirst = 0;  // generate_rays -> extend                 (wavefront 0)
constexpr int kBounceMiddle = 1; // shade -> extend, miss_kernel            (wavefronts 1 .. max-1)
constexpr int kBounceLast = 2;   // shade (throughput only), miss_kernel    (after the last extend)
constexpr int kBounceMiddleRetire = 3; // kBounceMiddle of a WFPT_FLAG_RETIRE context: shade ends with the termination step, a retired hit is not traced
constexpr int kBounceFirstMasked = 4;  // kBounceFirst of a WFPT_FLAG_ADAPTIVE context: a lane whose bit of its tile's mask word is clear generates no ray
// The termination step's inputs (include/wfpt.h "Path termination"): the wavefront b whose hits the shade step shades and the context's
// wfpt_termination_params. Read by the WFPT_FLAG_RETIRE kernels alone.
struct TermArgs {
    uint32_t wavefront, roulette_start;
    float q_min;
};
#ifndef WFPT_MISS_SEGS
#define WFPT_MISS_SEGS 16
#endif
constexpr int kMissSegsPerItem = WFPT_MISS_SEGS; // miss work item = this many input segments
#ifndef WFPT_MISS_EVERY
#define WFPT_MISS_EVERY 0
#endif
constexpr uint32_t kMissEvery = WFPT_MISS_EVERY; // fused bounce launches: every kMissEvery-th ticket is a miss item while both kinds are left; 0 = hit items / miss items + 1, per launch
#ifndef WFPT_FIRST_STATIC_SHARE_NUM
#define WFPT_FIRST_STATIC_SHARE_NUM 0
#endif
#ifndef WFPT_FIRST_STATIC_SHARE_DEN
#define WFPT_FIRST_STATIC_SHARE_DEN 2
#endif
// bounce_kernel<kBounceFirst>: the share of its items that the workgroups take without a ticket (wfpt_first_schedule.h); 0 = every item by ticket.
// 1/2 was the best of the sweep 0 .. 1 while every other item cost a draw (profiles/r07_first_schedule_ab.txt); since a draw buys a chunk
// (below) share 0 is the fastest at every chunk length (profiles/r09_chunk_schedule_ab.txt) and ships: the whole launch is handed out dynamically
constexpr uint32_t kFirstStaticNum = WFPT_FIRST_STATIC_SHARE_NUM, kFirstStaticDen = WFPT_FIRST_STATIC_SHARE_DEN;
static_assert(kFirstStaticDen > 0 && kFirstStaticNum <= kFirstStaticDen, "the static share of the first launch's items lies in [0, 1]");
#ifndef WFPT_FIRST_CHUNK
#define WFPT_FIRST_CHUNK 4
#endif
#ifndef WFPT_FIRST_TAIL_ROUNDS
#define WFPT_FIRST_TAIL_ROUNDS 4
#endif
#ifndef WFPT_BOUNCE_CHUNK
#define WFPT_BOUNCE_CHUNK 4
#endif
#ifndef WFPT_BOUNCE_TAIL_ROUNDS
#define WFPT_BOUNCE_TAIL_ROUNDS 4
#endif
// What one draw from Control::ticket buys (wfpt_ticket_chunks.h): a chunk of this many consecutive positions, but for the last
// `tail rounds` positions per workgroup, which go out singly. The first launch applies it to the items behind its static range, the
// middle and last launches to their tickets (before TicketMap). 1 = one position per draw, the launches as they were up to round 8.
// 4 and 4 tail rounds are the best of the sweeps for both (profiles/r09_chunk_schedule_ab.txt); the tail rounds hardly matter (2, 4, 8 alike).
constexpr uint32_t kFirstChunk = WFPT_FIRST_CHUNK, kFirstTailRounds = WFPT_FIRST_TAIL_ROUNDS;
constexpr uint32_t kBounceChunk = WFPT_BOUNCE_CHUNK, kBounceTailRounds = WFPT_BOUNCE_TAIL_ROUNDS;
static_assert(kFirstChunk >= 1 && kBounceChunk >= 1, "a draw buys at least one position");

struct BounceArgs {
    Batch batch;
    unsigned long long *stamps; // diagnostic builds (-DWFPT_STAMPS=1): per-phase wave-cycle sums, see wfpt_debug_read_stamps
    const float4 *rec_in;   // [batch][capacity][2]: (p.xyz | pixel), (d.xyz | prim) of the previous wavefront's hits
    float4 *rec_out;
    const uint32_t *in_hits, *in_hit_base, *in_miss; // per-segment counts / bases of the previous wavefront (scan's output)
    const uint32_t *in_first_seg;                    // segment holding hit 512*s, per output segment s (scan's output)
    uint32_t *out_hits, *out_miss;                   // per-segment counts of this wavefront
    MissQueue mq_in, mq_out;                         // (dy, pixel) payload of the misses; the ridx plane is unused here
    float *image;
    Control *ctl;
    const CameraDev *camera;
    uint32_t gx, gy;       // first wavefront: tiles of this context (gy counts this rank's bands)
    uint32_t capacity;
    uint32_t rng_mode;
    uint32_t image_width;
    Tiling tile;
    SceneDev scene;
    // ---- class-binned loop (bounce_binned_kernel; WFPT_RNG_PIXEL only, where the order of the queue is free): the hits of a segment are
    // stored sorted by COST CLASS (ShadeRec::cost_class of the primitive hit), and a work item of the next launch is kChunk hits of ONE
    // class (of one sample), found through the per-class tables the scan leaves.
    const uint32_t *plan;           // [n * K + 1] first hit item of each (sample, class) | [n + 1] first segment item of each sample | [n + 1] first miss item
    uint32_t plan_seg_off, plan_miss_off;
    const uint2 *cls_table;         // in:  [n][segments][K] {class-k hits before this segment, first slot of the segment's class-k run}
    const uint32_t *first_seg_cls;  // in:  [n][K][segments]: segment that holds class-k hit number kChunk * run
    uint32_t *out_cls;              // out: [n][segments][words] per-segment class totals, packed 10 bits each (ClsPack)
    // ---- first launch of WFPT_LOOP_FUSED over a scene in LDS, default walk: the per-tile candidate lists (wfpt_tile_lists.h), one
    // 64-byte record per local tile; null = every wave walks the tree
    const uint4 *tile_lists;
    TermArgs term; // kBounceMiddleRetire (appended: the offsets of everything above are those of the launches that do not read it)
    const uint64_t *mask; // kBounceFirstMasked (appended likewise): one word per 8x8 tile of generate_rays' numbering, [capacity / 64]
};

// The builder of the per-tile candidate lists (tile_lists_kernel): one wave per local tile, lanes over the nodes
struct TileListArgs {
    const float4 *nodes_ch;
    uint32_t n_nodes;
    const CameraDev *camera;
    uint32_t gx, gy;       // tiles of this context (gy counts this rank's bands)
    uint32_t width, height;
    Tiling tile;
    uint32_t *records;     // [gx * gy][kTileListCap]
};

// Packed counters of the class-binned compaction: field f of a word array sits in word f / 3 at bit 10 * (f % 3); a field holds at most
// kChunk = 512 < 1024, so packed words add without carries between fields. Fields 0 .. K-1: hits per class, K: misses, K + 1: all hits.
template <int K> struct ClsPack {
    static constexpr int kFields = K + 2, kWords = (kFields + 2) / 3;
};
constexpr int kBinClasses = 4; // classes of the binned loop: 0 = the dominant primitive (the Shirley scene's ground), 1 + material type otherwise
static_assert(kBinClasses <= kClsMax && kChunk <= 1023, "a packed field must hold a segment's count");

struct ScanBinnedArgs {
    Batch batch;
    const uint32_t *chunk_hits, *chunk_miss, *chunk_cls; // per-segment totals of this wavefront (chunk_cls: ClsPack words)
    uint2 *cls_table;
    uint32_t *first_seg_cls;
    Control *ctl;
    const uint32_t *n_in;
    uint32_t limit, miss_floor, bounce;
};

struct PlanArgs {
    Batch batch;
    const Control *ctl;
    uint32_t *plan;
    uint32_t plan_seg_off, plan_miss_off;
    uint32_t last; // 1: the next launch is the last one (shade without extend): its hit items are whole segments
};

// ---- HBM-resident scenes: traversal with dynamic lane refill. Rays of such scenes take very
// different numbers of steps (1M-triangle soup: mean 188, p99 650), so a wave that keeps its 64 rays until the longest one
// ends runs at 13-17 % lane utilisation. Here every wave is an independent worker: a lane that finishes its ray takes
// the next ray index from a global cursor (in groups, one atomic per group), reads the ray that generate_dense_kernel or
// shade_rays_kernel left at full waves in a DENSE per-ray array, and traces it. Results go to the same array; `compact_kernel`
// then builds the segment-compacted path-record / miss queues in ray order, so everything downstream (scan, RNG keying by
// queue position, the next wavefront) sees exactly the queues the fused bounce kernel would have written.
constexpr uint32_t kDenseMiss = 0xffffffffu, kDenseInactive = 0xfffffffeu; // primitive word of a dense record that is not a hit
#ifndef WFPT_TICKET_BLOCK
#define WFPT_TICKET_BLOCK 64
#endif
constexpr uint32_t kTicketBlock = WFPT_TICKET_BLOCK; // ray indices a wave of the refill traversal reserves per atomic
// refill when at least this many lanes of a wave are idle: a refill reads a ready ray, so waves refill early
#ifndef WFPT_REFILL_IDLE_PRESHADED
#define WFPT_REFILL_IDLE_PRESHADED 24 // middle wavefronts: extension rays from shade_rays_kernel
#endif
#ifndef WFPT_REFILL_IDLE_FIRST_PRE
#define WFPT_REFILL_IDLE_FIRST_PRE 16 // first wavefront: primary rays from generate_dense_kernel
#endif
constexpr uint32_t kRefillIdlePreshaded = WFPT_REFILL_IDLE_PRESHADED, kRefillIdleFirstPre = WFPT_REFILL_IDLE_FIRST_PRE;

struct RefillArgs {
    Batch batch;
    unsigned long long *stamps; // diagnostic builds (-DWFPT_STAMPS=1): 16 counters per launch kind, see wfpt_debug_read_stamps_ex
    const float4 *rec_in;  // compact hit records of the previous wavefront
    float4 *dense_out;     // [batch][capacity][2]: (p | pixel), (d | prim or kDenseMiss / kDenseInactive), indexed by ray
    const uint32_t *in_hits, *in_hit_base, *in_first_seg;
    float *image;
    Control *ctl;
    const CameraDev *camera;
    uint32_t gx, gy, capacity, rng_mode, image_width;
    Tiling tile;
    SceneDev scene;
    TermArgs term; // shade_rays_retire_kernel (appended, as in BounceArgs)
};

struct CompactArgs {
    Batch batch;
    const float4 *dense_in;
    float4 *rec_out;
    MissQueue mq_out;
    uint32_t *out_hits, *out_miss;
    const Control *ctl; // n_in = rays of this wavefront
    uint32_t capacity;
};

struct ShadeArgs {
    Batch batch;
    RayQueue q, ext;
    HitQueue hq;
    const uint32_t *chunk_hits, *chunk_hit_base;
    const float4 *rec_in;   // extend's path records of these hits (ExtendArgs::rec_out); null = gather the ray through hq.ridx() as shade.wgsl:76-78 does
    float *image;
    Control *ctl;
    const uint32_t *n_hits; // hits to shade = min(*n_hits, limit)
    uint32_t limit;
    uint32_t gx;            // stage API: the host's dispatch x extent; 0: use ctl->shade_gx
    uint32_t rng_mode;
    uint32_t material;      // split != 0: 0/1/2 = walk only that material's lists, 0xffffffff = blockIdx.z picks
    uint32_t split;         // walk the per-material lists instead of the whole hit queue
    const uint16_t *mat_list;
    const uint32_t *chunk_mat;
    size_t mat_list_mstride, chunk_mat_mstride;
    uint32_t count_out;     // stage API: counters[2] += rays emitted (sh:155)
    uint32_t image_width;   // for the tile mapping
    SceneDev scene;
    Tiling tile;
};

struct MissArgs {
    Batch batch;
    RayQueue q;
    MissQueue mq;
    const uint32_t *chunk_miss, *chunk_miss_base;
    float *image;
    const Control *ctl;
    const uint32_t *n_miss;
    uint32_t limit;
    uint32_t image_width;
    Tiling tile;
};

// The hits a shade step will shade, as the passes that precede the step walk them (for_each_shaded_hit). Two forms, as the shade steps read
// their hits:
//   records (rec_in != null): the fused loops' path records of the previous wavefront -- segment c holds in_hits[c] records, its first one
//            shade's hit in_hit_base[c]; the hits shaded are h < ctl->shade_n (0 once the loop has exited), as bounce_kernel and
//            shade_rays_kernel shade them;
//   queues  (rec_in == null): shade_kernel's hit queue (t, primitive, ray index) and ray queue: hits h < min(*n_hits, limit), of material
//            class `material` only unless it is 0xffffffff (the per-material shade stages).
struct HitWalk {
    Batch batch;
    const float4 *rec_in;
    const uint32_t *in_hits, *in_hit_base;
    RayQueue q;
    HitQueue hq;
    const uint32_t *n_hits;
    uint32_t limit;
    uint32_t material;
    uint32_t capacity;
    float *image;
    const Control *ctl;
    uint32_t image_width;
    Tiling tile;
    const float4 *shade_rec;  // spheres: the centre; the material class (the per-material shade stages' filter)
};

// The texture pass (texture_kernel): before a shade step, the throughput of every hit that step will shade is multiplied by the texture of
// the primitive hit, so that shade's own `*= albedo` makes (thr * tex) * albedo.
struct TextureArgs {
    HitWalk w;
    const float4 *prim_geom;  // triangles: the wfpt_triangle array (v0, e1, e2)
    uint32_t prim_kind;
    TexScene ts;
};

// The emission pass (emission_kernel; WFPT_FLAG_EMISSION, include/wfpt.h "Emission"): before a shade step -- and after that step's texture
// pass -- every hit the step will shade that lies on an emitter adds thr * e to the pixel's `emitted` and leaves thr = +0 (one multiply and
// one add per channel, no fma); shade then scatters the dead path as any other. It reads no hit point: the pixel and the primitive only.
// The table: prim_em[primitive] is the primitive's material_idx when that material emits and kNoEmission otherwise, in the order the
// device holds the primitives, and em[material_idx] its colour (w unused). An index per primitive rather than a float4: the pass reads
// 4 bytes for every hit and the colour for emitter hits only, out of a table of a few materials that stays in cache.
// The kernel's three kinds (launch_emission):
//   kEmitAll:     the contexts that do not connect;
//   kEmitGated:   the contexts that connect (WFPT_FLAG_NEE with an emitter, or WFPT_FLAG_ENV_NEE): thr * e is added only where the pixel's
//                 connected flag (emitted.w, set by the previous step's connect pass) is 0 -- after a diffuse bounce the connect pass
//                 has already counted this light;
//   kEmitWeighed: the contexts that connect and weigh (WFPT_FLAG_MIS with an emitter): where the flag is 1 the hit is not dropped but adds
//                 (thr * e) * wb (mis_hit_weight: the distance comes from `origin`, the scatter's density from the length of the ray's
//                 direction). The extra loads happen per hit on an emitter after a diffuse bounce only. The last four fields are its alone.
//   kEmitWeighedEnv: the contexts that weigh their map as well (WFPT_FLAG_ENV_MIS with a distribution and an emitter; include/wfpt.h
//                 "Environment multiple importance sampling"): kEmitWeighed with the light list's density scaled by the share of the
//                 connect samples that go to it, plq = pl * q. Its own kernel, emission_weighed_env_kernel, which takes q as a second
//                 argument: EmissionArgs, and with it the three kernels above, stay as they are.
constexpr uint32_t kNoEmission = 0xffffffffu;
//   kEmitWeighedPower: the weighing contexts whose light list has a distribution (WFPT_FLAG_LIGHT_POWER with WFPT_FLAG_MIS; include/wfpt.h
//                 "Light selection by power"): kEmitWeighed with nfi = f32(total) / f32(prim_k[hit primitive]) in nf's place, and wb = 1
//                 where that k is 0. Its own kernel, emission_weighed_power_kernel, which takes the distribution as a second argument.
enum EmissionKind : int { kEmitAll, kEmitGated, kEmitWeighed, kEmitWeighedEnv, kEmitWeighedPower };
struct EmissionArgs {
    HitWalk w;
    float *emitted;           // the second per-sample plane: image's shape and strides
    const uint32_t *prim_em;
    const float4 *em;
    const float4 *prim_geom;
    const float4 *origin;     // the hit points the previous step's MIS connect pass stored: `emitted`'s shape and strides
    uint32_t prim_kind;
    float nf;                 // f32(n_lights)
};

// The environment map as a light (WFPT_FLAG_ENV_NEE, include/wfpt.h "Environment next-event estimation"): the map and its sampling
// distribution. row[y * w + x]: the inclusive prefix sum of the integer texel weights k along row y; marg[y]: the inclusive prefix sum of
// the row totals; total = marg[h - 1] > 0; share: the effective probability p with which a diffuse hit picks the map rather than an emitter (1 with no light).
struct EnvDist {
    EnvDev env;
    const uint32_t *row;
    const uint64_t *marg;
    uint64_t total;
    float share;
};

// The light list's sampling distribution (WFPT_FLAG_LIGHT_POWER, include/wfpt.h "Light selection by power"): cdf[i] the inclusive prefix
// sum of the lights' integer weights k in list order, total = cdf[n_lights - 1] > 0, prim_k[primitive] = k of a light and 0 of every other
// primitive. All null / 0 while the list has no distribution.
struct LightDist {
    const uint64_t *cdf;
    const uint32_t *prim_k;
    uint64_t total;
};

// The analytic lights (WFPT_FLAG_ANALYTIC_LIGHTS, include/wfpt.h "Analytic lights"): three float4 rows per light, wfpt_light's own layout --
// (position, type's bits), (direction as stored: normalised, cos_inner), (colour, cos_outer). Null / 0 while the context holds none.
struct LightTable {
    const float4 *rows;
    uint32_t n;
};

// The connect pass (connect_kernel; WFPT_FLAG_NEE, include/wfpt.h "Next-event estimation"): before a shade step, after that step's texture
// and emission passes, every hit the step will shade either sends one shadow ray to a sampled point of a light and adds the unoccluded
// sample to the pixel's `emitted` (a diffuse hit: the pixel's connected flag, emitted.w, becomes 1) or only clears the flag (every other
// hit). It traces with the context's own walk (WFPT_TRACE_ANY), so it carries the scene like the other tracing kernels. `lights`: the
// primitives whose material emits, in primitive order. `wavefront`: the index b of the wavefront whose hits these are (the key of the
// pass's own random stream).
// The sampler form (sample_in != null; wfpt_sample_lights): sample_n rows of (point, normal, u0 u1 u2) instead of hits, one row of
// (q, light primitive, e_q G, occluded) each out; nothing else is read or written.
// The ENVS variants (launch_connect's `envs`; WFPT_FLAG_ENV_NEE contexts whose map has a distribution): a diffuse hit picks the map with
// probability envd.share (always, when n_lights is 0: prim_em may be null then) and an emitter otherwise; their sampler form
// (wfpt_sample_environment_light) takes rows of (point, normal, u1 u2 u3 u4) and answers (wdir, texel, e Genv, occluded) for the map alone.
// The MIS variants (WFPT_FLAG_MIS with an emitter; include/wfpt.h "Multiple importance sampling"): the balance heuristic between shade's
// cosine scatter and the connect pass's area sampling. They weigh their sample by wl and store the hit point of every diffuse hit in
// `origin` (one float4 per pixel per sample in flight, never zeroed: read only where the connected flag is 1, which the same lane set
// with it) for the next step's kEmitWeighed emission pass; their sampler form answers 12 floats a row (wfpt_sample_lights_mis).
// The ENVS MIS variants (WFPT_FLAG_ENV_MIS contexts whose map has a distribution; include/wfpt.h "Environment multiple importance
// sampling"): the ENVS variants with both branches weighed against the scatter -- the map's sample by we = pe / (pe + pb), pe = pdf * p,
// an emitter's by wl = plq / (plq + pb), plq = pl * (1 - p) -- and `origin` stored as the MIS variants do, for the kEmitWeighedEnv emission
// pass and for nothing else (miss_env_mis_kernel takes pb from the miss's own direction). Their sampler form
// (wfpt_sample_environment_light_mis) answers 12 floats a row with the effective share p.
// The POWER variants (WFPT_FLAG_LIGHT_POWER contexts whose list has a distribution; never with ENVS): the light is selected by a binary
// search of the distribution's cdf and weighed by nfi = f32(total) / f32(k) wherever nf stands; with and without MIS, render and sampler
// forms alike. Their kernels (connect_power_kernel) take the LightDist as a second argument: ConnectArgs, and with it the kernels above, stay
// as they are.
// The ANALYTIC variants (WFPT_FLAG_ANALYTIC_LIGHTS contexts that hold an analytic light; never with ENVS or POWER; include/wfpt.h
// "Analytic lights"): the selection runs over the emitters followed by the analytic lights, N = n_lights + n, and Nf = f32(N) stands
// wherever nf does; an index past the emitters evaluates a point, spot or directional light with no area, no cos_l and no texture, and
// under MIS with wl = 1. Their kernels (connect_analytic_kernel) take the LightTable as a second argument: ConnectArgs, and with it the
// kernels above, stay as they are. n_lights may be 0 there (lights, prim_em and em null).
struct ConnectArgs {
    HitWalk w;
    float *emitted;
    uint32_t n_chunks_max;    // segments per sample: the work items are (sample, segment) pairs, sample-major
    uint32_t wavefront;
    const uint32_t *prim_em;
    const float4 *em;
    const uint32_t *lights;
    uint32_t n_lights;
    const float *sample_in;
    float *sample_out;        // the sampler form: the rows out
    uint32_t sample_n;
    float4 *origin;           // the MIS variants' render form: the hit points of the diffuse hits, `emitted`'s shape and strides
    TexScene ts;              // the textures of the lights (the TEX variants only)
    SceneDev scene;
    EnvDist envd;             // the map as a light (the ENVS variants only; below)
};

// wfpt_mis_hit_weight (mis_weight_kernel): mis_hit_weight on caller rows of (o, d, t, primitive)
struct MisArgs {
    const float4 *prim_geom;
    uint32_t prim_kind;
    uint32_t n_prims;
    float nf;                 // f32(n_lights)
};

// The shading-normal pass (shading_normal_kernel; WFPT_FLAG_SHADING_NORMALS contexts that hold a table, include/wfpt.h "Shading normals"):
// the last pass before a shade step that scatters. For every hit the step will shade it forms the shading normal ns (shading_normal) and
// writes the hit's own shade record -- (ns | fuzz), rec1, rec2: the primitive's ShadeRec with ns in the stored normal's place -- at the
// hit's slot of `table` (3 x float4 per queue slot per sample in flight), then overwrites the primitive word of the record the shade step
// streams (rec_out[2 slot + 1].w) with the slot. The shade launch that follows is handed `table` as its scene.shade_rec, so it gathers
// `3 * slot` where it gathered `3 * prim`: shade_kernel, bounce_kernel and shade_rays_kernel run as they are. Nothing reads a record's
// primitive after its shade step (DESIGN.md 9r lists the read sites).
// normals: per PRIMITIVE, in the order the device holds them, three rows (corner normal | 0) -- the caller's table resolved through each
// triangle's _pad on the host (build_normal_rows), so the pass gathers geometry, normals and shade record side by side, none behind another.
struct ShadingArgs {
    HitWalk w;
    const float4 *prim_geom;
    const float4 *normals;
    float4 *table;
    float4 *rec_out;
};

// The microfacet pass (microfacet_kernel; WFPT_FLAG_MICROFACET contexts that hold a roughness above 0, include/wfpt.h "Microfacet metals"):
// it takes the shading-normal pass's place as the last pass before a shade step that scatters, and writes the same per-hit table -- every
// hit's own shade record at its slot, the slot in the primitive word of the record the step streams. At a rough hit the record is
// (m | +0), (F * G1(wo) | rec1.w), rec2: a microfacet normal for the metal branch of scatter() to reflect about and the estimator's weight
// for shade to multiply the throughput by; the shade launch is handed `table` exactly as after the shading-normal pass.
// mf_prim: per PRIMITIVE, in the order the device holds them, its material's roughness alpha where the primitive's material_type is 1
// (Metal) and +0 otherwise: the one 4-byte gather that decides whether a hit samples or only copies.
// normals: the shading-normal pass's per-primitive rows where the context holds a table of corner normals (microfacet_kernel<true>: every
// record carries the shading normal), null otherwise.
struct MicrofacetArgs {
    HitWalk w;
    const float4 *prim_geom;
    const float4 *normals;
    const float *mf_prim;
    float4 *table;
    float4 *rec_out;
    uint32_t wavefront;
};

// Normal maps (WFPT_FLAG_NORMAL_MAPS contexts that hold a binding, include/wfpt.h "Normal maps"), as the kernels of a mapped context read
// them: per PRIMITIVE, in the order the device holds them, {texture slot or kNoTexture, UV row, the strength's bits, 0} -- the bindings
// resolved through each primitive's material_idx and _pad on the host (build_nmap_tables), as TexScene::prim_tex is -- the
// WFPT_MAX_TEXTURES descriptors, the UV rows (null = (0, 0) at every corner) and the shading-normal pass's per-primitive rows of corner
// normals (null = no table is set: ns is the stored normal). Passed by value, as TexScene.
struct NmapScene {
    const uint4 *prim_map;
    const TexDev *tex;
    const float *uv6;
    const float4 *normals;
};

// Roughness maps (WFPT_FLAG_ROUGHNESS_MAPS contexts that hold a roughness above 0 and a binding, include/wfpt.h "Roughness maps"), as the
// record kernels of such a context read them: per PRIMITIVE, in the order the device holds them, {texture slot or kNoTexture, UV row,
// channel | remap << 2, the bits of the material's alpha as MicrofacetArgs::mf_prim holds it} -- the bindings resolved through each
// primitive's material_idx and _pad on the host (build_rmap_tables) --, the normal-map rows of NmapScene::prim_map (null = the context
// is not mapped), the WFPT_MAX_TEXTURES descriptors, the UV rows (null = (0, 0) at every corner) and the shading-normal pass's rows of
// corner normals (null = no table is set). Passed by value, as NmapScene.
struct RmapScene {
    const uint4 *prim_rough;
    const uint4 *prim_map;
    const TexDev *tex;
    const float *uv6;
    const float4 *normals;
};

struct AccumulateArgs {
    Batch batch;
    const float *image;
    float *accumulated;
    Control *ctl;
    uint32_t n_pixels;
    uint32_t bookkeeping; // fused loop: fold the bounce table into totals, frame += 1
};

// ---- adaptive sampling (WFPT_FLAG_ADAPTIVE; include/wfpt.h "Adaptive sampling"). The active mask is one 64-bit word per 8x8 tile of the
// context's slab, indexed by generate_rays' tile index (slot >> 6), bit ly * 8 + lx set = the pixel is rendered; `count` one u32 per pixel
// of the slab, indexed like `accumulated`. What a kernel that walks PIXELS needs to find a pixel's bit:
struct MaskArgs {
    const uint64_t *mask;
    uint32_t *count;
    uint32_t width, tiles_x; // pixel i of the slab: x = i % width, row r = i / width; tile (r / 8) * tiles_x + x / 8, bit (r % 8) * 8 + x % 8
};
__host__ __device__ inline uint32_t mask_tile_of(uint32_t i, uint32_t width, uint32_t tiles_x, uint32_t &bit) {
    const uint32_t r = i / width, x = i - r * width;
    bit = (r & 7u) * 8u + (x & 7u);
    return (r >> 3) * tiles_x + (x >> 3);
}
// wfpt_adaptive_update's criterion for one pixel (adaptive_update_kernel; compiled for the host as well, for the tests of the formula):
// one IEEE f32 operation per step in the header's order. max(0, d) keeps a NaN d, so a NaN anywhere leaves the pixel unconverged.
__host__ __device__ inline bool adaptive_unconverged(float s1, float s2, uint32_t n, uint32_t min_samples, float threshold, float luminance_floor) {
    const float nf = static_cast<float>(n);
    const float mu = s1 / nf;
    const float d = s2 / nf - mu * mu;
    const float v = (d < 0.0f ? 0.0f : d) / nf;
    const float tol = threshold * (mu + luminance_floor);
    return !(n >= min_samples && v <= tol * tol);
}
// one pixel of dilation inside the tile: horizontally, then vertically
__host__ __device__ inline uint64_t dilate_tile(uint64_t u) {
    const uint64_t h = u | ((u << 1) & ~0x0101010101010101ull) | ((u >> 1) & ~0x8080808080808080ull);
    return h | (h << 8) | (h >> 8);
}
struct AdaptiveArgs {
    const float *moments;     // kMomentPlanes planes of `plane`
    Stride32 plane;
    const uint32_t *count;
    uint64_t *mask;           // written: one word per tile
    uint32_t *n_active;       // += the set bits (zeroed by the caller)
    uint32_t gx, gy;          // tiles of this context (gy counts this rank's bands)
    uint32_t width, height;
    Tiling tile;
    uint32_t min_samples, max_samples;
    float threshold, luminance_floor;
    uint32_t dilate;
};
// The mean of a pixel's channel (wfpt_read_mean on the host, mean_resolve_kernel on the device): one IEEE f32 division, 0 where n == 0
__host__ __device__ inline float mean_resolve(float sum, uint32_t n) { return n ? sum / static_cast<float>(n) : 0.0f; }

// ---- first-hit AOVs (WFPT_FLAG_AOV; include/wfpt.h "AOVs"). The per-pixel sums are kAovPlanes planes of `plane` elements (the context's
// pixel capacity) behind one base pointer, indexed by the pixel's slot in this context's slab. All zero = nothing accumulated (the reset state).
// The id planes hold 0 until the first sample since the reset has run, then primitive / material_idx + 1 for a hit, kAovMissWord for a miss.
enum : uint32_t {
    kAovAlbedo = 0,   // 3 planes: sum of the first hit's albedo (rgb), or of the sky colour on a miss
    kAovNormal = 3,   // 3 planes: sum of the first hit's normal (xyz)
    kAovDepth = 6,    // sum of t over the hits
    kAovHits = 7,     // u32: samples that hit
    kAovPrim = 8,     // u32: see above
    kAovMaterial = 9, // u32
    kAovPlanes = 10
};
constexpr uint32_t kAovMissWord = 0xffffffffu;

struct AovArgs {
    uint32_t n;             // samples of this batch: frames ctl->frame.frame + 0 .. n - 1, added in that order
    float *sums;
    Stride32 plane;
    const Control *ctl;     // ctl->frame: the batch's first frame (read on the device: graph replays freeze arguments)
    const CameraDev *camera;
    uint32_t gx, gy;        // tiles of this context (gy counts this rank's bands)
    Tiling tile;
    SceneDev scene;
};

// Resolved element k of AOV `which` (k < channels * pixels) from the sums, n = samples accumulated. Compiled for the host
// (wfpt_read_aov) and the device (aov_resolve_kernel) from this one definition: the same IEEE f32 operations, the same bits.
__host__ __device__ inline uint32_t aov_resolve_word(const float *sums, size_t plane, uint32_t which, size_t k, uint32_t n) {
    auto as_u32 = [](float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; };
    auto word = [&](uint32_t p, size_t px) { return as_u32(sums[p * plane + px]); };
    const float nf = static_cast<float>(n);
    switch (which) {
    case WFPT_AOV_ALBEDO:
    case WFPT_AOV_NORMAL: {
        const uint32_t p = (which == WFPT_AOV_ALBEDO ? kAovAlbedo : kAovNormal) + static_cast<uint32_t>(k % 3u);
        return n ? as_u32(sums[p * plane + k / 3u] / nf) : 0u;
    }
    case WFPT_AOV_DEPTH: {
        const uint32_t hits = word(kAovHits, k);
        return hits ? as_u32(sums[kAovDepth * plane + k] / static_cast<float>(hits)) : 0u;
    }
    case WFPT_AOV_COVERAGE: return n ? as_u32(static_cast<float>(word(kAovHits, k)) / nf) : 0u;
    default: { // ids
        const uint32_t w = word(which == WFPT_AOV_PRIM_ID ? kAovPrim : kAovMaterial, k);
        return (w == 0u || w == kAovMissWord) ? 0xffffffffu : w - 1u;
    }
    }
}
__host__ __device__ inline uint32_t aov_channels(uint32_t which) { return which < 2u ? 3u : which < WFPT_AOV_COUNT ? 1u : 0u; }

// ---- denoiser (WFPT_FLAG_DENOISE; include/wfpt.h "Denoiser"). The luminance moments are two planes of `plane` floats (the pixel capacity)
// behind one base pointer, indexed like `accumulated`: S1 = sum of L_k, then S2 = sum of L_k * L_k, over the samples k since the last reset.
constexpr uint32_t kMomentPlanes = 2;
__host__ __device__ inline float denoise_luma(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }
// The variance of the n-sample mean's luminance from the moments (wfpt_read_variance on the host, denoise_prepare_kernel on the device):
// one IEEE f32 division per step, in this order.
__host__ __device__ inline float variance_resolve(float s1, float s2, uint32_t n) {
    if (n == 0u) return 0.0f;
    const float nf = static_cast<float>(n);
    const float mu = s1 / nf;
    const float d = s2 / nf - mu * mu;
    return (d > 0.0f ? d : 0.0f) / nf;
}

// One launch of the filter chain over a width x height row-major image (an unsharded context: pixel slot = x + y * width).
struct DenoiseArgs {
    uint32_t width, height;
    uint32_t n;                 // samples accumulated (>= 1)
    const float *accumulated;   // stride 3
    const float *aov_sums;      // kAovPlanes planes of `plane`
    const float *moments;       // kMomentPlanes planes of `plane`
    Stride32 plane;
    float4 *guide_nz;           // (normalised normal, depth): written by prepare, read by the passes
    float4 *guide_ag;           // (albedo, |grad z|)
    const float4 *cv_in;        // (c, v) of the previous pass
    float4 *cv_out;             // (c, v) this launch writes (prepare: pass 0's input)
    float *out;                 // when not null: also c, stride 3, the first out_floats floats (the caller's buffer)
    size_t out_floats;
    uint32_t step;              // a-trous pass: 2^i
    float sigma_l, sigma_n, sigma_z, sigma_a2; // sigma_a2 = sigma_albedo * sigma_albedo
};
constexpr uint32_t kDenoiseTile = 16; // a workgroup = 16 x 16 pixels, each of its four waves an 8 x 8 block

// ---- temporal denoiser (include/wfpt.h "Temporal denoiser"). A history slot: four SoA planes of `plane` pixels.
struct TemporalSlot {
    float4 *cl;  // (blended colour, history length L)
    float2 *m;   // per-sample moments (m1, m2)
    float4 *nz;  // (normalised normal, depth) as prepare makes them
    float2 *cm;  // (coverage, material id as its u32 bits)
};
constexpr float kNoMotion = -1e30f; // x', y' of a pixel without a projection
// temporal_prepare_kernel's launch beside the DenoiseArgs of the chain (cv_out, guides, out as prepare's)
struct TemporalArgs {
    const CameraDev *camera; // the current camera (the context's device copy)
    float m[16];             // world -> clip of the sealed camera, column-major (mat_mul's layout)
    float pos_s[3];          // the sealed camera's position
    uint32_t has_sealed;     // 0: no projection at all (first call, dropped history, another viewport)
    float history_cap, depth_tolerance, normal_cos;
    TemporalSlot sealed;     // read
    TemporalSlot live;       // written
    float4 *motion;          // (x', y', z', 0)
};

// mask (null = none; WFPT_FLAG_ADAPTIVE contexts, here and in launch_generate_dense): one word per tile, bit ly * 8 + lx clear = the
// lane leaves an inactive ray, as a lane outside the image does, and does not reset its pixel's image slice
hipError_t launch_generate(const GenerateArgs &a, hipStream_t s, const uint64_t *mask = nullptr);
hipError_t launch_extend(const ExtendArgs &a, uint32_t grid, hipStream_t s, bool env_dirs = false); // env_dirs: also write the miss queue's dx, dz planes
hipError_t launch_scan(const ScanArgs &a, hipStream_t s); // one workgroup per sample
// env_dirs: the variant of WFPT_FLAG_ENVIRONMENT contexts with a map: misses carry direction.x and .z, no miss items (launch_miss with the
// map lights them)
hipError_t launch_bounce(const BounceArgs &a, int mode, uint32_t grid, hipStream_t s, bool env_dirs = false);
hipError_t launch_tile_lists(const TileListArgs &a, hipStream_t s);
hipError_t launch_bounce_binned(const BounceArgs &a, int mode, uint32_t grid, hipStream_t s); // LDS-resident scenes only
hipError_t launch_scan_binned(const ScanBinnedArgs &a, hipStream_t s);
hipError_t launch_plan(const PlanArgs &a, hipStream_t s);
hipError_t bounce_binned_blocks_per_cu(const SceneDev &scene, int *blocks);
hipError_t launch_refill(const RefillArgs &a, int mode, uint32_t grid, hipStream_t s);
hipError_t launch_shade_rays(const RefillArgs &a, uint32_t n_chunks, hipStream_t s, bool retire = false);
hipError_t launch_generate_dense(const RefillArgs &a, hipStream_t s, const uint64_t *mask = nullptr); // the first wavefront's primary rays into the dense array
hipError_t launch_compact(const CompactArgs &a, uint32_t n_chunks, hipStream_t s, bool env_dirs = false);
hipError_t bounce_blocks_per_cu(const SceneDev &scene, int *blocks);
// retire: the termination step's inputs (shade_retire_kernel), null = shade_kernel
hipError_t launch_shade(const ShadeArgs &a, uint32_t grid, hipStream_t s, const TermArgs *retire = nullptr);
// the termination step for n caller rows (wfpt_sample_termination): p.wavefront is the caller's b
hipError_t launch_termination_sampler(const TermArgs &p, uint32_t frame, const float *in4, float *out8, uint32_t n, hipStream_t s);
// connected: the `emitted` plane of a context that connects to its map (WFPT_FLAG_ENV_NEE): miss_env_nee_kernel, which leaves thr = +0
// where the pixel's connected flag (emitted.w) is 1
// weigh: miss_env_mis_kernel instead (WFPT_FLAG_ENV_MIS; needs `connected` and env's tables), which keeps thr * c there, times the balance
// weight wb of the scatter against the map's own sampling (env_mis_weight)
hipError_t launch_miss(const MissArgs &a, uint32_t grid, hipStream_t s, const EnvDist *env = nullptr, const float *connected = nullptr,
                       bool weigh = false);
// wfpt_env_mis_miss_weight: n rows of an un-normalised direction -> (pe, pb, wb, texel), one thread per row
hipError_t launch_env_mis_weight(const EnvDist &env, const float *dirs3, float *out4, uint32_t n, hipStream_t s);
hipError_t launch_texture(const TextureArgs &a, uint32_t grid, hipStream_t s);
// q: kEmitWeighedEnv's alone, 1 - the effective environment share
// ld: kEmitWeighedPower's alone
hipError_t launch_emission(const EmissionArgs &a, EmissionKind kind, uint32_t grid, hipStream_t s, float q = 1.0f, const LightDist *ld = nullptr);
// wfpt_mis_hit_weight: n rows of (o.xyz, d.xyz, t, primitive) -> (pl, pb, wb, cos_l), one thread per row
// ld (null = none): the light list's distribution, nfi in nf's place (mis_weight_power_kernel)
hipError_t launch_mis_weight(const MisArgs &m, const float4 *shade_rec, const uint32_t *prim_em, const float *in8, float *out4, uint32_t n, hipStream_t s,
                             const LightDist *ld = nullptr);
// grid: at most extend's (the four-wide walk's spill area is sized for that); textured: a light's material is bound to a texture
// envs: the ENVS variants (a.envd holds a distribution)
// mis: the MIS variants (a.origin set, or the sampler form's rows out); with envs, the ENVS MIS variants
// power (null = none): the POWER variants with this distribution (never with envs)
// analytic (null = none): the ANALYTIC variants with this table (never with envs or power)
// shading (null = none): the SHADING variants with these per-primitive normal rows (triangles; never with power or analytic): the
// receiver's normal is the shading normal
// nmap (null = none): the NMAP variants (connect_nmap_kernel; triangles; never with power or analytic; `shading` is ignored, nmap->normals
// names the rows): the receiver's normal is the mapped normal
hipError_t launch_connect(const ConnectArgs &a, uint32_t grid, hipStream_t s, bool textured, bool envs = false, bool mis = false,
                          const LightDist *power = nullptr, const LightTable *analytic = nullptr, const float4 *shading = nullptr,
                          const NmapScene *nmap = nullptr);
hipError_t launch_shading_normal(const ShadingArgs &a, uint32_t grid, hipStream_t s);
// wfpt_sample_shading_normal: n rows of (p.xyz | the primitive's bits) -> (ns.xyz | 1 where it fell back to the stored normal, else 0), one
// thread per row; a primitive outside the scene answers (0, 0, 0, 1)
hipError_t launch_shading_sample(const float4 *prim_geom, const float4 *shade_rec, const float4 *normals, uint32_t n_prims, const float *in4,
                                 float *out4, uint32_t n, hipStream_t s);
hipError_t launch_microfacet(const MicrofacetArgs &a, uint32_t grid, hipStream_t s);
// wfpt_sample_microfacet: n rows of (d.xyz, n.xyz, u1, u2, alpha, F0.rgb) -> (m.xyz | 2 where step 1 fell back, 1 where step 10 left the
// weight at zero, else 0 | weight.rgb | cm), one thread per row; both buffers 16-byte aligned
hipError_t launch_microfacet_sample(const float *in12, float *out8, uint32_t n, hipStream_t s);
// The microfacet pass of a WFPT_FLAG_ROUGH_DIELECTRIC context that holds a roughness above 0 on a dielectric (rough_glass_kernel; include/wfpt.h
// "Rough dielectrics"), in launch_microfacet's place: a.mf_prim then holds the alpha of metal and dielectric primitives. A metal hit's record
// is launch_microfacet's; a rough glass hit's is (h | +0), (albedo * G1 | rec1.w), (material type 1 | rec2.yzw).
hipError_t launch_rough_glass(const MicrofacetArgs &a, uint32_t grid, hipStream_t s);
// wfpt_sample_rough_dielectric: n rows of (d.xyz, n.xyz, u1, u2 | u3, alpha, ior, albedo.rgb, 0, 0) -> (h.xyz | 2 fell back, 1 dead, else
// 0 | weight.rgb | 1 refracted, 0 reflected), one thread per row; both buffers 16-byte aligned
hipError_t launch_rough_glass_sample(const float *in16, float *out8, uint32_t n, hipStream_t s);
// The record pass of a mapped context (include/wfpt.h "Normal maps"), in the place of launch_shading_normal (a.mf_prim null:
// shading_nmap_kernel), launch_microfacet (microfacet_nmap_kernel) or, with glass, launch_rough_glass (rough_glass_nmap_kernel): the same
// walk, table and slot rewrite; the normal of every record, and the normal a rough hit samples about, is the mapped normal. A hit whose
// material has no map gets bit for bit the record of the kernel replaced. a.normals is ignored: nm.normals names the rows (or null).
hipError_t launch_nmap_record(const MicrofacetArgs &a, const NmapScene &nm, bool glass, uint32_t grid, hipStream_t s);
// wfpt_sample_normal_map: n rows of (p.xyz | the primitive's bits) -> (n.xyz | the header's probe code), one thread per row; a primitive
// outside the scene answers (0, 0, 0, 5)
hipError_t launch_nmap_sample(const float4 *prim_geom, const float4 *shade_rec, const NmapScene &nm, uint32_t n_prims, const float *in4,
                              float *out4, uint32_t n, hipStream_t s);
// The record pass of a roughness-mapped context (include/wfpt.h "Roughness maps"), in the place of launch_microfacet or launch_nmap_record
// (microfacet_rmap_kernel) or, with glass, launch_rough_glass (rough_glass_rmap_kernel): the same walk, table and slot rewrite; a rough
// hit of a bound material is sampled with alpha_m * the map's factor, or gets a non-rough hit's record where that is not above 0. The
// normal is the mapped one (rm.prim_map set), the shading one (rm.normals set) or the stored one. a.normals and a.mf_prim are ignored.
hipError_t launch_rmap_record(const MicrofacetArgs &a, const RmapScene &rm, bool glass, uint32_t grid, hipStream_t s);
// wfpt_sample_roughness_map: n rows of (p.xyz | the primitive's bits) -> (alpha_h | r | the header's probe code | 0), one thread per row;
// a primitive outside the scene answers (0, 0, 5, 0)
hipError_t launch_rmap_sample(const float4 *prim_geom, const RmapScene &rm, uint32_t n_prims, const float *in4, float *out4, uint32_t n,
                              hipStream_t s);
// The sampling distribution of a light list (include/wfpt.h "Light selection by power"), built on the device on `s`. lights: the n_l
// primitives that emit, in list order; geom / prim_kind: the primitives they index (SceneDev::prim_geom's layout); prim_em / em: the
// emission tables. First f = L * A per light into `f` and the bits of the largest f > 0 into *max_bits (zeroed by the caller); then, once the
// caller has read M back, k into `k` with the sum of every kLightTile lights into tile_sum; then cdf, and k scattered into prim_k
// (zeroed by the caller) at the lights' primitives.
constexpr uint32_t kLightTile = 256;
hipError_t launch_light_weights(const uint32_t *lights, uint32_t n_l, const float4 *geom, uint32_t prim_kind, const uint32_t *prim_em, const float4 *em,
                                float *f, uint32_t *max_bits, hipStream_t s);
hipError_t launch_light_tables(const uint32_t *lights, uint32_t n_l, const float *f, float M, uint32_t *k, uint32_t *tile_sum, uint64_t *cdf,
                               uint32_t *prim_k, hipStream_t s);
// The sampling distribution of a map (include/wfpt.h "Environment next-event estimation"), built on the device in three launches on `s`:
// f = Lm * s_y per texel into `f` (w * h floats) and its maximum's bits into *max_bits (zeroed by the caller); then, once the caller has
// read M back, row (w * h) and the row-total prefix marg (h).
hipError_t launch_env_weights(const EnvDev &env, float *f, uint32_t *max_bits, hipStream_t s);
hipError_t launch_env_tables(const EnvDev &env, const float *f, float M, uint32_t *row, uint64_t *marg, hipStream_t s);
hipError_t connect_prepare(const SceneDev &scene); // raises the connect kernels' dynamic-LDS limit where the scene needs more than 64 KiB
// The accumulate launch. emitted (null = none): the second per-sample plane, each sample's value is image_k + emitted_k. moments (null =
// none; WFPT_FLAG_DENOISE contexts): plus the luminance moments, two planes `plane` floats apart. One kernel of four, the same
// `accumulated` bits from each.
hipError_t launch_accumulate(const AccumulateArgs &a, const float *emitted, float *moments, size_t plane, uint32_t grid, hipStream_t s);
// The accumulate launch of WFPT_FLAG_ADAPTIVE contexts (include/wfpt.h "Adaptive sampling"): the moments always, and only for the pixels
// whose mask bit is set, whose count grows by the batch's samples. One kernel of two (emitted or not).
hipError_t launch_accumulate_masked(const AccumulateArgs &a, const float *emitted, float *moments, size_t plane, const MaskArgs &m, uint32_t grid,
                                    hipStream_t s);
hipError_t launch_adaptive_update(const AdaptiveArgs &a, hipStream_t s);  // one wave per tile of the context
// accumulated / count into out (stride 3), the first n_floats floats: wfpt_copy_mean_to_device
hipError_t launch_mean_resolve(const float *accumulated, const uint32_t *count, float *out, size_t n_floats, hipStream_t s);
hipError_t launch_fill(float *p, float v, size_t n, hipStream_t s);
hipError_t launch_set_frame(Control *ctl, const wfpt_frame_buffer &f, hipStream_t s); // ctl->frame = f, ordered on the stream
// frame band (j * world + rank) <- slab band j for the first n_valid floats of a slab: the root of the multi-GPU gather
hipError_t launch_band_scatter(float *frame, const float *slab, size_t n_valid, size_t band_floats, uint32_t world, uint32_t rank, hipStream_t s);
// AoS <-> SoA converters for the read-back / injection paths
hipError_t launch_rays_to_aos(const RayQueue &q, wfpt_ray *out, uint32_t n, hipStream_t s);
hipError_t launch_rays_from_aos(const RayQueue &q, const wfpt_ray *in, uint32_t n, hipStream_t s);
// AOV pass of one batch: `grid` persistent workgroups of kExtendThreads (at most the extend grid: the four-wide walk's stack spill area is
// sized for it)
// shading (null = none): aov_shading_kernel with these per-primitive normal rows (triangles): the normal sum takes the shading normal
// nmap (null = none): aov_nmap_kernel (triangles; `shading` is ignored, nmap->normals names the rows): the normal sum takes the mapped normal
hipError_t launch_aov(const AovArgs &a, uint32_t grid, hipStream_t s, const EnvDev *env = nullptr, const TexScene *tex = nullptr,
                      const float4 *shading = nullptr, const NmapScene *nmap = nullptr);
hipError_t aov_prepare(const SceneDev &scene); // raises the AOV kernels' dynamic-LDS limit where the scene needs more than 64 KiB
hipError_t launch_aov_resolve(const float *sums, size_t plane, uint32_t which, uint32_t n_samples, uint32_t *out, size_t n_words, hipStream_t s);
hipError_t launch_denoise_prepare(const DenoiseArgs &a, hipStream_t s);
hipError_t launch_denoise_atrous(const DenoiseArgs &a, hipStream_t s);
hipError_t launch_temporal_prepare(const DenoiseArgs &a, const TemporalArgs &t, hipStream_t s);
// env_lookup of n directions (xyz, stride 3) into rgb (stride 3): wfpt_sample_environment
hipError_t launch_env_sample(const EnvDev &env, const float *dirs, float *rgb, size_t n, hipStream_t s);
// tex_lookup of n UVs (stride 2) into rgb (stride 3): wfpt_sample_texture
hipError_t launch_tex_sample(const TexDev &tex, const float *uv, float *rgb, size_t n, hipStream_t s);
hipError_t launch_selftest_math(int op, const float *a, const float *b, float *out, size_t n, hipStream_t s);
// Occupancy of the extend kernel for a given dynamic LDS size (workgroups per CU); also raises the
// kernel's dynamic-LDS limit when the scene needs more than the default 64 KiB.
hipError_t extend_blocks_per_cu(const SceneDev &scene, int *blocks);
uint32_t extend_lds_bytes(uint32_t n_nodes, uint32_t n_prims, uint32_t prim_kind, bool lds_scene);

} // namespace wfpt
