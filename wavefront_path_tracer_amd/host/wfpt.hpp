// wfpt.hpp -- header-only C++ host mirror of the reference's API for the wavefront path, over the C ABI
// (include/wfpt.h). The reference's host is Rust; this image has no Rust toolchain, so the compiled-language
// host side is C++ with the reference's type and method names:
//
//   Scene, BVHTree                 wavefront_common/src/{scene,bvh}.rs
//   Camera, CameraController       wavefront_common/src/{camera,camera_controller}.rs
//   ProjectionMatrix               wavefront_common/src/projection_matrix.rs
//   RenderParameters, RenderProgress  wavefront_common/src/parameters.rs
//   Kernel                         gpu_wavefront_pt/src/kernel.rs
//   PathTracer                     gpu_wavefront_pt/src/path_tracer.rs
//
// Error behaviour: the reference unwraps/panics; here every negative wfpt_status becomes a wfpt::Error.
#pragma once
#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "wfpt.h"

namespace wfpt {

constexpr uint32_t SPP = 10; // wavefront_common/src/parameters.rs:4
constexpr uint32_t SPF = 1;  // wavefront_common/src/parameters.rs:5

struct Error : std::runtime_error {
    int status;
    Error(int st, const std::string &msg) : std::runtime_error("wfpt status " + std::to_string(st) + ": " + msg), status(st) {}
};

// wavefront_common/src/scene.rs
struct Scene {
    std::vector<wfpt_sphere> spheres;
    std::vector<wfpt_material> materials;

    static Scene new_scene() { // Scene::new, scene.rs:12-46
        Scene s;
        s.spheres.resize(5);
        s.materials.resize(5);
        wfpt_scene_new(s.spheres.data(), s.materials.data());
        return s;
    }
    static Scene book_one_final(uint64_t seed = 1) { // scene.rs:48-107, seeded
        Scene s;
        s.spheres.resize(512);
        s.materials.resize(512);
        const uint32_t n = wfpt_scene_book_one_final(seed, s.spheres.data(), s.materials.data(), 512);
        if (n == 0) throw Error(WFPT_ERR_INVALID_ARGUMENT, "wfpt_scene_book_one_final");
        s.spheres.resize(n);
        s.materials.resize(n);
        return s;
    }
};

// wavefront_common/src/bvh.rs:143-210
struct BVHTree {
    std::vector<wfpt_bvh_node> nodes;
    explicit BVHTree(size_t num_primitives) { nodes.reserve(2 * num_primitives); }
    float device_ms = 0.0f; // device builds: time between the first and the last build kernel
    // Reorders spheres in place (bvh.rs:182). device < 0: the host builder; otherwise the same builder on that HIP
    // device (build extension, wfpt_build_bvh_device) -- same nodes, same order, byte for byte.
    void build_bvh_tree(std::vector<wfpt_sphere> &spheres, int device = -1) {
        nodes.assign(2 * (spheres.empty() ? 1 : spheres.size()), wfpt_bvh_node{});
        uint32_t n = 0;
        const uint32_t count = static_cast<uint32_t>(spheres.size()), cap = static_cast<uint32_t>(nodes.size());
        const int st = device < 0 ? wfpt_build_bvh(spheres.data(), count, nodes.data(), cap, &n)
                                  : wfpt_build_bvh_device(spheres.data(), count, nodes.data(), cap, &n, device, &device_ms);
        if (st != WFPT_OK) throw Error(st, std::string("wfpt_build_bvh: ") + wfpt_last_error(nullptr));
        nodes.resize(n);
    }
    void build_bvh_tree_triangles(std::vector<wfpt_triangle> &triangles, uint32_t n_bins = 32, int device = -1) {
        nodes.assign(2 * (triangles.empty() ? 1 : triangles.size()), wfpt_bvh_node{});
        uint32_t n = 0;
        const uint32_t count = static_cast<uint32_t>(triangles.size()), cap = static_cast<uint32_t>(nodes.size());
        const int st = device < 0 ? wfpt_build_bvh_triangles(triangles.data(), count, nodes.data(), cap, &n, n_bins)
                                  : wfpt_build_bvh_triangles_device(triangles.data(), count, nodes.data(), cap, &n, n_bins, device, &device_ms);
        if (st != WFPT_OK) throw Error(st, std::string("wfpt_build_bvh_triangles: ") + wfpt_last_error(nullptr));
        nodes.resize(n);
    }
};

// wavefront_common/src/camera.rs
struct Camera {
    std::array<float, 3> position{};
    float pitch = 0.0f, yaw = 0.0f;
    Camera(std::array<float, 3> look_from, std::array<float, 3> look_at) : position(look_from) {
        wfpt_camera_new(look_from.data(), look_at.data(), &pitch, &yaw);
    }
    static Camera book_one_final_camera() { return Camera({13.0f, 2.0f, 3.0f}, {0.0f, 0.0f, 0.0f}); } // camera.rs:26-30
    std::array<float, 16> view_transform() const { // camera.rs:41-69
        std::array<float, 16> m{};
        wfpt_view_transform(position.data(), pitch, yaw, m.data());
        return m;
    }
};

// wavefront_common/src/camera_controller.rs:8-158
class CameraController {
  public:
    CameraController(Camera camera, float vfov, float defocus_angle, float focus_distance, float z_near, float z_far,
                     float speed = 4.0f, float sensitivity = 0.1f)
        : camera_(camera), vfov_rad_(wfpt_to_radians(vfov)), defocus_angle_rad_(wfpt_to_radians(defocus_angle)),
          focus_distance_(focus_distance), z_near_(z_near), z_far_(z_far), speed_(speed), sensitivity_(sensitivity) {}
    float vfov_rad() const { return vfov_rad_; }
    void set_vfov(float vfov) { vfov_rad_ = wfpt_to_radians(vfov); }
    std::pair<float, float> dof() const { return {defocus_angle_rad_, focus_distance_}; }
    void set_defocus_angle(float da) { defocus_angle_rad_ = wfpt_to_radians(da); }
    void set_focus_distance(float fd) { focus_distance_ = fd; }
    // camera_controller.rs:74-125: key state and pending mouse rotation
    void process_mouse(std::array<float, 2> delta) { rotate_ = delta; }
    void move_forward(uint32_t dir) { amounts_[0] = dir == 1 ? 1.0f : 0.0f; }
    void move_backwards(uint32_t dir) { amounts_[1] = dir == 1 ? 1.0f : 0.0f; }
    void move_right(uint32_t dir) { amounts_[2] = dir == 1 ? 1.0f : 0.0f; }
    void move_left(uint32_t dir) { amounts_[3] = dir == 1 ? 1.0f : 0.0f; }
    void move_up(uint32_t dir) { amounts_[4] = dir == 1 ? 1.0f : 0.0f; }
    void move_down(uint32_t dir) { amounts_[5] = dir == 1 ? 1.0f : 0.0f; }
    void update_camera(float dt) { // camera_controller.rs:125-158
        wfpt_camera_controller_update(camera_.position.data(), &camera_.pitch, &camera_.yaw, amounts_.data(), rotate_.data(),
                                      speed_, sensitivity_, dt);
    }
    std::pair<float, float> get_clip_planes() const { return {z_near_, z_far_}; }
    wfpt_gpu_camera get_GPU_camera() const { // camera_controller.rs:66-68
        wfpt_gpu_camera c{};
        wfpt_gpu_camera_new(camera_.position.data(), camera_.pitch, camera_.yaw, defocus_angle_rad_, focus_distance_, &c);
        return c;
    }
    std::array<float, 16> get_view_matrix() const { return camera_.view_transform(); }
    const Camera &camera() const { return camera_; }

  private:
    Camera camera_;
    float vfov_rad_, defocus_angle_rad_, focus_distance_, z_near_, z_far_, speed_, sensitivity_;
    std::array<float, 6> amounts_{}; // forward, backward, right, left, up, down
    std::array<float, 2> rotate_{};  // horizontal, vertical
};

// wavefront_common/src/projection_matrix.rs
struct ProjectionMatrix {
    float vfov_rad, aspect_ratio, z_near, z_far;
    ProjectionMatrix(float vfov, float ar, float zn, float zf) : vfov_rad(vfov), aspect_ratio(ar), z_near(zn), z_far(zf) {}
    std::array<float, 16> p_inv() const {
        std::array<float, 16> m{};
        wfpt_p_inv(vfov_rad, aspect_ratio, z_near, z_far, m.data());
        return m;
    }
};

// wavefront_common/src/parameters.rs:7-58
class RenderParameters {
  public:
    RenderParameters(CameraController cc, std::pair<uint32_t, uint32_t> viewport) : cc_(cc), viewport_(viewport) {}
    bool changed() const { return resized_ || camera_changed_; }
    bool resized() const { return resized_; }
    bool camera_changed() const { return camera_changed_; }
    void set_viewport(std::pair<uint32_t, uint32_t> size) { viewport_ = size; resized_ = true; }
    std::pair<uint32_t, uint32_t> viewport_size() const { return viewport_; }
    void reset() { resized_ = camera_changed_ = false; }
    const CameraController &camera_controller() const { return cc_; }
    void update_camera_controller(CameraController cc) { cc_ = cc; camera_changed_ = true; }

  private:
    CameraController cc_;
    std::pair<uint32_t, uint32_t> viewport_;
    bool resized_ = false, camera_changed_ = false;
};

// wavefront_common/src/parameters.rs:61-101
class RenderProgress {
  public:
    wfpt_frame_buffer get_next_frame(const RenderParameters &rp) {
        frame_ += 1;
        return {rp.viewport_size().first, rp.viewport_size().second, frame_, 0};
    }
    void incr_accumulated_samples(uint32_t d) { accumulated_samples_ += d; }
    void reset() { accumulated_samples_ = 0; frame_ = 0; }
    float progress() const { return static_cast<float>(accumulated_samples_) / static_cast<float>(SPP); }
    uint32_t accumulated_samples() const { return accumulated_samples_; }
    uint32_t frame() const { return frame_; }

  private:
    uint32_t frame_ = 0, accumulated_samples_ = 0;
};

inline std::pair<uint32_t, uint32_t> workgroup_size_64(uint32_t x) { // path_tracer.rs:282-289
    uint32_t gx = 0, gy = 0;
    wfpt_workgroup_size_64(x, &gx, &gy);
    return {gx, gy};
}

class PathTracer;

// gpu_wavefront_pt/src/kernel.rs
class Kernel {
  public:
    Kernel() = default;
    Kernel(const char *name, wfpt_ctx *ctx) : ctx_(ctx), stage_(wfpt_stage_from_name(name)) {
        if (stage_ < 0 || stage_ >= WFPT_STAGE_SCAN) throw Error(WFPT_ERR_INVALID_ARGUMENT, std::string("no such kernel stage: ") + name);
    }
    void run(std::pair<uint32_t, uint32_t> workgroup_size) { // kernel.rs:107-140
        const int st = wfpt_kernel_run(ctx_, stage_, workgroup_size.first, workgroup_size.second);
        if (st != WFPT_OK) throw Error(st, wfpt_last_error(ctx_));
    }
    float get_timing() { return wfpt_kernel_timing_us(ctx_, stage_); } // kernel.rs:142-146, microseconds

  private:
    wfpt_ctx *ctx_ = nullptr;
    int stage_ = -1;
};

// gpu_wavefront_pt/src/path_tracer.rs
class PathTracer {
  public:
    struct Options {
        uint32_t max_window_size = 0; // path_tracer.rs:44
        uint32_t max_wavefronts = 50; // path_tracer.rs:323
        uint32_t miss_floor = 128;    // path_tracer.rs:332
        uint32_t rng_mode = WFPT_RNG_DISPATCH;
        uint32_t flags = 0, tile_rank = 0, tile_world = 1;
        int32_t device = 0;
        uint32_t spp = SPP;
        uint32_t batch = 0; // samples in flight per launch of render(); 0 = library default
    };

    // PathTracer::new (path_tracer.rs:43-217): builds the BVH (reordering scene.spheres), uploads everything.
    PathTracer(Scene &scene, const RenderParameters &rp, const Options &opt)
        : render_parameters_(rp), opt_(opt), bvh_tree_(scene.spheres.size()) {
        bvh_tree_.build_bvh_tree(scene.spheres); // :117-118
        const CameraController &cc = rp.camera_controller();
        const auto [w, h] = rp.viewport_size();
        const float ar = static_cast<float>(w) / static_cast<float>(h);
        const auto [zn, zf] = cc.get_clip_planes();
        const auto proj = ProjectionMatrix(cc.vfov_rad(), ar, zn, zf).p_inv(); // :137-138
        const auto view = cc.get_view_matrix();
        const wfpt_gpu_camera cam = cc.get_GPU_camera();
        wfpt_params p{};
        p.width = w; p.height = h; p.max_pixels = opt.max_window_size;
        p.max_wavefronts = opt.max_wavefronts; p.miss_floor = opt.miss_floor;
        p.rng_mode = opt.rng_mode; p.flags = opt.flags;
        p.tile_rank = opt.tile_rank; p.tile_world = opt.tile_world; p.device = opt.device; p.batch = opt.batch;
        ctx_ = wfpt_create(&p, scene.spheres.data(), static_cast<uint32_t>(scene.spheres.size()), scene.materials.data(),
                           static_cast<uint32_t>(scene.materials.size()), bvh_tree_.nodes.data(),
                           static_cast<uint32_t>(bvh_tree_.nodes.size()), &cam, proj.data(), view.data());
        if (!ctx_) throw Error(WFPT_ERR_HIP, wfpt_last_error(nullptr));
        generate_ray_kernel_ = Kernel("generate_rays", ctx_); // :162
        extend_kernel_ = Kernel("extend", ctx_);              // :167
        shade_kernel_ = Kernel("shade", ctx_);                // :175
        miss_kernel_ = Kernel("miss_kernel", ctx_);           // :180
        accumulate_kernel_ = Kernel("accumulate", ctx_);      // :185
    }
    ~PathTracer() { wfpt_destroy(ctx_); }
    PathTracer(const PathTracer &) = delete;
    PathTracer &operator=(const PathTracer &) = delete;

    float progress() const { return render_progress_.progress(); }                    // :219-221
    RenderParameters get_render_parameters() const { return render_parameters_; }     // :227-229
    void update_render_parameters(const RenderParameters &rp) { render_parameters_ = rp; } // :236-238
    void resize(const RenderParameters &rp) { update_render_parameters(rp); }         // :231-235

    void update_buffers() { // :240-277
        if (!render_parameters_.changed()) return;
        const CameraController &cc = render_parameters_.camera_controller();
        const auto [w, h] = render_parameters_.viewport_size();
        const auto [zn, zf] = cc.get_clip_planes();
        const auto proj = ProjectionMatrix(cc.vfov_rad(), static_cast<float>(w) / static_cast<float>(h), zn, zf).p_inv();
        const auto view = cc.get_view_matrix();
        const wfpt_gpu_camera cam = cc.get_GPU_camera();
        check(wfpt_update_render_parameters(ctx_, w, h, &cam, proj.data(), view.data()));
        render_parameters_.reset();
        render_progress_.reset();
    }

    // PathTracer::run (path_tracer.rs:279-371): the host-driven loop over the five Kernels.
    void run() {
        update_buffers();
        if (render_progress_.accumulated_samples() < opt_.spp) {
            wfpt_frame_buffer frame = render_progress_.get_next_frame(render_parameters_);
            for (uint32_t sample_number = 0; sample_number < SPF; ++sample_number) {
                frame.sample_number = sample_number;
                check(wfpt_set_frame(ctx_, &frame));                           // :296-297
                check(wfpt_reset_image(ctx_));                                 // :305-306
                check(wfpt_clear_ray_queues(ctx_));                            // :309-310
                const auto [width, height] = render_parameters_.viewport_size();
                uint32_t counter[16] = {0};
                counter[2] = width * height;                                   // :313-316
                check(wfpt_set_counters(ctx_, counter));
                generate_ray_kernel_.run({width / 8, height / 8});             // :318
                uint32_t wavefront = 0;
                auto extend_size = workgroup_size_64(width * height);          // :322
                while (wavefront < opt_.max_wavefronts) {                      // :323
                    extend_kernel_.run(extend_size);                           // :325
                    check(wfpt_read_counters(ctx_, counter));                  // :327-328
                    const uint32_t num_misses = counter[0], num_hits = counter[1];
                    if (num_misses < opt_.miss_floor) break;                   // :332
                    counter[2] = 0;                                            // :335-336
                    check(wfpt_set_counters(ctx_, counter));
                    shade_kernel_.run(workgroup_size_64(num_hits));            // :339
                    miss_kernel_.run(workgroup_size_64(num_misses));           // :340
                    check(wfpt_read_counters(ctx_, counter));                  // :343-345
                    const uint32_t num_extension = counter[2];
                    check(wfpt_swap_ray_queues(ctx_));                         // :348
                    extend_size = workgroup_size_64(num_extension);            // :350
                    const uint32_t next[16] = {0, 0, num_extension, 0};        // :352
                    check(wfpt_set_counters(ctx_, next));
                    wavefront += 1;
                }
                last_wavefronts_ = wavefront;
                accumulate_kernel_.run(workgroup_size_64(width * height));     // :362
                render_progress_.incr_accumulated_samples(1);                  // :363
                frame.sample_number = render_progress_.accumulated_samples();  // :366-367
                check(wfpt_set_frame(ctx_, &frame));
            }
        }
    }

    // The same loop resident on the device (no host synchronisation).
    void render(uint32_t spp) { check(wfpt_render(ctx_, spp)); }

    std::vector<float> accumulated() {
        std::vector<float> a(3 * static_cast<size_t>(wfpt_n_pixels(ctx_)));
        check(wfpt_read_accumulated(ctx_, a.data(), a.size()));
        return a;
    }
    // Textures (WFPT_FLAG_TEXTURES, include/wfpt.h "Textures"): rgb = h rows of w linear texels, 3 floats each, row 0 = the top.
    void set_texture(uint32_t slot, const std::vector<float> &rgb, uint32_t w, uint32_t h, std::array<float, 2> scale = {1.0f, 1.0f},
                     std::array<float, 2> offset = {0.0f, 0.0f}, uint32_t filter = WFPT_TEXTURE_BILINEAR) {
        if (rgb.size() != 3 * static_cast<size_t>(w) * h) throw Error(WFPT_ERR_INVALID_ARGUMENT, "set_texture: rgb must hold w * h * 3 floats");
        wfpt_texture_params p;
        wfpt_texture_params_default(&p);
        p.scale[0] = scale[0]; p.scale[1] = scale[1];
        p.offset[0] = offset[0]; p.offset[1] = offset[1];
        p.filter = filter;
        check(wfpt_set_texture(ctx_, slot, rgb.data(), w, h, &p));
    }
    void clear_texture(uint32_t slot) { check(wfpt_clear_texture(ctx_, slot)); }
    void bind_texture(uint32_t material_idx, int32_t slot) { check(wfpt_bind_texture(ctx_, material_idx, slot)); } // slot -1 unbinds
    void set_triangle_uvs(const std::vector<float> &uv6) { // rows of u0 v0 u1 v1 u2 v2; empty clears
        check(wfpt_set_triangle_uvs(ctx_, uv6.empty() ? nullptr : uv6.data(), static_cast<uint32_t>(uv6.size() / 6)));
    }
    std::vector<float> sample_texture(uint32_t slot, const std::vector<float> &uv) { // (u, v) pairs -> rgb triples
        std::vector<float> rgb(3 * (uv.size() / 2));
        check(wfpt_sample_texture(ctx_, slot, uv.data(), uv.size() / 2, rgb.data()));
        return rgb;
    }
    std::pair<float, uint32_t> texture_timing() { return timing(wfpt_texture_timing_ms); }
    // Shading normals (WFPT_FLAG_SHADING_NORMALS, include/wfpt.h "Shading normals"): rows of the normals of corners 0, 1, 2, nine floats
    // each, row r for the triangles whose _pad is r; empty clears.
    void set_triangle_normals(const std::vector<float> &n9) {
        check(wfpt_set_triangle_normals(ctx_, n9.empty() ? nullptr : n9.data(), static_cast<uint32_t>(n9.size() / 9)));
    }
    std::vector<float> triangle_normals() { // the table as stored (normalised)
        uint32_t n = 0;
        check(wfpt_get_triangle_normals(ctx_, nullptr, 0, &n));
        std::vector<float> n9(9 * static_cast<size_t>(n));
        if (n) check(wfpt_get_triangle_normals(ctx_, n9.data(), n, &n));
        return n9;
    }
    std::vector<float> sample_shading_normal(const std::vector<float> &in4) { // (p.xyz | the triangle's bits) -> (ns.xyz | fell back)
        std::vector<float> out(in4.size() / 4 * 4);
        check(wfpt_sample_shading_normal(ctx_, in4.data(), in4.size() / 4, out.data()));
        return out;
    }
    std::pair<float, uint32_t> shading_normal_timing() { return timing(wfpt_shading_normal_timing_ms); }
    // Microfacet metals (WFPT_FLAG_MICROFACET, include/wfpt.h "Microfacet metals"): a material's GGX roughness alpha in [0, 1]; its metal
    // primitives are shaded as rough conductors while it is above 0.
    void set_roughness(uint32_t material_idx, float alpha) { check(wfpt_set_roughness(ctx_, material_idx, alpha)); }
    float roughness(uint32_t material_idx) {
        float alpha = 0.0f;
        check(wfpt_get_roughness(ctx_, material_idx, &alpha));
        return alpha;
    }
    void clear_roughness() { check(wfpt_clear_roughness(ctx_)); }
    std::vector<float> sample_microfacet(const std::vector<float> &in12) { // (d.xyz, n.xyz, u1, u2, alpha, F0.rgb) -> (m.xyz | state | weight.rgb | cm)
        std::vector<float> out(in12.size() / 12 * 8);
        check(wfpt_sample_microfacet(ctx_, in12.data(), in12.size() / 12, out.data()));
        return out;
    }
    std::pair<float, uint32_t> microfacet_timing() { return timing(wfpt_microfacet_timing_ms); }
    // Rough dielectrics (WFPT_FLAG_ROUGH_DIELECTRIC, include/wfpt.h "Rough dielectrics"): set_roughness on a dielectric's material counts too.
    std::vector<float> sample_rough_dielectric(const std::vector<float> &in16) { // (d.xyz, n.xyz, u1, u2 | u3, alpha, ior, albedo.rgb, 0, 0) -> (h.xyz | state | weight.rgb | refracted)
        std::vector<float> out(in16.size() / 16 * 8);
        check(wfpt_sample_rough_dielectric(ctx_, in16.data(), in16.size() / 16, out.data()));
        return out;
    }
    // Normal maps (WFPT_FLAG_NORMAL_MAPS, include/wfpt.h "Normal maps"): a material takes a texture slot as its tangent-space normal map
    // (rgb = 0.5 + 0.5 n, green = +v); slot -1 unbinds.
    void bind_normal_map(uint32_t material_idx, int32_t slot, float strength = 1.0f) { check(wfpt_bind_normal_map(ctx_, material_idx, slot, strength)); }
    std::pair<int32_t, float> normal_map(uint32_t material_idx) { // (slot or -1, strength)
        int32_t slot = -1;
        float strength = 0.0f;
        check(wfpt_get_normal_map(ctx_, material_idx, &slot, &strength));
        return {slot, strength};
    }
    std::vector<float> sample_normal_map(const std::vector<float> &in4) { // (p.xyz | the triangle's bits) -> (n.xyz | code 0..5)
        std::vector<float> out(in4.size() / 4 * 4);
        check(wfpt_sample_normal_map(ctx_, in4.data(), in4.size() / 4, out.data()));
        return out;
    }
    static std::vector<float> mapped_normal_host(const std::vector<float> &in22) { // steps B-F on the host: rows of 22 -> (n.xyz | code 0..3)
        std::vector<float> out(in22.size() / 22 * 4);
        if (wfpt_mapped_normal_host(in22.data(), in22.size() / 22, out.data()) != WFPT_OK) throw Error(WFPT_ERR_INVALID_ARGUMENT, "wfpt_mapped_normal_host");
        return out;
    }
    // Roughness maps (WFPT_FLAG_ROUGHNESS_MAPS, include/wfpt.h "Roughness maps"): a material takes one channel of a texture slot as the
    // per-hit factor of its GGX alpha (glTF keeps roughness in g, perceptual: WFPT_ROUGHNESS_SQUARED); slot -1 unbinds.
    struct RoughnessMap {
        int32_t slot; // -1 = none
        uint32_t channel, remap;
    };
    void bind_roughness_map(uint32_t material_idx, int32_t slot, uint32_t channel = 1, uint32_t remap = WFPT_ROUGHNESS_LINEAR) {
        check(wfpt_bind_roughness_map(ctx_, material_idx, slot, channel, remap));
    }
    RoughnessMap roughness_map(uint32_t material_idx) {
        RoughnessMap m{-1, 0u, 0u};
        check(wfpt_get_roughness_map(ctx_, material_idx, &m.slot, &m.channel, &m.remap));
        return m;
    }
    std::vector<float> sample_roughness_map(const std::vector<float> &in4) { // (p.xyz | the triangle's bits) -> (alpha_h | r | code | 0)
        std::vector<float> out(in4.size() / 4 * 4);
        check(wfpt_sample_roughness_map(ctx_, in4.data(), in4.size() / 4, out.data()));
        return out;
    }
    static std::vector<float> hit_roughness_host(const std::vector<float> &in4, uint32_t channel, uint32_t remap) { // (alpha_m, c.rgb) -> (alpha_h, r)
        std::vector<float> out(in4.size() / 4 * 2);
        if (wfpt_hit_roughness_host(in4.data(), channel, remap, in4.size() / 4, out.data()) != WFPT_OK) throw Error(WFPT_ERR_INVALID_ARGUMENT, "wfpt_hit_roughness_host");
        return out;
    }
    // Emission (WFPT_FLAG_EMISSION, include/wfpt.h "Emission"): a material with a non-zero colour lights the scene and ends the paths that hit it.
    void set_emission(uint32_t material_idx, std::array<float, 3> rgb) { check(wfpt_set_emission(ctx_, material_idx, rgb.data())); }
    std::array<float, 3> emission(uint32_t material_idx) {
        std::array<float, 3> rgb{};
        check(wfpt_get_emission(ctx_, material_idx, rgb.data()));
        return rgb;
    }
    void clear_emission() { check(wfpt_clear_emission(ctx_)); }
    std::pair<float, uint32_t> emission_timing() { return timing(wfpt_emission_timing_ms); }
    // Next-event estimation (WFPT_FLAG_EMISSION | WFPT_FLAG_NEE, include/wfpt.h "Next-event estimation"): shadow rays from diffuse hits to the emitters.
    uint32_t nee_light_count() {
        const int n = wfpt_nee_light_count(ctx_);
        if (n < 0) check(n);
        return static_cast<uint32_t>(n);
    }
    std::pair<float, uint32_t> nee_timing() { return timing(wfpt_nee_timing_ms); }
    // rows of (p.xyz, n.xyz, u0, u1, u2) -> rows of (q.xyz, light primitive, e_q G rgb, occluded)
    std::vector<float> sample_lights(const std::vector<float> &in9) {
        std::vector<float> out(in9.size() / 9 * 8);
        check(wfpt_sample_lights(ctx_, in9.data(), in9.size() / 9, out.data()));
        return out;
    }
    // Light selection by power (WFPT_FLAG_EMISSION | WFPT_FLAG_NEE | WFPT_FLAG_LIGHT_POWER, include/wfpt.h "Light selection by power"):
    // (the emitting primitives in list order, the inclusive prefix sums of their integer weights)
    std::pair<std::vector<uint32_t>, std::vector<uint64_t>> light_distribution() {
        const size_t n = nee_light_count();
        std::pair<std::vector<uint32_t>, std::vector<uint64_t>> t{std::vector<uint32_t>(n), std::vector<uint64_t>(n)};
        check(wfpt_read_light_distribution(ctx_, t.first.data(), t.second.data()));
        return t;
    }
    // Analytic lights (WFPT_FLAG_EMISSION | WFPT_FLAG_NEE | WFPT_FLAG_ANALYTIC_LIGHTS, include/wfpt.h "Analytic lights"): point, spot and
    // directional lights for the connect pass; an empty vector clears them. lights() returns them as stored (directions normalised).
    void set_lights(const std::vector<wfpt_light> &lights) {
        check(wfpt_set_lights(ctx_, lights.empty() ? nullptr : lights.data(), static_cast<uint32_t>(lights.size())));
    }
    std::vector<wfpt_light> lights() {
        std::vector<wfpt_light> out(analytic_light_count());
        uint32_t n = 0;
        check(wfpt_get_lights(ctx_, out.empty() ? nullptr : out.data(), static_cast<uint32_t>(out.size()), &n));
        out.resize(std::min<size_t>(out.size(), n));
        return out;
    }
    uint32_t analytic_light_count() {
        const int n = wfpt_analytic_light_count(ctx_);
        if (n < 0) check(n);
        return static_cast<uint32_t>(n);
    }
    // Environment next-event estimation (the three flags above | WFPT_FLAG_ENVIRONMENT | WFPT_FLAG_ENV_NEE, include/wfpt.h "Environment
    // next-event estimation"): the map as one more light of the connect pass, sampled in proportion to its radiance.
    void set_environment_share(float share) { check(wfpt_set_environment_share(ctx_, share)); }
    float environment_share() const { return wfpt_environment_share(ctx_); }
    // (row: w * h prefix sums of the texel weights along the rows, marg: h prefix sums of the row totals) of a w x h map
    std::pair<std::vector<uint32_t>, std::vector<uint64_t>> environment_distribution(uint32_t w, uint32_t h) {
        std::pair<std::vector<uint32_t>, std::vector<uint64_t>> t{std::vector<uint32_t>(static_cast<size_t>(w) * h), std::vector<uint64_t>(h)};
        check(wfpt_read_environment_distribution(ctx_, t.first.data(), t.second.data()));
        return t;
    }
    // rows of (p.xyz, n.xyz, u1, u2, u3, u4) -> rows of (wdir.xyz, texel index, e Genv rgb, occluded)
    std::vector<float> sample_environment_light(const std::vector<float> &in10) {
        std::vector<float> out(in10.size() / 10 * 8);
        check(wfpt_sample_environment_light(ctx_, in10.data(), in10.size() / 10, out.data()));
        return out;
    }
    // Multiple importance sampling (WFPT_FLAG_EMISSION | WFPT_FLAG_NEE | WFPT_FLAG_MIS, include/wfpt.h "Multiple importance sampling"): emitter
    // hits of scattered rays and the connect pass's shadow rays, both weighed by the balance heuristic.
    // rows of (p.xyz, n.xyz, u0, u1, u2) -> rows of (q.xyz, light primitive, (e_q G) wl rgb, occluded, pl, pb, wl, 0)
    std::vector<float> sample_lights_mis(const std::vector<float> &in9) {
        std::vector<float> out(in9.size() / 9 * 12);
        check(wfpt_sample_lights_mis(ctx_, in9.data(), in9.size() / 9, out.data()));
        return out;
    }
    // rows of (o.xyz, d.xyz, t, primitive) -> rows of (pl, pb, wb, cos_l)
    std::vector<float> mis_hit_weight(const std::vector<float> &in8) {
        std::vector<float> out(in8.size() / 8 * 4);
        check(wfpt_mis_hit_weight(ctx_, in8.data(), in8.size() / 8, out.data()));
        return out;
    }
    // Environment multiple importance sampling (the four flags of environment next-event estimation | WFPT_FLAG_ENV_MIS, include/wfpt.h
    // "Environment multiple importance sampling"): the map's connect samples and the scattered rays' misses, both weighed.
    // rows of (p.xyz, n.xyz, u1, u2, u3, u4) -> rows of (wdir.xyz, texel index, (e Genv) we rgb, occluded, pe, pb, we, 0)
    std::vector<float> sample_environment_light_mis(const std::vector<float> &in10) {
        std::vector<float> out(in10.size() / 10 * 12);
        check(wfpt_sample_environment_light_mis(ctx_, in10.data(), in10.size() / 10, out.data()));
        return out;
    }
    // rows of an un-normalised direction -> rows of (pe, pb, wb, texel index)
    std::vector<float> env_mis_miss_weight(const std::vector<float> &dirs3) {
        std::vector<float> out(dirs3.size() / 3 * 4);
        check(wfpt_env_mis_miss_weight(ctx_, dirs3.data(), dirs3.size() / 3, out.data()));
        return out;
    }
    // Path termination (WFPT_FLAG_RETIRE, include/wfpt.h "Path termination"): dead paths are retired, and from wavefront roulette_start on
    // (0xffffffff: never) Russian roulette retires or re-weights the others with the survival probability's floor q_min, in (0, 1].
    void set_termination(uint32_t roulette_start = 3, float q_min = 0.05f) {
        wfpt_termination_params p;
        wfpt_termination_params_default(&p);
        p.roulette_start = roulette_start;
        p.q_min = q_min;
        check(wfpt_set_termination(ctx_, &p));
    }
    wfpt_termination_params termination() {
        wfpt_termination_params p;
        check(wfpt_get_termination(ctx_, &p));
        return p;
    }
    // rows of t' = thr * albedo and their pixels -> rows of (q, u, verdict, 0, thr'.rgb, 0); verdict 0 = dead, 1 = retired by roulette, 2 = survives
    std::vector<float> sample_termination(const std::vector<float> &thr3, const std::vector<uint32_t> &pixel_idx, uint32_t frame, uint32_t b) {
        if (thr3.size() != 3 * pixel_idx.size()) throw Error(WFPT_ERR_INVALID_ARGUMENT, "sample_termination: thr3 must hold 3 floats per pixel index");
        std::vector<float> out(pixel_idx.size() * 8);
        check(wfpt_sample_termination(ctx_, thr3.data(), pixel_idx.data(), frame, b, pixel_idx.size(), out.data()));
        return out;
    }
    // Adaptive sampling (WFPT_FLAG_ADAPTIVE, include/wfpt.h "Adaptive sampling"): a per-pixel active mask the renders obey, per-pixel sample
    // counts, and the device pass that turns the luminance moments into the next mask.
    void set_adaptive(const wfpt_adaptive_params &p) { check(wfpt_set_adaptive(ctx_, &p)); }
    static wfpt_adaptive_params adaptive_defaults() {
        wfpt_adaptive_params p;
        wfpt_adaptive_params_default(&p);
        return p;
    }
    wfpt_adaptive_params adaptive() {
        wfpt_adaptive_params p;
        check(wfpt_get_adaptive(ctx_, &p));
        return p;
    }
    // the number of pixels the next render adds samples to (blocking)
    uint32_t adaptive_update() {
        uint32_t n = 0;
        check(wfpt_adaptive_update(ctx_, &n));
        return n;
    }
    // one byte per pixel of the context, non-zero = active
    void set_active_mask(const std::vector<uint8_t> &mask) { check(wfpt_set_active_mask(ctx_, mask.data(), mask.size())); }
    std::vector<uint8_t> active_mask() {
        std::vector<uint8_t> m(wfpt_n_pixels(ctx_));
        check(wfpt_read_active_mask(ctx_, m.data(), m.size()));
        return m;
    }
    std::vector<uint32_t> sample_counts() {
        std::vector<uint32_t> n(wfpt_n_pixels(ctx_));
        check(wfpt_read_sample_counts(ctx_, n.data(), n.size()));
        return n;
    }
    // accumulated / count per pixel (0 where the count is 0), 3 floats per pixel
    std::vector<float> mean() {
        std::vector<float> rgb(3 * static_cast<size_t>(wfpt_n_pixels(ctx_)));
        check(wfpt_read_mean(ctx_, rgb.data(), rgb.size()));
        return rgb;
    }
    void mean_to_device(void *device_ptr, size_t n_bytes) { check(wfpt_copy_mean_to_device(ctx_, device_ptr, n_bytes)); }
    // render(interval) and adaptive_update() in turn until no pixel is active or max_passes passes are done; the pixels still active
    uint32_t render_adaptive(uint32_t max_passes, uint32_t interval) {
        uint32_t n = 0;
        check(wfpt_render_adaptive(ctx_, max_passes, interval, &n));
        return n;
    }
    // Multi-GPU (build-side addition, include/wfpt.h): this context was created with Options::tile_rank / tile_world;
    // rank 0 makes the 128-byte id with wfpt::comm_unique_id() and hands it to every rank.
    void comm_init(const std::array<uint8_t, WFPT_COMM_UNIQUE_ID_BYTES> &id, int rank, int world) { check(wfpt_comm_init(ctx_, id.data(), rank, world)); }
    void gather_accumulated() { check(wfpt_gather_accumulated(ctx_)); } // peers -> rank 0 over xGMI, asynchronous
    std::vector<float> gathered(uint32_t width, uint32_t height) {     // rank 0: the assembled frame
        std::vector<float> a(3 * static_cast<size_t>(width) * height);
        check(wfpt_read_gathered(ctx_, a.data(), a.size()));
        return a;
    }
    uint32_t last_wavefronts() const { return last_wavefronts_; }
    wfpt_ctx *handle() { return ctx_; }
    Kernel &generate_ray_kernel() { return generate_ray_kernel_; }
    Kernel &extend_kernel() { return extend_kernel_; }
    Kernel &shade_kernel() { return shade_kernel_; }
    Kernel &miss_kernel() { return miss_kernel_; }
    Kernel &accumulate_kernel() { return accumulate_kernel_; }

  private:
    void check(int st) const {
        if (st != WFPT_OK) throw Error(st, wfpt_last_error(ctx_));
    }
    // (milliseconds, launches) as one of the wfpt_*_timing_ms entry points reports them
    std::pair<float, uint32_t> timing(int (*entry)(wfpt_ctx *, float *, uint32_t *)) {
        float ms = 0.0f;
        uint32_t n = 0;
        check(entry(ctx_, &ms, &n));
        return {ms, n};
    }
    wfpt_ctx *ctx_ = nullptr;
    RenderParameters render_parameters_;
    RenderProgress render_progress_;
    Options opt_;
    BVHTree bvh_tree_;
    Kernel generate_ray_kernel_, extend_kernel_, shade_kernel_, miss_kernel_, accumulate_kernel_;
    uint32_t last_wavefronts_ = 0;
};

inline std::array<uint8_t, WFPT_COMM_UNIQUE_ID_BYTES> comm_unique_id() {
    std::array<uint8_t, WFPT_COMM_UNIQUE_ID_BYTES> id{};
    const int st = wfpt_comm_unique_id(id.data());
    if (st != WFPT_OK) throw Error(st, wfpt_last_error(nullptr));
    return id;
}

} // namespace wfpt
