/* examples/wfpt_render.c -- the whole path through the C ABI (include/wfpt.h) from plain C99, the way the reference's
 * main.rs + PathTracer::new + PathTracer::run use it (gpu_wavefront_pt/src/main.rs:17-36, path_tracer.rs:43-371).
 *
 *   gcc -std=c99 -O1 -Iinclude examples/wfpt_render.c -Lwavefront_path_tracer_amd -lwfpt \
 *       -Wl,-rpath,$PWD/wavefront_path_tracer_amd -lm -o wfpt_render
 *   ./wfpt_render out.ppm [width height spp bounces [device_bvh]] [--obj-normals mesh.obj [--roughness alpha | --rough-glass alpha]
 *                 [--roughness-map] [--normal-map strength]] [--adaptive]
 * --adaptive: a WFPT_FLAG_ADAPTIVE context rendered with wfpt_render_adaptive (at most spp passes, an update every 8) at the default
 * parameters; the image written is the mean (each pixel divided by its own sample count).
 * --obj-normals mesh.obj: instead of the book's scene, the triangles of a Wavefront OBJ file (grey Lambertian, about the origin, seen from
 * (0, 1, 4.5)) shaded with the file's `vn` vertex normals: a WFPT_FLAG_SHADING_NORMALS context and wfpt_set_triangle_normals.
 * --roughness alpha (after --obj-normals mesh.obj): the mesh is a metal of that albedo with the GGX roughness alpha in (0, 1] instead:
 * WFPT_FLAG_MICROFACET as well, and wfpt_set_roughness.
 * --rough-glass alpha (after --obj-normals mesh.obj): the mesh is a white dielectric of refraction index 1.5 with the GGX roughness alpha
 * in (0, 1] -- frosted glass: WFPT_FLAG_MICROFACET | WFPT_FLAG_ROUGH_DIELECTRIC, and wfpt_set_roughness on the dielectric material.
 * --roughness-map (after --roughness alpha or --rough-glass alpha): the mesh's material takes the green channel of a procedural 64 x 64
 * map of brushed bands (factors from 0.1 to 1, a polished stripe of exact zeros) as its roughness map, through the file's `vt` UVs:
 * WFPT_FLAG_TEXTURES | WFPT_FLAG_ROUGHNESS_MAPS as well, wfpt_set_triangle_uvs, wfpt_set_texture and wfpt_bind_roughness_map.
 * --normal-map strength (after --obj-normals mesh.obj and its roughness options): the mesh's material takes a procedural 64 x 64 map of
 * ripples as its tangent-space normal map at that strength (> 0), through the file's `vt` UVs: WFPT_FLAG_TEXTURES |
 * WFPT_FLAG_NORMAL_MAPS as well, wfpt_set_triangle_uvs, wfpt_set_texture and wfpt_bind_normal_map.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "wfpt.h"

#define CHECK(call)                                                             \
    do {                                                                        \
        int st_ = (call);                                                       \
        if (st_ != WFPT_OK) {                                                   \
            fprintf(stderr, "%s -> %d: %s\n", #call, st_, wfpt_last_error(ctx)); \
            return 1;                                                           \
        }                                                                       \
    } while (0)

int main(int argc, char **argv) {
    wfpt_ctx *ctx = NULL;
    int adaptive = 0;
    const char *obj = NULL;
    if (argc > 2 && strcmp(argv[argc - 1], "--adaptive") == 0) {
        adaptive = 1;
        argc -= 1;
    }
    float roughness = 0.0f, map_strength = 0.0f;
    int glass = 0, roughness_map = 0;
    if (argc > 5 && strcmp(argv[argc - 2], "--normal-map") == 0) {
        map_strength = (float)atof(argv[argc - 1]);
        argc -= 2;
    }
    if (argc > 6 && strcmp(argv[argc - 1], "--roughness-map") == 0) {
        roughness_map = 1;
        argc -= 1;
    }
    if (argc > 5 && (strcmp(argv[argc - 2], "--roughness") == 0 || strcmp(argv[argc - 2], "--rough-glass") == 0)) {
        glass = strcmp(argv[argc - 2], "--rough-glass") == 0;
        roughness = (float)atof(argv[argc - 1]);
        argc -= 2;
    }
    if (argc > 3 && strcmp(argv[argc - 2], "--obj-normals") == 0) {
        obj = argv[argc - 1];
        argc -= 2;
    }
    if (argc < 2 || ((roughness != 0.0f || map_strength != 0.0f) && !obj) || (glass && !(roughness > 0.0f)) || map_strength < 0.0f || (roughness_map && !(roughness > 0.0f))) {
        fprintf(stderr, "usage: %s out.ppm [width height spp bounces [device_bvh]] [--obj-normals mesh.obj [--roughness alpha | --rough-glass alpha] [--roughness-map] [--normal-map strength]] [--adaptive]\n", argv[0]);
        return 2;
    }
    const uint32_t width = argc > 3 ? (uint32_t)atoi(argv[2]) : 400, height = argc > 3 ? (uint32_t)atoi(argv[3]) : 225;
    const uint32_t spp = argc > 4 ? (uint32_t)atoi(argv[4]) : 8, bounces = argc > 5 ? (uint32_t)atoi(argv[5]) : 8;
    const int device_bvh = argc > 6 ? atoi(argv[6]) : 0;
    if (obj) { /* a mesh with per-vertex normals (build extension; include/wfpt.h "Shading normals") */
        uint32_t n_tris = 0, n_mesh_nodes = 0;
        CHECK(wfpt_load_obj_normals(obj, NULL, NULL, NULL, 0, &n_tris, 0, 0));
        if (n_tris == 0) {
            fprintf(stderr, "%s holds no triangle\n", obj);
            return 1;
        }
        wfpt_triangle *tris = (wfpt_triangle *)calloc(n_tris, sizeof *tris);
        float *n9 = (float *)calloc(9u * (size_t)n_tris, sizeof *n9);
        float *uv6 = (float *)calloc(6u * (size_t)n_tris, sizeof *uv6);
        wfpt_bvh_node *mesh_nodes = (wfpt_bvh_node *)calloc(2u * (size_t)n_tris, sizeof *mesh_nodes);
        wfpt_material grey;
        memset(&grey, 0, sizeof grey);
        grey.albedo[0] = grey.albedo[1] = grey.albedo[2] = 0.7f;
        grey.albedo[3] = 1.0f;
        if (glass) { /* include/wfpt.h "Rough dielectrics" */
            grey.albedo[0] = grey.albedo[1] = grey.albedo[2] = 1.0f;
            grey.refract_index = 1.5f;
            grey.material_type = 2u;
        }
        CHECK(wfpt_load_obj_normals(obj, tris, uv6, n9, n_tris, &n_tris, 0, glass ? 2u : roughness > 0.0f ? 1u : 0u)); /* triangle i: _pad = i, row i of n9; --roughness: Metal, --rough-glass: Dielectric */
        CHECK(wfpt_build_bvh_triangles(tris, n_tris, mesh_nodes, 2u * n_tris, &n_mesh_nodes, 32)); /* reorders: the rows follow by _pad */
        const float from[3] = {0.0f, 1.0f, 4.5f}, at[3] = {0.0f, 0.0f, 0.0f};
        float pitch, yaw, view[16], inv_proj[16];
        wfpt_gpu_camera camera;
        wfpt_camera_new(from, at, &pitch, &yaw);
        wfpt_view_transform(from, pitch, yaw, view);
        wfpt_p_inv(wfpt_to_radians(40.0f), (float)width / (float)height, 0.1f, 100.0f, inv_proj);
        wfpt_gpu_camera_new(from, pitch, yaw, 0.0f, 10.0f, &camera);
        wfpt_params params;
        memset(&params, 0, sizeof params);
        params.width = width;
        params.height = height;
        params.max_wavefronts = bounces;
        params.miss_floor = 128;
        params.flags = WFPT_FLAG_SHADING_NORMALS | (roughness > 0.0f ? WFPT_FLAG_MICROFACET : 0u) | (glass ? WFPT_FLAG_ROUGH_DIELECTRIC : 0u) | (adaptive ? WFPT_FLAG_ADAPTIVE : 0u) |
                       (map_strength > 0.0f ? WFPT_FLAG_TEXTURES | WFPT_FLAG_NORMAL_MAPS : 0u) | (roughness_map ? WFPT_FLAG_TEXTURES | WFPT_FLAG_ROUGHNESS_MAPS : 0u);
        ctx = wfpt_create_mesh(&params, tris, n_tris, &grey, 1, mesh_nodes, n_mesh_nodes, &camera, inv_proj, view);
        if (!ctx) {
            fprintf(stderr, "wfpt_create_mesh: %s\n", wfpt_last_error(NULL));
            return 1;
        }
        CHECK(wfpt_set_triangle_normals(ctx, n9, n_tris));
        if (roughness > 0.0f) CHECK(wfpt_set_roughness(ctx, 0, roughness)); /* include/wfpt.h "Microfacet metals", "Rough dielectrics" */
        if (roughness_map) { /* include/wfpt.h "Roughness maps": slot 1's green channel scales alpha per hit; 8 bands along u, every fourth polished */
            enum { RMAP = 64 };
            float *rgb = (float *)calloc(3u * RMAP * RMAP, sizeof *rgb);
            for (int row = 0; row < RMAP; ++row)
                for (int col = 0; col < RMAP; ++col) {
                    const int band = col / (RMAP / 8);
                    const float u = ((float)col + 0.5f) / RMAP;
                    rgb[3 * (row * RMAP + col) + 1] = band % 4 == 3 ? 0.0f : 0.55f + 0.45f * sinf(8.0f * 6.2831853f * u);
                }
            CHECK(wfpt_set_triangle_uvs(ctx, uv6, n_tris));
            CHECK(wfpt_set_texture(ctx, 1, rgb, RMAP, RMAP, NULL));
            CHECK(wfpt_bind_roughness_map(ctx, 0, 1, 1, WFPT_ROUGHNESS_LINEAR));
            free(rgb);
        }
        if (map_strength > 0.0f) { /* include/wfpt.h "Normal maps": rgb = 0.5 + 0.5 n of the height field 0.02 sin(8 2pi u) sin(8 2pi v), green = +v, row 0 = the top */
            enum { MAP = 64 };
            float *rgb = (float *)calloc(3u * MAP * MAP, sizeof *rgb);
            const float k = 8.0f * 6.2831853f, amp = 0.02f;
            for (int row = 0; row < MAP; ++row)
                for (int col = 0; col < MAP; ++col) {
                    const float u = ((float)col + 0.5f) / MAP, v = 1.0f - ((float)row + 0.5f) / MAP;
                    const float dhu = amp * k * cosf(k * u) * sinf(k * v), dhv = amp * k * sinf(k * u) * cosf(k * v);
                    const float il = 1.0f / sqrtf(dhu * dhu + dhv * dhv + 1.0f);
                    float *c = rgb + 3 * (row * MAP + col);
                    c[0] = 0.5f - 0.5f * dhu * il;
                    c[1] = 0.5f - 0.5f * dhv * il;
                    c[2] = 0.5f + 0.5f * il;
                }
            CHECK(wfpt_set_triangle_uvs(ctx, uv6, n_tris));
            CHECK(wfpt_set_texture(ctx, 0, rgb, MAP, MAP, NULL));
            CHECK(wfpt_bind_normal_map(ctx, 0, 0, map_strength));
            free(rgb);
        }
        uint32_t still = 0;
        if (adaptive) CHECK(wfpt_render_adaptive(ctx, spp, 8, &still));
        else CHECK(wfpt_render(ctx, spp));
        CHECK(wfpt_save_ppm(ctx, argv[1]));
        printf("%ux%u, %u spp, %u bounces: %u triangles of %s with their vertex normals -> %s\n", width, height, spp, bounces, n_tris, obj, argv[1]);
        wfpt_destroy(ctx);
        free(mesh_nodes);
        free(n9);
        free(uv6);
        free(tris);
        return 0;
    }

    /* main.rs:20: the book's final scene (seeded here), path_tracer.rs:117-118: its BVH */
    wfpt_sphere spheres[512];
    wfpt_material materials[512];
    const uint32_t n = wfpt_scene_book_one_final(1, spheres, materials, 512);
    wfpt_bvh_node *nodes = (wfpt_bvh_node *)calloc(2u * n, sizeof *nodes);
    uint32_t n_nodes = 0;
    if (device_bvh) CHECK(wfpt_build_bvh_device(spheres, n, nodes, 2u * n, &n_nodes, 0, NULL)); /* build extension */
    else CHECK(wfpt_build_bvh(spheres, n, nodes, 2u * n, &n_nodes));

    /* main.rs:23-32: camera (13,2,3) -> origin, vfov 20, defocus angle 0.6, focus distance 10 */
    const float look_from[3] = {13.0f, 2.0f, 3.0f}, look_at[3] = {0.0f, 0.0f, 0.0f};
    float pitch, yaw, view[16], inv_proj[16];
    wfpt_gpu_camera camera;
    wfpt_camera_new(look_from, look_at, &pitch, &yaw);
    wfpt_view_transform(look_from, pitch, yaw, view);
    wfpt_p_inv(wfpt_to_radians(20.0f), (float)width / (float)height, 0.1f, 100.0f, inv_proj); /* path_tracer.rs:135-138 */
    wfpt_gpu_camera_new(look_from, pitch, yaw, wfpt_to_radians(0.6f), 10.0f, &camera);

    wfpt_params params;
    memset(&params, 0, sizeof params);
    params.width = width;
    params.height = height;
    params.max_wavefronts = bounces; /* path_tracer.rs:323 uses 50 */
    params.miss_floor = 128;         /* path_tracer.rs:332 */
    if (adaptive) params.flags |= WFPT_FLAG_ADAPTIVE;
    ctx = wfpt_create(&params, spheres, n, materials, n, nodes, n_nodes, &camera, inv_proj, view);
    if (!ctx) {
        fprintf(stderr, "wfpt_create: %s\n", wfpt_last_error(NULL));
        return 1;
    }
    uint32_t n_active = 0;
    if (adaptive) CHECK(wfpt_render_adaptive(ctx, spp, 8, &n_active)); /* render 8 passes, make the next mask of the moments, and again */
    else CHECK(wfpt_render(ctx, spp)); /* the loop of path_tracer.rs:291-368, resident on the device */
    CHECK(wfpt_save_ppm(ctx, argv[1])); /* (a flagged context writes its mean) */
    if (adaptive) {
        uint32_t *counts = (uint32_t *)calloc((size_t)width * height, sizeof *counts);
        unsigned long long samples = 0;
        CHECK(wfpt_read_sample_counts(ctx, counts, (size_t)width * height));
        for (size_t i = 0; i < (size_t)width * height; ++i) samples += counts[i];
        printf("adaptive: %u passes, %.2f samples per pixel, %u pixels still active\n", wfpt_accumulated_samples(ctx),
               (double)samples / ((double)width * height), n_active);
        free(counts);
    }
    uint64_t totals[4];
    CHECK(wfpt_read_totals(ctx, totals));
    printf("%ux%u, %u spp, %u bounces: %llu rays, %u BVH nodes%s -> %s\n", width, height, spp, bounces,
           (unsigned long long)totals[0], n_nodes, device_bvh ? " (built on the device)" : "", argv[1]);
    wfpt_destroy(ctx);
    free(nodes);
    return 0;
}
