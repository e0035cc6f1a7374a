#!/usr/bin/env python3
"""tools/bench_textures.py: frame time with and without surface textures (WFPT_FLAG_TEXTURES).

For each scene two contexts render --spp samples per frame: no flag, then the flag with textures bound --
  Shirley at 1920x1080: a 2048x2048 checker on the ground sphere's material and a 512x512 texture on every Lambertian material;
  the 1M-triangle soup: procedural UVs (one row per triangle) and one 2048x2048 texture on material 0.
The texture launches' share of a timed frame comes from wfpt_texture_timing_ms against the stage times. Prints one JSON line per scene."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import wavefront_path_tracer_amd as W  # noqa: E402


def frame_ms(pt, spp, frames):
    pt.render(spp)  # warm-up: graph capture, first touch of the textures
    pt.synchronize()
    t0 = time.perf_counter()
    for _ in range(frames):
        pt.render(spp)
    pt.synchronize()
    return (time.perf_counter() - t0) * 1e3 / frames


def make(scene, w, h, bounces, flags, tris):
    if scene == "shirley":
        return W.shirley_path_tracer(w, h, max_wavefronts=bounces, rng_mode=W.RNG_DISPATCH, flags=flags, batch=64)
    return W.mesh_path_tracer(w, h, tris, max_wavefronts=bounces, rng_mode=W.RNG_DISPATCH, flags=flags, batch=64)


def checker(n, cells=32):
    y, x = np.mgrid[0:n, 0:n]
    c = ((x * cells // n + y * cells // n) % 2).astype(np.float32)
    return np.stack([0.2 + 0.7 * c, 0.2 + 0.7 * c, 0.2 + 0.7 * c], axis=-1).astype(np.float32)


def texture(pt, scene, rng, n_tris):
    if scene == "shirley":
        sp, mt = pt.scene.spheres, pt.scene.materials
        ground = int(sp["material_idx"][np.argmax(sp["radius"])])
        pt.set_texture(0, checker(2048))
        pt.set_texture(1, rng.random((512, 512, 3), dtype=np.float32))
        pt.bind_texture(ground, 0)
        for m in np.flatnonzero(mt["material_type"] == 0):
            if int(m) != ground:
                pt.bind_texture(int(m), 1)
    else:
        # the soup's triangles are in BVH order with row 0 each: one procedural row per triangle instead
        pt.scene.triangles["_pad"] = np.arange(n_tris, dtype=np.uint32)
        pt.update_scene(pt.scene)
        uv = np.tile(np.float32([0.0, 0.0, 1.0, 0.0, 0.0, 1.0]), (n_tris, 1)) + rng.random((n_tris, 1), dtype=np.float32) * 4.0
        pt.set_triangle_uvs(uv)
        pt.set_texture(0, rng.random((2048, 2048, 3), dtype=np.float32))
        pt.bind_texture(0, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--triangles", type=int, default=1000000)
    ap.add_argument("--scenes", nargs="+", default=["shirley", "mesh"])
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    for scene in a.scenes:
        plain = make(scene, a.width, a.height, a.bounces, 0, a.triangles)
        ms_plain = frame_ms(plain, a.spp, a.frames)
        plain.close()
        tex = make(scene, a.width, a.height, a.bounces, W.FLAG_TEXTURES, a.triangles)
        texture(tex, scene, rng, a.triangles)
        ms_tex = frame_ms(tex, a.spp, a.frames)
        stage_ms, _ = tex.render_timed(a.spp)
        tex_ms, launches = tex.texture_timing()
        share = tex_ms / max(float(np.sum(stage_ms)) + tex_ms, 1e-9)
        print(json.dumps({"scene": scene, "loop": tex.loop_kind, "size": [a.width, a.height], "spp": a.spp, "bounces": a.bounces,
                          "frame_ms_plain": round(ms_plain, 3), "frame_ms_textured": round(ms_tex, 3),
                          "textured_over_plain": round(ms_tex / ms_plain - 1.0, 4), "texture_launches_timed": launches,
                          "texture_launch_share_timed": round(share, 4)}), flush=True)
        tex.close()


if __name__ == "__main__":
    main()
