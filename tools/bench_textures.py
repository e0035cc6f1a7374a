#!/usr/bin/env python3
"""tools/bench_textures.py: frame time with and without surface textures (WFPT_FLAG_TEXTURES).

Legs, --spp samples per frame: `<scene>:plain` no flag, `<scene>:textured` the flag with textures bound --
  shirley at --width x --height: a 2048x2048 checker on the ground sphere's material and a 512x512 texture on every Lambertian material;
  mesh, the 1M-triangle soup: procedural UVs (one row per triangle) and one 2048x2048 texture on material 0,
and, with --parent-tree DIR (a checkout of the parent commit with its library built), every leg once more in that tree, named
`<leg>@parent` and run right after its twin.

Method: tools/ab_bench.py's. The texture launches' own time and their share of a timed frame come from
wfpt_texture_timing_ms against the stage times."""
import json
import sys

import ab_bench as ab

EXTRA_KEYS, DIGITS = ("texture_ms_timed", "texture_launches_timed", "texture_launch_share_timed"), 4


def leg(a):
    sys.path.insert(0, a.tree)
    import numpy as np
    import wavefront_path_tracer_amd as W
    scene, kind = a.leg.split(":")
    flags = W.FLAG_TEXTURES if kind == "textured" else 0
    if scene == "shirley":
        pt = W.shirley_path_tracer(a.width, a.height, max_wavefronts=a.bounces, rng_mode=W.RNG_DISPATCH, flags=flags, batch=64)
    else:
        pt = W.mesh_path_tracer(a.width, a.height, a.triangles, max_wavefronts=a.bounces, rng_mode=W.RNG_DISPATCH, flags=flags, batch=64)
    rng = np.random.default_rng(1)
    if kind == "textured" and scene == "shirley":
        sp, mt = pt.scene.spheres, pt.scene.materials
        ground = int(sp["material_idx"][np.argmax(sp["radius"])])
        y, x = np.mgrid[0:2048, 0:2048]
        c = ((x * 32 // 2048 + y * 32 // 2048) % 2).astype(np.float32)
        pt.set_texture(0, np.stack([0.2 + 0.7 * c, 0.2 + 0.7 * c, 0.2 + 0.7 * c], axis=-1).astype(np.float32))
        pt.set_texture(1, rng.random((512, 512, 3), dtype=np.float32))
        pt.bind_texture(ground, 0)
        for m in np.flatnonzero(mt["material_type"] == 0):
            if int(m) != ground:
                pt.bind_texture(int(m), 1)
    elif kind == "textured":
        # the soup's triangles are in BVH order with row 0 each: one procedural row per triangle instead
        pt.scene.triangles["_pad"] = np.arange(a.triangles, dtype=np.uint32)
        pt.update_scene(pt.scene)
        uv = np.tile(np.float32([0.0, 0.0, 1.0, 0.0, 0.0, 1.0]), (a.triangles, 1)) + rng.random((a.triangles, 1), dtype=np.float32) * 4.0
        pt.set_triangle_uvs(uv)
        pt.set_texture(0, rng.random((2048, 2048, 3), dtype=np.float32))
        pt.bind_texture(0, 0)
    out = {"leg": a.leg, "loop": pt.loop_kind, "frame_ms": ab.timed_frames(pt, a.spp, a.frames)}
    if kind == "textured":
        stage_ms, _ = pt.render_timed(a.spp)
        tex_ms, launches = pt.texture_timing()
        out.update(texture_ms_timed=tex_ms, texture_launches_timed=launches,
                   texture_launch_share_timed=tex_ms / max(float(np.sum(stage_ms)) + tex_ms, 1e-9))
    print(json.dumps(out), flush=True)
    pt.close()


def options():
    ap = ab.parser(frames=5)
    ap.add_argument("--scenes", nargs="+", default=["shirley", "mesh"])
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its libwfpt.so built")
    return ap


def legs(a):
    return ab.with_twins([ab.entry(f"{scene}:{kind}") for scene in a.scenes for kind in ("plain", "textured")], a.parent_tree)


def main():
    a = options().parse_args()
    if a.leg:
        return leg(a)
    summary = ab.summarise(ab.run_legs(__file__, legs(a), a), a, EXTRA_KEYS, DIGITS)
    rel = ab.ratios(summary, [(f"{scene}:textured", f"{scene}:plain") for scene in a.scenes] + ab.twin_pairs(summary))
    print(json.dumps({"summary": rel}), flush=True)


if __name__ == "__main__":
    main()
