#!/usr/bin/env python3
"""tools/bench_textures.py: frame time with and without surface textures (WFPT_FLAG_TEXTURES).

Legs, --spp samples per frame: `<scene>:plain` no flag, `<scene>:textured` the flag with textures bound --
  shirley at --width x --height: a 2048x2048 checker on the ground sphere's material and a 512x512 texture on every Lambertian material;
  mesh, the 1M-triangle soup: procedural UVs (one row per triangle) and one 2048x2048 texture on material 0,
and, with --parent-tree DIR (a checkout of the parent commit with its library built), every leg once more in that tree, named
`<leg>@parent` and run right after its twin.

Method (tools/bench_nee.py's): every leg runs in a fresh child process, --rounds times, the legs alternating within a round so that
drift hits them alike. A child warms up (graph capture, first touch of the textures), then times --frames frames one by one, each ending
in a device synchronise. A leg's figure is the median of all its frames; its spread is the range of its per-round medians. The texture
launches' own time and their share of a timed frame come from wfpt_texture_timing_ms against the stage times. Prints one JSON line per
leg and one summary line."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    pt.render(a.spp)  # warm-up: graph capture, first touch of the textures
    pt.synchronize()
    ms = []
    for _ in range(a.frames):
        t0 = time.perf_counter()
        pt.render(a.spp)
        pt.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    out = {"leg": a.leg, "loop": pt.loop_kind, "frame_ms": ms}
    if kind == "textured":
        stage_ms, _ = pt.render_timed(a.spp)
        tex_ms, launches = pt.texture_timing()
        out.update(texture_ms_timed=tex_ms, texture_launches_timed=launches,
                   texture_launch_share_timed=tex_ms / max(float(np.sum(stage_ms)) + tex_ms, 1e-9))
    print(json.dumps(out), flush=True)
    pt.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--triangles", type=int, default=1000000)
    ap.add_argument("--scenes", nargs="+", default=["shirley", "mesh"])
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its libwfpt.so built")
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        return leg(a)
    legs = [(f"{scene}:{kind}", ROOT) for scene in a.scenes for kind in ("plain", "textured")]
    if a.parent_tree:
        legs = [x for name, tree in legs for x in ((name, tree), (name + "@parent", os.path.abspath(a.parent_tree)))]
    results = {name: {"rounds": [], "last": None} for name, _ in legs}
    for _ in range(a.rounds):
        for name, tree in legs:
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", name.split("@")[0], "--tree", tree, "--width", str(a.width), "--height",
                   str(a.height), "--spp", str(a.spp), "--bounces", str(a.bounces), "--frames", str(a.frames), "--triangles", str(a.triangles)]
            env = dict(os.environ)
            env.pop("WFPT_LIB", None)  # each tree loads its own library
            res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, env=env, timeout=600)  # a failed or hung leg ends the run
            if res.returncode != 0:
                sys.exit(f"bench_textures: leg {name} failed with status {res.returncode}")
            r = json.loads(res.stdout.strip().splitlines()[-1])
            results[name]["rounds"].append(r["frame_ms"])
            results[name]["last"] = r
            print(f"{name}: {statistics.median(r['frame_ms']):.3f} ms", file=sys.stderr, flush=True)  # progress; the figures follow
    summary = {}
    for name, _ in legs:
        rounds = results[name]["rounds"]
        per_round = [statistics.median(r) for r in rounds]
        line = {"leg": name, "loop": results[name]["last"]["loop"], "size": [a.width, a.height], "spp": a.spp, "bounces": a.bounces,
                "frames": a.frames, "rounds": a.rounds, "frame_ms_median": round(statistics.median(x for r in rounds for x in r), 3),
                "round_medians_ms": [round(x, 3) for x in per_round], "spread_ms": round(max(per_round) - min(per_round), 3)}
        for k in ("texture_ms_timed", "texture_launches_timed", "texture_launch_share_timed"):
            if k in results[name]["last"]:
                line[k] = round(results[name]["last"][k], 4) if isinstance(results[name]["last"][k], float) else results[name]["last"][k]
        summary[name] = line
        print(json.dumps(line), flush=True)
    rel = {}
    twins = [(name, name + "@parent") for name, _ in legs if not name.endswith("@parent")]
    for name, base in [(f"{scene}:textured", f"{scene}:plain") for scene in a.scenes] + twins:
        if name in summary and base in summary:
            rel[f"{name} over {base}"] = round(summary[name]["frame_ms_median"] / summary[base]["frame_ms_median"] - 1.0, 4)
    print(json.dumps({"summary": rel}), flush=True)


if __name__ == "__main__":
    main()
