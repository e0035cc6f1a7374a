#!/usr/bin/env python3
"""tools/bench_roughness_maps.py: what roughness maps cost per frame (WFPT_FLAG_ROUGHNESS_MAPS).

Legs, --spp samples per frame at --width x --height, the 1 M-triangle soup and the mesh camera of BASELINE config 5 (the soup's materials
by thirds: Lambertian, Metal, Dielectric), seeded UV rows and a seeded --map x --map map of factors in [0, 1.25):
  parent       the soup on the PARENT commit's library (--parent-root: a checkout of it with its library built); no flag
  off          the same on this tree, no flag                               (must lie within the spread of `parent`'s round medians)
  empty        TEXTURES | MICROFACET | ROUGH_DIELECTRIC | ROUGHNESS_MAPS, nothing set or bound (the launches of `off`; the same criterion)
  base         TEXTURES | MICROFACET | ROUGH_DIELECTRIC, the metal and the glass third at alpha 0.3   (rough_glass_kernel)
  mapped       `base` plus the flag and the map's green channel bound on both thirds                  (rough_glass_rmap_kernel)
  mapped_nmap  `mapped` plus bench_normal_maps.py's setup: SHADING_NORMALS | NORMAL_MAPS, a table of corner normals and a normal map
               on all three materials                                        (rough_glass_rmap_kernel, both lookups from one (u, v))

Method: tools/ab_bench.py's. The pass's own time comes from wfpt_microfacet_timing_ms over one timed frame
(hipEvent pairs around every launch, so it is slower than the frame it describes), beside the sum of that frame's stage times. The
parent prints a first line {"stamp": ...} with the command, the commit, the device and the date."""
import datetime
import json
import os
import subprocess
import sys

import ab_bench as ab

EXTRA_KEYS, DIGITS = ("triangles", "pass_ms_timed", "pass_launches_timed", "stages_ms_timed"), 6
ROUGH = ("base", "mapped", "mapped_nmap")
MAPPED = ("mapped", "mapped_nmap")
METAL, GLASS, ALPHA = 1, 2, 0.3


def leg(a):
    sys.path.insert(0, a.tree)
    import numpy as np
    import wavefront_path_tracer_amd as W
    if a.leg == "device":  # (the stamp's device name: a child of its own, so that the parent never opens the GPU)
        import torch
        print(json.dumps({"device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else "none"}), flush=True)
        return
    flags = 0
    if a.leg in ROUGH + ("empty",):
        flags |= W.FLAG_TEXTURES | W.FLAG_MICROFACET | W.FLAG_ROUGH_DIELECTRIC
    if a.leg in MAPPED + ("empty",):
        flags |= W.FLAG_ROUGHNESS_MAPS
    if a.leg == "mapped_nmap":
        flags |= W.FLAG_SHADING_NORMALS | W.FLAG_NORMAL_MAPS
    scene = W.Scene.random_mesh(a.triangles, 1)
    rng = np.random.default_rng(7)
    if flags:
        scene.triangles["_pad"] = np.arange(len(scene.triangles), dtype=np.uint32)
    cc = W.CameraController(W.Camera((0.0, 0.0, 30.0), (0.0, 0.0, 0.0)), 40.0, 0.0, 10.0, 0.1, 100.0)
    pt = W.PathTracer(scene, W.RenderParameters(cc, (a.width, a.height)), max_wavefronts=a.bounces, rng_mode=W.RNG_DISPATCH, flags=flags,
                      batch=a.batch, device_bvh=True)
    if a.leg in ROUGH:  # (bench_normal_maps.py's draws, in its order: the table of normals, then the UV rows)
        t = scene.triangles
        face = np.cross(t["e1"].astype(np.float64), t["e2"].astype(np.float64))
        face /= np.linalg.norm(face, axis=1)[:, None]
        n9 = (face[:, None, :] + 0.3 * rng.normal(size=(len(t), 3, 3))).reshape(-1, 9).astype(np.float32)
        pt.set_triangle_uvs(rng.random((len(t), 6), dtype=np.float32))
        pt.set_roughness(METAL, ALPHA)
        pt.set_roughness(GLASS, ALPHA)
    if a.leg == "mapped_nmap":
        pt.set_triangle_normals(n9)
        theta, phi = rng.uniform(0.0, 0.7, (a.map, a.map)), rng.uniform(0.0, 2.0 * np.pi, (a.map, a.map))
        img = 0.5 + 0.5 * np.stack([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)], 2)
        pt.set_texture(0, img.astype(np.float32))
        for m in range(3):
            pt.bind_normal_map(m, 0, 1.0)
    if a.leg in MAPPED:
        pt.set_texture(1, np.random.default_rng(8).uniform(0.0, 1.25, (a.map, a.map, 3)).astype(np.float32))
        for m in (METAL, GLASS):
            pt.bind_roughness_map(m, 1, 1, "linear")
    ms = ab.timed_frames(pt, a.spp, a.frames)
    stage_ms, _ = pt.render_timed(a.spp)
    pass_ms, launches = pt.microfacet_timing_ms() if a.leg in ROUGH + ("empty",) else (0.0, 0)
    print(json.dumps({"leg": a.leg, "loop": pt.loop_kind, "triangles": len(scene.triangles), "frame_ms": ms, "pass_ms_timed": pass_ms,
                      "pass_launches_timed": launches, "stages_ms_timed": float(np.sum(stage_ms))}), flush=True)
    pt.close()


def options():
    ap = ab.parser(frames=12)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--map", type=int, default=1024, help="the maps' edge in texels")
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with its library built (the `parent` leg)")
    ap.add_argument("--legs", nargs="+", default=["parent", "off", "empty", "base", "mapped", "mapped_nmap"])
    ap.add_argument("--commit", default=None, help="the stamp's commit where the tree carries no git data")
    return ap


def legs(a):
    return [ab.entry(name, "off", a.parent_root) if name == "parent" else ab.entry(name) for name in a.legs if name != "parent" or a.parent_root]


def stamp(a):
    git = lambda *cmd: subprocess.run(("git", "-C", ab.ROOT) + cmd, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True).stdout.strip()
    device = ab.run_child(__file__, ab.entry("device"), a)["device"]
    return {"command": "python tools/" + os.path.basename(__file__) + " " + " ".join(sys.argv[1:]), "commit": a.commit or git("rev-parse", "HEAD") or "unknown",
            "dirty": bool(git("status", "--porcelain")), "device": device, "date": datetime.datetime.now(datetime.timezone.utc).strftime("%Y-%m-%dT%H:%M:%SZ")}


def main():
    a = options().parse_args()
    if a.leg:
        return leg(a)
    print(json.dumps({"stamp": stamp(a)}), flush=True)
    summary = ab.summarise(ab.run_legs(__file__, legs(a), a), a, EXTRA_KEYS, DIGITS)
    rel = ab.ratios(summary, (("off", "parent"), ("empty", "off"), ("base", "off"), ("mapped", "base"), ("mapped_nmap", "mapped")), ", frame")
    for name in ("off", "empty"):
        if name in summary and "parent" in summary:
            p = summary["parent"]["round_medians_ms"]
            rel[f"{name} within the spread of parent's round medians"] = bool(min(p) <= summary[name]["frame_ms_median"] <= max(p))
    for name in ROUGH:
        if name in summary:
            p, s = summary[name]["pass_ms_timed"], summary[name]["stages_ms_timed"]  # (the pass is booked apart from the stages)
            rel[f"{name}: pass share of the timed frame"] = round(p / (p + s), 4)
    print(json.dumps({"summary": rel}), flush=True)


if __name__ == "__main__":
    main()
