#!/usr/bin/env python3
"""tools/bench_rough_dielectric.py: what GGX rough dielectrics cost per frame (WFPT_FLAG_ROUGH_DIELECTRIC).

Legs, --spp samples per frame at --width x --height, the 1 M-triangle soup and the mesh camera of BASELINE config 5 (the soup's materials
by thirds: Lambertian, Metal, Dielectric):
  parent   the soup on the PARENT commit's library (--parent-root: a checkout of it with its library built); no flag
  off      the same on this tree, no flag                                   (must lie within the spread of `parent`'s round medians)
  empty    the soup, WFPT_FLAG_MICROFACET | WFPT_FLAG_ROUGH_DIELECTRIC, no roughness          (the same launches as `off`)
  glass    the flags, the glass third at alpha 0.3         (rough_glass_kernel: a third of the hits sample, two thirds copy)
  both     the same with the metal third at alpha 0.3 as well               (two thirds of the hits sample)
  metal    WFPT_FLAG_MICROFACET alone, the metal third at alpha 0.3         (microfacet_kernel: what `glass` and `both` are read against)

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
METAL, GLASS, ALPHA = 1, 2, 0.3
FLAGGED = ("empty", "glass", "both")


def leg(a):
    sys.path.insert(0, a.tree)
    import numpy as np
    import wavefront_path_tracer_amd as W
    if a.leg == "device":  # (the stamp's device name: a child of its own, so that the parent never opens the GPU)
        import torch
        print(json.dumps({"device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else "none"}), flush=True)
        return
    flags = 0
    if a.leg in FLAGGED:
        flags |= W.FLAG_MICROFACET | W.FLAG_ROUGH_DIELECTRIC
    if a.leg == "metal":
        flags |= W.FLAG_MICROFACET
    scene = W.Scene.random_mesh(a.triangles, 1)
    cc = W.CameraController(W.Camera((0.0, 0.0, 30.0), (0.0, 0.0, 0.0)), 40.0, 0.0, 10.0, 0.1, 100.0)
    pt = W.PathTracer(scene, W.RenderParameters(cc, (a.width, a.height)), max_wavefronts=a.bounces, rng_mode=W.RNG_DISPATCH, flags=flags,
                      batch=a.batch, device_bvh=True)
    assert int(scene.materials["material_type"][METAL]) == 1 and int(scene.materials["material_type"][GLASS]) == 2
    if a.leg in ("glass", "both"):
        pt.set_roughness(GLASS, ALPHA)
    if a.leg in ("both", "metal"):
        pt.set_roughness(METAL, ALPHA)
    ms = ab.timed_frames(pt, a.spp, a.frames)
    stage_ms, _ = pt.render_timed(a.spp)
    pass_ms, launches = pt.microfacet_timing_ms() if a.leg in FLAGGED + ("metal",) else (0.0, 0)
    print(json.dumps({"leg": a.leg, "loop": pt.loop_kind, "triangles": len(scene.triangles), "frame_ms": ms, "pass_ms_timed": pass_ms,
                      "pass_launches_timed": launches, "stages_ms_timed": float(np.sum(stage_ms))}), flush=True)
    pt.close()


def options():
    ap = ab.parser(frames=12)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with its library built (the `parent` leg)")
    ap.add_argument("--legs", nargs="+", default=["parent", "off", "empty", "glass", "both", "metal"])
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
    rel = ab.ratios(summary, (("off", "parent"), ("empty", "off"), ("glass", "off"), ("both", "off"), ("metal", "off"), ("glass", "metal"), ("both", "metal")), ", frame")
    for name in ("off", "empty"):
        if name in summary and "parent" in summary:
            p = summary["parent"]["round_medians_ms"]
            rel[f"{name} within the spread of parent's round medians"] = bool(min(p) <= summary[name]["frame_ms_median"] <= max(p))
    for name in ("glass", "both", "metal"):
        if name in summary:
            p, s = summary[name]["pass_ms_timed"], summary[name]["stages_ms_timed"]  # (the pass is booked apart from the stages)
            rel[f"{name}: pass share of the timed frame"] = round(p / (p + s), 4)
    print(json.dumps({"summary": rel}), flush=True)


if __name__ == "__main__":
    main()
