#!/usr/bin/env python3
"""tools/bench_microfacet.py: what GGX microfacet metals cost per frame (WFPT_FLAG_MICROFACET).

Legs, --spp samples per frame at --width x --height, the 1 M-triangle soup and the mesh camera of BASELINE config 5 (the soup's materials
by thirds: Lambertian, Metal, Dielectric):
  parent   the soup on the PARENT commit's library (--parent-root: a checkout of it with its library built); no flag
  off      the same on this tree, no flag                                   (must lie within the spread of `parent`'s round medians)
  empty    the soup, the flag set, no roughness                             (the same launches as `off`)
  rough    the soup with its metal third at alpha 0.3                       (the pass: a third of the hits sample, two thirds copy)
  both     the same with a table of corner normals as well                  (microfacet_kernel<true> in shading_normal_kernel's place);
           `normals` is that table without roughness, the leg `both` is read against

Method: tools/ab_bench.py's. The pass's own time comes from wfpt_microfacet_timing_ms (wfpt_shading_normal_timing_ms
for `normals`) over one timed frame (hipEvent pairs around every launch, so it is slower than the frame it describes), beside the sum of
that frame's stage times."""
import json
import sys

import ab_bench as ab

EXTRA_KEYS, DIGITS = ("triangles", "pass_ms_timed", "pass_launches_timed", "stages_ms_timed"), 6
METAL, ALPHA = 1, 0.3


def leg(a):
    sys.path.insert(0, a.tree)
    import numpy as np
    import wavefront_path_tracer_amd as W
    flags = 0
    if a.leg in ("empty", "rough", "both"):
        flags |= W.FLAG_MICROFACET
    if a.leg in ("both", "normals"):
        flags |= W.FLAG_SHADING_NORMALS
    scene = W.Scene.random_mesh(a.triangles, 1)
    n9 = None
    if a.leg in ("both", "normals"):
        t = scene.triangles
        face = np.cross(t["e1"].astype(np.float64), t["e2"].astype(np.float64))
        face /= np.linalg.norm(face, axis=1)[:, None]
        n9 = (face[:, None, :] + 0.3 * np.random.default_rng(2).normal(size=(len(t), 3, 3))).reshape(-1, 9).astype(np.float32)
        scene.triangles["_pad"] = np.arange(len(scene.triangles), dtype=np.uint32)
    cc = W.CameraController(W.Camera((0.0, 0.0, 30.0), (0.0, 0.0, 0.0)), 40.0, 0.0, 10.0, 0.1, 100.0)
    pt = W.PathTracer(scene, W.RenderParameters(cc, (a.width, a.height)), max_wavefronts=a.bounces, rng_mode=W.RNG_DISPATCH, flags=flags,
                      batch=a.batch, device_bvh=True)
    if n9 is not None:
        pt.set_triangle_normals(n9)
    if a.leg in ("rough", "both"):
        assert int(scene.materials["material_type"][METAL]) == 1
        pt.set_roughness(METAL, ALPHA)
    ms = ab.timed_frames(pt, a.spp, a.frames)
    stage_ms, _ = pt.render_timed(a.spp)
    pass_ms, launches = 0.0, 0
    if a.leg in ("empty", "rough", "both"):
        pass_ms, launches = pt.microfacet_timing_ms()
    elif a.leg == "normals":
        pass_ms, launches = pt.shading_normal_timing()
    print(json.dumps({"leg": a.leg, "loop": pt.loop_kind, "triangles": len(scene.triangles), "frame_ms": ms, "pass_ms_timed": pass_ms,
                      "pass_launches_timed": launches, "stages_ms_timed": float(np.sum(stage_ms))}), flush=True)
    pt.close()


def options():
    ap = ab.parser(frames=12)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with its library built (the `parent` leg)")
    ap.add_argument("--legs", nargs="+", default=["parent", "off", "empty", "rough", "normals", "both"])
    return ap


def legs(a):
    return [ab.entry(name, "off", a.parent_root) if name == "parent" else ab.entry(name) for name in a.legs if name != "parent" or a.parent_root]


def main():
    a = options().parse_args()
    if a.leg:
        return leg(a)
    summary = ab.summarise(ab.run_legs(__file__, legs(a), a), a, EXTRA_KEYS, DIGITS)
    rel = ab.ratios(summary, (("off", "parent"), ("empty", "off"), ("rough", "off"), ("normals", "off"), ("both", "off"), ("both", "normals")), ", frame")
    if "off" in summary and "parent" in summary:
        p = summary["parent"]["round_medians_ms"]
        rel["off within the spread of parent's round medians"] = bool(min(p) <= summary["off"]["frame_ms_median"] <= max(p))
    for name in ("rough", "normals", "both"):
        if name in summary:
            p, s = summary[name]["pass_ms_timed"], summary[name]["stages_ms_timed"]  # (the pass is booked apart from the stages)
            rel[f"{name}: pass share of the timed frame"] = round(p / (p + s), 4)
    print(json.dumps({"summary": rel}), flush=True)


if __name__ == "__main__":
    main()
