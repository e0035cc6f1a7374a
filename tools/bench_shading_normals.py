#!/usr/bin/env python3
"""tools/bench_shading_normals.py: what per-vertex shading normals cost per frame (WFPT_FLAG_SHADING_NORMALS).

Legs, --spp samples per frame at --width x --height, the mesh camera of BASELINE config 5:
  parent   the 1 M-triangle soup on the PARENT commit's library (--parent-root: a checkout of it with its library built); no flag
  off      the same on this tree, no flag                                   (must lie within the spread of `parent`'s round medians)
  empty    the soup, the flag set, no table                                 (the same launches as `off`)
  soup     the soup with a table: every face normal tilted at its corners   (the pass and the table's traffic on an incoherent scene)
  sphere   a sphere tessellated to 1.3 M triangles (an icosphere, 8 subdivisions, radius 8; the soup's three materials by thirds) with
           its corner positions as normals; `sphere-flat` is the same mesh without a table

Method: tools/ab_bench.py's. The pass's own time comes from wfpt_shading_normal_timing_ms over one timed frame
(hipEvent pairs around every launch, so it is slower than the frame it describes), beside the sum of that frame's stage times."""
import json
import sys

import ab_bench as ab

EXTRA_KEYS, DIGITS = ("triangles", "pass_ms_timed", "pass_launches_timed", "stages_ms_timed"), 6


def icosphere(subdivisions, radius):
    import numpy as np
    g = (1.0 + 5.0 ** 0.5) / 2.0
    v = np.array([(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1),
                  (-g, 0, -1), (-g, 0, 1)], np.float64)
    v /= np.linalg.norm(v, axis=1)[:, None]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4),
         (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    tri = v[np.array(f)]
    for _ in range(subdivisions):
        a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
        ab, bc, ca = ((x + y) / np.linalg.norm(x + y, axis=1)[:, None] for x, y in ((a, b), (b, c), (c, a)))
        tri = np.concatenate([np.stack(q, 1) for q in ((a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca))])
    return tri * radius


def leg(a):
    sys.path.insert(0, a.tree)
    import numpy as np
    import wavefront_path_tracer_amd as W
    flagged = a.leg in ("empty", "soup", "sphere")
    flags = W.FLAG_SHADING_NORMALS if flagged else 0
    scene = W.Scene.random_mesh(a.triangles, 1)
    n9 = None
    if a.leg.startswith("sphere"):
        tri = icosphere(a.subdivisions, 8.0)
        t = np.zeros(len(tri), W.TRIANGLE)
        t["v0"], t["e1"], t["e2"] = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
        t["material_idx"] = (np.arange(len(t)) * 3) // len(t)
        t["material_type"] = scene.materials["material_type"][t["material_idx"]]
        scene = W.Scene(np.zeros(0, W.SPHERE), scene.materials, triangles=t)
        n9 = tri.reshape(-1, 9).astype(np.float32)
    elif a.leg == "soup":
        t = scene.triangles
        face = np.cross(t["e1"].astype(np.float64), t["e2"].astype(np.float64))
        face /= np.linalg.norm(face, axis=1)[:, None]
        n9 = (face[:, None, :] + 0.3 * np.random.default_rng(2).normal(size=(len(t), 3, 3))).reshape(-1, 9).astype(np.float32)
    if n9 is not None or flagged:
        scene.triangles["_pad"] = np.arange(len(scene.triangles), dtype=np.uint32)
    cc = W.CameraController(W.Camera((0.0, 0.0, 30.0), (0.0, 0.0, 0.0)), 40.0, 0.0, 10.0, 0.1, 100.0)
    pt = W.PathTracer(scene, W.RenderParameters(cc, (a.width, a.height)), max_wavefronts=a.bounces, rng_mode=W.RNG_DISPATCH, flags=flags,
                      batch=a.batch, device_bvh=True)
    if a.leg in ("soup", "sphere"):
        pt.set_triangle_normals(n9)
    ms = ab.timed_frames(pt, a.spp, a.frames)
    stage_ms, _ = pt.render_timed(a.spp)
    sn_ms, launches = pt.shading_normal_timing() if flagged else (0.0, 0)
    print(json.dumps({"leg": a.leg, "loop": pt.loop_kind, "triangles": len(scene.triangles), "frame_ms": ms, "pass_ms_timed": sn_ms,
                      "pass_launches_timed": launches, "stages_ms_timed": float(np.sum(stage_ms))}), flush=True)
    pt.close()


def options():
    ap = ab.parser(frames=12)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--subdivisions", type=int, default=8)
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with its library built (the `parent` leg)")
    ap.add_argument("--legs", nargs="+", default=["parent", "off", "empty", "soup", "sphere-flat", "sphere"])
    return ap


def legs(a):
    return [ab.entry(name, "off", a.parent_root) if name == "parent" else ab.entry(name) for name in a.legs if name != "parent" or a.parent_root]


def main():
    a = options().parse_args()
    if a.leg:
        return leg(a)
    summary = ab.summarise(ab.run_legs(__file__, legs(a), a), a, EXTRA_KEYS, DIGITS)
    rel = ab.ratios(summary, (("off", "parent"), ("empty", "off"), ("soup", "off"), ("sphere", "sphere-flat")), ", frame")
    for name in ("soup", "sphere"):
        if name in summary:
            p, s = summary[name]["pass_ms_timed"], summary[name]["stages_ms_timed"]  # (the pass is booked apart from the stages)
            rel[f"{name}: pass share of the timed frame"] = round(p / (p + s), 4)
    print(json.dumps({"summary": rel}), flush=True)


if __name__ == "__main__":
    main()
