#!/usr/bin/env python3
"""tools/bench_nee.py: what next-event estimation costs per frame (WFPT_FLAG_NEE).

Legs, --spp samples per frame; `lit` is the emission-only context of section 9g, `nee` the same scene with WFPT_FLAG_NEE:
  shirley  plain | lit | nee      (the three big spheres emit)                          at --width x --height
  lamp     lit | nee              (a small emitting sphere over a large Lambertian one, a black environment map, miss_floor = 0)
  mesh     lit | nee              (material 1 of the soup's three emits)                 the --triangles soup
and, with --parent-tree DIR (a checkout of the parent commit with its library built), the plain Shirley frame of that tree: the kernels a
context without the flag launches are the parent's, so the two are expected to be equal within the spread reported here. With
--closest-lib PATH (this tree's library built with WFPT_EXTRA_FLAGS=-DWFPT_NEE_EARLY_OUT=0 WFPT_LIB_OUT=PATH) the flagged Shirley and lamp
legs also run on that library, in which every shadow ray takes the closest-hit walk: the early-out occlusion walk against the first version.

Method: tools/ab_bench.py's. The connect launches' own time comes from wfpt_nee_timing_ms over one timed frame
(hipEvent pairs around every launch, so it is slower than the frame it describes)."""
import json
import sys

import ab_bench as ab

EXTRA_KEYS, DIGITS = ("lights", "connect_ms_timed", "connect_launches_timed", "emission_ms_timed", "stages_ms_timed"), 3


def leg(a):
    sys.path.insert(0, a.tree)
    import numpy as np
    import wavefront_path_tracer_amd as W
    scene, kind = a.leg.split(":")
    flags = 0 if kind == "plain" else W.FLAG_EMISSION | (W.FLAG_NEE if kind == "nee" else 0)
    if scene == "lamp":
        sp, mt = np.zeros(2, W.SPHERE), np.zeros(2, W.MATERIAL)
        mt["albedo"][:] = (0.5, 0.75, 0.25, 1.0)
        sp["center"][:, 3] = 1.0
        sp["center"][:, :3] = [(0.0, -100.0, 0.0), (0.0, 2.0, 0.0)]
        sp["radius"] = (100.0, 0.25)
        sp["material_idx"] = (0, 1)
        cc = W.CameraController(W.Camera((0.0, 6.0, 8.0), (0.0, 0.0, 0.0)), 40.0, 0.0, 10.0, 0.1, 100.0)
        pt = W.PathTracer(W.Scene(sp, mt), W.RenderParameters(cc, (a.width, a.height)), max_wavefronts=a.bounces, miss_floor=0,
                          rng_mode=W.RNG_DISPATCH, flags=flags | W.FLAG_ENVIRONMENT, batch=64)
        pt.set_environment(np.zeros((1, 1, 3), "<f4"))
        pt.set_emission(1, (16.0, 8.0, 32.0))
    elif scene == "shirley":
        pt = W.shirley_path_tracer(a.width, a.height, max_wavefronts=a.bounces, rng_mode=W.RNG_DISPATCH, flags=flags, batch=64)
        if kind != "plain":
            sp = pt.scene.spheres
            for m, c in zip(sp["material_idx"][sp["radius"] == 1.0], ((4.0, 3.0, 2.0), (0.25, 0.5, 1.5), (1.0, 1.0, 1.0))):
                pt.set_emission(int(m), c)
    else:
        pt = W.mesh_path_tracer(a.width, a.height, a.triangles, max_wavefronts=a.bounces, rng_mode=W.RNG_DISPATCH, flags=flags, batch=64)
        if kind != "plain":
            pt.set_emission(1, (2.0, 1.0, 0.5))
    out = {"leg": a.leg, "loop": pt.loop_kind, "frame_ms": ab.timed_frames(pt, a.spp, a.frames)}
    if kind == "nee":
        stage_ms, _ = pt.render_timed(a.spp)
        nee_ms, launches = pt.nee_timing()
        out.update(lights=pt.nee_light_count(), connect_ms_timed=nee_ms, connect_launches_timed=launches, emission_ms_timed=pt.emission_timing()[0],
                   stages_ms_timed=float(np.sum(stage_ms)))
    print(json.dumps(out), flush=True)
    pt.close()


def options():
    ap = ab.parser()
    ap.add_argument("--scenes", nargs="+", default=["shirley", "lamp", "mesh"])
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its libwfpt.so built")
    ap.add_argument("--closest-lib", default=None, help="this tree's library built with -DWFPT_NEE_EARLY_OUT=0")
    return ap


def legs(a):
    out = []
    if "shirley" in a.scenes:
        out += [ab.entry("shirley:plain"), ab.entry("shirley:lit"), ab.entry("shirley:nee")]
        if a.parent_tree:
            out.insert(1, ab.entry("shirley:plain@parent", tree=a.parent_tree))
        if a.closest_lib:
            out.append(ab.entry("shirley:nee@closest", lib=a.closest_lib))
    if "lamp" in a.scenes:
        out += [ab.entry("lamp:lit"), ab.entry("lamp:nee")]
        if a.closest_lib:
            out.append(ab.entry("lamp:nee@closest", lib=a.closest_lib))
    if "mesh" in a.scenes:
        out += [ab.entry("mesh:lit"), ab.entry("mesh:nee")]
    return out


def main():
    a = options().parse_args()
    if a.leg:
        return leg(a)
    summary = ab.summarise(ab.run_legs(__file__, legs(a), a), a, EXTRA_KEYS, DIGITS)
    rel = ab.ratios(summary, (("shirley:lit", "shirley:plain"), ("shirley:nee", "shirley:lit"), ("lamp:nee", "lamp:lit"), ("mesh:nee", "mesh:lit"),
                              ("shirley:plain", "shirley:plain@parent"), ("shirley:nee", "shirley:nee@closest"), ("lamp:nee", "lamp:nee@closest")))
    print(json.dumps({"summary": rel}), flush=True)


if __name__ == "__main__":
    main()
