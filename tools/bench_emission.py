#!/usr/bin/env python3
"""tools/bench_emission.py: what emissive materials cost per frame (WFPT_FLAG_EMISSION).

Legs, each against the context without the flag of the same tree, --spp samples per frame:
  shirley  plain | flag (the flag, no emitter) | lit (the three big spheres emit)       at --width x --height
  mesh     plain | lit (material 1 of the soup's three emits)                           the --triangles soup
and, with --parent-tree DIR (a checkout of the parent commit with its library built), the plain Shirley frame of that tree: the kernels a
context without the flag launches are the parent's, so the two are expected to be equal within the spread reported here.

Method: tools/ab_bench.py's. The emission launches' own time comes from wfpt_emission_timing_ms over one timed
frame (hipEvent pairs around every launch, so it is slower than the frame it describes)."""
import json
import sys

import ab_bench as ab

EXTRA_KEYS, DIGITS = ("emission_ms_timed", "emission_launches_timed", "stages_ms_timed"), 3


def leg(a):
    sys.path.insert(0, a.tree)
    import numpy as np
    import wavefront_path_tracer_amd as W
    scene, kind = a.leg.split(":")
    flags = 0 if kind == "plain" else W.FLAG_EMISSION
    if scene == "shirley":
        pt = W.shirley_path_tracer(a.width, a.height, max_wavefronts=a.bounces, rng_mode=W.RNG_DISPATCH, flags=flags, batch=64)
        if kind == "lit":
            sp = pt.scene.spheres
            for m, c in zip(sp["material_idx"][sp["radius"] == 1.0], ((4.0, 3.0, 2.0), (0.25, 0.5, 1.5), (1.0, 1.0, 1.0))):
                pt.set_emission(int(m), c)
    else:
        pt = W.mesh_path_tracer(a.width, a.height, a.triangles, max_wavefronts=a.bounces, rng_mode=W.RNG_DISPATCH, flags=flags, batch=64)
        if kind == "lit":
            pt.set_emission(1, (2.0, 1.0, 0.5))
    out = {"leg": a.leg, "loop": pt.loop_kind, "frame_ms": ab.timed_frames(pt, a.spp, a.frames)}
    if kind != "plain":
        stage_ms, _ = pt.render_timed(a.spp)
        em_ms, launches = pt.emission_timing()
        out.update(emission_ms_timed=em_ms, emission_launches_timed=launches, stages_ms_timed=float(np.sum(stage_ms)))
    print(json.dumps(out), flush=True)
    pt.close()


def options():
    ap = ab.parser()
    ap.add_argument("--scenes", nargs="+", default=["shirley", "mesh"])
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its libwfpt.so built")
    return ap


def legs(a):
    out = []
    if "shirley" in a.scenes:
        out += [ab.entry("shirley:plain"), ab.entry("shirley:flag"), ab.entry("shirley:lit")]
        if a.parent_tree:
            out.insert(1, ab.entry("shirley:plain@parent", tree=a.parent_tree))
    if "mesh" in a.scenes:
        out += [ab.entry("mesh:plain"), ab.entry("mesh:lit")]
    return out


def main():
    a = options().parse_args()
    if a.leg:
        return leg(a)
    summary = ab.summarise(ab.run_legs(__file__, legs(a), a), a, EXTRA_KEYS, DIGITS)
    rel = ab.ratios(summary, (("shirley:flag", "shirley:plain"), ("shirley:lit", "shirley:plain"), ("mesh:lit", "mesh:plain"),
                              ("shirley:plain", "shirley:plain@parent")))
    print(json.dumps({"summary": rel}), flush=True)


if __name__ == "__main__":
    main()
