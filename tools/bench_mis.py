#!/usr/bin/env python3
"""tools/bench_mis.py: what multiple importance sampling costs per frame (WFPT_FLAG_MIS).

Legs, --spp samples per frame: `plain` no flag, `lit` WFPT_FLAG_EMISSION, `nee` EMISSION|NEE, `mis` EMISSION|NEE|MIS:
  shirley  plain | lit | nee | mis   (the three big spheres emit)                          at --width x --height
  lamp     lit | nee | mis           (section 9h's small, far emitting sphere over a large Lambertian one, black map, miss_floor = 0)
  near     lit | nee | mis           (the near-lamp scene of the tests: radius 1, a gap of 0.05 to the radius-1000 ground)
and, with --parent-tree DIR (a checkout of the parent commit with its library built), every leg once more in that tree, named
`<leg>@parent` and run right after its twin: the kernels a context without the flag launches are the parent's, so the plain pair is
expected to be equal within the spread reported here, and the other pairs say what a change to the feature's own kernels costs.

Method: tools/ab_bench.py's. The connect and emission launches' own times come from wfpt_nee_timing_ms and
wfpt_emission_timing_ms over one timed frame (hipEvent pairs around every launch, so it is slower than the frame it describes). The lamp
legs also report the sum of wfpt_read_variance over the frame (WFPT_FLAG_DENOISE is set on them), for the equal-time product variance x
frame time."""
import json
import sys

import ab_bench as ab

EXTRA_KEYS, DIGITS = ("lights", "variance_sum", "connect_ms_timed", "connect_launches_timed", "emission_ms_timed", "stages_ms_timed"), 3


def leg(a):
    sys.path.insert(0, a.tree)
    import numpy as np
    import wavefront_path_tracer_amd as W
    scene, kind = a.leg.split(":")
    flags = {"plain": 0, "lit": W.FLAG_EMISSION, "nee": W.FLAG_EMISSION | W.FLAG_NEE}.get(kind)
    if flags is None:
        flags = W.FLAG_EMISSION | W.FLAG_NEE | W.FLAG_MIS
    if scene in ("lamp", "near"):
        sp, mt = np.zeros(2, W.SPHERE), np.zeros(2, W.MATERIAL)
        mt["albedo"][:] = (0.5, 0.75, 0.25, 1.0)
        sp["center"][:, 3] = 1.0
        far = scene == "lamp"
        sp["center"][:, :3] = [(0.0, -100.0, 0.0), (0.0, 2.0, 0.0)] if far else [(0.0, -1000.0, 0.0), (0.0, 1.05, 0.0)]
        sp["radius"] = (100.0, 0.25) if far else (1000.0, 1.0)
        sp["material_idx"] = (0, 1)
        cc = W.CameraController(W.Camera((0.0, 6.0, 8.0) if far else (0.0, 5.0, 7.0), (0.0, 0.0, 0.0)), 40.0, 0.0, 10.0, 0.1, 100.0)
        pt = W.PathTracer(W.Scene(sp, mt), W.RenderParameters(cc, (a.width, a.height)), max_wavefronts=a.bounces, miss_floor=0,
                          rng_mode=W.RNG_DISPATCH, flags=flags | W.FLAG_ENVIRONMENT | W.FLAG_DENOISE, batch=64)
        pt.set_environment(np.zeros((1, 1, 3), "<f4"))
        pt.set_emission(1, (16.0, 8.0, 32.0) if far else (4.0, 2.0, 8.0))
    elif scene == "shirley":
        pt = W.shirley_path_tracer(a.width, a.height, max_wavefronts=a.bounces, rng_mode=W.RNG_DISPATCH, flags=flags, batch=64)
        if kind != "plain":
            sp = pt.scene.spheres
            for m, c in zip(sp["material_idx"][sp["radius"] == 1.0], ((4.0, 3.0, 2.0), (0.25, 0.5, 1.5), (1.0, 1.0, 1.0))):
                pt.set_emission(int(m), c)
    else:
        sys.exit(f"bench_mis: unknown scene {scene}")
    out = {"leg": a.leg, "loop": pt.loop_kind, "frame_ms": ab.timed_frames(pt, a.spp, a.frames)}
    if scene in ("lamp", "near"):  # the variance of the last frame's mean, summed over the frame (every leg restarts from the same state)
        pt.reset_progress()
        pt.render(a.spp)
        out.update(variance_sum=float(pt.variance().astype(np.float64).sum()))
    if kind in ("nee", "mis"):
        stage_ms, _ = pt.render_timed(a.spp)
        nee_ms, launches = pt.nee_timing()
        out.update(lights=pt.nee_light_count(), connect_ms_timed=nee_ms, connect_launches_timed=launches, emission_ms_timed=pt.emission_timing()[0],
                   stages_ms_timed=float(np.sum(stage_ms)))
    print(json.dumps(out), flush=True)
    pt.close()


def options():
    ap = ab.parser(triangles=None)
    ap.add_argument("--scenes", nargs="+", default=["shirley", "lamp", "near"])
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its libwfpt.so built")
    return ap


def legs(a):
    out = []
    if "shirley" in a.scenes:
        out += [ab.entry(f"shirley:{kind}") for kind in ("plain", "lit", "nee", "mis")]
    for scene in ("lamp", "near"):
        if scene in a.scenes:
            out += [ab.entry(f"{scene}:{kind}") for kind in ("lit", "nee", "mis")]
    return ab.with_twins(out, a.parent_tree)


def main():
    a = options().parse_args()
    if a.leg:
        return leg(a)
    summary = ab.summarise(ab.run_legs(__file__, legs(a), a), a, EXTRA_KEYS, DIGITS)
    rel = {}
    for name, base in [("shirley:lit", "shirley:plain"), ("shirley:nee", "shirley:lit"), ("shirley:mis", "shirley:nee"), ("lamp:mis", "lamp:nee"),
                       ("near:mis", "near:nee"), ("near:mis", "near:lit")] + ab.twin_pairs(summary):
        rel.update(ab.ratios(summary, [(name, base)]))
        if "variance_sum" in summary.get(name, {}) and "variance_sum" in summary.get(base, {}):  # equal time: variance x frame time
            rel[f"{name} over {base}, variance x time"] = round(
                summary[name]["variance_sum"] * summary[name]["frame_ms_median"] / (summary[base]["variance_sum"] * summary[base]["frame_ms_median"]), 4)
    print(json.dumps({"summary": rel}), flush=True)


if __name__ == "__main__":
    main()
