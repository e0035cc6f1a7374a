#!/usr/bin/env python3
"""tools/bench_light_power.py: what selecting the connect pass's light by power costs and brings (WFPT_FLAG_LIGHT_POWER).

Legs, --spp samples per frame: `nee` EMISSION|NEE, `mis` EMISSION|NEE|MIS, and each with `+power`, WFPT_FLAG_LIGHT_POWER:
  shirley  nee | nee+power | mis | mis+power   (the three big spheres emit, three lights of unequal power)   at --width x --height
  lamps    nee | nee+power | mis | mis+power   (the payoff scene of tests/test_gpu_light_power.py: one lamp of radius 0.5 at (16, 16, 16)
                                                 among 63 spheres of radius 0.01 at (0.1, 0.1, 0.1) over a large Lambertian ground, black
                                                 map, miss_floor = 0, WFPT_RNG_PIXEL)
and, with --parent-tree DIR (a checkout of the parent commit with its library built), every unflagged leg once more in that tree, named
`<leg>@parent` and run right after its twin: the kernels a context without the flag launches are the parent's, so those pairs are
expected to be equal within the spread reported here.

Method: tools/ab_bench.py's. The connect and emission launches' own times come from wfpt_nee_timing_ms and
wfpt_emission_timing_ms over one timed frame (hipEvent pairs around every launch, so it is slower than the frame it describes). The lamps
legs also report the sum of wfpt_read_variance over the frame (WFPT_FLAG_DENOISE is set on them): the payoff test's figure at this
tool's size."""
import json
import sys

import ab_bench as ab

EXTRA_KEYS, DIGITS = ("lights", "variance_sum", "connect_ms_timed", "connect_launches_timed", "emission_ms_timed", "stages_ms_timed"), 3


def leg(a):
    sys.path.insert(0, a.tree)
    import numpy as np
    import wavefront_path_tracer_amd as W
    scene, kind = a.leg.split(":")
    flags = W.FLAG_EMISSION | W.FLAG_NEE | (W.FLAG_MIS if kind.startswith("mis") else 0)
    if kind.endswith("+power"):
        flags |= W.FLAG_LIGHT_POWER
    if scene == "lamps":
        n_dim = 63
        rng = np.random.default_rng(7)  # tests/light_power_ref.py's indicator_inputs
        sp, mt = np.zeros(2 + n_dim, W.SPHERE), np.zeros(3, W.MATERIAL)
        mt["albedo"][:] = (0.5, 0.5, 0.5, 1.0)
        mt["albedo"][0, :3] = (0.5, 0.75, 0.25)
        sp["center"][:, 3] = 1.0
        sp["center"][0, :3], sp["radius"][0] = (0.0, -100.0, 0.0), 100.0
        sp["center"][1, :3], sp["radius"][1] = (0.0, 2.0, 0.0), 0.5
        sp["material_idx"][:2] = (0, 1)
        sp["center"][2:, 0] = rng.uniform(-4.0, 4.0, n_dim)
        sp["center"][2:, 1] = rng.uniform(0.5, 3.0, n_dim)
        sp["center"][2:, 2] = rng.uniform(-4.0, 4.0, n_dim)
        sp["radius"][2:] = 0.01
        sp["material_idx"][2:] = 2
        cc = W.CameraController(W.Camera((0.0, 6.0, 8.0), (0.0, 0.0, 0.0)), 40.0, 0.0, 10.0, 0.1, 100.0)
        pt = W.PathTracer(W.Scene(sp, mt), W.RenderParameters(cc, (a.width, a.height)), max_wavefronts=a.bounces, miss_floor=0,
                          rng_mode=W.RNG_PIXEL, flags=flags | W.FLAG_ENVIRONMENT | W.FLAG_DENOISE, batch=64)
        pt.set_environment(np.zeros((1, 1, 3), "<f4"))
        pt.set_emission(1, (16.0, 16.0, 16.0))
        pt.set_emission(2, (0.1, 0.1, 0.1))
    elif scene == "shirley":
        pt = W.shirley_path_tracer(a.width, a.height, max_wavefronts=a.bounces, rng_mode=W.RNG_DISPATCH, flags=flags, batch=64)
        sp = pt.scene.spheres
        for m, c in zip(sp["material_idx"][sp["radius"] == 1.0], ((4.0, 3.0, 2.0), (0.25, 0.5, 1.5), (1.0, 1.0, 1.0))):
            pt.set_emission(int(m), c)
    else:
        sys.exit(f"bench_light_power: unknown scene {scene}")
    ms = ab.timed_frames(pt, a.spp, a.frames)
    out = {"leg": a.leg, "loop": pt.loop_kind, "frame_ms": ms}
    if scene == "lamps":  # the variance of the last frame's mean, summed over the frame (every leg restarts from the same state)
        pt.reset_progress()
        pt.render(a.spp)
        out.update(variance_sum=float(pt.variance().astype(np.float64).sum()))
    stage_ms, _ = pt.render_timed(a.spp)
    nee_ms, launches = pt.nee_timing()
    out.update(lights=pt.nee_light_count(), connect_ms_timed=nee_ms, connect_launches_timed=launches, emission_ms_timed=pt.emission_timing()[0],
               stages_ms_timed=float(np.sum(stage_ms)))
    print(json.dumps(out), flush=True)
    pt.close()


def options():
    ap = ab.parser(triangles=None)
    ap.add_argument("--scenes", nargs="+", default=["shirley", "lamps"])
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its libwfpt.so built")
    return ap


def legs(a):  # (the parent has no flag to set: the unflagged legs alone have a twin there)
    out = [ab.entry(f"{scene}:{kind}") for scene in ("shirley", "lamps") if scene in a.scenes for kind in ("nee", "nee+power", "mis", "mis+power")]
    return ab.with_twins(out, a.parent_tree, lambda name: "+power" not in name)


def main():
    a = options().parse_args()
    if a.leg:
        return leg(a)
    summary = ab.summarise(ab.run_legs(__file__, legs(a), a), a, EXTRA_KEYS, DIGITS)
    rel = {}
    for name, base in [(f"{scene}:{kind}+power", f"{scene}:{kind}") for scene in ("shirley", "lamps") for kind in ("nee", "mis")] + ab.twin_pairs(summary):
        if name in summary and base in summary:
            rel.update(ab.ratios(summary, [(name, base)]))
            if "connect_ms_timed" in summary[name] and summary[base].get("connect_ms_timed"):
                rel.update(ab.ratios(summary, [(name, base)], ", timed connect", "connect_ms_timed"))
            if "variance_sum" in summary[name] and "variance_sum" in summary[base]:
                rel[f"{name} over {base}, variance"] = round(summary[name]["variance_sum"] / summary[base]["variance_sum"], 4)
    print(json.dumps({"summary": rel}), flush=True)


if __name__ == "__main__":
    main()
