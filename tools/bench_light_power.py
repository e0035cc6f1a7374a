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

Method: tools/bench_mis.py's. Every leg runs in a fresh child process, --rounds times, the legs alternating within a round so that drift
hits them alike. A child warms up (graph capture, first touch), then times --frames frames one by one, each ending in a device
synchronise. A leg's figure is the median of all its frames; its spread is the range of its per-round medians. The connect and emission
launches' own times come from wfpt_nee_timing_ms and wfpt_emission_timing_ms over one timed frame (hipEvent pairs around every launch, so
it is slower than the frame it describes). The lamps legs also report the sum of wfpt_read_variance over the frame (WFPT_FLAG_DENOISE is
set on them): the payoff test's figure at this tool's size. Prints one JSON line per leg and one summary line."""
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
    pt.render(a.spp)  # warm-up: graph capture, first touch of every buffer
    pt.render(a.spp)
    pt.synchronize()
    ms = []
    for _ in range(a.frames):
        t0 = time.perf_counter()
        pt.render(a.spp)
        pt.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--scenes", nargs="+", default=["shirley", "lamps"])
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its libwfpt.so built")
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        return leg(a)
    legs = [(f"{scene}:{kind}", ROOT) for scene in ("shirley", "lamps") if scene in a.scenes for kind in ("nee", "nee+power", "mis", "mis+power")]
    if a.parent_tree:  # (the parent has no flag to set: the unflagged legs alone have a twin there)
        legs = [x for name, tree in legs
                for x in ([(name, tree), (name + "@parent", os.path.abspath(a.parent_tree))] if "+power" not in name else [(name, tree)])]
    results = {name: {"rounds": [], "last": None} for name, _ in legs}
    for _ in range(a.rounds):
        for name, tree in legs:
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", name.split("@")[0], "--tree", tree, "--width", str(a.width), "--height",
                   str(a.height), "--spp", str(a.spp), "--bounces", str(a.bounces), "--frames", str(a.frames)]
            env = dict(os.environ)
            env.pop("WFPT_LIB", None)  # each tree loads its own library
            res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, env=env, timeout=600)  # a failed or hung leg ends the run
            if res.returncode != 0:
                sys.exit(f"bench_light_power: leg {name} failed with status {res.returncode}")
            r = json.loads(res.stdout.strip().splitlines()[-1])
            results[name]["rounds"].append(r["frame_ms"])
            results[name]["last"] = r
            print(f"{name}: {statistics.median(r['frame_ms']):.3f} ms", file=sys.stderr, flush=True)  # progress; the figures follow
    summary = {}
    for name, _ in legs:
        rounds = results[name]["rounds"]
        med = statistics.median(x for r in rounds for x in r)
        per_round = [statistics.median(r) for r in rounds]
        line = {"leg": name, "loop": results[name]["last"]["loop"], "size": [a.width, a.height], "spp": a.spp, "bounces": a.bounces,
                "frames": a.frames, "rounds": a.rounds, "frame_ms_median": round(med, 3),
                "round_medians_ms": [round(x, 3) for x in per_round], "spread_ms": round(max(per_round) - min(per_round), 3)}
        for k in ("lights", "variance_sum", "connect_ms_timed", "connect_launches_timed", "emission_ms_timed", "stages_ms_timed"):
            if k in results[name]["last"]:
                line[k] = round(results[name]["last"][k], 3) if isinstance(results[name]["last"][k], float) else results[name]["last"][k]
        summary[name] = line
        print(json.dumps(line), flush=True)
    rel = {}
    twins = [(name, name + "@parent") for name, _ in legs if not name.endswith("@parent")]
    for name, base in [(f"{scene}:{kind}+power", f"{scene}:{kind}") for scene in ("shirley", "lamps") for kind in ("nee", "mis")] + twins:
        if name in summary and base in summary:
            rel[f"{name} over {base}"] = round(summary[name]["frame_ms_median"] / summary[base]["frame_ms_median"] - 1.0, 4)
            if "connect_ms_timed" in summary[name] and "connect_ms_timed" in summary[base] and summary[base]["connect_ms_timed"]:
                rel[f"{name} over {base}, timed connect"] = round(summary[name]["connect_ms_timed"] / summary[base]["connect_ms_timed"] - 1.0, 4)
            if "variance_sum" in summary[name] and "variance_sum" in summary[base]:
                rel[f"{name} over {base}, variance"] = round(summary[name]["variance_sum"] / summary[base]["variance_sum"], 4)
    print(json.dumps({"summary": rel}), flush=True)


if __name__ == "__main__":
    main()
