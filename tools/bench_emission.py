#!/usr/bin/env python3
"""tools/bench_emission.py: what emissive materials cost per frame (WFPT_FLAG_EMISSION).

Legs, each against the context without the flag of the same tree, --spp samples per frame:
  shirley  plain | flag (the flag, no emitter) | lit (the three big spheres emit)       at --width x --height
  mesh     plain | lit (material 1 of the soup's three emits)                           the --triangles soup
and, with --parent-tree DIR (a checkout of the parent commit with its library built), the plain Shirley frame of that tree: the kernels a
context without the flag launches are the parent's, so the two are expected to be equal within the spread reported here.

Method: every leg runs in a fresh child process (nothing is shared between legs but the machine), --rounds times, the legs alternating
within a round so that drift hits them alike. A child warms up (graph capture, first touch), then times --frames frames one by one, each
ending in a device synchronise. A leg's figure is the median of all its frames; its spread is the range of its per-round medians. The
emission launches' own time comes from wfpt_emission_timing_ms over one timed frame (hipEvent pairs around every launch, so it is
slower than the frame it describes). Prints one JSON line per leg and one summary line."""
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
    if kind != "plain":
        stage_ms, _ = pt.render_timed(a.spp)
        em_ms, launches = pt.emission_timing()
        out.update(emission_ms_timed=em_ms, emission_launches_timed=launches, stages_ms_timed=float(np.sum(stage_ms)))
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
    ap.add_argument("--triangles", type=int, default=1000000)
    ap.add_argument("--scenes", nargs="+", default=["shirley", "mesh"])
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its libwfpt.so built")
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        return leg(a)
    legs = []
    if "shirley" in a.scenes:
        legs += [("shirley:plain", ROOT), ("shirley:flag", ROOT), ("shirley:lit", ROOT)]
        if a.parent_tree:
            legs.insert(1, ("shirley:plain@parent", os.path.abspath(a.parent_tree)))
    if "mesh" in a.scenes:
        legs += [("mesh:plain", ROOT), ("mesh:lit", ROOT)]
    results = {name: {"rounds": [], "last": None} for name, _ in legs}
    for _ in range(a.rounds):
        for name, tree in legs:
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", name.split("@")[0], "--tree", tree, "--width", str(a.width), "--height",
                   str(a.height), "--spp", str(a.spp), "--bounces", str(a.bounces), "--frames", str(a.frames), "--triangles", str(a.triangles)]
            env = dict(os.environ)
            env.pop("WFPT_LIB", None)  # each tree loads its own library
            res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, env=env, timeout=600)  # a failed or hung leg ends the run
            if res.returncode != 0:
                sys.exit(f"bench_emission: leg {name} failed with status {res.returncode}")
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
        for k in ("emission_ms_timed", "emission_launches_timed", "stages_ms_timed"):
            if k in results[name]["last"]:
                line[k] = round(results[name]["last"][k], 3) if isinstance(results[name]["last"][k], float) else results[name]["last"][k]
        summary[name] = line
        print(json.dumps(line), flush=True)
    rel = {}
    for name, base in (("shirley:flag", "shirley:plain"), ("shirley:lit", "shirley:plain"), ("mesh:lit", "mesh:plain"),
                       ("shirley:plain", "shirley:plain@parent")):
        if name in summary and base in summary:
            rel[f"{name} over {base}"] = round(summary[name]["frame_ms_median"] / summary[base]["frame_ms_median"] - 1.0, 4)
    print(json.dumps({"summary": rel}), flush=True)


if __name__ == "__main__":
    main()
