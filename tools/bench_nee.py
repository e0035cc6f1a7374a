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

Method: every leg runs in a fresh child process (nothing is shared between legs but the machine), --rounds times, the legs alternating
within a round so that drift hits them alike. A child warms up (graph capture, first touch), then times --frames frames one by one, each
ending in a device synchronise. A leg's figure is the median of all its frames; its spread is the range of its per-round medians. The
connect launches' own time comes from wfpt_nee_timing_ms over one timed frame (hipEvent pairs around every launch, so it is slower than
the frame it describes). Prints one JSON line per leg and one summary line."""
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
    if kind == "nee":
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
    ap.add_argument("--triangles", type=int, default=1000000)
    ap.add_argument("--scenes", nargs="+", default=["shirley", "lamp", "mesh"])
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its libwfpt.so built")
    ap.add_argument("--closest-lib", default=None, help="this tree's library built with -DWFPT_NEE_EARLY_OUT=0")
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        return leg(a)
    legs = []
    if "shirley" in a.scenes:
        legs += [("shirley:plain", ROOT), ("shirley:lit", ROOT), ("shirley:nee", ROOT)]
        if a.parent_tree:
            legs.insert(1, ("shirley:plain@parent", os.path.abspath(a.parent_tree)))
        if a.closest_lib:
            legs.append(("shirley:nee@closest", ROOT))
    if "lamp" in a.scenes:
        legs += [("lamp:lit", ROOT), ("lamp:nee", ROOT)]
        if a.closest_lib:
            legs.append(("lamp:nee@closest", ROOT))
    if "mesh" in a.scenes:
        legs += [("mesh:lit", ROOT), ("mesh:nee", ROOT)]
    results = {name: {"rounds": [], "last": None} for name, _ in legs}
    for _ in range(a.rounds):
        for name, tree in legs:
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", name.split("@")[0], "--tree", tree, "--width", str(a.width), "--height",
                   str(a.height), "--spp", str(a.spp), "--bounces", str(a.bounces), "--frames", str(a.frames), "--triangles", str(a.triangles)]
            env = dict(os.environ)
            env.pop("WFPT_LIB", None)  # each tree loads its own library
            if name.endswith("@closest"):
                env["WFPT_LIB"] = os.path.abspath(a.closest_lib)
            res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, env=env, timeout=600)  # a failed or hung leg ends the run
            if res.returncode != 0:
                sys.exit(f"bench_nee: leg {name} failed with status {res.returncode}")
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
        for k in ("lights", "connect_ms_timed", "connect_launches_timed", "emission_ms_timed", "stages_ms_timed"):
            if k in results[name]["last"]:
                line[k] = round(results[name]["last"][k], 3) if isinstance(results[name]["last"][k], float) else results[name]["last"][k]
        summary[name] = line
        print(json.dumps(line), flush=True)
    rel = {}
    for name, base in (("shirley:lit", "shirley:plain"), ("shirley:nee", "shirley:lit"), ("lamp:nee", "lamp:lit"), ("mesh:nee", "mesh:lit"),
                       ("shirley:plain", "shirley:plain@parent"), ("shirley:nee", "shirley:nee@closest"), ("lamp:nee", "lamp:nee@closest")):
        if name in summary and base in summary:
            rel[f"{name} over {base}"] = round(summary[name]["frame_ms_median"] / summary[base]["frame_ms_median"] - 1.0, 4)
    print(json.dumps({"summary": rel}), flush=True)


if __name__ == "__main__":
    main()
