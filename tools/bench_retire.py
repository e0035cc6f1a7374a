#!/usr/bin/env python3
"""tools/bench_retire.py: what path termination brings per frame (WFPT_FLAG_RETIRE).

Legs, --spp samples per frame, named scene:kind:setting. Kinds: `plain` no feature flag, `lit` WFPT_FLAG_EMISSION, `nee` with WFPT_FLAG_NEE.
Settings: `off` without WFPT_FLAG_RETIRE, `dead` with the flag and roulette off (dead paths alone are retired: the same image), `rr`
with the default parameters (roulette from wavefront 3 on, q_min 0.05).
  shirley  plain:off | lit and nee: off, dead, rr   (the three big spheres emit)              at --width x --height, --bounces wavefronts
  room     lit: off, dead, rr                       (a closed sphere of fuzzy metal lit from inside by an emitting sphere: no ray misses;
                                                     miss_floor = 0 and --room-bounces wavefronts, the reference's 50)
  mesh     lit: off, dead, rr                       (material 1 of the soup's three emits)      the --triangles soup
and, with --parent-tree DIR (a checkout of the parent commit with its library built), the plain Shirley frame of that tree: the kernels a
context without the flag launches are the parent's, so the two are expected to be equal within the spread reported here.

Method: every leg runs in a fresh child process (nothing is shared between legs but the machine), --rounds times, the legs alternating
within a round so that drift hits them alike. A child warms up (graph capture, first touch), then times --frames frames one by one, each
ending in a device synchronise. A leg's figure is the median of all its frames; its spread is the range of its per-round medians. With
--equal-time MS the lit and nee legs of shirley and room then render on a second context with WFPT_FLAG_DENOISE (the luminance moments)
for MS milliseconds and report the samples that fitted and the image mean of wfpt_read_variance, the variance of the pixels' mean
luminance: the variance at equal time. Prints one JSON line per leg and one summary line."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make(W, np, a, scene, kind, setting, extra_flags=0):
    flags = extra_flags | (0 if kind == "plain" else W.FLAG_EMISSION | (W.FLAG_NEE if kind == "nee" else 0))
    if setting != "off":
        flags |= W.FLAG_RETIRE
    if scene == "room":
        sp, mt = np.zeros(3, W.SPHERE), np.zeros(3, W.MATERIAL)
        mt["albedo"][:] = (0.5, 0.5, 0.5, 1.0)
        mt["albedo"][0, :3] = (0.5, 0.75, 0.25)
        mt["albedo"][2, :3] = (0.75, 0.5, 0.5)
        mt["material_type"] = (1, 0, 0)
        mt["fuzz"][0] = 0.25
        sp["center"][:, 3] = 1.0
        sp["center"][:, :3] = [(0.0, 0.0, 0.0), (1.5, 1.0, -2.0), (-1.0, -0.5, -2.5)]
        sp["radius"] = (5.0, 1.0, 0.5)
        sp["material_idx"] = (0, 1, 2)
        sp["material_type"] = mt["material_type"][sp["material_idx"]]  # (extend hands shade the sphere's own copy of the type)
        cc = W.CameraController(W.Camera((0.5, 0.25, 1.0), (0.5, 0.0, -1.0)), 70.0, 0.0, 10.0, 0.1, 100.0)
        pt = W.PathTracer(W.Scene(sp, mt), W.RenderParameters(cc, (a.width, a.height)), max_wavefronts=a.room_bounces, miss_floor=0,
                          rng_mode=W.RNG_DISPATCH, flags=flags, batch=64)
        pt.set_emission(1, (4.0, 2.0, 8.0))
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
    if setting == "dead":
        pt.set_termination(W.NO_ROULETTE, 0.05)
    return pt


def leg(a):
    sys.path.insert(0, a.tree)
    import numpy as np
    import wavefront_path_tracer_amd as W
    scene, kind, setting = a.leg.split(":")
    pt = make(W, np, a, scene, kind, setting)
    pt.render(a.spp)  # warm-up: graph capture, first touch of every buffer
    pt.render(a.spp)
    pt.synchronize()
    ms = []
    for _ in range(a.frames):
        t0 = time.perf_counter()
        pt.render(a.spp)
        pt.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    totals = [int(x) for x in pt.totals()]
    frames = a.frames + 2
    out = {"leg": a.leg, "loop": pt.loop_kind, "frame_ms": ms, "rays_per_frame": totals[0] / frames, "hits_per_frame": totals[1] / frames,
           "wavefronts_last_sample": int(len(pt.bounce_table()))}
    pt.close()
    if a.equal_time > 0 and kind != "plain" and scene != "mesh":
        pt = make(W, np, a, scene, kind, setting, W.FLAG_DENOISE)
        pt.render(a.spp)
        pt.synchronize()
        pt.reset_progress()
        n, t0 = 0, time.perf_counter()
        while (time.perf_counter() - t0) * 1e3 < a.equal_time:
            pt.render(a.spp)
            pt.synchronize()
            n += a.spp
        out.update(equal_time_ms=a.equal_time, equal_time_samples=n, equal_time_variance=float(np.mean(pt.variance(), dtype=np.float64)))
        pt.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--room-bounces", type=int, default=50)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--triangles", type=int, default=1000000)
    ap.add_argument("--equal-time", type=float, default=0.0, help="milliseconds of rendering for the variance at equal time (0: skip)")
    ap.add_argument("--scenes", nargs="+", default=["shirley", "room", "mesh"])
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its libwfpt.so built")
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        return leg(a)
    legs = []
    if "shirley" in a.scenes:
        legs += [("shirley:plain:off", ROOT)]
        if a.parent_tree:
            legs.append(("shirley:plain:off@parent", os.path.abspath(a.parent_tree)))
        legs += [(f"shirley:{kind}:{setting}", ROOT) for kind in ("lit", "nee") for setting in ("off", "dead", "rr")]
    if "room" in a.scenes:
        legs += [(f"room:lit:{setting}", ROOT) for setting in ("off", "dead", "rr")]
    if "mesh" in a.scenes:
        legs += [(f"mesh:lit:{setting}", ROOT) for setting in ("off", "dead", "rr")]
    results = {name: {"rounds": [], "last": None} for name, _ in legs}
    for _ in range(a.rounds):
        for name, tree in legs:
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", name.split("@")[0], "--tree", tree, "--width", str(a.width), "--height",
                   str(a.height), "--spp", str(a.spp), "--bounces", str(a.bounces), "--room-bounces", str(a.room_bounces), "--frames",
                   str(a.frames), "--triangles", str(a.triangles), "--equal-time", str(0.0 if "@" in name else a.equal_time)]
            env = dict(os.environ)
            env.pop("WFPT_LIB", None)  # each tree loads its own library
            res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, env=env, timeout=600)  # a failed or hung leg ends the run
            if res.returncode != 0:
                sys.exit(f"bench_retire: leg {name} failed with status {res.returncode}")
            r = json.loads(res.stdout.strip().splitlines()[-1])
            results[name]["rounds"].append(r["frame_ms"])
            results[name]["last"] = r
            print(f"{name}: {statistics.median(r['frame_ms']):.3f} ms", file=sys.stderr, flush=True)  # progress; the figures follow
    summary = {}
    for name, _ in legs:
        rounds = results[name]["rounds"]
        med = statistics.median(x for r in rounds for x in r)
        per_round = [statistics.median(r) for r in rounds]
        last = results[name]["last"]
        line = {"leg": name, "loop": last["loop"], "size": [a.width, a.height], "spp": a.spp,
                "bounces": a.room_bounces if name.startswith("room") else a.bounces, "frames": a.frames, "rounds": a.rounds,
                "frame_ms_median": round(med, 3), "round_medians_ms": [round(x, 3) for x in per_round],
                "spread_ms": round(max(per_round) - min(per_round), 3)}
        for k in ("rays_per_frame", "hits_per_frame", "wavefronts_last_sample", "equal_time_ms", "equal_time_samples", "equal_time_variance"):
            if k in last:
                line[k] = last[k]
        summary[name] = line
        print(json.dumps(line), flush=True)
    rel = {}
    for name in summary:
        scene, kind, setting = name.split("@")[0].split(":")
        base = f"{scene}:{kind}:off"
        if "@" in name:
            rel[f"{base} over {name}"] = round(summary[base]["frame_ms_median"] / summary[name]["frame_ms_median"] - 1.0, 4)
        elif setting != "off":
            rel[f"{name} over {base}"] = round(summary[name]["frame_ms_median"] / summary[base]["frame_ms_median"] - 1.0, 4)
            if "equal_time_variance" in summary[name] and summary[base].get("equal_time_variance"):
                rel[f"{name} over {base}, variance at equal time"] = round(summary[name]["equal_time_variance"] / summary[base]["equal_time_variance"] - 1.0, 4)
    print(json.dumps({"summary": rel}), flush=True)


if __name__ == "__main__":
    main()
