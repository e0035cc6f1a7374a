#!/usr/bin/env python3
"""tools/bench_env_nee.py: what importance-sampling the environment map costs per frame, and what it buys (WFPT_FLAG_ENV_NEE, DESIGN.md
section 9i).

Legs, --spp samples per frame, all on Shirley's scene under a 2048 x 1024 map with a sun (a dim sky and a disc of about 1e-4 of the
sphere of directions, 50 000 times brighter):
  shirley:off      WFPT_FLAG_ENVIRONMENT | EMISSION | NEE, no emitter: the flag off
  shirley:env      WFPT_FLAG_ENVIRONMENT only
  shirley:env_nee  the three flags | WFPT_FLAG_ENV_NEE
and, with --parent-tree DIR (a checkout of the parent commit with its library built), every leg once more in that tree, named
`<leg>@parent` and run right after its twin: the kernels a context without the flag launches are the parent's, so the off pair is
expected to agree within the spread reported here, and the other pairs say what a change to the feature's own kernels costs.

Method (tools/bench_nee.py's): every leg runs in a fresh child process, --rounds times, the legs alternating within a round so that
drift hits them alike. A child warms up, then times --frames frames one by one, each ending in a device synchronise. A leg's figure is
the median of all its frames; its spread is the range of its per-round medians. The env and env_nee legs then render one frame on a
second context with WFPT_FLAG_DENOISE and report the sum of wfpt_read_variance over the frame. The summary gives the frame-time ratio,
the variance ratio at equal spp and, as section 9h does, the variance ratio at equal time = (variance ratio) * (frame-time ratio).
Prints one JSON line per leg and one summary line."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sun_map(np, w=2048, h=1024):
    """A dim blue-ish sky and a sun of angular radius 0.02 rad (1e-4 of the sphere) at 50 degrees elevation."""
    v = (np.arange(h, dtype=np.float64) + 0.5) / h
    u = (np.arange(w, dtype=np.float64) + 0.5) / w
    theta, phi = np.pi * v[:, None], 2 * np.pi * (u[None, :] - 0.5)
    d = np.stack([np.sin(theta) * np.sin(phi), np.cos(theta) * np.ones_like(phi), -np.sin(theta) * np.cos(phi)], -1)
    env = np.empty((h, w, 3), "<f4")
    env[...] = (0.08, 0.12, 0.2)
    el, az = np.radians(50.0), np.radians(60.0)
    sun = np.array([np.cos(el) * np.sin(az), np.sin(el), -np.cos(el) * np.cos(az)])
    env[(d @ sun) > np.cos(0.02)] = (6000.0, 5000.0, 4000.0)
    return env


def leg(a):
    sys.path.insert(0, a.tree)
    import numpy as np
    import wavefront_path_tracer_amd as W
    kind = a.leg.split(":")[1]
    flags = W.FLAG_ENVIRONMENT
    if kind != "env":
        flags |= W.FLAG_EMISSION | W.FLAG_NEE
    if kind == "env_nee":
        flags |= W.FLAG_ENV_NEE
    env = sun_map(np)

    def tracer(extra=0):
        pt = W.shirley_path_tracer(a.width, a.height, max_wavefronts=a.bounces, rng_mode=W.RNG_DISPATCH, flags=flags | extra, batch=64)
        pt.set_environment(env)
        return pt

    pt = tracer()
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
    if kind == "env_nee":
        stage_ms, _ = pt.render_timed(a.spp)
        nee_ms, launches = pt.nee_timing()
        out.update(connect_ms_timed=nee_ms, connect_launches_timed=launches, stages_ms_timed=float(np.sum(stage_ms)))
    pt.close()
    if kind in ("env", "env_nee"):
        pt = tracer(W.FLAG_DENOISE)
        pt.render(a.spp)
        out["variance_sum"] = float(pt.variance().astype(np.float64).sum())
        pt.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its libwfpt.so built")
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        return leg(a)
    legs = [("shirley:off", ROOT), ("shirley:env", ROOT), ("shirley:env_nee", ROOT)]
    if a.parent_tree:
        legs = [x for name, tree in legs for x in ((name, tree), (name + "@parent", os.path.abspath(a.parent_tree)))]
    results = {name: {"rounds": [], "last": None} for name, _ in legs}
    for _ in range(a.rounds):
        for name, tree in legs:
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", name.split("@")[0], "--tree", tree, "--width", str(a.width), "--height",
                   str(a.height), "--spp", str(a.spp), "--bounces", str(a.bounces), "--frames", str(a.frames)]
            env = dict(os.environ)
            env.pop("WFPT_LIB", None)  # each tree loads its own library
            res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, env=env, timeout=600)  # a failed or hung leg ends the run
            if res.returncode != 0:
                sys.exit(f"bench_env_nee: leg {name} failed with status {res.returncode}")
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
        for k in ("connect_ms_timed", "connect_launches_timed", "stages_ms_timed", "variance_sum"):
            if k in results[name]["last"]:
                line[k] = round(results[name]["last"][k], 6) if isinstance(results[name]["last"][k], float) else results[name]["last"][k]
        summary[name] = line
        print(json.dumps(line), flush=True)
    rel = {}
    twins = [(name, name + "@parent") for name, _ in legs if not name.endswith("@parent")]
    for name, base in twins + [("shirley:off", "shirley:env"), ("shirley:env_nee", "shirley:env")]:
        if name in summary and base in summary:
            rel[f"{name} over {base}"] = round(summary[name]["frame_ms_median"] / summary[base]["frame_ms_median"] - 1.0, 4)
    if "variance_sum" in summary.get("shirley:env_nee", {}) and "variance_sum" in summary.get("shirley:env", {}):
        t = summary["shirley:env_nee"]["frame_ms_median"] / summary["shirley:env"]["frame_ms_median"]
        v = summary["shirley:env_nee"]["variance_sum"] / summary["shirley:env"]["variance_sum"]
        rel.update(frame_time_ratio=round(t, 4), variance_ratio_equal_spp=float(f"{v:.4g}"), variance_ratio_equal_time=float(f"{v * t:.4g}"))
    print(json.dumps({"summary": rel}), flush=True)


if __name__ == "__main__":
    main()
