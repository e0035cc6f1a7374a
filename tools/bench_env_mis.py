#!/usr/bin/env python3
"""tools/bench_env_mis.py: what weighing the environment map against the scatter costs per frame, and what it buys (WFPT_FLAG_ENV_MIS,
DESIGN.md section 9l).

Legs, --spp samples per frame, all on Shirley's scene (no emitter: the effective share is 1) under a 2048 x 1024 map, `<map>:<kind>`:
  maps   sun   tools/bench_env_nee.py's: a dim sky and a disc of about 1e-4 of the sphere of directions, 50 000 times brighter
         soft  the same sky without the sun, brightening towards the zenith: no small bright region at all
  kinds  env      WFPT_FLAG_ENVIRONMENT only: the scatter alone
         env_nee  ENVIRONMENT | EMISSION | NEE | ENV_NEE: the shadow ray alone -- the flag off
         env_mis  the same | WFPT_FLAG_ENV_MIS: both, weighed
and, with --parent-tree DIR (a checkout of the parent commit with its library built), the env and env_nee legs once more in that tree,
named `<leg>@parent` and run right after their twins: the kernels a context without the flag launches are the parent's, so each pair is
expected to agree within the larger spread of the two.

Method (tools/bench_nee.py's): every leg runs in a fresh child process, --rounds times, the legs alternating within a round so that
drift hits them alike. A child warms up, then times --frames frames one by one, each ending in a device synchronise. A leg's figure is
the median of all its frames; its spread is the range of its per-round medians. Each leg then renders one frame on a second context with
WFPT_FLAG_DENOISE and reports the sum of wfpt_read_variance over the frame. The summary gives, per map, the frame-time ratios, the
variance ratios at equal spp and the variance ratios at equal time = (variance ratio) * (frame-time ratio) of env_mis against env_nee and
against env. Prints one JSON line per leg and one summary line."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def soft_map(np, w=2048, h=1024):
    """bench_env_nee's dim sky, three times brighter at the zenith than at the horizon and below, and no sun."""
    v = (np.arange(h, dtype=np.float64) + 0.5) / h
    up = np.clip(np.cos(np.pi * v), 0.0, 1.0)[:, None, None]
    env = np.empty((h, w, 3), "<f4")
    env[...] = np.asarray((0.08, 0.12, 0.2))[None, None] * (1.0 + 2.0 * up)
    return env


def leg(a):
    sys.path.insert(0, a.tree)
    import numpy as np
    import wavefront_path_tracer_amd as W
    from bench_env_nee import sun_map
    which, kind = a.leg.split(":")
    flags = W.FLAG_ENVIRONMENT
    if kind != "env":
        flags |= W.FLAG_EMISSION | W.FLAG_NEE | W.FLAG_ENV_NEE
    if kind == "env_mis":
        flags |= W.FLAG_ENV_MIS
    env = sun_map(np) if which == "sun" else soft_map(np)

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
    stage_ms, _ = pt.render_timed(a.spp)
    out.update(stages_ms_timed=float(np.sum(stage_ms)), miss_ms_timed=float(stage_ms[W.STAGES["miss_kernel"]]))
    if kind != "env":
        nee_ms, launches = pt.nee_timing()
        out.update(connect_ms_timed=nee_ms, connect_launches_timed=launches)
    pt.close()
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
    legs = [(f"{m}:{k}", ROOT) for m in ("sun", "soft") for k in ("env", "env_nee", "env_mis")]
    if a.parent_tree:  # the parent has no env_mis leg
        legs = [x for name, tree in legs
                for x in ([(name, tree)] + ([(name + "@parent", os.path.abspath(a.parent_tree))] if not name.endswith("env_mis") else []))]
    results = {name: {"rounds": [], "last": None} for name, _ in legs}
    for _ in range(a.rounds):
        for name, tree in legs:
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", name.split("@")[0], "--tree", tree, "--width", str(a.width), "--height",
                   str(a.height), "--spp", str(a.spp), "--bounces", str(a.bounces), "--frames", str(a.frames)]
            env = dict(os.environ)
            env.pop("WFPT_LIB", None)  # each tree loads its own library
            res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, env=env, timeout=600)  # a failed or hung leg ends the run
            if res.returncode != 0:
                sys.exit(f"bench_env_mis: leg {name} failed with status {res.returncode}")
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
        for k in ("connect_ms_timed", "connect_launches_timed", "miss_ms_timed", "stages_ms_timed", "variance_sum"):
            if k in results[name]["last"]:
                line[k] = round(results[name]["last"][k], 6) if isinstance(results[name]["last"][k], float) else results[name]["last"][k]
        summary[name] = line
        print(json.dumps(line), flush=True)
    rel = {}
    for name, _ in legs:
        base = name + "@parent"
        if base in summary:  # the flag-off pairs: the difference against the larger spread of the two
            rel[f"{name} minus {base} ms"] = round(summary[name]["frame_ms_median"] - summary[base]["frame_ms_median"], 3)
            rel[f"{name} bound ms"] = max(summary[name]["spread_ms"], summary[base]["spread_ms"])
    for m in ("sun", "soft"):
        mis = summary[f"{m}:env_mis"]
        for other in ("env_nee", "env"):
            o = summary[f"{m}:{other}"]
            t = mis["frame_ms_median"] / o["frame_ms_median"]
            v = mis["variance_sum"] / o["variance_sum"]
            rel[f"{m}: env_mis over {other}"] = {"frame_time_ratio": round(t, 4), "variance_ratio_equal_spp": float(f"{v:.4g}"),
                                                 "variance_ratio_equal_time": float(f"{v * t:.4g}")}
    print(json.dumps({"summary": rel}), flush=True)


if __name__ == "__main__":
    main()
