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

Method: tools/ab_bench.py's. Each leg then renders one frame on a second context with WFPT_FLAG_DENOISE and
reports the sum of wfpt_read_variance over the frame. The summary gives, per map, the frame-time ratios, the variance ratios at equal spp
and the variance ratios at equal time = (variance ratio) * (frame-time ratio) of env_mis against env_nee and against env."""
import json
import sys

import ab_bench as ab
from bench_env_nee import sun_map

EXTRA_KEYS, DIGITS = ("connect_ms_timed", "connect_launches_timed", "miss_ms_timed", "stages_ms_timed", "variance_sum"), 6


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
    out = {"leg": a.leg, "loop": pt.loop_kind, "frame_ms": ab.timed_frames(pt, a.spp, a.frames)}
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


def options():
    ap = ab.parser(triangles=None)
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its libwfpt.so built")
    return ap


def legs(a):  # the parent has no env_mis leg
    return ab.with_twins([ab.entry(f"{m}:{k}") for m in ("sun", "soft") for k in ("env", "env_nee", "env_mis")], a.parent_tree,
                         lambda name: not name.endswith("env_mis"))


def main():
    a = options().parse_args()
    if a.leg:
        return leg(a)
    summary = ab.summarise(ab.run_legs(__file__, legs(a), a), a, EXTRA_KEYS, DIGITS)
    rel = {}
    for name, base in ab.twin_pairs(summary):
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
