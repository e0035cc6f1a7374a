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

Method: tools/ab_bench.py's. The env and env_nee legs then render one frame on a second context with
WFPT_FLAG_DENOISE and report the sum of wfpt_read_variance over the frame. The summary gives the frame-time ratio, the variance ratio at
equal spp and, as section 9h does, the variance ratio at equal time = (variance ratio) * (frame-time ratio)."""
import json
import sys

import ab_bench as ab

EXTRA_KEYS, DIGITS = ("connect_ms_timed", "connect_launches_timed", "stages_ms_timed", "variance_sum"), 6


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
    out = {"leg": a.leg, "loop": pt.loop_kind, "frame_ms": ab.timed_frames(pt, a.spp, a.frames)}
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


def options():
    ap = ab.parser(triangles=None)
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its libwfpt.so built")
    return ap


def legs(a):
    return ab.with_twins([ab.entry("shirley:off"), ab.entry("shirley:env"), ab.entry("shirley:env_nee")], a.parent_tree)


def main():
    a = options().parse_args()
    if a.leg:
        return leg(a)
    summary = ab.summarise(ab.run_legs(__file__, legs(a), a), a, EXTRA_KEYS, DIGITS)
    rel = ab.ratios(summary, ab.twin_pairs(summary) + [("shirley:off", "shirley:env"), ("shirley:env_nee", "shirley:env")])
    if "variance_sum" in summary.get("shirley:env_nee", {}) and "variance_sum" in summary.get("shirley:env", {}):
        t = summary["shirley:env_nee"]["frame_ms_median"] / summary["shirley:env"]["frame_ms_median"]
        v = summary["shirley:env_nee"]["variance_sum"] / summary["shirley:env"]["variance_sum"]
        rel.update(frame_time_ratio=round(t, 4), variance_ratio_equal_spp=float(f"{v:.4g}"), variance_ratio_equal_time=float(f"{v * t:.4g}"))
    print(json.dumps({"summary": rel}), flush=True)


if __name__ == "__main__":
    main()
