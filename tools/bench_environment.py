#!/usr/bin/env python3
"""tools/bench_environment.py: frame time with and without an environment map (WFPT_FLAG_ENVIRONMENT).

For each scene (Shirley at 1920x1080, the 1M-triangle soup) three contexts render --spp samples per frame: no flag (the gradient sky), the
flag with a 2048x1024 map set, and the share of the miss launches (WFPT_STAGE_MISS: with a map they light every miss) in a timed frame.
Misses per frame come from the bounce-table totals. Prints one JSON line per scene."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import wavefront_path_tracer_amd as W  # noqa: E402


def frame_ms(pt, spp, frames):
    pt.render(spp)  # warm-up: graph capture, first touch of the map
    pt.synchronize()
    t0 = time.perf_counter()
    for _ in range(frames):
        pt.render(spp)
    pt.synchronize()
    return (time.perf_counter() - t0) * 1e3 / frames


def make(scene, w, h, bounces, flags, tris):
    if scene == "shirley":
        return W.shirley_path_tracer(w, h, max_wavefronts=bounces, rng_mode=W.RNG_DISPATCH, flags=flags, batch=64)
    return W.mesh_path_tracer(w, h, tris, max_wavefronts=bounces, rng_mode=W.RNG_DISPATCH, flags=flags, batch=64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--map", type=int, nargs=2, default=(2048, 1024), metavar=("W", "H"))
    ap.add_argument("--triangles", type=int, default=1000000)
    ap.add_argument("--scenes", nargs="+", default=["shirley", "mesh"])
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    env = (rng.random((a.map[1], a.map[0], 3)) * 2.0).astype(np.float32)
    for scene in a.scenes:
        sky = make(scene, a.width, a.height, a.bounces, 0, a.triangles)
        ms_sky = frame_ms(sky, a.spp, a.frames)
        sky.close()
        lit = make(scene, a.width, a.height, a.bounces, W.FLAG_ENVIRONMENT, a.triangles)
        lit.set_environment(env)
        ms_env = frame_ms(lit, a.spp, a.frames)
        t0 = lit.totals()
        lit.render(a.spp)
        misses = int(lit.totals()[2] - t0[2])
        stage_ms, launches = lit.render_timed(a.spp)
        miss_share = float(stage_ms[W.STAGES["miss_kernel"]]) / max(float(np.sum(stage_ms)), 1e-9)
        print(json.dumps({"scene": scene, "loop": lit.loop_kind, "size": [a.width, a.height], "spp": a.spp, "bounces": a.bounces,
                          "map": list(a.map), "frame_ms_sky": round(ms_sky, 3), "frame_ms_env": round(ms_env, 3),
                          "env_over_sky": round(ms_env / ms_sky - 1.0, 4), "misses_per_frame": misses,
                          "miss_launch_share_timed": round(miss_share, 4)}), flush=True)
        lit.close()


if __name__ == "__main__":
    main()
