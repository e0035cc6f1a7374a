"""Prices the denoiser (WFPT_FLAG_DENOISE): the filter's own time, and what the luminance moments add to a frame.

    python tools/bench_denoise.py [--spp 64] [--calls 20] [--warmup 3] [--steps 5] [--width 1920 --height 1080]

The seeded Shirley spheres in bench.py's flagship configuration (8 bounces, the dispatch-keyed RNG, all samples of a frame in flight).
`denoise_ms`: the hipEvent time of one wfpt_denoise call's launches (prepare and the passes) at the default parameters, median over
--calls calls after --warmup; `prepare_ms` the same with iterations = 0, and `ms_per_pass` = (denoise_ms - prepare_ms) / iterations.
`ms_per_frame` is the wall time of render(spp) + synchronize, median over --steps frames, with WFPT_FLAG_AOV and with
WFPT_FLAG_DENOISE; `moments_cost` is their ratio - 1. Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import wavefront_path_tracer_amd as W  # noqa: E402


def tracer(args, flags):
    return W.shirley_path_tracer(args.width, args.height, seed=1, max_wavefronts=args.bounces, rng_mode=W.RNG_DISPATCH, flags=flags,
                                 batch=min(args.spp, 128))


def frame_ms(args, pt):
    L = W.lib()
    walls = []
    for k in range(args.warmup + args.steps):
        L.wfpt_reset_progress(pt.handle)
        pt.synchronize()
        t0 = time.perf_counter()
        pt.render(args.spp)
        pt.synchronize()
        if k >= args.warmup:
            walls.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(walls), walls


def denoise_ms(args, pt, **params):
    times = []
    for k in range(args.warmup + args.calls):
        pt.denoise(**params)
        if k >= args.warmup:
            times.append(pt.denoise_timing()[0])
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if W.device_count() < 1:
        raise SystemExit("bench_denoise: no HIP device (there is no CPU fallback)")
    aov = tracer(args, W.FLAG_AOV)
    aov_ms, aov_all = frame_ms(args, aov)
    aov.close()
    pt = tracer(args, W.FLAG_DENOISE)
    dn_frame_ms, dn_all = frame_ms(args, pt)
    iters = W.DENOISE_DEFAULTS["iterations"]
    full = denoise_ms(args, pt)
    prep = denoise_ms(args, pt, iterations=0)
    pt.close()
    print(json.dumps({"size": f"{args.width}x{args.height}", "spp": args.spp, "bounces": args.bounces, "iterations": iters,
                      "denoise_ms": round(full, 4), "prepare_ms": round(prep, 4), "ms_per_pass": round((full - prep) / iters, 4),
                      "ms_per_frame_aov": round(aov_ms, 3), "ms_per_frame_denoise_flag": round(dn_frame_ms, 3),
                      "moments_cost": round(dn_frame_ms / aov_ms - 1.0, 4), "ms_per_frame_aov_all": [round(x, 3) for x in aov_all],
                      "ms_per_frame_denoise_flag_all": [round(x, 3) for x in dn_all], "build": W._build.build_info().get("git_head")}),
          flush=True)


if __name__ == "__main__":
    main()
