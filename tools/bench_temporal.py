"""Prices the temporal denoiser (include/wfpt.h "Temporal denoiser") next to the spatial one.

    python tools/bench_temporal.py [--spp 4] [--calls 20] [--warmup 3] [--width 1920 --height 1080]

The seeded Shirley spheres in bench.py's flagship configuration (8 bounces, the dispatch-keyed RNG). One epoch of --spp samples and a
temporal call, a yaw of ~4 px, the frame offset continued, another --spp samples: the calls below then reproject a real history.
`temporal_prepare_ms`: the hipEvent time of one wfpt_denoise_temporal call's launches with iterations = 0 (temporal_prepare_kernel alone),
median over --calls calls after --warmup; `temporal_ms` the same at the default parameters and `denoise_ms` wfpt_denoise's (prepare and the
passes), `prepare_ms` wfpt_denoise with iterations = 0. Every call is a pure function of the sealed history and the sums, so repeating it
measures the same work. Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import wavefront_path_tracer_amd as W  # noqa: E402


def median_ms(args, call, timing):
    times = []
    for k in range(args.warmup + args.calls):
        call()
        if k >= args.warmup:
            times.append(timing()[0])
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if W.device_count() < 1:
        raise SystemExit("bench_temporal: no HIP device (there is no CPU fallback)")
    pt = W.shirley_path_tracer(args.width, args.height, seed=1, max_wavefronts=args.bounces, rng_mode=W.RNG_DISPATCH, flags=W.FLAG_DENOISE,
                               batch=min(args.spp, 128))
    pt.render(args.spp)
    pt.denoise_temporal()
    cc = pt.render_parameters.camera_controller().copy()
    cc.camera.yaw = cc.camera.yaw + 4.0 * 0.3527 / args.height  # about 4 px: 2 tan(10 deg) per image height (the book camera)
    pt.render_parameters.update_camera_controller(cc)
    pt.update_buffers()
    pt.set_frame_offset(args.spp)
    pt.render(args.spp)
    pt.synchronize()
    prep_t = median_ms(args, lambda: pt.denoise_temporal(iterations=0), pt.temporal_timing)
    full_t = median_ms(args, pt.denoise_temporal, pt.temporal_timing)
    history = float((pt.temporal("length") > args.spp).mean())
    prep_d = median_ms(args, lambda: pt.denoise(iterations=0), pt.denoise_timing)
    full_d = median_ms(args, pt.denoise, pt.denoise_timing)
    pt.close()
    px = args.width * args.height
    print(json.dumps({"size": f"{args.width}x{args.height}", "spp": args.spp, "bounces": args.bounces,
                      "iterations": W.TEMPORAL_DEFAULTS["iterations"], "history_cap": W.TEMPORAL_DEFAULTS["history_cap"],
                      "temporal_prepare_ms": round(prep_t, 4), "temporal_ms": round(full_t, 4), "prepare_ms": round(prep_d, 4),
                      "denoise_ms": round(full_d, 4), "temporal_extra_ms": round(full_t - full_d, 4),
                      "temporal_prepare_gb_s_at_350_b_per_px": round(350.0 * px / (prep_t * 1e-3) / 1e9, 1),
                      "pixels_with_history": round(history, 4), "build": W._build.build_info().get("git_head")}), flush=True)


if __name__ == "__main__":
    main()
