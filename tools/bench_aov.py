"""Prices the first-hit AOV pass (WFPT_FLAG_AOV): the same frames rendered with and without the flag.

    python tools/bench_aov.py [--scene shirley|mesh|both] [--spp 64] [--steps 5] [--warmup 1] [--width 1920 --height 1080]

Per scene (the seeded Shirley spheres; the 1 M-triangle soup), bench.py's flagship configuration: 8 bounces, the dispatch-keyed RNG,
all samples of a frame in flight. For each of flags 0 and WFPT_FLAG_AOV: `ms_per_frame` is the wall time of render(spp) +
synchronize (the captured graph, as bench.py times it), median over --steps frames; then one timed frame (hipEvent pairs around
every launch) gives the AOV launches' own time and bounce_kernel<first>'s, and their ratio. Prints one JSON line per scene.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import wavefront_path_tracer_amd as W  # noqa: E402


def tracer(args, scene, flags):
    kw = dict(seed=1, max_wavefronts=args.bounces, rng_mode=W.RNG_DISPATCH, flags=flags, batch=min(args.spp, 128))
    if scene == "mesh":
        return W.mesh_path_tracer(args.width, args.height, args.triangles, **kw)
    return W.shirley_path_tracer(args.width, args.height, **kw)


def measure(args, scene, flags):
    pt = tracer(args, scene, flags)
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
    L.wfpt_reset_progress(pt.handle)
    ms, launches = pt.render_timed(args.spp)
    out = {"ms_per_frame": round(statistics.median(walls), 3), "ms_per_frame_all": [round(x, 3) for x in walls],
           "loop": pt.loop_kind, "bounce_first_ms": round(float(ms[W.STAGES["bounce_first"]]), 3),
           "timed_frame_ms": round(float(ms.sum()), 3)}
    if flags & W.FLAG_AOV:
        aov_ms, aov_launches = pt.aov_timing()
        out.update(aov_ms=round(aov_ms, 3), aov_launches=aov_launches, timed_frame_ms=round(float(ms.sum()) + aov_ms, 3))
    pt.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", choices=["shirley", "mesh", "both"], default="both")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--triangles", type=int, default=1000000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    if W.device_count() < 1:
        raise SystemExit("bench_aov: no HIP device (there is no CPU fallback)")
    scenes = ["shirley", "mesh"] if args.scene == "both" else [args.scene]
    for scene in scenes:
        off, on = measure(args, scene, 0), measure(args, scene, W.FLAG_AOV)
        line = {"scene": scene, "size": f"{args.width}x{args.height}", "spp": args.spp, "bounces": args.bounces, "without_aov": off,
                "with_aov": on, "aov_ms_per_frame": on["aov_ms"],
                "aov_over_bounce_first": round(on["aov_ms"] / on["bounce_first_ms"], 3) if on["bounce_first_ms"] else None,
                "frame_cost": round(on["ms_per_frame"] / off["ms_per_frame"] - 1.0, 4), "build": W._build.build_info().get("git_head")}
        if scene == "mesh":
            line["triangles"] = args.triangles
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
