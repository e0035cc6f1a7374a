#!/usr/bin/env python3
"""tools/bench_adaptive.py: what adaptive sampling costs and brings (WFPT_FLAG_ADAPTIVE).

Frame legs, --spp samples per frame, named scene:setting; scenes `shirley` and `mesh` (the --triangles soup) at --width x --height:
  off      no flag                                   (a) with --parent-tree DIR also the same frame of that tree (`off@parent`): a context
                                                         without the flag launches the parent's kernels, so the two should be equal
                                                         within the spread reported here
  on       the flag, every pixel active              (b) the price of the mask loads, the counts and the moments
  random   the flag, a seeded random half of the 8x8 tiles masked off
  contig   the flag, the left half of the tile columns masked off (sky and ground on both sides: with the upper half off no primary ray
           of Shirley's frame misses, and the reference's loop exit `misses < miss_floor` ends every sample after its first wavefront)
                                                     (c) how much of a dead tile's cost the first launch and accumulate shed without
                                                         compacting slots
and one quality leg per scene, scene:adaptive (d): wfpt_render_adaptive at the default parameters (at most --max-passes passes, an update
every --interval) against uniform --spp, both measured against a uniform --reference-spp render of the same context whose frames are
offset (wfpt_set_frame_offset) so that it shares no sample with either: wall time, total samples (the sum of the counts), RMSE of the
mean over the pixels that are finite in both (the reference's shaders leave a few NaN pixels on Shirley; their number is reported) and,
since the criterion is a relative one, the RMS of the luminance error relative to the reference's luminance + luminance_floor; then the
uniform render that takes the adaptive one's time (equal time: its RMSE), and the uniform samples that would reach the adaptive RMSE
under the 1/n law (equal error: its time, extrapolated).

Method: tools/ab_bench.py's. The quality leg runs once, in a child of its own, after the frame legs."""
import json
import sys
import time

import ab_bench as ab

EXTRA_KEYS, DIGITS = ("rays_per_frame", "active_share"), None  # (as they came)


def make(W, a, scene, flags):
    if scene == "shirley":
        return W.shirley_path_tracer(a.width, a.height, max_wavefronts=a.bounces, rng_mode=W.RNG_DISPATCH, flags=flags, batch=64)
    return W.mesh_path_tracer(a.width, a.height, a.triangles, max_wavefronts=a.bounces, rng_mode=W.RNG_DISPATCH, flags=flags, batch=64)


def tile_mask(np, a, setting):
    """one bool per pixel: half of the 8x8 tiles off"""
    tx, ty = (a.width + 7) // 8, (a.height + 7) // 8
    if setting == "random":
        on = np.random.default_rng(1).permutation(tx * ty).reshape(ty, tx) % 2 == 0
    else:
        on = np.repeat((np.arange(tx) >= tx // 2)[None, :], ty, axis=0)
    return np.repeat(np.repeat(on, 8, axis=0), 8, axis=1)[:a.height, :a.width]


def frame_leg(W, np, a, scene, setting):
    pt = make(W, a, scene, 0 if setting == "off" else W.FLAG_ADAPTIVE)
    active = 1.0
    if setting in ("random", "contig"):
        m = tile_mask(np, a, setting)
        pt.set_active_mask(m)
        active = float(m.mean())
    ms = ab.timed_frames(pt, a.spp, a.frames)
    totals = [int(x) for x in pt.totals()]
    out = {"leg": a.leg, "loop": pt.loop_kind, "frame_ms": ms, "rays_per_frame": totals[0] / (a.frames + 2),  # (timed_frames warms up with two)
           "active_share": active}
    pt.close()
    return out


def quality_leg(W, np, a, scene):
    pt = make(W, a, scene, W.FLAG_ADAPTIVE)

    def timed(call):
        pt.synchronize()
        t0 = time.perf_counter()
        call()
        pt.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def luma(v):
        return 0.2126 * v[:, 0] + 0.7152 * v[:, 1] + 0.0722 * v[:, 2]

    def errors(ref):
        """(RMSE of the mean, relative RMS error of its luminance, pixels left out as not finite)"""
        m = pt.mean().astype(np.float64)
        ok = np.isfinite(m).all(axis=1) & np.isfinite(ref).all(axis=1)
        d = m[ok] - ref[ok]
        rel = (luma(m[ok]) - luma(ref[ok])) / (luma(ref[ok]) + floor)
        return float(np.sqrt(np.mean(d * d))), float(np.sqrt(np.mean(rel * rel))), int((~ok).sum())

    floor = pt.adaptive()["luminance_floor"]

    pt.render(a.spp)  # warm-up
    pt.adaptive_update()
    pt.reset_progress()
    pt.set_frame_offset(1 << 20)
    pt.render(a.reference_spp)
    ref = pt.mean().astype(np.float64)
    pt.set_frame_offset(0)
    pt.reset_progress()
    n_active = [0]

    def adaptive():
        n_active[0] = pt.render_adaptive(a.max_passes, a.interval)

    t_a = timed(adaptive)
    counts = pt.sample_counts()
    (e_a, r_a, bad_a), samples_a, passes_a = errors(ref), int(counts.sum(dtype=np.int64)), int(W.lib().wfpt_accumulated_samples(pt.handle))
    pt.reset_progress()
    t_u = timed(lambda: pt.render(a.spp))
    e_u, r_u, _ = errors(ref)
    n_eq = max(1, int(round(a.spp * t_a / t_u)))
    pt.reset_progress()
    t_eq = timed(lambda: pt.render(n_eq))
    e_eq, r_eq, _ = errors(ref)
    n_err = a.spp * (e_u / e_a) ** 2 if e_a > 0 else float("inf")
    out = {"leg": a.leg, "loop": pt.loop_kind, "params": pt.adaptive(), "max_passes": a.max_passes, "interval": a.interval,
           "reference_spp": a.reference_spp, "pixels": a.width * a.height,
           "adaptive": {"ms": t_a, "passes": passes_a, "samples": samples_a, "samples_per_pixel": samples_a / (a.width * a.height),
                        "max_count": int(counts.max()), "min_count": int(counts.min()), "still_active": n_active[0], "rmse": e_a, "relative_rms": r_a,
                        "pixels_not_finite": bad_a},
           "uniform": {"spp": a.spp, "ms": t_u, "samples": a.spp * a.width * a.height, "rmse": e_u, "relative_rms": r_u},
           "equal_time": {"uniform_spp": n_eq, "ms": t_eq, "rmse": e_eq, "relative_rms": r_eq,
                          "rmse_uniform_over_adaptive": e_eq / e_a if e_a > 0 else None,
                          "relative_rms_uniform_over_adaptive": r_eq / r_a if r_a > 0 else None},
           "equal_error": {"uniform_spp_1_over_n_law": n_err, "ms_extrapolated": t_u * n_err / a.spp,
                           "time_uniform_over_adaptive": t_u * n_err / a.spp / t_a}}
    pt.close()
    return out


def leg(a):
    sys.path.insert(0, a.tree)
    import numpy as np
    import wavefront_path_tracer_amd as W
    scene, setting = a.leg.split(":")
    out = quality_leg(W, np, a, scene) if setting == "adaptive" else frame_leg(W, np, a, scene, setting)
    print(json.dumps(out), flush=True)


def options():
    ap = ab.parser(frames=12)
    ap.add_argument("--max-passes", type=int, default=256)
    ap.add_argument("--interval", type=int, default=16)
    ap.add_argument("--reference-spp", type=int, default=1024)
    ap.add_argument("--scenes", nargs="+", default=["shirley", "mesh"])
    ap.add_argument("--no-quality", action="store_true", help="skip the scene:adaptive legs")
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its libwfpt.so built")
    return ap


def legs(a):
    out = []
    for scene in a.scenes:
        out.append(ab.entry(f"{scene}:off"))
        if a.parent_tree:
            out.append(ab.entry(f"{scene}:off@parent", tree=a.parent_tree))
        out += [ab.entry(f"{scene}:{setting}") for setting in ("on", "random", "contig")]
    return out


def main():
    a = options().parse_args()
    if a.leg:
        return leg(a)
    summary = ab.summarise(ab.run_legs(__file__, legs(a), a), a, EXTRA_KEYS, DIGITS)
    rel = {}
    for name in summary:
        scene, setting = name.split("@")[0].split(":")
        if "@" in name:
            rel.update(ab.ratios(summary, [(f"{scene}:off", name)]))
        elif setting == "on":
            rel.update(ab.ratios(summary, [(name, f"{scene}:off")]))
        elif setting != "off":  # a share of the all-active frame, not an excess over it
            rel[f"{name} over {scene}:on"] = round(summary[name]["frame_ms_median"] / summary[f"{scene}:on"]["frame_ms_median"], 4)
    if not a.no_quality:
        for scene in a.scenes:
            q = ab.run_child(__file__, ab.entry(f"{scene}:adaptive"), a)
            print(json.dumps(q), flush=True)
            rel[f"{scene}: equal time, RMSE uniform over adaptive"] = q["equal_time"]["rmse_uniform_over_adaptive"]
            rel[f"{scene}: equal time, relative RMS uniform over adaptive"] = q["equal_time"]["relative_rms_uniform_over_adaptive"]
            rel[f"{scene}: equal error, time uniform over adaptive (1/n law)"] = q["equal_error"]["time_uniform_over_adaptive"]
    print(json.dumps({"summary": rel}), flush=True)


if __name__ == "__main__":
    main()
