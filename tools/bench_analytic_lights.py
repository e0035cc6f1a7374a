#!/usr/bin/env python3
"""tools/bench_analytic_lights.py: what the analytic lights cost per frame and what a sun brings over its workaround
(WFPT_FLAG_ANALYTIC_LIGHTS).

Legs on the Shirley scene, --spp samples per frame, all with WFPT_FLAG_EMISSION | WFPT_FLAG_NEE:
  nee       the three big spheres emit                                         (section 9h's flagged leg: the reference point)
  analytic  the same, plus WFPT_FLAG_ANALYTIC_LIGHTS with one point, one spot and one directional light
  sun       WFPT_FLAG_ANALYTIC_LIGHTS, nothing emits, one directional light     (the main case)
  far       no flag: the workaround, a huge far emissive sphere in the sun's direction with the sun's irradiance
            (radius --far-radius at distance --far-distance; radiance = irradiance / (pi (radius / distance)^2))
`sun` and `far` carry WFPT_FLAG_DENOISE as well: after the timed frames each renders --variance-spp samples into a fresh accumulation
and reports the sum of wfpt_read_variance over the image, the variance of the frame at equal samples.

Method: tools/ab_bench.py's. The connect launches' own time comes from wfpt_nee_timing_ms over one timed frame
(hipEvent pairs around every launch, so it is slower than the frame it describes); connect_ms_per_launch is that total over its launch
count."""
import json
import sys

import ab_bench as ab

EXTRA_KEYS = ("emitters", "analytic_lights", "connect_ms_timed", "connect_launches_timed", "connect_ms_per_launch", "stages_ms_timed", "variance_sum",
              "mean_luminance")
DIGITS = 6
SUN_DIRECTION, SUN_IRRADIANCE = (-0.4, -1.0, -0.3), (3.0, 2.7, 2.1)


def leg(a):
    sys.path.insert(0, a.tree)
    import numpy as np
    import wavefront_path_tracer_amd as W
    flags = W.FLAG_EMISSION | W.FLAG_NEE
    if a.leg in ("analytic", "sun"):
        flags |= W.FLAG_ANALYTIC_LIGHTS
    if a.leg in ("sun", "far"):
        flags |= W.FLAG_DENOISE
    scene = W.Scene.book_one_final(1)
    far_material = None
    if a.leg == "far":  # one more sphere and one more material: the BVH has to carry it
        d = np.asarray(SUN_DIRECTION, np.float64)
        d /= np.linalg.norm(d)
        sp, mt = np.zeros(1, W.SPHERE), np.zeros(1, W.MATERIAL)
        sp["center"][0] = (*(-d * a.far_distance), 1.0)
        sp["radius"] = a.far_radius
        sp["material_idx"] = far_material = len(scene.materials)
        mt["albedo"][0] = (0.0, 0.0, 0.0, 1.0)
        scene = W.Scene(np.concatenate([scene.spheres, sp]), np.concatenate([scene.materials, mt]))
    cc = W.CameraController(W.Camera.book_one_final_camera(), 20.0, 0.6, 10.0, 0.1, 100.0, 4.0, 0.1)
    pt = W.PathTracer(scene, W.RenderParameters(cc, (a.width, a.height)), max_wavefronts=a.bounces, rng_mode=W.RNG_DISPATCH, flags=flags, batch=64)
    if a.leg in ("nee", "analytic"):
        sp = pt.scene.spheres
        for m, c in zip(sp["material_idx"][sp["radius"] == 1.0], ((4.0, 3.0, 2.0), (0.25, 0.5, 1.5), (1.0, 1.0, 1.0))):
            pt.set_emission(int(m), c)
    lights = np.zeros(3, W.LIGHT)
    lights["type"] = (W.LIGHT_POINT, W.LIGHT_SPOT, W.LIGHT_DIRECTIONAL)
    lights["position"] = [(0.5, 3.0, 2.0), (3.0, 5.0, 3.0), (0.0, 0.0, 0.0)]
    lights["direction"] = [(0.0, 0.0, 0.0), (-3.0, -5.0, -3.0), SUN_DIRECTION]
    lights["colour"] = [(20.0, 10.0, 5.0), (60.0, 60.0, 90.0), SUN_IRRADIANCE]
    lights["cos_inner"], lights["cos_outer"] = 0.9, 0.6
    if a.leg == "analytic":
        pt.set_lights(lights)
    elif a.leg == "sun":
        pt.set_lights(lights[2:])
    elif a.leg == "far":
        omega = np.pi * (a.far_radius / a.far_distance) ** 2
        pt.set_emission(far_material, tuple(float(e) / omega for e in SUN_IRRADIANCE))
    ms = ab.timed_frames(pt, a.spp, a.frames)
    stage_ms, _ = pt.render_timed(a.spp)
    nee_ms, launches = pt.nee_timing()
    out = {"leg": a.leg, "loop": pt.loop_kind, "frame_ms": ms, "emitters": pt.nee_light_count(),
           "analytic_lights": pt.analytic_light_count() if flags & W.FLAG_ANALYTIC_LIGHTS else 0, "connect_ms_timed": nee_ms,
           "connect_launches_timed": launches, "connect_ms_per_launch": nee_ms / max(launches, 1), "stages_ms_timed": float(np.sum(stage_ms))}
    if flags & W.FLAG_DENOISE:
        pt.reset_progress()
        pt.render(a.variance_spp)
        out["variance_sum"] = float(pt.variance().astype(np.float64).sum())
        out["mean_luminance"] = float((pt.accumulated().astype(np.float64) @ (0.2126, 0.7152, 0.0722)).mean() / a.variance_spp)
    print(json.dumps(out), flush=True)
    pt.close()


def options():
    ap = ab.parser(triangles=None)
    ap.add_argument("--variance-spp", type=int, default=64)
    ap.add_argument("--far-radius", type=float, default=50.0)
    ap.add_argument("--far-distance", type=float, default=1000.0)
    ap.add_argument("--legs", nargs="+", default=["nee", "analytic", "sun", "far"])
    return ap


def legs(a):
    return [ab.entry(name) for name in a.legs]


def main():
    a = options().parse_args()
    if a.leg:
        return leg(a)
    summary = ab.summarise(ab.run_legs(__file__, legs(a), a), a, EXTRA_KEYS, DIGITS)
    rel = ab.ratios(summary, [("analytic", "nee")], ", frame")
    if rel:
        rel["analytic over nee, connect launch"] = round(summary["analytic"]["connect_ms_per_launch"] / summary["nee"]["connect_ms_per_launch"] - 1.0, 4)
    if "sun" in summary and "far" in summary:
        rel.update(ab.ratios(summary, [("sun", "far")], ", frame"))
        rel["variance sum, sun over far"] = round(summary["sun"]["variance_sum"] / summary["far"]["variance_sum"], 6)
    print(json.dumps({"summary": rel}), flush=True)


if __name__ == "__main__":
    main()
