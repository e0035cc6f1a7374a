#!/usr/bin/env python3
"""tools/bench_retire.py: what path termination brings per frame (WFPT_FLAG_RETIRE).

Legs, --spp samples per frame, named scene:kind:setting. Kinds: `plain` no feature flag, `lit` WFPT_FLAG_EMISSION, `nee` with WFPT_FLAG_NEE.
Settings: `off` without WFPT_FLAG_RETIRE, `dead` with the flag and roulette off (dead paths alone are retired: the same image), `rr`
with the default parameters (roulette from wavefront 3 on, q_min 0.05).
  shirley  plain:off | lit and nee: off, dead, rr   (the three big spheres emit)              at --width x --height, --bounces wavefronts
  room     lit: off, dead, rr                       (a closed sphere of fuzzy metal lit from inside by an emitting sphere: no ray misses;
                                                     miss_floor = 0 and --room-bounces wavefronts, the reference's 50)
  mesh     lit: off, dead, rr                       (material 1 of the soup's three emits)      the --triangles soup
and, with --parent-tree DIR (a checkout of the parent commit with its library built), the plain Shirley frame of that tree: the kernels a
context without the flag launches are the parent's, so the two are expected to be equal within the spread reported here.

Method: tools/ab_bench.py's. With --equal-time MS the lit and nee legs of shirley and room then render on a second
context with WFPT_FLAG_DENOISE (the luminance moments) for MS milliseconds and report the samples that fitted and the image mean of
wfpt_read_variance, the variance of the pixels' mean luminance: the variance at equal time."""
import json
import sys

import ab_bench as ab

EXTRA_KEYS = ("rays_per_frame", "hits_per_frame", "wavefronts_last_sample", "equal_time_ms", "equal_time_samples", "equal_time_variance")
DIGITS = None  # (as they came)


def make(W, np, a, scene, kind, setting, extra_flags=0):
    flags = extra_flags | (0 if kind == "plain" else W.FLAG_EMISSION | (W.FLAG_NEE if kind == "nee" else 0))
    if setting != "off":
        flags |= W.FLAG_RETIRE
    if scene == "room":
        sp, mt = np.zeros(3, W.SPHERE), np.zeros(3, W.MATERIAL)
        mt["albedo"][:] = (0.5, 0.5, 0.5, 1.0)
        mt["albedo"][0, :3] = (0.5, 0.75, 0.25)
        mt["albedo"][2, :3] = (0.75, 0.5, 0.5)
        mt["material_type"] = (1, 0, 0)
        mt["fuzz"][0] = 0.25
        sp["center"][:, 3] = 1.0
        sp["center"][:, :3] = [(0.0, 0.0, 0.0), (1.5, 1.0, -2.0), (-1.0, -0.5, -2.5)]
        sp["radius"] = (5.0, 1.0, 0.5)
        sp["material_idx"] = (0, 1, 2)
        sp["material_type"] = mt["material_type"][sp["material_idx"]]  # (extend hands shade the sphere's own copy of the type)
        cc = W.CameraController(W.Camera((0.5, 0.25, 1.0), (0.5, 0.0, -1.0)), 70.0, 0.0, 10.0, 0.1, 100.0)
        pt = W.PathTracer(W.Scene(sp, mt), W.RenderParameters(cc, (a.width, a.height)), max_wavefronts=a.room_bounces, miss_floor=0,
                          rng_mode=W.RNG_DISPATCH, flags=flags, batch=64)
        pt.set_emission(1, (4.0, 2.0, 8.0))
    elif scene == "shirley":
        pt = W.shirley_path_tracer(a.width, a.height, max_wavefronts=a.bounces, rng_mode=W.RNG_DISPATCH, flags=flags, batch=64)
        if kind != "plain":
            sp = pt.scene.spheres
            for m, c in zip(sp["material_idx"][sp["radius"] == 1.0], ((4.0, 3.0, 2.0), (0.25, 0.5, 1.5), (1.0, 1.0, 1.0))):
                pt.set_emission(int(m), c)
    else:
        pt = W.mesh_path_tracer(a.width, a.height, a.triangles, max_wavefronts=a.bounces, rng_mode=W.RNG_DISPATCH, flags=flags, batch=64)
        if kind != "plain":
            pt.set_emission(1, (2.0, 1.0, 0.5))
    if setting == "dead":
        pt.set_termination(W.NO_ROULETTE, 0.05)
    return pt


def leg(a):
    sys.path.insert(0, a.tree)
    import numpy as np
    import wavefront_path_tracer_amd as W
    scene, kind, setting = a.leg.split(":")
    pt = make(W, np, a, scene, kind, setting)
    ms = ab.timed_frames(pt, a.spp, a.frames)
    totals = [int(x) for x in pt.totals()]
    frames = a.frames + 2  # (timed_frames warms up with two)
    out = {"leg": a.leg, "loop": pt.loop_kind, "frame_ms": ms, "rays_per_frame": totals[0] / frames, "hits_per_frame": totals[1] / frames,
           "wavefronts_last_sample": int(len(pt.bounce_table()))}
    pt.close()
    if a.equal_time > 0 and kind != "plain" and scene != "mesh":
        pt = make(W, np, a, scene, kind, setting, W.FLAG_DENOISE)
        pt.render(a.spp)
        pt.synchronize()
        pt.reset_progress()
        n = a.spp * ab.frames_within(pt, a.spp, a.equal_time)
        out.update(equal_time_ms=a.equal_time, equal_time_samples=n, equal_time_variance=float(np.mean(pt.variance(), dtype=np.float64)))
        pt.close()
    print(json.dumps(out), flush=True)


def options():
    ap = ab.parser(frames=12)
    ap.add_argument("--room-bounces", type=int, default=50)
    ap.add_argument("--equal-time", type=float, default=0.0, help="milliseconds of rendering for the variance at equal time (0: skip)")
    ap.add_argument("--scenes", nargs="+", default=["shirley", "room", "mesh"])
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its libwfpt.so built")
    return ap


def legs(a):
    out = []
    if "shirley" in a.scenes:
        out += [ab.entry("shirley:plain:off")]
        if a.parent_tree:  # (no variance at equal time in the parent's tree)
            out.append(ab.entry("shirley:plain:off@parent", tree=a.parent_tree, equal_time=0.0))
        out += [ab.entry(f"shirley:{kind}:{setting}") for kind in ("lit", "nee") for setting in ("off", "dead", "rr")]
    for scene in ("room", "mesh"):
        if scene in a.scenes:
            out += [ab.entry(f"{scene}:lit:{setting}") for setting in ("off", "dead", "rr")]
    return out


def main():
    a = options().parse_args()
    if a.leg:
        return leg(a)
    summary = ab.summarise(ab.run_legs(__file__, legs(a), a), a, EXTRA_KEYS, DIGITS,
                           bounces_of=lambda name: a.room_bounces if name.startswith("room") else a.bounces)
    rel = {}
    for name in summary:
        scene, kind, setting = name.split("@")[0].split(":")
        base = f"{scene}:{kind}:off"
        if "@" in name:
            rel.update(ab.ratios(summary, [(base, name)]))
        elif setting != "off":
            rel.update(ab.ratios(summary, [(name, base)]))
            if "equal_time_variance" in summary[name] and summary[base].get("equal_time_variance"):
                rel.update(ab.ratios(summary, [(name, base)], ", variance at equal time", "equal_time_variance"))
    print(json.dumps({"summary": rel}), flush=True)


if __name__ == "__main__":
    main()
