#!/usr/bin/env python3
"""tools/bench_microfacet.py: what GGX microfacet metals cost per frame (WFPT_FLAG_MICROFACET).

Legs, --spp samples per frame at --width x --height, the 1 M-triangle soup and the mesh camera of BASELINE config 5 (the soup's materials
by thirds: Lambertian, Metal, Dielectric):
  parent   the soup on the PARENT commit's library (--parent-root: a checkout of it with its library built); no flag
  off      the same on this tree, no flag                                   (must lie within the spread of `parent`'s round medians)
  empty    the soup, the flag set, no roughness                             (the same launches as `off`)
  rough    the soup with its metal third at alpha 0.3                       (the pass: a third of the hits sample, two thirds copy)
  both     the same with a table of corner normals as well                  (microfacet_kernel<true> in shading_normal_kernel's place);
           `normals` is that table without roughness, the leg `both` is read against

Method, section 9o's (as tools/bench_shading_normals.py): every leg runs in a fresh child process, --rounds times, the legs alternating
within a round so that drift hits them alike. A child warms up (graph capture, first touch), then times --frames frames one by one, each
ending in a device synchronise. A leg's figure is the median of all its frames; its spread is the range of its per-round medians. The
pass's own time comes from wfpt_microfacet_timing_ms (wfpt_shading_normal_timing_ms for `normals`) over one timed frame (hipEvent pairs
around every launch, so it is slower than the frame it describes), beside the sum of that frame's stage times. Prints one JSON line per
leg and one summary line."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METAL, ALPHA = 1, 0.3


def leg(a):
    sys.path.insert(0, a.root)
    import numpy as np
    import wavefront_path_tracer_amd as W
    flags = 0
    if a.leg in ("empty", "rough", "both"):
        flags |= W.FLAG_MICROFACET
    if a.leg in ("both", "normals"):
        flags |= W.FLAG_SHADING_NORMALS
    scene = W.Scene.random_mesh(a.triangles, 1)
    n9 = None
    if a.leg in ("both", "normals"):
        t = scene.triangles
        face = np.cross(t["e1"].astype(np.float64), t["e2"].astype(np.float64))
        face /= np.linalg.norm(face, axis=1)[:, None]
        n9 = (face[:, None, :] + 0.3 * np.random.default_rng(2).normal(size=(len(t), 3, 3))).reshape(-1, 9).astype(np.float32)
        scene.triangles["_pad"] = np.arange(len(scene.triangles), dtype=np.uint32)
    cc = W.CameraController(W.Camera((0.0, 0.0, 30.0), (0.0, 0.0, 0.0)), 40.0, 0.0, 10.0, 0.1, 100.0)
    pt = W.PathTracer(scene, W.RenderParameters(cc, (a.width, a.height)), max_wavefronts=a.bounces, rng_mode=W.RNG_DISPATCH, flags=flags,
                      batch=a.batch, device_bvh=True)
    if n9 is not None:
        pt.set_triangle_normals(n9)
    if a.leg in ("rough", "both"):
        assert int(scene.materials["material_type"][METAL]) == 1
        pt.set_roughness(METAL, ALPHA)
    pt.render(a.spp)  # warm-up: graph capture, first touch of every buffer
    pt.render(a.spp)
    pt.synchronize()
    ms = []
    for _ in range(a.frames):
        t0 = time.perf_counter()
        pt.render(a.spp)
        pt.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    stage_ms, _ = pt.render_timed(a.spp)
    pass_ms, launches = 0.0, 0
    if a.leg in ("empty", "rough", "both"):
        pass_ms, launches = pt.microfacet_timing_ms()
    elif a.leg == "normals":
        pass_ms, launches = pt.shading_normal_timing()
    print(json.dumps({"leg": a.leg, "loop": pt.loop_kind, "triangles": len(scene.triangles), "frame_ms": ms, "pass_ms_timed": pass_ms,
                      "pass_launches_timed": launches, "stages_ms_timed": float(np.sum(stage_ms))}), flush=True)
    pt.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--triangles", type=int, default=1000000)
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with its library built (the `parent` leg)")
    ap.add_argument("--legs", nargs="+", default=["parent", "off", "empty", "rough", "normals", "both"])
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        return leg(a)
    legs = [name for name in a.legs if name != "parent" or a.parent_root]
    results = {name: {"rounds": [], "last": None} for name in legs}
    for _ in range(a.rounds):
        for name in legs:
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", "off" if name == "parent" else name, "--root",
                   os.path.abspath(a.parent_root) if name == "parent" else ROOT, "--width", str(a.width), "--height", str(a.height),
                   "--spp", str(a.spp), "--batch", str(a.batch), "--bounces", str(a.bounces), "--frames", str(a.frames),
                   "--triangles", str(a.triangles)]
            res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=600)  # a failed or hung leg ends the run
            if res.returncode != 0:
                sys.exit(f"bench_microfacet: leg {name} failed with status {res.returncode}")
            r = json.loads(res.stdout.strip().splitlines()[-1])
            results[name]["rounds"].append(r["frame_ms"])
            results[name]["last"] = r
            print(f"{name}: {statistics.median(r['frame_ms']):.3f} ms", file=sys.stderr, flush=True)  # progress; the figures follow
    summary = {}
    for name in legs:
        rounds, last = results[name]["rounds"], results[name]["last"]
        per_round = [statistics.median(r) for r in rounds]
        line = {"leg": name, "loop": last["loop"], "size": [a.width, a.height], "spp": a.spp, "bounces": a.bounces, "frames": a.frames,
                "rounds": a.rounds, "frame_ms_median": round(statistics.median(x for r in rounds for x in r), 3),
                "round_medians_ms": [round(x, 3) for x in per_round], "spread_ms": round(max(per_round) - min(per_round), 3)}
        for k, v in last.items():
            if k not in ("leg", "loop", "frame_ms"):
                line[k] = round(v, 6) if isinstance(v, float) else v
        summary[name] = line
        print(json.dumps(line), flush=True)
    rel = {}
    for num, den in (("off", "parent"), ("empty", "off"), ("rough", "off"), ("normals", "off"), ("both", "off"), ("both", "normals")):
        if num in summary and den in summary:
            rel[f"{num} over {den}, frame"] = round(summary[num]["frame_ms_median"] / summary[den]["frame_ms_median"] - 1.0, 4)
    if "off" in summary and "parent" in summary:
        p = summary["parent"]["round_medians_ms"]
        rel["off within the spread of parent's round medians"] = bool(min(p) <= summary["off"]["frame_ms_median"] <= max(p))
    for name in ("rough", "normals", "both"):
        if name in summary:
            p, s = summary[name]["pass_ms_timed"], summary[name]["stages_ms_timed"]  # (the pass is booked apart from the stages)
            rel[f"{name}: pass share of the timed frame"] = round(p / (p + s), 4)
    print(json.dumps({"summary": rel}), flush=True)


if __name__ == "__main__":
    main()
