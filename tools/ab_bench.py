"""tools/ab_bench.py: the child-process A/B method of the per-feature benchmarks (tools/bench_<feature>.py), once.

Every leg runs in a fresh child process (nothing is shared between legs but the machine), --rounds times, the legs alternating within a
round so that drift hits them alike. A child warms up with two frames (graph capture, first touch of every buffer), synchronises, then
times --frames frames one by one, each ending in a device synchronise. A leg's figure is the median of all its frames; its spread is the
range of its per-round medians. One JSON line is printed per leg, then one {"summary": ...} line of ratios. A leg that fails or takes
more than 600 s ends the whole run: no further child is started.

A tool is one file run in two roles. Without --leg it is the parent: it lists its legs and calls run_legs, summarise and ratios. With
--leg (hidden, as --tree is) it is a child: it builds the leg's scene in the tree named, calls timed_frames and prints one JSON line with
"leg", "loop", "frame_ms" and the tool's extra fields. A child starts with WFPT_LIB removed from its environment, so every tree loads its
own library; a leg that names a library gets WFPT_LIB set to it."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMMON = {"width": 1920, "height": 1080, "spp": 64, "bounces": 8, "frames": 20, "rounds": 3, "triangles": 1000000}
# what steers the parent and never reaches a child; every other option of a tool is handed on with its value
ORCHESTRATION = {"rounds", "legs", "scenes", "parent_tree", "parent_root", "closest_lib", "no_quality", "leg", "tree"}


def parser(**defaults):
    """The common options, each an int, with COMMON's defaults or the tool's own (None: the tool has no such option), and the two hidden
    child options. A tool adds its own options, spelled --like-their-dest: child_command relies on that."""
    ap = argparse.ArgumentParser()
    for name, value in {**COMMON, **defaults}.items():
        if value is not None:
            ap.add_argument("--" + name, type=int, default=value)
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    return ap


def entry(name, arg=None, tree=ROOT, lib=None, **overrides):
    """One leg of a tool's list: (name, the child's --leg (the name up to its '@'), the tree to import, a library for WFPT_LIB or None,
    option values for this leg alone)."""
    return name, arg or name.split("@")[0], os.path.abspath(tree), lib and os.path.abspath(lib), overrides


def with_twins(legs, parent_tree, has_twin=lambda name: True):
    """The legs, each followed by its `<leg>@parent` twin in parent_tree (if one is given) where has_twin(name)."""
    if not parent_tree:
        return list(legs)
    return [x for leg in legs for x in ([leg, entry(leg[0] + "@parent", tree=parent_tree)] if has_twin(leg[0]) else [leg])]


def twin_pairs(summary):
    """(leg, its twin) for ratios, for every leg that is no twin itself; ratios skips those whose twin did not run."""
    return [(name, name + "@parent") for name in summary if not name.endswith("@parent")]


def timed_frames(pt, spp, frames):
    """Milliseconds of `frames` frames of spp samples, one by one, after two warm-up frames (graph capture, first touch of every buffer)."""
    pt.render(spp)
    pt.render(spp)
    pt.synchronize()
    ms = []
    for _ in range(frames):
        t0 = time.perf_counter()
        pt.render(spp)
        pt.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def frames_within(pt, spp, ms):
    """Render frames of spp samples, each ending in a device synchronise, until `ms` milliseconds have passed; the number of frames."""
    n, t0 = 0, time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < ms:
        pt.render(spp)
        pt.synchronize()
        n += 1
    return n


def child_command(script, arg, tree, args, overrides):
    cmd = [sys.executable, os.path.abspath(script), "--leg", arg, "--tree", tree]
    for dest, value in {**vars(args), **overrides}.items():
        if dest in ORCHESTRATION or value is None or value is False:
            continue
        cmd.append("--" + dest.replace("_", "-"))
        if value is not True:
            cmd += [str(x) for x in value] if isinstance(value, (list, tuple)) else [str(value)]
    return cmd


def run_child(script, leg, args):
    """Start one leg's child and return its last stdout line, parsed. A failed or hung child ends the run."""
    name, arg, tree, lib, overrides = leg
    env = dict(os.environ)
    env.pop("WFPT_LIB", None)  # each tree loads its own library
    if lib:
        env["WFPT_LIB"] = lib
    res = subprocess.run(child_command(script, arg, tree, args, overrides), stdout=subprocess.PIPE, text=True, env=env, timeout=600)
    if res.returncode != 0:
        sys.exit(f"{os.path.splitext(os.path.basename(script))[0]}: leg {name} failed with status {res.returncode}")
    return json.loads(res.stdout.strip().splitlines()[-1])


def run_legs(script, legs, args):
    """args.rounds rounds of the legs in list order; {name: [the child's line of round 0, of round 1, ...]}."""
    results = {leg[0]: [] for leg in legs}
    for _ in range(args.rounds):
        for leg in legs:
            r = run_child(script, leg, args)
            results[leg[0]].append(r)
            print(f"{leg[0]}: {statistics.median(r['frame_ms']):.3f} ms", file=sys.stderr, flush=True)  # progress; the figures follow
    return results


def summarise(results, args, extra_keys, digits=None, bounces_of=None):
    """Print and return {name: line}, one line per leg: the run's settings, the three figures, then those of extra_keys that the leg's last
    child reported, floats rounded to `digits` (None: as they came). bounces_of(name) replaces args.bounces where a leg has its own."""
    summary = {}
    for name, rounds in results.items():
        per_round = [statistics.median(r["frame_ms"]) for r in rounds]
        last = rounds[-1]
        line = {"leg": name, "loop": last["loop"], "size": [args.width, args.height], "spp": args.spp,
                "bounces": bounces_of(name) if bounces_of else args.bounces, "frames": args.frames, "rounds": args.rounds,
                "frame_ms_median": round(statistics.median(x for r in rounds for x in r["frame_ms"]), 3),
                "round_medians_ms": [round(x, 3) for x in per_round], "spread_ms": round(max(per_round) - min(per_round), 3)}
        for k in extra_keys:
            if k in last:
                line[k] = round(last[k], digits) if digits is not None and isinstance(last[k], float) else last[k]
        summary[name] = line
        print(json.dumps(line), flush=True)
    return summary


def ratios(summary, pairs, suffix="", key="frame_ms_median"):
    """{"num over den<suffix>": num's figure over den's, less one} for the pairs both of whose legs ran."""
    return {f"{num} over {den}{suffix}": round(summary[num][key] / summary[den][key] - 1.0, 4)
            for num, den in pairs if num in summary and den in summary}
