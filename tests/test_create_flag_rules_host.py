"""What wfpt_create makes of every combination of the optional features' flags, without a GPU.

The rules ("X needs Y", "X does not go with Z") are checked before wfpt_create looks for a device, so with params.device = -1 a refused
combination reports its rule and an accepted one ends at "no HIP device", on any machine, with nothing allocated. Every combination of
the fourteen flags the rules mention, times the two rng_modes (32768 cases), is compared with tests/golden/create_flag_refusals.json.

The fixture was recorded from the library of commit 81c2c42, the last one that spelt the rules as a chain of ifs:
    WFPT_LIB=<that library> python tests/test_create_flag_rules_host.py --record
It holds the flag names (bit k of a case's index is flags[k]), the distinct messages, and per rng_mode one string with one base-36 digit
per case: the index of the case's message."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "create_flag_refusals.json")
FLAGS = ["BINNING", "RETIRE", "ADAPTIVE", "AOV", "DENOISE", "ENVIRONMENT", "EMISSION", "NEE", "ENV_NEE", "MIS", "ENV_MIS", "LIGHT_POWER",
         "ANALYTIC_LIGHTS", "SHADING_NORMALS"]
DIGITS = "0123456789abcdefghijklmnopqrstuvwxyz"


def refusals(W):
    """Per rng_mode, per case: wfpt_last_error(NULL) after wfpt_create of one sphere, one material and one node on device -1."""
    L = W.lib()
    bit = [getattr(W, "FLAG_" + name) for name in FLAGS]
    spheres, materials, nodes = np.zeros(1, W.SPHERE), np.zeros(1, W.MATERIAL), np.zeros(1, W.BVH_NODE)
    spheres["radius"] = 1.0
    nodes["aabb_min"], nodes["aabb_max"], nodes["prim_count"] = -1.0, 1.0, 1
    cam, mat = np.zeros(1, W.GPU_CAMERA), np.eye(4, dtype="<f4")
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    out = []
    for rng_mode in (W.RNG_DISPATCH, W.RNG_PIXEL):
        msgs = []
        for case in range(1 << len(FLAGS)):
            flags = sum(b for k, b in enumerate(bit) if case >> k & 1)
            p = W._Params(16, 16, 0, 4, 0, rng_mode, flags, 0, 0, -1, 1)
            handle = L.wfpt_create(C.byref(p), ptr(spheres), 1, ptr(materials), 1, ptr(nodes), 1, ptr(cam), ptr(mat), ptr(mat))
            assert not handle, f"wfpt_create succeeded on device -1 (flags {flags:#x})"
            msgs.append(L.wfpt_last_error(None).decode())
        out.append(msgs)
    return out


def names(case):
    return " | ".join(n for k, n in enumerate(FLAGS) if case >> k & 1) or "none"


def test_every_flag_combination_is_refused_or_accepted_as_recorded():
    import wavefront_path_tracer_amd as W
    fx = json.load(open(FIXTURE))
    assert fx["flags"] == FLAGS and len(fx["cases"]) == 2 and all(len(s) == 1 << len(FLAGS) for s in fx["cases"])
    got = refusals(W)
    bad = [(mode, case) for mode in range(2) for case in range(1 << len(FLAGS))
           if got[mode][case] != fx["messages"][DIGITS.index(fx["cases"][mode][case])]]
    report = "\n".join(f"rng_mode {m}, {names(c)}: {got[m][c]!r}, recorded {fx['messages'][DIGITS.index(fx['cases'][m][c])]!r}" for m, c in bad[:8])
    assert not bad, f"{len(bad)} of {2 << len(FLAGS)} cases differ from the recording:\n{report}"


def test_the_recording_is_what_the_rules_say():
    """The fixture itself: an accepted case ends at the device check; every rule's message occurs; WFPT_FLAG_ENV_MIS's own refusal of
    WFPT_FLAG_MIS occurs nowhere (no combination reaches it: the WFPT_FLAG_ENV_NEE it needs is refused with WFPT_FLAG_MIS first), which
    is why the rule table has no row for it."""
    fx = json.load(open(FIXTURE))
    msgs = fx["messages"]
    assert len(set(msgs)) == len(msgs) <= len(DIGITS)
    used = {DIGITS.index(d) for s in fx["cases"] for d in s}
    assert used == set(range(len(msgs)))
    assert fx["cases"][0][0] == fx["cases"][1][0] and "no HIP device" in msgs[DIGITS.index(fx["cases"][0][0])], "no flag at all is accepted"
    assert sum("no HIP device" in m for m in msgs) == 1
    assert all(m.startswith("wfpt_create: ") for m in msgs)
    for name in FLAGS:
        if name not in ("AOV", "DENOISE", "ENVIRONMENT", "EMISSION"):  # (these four only occur in other flags' rules)
            assert any(m.startswith(f"wfpt_create: WFPT_FLAG_{name} ") for m in msgs), name
    assert not any("WFPT_FLAG_ENV_MIS does not go with" in m for m in msgs)
    # the binned loop's rule is the only one that reads rng_mode: the two modes differ exactly where BINNING is set and it fires
    a, b = fx["cases"]
    binning = next(k for k, m in enumerate(msgs) if "WFPT_FLAG_BINNING needs WFPT_RNG_PIXEL" in m)
    assert all((x == y) or (case & 1 and x == DIGITS[binning]) for case, (x, y) in enumerate(zip(a, b)))
    assert all(x == DIGITS[binning] for case, x in enumerate(a) if case & 1)


def record():
    import wavefront_path_tracer_amd as W
    got = refusals(W)
    msgs = []
    for m in got[0] + got[1]:
        if m not in msgs:
            msgs.append(m)
    assert len(msgs) <= len(DIGITS)
    fx = {"flags": FLAGS, "messages": msgs, "cases": ["".join(DIGITS[msgs.index(m)] for m in mode) for mode in got]}
    with open(FIXTURE, "w") as f:
        json.dump(fx, f, indent=0)
        f.write("\n")
    print(f"{FIXTURE}: {len(msgs)} messages, {sum(len(s) for s in fx['cases'])} cases")


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: WFPT_LIB=<library> python tests/test_create_flag_rules_host.py --record")
    record()
