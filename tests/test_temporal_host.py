"""The temporal denoiser (include/wfpt.h "Temporal denoiser") without a GPU: the ABI declares and exports it, wfpt_temporal_params has
its layout and defaults, calls without a context are refused, temporal_prepare_kernel compiles to gfx950 without scratch, and the numpy
restatement (tests/temporal_ref.py) accepts, rejects and blends history as specified."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import denoise_ref as R
import temporal_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("wfpt_set_frame_offset", "wfpt_frame_offset", "wfpt_temporal_params_default", "wfpt_denoise_temporal",
       "wfpt_denoise_temporal_to_device", "wfpt_read_temporal", "wfpt_reset_history", "wfpt_temporal_timing_ms")
F = np.float32


def test_header_and_library_carry_the_temporal_abi(wf):
    declared = wf.abi_symbols()
    L = wf.lib()
    for name in NEW:
        assert name in declared and hasattr(L, name), name
    hdr = open(os.path.join(ROOT, "include", "wfpt.h")).read()
    body = re.search(r"typedef struct wfpt_temporal_params \{(.*?)\} wfpt_temporal_params;", hdr, re.S).group(1)
    fields = re.findall(r"(wfpt_denoise_params|uint32_t|float)\s+(\w+)(\[\d+\])?;", body)
    assert [f[1] for f in fields] == ["spatial", "history_cap", "depth_tolerance", "normal_cos", "_reserved"]
    assert "sizeof(wfpt_temporal_params) == 64" in hdr
    for k, v in {"COLOR": 0, "MOMENTS": 1, "LENGTH": 2, "MOTION": 3}.items():
        assert re.search(rf"WFPT_TEMPORAL_{k} = {v}\b", hdr), k
    assert wf.TEMPORAL_OUTPUTS == {"color": (0, 3), "moments": (1, 2), "length": (2, 1), "motion": (3, 3)}
    lib_rs = open(os.path.join(ROOT, "wfpt-sys", "src", "lib.rs")).read()
    assert "pub spatial: wfpt_denoise_params," in lib_rs and "pub fn wfpt_denoise_temporal(" in lib_rs


def test_layout_and_defaults(wf, tmp_path):
    P = wf._TemporalParams
    assert C.sizeof(P) == 64 and P.history_cap.offset == 32 and P.depth_tolerance.offset == 36
    assert P.normal_cos.offset == 40 and P._reserved.offset == 44
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wfpt.h"\nint main(void) { printf("%zu %zu %zu\\n", '
                   'sizeof(wfpt_temporal_params), offsetof(wfpt_temporal_params, history_cap), offsetof(wfpt_temporal_params, _reserved)); '
                   'return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split() == ["64", "32", "44"]
    p = P()
    C.memset(C.byref(p), 0xFF, C.sizeof(p))
    wf.lib().wfpt_temporal_params_default(C.byref(p))
    got = {k: getattr(p.spatial, k) for k in wf.DENOISE_DEFAULTS}
    got.update({k: getattr(p, k) for k in ("history_cap", "depth_tolerance", "normal_cos")})
    assert got == {k: float(F(v)) if isinstance(v, float) else v for k, v in wf.TEMPORAL_DEFAULTS.items()}
    assert list(p._reserved) == [0] * 5 and list(p.spatial._reserved) == [0] * 3
    assert wf.TEMPORAL_DEFAULTS == T.DEFAULTS
    assert wf.TEMPORAL_DEFAULTS["depth_tolerance"] == 0.05 and wf.TEMPORAL_DEFAULTS["normal_cos"] == 0.9
    assert wf.TEMPORAL_DEFAULTS["history_cap"] in (8.0, 16.0, 32.0, 64.0, 128.0)
    # the Python side packs the same struct
    q = wf.PathTracer._temporal_params({"history_cap": 0.0, "iterations": 2})
    assert q.history_cap == 0.0 and q.spatial.iterations == 2 and q.spatial.sigma_albedo == F(0.5)
    with pytest.raises(TypeError):
        wf.PathTracer._temporal_params({"history": 3})


def test_temporal_calls_without_a_context_are_refused(wf):
    L = wf.lib()
    p = wf._TemporalParams()
    L.wfpt_temporal_params_default(C.byref(p))
    buf = np.zeros(12, "<f4")
    assert L.wfpt_denoise_temporal(None, C.byref(p), wf._p(buf), 3) == -1
    assert L.wfpt_denoise_temporal_to_device(None, C.byref(p), wf._p(buf), 12) == -1
    assert L.wfpt_read_temporal(None, 0, wf._p(buf), 3) == -1
    assert L.wfpt_reset_history(None) == -1
    assert L.wfpt_temporal_timing_ms(None, None, None) == -1
    assert L.wfpt_set_frame_offset(None, 3) == -1
    assert L.wfpt_frame_offset(None) == 0


@pytest.fixture(scope="module")
def kernel_metadata(tmp_path_factory):
    """wfpt_kernels.hip compiled for gfx950 to assembly (as tests/test_denoise_host.py does): kernel name -> its metadata numbers."""
    from wavefront_path_tracer_amd import _build
    out = tmp_path_factory.mktemp("isa_temporal") / "wfpt_kernels.s"
    flags = [f for f in _build.FLAGS if f not in ("-shared", "-fPIC")]
    cmd = [_build.hipcc()] + flags + ["--offload-device-only", "-S", "-I" + os.path.join(ROOT, "include"), "-I" + _build.CSRC, "-o", str(out),
                                      os.path.join(_build.CSRC, "wfpt_kernels.hip")]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-3000:]
    asm = open(out).read()
    return {m.group(1): {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\n", m.group(2))}
            for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size:", asm, re.S)}


def test_temporal_prepare_runs_without_scratch(kernel_metadata):
    hits = [n for n in kernel_metadata if "temporal_prepare_kernel" in n]
    assert len(hits) == 1, sorted(kernel_metadata)
    md = kernel_metadata[hits[0]]
    assert md["private_segment_fixed_size"] == 0, md
    assert md.get("agpr_count", 0) == 0, md
    assert md["vgpr_count"] <= 128, md


# ---- the numpy restatement on synthetic inputs
def scene(h, w, seed, n):
    """A flat, fully covered surface at depth 2 with noisy colour: current sums of n samples and a sealed epoch's state."""
    rng = np.random.default_rng(seed)
    cur = {"n": n, "sum": (F(n) * rng.random((h, w, 3), F)).astype(F), "albedo": np.full((h, w, 3), 0.5, F),
           "normal": np.repeat(np.array([[[0.0, 0.0, 1.0]]], F), h, 0).repeat(w, 1), "depth": np.full((h, w), 2.0, F),
           "coverage": np.ones((h, w), F), "material_id": np.full((h, w), 3, np.uint32)}
    L = R.luma(cur["sum"] / F(n))
    cur["s1"] = (F(n) * L).astype(F)
    cur["s2"] = (F(n) * L * L * F(1.1)).astype(F)
    sealed = {"color": rng.random((h, w, 3), F), "moments": rng.random((h, w, 2), F), "length": np.full((h, w), 8.0, F),
              "normal": cur["normal"].copy(), "depth": cur["depth"].copy(), "coverage": cur["coverage"].copy(),
              "material_id": cur["material_id"].copy()}
    return cur, sealed


def identity_motion(h, w, z):
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([x.astype(F), y.astype(F), np.full((h, w), z, F)], axis=2)


def test_reference_identity_motion_accepts_every_tap():
    h, w, n = 12, 16, 4
    cur, sealed = scene(h, w, 1, n)
    motion = identity_motion(h, w, 2.0)
    acc, tp = T.accepted(T.nhat(cur["normal"]), cur["coverage"], cur["material_id"], T.nhat(sealed["normal"]), sealed["depth"],
                         sealed["coverage"], sealed["material_id"], motion, 0.05, 0.9)
    inside = np.stack([t[3] for t in tp], axis=2)
    assert acc[inside].all() and inside[:-1, :-1].all()
    out = T.temporal_prepare(cur, sealed, motion, history_cap=32.0)
    assert (out["length"] == F(8 + n)).all()
    want = (F(8) * sealed["color"] + cur["sum"]) / F(8 + n)
    np.testing.assert_array_equal(out["color"], want.astype(F))  # the centre tap's weight is exactly 1
    # the cap limits the history a pixel carries
    capped = T.temporal_prepare(cur, sealed, motion, history_cap=2.0)
    assert (capped["length"] == F(2 + n)).all()


def test_reference_depth_step_rejects_the_disoccluded_strip():
    """The camera moved 3 px right: the old image's left strip is disoccluded where the current depth jumps, so those pixels keep only the
    current samples; the rest carry their history."""
    h, w, n = 10, 24, 2
    cur, sealed = scene(h, w, 2, n)
    cur["depth"][:, :6] = 5.0  # a far wall behind the left strip now
    motion = identity_motion(h, w, 2.0)
    motion[..., 0] += F(3.0)
    motion[:, :6, 2] = 5.0
    out = T.temporal_prepare(cur, sealed, motion)
    assert (out["length"][:, :6] == F(n)).all()              # depth 5 against the history's 2: rejected
    assert (out["length"][:, 6:w - 4] == F(8 + n)).all()     # taps inside the old image: history
    assert (out["length"][:, w - 3:] == F(n)).all()          # x' >= w: outside the old image
    # and a material or normal change rejects as well
    cur2, sealed2 = scene(h, w, 3, n)
    sealed2["material_id"][:, :4] = 7
    sealed2["normal"][:, 4:8] = [1.0, 0.0, 0.0]
    out2 = T.temporal_prepare(cur2, sealed2, identity_motion(h, w, 2.0))
    assert (out2["length"][:, :8] == F(n)).all() and (out2["length"][:, 8:] == F(8 + n)).all()


def test_reference_misses_take_only_missed_history():
    h, w, n = 8, 8, 3
    cur, sealed = scene(h, w, 4, n)
    cur["coverage"][:, :4] = 0.0
    cur["material_id"][:, :4] = 0xFFFFFFFF
    motion = identity_motion(h, w, 0.0)
    out = T.temporal_prepare(cur, sealed, motion)
    assert (out["length"][:, :4] == F(n)).all()  # the history there was covered
    sealed["coverage"][:, :4] = 0.0
    out = T.temporal_prepare(cur, sealed, motion)
    assert (out["length"][:, :4] == F(8 + n)).all()


@pytest.mark.parametrize("n", [1, 6])
def test_reference_without_history_is_the_spatial_prepare(n):
    h, w = 9, 11
    cur, sealed = scene(h, w, 5, n)
    motion = identity_motion(h, w, 2.0)
    c = cur["sum"] / F(n)
    var = R.variance_resolve(cur["s1"], cur["s2"], n)
    nz, ag, cv = R.prepare(c, cur["albedo"], cur["normal"], cur["depth"], var, n)
    for out in (T.temporal_prepare(cur, sealed, motion, history_cap=0.0), T.temporal_prepare(cur, None, None)):
        for got, want in ((out["cv"], cv), (out["nz"], nz), (out["ag"], ag)):
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert (out["length"] == F(n)).all()
        assert np.array_equal(out["moments"][..., 0], cur["s1"] / F(n))
    # no projection at all
    none = np.full((h, w, 3), T.NO_MOTION, F)
    none[..., 2] = 0.0
    out = T.temporal_prepare(cur, sealed, none)
    assert np.array_equal(out["cv"].view(np.uint32), cv.view(np.uint32))


def test_reference_short_history_scales_the_spatial_variance():
    h, w = 8, 8
    cur, sealed = scene(h, w, 6, 1)
    sealed["length"][:] = 2.0
    out = T.temporal_prepare(cur, sealed, identity_motion(h, w, 2.0))
    assert (out["length"] == F(3)).all()
    _, _, cv = R.prepare(cur["sum"], cur["albedo"], cur["normal"], cur["depth"], np.zeros((h, w), F), 1)
    np.testing.assert_array_equal(out["cv"][..., 3], cv[..., 3] * (F(1) / F(3)))


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="only meaningful on a box without a GPU")
def test_no_gpu_means_temporal_contexts_fail_loudly(wf):
    assert wf.device_count() == 0
    with pytest.raises(wf.WfptError):
        wf.shirley_path_tracer(64, 64, flags=wf.FLAG_DENOISE)
