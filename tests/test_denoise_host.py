"""The denoiser (WFPT_FLAG_DENOISE) without a GPU: the ABI declares and exports it, its kernels compile to gfx950 without scratch next to
an unchanged accumulate_kernel, the numpy restatement (tests/denoise_ref.py) behaves like an edge-avoiding filter, and on a box without
a device a flagged context fails loudly."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import denoise_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("wfpt_denoise_params_default", "wfpt_denoise", "wfpt_denoise_to_device", "wfpt_read_variance", "wfpt_denoise_timing_ms")
F = np.float32


def test_header_and_library_carry_the_denoise_abi(wf):
    declared = wf.abi_symbols()
    L = wf.lib()
    for name in NEW:
        assert name in declared and hasattr(L, name), name
    hdr = open(os.path.join(ROOT, "include", "wfpt.h")).read()
    assert re.search(r"WFPT_FLAG_DENOISE = 1u << 11\b", hdr)
    assert re.search(r"WFPT_FLAG_AOV = 1u << 10\b", hdr)
    body = re.search(r"typedef struct wfpt_denoise_params \{(.*?)\} wfpt_denoise_params;", hdr, re.S).group(1)
    fields = re.findall(r"(uint32_t|float)\s+(\w+)(\[\d+\])?;", body)
    assert [f[1] for f in fields] == ["iterations", "sigma_luminance", "sigma_normal", "sigma_depth", "sigma_albedo", "_reserved"]
    assert "sizeof(wfpt_denoise_params) == 32" in hdr
    assert C.sizeof(wf._DenoiseParams) == 32 and wf._DenoiseParams._reserved.offset == 20


def test_python_flag_and_default_params(wf):
    assert wf.FLAG_DENOISE == 1 << 11 and "FLAG_DENOISE" in wf.__all__
    p = wf._DenoiseParams()
    C.memset(C.byref(p), 0xFF, C.sizeof(p))
    wf.lib().wfpt_denoise_params_default(C.byref(p))
    got = {k: getattr(p, k) for k in wf.DENOISE_DEFAULTS}
    assert got == {k: float(F(v)) if isinstance(v, float) else v for k, v in wf.DENOISE_DEFAULTS.items()}
    assert list(p._reserved) == [0, 0, 0]
    assert wf.DENOISE_DEFAULTS == R.DEFAULTS
    assert wf.DENOISE_DEFAULTS["iterations"] == 5 and wf.DENOISE_DEFAULTS["sigma_luminance"] == 4.0
    assert wf.DENOISE_DEFAULTS["sigma_normal"] == 128.0 and wf.DENOISE_DEFAULTS["sigma_depth"] == 1.0


def test_denoise_calls_without_a_context_are_refused(wf):
    L = wf.lib()
    p = wf._DenoiseParams()
    L.wfpt_denoise_params_default(C.byref(p))
    buf = np.zeros(12, "<f4")
    assert L.wfpt_denoise(None, C.byref(p), wf._p(buf), 3) == -1
    assert L.wfpt_denoise_to_device(None, C.byref(p), wf._p(buf), 12) == -1
    assert L.wfpt_read_variance(None, wf._p(buf), 1) == -1
    assert L.wfpt_denoise_timing_ms(None, None, None) == -1


@pytest.fixture(scope="module")
def kernel_metadata(tmp_path_factory):
    """wfpt_kernels.hip compiled for gfx950 to assembly (as tests/test_aov_host.py does): kernel name -> its metadata numbers."""
    from wavefront_path_tracer_amd import _build
    out = tmp_path_factory.mktemp("isa_denoise") / "wfpt_kernels.s"
    flags = [f for f in _build.FLAGS if f not in ("-shared", "-fPIC")]
    cmd = [_build.hipcc()] + flags + ["--offload-device-only", "-S", "-I" + os.path.join(ROOT, "include"), "-I" + _build.CSRC, "-o", str(out),
                                      os.path.join(_build.CSRC, "wfpt_kernels.hip")]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-3000:]
    asm = open(out).read()
    return {m.group(1): {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\n", m.group(2))}
            for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size:", asm, re.S)}


def test_denoise_kernels_run_without_scratch(kernel_metadata):
    for base in ("accumulate_moments_kernel", "denoise_prepare_kernel", "denoise_atrous_kernel"):
        hits = [n for n in kernel_metadata if base in n]
        assert len(hits) == 1, (base, sorted(kernel_metadata))
        md = kernel_metadata[hits[0]]
        assert md["private_segment_fixed_size"] == 0, (base, md)
        assert md.get("agpr_count", 0) == 0, (base, md)
        assert md["vgpr_count"] <= 128, (base, md)
    # accumulate_kernel is still there, untemplated, and no new kernel name contains it
    plain = [n for n in kernel_metadata if "accumulate_kernel" in n]
    assert len(plain) == 1 and "17accumulate_kernelE" in plain[0] and not plain[0].split("17accumulate_kernelE")[1].startswith("I"), plain
    assert not [n for n in kernel_metadata if re.search(r"aov_kernel|aov_resolve_kernel", n) and "denoise" in n]


# ---- the numpy restatement on synthetic inputs
def flat_guides(h, w):
    albedo = np.full((h, w, 3), 0.5, F)
    normal = np.zeros((h, w, 3), F)
    normal[..., 2] = 1.0
    depth = np.full((h, w), 3.0, F)
    return albedo, normal, depth


def test_reference_constant_image_is_a_fixed_point():
    h, w = 24, 40
    rng = np.random.default_rng(1)
    c = np.full((h, w, 3), [0.3, 0.6, 0.9], F)
    albedo = rng.random((h, w, 3), F)
    normal = rng.standard_normal((h, w, 3)).astype(F)
    depth = (1.0 + rng.random((h, w))).astype(F)
    var = np.full((h, w), 0.01, F)
    for n in (1, 16):
        out = R.denoise(c, albedo, normal, depth, var, n)
        np.testing.assert_allclose(out, c, rtol=2e-6, atol=0)


def test_reference_zero_iterations_is_the_identity():
    h, w = 16, 20
    rng = np.random.default_rng(2)
    c = rng.random((h, w, 3), F)
    albedo, normal, depth = flat_guides(h, w)
    out = R.denoise(c, albedo, normal, depth, np.zeros((h, w), F), 8, iterations=0)
    assert np.array_equal(out.view(np.uint32), c.view(np.uint32))


def test_reference_removes_white_noise_on_flat_guides():
    h, w, n = 64, 64, 8
    rng = np.random.default_rng(3)
    noise = F(0.2) * rng.standard_normal((h, w)).astype(F)
    c = np.repeat((F(0.5) + noise)[..., None], 3, axis=2).astype(F)
    albedo, normal, depth = flat_guides(h, w)
    L = R.luma(c)
    var = np.full((h, w), np.var(L), F)  # the variance of the mean: the noise left in c
    out = R.denoise(c, albedo, normal, depth, var, n)
    before, after = np.var(L), np.var(R.luma(out))
    assert after < 0.05 * before, (before, after)
    assert abs(float(out.mean()) - float(c.mean())) < 0.01


@pytest.mark.parametrize("edge", ["albedo", "normal"])
def test_reference_does_not_bleed_across_an_edge(edge):
    """Two halves of different colour separated by an albedo or a normal step: each half stays its own colour."""
    h, w = 32, 64
    rng = np.random.default_rng(4)
    c = np.zeros((h, w, 3), F)
    c[:, : w // 2] = [0.9, 0.1, 0.1]
    c[:, w // 2:] = [0.1, 0.1, 0.9]
    c += F(0.05) * rng.standard_normal((h, w, 3)).astype(F)
    albedo, normal, depth = flat_guides(h, w)
    if edge == "albedo":
        albedo[:, : w // 2] = [0.8, 0.2, 0.2]
        albedo[:, w // 2:] = [0.2, 0.2, 0.8]
    else:
        normal[:, w // 2:] = [1.0, 0.0, 0.0]
    var = np.full((h, w), 0.05, F)
    out = R.denoise(c, albedo, normal, depth, var, 16)
    left, right = out[:, : w // 2], out[:, w // 2:]
    assert left[..., 2].max() < 0.35 and left[..., 0].min() > 0.65, (left[..., 2].max(), left[..., 0].min())
    assert right[..., 0].max() < 0.35 and right[..., 2].min() > 0.65, (right[..., 0].max(), right[..., 2].min())
    # and the noise inside each half is smoothed
    assert np.std(left[..., 0]) < 0.5 * np.std(c[:, : w // 2, 0])


def test_reference_short_history_uses_the_spatial_variance():
    h, w = 12, 10
    rng = np.random.default_rng(5)
    c = rng.random((h, w, 3), F)
    albedo, normal, depth = flat_guides(h, w)
    var = np.full((h, w), 123.0, F)
    _, _, cv1 = R.prepare(c, albedo, normal, depth, var, 1)
    _, _, cv4 = R.prepare(c, albedo, normal, depth, var, 4)
    assert (cv4[..., 3] == F(123.0)).all()
    L = R.luma(c).astype(np.float64)
    want = L[0:4, 0:4].var()  # pixel (0, 0): its window clipped to rows 0..3, columns 0..3
    assert abs(float(cv1[0, 0, 3]) - want) < 1e-5 * max(want, 1.0)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="only meaningful on a box without a GPU")
def test_no_gpu_means_denoise_contexts_fail_loudly(wf):
    assert wf.device_count() == 0
    with pytest.raises(wf.WfptError):
        wf.shirley_path_tracer(64, 64, flags=wf.FLAG_DENOISE)
