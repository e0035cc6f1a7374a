"""Environment map (WFPT_FLAG_ENVIRONMENT) without a GPU: the numpy restatement's own properties (tests/environment_ref.py), the .pfm / .hdr
readers, the parameter struct's layout and the registers of every environment kernel variant (hipcc cross-compiles)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import environment_ref as R

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ulps(got, want):
    want = np.asarray(want, np.float64)
    return np.abs(np.asarray(got, np.float64) - want) / np.spacing(np.abs(want).astype(F)).astype(np.float64)


def test_atan2_within_two_ulp():
    rng = np.random.default_rng(1)
    y, x = rng.standard_normal(400000).astype(F), rng.standard_normal(400000).astype(F)
    y[:1000] *= F(1e-4)
    x[1000:2000] *= F(1e-4)
    x[2000:3000] = y[2000:3000]  # |y| == |x|
    assert ulps(R.atan2_(y, x), np.arctan2(y.astype(np.float64), x.astype(np.float64))).max() <= 2.0


def test_atan2_signed_zeros_and_axes():
    y = F([0, -0.0, 0, -0.0, 0, 1, -1, 2, -2])
    x = F([0, 0, -1, -1, 1, 0, -0.0, 0, 0])
    got = R.atan2_(y, x)
    want = F([0, 0, np.pi, np.pi, 0, np.pi / 2, -np.pi / 2, np.pi / 2, -np.pi / 2])
    assert np.array_equal(got, want), got


def test_seam_is_continuous_and_poles_are_single_points():
    h, w = 16, 64
    m = np.random.default_rng(2).random((h, w, 3)).astype(F)
    eps = F(1e-6)
    left = R.env_lookup(m, np.array([[-eps, 0.3, 1.0]], F))  # just either side of +z, where u wraps from 1 to 0
    right = R.env_lookup(m, np.array([[eps, 0.3, 1.0]], F))
    assert np.abs(left - right).max() < 1e-4
    u, _ = R.env_uv(np.array([[-eps, 0.3, 1.0], [eps, 0.3, 1.0]], F))
    assert min(u) < 0.01 and max(u) > 0.99  # the two sides of the seam
    for dy in (1.0, -1.0):  # a pole: every azimuth nearby gives (nearly) the same row blend
        a = np.linspace(0, 2 * np.pi, 50, endpoint=False)
        d = np.stack([np.cos(a) * 1e-7, np.full_like(a, dy), np.sin(a) * 1e-7], axis=1).astype(F)
        _, v = R.env_uv(d)
        assert np.all(v == v[0]) and abs(float(v[0]) - (0.0 if dy > 0 else 1.0)) < 1e-6
        c = R.env_lookup(m, d)
        row = 0 if dy > 0 else h - 1  # clamped rows: the lookup is a blend along the edge row only
        assert np.all(c >= m[row].min(axis=0) - 1e-6) and np.all(c <= m[row].max(axis=0) + 1e-6)


def test_constant_map_within_two_ulp():
    """The four weights of the fixed bilinear form are rounded products and their weighted sum rounds three times: 2 ulp at most (1 ulp is
    not reachable with the operation order the device pins)."""
    d = np.random.default_rng(3).standard_normal((100000, 3)).astype(F)
    for value in (F(1.0), F(0.37), F(1234.5)):
        m = np.full((8, 16, 3), value, F)
        assert ulps(R.env_lookup(m, d), np.full((len(d), 3), value, np.float64)).max() <= 2.0


def test_sky_restatement_equals_the_oracle():
    """render_with_environment without a map drives the oracle's stages into its own render: the driver itself is right."""
    from oracle import oracle as O
    want = O.shirley_oracle(40, 24, max_wavefronts=6).render(2)
    got = R.render_with_environment(O.shirley_oracle(40, 24, max_wavefronts=6), None, spp=2)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---------------------------------------------------------------- readers
def write_pfm(path, img, little=True):
    h, w, _ = img.shape
    with open(path, "wb") as f:
        f.write(f"PF\n{w} {h}\n{-1.0 if little else 1.0}\n".encode())
        f.write(np.ascontiguousarray(img[::-1], "<f4" if little else ">f4").tobytes())


def to_rgbe(img):
    m = img.max(axis=2)
    e = np.zeros(m.shape, np.int32)
    mant, ex = np.frexp(m)
    ok = m > 1e-32
    e[ok] = ex[ok]
    scale = np.where(ok, 256.0 / np.ldexp(1.0, e), 0.0)
    rgb = np.floor(img * scale[..., None]).clip(0, 255).astype(np.uint8)
    return np.concatenate([rgb, np.where(ok, e + 128, 0).astype(np.uint8)[..., None]], axis=2)


def from_rgbe(rgbe):
    e = rgbe[..., 3].astype(np.int32)
    return (rgbe[..., :3] * np.where(e > 0, np.ldexp(1.0, e - 136), 0.0)[..., None]).astype(F)


def rle_channel(vals):
    """New-style RLE of one channel of a scanline: runs of >= 3 equal bytes as (128 + n, v), the rest as literals."""
    out, i, n = bytearray(), 0, len(vals)
    while i < n:
        j = i
        while j < n and j - i < 127 and vals[j] == vals[i]:
            j += 1
        if j - i >= 3:
            out += bytes([128 + j - i, vals[i]])
            i = j
            continue
        k = i
        while k < n and k - i < 128 and not (k + 2 < n and vals[k] == vals[k + 1] == vals[k + 2]):
            k += 1
        k = max(k, i + 1)
        out += bytes([k - i]) + bytes(vals[i:k])
        i = k
    return bytes(out)


def write_hdr(path, rgbe, rle_rows=()):
    h, w, _ = rgbe.shape
    with open(path, "wb") as f:
        f.write(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n" + f"-Y {h} +X {w}\n".encode())
        for y in range(h):
            if y in rle_rows:
                f.write(bytes([2, 2, w >> 8, w & 255]))
                for ch in range(4):
                    f.write(rle_channel(rgbe[y, :, ch].tolist()))
            else:
                f.write(rgbe[y].tobytes())


@pytest.mark.parametrize("little", [True, False])
def test_pfm_round_trip(tmp_path, little):
    import wavefront_path_tracer_amd as W
    img = np.random.default_rng(4).random((5, 7, 3)).astype(F) * F(10)
    p = tmp_path / "m.pfm"
    write_pfm(p, img, little)
    got = W.load_environment(str(p))
    assert got.dtype == np.float32 and np.array_equal(got, img)


def test_hdr_round_trip_flat_and_rle(tmp_path):
    import wavefront_path_tracer_amd as W
    h, w = 6, 40
    img = np.random.default_rng(5).random((h, w, 3)) * 50
    img[2, 5:30] = 3.0  # a long run for the RLE rows
    img[4] = 0.0
    rgbe = to_rgbe(img)
    p = tmp_path / "m.hdr"
    write_hdr(p, rgbe, rle_rows=(1, 2, 4))
    got = W.load_environment(str(p))
    assert got.shape == (h, w, 3) and np.array_equal(got, from_rgbe(rgbe))
    assert np.abs(got - img).max() <= img.max() / 128  # RGBE keeps 8 bits of mantissa


# ---------------------------------------------------------------- ABI and kernels
def test_environment_params_layout():
    import wavefront_path_tracer_amd as W
    P = W._EnvironmentParams
    assert C.sizeof(P) == 32 and P.rotation.offset == 4 and P._reserved.offset == 8
    hdr = open(os.path.join(ROOT, "include", "wfpt.h")).read()
    assert "WFPT_FLAG_ENVIRONMENT = 1u << 12" in hdr and W.FLAG_ENVIRONMENT == 1 << 12
    assert "sizeof(wfpt_environment_params) == 32" in hdr


@pytest.fixture(scope="module")
def device_asm(tmp_path_factory):
    from wavefront_path_tracer_amd import _build
    out = tmp_path_factory.mktemp("isa_env") / "wfpt_kernels.s"
    flags = [f for f in _build.FLAGS if f not in ("-shared", "-fPIC")]
    cmd = [_build.hipcc()] + flags + ["--offload-device-only", "-S", "-I" + os.path.join(ROOT, "include"), "-I" + _build.CSRC, "-o", str(out),
                                      os.path.join(_build.CSRC, "wfpt_kernels.hip")]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-3000:]
    return open(out).read()


def kernels(asm):
    return {m.group(1): {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\n", m.group(2))}
            for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size:", asm, re.S)}


def test_environment_variants_meet_their_twins_budgets(device_asm):
    """Every environment instantiation (a trailing `true` template argument, or a kernel of its own) keeps the budgets of its flag-off twin:
    <= 64 vector and <= 80 scalar registers, no AGPRs, and no more scratch than the twin (the launches that run by default: none)."""
    md = kernels(device_asm)
    env = {n: m for n, m in md.items() if re.search(r"(bounce|extend)_kernelI.*ELb1EEEv|compact_kernelILb1E|miss_env_kernel", n)}
    assert len(env) >= 25 + 24 + 1 + 1, sorted(env)
    for name, m in env.items():
        twin = name.replace("ELb1EEEv", "ELb0EEEv").replace("compact_kernelILb1E", "compact_kernelILb0E")
        if "miss_env_kernel" in name:
            twin = next(k for k in md if k.endswith("miss_kernelENS_8MissArgsE"))
        t = md[twin]
        assert m["vgpr_count"] <= max(64, t["vgpr_count"]) and m["sgpr_count"] <= max(80, t["sgpr_count"]), (name, m)
        assert m.get("agpr_count", 0) == 0, (name, m)
    for frag, scratch in [("bounce_kernelILi1EjLi0ELb1ELb0ELb1E", 0), ("bounce_kernelILi0EjLi0ELb1ELb0ELb1E", 24),
                          ("bounce_kernelILi2EjLi0ELb0ELb0ELb1E", 0), ("extend_kernelILb0EjLi0ELb1ELb0ELb1E", 0),
                          ("compact_kernelILb1E", 0), ("miss_env_kernel", 0)]:
        m = next(v for k, v in md.items() if frag in k)
        assert m["vgpr_count"] <= 64 and m["sgpr_count"] <= 80 and m["private_segment_fixed_size"] <= scratch, (frag, m)
