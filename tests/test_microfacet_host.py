"""GGX microfacet metals (WFPT_FLAG_MICROFACET, include/wfpt.h "Microfacet metals") without a GPU: the numpy float32 restatement
(tests/microfacet_ref.py) against a float64 quadrature of the directional albedo, three mutations the same comparison must reject, the
energy bound and the flat limit of the weight, the flag's place in wfpt_create's rules on device -1, and the argument checks of the entry
points that need no device."""
import ctypes as C
import json

import numpy as np
import pytest

import microfacet_ref as MF
from test_create_flag_rules_host import DIGITS, FIXTURE, FLAGS

F = np.float32
ALPHAS, COSINES, F0 = (0.1, 0.3, 0.6, 1.0), (0.95, 0.5, 0.15), (0.8, 0.5, 1.0)
DRAWS = 1 << 16
GRID = (1500, 3000)


# ---------------------------------------------------------------- the estimator against the quadrature
_cells = {}


def cell(alpha, cn):
    """(the rows, the quadrature on GRID, its move when the grid is halved), once per cell"""
    key = (alpha, cn)
    if key not in _cells:
        rows = MF.cell_rows(alpha, cn, F0, DRAWS, seed=1)
        fine = MF.directional_albedo(alpha, cn, F0, *GRID)
        coarse = MF.directional_albedo(alpha, cn, F0, GRID[0] // 2, GRID[1] // 2)
        _cells[key] = (rows, fine, np.abs(fine - coarse))
    return _cells[key]


def deviation(weight, want):
    """(mean - want) in standard errors of the mean, per channel; the standard error is that of these draws"""
    w = weight.astype(np.float64)
    se = w.std(axis=0, ddof=1) / np.sqrt(len(w))
    return (w.mean(axis=0) - want) / se, se


def worst(**mutations):
    out = 0.0
    for alpha in ALPHAS:
        for cn in COSINES:
            rows, want, _ = cell(alpha, cn)
            z, _ = deviation(MF.sample_rows(rows, **mutations)[:, 4:7], want)
            out = max(out, float(np.abs(z).max()))
    return out


@pytest.mark.parametrize("cn", COSINES)
@pytest.mark.parametrize("alpha", ALPHAS)
def test_the_mean_weight_is_the_directional_albedo(alpha, cn):
    rows, want, moved = cell(alpha, cn)
    out = MF.sample_rows(rows)
    assert not (out[:, 3] == 2).any(), "a draw of the cell fell back"
    z, se = deviation(out[:, 4:7], want)
    below = float((out[:, 3] == 1).mean())
    print(f"alpha {alpha} cn {cn}: mean {out[:, 4:7].astype(np.float64).mean(axis=0)} quadrature {want} z {z} below the horizon {below:.3f}")
    assert (moved < se / 4).all(), f"halving the quadrature's grid moves it by {moved}, a quarter of the standard error is {se / 4}"
    assert (np.abs(z) < 4).all(), (alpha, cn, z)


@pytest.mark.parametrize("mutation", sorted(MF.MUTATIONS))
def test_the_comparison_rejects_a_mutated_restatement(mutation):
    z = worst(**{mutation: True})
    print(mutation, ": the worst cell lies", z, "standard errors from the quadrature")
    assert z > 4, (mutation, z)


# ---------------------------------------------------------------- the weight's bounds
def random_rows(k, seed, alpha=None):
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((k, 3)) * rng.uniform(0.2, 3.0, (k, 1))
    n = rng.standard_normal((k, 3))
    n /= np.linalg.norm(n, axis=1)[:, None]
    a = rng.uniform(0.0, 1.0, k) if alpha is None else np.full(k, alpha)
    return MF.probe_rows(d, n, rng.random(k, dtype=F), rng.random(k, dtype=F), a, rng.uniform(0.0, 1.0, (k, 3)))


def test_no_weight_leaves_the_unit_interval():
    rows = random_rows(1 << 16, 2)
    rows[: 1 << 12, 9:12] = np.random.default_rng(3).integers(0, 2, (1 << 12, 3))  # F0 channels of exactly 0 and 1
    out = MF.sample_rows(rows)
    w = out[:, 4:7]
    assert (w >= 0).all() and (w <= 1).all(), (float(w.min()), float(w.max()))
    dead = out[:, 3] == 1
    assert 0 < dead.sum() < len(rows)
    assert (w[dead].view(np.uint32) == 0).all(), "a dead path's weight is not +0"


def test_the_flat_limit():
    """alpha = 1e-4: the weight is +0 or Schlick's term times a G <= 1, and m is the (two-sided) normal within 1e-3. GGX has a heavy tail
    at any alpha -- the tangent of the angle between m and nf is alpha times the tangent of the sampled hemisphere normal's polar angle,
    which step 6 makes sqrt(r2 / (1 - r2)) with r2 <= u1 about a vh that is the pole here -- so the rows keep u1 <= 0.98 (tangent <= 7,
    distance <= 7e-4) and cn >= 0.05 (vh.z >= 1 - 2e-6); the bits of the tail are the probe test's business."""
    rows = random_rows(1 << 14, 4, alpha=1e-4)
    rows[:, 6] *= F(0.98)
    d, n = rows[:, 0:3].astype(np.float64), rows[:, 3:6].astype(np.float64)
    cn = np.abs(np.einsum("ij,ij->i", n, d)) / np.linalg.norm(d, axis=1)
    rows = rows[cn >= 0.05]
    assert len(rows) > 1 << 13
    out = MF.sample_rows(rows)
    assert not (out[:, 3] == 2).any()
    r = MF.sample(rows[:, 0:3], rows[:, 3:6], rows[:, 6], rows[:, 7], rows[:, 8], rows[:, 9:12], no_G=True)
    live = out[:, 3] == 0
    assert live.sum() > len(rows) // 2
    f = F(1) - out[live, 7]
    fresnel = (rows[live, 9:12] + (F(1) - rows[live, 9:12]) * ((((f * f) * (f * f)) * f)[:, None])).astype(F)
    assert np.array_equal(fresnel.view(np.uint32), r["weight"][live].view(np.uint32)), "without G the weight is F0 + (1 - F0) f5"
    assert (out[live, 4:7] <= fresnel).all(), "the weight is Schlick's term times a G <= 1"
    assert (out[~live, 4:7].view(np.uint32) == 0).all()
    n = rows[:, 3:6].astype(np.float64)
    wi = -rows[:, 0:3].astype(np.float64)
    nf = np.where((np.einsum("ij,ij->i", n, wi) < 0)[:, None], -n, n)
    assert np.abs(out[:, 0:3] - nf).max() < 1e-3, "with alpha = 1e-4 the microfacet normal is the (two-sided) normal"


# ---------------------------------------------------------------- the flag in wfpt_create's rules, on device -1
def create_message(W, flags, rng_mode):
    L = W.lib()
    spheres, materials, nodes = np.zeros(1, W.SPHERE), np.zeros(1, W.MATERIAL), np.zeros(1, W.BVH_NODE)
    spheres["radius"] = 1.0
    nodes["aabb_min"], nodes["aabb_max"], nodes["prim_count"] = -1.0, 1.0, 1
    cam, mat = np.zeros(1, W.GPU_CAMERA), np.eye(4, dtype="<f4")
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    p = W._Params(16, 16, 0, 4, 0, rng_mode, flags, 0, 0, -1, 1)
    handle = L.wfpt_create(C.byref(p), ptr(spheres), 1, ptr(materials), 1, ptr(nodes), 1, ptr(cam), ptr(mat), ptr(mat))
    assert not handle, f"wfpt_create succeeded on device -1 (flags {flags:#x})"
    return L.wfpt_last_error(None).decode()


def test_the_flag_alone_and_with_each_other_flag_is_accepted():
    """on device -1 an accepted combination ends at "no HIP device". Each other flag comes with the flags its own rule needs; with
    WFPT_FLAG_BINNING the flag is accepted as WFPT_FLAG_TEXTURES is (the refusal comes with the first roughness), under WFPT_RNG_PIXEL."""
    import wavefront_path_tracer_amd as W
    assert W.FLAG_MICROFACET == 1 << 25
    assert "no HIP device" in create_message(W, W.FLAG_MICROFACET, W.RNG_DISPATCH)
    connect = W.FLAG_EMISSION | W.FLAG_NEE
    needs = {"NEE": W.FLAG_EMISSION, "MIS": connect, "LIGHT_POWER": connect, "ANALYTIC_LIGHTS": connect,
             "ENV_NEE": connect | W.FLAG_ENVIRONMENT, "ENV_MIS": connect | W.FLAG_ENVIRONMENT | W.FLAG_ENV_NEE}
    others = ["SPLIT_SHADE", "NO_GRAPH", "UNFUSED", "BINARY_BVH", "NO_REFILL", "NO_LDS_SCENE", "EXACT_TRAVERSAL", "NO_BINNING", "BINNING", "AOV",
              "DENOISE", "ENVIRONMENT", "TEXTURES", "EMISSION", "NEE", "ENV_NEE", "MIS", "ENV_MIS", "NO_TILE_LISTS", "RETIRE", "ADAPTIVE",
              "LIGHT_POWER", "ANALYTIC_LIGHTS", "SHADING_NORMALS"]
    for name in others:
        flags = W.FLAG_MICROFACET | getattr(W, "FLAG_" + name) | needs.get(name, 0)
        msg = create_message(W, flags, W.RNG_PIXEL)
        assert "no HIP device" in msg, (name, msg)
        assert msg == create_message(W, flags & ~W.FLAG_MICROFACET, W.RNG_PIXEL), name
    binned = W.FLAG_BINNING | W.FLAG_MICROFACET
    assert create_message(W, binned, W.RNG_DISPATCH) == create_message(W, W.FLAG_BINNING | W.FLAG_TEXTURES, W.RNG_DISPATCH)
    assert "WFPT_FLAG_BINNING needs WFPT_RNG_PIXEL" in create_message(W, binned, W.RNG_DISPATCH)


def test_the_flag_changes_no_recorded_rule():
    """every recorded combination of the fourteen flags of the rules answers the same with WFPT_FLAG_MICROFACET added"""
    import wavefront_path_tracer_amd as W
    fx = json.load(open(FIXTURE))
    bit = [getattr(W, "FLAG_" + name) for name in FLAGS]
    for mode in (W.RNG_DISPATCH, W.RNG_PIXEL):
        for case in range(0, 1 << len(FLAGS)):
            flags = sum(b for k, b in enumerate(bit) if case >> k & 1) | W.FLAG_MICROFACET
            want = fx["messages"][DIGITS.index(fx["cases"][mode][case])]
            got = create_message(W, flags, mode)
            assert got == want, (mode, case, got, want)


# ---------------------------------------------------------------- argument checks that need no device
def test_entry_points_refuse_a_null_context():
    import wavefront_path_tracer_amd as W
    L = W.lib()
    alpha, ms, n = C.c_float(7.0), C.c_float(7.0), C.c_uint32(7)
    rows, out = np.zeros((1, 12), F), np.zeros((1, 8), F)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    calls = {"wfpt_set_roughness": lambda: L.wfpt_set_roughness(None, 0, 0.5),
             "wfpt_get_roughness": lambda: L.wfpt_get_roughness(None, 0, C.byref(alpha)),
             "wfpt_clear_roughness": lambda: L.wfpt_clear_roughness(None),
             "wfpt_sample_microfacet": lambda: L.wfpt_sample_microfacet(None, ptr(rows), 1, ptr(out)),
             "wfpt_microfacet_timing_ms": lambda: L.wfpt_microfacet_timing_ms(None, C.byref(ms), C.byref(n))}
    for name, call in calls.items():
        assert call() == W.ERR_INVALID_ARGUMENT, name
        assert L.wfpt_last_error(None).decode() == f"{name}: null context"
    assert (alpha.value, ms.value, n.value) == (7.0, 7.0, 7), "a refused call wrote its outputs"


def test_python_wrappers_check_their_arguments_before_the_library():
    import wavefront_path_tracer_amd as W
    pt = W.PathTracer.__new__(W.PathTracer)  # no context: the checks below come before any call into the library
    pt.handle = None
    with pytest.raises(ValueError):
        pt.set_roughness(-1, 0.5)
    with pytest.raises(ValueError):
        pt.get_roughness(1.5)
    with pytest.raises(ValueError):
        pt.sample_microfacet(np.zeros((3, 8), F))
