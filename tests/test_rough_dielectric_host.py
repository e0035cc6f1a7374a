"""GGX rough dielectrics (WFPT_FLAG_ROUGH_DIELECTRIC, include/wfpt.h "Rough dielectrics") without a GPU: the numpy float32 restatement
(tests/rough_dielectric_ref.py) against a float64 quadrature over the microfacet normals, four mutations the same comparison must reject,
the bounds of the weight, the accuracy of the pseudo-normal that turns a refraction into a reflection, the smooth limit, the flag's place
in wfpt_create's rules on device -1, and the argument checks that need no device."""
import ctypes as C
import json

import numpy as np
import pytest

import rough_dielectric_ref as RD
import shading_normals_ref as S
from test_create_flag_rules_host import DIGITS, FIXTURE, FLAGS
from test_microfacet_host import ALPHAS, COSINES, create_message

F = np.float32
IOR = 1.5
SIDES = ("outside", "inside")  # eta = 1 / 1.5 and eta = 1.5
DRAWS = 1 << 16
GRID = (1200, 2400)
CRITICAL = float(np.sqrt(1.0 - 1.0 / (IOR * IOR)))  # from inside, a macro-normal cosine below this is beyond the critical angle
# reflect(uv, h) against the float64 evaluation of steps 10-11: 4 x the worst deviation test_the_pseudo_normal_reproduces_the_direction
# measures (its docstring)
REFLECT_BOUND = 4 * 1.36e-5


# ---------------------------------------------------------------- the estimator against the quadrature
_cells = {}


def cell(alpha, cn, side):
    """(the rows at albedo 1, the quadrature on GRID, its move when the grid is halved), once per cell"""
    key = (alpha, cn, side)
    if key not in _cells:
        eta = IOR if side == "inside" else 1.0 / IOR
        rows = RD.cell_rows(alpha, cn, side == "inside", DRAWS, seed=1, ior=IOR)
        fine = RD.directional_albedo_rt(alpha, cn, eta, *GRID)
        coarse = RD.directional_albedo_rt(alpha, cn, eta, GRID[0] // 2, GRID[1] // 2)
        _cells[key] = (rows, fine, abs(fine - coarse))
    return _cells[key]


def deviation(weight, want):
    """(mean - want) in standard errors of the mean, and that standard error (of these draws)"""
    w = np.asarray(weight, np.float64)
    se = w.std(ddof=1) / np.sqrt(len(w))
    return (w.mean() - want) / se, se


def all_cells():
    return [(a, c, s) for s in SIDES for a in ALPHAS for c in COSINES]


def worst(stop=np.inf, **mutations):
    """the largest |z| over the cells; the walk ends at the first cell beyond `stop`"""
    out = 0.0
    for key in all_cells():
        rows, want, _ = cell(*key)
        w = RD.sample_rows(rows, **mutations)[:, 4]
        z, _ = deviation(np.nan_to_num(w, nan=1e3), want)
        out = max(out, abs(float(z)))
        if out > stop:
            break
    return out


def test_a_cell_lies_beyond_the_critical_angle():
    assert sum(1 for c in COSINES if c < CRITICAL) >= 1, (COSINES, CRITICAL)


@pytest.mark.parametrize("cn", COSINES)
@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("side", SIDES)
def test_the_mean_weight_is_the_quadrature(side, alpha, cn):
    rows, want, moved = cell(alpha, cn, side)
    out = RD.sample_rows(rows)
    assert not (out[:, 3] == 2).any(), "a draw of the cell fell back"
    z, se = deviation(out[:, 4], want)
    live = out[:, 3] == 0
    print(f"{side} alpha {alpha} cn {cn}: mean {out[:, 4].astype(np.float64).mean():.6f} quadrature {want:.6f} z {z:+.2f} "
          f"refracted {float((out[live, 7] == 1).mean()):.3f} dead {float((~live).mean()):.3f}")
    assert moved < se / 5, f"halving the quadrature's grid moves it by {moved}, a fifth of the standard error is {se / 5}"
    assert abs(z) < 4, (side, alpha, cn, z)


def test_the_worst_cell():
    z = worst()
    print("the worst of the", len(all_cells()), "cells lies", z, "standard errors from the quadrature")
    assert z < 4


@pytest.mark.parametrize("mutation", sorted(RD.MUTATIONS))
def test_the_comparison_rejects_a_mutated_restatement(mutation):
    z = worst(stop=4, **{mutation: True})
    print(mutation, ": a cell lies", z, "standard errors from the quadrature")
    assert z > 4, (mutation, z)


# ---------------------------------------------------------------- the weight's bounds
def random_rows(k, seed, alpha=None, ior=None):
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((k, 3)) * rng.uniform(0.2, 3.0, (k, 1))
    n = rng.standard_normal((k, 3))
    n /= np.linalg.norm(n, axis=1)[:, None]
    a = rng.uniform(0.0, 1.0, k) if alpha is None else np.full(k, alpha)
    i = rng.uniform(1.2, 2.5, k) if ior is None else np.full(k, ior)
    return RD.probe_rows(d, n, rng.random(k, dtype=F), rng.random(k, dtype=F), rng.random(k, dtype=F), a, i, rng.uniform(0.0, 1.0, (k, 3)))


def test_no_weight_leaves_zero_to_albedo():
    rows = random_rows(1 << 16, 2)
    rows[: 1 << 12, 11:14] = np.random.default_rng(3).integers(0, 2, (1 << 12, 3))  # albedo channels of exactly 0 and 1
    out = RD.sample_rows(rows)
    w = out[:, 4:7]
    assert (w >= 0).all() and (w <= rows[:, 11:14]).all(), (float(w.min()), float((w - rows[:, 11:14]).max()))
    dead = out[:, 3] == 1
    assert 0 < dead.sum() < len(rows)
    assert (w[dead].view(np.uint32) == 0).all(), "a dead path's weight is not +0"
    assert not (out[:, 3] == 2).any()


# ---------------------------------------------------------------- the pseudo-normal
def test_the_pseudo_normal_reproduces_the_direction():
    """reflect(uv, h) in f32 -- what the metal branch of scatter() emits for a unit d -- against steps 10-11 evaluated in float64 from the
    same f32 uv, m and eta, over 4096 random rows with ior in [1.2, 2.5]. Measured worst deviation (largest component, rows that did not
    fall back): 1.75e-7 in the reflect arm, 1.36e-5 in the refract arm (step 11's own sqrt(k) in f32 near k = 0, a refraction that grazes the
    microfacet, not the pseudo-normal); REFLECT_BOUND is 4 x 1.36e-5. Rows with |w - uv|^2 < 1e-6 (a
    refraction that hardly bends: the normalisation of w - uv loses its digits there) are left out and counted: under 1 % of the rows."""
    rows = random_rows(4096, 11)
    r = RD.sample_row_parts(rows)
    want = RD.outgoing_f64(r["uv"], r["m"], r["eta"], r["refracted"])
    got = RD.reflect_about(r["uv"], r["h"]).astype(np.float64)
    bend = ((want - r["uv"].astype(np.float64)) ** 2).sum(axis=1)
    live = ~r["fell"] & np.isfinite(want).all(axis=1)
    live &= np.einsum("ij,ij->i", -r["uv"].astype(np.float64), r["m"].astype(np.float64)) > 0  # (step 10's dead rows have no direction)
    flat = live & (bend < 1e-6)
    print("left out:", int(flat.sum()), "of", len(rows))
    assert flat.sum() < len(rows) // 100
    keep = live & ~flat
    assert keep.sum() > 3000 and (keep & r["refracted"]).sum() > 500 and (keep & ~r["refracted"]).sum() > 200
    err = np.abs(got - want).max(axis=1)
    for name, arm in (("reflect", ~r["refracted"]), ("refract", r["refracted"])):
        print(name, "arm: worst deviation", float(err[keep & arm].max()))
    assert err[keep].max() < REFLECT_BOUND, float(err[keep].max())


# ---------------------------------------------------------------- the smooth limit
@pytest.mark.parametrize("side", SIDES)
def test_the_smooth_limit(side):
    """alpha = 1e-4 at the macro cosine 0.8 (inside the critical angle from either side): the reflected share is schlick(cn, eta) within 4
    binomial standard errors, and the mean outgoing direction of either arm is scatter()'s smooth one within REFLECT_BOUND + alpha."""
    alpha, cn = 1e-4, 0.8
    eta = IOR if side == "inside" else 1.0 / IOR
    rows = RD.cell_rows(alpha, cn, side == "inside", DRAWS, seed=5, ior=IOR)
    r = RD.sample_row_parts(rows)
    assert not r["fell"].any() and r["dead"].mean() < 0.01
    r0 = ((1.0 - eta) / (1.0 + eta)) ** 2
    p = r0 + (1.0 - r0) * (1.0 - cn) ** 5
    share = float((~r["refracted"] & ~r["dead"]).sum()) / float((~r["dead"]).sum())
    se = np.sqrt(p * (1.0 - p) / DRAWS)
    print(f"{side}: reflected share {share:.5f} schlick {p:.5f} z {(share - p) / se:+.2f}")
    assert abs(share - p) < 4 * se
    out = RD.reflect_about(r["uv"], r["h"]).astype(np.float64)
    one = np.ones(1, F)
    for name, arm, u in (("reflect", ~r["refracted"], 0.0), ("refract", r["refracted"], 1.0)):
        smooth = S.scatter(rows[:1, 3:6], r["uv"][:1], [2], 0 * one, IOR * one, np.zeros((1, 3), F), u * one)[0].astype(np.float64)
        mean = out[arm & ~r["dead"]].mean(axis=0)
        print(f"{side} {name}: mean direction {mean} smooth {smooth}")
        assert np.abs(mean - smooth).max() < REFLECT_BOUND + alpha, (name, mean, smooth)


# ---------------------------------------------------------------- the flag in wfpt_create's rules, on device -1
def test_the_flag_needs_microfacet_and_goes_with_each_other_flag():
    """on device -1 an accepted combination ends at "no HIP device". Each other flag comes with the flags its own rule needs."""
    import wavefront_path_tracer_amd as W
    assert W.FLAG_ROUGH_DIELECTRIC == 1 << 26
    assert create_message(W, W.FLAG_ROUGH_DIELECTRIC, W.RNG_DISPATCH).startswith("wfpt_create: WFPT_FLAG_ROUGH_DIELECTRIC needs")
    both = W.FLAG_MICROFACET | W.FLAG_ROUGH_DIELECTRIC
    assert "no HIP device" in create_message(W, both, W.RNG_DISPATCH)
    connect = W.FLAG_EMISSION | W.FLAG_NEE
    needs = {"NEE": W.FLAG_EMISSION, "MIS": connect, "LIGHT_POWER": connect, "ANALYTIC_LIGHTS": connect,
             "ENV_NEE": connect | W.FLAG_ENVIRONMENT, "ENV_MIS": connect | W.FLAG_ENVIRONMENT | W.FLAG_ENV_NEE}
    others = ["SPLIT_SHADE", "NO_GRAPH", "UNFUSED", "BINARY_BVH", "NO_REFILL", "NO_LDS_SCENE", "EXACT_TRAVERSAL", "NO_BINNING", "BINNING", "AOV",
              "DENOISE", "ENVIRONMENT", "TEXTURES", "EMISSION", "NEE", "ENV_NEE", "MIS", "ENV_MIS", "NO_TILE_LISTS", "RETIRE", "ADAPTIVE",
              "LIGHT_POWER", "ANALYTIC_LIGHTS", "SHADING_NORMALS"]
    for name in others:
        flags = both | getattr(W, "FLAG_" + name) | needs.get(name, 0)
        msg = create_message(W, flags, W.RNG_PIXEL)
        assert "no HIP device" in msg, (name, msg)
        assert msg == create_message(W, flags & ~both, W.RNG_PIXEL), name
        assert create_message(W, flags & ~W.FLAG_MICROFACET, W.RNG_PIXEL).startswith("wfpt_create: WFPT_FLAG_ROUGH_DIELECTRIC needs"), name


def test_the_flag_changes_no_recorded_rule():
    """every recorded combination of the fourteen flags of the rules answers the same with the two flags added"""
    import wavefront_path_tracer_amd as W
    fx = json.load(open(FIXTURE))
    bit = [getattr(W, "FLAG_" + name) for name in FLAGS]
    for mode in (W.RNG_DISPATCH, W.RNG_PIXEL):
        for case in range(0, 1 << len(FLAGS)):
            flags = sum(b for k, b in enumerate(bit) if case >> k & 1) | W.FLAG_MICROFACET | W.FLAG_ROUGH_DIELECTRIC
            want = fx["messages"][DIGITS.index(fx["cases"][mode][case])]
            got = create_message(W, flags, mode)
            assert got == want, (mode, case, got, want)


# ---------------------------------------------------------------- argument checks that need no device
def test_the_entry_point_refuses_a_null_context():
    import wavefront_path_tracer_amd as W
    L = W.lib()
    rows, out = np.zeros((1, 16), F), np.full((1, 8), 7.0, F)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.wfpt_sample_rough_dielectric(None, ptr(rows), 1, ptr(out)) == W.ERR_INVALID_ARGUMENT
    assert L.wfpt_last_error(None).decode() == "wfpt_sample_rough_dielectric: null context"
    assert (out == 7.0).all(), "a refused call wrote its output"


def test_the_python_wrapper_checks_its_rows_before_the_library():
    import wavefront_path_tracer_amd as W
    pt = W.PathTracer.__new__(W.PathTracer)  # no context: the check below comes before any call into the library
    pt.handle = None
    with pytest.raises(ValueError):
        pt.sample_rough_dielectric(np.zeros((3, 12), F))
    with pytest.raises(ValueError):
        pt.sample_rough_dielectric(np.zeros(16, F))
