"""Light selection by power (WFPT_FLAG_LIGHT_POWER, include/wfpt.h "Light selection by power") without a GPU: the restatement's tables
against values worked out by hand, the edges of the selection, the one-light identity with nee_ref.Lights, and the estimator's
unbiasedness with the mutation that must fail (the selection by power with the weight left at nf)."""
import numpy as np
import pytest

import emission_ref as E
import light_power_ref as P
import nee_ref as N

F = np.float32
PI = F(3.1415927)


def spheres_em(orc, radii, colours):
    """sphere i (material i) of radius radii[i] at (3 i, 0, 0), emitting colours[i]"""
    n = len(radii)
    sp = np.zeros(n, orc.SPHERE)
    mt = np.zeros(n, orc.MATERIAL)
    sp["center"][:, 0] = 3.0 * np.arange(n)
    sp["center"][:, 3] = 1.0
    sp["radius"] = radii
    sp["material_idx"] = np.arange(n)
    return E.Emission({i: c for i, c in enumerate(colours)}, spheres=sp, materials=mt)


def luma_by_hand(r, g, b):
    return (F(0.2126) * F(r) + F(0.7152) * F(g)) + F(0.0722) * F(b)


# ---------------------------------------------------------------- the tables
def test_three_spheres_by_hand(orc):
    """f = L * (4 pi) * (ra ra): radius 2 white -> 16 pi L(1,1,1), the maximum; radius 1 pure red at 2 -> 4 pi * 0.4252, a quotient of
    0.4252 / 4 = 0.1063 -> ceil(6966.37) = 6967; radius 0.5 (0, 1, 4) -> pi * 1.004, a quotient of 1.004 / 16 = 0.06275 ->
    ceil(4112.3) = 4113."""
    lights = P.PowerLights(spheres_em(orc, [2.0, 1.0, 0.5], [(1, 1, 1), (2, 0, 0), (0, 1, 4)]))
    assert lights.has_distribution and lights.n == 3
    # the same figures from scalar f32 operations, one at a time
    f = [luma_by_hand(*c) * ((F(4) * PI) * (F(r) * F(r))) for r, c in ((2.0, (1, 1, 1)), (1.0, (2, 0, 0)), (0.5, (0, 1, 4)))]
    m = max(f)
    k = [int(np.ceil((x / m) * F(65535.0))) for x in f]
    assert k == [65535, 6967, 4113]
    assert lights.k.tolist() == k and lights.k.dtype == np.uint32
    assert lights.cdf.tolist() == [65535, 72502, 76615] and lights.cdf.dtype == np.uint64
    assert lights.total == 76615
    assert lights.prim_k.tolist() == k  # every primitive is a light here


def test_a_quotient_that_underflows_gets_weight_one_and_a_dark_primitive_none(orc):
    """radius 1e5 at colour 1e5: f about 1.26e16; radius 1e-17 at colour 1: f about 1.26e-33; the quotient, 1e-49, is below the smallest
    f32 and becomes 0: k = 1. The third sphere does not emit: it is no light, and its prim_k is 0."""
    em = spheres_em(orc, [1e5, 1e-17, 1.0], [(1e5, 1e5, 1e5), (1, 1, 1), (0, 0, 0)])
    lights = P.PowerLights(em)
    assert lights.list.tolist() == [0, 1]
    f = lights.weights()
    assert f[1] > 0 and (f[1] / f[0]) == 0
    assert lights.k.tolist() == [65535, 1]
    assert lights.cdf.tolist() == [65535, 65536] and lights.total == 65536
    assert lights.prim_k.tolist() == [65535, 1, 0]


def test_two_triangles_one_of_no_area(orc):
    """e1 = (1, 0, 0), e2 = (0, 1, 0): cr = (0, 0, 1), A = 0.5; e2 = 2 e1: cr = 0, A = 0, f > 0 fails: k = 0, and the prefix sums stand
    still over it."""
    tr = np.zeros(3, orc.TRIANGLE)
    mt = np.zeros(2, orc.MATERIAL)
    tr["e1"] = (1, 0, 0)
    tr["e2"][0] = (2, 0, 0)
    tr["e2"][1] = (0, 1, 0)
    tr["e2"][2] = (0, 3, 0)
    tr["material_idx"] = (1, 1, 0)
    lights = P.PowerLights(E.Emission({1: (1.0, 2.0, 3.0)}, triangles=tr, materials=mt))
    assert lights.list.tolist() == [0, 1]
    assert lights.weights()[0] == 0 and lights.weights()[1] == luma_by_hand(1, 2, 3) * F(0.5)
    assert lights.k.tolist() == [0, 65535]
    assert lights.cdf.tolist() == [0, 65535] and lights.total == 65535
    assert lights.prim_k.tolist() == [0, 65535, 0]
    i, nfi = lights.select(np.linspace(0, 1, 4097).astype(F))
    assert (i == 1).all() and (nfi == 1).all()


def test_no_distribution_where_the_maximum_is_not_finite_or_not_above_zero(orc):
    assert not P.PowerLights(spheres_em(orc, [np.inf, 1.0], [(1, 1, 1), (1, 1, 1)])).has_distribution  # an infinite area
    assert not P.PowerLights(spheres_em(orc, [0.0, 0.0], [(1, 1, 1), (1, 1, 1)])).has_distribution  # no f above 0
    assert not P.PowerLights(spheres_em(orc, [1.0], [(0, 0, 0)])).has_distribution  # no light at all
    nan = P.PowerLights(spheres_em(orc, [np.nan, 1.0], [(1, 1, 1), (1, 1, 1)]))  # a NaN is no maximum: it only gets k = 0
    assert nan.has_distribution and nan.k.tolist() == [0, 65535]


# ---------------------------------------------------------------- the selection
def test_selection_edges(orc):
    lights = P.PowerLights(spheres_em(orc, [0.0, 2.0, 1.0, 0.0, 0.5, 0.0], [(1, 1, 1)] * 3 + [(2, 2, 2)] + [(0, 1, 4)] + [(1, 1, 1)]))
    assert lights.k.tolist()[0] == 0 and lights.k.tolist()[3] == 0 and lights.k.tolist()[5] == 0
    u0 = np.array([0.0, 1 - 2.0 ** -24, 1.0, np.nan, -0.25, -np.inf, np.inf, 2.0], F)
    i, nfi = lights.select(u0)
    last = 4  # the last light with k > 0
    assert i.tolist() == [1, last, last, 1, 1, 1, last, last]
    total, k = lights.total, lights.k
    assert np.array_equal(nfi, (np.full(len(i), total, np.uint64).astype(F) / k[i].astype(F)))
    # a sweep: a light with k = 0 is never returned, every other one is, and each T lands where the prefix sums say
    sweep = np.linspace(0.0, 1.0, 200001).astype(F)
    i, _ = lights.select(sweep)
    assert set(i.tolist()) == {1, 2, 4}
    T = np.minimum(np.floor(sweep.astype(np.float64) * total), total - 1).astype(np.uint64)
    assert (lights.cdf[i] > T).all() and (np.where(i > 0, lights.cdf[np.maximum(i, 1) - 1], 0) <= T).all()


def receivers(k, seed):
    rng = np.random.default_rng(seed)
    p = (rng.standard_normal((k, 3)) * 3).astype(F)
    n = rng.standard_normal((k, 3))
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(F)
    return p, n, rng.random((k, 3)).astype(F)


def test_one_light_is_nee_refs_sample_bit_for_bit(orc):
    for em in (spheres_em(orc, [0.7, 1.0], [(3, 2, 1), (0, 0, 0)]),):
        power, plain = P.PowerLights(em), N.Lights(em)
        assert power.total == 65535 and power.k.tolist() == [65535]
        p, n, u = receivers(4000, 3)
        u[:4, 0] = (0.0, 1 - 2.0 ** -24, 1.0, np.nan)
        a, b = power.sample(p, n, u[:, 0], u[:, 1], u[:, 2]), plain.sample(p, n, u[:, 0], u[:, 1], u[:, 2])
        assert (a["nfi"] == 1).all()
        for key in ("q", "w", "dist", "e_q", "G"):
            assert np.array_equal(a[key].view(np.uint32), b[key].view(np.uint32)), key
        assert np.array_equal(a["prim"], b["prim"]) and np.array_equal(a["lit"], b["lit"]) and a["lit"].any()
    tr = np.zeros(2, orc.TRIANGLE)
    tr["e1"], tr["e2"], tr["material_idx"] = (1, 0.5, 0), (0, 1, 0.25), (0, 1)
    em = E.Emission({1: (1.0, 2.0, 3.0)}, triangles=tr, materials=np.zeros(2, orc.MATERIAL))
    p, n, u = receivers(1000, 4)
    a, b = P.PowerLights(em).sample(p, n, u[:, 0], u[:, 1], u[:, 2]), N.Lights(em).sample(p, n, u[:, 0], u[:, 1], u[:, 2])
    for key in ("q", "w", "dist", "e_q", "G"):
        assert np.array_equal(a[key].view(np.uint32), b[key].view(np.uint32)), key


# ---------------------------------------------------------------- unbiasedness
def direct_light(lights, n_draws, seed):
    """Per draw, the luminance of e_q G at a fixed receiver under unoccluded lights: the estimator's direct light per unit throughput."""
    rng = np.random.default_rng(seed)
    u = rng.random((n_draws, 3)).astype(F)
    p = np.tile(np.array([[0.5, -1.0, 0.25]], F), (n_draws, 1))
    n = np.tile(np.array([[0.0, 1.0, 0.0]], F), (n_draws, 1))
    s = lights.sample(p, n, u[:, 0], u[:, 1], u[:, 2])
    with np.errstate(all="ignore"):
        v = np.where(s["lit"][:, None], s["e_q"] * s["G"][:, None], F(0)).astype(np.float64)
    return 0.2126 * v[:, 0] + 0.7152 * v[:, 1] + 0.0722 * v[:, 2]


def two_unequal_lights(orc):
    """a big bright sphere and a small dim one, both above the receiver's tangent plane, neither hiding the other from it"""
    sp = np.zeros(2, orc.SPHERE)
    sp["center"][0, :3], sp["radius"][0] = (-2.0, 2.0, 0.0), 1.0
    sp["center"][1, :3], sp["radius"][1] = (2.5, 1.0, 1.0), 0.2
    sp["center"][:, 3] = 1.0
    sp["material_idx"] = (0, 1)
    return E.Emission({0: (8.0, 6.0, 4.0), 1: (0.5, 1.0, 0.25)}, spheres=sp, materials=np.zeros(2, orc.MATERIAL))


def z_score(a, b):
    se = np.sqrt(a.var(ddof=1) / len(a) + b.var(ddof=1) / len(b))
    return (a.mean() - b.mean()) / se


def test_power_selection_is_unbiased_and_a_missing_weight_is_seen(orc):
    """N = 400 000 draws each. The two estimators' means agree within 5 standard errors (from the two sample variances); with the weight
    left at nf -- the selection by power without its 1 / P -- they do not: the test sees a missing 1 / P."""
    em = two_unequal_lights(orc)
    n_draws = 400000
    uniform = direct_light(N.Lights(em), n_draws, 11)
    power = direct_light(P.PowerLights(em), n_draws, 12)
    z = z_score(power, uniform)
    print(f"uniform {uniform.mean():.6g} (var {uniform.var():.4g}), power {power.mean():.6g} (var {power.var():.4g}), z {z:.2f}")
    assert abs(z) <= 5.0
    mutant = direct_light(P.PowerLights(em, uniform_weight=True), n_draws, 12)
    zm = z_score(mutant, uniform)
    print(f"mutation (weight nf): {mutant.mean():.6g}, z {zm:.2f}")
    assert abs(zm) > 5.0
