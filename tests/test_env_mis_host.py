"""Multiple importance sampling between the environment map and the scatter (WFPT_FLAG_ENV_MIS) without a GPU: the weights of
tests/env_mis_ref.py, its estimator on the oracle against closed forms, its mutations, its variance against the two estimators it
combines, the edge directions of the miss weight and the interface.

The ground scene of tests/test_env_nee_host.py: one Lambertian sphere of radius 1000, convex, so every scattered ray misses. A ground
pixel expects albedo * the integral of env_lookup(w) cos / pi over the hemisphere of its normal, plus albedo * e * F for the lamp."""
import os

import numpy as np
import pytest

import emission_ref as E
import env_mis_ref as X
import env_nee_ref as V
from environment_ref import env_lookup
from helpers import make_oracle
from test_env_nee_host import H_, LAMP_E, LUMA, W_, expected_luminance, ground_geometry, lit_directions
from test_nee_host import pixel_mean

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PI = F(3.1415927)
BOUND = 4.0  # standard errors: test_env_nee_host.test_ground_matches_the_closed_form's bound, over ground_geometry's footprint mask


@pytest.fixture(scope="module")
def W():
    import wavefront_path_tracer_amd as W
    return W


# ---------------------------------------------------------------- the two weights of one direction
WEIGHT_MAPS = {"sun": V.sun_map, "block": V.block_map, "soft sky": X.soft_sky}
# The next power of two above the worst |we + wb - 1| measured below over 6 x 12 000 samples whose reverse texel is the sampled one:
# 1.19e-07 = 2^-23 (both rotations of the soft sky and the sun map at 0.3; the block map 1.04e-07), and no row's reverse texel differed.
# The two sides take pb from cos_s / pi and from (0.5 |d|) / pi with |d| = 2 cos_s rounded, and pe from the same table entry: the sum is 1
# to the rounding of two divisions.
SUM_BOUND = 2.0 ** -22
TEXEL_CAP = 1e-3


def contributing_samples(light, k, seed, share):
    rng = np.random.default_rng(seed)
    m = 4 * k
    n = rng.standard_normal((m, 3)) + np.array([0.0, 1.5, 0.0])
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(F)
    u = rng.random((m, 4)).astype(F)
    s = light.sample(n, u[:, 0], u[:, 1], u[:, 2], u[:, 3], share)
    keep = np.flatnonzero(s["lit"])[:k]
    assert len(keep) == k
    return n[keep], {key: v[keep] for key, v in s.items()}


@pytest.mark.parametrize("rotation", [0.0, 0.3])
@pytest.mark.parametrize("name", list(WEIGHT_MAPS))
def test_weights_sum_to_one(orc, name, rotation):
    share = 0.5
    light = V.EnvLight(WEIGHT_MAPS[name](), rotation=rotation)
    n, s = contributing_samples(light, 12000, 11, share)
    pe, pb, we = X.env_densities(s, n, share)
    with np.errstate(all="ignore"):
        cos_s = V.dot3(n, s["w"])
        d = (s["w"] * (F(2) * cos_s)[:, None]).astype(F)  # the scattered ray that would carry this direction: |d| = 2 cos
    m = X.miss_weight(light, d, share)
    same = m["texel"] == s["texel"]
    differing = 1.0 - same.mean()
    worst = float(np.abs((we[same].astype(np.float64) + m["wb"][same].astype(np.float64)) - 1.0).max())
    print(f"{name} rotation {rotation}: worst |we + wb - 1| {worst:.3g} over {int(same.sum())} rows, reverse texel differs in {differing:.2g} of the rows")
    assert differing <= TEXEL_CAP
    assert worst < SUM_BOUND
    assert (we > 0).all() and (we < 1).all() and (m["wb"][same] > 0).all()


def test_edge_directions(orc):
    """Zero, NaN, infinite and straight-up / straight-down directions: st = 0 (or NaN) gives wb = 1 and pe = 0, and no index leaves the table
    (miss_weight asserts that itself)."""
    for make in WEIGHT_MAPS.values():
        for rotation in (0.0, 0.3):
            light = V.EnvLight(make(), rotation=rotation)
            dirs = np.array([(0, 0, 0), (np.nan, 0, 1), (0, np.nan, 0), (np.inf, 0, 0), (0, -np.inf, 0), (np.inf, np.inf, np.inf), (0, 1, 0), (0, -1, 0),
                             (0, 2.5, 0), (0, -1e-30, 0), (1e-30, 0, 0), (1e30, 1e30, 1e30), (0, 0, -1), (-1e-9, 0, -1), (1e-9, 0, -1)], F)
            m = X.miss_weight(light, dirs, 0.5)
            assert (m["wb"][:10] == 1).all() and (m["pe"][:10] == 0).all(), m
            assert ((0 <= m["texel"]) & (m["texel"] < light.dist.w * light.dist.h)).all()
            assert np.isfinite(m["wb"][10:]).all() and (m["wb"][10:] > 0).all() and (m["wb"][10:] <= 1).all()


# ---------------------------------------------------------------- the estimator on the ground
def ground_render(orc, env, lamp, share=0.5, spp=8, occluder=False, w=W_, h=H_, kind="env_mis", lamp_e=LAMP_E, **mut):
    inputs = V.ground_inputs(orc, w, h, lamp=lamp, occluder=occluder)
    em = E.Emission({1: lamp_e} if lamp else {}, spheres=inputs[0], materials=inputs[1])
    o = make_oracle(orc, inputs, w, h, max_wavefronts=4, miss_floor=0, rng_mode=1)
    if kind == "environment":
        return inputs, E.render_with_emission(o, em, spp=spp, env=env, parts=True)
    shadow = make_oracle(orc, inputs, w, h)
    light = V.EnvLight(env)
    if kind == "env_nee":
        return inputs, V.render_with_env_nee(o, shadow, em, light, share=share, spp=spp, parts=True)
    return inputs, X.render_with_env_mis(o, shadow, em, light, share=share, spp=spp, parts=True, **mut)


def sky_and_lamp_luminance(env, inputs, lamp_e=LAMP_E):
    """(per-pixel expected luminance, mask) of the ground pixels under a map that is lit everywhere, with the lamp: albedo times
    (env_nee_ref.irradiance of the pixel's normal, less what the lamp hides, plus e F). The ground's normals lie within 0.01 rad of +y, so the
    irradiance is taken at +y and at two tilted normals and interpolated linearly (what that leaves out is of the order of the tilt
    squared, 1e-4 relative). The lamp hides F times the map's value in its direction; pixels where it can stand between the ground point and
    the sun's texel (widened by a texel) are left out, as expected_luminance does."""
    p, n, ok, form = ground_geometry(inputs, True)
    eps = 0.02
    e0 = V.irradiance(env, (0.0, 1.0, 0.0))
    tilt = lambda a, b: np.array([a, 1.0, b]) / np.linalg.norm([a, 1.0, b])
    ex, ez = V.irradiance(env, tilt(eps, 0.0)), V.irradiance(env, tilt(0.0, eps))
    sky = e0[None] + (n[:, 0] / tilt(eps, 0.0)[0])[:, None] * (ex - e0)[None] + (n[:, 2] / tilt(0.0, eps)[2])[:, None] * (ez - e0)[None]
    lc = np.array([0.0, 2.0, 0.0])
    v = lc[None] - p
    to_lamp = v / np.linalg.norm(v, axis=1, keepdims=True)
    sky = sky - env_lookup(env, to_lamp.astype(F)).astype(np.float64) * form[:, None]
    sun = np.where((env > 1.0).any(axis=2, keepdims=True), env, 0.0).astype(F)
    for d in lit_directions(sun):
        along = v @ d
        off = np.linalg.norm(v - along[:, None] * d[None], axis=1)
        ok = ok & ~((along > 0) & (off < 2 * 0.25))
    albedo = np.asarray(V.GROUND["albedo"])
    rgb = albedo[None] * sky + albedo[None] * np.asarray(lamp_e)[None] * form[:, None]
    return rgb @ LUMA, ok


def z_of(r, spp, want, ok):
    mean, se = pixel_mean(r, spp, ok)
    return (mean - want[ok].mean()) / se, mean, se


LEN_OVER_PI = lambda ln: ln / PI
# The lamp of the sun-map case, 100 times test_env_nee_host's: over the footprint mask the lamp's form factor averages about 2e-3, and only
# with a lamp this bright does its light (2.0 of the mean luminance 2.86) outweigh the sky's (0.8) enough for a wrong emission-pass weight
# to move the mean by more than the noise at a spp the CPU can render. The closed form takes the form factor at the pixel's centre, which
# leaves out about -0.7 % of the lamp's part (the footprint's curvature; ENV_NEE without this flag shows the same: z = -1.44 at 64 spp,
# -3.35 at 256), so the true render drifts to negative z as the spp grows; every spp used below keeps it inside the bound.
SUN_LAMP_E = tuple(100.0 * c for c in LAMP_E)
# mutation -> (keywords of render_with_env_mis, spp on the block map (None: a no-op there, p = 1), spp on the sun map with the lamp): the
# smallest power of two at which the mutation falls outside the bound. z, true render -> mutation:
#   block map:          2 spp +1.29 -> +21.96 (both at full weight), +7.05 (pb = len / pi); the true render at 8 spp: -0.02
#   sun map + lamp:     2 spp -0.94 -> +7.69 (both at full weight; the true render at 8 spp: -1.00); 32 spp -0.82 -> +6.29 (pb = len / pi; +3.97 at 16);
#                       16 spp -1.16 -> -5.14 (pe without p; -3.81 at 8); 64 spp -1.38 -> -4.94 (plq without q; -3.40 at 32, -8.16 at 128)
MUTATIONS = {
    "we dropped: both strategies at full weight": (dict(full_weight=True), 2, 2),
    "pb = len / pi in the miss": (dict(miss_pb_of_len=LEN_OVER_PI), 2, 32),
    "pe without p in the miss": (dict(miss_pe_without_p=True), None, 16),
    "plq without q in the emission pass": (dict(emission_plq_without_q=True), None, 64),
}


def check_case(orc, env, lamp, want, ok, column, lamp_e=LAMP_E):
    """The true render inside the bound and each mutation outside it, at the mutation's own spp (the true render is checked at every spp a
    mutation is judged at). p = 1 makes two of the mutations no-ops: asserted bit for bit."""
    true = {}

    def true_at(spp):
        if spp not in true:
            _, r = ground_render(orc, env, lamp, spp=spp, lamp_e=lamp_e)
            z, mean, se = z_of(r, spp, want, ok)
            print(f"true render at {spp} spp: closed form {want[ok].mean():.6g}, restatement {mean:.6g}, se {se:.3g}, z {z:.2f}; {r['stats']}")
            assert abs(z) <= BOUND
            true[spp] = r
        return true[spp]

    r8 = true_at(8)
    for name, spec in MUTATIONS.items():
        mut, spp = spec[0], spec[column]
        if spp is None:  # p = 1: the share is not there to drop
            _, same = ground_render(orc, env, lamp, spp=2, lamp_e=lamp_e, **mut)
            assert np.array_equal(same["acc"].view(np.uint32), true_at(2)["acc"].view(np.uint32)), name
            continue
        true_at(spp)
        _, wrong = ground_render(orc, env, lamp, spp=spp, lamp_e=lamp_e, **mut)
        zw, m, s = z_of(wrong, spp, want, ok)
        print(f"  mutation '{name}' at {spp} spp: {m:.6g}, se {s:.3g}, z {zw:.2f}")
        assert abs(zw) > BOUND, f"the mutation '{name}' passes the closed-form check"
    return r8


def test_block_map_matches_the_closed_form(orc):
    """No emitter, p = 1: the environment branch and the weighed miss. Measured (96 x 72): the figures above MUTATIONS and in DESIGN.md 9l."""
    env = V.block_map()
    inputs = V.ground_inputs(orc, W_, H_)
    want, ok = expected_luminance(env, inputs, False)
    assert ok.sum() > 2000
    r = check_case(orc, env, False, want, ok, 1)
    st = r["stats"]
    assert st["weighed_misses"] > 0 and st["env_samples"] > 0 and st["weighed_hits"] == 0 and st["light_samples"] == 0
    assert r["image"][:, ok].any(), "the scattered rays' misses count"


def test_sun_map_with_the_lamp_matches_the_closed_form(orc):
    """p = 0.5: both branches of the connect pass, the weighed emission pass and the weighed miss all run."""
    env = V.sun_map()
    inputs = V.ground_inputs(orc, W_, H_, lamp=True)
    want, ok = sky_and_lamp_luminance(env, inputs, SUN_LAMP_E)
    assert ok.sum() > 2000
    st = check_case(orc, env, True, want, ok, 2, SUN_LAMP_E)["stats"]
    assert min(st.values()) > 0, st


# ---------------------------------------------------------------- variance
def variance_sum(r, spp):
    s1, s2 = r["s1"].astype(np.float64), r["s2"].astype(np.float64)
    return float(((s2 - s1 * s1 / spp) / (spp - 1)).sum())


def test_variance_against_the_two_estimators_it_combines(orc):
    """160 x 120, the ground with the occluder, equal spp, the summed per-pixel sample variance of the luminance. Under the soft sky the
    scatter is the better strategy and ENV_NEE wastes its shadow rays below the horizon; under the sun map the scatter alone almost never
    finds the sun. The combination is below both."""
    w, h, spp = 160, 120, 8
    for name, env, other in (("soft sky", X.soft_sky(), "env_nee"), ("sun map", V.sun_map(), "environment")):
        _, a = ground_render(orc, env, False, spp=spp, occluder=True, w=w, h=h)
        _, b = ground_render(orc, env, False, spp=spp, occluder=True, w=w, h=h, kind=other)
        va, vb = variance_sum(a, spp), variance_sum(b, spp)
        print(f"{name}: variance sum with the flag {va:.6g}, {other} {vb:.6g}, ratio {va / vb:.4g}")
        assert va < vb


# ---------------------------------------------------------------- the interface without a device
def test_flag_and_bindings(W):
    assert W.FLAG_ENV_MIS == 1 << 18 and "FLAG_ENV_MIS" in W.__all__
    hdr = open(os.path.join(ROOT, "include", "wfpt.h")).read()
    assert "WFPT_FLAG_ENV_MIS = 1u << 18" in hdr
    for name in ("wfpt_sample_environment_light_mis", "wfpt_env_mis_miss_weight"):
        assert name in W.abi_symbols() and hasattr(W.lib(), name)
    for name in ("sample_environment_light_mis", "env_mis_miss_weight"):
        assert callable(getattr(W.PathTracer, name))


def test_the_flag_is_refused_without_each_companion_and_with_mis(W):
    """wfpt_create checks its flags before it looks for a device."""
    all4 = W.FLAG_ENVIRONMENT | W.FLAG_EMISSION | W.FLAG_NEE | W.FLAG_ENV_NEE
    for missing in (W.FLAG_ENVIRONMENT, W.FLAG_EMISSION, W.FLAG_NEE, W.FLAG_ENV_NEE, all4):
        with pytest.raises(W.WfptError) as e:
            W.shirley_path_tracer(32, 32, flags=W.FLAG_ENV_MIS | (all4 & ~missing))
        assert "needs WFPT_FLAG_" in str(e.value), str(e.value)
    with pytest.raises(W.WfptError) as e:
        W.shirley_path_tracer(32, 32, flags=W.FLAG_ENV_MIS | all4 | W.FLAG_MIS)
    assert "WFPT_FLAG_MIS" in str(e.value), str(e.value)
