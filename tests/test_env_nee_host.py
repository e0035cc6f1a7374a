"""Environment next-event estimation (WFPT_FLAG_ENV_NEE) without a GPU: the tables of tests/env_nee_ref.py, its estimator on the oracle
against closed forms, its mutations, the double-counting rule and the interface.

The ground scene: one Lambertian sphere of radius 1000. It is convex, so every scattered ray misses: exactly one bounce, and a ground
pixel expects albedo * integral of env_lookup(w) cos / pi over the hemisphere of its normal. For the constant map that is the albedo.
For the block map every lit direction is far above every ground pixel's horizon, so the integral is n . V with V the map's vector
irradiance (float64 quadrature of the restatement's own lookup). A lamp (sphere of radius r at distance d, wholly above the horizon)
adds albedo * e * F and hides F of a constant sky, F = (r / d)^2 cos(theta)."""
import os

import numpy as np
import pytest

import emission_ref as E
import env_nee_ref as V
from environment_ref import env_lookup
from helpers import make_oracle
from test_nee_host import camera_rays, hit_sphere, pixel_mean

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W_, H_, SPP = 96, 72, 8
LAMP_E = (16.0, 8.0, 32.0)
LUMA = np.array([0.2126, 0.7152, 0.0722])


@pytest.fixture(scope="module")
def W():
    import wavefront_path_tracer_amd as W
    return W


# ---------------------------------------------------------------- the tables
def maps():
    rng = np.random.default_rng(7)
    black_rows = (rng.random((8, 16, 3)) + 0.1).astype(F)
    black_rows[:3] = 0  # rows 0 and 1 have no lit neighbour: their totals are 0 (row 2 borders row 3)
    black_rows[6:] = 0
    single = np.zeros((8, 16, 3), F)
    single[5, 0] = (0.0, 2.0, 0.0)
    return {"1x1": np.full((1, 1, 3), 0.5, F), "1x4": rng.random((4, 1, 3)).astype(F), "3x2": rng.random((2, 3, 3)).astype(F),
            "16x8": rng.random((8, 16, 3)).astype(F), "black rows": black_rows, "single texel": single, "constant": np.ones((8, 16, 3), F)}


@pytest.mark.parametrize("name", list(maps()))
def test_tables(orc, name):
    env = maps()[name]
    d = V.Distribution(env)
    h, w = env.shape[:2]
    assert d.ok and d.total > 0 and d.total == int(d.k.sum())
    assert d.k.min() >= 0 and d.k.max() == 65535
    assert (np.diff(d.row.astype(np.int64), axis=1) >= 0).all() and (np.diff(d.marg.astype(np.int64)) >= 0).all(), "prefix sums are monotone"
    lit = (env != 0).any(axis=2)
    near = np.zeros_like(lit)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            near |= np.roll(lit, dx, axis=1)[np.clip(np.arange(h) + dy, 0, h - 1)]
    assert (d.k[near] >= 1).all(), "a texel a lit texel's taps reach has weight 0"
    assert (d.k[~near] == 0).all()
    row_total = d.row[:, -1].astype(np.int64)
    black = ~near.any(axis=1)
    assert (row_total[black] == 0).all() and (row_total[~black] > 0).all()
    # the extremes of both draws: never a black row or column, never an index out of range
    us = np.array([0.0, 2.0 ** -24, 0.5, 1 - 2.0 ** -24, 1.0], F)
    u1, u2 = [a.reshape(-1) for a in np.meshgrid(us, us, indexing="ij")]
    y, x, k = d.select(u1, u2)
    assert ((0 <= y) & (y < h) & (0 <= x) & (x < w)).all()
    assert (k >= 1).all() and not black[y].any() and (k == d.k[y, x]).all()
    last_row = np.flatnonzero(~black)[-1]
    assert (y[u1 == 1.0] == last_row).all(), "u1 = 1.0 selects the last lit row"
    assert (x[(u1 == 1.0) & (u2 == 1.0)] == np.flatnonzero(d.k[last_row])[-1]).all(), "u2 = 1.0 selects the row's last lit column"
    assert (y[u1 == 0.0] == np.flatnonzero(~black)[0]).all()
    # NaN, negative and infinite draws of a caller's row stay inside the tables
    y, x, k = d.select(np.array([np.nan, -1.0, np.inf, 2.0], F), np.array([np.nan, -np.inf, np.inf, 0.5], F))
    assert ((0 <= y) & (y < h) & (0 <= x) & (x < w) & (k >= 1)).all()


def test_a_black_map_has_no_distribution(orc):
    assert not V.Distribution(np.zeros((4, 8, 3), F)).ok


def test_selection_frequencies_follow_the_weights(orc):
    env = V.sun_map()
    d = V.Distribution(env)
    n = 200000
    u = np.random.default_rng(5).random((n, 2)).astype(F)
    y, x, _ = d.select(u[:, 0], u[:, 1])
    got = np.bincount(y * d.w + x, minlength=d.w * d.h) / n
    want = d.k.reshape(-1) / d.total
    assert np.abs(got - want).max() < 5 * np.sqrt(want.max() / n)


# ---------------------------------------------------------------- the estimator on the ground
def ground_geometry(inputs, lamp=False):
    """Per pixel: the ground point's unit normal (float64), the mask of the pixels whose whole footprint lies on the ground (and clear of
    the lamp's image), and the lamp's form factor F there."""
    ys, xs = np.mgrid[0:H_, 0:W_].astype(np.float64)
    gc, gr = np.array([0.0, -V.GROUND["r"], 0.0]), V.GROUND["r"]
    lc, lr = np.array([0.0, 2.0, 0.0]), 0.25
    ok = np.ones((H_, W_), bool)
    for dx, dy in ((0, 0), (-1, -1), (1, -1), (-1, 1), (1, 1)):
        o, d = camera_rays(inputs, W_, H_, xs + 0.5 + dx, ys + 0.5 + dy)
        t = hit_sphere(o, d, gc, gr)
        ok &= np.isfinite(t)
        if lamp:
            ok &= ~np.isfinite(hit_sphere(o, d, lc, 2.0 * lr))
        if (dx, dy) == (0, 0):
            p = o + np.where(np.isfinite(t), t, 0.0)[..., None] * d
    n = (p - gc) / gr
    v = lc - p
    dist = np.linalg.norm(v, axis=-1)
    form = (lr / dist) ** 2 * (n * v).sum(-1) / dist
    return p.reshape(-1, 3), n.reshape(-1, 3), ok.reshape(-1), form.reshape(-1)


def lit_directions(env):
    """Unit directions (float64) covering every direction whose lookup can be non-zero: the lit texels widened by one texel."""
    h, w = env.shape[:2]
    lit = np.argwhere((env != 0).any(axis=2))
    out = []
    for yy, xx in lit:
        for v in np.linspace(yy - 0.5, yy + 1.5, 9) / h:
            for u in np.linspace(xx - 0.5, xx + 1.5, 9) / w:
                th, ph = np.pi * v, 2 * np.pi * (u - 0.5)
                out.append((np.sin(th) * np.sin(ph), np.cos(th), -np.sin(th) * np.cos(ph)))
    return np.array(out)


def vector_irradiance(env, n_theta=1024, n_phi=2048):
    """V[c] (3 x 3 float64): sum of env_lookup_c(w) w dw / pi over the sphere; n . V[c] is the irradiance integral of a receiver whose
    horizon lies below every lit direction."""
    th = (np.arange(n_theta) + 0.5) * np.pi / n_theta
    ph = (np.arange(n_phi) + 0.5) * 2 * np.pi / n_phi
    T, Ph = np.meshgrid(th, ph, indexing="ij")
    d = np.stack([np.sin(T) * np.cos(Ph), np.cos(T), np.sin(T) * np.sin(Ph)], -1).reshape(-1, 3)
    val = env_lookup(env, d.astype(F)).astype(np.float64)
    keep = val.any(axis=1)
    dw = (np.sin(T) * (np.pi / n_theta) * (2 * np.pi / n_phi)).reshape(-1)
    return np.einsum("ic,ij->cj", val[keep] * dw[keep, None], d[keep]) / np.pi


def ground_render(orc, env, lamp=False, share=0.5, spp=SPP, mirror=False, look_at=(0.0, 0.0, 0.0), **mut):
    inputs = V.ground_inputs(orc, W_, H_, lamp=lamp, mirror=mirror, look_at=look_at)
    em = E.Emission({1: LAMP_E} if lamp else {}, spheres=inputs[0], materials=inputs[1])
    o = make_oracle(orc, inputs, W_, H_, max_wavefronts=4, miss_floor=0, rng_mode=1)
    shadow = make_oracle(orc, inputs, W_, H_)
    light = V.EnvLight(env, **{k: mut.pop(k) for k in ("drop_st", "drop_p") if k in mut})
    return inputs, V.render_with_env_nee(o, shadow, em, light, share=share, spp=spp, parts=True, **mut)


def expected_luminance(env, inputs, lamp):
    """(per-pixel expected luminance, mask) of the ground pixels, float64."""
    p, n, ok, form = ground_geometry(inputs, lamp)
    albedo = np.asarray(V.GROUND["albedo"])
    if (env == env[0, 0]).all():  # a constant sky: the albedo times the value, less what the lamp hides
        sky = np.broadcast_to(np.asarray(env[0, 0], np.float64), (len(n), 3)) * ((1.0 - form)[:, None] if lamp else 1.0)
    else:
        dirs = lit_directions(env)
        assert (n[ok] @ dirs.T).min() > 0.2, "a lit direction is near a ground pixel's horizon: n . V does not hold"
        sky = n @ vector_irradiance(env).T
        if lamp:  # leave out the pixels where the lamp can stand between the ground point and a lit direction
            lc = np.array([0.0, 2.0, 0.0])
            v = lc[None] - p
            for d in dirs:
                along = v @ d
                off = np.linalg.norm(v - along[:, None] * d[None], axis=1)
                ok = ok & ~((along > 0) & (off < 2 * 0.25))
    rgb = albedo[None] * sky
    if lamp:
        rgb = rgb + albedo[None] * np.asarray(LAMP_E)[None] * form[:, None]
    return rgb @ LUMA, ok


@pytest.mark.parametrize("which", ["constant", "block"])
@pytest.mark.parametrize("lamp", [False, True])
def test_ground_matches_the_closed_form(orc, which, lamp):
    """Measured (96 x 72, 8 spp, 3 900 to 6 700 ground pixels; z = (mean - closed form) / standard error, the standard error from the
    per-sample luminances): constant map z = +1.11, with the lamp +2.79; block map z = +0.01, with the lamp +0.73. Mutations, each in
    its own standard errors: the pdf without st: +58.6 and +53.1 (with the lamp +39.6 and +31.8); Genv without the division by p (lamp
    present, share 0.5): -103.8 and -101.2.
    The closed form leaves out one thing the scene does have: on a sphere of radius 1000 the float32 hit point lies up to 1e-4 off the
    surface, and a few grazing scattered rays meet the ground again beyond t_min. They are connected again, correctly, and add about
    +0.3 % (constant map, three other frame ranges at 16 spp: z = +0.37, +0.65, +0.73, +1.00) -- below the standard error here."""
    env = np.ones((8, 16, 3), F) if which == "constant" else V.block_map()
    inputs, r = ground_render(orc, env, lamp=lamp)
    want, ok = expected_luminance(env, inputs, lamp)
    assert ok.sum() > 2000
    mean, se = pixel_mean(r, SPP, ok)
    z = (mean - want[ok].mean()) / se
    print(f"{which} lamp={lamp}: closed form {want[ok].mean():.6g}, restatement {mean:.6g}, se {se:.3g}, z {z:.2f}")
    assert abs(z) <= 4.0
    assert not r["image"][:, ok].any(), "a convex ground: the connect pass alone lights a ground pixel (the miss after it is gated)"
    muts = [{"drop_st": True}] + ([{"drop_p": True}] if lamp else [])
    for mut in muts:
        _, wrong = ground_render(orc, env, lamp=lamp, **mut)
        m, s = pixel_mean(wrong, SPP, ok)
        zw = (m - want[ok].mean()) / s
        print(f"  mutation {mut}: {m:.6g}, se {s:.3g}, z {zw:.1f}")
        assert abs(zw) > 10.0, f"the mutation {mut} passes the closed-form check"


def test_share_one_and_a_small_share_agree(orc):
    """share = 1 never picks the lamp (its light is lost: no emitter branch, and the emission pass is gated); share = 0.25 must still
    meet the closed form."""
    env = V.block_map()
    inputs, r = ground_render(orc, env, lamp=True, share=0.25)
    want, ok = expected_luminance(env, inputs, True)
    mean, se = pixel_mean(r, SPP, ok)
    print(f"share 0.25: z {(mean - want[ok].mean()) / se:.2f}")
    assert abs(mean - want[ok].mean()) <= 4.0 * se


# ---------------------------------------------------------------- the map is counted once
def test_the_map_is_counted_once(orc):
    env = np.ones((8, 16, 3), F)
    inputs, r = ground_render(orc, env, mirror=True, look_at=(0.0, 3.5, 0.0))
    sp = inputs[0]
    o = make_oracle(orc, inputs, W_, H_, max_wavefronts=1, miss_floor=0, rng_mode=1)
    first = E.render_with_emission(o, E.Emission({}, spheres=sp, materials=inputs[1]), spp=1, env=env, parts=True)["first_prim"][0]
    metal, ground = int(np.flatnonzero(sp["material_idx"] == 3)[0]), int(np.argmax(sp["radius"]))
    # far from the mirror (it hides less than 0.1 % of the sky there) the ground sees the whole sky: the albedo; counted twice, twice that
    p, _, ok, _ = ground_geometry(inputs)
    far = ok & (first == ground) & (np.linalg.norm(p - sp["center"][metal, :3].astype(np.float64), axis=1) > 6.0)
    assert far.sum() > 1000
    want = float(np.asarray(V.GROUND["albedo"]) @ LUMA)
    mean, se = pixel_mean(r, SPP, far)
    _, wrong = ground_render(orc, env, mirror=True, look_at=(0.0, 3.5, 0.0), never_gate_miss=True)
    mean_w, se_w = pixel_mean(wrong, SPP, far)
    print(f"gated {mean:.6g} (z {(mean - want) / se:.2f}), never gated {mean_w:.6g} (z {(mean_w - want) / se_w:.1f}), albedo {want:.6g}")
    assert abs(mean - want) <= 4.0 * se
    assert abs(mean_w - 2 * want) <= 4.0 * se_w and abs(mean_w - want) > 10.0 * se_w, "the test cannot tell the never-gate-the-miss mutation"
    # a primary miss shows the map itself; a mirror shows it wherever its reflection misses (albedo 1, fuzz 0)
    sky = (first == -1).reshape(H_, W_)
    missed = sky & np.roll(sky, -2, axis=0)  # two rows clear of the horizon: the jitter spans one pixel
    missed[-2:] = False
    missed = missed.reshape(-1)
    # (the map's value: 1 up to the rounding of the four bilinear weights' sum)
    assert missed.sum() > 100 and (np.abs(r["value"][:, missed] - 1.0) < 1e-6).all()
    on_mirror = first == metal
    assert on_mirror.sum() > 50
    sky_in_mirror = on_mirror & (np.abs(r["image"] - 1.0) < 1e-6).all(axis=2).any(axis=0)
    assert sky_in_mirror.sum() > 20, "no pixel on the metal sphere mirrors the sky"
    assert (r["acc"][on_mirror] > 0).all()


# ---------------------------------------------------------------- the interface without a device
def test_flag_and_bindings(W):
    assert W.FLAG_ENV_NEE == 1 << 16
    hdr = open(os.path.join(ROOT, "include", "wfpt.h")).read()
    assert "WFPT_FLAG_ENV_NEE = 1u << 16" in hdr
    for name in ("FLAG_ENV_NEE",):
        assert name in W.__all__
    for name in ("wfpt_set_environment_share", "wfpt_environment_share", "wfpt_read_environment_distribution", "wfpt_sample_environment_light"):
        assert name in W.abi_symbols() and hasattr(W.lib(), name)
    for name in ("set_environment_share", "environment_share", "environment_distribution", "sample_environment_light"):
        assert callable(getattr(W.PathTracer, name))


def test_the_flag_is_refused_without_each_companion(W):
    """wfpt_create checks its flags before it looks for a device."""
    all3 = W.FLAG_ENVIRONMENT | W.FLAG_EMISSION | W.FLAG_NEE
    for missing in (W.FLAG_ENVIRONMENT, W.FLAG_EMISSION, W.FLAG_NEE, all3):
        with pytest.raises(W.WfptError) as e:
            W.shirley_path_tracer(32, 32, flags=W.FLAG_ENV_NEE | (all3 & ~missing))
        assert "needs WFPT_FLAG_" in str(e.value), str(e.value)
