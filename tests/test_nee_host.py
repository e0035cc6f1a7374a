"""Next-event estimation (WFPT_FLAG_NEE) without a GPU: the numpy restatement (tests/nee_ref.py) on the oracle against the closed form of
the lamp scene, against the plain estimator (tests/emission_ref.py), the restatement's two mutations, and facts of the light sampler.

The lamp scene: a large Lambertian ground sphere under a small emitting sphere, a black environment (a 1 x 1 zero map in the restatement's
`env` argument). The ground is convex, so only one-bounce light exists and every ground pixel expects albedo * e * (r / d)^2 * cos(theta),
d and theta the distance and the angle to the lamp's centre, wherever the whole lamp is above the point's tangent plane. (Shade reuses one
random stream at every bounce, shade.wgsl:72; with a single scatter that reuse cannot bias this scene.)"""
import os

import numpy as np
import pytest

import emission_ref as E
import nee_ref as N
from helpers import make_oracle
from nee_ref import LAMP

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W_, H_, SPP = 160, 120, 16


@pytest.fixture(scope="module")
def W():
    import wavefront_path_tracer_amd as W
    return W


# ---------------------------------------------------------------- the closed form, in float64
def camera_rays(inputs, w, h, fx, fy):
    """Unit directions (float64) of generate_rays' rays through the image points (fx, fy) in pixel units (generate_rays.wgsl:66-86, no defocus)."""
    cam, ip, vw = inputs[3], np.asarray(inputs[4], np.float64).reshape(4, 4).T, np.asarray(inputs[5], np.float64).reshape(4, 4).T
    ndc = np.stack([2.0 * (fx / w) - 1.0, 2.0 * (1.0 - fy / h) - 1.0, np.ones_like(fx), np.ones_like(fx)], -1)
    pp = ndc @ ip.T  # the matrices cross the ABI column-major
    pp = pp / pp[..., 3:4]
    pp[..., 3] = 0.0
    d = (pp @ vw.T)[..., :3]
    return np.asarray(cam["position"][0, :3], np.float64), d / np.linalg.norm(d, axis=-1, keepdims=True)


def hit_sphere(o, d, c, r):
    """Nearest positive t of rays (o, d) with the sphere (c, r), inf where they miss."""
    oc = o - np.asarray(c, np.float64)
    b = (d * oc).sum(-1)
    disc = b * b - ((oc * oc).sum(-1) - r * r)
    t = -b - np.sqrt(np.maximum(disc, 0.0))
    return np.where((disc > 0) & (t > 0), t, np.inf)


def closed_form(inputs, w, h, lamp_r):
    """Per pixel: the closed form's luminance averaged over the pixel's footprint, a bound on what that average leaves out, and the mask
    of the pixels the form holds for. generate_rays jitters within a disk of radius one pixel, uniformly by area: the average is a
    32-point equal-area quadrature of that disk (4 rings x 8 angles). Over a disk every odd term of the form's expansion cancels; what the
    quadrature can miss is of the order of the curvature term, and the bound is that whole term measured at the corners of the square
    around the disk: |mean of the four corner values - centre value|. The mask: centre and corners on the ground, clear of the lamp's
    image, the whole lamp above the tangent plane."""
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    gc, gr = np.array([0.0, -LAMP["ground_r"], 0.0]), LAMP["ground_r"]
    lc = np.asarray(LAMP["lamp_c"], np.float64)

    def at(dx, dy):
        o, d = camera_rays(inputs, w, h, xs + dx, ys + dy)
        t = hit_sphere(o, d, gc, gr)
        good = np.isfinite(t) & ~np.isfinite(hit_sphere(o, d, lc, 2.0 * lamp_r))
        p = o + np.where(np.isfinite(t), t, 0.0)[..., None] * d
        n = (p - gc) / gr
        v = lc - p
        dist = np.linalg.norm(v, axis=-1)
        above = (n * v).sum(-1)
        rgb = np.asarray(LAMP["albedo"])[None, None] * np.asarray(LAMP["e"])[None, None] * ((lamp_r / dist) ** 2 * above / dist)[..., None]
        return 0.2126 * rgb[..., 0] + 0.7152 * rgb[..., 1] + 0.0722 * rgb[..., 2], good & (above > lamp_r)

    centre, ok = at(0, 0)
    corners = []
    for dx, dy in ((-1, -1), (1, -1), (-1, 1), (1, 1)):
        v, good = at(dx, dy)
        corners.append(v)
        ok &= good
    disk = [at(np.sqrt((i + 0.5) / 4) * np.cos(2 * np.pi * (k + 0.5) / 8), np.sqrt((i + 0.5) / 4) * np.sin(2 * np.pi * (k + 0.5) / 8))[0]
            for i in range(4) for k in range(8)]
    bound = np.abs(np.mean(corners, axis=0) - centre)
    return np.mean(disk, axis=0).reshape(-1), bound.reshape(-1), ok.reshape(-1)


def pixel_mean(r, spp, sel):
    """(mean, standard error) of the per-sample luminance over the pixels sel, from the per-pixel moments the restatement returns (the
    pixels' streams are independent: the variance of the mean is the sum of the pixels' variances of their means)."""
    s1, s2 = r["s1"].astype(np.float64)[sel], r["s2"].astype(np.float64)[sel]
    m = s1 / spp
    var = np.maximum(s2 / spp - m * m, 0.0) * spp / (spp - 1)
    return m.mean(), np.sqrt((var / spp).sum()) / sel.sum()


def lamp_render(orc, lamp_r=LAMP["lamp_r"], spp=SPP, nee=True, mirror=False, **mut):
    inputs = N.lamp_inputs(orc, W_, H_, lamp_r=lamp_r, mirror=mirror)
    em = E.Emission({1: LAMP["e"]}, spheres=inputs[0], materials=inputs[1])
    o = make_oracle(orc, inputs, W_, H_, max_wavefronts=4, miss_floor=0, rng_mode=1)
    if not nee:
        return inputs, E.render_with_emission(o, em, spp=spp, env=N.black_env(), parts=True)
    shadow = make_oracle(orc, inputs, W_, H_)
    return inputs, N.render_with_nee(o, shadow, em, spp=spp, env=N.black_env(), parts=True, **mut)


@pytest.fixture(scope="module")
def lamp(orc):
    return lamp_render(orc)


def test_lamp_scene_matches_the_closed_form(orc, lamp):
    """Measured on this scene (160 x 120, 16 spp, over 10 000 ground pixels): z = (mean - closed form) / standard error = -0.63 (0.020859
    against 0.0209095, standard error 7.96e-05); the footprint bound is 0.27 standard errors, so the 5 standard errors bind: a bias of 2 %
    in G would fail. The never_set_flag mutation, which counts the lamp again when the scattered ray finds it, gives 0.0419: 30.7 of its
    own standard errors out."""
    inputs, r = lamp
    want, bound, ok = closed_form(inputs, W_, H_, LAMP["lamp_r"])
    assert ok.sum() > 10000
    mean, se = pixel_mean(r, SPP, ok)
    z = (mean - want[ok].mean()) / se
    print(f"closed form {want[ok].mean():.6g}, restatement {mean:.6g}, se {se:.3g}, z {z:.2f}, footprint bound {bound[ok].mean() / se:.2f} se")
    assert abs(mean - want[ok].mean()) <= 5.0 * se + bound[ok].mean()
    assert not r["image"].any(), "a convex ground under a black sky: nothing but the connect pass lights a ground pixel"
    # mutation: the flag never set -- the emission pass adds the lamp again after the diffuse bounce
    _, wrong = lamp_render(orc, never_set_flag=True)
    mean_w, se_w = pixel_mean(wrong, SPP, ok)
    print(f"never_set_flag: {mean_w:.6g}, se {se_w:.3g}, z {(mean_w - want[ok].mean()) / se_w:.2f}")
    assert abs(mean_w - want[ok].mean()) > 5.0 * se_w + bound[ok].mean(), "the double-counting mutation passes the closed-form check"
    assert mean_w > mean


def test_agrees_with_the_plain_estimator(orc, lamp):
    """The flag-off restatement finds the lamp by path hits only; the two means over the ground pixels agree within 5 combined standard
    errors. (The lamp as it is: the ground pixels' 16 samples each give the plain estimator a few thousand lamp hits.)"""
    inputs, r = lamp
    _, _, ok = closed_form(inputs, W_, H_, LAMP["lamp_r"])
    _, plain = lamp_render(orc, nee=False)
    (m1, s1), (m0, s0) = pixel_mean(r, SPP, ok), pixel_mean(plain, SPP, ok)
    print(f"nee {m1:.6g} +- {s1:.3g}, plain {m0:.6g} +- {s0:.3g}, z {(m1 - m0) / np.hypot(s0, s1):.2f}")
    assert s0 < 0.1 * m0, "the plain estimator is too noisy for the comparison to mean anything"
    assert abs(m1 - m0) <= 5.0 * np.hypot(s0, s1)
    assert s1 < 0.5 * s0, "connecting to the lamp does not lower the noise"


def test_a_lamp_in_a_mirror_is_still_seen(orc):
    """A fuzz-0 metal sphere beside the lamp: the pixels on it that mirror the lamp are lit by the emission pass (the flag is 0 after a
    metal hit). A primary metal hit finds the flag 0 with or without the clear, so the pixel itself cannot tell the never_clear_flag
    mutation; the ground around the mirror can: a path ground -> mirror -> lamp keeps the flag the ground hit set, and its light is lost."""
    spp = 16
    inputs, r = lamp_render(orc, lamp_r=0.5, mirror=True, spp=spp)
    sp = inputs[0]
    o = make_oracle(orc, inputs, W_, H_, max_wavefronts=1, miss_floor=0, rng_mode=1)
    first = E.render_with_emission(o, E.Emission({}, spheres=sp, materials=inputs[1]), spp=1, env=N.black_env(), parts=True)["first_prim"][0]
    metal, ground = int(np.flatnonzero(sp["material_idx"] == 3)[0]), int(np.argmax(sp["radius"]))
    on_mirror = first == metal
    assert on_mirror.sum() > 50
    # albedo 1, fuzz 0: a sample that sees the lamp in the mirror is the lamp's colour exactly
    mirrors = on_mirror & (r["emitted"] == np.asarray(LAMP["e"], F)).all(axis=2).any(axis=0)
    assert mirrors.any(), "no pixel on the metal sphere mirrors the lamp"
    assert (r["acc"][mirrors] > 0).all(), "a pixel on the metal sphere that mirrors the lamp is black"
    _, wrong = lamp_render(orc, lamp_r=0.5, mirror=True, spp=spp, never_clear_flag=True)
    assert (wrong["acc"] <= r["acc"]).all()
    lost = (wrong["acc"] < r["acc"]).any(axis=1)
    print(f"{int(mirrors.sum())} mirror pixels see the lamp; never_clear_flag loses light at {int(lost.sum())} pixels, {int((lost & (first == ground)).sum())} of them on the ground")
    assert (lost & (first == ground)).any(), "never_clear_flag loses no light on the ground beside the mirror: the case does not tell it"


# ---------------------------------------------------------------- the sampler
def sphere_lights(orc):
    sp = np.zeros(4, orc.SPHERE)
    mt = np.zeros(3, orc.MATERIAL)
    mt["albedo"][:] = (0.5, 0.5, 0.5, 1.0)
    sp["center"][:, 3] = 1.0
    sp["center"][:, :3] = [(0, 0, 0), (3, 1, -2), (-4, 2, 1), (0, -5, 0)]
    sp["radius"] = (1.0, 0.5, -0.75, 0.0)  # a negative radius, and a radius-0 light
    sp["material_idx"] = (0, 1, 1, 2)
    return sp, mt


def test_sphere_samples_lie_on_the_sphere_and_the_last_light_is_reached(orc):
    sp, mt = sphere_lights(orc)
    L = N.Lights(E.Emission({1: (1.0, 2.0, 3.0), 2: (1.0, 1.0, 1.0)}, spheres=sp, materials=mt))
    assert L.list.tolist() == [1, 2, 3]
    rng = np.random.default_rng(3)
    k = 4000
    u = rng.random((k, 3)).astype(F)
    u[:8] = [(0, 0, 0), (1 - 2.0 ** -24, 0, 0), (0.5, 1, 1), (0.5, 0, 1), (0.5, 1, 0), (0.5, 0.5, 1 - 2.0 ** -24), (1.0, 0.5, 0.5), (0.999, 1 - 2.0 ** -24, 0.25)]
    p = (rng.standard_normal((k, 3)) * 6).astype(F)
    n = rng.standard_normal((k, 3)).astype(F)
    s = L.sample(p, n, u[:, 0], u[:, 1], u[:, 2])
    assert s["prim"][1] == 3 and s["prim"][6] == 3 and s["prim"][0] == 1, "u0 = 1 - 2^-24 (and the draw 1.0) picks the last light"
    c, ra = sp["center"][s["prim"], :3].astype(np.float64), np.abs(sp["radius"][s["prim"]].astype(np.float64))
    err = np.abs(np.linalg.norm(s["q"].astype(np.float64) - c, axis=1) - ra)
    assert (err <= 4e-7 * np.maximum(ra, 1.0)).all(), err.max()
    zero = s["prim"] == 3
    assert zero.any() and not s["lit"][zero].any(), "a radius-0 light contributes"
    assert s["lit"].any() and np.isfinite(s["G"][s["lit"]]).all() and (s["G"][s["lit"]] > 0).all()
    back = (np.einsum("ij,ij->i", n.astype(np.float64), s["q"].astype(np.float64) - p) < -1e-3)
    assert back.any() and not s["lit"][back].any(), "a back-facing receiver is lit"


def test_triangle_samples_stay_inside_and_the_zero_cases_contribute_nothing(orc):
    tr = np.zeros(3, orc.TRIANGLE)
    mt = np.zeros(2, orc.MATERIAL)
    tr["v0"] = [(0, 0, 0), (2, 1, 0), (5, 5, 5)]
    tr["e1"] = [(1, 0, 0), (0, 0.5, 1.5), (1, 2, 3)]
    tr["e2"] = [(0, 1, 0), (1, 0.25, 0), (2, 4, 6)]  # the last one has no area
    tr["material_idx"] = (1, 1, 1)
    L = N.Lights(E.Emission({1: (1.0, 1.0, 1.0)}, triangles=tr, materials=mt))
    assert L.n == 3
    rng = np.random.default_rng(4)
    k = 3000
    u = rng.random((k, 3)).astype(F)
    u[:4] = [(0, 0, 0), (0.4, 1, 1), (0.4, 1 - 2.0 ** -24, 1 - 2.0 ** -24), (0.9, 0.5, 0.5)]
    p = (rng.standard_normal((k, 3)) * 3).astype(F)
    p[4] = tr["v0"][0]  # the receiver at the sampled point itself: dist^2 = 0
    u[4] = (0.0, 1.0, 0.0)
    n = rng.standard_normal((k, 3)).astype(F)
    s = L.sample(p, n, u[:, 0], u[:, 1], u[:, 2])
    t = tr[s["prim"]]
    rel = (s["q"] - t["v0"]).astype(np.float64)
    e1, e2 = t["e1"].astype(np.float64), t["e2"].astype(np.float64)
    good = s["prim"] != 2
    sol = np.stack([np.linalg.lstsq(np.stack([a, b], 1), r, rcond=None)[0] for a, b, r in zip(e1[good], e2[good], rel[good])])
    assert (sol >= -1e-6).all() and (sol <= 1 + 1e-6).all() and (sol.sum(axis=1) <= 1 + 1e-6).all()
    su = np.sqrt(u[:, 1])
    assert ((F(1) - su) >= 0).all() and (u[:, 2] * su <= su).all() and ((F(1) - su) + u[:, 2] * su <= 1).all()
    assert (s["prim"] == 2).any() and not s["lit"][s["prim"] == 2].any(), "a zero-area triangle contributes"
    assert s["dist"][4] == 0 and not s["lit"][4], "dist^2 = 0 contributes"
    with np.errstate(all="ignore"):
        f = np.where(s["lit"][:, None], s["e_q"] * s["G"][:, None], F(0))
    assert np.isfinite(f).all(), "something non-finite leaves a zero case"
    assert s["lit"].any()


def polygon_form_factor(p, n, verts):
    """Lambert's formula, float64: the form factor of a polygon seen from p with normal n (the polygon wholly above the tangent plane),
    (1 / 2 pi) * sum over edges of the angle the edge subtends times n . (the unit normal of the plane through p and the edge)."""
    v = [np.asarray(q, np.float64) - p for q in verts]
    v = [q / np.linalg.norm(q) for q in v]
    total = 0.0
    for a, b in zip(v, v[1:] + v[:1]):
        c = np.cross(a, b)
        total += np.arccos(np.clip(a @ b, -1, 1)) * (n @ (c / np.linalg.norm(c)))
    return abs(total) / (2 * np.pi)


def test_the_sampler_integrates_to_the_form_factors(orc):
    """What neither the lamp scene nor the kernel's own text pins: the weight n_lights of a list with several lights and the area
    sampling of triangles. The mean of the sampler's G over many draws at one receiver must be the sum of the lights' form factors, known
    in float64 from formulas of their own: (r / d)^2 cos(theta) per sphere, Lambert's polygon formula per triangle. 5 standard errors."""
    k = 400000
    u = np.random.default_rng(11).random((k, 3)).astype(F)
    p, n = np.array([0.25, 0.0, -0.5]), np.array([0.0, 1.0, 0.0])
    P, Nn = np.broadcast_to(p.astype(F), (k, 3)), np.broadcast_to(n.astype(F), (k, 3))
    # three sphere lights of different sizes (one of them twice in the list's material), none hiding another
    sp = np.zeros(3, orc.SPHERE)
    mt = np.zeros(2, orc.MATERIAL)
    sp["center"][:, :3] = [(0, 3, 0), (4, 2, 1), (-3, 5, -2)]
    sp["radius"] = (0.5, 1.0, 0.25)
    sp["material_idx"] = 1
    s = N.Lights(E.Emission({1: (1.0, 1.0, 1.0)}, spheres=sp, materials=mt)).sample(P, Nn, u[:, 0], u[:, 1], u[:, 2])
    # a sphere's far side is hidden by the sphere itself: the tracer's occlusion, here by geometry (the light's own normal faces away)
    c = sp["center"][s["prim"], :3].astype(np.float64)
    front = np.einsum("ij,ij->i", s["q"].astype(np.float64) - c, p - s["q"].astype(np.float64)) > 0
    g = np.where(s["lit"] & front, s["G"], 0).astype(np.float64)
    want = sum((r / np.linalg.norm(cc - p)) ** 2 * (n @ (cc - p)) / np.linalg.norm(cc - p) for cc, r in zip(sp["center"][:, :3].astype(np.float64), sp["radius"].astype(np.float64)))
    z = (g.mean() - want) / (g.std() / np.sqrt(k))
    print(f"spheres: {g.mean():.6g} against {want:.6g}, z {z:.2f}")
    assert abs(z) <= 5.0
    # two triangle lights of different areas and tilts
    tr = np.zeros(2, orc.TRIANGLE)
    tr["v0"] = [(-1, 2, -1), (2, 1.5, 0)]
    tr["e1"] = [(2, 0, 0), (0, 1, 1.5)]
    tr["e2"] = [(0, 0.5, 2), (1.5, 0.25, 0)]
    tr["material_idx"] = 1
    s = N.Lights(E.Emission({1: (1.0, 1.0, 1.0)}, triangles=tr, materials=mt)).sample(P, Nn, u[:, 0], u[:, 1], u[:, 2])
    assert s["lit"].all()
    g = s["G"].astype(np.float64)
    want = sum(polygon_form_factor(p, n, [t["v0"], t["v0"] + t["e1"], t["v0"] + t["e2"]]) for t in tr.astype(tr.dtype))
    z = (g.mean() - want) / (g.std() / np.sqrt(k))
    print(f"triangles: {g.mean():.6g} against {want:.6g}, z {z:.2f}")
    assert abs(z) <= 5.0


# ---------------------------------------------------------------- the interface without a device
def test_flag_and_bindings(W):
    assert W.FLAG_NEE == 1 << 15 and "FLAG_NEE" in W.__all__
    hdr = open(os.path.join(ROOT, "include", "wfpt.h")).read()
    assert "WFPT_FLAG_NEE = 1u << 15" in hdr
    for name in ("wfpt_nee_light_count", "wfpt_nee_timing_ms", "wfpt_sample_lights"):
        assert name in W.abi_symbols() and hasattr(W.lib(), name)
    for name in ("nee_light_count", "nee_timing", "sample_lights"):
        assert callable(getattr(W.PathTracer, name))
