"""Multiple importance sampling (WFPT_FLAG_MIS) without a GPU: the numpy restatement (tests/mis_ref.py) on the oracle against the closed
forms of the lamp scene and of the near-lamp scene, its mutations, the two weights' sum, the identity the scatter's density rests on, and
the zero cases. The scenes have a convex ground under a black environment, so only one-bounce light exists (tests/test_nee_host.py)."""
import os

import numpy as np
import pytest

import emission_ref as E
import mis_ref as M
import nee_ref as N
from helpers import make_oracle
from mis_ref import NEAR
from nee_ref import LAMP, PI
from test_nee_host import camera_rays, closed_form, hit_sphere, pixel_mean

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W_, H_, SPP = 160, 120, 16


@pytest.fixture(scope="module")
def W():
    import wavefront_path_tracer_amd as W
    return W


def render(orc, inputs, e, kind="mis", spp=SPP, **mut):
    em = E.Emission({1: e}, spheres=inputs[0], materials=inputs[1])
    o = make_oracle(orc, inputs, W_, H_, max_wavefronts=4, miss_floor=0, rng_mode=1)
    if kind == "plain":
        return E.render_with_emission(o, em, spp=spp, env=N.black_env(), parts=True)
    shadow = make_oracle(orc, inputs, W_, H_)
    if kind == "nee":
        return N.render_with_nee(o, shadow, em, spp=spp, env=N.black_env(), parts=True)
    return M.render_with_mis(o, shadow, em, spp=spp, env=N.black_env(), parts=True, **mut)


MUTATIONS = {"both strategies at full weight": dict(no_wl=True, no_wb=True), "wb applied but wl not": dict(no_wl=True),
             "pl without nf": dict(no_nf=True), "pb taken as len / pi": dict(pb_of_len=lambda ln: ln / PI)}


# ---------------------------------------------------------------- the lamp scene (the far, small lamp of tests/test_nee_host.py)
def test_lamp_scene_matches_the_closed_form(orc):
    """Measured (160 x 120, 16 spp, 10 000+ ground pixels): z = -0.32 (0.0208843 against 0.0209095, standard error 7.90e-05), footprint bound
    0.27 standard errors; the bound is test_nee_host's 5 standard errors + footprint. Both strategies at full weight: z = 30.7, outside.
    On this scene the lamp is small and far and wb is about 2 %, so a wrong weight moves the mean by 2 % at the most: at 16 spp wl dropped
    gives z = 4.67 and pb = len / pi z = 4.49, inside the bound. The bound is in standard errors, so these are rendered at 64 spp, where
    they fall outside it: z = 10.7 and 10.1 (footprint 0.53 and 0.51 standard errors). The scene's light list has one entry, and with
    nf = 1 `pl without nf` is the true render bit for bit (asserted): test_lamp_scene_pl_without_nf gives the scene a second light."""
    inputs = N.lamp_inputs(orc, W_, H_)
    r = render(orc, inputs, LAMP["e"])
    want, bound, ok = closed_form(inputs, W_, H_, LAMP["lamp_r"])
    assert ok.sum() > 10000
    mean, se = pixel_mean(r, SPP, ok)
    print(f"closed form {want[ok].mean():.6g}, restatement {mean:.6g}, se {se:.3g}, z {(mean - want[ok].mean()) / se:.2f}")
    assert abs(mean - want[ok].mean()) <= 5.0 * se + bound[ok].mean()
    assert not r["image"].any()
    for name, mut in MUTATIONS.items():
        spp = SPP if name in ("both strategies at full weight", "pl without nf") else 64
        wrong = render(orc, inputs, LAMP["e"], spp=spp, **mut)
        m, s = pixel_mean(wrong, spp, ok)
        print(f"{name}, {spp} spp: {m:.6g}, se {s:.3g}, z {(m - want[ok].mean()) / s:.2f}, footprint {bound[ok].mean() / s:.2f} se")
        if name == "pl without nf":
            assert np.array_equal(wrong["acc"].view(np.uint32), r["acc"].view(np.uint32)), "nf = 1: dividing by it or not is the same operation"
        else:
            assert abs(m - want[ok].mean()) > 5.0 * s + bound[ok].mean(), name + " passes the closed-form check"


def test_lamp_scene_pl_without_nf(orc):
    """`pl without nf` can only show where the light list is longer than one. The lamp scene with a second sphere of the lamp's material
    buried in the ground at half its radius: it lies below every ground point's tangent plane, so it lights nothing and the closed form
    stands, but nf = 2. At 128 spp (the mutation moves the mean by under 2 %) the true render stays inside test_nee_host's bound and the
    mutation falls outside it. Measured: true z = -0.31, `pl without nf` z = -9.65, footprint 0.50 and 0.51 standard errors."""
    spp = 128
    inputs = N.lamp_inputs(orc, W_, H_)
    want, bound, ok = closed_form(inputs, W_, H_, LAMP["lamp_r"])
    buried = inputs[0][:1].copy()
    buried["center"][0, :3] = (0.0, -0.5 * LAMP["ground_r"], 0.0)
    buried["radius"][0] = LAMP["lamp_r"]
    buried["material_idx"][0] = 1
    buried["material_type"][0] = inputs[1]["material_type"][1]
    sp, nodes = orc.build_bvh(np.concatenate([inputs[0], buried]))
    two = (sp, inputs[1], nodes) + tuple(inputs[3:])
    z = {}
    for name, mut in (("true", {}), ("pl without nf", MUTATIONS["pl without nf"])):
        m, s = pixel_mean(render(orc, two, LAMP["e"], spp=spp, **mut), spp, ok)
        z[name] = (abs(m - want[ok].mean()), 5.0 * s + bound[ok].mean())
        print(f"two lights, {name}, {spp} spp: {m:.6g}, se {s:.3g}, z {(m - want[ok].mean()) / s:.2f}, footprint {bound[ok].mean() / s:.2f} se")
    assert z["true"][0] <= z["true"][1]
    assert z["pl without nf"][0] > z["pl without nf"][1]


# ---------------------------------------------------------------- the near-lamp scene
def near_closed_form(inputs, w, h):
    """test_nee_host.closed_form for the near-lamp scene (float64): a sphere light wholly above the tangent plane gives the irradiance
    pi L (r / d)^2 cos(theta), so a ground pixel expects albedo * e * (r / d)^2 * cos(theta); the same footprint average, bound and mask,
    the mask clear of 1.25 lamp radii around the lamp's image."""
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    sp = inputs[0]
    g = int(np.argmax(sp["radius"]))
    lamp = int(np.flatnonzero((sp["material_idx"] == 1) & (sp["center"][:, 1] > 0))[0])
    gc, gr = sp["center"][g, :3].astype(np.float64), float(sp["radius"][g])
    lc, lr = sp["center"][lamp, :3].astype(np.float64), float(sp["radius"][lamp])

    def at(dx, dy):
        o, d = camera_rays(inputs, w, h, xs + dx, ys + dy)
        t = hit_sphere(o, d, gc, gr)
        good = np.isfinite(t) & ~np.isfinite(hit_sphere(o, d, lc, 1.25 * lr))
        p = o + np.where(np.isfinite(t), t, 0.0)[..., None] * d
        n = (p - gc) / gr
        v = lc - p
        dist = np.linalg.norm(v, axis=-1)
        above = (n * v).sum(-1)
        rgb = np.asarray(NEAR["albedo"])[None, None] * np.asarray(NEAR["e"])[None, None] * ((lr / dist) ** 2 * above / dist)[..., None]
        return 0.2126 * rgb[..., 0] + 0.7152 * rgb[..., 1] + 0.0722 * rgb[..., 2], good & (above > lr)

    centre, ok = at(0, 0)
    corners = []
    for dx, dy in ((-1, -1), (1, -1), (-1, 1), (1, 1)):
        v, good = at(dx, dy)
        corners.append(v)
        ok &= good
    disk = [at(np.sqrt((i + 0.5) / 4) * np.cos(2 * np.pi * (k + 0.5) / 8), np.sqrt((i + 0.5) / 4) * np.sin(2 * np.pi * (k + 0.5) / 8))[0]
            for i in range(4) for k in range(8)]
    return np.mean(disk, axis=0).reshape(-1), np.abs(np.mean(corners, axis=0) - centre).reshape(-1), ok.reshape(-1)


def variance_sum(r, spp, sel):
    s1, s2 = r["s1"].astype(np.float64)[sel], r["s2"].astype(np.float64)[sel]
    m = s1 / spp
    return float((np.maximum(s2 / spp - m * m, 0.0) * spp / (spp - 1)).sum())


def test_near_lamp_closed_form_and_variance(orc):
    """The lamp of radius 1 with a gap of 0.05 over the radius-1000 ground. Measured (160 x 120, 16 spp, 15 677 ground pixels): closed form
    0.0914628, MIS 0.0914055 (standard error 4.59e-04, z = -0.12, footprint bound 0.24 standard errors). Sums of the per-pixel sample
    variance: MIS 826.8, EMISSION|NEE 4537.5, EMISSION alone 1998.3 -- 5.5 and 2.4 times more."""
    inputs = M.near_lamp_inputs(orc, W_, H_)
    want, bound, ok = near_closed_form(inputs, W_, H_)
    assert ok.sum() > 10000
    r = render(orc, inputs, NEAR["e"])
    mean, se = pixel_mean(r, SPP, ok)
    print(f"closed form {want[ok].mean():.6g}, MIS {mean:.6g}, se {se:.3g}, z {(mean - want[ok].mean()) / se:.2f}, footprint {bound[ok].mean() / se:.2f} se")
    assert abs(mean - want[ok].mean()) <= 4.0 * se
    v_mis = variance_sum(r, SPP, ok)
    v_nee = variance_sum(render(orc, inputs, NEAR["e"], kind="nee"), SPP, ok)
    v_plain = variance_sum(render(orc, inputs, NEAR["e"], kind="plain"), SPP, ok)
    print(f"variance sums: MIS {v_mis:.6g}, EMISSION|NEE {v_nee:.6g}, EMISSION {v_plain:.6g}")
    assert v_mis < v_nee and v_mis < v_plain


def test_near_lamp_mutations(orc):
    """Each mutation against the near-lamp closed form, 4 standard errors as above. `pl without nf` needs a list of two lights: the scene
    with a second emitter buried in the ground, which lights nothing (the true render of that scene must still pass). Measured z-scores:
    both at full weight 70.3, wl dropped 35.3, pb = len / pi 20.4; with the buried light: true -0.54, pl without nf -23.4."""
    inputs = M.near_lamp_inputs(orc, W_, H_)
    want, _, ok = near_closed_form(inputs, W_, H_)
    for name, mut in MUTATIONS.items():
        if name == "pl without nf":
            continue
        m, s = pixel_mean(render(orc, inputs, NEAR["e"], **mut), SPP, ok)
        print(f"{name}: z {(m - want[ok].mean()) / s:.2f}")
        assert abs(m - want[ok].mean()) > 4.0 * s, name
    two = M.near_lamp_inputs(orc, W_, H_, buried=True)
    want2, _, ok2 = near_closed_form(two, W_, H_)
    m, s = pixel_mean(render(orc, two, NEAR["e"]), SPP, ok2)
    print(f"two lights, true: z {(m - want2[ok2].mean()) / s:.2f}")
    assert abs(m - want2[ok2].mean()) <= 4.0 * s
    m, s = pixel_mean(render(orc, two, NEAR["e"], no_nf=True), SPP, ok2)
    print(f"two lights, pl without nf: z {(m - want2[ok2].mean()) / s:.2f}")
    assert abs(m - want2[ok2].mean()) > 4.0 * s


# ---------------------------------------------------------------- the weights
def light_sets(orc):
    mt = np.zeros(2, orc.MATERIAL)
    sp = np.zeros(3, orc.SPHERE)
    sp["center"][:, :3] = [(0, 3, 0), (4, 2, 1), (-3, 5, -2)]
    sp["radius"] = (0.5, 1.0, 0.25)
    sp["material_idx"] = 1
    tr = np.zeros(3, orc.TRIANGLE)
    tr["v0"] = [(-1, 2, -1), (2, 1.5, 0), (-3, 3, 1)]
    tr["e1"] = [(2, 0, 0), (0, 1, 1.5), (0.5, 0, 1)]
    tr["e2"] = [(0, 0.5, 2), (1.5, 0.25, 0), (0, 1, 0.25)]
    tr["material_idx"] = 1
    e = {1: (1.0, 2.0, 3.0)}
    return [N.Lights(E.Emission(e, spheres=sp[:1].copy(), materials=mt)), N.Lights(E.Emission(e, spheres=sp, materials=mt)),
            N.Lights(E.Emission(e, triangles=tr[:1].copy(), materials=mt)), N.Lights(E.Emission(e, triangles=tr, materials=mt))]


SUM_BOUND = 2.0 ** -21  # the next power of two above the worst |wl + wb - 1| measured below: 4.02e-07 (4 light sets x 12 000 draws)


def test_weights_sum_to_one(orc):
    """A connect sample (p, n) -> q replayed as the scattered ray that would have found q: o = p, d = (2 cos_s) w, t = dist / (2 cos_s), so
    |d| / 2 = cos_s and o + t d = q to rounding. wl of the connect side plus wb of the hit side is 1 to rounding only."""
    rng = np.random.default_rng(5)
    worst = 0.0
    for L in light_sets(orc):
        k = 12000
        u = rng.random((k, 3)).astype(F)
        p = (rng.standard_normal((k, 3)) * 2).astype(F)
        p[:, 1] = -np.abs(p[:, 1])
        n = np.broadcast_to(np.array([0.0, 1.0, 0.0], F), (k, 3))
        s = L.sample(p, n, u[:, 0], u[:, 1], u[:, 2])
        s["n"] = n
        _, pb, wl = M.light_densities(L, p, s)
        lit = s["lit"]
        assert lit.sum() > k // 4
        with np.errstate(all="ignore"):
            cos_s = pb * PI
            d = (F(2) * cos_s)[:, None] * s["w"]
            t = s["dist"] / (F(2) * cos_s)
            rows = np.concatenate([p, d, t[:, None], s["prim"].astype(F)[:, None]], 1)[lit]
        out = M.hit_weight_rows(L, rows)
        gap = np.abs((wl[lit].astype(np.float64) + out[:, 2].astype(np.float64)) - 1.0)
        worst = max(worst, float(gap.max()))
    print(f"worst |wl + wb - 1| = {worst:.3g}, bound {SUM_BOUND:.3g}")
    assert worst <= SUM_BOUND


ID_ABS, ID_REL = 2.0 ** -14, 2.0 ** -14  # next powers of two above the measured 5.35e-05 and 3.39e-05 (306 729 scatters)


def test_the_identity_of_the_scatter(orc):
    """Over every Lambertian scatter of the lamp render (160 x 120, 16 spp, 4 wavefronts): 0.5 |d| against n.d / |d|. n and r are unit
    vectors to rounding only, and the gap grows as d gets short (the shortest measured: 0.0021)."""
    inputs = N.lamp_inputs(orc, W_, H_)
    sc = []
    render(orc, inputs, LAMP["e"], scatters=sc)
    n, d = np.concatenate([a for a, _ in sc]), np.concatenate([b for _, b in sc])
    assert len(d) > 100000
    ln = np.sqrt(N.dot3(d, d))
    c = N.dot3(n, d) / ln
    gap = np.abs(F(0.5) * ln - c)
    rel = (gap / c)[ln > 0.1]
    print(f"{len(d)} scatters: worst absolute gap {gap.max():.3g}, worst relative gap for len > 0.1 {rel.max():.3g}, shortest {ln.min():.3g}")
    assert gap.max() <= ID_ABS and rel.max() <= ID_REL


def test_zero_cases(orc):
    mt = np.zeros(2, orc.MATERIAL)
    sp = np.zeros(2, orc.SPHERE)
    sp["center"][:, :3] = [(0, 3, 0), (2, 2, 0)]
    sp["radius"] = (0.0, 1.0)
    sp["material_idx"] = 1
    L = N.Lights(E.Emission({1: (1.0, 1.0, 1.0)}, spheres=sp, materials=mt))
    # a zero-radius emitter; a hit seen edge-on (cos_l = 0: the ray grazes the sphere's pole along its tangent); a non-emitter; NaN
    rows = np.array([[0, 0, 0, 0, 3, 0, 1, 0], [0, 3, 0, 1, 0, 0, 2, 1], [0, 0, 0, 0, 1, 0, 1, 7], [0, 0, 0, 0, 1, 0, 1, np.nan]], F)
    out = M.hit_weight_rows(L, rows)
    assert (out[:, 2] == 1).all(), out
    assert out[1, 3] == 0 and out[1, 0] == 0, "cos_l = 0 must give pl = 0"
    assert (out[2:, [0, 3]] == 0).all() and np.isfinite(out[2:, 1]).all()
    tr = np.zeros(1, orc.TRIANGLE)
    tr["v0"], tr["e1"], tr["e2"] = (5, 5, 5), (1, 2, 3), (2, 4, 6)  # no area
    tr["material_idx"] = 1
    Lt = N.Lights(E.Emission({1: (1.0, 1.0, 1.0)}, triangles=tr, materials=mt))
    assert M.hit_weight_rows(Lt, np.array([[0, 0, 0, 1, 1, 1, 5, 0]], F))[0, 2] == 1


def test_full_weight_where_the_flag_is_zero_and_no_emitter(orc):
    """A primary hit on the lamp and a hit after metal take full weight: the lamp scene with the mirror renders the lamp's own pixels and
    the mirror's as nee_ref does, bit for bit (only ground pixels differ). With no emitter the render is the unflagged one."""
    inputs = N.lamp_inputs(orc, W_, H_, lamp_r=0.5, mirror=True)
    a, b = render(orc, inputs, LAMP["e"], spp=4), render(orc, inputs, LAMP["e"], kind="nee", spp=4)
    o = make_oracle(orc, inputs, W_, H_, max_wavefronts=1, miss_floor=0, rng_mode=1)
    first = E.render_with_emission(o, E.Emission({}, spheres=inputs[0], materials=inputs[1]), spp=1, env=N.black_env(), parts=True)["first_prim"][0]
    sp = inputs[0]
    lamp = int(np.flatnonzero(sp["material_idx"] == 1)[0])
    metal = int(np.flatnonzero(sp["material_idx"] == 3)[0])
    # a sample that sees the lamp directly, or in the mirror (fuzz 0, albedo 1), is the lamp's colour exactly: the flag is 0 there
    seen = (b["emitted"] == np.asarray(LAMP["e"], F)).all(axis=2)
    assert seen[:, first == lamp].any() and seen[:, first == metal].any()
    assert np.array_equal(a["emitted"][seen], b["emitted"][seen])
    assert not np.array_equal(a["acc"], b["acc"])
    none_a, none_b = render(orc, inputs, (0.0, 0.0, 0.0), spp=2), render(orc, inputs, (0.0, 0.0, 0.0), kind="plain", spp=2)
    assert np.array_equal(none_a["acc"].view(np.uint32), none_b["acc"].view(np.uint32))


# ---------------------------------------------------------------- the interface without a device
def test_flag_and_bindings(W):
    assert W.FLAG_MIS == 1 << 17 and "FLAG_MIS" in W.__all__
    hdr = open(os.path.join(ROOT, "include", "wfpt.h")).read()
    assert "WFPT_FLAG_MIS = 1u << 17" in hdr
    for name in ("wfpt_sample_lights_mis", "wfpt_mis_hit_weight"):
        assert name in W.abi_symbols() and hasattr(W.lib(), name)
    for name in ("sample_lights_mis", "mis_hit_weight"):
        assert callable(getattr(W.PathTracer, name))
