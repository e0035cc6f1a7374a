"""Analytic lights (WFPT_FLAG_ANALYTIC_LIGHTS) without a GPU: the numpy restatement (tests/analytic_lights_ref.py) on the oracle against
the closed form of a point, a directional and a spot light over the lamp scene's ground, and the restatement's four mutations.

The scene: nee_ref.lamp_inputs with no material emitting, a black environment (nee_ref.black_env), miss_floor = 0. The ground sphere is
convex, so a ground point sees no other ground point, and the one other object, the former lamp sphere, is made black (albedo 0) and is
kept out of every checked shadow ray's way: the point and the spot light hang below it, and the sun stands so low behind the scene that
the sphere's shadow falls in front of the frame's bottom edge (asserted per sample below). Light then arrives by the direct term alone,
and the value of every sample whose primary hit is on the ground is albedo * e * cos_s * fall / (pi * dist2) (the sun: albedo * e *
cos_s / pi), evaluated here in float64 at that sample's own hit point and normal.

"Convex" holds for the sphere, not quite for its f32 hit points: a point rounded to just inside the sphere, left by a scattered ray that
grazes the tangent plane, meets the ground again beyond t_min (one sample in 1527 of the first frame), and that second hit is lit too.
So the direct term is checked where it is exact by construction -- the `emitted` plane of a one-wavefront render, every ground sample,
none left out -- and the four-wavefront render's value is then required to be that plane bit for bit on all but 1 % of the samples.

The tolerance is relative 1e-5: about a dozen f32 roundings of 6e-8 each give 1e-6, and the margin is a factor of ten. Inside the spot's
falloff the smoothstep amplifies the error of s = (cd - cos_outer) / (cos_inner - cos_outer), about 1e-6 absolute for this cone, by
6 (1 - s) / (s (3 - 2 s)): below 6 for s >= 0.3, where the relative bound is asserted as it stands, and without bound as s -> 0, where
the same 1e-5 is asserted relative to the unattenuated value instead (fall's absolute error is 6 s (1 - s) ds <= 1.5e-6)."""
import numpy as np
import pytest

import analytic_lights_ref as A
import nee_ref as N
from helpers import make_oracle
from nee_ref import LAMP

F = np.float32
W_, H_, SPP, MAXW = 48, 32, 2, 4
ALBEDO = np.asarray(LAMP["albedo"], np.float64)
GC, GR = np.array([0.0, -LAMP["ground_r"], 0.0]), LAMP["ground_r"]
LC, LR = np.asarray(LAMP["lamp_c"], np.float64), LAMP["lamp_r"]
E_POINT, E_SUN, E_SPOT = (6.0, 3.0, 12.0), (2.0, 1.5, 1.0), (8.0, 8.0, 4.0)
POINT_AT = (0.5, 1.0, 0.25)  # below the black sphere (its lowest point is at y = 1.75)
SUN_DIR = (0.0, -0.3, 1.0)  # travels down and towards the camera: the sphere's shadow lands around z = +6.7, the frame ends at z = +4.1
SPOT_AT, SPOT_DIR, COS_IN, COS_OUT = (0.0, 1.5, 0.0), (0.0, -2.0, 0.0), float(np.cos(np.radians(25.0))), float(np.cos(np.radians(45.0)))


@pytest.fixture(scope="module")
def scene(orc):
    inputs = N.lamp_inputs(orc, W_, H_)
    inputs[1]["albedo"][1, :3] = 0.0  # the former lamp: black, it reflects nothing onto the ground
    return inputs


def oracles(orc, inputs, maxw):
    return make_oracle(orc, inputs, W_, H_, max_wavefronts=maxw, miss_floor=0), make_oracle(orc, inputs, W_, H_)


def run(orc, inputs, lights, mis=False, spp=SPP, maxw=MAXW, **mutations):
    o, shadow = oracles(orc, inputs, maxw)
    em = A.no_emission(spheres=inputs[0], materials=inputs[1])
    al = A.AnalyticLights(em, lights, **mutations)
    r = A.render_with_lights(o, shadow, em, al, mis=mis, spp=spp, env=N.black_env(), parts=True)
    o.close()
    shadow.close()
    return r


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def primary_hits(orc, inputs, frame):
    """(pixel, primitive, hit point as shade computes it) of the primary hits of the sample of frame `frame`: the oracle's own generate_rays
    and extend, as transport_ref.render starts every sample"""
    o = make_oracle(orc, inputs, W_, H_, max_wavefronts=MAXW, miss_floor=0)
    gx, gy = (W_ + 7) // 8, (H_ + 7) // 8
    o.set_frame(frame, 0)
    o.reset_image()
    o.set_counters([0, 0, gx * gy * 64])
    o.generate_rays(gx, gy, True)
    n_rays = int(o.counters()[2])
    o.extend(*orc.workgroup_size_64(gx * gy * 64))
    rays, hits = o.rays(n_rays), o.hits(int(o.counters()[1]))
    ridx = hits["ray_idx"].astype(np.int64)
    p = rays["origin"][ridx, :3].astype(F) + hits["t"].astype(F)[:, None] * rays["direction"][ridx, :3].astype(F)
    out = rays["pixel_idx"][ridx].astype(np.int64), hits["sphere_idx"].astype(np.int64), p.astype(np.float64)
    o.close()
    return out


def check_closed_form(orc, inputs, lights, expect, what, min_lit):
    """every sample whose primary hit is on the ground: the direct term == expect(p, n) within the module's tolerance. expect returns
    (value (k, 3), unattenuated value (k, 3), s (k,) -- 1 outside a falloff --, w (k, 3) the direction to the light, the distance to it)"""
    ground = int(np.argmax(inputs[0]["radius"]))
    r1, r = run(orc, inputs, lights, maxw=1), run(orc, inputs, lights)
    checked = lit = same = 0
    zones = set()
    for k in range(SPP):
        pix, prim, p = primary_hits(orc, inputs, 1 + k)
        sel = prim == ground
        pix, p = pix[sel], p[sel]
        n = (p - GC) / np.linalg.norm(p - GC, axis=1, keepdims=True)
        want, full, s, w, reach = expect(p, n)
        # no checked shadow ray comes near the black sphere: the distance of its centre from the segment between the point and the light
        along = np.clip(((LC - p) * w).sum(1), 0.0, reach)
        off = np.linalg.norm((LC - p) - along[:, None] * w, axis=1)
        assert ((off > 1.5 * LR) | ~(want > 0).any(axis=1)).all(), what + ": a shadow ray passes the black sphere"
        got = r1["emitted"][k][pix].astype(np.float64)
        same += int((bits(r["value"][k][pix]) == bits(r1["emitted"][k][pix])).all(axis=1).sum())
        steep = (s > 0) & (s < 0.3)
        tol = np.where(steep[:, None], 1e-5 * full, 1e-5 * want)
        err = np.abs(got - want)
        worst = float((err / np.maximum(tol, 1e-300)).max())
        print(f"{what}: sample {k}: {len(pix)} ground samples, {int((want > 0).any(axis=1).sum())} lit, worst error / tolerance {worst:.3f}")
        assert (err <= tol).all(), (what, k, worst)
        checked += len(pix)
        lit += int((want > 0).any(axis=1).sum())
        zones |= {"inner"} if (s >= 1).any() else set()
        zones |= {"falloff"} if ((s > 0) & (s < 1)).any() else set()
        zones |= {"outside"} if (s <= 0).any() else set()
    assert checked > W_ * H_ and lit >= min_lit, (what, checked, lit)
    assert same >= 0.99 * checked and r["stats"]["light_samples"] > 0, (what, same, checked)
    return zones


def test_point_light_matches_the_closed_form(orc, scene):
    c, e = np.asarray(POINT_AT, np.float64), np.asarray(E_POINT, np.float64)

    def expect(p, n):
        v = c - p
        d2 = (v * v).sum(1)
        w = v / np.sqrt(d2)[:, None]
        cos_s = np.maximum((n * w).sum(1), 0.0)
        val = ALBEDO * e * (cos_s / (np.pi * d2))[:, None]
        return val, val, np.ones(len(p)), w, np.sqrt(d2)

    check_closed_form(orc, scene, A.point(POINT_AT, E_POINT), expect, "point", 2000)


def test_directional_light_matches_the_closed_form(orc, scene):
    a = np.asarray(SUN_DIR, np.float64)
    a /= np.linalg.norm(a)
    e = np.asarray(E_SUN, np.float64)

    def expect(p, n):
        w = np.broadcast_to(-a, p.shape)
        cos_s = np.maximum((n * w).sum(1), 0.0)
        val = ALBEDO * e * (cos_s / np.pi)[:, None]
        return val, val, np.ones(len(p)), w, np.full(len(p), np.inf)

    check_closed_form(orc, scene, A.directional(SUN_DIR, E_SUN), expect, "sun", 2000)


def test_spot_light_matches_the_closed_form_in_its_three_zones(orc, scene):
    c, e = np.asarray(SPOT_AT, np.float64), np.asarray(E_SPOT, np.float64)
    a = np.asarray(SPOT_DIR, np.float64) / np.linalg.norm(SPOT_DIR)
    ci, co = np.float64(F(COS_IN)), np.float64(F(COS_OUT))  # the cosines as the f32 fields hold them

    def expect(p, n):
        v = c - p
        d2 = (v * v).sum(1)
        w = v / np.sqrt(d2)[:, None]
        cos_s = np.maximum((n * w).sum(1), 0.0)
        s = np.clip((-(a * w).sum(1) - co) / (ci - co), 0.0, 1.0)
        full = ALBEDO * e * (cos_s / (np.pi * d2))[:, None]
        return full * (s * s * (3.0 - 2.0 * s))[:, None], full, s, w, np.sqrt(d2)

    zones = check_closed_form(orc, scene, A.spot(SPOT_AT, SPOT_DIR, E_SPOT, COS_IN, COS_OUT), expect, "spot", 200)
    assert zones == {"inner", "falloff", "outside"}, zones


# ---------------------------------------------------------------- the restatement can fail: each mutation changes the image
MIX = np.concatenate([A.point(POINT_AT, E_POINT), A.spot(SPOT_AT, SPOT_DIR, E_SPOT, COS_IN, COS_OUT),
                      A.directional((0.3, -1.0, 0.2), E_SUN)])  # a high sun: the sphere's shadow lies in the frame


@pytest.mark.parametrize("mutation,mis", [("nf_emitters_only", False), ("weigh_analytic", True), ("sun_window", False), ("no_falloff", False)])
def test_each_mutation_changes_the_image(orc, scene, mutation, mis):
    want = run(orc, scene, MIX, mis=mis, spp=1)["acc"]
    assert want.any()
    got = run(orc, scene, MIX, mis=mis, spp=1, **{mutation: True})["acc"]
    assert not np.array_equal(bits(got), bits(want)), mutation + " changes nothing"


def test_mis_leaves_analytic_samples_unweighed(orc, scene):
    """wl = 1: with no emitter, the weighing context renders the bits of the one that does not weigh"""
    assert np.array_equal(bits(run(orc, scene, MIX, mis=True, spp=1)["acc"]), bits(run(orc, scene, MIX, mis=False, spp=1)["acc"]))


def test_stored_directions_are_normalised_once_in_f32():
    s = A.stored(np.concatenate([A.directional((3.0, -4.0, 12.0), E_SUN), A.point(POINT_AT, E_POINT), A.spot(SPOT_AT, SPOT_DIR, E_SPOT, COS_IN, COS_OUT)]))
    ln = np.sqrt(F(F(F(3.0) * F(3.0) + F(4.0) * F(4.0)) + F(12.0) * F(12.0)))
    assert np.array_equal(s["direction"][0], np.array([3.0, -4.0, 12.0], F) / ln)
    assert np.array_equal(s["direction"][1], np.zeros(3, F)) and np.array_equal(s["direction"][2], np.array([0.0, -1.0, 0.0], F))
