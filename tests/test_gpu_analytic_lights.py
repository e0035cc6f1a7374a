"""Analytic lights (WFPT_FLAG_ANALYTIC_LIGHTS, include/wfpt.h "Analytic lights") on the GPU.

The two samplers and whole renders are compared bit for bit with tests/analytic_lights_ref.py: nee_ref's and mis_ref's restatements with
the selection over emitters and analytic lights, Nf in nf's place and the point, spot and directional branch. The restatement of a
(scene, RNG mode, MIS) is rendered once and shared by the loops compared with it."""
import numpy as np
import pytest

import analytic_lights_ref as A
import emission_ref as E
import nee_ref as N
import retire_ref as RR
import test_gpu_nee as G
import texture_ref as T
from helpers import make_oracle
from test_analytic_lights_host import primary_hits  # (the lamp scene at its 48 x 32)
from test_gpu_nee import assert_bits, bits, compare, light, mesh_inputs, mesh_tracer, shirley_scene

pytestmark = pytest.mark.gpu

F = np.float32
SW, SH, MW, MH, MAXW = 160, 96, 120, 72, 6  # test_gpu_nee.py's Shirley and mesh sizes
MESH_COLOURS = {1: (2.0, 1.0, 0.5)}
COS_IN, COS_OUT = 0.9, 0.6
# one point, one spot and one directional light
SHIRLEY_MIX = np.concatenate([A.point((0.5, 3.0, 2.0), (20.0, 10.0, 5.0)),
                              A.spot((3.0, 5.0, 3.0), (-3.0, -5.0, -3.0), (60.0, 60.0, 90.0), COS_IN, COS_OUT),
                              A.directional((-0.4, -1.0, -0.3), (1.0, 0.9, 0.7))])
MESH_MIX = np.concatenate([A.point((0.0, 0.0, 12.0), (40.0, 20.0, 10.0)),
                           A.spot((8.0, 8.0, 15.0), (-8.0, -8.0, -15.0), (300.0, 300.0, 450.0), COS_IN, COS_OUT),
                           A.directional((0.2, -0.3, -1.0), (1.0, 0.9, 0.7))])
SUN = A.directional((0.3, -1.0, 0.2), (2.0, 1.5, 1.0))


@pytest.fixture(scope="module")
def W(gpu):
    return gpu


@pytest.fixture(scope="module")
def O(orc):
    return orc


def flags_of(W, names, mis=False, analytic=True):
    f = W.FLAG_EMISSION | W.FLAG_NEE | (W.FLAG_MIS if mis else 0) | (W.FLAG_ANALYTIC_LIGHTS if analytic else 0)
    for n in (names.split("|") if names else []):
        f |= getattr(W, "FLAG_" + n)
    return f


def as_lights(W, lights):
    return np.asarray(lights).astype(W.LIGHT)


def mesh_oracles(O, w, h, **kw):
    tris, mt, nodes, cam, ip, vw = mesh_inputs(O, w, h)
    o = O.Oracle(w, h, np.zeros(1, O.SPHERE), mt, nodes, cam, ip, vw, triangles=tris, **kw)
    shadow = O.Oracle(w, h, np.zeros(1, O.SPHERE), mt, nodes, cam, ip, vw, triangles=tris)
    return tris, mt, o, shadow


_REFS = {}


def reference(O, scene, rng, mis, spp=2):
    """the restatement's render of `scene` with its light mix and its emitters: computed once, shared, never changed"""
    key = (scene, rng, mis, spp)
    if key not in _REFS:
        if scene == "shirley":
            sp, mt, colours = shirley_scene(O)
            em = E.Emission(colours, spheres=sp, materials=mt)
            o, shadow = O.shirley_oracle(SW, SH, max_wavefronts=MAXW, rng_mode=rng), O.shirley_oracle(SW, SH)
            r = A.render_with_lights(o, shadow, em, SHIRLEY_MIX, mis=mis, spp=spp, parts=True)
        else:
            tris, mt, o, shadow = mesh_oracles(O, MW, MH, max_wavefronts=MAXW, rng_mode=rng)
            em = E.Emission(MESH_COLOURS, triangles=tris, materials=mt)
            r = A.render_with_lights(o, shadow, em, MESH_MIX, mis=mis, spp=spp, parts=True)
        assert r["stats"]["light_samples"] > 0
        for a in r.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _REFS[key] = r
    return _REFS[key]


# ---------------------------------------------------------------- the samplers
def edge_rows(rows, lights):
    """caller rows at the selection's edges and receivers at the lights' own singular places: exactly at a position, and on the inner and
    the outer edge of the spot's cone (one unit down the cone's surface, facing the spot)"""
    rows[4:9, 6] = (np.nan, -0.5, 2.0, 1.0, 1 - 2.0 ** -24)  # beside sampler_rows' own 0, 1 - 2^-24, 1.0
    st = A.stored(lights)
    n_all = 64
    for j, l in enumerate(st):
        if l["type"] == A.DIRECTIONAL:
            continue
        base = 16 + 8 * j
        rows[base:base + 4, :3] = l["position"]  # dist2 = 0, whichever light the draw picks
        rows[base:base + 4, 6] = np.linspace(0.0, 0.999, 4)
        if l["type"] == A.SPOT:
            a = l["direction"].astype(np.float64)
            t = np.cross(a, (0.0, 1.0, 0.0))
            t /= np.linalg.norm(t)
            for k, c in enumerate((l["cos_inner"], l["cos_outer"])):
                d = float(c) * a + np.sqrt(1.0 - float(c) ** 2) * t
                rows[base + 4 + k, :3] = l["position"] + d
                rows[base + 4 + k, 3:6] = -d
                rows[base + 4 + k, 6] = np.nan  # placeholder: set by the caller to the spot's own slot
    assert base + 8 <= n_all
    return rows


def check_samplers(O, pt, lights, shadow, rows, n_prims, mis, what):
    got = pt.sample_lights(rows)
    want, s = lights.sample_rows(shadow, rows)
    G.check_sampler(O, got, s, rows, shadow, what)  # q, primitive, e_q G, occlusion, and its non-vacuity conditions
    assert_bits(got, want, what + ": wfpt_sample_lights")
    picked = set(s["prim"][s["prim"] < 0].tolist())
    assert picked == {-1, -2, -3} and (s["prim"] >= 0).sum() > len(rows) // 10, what + ": the rows do not reach every kind of light"
    sun = s["prim"] == -3
    assert np.isinf(s["dist"][sun]).all() and (got[sun, 7] != 0).any() and (s["lit"][sun] & (got[sun, 7] == 0)).any(), what + ": the sun"
    spot = s["prim"] == -2
    assert (s["lit"][spot]).any() and (~s["lit"][spot]).any(), what + ": the spot"
    if not mis:
        return
    got = pt.sample_lights_mis(rows)
    want = lights.sample_rows_mis(shadow, rows)
    assert got.shape == (len(rows), 12)
    assert_bits(got, want, what + ": wfpt_sample_lights_mis")
    an = s["prim"] < 0
    assert (want[an & s["lit"], 10] == 1).all() and (want[an, 8] == 0).all() and (want[an & s["lit"], 9] > 0).all()
    assert ((want[~an, 10] > 0) & (want[~an, 10] < 1)).any()
    rng = np.random.default_rng(12)
    hits = np.concatenate([rng.standard_normal((500, 6)) * 3, rng.random((500, 1)) * 4, rng.integers(-2, n_prims + 2, (500, 1))], 1).astype(F)
    hits[:len(lights.list[:200]), 7] = lights.list[:200]  # emitters among them
    gw, ww = pt.mis_hit_weight(hits), lights.hit_weight_rows(hits)
    both_nan = np.isnan(gw) & np.isnan(ww)  # (a NaN's payload is not part of the contract)
    assert_bits(np.where(both_nan, F(0), gw), np.where(both_nan, F(0), ww), what + ": wfpt_mis_hit_weight")
    assert (gw[:, 2] < 1).any() and (gw[:, 2] == 1).any(), what


@pytest.mark.parametrize("mis", [False, True])
@pytest.mark.parametrize("loop", ["", "EXACT_TRAVERSAL", "NO_LDS_SCENE", "NO_LDS_SCENE|BINARY_BVH"])
def test_samplers_equal_the_restatement(W, O, loop, mis):
    k = 3000
    sp, mt, colours = shirley_scene(O)
    pt = W.shirley_path_tracer(64, 48, max_wavefronts=2, flags=flags_of(W, loop, mis))
    light(pt, colours)
    pt.set_lights(as_lights(W, SHIRLEY_MIX))
    lights = A.AnalyticLights(E.Emission(colours, spheres=sp, materials=mt), SHIRLEY_MIX)
    assert lights.n == 6 and pt.nee_light_count() == 3 and pt.analytic_light_count() == 3
    rows = edge_rows(G.sampler_rows((0.0, 1.0, 0.0), k, 5), SHIRLEY_MIX)
    rows[np.isnan(rows[:, 6]) & (np.arange(k) >= 16), 6] = (3 + 1 + 0.5) / 6  # the cone-edge receivers pick the spot, light 4 of 6
    check_samplers(O, pt, lights, O.shirley_oracle(64, 48), rows, len(sp), mis, f"spheres {loop}")
    pt.close()
    tris, mt, nodes, cam, ip, vw = mesh_inputs(O, 64, 48)
    pt = mesh_tracer(W, 64, 48, max_wavefronts=2, flags=flags_of(W, loop, mis))
    light(pt, MESH_COLOURS)
    pt.set_lights(as_lights(W, MESH_MIX))
    lights = A.AnalyticLights(E.Emission(MESH_COLOURS, triangles=tris, materials=mt), MESH_MIX)
    shadow = O.Oracle(64, 48, np.zeros(1, O.SPHERE), mt, nodes, cam, ip, vw, triangles=tris)
    rows = edge_rows(G.sampler_rows((0.0, 0.0, 0.0), k, 6), MESH_MIX)
    rows[np.isnan(rows[:, 6]) & (np.arange(k) >= 16), 6] = (lights.n_l + 1 + 0.5) / lights.n
    # the mesh's emitters outnumber the three lights by hundreds: half the rows draw among the analytic lights
    rows[k // 2:, 6] = (lights.n_l + np.random.default_rng(3).random(k - k // 2) * 3) / lights.n
    check_samplers(O, pt, lights, shadow, rows, len(tris), mis, f"mesh {loop}")
    pt.close()


def test_samplers_work_with_no_emitter(W, O):
    """N > 0 with n_l = 0: the samplers answer, wfpt_mis_hit_weight still needs an emitter"""
    sp, mt, _ = shirley_scene(O)
    pt = W.shirley_path_tracer(64, 48, max_wavefronts=2, flags=flags_of(W, "", True))
    rows = G.sampler_rows((0.0, 1.0, 0.0), 1000, 5)
    with pytest.raises(W.WfptError):
        pt.sample_lights(rows)
    pt.set_lights(as_lights(W, SHIRLEY_MIX))
    lights = A.AnalyticLights(A.no_emission(spheres=sp, materials=mt), SHIRLEY_MIX)
    shadow = O.shirley_oracle(64, 48)
    assert_bits(pt.sample_lights(rows), lights.sample_rows(shadow, rows)[0], "no emitter: wfpt_sample_lights")
    assert_bits(pt.sample_lights_mis(rows), lights.sample_rows_mis(shadow, rows), "no emitter: wfpt_sample_lights_mis")
    with pytest.raises(W.WfptError) as e:
        pt.mis_hit_weight(np.zeros((4, 8), F))
    assert e.value.status == -1
    pt.close()


# ---------------------------------------------------------------- renders, bit for bit
@pytest.mark.parametrize("mis", [False, True])
@pytest.mark.parametrize("rng", [0, 1])
@pytest.mark.parametrize("loop", ["", "UNFUSED", "NO_LDS_SCENE", "NO_LDS_SCENE|NO_REFILL"])
def test_shirley_equals_restatement(W, O, loop, rng, mis):
    spp = 2
    _, _, colours = shirley_scene(O)
    pt = W.shirley_path_tracer(SW, SH, max_wavefronts=MAXW, rng_mode=rng, flags=flags_of(W, loop, mis) | W.FLAG_DENOISE)
    light(pt, colours)
    pt.set_lights(as_lights(W, SHIRLEY_MIX))
    pt.render(spp)
    compare(pt, reference(O, "shirley", rng, mis), spp, SW, SH, f"shirley {loop} rng {rng} mis {mis}")
    pt.close()


@pytest.mark.parametrize("mis", [False, True])
@pytest.mark.parametrize("rng", [0, 1])
@pytest.mark.parametrize("loop", ["", "UNFUSED", "NO_LDS_SCENE", "NO_LDS_SCENE|NO_REFILL"])
def test_mesh_equals_restatement(W, O, loop, rng, mis):
    spp = 2
    pt = mesh_tracer(W, MW, MH, max_wavefronts=MAXW, rng_mode=rng, flags=flags_of(W, loop, mis))
    light(pt, MESH_COLOURS)
    pt.set_lights(as_lights(W, MESH_MIX))
    pt.render(spp)
    compare(pt, reference(O, "mesh", rng, mis), spp, MW, MH, f"mesh {loop} rng {rng} mis {mis}")
    pt.close()


def test_the_lights_change_the_image_and_mis_weighs_only_the_emitters(W, O):
    _, _, colours = shirley_scene(O)
    sp, mt, _ = shirley_scene(O)
    em = E.Emission(colours, spheres=sp, materials=mt)
    plain = N.render_with_nee(O.shirley_oracle(SW, SH, max_wavefronts=MAXW), O.shirley_oracle(SW, SH), em, spp=2)
    assert not np.array_equal(bits(plain), bits(reference(O, "shirley", 0, False)["acc"])), "the lights change nothing"
    assert not np.array_equal(bits(reference(O, "shirley", 0, True)["acc"]), bits(reference(O, "shirley", 0, False)["acc"]))


# ---------------------------------------------------------------- a sun and no emissive material
@pytest.mark.parametrize("mis", [False, True])
def test_sun_only_lights_the_lamp_scene_and_the_blocker_casts_a_black_shadow(W, O, mis):
    """The lamp scene at 48 x 32, 2 spp, nothing emits. One wavefront: `emitted` is then the direct term alone, and the device's
    accumulated image, thr + emitted, equals the restatement's bit for bit; the restatement's `emitted` is black under the blocker."""
    w, h, spp = 48, 32, 2
    inputs = N.lamp_inputs(O, w, h, blocker=True)
    em = A.no_emission(spheres=inputs[0], materials=inputs[1])
    sun_up = A.directional((0.0, -1.0, 0.0), (2.0, 1.5, 1.0))  # straight down: the blocker's shadow lies under it, mid-frame
    for maxw in (1, 4):
        pt = G.lamp_tracer(W, inputs, w, h, max_wavefronts=maxw, miss_floor=0, flags=flags_of(W, "", mis) | W.FLAG_ENVIRONMENT)
        pt.set_environment(N.black_env())
        pt.set_lights(as_lights(W, sun_up))
        assert pt.nee_light_count() == 0 and pt.analytic_light_count() == 1
        pt.render(spp)
        o = make_oracle(O, inputs, w, h, max_wavefronts=maxw, miss_floor=0)
        r = A.render_with_lights(o, make_oracle(O, inputs, w, h), em, sun_up, mis=mis, spp=spp, env=N.black_env(), parts=True)
        compare(pt, r, spp, w, h, f"sun only, {maxw} wavefronts, mis {mis}")
        assert pt.emission_timing()[1] == 0 and r["stats"]["light_samples"] > 0
        pt.close()
        plain = G.lamp_tracer(W, inputs, w, h, max_wavefronts=maxw, miss_floor=0, flags=flags_of(W, "", mis, False) | W.FLAG_ENVIRONMENT)
        plain.set_environment(N.black_env())
        plain.render(spp)
        assert not np.array_equal(bits(plain.accumulated()), bits(r["acc"])), "the sun changes nothing"
        plain.close()
        if maxw == 1:  # the blocker (radius 0.4 about the y axis) under a vertical sun: every ground sample inside its cylinder is black
            ground = int(np.argmax(inputs[0]["radius"]))
            dark = 0
            for k in range(spp):
                pix, prim, p = primary_hits(O, inputs, 1 + k)
                rad = np.hypot(p[:, 0], p[:, 2])
                umbra, open_ = pix[(prim == ground) & (rad < 0.36)], pix[(prim == ground) & (rad > 0.44)]
                assert not r["emitted"][k][umbra].any(), "the blocker's shadow is not black"
                assert (r["emitted"][k][open_] > 0).all() and len(open_) > 1000, "the ground beside the shadow is not lit"
                dark += len(umbra)
            assert dark >= 3, dark


# ---------------------------------------------------------------- the same bits however the samples are scheduled
@pytest.mark.parametrize("mis", [False, True])
def test_same_bits_across_batches_stage_loop_split_shade_and_shards(W, O, mis):
    w, h, spp = 100, 60, 130  # no multiple of 8 either way; 128 + a remainder
    _, _, colours = shirley_scene(O)
    kw = dict(max_wavefronts=5, miss_floor=0, rng_mode=W.RNG_PIXEL)

    def tracer(w, h, loop="", **more):
        pt = W.shirley_path_tracer(w, h, flags=flags_of(W, loop, mis), **kw, **more)
        light(pt, colours)
        pt.set_lights(as_lights(W, SHIRLEY_MIX))
        return pt

    base = None
    for loop, batch in [("", 1), ("", 16), ("", 128), ("SPLIT_SHADE", 0), ("UNFUSED", 16)]:
        pt = tracer(w, h, loop, batch=batch)
        pt.render(spp)
        if base is None:
            base = pt.accumulated()
        else:
            assert_bits(pt.accumulated(), base, f"loop {loop} batch {batch}")
        pt.close()
    for world in (2, 3):
        full = np.zeros((((h + 7) // 8) * 8, w, 3), F)
        for r in range(world):
            pt = tracer(w, h, tile_rank=r, tile_world=world)
            pt.render(spp)
            b = pt.accumulated().reshape(-1, 8, w, 3)
            pt.close()
            for j in range(b.shape[0]):
                y0 = (j * world + r) * 8
                full[y0:y0 + 8] = b[j]
        assert_bits(full[:h].reshape(-1, 3), base, f"{world} band-sharded contexts")
    w8, h8 = 96, 56  # the host-driven stage loop: whole tiles only
    pt = tracer(w8, h8)
    for _ in range(3):
        pt.run()
    host = pt.accumulated()
    pt.close()
    pt = tracer(w8, h8)
    pt.render(3)
    assert_bits(host, pt.accumulated(), "host-driven stage loop")
    pt.close()


@pytest.mark.parametrize("mis", [False, True])
def test_textured_emitter_and_retire_beside_the_lights(W, O, mis):
    w, h, spp, maxw = 64, 48, 2, 4
    sp, mt, colours = shirley_scene(O)
    lamps = sorted(colours)
    slots = {0: (G.random_tex(64, 32, 1), {"scale": (3.0, 2.0), "offset": (0.25, -0.5)})}
    bind = {lamps[0]: 0}
    pt = W.shirley_path_tracer(w, h, max_wavefronts=maxw, flags=flags_of(W, "", mis) | W.FLAG_TEXTURES)
    pt.set_texture(0, slots[0][0], **slots[0][1])
    light(pt, colours)
    pt.set_lights(as_lights(W, SHIRLEY_MIX))
    pt.bind_texture(lamps[0], 0)
    pt.render(spp)
    em = E.Emission(colours, spheres=sp, materials=mt)
    tx = T.Textures(spheres=sp, materials=mt, slots=slots, bind=bind)
    r = A.render_with_lights(O.shirley_oracle(w, h, max_wavefronts=maxw), O.shirley_oracle(w, h), em, SHIRLEY_MIX, mis=mis, tx=tx, spp=spp, parts=True)
    compare(pt, r, spp, w, h, f"textured emitter, mis {mis}")
    pt.close()
    pt = W.shirley_path_tracer(w, h, max_wavefronts=maxw, flags=flags_of(W, "RETIRE", mis))
    pt.set_termination(roulette_start=1, q_min=0.25)
    light(pt, colours)
    pt.set_lights(as_lights(W, SHIRLEY_MIX))
    pt.render(spp)
    o = RR.Retiring(O.shirley_oracle(w, h, max_wavefronts=maxw), roulette_start=1, q_min=0.25)
    r = A.render_with_lights(o, O.shirley_oracle(w, h), em, SHIRLEY_MIX, mis=mis, spp=spp, parts=True, termination=o)
    assert_bits(pt.accumulated(), r["acc"], f"retire, mis {mis}")
    assert sum(map(sum, o.retired)) > 0
    pt.close()


# ---------------------------------------------------------------- no analytic light: the unflagged context
@pytest.mark.parametrize("mis", [False, True])
@pytest.mark.parametrize("emitters", [False, True])
def test_no_analytic_light_is_the_unflagged_context_and_clear_makes_a_fresh_one(W, O, mis, emitters):
    w, h, spp = 100, 60, 8
    _, _, colours = shirley_scene(O)
    res = {}
    for analytic in (False, True):
        pt = W.shirley_path_tracer(w, h, max_wavefronts=5, flags=flags_of(W, "", mis, analytic))
        if emitters:
            light(pt, colours)
        pt.render(spp)
        acc = pt.accumulated()
        _, launches = pt.render_timed(spp)
        res[analytic] = (acc, launches, pt.totals(), pt.nee_timing()[1], pt.emission_timing()[1])
        if analytic:
            assert pt.analytic_light_count() == 0 and len(pt.lights()) == 0
            if not emitters:
                assert pt.nee_timing() == (0.0, 0) and pt.emission_timing() == (0.0, 0)
            pt.set_lights(as_lights(W, SHIRLEY_MIX))
            assert pt.analytic_light_count() == 3
            pt.render(spp)
            assert not np.array_equal(bits(pt.accumulated()), bits(acc))
            pt.set_lights(None)
            assert pt.analytic_light_count() == 0
            pt.render(spp)
            assert_bits(pt.accumulated(), acc, "after set and clear")
        pt.close()
    assert_bits(res[True][0], res[False][0], "no analytic light")
    assert np.array_equal(res[True][1], res[False][1]) and np.array_equal(res[True][2], res[False][2])
    assert res[True][3:] == res[False][3:], "the connect and emission launch counts"


# ---------------------------------------------------------------- what keeps the lights
def test_scene_updates_and_resizes_keep_the_lights_and_get_returns_them_normalised(W, O):
    w, h, spp = 64, 48, 2
    pt = mesh_tracer(W, w, h, max_wavefronts=4, flags=flags_of(W, ""), max_window_size=128 * 80)
    light(pt, MESH_COLOURS)
    given = as_lights(W, MESH_MIX)
    pt.set_lights(given)
    want = A.stored(MESH_MIX)
    got = pt.lights()
    assert got.dtype == W.LIGHT and got.tobytes() == want.astype(W.LIGHT).tobytes(), "wfpt_get_lights: not the stored lights"
    ln = np.linalg.norm(got["direction"][1:].astype(np.float64), axis=1)
    assert np.abs(ln - 1).max() < 1e-6 and not np.array_equal(got["direction"], given["direction"])
    n = W.C.c_uint32(0)  # (a short buffer gets its part, the count is whole; both pointers may be NULL)
    one = np.zeros(1, W.LIGHT)
    assert W.lib().wfpt_get_lights(pt.handle, one.ctypes.data_as(W.C.c_void_p), 1, W.C.byref(n)) == 0 and n.value == 3
    assert one.tobytes() == got[:1].tobytes() and W.lib().wfpt_get_lights(pt.handle, None, 0, None) == 0
    scene = W.Scene.random_mesh(5000, 1)
    scene.triangles["e1"] *= F(5.0)
    scene.triangles["e2"] *= F(5.0)
    pt.update_scene(W.Scene.random_mesh(3000, 1))
    assert pt.analytic_light_count() == 3
    pt.update_scene(scene)
    pt.render_parameters.set_viewport((120, 72))
    pt.update_buffers()
    assert pt.lights().tobytes() == got.tobytes()
    pt.render(spp)
    fresh = mesh_tracer(W, 120, 72, max_wavefronts=4, flags=flags_of(W, ""))
    light(fresh, MESH_COLOURS)
    fresh.set_lights(given)
    fresh.render(spp)
    assert_bits(pt.accumulated(), fresh.accumulated(), "after two scene updates and a resize")
    plain = mesh_tracer(W, 120, 72, max_wavefronts=4, flags=flags_of(W, "", analytic=False))
    light(plain, MESH_COLOURS)
    plain.render(spp)
    assert not np.array_equal(bits(plain.accumulated()), bits(pt.accumulated())), "the lights were lost"
    for p in (pt, fresh, plain):
        p.close()


# ---------------------------------------------------------------- refusals
def bad_lights(W):
    """(what, lights) for every invalid argument of wfpt_set_lights"""
    def one(**fields):
        l = as_lights(W, SHIRLEY_MIX)
        for k, v in fields.items():
            name, j = k.rsplit("_", 1)
            l[name][int(j)] = v
        return l
    inf, nan = np.inf, np.nan
    return [("too many", np.tile(as_lights(W, SHIRLEY_MIX), 342)[:W.MAX_LIGHTS + 1]),
            ("an unknown type", one(type_0=3)),
            ("a point's position is not finite", one(position_0=(0.0, inf, 0.0))),
            ("a spot's position is not finite", one(position_1=(nan, 0.0, 0.0))),
            ("a colour is not finite", one(colour_2=(1.0, inf, 1.0))),
            ("a colour is NaN", one(colour_0=(nan, 1.0, 1.0))),
            ("a colour is negative", one(colour_1=(1.0, 1.0, -0.5))),
            ("a spot's direction is not finite", one(direction_1=(1.0, nan, 0.0))),
            ("a sun's direction is not finite", one(direction_2=(inf, 0.0, 0.0))),
            ("a spot's direction has length 0", one(direction_1=(0.0, 0.0, 0.0))),
            ("a sun's direction has length 0", one(direction_2=(0.0, -0.0, 0.0))),
            ("cos_outer = cos_inner", one(cos_outer_1=COS_IN)),
            ("cos_outer > cos_inner", one(cos_outer_1=0.95)),
            ("cos_inner > 1", one(cos_inner_1=1.5)),
            ("cos_outer < -1", one(cos_outer_1=-1.5)),
            ("cos_inner is NaN", one(cos_inner_1=nan))]


def test_refusals_leave_the_context_as_it_was(W, O):
    w, h = 48, 32
    base = W.FLAG_EMISSION | W.FLAG_NEE | W.FLAG_ANALYTIC_LIGHTS
    for flags in (W.FLAG_ANALYTIC_LIGHTS, W.FLAG_EMISSION | W.FLAG_ANALYTIC_LIGHTS,  # without WFPT_FLAG_NEE (which needs WFPT_FLAG_EMISSION)
                  base | W.FLAG_ENVIRONMENT | W.FLAG_ENV_NEE, base | W.FLAG_ENVIRONMENT | W.FLAG_ENV_NEE | W.FLAG_ENV_MIS, base | W.FLAG_LIGHT_POWER):
        with pytest.raises(W.WfptError) as e:
            W.shirley_path_tracer(w, h, max_wavefronts=4, flags=flags)
        assert "WFPT_FLAG_ANALYTIC_LIGHTS" in str(e.value)  # (PathTracer reports every failed wfpt_create* alike: the reason names the rule)
    for extra in ("MIS", "TEXTURES", "ENVIRONMENT", "RETIRE", "ADAPTIVE", "AOV", "DENOISE"):  # the combinations the header promises
        W.shirley_path_tracer(w, h, max_wavefronts=4, flags=flags_of(W, extra)).close()
    _, _, colours = shirley_scene(O)
    # a context without the flag
    plain = W.shirley_path_tracer(w, h, max_wavefronts=4, flags=flags_of(W, "", analytic=False))
    light(plain, colours)
    plain.render(2)
    want = plain.accumulated()
    for call in (lambda: plain.set_lights(as_lights(W, SHIRLEY_MIX)), plain.lights, plain.analytic_light_count):
        with pytest.raises(W.WfptError) as e:
            call()
        assert e.value.status == -1
    assert_bits(plain.accumulated(), want, "a refused call resets nothing")
    plain.close()
    # the class-binned loop
    binned = W.shirley_path_tracer(200, 120, max_wavefronts=4, rng_mode=W.RNG_PIXEL, flags=base | W.FLAG_BINNING)
    assert binned.loop_kind == "fused_binned"
    with pytest.raises(W.WfptError) as e:
        binned.set_lights(as_lights(W, SHIRLEY_MIX))
    assert e.value.status == -4 and binned.loop_kind == "fused_binned" and binned.analytic_light_count() == 0
    binned.close()
    # every invalid argument, on a context that holds lights and has rendered
    pt = W.shirley_path_tracer(w, h, max_wavefronts=4, flags=flags_of(W, ""))
    light(pt, colours)
    pt.set_lights(as_lights(W, SHIRLEY_MIX))
    pt.render(2)
    want, held = pt.accumulated(), pt.lights().tobytes()
    for what, lights in bad_lights(W):
        with pytest.raises(W.WfptError) as e:
            pt.set_lights(lights)
        assert e.value.status == -1, what
        assert pt.lights().tobytes() == held, what
        assert_bits(pt.accumulated(), want, what + ": a refused call resets nothing")
    assert W.lib().wfpt_set_lights(pt.handle, None, 2) == -1
    pt.render(2)
    fresh = W.shirley_path_tracer(w, h, max_wavefronts=4, flags=flags_of(W, ""))
    light(fresh, colours)
    fresh.set_lights(as_lights(W, SHIRLEY_MIX))
    fresh.render(4)
    assert_bits(pt.accumulated(), fresh.accumulated(), "the context renders as before")
    # the fields a type does not read are not validated
    odd = as_lights(W, SHIRLEY_MIX)
    odd["position"][2] = (np.nan, np.inf, 0.0)
    odd["direction"][0] = (np.nan, 0.0, 0.0)
    odd["cos_inner"][0], odd["cos_outer"][2] = 7.0, np.nan
    pt.set_lights(odd)
    pt.render(4)
    assert_bits(pt.accumulated(), fresh.accumulated(), "the fields a type does not read")
    fresh.close()
    pt.close()
