"""GGX microfacet metals (WFPT_FLAG_MICROFACET, include/wfpt.h "Microfacet metals") on the GPU.

The device's sampler and whole renders are compared bit for bit with tests/microfacet_ref.py: the numpy float32 restatement of steps 0-11
and of the per-hit record of step 12, driven through the oracle's stages. The scene is tests/test_gpu_shading_normals.py's: a 320-triangle
icosphere of radius 1 (Lambertian, fuzzy metal and glass by thirds) over a two-triangle ground, 3 samples, 4 wavefronts; the metal's
roughness is 0.3."""
import numpy as np
import pytest

import adaptive_ref as A
import emission_ref as E
import light_power_ref as P
import microfacet_ref as MF
import mis_ref as M
import retire_ref as RR
import shading_normals_ref as S
import texture_ref as T
import transport_ref
from helpers import assert_bits_or_nan
from test_gpu_shading_normals import FLOOR, LAMP_E, SIZES, SPP, WAVES, assert_bits, bits, flags_of, oracle_of, scene
from test_microfacet_host import ALPHAS, COSINES, cell, deviation, random_rows

pytestmark = pytest.mark.gpu

F = np.float32
METAL, ALPHA = 1, 0.3


@pytest.fixture(scope="module")
def W():
    import wavefront_path_tracer_amd as W
    return W


@pytest.fixture(scope="module")
def O():
    from oracle import oracle as O
    return O


def tracer(W, O, emitter, w, h, flags="", alphas={METAL: ALPHA}, table=False, microfacet=True, **kw):
    t, mt, n9, _, created = scene(O, emitter)
    sc = W.Scene(np.zeros(0, W.SPHERE), mt.copy(), triangles=created.copy())
    cc = W.CameraController(W.Camera((0.0, 1.0, 4.5), (0.0, -0.1, 0.0)), 40.0, 0.0, 10.0, 0.1, 100.0)
    kw.setdefault("max_wavefronts", WAVES)
    kw.setdefault("miss_floor", FLOOR)
    f = flags if isinstance(flags, int) else flags_of(W, flags)
    pt = W.PathTracer(sc, W.RenderParameters(cc, (w, h)), flags=(W.FLAG_MICROFACET if microfacet else 0) | f, **kw)
    assert np.array_equal(pt.scene.triangles, t), "the tracer's triangles are not in the oracle's order"
    if table:
        pt.set_triangle_normals(n9)
    for m, a in alphas.items():
        pt.set_roughness(m, a)
    return pt


def rough(O, emitter, w, h, alphas={METAL: ALPHA}, table=False, **kw):
    t, mt, n9, _, _ = scene(O, emitter)
    return MF.Rough(oracle_of(O, emitter, w, h, **kw), t, mt, alphas, S.Normals(t, n9) if table else None)


def plain_render(O, r, emitter=False, wrap=lambda o: o):
    """transport_ref.render of the Rough `r` with no other pass: an unbound texture table only makes the loop keep the throughput itself"""
    t, mt, _, _, _ = scene(O, emitter)
    with MF.rough_weights(r):
        return T.render_with_textures(wrap(r), T.Textures(triangles=t, materials=mt), spp=SPP)


def check(pt, want, o, what):
    assert_bits(pt.accumulated(), want, what)
    assert np.array_equal(pt.bounce_table(), o.bounce_table()), f"{what}: bounce table\n{pt.bounce_table()}\nvs\n{o.bounce_table()}"


# ---------------------------------------------------------------- 1. the sampler alone
def edge_rows():
    """(rows, may be NaN): back-facing d, cn == 0, alpha 1 and 1e-4, n = (0, 0, -1) and (0, 0, 1), u1 = 0 and u1 at the largest value
    rng_next_float yields (f32(2^32 - 1) * 2^-32 = 1), a NaN normal, F0 of 0 and 1 -- each over a few directions and draws"""
    rng = np.random.default_rng(5)
    k = 16
    d = rng.standard_normal((k, 3))
    n = rng.standard_normal((k, 3))
    n /= np.linalg.norm(n, axis=1)[:, None]
    u1, u2 = rng.random(k, dtype=F), rng.random(k, dtype=F)
    f0 = rng.uniform(0.0, 1.0, (k, 3))
    up = np.tile((0.0, 0.0, 1.0), (k, 1))
    facing = np.where((np.einsum("ij,ij->i", n, d) > 0)[:, None], -d, d)  # dot(n, wi) > 0
    top = F(np.uint32(0xFFFFFFFF)) * F(2.3283064365387e-10)
    assert top == 1.0
    flat = d.copy()
    flat[:, 2] = 0.0  # perpendicular to (0, 0, 1): cn is exactly 0
    parts = [MF.probe_rows(-facing, n, u1, u2, 0.3, f0), MF.probe_rows(flat, up, u1, u2, 0.3, f0), MF.probe_rows(facing, n, u1, u2, 1.0, f0),
             MF.probe_rows(facing, n, u1, u2, 1e-4, f0), MF.probe_rows(d, -up, u1, u2, 0.5, f0), MF.probe_rows(d, up, u1, u2, 0.5, f0),
             MF.probe_rows(facing, n, 0.0, u2, 0.3, f0), MF.probe_rows(facing, n, top, u2, 0.3, f0),
             MF.probe_rows(facing, n, u1, u2, 0.3, np.zeros((k, 3))), MF.probe_rows(facing, n, u1, u2, 0.3, np.ones((k, 3)))]
    nan = MF.probe_rows(facing, n, u1, u2, 0.3, f0)
    nan[:, 3 + np.arange(k) % 3] = np.nan
    rows = np.concatenate(parts + [nan])
    maybe = np.zeros(len(rows), bool)
    maybe[-k:] = True
    return rows, maybe


def test_sample_microfacet_equals_restatement(W, O):
    edges, maybe = edge_rows()
    rows = np.concatenate([random_rows(4096, 6), edges])
    maybe = np.concatenate([np.zeros(4096, bool), maybe])
    want = MF.sample_rows(rows)
    assert not np.isnan(want[~maybe]).any()
    state = want[4096:, 3].reshape(-1, 16)
    assert (state[1] == 2).all() and (state[10] == 2).all(), "cn == 0 and a NaN normal fall back"
    assert not (state[[0, 2, 3, 4, 5, 6, 7, 8, 9]] == 2).any() and (want[:4096, 3] == 0).sum() > 2048 and (want[:4096, 3] == 1).sum() > 100
    pt = tracer(W, O, False, 16, 16, alphas={})
    got = pt.sample_microfacet(rows)
    assert_bits(got[~maybe], want[~maybe], "finite rows")
    assert_bits_or_nan(got[maybe], want[maybe], "may-be-NaN rows")
    assert len(pt.sample_microfacet(np.zeros((0, 12), F))) == 0
    pt.close()


@pytest.fixture(scope="module")
def probe_tracer(W, O):
    pt = tracer(W, O, False, 16, 16, alphas={})
    yield pt
    pt.close()


@pytest.mark.parametrize("cn", COSINES)
@pytest.mark.parametrize("alpha", ALPHAS)
def test_the_device_mean_weight_is_the_directional_albedo(probe_tracer, alpha, cn):
    """the twelve cells of tests/test_microfacet_host.py through the probe: within 4 standard errors (those of the reference draws) of the
    quadrature"""
    rows, want, _ = cell(alpha, cn)
    _, se = deviation(MF.sample_rows(rows)[:, 4:7], want)
    got = probe_tracer.sample_microfacet(rows)[:, 4:7].astype(np.float64)
    z = (got.mean(axis=0) - want) / se
    print(f"alpha {alpha} cn {cn}: device mean {got.mean(axis=0)} quadrature {want} z {z}")
    assert (np.abs(z) < 4).all(), (alpha, cn, z)


# ---------------------------------------------------------------- 2. frames against the restatement
_refs = {}


def plain_reference(O, w, h, rng, **kw):
    key = (w, h, rng, tuple(sorted(kw.items())))
    if key not in _refs:
        r = rough(O, False, w, h, rng_mode=rng, **kw)
        _refs[key] = (plain_render(O, r), r)
        assert r.sampled > 100, "hardly a rough hit in the scene"
    return _refs[key]


@pytest.mark.parametrize("rng", [0, 1])
@pytest.mark.parametrize("loop", ["", "UNFUSED", "SPLIT_SHADE", "NO_LDS_SCENE"])
def test_loops_equal_restatement(W, O, loop, rng):
    w, h = SIZES["61x37"]
    want, o = plain_reference(O, w, h, rng)
    pt = tracer(W, O, False, w, h, loop, rng_mode=rng)
    assert pt.loop_kind == {"": "fused", "UNFUSED": "stages", "SPLIT_SHADE": "stages", "NO_LDS_SCENE": "refill"}[loop]
    pt.render(SPP)
    check(pt, want, o, f"{loop} rng {rng}")
    unflagged = oracle_of(O, False, w, h, rng_mode=rng).render(SPP)
    assert not np.array_equal(bits(want), bits(unflagged)), "the roughness changed nothing"
    pt.close()


@pytest.mark.parametrize("batch", [1, 3])
def test_batches_and_the_second_size_equal_restatement(W, O, batch):
    w, h = SIZES["64x64"]
    want, o = plain_reference(O, w, h, 0)
    pt = tracer(W, O, False, w, h, rng_mode=0, batch=batch)
    stage_ms, stage_launches = pt.render_timed(SPP)
    check(pt, want, o, f"64x64 batch {batch}")
    ms, launches = pt.microfacet_timing_ms()
    assert launches == (WAVES - 1) * (SPP // batch) and ms > 0.0, "one launch per batch before every shade step that scatters"
    pt.close()


def test_band_sharding_equals_restatement(W, O):
    w, h = SIZES["61x37"]
    for rank in range(2):
        r = rough(O, False, w, h, rng_mode=1, miss_floor=0, tile_rank=rank, tile_world=2)
        want = plain_render(O, r, wrap=A.Local)
        pt = tracer(W, O, False, w, h, rng_mode=1, miss_floor=0, tile_rank=rank, tile_world=2)
        pt.render(SPP)
        check(pt, want, r, f"rank {rank} of 2")
        pt.close()


@pytest.mark.parametrize("loop", ["", "UNFUSED", "NO_LDS_SCENE"])
def test_with_a_table_of_normals_equals_restatement(W, O, loop):
    """both features: every hit's record carries the shading normal, a rough hit samples about it (microfacet_kernel<true>)"""
    w, h = SIZES["61x37"]
    r = rough(O, False, w, h, table=True)
    want = plain_render(O, r)
    pt = tracer(W, O, False, w, h, "SHADING_NORMALS" + ("|" + loop if loop else ""), table=True)
    pt.render_timed(SPP)
    check(pt, want, r, f"SHADING_NORMALS {loop}")
    assert pt.shading_normal_timing()[1] == 0 and pt.microfacet_timing_ms()[1] > 0, "the microfacet pass takes the shading-normal pass's place"
    pt.set_roughness(METAL, 0.0)  # the table of normals alone: shading_normals_ref's frame
    t, mt, n9, _, _ = scene(O)
    so = S.Shaded(oracle_of(O, False, w, h), S.Normals(t, n9), mt)
    pt.render(SPP)
    check(pt, transport_ref.render(so, spp=SPP), so, f"the normals alone {loop}")
    pt.close()


def test_retire_equals_restatement(W, O):
    w, h = SIZES["61x37"]
    t, mt, _, _, _ = scene(O, True)
    inner = rough(O, True, w, h, rng_mode=1)
    o = RR.Retiring(inner, roulette_start=1, q_min=0.25)
    with MF.rough_weights(inner):
        want = E.render_with_emission(o, E.Emission({4: LAMP_E}, triangles=t, materials=mt), spp=SPP, termination=o)
    assert sum(sum(k) for k in o.retired) > 0 and inner.sampled > 100
    pt = tracer(W, O, True, w, h, "EMISSION|RETIRE", rng_mode=1)
    pt.set_emission(4, LAMP_E)
    pt.set_termination(1, 0.25)
    pt.render(SPP)
    check(pt, want, o, "retire")
    pt.close()


@pytest.mark.parametrize("power", [False, True])
def test_light_transport_equals_restatement(W, O, power):
    """EMISSION | NEE | MIS with a lamp: a rough hit is "specular" for the connect pass. power: WFPT_FLAG_LIGHT_POWER as well, which
    WFPT_FLAG_SHADING_NORMALS refuses and this flag accepts."""
    w, h = SIZES["61x37"]
    t, mt, _, _, _ = scene(O, True)
    o = rough(O, True, w, h, rng_mode=1, miss_floor=0)
    shadow = oracle_of(O, True, w, h)
    em = E.Emission({4: LAMP_E}, triangles=t, materials=mt)
    with MF.rough_weights(o):
        r = P.render_with_power(o, shadow, em, mis=True, spp=SPP, parts=True) if power else M.render_with_mis(o, shadow, em, spp=SPP, parts=True)
    assert r["stats"]["light_samples"] > 100 and o.sampled > 100
    flags = "EMISSION|NEE|MIS" + ("|LIGHT_POWER" if power else "")
    if power:
        with pytest.raises(W.WfptError):
            tracer(W, O, True, w, h, flags + "|SHADING_NORMALS", alphas={})
    pt = tracer(W, O, True, w, h, flags, rng_mode=1, miss_floor=0)
    pt.set_emission(4, LAMP_E)
    pt.render(SPP)
    check(pt, r["acc"], o, flags)
    pt.close()


def test_a_texture_on_the_metal_equals_restatement(W, O):
    w, h = SIZES["61x37"]
    t, mt, n9, _, _ = scene(O)
    uv = np.random.default_rng(8).uniform(-1.5, 2.5, (len(n9), 6)).astype(F)
    img = (np.random.default_rng(9).random((32, 48, 3)) * 1.2).astype(F)
    o = rough(O, False, w, h)
    with MF.rough_weights(o):
        want = T.render_with_textures(o, T.Textures(triangles=t, materials=mt, slots={0: (img, {})}, bind={METAL: 0, 3: 0}, uv=uv), spp=SPP)
    pt = tracer(W, O, False, w, h, "TEXTURES")
    pt.set_texture(0, img)
    pt.bind_texture(METAL, 0)
    pt.bind_texture(3, 0)
    pt.set_triangle_uvs(uv)
    pt.render(SPP)
    check(pt, want, o, "textures")
    pt.close()


# ---------------------------------------------------------------- 3. identity
@pytest.mark.parametrize("loop", ["", "UNFUSED", "NO_LDS_SCENE"])
def test_no_roughness_is_the_unflagged_context(W, O, loop):
    """the frame's bits and the launches: flag set and nothing else, a roughness on a material that is not metal, set then clear"""
    w, h = SIZES["61x37"]
    plain = tracer(W, O, False, w, h, loop, alphas={}, microfacet=False, batch=3)
    _, want_launches = plain.render_timed(SPP)
    want = plain.accumulated()
    assert_bits(want, oracle_of(O, False, w, h).render(SPP), "the unflagged context")
    plain.close()
    pt = tracer(W, O, False, w, h, loop, alphas={}, batch=3)
    _, launches = pt.render_timed(SPP)
    assert_bits(pt.accumulated(), want, "flag set, no roughness")
    assert np.array_equal(launches, want_launches) and pt.microfacet_timing_ms() == (0.0, 0)
    pt.set_roughness(0, 0.5)  # Lambertian: stored and inert
    assert pt.get_roughness(0) == 0.5
    pt.render(SPP)
    assert_bits(pt.accumulated(), want, "a roughness on a material that is not metal")
    pt.set_roughness(METAL, ALPHA)
    pt.render(SPP)
    assert not np.array_equal(bits(pt.accumulated()), bits(want))
    pt.clear_roughness()
    assert pt.get_roughness(0) == 0.0 and pt.get_roughness(METAL) == 0.0
    before = pt.microfacet_timing_ms()
    _, launches = pt.render_timed(SPP)
    assert_bits(pt.accumulated(), want, "set, then cleared")
    assert np.array_equal(launches, want_launches) and pt.microfacet_timing_ms() == before
    pt.close()


# ---------------------------------------------------------------- 4. scene updates, state and refusals
def test_update_scene_keeps_and_drops_alphas(W, O):
    w, h = SIZES["61x37"]
    t, mt, _, _, created = scene(O)
    want, o = plain_reference(O, w, h, 0)
    pt = tracer(W, O, False, w, h, rng_mode=0, alphas={METAL: ALPHA, 4: 0.75})
    pt.render(1)
    sp = np.zeros(1, W.SPHERE)
    sp["radius"] = 1.0
    with pytest.raises(W.WfptError):
        pt.update_scene(W.Scene(sp, mt.copy()))  # spheres, while an alpha is above 0
    pt.render(SPP - 1)
    check(pt, want, o, "after a refused update the render goes on")
    shuffled = created.copy()[::-1].copy()
    pt.update_scene(W.Scene(np.zeros(0, W.SPHERE), mt[:4].copy(), triangles=shuffled))  # four materials: index 4 goes
    assert pt.get_roughness(METAL) == F(ALPHA)
    with pytest.raises(W.WfptError):
        pt.get_roughness(4)
    pt.render(SPP)
    check(pt, want, o, "after an update to the same scene with four materials")
    pt.update_scene(W.Scene(np.zeros(0, W.SPHERE), mt.copy(), triangles=created.copy()))
    assert pt.get_roughness(METAL) == F(ALPHA) and pt.get_roughness(4) == 0.0, "a dropped alpha does not come back"
    pt.render(SPP)
    check(pt, want, o, "after an update back to five materials")
    pt.close()


def test_refusals_and_the_restart(W, O):
    w, h = 16, 16
    t, mt, _, _, created = scene(O)
    sphere = W.shirley_path_tracer(w, h, flags=W.FLAG_MICROFACET)
    for call in (lambda: sphere.set_roughness(0, 0.5), sphere.clear_roughness):
        with pytest.raises(W.WfptError) as e:
            call()
        assert e.value.status == -1
    assert sphere.get_roughness(0) == 0.0 and len(sphere.sample_microfacet(random_rows(4, 1))) == 4
    sphere.close()
    unflagged = tracer(W, O, False, w, h, alphas={}, microfacet=False)
    for call in (lambda: unflagged.set_roughness(METAL, 0.5), lambda: unflagged.get_roughness(METAL), unflagged.clear_roughness,
                 unflagged.microfacet_timing_ms, lambda: unflagged.sample_microfacet(np.zeros((1, 12), F))):
        with pytest.raises(W.WfptError) as e:
            call()
        assert e.value.status == -1
    unflagged.close()
    binned = tracer(W, O, False, 200, 120, "BINNING", alphas={}, rng_mode=W.RNG_PIXEL)
    assert binned.loop_kind == "fused_binned"
    with pytest.raises(W.WfptError) as e:
        binned.set_roughness(METAL, 0.5)
    assert e.value.status == -4
    binned.set_roughness(METAL, 0.0)  # (nothing the loop has no form of)
    binned.clear_roughness()
    assert binned.loop_kind == "fused_binned" and binned.get_roughness(METAL) == 0.0
    binned.close()
    pt = tracer(W, O, False, w, h)
    pt.render(2)
    before = pt.accumulated()
    for m, a in ((METAL, 1.5), (METAL, -0.25), (METAL, np.nan), (METAL, np.inf), (len(mt), 0.5)):
        with pytest.raises(W.WfptError) as e:
            pt.set_roughness(m, a)
        assert e.value.status == -1
    assert_bits(pt.accumulated(), before, "a refused call restarted the accumulation")
    assert pt.get_roughness(METAL) == F(ALPHA)
    pt.render(1)
    assert W.lib().wfpt_accumulated_samples(pt.handle) == 3
    pt.set_roughness(METAL, 0.5)
    assert W.lib().wfpt_accumulated_samples(pt.handle) == 0, "a set restarts the accumulation"
    pt.set_roughness(METAL, ALPHA)
    pt.render(3)
    fresh = tracer(W, O, False, w, h)
    fresh.render(3)
    assert_bits(pt.accumulated(), fresh.accumulated(), "after the restart the frames are a fresh context's")
    fresh.close()
    pt.close()
