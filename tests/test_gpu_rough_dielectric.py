"""GGX rough dielectrics (WFPT_FLAG_ROUGH_DIELECTRIC, include/wfpt.h "Rough dielectrics") on the GPU.

The device's sampler and whole renders are compared bit for bit with tests/rough_dielectric_ref.py: the numpy float32 restatement of steps
0-12 and of the retyped per-hit record of step 13, driven through the oracle's stages. The scene is tests/test_gpu_shading_normals.py's: a
320-triangle icosphere of radius 1 (Lambertian, fuzzy metal and glass of refraction index 1.5 by thirds) over a two-triangle ground, 3
samples, 4 wavefronts; the glass's and the metal's roughness are 0.3."""
import numpy as np
import pytest

import adaptive_ref as A
import emission_ref as E
import mis_ref as M
import retire_ref as RR
import rough_dielectric_ref as RD
import shading_normals_ref as S
import texture_ref as T
from helpers import assert_bits_or_nan
from test_gpu_microfacet import check, plain_render
from test_gpu_shading_normals import FLOOR, LAMP_E, SIZES, SPP, WAVES, assert_bits, bits, flags_of, oracle_of, scene
from test_rough_dielectric_host import ALPHAS, COSINES, SIDES, cell, deviation, random_rows

pytestmark = pytest.mark.gpu

F = np.float32
METAL, GLASS, ALPHA = 1, 2, 0.3
BOTH = {METAL: ALPHA, GLASS: ALPHA}


@pytest.fixture(scope="module")
def W():
    import wavefront_path_tracer_amd as W
    return W


@pytest.fixture(scope="module")
def O():
    from oracle import oracle as O
    return O


def tracer(W, O, emitter, w, h, flags="", alphas=BOTH, table=False, dielectric=True, **kw):
    t, mt, n9, _, created = scene(O, emitter)
    assert (t["material_type"][t["material_idx"] == GLASS] == 2).all() and (mt["refract_index"][GLASS] == F(1.5))
    sc = W.Scene(np.zeros(0, W.SPHERE), mt.copy(), triangles=created.copy())
    cc = W.CameraController(W.Camera((0.0, 1.0, 4.5), (0.0, -0.1, 0.0)), 40.0, 0.0, 10.0, 0.1, 100.0)
    kw.setdefault("max_wavefronts", WAVES)
    kw.setdefault("miss_floor", FLOOR)
    f = flags if isinstance(flags, int) else flags_of(W, flags)
    pt = W.PathTracer(sc, W.RenderParameters(cc, (w, h)), flags=W.FLAG_MICROFACET | (W.FLAG_ROUGH_DIELECTRIC if dielectric else 0) | f, **kw)
    assert np.array_equal(pt.scene.triangles, t), "the tracer's triangles are not in the oracle's order"
    if table:
        pt.set_triangle_normals(n9)
    for m, a in alphas.items():
        pt.set_roughness(m, a)
    return pt


def rough(O, emitter, w, h, alphas=BOTH, table=False, **kw):
    t, mt, n9, _, _ = scene(O, emitter)
    return RD.RoughGlass(oracle_of(O, emitter, w, h, **kw), t, mt, alphas, S.Normals(t, n9) if table else None)


def assert_all_four(r):
    assert r.glass_sampled > 100 and r.sampled > 100, (r.glass_sampled, r.sampled)
    assert all(v > 0 for v in r.counts.values()), r.counts


# ---------------------------------------------------------------- 1. the sampler alone
def edge_rows():
    """(rows, may be NaN): back-facing and front-facing d, cn == 0, alpha 1 and 1e-4, ior 1 (a refraction falls back), ior 1.5 from inside
    beyond the critical angle, u3 = 0 and u3 at the largest value rng_next_float yields (f32(2^32 - 1) * 2^-32 = 1), the same for u1, a
    NaN normal -- each over a few directions and draws"""
    rng = np.random.default_rng(5)
    k = 16
    d = rng.standard_normal((k, 3))
    n = rng.standard_normal((k, 3))
    n /= np.linalg.norm(n, axis=1)[:, None]
    u1, u2, u3 = rng.random(k, dtype=F), rng.random(k, dtype=F), rng.random(k, dtype=F)
    alb = rng.uniform(0.0, 1.0, (k, 3))
    up = np.tile((0.0, 0.0, 1.0), (k, 1))
    facing = np.where((np.einsum("ij,ij->i", n, d) > 0)[:, None], -d, d)  # dot(n, wi) > 0: from outside
    top = F(np.uint32(0xFFFFFFFF)) * F(2.3283064365387e-10)
    assert top == 1.0
    flat = d.copy()
    flat[:, 2] = 0.0  # perpendicular to (0, 0, 1): cn is exactly 0
    side = np.cross(n, rng.standard_normal((k, 3)))
    side /= np.linalg.norm(side, axis=1)[:, None]
    grazing = 0.3 * n + np.sqrt(1.0 - 0.09) * side  # leaves through the back at the macro cosine 0.3 < 0.745: beyond the critical angle
    parts = [RD.probe_rows(-facing, n, u1, u2, u3, 0.3, 1.5, alb), RD.probe_rows(facing, n, u1, u2, u3, 0.3, 1.5, alb),
             RD.probe_rows(flat, up, u1, u2, u3, 0.3, 1.5, alb), RD.probe_rows(facing, n, u1, u2, u3, 1.0, 1.5, alb),
             RD.probe_rows(facing, n, u1, u2, u3, 1e-4, 1.5, alb), RD.probe_rows(facing, n, u1, u2, top, 0.3, 1.0, alb),
             RD.probe_rows(grazing, n, u1, u2, u3, 0.3, 1.5, alb), RD.probe_rows(facing, n, u1, u2, 0.0, 0.3, 1.5, alb),
             RD.probe_rows(facing, n, u1, u2, top, 0.3, 1.5, alb), RD.probe_rows(facing, n, 0.0, u2, u3, 0.3, 1.5, alb),
             RD.probe_rows(facing, n, top, u2, u3, 0.3, 1.5, alb)]
    nan = RD.probe_rows(facing, n, u1, u2, u3, 0.3, 1.5, alb)
    nan[:, 3 + np.arange(k) % 3] = np.nan
    rows = np.concatenate(parts + [nan])
    maybe = np.zeros(len(rows), bool)
    maybe[-k:] = True
    return rows, maybe


def test_sample_rough_dielectric_equals_restatement(W, O):
    edges, maybe = edge_rows()
    rows = np.concatenate([random_rows(4096, 6), edges])
    maybe = np.concatenate([np.zeros(4096, bool), maybe])
    want = RD.sample_rows(rows)
    assert not np.isnan(want[~maybe]).any()
    state, arm = want[4096:, 3].reshape(-1, 16), want[4096:, 7].reshape(-1, 16)
    assert (state[2] == 2).all() and (state[5] == 2).all() and (state[11] == 2).all(), "cn == 0, ior 1 and a NaN normal fall back"
    assert (want[4096:][state.reshape(-1) == 2] == np.array([0, 0, 0, 2, 0, 0, 0, 0], F)).all()
    assert not (state[[0, 1, 3, 4, 6, 7, 8, 9, 10]] == 2).any()
    assert (arm[7] == 0).all() and (arm[8] == 1).all(), "u3 = 0 reflects, the largest u3 refracts (from outside nothing reflects totally)"
    assert (arm[6][state[6] == 0] == 0).sum() > 8, "beyond the critical angle most microfacets reflect totally"
    live = want[:4096, 3] == 0
    assert live.sum() > 2048 and (want[:4096, 3] == 1).sum() > 100 and (want[:4096, 7][live] == 1).sum() > 500 and (want[:4096, 7][live] == 0).sum() > 200
    pt = tracer(W, O, False, 16, 16, alphas={})
    got = pt.sample_rough_dielectric(rows)
    assert_bits(got[~maybe], want[~maybe], "finite rows")
    assert_bits_or_nan(got[maybe], want[maybe], "may-be-NaN rows")
    assert len(pt.sample_rough_dielectric(np.zeros((0, 16), F))) == 0
    pt.close()


@pytest.fixture(scope="module")
def probe_tracer(W, O):
    pt = tracer(W, O, False, 16, 16, alphas={})
    yield pt
    pt.close()


@pytest.mark.parametrize("cn", COSINES)
@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("side", SIDES)
def test_the_device_mean_weight_is_the_quadrature(probe_tracer, side, alpha, cn):
    """the cells of tests/test_rough_dielectric_host.py through the probe: within 4 standard errors (those of the reference draws) of the
    quadrature"""
    rows, want, _ = cell(alpha, cn, side)
    _, se = deviation(RD.sample_rows(rows)[:, 4], want)
    got = probe_tracer.sample_rough_dielectric(rows)[:, 4].astype(np.float64)
    z = (got.mean() - want) / se
    print(f"{side} alpha {alpha} cn {cn}: device mean {got.mean():.6f} quadrature {want:.6f} z {z:+.2f}")
    assert abs(z) < 4, (side, alpha, cn, z)


# ---------------------------------------------------------------- 2. frames against the restatement
_refs = {}


def plain_reference(O, w, h, rng, **kw):
    key = (w, h, rng, tuple(sorted(kw.items())))
    if key not in _refs:
        r = rough(O, False, w, h, rng_mode=rng, **kw)
        _refs[key] = (plain_render(O, r), r)
        assert_all_four(r)
    return _refs[key]


_metal_only = {}


def metal_only_frame(W, O, w, h, rng):
    """the WFPT_FLAG_MICROFACET-only context's frame with the same alphas: the glass alpha is inert there"""
    if (w, h, rng) not in _metal_only:
        pt = tracer(W, O, False, w, h, rng_mode=rng, dielectric=False)
        pt.render(SPP)
        _metal_only[(w, h, rng)] = pt.accumulated()
        pt.close()
    return _metal_only[(w, h, rng)]


@pytest.mark.parametrize("rng", [0, 1])
@pytest.mark.parametrize("loop", ["", "UNFUSED", "SPLIT_SHADE", "NO_LDS_SCENE"])
def test_loops_equal_restatement(W, O, loop, rng):
    w, h = SIZES["61x37"]
    want, o = plain_reference(O, w, h, rng)
    pt = tracer(W, O, False, w, h, loop, rng_mode=rng)
    assert pt.loop_kind == {"": "fused", "UNFUSED": "stages", "SPLIT_SHADE": "stages", "NO_LDS_SCENE": "refill"}[loop]
    pt.render(SPP)
    check(pt, want, o, f"{loop} rng {rng}")
    assert not np.array_equal(bits(want), bits(metal_only_frame(W, O, w, h, rng))), "the glass's roughness changed nothing"
    pt.close()


@pytest.mark.parametrize("batch", [1, 3])
def test_batches_and_the_second_size_equal_restatement(W, O, batch):
    w, h = SIZES["64x64"]
    want, o = plain_reference(O, w, h, 0)
    pt = tracer(W, O, False, w, h, rng_mode=0, batch=batch)
    pt.render_timed(SPP)
    check(pt, want, o, f"64x64 batch {batch}")
    ms, launches = pt.microfacet_timing_ms()
    assert launches == (WAVES - 1) * (SPP // batch) and ms > 0.0, "one launch per batch before every shade step that scatters"
    pt.close()


def test_band_sharding_equals_restatement(W, O):
    w, h = SIZES["61x37"]
    for rank in range(2):
        r = rough(O, False, w, h, rng_mode=1, miss_floor=0, tile_rank=rank, tile_world=2)
        want = plain_render(O, r, wrap=A.Local)
        assert r.glass_sampled > 50
        pt = tracer(W, O, False, w, h, rng_mode=1, miss_floor=0, tile_rank=rank, tile_world=2)
        pt.render(SPP)
        check(pt, want, r, f"rank {rank} of 2")
        pt.close()


@pytest.mark.parametrize("loop", ["", "UNFUSED", "NO_LDS_SCENE"])
def test_with_a_table_of_normals_equals_restatement(W, O, loop):
    """both features: every hit's record carries the shading normal, a rough glass hit samples about it (rough_glass_kernel<true>)"""
    w, h = SIZES["61x37"]
    r = rough(O, False, w, h, table=True)
    want = plain_render(O, r)
    assert_all_four(r)
    pt = tracer(W, O, False, w, h, "SHADING_NORMALS" + ("|" + loop if loop else ""), table=True)
    pt.render_timed(SPP)
    check(pt, want, r, f"SHADING_NORMALS {loop}")
    assert pt.shading_normal_timing()[1] == 0 and pt.microfacet_timing_ms()[1] > 0, "the pass takes the shading-normal pass's place"
    pt.close()


def test_retire_equals_restatement(W, O):
    w, h = SIZES["61x37"]
    t, mt, _, _, _ = scene(O, True)
    inner = rough(O, True, w, h, rng_mode=1)
    o = RR.Retiring(inner, roulette_start=1, q_min=0.25)
    with RD.MF.rough_weights(inner):
        want = E.render_with_emission(o, E.Emission({4: LAMP_E}, triangles=t, materials=mt), spp=SPP, termination=o)
    assert sum(sum(k) for k in o.retired) > 0 and inner.glass_sampled > 100
    pt = tracer(W, O, True, w, h, "EMISSION|RETIRE", rng_mode=1)
    pt.set_emission(4, LAMP_E)
    pt.set_termination(1, 0.25)
    pt.render(SPP)
    check(pt, want, o, "retire")
    pt.close()


def test_light_transport_equals_restatement(W, O):
    """EMISSION | NEE | MIS with a lamp: a rough glass hit stays "specular" for the connect pass and the emission pass, which read the
    primitive's own type before the pass retypes the record"""
    w, h = SIZES["61x37"]
    t, mt, _, _, _ = scene(O, True)
    o = rough(O, True, w, h, rng_mode=1, miss_floor=0)
    shadow = oracle_of(O, True, w, h)
    em = E.Emission({4: LAMP_E}, triangles=t, materials=mt)
    with RD.MF.rough_weights(o):
        r = M.render_with_mis(o, shadow, em, spp=SPP, parts=True)
    assert r["stats"]["light_samples"] > 100 and o.glass_sampled > 100
    pt = tracer(W, O, True, w, h, "EMISSION|NEE|MIS", rng_mode=1, miss_floor=0)
    pt.set_emission(4, LAMP_E)
    pt.render(SPP)
    check(pt, r["acc"], o, "EMISSION|NEE|MIS")
    pt.close()


def test_a_texture_on_the_glass_equals_restatement(W, O):
    w, h = SIZES["61x37"]
    t, mt, n9, _, _ = scene(O)
    uv = np.random.default_rng(8).uniform(-1.5, 2.5, (len(n9), 6)).astype(F)
    img = (np.random.default_rng(9).random((32, 48, 3)) * 1.2).astype(F)
    o = rough(O, False, w, h)
    with RD.MF.rough_weights(o):
        want = T.render_with_textures(o, T.Textures(triangles=t, materials=mt, slots={0: (img, {})}, bind={GLASS: 0, 3: 0}, uv=uv), spp=SPP)
    assert o.glass_sampled > 100
    pt = tracer(W, O, False, w, h, "TEXTURES")
    pt.set_texture(0, img)
    pt.bind_texture(GLASS, 0)
    pt.bind_texture(3, 0)
    pt.set_triangle_uvs(uv)
    pt.render(SPP)
    check(pt, want, o, "textures")
    pt.close()


# ---------------------------------------------------------------- 3. identity
@pytest.mark.parametrize("loop", ["", "UNFUSED", "NO_LDS_SCENE"])
def test_no_glass_roughness_is_the_microfacet_context(W, O, loop):
    """the frame's bits and the launches, with the flag but no glass alpha above 0: with no alpha at all, with the metal's alone, and
    after the glass's was set and taken back"""
    w, h = SIZES["61x37"]
    for alphas in ({}, {METAL: ALPHA}):
        plain = tracer(W, O, False, w, h, loop, alphas=alphas, dielectric=False, batch=3)
        _, want_launches = plain.render_timed(SPP)
        want, want_pass = plain.accumulated(), plain.microfacet_timing_ms()[1]
        plain.close()
        pt = tracer(W, O, False, w, h, loop, alphas=alphas, batch=3)
        _, launches = pt.render_timed(SPP)
        assert_bits(pt.accumulated(), want, f"flag set, alphas {alphas}")
        assert np.array_equal(launches, want_launches) and pt.microfacet_timing_ms()[1] == want_pass
        pt.set_roughness(GLASS, ALPHA)
        pt.render(SPP)
        assert not np.array_equal(bits(pt.accumulated()), bits(want))
        pt.set_roughness(GLASS, 0.0)
        pt.render(SPP)
        assert_bits(pt.accumulated(), want, f"set, then taken back, alphas {alphas}")
        pt.close()


def test_without_the_flag_a_glass_alpha_is_inert(W, O):
    """WFPT_FLAG_MICROFACET alone: the roughness of the glass is stored and the frame is the smooth glass's"""
    w, h = SIZES["61x37"]
    pt = tracer(W, O, False, w, h, alphas={GLASS: ALPHA}, dielectric=False)
    assert pt.get_roughness(GLASS) == F(ALPHA)
    pt.render(SPP)
    assert_bits(pt.accumulated(), oracle_of(O, False, w, h).render(SPP), "the smooth glass")
    with pytest.raises(W.WfptError) as e:
        pt.sample_rough_dielectric(np.zeros((1, 16), F))
    assert e.value.status == -1
    pt.close()


# ---------------------------------------------------------------- 4. scene updates, state and refusals
def test_update_scene_keeps_alphas(W, O):
    w, h = SIZES["61x37"]
    t, mt, _, _, created = scene(O)
    want, o = plain_reference(O, w, h, 0)
    pt = tracer(W, O, False, w, h, rng_mode=0)
    pt.render(1)
    sp = np.zeros(1, W.SPHERE)
    sp["radius"] = 1.0
    with pytest.raises(W.WfptError):
        pt.update_scene(W.Scene(sp, mt.copy()))  # spheres, while an alpha is above 0
    pt.render(SPP - 1)
    check(pt, want, o, "after a refused update the render goes on")
    pt.update_scene(W.Scene(np.zeros(0, W.SPHERE), mt.copy(), triangles=created.copy()[::-1].copy()))
    assert pt.get_roughness(GLASS) == F(ALPHA) and pt.get_roughness(METAL) == F(ALPHA)
    pt.render(SPP)
    check(pt, want, o, "after an update to the same scene")
    pt.close()


def test_refusals_and_the_restart(W, O):
    w, h = 16, 16
    both = W.FLAG_MICROFACET | W.FLAG_ROUGH_DIELECTRIC
    with pytest.raises(W.WfptError) as e:
        W.shirley_path_tracer(w, h, flags=W.FLAG_ROUGH_DIELECTRIC)
    assert "WFPT_FLAG_ROUGH_DIELECTRIC needs" in str(e.value)
    sphere = W.shirley_path_tracer(w, h, flags=both)
    with pytest.raises(W.WfptError) as e:
        sphere.set_roughness(0, 0.5)
    assert e.value.status == -1
    assert len(sphere.sample_rough_dielectric(random_rows(4, 1))) == 4
    sphere.close()
    binned = tracer(W, O, False, 200, 120, "BINNING", alphas={}, rng_mode=W.RNG_PIXEL)
    assert binned.loop_kind == "fused_binned"
    with pytest.raises(W.WfptError) as e:
        binned.set_roughness(GLASS, 0.5)
    assert e.value.status == -4
    binned.set_roughness(GLASS, 0.0)
    assert binned.loop_kind == "fused_binned"
    binned.close()
    pt = tracer(W, O, False, w, h)
    pt.render(2)
    assert W.lib().wfpt_accumulated_samples(pt.handle) == 2
    pt.set_roughness(GLASS, 0.5)
    assert W.lib().wfpt_accumulated_samples(pt.handle) == 0, "a set restarts the accumulation"
    pt.set_roughness(GLASS, ALPHA)
    pt.render(3)
    fresh = tracer(W, O, False, w, h)
    fresh.render(3)
    assert_bits(pt.accumulated(), fresh.accumulated(), "after the restart the frames are a fresh context's")
    fresh.close()
    pt.close()
