"""Roughness maps (WFPT_FLAG_ROUGHNESS_MAPS, include/wfpt.h "Roughness maps") on the GPU.

The device's steps R1-R4 and whole renders are compared bit for bit with tests/roughness_map_ref.py: the numpy float32 restatement, driven
through the oracle's stages by roughness_map_ref.RoughMapped. The scene is tests/test_gpu_normal_maps.py's -- a 320-triangle icosphere
(Lambertian, fuzzy metal and glass by thirds) over a two-triangle ground, with spherical UVs -- the metal and the glass third at alpha 0.3
with the green channel of the seeded 16x8 stripe map (exact zeros, values above 1, values between) bound on both; 3 samples, 4 wavefronts.
Before a stripe-map reference is compared with anything it must hold at least 20 hits in each of the six classes
{metal, glass} x {texel 0, above 1, between}, and a rough glass hit in each of RoughGlass's four cells."""
import numpy as np
import pytest

import adaptive_ref as A
import emission_ref as E
import microfacet_ref as MF
import mis_ref as M
import nee_ref as N
import normal_map_ref as NM
import retire_ref as RR
import rough_dielectric_ref as RD
import roughness_map_ref as RM
import shading_normals_ref as S
import texture_ref as T
import transport_ref
from helpers import assert_bits_or_nan
from test_gpu_normal_maps import uv_table
from test_gpu_shading_normals import FLOOR, LAMP_E, SIZES, SPP, WAVES, assert_bits, bits, check, flags_of, oracle_of, probe_points, scene
from test_roughness_map_host import assert_conditions

pytestmark = pytest.mark.gpu

F = np.float32
SLOT, CHANNEL = 2, 1
METAL, GLASS, ALPHA = 1, 2, 0.3
BOTH = {METAL: ALPHA, GLASS: ALPHA}
BIND = {METAL: (SLOT, CHANNEL, "linear"), GLASS: (SLOT, CHANNEL, "linear")}
STRIPES = {SLOT: (RM.stripe_map(), {})}
ONES = {SLOT: (RM.constant_map(1.0), {"filter": "nearest"})}  # (a bilinear lookup of equal texels need not round to exactly 1)
NSLOT = 1
NSLOTS = {NSLOT: (NM.tilt_map(), {})}
NBIND = {m: (NSLOT, 1.0) for m in range(4)}


@pytest.fixture(scope="module")
def W():
    import wavefront_path_tracer_amd as W
    return W


@pytest.fixture(scope="module")
def O():
    from oracle import oracle as O
    return O


def tracer(W, O, emitter, w, h, flags="", alphas=BOTH, bind=BIND, slots=STRIPES, dielectric=True, table=False, nbind=None, flag=True, **kw):
    """flags may name SHADING_NORMALS and NORMAL_MAPS: table sets the corner normals, nbind binds normal maps"""
    t, mt, n9, _, created = scene(O, emitter)
    sc = W.Scene(np.zeros(0, W.SPHERE), mt.copy(), triangles=created.copy())
    cc = W.CameraController(W.Camera((0.0, 1.0, 4.5), (0.0, -0.1, 0.0)), 40.0, 0.0, 10.0, 0.1, 100.0)
    kw.setdefault("max_wavefronts", WAVES)
    kw.setdefault("miss_floor", FLOOR)
    f = W.FLAG_TEXTURES | W.FLAG_MICROFACET | (W.FLAG_ROUGH_DIELECTRIC if dielectric else 0) | (W.FLAG_ROUGHNESS_MAPS if flag else 0)
    pt = W.PathTracer(sc, W.RenderParameters(cc, (w, h)), flags=f | flags_of(W, flags), **kw)
    assert np.array_equal(pt.scene.triangles, t), "the tracer's triangles are not in the oracle's order"
    pt.set_triangle_uvs(uv_table(O, emitter))
    if table:
        pt.set_triangle_normals(n9)
    for m, a in alphas.items():
        pt.set_roughness(m, a)
    for s, (img, params) in slots.items():
        pt.set_texture(s, img, **params)
    for m, (s, strength) in (nbind or {}).items():
        pt.bind_normal_map(m, s, strength)
    for m, (s, channel, remap) in bind.items():
        pt.bind_roughness_map(m, s, channel, remap)
    return pt


def mapped(O, emitter, w, h, alphas=BOTH, bind=BIND, slots=STRIPES, dielectric=True, table=False, nbind=None, **kw):
    """the restatement of tracer()'s context"""
    t, mt, n9, _, _ = scene(O, emitter)
    uv = uv_table(O, emitter)
    normals = S.Normals(t, n9) if table else None
    if nbind:
        normals = NM.Mapped(t, uv, slots, nbind, normals)
    return RM.RoughMapped(oracle_of(O, emitter, w, h, **kw), t, mt, alphas, RM.Roughness(t, uv, slots, bind), normals, glass=dielectric)


def plain_render(O, r, emitter=False, wrap=lambda o: o, textures=None):
    t, mt, _, _, _ = scene(O, emitter)
    with MF.rough_weights(r):
        return T.render_with_textures(wrap(r), textures or T.Textures(triangles=t, materials=mt), spp=SPP)


# ---------------------------------------------------------------- 1. steps R1-R4 alone
@pytest.mark.parametrize("remap", RM.REMAPS)
@pytest.mark.parametrize("filter", ["bilinear", "nearest"])
def test_sample_roughness_map_equals_restatement(W, O, filter, remap):
    """test_sample_shading_normal_equals_restatement's probe set plus 400 points on the ground, on a scene of its own whose ground is a
    metal: the metal third reads the red channel, the glass third the green one and the ground the blue one of a slot with a scale and an
    offset. Material 0 (Lambertian) is bound and holds an alpha, which is inert: code 2. The zero-row triangle's material 4 is a metal with
    an alpha and no binding: code 1. Then the metal's alpha is set to 0 under its binding: code 2."""
    t, n9, p, prim, maybe_nan = probe_points(O)
    t = t.copy()
    n_all = len(t)
    t["material_idx"][n_all - 1] = 4
    t["material_type"][n_all - 1] = 1
    ground = np.flatnonzero(t["material_idx"] == 3)
    assert len(ground) == 2
    t["material_type"][ground] = 1
    uv = np.concatenate([uv_table(O), np.random.default_rng(2).uniform(-1.0, 2.0, (3, 6)).astype(F)])
    rng = np.random.default_rng(12)
    gp = rng.choice(ground, 400)
    b = rng.dirichlet((1.0, 1.0, 1.0), 400)
    gpts = (t["v0"][gp].astype(np.float64) + t["e1"][gp] * b[:, 1:2] + t["e2"][gp] * b[:, 2:3]).astype(F)
    p, prim, maybe_nan = np.concatenate([p, gpts]), np.concatenate([prim, gp]), np.concatenate([maybe_nan, np.zeros(400, bool)])
    slots = {SLOT: (RM.stripe_map(), {"filter": filter, "scale": (2.0, 1.0), "offset": (0.25, 0.5)})}
    bind = {0: (SLOT, 1, remap), METAL: (SLOT, 0, remap), GLASS: (SLOT, 1, remap), 3: (SLOT, 2, remap)}
    alphas = np.array([0.7, 0.3, 0.3, 0.5, 0.4], F)
    rm = RM.Roughness(t, uv, slots, bind)
    mt = scene(O)[1]
    assert len(mt) >= 5
    cc = W.CameraController(W.Camera((0.0, 1.0, 4.5), (0.0, -0.1, 0.0)), 40.0, 0.0, 10.0, 0.1, 100.0)
    tree = W.BVHTree(len(t))
    order = t.copy()
    tree.build_bvh_tree_triangles(order, 32)
    pt = W.PathTracer(W.Scene(np.zeros(0, W.SPHERE), mt, triangles=order), W.RenderParameters(cc, (16, 16)),
                      flags=flags_of(W, "TEXTURES|MICROFACET|ROUGH_DIELECTRIC|ROUGHNESS_MAPS"), bvh=tree)
    pt.set_triangle_uvs(uv)
    pt.set_texture(SLOT, slots[SLOT][0], **slots[SLOT][1])
    for m, (s, channel, rmp) in bind.items():
        pt.bind_roughness_map(m, s, channel, rmp)
    index = {tuple(r): i for i, r in enumerate(np.concatenate([order["v0"], order["e1"], order["e2"]], 1).tolist())}
    where = np.array([index[tuple(r)] for r in np.concatenate([t["v0"], t["e1"], t["e2"]], 1).tolist()])  # creation index -> device index
    rows = RM.probe_rows(p, where[prim])
    mat = t["material_idx"][prim]
    # bound, no alpha above 0 yet: the probe answers, every row is code 2
    got = pt.sample_roughness_map(rows)
    assert np.array_equal(got, np.tile(np.array([0, 0, 2, 0], F), (len(rows), 1))), "no alpha is above 0"
    for m, a in enumerate(alphas):
        pt.set_roughness(m, float(a))
    for zeroed in (False, True):
        if zeroed:
            alphas[METAL] = 0.0
            pt.set_roughness(METAL, 0.0)
            assert pt.get_roughness_map(METAL) == (SLOT, 0, remap)
        want = RM.sample_rows(rm, alphas, p, prim)
        assert not np.isnan(want[~maybe_nan]).any()
        got = pt.sample_roughness_map(rows)
        assert_bits(got[~maybe_nan], want[~maybe_nan], f"finite rows, metal zeroed {zeroed}")
        assert_bits_or_nan(got[maybe_nan], want[maybe_nan], "may-be-NaN rows")
        code = want[:, 2]
        assert (code[mat == 0] == 2).all() and (want[mat == 0, :2] == 0).all(), "a Lambertian's alpha is inert"
        assert (code[mat == 4] == 1).all() and (mat == 4).sum() >= 100 and (want[mat == 4, 0] == F(0.4)).all() and (want[mat == 4, 1] == 1).all()
        assert ((code[mat == METAL] == 2).all() if zeroed else np.isin(code[mat == METAL], (0, 3)).all())
        for m in (GLASS, 3) if zeroed else (METAL, GLASS, 3):
            c = code[(mat == m) & ~maybe_nan]
            assert (c == 0).sum() >= 20 and (c == 3).sum() >= 20 and np.isin(c, (0, 3)).all(), (m, np.bincount(c.astype(int)))
        assert (want[code == 3, 0] == 0).all() and (want[code == 0, 0] > 0).all()
    out = pt.sample_roughness_map(RM.probe_rows(p[:2], [len(t), 0xFFFFFFFF]))
    assert np.array_equal(out, [(0, 0, 5, 0)] * 2), "a primitive outside the scene"
    assert len(pt.sample_roughness_map(np.zeros((0, 4), F))) == 0
    pt.close()


# ---------------------------------------------------------------- 2. frames against the restatement
_refs = {}


def plain_reference(O, w, h, rng, **kw):
    key = (w, h, rng, tuple(sorted(kw.items())))
    if key not in _refs:
        r = mapped(O, False, w, h, rng_mode=rng, **kw)
        _refs[key] = (plain_render(O, r), r)
        assert_conditions(r, f"{w}x{h} rng {rng}")
    return _refs[key]


LOOPS = {"": "fused", "UNFUSED": "stages", "SPLIT_SHADE": "stages", "NO_LDS_SCENE": "refill", "NO_GRAPH": "fused", "EXACT_TRAVERSAL": "fused"}


@pytest.mark.parametrize("rng", [0, 1])
@pytest.mark.parametrize("loop", list(LOOPS))
def test_loops_equal_restatement(W, O, loop, rng):
    w, h = SIZES["61x37"]
    want, o = plain_reference(O, w, h, rng)
    pt = tracer(W, O, False, w, h, loop, rng_mode=rng)
    assert pt.loop_kind == LOOPS[loop]
    pt.render(SPP)
    check(pt, want, o, f"{loop} rng {rng}")
    pt.close()


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("batch", [1, 2, 3])
def test_batches_at_both_sizes_equal_restatement_and_book_the_pass(W, O, batch, size):
    """7. the pass is booked in wfpt_microfacet_timing_ms with the launch count of the pass it replaces"""
    w, h = SIZES[size]
    want, o = plain_reference(O, w, h, 0)
    pt = tracer(W, O, False, w, h, rng_mode=0, batch=batch)
    pt.render_timed(SPP)
    check(pt, want, o, f"{size} batch {batch}")
    ms, launches = pt.microfacet_timing_ms()
    assert launches == (WAVES - 1) * ((SPP + batch - 1) // batch) and ms > 0.0, "one launch per batch before every shade step that scatters"
    pt.close()


def test_band_sharding_equals_restatement(W, O):
    w, h = SIZES["61x37"]
    for rank in range(2):
        r = mapped(O, False, w, h, rng_mode=1, miss_floor=0, tile_rank=rank, tile_world=2)
        want = plain_render(O, r, wrap=A.Local)
        assert r.sampled > 50 and r.glass_sampled > 50
        pt = tracer(W, O, False, w, h, rng_mode=1, miss_floor=0, tile_rank=rank, tile_world=2)
        pt.render(SPP)
        check(pt, want, r, f"rank {rank} of 2")
        pt.close()


# ---------------------------------------------------------------- 3. the three sources of the normal
@pytest.mark.parametrize("loop", ["", "UNFUSED"])
def test_with_a_table_of_normals_equals_restatement(W, O, loop):
    w, h = SIZES["61x37"]
    r = mapped(O, False, w, h, table=True)
    want = plain_render(O, r)
    assert_conditions(r, "table of normals")
    pt = tracer(W, O, False, w, h, "SHADING_NORMALS" + ("|" + loop if loop else ""), table=True)
    pt.render_timed(SPP)
    check(pt, want, r, f"SHADING_NORMALS {loop}")
    assert pt.shading_normal_timing()[1] == 0 and pt.microfacet_timing_ms()[1] > 0
    pt.close()


@pytest.mark.parametrize("table", [True, False])
def test_with_a_normal_map_on_the_same_materials_equals_restatement(W, O, table):
    """both maps on the metal and the glass third: one (u, v), two lookups; the Lambertian third and the ground have the normal map alone"""
    w, h = SIZES["61x37"]
    slots = {**STRIPES, **NSLOTS}
    r = mapped(O, False, w, h, slots=slots, table=table, nbind=NBIND)
    with S.shading_receivers(r.normals):
        want = plain_render(O, r)
    assert_conditions(r, f"normal map, table {table}")
    pt = tracer(W, O, False, w, h, "SHADING_NORMALS|NORMAL_MAPS", slots=slots, table=table, nbind=NBIND, batch=1)
    pt.render_timed(SPP)
    check(pt, want, r, f"NORMAL_MAPS, table {table}")
    assert pt.shading_normal_timing()[1] == 0 and pt.microfacet_timing_ms()[1] == (WAVES - 1) * SPP
    pt.close()


def test_one_slot_serves_colour_normal_and_roughness(W, O):
    w, h = SIZES["61x37"]
    t, mt, _, _, _ = scene(O)
    slots = {SLOT: (NM.tilt_map(), {})}
    nbind = {m: (SLOT, 1.0) for m in range(4)}
    r = mapped(O, False, w, h, slots=slots, table=True, nbind=nbind)
    colour = T.Textures(triangles=t, materials=mt, slots=slots, bind={0: SLOT, METAL: SLOT, 3: SLOT}, uv=uv_table(O))
    want = plain_render(O, r, textures=colour)
    assert r.sampled > 100 and r.glass_sampled > 100
    pt = tracer(W, O, False, w, h, "SHADING_NORMALS|NORMAL_MAPS", slots=slots, table=True, nbind=nbind)
    for m in (0, METAL, 3):
        pt.bind_texture(m, SLOT)
    pt.render(SPP)
    check(pt, want, r, "one slot, three kinds")
    assert pt.get_roughness_map(METAL) == (SLOT, CHANNEL, "linear") and pt.normal_map(METAL) == (SLOT, 1.0)
    pt.close()


# ---------------------------------------------------------------- 4. metal alone
def test_without_rough_dielectric_the_glass_binding_is_inert(W, O):
    w, h = SIZES["61x37"]
    r = mapped(O, False, w, h, dielectric=False)
    want = plain_render(O, r)
    assert r.sampled > 100 and r.glass_sampled == 0 and all(r.classes[("metal", c)] >= 20 for c in ("zero", "above_one", "between"))
    assert all(r.classes[("glass", c)] == 0 for c in ("zero", "above_one", "between"))
    pt = tracer(W, O, False, w, h, dielectric=False)
    pt.render(SPP)
    check(pt, want, r, "MICROFACET alone")
    metal_only = tracer(W, O, False, w, h, dielectric=False, bind={METAL: BIND[METAL]})
    metal_only.render(SPP)
    assert_bits(metal_only.accumulated(), want, "the glass binding changes nothing")
    metal_only.close()
    pt.close()


# ---------------------------------------------------------------- 5. with the other passes
@pytest.mark.parametrize("flags", ["EMISSION|NEE", "EMISSION|NEE|MIS"])
def test_light_transport_equals_restatement(W, O, flags):
    w, h = SIZES["61x37"]
    t, mt, _, _, _ = scene(O, True)
    o = mapped(O, True, w, h, rng_mode=1, miss_floor=0)
    shadow = oracle_of(O, True, w, h)
    em = E.Emission({4: LAMP_E}, triangles=t, materials=mt)
    with MF.rough_weights(o):
        r = (M.render_with_mis if "MIS" in flags.split("|") else N.render_with_nee)(o, shadow, em, spp=SPP, parts=True)
    assert r["stats"]["light_samples"] > 100 and o.glass_sampled > 100 and o.sampled > 100
    pt = tracer(W, O, True, w, h, flags, rng_mode=1, miss_floor=0)
    pt.set_emission(4, LAMP_E)
    pt.render(SPP)
    check(pt, r["acc"], o, flags)
    pt.close()


def test_retire_equals_restatement(W, O):
    w, h = SIZES["61x37"]
    t, mt, _, _, _ = scene(O, True)
    inner = mapped(O, True, w, h, rng_mode=1)
    o = RR.Retiring(inner, roulette_start=1, q_min=0.25)
    with MF.rough_weights(inner):
        want = E.render_with_emission(o, E.Emission({4: LAMP_E}, triangles=t, materials=mt), spp=SPP, termination=o)
    assert sum(sum(k) for k in o.retired) > 0 and inner.glass_sampled > 100
    pt = tracer(W, O, True, w, h, "EMISSION|RETIRE", rng_mode=1)
    pt.set_emission(4, LAMP_E)
    pt.set_termination(1, 0.25)
    pt.render(SPP)
    check(pt, want, o, "retire")
    pt.close()


def test_adaptive_mask_equals_restatement(W, O):
    w, h = SIZES["61x37"]
    y, x = np.mgrid[0:h, 0:w]
    mask = ((x // 5 + y // 3) % 3 != 0).reshape(-1)
    t, mt, _, _, _ = scene(O)
    inner = mapped(O, False, w, h, rng_mode=1)
    o = A.Masked(inner, mask)
    with MF.rough_weights(inner):  # (the unbound texture table makes the loop keep the throughput itself, as in plain_render)
        r = transport_ref.render(o, tx=T.Textures(triangles=t, materials=mt), spp=SPP, parts=True)
    assert inner.sampled > 100 and inner.glass_sampled > 100
    sums = A.Sums(w * h).add(r, mask)
    pt = tracer(W, O, False, w, h, "ADAPTIVE", rng_mode=1)
    pt.set_active_mask(mask)
    pt.render(SPP)
    check(pt, sums.acc, o, "adaptive mask")
    assert np.array_equal(pt.sample_counts().reshape(-1), sums.count)
    pt.close()


# ---------------------------------------------------------------- 6. identities
def timed(pt):
    _, launches = pt.render_timed(SPP)
    return pt.accumulated(), launches, pt.microfacet_timing_ms()[1], pt.texture_timing()[1]


@pytest.mark.parametrize("loop", ["", "UNFUSED", "NO_LDS_SCENE"])
def test_nothing_bound_no_alpha_and_an_all_ones_map_are_the_unflagged_frames(W, O, loop):
    w, h = SIZES["61x37"]
    for alphas in (BOTH, {}):  # the rough and the smooth TEXTURES | MICROFACET | ROUGH_DIELECTRIC context
        ref = tracer(W, O, False, w, h, loop, alphas=alphas, bind={}, slots={}, flag=False, rng_mode=0, batch=3)
        want, launches, mf_launches, tex_launches = timed(ref)
        ref.close()
        assert (mf_launches > 0) == bool(alphas)
        pt = tracer(W, O, False, w, h, loop, alphas=alphas, bind={} if alphas else BIND, rng_mode=0, batch=3)
        got, got_launches, got_mf, got_tex = timed(pt)
        what = "the flag with nothing bound" if alphas else "bound while every alpha is 0"
        assert_bits(got, want, what)
        assert np.array_equal(got_launches, launches) and got_mf == mf_launches and got_tex == tex_launches, what + ": the launches"
        if alphas:
            pt.set_texture(SLOT, *ONES[SLOT][:1], **ONES[SLOT][1])
            for m, (s, channel, remap) in BIND.items():
                pt.bind_roughness_map(m, s, channel, remap)
            pt.render(SPP)
            assert_bits(pt.accumulated(), want, "an all-ones map is the un-mapped rough frame")
        pt.close()


def test_the_stripe_map_changes_most_of_the_metal_and_the_glass(W, O):
    """against a pass that silently copies: more than half of the pixels that see the metal and glass thirds differ from the un-mapped frame"""
    w, h = SIZES["61x37"]
    t = scene(O)[0]
    ref = tracer(W, O, False, w, h, bind={}, slots={}, flag=False, rng_mode=0)
    ref.render(SPP)
    base = ref.accumulated()
    ref.close()
    pt = tracer(W, O, False, w, h, rng_mode=0)
    pt.render(SPP)
    got = pt.accumulated()
    pt.close()
    changed = (bits(got).reshape(w * h, -1) != bits(base).reshape(w * h, -1)).any(axis=1)
    o = oracle_of(O, False, w, h)
    gx, gy = (w + 7) // 8, (h + 7) // 8
    o.set_frame(1, 0)
    o.set_counters([0, 0, gx * gy * 64])
    o.generate_rays(gx, gy, True)
    o.extend(*O.workgroup_size_64(gx * gy * 64))
    hits = o.hits(int(o.counters()[1]))
    rays = o.rays()[hits["ray_idx"].astype(np.int64)]
    sees = np.zeros(w * h, bool)
    sees[rays["pixel_idx"][np.isin(t["material_idx"][hits["sphere_idx"].astype(np.int64)], (METAL, GLASS))]] = True
    assert sees.sum() > 100 and changed[sees].mean() > 0.5, (int(sees.sum()), float(changed[sees].mean()))


# ---------------------------------------------------------------- 8. life cycle and refusals
def test_texture_roughness_and_scene_updates_keep_or_drop_the_bindings(W, O):
    w, h = SIZES["61x37"]
    t, mt, n9, _, created = scene(O)
    want, o = plain_reference(O, w, h, 0)
    rough = RD.RoughGlass(oracle_of(O, False, w, h), t, mt, BOTH)
    unmapped = plain_render(O, rough)
    pt = tracer(W, O, False, w, h, rng_mode=0)
    pt.render(1)
    sp = np.zeros(1, W.SPHERE)
    sp["radius"] = 1.0
    with pytest.raises(W.WfptError):
        pt.update_scene(W.Scene(sp, mt.copy()))  # to spheres while a roughness binding is held
    pt.render(SPP - 1)
    check(pt, want, o, "after a refused update the render goes on")
    pt.update_scene(W.Scene(np.zeros(0, W.SPHERE), mt.copy(), triangles=created.copy()[::-1].copy()))
    assert pt.get_roughness_map(METAL) == BIND[METAL] and pt.get_roughness_map(GLASS) == BIND[GLASS]
    pt.render(SPP)
    check(pt, want, o, "after an update to the same scene")
    # set_roughness(0) then back: the binding stays, inert in between
    pt.set_roughness(GLASS, 0.0)
    assert pt.get_roughness_map(GLASS) == BIND[GLASS]
    pt.render(SPP)
    metal = mapped(O, False, w, h, alphas={METAL: ALPHA})
    check(pt, plain_render(O, metal), metal, "the glass's alpha at 0")
    pt.set_roughness(GLASS, ALPHA)
    pt.render(SPP)
    check(pt, want, o, "and back")
    # set_texture on the bound slot keeps the bindings; clear_texture drops them
    pt.set_texture(SLOT, ONES[SLOT][0], **ONES[SLOT][1])
    assert pt.get_roughness_map(METAL) == BIND[METAL]
    pt.render(SPP)
    check(pt, unmapped, rough, "the slot set to all ones")
    pt.set_texture(SLOT, STRIPES[SLOT][0])
    pt.render(SPP)
    check(pt, want, o, "the slot set to the stripes again")
    pt.clear_texture(SLOT)
    assert all(pt.get_roughness_map(m) == (None, 0, "linear") for m in range(5))
    pt.render(SPP)
    check(pt, unmapped, rough, "the slot cleared: the un-mapped rough frame")
    with pytest.raises(W.WfptError):
        pt.sample_roughness_map(np.zeros((1, 4), F))  # nothing is bound
    pt.set_texture(SLOT, STRIPES[SLOT][0])
    pt.bind_roughness_map(GLASS, SLOT, 0, "squared")
    assert pt.get_roughness_map(GLASS) == (SLOT, 0, "squared")
    pt.bind_roughness_map(GLASS, None)
    pt.render(SPP)
    check(pt, unmapped, rough, "bound and unbound again")
    # an update to fewer materials drops the bindings of the ones that are gone
    pt.bind_roughness_map(4, SLOT, 1, "linear")
    pt.bind_roughness_map(METAL, SLOT, 1, "linear")
    fewer = created.copy()
    fewer["material_idx"][fewer["material_idx"] == 4] = 3
    pt.update_scene(W.Scene(np.zeros(0, W.SPHERE), mt[:4].copy(), triangles=fewer))
    assert pt.get_roughness_map(METAL) == BIND[METAL]
    with pytest.raises(W.WfptError):
        pt.get_roughness_map(4)
    pt.update_scene(W.Scene(np.zeros(0, W.SPHERE), mt.copy(), triangles=created.copy()))
    assert pt.get_roughness_map(4) == (None, 0, "linear") and pt.get_roughness_map(METAL) == BIND[METAL]
    pt.close()


def test_refusals(W, O):
    w, h = 16, 16
    t, mt, n9, _, created = scene(O)
    sc = W.Scene(np.zeros(0, W.SPHERE), mt.copy(), triangles=created.copy())
    cc = W.CameraController(W.Camera((0.0, 1.0, 4.5), (0.0, -0.1, 0.0)), 40.0, 0.0, 10.0, 0.1, 100.0)
    for flags in ("ROUGHNESS_MAPS", "ROUGHNESS_MAPS|TEXTURES", "ROUGHNESS_MAPS|MICROFACET", "ROUGHNESS_MAPS|MICROFACET|ROUGH_DIELECTRIC"):
        with pytest.raises(W.WfptError) as e:
            W.PathTracer(sc, W.RenderParameters(cc, (w, h)), flags=flags_of(W, flags), max_wavefronts=WAVES)
        assert "WFPT_FLAG_ROUGHNESS_MAPS needs" in str(e.value)
    sphere = W.shirley_path_tracer(w, h, flags=flags_of(W, "TEXTURES|MICROFACET|ROUGHNESS_MAPS"))
    sphere.set_texture(SLOT, STRIPES[SLOT][0])
    with pytest.raises(W.WfptError) as e:
        sphere.bind_roughness_map(0, SLOT)
    assert e.value.status == W.ERR_INVALID_ARGUMENT
    sphere.close()
    unflagged = tracer(W, O, False, w, h, bind={}, flag=False)
    for call in (lambda: unflagged.bind_roughness_map(METAL, SLOT), lambda: unflagged.get_roughness_map(METAL),
                 lambda: unflagged.sample_roughness_map(np.zeros((1, 4), F))):
        with pytest.raises(W.WfptError) as e:
            call()
        assert e.value.status == W.ERR_INVALID_ARGUMENT
    unflagged.close()
    pt = tracer(W, O, False, w, h)
    pt.render(2)
    before = pt.accumulated()
    for call in (lambda: pt.bind_roughness_map(5, SLOT), lambda: pt.bind_roughness_map(METAL, 0), lambda: pt.bind_roughness_map(METAL, W.MAX_TEXTURES),
                 lambda: pt.bind_roughness_map(METAL, -2), lambda: pt.bind_roughness_map(METAL, SLOT, 3), lambda: pt.bind_roughness_map(METAL, SLOT, 1, 2),
                 lambda: pt.get_roughness_map(5)):
        with pytest.raises(W.WfptError) as e:
            call()
        assert e.value.status == W.ERR_INVALID_ARGUMENT
    assert_bits(pt.accumulated(), before, "a refused call restarted the accumulation")
    assert pt.get_roughness_map(METAL) == BIND[METAL]
    pt.render(1)
    assert W.lib().wfpt_accumulated_samples(pt.handle) == 3
    pt.bind_roughness_map(METAL, SLOT, 0, "squared")
    assert W.lib().wfpt_accumulated_samples(pt.handle) == 0, "a bind restarts the accumulation"
    pt.close()
    binned = W.PathTracer(sc, W.RenderParameters(cc, (200, 120)), flags=flags_of(W, "TEXTURES|MICROFACET|ROUGHNESS_MAPS|BINNING"),
                          max_wavefronts=WAVES, rng_mode=W.RNG_PIXEL)
    assert binned.loop_kind == "fused_binned"
    with pytest.raises(W.WfptError) as e:
        binned.bind_roughness_map(METAL, SLOT)
    assert e.value.status == W.ERR_UNSUPPORTED
    binned.bind_roughness_map(METAL, None)  # (nothing the loop has no form of)
    assert binned.loop_kind == "fused_binned"
    binned.close()
