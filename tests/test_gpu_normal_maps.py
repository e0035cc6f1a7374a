"""Tangent-space normal maps (WFPT_FLAG_NORMAL_MAPS, include/wfpt.h "Normal maps") on the GPU.

The device's steps A-F and whole renders are compared bit for bit with tests/normal_map_ref.py: the numpy float32 restatement, driven
through the oracle's stages by shading_normals_ref.Shaded with a normal_map_ref.Mapped in the table's place. The scene is
tests/test_gpu_shading_normals.py's -- a 320-triangle icosphere (Lambertian, fuzzy metal and glass by thirds) over a two-triangle ground --
with spherical UVs on the sphere, planar and mirrored UVs on the ground and a seeded 16x8 map of normals tilted up to 0.7 rad; 3 samples,
4 wavefronts."""
import numpy as np
import pytest

import adaptive_ref as A
import emission_ref as E
import env_mis_ref as X
import env_nee_ref as V
import mis_ref as M
import nee_ref as N
import normal_map_ref as NM
import retire_ref as RR
import rough_dielectric_ref as RD
import shading_normals_ref as S
import texture_ref as T
import transport_ref
from helpers import assert_bits_or_nan
from test_gpu_shading_normals import FLOOR, LAMP_E, SIZES, SPP, WAVES, assert_bits, bits, check, flags_of, oracle_of, probe_points, scene

pytestmark = pytest.mark.gpu

F = np.float32
SLOT = 1
SLOTS = {SLOT: (NM.tilt_map(), {})}
BIND = {0: (SLOT, 1.0), 1: (SLOT, 1.0), 2: (SLOT, 1.0), 3: (SLOT, 1.0)}  # the sphere's thirds and the ground; a lamp (4) has none
BASE = "TEXTURES|SHADING_NORMALS"


@pytest.fixture(scope="module")
def W():
    import wavefront_path_tracer_amd as W
    return W


@pytest.fixture(scope="module")
def O():
    from oracle import oracle as O
    return O


_uv = {}


def uv_table(O, emitter=False):
    if emitter not in _uv:
        created, _, _, uv = NM.sphere_scene(O, emitter=emitter)
        assert np.array_equal(created, scene(O, emitter)[4]), "normal_map_ref's scene is not shading_normals_ref's"
        _uv[emitter] = uv
    return _uv[emitter]


def tracer(W, O, emitter, w, h, flags="", bind=BIND, slots=SLOTS, table=True, mapped_flag=True, **kw):
    t, mt, n9, _, created = scene(O, emitter)
    sc = W.Scene(np.zeros(0, W.SPHERE), mt.copy(), triangles=created.copy())
    cc = W.CameraController(W.Camera((0.0, 1.0, 4.5), (0.0, -0.1, 0.0)), 40.0, 0.0, 10.0, 0.1, 100.0)
    kw.setdefault("max_wavefronts", WAVES)
    kw.setdefault("miss_floor", FLOOR)
    f = flags_of(W, BASE) | (W.FLAG_NORMAL_MAPS if mapped_flag else 0) | flags_of(W, flags)
    pt = W.PathTracer(sc, W.RenderParameters(cc, (w, h)), flags=f, **kw)
    assert np.array_equal(pt.scene.triangles, t), "the tracer's triangles are not in the oracle's order"
    pt.set_triangle_uvs(uv_table(O, emitter))
    if table:
        pt.set_triangle_normals(n9)
    for s, (img, params) in slots.items():
        pt.set_texture(s, img, **params)
    for m, (s, strength) in bind.items():
        pt.bind_normal_map(m, s, strength)
    return pt


def mapped_of(O, emitter=False, bind=BIND, slots=SLOTS, table=True):
    t, _, n9, _, _ = scene(O, emitter)
    return NM.Mapped(t, uv_table(O, emitter), slots, bind, S.Normals(t, n9) if table else None)


def shaded(O, emitter, w, h, bind=BIND, slots=SLOTS, table=True, **kw):
    mt = scene(O, emitter)[1]
    nm = mapped_of(O, emitter, bind, slots, table)
    return S.Shaded(oracle_of(O, emitter, w, h, **kw), nm, mt), nm


# ---------------------------------------------------------------- 1. steps A-F alone
@pytest.mark.parametrize("table", [True, False])
@pytest.mark.parametrize("filter", ["bilinear", "nearest"])
def test_sample_normal_map_equals_restatement(W, O, filter, table):
    """test_sample_shading_normal_equals_restatement's probe set (corners, edge midpoints, points outside, the degenerate triangle, normals
    facing away, NaN and inf points) plus both ground triangles (the second has mirrored UVs), a triangle of an unbound material and
    indices outside the scene; strengths 0, 1 and 4 on the sphere's thirds."""
    t, n9, p, prim, maybe_nan = probe_points(O)
    t = t.copy()
    n_all = len(t)
    t["material_idx"][n_all - 1] = 4  # the zero-row triangle: an unbound material
    uv = np.concatenate([uv_table(O), np.random.default_rng(2).uniform(-1.0, 2.0, (3, 6)).astype(F)])
    ground = np.flatnonzero(t["material_idx"] == 3)
    assert len(ground) == 2
    rng = np.random.default_rng(12)
    gp = rng.choice(ground, 400)
    b = rng.dirichlet((1.0, 1.0, 1.0), 400)
    gpts = (t["v0"][gp].astype(np.float64) + t["e1"][gp] * b[:, 1:2] + t["e2"][gp] * b[:, 2:3]).astype(F)
    p, prim, maybe_nan = np.concatenate([p, gpts]), np.concatenate([prim, gp]), np.concatenate([maybe_nan, np.zeros(400, bool)])
    slots = {SLOT: (NM.tilt_map(), {"filter": filter, "scale": (2.0, 1.0), "offset": (0.25, 0.5)})}
    bind = {0: (SLOT, 0.0), 1: (SLOT, 1.0), 2: (SLOT, 4.0), 3: (SLOT, 1.0)}
    nm = NM.Mapped(t, uv, slots, bind, S.Normals(t, n9) if table else None)
    want = nm.sample_rows(p, prim)
    rows = uv[t["_pad"][ground].astype(np.int64)]
    det = (rows[:, 2] - rows[:, 0]) * (rows[:, 5] - rows[:, 1]) - (rows[:, 4] - rows[:, 0]) * (rows[:, 3] - rows[:, 1])
    assert (det > 0).sum() == 1 and (det < 0).sum() == 1, "one ground triangle is mirrored"
    mt = scene(O)[1]
    cc = W.CameraController(W.Camera((0.0, 1.0, 4.5), (0.0, -0.1, 0.0)), 40.0, 0.0, 10.0, 0.1, 100.0)
    tree = W.BVHTree(len(t))
    order = t.copy()
    tree.build_bvh_tree_triangles(order, 32)
    pt = W.PathTracer(W.Scene(np.zeros(0, W.SPHERE), mt, triangles=order), W.RenderParameters(cc, (16, 16)),
                      flags=flags_of(W, BASE + "|NORMAL_MAPS"), bvh=tree)
    pt.set_triangle_uvs(uv)
    if table:
        pt.set_triangle_normals(n9)
    pt.set_texture(SLOT, slots[SLOT][0], **slots[SLOT][1])
    for m, (s, strength) in bind.items():
        pt.bind_normal_map(m, s, strength)
    index = {tuple(r): i for i, r in enumerate(np.concatenate([order["v0"], order["e1"], order["e2"]], 1).tolist())}
    where = np.array([index[tuple(r)] for r in np.concatenate([t["v0"], t["e1"], t["e2"]], 1).tolist()])  # creation index -> device index
    got = pt.sample_normal_map(NM.probe_rows(p, where[prim]))
    assert not np.isnan(want[~maybe_nan]).any()
    assert_bits(got[~maybe_nan], want[~maybe_nan], "finite rows")
    assert_bits_or_nan(got[maybe_nan], want[maybe_nan], "may-be-NaN rows")
    code, mat = want[:, 3], t["material_idx"][prim]
    assert (code[(mat == 0) & ~maybe_nan] == 1).all(), "strength 0 is the identity"
    assert (code[mat == 4] == 4).all() and (mat == 4).sum() >= 100, "an unbound material"
    assert (code[(mat == 1) | (mat == 2)][:1000] == 0).sum() > 500 and (code[-400:] == 0).all(), "mapped rows, the ground's included"
    out = pt.sample_normal_map(NM.probe_rows(p[:2], [len(t), 0xFFFFFFFF]))
    assert np.array_equal(out, [(0, 0, 0, 5)] * 2), "a primitive outside the scene"
    pt.close()


# ---------------------------------------------------------------- 2. frames against the restatement
_refs = {}


def plain_reference(O, w, h, rng, **kw):
    key = (w, h, rng, tuple(sorted(kw.items())))
    if key not in _refs:
        o, _ = shaded(O, False, w, h, rng_mode=rng, **kw)
        _refs[key] = (transport_ref.render(o, spp=SPP), o)
    return _refs[key]


_base = {}


def base_frame(W, O, w, h, rng, table=True):
    """the TEXTURES|SHADING_NORMALS context's frame and its timed launch counts: the flag absent"""
    key = (w, h, rng, table)
    if key not in _base:
        pt = tracer(W, O, False, w, h, rng_mode=rng, bind={}, slots={}, table=table, mapped_flag=False, batch=3)
        _, launches = pt.render_timed(SPP)
        _base[key] = (pt.accumulated(), launches, pt.shading_normal_timing()[1], pt.texture_timing()[1])
        pt.close()
    return _base[key]


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


@pytest.mark.parametrize("batch", [1, 2, 3])
def test_batches_and_the_second_size_equal_restatement(W, O, batch):
    w, h = SIZES["64x64"]
    want, o = plain_reference(O, w, h, 0)
    pt = tracer(W, O, False, w, h, rng_mode=0, batch=batch)
    pt.render_timed(SPP)
    check(pt, want, o, f"64x64 batch {batch}")
    ms, launches = pt.shading_normal_timing()
    assert launches == (WAVES - 1) * ((SPP + batch - 1) // batch) and ms > 0.0, "booked where the pass it replaces is booked"
    pt.close()


def test_without_a_table_of_normals_equals_restatement(W, O):
    """ns = ng: the new kernels' block-uniform branch"""
    w, h = SIZES["61x37"]
    o, _ = shaded(O, False, w, h, table=False)
    want = transport_ref.render(o, spp=SPP)
    pt = tracer(W, O, False, w, h, table=False)
    pt.render(SPP)
    check(pt, want, o, "no table")
    pt.close()


def test_band_sharding_equals_restatement(W, O):
    w, h = SIZES["61x37"]
    for rank in range(2):
        o, _ = shaded(O, False, w, h, rng_mode=1, miss_floor=0, tile_rank=rank, tile_world=2)
        want = transport_ref.render(A.Local(o), spp=SPP)
        pt = tracer(W, O, False, w, h, rng_mode=1, miss_floor=0, tile_rank=rank, tile_world=2)
        pt.render(SPP)
        check(pt, want, o, f"rank {rank} of 2")
        pt.close()


@pytest.mark.parametrize("flags", ["EMISSION|NEE", "EMISSION|NEE|MIS", "ENVIRONMENT|EMISSION|NEE|ENV_NEE", "ENVIRONMENT|EMISSION|NEE|ENV_NEE|ENV_MIS"])
def test_light_transport_equals_restatement(W, O, flags):
    """the connect pass takes the mapped normal as the receiver's, in the emitter and the map branch, weighed or not"""
    w, h = SIZES["61x37"]
    t, mt, _, _, _ = scene(O, True)
    o, nm = shaded(O, True, w, h, rng_mode=1, miss_floor=0)
    shadow = oracle_of(O, True, w, h)
    em = E.Emission({4: LAMP_E}, triangles=t, materials=mt)
    names = flags.split("|")
    with S.shading_receivers(nm):
        if "ENV_MIS" in names:
            r = X.render_with_env_mis(o, shadow, em, V.EnvLight(V.sun_map()), spp=SPP, parts=True)
        elif "ENV_NEE" in names:
            r = V.render_with_env_nee(o, shadow, em, V.EnvLight(V.sun_map()), spp=SPP, parts=True)
        elif "MIS" in names:
            r = M.render_with_mis(o, shadow, em, spp=SPP, parts=True)
        else:
            r = N.render_with_nee(o, shadow, em, spp=SPP, parts=True)
    assert r["stats"]["light_samples"] + r["stats"]["env_samples"] > 100
    pt = tracer(W, O, True, w, h, flags, rng_mode=1, miss_floor=0)
    if "ENVIRONMENT" in names:
        pt.set_environment(V.sun_map())
    pt.set_emission(4, LAMP_E)
    pt.render(SPP)
    check(pt, r["acc"], o, flags)
    pt.close()


@pytest.mark.parametrize("table", [True, False])
def test_rough_metal_and_glass_sample_about_the_mapped_normal(W, O, table):
    """MICROFACET | ROUGH_DIELECTRIC, the metal and the glass third at alpha 0.3 (rough_glass_nmap_kernel); then the glass smooth again
    (microfacet_nmap_kernel)"""
    w, h = SIZES["61x37"]
    t, mt, _, _, _ = scene(O)
    pt = tracer(W, O, False, w, h, "MICROFACET|ROUGH_DIELECTRIC", table=table)
    for alphas in ({1: 0.3, 2: 0.3}, {1: 0.3}):
        r = RD.RoughGlass(oracle_of(O, False, w, h), t, mt, alphas, mapped_of(O, table=table))
        with RD.MF.rough_weights(r):
            want = T.render_with_textures(r, T.Textures(triangles=t, materials=mt), spp=SPP)
        assert r.sampled > 100 and (r.glass_sampled > 100) == (2 in alphas)
        for m in (1, 2):
            pt.set_roughness(m, alphas.get(m, 0.0))
        pt.render_timed(SPP)
        check(pt, want, r, f"alphas {alphas}")
        assert pt.shading_normal_timing()[1] == 0 and pt.microfacet_timing_ms()[1] > 0, "booked as the microfacet pass"
    pt.close()


def test_retire_equals_restatement(W, O):
    w, h = SIZES["61x37"]
    t, mt, _, _, _ = scene(O, True)
    inner, _ = shaded(O, True, w, h, rng_mode=1)
    o = RR.Retiring(inner, roulette_start=1, q_min=0.25)
    want = E.render_with_emission(o, E.Emission({4: LAMP_E}, triangles=t, materials=mt), spp=SPP, termination=o)
    assert sum(sum(k) for k in o.retired) > 0
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
    inner, _ = shaded(O, False, w, h, rng_mode=1)
    o = A.Masked(inner, mask)
    r = transport_ref.render(o, spp=SPP, parts=True)
    sums = A.Sums(w * h).add(r, mask)
    pt = tracer(W, O, False, w, h, "ADAPTIVE", rng_mode=1)
    pt.set_active_mask(mask)
    pt.render(SPP)
    check(pt, sums.acc, o, "adaptive mask")
    assert np.array_equal(pt.sample_counts().reshape(-1), sums.count)
    pt.close()


@pytest.mark.parametrize("one_slot", [False, True])
def test_a_colour_texture_and_a_normal_map_on_one_material(W, O, one_slot):
    """materials 0 and 3 hold both kinds of binding; one_slot: the normal map's own slot serves as the colour texture too"""
    w, h = SIZES["61x37"]
    t, mt, _, _, _ = scene(O)
    colour = (np.random.default_rng(9).random((32, 48, 3)) * 1.2).astype(F)
    slots = dict(SLOTS) if one_slot else {**SLOTS, 0: (colour, {})}
    cslot = SLOT if one_slot else 0
    o, _ = shaded(O, False, w, h, slots=slots)
    want = T.render_with_textures(o, T.Textures(triangles=t, materials=mt, slots=slots, bind={0: cslot, 3: cslot}, uv=uv_table(O)), spp=SPP)
    pt = tracer(W, O, False, w, h, slots=slots)
    for m in (0, 3):
        pt.bind_texture(m, cslot)
    pt.render(SPP)
    check(pt, want, o, f"both kinds, one slot {one_slot}")
    assert pt.normal_map(0) == (SLOT, 1.0) and pt.normal_map(4) == (None, 0.0)
    pt.close()


def test_aov_normal_is_the_mapped_normal(W, O):
    w, h = SIZES["61x37"]
    t = scene(O)[0]
    nm = mapped_of(O)
    o = oracle_of(O, False, w, h)
    gx, gy = (w + 7) // 8, (h + 7) // 8
    total = np.zeros((w * h, 3), F)
    for k in range(SPP):
        o.set_frame(1 + k, 0)
        o.set_counters([0, 0, gx * gy * 64])
        o.generate_rays(gx, gy, True)
        o.extend(*O.workgroup_size_64(gx * gy * 64))
        hits = o.hits(int(o.counters()[1]))
        rays = o.rays()[hits["ray_idx"].astype(np.int64)]
        p = rays["origin"][:, :3] + hits["t"][:, None] * rays["direction"][:, :3]
        add = np.zeros_like(total)
        add[rays["pixel_idx"]] = nm.at(hits["sphere_idx"].astype(np.int64), p)[0]
        total = total + add
    pt = tracer(W, O, False, w, h, "AOV")
    pt.render(SPP)
    assert_bits(pt.aov("normal").reshape(-1, 3), total / F(SPP), "the AOV normal")
    pt.close()


# ---------------------------------------------------------------- 3. identity and non-identity
@pytest.mark.parametrize("loop", ["", "UNFUSED", "NO_LDS_SCENE"])
def test_nothing_bound_strength_zero_and_a_flat_map_are_the_unflagged_frame(W, O, loop):
    w, h = SIZES["61x37"]
    want, launches, sn_launches, tex_launches = base_frame(W, O, w, h, 0) if not loop else (None,) * 4
    if loop:
        ref = tracer(W, O, False, w, h, loop, rng_mode=0, bind={}, slots={}, mapped_flag=False, batch=3)
        _, launches = ref.render_timed(SPP)
        want, sn_launches, tex_launches = ref.accumulated(), ref.shading_normal_timing()[1], ref.texture_timing()[1]
        ref.close()
    pt = tracer(W, O, False, w, h, loop, rng_mode=0, bind={}, batch=3)
    _, got = pt.render_timed(SPP)
    assert_bits(pt.accumulated(), want, "the flag with nothing bound")
    assert np.array_equal(got, launches) and pt.shading_normal_timing()[1] == sn_launches and pt.texture_timing()[1] == tex_launches, \
        "nothing bound: the launches of the unflagged context"
    for m in range(4):
        pt.bind_normal_map(m, SLOT, 0.0)
    pt.render(SPP)
    assert_bits(pt.accumulated(), want, "strength 0")
    pt.set_texture(SLOT, NM.flat_map(), filter="nearest")  # (the bindings stay)
    for m in range(4):
        pt.bind_normal_map(m, SLOT, 1.0)
    assert pt.normal_map(2) == (SLOT, 1.0)
    pt.render(SPP)
    assert_bits(pt.accumulated(), want, "an all-(0.5, 0.5, 1) map")
    pt.close()


def test_a_bound_map_changes_most_of_the_sphere(W, O):
    """against a pass that silently copies: more than half of the pixels that see the sphere differ from the unmapped frame"""
    w, h = SIZES["61x37"]
    t = scene(O)[0]
    base = base_frame(W, O, w, h, 0)[0]
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
    sees[rays["pixel_idx"][t["material_idx"][hits["sphere_idx"].astype(np.int64)] < 3]] = True
    assert sees.sum() > 200 and changed[sees].mean() > 0.5, (int(sees.sum()), float(changed[sees].mean()))


# ---------------------------------------------------------------- 4. life cycle and refusals
def test_clear_texture_unbinds_and_scene_updates_keep_the_binding(W, O):
    w, h = SIZES["61x37"]
    t, mt, n9, _, created = scene(O)
    want, o = plain_reference(O, w, h, 0)
    base = base_frame(W, O, w, h, 0)[0]
    pt = tracer(W, O, False, w, h, rng_mode=0)
    pt.render(1)
    far = created.copy()
    far["_pad"][5] = len(n9)
    with pytest.raises(W.WfptError):
        pt.update_scene(W.Scene(np.zeros(0, W.SPHERE), mt.copy(), triangles=far))  # a row beyond the UV table
    sp = np.zeros(1, W.SPHERE)
    sp["radius"] = 1.0
    with pytest.raises(W.WfptError):
        pt.update_scene(W.Scene(sp, mt.copy()))  # to spheres while a map is bound
    pt.render(SPP - 1)
    check(pt, want, o, "after two refused updates the render goes on")
    pt.update_scene(W.Scene(np.zeros(0, W.SPHERE), mt.copy(), triangles=created.copy()[::-1].copy()))
    assert pt.normal_map(1) == (SLOT, 1.0)
    pt.render(SPP)
    check(pt, want, o, "after an update to the same scene")
    pt.clear_texture(SLOT)
    assert all(pt.normal_map(m) == (None, 0.0) for m in range(5))
    pt.render(SPP)
    assert_bits(pt.accumulated(), base, "the slot cleared: the unbound frame")
    with pytest.raises(W.WfptError):
        pt.sample_normal_map(np.zeros((1, 4), F))  # nothing is bound
    pt.set_texture(SLOT, SLOTS[SLOT][0])
    pt.bind_normal_map(2, SLOT, 2.0)
    pt.bind_normal_map(2, None)
    pt.render(SPP)
    assert_bits(pt.accumulated(), base, "bound and unbound again")
    pt.close()


def test_refusals(W, O):
    w, h = 16, 16
    t, mt, n9, _, created = scene(O)
    sc = W.Scene(np.zeros(0, W.SPHERE), mt.copy(), triangles=created.copy())
    cc = W.CameraController(W.Camera((0.0, 1.0, 4.5), (0.0, -0.1, 0.0)), 40.0, 0.0, 10.0, 0.1, 100.0)
    for flags in ("NORMAL_MAPS", "NORMAL_MAPS|TEXTURES", "NORMAL_MAPS|SHADING_NORMALS", BASE + "|NORMAL_MAPS|EMISSION|NEE|LIGHT_POWER",
                  BASE + "|NORMAL_MAPS|EMISSION|NEE|ANALYTIC_LIGHTS"):
        with pytest.raises(W.WfptError):
            W.PathTracer(sc, W.RenderParameters(cc, (w, h)), flags=flags_of(W, flags), max_wavefronts=WAVES)
    sphere = W.shirley_path_tracer(w, h, flags=flags_of(W, BASE + "|NORMAL_MAPS"))
    sphere.set_texture(SLOT, SLOTS[SLOT][0])
    with pytest.raises(W.WfptError):
        sphere.bind_normal_map(0, SLOT, 1.0)
    sphere.close()
    unflagged = tracer(W, O, False, w, h, bind={}, mapped_flag=False)
    for call in (lambda: unflagged.bind_normal_map(0, SLOT, 1.0), lambda: unflagged.normal_map(0),
                 lambda: unflagged.sample_normal_map(np.zeros((1, 4), F))):
        with pytest.raises(W.WfptError):
            call()
    unflagged.close()
    pt = tracer(W, O, False, w, h)
    pt.render(2)
    before = pt.accumulated()
    for call in (lambda: pt.bind_normal_map(5, SLOT, 1.0), lambda: pt.bind_normal_map(0, 0, 1.0), lambda: pt.bind_normal_map(0, W.MAX_TEXTURES, 1.0),
                 lambda: pt.bind_normal_map(0, -2, 1.0), lambda: pt.bind_normal_map(0, SLOT, np.nan), lambda: pt.bind_normal_map(0, SLOT, np.inf),
                 lambda: pt.bind_normal_map(0, SLOT, -1.0), lambda: pt.normal_map(5)):
        with pytest.raises(W.WfptError) as e:
            call()
        assert e.value.status == W.ERR_INVALID_ARGUMENT
    assert_bits(pt.accumulated(), before, "a refused call restarted the accumulation")
    assert pt.normal_map(0) == (SLOT, 1.0)
    pt.render(1)
    assert W.lib().wfpt_accumulated_samples(pt.handle) == 3
    pt.bind_normal_map(0, SLOT, 0.5)
    assert W.lib().wfpt_accumulated_samples(pt.handle) == 0, "a bind restarts the accumulation"
    pt.close()
    binned = W.PathTracer(sc, W.RenderParameters(cc, (200, 120)), flags=flags_of(W, BASE + "|NORMAL_MAPS|BINNING"), max_wavefronts=WAVES,
                          rng_mode=W.RNG_PIXEL)
    assert binned.loop_kind == "fused_binned"
    with pytest.raises(W.WfptError) as e:
        binned.bind_normal_map(0, SLOT, 1.0)
    assert e.value.status == W.ERR_UNSUPPORTED
    binned.bind_normal_map(0, None)  # (nothing the loop has no form of)
    assert binned.loop_kind == "fused_binned"
    binned.close()
