"""Per-vertex shading normals (WFPT_FLAG_SHADING_NORMALS, include/wfpt.h "Shading normals") on the GPU.

The device's interpolation and whole renders are compared bit for bit with tests/shading_normals_ref.py: the numpy float32 restatement of
steps 1-5 and of scatter() about the shading normal, driven through the oracle's stages. The scene: a 320-triangle icosphere of radius 1
(Lambertian, fuzzy metal and glass by thirds, corner normals = corner positions) over a two-triangle ground, 3 samples, 4 wavefronts."""
import numpy as np
import pytest

import adaptive_ref as A
import emission_ref as E
import env_mis_ref as X
import env_nee_ref as V
import mis_ref as M
import nee_ref as N
import retire_ref as RR
import shading_normals_ref as S
import texture_ref as T
import transport_ref
from helpers import assert_bits_or_nan

pytestmark = pytest.mark.gpu

F = np.float32
SPP, WAVES, FLOOR = 3, 4, 16
LAMP_E = (8.0, 4.0, 16.0)
SIZES = {"61x37": (61, 37), "64x64": (64, 64)}


@pytest.fixture(scope="module")
def W():
    import wavefront_path_tracer_amd as W
    return W


@pytest.fixture(scope="module")
def O():
    from oracle import oracle as O
    return O


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def assert_bits(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = g != w
    assert not bad.any(), f"{what}: {int(bad.sum())} of {g.size} values differ, first at {np.argwhere(bad)[0]}"


def flags_of(W, names):
    f = 0
    for name in (names.split("|") if names else []):
        f |= getattr(W, "FLAG_" + name)
    return f


_scenes = {}


def scene(O, emitter=False):
    """(triangles in the device's order, materials, the table, nodes, triangles in creation order), built once"""
    if emitter not in _scenes:
        created, mt, n9 = S.sphere_scene(O, emitter=emitter)
        t, nodes = O.build_bvh_triangles(created, 32)
        _scenes[emitter] = (t, mt, n9, nodes, created)
    return _scenes[emitter]


def oracle_of(O, emitter, w, h, **kw):
    t, mt, _, nodes, _ = scene(O, emitter)
    cam, ip, vw = S.sphere_camera(O, w, h)
    kw.setdefault("max_wavefronts", WAVES)
    kw.setdefault("miss_floor", FLOOR)
    return O.Oracle(w, h, np.zeros(1, O.SPHERE), mt, nodes, cam, ip, vw, triangles=t, **kw)


def tracer(W, O, emitter, w, h, flags="", table=True, **kw):
    t, mt, n9, _, created = scene(O, emitter)
    sc = W.Scene(np.zeros(0, W.SPHERE), mt.copy(), triangles=created.copy())
    cc = W.CameraController(W.Camera((0.0, 1.0, 4.5), (0.0, -0.1, 0.0)), 40.0, 0.0, 10.0, 0.1, 100.0)
    kw.setdefault("max_wavefronts", WAVES)
    kw.setdefault("miss_floor", FLOOR)
    f = flags if isinstance(flags, int) else flags_of(W, flags)
    pt = W.PathTracer(sc, W.RenderParameters(cc, (w, h)), flags=W.FLAG_SHADING_NORMALS | f, **kw)
    assert np.array_equal(pt.scene.triangles, t), "the tracer's triangles are not in the oracle's order"
    if table:
        pt.set_triangle_normals(n9)
    return pt


def shaded(O, emitter, w, h, **kw):
    t, mt, n9, _, _ = scene(O, emitter)
    nm = S.Normals(t, n9)
    return S.Shaded(oracle_of(O, emitter, w, h, **kw), nm, mt), nm


def check(pt, want, o, what):
    assert_bits(pt.accumulated(), want, what)
    assert np.array_equal(pt.bounce_table(), o.bounce_table()), f"{what}: bounce table\n{pt.bounce_table()}\nvs\n{o.bounce_table()}"


# ---------------------------------------------------------------- 1. the interpolation alone
def probe_points(O):
    """(p, prim, may be NaN) over a scene of its own: the icosphere plus a degenerate triangle, a triangle whose normals face away from
    its stored normal, and one with a zero row"""
    t, _, n9, _, _ = scene(O)
    t, n9 = t.copy(), n9.copy()
    extra = np.zeros(3, t.dtype)
    extra["v0"][:, 0] = (3.0, 5.0, 7.0)
    extra["e1"][:] = (1.0, 0.0, 0.0)
    extra["e2"][:] = (0.0, 1.0, 0.5)
    extra["e2"][0] = (2.0, 0.0, 0.0)  # den = 0, the stored normal is NaN
    extra["_pad"] = len(n9) + np.arange(3)
    rows = np.zeros((3, 9), F)
    rows[0] = (0, 0, 1) * 3
    rows[1] = (0, 1, -2, 0, 1, -2, 1, 1, -2)  # faces away from ng = normalize(cross(e1, e2)) = (0, -0.5, 1) / |.|
    t, n9 = np.concatenate([t, extra]), np.concatenate([n9, rows])
    rng = np.random.default_rng(11)
    n_s = len(t) - 3
    prim = rng.choice(np.flatnonzero(t["material_idx"][:n_s] < 3), 4000)  # the icosphere's faces (the ground's rows are zero)
    b = rng.dirichlet((1.0, 1.0, 1.0), 4000)
    b[:600] = np.eye(3)[rng.integers(0, 3, 600)]                                 # corners
    b[600:1200] = (np.ones((3, 3)) - np.eye(3))[rng.integers(0, 3, 600)] / 2.0    # edge midpoints
    b[1200:1800] = 1.0 / 3.0                                                      # centroids
    b[1800:2400] = rng.uniform(-2.0, 3.0, (600, 3))                               # outside the triangle (negative b)
    prim[2400:2500], prim[2500:2600], prim[2600:2700] = n_s, n_s + 1, n_s + 2
    v0, e1, e2 = (t[k][prim].astype(np.float64) for k in ("v0", "e1", "e2"))
    p = (v0 + e1 * b[:, 1:2] + e2 * b[:, 2:3]).astype(F)
    p[2700:2710] = np.nan
    p[2710:2720, 1] = np.inf
    maybe_nan = (prim == n_s) | ~np.isfinite(p).all(axis=1)
    return t, n9, p, prim, maybe_nan


def test_sample_shading_normal_equals_restatement(W, O):
    t, n9, p, prim, maybe_nan = probe_points(O)
    nm = S.Normals(t, n9)
    want = nm.sample_rows(p, prim)
    mt = scene(O)[1]
    cc = W.CameraController(W.Camera((0.0, 1.0, 4.5), (0.0, -0.1, 0.0)), 40.0, 0.0, 10.0, 0.1, 100.0)
    tree = W.BVHTree(len(t))
    order = t.copy()
    tree.build_bvh_tree_triangles(order, 32)
    pt = W.PathTracer(W.Scene(np.zeros(0, W.SPHERE), mt, triangles=order), W.RenderParameters(cc, (16, 16)), flags=W.FLAG_SHADING_NORMALS,
                      bvh=tree)
    pt.set_triangle_normals(n9)
    assert_bits(pt.triangle_normals(), nm.rows, "the table as stored")
    index = {tuple(r): i for i, r in enumerate(np.concatenate([order["v0"], order["e1"], order["e2"]], 1).tolist())}
    where = np.array([index[tuple(r)] for r in np.concatenate([t["v0"], t["e1"], t["e2"]], 1).tolist()])  # creation index -> device index
    got = pt.sample_shading_normal(S.probe_rows(p, where[prim]))
    assert not np.isnan(want[~maybe_nan]).any()
    assert_bits(got[~maybe_nan], want[~maybe_nan], "finite rows")
    assert_bits_or_nan(got[maybe_nan], want[maybe_nan], "may-be-NaN rows")
    fell = want[:, 3] == 1
    assert fell[2400:2720].all() and not fell[:1800].any(), "the classes are not what they are meant to be"
    out = pt.sample_shading_normal(S.probe_rows(p[:2], [len(t), 0xFFFFFFFF]))
    assert np.array_equal(out, [(0, 0, 0, 1)] * 2), "a primitive outside the scene"
    pt.close()


# ---------------------------------------------------------------- 2. frames against the restatement
_refs = {}


def plain_reference(O, w, h, rng, **kw):
    key = (w, h, rng, tuple(sorted(kw.items())))
    if key not in _refs:
        o, _ = shaded(O, False, w, h, rng_mode=rng, **kw)
        _refs[key] = (transport_ref.render(o, spp=SPP), o)
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
    assert not np.array_equal(bits(want), bits(unflagged)), "the table changed nothing"
    pt.close()


@pytest.mark.parametrize("batch", [1, 3])
def test_batches_and_the_second_size_equal_restatement(W, O, batch):
    w, h = SIZES["64x64"]
    want, o = plain_reference(O, w, h, 0)
    pt = tracer(W, O, False, w, h, rng_mode=0, batch=batch)
    pt.render(SPP)
    check(pt, want, o, f"64x64 batch {batch}")
    ms, launches = pt.shading_normal_timing()
    assert launches == 0
    pt.close()


def test_timed_render_books_the_pass_apart(W, O):
    w, h = SIZES["64x64"]
    want, o = plain_reference(O, w, h, 0)
    pt = tracer(W, O, False, w, h, rng_mode=0, batch=3)
    stage_ms, stage_launches = pt.render_timed(SPP)
    check(pt, want, o, "timed render")
    ms, launches = pt.shading_normal_timing()
    assert launches == WAVES - 1 and ms > 0.0, "one launch before every shade step that scatters"
    pt.close()


def test_timed_render_books_every_pass_in_its_own_counter(W, O):
    """A context with all five passes that are no stage of render_timed's arrays -- AOV, texture, emission, connect, shading normals -- on
    a 64-triangle mesh, 16 x 16, one sample in flight, N = 3 wavefronts. Per timed sample: one AOV launch; a texture, an emission and a
    connect launch before each of the N shade steps, the second plane's memset at the head of the batch booked with the emission
    launches; a shading-normal launch before the N - 1 shade steps that scatter."""
    n_waves = 3
    sc = W.Scene.random_mesh(64, 1)
    cc = W.CameraController(W.Camera((0.0, 0.0, 30.0), (0.0, 0.0, 0.0)), 40.0, 0.0, 10.0, 0.1, 100.0)
    pt = W.PathTracer(sc, W.RenderParameters(cc, (16, 16)), max_wavefronts=n_waves, batch=1,
                      flags=flags_of(W, "AOV|TEXTURES|EMISSION|NEE|SHADING_NORMALS"))
    tri = pt.scene.triangles
    rows = int(tri["_pad"].max()) + 1
    rng = np.random.default_rng(21)
    pt.set_texture(0, rng.random((4, 8, 3)).astype(F))
    pt.bind_texture(int(tri["material_idx"][1]), 0)
    pt.set_triangle_uvs(rng.random((rows, 6)).astype(F))
    pt.set_emission(int(tri["material_idx"][0]), LAMP_E)
    pt.set_triangle_normals(rng.standard_normal((rows, 9)).astype(F))
    assert pt.loop_kind == "fused" and pt.nee_light_count() > 0
    timings = (pt.aov_timing, pt.texture_timing, pt.emission_timing, pt.nee_timing, pt.shading_normal_timing)
    per_sample = np.array([1, n_waves, n_waves + 1, n_waves, n_waves - 1])
    assert [t() for t in timings] == [(0.0, 0)] * 5
    stage_ms, stage_launches = pt.render_timed(1)
    # the stages' own array holds the fused loop's chain and nothing of the passes: bounce<first>, then N - 1 times (scan, bounce<middle>),
    # scan, bounce<last>, accumulate (the library of the commit before the pass array returns this array for this context:
    # [0, 0, 0, 0, 1, 0, 0, 0, 3, 1, 2, 1, 0])
    want = np.zeros(W.STAGE_COUNT, np.uint32)
    for name, n in (("bounce_first", 1), ("scan", n_waves), ("bounce", n_waves - 1), ("bounce_last", 1), ("accumulate", 1)):
        want[W.STAGES[name]] = n
    assert want.tolist() == [0, 0, 0, 0, 1, 0, 0, 0, 3, 1, 2, 1, 0]
    assert stage_launches.tolist() == want.tolist()
    assert np.array_equal(stage_ms > 0, want > 0), "a stage's time without its launches, or the reverse"
    assert [t()[1] for t in timings] == per_sample.tolist()
    assert all(t()[0] > 0.0 for t in timings)
    _, again = pt.render_timed(1)
    assert [t()[1] for t in timings] == (2 * per_sample).tolist()
    assert np.array_equal(again, stage_launches), "the stages' own counts are per call"
    pt.render(1)
    assert [t()[1] for t in timings] == (2 * per_sample).tolist(), "an untimed render books nothing"
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


def textures(O):
    n = len(scene(O)[2])
    uv = np.random.default_rng(8).uniform(-1.5, 2.5, (n, 6)).astype(F)
    img = (np.random.default_rng(9).random((32, 48, 3)) * 1.2).astype(F)
    return {0: (img, {})}, {0: 0, 3: 0}, uv


def test_textures_equal_restatement(W, O):
    w, h = SIZES["61x37"]
    slots, bind, uv = textures(O)
    t, mt, n9, _, _ = scene(O)
    o, _ = shaded(O, False, w, h)
    want = T.render_with_textures(o, T.Textures(triangles=t, materials=mt, slots=slots, bind=bind, uv=uv), spp=SPP)
    pt = tracer(W, O, False, w, h, "TEXTURES")
    pt.set_texture(0, slots[0][0])
    for m, s in bind.items():
        pt.bind_texture(m, s)
    pt.set_triangle_uvs(uv)
    pt.render(SPP)
    check(pt, want, o, "textures")
    pt.close()


@pytest.mark.parametrize("flags,loop", [("EMISSION|NEE", ""), ("EMISSION|NEE|MIS", ""), ("ENVIRONMENT|EMISSION|NEE|ENV_NEE", ""),
                                        ("ENVIRONMENT|EMISSION|NEE|ENV_NEE|ENV_MIS", ""), ("EMISSION|NEE|MIS", "UNFUSED"),
                                        ("ENVIRONMENT|EMISSION|NEE|ENV_NEE", "UNFUSED"), ("EMISSION|NEE|MIS", "NO_LDS_SCENE"),
                                        ("ENVIRONMENT|EMISSION|NEE|ENV_NEE", "NO_LDS_SCENE")])
def test_light_transport_equals_restatement(W, O, flags, loop):
    """the connect pass takes the shading normal as the receiver's, in the emitter and the map branch, weighed or not"""
    w, h = SIZES["61x37"]
    t, mt, n9, _, _ = scene(O, True)
    o, nm = shaded(O, True, w, h, rng_mode=1, miss_floor=0)
    shadow = oracle_of(O, True, w, h)
    em = E.Emission({4: LAMP_E}, triangles=t, materials=mt)
    names = flags.split("|")  # ("MIS" is a substring of "EMISSION")
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
    pt = tracer(W, O, True, w, h, flags + ("|" + loop if loop else ""), rng_mode=1, miss_floor=0)
    if "ENVIRONMENT" in names:
        pt.set_environment(V.sun_map())
    pt.set_emission(4, LAMP_E)
    pt.render(SPP)
    check(pt, r["acc"], o, f"{flags} {loop}")
    pt.close()


def test_retire_equals_restatement(W, O):
    w, h = SIZES["61x37"]
    t, mt, n9, _, _ = scene(O, True)
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
    t, mt, n9, _, _ = scene(O)
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


def test_aov_normal_is_the_shading_normal(W, O):
    w, h = SIZES["61x37"]
    t, mt, n9, _, _ = scene(O)
    nm = S.Normals(t, n9)
    o = oracle_of(O, False, w, h)
    gx, gy = (w + 7) // 8, (h + 7) // 8
    total, flat = np.zeros((w * h, 3), F), np.zeros((w * h, 3), F)
    for k in range(SPP):
        o.set_frame(1 + k, 0)
        o.set_counters([0, 0, gx * gy * 64])
        o.generate_rays(gx, gy, True)
        o.extend(*O.workgroup_size_64(gx * gy * 64))
        hits = o.hits(int(o.counters()[1]))
        rays = o.rays()[hits["ray_idx"].astype(np.int64)]
        p = rays["origin"][:, :3] + hits["t"][:, None] * rays["direction"][:, :3]
        prim = hits["sphere_idx"].astype(np.int64)
        add, add_flat = np.zeros_like(total), np.zeros_like(total)
        add[rays["pixel_idx"]] = nm.at(prim, p)[0]
        add_flat[rays["pixel_idx"]] = transport_ref.triangle_normal_area(t[prim])[0]
        total, flat = total + add, flat + add_flat
    pt = tracer(W, O, False, w, h, "AOV")
    pt.render(SPP)
    assert_bits(pt.aov("normal").reshape(-1, 3), total / F(SPP), "the AOV normal")
    pt.set_triangle_normals(None)
    pt.render(SPP)
    assert_bits(pt.aov("normal").reshape(-1, 3), flat / F(SPP), "the AOV normal without a table")
    pt.close()


# ---------------------------------------------------------------- 3. identity
@pytest.mark.parametrize("loop", ["", "UNFUSED", "NO_LDS_SCENE"])
def test_no_table_and_a_flat_table_are_the_unflagged_frame(W, O, loop):
    w, h = SIZES["61x37"]
    t, mt, n9, _, created = scene(O)
    want = oracle_of(O, False, w, h).render(SPP)
    pt = tracer(W, O, False, w, h, loop, table=False, batch=3)
    pt.render_timed(SPP)
    assert_bits(pt.accumulated(), want, "flag set, no table")
    assert pt.shading_normal_timing() == (0.0, 0) and len(pt.triangle_normals()) == 0
    pt.set_triangle_normals(np.zeros_like(n9))
    pt.render_timed(SPP)
    assert_bits(pt.accumulated(), want, "an all-zero table")
    assert pt.shading_normal_timing()[1] == WAVES - 1
    pt.set_triangle_normals(n9)
    pt.render(SPP)
    assert not np.array_equal(bits(pt.accumulated()), bits(want))
    pt.set_triangle_normals(None)
    pt.render(SPP)
    assert_bits(pt.accumulated(), want, "the table cleared")
    pt.close()


# ---------------------------------------------------------------- 4. scene updates and refusals
def test_update_scene_keeps_the_table_and_refuses_a_row_beyond_it(W, O):
    w, h = SIZES["61x37"]
    t, mt, n9, _, created = scene(O)
    want, o = plain_reference(O, w, h, 0)
    pt = tracer(W, O, False, w, h, rng_mode=0)
    pt.render(1)
    far = created.copy()
    far["_pad"][5] = len(n9)
    with pytest.raises(W.WfptError):
        pt.update_scene(W.Scene(np.zeros(0, W.SPHERE), mt.copy(), triangles=far))
    sp = np.zeros(1, W.SPHERE)
    sp["radius"] = 1.0
    with pytest.raises(W.WfptError):
        pt.update_scene(W.Scene(sp, mt.copy()))
    pt.render(SPP - 1)
    check(pt, want, o, "after two refused updates the render goes on")
    shuffled = created.copy()[::-1].copy()  # another order in, the same scene: the rows follow the triangles
    pt.update_scene(W.Scene(np.zeros(0, W.SPHERE), mt.copy(), triangles=shuffled))
    pt.render(SPP)
    check(pt, want, o, "after an update to the same scene")
    pt.close()


def test_refusals(W, O):
    w, h = 16, 16
    t, mt, n9, _, created = scene(O)
    for other in ("LIGHT_POWER", "ANALYTIC_LIGHTS"):
        with pytest.raises(W.WfptError):
            tracer(W, O, False, w, h, "EMISSION|NEE|" + other, table=False)
    sphere = W.shirley_path_tracer(w, h, flags=W.FLAG_SHADING_NORMALS)
    with pytest.raises(W.WfptError):
        sphere.set_triangle_normals(n9)
    sphere.close()
    sc = W.Scene(np.zeros(0, W.SPHERE), mt.copy(), triangles=created.copy())
    cc = W.CameraController(W.Camera((0.0, 1.0, 4.5), (0.0, -0.1, 0.0)), 40.0, 0.0, 10.0, 0.1, 100.0)
    unflagged = W.PathTracer(sc, W.RenderParameters(cc, (w, h)), max_wavefronts=WAVES)
    for call in (lambda: unflagged.set_triangle_normals(n9), unflagged.triangle_normals, unflagged.shading_normal_timing,
                 lambda: unflagged.sample_shading_normal(np.zeros((1, 4), F))):
        with pytest.raises(W.WfptError):
            call()
    unflagged.close()
    pt = tracer(W, O, False, w, h)
    pt.render(2)
    before, stored = pt.accumulated(), pt.triangle_normals()
    for bad in (np.nan, np.inf):
        rows = n9.copy()
        rows[17, 4] = bad
        with pytest.raises(W.WfptError):
            pt.set_triangle_normals(rows)
    with pytest.raises(W.WfptError):
        pt.set_triangle_normals(n9[:-1])  # a triangle's row is beyond the table
    assert_bits(pt.accumulated(), before, "a refused call restarted the accumulation")
    assert_bits(pt.triangle_normals(), stored, "a refused call changed the table")
    pt.render(1)
    assert W.lib().wfpt_accumulated_samples(pt.handle) == 3
    pt.set_triangle_normals(None)
    with pytest.raises(W.WfptError):
        pt.sample_shading_normal(np.zeros((1, 4), F))  # no table is set
    pt.close()
