"""Surface textures (WFPT_FLAG_TEXTURES, include/wfpt.h "Textures") on the GPU.

The device lookup and whole textured renders are compared bit for bit with tests/texture_ref.py: the numpy float32 restatement of the UVs
and the lookup, and the oracle's stages driven from Python with the texture applied where its shade multiplies by the albedo."""
import hashlib
import os

import numpy as np
import pytest

import texture_ref as T

pytestmark = pytest.mark.gpu

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


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
    assert not bad.any(), f"{what}: {int(bad.sum())} values differ, first at {np.argwhere(bad)[0]}"


def random_tex(w, h, seed):
    return (np.random.default_rng(seed).random((h, w, 3)) * 1.2).astype(F)


def checker(n, cells=16):
    y, x = np.mgrid[0:n, 0:n]
    c = ((x * cells // n + y * cells // n) % 2).astype(F)
    return np.stack([0.2 + 0.7 * c, 0.3 + 0.5 * c, 0.1 + 0.8 * c], axis=-1).astype(F)


def probe_uvs(n=100000, seed=5):
    rng = np.random.default_rng(seed)
    uv = rng.uniform(-3.0, 3.0, (n, 2)).astype(F)
    uv[: n // 10] *= F(1000.0)  # large values
    special = [(0, 0), (1, 1), (-0.0, 0), (1e-9, -1e-9), (-1e-9, 1e-9), (0.5, 0.5), (0.999999, 0.000001), (-1, -1), (2, 3),
               (1 - 2 ** -24, 1 - 2 ** -24), (-2 ** -30, 0.25)]  # seams: either side of the wrap
    return np.concatenate([np.asarray(special, F), uv])


# ---------------------------------------------------------------- the scenes
SHIRLEY_W, SHIRLEY_H = 400, 224


def shirley_textures(O, sp, mt):
    """A checker on the ground sphere's material, random textures (both filters, scaled and offset) on some Lambertian, metal and
    dielectric materials."""
    ground = int(sp["material_idx"][np.argmax(sp["radius"])])
    kinds = mt["material_type"]
    pick = [int(np.flatnonzero(kinds == k)[j]) for k in (0, 1, 2) for j in (0, 1) if (np.flatnonzero(kinds == k)).size > j]
    pick = [m for m in pick if m != ground]
    slots = {0: (checker(256), {}),
             1: (random_tex(64, 32, 1), {"scale": (3.0, 2.0), "offset": (0.25, -0.5)}),
             2: (random_tex(17, 9, 2), {"filter": "nearest"})}
    bind = {ground: 0}
    for k, m in enumerate(pick):
        bind[m] = 1 + k % 2
    return slots, bind


def apply(pt, slots, bind, uv=None):
    for s, (img, params) in slots.items():
        pt.set_texture(s, img, **params)
    for m, s in bind.items():
        pt.bind_texture(m, s)
    if uv is not None:
        pt.set_triangle_uvs(uv)


def test_sample_texture_equals_restatement(W):
    pt = W.shirley_path_tracer(16, 16, flags=W.FLAG_TEXTURES)
    uv = probe_uvs()
    for s, (img, params) in enumerate([(random_tex(1, 1, 3), {}), (random_tex(3, 2, 4), {"scale": (1.5, -2.0), "offset": (0.1, 7.0)}),
                                       (random_tex(64, 48, 5), {}), (random_tex(2048, 1024, 6), {"offset": (-0.3, 0.2)}),
                                       (random_tex(1025, 1024, 7), {})]):  # (a whole piece of the upload and a partial one)
        for flt in ("bilinear", "nearest"):
            pt.set_texture(s, img, filter=flt, **params)
            assert_bits(pt.sample_texture(s, uv), T.tex_lookup(img, uv[:, 0], uv[:, 1], filter=flt, **params), f"{img.shape} {flt}")
    pt.close()


@pytest.mark.parametrize("flags", [0, "UNFUSED", "SPLIT_SHADE"])
@pytest.mark.parametrize("rng", ["dispatch", "pixel"])
def test_shirley_equals_restatement(W, O, flags, rng):
    mode = W.RNG_DISPATCH if rng == "dispatch" else W.RNG_PIXEL
    f = W.FLAG_TEXTURES | (getattr(W, "FLAG_" + flags) if flags else 0)
    sp, mt = O.scene_book_one_final(1)
    sp, _ = O.build_bvh(sp)
    slots, bind = shirley_textures(O, sp, mt)
    pt = W.shirley_path_tracer(SHIRLEY_W, SHIRLEY_H, max_wavefronts=8, rng_mode=mode, flags=f)
    apply(pt, slots, bind)
    pt.render(2)
    got = pt.accumulated()
    o = O.shirley_oracle(SHIRLEY_W, SHIRLEY_H, max_wavefronts=8, rng_mode=mode)
    want = T.render_with_textures(o, T.Textures(spheres=sp, materials=mt, slots=slots, bind=bind), spp=2)
    assert_bits(got, want, f"shirley {flags} {rng}")
    plain = O.shirley_oracle(SHIRLEY_W, SHIRLEY_H, max_wavefronts=8, rng_mode=mode).render(2)
    assert not np.array_equal(bits(got), bits(plain)), "the textures changed nothing"
    pt.close()


def mesh_uv_inputs(O, w, h, n=5000):
    tris, mt = O.scene_random_mesh(n, 1)
    tris["_pad"] = np.arange(n, dtype=np.uint32)[::-1]  # row i of the table belongs to triangle n - 1 - i of the file order
    uv = np.random.default_rng(8).uniform(-1.5, 2.5, (n, 6)).astype(F)
    tris, nodes = O.build_bvh_triangles(tris, 32)
    cam, ip, vw = O.mesh_camera(w, h)
    return tris, mt, nodes, cam, ip, vw, uv


def mesh_tracer(W, w, h, n=5000, **kw):
    scene = W.Scene.random_mesh(n, 1)
    scene.triangles["_pad"] = np.arange(n, dtype=np.uint32)[::-1]
    cc = W.CameraController(W.Camera((0.0, 0.0, 30.0), (0.0, 0.0, 0.0)), 40.0, 0.0, 10.0, 0.1, 100.0)
    return W.PathTracer(scene, W.RenderParameters(cc, (w, h)), **kw)


MESH_SLOTS = {0: (random_tex(128, 128, 11), {}), 5: (random_tex(9, 31, 12), {"filter": "nearest", "scale": (2.0, 0.5)})}
MESH_BIND = {0: 0, 2: 5}


@pytest.mark.parametrize("flags", [0, "EXACT_TRAVERSAL", "NO_LDS_SCENE", "NO_LDS_SCENE|EXACT_TRAVERSAL"])
def test_mesh_equals_restatement(W, O, flags):
    w, h = 200, 120
    f = W.FLAG_TEXTURES
    for name in (flags.split("|") if flags else []):
        f |= getattr(W, "FLAG_" + name)
    tris, mt, nodes, cam, ip, vw, uv = mesh_uv_inputs(O, w, h)
    pt = mesh_tracer(W, w, h, max_wavefronts=8, flags=f)
    if flags == "NO_LDS_SCENE":
        assert pt.loop_kind == "refill"
    apply(pt, MESH_SLOTS, MESH_BIND, uv)
    pt.render(2)
    o = O.Oracle(w, h, np.zeros(1, O.SPHERE), mt, nodes, cam, ip, vw, triangles=tris, max_wavefronts=8)
    want = T.render_with_textures(o, T.Textures(triangles=tris, materials=mt, slots=MESH_SLOTS, bind=MESH_BIND, uv=uv), spp=2)
    assert_bits(pt.accumulated(), want, f"mesh {flags}")
    pt.close()


def test_same_bits_across_loops_batches_stage_loop_and_shards(W, O):
    """(miss_floor 0: a band-sharded context counts only its own misses against the floor, so with a floor its loop may exit elsewhere)"""
    w, h, spp = 72, 48, 4
    sp, mt = O.scene_book_one_final(1)
    sp, _ = O.build_bvh(sp)
    slots, bind = shirley_textures(O, sp, mt)
    base = None
    for flags, batch in [(0, 0), (W.FLAG_UNFUSED, 0), (W.FLAG_SPLIT_SHADE, 0), (W.FLAG_NO_GRAPH, 0), (0, 1), (0, 3), (0, 64)]:
        pt = W.shirley_path_tracer(w, h, max_wavefronts=8, miss_floor=0, rng_mode=W.RNG_PIXEL, flags=W.FLAG_TEXTURES | flags, batch=batch)
        apply(pt, slots, bind)
        pt.render(spp)
        got = pt.accumulated()
        if base is None:
            base = got
        else:
            assert_bits(got, base, f"flags {flags} batch {batch}")
        pt.close()
    # the host-driven stage loop (the reference's run(): one wfpt_kernel_run per stage)
    pt = W.shirley_path_tracer(w, h, max_wavefronts=8, miss_floor=0, rng_mode=W.RNG_PIXEL, flags=W.FLAG_TEXTURES)
    apply(pt, slots, bind)
    for _ in range(spp):
        pt.run()
    assert_bits(pt.accumulated(), base, "host-driven stage loop")
    pt.close()
    bands = []
    for r in range(3):
        pt = W.shirley_path_tracer(w, h, max_wavefronts=8, miss_floor=0, rng_mode=W.RNG_PIXEL, flags=W.FLAG_TEXTURES, tile_rank=r,
                                   tile_world=3)
        apply(pt, slots, bind)
        pt.render(spp)
        bands.append(pt.accumulated().reshape(-1, 8, w, 3))
        pt.close()
    full = np.zeros((h, w, 3), F)
    for r, b in enumerate(bands):
        for j in range(b.shape[0]):
            y0 = (j * 3 + r) * 8
            full[y0:y0 + 8] = b[j][:max(0, min(8, h - y0))]
    assert_bits(full.reshape(-1, 3), base, "three band-sharded contexts")


@pytest.mark.parametrize("mode", [0, 1])
def test_nothing_bound_and_all_ones_give_the_golden_image(W, mode):
    g = np.load(os.path.join(GOLDEN, f"shirley_400x224_mode{mode}.npz"))
    w, h, spp, bounces = int(g["width"]), int(g["height"]), int(g["spp"]), int(g["bounces"])
    for case in ("flag only", "all ones"):
        pt = W.shirley_path_tracer(w, h, max_wavefronts=bounces, rng_mode=mode, flags=W.FLAG_TEXTURES)
        if case == "all ones":
            # (nearest: a texel of ones is exactly 1; bilinear weights of ones sum to 1 within rounding, not exactly)
            pt.set_texture(0, np.ones((3, 5, 3), F), filter="nearest", scale=(3.0, -2.0), offset=(0.5, 0.25))
            pt.set_texture(1, np.ones((2, 2, 3), F), filter="nearest")
            for m in range(len(pt.scene.materials)):
                pt.bind_texture(m, m % 2)
        for _ in range(spp):
            pt.render_sample()
        acc = pt.accumulated()
        assert hashlib.sha256(acc.tobytes()).hexdigest() == str(g["acc_sha256"]), case
        assert np.array_equal(pt.totals(), g["totals"]), case
        pt.close()


def test_albedo_aov_is_the_textured_albedo(W, O):
    w, h = 96, 64
    sp, mt = O.scene_book_one_final(1)
    sp, _ = O.build_bvh(sp)
    slots, bind = shirley_textures(O, sp, mt)
    for env in (None, random_tex(32, 16, 21)):
        f = W.FLAG_TEXTURES | W.FLAG_AOV | (W.FLAG_ENVIRONMENT if env is not None else 0)
        pt = W.shirley_path_tracer(w, h, max_wavefronts=6, flags=f)
        apply(pt, slots, bind)
        if env is not None:
            pt.set_environment(env, intensity=1.5)
        pt.render(3)
        o = O.shirley_oracle(w, h, max_wavefronts=6)
        acc, alb = T.render_with_textures(o, T.Textures(spheres=sp, materials=mt, slots=slots, bind=bind), spp=3, aov=True,
                                          env=env, env_params={"intensity": 1.5})
        assert_bits(pt.aov("albedo").reshape(-1, 3), alb / F(3), f"albedo AOV (env={env is not None})")
        assert_bits(pt.accumulated(), acc, f"image (env={env is not None})")
        pt.close()


def test_textures_with_environment(W, O):
    w, h = 64, 48
    tris, mt, nodes, cam, ip, vw, uv = mesh_uv_inputs(O, w, h, 20000)
    env = random_tex(64, 32, 22)
    pt = mesh_tracer(W, w, h, 20000, max_wavefronts=6, flags=W.FLAG_TEXTURES | W.FLAG_ENVIRONMENT)
    apply(pt, MESH_SLOTS, MESH_BIND, uv)
    pt.set_environment(env, intensity=2.0, rotation=0.25)
    pt.render(2)
    o = O.Oracle(w, h, np.zeros(1, O.SPHERE), mt, nodes, cam, ip, vw, triangles=tris, max_wavefronts=6)
    want = T.render_with_textures(o, T.Textures(triangles=tris, materials=mt, slots=MESH_SLOTS, bind=MESH_BIND, uv=uv), spp=2, env=env,
                                  env_params={"intensity": 2.0, "rotation": 0.25})
    assert_bits(pt.accumulated(), want, "mesh + environment")
    pt.close()


def test_device_rebuild_keeps_rows_and_bindings_and_changes_reset(W, O):
    w, h = 96, 64
    tris, mt, nodes, cam, ip, vw, uv = mesh_uv_inputs(O, w, h)
    pt = mesh_tracer(W, w, h, max_wavefronts=6, flags=W.FLAG_TEXTURES | W.FLAG_DENOISE)
    apply(pt, MESH_SLOTS, MESH_BIND, uv)
    pt.render(2)  # captures a graph
    pt.denoise_temporal()
    # a device rebuild from the file-order triangles: the rows follow the triangles through the device builder
    scene = W.Scene.random_mesh(5000, 1)
    scene.triangles["_pad"] = np.arange(5000, dtype=np.uint32)[::-1]
    pt.update_scene(scene)
    pt.render(2)
    o = O.Oracle(w, h, np.zeros(1, O.SPHERE), mt, nodes, cam, ip, vw, triangles=tris, max_wavefronts=6)
    want = T.render_with_textures(o, T.Textures(triangles=tris, materials=mt, slots=MESH_SLOTS, bind=MESH_BIND, uv=uv), spp=2)
    assert_bits(pt.accumulated(), want, "after a device rebuild")
    # set / bind / clear restart the accumulation, drop the graphs (no stale texture) and the history
    other = random_tex(40, 40, 30)
    pt.set_texture(0, other)
    assert not pt.accumulated().any(), "set_texture restarts the accumulation"
    pt.render(2)
    assert_bits(pt.denoise_temporal(), pt.denoise(), "temporal after a new texture = spatial")
    slots = dict(MESH_SLOTS)
    slots[0] = (other, {})
    o = O.Oracle(w, h, np.zeros(1, O.SPHERE), mt, nodes, cam, ip, vw, triangles=tris, max_wavefronts=6)
    want = T.render_with_textures(o, T.Textures(triangles=tris, materials=mt, slots=slots, bind=MESH_BIND, uv=uv), spp=2)
    assert_bits(pt.accumulated(), want, "after set_texture (no stale graph)")
    pt.bind_texture(2, None)
    assert not pt.accumulated().any()
    pt.clear_texture(0)  # unbinds material 0 too
    assert not pt.accumulated().any()
    pt.render(2)
    o = O.Oracle(w, h, np.zeros(1, O.SPHERE), mt, nodes, cam, ip, vw, triangles=tris, max_wavefronts=6)
    assert_bits(pt.accumulated(), o.render(2), "everything unbound")
    pt.close()


def test_refusals_leave_the_context_usable(W, O):
    w, h = 48, 32
    plain = W.shirley_path_tracer(w, h, max_wavefronts=4)
    with pytest.raises(W.WfptError) as e:
        plain.set_texture(0, np.ones((2, 2, 3), F))
    assert e.value.status == -1
    with pytest.raises(W.WfptError) as e:
        plain.texture_timing()
    assert e.value.status == -1
    plain.close()
    # (Shirley 200x120, pixel-keyed, WFPT_FLAG_BINNING: a shape the class-binned loop takes, as tests/test_gpu_binning.py shows)
    binned = W.shirley_path_tracer(200, 120, max_wavefronts=4, rng_mode=W.RNG_PIXEL, flags=W.FLAG_TEXTURES | W.FLAG_BINNING)
    assert binned.loop_kind == "fused_binned"
    for call in (lambda: binned.set_texture(0, np.ones((2, 2, 3), F)), lambda: binned.bind_texture(0, None),
                 lambda: binned.set_triangle_uvs(None), lambda: binned.clear_texture(0),
                 lambda: binned.sample_texture(0, np.zeros((1, 2), F))):
        with pytest.raises(W.WfptError) as e:
            call()
        assert e.value.status == -4
    assert binned.loop_kind == "fused_binned"
    binned.close()

    tris, mt, nodes, cam, ip, vw, uv = mesh_uv_inputs(O, w, h)
    pt = mesh_tracer(W, w, h, max_wavefronts=4, flags=W.FLAG_TEXTURES)
    apply(pt, MESH_SLOTS, MESH_BIND, uv)
    pt.render(2)
    want = pt.accumulated()
    t = np.ones((4, 4, 3), F)
    bad = [lambda: pt.set_texture(64, t), lambda: pt.set_texture(0, np.full((4, 4, 3), np.nan, F)),
           lambda: pt.set_texture(0, -t), lambda: pt.set_texture(0, np.full((4, 4, 3), np.inf, F)),
           lambda: pt.set_texture(0, np.ones((1, 16385, 3), F)), lambda: pt.set_texture(0, np.ones((0, 4, 3), F)),
           lambda: pt.set_texture(0, t, scale=(np.inf, 1.0)), lambda: pt.set_texture(0, t, offset=(0.0, np.nan)),
           lambda: pt.clear_texture(64), lambda: pt.bind_texture(0, 3), lambda: pt.bind_texture(0, 64), lambda: pt.bind_texture(0, -2),
           lambda: pt.bind_texture(99, 0), lambda: pt.set_triangle_uvs(uv[:100]),
           lambda: pt.set_triangle_uvs(np.where(np.arange(uv.size).reshape(uv.shape) == 7, np.nan, uv).astype(F)),
           lambda: pt.sample_texture(3, np.zeros((2, 2), F))]
    for k, call in enumerate(bad):
        with pytest.raises(W.WfptError) as e:
            call()
        assert e.value.status == -1, k
    scene = W.Scene.random_mesh(5000, 1)
    scene.triangles["_pad"] = 5000  # beyond the table
    with pytest.raises(W.WfptError) as e:
        pt.update_scene(scene)
    assert e.value.status == -1
    assert_bits(pt.accumulated(), want, "a refused call resets nothing")
    pt.render(2)
    fresh = mesh_tracer(W, w, h, max_wavefronts=4, flags=W.FLAG_TEXTURES)
    apply(fresh, MESH_SLOTS, MESH_BIND, uv)
    fresh.render(4)
    assert_bits(pt.accumulated(), fresh.accumulated(), "the context renders as before")
    ms, n = pt.texture_timing()
    assert n == 0 and ms == 0.0
    fresh.close()
    pt.close()


def test_texture_timing_counts_the_passes(W):
    pt = W.shirley_path_tracer(64, 48, max_wavefronts=4, flags=W.FLAG_TEXTURES)
    stages_before = pt.render_timed(1)
    assert pt.texture_timing() == (0.0, 0)  # nothing bound: nothing launched
    pt.set_texture(0, checker(32))
    pt.bind_texture(0, 0)
    pt.render_timed(1)
    ms, n = pt.texture_timing()
    assert n >= 1 and ms > 0.0
    del stages_before
    pt.close()
