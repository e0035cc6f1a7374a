"""Emissive materials (WFPT_FLAG_EMISSION, include/wfpt.h "Emission") on the GPU.

Whole renders are compared bit for bit with tests/emission_ref.py: the oracle's stages driven from Python with the throughput and the second
per-sample plane kept in numpy float32. Every material in these scenes is finite, so every pixel is compared and none is left out."""
import numpy as np
import pytest

import denoise_ref as R
import emission_ref as E
from emission_ref import COLOUR, furnace_inputs
import texture_ref as T
from helpers import closed_room_inputs, make_oracle

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def W(gpu):
    return gpu


@pytest.fixture(scope="module")
def O(orc):
    return orc


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def assert_bits(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = g != w
    assert not bad.any(), f"{what}: {int(bad.sum())} values differ, first at {np.argwhere(bad)[0]}: {np.ravel(got)[np.flatnonzero(bad)[0]]} vs {np.ravel(want)[np.flatnonzero(bad)[0]]}"


def flags_of(W, names):
    f = W.FLAG_EMISSION
    for n in (names.split("|") if names else []):
        f |= getattr(W, "FLAG_" + n)
    return f


def random_tex(w, h, seed):
    return (np.random.default_rng(seed).random((h, w, 3)) * 1.2).astype(F)


def light(pt, colours):
    for m, c in colours.items():
        pt.set_emission(m, c)


# ---------------------------------------------------------------- the scenes
def shirley_scene(O):
    """Shirley's final scene with its three big spheres emitting (three colours, one of them dim)."""
    sp, mt = O.scene_book_one_final(1)
    sp, _ = O.build_bvh(sp)
    big = [int(m) for m in sp["material_idx"][sp["radius"] == 1.0]]
    assert len(big) == 3
    return sp, mt, {big[0]: (4.0, 3.0, 2.0), big[1]: (0.25, 0.5, 1.5), big[2]: (0.0, 0.125, 0.0)}


def room_tracer(W, inputs, scene, w, h, **kw):
    pos = (0.0, 0.0, 0.0) if scene in ("centre", "furnace") else (0.5, 0.25, 1.0)
    cc = W.CameraController(W.Camera(pos, (0.5, 0.0, -1.0)), 70.0, 0.0, 10.0, 0.1, 100.0)
    scn = W.Scene(inputs[0].view(W.SPHERE).copy(), inputs[1].view(W.MATERIAL))
    return W.PathTracer(scn, W.RenderParameters(cc, (w, h)), **kw)


def mesh_inputs(O, w, h, n=5000):
    tris, mt = O.scene_random_mesh(n, 1)
    tris["e1"] *= F(5.0)  # longer edges: a mesh this small gets hit, and hit again after a bounce
    tris["e2"] *= F(5.0)
    tris, nodes = O.build_bvh_triangles(tris, 32)
    cam, ip, vw = O.mesh_camera(w, h)
    return tris, mt, nodes, cam, ip, vw


def mesh_tracer(W, w, h, n=5000, **kw):
    scene = W.Scene.random_mesh(n, 1)
    scene.triangles["e1"] *= F(5.0)
    scene.triangles["e2"] *= F(5.0)
    cc = W.CameraController(W.Camera((0.0, 0.0, 30.0), (0.0, 0.0, 0.0)), 40.0, 0.0, 10.0, 0.1, 100.0)
    return W.PathTracer(scene, W.RenderParameters(cc, (w, h)), **kw)


LOOPS = ["", "UNFUSED", "SPLIT_SHADE", "NO_LDS_SCENE", "NO_LDS_SCENE|NO_REFILL"]


@pytest.mark.parametrize("loop", LOOPS)
@pytest.mark.parametrize("rng", [0, 1])
def test_shirley_equals_restatement(W, O, loop, rng):
    w, h, spp = 160, 96, 2
    sp, mt, colours = shirley_scene(O)
    pt = W.shirley_path_tracer(w, h, max_wavefronts=6, rng_mode=rng, flags=flags_of(W, loop))
    assert pt.loop_kind == {"": "fused", "UNFUSED": "stages", "SPLIT_SHADE": "stages", "NO_LDS_SCENE": "refill"}.get(loop, pt.loop_kind)
    light(pt, colours)
    pt.render(spp)
    got = pt.accumulated()
    o = O.shirley_oracle(w, h, max_wavefronts=6, rng_mode=rng)
    r = E.render_with_emission(o, E.Emission(colours, spheres=sp, materials=mt), spp=spp, parts=True)
    assert_bits(got, r["acc"], f"shirley {loop} rng {rng}")
    assert r["emitted"].any() and r["emitted"].max() > 1.0, "the lamps lit something"
    pt.close()


@pytest.mark.parametrize("scene", ["closed-metal", "closed-glass", "centre"])
@pytest.mark.parametrize("loop", ["", "UNFUSED", "NO_LDS_SCENE"])
def test_closed_rooms_equal_restatement(W, O, scene, loop):
    """miss_floor = 0: a closed room has no misses at all (include/wfpt.h "Emission")"""
    w, h, spp = 72, 40, 2
    inputs = closed_room_inputs(O, scene, w, h)
    colours = {1: COLOUR, 2: (0.0, 0.0, 3.0)} if scene != "closed-glass" else {1: COLOUR}
    for rng, max_wavefronts in ((0, 1), (1, 2), (0, 12)):
        pt = room_tracer(W, inputs, scene, w, h, max_wavefronts=max_wavefronts, miss_floor=0, rng_mode=rng, flags=flags_of(W, loop))
        light(pt, colours)
        pt.render(spp)
        o = make_oracle(O, inputs, w, h, max_wavefronts=max_wavefronts, miss_floor=0, rng_mode=rng)
        r = E.render_with_emission(o, E.Emission(colours, spheres=inputs[0], materials=inputs[1]), spp=spp, parts=True)
        assert_bits(pt.accumulated(), r["acc"], f"{scene} {loop} rng {rng} max {max_wavefronts}")
        assert (pt.bounce_table()[:, 2] == 0).all() and len(pt.bounce_table()) == max_wavefronts, "no miss, and no early exit"
        assert r["emitted"].any()
        pt.close()


@pytest.mark.parametrize("loop", ["", "EXACT_TRAVERSAL", "NO_LDS_SCENE", "NO_LDS_SCENE|NO_REFILL", "UNFUSED"])
def test_mesh_equals_restatement(W, O, loop):
    w, h, spp = 120, 72, 2
    tris, mt, nodes, cam, ip, vw = mesh_inputs(O, w, h)
    colours = {1: (2.0, 1.0, 0.5)}
    for rng in (0, 1):
        pt = mesh_tracer(W, w, h, max_wavefronts=6, rng_mode=rng, flags=flags_of(W, loop))
        if loop == "NO_LDS_SCENE":
            assert pt.loop_kind == "refill"
        light(pt, colours)
        pt.render(spp)
        o = O.Oracle(w, h, np.zeros(1, O.SPHERE), mt, nodes, cam, ip, vw, triangles=tris, max_wavefronts=6, rng_mode=rng)
        r = E.render_with_emission(o, E.Emission(colours, triangles=tris, materials=mt), spp=spp, parts=True)
        assert_bits(pt.accumulated(), r["acc"], f"mesh {loop} rng {rng}")
        assert (r["emitted"] != 0).any(axis=2).mean() > 0.01
        pt.close()


def test_same_bits_across_batches_loops_stage_loop_and_shards(W, O):
    """A viewport that is no multiple of 8 either way. (miss_floor 0: a band-sharded context counts only its own misses against the floor.)"""
    w, h, spp = 100, 60, 130
    sp, mt, colours = shirley_scene(O)
    base = None
    for loop, batch in [("", 1), ("", 16), ("", 128), ("UNFUSED", 16), ("SPLIT_SHADE", 0), ("NO_GRAPH", 0), ("NO_LDS_SCENE", 16),
                        ("NO_LDS_SCENE|NO_REFILL", 0)]:
        pt = W.shirley_path_tracer(w, h, max_wavefronts=5, miss_floor=0, rng_mode=W.RNG_PIXEL, flags=flags_of(W, loop), batch=batch)
        light(pt, colours)
        pt.render(spp)
        got = pt.accumulated()
        if base is None:
            base = got
        else:
            assert_bits(got, base, f"loop {loop} batch {batch}")
        pt.close()
    o = O.shirley_oracle(w, h, max_wavefronts=5, miss_floor=0, rng_mode=W.RNG_PIXEL)
    want = E.render_with_emission(o, E.Emission(colours, spheres=sp, materials=mt), spp=3)
    pt = W.shirley_path_tracer(w, h, max_wavefronts=5, miss_floor=0, rng_mode=W.RNG_PIXEL, flags=W.FLAG_EMISSION, batch=128)
    light(pt, colours)
    pt.render(3)
    assert_bits(pt.accumulated(), want, "100x60 against the restatement")
    pt.close()
    # the host-driven stage loop (one wfpt_kernel_run per stage); its generate_rays covers whole tiles only
    w8, h8 = 96, 56
    pt = W.shirley_path_tracer(w8, h8, max_wavefronts=5, miss_floor=0, rng_mode=W.RNG_PIXEL, flags=W.FLAG_EMISSION)
    light(pt, colours)
    for _ in range(3):
        pt.run()
    host = pt.accumulated()
    pt.close()
    pt = W.shirley_path_tracer(w8, h8, max_wavefronts=5, miss_floor=0, rng_mode=W.RNG_PIXEL, flags=W.FLAG_EMISSION)
    light(pt, colours)
    pt.render(3)
    assert_bits(host, pt.accumulated(), "host-driven stage loop")
    pt.close()


def test_two_band_shards_equal_the_whole_frame(W, O):
    w, h, spp = 100, 60, 4
    _, _, colours = shirley_scene(O)
    whole = W.shirley_path_tracer(w, h, max_wavefronts=6, miss_floor=0, rng_mode=W.RNG_PIXEL, flags=W.FLAG_EMISSION)
    light(whole, colours)
    whole.render(spp)
    base = whole.accumulated()
    whole.close()
    full = np.zeros((h, w, 3), F)
    for r in range(2):
        pt = W.shirley_path_tracer(w, h, max_wavefronts=6, miss_floor=0, rng_mode=W.RNG_PIXEL, flags=W.FLAG_EMISSION, tile_rank=r, tile_world=2)
        light(pt, colours)
        pt.render(spp)
        b = pt.accumulated().reshape(-1, 8, w, 3)
        pt.close()
        for j in range(b.shape[0]):
            y0 = (j * 2 + r) * 8
            full[y0:y0 + 8] = b[j][:max(0, min(8, h - y0))]
    assert_bits(full.reshape(-1, 3), base, "two band-sharded contexts")


# ---------------------------------------------------------------- composition
@pytest.mark.parametrize("loop", ["", "UNFUSED", "NO_LDS_SCENE"])
def test_textured_emitter_takes_the_texture_first(W, O, loop):
    w, h, spp = 128, 80, 2
    sp, mt, colours = shirley_scene(O)
    lamps = sorted(colours)
    ground = int(sp["material_idx"][np.argmax(sp["radius"])])
    slots = {0: (random_tex(64, 32, 1), {"scale": (3.0, 2.0), "offset": (0.25, -0.5)}), 1: (random_tex(17, 9, 2), {"filter": "nearest"})}
    bind = {lamps[0]: 0, lamps[1]: 1, ground: 0}  # two textured lamps, one plain; a textured surface that does not emit
    pt = W.shirley_path_tracer(w, h, max_wavefronts=6, flags=flags_of(W, loop) | W.FLAG_TEXTURES)
    for s, (img, params) in slots.items():
        pt.set_texture(s, img, **params)
    light(pt, colours)  # (in between: the order of the calls does not matter)
    for m, s in bind.items():
        pt.bind_texture(m, s)
    pt.render(spp)
    tx = T.Textures(spheres=sp, materials=mt, slots=slots, bind=bind)
    o = O.shirley_oracle(w, h, max_wavefronts=6)
    want = E.render_with_emission(o, E.Emission(colours, spheres=sp, materials=mt), spp=spp, tx=tx)
    assert_bits(pt.accumulated(), want, f"textured emitters {loop}")
    o = O.shirley_oracle(w, h, max_wavefronts=6)
    wrong = E.render_with_emission(o, E.Emission(colours, spheres=sp, materials=mt, pass_first=True), spp=spp, tx=tx)
    assert not np.array_equal(bits(want), bits(wrong)), "the case does not tell the pass order"
    pt.close()


@pytest.mark.parametrize("loop", ["", "UNFUSED", "NO_LDS_SCENE"])
def test_emission_with_environment_map(W, O, loop):
    w, h, spp = 96, 64, 2
    sp, mt, colours = shirley_scene(O)
    env = random_tex(64, 32, 22)
    pt = W.shirley_path_tracer(w, h, max_wavefronts=6, flags=flags_of(W, loop) | W.FLAG_ENVIRONMENT)
    light(pt, colours)
    pt.set_environment(env, intensity=1.5, rotation=0.25)
    pt.render(spp)
    o = O.shirley_oracle(w, h, max_wavefronts=6)
    want = E.render_with_emission(o, E.Emission(colours, spheres=sp, materials=mt), spp=spp, env=env,
                                  env_params={"intensity": 1.5, "rotation": 0.25})
    assert_bits(pt.accumulated(), want, f"emission + environment {loop}")
    pt.close()


def test_moments_take_image_plus_emitted_and_the_denoisers_run(W, O):
    w, h, spp = 96, 64, 5
    sp, mt, colours = shirley_scene(O)
    o = O.shirley_oracle(w, h, max_wavefronts=6)
    r = E.render_with_emission(o, E.Emission(colours, spheres=sp, materials=mt), spp=spp, parts=True)
    want_var = R.variance_resolve(r["s1"], r["s2"], spp).reshape(h, w)
    for loop, batch in (("", 1), ("", 4), ("", 16), ("UNFUSED", 0), ("NO_LDS_SCENE", 0)):
        pt = W.shirley_path_tracer(w, h, max_wavefronts=6, flags=flags_of(W, loop) | W.FLAG_DENOISE, batch=batch)
        light(pt, colours)
        pt.render(spp)
        assert_bits(pt.accumulated(), r["acc"], f"image {loop} {batch}")
        assert_bits(pt.variance(), want_var, f"variance {loop} {batch}")
        d = pt.denoise()
        assert np.isfinite(d).all() and d.max() > 1.0
        assert_bits(pt.denoise(), d, "a repeated denoise call")
        t = pt.denoise_temporal()
        assert np.isfinite(t).all()
        pt.close()


def test_aovs_are_those_of_a_context_without_the_flag(W, O):
    w, h, spp = 96, 64, 3
    _, _, colours = shirley_scene(O)
    lit = W.shirley_path_tracer(w, h, max_wavefronts=6, flags=W.FLAG_EMISSION | W.FLAG_AOV)
    light(lit, colours)
    plain = W.shirley_path_tracer(w, h, max_wavefronts=6, flags=W.FLAG_AOV)
    lit.render(spp)
    plain.render(spp)
    for name in W.AOVS:
        a, b = lit.aov(name), plain.aov(name)
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32)), name
    assert not np.array_equal(bits(lit.accumulated()), bits(plain.accumulated()))
    lit.close()
    plain.close()


# ---------------------------------------------------------------- no emitter: the flag costs nothing
@pytest.mark.parametrize("loop", ["", "UNFUSED", "SPLIT_SHADE", "NO_LDS_SCENE", "DENOISE"])
def test_flag_without_an_emitter_is_a_context_without_the_flag(W, O, loop):
    w, h, spp = 100, 60, 20
    extra = flags_of(W, loop) & ~W.FLAG_EMISSION
    results = {}
    for flag in (0, W.FLAG_EMISSION):
        pt = W.shirley_path_tracer(w, h, max_wavefronts=6, flags=extra | flag)
        if flag:
            pt.set_emission(0, (1.0, 1.0, 1.0))
            pt.set_emission(0, (0.0, 0.0, 0.0))  # an emitter that came and went
            assert pt.emission(0).tolist() == [0.0, 0.0, 0.0]
        pt.render(spp)
        acc = pt.accumulated()
        _, launches = pt.render_timed(spp)
        results[flag] = (acc, launches, pt.totals(), pt.variance() if loop == "DENOISE" else None)
        if flag:
            assert pt.emission_timing() == (0.0, 0)
        pt.close()
    a, b = results[0], results[W.FLAG_EMISSION]
    assert_bits(b[0], a[0], f"flag only, {loop}")
    assert np.array_equal(a[1], b[1]), f"launch counts per stage: {a[1]} vs {b[1]}"
    assert np.array_equal(a[2], b[2])
    if loop == "DENOISE":
        assert_bits(b[3], a[3], "variance")


# ---------------------------------------------------------------- lifecycle
def test_set_render_clear_render_is_a_fresh_context(W, O):
    w, h, spp = 96, 64, 3
    sp, mt, colours = shirley_scene(O)
    pt = W.shirley_path_tracer(w, h, max_wavefronts=6, flags=W.FLAG_EMISSION | W.FLAG_DENOISE)
    pt.render(spp)  # captures a graph without the pass
    plain = pt.accumulated()
    light(pt, colours)
    for m, c in colours.items():
        assert pt.emission(m).tolist() == list(c)
    assert not pt.accumulated().any(), "set_emission restarts the accumulation"
    pt.render(spp)
    o = O.shirley_oracle(w, h, max_wavefronts=6)
    assert_bits(pt.accumulated(), E.render_with_emission(o, E.Emission(colours, spheres=sp, materials=mt), spp=spp), "after set (no stale graph)")
    pt.denoise_temporal()
    pt.clear_emission()
    assert not pt.accumulated().any() and all(not pt.emission(m).any() for m in colours)
    pt.render(spp)
    assert_bits(pt.accumulated(), plain, "after clear")
    assert_bits(pt.denoise_temporal(), pt.denoise(), "temporal after clear = spatial: the history was dropped")
    fresh = W.shirley_path_tracer(w, h, max_wavefronts=6, flags=W.FLAG_DENOISE)
    fresh.render(spp)
    assert_bits(plain, fresh.accumulated(), "a fresh context without the flag")
    fresh.close()
    pt.close()


def test_update_scene_keeps_the_colours_and_a_resize_keeps_everything(W, O):
    w, h, spp = 96, 64, 2
    tris, mt, nodes, cam, ip, vw = mesh_inputs(O, w, h)
    colours = {1: (2.0, 1.0, 0.5)}
    pt = mesh_tracer(W, w, h, max_wavefronts=6, flags=W.FLAG_EMISSION, max_window_size=128 * 80)
    light(pt, colours)
    pt.render(spp)
    scene = W.Scene.random_mesh(5000, 1)  # file order: the device rebuild reorders it, the table follows
    scene.triangles["e1"] *= F(5.0)
    scene.triangles["e2"] *= F(5.0)
    pt.update_scene(scene)
    assert pt.emission(1).tolist() == [2.0, 1.0, 0.5]
    pt.render(spp)
    o = O.Oracle(w, h, np.zeros(1, O.SPHERE), mt, nodes, cam, ip, vw, triangles=tris, max_wavefronts=6)
    assert_bits(pt.accumulated(), E.render_with_emission(o, E.Emission(colours, triangles=tris, materials=mt), spp=spp), "after a device rebuild")
    # fewer materials: the colours at and beyond the new count are dropped
    fewer = W.Scene.random_mesh(5000, 1)
    fewer.triangles["material_idx"] = 0
    fewer.triangles["material_type"] = fewer.materials["material_type"][0]
    fewer.materials = fewer.materials[:1].copy()
    pt.update_scene(fewer)
    with pytest.raises(W.WfptError):
        pt.emission(1)
    pt.update_scene(scene)
    assert pt.emission(1).tolist() == [0.0, 0.0, 0.0]
    light(pt, colours)
    # a resize within the capacity
    pt.render_parameters.set_viewport((120, 72))
    pt.update_buffers()
    pt.render(spp)
    fresh = mesh_tracer(W, 120, 72, max_wavefronts=6, flags=W.FLAG_EMISSION)
    light(fresh, colours)
    fresh.render(spp)
    assert_bits(pt.accumulated(), fresh.accumulated(), "after a resize")
    fresh.close()
    pt.close()


def test_refusals_leave_the_context_as_it_was(W, O):
    w, h = 48, 32
    L = W.lib()
    c3 = lambda *v: (W.C.c_float * 3)(*v)  # noqa: E731
    plain = W.shirley_path_tracer(w, h, max_wavefronts=4)
    for call in (lambda: plain.set_emission(0, (1.0, 1.0, 1.0)), lambda: plain.emission(0), plain.clear_emission, plain.emission_timing):
        with pytest.raises(W.WfptError) as e:
            call()
        assert e.value.status == -1
    plain.close()
    binned = W.shirley_path_tracer(200, 120, max_wavefronts=4, rng_mode=W.RNG_PIXEL, flags=W.FLAG_EMISSION | W.FLAG_BINNING)
    assert binned.loop_kind == "fused_binned"
    for call in (lambda: binned.set_emission(0, (1.0, 1.0, 1.0)), binned.clear_emission):
        with pytest.raises(W.WfptError) as e:
            call()
        assert e.value.status == -4
    assert binned.loop_kind == "fused_binned" and binned.emission(0).tolist() == [0.0, 0.0, 0.0]
    binned.close()

    _, _, colours = shirley_scene(O)
    pt = W.shirley_path_tracer(w, h, max_wavefronts=4, flags=W.FLAG_EMISSION)
    light(pt, colours)
    pt.render(2)
    want = pt.accumulated()
    n_mat = len(pt.scene.materials)
    m = sorted(colours)[0]
    for k, rgb in enumerate([c3(np.nan, 0, 0), c3(0, np.inf, 0), c3(0, 0, -1.0), c3(-np.inf, 1, 1), c3(1, -1e-30, 1)]):  # the library's own checks
        assert L.wfpt_set_emission(pt.handle, m, rgb) == -1, k
    assert L.wfpt_set_emission(pt.handle, n_mat, c3(1, 1, 1)) == -1
    assert L.wfpt_set_emission(pt.handle, 0xffffffff, c3(1, 1, 1)) == -1
    assert L.wfpt_set_emission(pt.handle, m, None) == -1
    assert L.wfpt_get_emission(pt.handle, n_mat, c3(0, 0, 0)) == -1
    with pytest.raises(ValueError):
        pt.set_emission(m, (np.nan, 0.0, 0.0))
    assert pt.emission(m).tolist() == list(colours[m])
    assert_bits(pt.accumulated(), want, "a refused call resets nothing")
    pt.render(2)
    fresh = W.shirley_path_tracer(w, h, max_wavefronts=4, flags=W.FLAG_EMISSION)
    light(fresh, colours)
    fresh.render(4)
    assert_bits(pt.accumulated(), fresh.accumulated(), "the context renders as before")
    assert pt.emission_timing() == (0.0, 0)
    pt.render_timed(1)
    ms, n = pt.emission_timing()
    assert n >= 2 and ms > 0.0  # the zeroing of the plane and at least one pass
    fresh.close()
    pt.close()


# ---------------------------------------------------------------- the furnace
@pytest.mark.parametrize("loop", LOOPS)
def test_furnace_on_the_device(W, O, loop):
    """The camera inside one closed emitting sphere: every pixel of every sample is exactly e, n samples give exactly n * e."""
    w, h, n = 72, 40, 8
    inputs = furnace_inputs(O, w, h)
    e = np.asarray(COLOUR, F)
    for rng in (0, 1):
        pt = room_tracer(W, inputs, "furnace", w, h, max_wavefronts=6, miss_floor=0, rng_mode=rng, flags=flags_of(W, loop), batch=3)
        pt.set_emission(0, COLOUR)
        for k in (1, n):
            pt.reset_progress()
            pt.render(k)
            assert_bits(pt.accumulated(), np.broadcast_to(F(k) * e, (w * h, 3)), f"furnace {loop} rng {rng}, {k} samples")
        pt.close()
