"""Next-event estimation (WFPT_FLAG_NEE, include/wfpt.h "Next-event estimation") on the GPU.

Whole renders are compared bit for bit with tests/nee_ref.py: the oracle's stages driven from Python with the throughput, the second
per-sample plane and the connected flag kept in numpy float32, the shadow rays traced by a second oracle. Every material in these scenes
is finite, so every pixel is compared and none is left out."""
import numpy as np
import pytest

import denoise_ref as R
import emission_ref as E
import nee_ref as N
import texture_ref as T
from helpers import closed_room_inputs, make_oracle
from nee_ref import LAMP
from test_nee_host import closed_form

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
    f = W.FLAG_EMISSION | W.FLAG_NEE
    for n in (names.split("|") if names else []):
        f |= getattr(W, "FLAG_" + n)
    return f


def random_tex(w, h, seed):
    return (np.random.default_rng(seed).random((h, w, 3)) * 1.2).astype(F)


def light(pt, colours):
    for m, c in colours.items():
        pt.set_emission(m, c)


def compare(pt, r, spp, w, h, what):
    """accumulated, the luminance moments (WFPT_FLAG_DENOISE contexts) and wfpt_read_image against the restatement's"""
    assert_bits(pt.accumulated(), r["acc"], what + ": accumulated")
    img = bits(pt.image())  # wfpt_read_image: thr of the first sample of the last batch (the batch size is the context's choice)
    assert any(np.array_equal(img, bits(k)) for k in r["image"]), what + ": read_image is no sample's throughput"
    if pt._params.flags & 1 << 11:
        assert_bits(pt.variance(), R.variance_resolve(r["s1"], r["s2"], spp).reshape(h, w), what + ": variance")


# ---------------------------------------------------------------- the scenes
def shirley_scene(O):
    """Shirley's final scene with its three big spheres emitting (three colours, one of them dim)."""
    sp, mt = O.scene_book_one_final(1)
    sp, _ = O.build_bvh(sp)
    big = [int(m) for m in sp["material_idx"][sp["radius"] == 1.0]]
    assert len(big) == 3
    return sp, mt, {big[0]: (4.0, 3.0, 2.0), big[1]: (0.25, 0.5, 1.5), big[2]: (0.0, 0.125, 0.0)}


def sphere_tracer(W, inputs, pos, look_at, vfov, w, h, **kw):
    cc = W.CameraController(W.Camera(pos, look_at), vfov, 0.0, 10.0, 0.1, 100.0)
    scn = W.Scene(inputs[0].view(W.SPHERE).copy(), inputs[1].view(W.MATERIAL))
    return W.PathTracer(scn, W.RenderParameters(cc, (w, h)), **kw)


def lamp_tracer(W, inputs, w, h, **kw):
    return sphere_tracer(W, inputs, (0.0, 6.0, 8.0), (0.0, 0.0, 0.0), 40.0, w, h, **kw)


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


LOOPS = ["", "UNFUSED", "SPLIT_SHADE", "EXACT_TRAVERSAL", "NO_LDS_SCENE", "NO_LDS_SCENE|NO_REFILL", "NO_LDS_SCENE|BINARY_BVH", "NO_GRAPH"]


# ---------------------------------------------------------------- bit for bit against the restatement
@pytest.mark.parametrize("loop", LOOPS)
@pytest.mark.parametrize("rng", [0, 1])
def test_shirley_equals_restatement(W, O, loop, rng):
    w, h, spp = 160, 96, 2
    sp, mt, colours = shirley_scene(O)
    pt = W.shirley_path_tracer(w, h, max_wavefronts=6, rng_mode=rng, flags=flags_of(W, loop) | W.FLAG_DENOISE)
    light(pt, colours)
    assert pt.nee_light_count() == 3
    pt.render(spp)
    o, shadow = O.shirley_oracle(w, h, max_wavefronts=6, rng_mode=rng), O.shirley_oracle(w, h)
    r = N.render_with_nee(o, shadow, E.Emission(colours, spheres=sp, materials=mt), spp=spp, parts=True)
    compare(pt, r, spp, w, h, f"shirley {loop} rng {rng}")
    plain = E.render_with_emission(O.shirley_oracle(w, h, max_wavefronts=6, rng_mode=rng), E.Emission(colours, spheres=sp, materials=mt), spp=spp)
    assert not np.array_equal(bits(plain), bits(r["acc"])), "the connect pass changes nothing"
    pt.close()


@pytest.mark.parametrize("loop", ["", "UNFUSED", "NO_LDS_SCENE"])
def test_lamp_with_a_blocker_casts_a_hard_shadow(W, O, loop):
    w, h, spp = 96, 72, 4
    inputs = N.lamp_inputs(O, w, h, blocker=True)
    colours = {1: LAMP["e"]}
    for rng in (0, 1):
        pt = lamp_tracer(W, inputs, w, h, max_wavefronts=4, miss_floor=0, rng_mode=rng, flags=flags_of(W, loop) | W.FLAG_ENVIRONMENT | W.FLAG_DENOISE)
        pt.set_environment(N.black_env())
        light(pt, colours)
        pt.render(spp)
        o = make_oracle(O, inputs, w, h, max_wavefronts=4, miss_floor=0, rng_mode=rng)
        r = N.render_with_nee(o, make_oracle(O, inputs, w, h), E.Emission(colours, spheres=inputs[0], materials=inputs[1]), spp=spp,
                              env=N.black_env(), parts=True)
        compare(pt, r, spp, w, h, f"lamp + blocker {loop} rng {rng}")
        lum = R.luma(r["acc"]).reshape(h, w)
        umbra = lum[h // 2 - 1:h // 2 + 1, w // 2 - 1:w // 2 + 1]  # under the blocker, in the middle of the frame: indirect light only
        assert umbra.max() < 0.25 * lum[h // 2, w // 2 + 20:w // 2 + 28].mean(), "no hard shadow under the blocker"
        pt.close()


@pytest.mark.parametrize("scene", ["closed-metal", "closed-glass", "centre"])
@pytest.mark.parametrize("loop", ["", "UNFUSED", "NO_LDS_SCENE"])
def test_closed_rooms_equal_restatement(W, O, scene, loop):
    """miss_floor = 0: a closed room has no misses at all. The Lambertian sphere inside (material 1) connects to the glass or metal lamps."""
    w, h, spp = 72, 40, 2
    inputs = closed_room_inputs(O, scene, w, h)
    colours = {0: E.COLOUR, 2: (0.0, 0.0, 3.0)} if scene != "closed-glass" else {0: E.COLOUR}
    pos = (0.0, 0.0, 0.0) if scene == "centre" else (0.5, 0.25, 1.0)
    for rng, max_wavefronts in ((0, 1), (1, 2), (0, 8)):
        pt = sphere_tracer(W, inputs, pos, (0.5, 0.0, -1.0), 70.0, w, h, max_wavefronts=max_wavefronts, miss_floor=0, rng_mode=rng, flags=flags_of(W, loop))
        light(pt, colours)
        pt.render(spp)
        o = make_oracle(O, inputs, w, h, max_wavefronts=max_wavefronts, miss_floor=0, rng_mode=rng)
        r = N.render_with_nee(o, make_oracle(O, inputs, w, h), E.Emission(colours, spheres=inputs[0], materials=inputs[1]), spp=spp, parts=True)
        compare(pt, r, spp, w, h, f"{scene} {loop} rng {rng} max {max_wavefronts}")
        assert (pt.bounce_table()[:, 2] == 0).all() and len(pt.bounce_table()) == max_wavefronts, "no miss, and no early exit"
        pt.close()


@pytest.mark.parametrize("loop", ["", "EXACT_TRAVERSAL", "NO_LDS_SCENE", "NO_LDS_SCENE|NO_REFILL", "NO_LDS_SCENE|BINARY_BVH", "UNFUSED"])
def test_mesh_equals_restatement(W, O, loop):
    w, h, spp = 120, 72, 2
    tris, mt, nodes, cam, ip, vw = mesh_inputs(O, w, h)
    colours = {1: (2.0, 1.0, 0.5)}
    for rng in (0, 1):
        pt = mesh_tracer(W, w, h, max_wavefronts=6, rng_mode=rng, flags=flags_of(W, loop))
        light(pt, colours)
        assert pt.nee_light_count() == int((tris["material_idx"] == 1).sum())
        pt.render(spp)
        o = O.Oracle(w, h, np.zeros(1, O.SPHERE), mt, nodes, cam, ip, vw, triangles=tris, max_wavefronts=6, rng_mode=rng)
        shadow = O.Oracle(w, h, np.zeros(1, O.SPHERE), mt, nodes, cam, ip, vw, triangles=tris)
        r = N.render_with_nee(o, shadow, E.Emission(colours, triangles=tris, materials=mt), spp=spp, parts=True)
        compare(pt, r, spp, w, h, f"mesh {loop} rng {rng}")
        pt.close()


@pytest.mark.parametrize("loop", ["", "UNFUSED", "NO_LDS_SCENE"])
def test_textured_emitter_lights_with_its_texture(W, O, loop):
    w, h, spp = 128, 80, 2
    sp, mt, colours = shirley_scene(O)
    lamps = sorted(colours)
    ground = int(sp["material_idx"][np.argmax(sp["radius"])])
    slots = {0: (random_tex(64, 32, 1), {"scale": (3.0, 2.0), "offset": (0.25, -0.5)}), 1: (random_tex(17, 9, 2), {"filter": "nearest"})}
    bind = {lamps[0]: 0, lamps[1]: 1, ground: 0}  # two textured lamps, one plain; a textured surface that does not emit
    pt = W.shirley_path_tracer(w, h, max_wavefronts=6, flags=flags_of(W, loop) | W.FLAG_TEXTURES)
    for s, (img, params) in slots.items():
        pt.set_texture(s, img, **params)
    light(pt, colours)
    for m, s in bind.items():
        pt.bind_texture(m, s)
    pt.render(spp)
    tx = T.Textures(spheres=sp, materials=mt, slots=slots, bind=bind)
    em = E.Emission(colours, spheres=sp, materials=mt)
    r = N.render_with_nee(O.shirley_oracle(w, h, max_wavefronts=6), O.shirley_oracle(w, h), em, spp=spp, tx=tx, parts=True)
    compare(pt, r, spp, w, h, f"textured emitters {loop}")
    pt.close()


@pytest.mark.parametrize("loop", ["", "UNFUSED", "NO_LDS_SCENE"])
def test_nee_with_environment_map(W, O, loop):
    w, h, spp = 96, 64, 2
    sp, mt, colours = shirley_scene(O)
    env = random_tex(64, 32, 22)
    pt = W.shirley_path_tracer(w, h, max_wavefronts=6, flags=flags_of(W, loop) | W.FLAG_ENVIRONMENT)
    light(pt, colours)
    pt.set_environment(env, intensity=1.5, rotation=0.25)
    pt.render(spp)
    r = N.render_with_nee(O.shirley_oracle(w, h, max_wavefronts=6), O.shirley_oracle(w, h), E.Emission(colours, spheres=sp, materials=mt), spp=spp,
                          env=env, env_params={"intensity": 1.5, "rotation": 0.25}, parts=True)
    compare(pt, r, spp, w, h, f"nee + environment {loop}")
    pt.close()


# ---------------------------------------------------------------- the same bits however the samples are scheduled
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
    # the host-driven stage loop (one wfpt_kernel_run per stage); its generate_rays covers whole tiles only
    w8, h8 = 96, 56
    pt = W.shirley_path_tracer(w8, h8, max_wavefronts=5, miss_floor=0, rng_mode=W.RNG_PIXEL, flags=flags_of(W, ""))
    light(pt, colours)
    for _ in range(3):
        pt.run()
    host = pt.accumulated()
    pt.close()
    pt = W.shirley_path_tracer(w8, h8, max_wavefronts=5, miss_floor=0, rng_mode=W.RNG_PIXEL, flags=flags_of(W, ""))
    light(pt, colours)
    pt.render(3)
    assert_bits(host, pt.accumulated(), "host-driven stage loop")
    pt.close()


def test_per_material_stages_connect_like_the_single_shade_stage(W, O):
    """The host-driven loop with shade_lambertian, shade_metal and shade_dielectric in place of shade: the Lambertian stage connects, the
    other two only clear the pixels' connected flags (connect_kernel's class filter). Same bits as render()."""
    w, h = 96, 56
    _, _, colours = shirley_scene(O)

    class ThreeStages:
        def __init__(self, pt):
            self.stages = [W.Kernel(name, pt) for name in ("shade_metal", "shade_lambertian", "shade_dielectric")]

        def run(self, size):
            for k in self.stages:
                k.run(size)

    for rng in (0, 1):
        pt = W.shirley_path_tracer(w, h, max_wavefronts=5, miss_floor=0, rng_mode=rng, flags=flags_of(W, ""))
        light(pt, colours)
        pt.shade_kernel = ThreeStages(pt)
        for _ in range(3):
            pt.run()
        host = pt.accumulated()
        pt.close()
        pt = W.shirley_path_tracer(w, h, max_wavefronts=5, miss_floor=0, rng_mode=rng, flags=flags_of(W, ""))
        light(pt, colours)
        pt.render(3)
        assert_bits(host, pt.accumulated(), f"per-material stages, rng {rng}")
        pt.close()


def test_two_band_shards_equal_the_whole_frame(W, O):
    w, h, spp = 100, 60, 4
    _, _, colours = shirley_scene(O)
    whole = W.shirley_path_tracer(w, h, max_wavefronts=6, miss_floor=0, rng_mode=W.RNG_PIXEL, flags=flags_of(W, ""))
    light(whole, colours)
    whole.render(spp)
    base = whole.accumulated()
    whole.close()
    full = np.zeros((h, w, 3), F)
    for r in range(2):
        pt = W.shirley_path_tracer(w, h, max_wavefronts=6, miss_floor=0, rng_mode=W.RNG_PIXEL, flags=flags_of(W, ""), tile_rank=r, tile_world=2)
        light(pt, colours)
        pt.render(spp)
        b = pt.accumulated().reshape(-1, 8, w, 3)
        pt.close()
        for j in range(b.shape[0]):
            y0 = (j * 2 + r) * 8
            full[y0:y0 + 8] = b[j][:max(0, min(8, h - y0))]
    assert_bits(full.reshape(-1, 3), base, "two band-sharded contexts")


# ---------------------------------------------------------------- the sampler
def sampler_rows(prims_centre, k, seed):
    """k receivers around the scene: random ones, some far away, some grazing (the normal nearly perpendicular to the light's direction)"""
    rng = np.random.default_rng(seed)
    rows = np.zeros((k, 9), F)
    rows[:, :3] = rng.standard_normal((k, 3)) * 4 + np.asarray(prims_centre)
    rows[: k // 8, :3] *= 20  # far-side and far-away points
    n = rng.standard_normal((k, 3))
    rows[:, 3:6] = n / np.linalg.norm(n, axis=1, keepdims=True)
    rows[:, 6:] = rng.random((k, 3))
    rows[:4, 6] = (0.0, 1 - 2.0 ** -24, 1.0, 0.5)
    rows[:4, 7] = (0.0, 1.0, 1 - 2.0 ** -24, 0.0)
    return rows


@pytest.mark.parametrize("loop", ["", "EXACT_TRAVERSAL", "NO_LDS_SCENE", "NO_LDS_SCENE|BINARY_BVH"])
def test_sample_lights_equals_the_restatement(W, O, loop):
    k = 3000
    # spheres
    sp, mt, colours = shirley_scene(O)
    pt = W.shirley_path_tracer(64, 48, max_wavefronts=2, flags=flags_of(W, loop))
    light(pt, colours)
    lights = N.Lights(E.Emission(colours, spheres=sp, materials=mt))
    rows = sampler_rows((0.0, 1.0, 0.0), k, 5)
    # grazing: the normal turned to within 1e-3 of perpendicular to the direction of the first light's centre
    c = sp["center"][lights.list[0], :3]
    d = c - rows[k // 2:, :3]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    t = np.cross(d, rows[k // 2:, 3:6])
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    rows[k // 2:, 3:6] = t + d * np.linspace(-1e-3, 1e-3, k - k // 2)[:, None]
    got = pt.sample_lights(rows)
    s = lights.sample(rows[:, :3], rows[:, 3:6], rows[:, 6], rows[:, 7], rows[:, 8])
    check_sampler(O, got, s, rows, O.shirley_oracle(64, 48), f"spheres {loop}")
    pt.close()
    # triangles
    w, h = 64, 48
    tris, mt, nodes, cam, ip, vw = mesh_inputs(O, w, h)
    pt = mesh_tracer(W, w, h, max_wavefronts=2, flags=flags_of(W, loop))
    pt.set_emission(1, (2.0, 1.0, 0.5))
    lights = N.Lights(E.Emission({1: (2.0, 1.0, 0.5)}, triangles=tris, materials=mt))
    rows = sampler_rows((0.0, 0.0, 0.0), k, 6)
    got = pt.sample_lights(rows)
    s = lights.sample(rows[:, :3], rows[:, 3:6], rows[:, 6], rows[:, 7], rows[:, 8])
    check_sampler(O, got, s, rows, O.Oracle(w, h, np.zeros(1, O.SPHERE), mt, nodes, cam, ip, vw, triangles=tris), f"mesh {loop}")
    pt.close()


def check_sampler(O, got, s, rows, shadow, what):
    lit = s["lit"]
    assert lit.sum() > len(rows) // 10 and (~lit).sum() > len(rows) // 10, what
    assert_bits(got[:, :3], s["q"], what + ": q")
    assert np.array_equal(got[:, 3].astype(np.int64), s["prim"]), what + ": the light's primitive"
    with np.errstate(all="ignore"):
        f = np.where(lit[:, None], s["e_q"] * s["G"][:, None], F(0)).astype(F)
    assert_bits(got[:, 4:7], f, what + ": e_q G")
    occ = np.zeros(len(rows), bool)
    occ[lit] = N.occluded(shadow, rows[lit, :3], s["w"][lit], s["dist"][lit])  # the oracle's closest-hit verdict on the same rays
    assert np.array_equal(got[:, 7] != 0, occ), what + ": occlusion"
    assert occ.any() and (lit & ~occ).any(), what


# ---------------------------------------------------------------- no emitter: the flag costs nothing
@pytest.mark.parametrize("loop", ["", "UNFUSED", "SPLIT_SHADE", "NO_LDS_SCENE", "DENOISE"])
def test_flag_without_an_emitter_is_a_context_without_the_flag(W, O, loop):
    w, h, spp = 100, 60, 20
    extra = flags_of(W, loop) & ~(W.FLAG_EMISSION | W.FLAG_NEE)
    results = {}
    for flag in (0, W.FLAG_EMISSION | W.FLAG_NEE):
        pt = W.shirley_path_tracer(w, h, max_wavefronts=6, flags=extra | flag)
        if flag:
            pt.set_emission(0, (1.0, 1.0, 1.0))
            assert pt.nee_light_count() >= 1
            pt.set_emission(0, (0.0, 0.0, 0.0))  # an emitter that came and went
            assert pt.nee_light_count() == 0
        pt.render(spp)
        acc = pt.accumulated()
        ms, launches = pt.render_timed(spp)
        results[flag] = (acc, launches, pt.totals(), pt.variance() if loop == "DENOISE" else None)
        if flag:
            assert pt.nee_timing() == (0.0, 0) and pt.emission_timing() == (0.0, 0)
        pt.close()
    a, b = results[0], results[W.FLAG_EMISSION | W.FLAG_NEE]
    assert_bits(b[0], a[0], f"flag only, {loop}")
    assert np.array_equal(a[1], b[1]), f"launch counts per stage: {a[1]} vs {b[1]}"
    assert np.array_equal(a[2], b[2])
    if loop == "DENOISE":
        assert_bits(b[3], a[3], "variance")


# ---------------------------------------------------------------- lifecycle
def test_set_render_clear_render_is_a_fresh_context(W, O):
    w, h, spp = 96, 64, 3
    sp, mt, colours = shirley_scene(O)
    pt = W.shirley_path_tracer(w, h, max_wavefronts=6, flags=flags_of(W, "DENOISE"))
    pt.render(spp)  # captures a graph without the pass
    plain = pt.accumulated()
    light(pt, colours)
    assert not pt.accumulated().any(), "set_emission restarts the accumulation"
    pt.render(spp)
    r = N.render_with_nee(O.shirley_oracle(w, h, max_wavefronts=6), O.shirley_oracle(w, h), E.Emission(colours, spheres=sp, materials=mt), spp=spp)
    assert_bits(pt.accumulated(), r, "after set (no stale graph)")
    pt.clear_emission()
    assert pt.nee_light_count() == 0 and not pt.accumulated().any()
    pt.render(spp)
    assert_bits(pt.accumulated(), plain, "after clear")
    fresh = W.shirley_path_tracer(w, h, max_wavefronts=6, flags=W.FLAG_DENOISE)
    fresh.render(spp)
    assert_bits(plain, fresh.accumulated(), "a fresh context without the flags")
    fresh.close()
    pt.close()


def test_update_scene_rebuilds_the_light_list_and_a_resize_keeps_it(W, O):
    w, h, spp = 96, 64, 2
    tris, mt, nodes, cam, ip, vw = mesh_inputs(O, w, h)
    colours = {1: (2.0, 1.0, 0.5)}
    pt = mesh_tracer(W, w, h, max_wavefronts=6, flags=flags_of(W, ""), max_window_size=128 * 80)
    light(pt, colours)
    n_lights = pt.nee_light_count()
    small = W.Scene.random_mesh(3000, 1)
    small.triangles["e1"] *= F(5.0)
    small.triangles["e2"] *= F(5.0)
    pt.update_scene(small)
    assert pt.nee_light_count() == int((small.triangles["material_idx"] == 1).sum()) != n_lights
    scene = W.Scene.random_mesh(5000, 1)  # file order: the device rebuild reorders it, the list follows
    scene.triangles["e1"] *= F(5.0)
    scene.triangles["e2"] *= F(5.0)
    pt.update_scene(scene)
    assert pt.nee_light_count() == n_lights
    pt.render(spp)
    o = O.Oracle(w, h, np.zeros(1, O.SPHERE), mt, nodes, cam, ip, vw, triangles=tris, max_wavefronts=6)
    shadow = O.Oracle(w, h, np.zeros(1, O.SPHERE), mt, nodes, cam, ip, vw, triangles=tris)
    assert_bits(pt.accumulated(), N.render_with_nee(o, shadow, E.Emission(colours, triangles=tris, materials=mt), spp=spp), "after a device rebuild")
    pt.render_parameters.set_viewport((120, 72))
    pt.update_buffers()
    assert pt.nee_light_count() == n_lights
    pt.render(spp)
    fresh = mesh_tracer(W, 120, 72, max_wavefronts=6, flags=flags_of(W, ""))
    light(fresh, colours)
    fresh.render(spp)
    assert_bits(pt.accumulated(), fresh.accumulated(), "after a resize")
    fresh.close()
    pt.close()


def test_refusals_leave_the_context_as_it_was(W, O):
    w, h = 48, 32
    with pytest.raises(W.WfptError):  # the flag without WFPT_FLAG_EMISSION
        W.shirley_path_tracer(w, h, max_wavefronts=4, flags=W.FLAG_NEE)
    plain = W.shirley_path_tracer(w, h, max_wavefronts=4, flags=W.FLAG_EMISSION)
    for call in (plain.nee_light_count, plain.nee_timing, lambda: plain.sample_lights(np.zeros((1, 9), F))):
        with pytest.raises(W.WfptError) as e:
            call()
        assert e.value.status == -1
    plain.close()
    binned = W.shirley_path_tracer(200, 120, max_wavefronts=4, rng_mode=W.RNG_PIXEL, flags=flags_of(W, "BINNING"))
    assert binned.loop_kind == "fused_binned"
    for call in (lambda: binned.set_emission(0, (1.0, 1.0, 1.0)), binned.clear_emission):
        with pytest.raises(W.WfptError) as e:
            call()
        assert e.value.status == -4
    assert binned.loop_kind == "fused_binned" and binned.nee_light_count() == 0
    binned.close()

    _, _, colours = shirley_scene(O)
    pt = W.shirley_path_tracer(w, h, max_wavefronts=4, flags=flags_of(W, ""))
    with pytest.raises(W.WfptError) as e:  # no emitter yet: nothing to sample
        pt.sample_lights(np.zeros((1, 9), F))
    assert e.value.status == -1
    light(pt, colours)
    pt.render(2)
    want = pt.accumulated()
    L = W.lib()
    assert L.wfpt_sample_lights(pt.handle, None, 4, None) == -1
    assert L.wfpt_set_emission(pt.handle, 0xffffffff, (W.C.c_float * 3)(1, 1, 1)) == -1
    with pytest.raises(ValueError):
        pt.sample_lights(np.zeros((3, 8), F))
    assert pt.sample_lights(np.zeros((0, 9), F)).shape == (0, 8)
    pt.sample_lights(np.ones((5, 9), F))  # a sampler call in between changes nothing
    assert_bits(pt.accumulated(), want, "a refused call resets nothing")
    pt.render(2)
    fresh = W.shirley_path_tracer(w, h, max_wavefronts=4, flags=flags_of(W, ""))
    light(fresh, colours)
    fresh.render(4)
    assert_bits(pt.accumulated(), fresh.accumulated(), "the context renders as before")
    assert pt.nee_timing() == (0.0, 0)
    pt.render_timed(1)
    ms, n = pt.nee_timing()
    assert n >= 1 and ms > 0.0
    fresh.close()
    pt.close()


# ---------------------------------------------------------------- the payoff
def test_connecting_lowers_the_variance_of_the_lamp_scene(W, O):
    """Equal spp, WFPT_FLAG_DENOISE: the sum of wfpt_read_variance over the ground pixels of the flagged context is below the unflagged
    one's. The ratio is printed; DESIGN.md 9h records it."""
    w, h, spp = 320, 240, 64
    inputs = N.lamp_inputs(O, w, h)
    _, _, ok = closed_form(inputs, w, h, LAMP["lamp_r"])
    sums = {}
    for name, flags in (("plain", W.FLAG_EMISSION), ("nee", W.FLAG_EMISSION | W.FLAG_NEE)):
        pt = lamp_tracer(W, inputs, w, h, max_wavefronts=4, miss_floor=0, rng_mode=W.RNG_PIXEL, flags=flags | W.FLAG_ENVIRONMENT | W.FLAG_DENOISE)
        pt.set_environment(N.black_env())
        pt.set_emission(1, LAMP["e"])
        pt.render(spp)
        sums[name] = float(pt.variance().reshape(-1)[ok].astype(np.float64).sum())
        mean = R.luma(pt.accumulated())[ok].astype(np.float64).mean() / spp
        print(f"{name}: variance sum over {int(ok.sum())} ground pixels {sums[name]:.6g}, mean luminance {mean:.6g}")
        pt.close()
    print(f"variance ratio nee / plain at {spp} spp: {sums['nee'] / sums['plain']:.4g}")
    assert sums["nee"] < sums["plain"]
