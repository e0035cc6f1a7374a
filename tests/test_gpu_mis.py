"""Multiple importance sampling (WFPT_FLAG_MIS, include/wfpt.h "Multiple importance sampling") on the GPU.

Whole renders are compared bit for bit with tests/mis_ref.py (nee_ref's restatement with the two weights and the origin plane), the two
device samplers with its row functions. Scene builders and tracers are test_gpu_nee's."""
import numpy as np
import pytest

import denoise_ref as R
import emission_ref as E
import mis_ref as M
import nee_ref as N
import texture_ref as T
from helpers import assert_second_trips, closed_room_inputs, make_oracle
from mis_ref import NEAR
from nee_ref import LAMP
from test_gpu_nee import (assert_bits, bits, compare, lamp_tracer, light, mesh_inputs, mesh_tracer, random_tex, sampler_rows, shirley_scene,
                          sphere_tracer)
from test_mis_host import near_closed_form
from test_nee_host import closed_form

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def W(gpu):
    return gpu


@pytest.fixture(scope="module")
def O(orc):
    return orc


def flags_of(W, names):
    f = W.FLAG_EMISSION | W.FLAG_NEE | W.FLAG_MIS
    for n in (names.split("|") if names else []):
        f |= getattr(W, "FLAG_" + n)
    return f


def near_tracer(W, inputs, w, h, **kw):
    return sphere_tracer(W, inputs, (0.0, 5.0, 7.0), (0.0, 0.0, 0.0), 40.0, w, h, **kw)


LOOPS = ["", "UNFUSED", "SPLIT_SHADE", "NO_GRAPH", "NO_LDS_SCENE", "EXACT_TRAVERSAL"]


# ---------------------------------------------------------------- bit for bit against the restatement
@pytest.mark.parametrize("loop", LOOPS)
@pytest.mark.parametrize("scene", ["lamp", "near"])
def test_lamps_equal_restatement(W, O, scene, loop):
    w, h, spp = 96, 72, 4
    inputs = N.lamp_inputs(O, w, h, mirror=True) if scene == "lamp" else M.near_lamp_inputs(O, w, h)
    colours = {1: LAMP["e"] if scene == "lamp" else NEAR["e"]}
    tracer = lamp_tracer if scene == "lamp" else near_tracer
    for rng in (0, 1):
        pt = tracer(W, inputs, w, h, max_wavefronts=4, miss_floor=0, rng_mode=rng, flags=flags_of(W, loop) | W.FLAG_ENVIRONMENT | W.FLAG_DENOISE)
        pt.set_environment(N.black_env())
        light(pt, colours)
        pt.render(spp)
        o = make_oracle(O, inputs, w, h, max_wavefronts=4, miss_floor=0, rng_mode=rng)
        em = E.Emission(colours, spheres=inputs[0], materials=inputs[1])
        r = M.render_with_mis(o, make_oracle(O, inputs, w, h), em, spp=spp, env=N.black_env(), parts=True)
        compare(pt, r, spp, w, h, f"{scene} {loop} rng {rng}")
        if rng == 0:
            nee = N.render_with_nee(make_oracle(O, inputs, w, h, max_wavefronts=4, miss_floor=0, rng_mode=rng), make_oracle(O, inputs, w, h), em,
                                    spp=spp, env=N.black_env())
            assert not np.array_equal(bits(nee), bits(r["acc"])), "the weights change nothing"
        pt.close()


@pytest.mark.parametrize("loop", LOOPS)
@pytest.mark.parametrize("rng", [0, 1])
def test_three_sphere_lights_equal_restatement(W, O, loop, rng):
    w, h, spp = 160, 96, 2
    sp, mt, colours = shirley_scene(O)
    pt = W.shirley_path_tracer(w, h, max_wavefronts=6, rng_mode=rng, flags=flags_of(W, loop) | W.FLAG_DENOISE)
    light(pt, colours)
    assert pt.nee_light_count() == 3
    pt.render(spp)
    o, shadow = O.shirley_oracle(w, h, max_wavefronts=6, rng_mode=rng), O.shirley_oracle(w, h)
    r = M.render_with_mis(o, shadow, E.Emission(colours, spheres=sp, materials=mt), spp=spp, parts=True)
    compare(pt, r, spp, w, h, f"shirley {loop} rng {rng}")
    pt.close()


def two_triangle_lights(O):
    """A Lambertian wall (two triangles in the plane z = 0, facing the mesh camera) with two emitting triangles of different size and tilt in
    front of it: a light list of two triangles. The camera sees both lights directly (full weight), the wall connects to them and finds them
    by scatter (wl and wb), and rays that pass the wall's edge miss. Returns (triangles as given to the scene, materials)."""
    mt = np.zeros(2, O.MATERIAL)
    mt["albedo"][0] = (0.7, 0.6, 0.5, 1.0)
    mt["albedo"][1] = (0.5, 0.5, 0.5, 1.0)
    tris = np.zeros(4, O.TRIANGLE)
    tris["v0"] = [(-12, -12, 0), (12, 12, 0), (-5, -2, 3), (2, -3, 2)]
    tris["e1"] = [(24, 0, 0), (-24, 0, 0), (4, 0, 1), (3, 1, 0)]
    tris["e2"] = [(0, 24, 0), (0, -24, 0), (0, 4, 0.5), (0, 3, 2)]
    tris["material_idx"] = (0, 0, 1, 1)
    tris["material_type"] = mt["material_type"][tris["material_idx"]]
    return tris, mt


@pytest.mark.parametrize("loop", LOOPS)
def test_two_triangle_lights_equal_restatement(W, O, loop):
    w, h, spp = 96, 72, 4
    tris, mt = two_triangle_lights(O)
    tb, nodes = O.build_bvh_triangles(tris, 32)
    cam, ip, vw = O.mesh_camera(w, h)
    colours = {1: (3.0, 2.0, 1.0)}
    em = E.Emission(colours, triangles=tb, materials=mt)
    cc = W.CameraController(W.Camera((0.0, 0.0, 30.0), (0.0, 0.0, 0.0)), 40.0, 0.0, 10.0, 0.1, 100.0)
    for rng in (0, 1):
        scene = W.Scene(np.zeros(0, W.SPHERE), mt.view(W.MATERIAL), triangles=tris.view(W.TRIANGLE).copy())
        pt = W.PathTracer(scene, W.RenderParameters(cc, (w, h)), max_wavefronts=4, miss_floor=0, rng_mode=rng, flags=flags_of(W, loop) | W.FLAG_DENOISE)
        light(pt, colours)
        assert pt.nee_light_count() == 2
        pt.render(spp)

        def oracles():
            return (O.Oracle(w, h, np.zeros(1, O.SPHERE), mt, nodes, cam, ip, vw, triangles=tb, max_wavefronts=4, miss_floor=0, rng_mode=rng),
                    O.Oracle(w, h, np.zeros(1, O.SPHERE), mt, nodes, cam, ip, vw, triangles=tb))

        r = M.render_with_mis(*oracles(), em, spp=spp, parts=True)
        compare(pt, r, spp, w, h, f"two triangle lights {loop} rng {rng}")
        if rng == 1:
            nee = N.render_with_nee(*oracles(), em, spp=spp, parts=True)
            assert (r["emitted"] > nee["emitted"]).any(), "no scattered ray found a light: wb is not exercised"
            assert (r["emitted"] < nee["emitted"]).any(), "no connect sample was weighed down: wl is not exercised"
        pt.close()


@pytest.mark.parametrize("scene", ["closed-metal", "closed-glass"])
@pytest.mark.parametrize("loop", ["", "UNFUSED", "NO_LDS_SCENE"])
def test_emitters_behind_glass_and_metal_equal_restatement(W, O, scene, loop):
    """test_gpu_nee's closed rooms: the Lambertian sphere inside connects to lamps of glass or metal class, and finds them by scatter."""
    w, h, spp = 72, 40, 2
    inputs = closed_room_inputs(O, scene, w, h)
    colours = {0: E.COLOUR, 2: (0.0, 0.0, 3.0)} if scene != "closed-glass" else {0: E.COLOUR}
    for rng, max_wavefronts in ((1, 2), (0, 8)):
        pt = sphere_tracer(W, inputs, (0.5, 0.25, 1.0), (0.5, 0.0, -1.0), 70.0, w, h, max_wavefronts=max_wavefronts, miss_floor=0, rng_mode=rng,
                           flags=flags_of(W, loop))
        light(pt, colours)
        pt.render(spp)
        o = make_oracle(O, inputs, w, h, max_wavefronts=max_wavefronts, miss_floor=0, rng_mode=rng)
        r = M.render_with_mis(o, make_oracle(O, inputs, w, h), E.Emission(colours, spheres=inputs[0], materials=inputs[1]), spp=spp, parts=True)
        compare(pt, r, spp, w, h, f"{scene} {loop} rng {rng} max {max_wavefronts}")
        pt.close()


@pytest.mark.parametrize("loop", ["", "EXACT_TRAVERSAL", "NO_LDS_SCENE", "NO_LDS_SCENE|NO_REFILL", "NO_LDS_SCENE|BINARY_BVH", "NO_LDS_SCENE|BINARY_BVH|NO_REFILL", "UNFUSED"])
def test_mesh_equals_restatement(W, O, loop):
    """The 5 000-triangle mesh with one emitting material (several hundred triangle lights), the four-wide and binary walks, refill on and off."""
    w, h, spp = 200, 120, 2
    tris, mt, nodes, cam, ip, vw = mesh_inputs(O, w, h)
    colours = {1: (2.0, 1.0, 0.5)}
    pt = mesh_tracer(W, w, h, max_wavefronts=6, rng_mode=1, flags=flags_of(W, loop))
    light(pt, colours)
    pt.render(spp)
    o = O.Oracle(w, h, np.zeros(1, O.SPHERE), mt, nodes, cam, ip, vw, triangles=tris, max_wavefronts=6, rng_mode=1)
    shadow = O.Oracle(w, h, np.zeros(1, O.SPHERE), mt, nodes, cam, ip, vw, triangles=tris)
    r = M.render_with_mis(o, shadow, E.Emission(colours, triangles=tris, materials=mt), spp=spp, parts=True)
    compare(pt, r, spp, w, h, f"mesh {loop}")
    pt.close()


@pytest.mark.parametrize("loop", ["", "UNFUSED", "NO_LDS_SCENE"])
def test_textured_emitter(W, O, loop):
    w, h, spp = 128, 80, 2
    sp, mt, colours = shirley_scene(O)
    lamps = sorted(colours)
    slots = {0: (random_tex(64, 32, 1), {"scale": (3.0, 2.0), "offset": (0.25, -0.5)}), 1: (random_tex(17, 9, 2), {"filter": "nearest"})}
    bind = {lamps[0]: 0, lamps[1]: 1}
    pt = W.shirley_path_tracer(w, h, max_wavefronts=6, flags=flags_of(W, loop) | W.FLAG_TEXTURES)
    for s, (img, params) in slots.items():
        pt.set_texture(s, img, **params)
    light(pt, colours)
    for m, s in bind.items():
        pt.bind_texture(m, s)
    pt.render(spp)
    tx = T.Textures(spheres=sp, materials=mt, slots=slots, bind=bind)
    r = M.render_with_mis(O.shirley_oracle(w, h, max_wavefronts=6), O.shirley_oracle(w, h), E.Emission(colours, spheres=sp, materials=mt), spp=spp,
                          tx=tx, parts=True)
    compare(pt, r, spp, w, h, f"textured emitters {loop}")
    pt.close()


# ---------------------------------------------------------------- the same bits however the samples are scheduled
def test_same_bits_across_batches_stage_loops_and_shards(W, O):
    w, h, spp = 100, 60, 19  # 16 + a remainder of 3
    _, _, colours = shirley_scene(O)
    base = None
    for loop, batch in [("", 1), ("", 3), ("", 16), ("UNFUSED", 16), ("SPLIT_SHADE", 3), ("NO_LDS_SCENE", 16)]:
        pt = W.shirley_path_tracer(w, h, max_wavefronts=5, miss_floor=0, rng_mode=W.RNG_PIXEL, flags=flags_of(W, loop), batch=batch)
        light(pt, colours)
        pt.render(spp)
        got = pt.accumulated()
        if base is None:
            base = got
        else:
            assert_bits(got, base, f"loop {loop} batch {batch}")
        pt.close()
    full = np.zeros((h, w, 3), F)
    for r in range(2):
        pt = W.shirley_path_tracer(w, h, max_wavefronts=5, miss_floor=0, rng_mode=W.RNG_PIXEL, flags=flags_of(W, ""), tile_rank=r, tile_world=2)
        light(pt, colours)
        pt.render(spp)
        b = pt.accumulated().reshape(-1, 8, w, 3)
        pt.close()
        for j in range(b.shape[0]):
            y0 = (j * 2 + r) * 8
            full[y0:y0 + 8] = b[j][:max(0, min(8, h - y0))]
    assert_bits(full.reshape(-1, 3), base, "two band-sharded contexts")


def test_second_trips_through_the_segment_loop(W, O):
    """68 segments: at batch 128 the texture and emission passes launch 64 workgroups per sample, so four of them walk a second segment;
    at batch 16 they launch 68 and none does. Same bits."""
    w, h, spp = 256, 136, 128
    _, _, colours = shirley_scene(O)
    lamps = sorted(colours)
    got = {}
    for batch in (128, 16):
        pt = W.shirley_path_tracer(w, h, max_wavefronts=5, miss_floor=0, rng_mode=W.RNG_PIXEL, flags=flags_of(W, "TEXTURES"), batch=batch)
        assert_second_trips(W, pt, 128, 16)
        pt.set_texture(0, random_tex(64, 32, 1), scale=(3.0, 2.0), offset=(0.25, -0.5))
        light(pt, colours)
        pt.bind_texture(lamps[0], 0)
        pt.render(spp)
        got[batch] = pt.accumulated()
        pt.close()
    assert_bits(got[128], got[16], "batch 128 against batch 16")


@pytest.mark.parametrize("three", [False, True])
def test_stage_api_equals_render(W, O, three):
    """The host-driven stage loop with one shade stage and with the three per-material ones, against render()."""
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
        if three:
            pt.shade_kernel = ThreeStages(pt)
        for _ in range(3):
            pt.run()
        host = pt.accumulated()
        pt.close()
        pt = W.shirley_path_tracer(w, h, max_wavefronts=5, miss_floor=0, rng_mode=rng, flags=flags_of(W, ""))
        light(pt, colours)
        pt.render(3)
        assert_bits(host, pt.accumulated(), f"stage API, three stages {three}, rng {rng}")
        pt.close()


# ---------------------------------------------------------------- the samplers
def fence(rows, seed):
    """rows with NaN and infinite entries sprinkled over a few of them"""
    rng = np.random.default_rng(seed)
    bad = rows.copy()
    k = len(bad)
    idx = rng.choice(k, 48, replace=False)
    bad[idx[:16], rng.integers(0, rows.shape[1], 16)] = np.nan
    bad[idx[16:32], rng.integers(0, rows.shape[1], 16)] = np.inf
    bad[idx[32:], rng.integers(0, rows.shape[1], 16)] = -np.inf
    return bad, idx


@pytest.mark.parametrize("loop", ["", "NO_LDS_SCENE"])
def test_samplers_equal_the_restatement(W, O, loop):
    k = 3000
    sp, mt, colours = shirley_scene(O)
    pt = W.shirley_path_tracer(64, 48, max_wavefronts=2, flags=flags_of(W, loop))
    light(pt, colours)
    lights = N.Lights(E.Emission(colours, spheres=sp, materials=mt))
    check_samplers(pt, lights, O.shirley_oracle(64, 48), sampler_rows((0.0, 1.0, 0.0), k, 5), len(sp), f"spheres {loop}")
    pt.close()
    w, h = 64, 48
    tris, mt, nodes, cam, ip, vw = mesh_inputs(O, w, h)
    pt = mesh_tracer(W, w, h, max_wavefronts=2, flags=flags_of(W, loop))
    pt.set_emission(1, (2.0, 1.0, 0.5))
    lights = N.Lights(E.Emission({1: (2.0, 1.0, 0.5)}, triangles=tris, materials=mt))
    shadow = O.Oracle(w, h, np.zeros(1, O.SPHERE), mt, nodes, cam, ip, vw, triangles=tris)
    check_samplers(pt, lights, shadow, sampler_rows((0.0, 0.0, 0.0), k, 6), len(tris), f"mesh {loop}")
    pt.close()


def check_samplers(pt, lights, shadow, rows, n_prims, what):
    got = pt.sample_lights_mis(rows)
    want = M.sample_rows(lights, shadow, rows)
    assert got.shape == (len(rows), 12)
    assert_bits(got[:, :7], want[:, :7], what + ": q, primitive, (e_q G) wl")
    assert np.array_equal(got[:, 7] != 0, want[:, 7] != 0), what + ": the occlusion verdict is not the oracle's"
    assert_bits(got[:, 8:], want[:, 8:], what + ": pl, pb, wl")
    lit = want[:, 10] > 0
    assert lit.sum() > len(rows) // 10 and (want[:, 7] != 0).any() and (lit & (want[:, 7] == 0)).any(), what
    # the unweighed sampler's factor times wl: the same sample
    plain = pt.sample_lights(rows)
    assert_bits(got[:, 4:7], (plain[:, 4:7] * got[:, 10:11]).astype(F), what + ": against wfpt_sample_lights")
    # NaN and infinite rows: fenced, every finite row unchanged, nothing non-finite in the three channels
    bad, idx = fence(rows, 9)
    g2 = pt.sample_lights_mis(bad)
    keep = np.setdiff1d(np.arange(len(rows)), idx)
    assert_bits(g2[keep], got[keep], what + ": rows beside the bad ones")
    assert set(np.unique(g2[:, 7])) <= {0.0, 1.0} and (g2[:, 11] == 0).all(), what + ": a bad row's verdict"
    # the hit side: the connect samples replayed as scattered rays, random hits on any primitive, and bad rows
    rng = np.random.default_rng(12)
    with np.errstate(all="ignore"):
        cos_s = want[:, 9] * N.PI
        v = want[:, :3] - rows[:, :3]
        dist = np.sqrt(N.dot3(v, v))
        d = (F(2) * cos_s)[:, None] * (v / dist[:, None])
        t = dist / (F(2) * cos_s)
    hit = np.concatenate([rows[:, :3], d, t[:, None], want[:, 3:4]], 1).astype(F)[lit]
    rnd = np.concatenate([rng.standard_normal((500, 6)) * 3, rng.random((500, 1)) * 4, rng.integers(-2, n_prims + 2, (500, 1))], 1).astype(F)
    hits = np.concatenate([hit, rnd, fence(np.concatenate([hit[:200], rnd[:200]]), 10)[0]])
    gw = pt.mis_hit_weight(hits)
    ww = M.hit_weight_rows(lights, hits)
    both_nan = np.isnan(gw) & np.isnan(ww)  # (a NaN's payload is not part of the contract)
    assert_bits(np.where(both_nan, F(0), gw), np.where(both_nan, F(0), ww), what + ": wfpt_mis_hit_weight")
    n_fin = len(hit) + 500
    assert (gw[:n_fin, 2] <= 1).all() and (gw[:n_fin, 2] >= 0).all() and (gw[len(hit):n_fin, 2] == 1).any() and (gw[:len(hit), 2] < 1).mean() > 0.99
    gap = np.abs(want[lit, 10].astype(np.float64) + gw[:len(hit), 2].astype(np.float64) - 1.0)[gw[:len(hit), 2] < 1]
    print(f"{what}: worst |wl + wb - 1| on the device {gap.max():.3g}")
    assert gap.max() <= 2.0 ** -20  # the next power of two above the restatement's worst on these rows (grazing and far receivers): 5.87e-07


# ---------------------------------------------------------------- no emitter, refusals
@pytest.mark.parametrize("loop", ["", "UNFUSED", "NO_LDS_SCENE"])
def test_flag_without_an_emitter_is_a_context_without_the_flag(W, O, loop):
    w, h, spp = 100, 60, 20
    extra = flags_of(W, loop) & ~(W.FLAG_EMISSION | W.FLAG_NEE | W.FLAG_MIS)
    results = {}
    for flag in (0, W.FLAG_EMISSION | W.FLAG_NEE | W.FLAG_MIS):
        pt = W.shirley_path_tracer(w, h, max_wavefronts=6, flags=extra | flag)
        if flag:
            pt.set_emission(0, (1.0, 1.0, 1.0))
            pt.set_emission(0, (0.0, 0.0, 0.0))  # an emitter that came and went: the planes stay, nothing is launched
            assert pt.nee_light_count() == 0
        pt.render(spp)
        acc = pt.accumulated()
        ms, launches = pt.render_timed(spp)
        results[flag] = (acc, launches, pt.totals())
        if flag:
            assert pt.nee_timing() == (0.0, 0) and pt.emission_timing() == (0.0, 0)
        pt.close()
    a, b = results[0], results[W.FLAG_EMISSION | W.FLAG_NEE | W.FLAG_MIS]
    assert_bits(b[0], a[0], f"flag only, {loop}")
    assert np.array_equal(a[1], b[1]), f"launch counts per stage: {a[1]} vs {b[1]}"
    assert np.array_equal(a[2], b[2])


def test_refusals(W, O):
    w, h = 48, 32
    for flags in (W.FLAG_MIS, W.FLAG_MIS | W.FLAG_EMISSION, W.FLAG_MIS | W.FLAG_NEE,
                  W.FLAG_MIS | W.FLAG_EMISSION | W.FLAG_NEE | W.FLAG_ENVIRONMENT | W.FLAG_ENV_NEE):
        with pytest.raises(W.WfptError):
            W.shirley_path_tracer(w, h, max_wavefronts=4, flags=flags)
    _, _, colours = shirley_scene(O)
    plain = W.shirley_path_tracer(w, h, max_wavefronts=4, flags=W.FLAG_EMISSION | W.FLAG_NEE)
    light(plain, colours)
    for call in (lambda: plain.sample_lights_mis(np.zeros((1, 9), F)), lambda: plain.mis_hit_weight(np.zeros((1, 8), F))):
        with pytest.raises(W.WfptError) as e:
            call()
        assert e.value.status == -1
    plain.close()
    pt = W.shirley_path_tracer(w, h, max_wavefronts=4, flags=flags_of(W, ""))
    for call in (lambda: pt.sample_lights_mis(np.zeros((1, 9), F)), lambda: pt.mis_hit_weight(np.zeros((1, 8), F))):
        with pytest.raises(W.WfptError) as e:  # no emitter yet
            call()
        assert e.value.status == -1
    light(pt, colours)
    assert pt.sample_lights_mis(np.zeros((0, 9), F)).shape == (0, 12) and pt.mis_hit_weight(np.zeros((0, 8), F)).shape == (0, 4)
    L = W.lib()
    assert L.wfpt_sample_lights_mis(pt.handle, None, 4, None) == -1 and L.wfpt_mis_hit_weight(pt.handle, None, 4, None) == -1
    pt.close()
    binned = W.shirley_path_tracer(200, 120, max_wavefronts=4, rng_mode=W.RNG_PIXEL, flags=flags_of(W, "BINNING"))
    assert binned.loop_kind == "fused_binned"
    with pytest.raises(W.WfptError) as e:
        binned.set_emission(0, (1.0, 1.0, 1.0))
    assert e.value.status == -4
    binned.close()


# ---------------------------------------------------------------- the payoff
def test_weighing_lowers_the_variance_of_the_near_lamp_scene(W, O):
    """Equal spp (320 x 240, 64 spp, WFPT_RNG_PIXEL, WFPT_FLAG_DENOISE, miss_floor 0): the sum of wfpt_read_variance over the ground pixels
    with MIS is below EMISSION|NEE's and below EMISSION's alone, and the three means agree within 4 combined standard errors. The far-lamp
    scene of DESIGN.md 9h is reported, not asserted: there MIS may lose up to the balance heuristic's own term."""
    w, h, spp = 320, 240, 64
    legs = (("plain", W.FLAG_EMISSION), ("nee", W.FLAG_EMISSION | W.FLAG_NEE), ("mis", W.FLAG_EMISSION | W.FLAG_NEE | W.FLAG_MIS))
    for scene in ("near", "far"):
        if scene == "near":
            inputs = M.near_lamp_inputs(O, w, h)
            _, _, ok = near_closed_form(inputs, w, h)
            tracer, e = near_tracer, NEAR["e"]
        else:
            inputs = N.lamp_inputs(O, w, h)
            _, _, ok = closed_form(inputs, w, h, LAMP["lamp_r"])
            tracer, e = lamp_tracer, LAMP["e"]
        sums, means, ses = {}, {}, {}
        for name, flags in legs:
            pt = tracer(W, inputs, w, h, max_wavefronts=4, miss_floor=0, rng_mode=W.RNG_PIXEL, flags=flags | W.FLAG_ENVIRONMENT | W.FLAG_DENOISE)
            pt.set_environment(N.black_env())
            pt.set_emission(1, e)
            pt.render(spp)
            var = pt.variance().reshape(-1)[ok].astype(np.float64)
            sums[name] = float(var.sum())
            means[name] = R.luma(pt.accumulated())[ok].astype(np.float64).mean() / spp
            ses[name] = np.sqrt(var.sum() * spp / (spp - 1)) / ok.sum()  # wfpt_read_variance is the variance of the pixel's mean (s2 / n - mu^2) / n
            print(f"{scene} {name}: variance sum over {int(ok.sum())} ground pixels {sums[name]:.6g}, mean luminance {means[name]:.6g} +- {ses[name]:.3g}")
            pt.close()
        print(f"{scene}: variance ratio mis / nee {sums['mis'] / sums['nee']:.4g}, mis / plain {sums['mis'] / sums['plain']:.4g}")
        if scene == "near":
            assert sums["mis"] < sums["nee"] and sums["mis"] < sums["plain"]
            for a, b in (("mis", "nee"), ("mis", "plain"), ("nee", "plain")):
                assert abs(means[a] - means[b]) <= 4.0 * np.hypot(ses[a], ses[b]), (a, b, means, ses)
