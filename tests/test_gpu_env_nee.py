"""Environment next-event estimation (WFPT_FLAG_ENV_NEE, include/wfpt.h "Environment next-event estimation") on the GPU.

Whole renders are compared bit for bit with tests/env_nee_ref.py: the oracle's stages driven from Python with the throughput, the second
per-sample plane and the connected flag kept in numpy float32, the shadow rays traced by a second oracle. Every material and map in
these scenes is finite, so every pixel is compared and none is left out."""
import numpy as np
import pytest

import denoise_ref as R
import emission_ref as E
import env_nee_ref as V
import nee_ref as N
from helpers import assert_bits_or_nan, assert_second_trips, make_oracle, make_tracer, simple_inputs
from test_env_nee_host import maps
from test_gpu_nee import assert_bits, bits, compare, light, mesh_inputs, mesh_tracer, sphere_tracer

pytestmark = pytest.mark.gpu

F = np.float32
LAMP_E = (16.0, 8.0, 32.0)
ENV_PARAMS = {"intensity": 1.5, "rotation": 0.375}


@pytest.fixture(scope="module")
def W(gpu):
    return gpu


@pytest.fixture(scope="module")
def O(orc):
    return orc


def base_flags(W):
    return W.FLAG_ENVIRONMENT | W.FLAG_EMISSION | W.FLAG_NEE


def flags_of(W, names, env_nee=True):
    f = base_flags(W) | (W.FLAG_ENV_NEE if env_nee else 0)
    for n in (names.split("|") if names else []):
        f |= getattr(W, "FLAG_" + n)
    return f


def ground_tracer(W, inputs, w, h, look_at=(0.0, 0.0, 0.0), **kw):
    return sphere_tracer(W, inputs, (0.0, 6.0, 8.0), look_at, 40.0, w, h, **kw)


def env_light(env):
    return V.EnvLight(env, **ENV_PARAMS)


LOOPS = ["", "UNFUSED", "SPLIT_SHADE", "EXACT_TRAVERSAL", "NO_LDS_SCENE", "NO_LDS_SCENE|NO_REFILL", "NO_LDS_SCENE|BINARY_BVH", "NO_GRAPH"]


# ---------------------------------------------------------------- bit for bit against the restatement
@pytest.mark.parametrize("loop", ["", "UNFUSED", "NO_LDS_SCENE"])
def test_ground_equals_restatement(W, O, loop):
    """No emitter: the effective share is 1, every diffuse hit connects to the map, and the light list is empty."""
    w, h, spp = 64, 64, 4
    inputs = V.ground_inputs(O, w, h, look_at=(0.0, 3.5, 0.0))
    env = V.block_map()
    for rng in (0, 1):
        pt = ground_tracer(W, inputs, w, h, look_at=(0.0, 3.5, 0.0), max_wavefronts=4, miss_floor=0, rng_mode=rng, flags=flags_of(W, loop) | W.FLAG_DENOISE)
        pt.set_environment(env, **ENV_PARAMS)
        assert pt.nee_light_count() == 0
        pt.render(spp)
        o = make_oracle(O, inputs, w, h, max_wavefronts=4, miss_floor=0, rng_mode=rng)
        r = V.render_with_env_nee(o, make_oracle(O, inputs, w, h), E.Emission({}, spheres=inputs[0], materials=inputs[1]), env_light(env), spp=spp, parts=True)
        compare(pt, r, spp, w, h, f"ground {loop} rng {rng}")
        assert r["emitted"].any()
        pt.close()


@pytest.mark.parametrize("loop", LOOPS)
@pytest.mark.parametrize("rng", [0, 1])
def test_simple_scene_equals_restatement(W, O, loop, rng):
    """The 5-sphere scene (all three material classes, occluders) under a 16 x 8 map with a sun; rotation and intensity off their defaults."""
    w, h, spp = 64, 64, 3
    inputs = simple_inputs(O, w, h)
    env = V.sun_map()
    pt = make_tracer(W, "simple", w, h, max_wavefronts=6, rng_mode=rng, flags=flags_of(W, loop) | W.FLAG_DENOISE)
    pt.set_environment(env, **ENV_PARAMS)
    pt.render(spp)
    o = make_oracle(O, inputs, w, h, max_wavefronts=6, rng_mode=rng)
    em = E.Emission({}, spheres=inputs[0], materials=inputs[1])
    r = V.render_with_env_nee(o, make_oracle(O, inputs, w, h), em, env_light(env), spp=spp, parts=True)
    compare(pt, r, spp, w, h, f"simple {loop} rng {rng}")
    plain = N.render_with_nee(make_oracle(O, inputs, w, h, max_wavefronts=6, rng_mode=rng), make_oracle(O, inputs, w, h), em, spp=spp, env=env, env_params=ENV_PARAMS)
    assert not np.array_equal(bits(plain), bits(r["acc"])), "connecting to the map changes nothing"
    pt.close()


@pytest.mark.parametrize("loop", ["", "UNFUSED", "NO_LDS_SCENE"])
@pytest.mark.parametrize("share", [0.5, 0.25])
def test_lamp_and_map_together_equal_restatement(W, O, loop, share):
    """An emitter and a map: both branches, the emitter's u0' and the division by 1 - p; an occluder and a mirror beside the lamp."""
    w, h, spp = 64, 64, 4
    inputs = V.ground_inputs(O, w, h, occluder=True, mirror=True, lamp=True)
    env = V.block_map()
    colours = {1: LAMP_E}
    for rng in (0, 1):
        pt = ground_tracer(W, inputs, w, h, max_wavefronts=5, miss_floor=0, rng_mode=rng, flags=flags_of(W, loop) | W.FLAG_DENOISE)
        pt.set_environment(env, **ENV_PARAMS)
        light(pt, colours)
        if share != 0.5:
            pt.set_environment_share(share)
        assert pt.environment_share() == F(share) and pt.nee_light_count() == 1
        pt.render(spp)
        o = make_oracle(O, inputs, w, h, max_wavefronts=5, miss_floor=0, rng_mode=rng)
        r = V.render_with_env_nee(o, make_oracle(O, inputs, w, h), E.Emission(colours, spheres=inputs[0], materials=inputs[1]), env_light(env),
                                  share=share, spp=spp, parts=True)
        compare(pt, r, spp, w, h, f"lamp + map {loop} share {share} rng {rng}")
        pt.close()


@pytest.mark.parametrize("loop", ["NO_LDS_SCENE", "NO_LDS_SCENE|BINARY_BVH", "NO_LDS_SCENE|NO_REFILL", ""])
def test_mesh_equals_restatement(W, O, loop):
    """5 000 triangles, one material in three emitting, under the sun map: the four-wide and the binary walk trace the shadow rays."""
    w, h, spp = 120, 72, 2
    tris, mt, nodes, cam, ip, vw = mesh_inputs(O, w, h)
    colours = {1: (2.0, 1.0, 0.5)}
    env = V.sun_map()
    for rng in (0, 1):
        pt = mesh_tracer(W, w, h, max_wavefronts=5, rng_mode=rng, flags=flags_of(W, loop))
        light(pt, colours)
        pt.set_environment(env, **ENV_PARAMS)
        pt.render(spp)
        o = O.Oracle(w, h, np.zeros(1, O.SPHERE), mt, nodes, cam, ip, vw, triangles=tris, max_wavefronts=5, rng_mode=rng)
        shadow = O.Oracle(w, h, np.zeros(1, O.SPHERE), mt, nodes, cam, ip, vw, triangles=tris)
        r = V.render_with_env_nee(o, shadow, E.Emission(colours, triangles=tris, materials=mt), env_light(env), spp=spp, parts=True)
        compare(pt, r, spp, w, h, f"mesh {loop} rng {rng}")
        pt.close()


# ---------------------------------------------------------------- the same bits however the samples are scheduled
def lamp_scene(W, O, w, h, **kw):
    inputs = V.ground_inputs(O, w, h, occluder=True, mirror=True, lamp=True)
    pt = ground_tracer(W, inputs, w, h, max_wavefronts=5, miss_floor=0, **kw)
    pt.set_environment(V.block_map(), **ENV_PARAMS)
    pt.set_emission(1, LAMP_E)
    return pt


def test_same_bits_across_batches_and_loops(W, O):
    w, h, spp = 100, 60, 16
    base = None
    for loop, batch in [("", 1), ("", 16), ("UNFUSED", 16), ("SPLIT_SHADE", 0), ("NO_GRAPH", 0), ("NO_LDS_SCENE", 16), ("NO_LDS_SCENE|NO_REFILL", 0)]:
        pt = lamp_scene(W, O, w, h, rng_mode=W.RNG_PIXEL, flags=flags_of(W, loop), batch=batch)
        pt.render(spp)
        got = pt.accumulated()
        if base is None:
            base = got
        else:
            assert_bits(got, base, f"loop {loop} batch {batch}")
        pt.close()


def test_second_trips_through_the_segment_loop(W, O):
    """68 segments: at batch 128 the miss launches (and the stage loop's emission pass) run 64 workgroups per sample, so four of them walk
    a second segment; at batch 16 they run 68 and none does. Same bits, and the stage loop's at batch 128 as well."""
    w, h, spp = 256, 136, 128
    got = {}
    for loop, batch in (("", 128), ("", 16), ("UNFUSED", 128)):
        pt = lamp_scene(W, O, w, h, rng_mode=W.RNG_PIXEL, flags=flags_of(W, loop), batch=batch)
        assert_second_trips(W, pt, 128, 16)
        pt.render(spp)
        got[loop, batch] = pt.accumulated()
        pt.close()
    assert_bits(got["", 128], got["", 16], "batch 128 against batch 16")
    assert_bits(got["UNFUSED", 128], got["", 128], "the stage loop against the fused one, batch 128")


def test_stage_loops_equal_render(W, O):
    """The host-driven loop, with the single shade stage and with the three per-material shade stages (the Lambertian stage connects, the
    other two only clear the flags; the miss stage is gated): same bits as render()."""
    w, h = 96, 56

    class ThreeStages:
        def __init__(self, pt):
            self.stages = [W.Kernel(name, pt) for name in ("shade_metal", "shade_lambertian", "shade_dielectric")]

        def run(self, size):
            for k in self.stages:
                k.run(size)

    for rng in (0, 1):
        pt = lamp_scene(W, O, w, h, rng_mode=rng, flags=flags_of(W, ""))
        pt.render(3)
        want = pt.accumulated()
        pt.close()
        for split in (False, True):
            pt = lamp_scene(W, O, w, h, rng_mode=rng, flags=flags_of(W, ""))
            if split:
                pt.shade_kernel = ThreeStages(pt)
            for _ in range(3):
                pt.run()
            assert_bits(pt.accumulated(), want, f"host-driven stage loop, per-material {split}, rng {rng}")
            pt.close()


def test_two_band_shards_equal_the_whole_frame(W, O):
    w, h, spp = 100, 60, 4
    whole = lamp_scene(W, O, w, h, rng_mode=W.RNG_PIXEL, flags=flags_of(W, ""))
    whole.render(spp)
    base = whole.accumulated()
    whole.close()
    full = np.zeros((h, w, 3), F)
    for r in range(2):
        pt = lamp_scene(W, O, w, h, rng_mode=W.RNG_PIXEL, flags=flags_of(W, ""), tile_rank=r, tile_world=2)
        pt.render(spp)
        b = pt.accumulated().reshape(-1, 8, w, 3)
        pt.close()
        for j in range(b.shape[0]):
            y0 = (j * 2 + r) * 8
            full[y0:y0 + 8] = b[j][:max(0, min(8, h - y0))]
    assert_bits(full.reshape(-1, 3), base, "two band-sharded contexts")


# ---------------------------------------------------------------- the tables and the sampler
@pytest.mark.parametrize("name", list(maps()))
def test_distribution_equals_the_restatement(W, O, name):
    env = maps()[name]
    pt = W.shirley_path_tracer(32, 32, max_wavefronts=2, flags=flags_of(W, ""))
    with pytest.raises(W.WfptError):
        pt.environment_distribution()
    pt.set_environment(env)
    row, marg = pt.environment_distribution()
    d = V.Distribution(env)
    assert np.array_equal(row, d.row) and np.array_equal(marg, d.marg)
    pt.close()


def sampler_rows(k, seed):
    rng = np.random.default_rng(seed)
    rows = np.zeros((k, 10), F)
    rows[:, :3] = rng.standard_normal((k, 3)) * 1.5 + np.array([0.0, 0.0, -1.0])
    n = rng.standard_normal((k, 3))
    rows[:, 3:6] = n / np.linalg.norm(n, axis=1, keepdims=True)
    rows[:, 6:] = rng.random((k, 4))
    rows[:5, 6] = (0.0, 1.0, 1 - 2.0 ** -24, 2.0 ** -24, 0.5)
    rows[:5, 7] = (0.0, 1.0, 0.0, 1.0, 1 - 2.0 ** -24)
    rows[5:9, 8] = (0.0, 1.0, 0.0, 1.0)
    rows[5:9, 9] = (0.0, 1.0, 1.0, 0.0)
    return rows


@pytest.mark.parametrize("loop", ["", "EXACT_TRAVERSAL", "NO_LDS_SCENE", "NO_LDS_SCENE|BINARY_BVH"])
def test_sample_environment_light_equals_the_restatement(W, O, loop):
    k = 2000
    w, h = 64, 64
    inputs = simple_inputs(O, w, h)
    env = V.sun_map()
    pt = make_tracer(W, "simple", w, h, max_wavefronts=2, flags=flags_of(W, loop))
    pt.set_environment(env, **ENV_PARAMS)
    pt.set_environment_share(0.25)  # the sampler is the branch with p = 1 whatever the share
    rows = sampler_rows(k, 9)
    rows[k // 2:, 3:6] = (0.0, 1.0, 0.0)  # half of the receivers face up: most of their samples contribute
    rows[20:40, 3:6] = (0.0, -1.0, 0.0)  # facing away from the sun
    lightr = env_light(env)
    shadow = make_oracle(O, inputs, w, h)

    def check(rows, what, may_nan):
        got = pt.sample_environment_light(rows)
        s = lightr.sample(rows[:, 3:6], rows[:, 6], rows[:, 7], rows[:, 8], rows[:, 9], 1.0)
        lit = s["lit"]
        with np.errstate(all="ignore"):
            f = np.where(lit[:, None], s["e"] * s["G"][:, None], F(0)).astype(F)
        eq = assert_bits_or_nan if may_nan else assert_bits
        eq(got[:, :3], s["w"], what + ": wdir")
        assert np.array_equal(got[:, 3].astype(np.int64), s["texel"]), what + ": the texel"
        eq(got[:, 4:7], f, what + ": e Genv")
        occ = np.zeros(len(rows), bool)
        if lit.any():
            occ[lit] = V.any_hit(shadow, rows[lit, :3], s["w"][lit])
        assert np.array_equal(got[:, 7] != 0, occ), what + ": occlusion"
        return lit, occ

    lit, occ = check(rows, f"finite rows {loop}", False)
    assert lit.sum() > k // 4 and (~lit).sum() > k // 10 and occ.any() and (lit & ~occ).any()
    assert not lit[20:40].any()
    bad = sampler_rows(64, 10)  # NaN and infinite receivers, normals and draws
    for j, col in enumerate(range(10)):
        bad[j, col] = np.nan
        bad[10 + j, col] = np.inf
        bad[20 + j, col] = -np.inf
    for j in (0, 1, 2, 10, 11, 12, 20, 21, 22):
        bad[j, 3:6] = 0.0  # a receiver that is no point sends no shadow ray (cos_s = 0): there is no verdict to compare
    check(bad, f"NaN and inf rows {loop}", True)
    pt.close()


# ---------------------------------------------------------------- no map, or a black one: the flag costs nothing
@pytest.mark.parametrize("loop", ["", "UNFUSED", "NO_LDS_SCENE", "DENOISE"])
@pytest.mark.parametrize("emitter", [False, True])
@pytest.mark.parametrize("black", [False, True])
def test_flag_without_a_lit_map_is_a_context_without_the_flag(W, O, loop, emitter, black):
    w, h, spp = 100, 60, 8
    results = []
    for env_nee in (False, True):
        pt = W.shirley_path_tracer(w, h, max_wavefronts=6, flags=flags_of(W, loop, env_nee))
        if env_nee:
            pt.set_environment(V.sun_map())  # a map that came and went
            pt.environment_distribution()
            pt.clear_environment()
        if black:
            pt.set_environment(np.zeros((4, 8, 3), F))
        if emitter:
            pt.set_emission(0, (4.0, 3.0, 2.0))
        if env_nee:
            with pytest.raises(W.WfptError):
                pt.environment_distribution()
        pt.render(spp)
        acc = pt.accumulated()
        ms, launches = pt.render_timed(spp)
        results.append((acc, launches, pt.totals(), pt.nee_timing()[1], pt.emission_timing()[1], pt.variance() if loop == "DENOISE" else None))
        pt.close()
    a, b = results
    assert_bits(b[0], a[0], f"{loop} emitter {emitter} black {black}")
    assert np.array_equal(a[1], b[1]), f"launch counts per stage: {a[1]} vs {b[1]}"
    assert np.array_equal(a[2], b[2]) and a[3] == b[3] and a[4] == b[4]
    assert (a[3] > 0) == emitter
    if loop == "DENOISE":
        assert_bits(b[5], a[5], "variance")


# ---------------------------------------------------------------- lifecycle and refusals
def test_lifecycle_and_refusals(W, O):
    w, h, spp = 64, 48, 2
    with pytest.raises(W.WfptError):
        W.shirley_path_tracer(w, h, max_wavefronts=4, flags=W.FLAG_ENV_NEE | W.FLAG_EMISSION | W.FLAG_NEE)
    plain = W.shirley_path_tracer(w, h, max_wavefronts=4, flags=base_flags(W))
    plain.set_environment(V.sun_map())
    for call in (lambda: plain.set_environment_share(0.5), plain.environment_distribution, lambda: plain.sample_environment_light(np.zeros((1, 10), F))):
        with pytest.raises(W.WfptError) as e:
            call()
        assert e.value.status == -1
    assert plain.environment_share() == 0.0
    plain.close()

    inputs = simple_inputs(O, w, h)
    env = V.sun_map()
    pt = make_tracer(W, "simple", w, h, max_wavefronts=5, flags=flags_of(W, "DENOISE"), max_window_size=80 * 48)
    pt.render(spp)  # captures a graph without the pass
    before = pt.accumulated()
    assert pt.environment_share() == 0.5
    for bad in (0.0, -0.5, 1.5, float("nan"), float("inf")):
        with pytest.raises(W.WfptError):
            pt.set_environment_share(bad)
    with pytest.raises(W.WfptError):
        pt.sample_environment_light(np.zeros((1, 10), F))  # no map yet
    assert_bits(pt.accumulated(), before, "a refused call resets nothing")
    pt.set_environment(env, **ENV_PARAMS)
    assert not pt.accumulated().any()
    pt.render(spp)
    em = E.Emission({}, spheres=inputs[0], materials=inputs[1])
    r = V.render_with_env_nee(make_oracle(O, inputs, w, h, max_wavefronts=5), make_oracle(O, inputs, w, h), em, env_light(env), spp=spp)
    assert_bits(pt.accumulated(), r, "after set_environment (no stale graph)")
    assert pt.nee_timing() == (0.0, 0)
    pt.render_timed(1)
    ms, n = pt.nee_timing()
    assert n >= 1 and ms > 0.0
    pt.set_environment_share(1.0)
    assert not pt.accumulated().any(), "set_environment_share restarts the accumulation"
    pt.render(spp)
    assert_bits(pt.accumulated(), r, "no emitter: the share does not matter")
    pt.render_parameters.set_viewport((80, 40))
    pt.update_buffers()
    row, marg = pt.environment_distribution()
    assert np.array_equal(row, V.Distribution(env).row), "a resize keeps the distribution"
    pt.render(spp)
    fresh = make_tracer(W, "simple", 80, 40, max_wavefronts=5, flags=flags_of(W, "DENOISE"))
    fresh.set_environment(env, **ENV_PARAMS)
    fresh.render(spp)
    assert_bits(pt.accumulated(), fresh.accumulated(), "after a resize")
    fresh.close()
    pt.clear_environment()
    pt.render_parameters.set_viewport((w, h))
    pt.update_buffers()
    pt.render(spp)
    assert_bits(pt.accumulated(), before, "after clear_environment")
    pt.close()


# ---------------------------------------------------------------- the payoff
def test_connecting_to_the_map_lowers_the_variance(W, O):
    """The ground with one occluder under the 2 x 2-block map, 160 x 120, 64 spp, miss_floor 0. Without the flag a sample is lit only if its
    scattered ray happens to leave through the block: probability about (solid angle) cos / pi = 1e-3, so its relative variance is about
    1 / p. With the flag what is left is the jitter inside a few texels. The ratio of the summed per-pixel variances is therefore far below
    1 / 10 whatever the machine. Measured on an MI355X: see DESIGN.md 9i. The two means must agree within 4 combined standard errors."""
    w, h, spp = 160, 120, 64
    inputs = V.ground_inputs(O, w, h, occluder=True)
    env = V.block_map()
    o = make_oracle(O, inputs, w, h, max_wavefronts=1, miss_floor=0, rng_mode=1)
    first = E.render_with_emission(o, E.Emission({}, spheres=inputs[0], materials=inputs[1]), spp=1, env=env, parts=True)["first_prim"][0]
    ok = first == int(np.argmax(inputs[0]["radius"]))
    assert ok.sum() > 10000
    stats = {}
    for name, env_nee in (("plain", False), ("env_nee", True)):
        pt = ground_tracer(W, inputs, w, h, max_wavefronts=4, miss_floor=0, rng_mode=W.RNG_PIXEL, flags=flags_of(W, "DENOISE", env_nee))
        pt.set_environment(env)
        pt.render(spp)
        var = pt.variance().reshape(-1)[ok].astype(np.float64)
        mean = R.luma(pt.accumulated())[ok].astype(np.float64).mean() / spp
        stats[name] = (var.sum(), mean, np.sqrt(var.sum()) / ok.sum())
        print(f"{name}: variance sum over {int(ok.sum())} ground pixels {var.sum():.6g}, mean luminance {mean:.6g} +- {stats[name][2]:.3g}")
        pt.close()
    ratio = stats["env_nee"][0] / stats["plain"][0]
    z = (stats["env_nee"][1] - stats["plain"][1]) / np.hypot(stats["env_nee"][2], stats["plain"][2])
    print(f"variance ratio env_nee / plain at {spp} spp: {ratio:.4g}; means differ by {z:.2f} combined standard errors")
    assert ratio < 0.1
    assert abs(z) <= 4.0
