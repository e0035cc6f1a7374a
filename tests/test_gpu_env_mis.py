"""Multiple importance sampling between the environment map and the scatter (WFPT_FLAG_ENV_MIS, include/wfpt.h "Environment multiple
importance sampling") on the GPU.

Whole renders are compared bit for bit with tests/env_mis_ref.py: the oracle's stages driven from Python with the throughput, the second
per-sample plane, the connected flag and the origin plane kept in numpy float32, the shadow rays traced by a second oracle. Every
material and map in these scenes is finite, so every pixel is compared. A restatement render depends on the scene, the size, the RNG mode
and the share alone -- not on the loop or the batch -- so each is computed once and shared."""
import numpy as np
import pytest

import denoise_ref as R
import emission_ref as E
import env_mis_ref as X
import env_nee_ref as V
import texture_ref as T
from helpers import assert_bits_or_nan, assert_second_trips, make_oracle
from test_gpu_env_nee import ENV_PARAMS, LAMP_E, LOOPS, env_light, ground_tracer, sampler_rows
from test_gpu_mis import two_triangle_lights
from test_gpu_nee import assert_bits, bits, compare, light, random_tex, shirley_scene

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def W(gpu):
    return gpu


@pytest.fixture(scope="module")
def O(orc):
    return orc


def flags_of(W, names, env_mis=True):
    f = W.FLAG_ENVIRONMENT | W.FLAG_EMISSION | W.FLAG_NEE | W.FLAG_ENV_NEE | (W.FLAG_ENV_MIS if env_mis else 0)
    for n in (names.split("|") if names else []):
        f |= getattr(W, "FLAG_" + n)
    return f


# ---------------------------------------------------------------- bit for bit against the restatement
SIZES = [(64, 48), (100, 60)]  # (100 x 60: not a multiple of 8)
CASES = {"share 0.5": (True, 0.5), "share 1.0": (True, 1.0), "no emitter": (False, 0.5)}
SPP, WAVEFRONTS = 3, 4
_ground = {}


def ground_reference(O, w, h, rng, case):
    """The restatement's render of ground + lamp + occluder + mirror under the sun map, once per (size, RNG mode, case)."""
    key = (w, h, rng, case)
    if key not in _ground:
        lamp, share = CASES[case]
        inputs = V.ground_inputs(O, w, h, occluder=True, mirror=True, lamp=True)
        em = E.Emission({1: LAMP_E} if lamp else {}, spheres=inputs[0], materials=inputs[1])
        o = make_oracle(O, inputs, w, h, max_wavefronts=WAVEFRONTS, miss_floor=0, rng_mode=rng)
        _ground[key] = X.render_with_env_mis(o, make_oracle(O, inputs, w, h), em, env_light(V.sun_map()), share=share, spp=SPP, parts=True)
    return _ground[key]


def ground_scene(W, O, w, h, case="share 0.5", env=None, **kw):
    lamp, share = CASES[case]
    inputs = V.ground_inputs(O, w, h, occluder=True, mirror=True, lamp=True)
    pt = ground_tracer(W, inputs, w, h, max_wavefronts=WAVEFRONTS, miss_floor=0, **kw)
    pt.set_environment(V.sun_map() if env is None else env, **ENV_PARAMS)
    if lamp:
        pt.set_emission(1, LAMP_E)
    if share != 0.5:
        pt.set_environment_share(share)
    return pt


@pytest.mark.parametrize("rng", [0, 1])
@pytest.mark.parametrize("loop", LOOPS)
def test_ground_equals_restatement(W, O, loop, rng):
    for w, h in SIZES:
        for case in CASES:
            r = ground_reference(O, w, h, rng, case)
            st = r["stats"]
            assert st["weighed_misses"] > 0 and st["env_samples"] > 0
            assert (st["light_samples"] > 0) == (case == "share 0.5") and (st["weighed_hits"] > 0) == CASES[case][0], (case, st)
            for batch in (1, 3):
                pt = ground_scene(W, O, w, h, case, rng_mode=rng, flags=flags_of(W, loop) | W.FLAG_DENOISE, batch=batch)
                assert pt.nee_light_count() == int(CASES[case][0])
                pt.render(SPP)
                compare(pt, r, SPP, w, h, f"ground {w}x{h} {case} {loop} rng {rng} batch {batch}")
                pt.close()


def test_the_flag_changes_the_render(W, O):
    """The parity above would hold trivially if the restatement's weights did nothing: it differs from ENV_NEE's, in both planes."""
    w, h = SIZES[0]
    r = ground_reference(O, w, h, 1, "share 0.5")
    inputs = V.ground_inputs(O, w, h, occluder=True, mirror=True, lamp=True)
    em = E.Emission({1: LAMP_E}, spheres=inputs[0], materials=inputs[1])
    o = make_oracle(O, inputs, w, h, max_wavefronts=WAVEFRONTS, miss_floor=0, rng_mode=1)
    nee = V.render_with_env_nee(o, make_oracle(O, inputs, w, h), em, env_light(V.sun_map()), spp=SPP, parts=True)
    assert (r["image"] > nee["image"]).any(), "no weighed miss kept its throughput"
    assert (r["emitted"] < nee["emitted"]).any(), "no connect sample was weighed down"
    assert (r["emitted"] > nee["emitted"]).any(), "no scattered ray's hit on the lamp was kept"


@pytest.mark.parametrize("loop", ["", "UNFUSED", "NO_LDS_SCENE", "NO_LDS_SCENE|BINARY_BVH", "NO_LDS_SCENE|NO_REFILL"])
def test_triangle_ground_with_a_triangle_light_equals_restatement(W, O, loop):
    """A Lambertian wall of two triangles with two emitting triangles in front of it, under the sun map: the triangle forms of both
    branches and of the emission pass's weight; rays that pass the wall's edge, and the wall's scattered rays, miss into the map."""
    w, h = 100, 60
    tris, mt = two_triangle_lights(O)
    tb, nodes = O.build_bvh_triangles(tris, 32)
    cam, ip, vw = O.mesh_camera(w, h)
    colours = {1: (3.0, 2.0, 1.0)}
    em = E.Emission(colours, triangles=tb, materials=mt)
    cc = W.CameraController(W.Camera((0.0, 0.0, 30.0), (0.0, 0.0, 0.0)), 40.0, 0.0, 10.0, 0.1, 100.0)
    env = V.sun_map()
    for rng in (0, 1):
        o = O.Oracle(w, h, np.zeros(1, O.SPHERE), mt, nodes, cam, ip, vw, triangles=tb, max_wavefronts=WAVEFRONTS, miss_floor=0, rng_mode=rng)
        shadow = O.Oracle(w, h, np.zeros(1, O.SPHERE), mt, nodes, cam, ip, vw, triangles=tb)
        r = X.render_with_env_mis(o, shadow, em, env_light(env), spp=SPP, parts=True)
        st = r["stats"]
        assert min(st.values()) > 0, st
        for batch in (1, 3):
            scene = W.Scene(np.zeros(0, W.SPHERE), mt.view(W.MATERIAL), triangles=tris.view(W.TRIANGLE).copy())
            pt = W.PathTracer(scene, W.RenderParameters(cc, (w, h)), max_wavefronts=WAVEFRONTS, miss_floor=0, rng_mode=rng,
                              flags=flags_of(W, loop) | W.FLAG_DENOISE, batch=batch)
            light(pt, colours)
            pt.set_environment(env, **ENV_PARAMS)
            assert pt.nee_light_count() == 2
            pt.render(SPP)
            compare(pt, r, SPP, w, h, f"triangles {loop} rng {rng} batch {batch}")
            pt.close()


@pytest.mark.parametrize("loop", ["", "UNFUSED", "NO_LDS_SCENE"])
def test_textured_light_equals_restatement(W, O, loop):
    w, h = 100, 60
    sp, mt, colours = shirley_scene(O)
    lamps = sorted(colours)
    slots = {0: (random_tex(64, 32, 1), {"scale": (3.0, 2.0), "offset": (0.25, -0.5)}), 1: (random_tex(17, 9, 2), {"filter": "nearest"})}
    bind = {lamps[0]: 0, lamps[1]: 1}
    env = V.sun_map()
    tx = T.Textures(spheres=sp, materials=mt, slots=slots, bind=bind)
    r = X.render_with_env_mis(O.shirley_oracle(w, h, max_wavefronts=WAVEFRONTS), O.shirley_oracle(w, h), E.Emission(colours, spheres=sp, materials=mt),
                              env_light(env), spp=SPP, tx=tx, parts=True)
    assert min(r["stats"].values()) > 0, r["stats"]
    pt = W.shirley_path_tracer(w, h, max_wavefronts=WAVEFRONTS, flags=flags_of(W, loop) | W.FLAG_TEXTURES)
    for s, (img, params) in slots.items():
        pt.set_texture(s, img, **params)
    light(pt, colours)
    for m, s in bind.items():
        pt.bind_texture(m, s)
    pt.set_environment(env, **ENV_PARAMS)
    pt.render(SPP)
    compare(pt, r, SPP, w, h, f"textured lights {loop}")
    pt.close()


# ---------------------------------------------------------------- the same bits however the samples are scheduled
def test_two_band_shards_equal_the_whole_frame(W, O):
    w, h, spp = 100, 60, 4
    whole = ground_scene(W, O, w, h, rng_mode=W.RNG_PIXEL, flags=flags_of(W, ""))
    whole.render(spp)
    base = whole.accumulated()
    whole.close()
    full = np.zeros((h, w, 3), F)
    for r in range(2):
        pt = ground_scene(W, O, w, h, rng_mode=W.RNG_PIXEL, flags=flags_of(W, ""), tile_rank=r, tile_world=2)
        pt.render(spp)
        b = pt.accumulated().reshape(-1, 8, w, 3)
        pt.close()
        for j in range(b.shape[0]):
            y0 = (j * 2 + r) * 8
            full[y0:y0 + 8] = b[j][:max(0, min(8, h - y0))]
    assert_bits(full.reshape(-1, 3), base, "two band-sharded contexts")


def test_second_trips_through_the_segment_loop(W, O):
    """68 segments: at batch 128 the miss and emission launches run 64 workgroups per sample, so four of them walk a second segment; at
    batch 16 they run 68 and none does. Same bits, and the stage loop's at batch 128 as well."""
    w, h, spp = 256, 136, 128
    got = {}
    for loop, batch in (("", 128), ("", 16), ("UNFUSED", 128)):
        pt = ground_scene(W, O, w, h, rng_mode=W.RNG_PIXEL, flags=flags_of(W, loop), batch=batch)
        assert_second_trips(W, pt, 128, 16)
        pt.render(spp)
        got[loop, batch] = pt.accumulated()
        pt.close()
    assert_bits(got["", 128], got["", 16], "batch 128 against batch 16")
    assert_bits(got["UNFUSED", 128], got["", 128], "the stage loop against the fused one, batch 128")


def test_a_change_between_renders_switches_kernels_and_drops_the_graphs(W, O):
    """set_environment_share, set_emission and clear_environment between renders: each leg equals a fresh context in that state."""
    w, h, spp = 64, 48, 2
    inputs = V.ground_inputs(O, w, h, occluder=True, mirror=True, lamp=True)
    kw = dict(max_wavefronts=WAVEFRONTS, miss_floor=0, rng_mode=W.RNG_PIXEL, flags=flags_of(W, ""))

    def fresh(env, lamp, share):
        pt = ground_tracer(W, inputs, w, h, **kw)
        if env:
            pt.set_environment(V.sun_map(), **ENV_PARAMS)
        if lamp:
            pt.set_emission(1, LAMP_E)
        pt.set_environment_share(share)
        pt.render(spp)
        acc = pt.accumulated()
        pt.close()
        return acc

    pt = ground_tracer(W, inputs, w, h, **kw)
    pt.set_environment(V.sun_map(), **ENV_PARAMS)
    pt.render(spp)  # captures graphs with the no-emitter kernels
    assert_bits(pt.accumulated(), fresh(True, False, 0.5), "map only")
    pt.set_emission(1, LAMP_E)
    pt.render(spp)
    assert_bits(pt.accumulated(), fresh(True, True, 0.5), "after set_emission")
    pt.set_environment_share(0.25)
    pt.render(spp)
    assert_bits(pt.accumulated(), fresh(True, True, 0.25), "after set_environment_share")
    pt.clear_environment()
    pt.render(spp)
    assert_bits(pt.accumulated(), fresh(False, True, 0.25), "after clear_environment")
    pt.set_environment(V.sun_map(), **ENV_PARAMS)
    pt.clear_emission()
    pt.render(spp)
    assert_bits(pt.accumulated(), fresh(True, False, 0.25), "the map again, the lamp gone")
    pt.close()


# ---------------------------------------------------------------- the samplers
def test_samplers_equal_the_restatement(W, O):
    k = 4096
    w, h = 64, 48
    inputs = V.ground_inputs(O, w, h, occluder=True, mirror=True, lamp=True)
    env = V.sun_map()
    lightr = env_light(env)
    shadow = make_oracle(O, inputs, w, h)
    for lamp, share in ((True, 0.25), (False, 0.5)):
        pt = ground_tracer(W, inputs, w, h, max_wavefronts=2, flags=flags_of(W, ""))
        pt.set_environment(env, **ENV_PARAMS)
        if lamp:
            pt.set_emission(1, LAMP_E)
        pt.set_environment_share(share)
        p_eff = share if lamp else 1.0  # the effective share
        rows = sampler_rows(k, 9)
        rows[:, :3] = rows[:, :3] + np.array([0.0, 2.0, 1.0], F)  # above the ground
        rows[k // 2:, 3:6] = (0.0, 1.0, 0.0)
        got = pt.sample_environment_light_mis(rows)
        want = X.sample_rows(lightr, shadow, rows, p_eff)
        assert got.shape == (k, 12)
        assert_bits(got[:, :7], want[:, :7], f"lamp {lamp}: wdir, texel, (e Genv) we")
        assert np.array_equal(got[:, 7] != 0, want[:, 7] != 0), "the occlusion verdict is not the oracle's"
        assert_bits(got[:, 8:], want[:, 8:], f"lamp {lamp}: pe, pb, we")
        lit = want[:, 10] > 0
        assert lit.sum() > k // 4 and (~lit).sum() > k // 10 and (want[:, 7] != 0).any() and (lit & (want[:, 7] == 0)).any()
        # the miss side: the samples replayed as scattered rays, random directions, the edge directions and bad rows
        rng = np.random.default_rng(12)
        with np.errstate(all="ignore"):
            cos_s = want[lit, 9] * X.PI
            d = (want[lit, :3] * (F(2) * cos_s)[:, None]).astype(F)
        dirs = np.concatenate([d, (rng.standard_normal((k - len(d), 3)) * rng.random((k - len(d), 1)) * 2).astype(F)])
        gw = pt.env_mis_miss_weight(dirs)
        ww = X.miss_weight_rows(lightr, dirs, p_eff)
        assert_bits(gw, ww, f"lamp {lamp}: wfpt_env_mis_miss_weight")
        same = gw[:len(d), 3] == want[lit, 3]
        gap = np.abs(want[lit, 10].astype(np.float64) + gw[:len(d), 2].astype(np.float64) - 1.0)[same]
        print(f"lamp {lamp}: worst |we + wb - 1| on the device {gap.max():.3g}; the reverse texel differs in {1 - same.mean():.2g} of {len(d)} rows")
        assert gap.max() < 2.0 ** -22 and 1 - same.mean() <= 1e-3  # tests/test_env_mis_host.py's bound and cap (the restatement on these rows: 1.19e-07, 3.3e-04)
        edge = np.array([(0, 0, 0), (np.nan, 0, 1), (0, np.nan, 0), (np.inf, 0, 0), (0, -np.inf, 0), (np.inf, np.inf, np.inf), (0, 1, 0), (0, -1, 0),
                         (0, 2.5, 0), (0, -1e-30, 0), (1e-30, 0, 0), (1e30, 1e30, 1e30), (0, 0, -1), (-1e-9, 0, -1), (1e-9, 0, -1), (1e-30, 1e-30, 1e-30)], F)
        ge = pt.env_mis_miss_weight(edge)
        assert_bits_or_nan(ge, X.miss_weight_rows(lightr, edge, p_eff), "edge directions")
        assert (ge[:10, 2] == 1).all() and (ge[:10, 0] == 0).all() and ((ge[:, 3] >= 0) & (ge[:, 3] < env.shape[0] * env.shape[1])).all()
        bad = sampler_rows(64, 10)  # NaN and infinite receivers, normals and draws
        for j, col in enumerate(range(10)):
            bad[j, col] = np.nan
            bad[10 + j, col] = np.inf
            bad[20 + j, col] = -np.inf
        for j in (0, 1, 2, 10, 11, 12, 20, 21, 22):
            bad[j, 3:6] = 0.0  # a receiver that is no point sends no shadow ray (cos_s = 0): there is no verdict to compare
        gb, wb_ = pt.sample_environment_light_mis(bad), X.sample_rows(lightr, shadow, bad, p_eff)
        assert_bits_or_nan(gb[:, :7], wb_[:, :7], "NaN and inf rows: wdir, texel, value")
        assert_bits_or_nan(gb[:, 8:], wb_[:, 8:], "NaN and inf rows: pe, pb, we")
        assert np.array_equal(gb[:, 7] != 0, wb_[:, 7] != 0)
        pt.close()


# ---------------------------------------------------------------- no map, a black one, or one that came and went: the flag does nothing
@pytest.mark.parametrize("loop", ["", "UNFUSED", "NO_LDS_SCENE"])
@pytest.mark.parametrize("emitter", [False, True])
@pytest.mark.parametrize("state", ["no map", "black map", "set then cleared"])
def test_flag_without_a_distribution_is_a_context_without_the_flag(W, O, loop, emitter, state):
    w, h, spp = 100, 60, 4
    results = []
    for env_mis in (False, True):
        pt = W.shirley_path_tracer(w, h, max_wavefronts=6, flags=flags_of(W, loop, env_mis))
        if state == "set then cleared":
            pt.set_environment(V.sun_map())
            if env_mis:
                assert pt.env_mis_miss_weight(np.ones((1, 3), F)).shape == (1, 4)
            pt.clear_environment()
        if state == "black map":
            pt.set_environment(np.zeros((4, 8, 3), F))
        if emitter:
            pt.set_emission(0, (4.0, 3.0, 2.0))
        if env_mis:
            with pytest.raises(W.WfptError):
                pt.env_mis_miss_weight(np.ones((1, 3), F))
        pt.render(spp)
        acc = pt.accumulated()
        ms, launches = pt.render_timed(spp)
        results.append((acc, launches, pt.totals(), pt.nee_timing()[1], pt.emission_timing()[1]))
        pt.close()
    a, b = results
    assert_bits(b[0], a[0], f"{loop} emitter {emitter} {state}")
    assert np.array_equal(a[1], b[1]), f"launch counts per stage: {a[1]} vs {b[1]}"
    assert np.array_equal(a[2], b[2]) and a[3] == b[3] and a[4] == b[4]


# ---------------------------------------------------------------- refusals
def test_refusals(W, O):
    w, h = 48, 32
    all4 = W.FLAG_ENVIRONMENT | W.FLAG_EMISSION | W.FLAG_NEE | W.FLAG_ENV_NEE
    for flags in [W.FLAG_ENV_MIS | (all4 & ~m) for m in (W.FLAG_ENVIRONMENT, W.FLAG_EMISSION, W.FLAG_NEE, W.FLAG_ENV_NEE)] + [W.FLAG_ENV_MIS | all4 | W.FLAG_MIS]:
        with pytest.raises(W.WfptError):
            W.shirley_path_tracer(w, h, max_wavefronts=4, flags=flags)
    plain = W.shirley_path_tracer(w, h, max_wavefronts=4, flags=all4)
    plain.set_environment(V.sun_map())
    for call in (lambda: plain.sample_environment_light_mis(np.zeros((1, 10), F)), lambda: plain.env_mis_miss_weight(np.zeros((1, 3), F))):
        with pytest.raises(W.WfptError) as e:
            call()
        assert e.value.status == -1
    plain.close()
    pt = W.shirley_path_tracer(w, h, max_wavefronts=4, flags=flags_of(W, ""))
    for call in (lambda: pt.sample_environment_light_mis(np.zeros((1, 10), F)), lambda: pt.env_mis_miss_weight(np.zeros((1, 3), F))):
        with pytest.raises(W.WfptError) as e:  # no map yet
            call()
        assert e.value.status == -1
    pt.set_environment(V.sun_map())
    assert pt.sample_environment_light_mis(np.zeros((0, 10), F)).shape == (0, 12) and pt.env_mis_miss_weight(np.zeros((0, 3), F)).shape == (0, 4)
    L = W.lib()
    assert L.wfpt_sample_environment_light_mis(pt.handle, None, 4, None) == -1 and L.wfpt_env_mis_miss_weight(pt.handle, None, 4, None) == -1
    pt.close()


# ---------------------------------------------------------------- the payoff
def test_weighing_the_map_lowers_the_variance(W, O):
    """160 x 120, 32 spp, WFPT_RNG_PIXEL, WFPT_FLAG_DENOISE, miss_floor 0, the ground with the occluder: under the soft sky (the sun map
    without its sun) the sum of wfpt_read_variance over the ground pixels with the flag is below ENV_NEE's, under the sun map it is below
    ENVIRONMENT's alone, and in each pair the means agree within 4 combined standard errors."""
    w, h, spp = 160, 120, 32
    inputs = V.ground_inputs(O, w, h, occluder=True)
    o = make_oracle(O, inputs, w, h, max_wavefronts=1, miss_floor=0, rng_mode=1)
    first = E.render_with_emission(o, E.Emission({}, spheres=inputs[0], materials=inputs[1]), spp=1, env=V.sun_map(), parts=True)["first_prim"][0]
    ok = first == int(np.argmax(inputs[0]["radius"]))
    assert ok.sum() > 10000
    legs = {"environment": W.FLAG_ENVIRONMENT, "env_nee": flags_of(W, "", False), "env_mis": flags_of(W, "")}
    for name, env, other in (("soft sky", X.soft_sky(), "env_nee"), ("sun map", V.sun_map(), "environment")):
        sums, means, ses = {}, {}, {}
        for leg in ("env_mis", other):
            pt = ground_tracer(W, inputs, w, h, max_wavefronts=4, miss_floor=0, rng_mode=W.RNG_PIXEL, flags=legs[leg] | W.FLAG_DENOISE)
            pt.set_environment(env)
            pt.render(spp)
            var = pt.variance().reshape(-1)[ok].astype(np.float64)
            sums[leg] = float(var.sum())
            means[leg] = R.luma(pt.accumulated())[ok].astype(np.float64).mean() / spp
            ses[leg] = np.sqrt(var.sum() * spp / (spp - 1)) / ok.sum()  # wfpt_read_variance is the variance of the pixel's mean
            print(f"{name} {leg}: variance sum over {int(ok.sum())} ground pixels {sums[leg]:.6g}, mean luminance {means[leg]:.6g} +- {ses[leg]:.3g}")
            pt.close()
        z = (means["env_mis"] - means[other]) / np.hypot(ses["env_mis"], ses[other])
        print(f"{name}: variance ratio env_mis / {other} {sums['env_mis'] / sums[other]:.4g}; means differ by {z:.2f} combined standard errors")
        assert sums["env_mis"] < sums[other]
        assert abs(z) <= 4.0
