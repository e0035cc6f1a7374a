"""Light selection by power (WFPT_FLAG_LIGHT_POWER, include/wfpt.h "Light selection by power") on the GPU.

The device's tables, its three samplers and whole renders are compared bit for bit with tests/light_power_ref.py: nee_ref's and mis_ref's
restatements with the selection by the integer distribution and nfi in nf's place. Renders compared with the restatement stay at 64 x 48
with at most 4 wavefronts (the restatement drives the CPU oracle)."""
import numpy as np
import pytest

import denoise_ref as R
import emission_ref as E
import light_power_ref as P
import nee_ref as N
import retire_ref as RR
import test_gpu_nee as G
import texture_ref as T
from test_gpu_nee import assert_bits, bits, compare, light, mesh_inputs, mesh_tracer, shirley_scene
from test_nee_host import closed_form

pytestmark = pytest.mark.gpu

F = np.float32
W_, H_, MAXW = 64, 48, 4


@pytest.fixture(scope="module")
def W(gpu):
    return gpu


@pytest.fixture(scope="module")
def O(orc):
    return orc


def flags_of(W, names, mis=False, power=True):
    f = W.FLAG_EMISSION | W.FLAG_NEE | (W.FLAG_MIS if mis else 0) | (W.FLAG_LIGHT_POWER if power else 0)
    for n in (names.split("|") if names else []):
        f |= getattr(W, "FLAG_" + n)
    return f


MESH_COLOURS = {1: (2.0, 1.0, 0.5)}


def mesh_oracles(O, w, h, **kw):
    tris, mt, nodes, cam, ip, vw = mesh_inputs(O, w, h)
    o = O.Oracle(w, h, np.zeros(1, O.SPHERE), mt, nodes, cam, ip, vw, triangles=tris, **kw)
    shadow = O.Oracle(w, h, np.zeros(1, O.SPHERE), mt, nodes, cam, ip, vw, triangles=tris)
    return tris, mt, o, shadow


def assert_tables(pt, lights, what):
    """light_distribution() against PowerLights.tables(), exactly"""
    prims, cdf = pt.light_distribution()
    assert prims.dtype == np.uint32 and cdf.dtype == np.uint64
    assert np.array_equal(prims.astype(np.int64), lights.list), what + ": the light list"
    assert np.array_equal(cdf, lights.cdf), what + ": cdf"
    assert int(cdf[-1]) == lights.total
    k = np.diff(np.concatenate([[0], cdf.astype(np.int64)]))
    assert np.array_equal(k, lights.k.astype(np.int64)), what + ": k"


# ---------------------------------------------------------------- the tables
def test_tables_equal_the_restatement(W, O):
    """3 lights (fewer than a wave) and the mesh's material 1 (more than one workgroup of the scan, no multiple of its 256 lights)."""
    sp, mt, colours = shirley_scene(O)
    pt = W.shirley_path_tracer(W_, H_, max_wavefronts=2, flags=flags_of(W, ""))
    light(pt, colours)
    lights = P.PowerLights(E.Emission(colours, spheres=sp, materials=mt))
    assert lights.n == 3 == pt.nee_light_count() and len(set(lights.k.tolist())) == 3
    assert_tables(pt, lights, "shirley")
    # (either pointer may be NULL)
    L = W.lib()
    cdf = np.zeros(3, "<u8")
    assert L.wfpt_read_light_distribution(pt.handle, None, cdf.ctypes.data_as(W.C.c_void_p)) == 0 and np.array_equal(cdf, lights.cdf)
    assert L.wfpt_read_light_distribution(pt.handle, None, None) == 0
    pt.close()
    tris, mt, nodes, cam, ip, vw = mesh_inputs(O, W_, H_)
    pt = mesh_tracer(W, W_, H_, max_wavefronts=2, flags=flags_of(W, ""))
    light(pt, MESH_COLOURS)
    lights = P.PowerLights(E.Emission(MESH_COLOURS, triangles=tris, materials=mt))
    assert lights.n == pt.nee_light_count() and lights.n > 2 * 256 and lights.n % 256 != 0 and lights.total > 2 ** 24
    assert_tables(pt, lights, "mesh")
    pt.close()


# ---------------------------------------------------------------- the samplers
def check_power_samplers(O, pt, lights, shadow, rows, n_prims, mis, what):
    got = pt.sample_lights(rows)
    want, s = lights.sample_rows(shadow, rows)
    G.check_sampler(O, got, s, rows, shadow, what)  # q, primitive, e_q G, occlusion, and its non-vacuity conditions
    assert_bits(got, want, what + ": wfpt_sample_lights")
    assert len(set(s["prim"].tolist())) > 1 and (s["nfi"] != F(lights.n)).any(), what + ": nfi is nf everywhere"
    plain = N.Lights(lights.em)
    ps = plain.sample(rows[:, :3], rows[:, 3:6], rows[:, 6], rows[:, 7], rows[:, 8])
    assert not np.array_equal(ps["prim"], s["prim"]), what + ": the selection is the uniform one"
    if not mis:
        return
    got = pt.sample_lights_mis(rows)
    want = P.sample_rows_mis(lights, shadow, rows)
    assert got.shape == (len(rows), 12)
    assert_bits(got, want, what + ": wfpt_sample_lights_mis")
    lit = want[:, 10] > 0
    assert lit.sum() > len(rows) // 10 and (~lit).sum() > len(rows) // 10 and (want[:, 7] != 0).any() and (lit & (want[:, 7] == 0)).any(), what
    # the hit side: the connect samples replayed as scattered rays (test_gpu_mis.py's construction), and random hits on any primitive
    rng = np.random.default_rng(12)
    with np.errstate(all="ignore"):
        cos_s = want[:, 9] * N.PI
        v = want[:, :3] - rows[:, :3]
        dist = np.sqrt(N.dot3(v, v))
        d = (F(2) * cos_s)[:, None] * (v / dist[:, None])
        t = dist / (F(2) * cos_s)
    hit = np.concatenate([rows[:, :3], d, t[:, None], want[:, 3:4]], 1).astype(F)[lit]
    rnd = np.concatenate([rng.standard_normal((500, 6)) * 3, rng.random((500, 1)) * 4, rng.integers(-2, n_prims + 2, (500, 1))], 1).astype(F)
    hits = np.concatenate([hit, rnd])
    gw, ww = pt.mis_hit_weight(hits), P.hit_weight_rows(lights, hits)
    both_nan = np.isnan(gw) & np.isnan(ww)  # (a NaN's payload is not part of the contract)
    assert_bits(np.where(both_nan, F(0), gw), np.where(both_nan, F(0), ww), what + ": wfpt_mis_hit_weight")
    assert (gw[:len(hit), 2] < 1).mean() > 0.9 and (gw[len(hit):, 2] == 1).any(), what


@pytest.mark.parametrize("mis", [False, True])
@pytest.mark.parametrize("loop", ["", "EXACT_TRAVERSAL", "NO_LDS_SCENE", "NO_LDS_SCENE|BINARY_BVH"])
def test_samplers_equal_the_restatement(W, O, loop, mis):
    k = 3000
    sp, mt, colours = shirley_scene(O)
    pt = W.shirley_path_tracer(W_, H_, max_wavefronts=2, flags=flags_of(W, loop, mis))
    light(pt, colours)
    lights = P.PowerLights(E.Emission(colours, spheres=sp, materials=mt))
    rows = G.sampler_rows((0.0, 1.0, 0.0), k, 5)
    c = sp["center"][lights.list[0], :3]  # grazing, as test_gpu_nee.py turns the normals
    d = c - rows[k // 2:, :3]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    t = np.cross(d, rows[k // 2:, 3:6])
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    rows[k // 2:, 3:6] = t + d * np.linspace(-1e-3, 1e-3, k - k // 2)[:, None]
    rows[4:8, 6] = (np.nan, -0.5, 2.0, 1.0)  # selection edges beside sampler_rows' own 0, 1 - 2^-24, 1.0
    check_power_samplers(O, pt, lights, O.shirley_oracle(W_, H_), rows, len(sp), mis, f"spheres {loop}")
    pt.close()
    tris, mt, nodes, cam, ip, vw = mesh_inputs(O, W_, H_)
    pt = mesh_tracer(W, W_, H_, max_wavefronts=2, flags=flags_of(W, loop, mis))
    light(pt, MESH_COLOURS)
    lights = P.PowerLights(E.Emission(MESH_COLOURS, triangles=tris, materials=mt))
    shadow = O.Oracle(W_, H_, np.zeros(1, O.SPHERE), mt, nodes, cam, ip, vw, triangles=tris)
    rows = G.sampler_rows((0.0, 0.0, 0.0), k, 6)
    rows[4:8, 6] = (np.nan, -0.5, 2.0, 1.0)
    check_power_samplers(O, pt, lights, shadow, rows, len(tris), mis, f"mesh {loop}")
    pt.close()


# ---------------------------------------------------------------- renders, bit for bit
@pytest.mark.parametrize("mis", [False, True])
@pytest.mark.parametrize("rng", [0, 1])
@pytest.mark.parametrize("loop", ["", "UNFUSED", "NO_LDS_SCENE"])
def test_shirley_equals_restatement(W, O, loop, rng, mis):
    spp = 2
    sp, mt, colours = shirley_scene(O)
    pt = W.shirley_path_tracer(W_, H_, max_wavefronts=MAXW, rng_mode=rng, flags=flags_of(W, loop, mis) | W.FLAG_DENOISE)
    light(pt, colours)
    pt.render(spp)
    em = E.Emission(colours, spheres=sp, materials=mt)
    r = P.render_with_power(O.shirley_oracle(W_, H_, max_wavefronts=MAXW, rng_mode=rng), O.shirley_oracle(W_, H_), em, mis=mis, spp=spp, parts=True)
    compare(pt, r, spp, W_, H_, f"shirley {loop} rng {rng} mis {mis}")
    if loop == "":
        ref = (P.M.render_with_mis if mis else N.render_with_nee)(O.shirley_oracle(W_, H_, max_wavefronts=MAXW, rng_mode=rng), O.shirley_oracle(W_, H_),
                                                                  em, spp=spp)
        assert not np.array_equal(bits(ref), bits(r["acc"])), "the selection by power changes nothing"
    pt.close()


@pytest.mark.parametrize("mis", [False, True])
@pytest.mark.parametrize("loop", ["", "NO_LDS_SCENE", "NO_LDS_SCENE|NO_REFILL", "UNFUSED"])
def test_mesh_equals_restatement(W, O, loop, mis):
    spp = 2
    pt = mesh_tracer(W, W_, H_, max_wavefronts=MAXW, rng_mode=1, flags=flags_of(W, loop, mis))
    light(pt, MESH_COLOURS)
    pt.render(spp)
    tris, mt, o, shadow = mesh_oracles(O, W_, H_, max_wavefronts=MAXW, rng_mode=1)
    r = P.render_with_power(o, shadow, E.Emission(MESH_COLOURS, triangles=tris, materials=mt), mis=mis, spp=spp, parts=True)
    compare(pt, r, spp, W_, H_, f"mesh {loop} mis {mis}")
    pt.close()


@pytest.mark.parametrize("mis", [False, True])
def test_textured_light_and_retire(W, O, mis):
    """A textured light: the texture modulates e_q and does not enter the distribution. And WFPT_FLAG_RETIRE with roulette from wavefront 1
    on, against the restatement over retire_ref's wrapped oracle."""
    spp = 2
    sp, mt, colours = shirley_scene(O)
    lamps = sorted(colours)
    slots = {0: (G.random_tex(64, 32, 1), {"scale": (3.0, 2.0), "offset": (0.25, -0.5)})}
    bind = {lamps[0]: 0}
    pt = W.shirley_path_tracer(W_, H_, max_wavefronts=MAXW, flags=flags_of(W, "", mis) | W.FLAG_TEXTURES)
    pt.set_texture(0, slots[0][0], **slots[0][1])
    light(pt, colours)
    before = pt.light_distribution()[1]
    pt.bind_texture(lamps[0], 0)
    assert np.array_equal(pt.light_distribution()[1], before), "a texture binding enters the distribution"
    pt.render(spp)
    em = E.Emission(colours, spheres=sp, materials=mt)
    tx = T.Textures(spheres=sp, materials=mt, slots=slots, bind=bind)
    r = P.render_with_power(O.shirley_oracle(W_, H_, max_wavefronts=MAXW), O.shirley_oracle(W_, H_), em, mis=mis, spp=spp, tx=tx, parts=True)
    compare(pt, r, spp, W_, H_, f"textured light, mis {mis}")
    pt.close()
    pt = W.shirley_path_tracer(W_, H_, max_wavefronts=MAXW, flags=flags_of(W, "RETIRE", mis))
    pt.set_termination(roulette_start=1, q_min=0.25)
    light(pt, colours)
    pt.render(spp)
    o = RR.Retiring(O.shirley_oracle(W_, H_, max_wavefronts=MAXW), roulette_start=1, q_min=0.25)
    r = P.render_with_power(o, O.shirley_oracle(W_, H_), em, mis=mis, spp=spp, parts=True, termination=o)
    assert_bits(pt.accumulated(), r["acc"], f"retire, mis {mis}")
    assert sum(map(sum, o.retired)) > 0
    pt.close()


# ---------------------------------------------------------------- the same bits however the samples are scheduled
@pytest.mark.parametrize("mis", [False, True])
def test_same_bits_across_batches_stage_loop_split_shade_and_shards(W, O, mis):
    w, h, spp = 100, 60, 130  # no multiple of 8 either way; 128 + a remainder
    _, _, colours = shirley_scene(O)
    kw = dict(max_wavefronts=5, miss_floor=0, rng_mode=W.RNG_PIXEL)
    base = None
    for loop, batch in [("", 1), ("", 16), ("", 128), ("SPLIT_SHADE", 0), ("UNFUSED", 16)]:
        pt = W.shirley_path_tracer(w, h, flags=flags_of(W, loop, mis), batch=batch, **kw)
        light(pt, colours)
        pt.render(spp)
        if base is None:
            base = pt.accumulated()
        else:
            assert_bits(pt.accumulated(), base, f"loop {loop} batch {batch}")
        pt.close()
    full = np.zeros((h, w, 3), F)
    for r in range(2):
        pt = W.shirley_path_tracer(w, h, flags=flags_of(W, "", mis), tile_rank=r, tile_world=2, **kw)
        light(pt, colours)
        pt.render(spp)
        b = pt.accumulated().reshape(-1, 8, w, 3)
        pt.close()
        for j in range(b.shape[0]):
            y0 = (j * 2 + r) * 8
            full[y0:y0 + 8] = b[j][:max(0, min(8, h - y0))]
    assert_bits(full.reshape(-1, 3), base, "two band-sharded contexts")
    w8, h8 = 96, 56  # the host-driven stage loop: whole tiles only
    pt = W.shirley_path_tracer(w8, h8, flags=flags_of(W, "", mis), **kw)
    light(pt, colours)
    for _ in range(3):
        pt.run()
    host = pt.accumulated()
    pt.close()
    pt = W.shirley_path_tracer(w8, h8, flags=flags_of(W, "", mis), **kw)
    light(pt, colours)
    pt.render(3)
    assert_bits(host, pt.accumulated(), "host-driven stage loop")
    pt.close()


# ---------------------------------------------------------------- one light, no emitter
@pytest.mark.parametrize("mis", [False, True])
def test_one_light_is_the_unflagged_context(W, O, mis):
    w, h, spp = 96, 72, 4
    inputs = N.lamp_inputs(O, w, h, mirror=True)
    rows = G.sampler_rows((0.0, 1.0, 0.0), 2000, 8)
    out = {}
    for power in (False, True):
        pt = G.lamp_tracer(W, inputs, w, h, max_wavefronts=4, miss_floor=0, flags=flags_of(W, "", mis, power) | W.FLAG_ENVIRONMENT)
        pt.set_environment(N.black_env())
        pt.set_emission(1, N.LAMP["e"])
        if power:
            prims, cdf = pt.light_distribution()
            assert prims.tolist() == [int(np.flatnonzero(inputs[0]["material_idx"] == 1)[0])] and cdf.tolist() == [65535]
        pt.render(spp)
        hits = np.concatenate([rows[:, :6], rows[:, 6:7] * 4, np.full((len(rows), 1), prims[0] if power else 0, F)], 1).astype(F)
        out[power] = (pt.accumulated(), pt.sample_lights(rows), pt.sample_lights_mis(rows) if mis else None, hits)
        if mis and power:
            out["w"] = pt.mis_hit_weight(hits)
        if mis and not power:
            out["pt0"] = pt
        else:
            pt.close()
    assert_bits(out[True][0], out[False][0], "one light: accumulated")
    assert_bits(out[True][1], out[False][1], "one light: wfpt_sample_lights")
    assert out[True][0].any() and (out[True][1][:, 4:7] != 0).any()
    if mis:
        assert_bits(out[True][2], out[False][2], "one light: wfpt_sample_lights_mis")
        w0 = out["pt0"].mis_hit_weight(out[True][3])
        out["pt0"].close()
        both_nan = np.isnan(w0) & np.isnan(out["w"])
        assert_bits(np.where(both_nan, F(0), out["w"]), np.where(both_nan, F(0), w0), "one light: wfpt_mis_hit_weight")


@pytest.mark.parametrize("mis", [False, True])
def test_no_emitter_is_the_unflagged_context_and_clear_makes_a_fresh_one(W, O, mis):
    w, h, spp = 100, 60, 8
    _, _, colours = shirley_scene(O)
    res = {}
    for power in (False, True):
        pt = W.shirley_path_tracer(w, h, max_wavefronts=5, flags=flags_of(W, "", mis, power))
        pt.render(spp)
        acc = pt.accumulated()
        _, launches = pt.render_timed(spp)
        res[power] = (acc, launches, pt.totals())
        if power:
            assert pt.nee_timing() == (0.0, 0) and pt.emission_timing() == (0.0, 0)
            with pytest.raises(W.WfptError) as e:
                pt.light_distribution()
            assert e.value.status == -1
            light(pt, colours)
            assert len(pt.light_distribution()[1]) == 3
            pt.render(spp)
            assert not np.array_equal(bits(pt.accumulated()), bits(acc))
            pt.clear_emission()
            with pytest.raises(W.WfptError):
                pt.light_distribution()
            pt.render(spp)
            assert_bits(pt.accumulated(), acc, "after set and clear")
        pt.close()
    assert_bits(res[True][0], res[False][0], "no emitter")
    assert np.array_equal(res[True][1], res[False][1]) and np.array_equal(res[True][2], res[False][2])


# ---------------------------------------------------------------- rebuilds
def test_rebuilds_follow_the_light_list(W, O):
    w, h, spp = W_, H_, 2
    tris, mt, nodes, cam, ip, vw = mesh_inputs(O, w, h)
    pt = mesh_tracer(W, w, h, max_wavefronts=MAXW, flags=flags_of(W, ""), max_window_size=128 * 80)
    light(pt, MESH_COLOURS)
    assert_tables(pt, P.PowerLights(E.Emission(MESH_COLOURS, triangles=tris, materials=mt)), "set_emission")
    two = {1: (2.0, 1.0, 0.5), 2: (0.125, 0.0, 4.0)}  # wfpt_set_emission again: a second material, another colour
    pt.set_emission(2, two[2])
    assert_tables(pt, P.PowerLights(E.Emission(two, triangles=tris, materials=mt)), "a second set_emission")
    small = W.Scene.random_mesh(3000, 1)  # wfpt_update_scene_mesh: the areas are the NEW scene's
    small.triangles["e1"] *= F(3.0)
    small.triangles["e2"] *= F(7.0)
    pt.update_scene(small)
    # (the rebuild reorders scene.triangles in place: they are now in the device's order)
    assert_tables(pt, P.PowerLights(E.Emission(two, triangles=small.triangles.copy(), materials=mt)), "update_scene")
    scene = W.Scene.random_mesh(5000, 1)
    scene.triangles["e1"] *= F(5.0)
    scene.triangles["e2"] *= F(5.0)
    pt.update_scene(scene)
    lights = P.PowerLights(E.Emission(two, triangles=tris, materials=mt))
    assert_tables(pt, lights, "a second update_scene")
    pt.render_parameters.set_viewport((120, 72))  # a resize keeps the tables
    pt.update_buffers()
    assert_tables(pt, lights, "after a resize")
    pt.render(spp)
    fresh = mesh_tracer(W, 120, 72, max_wavefronts=MAXW, flags=flags_of(W, ""))
    light(fresh, two)
    fresh.render(spp)
    assert_bits(pt.accumulated(), fresh.accumulated(), "after a resize")
    fresh.close()
    pt.close()


def test_a_light_of_non_finite_area_drops_the_distribution(W, O):
    """One of the dim lights is a sphere of radius 2e19 far below the ground: ra ra overflows, its area is infinite, M is not finite."""
    w, h, spp = W_, H_, 2
    inputs = P.indicator_inputs(O, w, h, n_dim=5, giant=True)
    acc = {}
    for power in (False, True):
        pt = G.lamp_tracer(W, inputs, w, h, max_wavefronts=3, miss_floor=0, flags=flags_of(W, "", False, power))
        light(pt, P.INDICATOR_COLOURS)
        assert pt.nee_light_count() == 6
        if power:
            with pytest.raises(W.WfptError) as e:
                pt.light_distribution()
            assert e.value.status == -1
        pt.render(spp)
        acc[power] = pt.accumulated()
        pt.close()
    both_nan = np.isnan(acc[True]) & np.isnan(acc[False])
    assert_bits(np.where(both_nan, F(0), acc[True]), np.where(both_nan, F(0), acc[False]), "no distribution: the unflagged render")


# ---------------------------------------------------------------- refusals
def test_refusals_leave_nothing_behind(W, O):
    w, h = 48, 32
    for flags in (W.FLAG_EMISSION | W.FLAG_LIGHT_POWER,  # without WFPT_FLAG_NEE
                  W.FLAG_LIGHT_POWER,
                  W.FLAG_EMISSION | W.FLAG_NEE | W.FLAG_ENVIRONMENT | W.FLAG_ENV_NEE | W.FLAG_LIGHT_POWER,
                  W.FLAG_EMISSION | W.FLAG_NEE | W.FLAG_ENVIRONMENT | W.FLAG_ENV_NEE | W.FLAG_ENV_MIS | W.FLAG_LIGHT_POWER):
        with pytest.raises(W.WfptError) as e:
            W.shirley_path_tracer(w, h, max_wavefronts=4, flags=flags)
        assert "WFPT_FLAG_LIGHT_POWER" in str(e.value)  # (PathTracer reports every failed wfpt_create* alike: the reason names the rule)
    _, _, colours = shirley_scene(O)
    plain = W.shirley_path_tracer(w, h, max_wavefronts=4, flags=flags_of(W, "", power=False))
    light(plain, colours)
    plain.render(2)
    want = plain.accumulated()
    with pytest.raises(W.WfptError) as e:  # without the flag
        plain.light_distribution()
    assert e.value.status == -1
    assert_bits(plain.accumulated(), want, "a refused call resets nothing")
    plain.render(2)
    fresh = W.shirley_path_tracer(w, h, max_wavefronts=4, flags=flags_of(W, "", power=False))
    light(fresh, colours)
    fresh.render(4)
    assert_bits(plain.accumulated(), fresh.accumulated(), "the context renders as before")
    fresh.close()
    plain.close()


# ---------------------------------------------------------------- the payoff
def test_selecting_by_power_lowers_the_variance_among_dim_lights(W, O):
    """One lamp of radius 0.5 at (16, 16, 16) and 63 spheres of radius 0.01 at (0.1, 0.1, 0.1) above the ground; 320 x 240, 64 spp,
    WFPT_RNG_PIXEL, miss_floor 0, a black environment, WFPT_FLAG_DENOISE. The sum of wfpt_read_variance over the ground pixels with the flag
    is below the unflagged context's; the two mean luminances over those pixels agree within 5 standard errors, from the two variance sums.
    The ratio is printed; DESIGN.md 9p records it."""
    w, h, spp = 320, 240, 64
    inputs = P.indicator_inputs(O, w, h)
    _, _, ok = closed_form(inputs, w, h, 0.5)  # the ground pixels clear of the lamp's image
    assert ok.sum() > 20000
    sums, means = {}, {}
    for name, power in (("uniform", False), ("power", True)):
        pt = G.lamp_tracer(W, inputs, w, h, max_wavefronts=4, miss_floor=0, rng_mode=W.RNG_PIXEL,
                           flags=flags_of(W, "", False, power) | W.FLAG_ENVIRONMENT | W.FLAG_DENOISE)
        pt.set_environment(N.black_env())
        light(pt, P.INDICATOR_COLOURS)
        assert pt.nee_light_count() == 64
        pt.render(spp)
        sums[name] = float(pt.variance().reshape(-1)[ok].astype(np.float64).sum())
        means[name] = float(R.luma(pt.accumulated())[ok].astype(np.float64).mean() / spp)
        print(f"{name}: variance sum over {int(ok.sum())} ground pixels {sums[name]:.6g}, mean luminance {means[name]:.6g}")
        pt.close()
    print(f"variance ratio power / uniform at {spp} spp: {sums['power'] / sums['uniform']:.4g}")
    assert sums["power"] < sums["uniform"]
    # wfpt_read_variance is the variance of each pixel's mean; the pixels' streams are independent
    se = np.sqrt(sums["power"] + sums["uniform"]) / ok.sum()
    print(f"means differ by {(means['power'] - means['uniform']) / se:.2f} standard errors")
    assert abs(means["power"] - means["uniform"]) <= 5.0 * se
