"""Path termination (WFPT_FLAG_RETIRE, include/wfpt.h "Path termination") on the GPU.

Whole renders are compared bit for bit with tests/retire_ref.py: the restatement of the context's other flags (emission_ref, mis_ref,
env_mis_ref) driven over an oracle wrapped in retire_ref.Retiring. A restatement render depends on the scene, the size, the RNG mode and
the parameters alone -- not on the loop or the batch -- so each is computed once and shared among the loops. Every test renders
max_wavefronts = 6 and 3 spp at batch = 2: a batch boundary is crossed, and wfpt_read_bounce_table gives the third sample's table."""
import numpy as np
import pytest

import emission_ref as E
import env_mis_ref as X
import env_nee_ref as V
import mis_ref as M
import retire_ref as RR
from emission_ref import COLOUR, furnace_inputs
from helpers import make_oracle
from test_gpu_env_nee import ENV_PARAMS, LAMP_E, env_light, ground_tracer
from test_gpu_nee import assert_bits, bits, compare, light, mesh_inputs, mesh_tracer, shirley_scene, sphere_tracer
from test_retire_host import hand_rows

pytestmark = pytest.mark.gpu

F = np.float32
SPP, BATCH, WAVEFRONTS = 3, 2, 6
W_, H_ = 69, 43  # no multiple of 8: padding rays and retired rays share the queues; 2967 pixels = five 512-hit segments and a partial one
NO = RR.NO_ROULETTE
LOOPS = ["", "UNFUSED", "SPLIT_SHADE", "NO_GRAPH", "NO_LDS_SCENE", "NO_LDS_SCENE|NO_REFILL", "NO_LDS_SCENE|BINARY_BVH"]
LOOP_KIND = {"": "fused", "UNFUSED": "stages", "SPLIT_SHADE": "stages", "NO_GRAPH": "fused", "NO_LDS_SCENE": "refill",
             "NO_LDS_SCENE|NO_REFILL": "fused", "NO_LDS_SCENE|BINARY_BVH": "fused"}


@pytest.fixture(scope="module")
def W(gpu):
    return gpu


@pytest.fixture(scope="module")
def O(orc):
    return orc


def flags_of(W, *names):
    f = W.FLAG_RETIRE
    for group in names:
        for n in (group.split("|") if group else []):
            f |= getattr(W, "FLAG_" + n)
    return f


# ---------------------------------------------------------------- the cases: other flags x termination parameters
# name -> (the context's other flags, (roulette_start, q_min) settings)
CASES = {
    "alone": ("", [(0, 0.25), (3, 0.05)]),
    "emission": ("EMISSION", [(NO, 0.05), (1, 0.25)]),
    "mis": ("EMISSION|NEE|MIS|DENOISE", [(1, 0.25), (0, 1.0)]),
    "env": ("ENVIRONMENT|EMISSION|NEE|ENV_NEE|ENV_MIS", [(1, 0.25)]),
}
_refs = {}


def wrapped(o, params):
    return RR.Retiring(o, roulette_start=params[0], q_min=params[1])


def reference(O, case, rng, params):
    """(the restatement's render, the third sample's bounce table, hits retired per sample and wavefront), once per (case, RNG mode,
    parameters)"""
    key = (case, rng, params)
    if key not in _refs:
        if case == "env":
            inputs = V.ground_inputs(O, W_, H_, occluder=True, mirror=True, lamp=True)
            em = E.Emission({1: LAMP_E}, spheres=inputs[0], materials=inputs[1])
            o = wrapped(make_oracle(O, inputs, W_, H_, max_wavefronts=WAVEFRONTS, miss_floor=0, rng_mode=rng), params)
            r = X.render_with_env_mis(o, make_oracle(O, inputs, W_, H_), em, env_light(V.sun_map()), spp=SPP, parts=True, termination=o)
        else:
            sp, mt, colours = shirley_scene(O)
            em = E.Emission(colours if case != "alone" else {}, spheres=sp, materials=mt)
            o = wrapped(O.shirley_oracle(W_, H_, max_wavefronts=WAVEFRONTS, rng_mode=rng), params)
            if case == "mis":
                r = M.render_with_mis(o, O.shirley_oracle(W_, H_), em, spp=SPP, parts=True, termination=o)
            else:
                r = E.render_with_emission(o, em, spp=SPP, parts=True, termination=o)
        _refs[key] = (r, o.bounce_table(), o.retired)
    return _refs[key]


def tracer(W, O, case, loop, rng, params, **kw):
    flags = flags_of(W, CASES[case][0], loop)
    if case == "env":
        inputs = V.ground_inputs(O, W_, H_, occluder=True, mirror=True, lamp=True)
        pt = ground_tracer(W, inputs, W_, H_, max_wavefronts=WAVEFRONTS, miss_floor=0, rng_mode=rng, flags=flags, batch=BATCH, **kw)
        pt.set_environment(V.sun_map(), **ENV_PARAMS)
        pt.set_emission(1, LAMP_E)
    else:
        pt = W.shirley_path_tracer(W_, H_, max_wavefronts=WAVEFRONTS, rng_mode=rng, flags=flags, batch=BATCH, **kw)
        if case != "alone":
            light(pt, shirley_scene(O)[2])
    pt.set_termination(*params)
    return pt


@pytest.mark.parametrize("rng", [0, 1])
@pytest.mark.parametrize("loop", LOOPS)
def test_spheres_equal_restatement(W, O, loop, rng):
    for case, (_, settings) in CASES.items():
        for params in settings:
            r, table, retired = reference(O, case, rng, params)
            assert sum(map(sum, retired)) > 0, (case, params, "the restatement retires nothing")
            pt = tracer(W, O, case, loop, rng, params)
            assert pt.loop_kind == LOOP_KIND[loop] and pt.termination() == (params[0], float(F(params[1])))
            pt.render(SPP)
            what = f"{case} {params} {loop} rng {rng}"
            compare(pt, r, SPP, W_, H_, what)
            assert np.array_equal(pt.bounce_table(), table), f"{what}: bounce table\n{pt.bounce_table()}\nvs\n{table}"
            pt.close()


def test_cases_retire_dead_paths_and_play_roulette(O):
    """What the parity above rests on: the references retire dead hits where a material emits, roulette retires hits in later wavefronts,
    survivors are re-weighted (the image differs from the unflagged restatement's), and padding and retired rays meet in one queue."""
    r, table, retired = reference(O, "emission", 1, (NO, 0.05))
    t = table.astype(np.int64)
    assert retired[0][0] > 0 and (t[:, 1] + t[:, 2] < t[:, 0]).any()
    assert t[0, 0] > W_ * H_ and t[0, 1] + t[0, 2] == W_ * H_, "padding rays"
    sp, mt, colours = shirley_scene(O)
    plain = E.render_with_emission(O.shirley_oracle(W_, H_, max_wavefronts=WAVEFRONTS, rng_mode=1), E.Emission(colours, spheres=sp, materials=mt),
                                   spp=SPP, parts=True)
    r2, _, retired2 = reference(O, "emission", 1, (1, 0.25))
    assert sum(retired2[0][1:]) > sum(retired[0][1:]), "roulette retires more"
    assert not np.array_equal(bits(r2["acc"]), bits(plain["acc"])), "no survivor was re-weighted"


MESH_LOOPS = ["", "UNFUSED", "NO_LDS_SCENE", "NO_LDS_SCENE|NO_REFILL", "NO_LDS_SCENE|BINARY_BVH"]
_mesh = {}


def mesh_reference(O, rng):
    if rng not in _mesh:
        w, h = 96, 64
        tris, mt, nodes, cam, ip, vw = mesh_inputs(O, w, h)
        o = wrapped(O.Oracle(w, h, np.zeros(1, O.SPHERE), mt, nodes, cam, ip, vw, triangles=tris, max_wavefronts=WAVEFRONTS, rng_mode=rng,
                             miss_floor=16), (1, 0.25))
        r = E.render_with_emission(o, E.Emission({1: (2.0, 1.0, 0.5)}, triangles=tris, materials=mt), spp=SPP, parts=True, termination=o)
        _mesh[rng] = (r, o.bounce_table(), o.retired)
    return _mesh[rng]


@pytest.mark.parametrize("rng", [0, 1])
@pytest.mark.parametrize("loop", MESH_LOOPS)
def test_mesh_equals_restatement(W, O, loop, rng):
    """The 5 000-triangle mesh with one emitting material: the triangle forms of every loop, the four-wide and binary walks, refill on and off."""
    w, h = 96, 64
    r, table, retired = mesh_reference(O, rng)
    assert retired[-1][0] > 0 and sum(retired[-1][1:]) > 0
    pt = mesh_tracer(W, w, h, max_wavefronts=WAVEFRONTS, miss_floor=16, rng_mode=rng, flags=flags_of(W, "EMISSION|DENOISE", loop), batch=BATCH)
    pt.set_emission(1, (2.0, 1.0, 0.5))
    pt.set_termination(1, 0.25)
    pt.render(SPP)
    compare(pt, r, SPP, w, h, f"mesh {loop} rng {rng}")
    assert np.array_equal(pt.bounce_table(), table), f"mesh {loop}: bounce table\n{pt.bounce_table()}\nvs\n{table}"
    pt.close()


# ---------------------------------------------------------------- the furnace: the whole wavefront retires at b = 0
FURNACE_LOOPS = ["", "UNFUSED", "NO_LDS_SCENE"]


@pytest.mark.parametrize("loop", FURNACE_LOOPS)
def test_furnace_retires_the_whole_wavefront(W, O, loop):
    """The camera inside one closed emitting sphere, miss_floor = 0: every primary ray hits the emitter, every hit is retired."""
    w, h = W_, H_
    inputs = furnace_inputs(O, w, h)
    e = np.asarray(COLOUR, F)
    pt = sphere_tracer(W, inputs, (0.0, 0.0, 0.0), (0.5, 0.0, -1.0), 70.0, w, h, max_wavefronts=WAVEFRONTS, miss_floor=0,
                       flags=flags_of(W, "EMISSION", loop), batch=BATCH)
    pt.set_emission(0, COLOUR)
    pt.render(SPP)
    assert_bits(pt.accumulated(), np.broadcast_to(F(SPP) * e, (w * h, 3)), f"furnace {loop}: every sample is e")
    assert not pt.image().any(), "the paths are dead"
    t = pt.bounce_table().astype(np.int64)
    assert t[0, 1] == w * h and t[0, 2] == 0, t
    assert len(t) >= 2 and not t[1:, 1:3].any(), f"rows 1 and up have neither hits nor misses\n{t}"
    assert t[1, 0] == w * h, "the retired hits still occupy their slots"
    pt.close()


_open_furnace = {}


@pytest.mark.parametrize("loop", FURNACE_LOOPS)
def test_open_furnace_leaves_the_loop_at_row_one(W, O, loop):
    """Shirley's scene with every material emitting, miss_floor = 128 (a closed furnace has no miss: its loop ends at row 0, before any
    shade, flagged or not): the primary misses keep the loop going past row 0, every hit is an emitter and is retired at b = 0, row 1
    holds the slots and neither a hit nor a miss, and the loop exits there. Every sample of a pixel whose primary ray hits is exactly e."""
    w, h = W_, H_
    sp, mt = O.scene_book_one_final(1)
    sp, _ = O.build_bvh(sp)
    e = np.asarray(COLOUR, F)
    if not _open_furnace:
        o = wrapped(O.shirley_oracle(w, h, max_wavefronts=WAVEFRONTS, miss_floor=128), (NO, 0.05))
        r = E.render_with_emission(o, E.Emission({m: COLOUR for m in range(len(mt))}, spheres=sp, materials=mt), spp=SPP, parts=True,
                                   termination=o)
        _open_furnace.update(r=r, table=o.bounce_table())
    r, table = _open_furnace["r"], _open_furnace["table"]
    for k in range(SPP):
        hit = r["first_prim"][k] >= 0
        assert hit.sum() > 128 and (~hit).sum() > 128
        assert_bits((r["image"][k] + r["emitted"][k])[hit], np.broadcast_to(e, (int(hit.sum()), 3)), f"sample {k}: a hit pixel is not e")
    t = table.astype(np.int64)
    assert len(t) == 2 and t[1, 0] == t[0, 1] > 0 and not t[1, 1:].any(), f"the loop exits at row 1 with nothing traced\n{t}"
    pt = W.shirley_path_tracer(w, h, max_wavefronts=WAVEFRONTS, miss_floor=128, flags=flags_of(W, "EMISSION", loop), batch=BATCH)
    for m in range(len(mt)):
        pt.set_emission(m, COLOUR)
    pt.set_termination(NO, 0.05)
    pt.render(SPP)
    compare(pt, r, SPP, w, h, f"open furnace {loop}")
    assert np.array_equal(pt.bounce_table(), table), f"open furnace {loop}: bounce table\n{pt.bounce_table()}\nvs\n{table}"
    # the unflagged context traces the dead paths on: its row 1 has hits and misses
    plain = W.shirley_path_tracer(w, h, max_wavefronts=WAVEFRONTS, miss_floor=128, flags=flags_of(W, "EMISSION", loop) & ~W.FLAG_RETIRE, batch=BATCH)
    for m in range(len(mt)):
        plain.set_emission(m, COLOUR)
    plain.render(SPP)
    u = plain.bounce_table().astype(np.int64)
    assert len(u) > 2 and u[1, 1] + u[1, 2] == u[1, 0] > 0, u
    assert_bits(plain.accumulated(), pt.accumulated(), f"open furnace {loop}: the dead paths added nothing")
    plain.close()
    pt.close()


# ---------------------------------------------------------------- roulette off: the same frame with fewer rays
@pytest.mark.parametrize("loop", LOOPS)
def test_roulette_off_equals_the_unflagged_frame(W, O, loop):
    _, _, colours = shirley_scene(O)
    got = {}
    for flagged in (False, True):
        f = flags_of(W, "EMISSION|NEE", loop) & ~(0 if flagged else W.FLAG_RETIRE)
        pt = W.shirley_path_tracer(W_, H_, max_wavefronts=WAVEFRONTS, miss_floor=0, rng_mode=W.RNG_PIXEL, flags=f, batch=BATCH)
        light(pt, colours)
        if flagged:
            pt.set_termination(NO, 0.05)
        pt.render(SPP)
        got[flagged] = (pt.accumulated(), pt.image(), pt.totals(), pt.bounce_table().astype(np.int64))
        pt.close()
    assert_bits(got[True][0], got[False][0], f"{loop}: accumulated")
    assert_bits(got[True][1], got[False][1], f"{loop}: read_image")
    # totals[0] counts the rays extend traced, hits + misses: the retired slots are not in it
    assert got[True][2][0] < got[False][2][0], f"{loop}: no ray was saved: {got[True][2]} vs {got[False][2]}"
    t = got[True][3]
    assert (t[:, 1] + t[:, 2] < t[:, 0]).any() and (t[1:, 0] == t[:-1, 1]).all()
    u = got[False][3]
    assert (u[1:, 1] + u[1:, 2] == u[1:, 0]).all(), "an unflagged context retires nothing"


# ---------------------------------------------------------------- the sampler
def test_sampler_equals_the_restatement(W, O):
    t, pix = hand_rows()
    rng = np.random.default_rng(11)
    k = 4000
    rnd = rng.random((k, 3)).astype(F) * rng.choice(np.asarray([0.05, 0.3, 1.0, 1.5], F), (k, 1))
    rnd[rng.random(k) < 0.1] = 0
    rnd[rng.random(k) < 0.02, 1] = np.nan
    thr = np.concatenate([t, rnd])
    pixels = np.concatenate([pix, rng.integers(0, 2 ** 32, k, dtype=np.uint64).astype(np.uint32)])
    pt = W.shirley_path_tracer(64, 48, max_wavefronts=2, flags=flags_of(W))
    seen = set()
    for params, frame, b in (((3, 0.05), 1, 2), ((3, 0.05), 1, 3), ((0, 0.25), 7, 0), ((1, 1.0), 2 ** 32 - 1, 63), ((NO, 0.25), 3, 5),
                             ((2, 0.25), 5, 2 ** 32 - 1)):
        pt.set_termination(*params)
        got = pt.sample_termination(thr, pixels, frame, b)
        want = RR.sample_rows(thr, pixels, frame, b, *params)
        assert got.shape == (len(thr), 8)
        assert_bits(got, want, f"sampler {params} frame {frame} b {b}")
        seen |= set(got[:, 2])
    assert seen == {0.0, 1.0, 2.0}
    assert pt.sample_termination(np.zeros((0, 3), F), np.zeros(0, np.uint32), 1, 0).shape == (0, 8)
    pt.close()


# ---------------------------------------------------------------- the stage API
@pytest.mark.parametrize("three", [False, True])
def test_stage_api_equals_render(W, O, three):
    """The host-driven stage loop with one shade stage and with the three per-material ones, against render()."""
    w, h = 72, 40
    _, _, colours = shirley_scene(O)

    class ThreeStages:
        def __init__(self, pt):
            self.stages = [W.Kernel(name, pt) for name in ("shade_metal", "shade_lambertian", "shade_dielectric")]

        def run(self, size):
            for k in self.stages:
                k.run(size)

    for rng in (0, 1):
        def make():
            pt = W.shirley_path_tracer(w, h, max_wavefronts=5, miss_floor=0, rng_mode=rng, flags=flags_of(W, "EMISSION|NEE"))
            light(pt, colours)
            pt.set_termination(1, 0.25)
            return pt
        pt = make()
        if three:
            pt.shade_kernel = ThreeStages(pt)
        for _ in range(3):
            pt.run()
        host = pt.accumulated()
        pt.close()
        pt = make()
        pt.render(3)
        assert_bits(host, pt.accumulated(), f"stage API, three stages {three}, rng {rng}")
        t = pt.bounce_table().astype(np.int64)
        assert (t[:, 1] + t[:, 2] < t[:, 0]).any()
        pt.close()


# ---------------------------------------------------------------- parameters
def test_refusals_leave_the_context_as_it_was(W, O):
    with pytest.raises(W.WfptError):
        W.shirley_path_tracer(64, 48, rng_mode=W.RNG_PIXEL, flags=W.FLAG_RETIRE | W.FLAG_BINNING)
    # without the flag
    pt = W.shirley_path_tracer(64, 48, max_wavefronts=3)
    for call in (lambda: pt.set_termination(3, 0.05), pt.termination, lambda: pt.sample_termination(np.ones((1, 3), F), [0], 1, 0)):
        with pytest.raises(W.WfptError):
            call()
    pt.close()
    # bad parameters
    pt = W.shirley_path_tracer(64, 48, max_wavefronts=4, flags=flags_of(W), batch=BATCH)
    assert pt.termination() == (3, float(F(0.05))) and pt.loop_kind == "fused"
    pt.set_termination(1, 0.25)
    pt.render(SPP)
    before = pt.accumulated()
    n = W.lib().wfpt_accumulated_samples(pt.handle)
    assert n == SPP
    for q in (0.0, -0.25, 1.5, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(W.WfptError):
            pt.set_termination(1, q)
    p = W._TerminationParams(1, 0.5)
    p._reserved[3] = 1
    assert W.lib().wfpt_set_termination(pt.handle, W.C.byref(p)) == -1
    assert W.lib().wfpt_set_termination(pt.handle, None) == -1 and W.lib().wfpt_get_termination(pt.handle, None) == -1
    assert W.lib().wfpt_sample_termination(pt.handle, None, None, 1, 0, 4, None) == -1
    assert pt.termination() == (1, 0.25) and W.lib().wfpt_accumulated_samples(pt.handle) == n
    assert_bits(pt.accumulated(), before, "a refused call touched the accumulation")
    pt.render(1)  # ... and goes on from where it was
    fresh = W.shirley_path_tracer(64, 48, max_wavefronts=4, flags=flags_of(W), batch=BATCH)
    fresh.set_termination(1, 0.25)
    fresh.render(SPP + 1)
    assert_bits(pt.accumulated(), fresh.accumulated(), "after the refused calls")
    fresh.close()
    pt.close()


@pytest.mark.parametrize("loop", ["", "NO_GRAPH", "UNFUSED"])
def test_a_parameter_change_restarts_the_accumulation(W, O, loop):
    pt = W.shirley_path_tracer(W_, H_, max_wavefronts=WAVEFRONTS, miss_floor=0, flags=flags_of(W, loop), batch=BATCH)
    pt.render(SPP)  # (the captured graphs hold the defaults)
    first = pt.accumulated()
    pt.set_termination(0, 0.5)
    assert W.lib().wfpt_accumulated_samples(pt.handle) == 0 and not pt.accumulated().any()
    pt.render(SPP)
    fresh = W.shirley_path_tracer(W_, H_, max_wavefronts=WAVEFRONTS, miss_floor=0, flags=flags_of(W, loop), batch=BATCH)
    fresh.set_termination(0, 0.5)
    fresh.render(SPP)
    assert_bits(pt.accumulated(), fresh.accumulated(), f"{loop}: after the change")
    assert not np.array_equal(bits(first), bits(fresh.accumulated())), "the parameters change nothing"
    fresh.close()
    pt.close()
