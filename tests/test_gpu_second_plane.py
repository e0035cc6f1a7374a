"""The second per-sample plane (`emitted`) and its companion of hit points (`mis_origin`) come with whichever of a context's features
needs them first -- an emitter, a map with a sampling distribution, an analytic light -- and stay. Whoever brings them, the context
must be the same one: the same accumulated bits, the same answers of the MIS probes (which read the hit-point plane's existence), in
either order of first use, and again after everything was cleared and set anew.

The lamp scene of tests/test_gpu_nee.py (a ground sphere under a small emitting one), 16 x 16, three wavefronts, two samples in flight."""
import numpy as np
import pytest

from nee_ref import LAMP, lamp_inputs

pytestmark = pytest.mark.gpu

F = np.float32
SIZE, SPP, ROWS = 16, 2, 64


@pytest.fixture(scope="module")
def W(gpu):
    return gpu


def tracer(W, orc, flags):
    inputs = lamp_inputs(orc, SIZE, SIZE)
    cc = W.CameraController(W.Camera((0.0, 6.0, 8.0), (0.0, 0.0, 0.0)), 40.0, 0.0, 10.0, 0.1, 100.0)
    scn = W.Scene(inputs[0].view(W.SPHERE).copy(), inputs[1].view(W.MATERIAL))
    return W.PathTracer(scn, W.RenderParameters(cc, (SIZE, SIZE)), max_wavefronts=3, batch=2, miss_floor=0, flags=flags)


def receiver_rows(width, seed):
    """Receivers a little above the ground, normals up, draws in [0, 1)."""
    rng = np.random.default_rng(seed)
    rows = rng.random((ROWS, width)).astype(F)
    rows[:, :3] = (rows[:, :3] - F(0.5)) * F(4.0)
    rows[:, 1] = F(0.01)
    rows[:, 3:6] = (0.0, 1.0, 0.0)
    return rows


def env_kind(W):
    env = (np.random.default_rng(3).random((2, 4, 3)) + 0.25).astype(F)  # a lit 4 x 2 map
    dirs = np.random.default_rng(4).standard_normal((ROWS, 3)).astype(F)
    return (W.FLAG_ENVIRONMENT | W.FLAG_EMISSION | W.FLAG_NEE | W.FLAG_ENV_NEE | W.FLAG_ENV_MIS,
            lambda pt: pt.set_environment(env), lambda pt: pt.clear_environment(),
            lambda pt: (pt.sample_environment_light_mis(receiver_rows(10, 5)), pt.env_mis_miss_weight(dirs)))


def lights_kind(W):
    point = np.zeros(1, W.LIGHT)
    point["position"], point["type"], point["colour"] = (1.0, 3.0, 1.0), W.LIGHT_POINT, (6.0, 5.0, 4.0)
    rng = np.random.default_rng(6)
    hits = np.concatenate([rng.standard_normal((ROWS, 6)) * 3, rng.random((ROWS, 1)) * 4, rng.integers(0, 2, (ROWS, 1))], 1).astype(F)
    return (W.FLAG_EMISSION | W.FLAG_NEE | W.FLAG_MIS | W.FLAG_ANALYTIC_LIGHTS,
            lambda pt: pt.set_lights(point), lambda pt: pt.set_lights(None),
            lambda pt: (pt.sample_lights_mis(receiver_rows(9, 7)), pt.mis_hit_weight(hits)))


def same_bits(got, want, what):
    g, w = np.ascontiguousarray(got, F).view(np.uint32), np.ascontiguousarray(want, F).view(np.uint32)
    assert g.shape == w.shape and np.array_equal(g, w), f"{what}: {int((g != w).sum())} of {g.size} values differ"


@pytest.mark.parametrize("loop", ["", "UNFUSED", "NO_LDS_SCENE"])
@pytest.mark.parametrize("kind", [env_kind, lights_kind])
def test_the_order_of_first_use_does_not_matter(W, orc, kind, loop):
    flags, set_other, clear_other, probes = kind(W)
    for name in loop.split("|") if loop else []:
        flags |= getattr(W, "FLAG_" + name)
    emit = lambda pt: pt.set_emission(1, LAMP["e"])
    a, b = tracer(W, orc, flags), tracer(W, orc, flags)
    emit(a), set_other(a)
    set_other(b), emit(b)
    a.render(SPP), b.render(SPP)
    acc = a.accumulated()
    assert acc.any() and np.isfinite(acc).all()
    same_bits(b.accumulated(), acc, "accumulated, the emitter first against the emitter last")
    pa, pb = probes(a), probes(b)
    for k, what in enumerate(("the light sampler", "the scatter's weight")):
        assert pa[k].shape[0] == ROWS and np.isfinite(pa[k]).any()
        same_bits(pb[k], pa[k], what)
    # everything cleared and set again, in the other order: the context a fresh one would be
    a.clear_emission(), clear_other(a)
    a.render(SPP)
    assert not np.array_equal(a.accumulated(), acc), "clearing the lights changes nothing"
    set_other(a), emit(a)
    a.render(SPP)
    same_bits(a.accumulated(), acc, "accumulated after clearing and setting again")
    again = probes(a)
    for k in range(2):
        same_bits(again[k], pa[k], "the probes after clearing and setting again")
    a.close(), b.close()
