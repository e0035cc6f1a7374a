"""The fused bounce launches read their argument block inside the work-item loop, field by field where an item uses it (bounce_args_here,
csrc/wfpt_kernels.hip). A field read at the wrong offset, a stride applied to the wrong sample or a pointer
taken for the wrong queue shows in the image, the totals or the per-bounce table, so every case here is compared bit for bit with the
oracle (tests/helpers.py builds both sides; the flagged contexts go through the restatements the flags' own tests use). The shapes are the
smallest at which each argument matters:

  frames    64x64 and 128x72 of the five-sphere scene (also against the committed goldens simple_*), Shirley 400x225: a true-size frame
            with a partial tile row (225 = 28 * 8 + 1), 182 work items of the first launch
  batching  8 samples in batches of 1, 3 and 8: the batch strides of every queue, and a remainder batch (8 = 3 + 3 + 2)
  RNG       both modes (rng_mode, shade_gx, the frame counters)
  flags     0, RETIRE, ADAPTIVE, ENVIRONMENT with a small map, and RETIRE / ADAPTIVE together with ENVIRONMENT: every MODE and ENV
            instantiation of bounce_kernel (`term`, `mask`, the five-plane miss queue)
  sharding  two band shards (tile_world = 2): `tile` and `image_width` in local_pixel and tile_pixel
  capacity  a context whose ray capacity is not its slot count (max_window_size above the frame, as tests/test_gpu_capacity.py makes them;
            a viewport with more slots than the capacity is refused at wfpt_update_render_parameters, so "different" is the case that exists)
"""
import os

import numpy as np
import pytest

import capacity_ref as R
from conftest import assert_bit_equal
from helpers import inputs_for, make_oracle, make_tracer

pytestmark = pytest.mark.gpu

SPP, MW = 8, 4
FRAMES = [("simple", 64, 64), ("simple", 128, 72), ("shirley", 400, 225)]
_oracles = {}


def oracle_result(orc, kind, w, h, rng_mode):
    """(accumulated, totals, last sample's bounce table) of SPP samples, once per frame and RNG mode"""
    key = (kind, w, h, rng_mode)
    if key not in _oracles:
        o = make_oracle(orc, inputs_for(orc, kind, w, h), w, h, rng_mode=rng_mode, max_wavefronts=MW)
        o.render(SPP)
        _oracles[key] = (o.accumulated().copy(), o.totals().copy(), o.bounce_table().copy())
        o.close()
    return _oracles[key]


def assert_same(pt, want, what):
    assert_bit_equal(pt.accumulated(), want[0], what + ": accumulated image")
    assert np.array_equal(pt.totals(), want[1]), f"{what}: totals {pt.totals()} vs {want[1]}"
    assert np.array_equal(pt.bounce_table(), want[2]), f"{what}: bounce table\n{pt.bounce_table()}\nvs\n{want[2]}"


@pytest.mark.parametrize("batch", [1, 3, 8])
@pytest.mark.parametrize("rng_mode", [0, 1])
@pytest.mark.parametrize("kind,w,h", FRAMES)
def test_frames_modes_and_batches(gpu, orc, kind, w, h, rng_mode, batch):
    W = gpu
    pt = make_tracer(W, kind, w, h, rng_mode=rng_mode, max_wavefronts=MW, batch=batch)
    assert pt.loop_kind == "fused"
    pt.render(SPP)
    assert_same(pt, oracle_result(orc, kind, w, h, rng_mode), f"{kind} {w}x{h} rng {rng_mode} batch {batch}")
    pt.close()


@pytest.mark.parametrize("rng_mode", [0, 1])
@pytest.mark.parametrize("w,h", [(64, 64), (128, 72)])
def test_goldens(gpu, w, h, rng_mode):
    """the committed dumps of the five-sphere scene: 4 samples, 4 wavefronts, here in batches of 3 + 1"""
    W = gpu
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"simple_{w}x{h}_mode{rng_mode}.npz"))
    pt = make_tracer(W, "simple", w, h, max_wavefronts=4, rng_mode=rng_mode, batch=3)
    pt.render(4)
    assert_bit_equal(pt.accumulated(), g["acc"], f"golden {w}x{h} mode {rng_mode}")
    pt.close()


def test_two_band_shards(gpu, orc):
    from wavefront_path_tracer_amd import tiles
    W = gpu
    kind, w, h = FRAMES[2]
    slabs = []
    for rank in range(2):
        pt = make_tracer(W, kind, w, h, max_wavefronts=MW, rng_mode=W.RNG_PIXEL, tile_rank=rank, tile_world=2, batch=3)
        assert pt.loop_kind == "fused"
        pt.render(SPP)
        slabs.append(pt.accumulated())
        pt.close()
    assert_bit_equal(tiles.assemble(slabs, w, h), oracle_result(orc, kind, w, h, W.RNG_PIXEL)[0], "assembled from two band shards")


@pytest.mark.parametrize("rng_mode", [0, 1])
def test_capacity_above_the_slot_count(gpu, orc, rng_mode):
    W = gpu
    kind, w, h = FRAMES[2]
    pt = make_tracer(W, kind, w, h, max_wavefronts=MW, rng_mode=rng_mode, batch=3, max_window_size=200000)
    slots = ((w + 7) // 8) * ((h + 7) // 8) * 64
    cap = R.capacity_rule(w, h, max_pixels=200000, batch=3, rng_mode=rng_mode)
    assert 6 * slots < pt.ray_capacity == cap.capacity, (slots, pt.ray_capacity, cap.capacity)  # (the first launch stops at its slots, far below the capacity)
    pt.render(SPP)
    assert_same(pt, oracle_result(orc, kind, w, h, rng_mode), f"capacity {pt.ray_capacity} for {slots} slots, rng {rng_mode}")
    pt.close()


# ---------------------------------------------------------------- the flags: through the restatements their own tests use
@pytest.mark.parametrize("rng_mode", [0, 1])
@pytest.mark.parametrize("case", ["alone", "env"])
def test_retire(gpu, orc, case, rng_mode):
    """WFPT_FLAG_RETIRE: bounce_kernel<kBounceMiddleRetire> (`term`), alone and over an environment map (ENV); 3 samples in batches of 2."""
    import test_gpu_retire as TR
    from test_gpu_nee import compare
    W = gpu
    params = TR.CASES[case][1][0]
    r, table, retired = TR.reference(orc, case, rng_mode, params)
    assert sum(map(sum, retired)) > 0
    pt = TR.tracer(W, orc, case, "", rng_mode, params)
    assert pt.loop_kind == "fused"
    pt.render(TR.SPP)
    compare(pt, r, TR.SPP, TR.W_, TR.H_, f"retire {case} rng {rng_mode}")
    assert np.array_equal(pt.bounce_table(), table)
    pt.close()


@pytest.mark.parametrize("rng_mode", [0, 1])
@pytest.mark.parametrize("case", ["alone", "env"])
def test_adaptive(gpu, orc, case, rng_mode):
    """WFPT_FLAG_ADAPTIVE under a checkerboard mask: bounce_kernel<kBounceFirstMasked> (`mask`), alone and over an environment map."""
    import test_gpu_adaptive as TA
    W = gpu
    ref = TA.Ref(orc, case, rng_mode).render(TA.hand_mask("checker"))
    pt = TA.tracer(W, orc, case, "", rng_mode)
    assert pt.loop_kind == "fused"
    pt.set_active_mask(TA.hand_mask("checker"))
    pt.render(TA.SPP)
    TA.check(pt, ref, f"adaptive {case} rng {rng_mode}")
    pt.close()


@pytest.mark.parametrize("rng_mode", [0, 1])
def test_environment_with_a_small_map(gpu, orc, rng_mode):
    """WFPT_FLAG_ENVIRONMENT with an 8x4 map: the ENV instantiations of the first and middle launches (dx and dz planes of the miss queue)."""
    import environment_ref as ER
    from test_gpu_environment import assert_bits, make_map
    W = gpu
    w, h = 64, 64
    m, params = make_map(8, 4), {"intensity": 1.5, "rotation": 0.3}
    pt = W.shirley_path_tracer(w, h, max_wavefronts=MW, rng_mode=rng_mode, flags=W.FLAG_ENVIRONMENT, batch=3)
    pt.set_environment(m, **params)
    pt.render(SPP)
    o = orc.shirley_oracle(w, h, max_wavefronts=MW, rng_mode=rng_mode)
    assert_bits(pt.accumulated(), ER.render_with_environment(o, m, params, spp=SPP), f"environment rng {rng_mode}")
    o.close()
    pt.close()
