"""The first fused launch's hand-out of its work items (csrc/wfpt_first_schedule.h) on the device: whichever
workgroup runs an item, by its index or by a ticket, image and bounce table equal the oracle's bit for bit. The shapes are the smallest
that take each branch of the rule on a grid of 1024 workgroups:
  * 64x64, 1 sample: 8 items, fewer than the workgroups -- no static round, most workgroups leave at once;
  * 400x225 (182 items per sample, partial tiles on the right and bottom edge), 16 samples in flight, 20 samples: a launch of 2912 items
    (static rounds, then the tail by ticket) and one of 728 items (fewer than the grid);
  * rank 1 of 3 of the band-sharded frame: another tiles_y_local, 64 items per sample;
and the arms that share the kernel: the lists, WFPT_FLAG_NO_TILE_LISTS, WFPT_FLAG_EXACT_TRAVERSAL, WFPT_FLAG_NO_LDS_SCENE, a context with
an environment map, and the batch after a camera change (which walks) followed by one that tests the lists."""
import numpy as np
import pytest

import environment_ref as R
from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu

W_, H_, BATCH, SPP, BOUNCES = 400, 225, 16, 20, 4
MOVED = ((9.0, 3.0, -5.0), (0.0, 0.5, 0.0), 25.0, 0.4, 9.0)


@pytest.fixture(scope="module")
def oracle_renders(orc):
    """(accumulated, bounce table) of the book scene, computed once per (size, samples, RNG mode, rank, world)."""
    cache = {}

    def get(w, h, spp, mode, rank=0, world=1):
        key = (w, h, spp, mode, rank, world)
        if key not in cache:
            o = orc.shirley_oracle(w, h, max_wavefronts=BOUNCES, rng_mode=mode, tile_rank=rank, tile_world=world)
            acc = o.render(spp)
            acc.setflags(write=False)
            cache[key] = (acc, o.bounce_table())
            o.close()
        return cache[key]
    return get


def check(pt, want, what):
    acc, table = want
    assert np.array_equal(pt.bounce_table(), table), what
    assert_bit_equal(pt.accumulated(), acc, what)


@pytest.mark.parametrize("mode", [0, 1])
def test_fewer_items_than_workgroups(gpu, oracle_renders, mode):
    W = gpu
    pt = W.shirley_path_tracer(64, 64, max_wavefronts=BOUNCES, rng_mode=mode)
    pt.read_tile_lists()  # (builds the table at once: the sample tests the lists)
    pt.render(1)
    check(pt, oracle_renders(64, 64, 1, mode), f"64x64 mode {mode}")
    pt.close()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("arm", ["lists", "NO_TILE_LISTS", "EXACT_TRAVERSAL", "NO_LDS_SCENE"])
def test_static_rounds_and_a_dynamic_tail(gpu, oracle_renders, arm, mode):
    """20 samples, 16 in flight: 2912 items on 1024 workgroups (one static round at a share of 1/2, the rest by ticket), then 728."""
    W = gpu
    flags = 0 if arm == "lists" else getattr(W, "FLAG_" + arm)
    if arm == "NO_LDS_SCENE":
        flags |= W.FLAG_NO_REFILL  # (a scene in HBM would run the refill traversal: this is bounce_kernel over a scene it reads through L2)
    pt = W.shirley_path_tracer(W_, H_, max_wavefronts=BOUNCES, rng_mode=mode, flags=flags, batch=BATCH)
    assert pt.loop_kind == "fused"
    rec = pt.read_tile_lists()
    assert (rec is not None) == (arm == "lists")
    pt.render(SPP)
    check(pt, oracle_renders(W_, H_, SPP, mode), f"{arm} mode {mode}")
    pt.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_rank_1_of_3_of_a_band_sharded_frame(gpu, oracle_renders, mode):
    W = gpu
    pt = W.shirley_path_tracer(W_, H_, max_wavefronts=BOUNCES, rng_mode=mode, batch=BATCH, tile_rank=1, tile_world=3)
    pt.read_tile_lists()
    pt.render(SPP)
    check(pt, oracle_renders(W_, H_, SPP, mode, 1, 3), f"rank 1 of 3, mode {mode}")
    pt.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_a_context_with_an_environment_map(gpu, orc, mode):
    W = gpu
    m = (np.random.default_rng(3).random((32, 64, 3)).astype(np.float32) * np.float32(4.0))
    params = {"intensity": 1.5, "rotation": 0.3}
    pt = W.shirley_path_tracer(W_, H_, max_wavefronts=BOUNCES, rng_mode=mode, flags=W.FLAG_ENVIRONMENT, batch=BATCH)
    pt.set_environment(m, **params)
    pt.read_tile_lists()
    pt.render(SPP)
    o = orc.shirley_oracle(W_, H_, max_wavefronts=BOUNCES, rng_mode=mode)
    want = R.render_with_environment(o, m, params, spp=SPP)
    o.close()
    assert_bit_equal(pt.accumulated(), want, f"environment, mode {mode}")
    pt.close()


def test_the_batch_after_a_camera_change_walks_and_the_next_tests_the_lists(gpu, orc):
    W = gpu
    pt = W.shirley_path_tracer(W_, H_, max_wavefronts=BOUNCES, batch=BATCH)
    pt.render(BATCH)  # the first batch after wfpt_create walks
    assert pt.tile_lists_timing()[1] == 0
    look_from, look_at, vfov, defocus, focus = MOVED
    rp = pt.get_render_parameters()
    rp.update_camera_controller(W.CameraController(W.Camera(look_from, look_at), vfov, defocus, focus, 0.1, 100.0))
    pt.update_render_parameters(rp)
    pt.update_buffers()
    pt.render(BATCH)  # every tile walks: 2912 items, static rounds and tail
    assert pt.tile_lists_timing()[1] == 0
    pt.render(SPP - BATCH)  # the camera has stood for a batch: the table is built, and this batch (728 items) tests the lists
    assert pt.tile_lists_timing()[1] == 1
    sp, mt = orc.scene_book_one_final(1)
    sp, nodes = orc.build_bvh(sp)
    cam, ip, vw = orc.camera(look_from, look_at, vfov, defocus, focus, 0.1, 100.0, W_, H_)
    o = orc.Oracle(W_, H_, sp, mt, nodes, cam, ip, vw, max_wavefronts=BOUNCES)
    want = o.render(SPP)
    assert np.array_equal(pt.bounce_table(), o.bounce_table())
    assert_bit_equal(pt.accumulated(), want, "after the camera moved")
    o.close()
    pt.close()
