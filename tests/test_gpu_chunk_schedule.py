"""The fused launches' chunked hand-out of their work items (csrc/wfpt_ticket_chunks.h) on the device:
whichever workgroup runs an item, and whether it drew it or followed into it, image and bounce table equal the oracle's bit for bit, in
both RNG modes. The shapes are the smallest that take each branch of the rule on a grid of 1024 workgroups with the shipped constants
(no static share, WFPT_FIRST_CHUNK 4, 4 tail rounds: the last 4096 positions of a launch go out singly):
  * 64x64, 1 sample: 8 first-launch items, fewer than the workgroups -- no static round, no chunk completes, most workgroups leave at once;
  * 400x225 (182 items per sample), 128 samples in flight, 130 samples: a first launch of 23 296 items -- 4800 whole chunks (19 200 items), no leftover, 4096
    singles -- then one of 364 items, fewer than the grid: all singles;
  * the same with 127 samples in flight (an addition to the shapes asked for: 23 296 - 4096 is a multiple of every chunk length of the sweep):
    23 114 items -- 4754 chunks, a leftover of 2, 4096 singles -- then 546;
  * the same with WFPT_FLAG_NO_TILE_LISTS (every tile walks), and rank 1 of 3 of the band-sharded frame (64 items per sample: 8192 items,
    then 128).
With 4 bounces the same renders run the middle and the last launches over their tickets at WFPT_BOUNCE_CHUNK (4, 4 tail rounds): hit and miss items interleaved by TicketMap,
whole chunks, leftover and tail at whatever counts the scene gives, and launches of fewer items than the grid."""
import numpy as np
import pytest

from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu

W_, H_, BATCH, SPP, BOUNCES = 400, 225, 128, 130, 4


@pytest.fixture(scope="module")
def oracle_renders(orc):
    """(accumulated, bounce table) of the book scene, computed once per (size, samples, RNG mode, rank, world) and left unchanged."""
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
@pytest.mark.parametrize("arm", ["lists", "NO_TILE_LISTS", "lists_127_in_flight"])
def test_whole_chunks_leftover_and_tail(gpu, oracle_renders, arm, mode):
    """130 samples, 128 in flight: 23 296 first-launch items on 1024 workgroups, then 364 (127 in flight: 23 114, then 546)."""
    W = gpu
    flags = W.FLAG_NO_TILE_LISTS if arm == "NO_TILE_LISTS" else 0
    pt = W.shirley_path_tracer(W_, H_, max_wavefronts=BOUNCES, rng_mode=mode, flags=flags, batch=127 if arm == "lists_127_in_flight" else BATCH)
    assert pt.loop_kind == "fused"
    assert (pt.read_tile_lists() is not None) == (arm != "NO_TILE_LISTS")
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
