"""The first fused launch's per-tile candidate lists on the device (include/wfpt.h "Tile lists"): the device builder against its host
twin, the renders against the oracle bit for bit -- with lists, with WFPT_FLAG_NO_TILE_LISTS, where both arms run in one launch and
where every tile has a list -- and the table's invalidation by a moved camera and a changed scene."""
import numpy as np
import pytest

from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu

BOOK = ((13.0, 2.0, 3.0), (0.0, 0.0, 0.0), 20.0, 0.6, 10.0)
PINHOLE = ((13.0, 2.0, 3.0), (0.0, 0.0, 0.0), 20.0, 0.0, 10.0)
HEAD_ON = ((0.0, 0.0, 1.0), (0.0, 0.0, -1.0), 90.0, 0.0, 10.0)


def controller(W, camera):
    look_from, look_at, vfov, defocus, focus = camera
    return W.CameraController(W.Camera(look_from, look_at), vfov, defocus, focus, 0.1, 100.0)


def tracer(W, kind, camera, w, h, **kw):
    scene = W.Scene.book_one_final(1) if kind == "shirley" else W.Scene.new()
    return W.PathTracer(scene, W.RenderParameters(controller(W, camera), (w, h)), **kw)


def oracle_for(O, kind, camera, w, h, spheres=None, **kw):
    sp, mt = O.scene_book_one_final(1) if kind == "shirley" else O.scene_new()
    sp, nodes = O.build_bvh(sp if spheres is None else spheres)
    look_from, look_at, vfov, defocus, focus = camera
    cam, ip, vw = O.camera(look_from, look_at, vfov, defocus, focus, 0.1, 100.0, w, h)
    return O.Oracle(w, h, sp, mt, nodes, cam, ip, vw, **kw)


def host_twin(W, pt, w, h, rank=0, world=1):
    cc = pt.render_parameters.camera_controller()
    proj = W.ProjectionMatrix(cc.vfov_rad(), np.float32(w) / np.float32(h), *cc.get_clip_planes()).p_inv()
    return W.tile_lists_host(pt.bvh_tree.nodes, cc.get_GPU_camera(), proj, cc.get_view_matrix(), w, h, rank, world)


@pytest.mark.parametrize("kind,camera,w,h,rank,world", [
    ("shirley", BOOK, 128, 72, 0, 1), ("shirley", BOOK, 64, 40, 0, 1), ("shirley", BOOK, 60, 44, 0, 1), ("simple", HEAD_ON, 64, 64, 0, 1),
    ("shirley", BOOK, 128, 72, 1, 3), ("shirley", PINHOLE, 128, 72, 0, 1), ("shirley", PINHOLE, 60, 44, 0, 1)])
def test_device_builder_equals_the_host_twin(gpu, kind, camera, w, h, rank, world):
    W = gpu
    pt = tracer(W, kind, camera, w, h, max_wavefronts=3, tile_rank=rank, tile_world=world)
    got = pt.read_tile_lists()
    want = host_twin(W, pt, w, h, rank, world)
    assert got is not None and got.shape == want.shape
    assert np.array_equal(got, want), np.argwhere((got != want).any(axis=1))[:8]
    ms, builds = pt.tile_lists_timing()
    assert builds == 1 and ms >= 0.0
    pt.close()


def test_contexts_that_keep_no_lists(gpu):
    W = gpu
    for flags in (W.FLAG_NO_TILE_LISTS, W.FLAG_EXACT_TRAVERSAL, W.FLAG_NO_LDS_SCENE, W.FLAG_UNFUSED):
        pt = tracer(W, "shirley", BOOK, 64, 40, max_wavefronts=3, flags=flags)
        assert pt.read_tile_lists() is None, flags
        pt.close()
    pt = tracer(W, "shirley", BOOK, 64, 40, max_wavefronts=3, flags=W.FLAG_BINNING, rng_mode=W.RNG_PIXEL)
    assert pt.read_tile_lists() is None
    pt.close()


@pytest.fixture(scope="module")
def oracle_renders(orc):
    """(accumulated, bounce table, totals) of 4 samples of the book scene, computed once per (size, RNG mode)."""
    cache = {}

    def get(w, h, mode):
        if (w, h, mode) not in cache:
            o = oracle_for(orc, "shirley", BOOK, w, h, max_wavefronts=5, rng_mode=mode)
            acc = o.render(4)
            cache[(w, h, mode)] = (acc, o.bounce_table(), o.totals())
            o.close()
        return cache[(w, h, mode)]
    return get


@pytest.mark.parametrize("w,h", [(128, 72), (64, 40), (400, 224)])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("lists", [True, False])
def test_image_and_table_against_the_oracle(gpu, oracle_renders, w, h, mode, lists):
    """128x72 and 64x40: tiles with and without a list, so both arms run in the one launch; 400x224: every tile has a list."""
    W = gpu
    want_acc, want_table, want_totals = oracle_renders(w, h, mode)
    pt = tracer(W, "shirley", BOOK, w, h, max_wavefronts=5, rng_mode=mode, flags=0 if lists else W.FLAG_NO_TILE_LISTS)
    rec = pt.read_tile_lists()  # (builds the table at once; without this the first batch would walk)
    if lists:
        none = rec[:, 0] == W.TILE_NO_LIST
        assert not none.all() and (none.any() if (w, h) != (400, 224) else not none.any()), (w, h, float(none.mean()))
    else:
        assert rec is None
    pt.render(4)
    assert np.array_equal(pt.bounce_table(), want_table)
    assert_bit_equal(pt.accumulated(), want_acc, f"{w}x{h} mode {mode} lists {lists}")
    assert np.array_equal(pt.totals(), want_totals)
    pt.close()


def test_a_moved_camera_and_a_changed_scene_rebuild_the_table(gpu, orc):
    W = gpu
    w, h, bounces = 128, 72, 4
    pt = tracer(W, "shirley", BOOK, w, h, max_wavefronts=bounces)
    pt.render(1)  # the first batch after wfpt_create walks: the table is built before the second one
    assert pt.tile_lists_timing()[1] == 0
    pt.render(1)
    assert pt.tile_lists_timing()[1] == 1
    first = pt.read_tile_lists()
    assert pt.tile_lists_timing()[1] == 1 and np.array_equal(first, host_twin(W, pt, w, h))
    o = oracle_for(orc, "shirley", BOOK, w, h, max_wavefronts=bounces)
    assert_bit_equal(pt.accumulated(), o.render(2), "before anything moved")
    o.close()
    # the camera moves
    moved_cam = ((9.0, 3.0, -5.0), (0.0, 0.5, 0.0), 25.0, 0.4, 9.0)
    rp = pt.get_render_parameters()
    rp.update_camera_controller(controller(W, moved_cam))
    pt.update_render_parameters(rp)
    pt.update_buffers()
    pt.render(1)  # every record reads "no list" now: a stale list would show in the image
    assert pt.tile_lists_timing()[1] == 1
    pt.render(1)  # the camera has been kept for a second batch: built, and used by this one
    assert pt.tile_lists_timing()[1] == 2
    second = pt.read_tile_lists()
    assert not np.array_equal(first, second) and np.array_equal(second, host_twin(W, pt, w, h))
    o = oracle_for(orc, "shirley", moved_cam, w, h, max_wavefronts=bounces)
    assert_bit_equal(pt.accumulated(), o.render(2), "after the camera moved")
    o.close()
    # a sphere moves into the view: the lists of the tiles that see it must name its new leaf
    scene = W.Scene.book_one_final(1)
    k = int(np.argmax(scene.spheres["radius"] == 1.0))
    scene.spheres["center"][k, :3] = (2.0, 2.5, -1.0)
    sp_o = scene.spheres.view(orc.SPHERE).copy()
    pt.update_scene(W.Scene(scene.spheres.copy(), scene.materials.copy()))
    pt.render(1)
    pt.render(1)
    assert pt.tile_lists_timing()[1] == 3
    o = oracle_for(orc, "shirley", moved_cam, w, h, spheres=sp_o, max_wavefronts=bounces)
    assert_bit_equal(pt.accumulated(), o.render(2), "after the scene changed")
    assert np.array_equal(pt.bounce_table(), o.bounce_table())
    o.close()
    pt.close()


@pytest.mark.parametrize("camera,inside", [(((4.0, 1.0, 3.0), (4.0, 1.0, 0.0), 40.0, 0.6, 3.0), True),
                                           (((60.0, 20.0, 30.0), (0.0, 0.0, 0.0), 8.0, 0.6, 70.0), False)])
def test_cameras_near_a_marble_and_outside_the_safe_region(gpu, orc, camera, inside):
    """2 units in front of a big marble (inside the ball of origins the free walks are proven for), and 70 units out, beyond it: there
    every primary ray is handed to the reference's walk, list or no list."""
    W = gpu
    w, h, bounces = 128, 72, 4
    o = oracle_for(orc, "shirley", camera, w, h, max_wavefronts=bounces)
    want = o.render(2)
    for flags in (0, W.FLAG_NO_TILE_LISTS):
        pt = tracer(W, "shirley", camera, w, h, max_wavefronts=bounces, flags=flags)
        rec = pt.read_tile_lists()  # (builds the table at once: both samples below run the list arm)
        if flags == 0:
            assert rec is not None and (rec[:, 0] != W.TILE_NO_LIST).any(), "the context keeps no list: only the walk would be tested"
        else:
            assert rec is None
        pt.render(2)
        assert np.array_equal(pt.bounce_table(), o.bounce_table())
        assert_bit_equal(pt.accumulated(), want, f"inside {inside} flags {flags}")
        pt.close()
    o.close()
