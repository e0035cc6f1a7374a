"""Environment-map lighting of misses (WFPT_FLAG_ENVIRONMENT, include/wfpt.h "Environment map") on the GPU.

The device lookup and whole lit renders are compared bit for bit with tests/environment_ref.py: the numpy float32 restatement of the lookup,
and the oracle's stages driven from Python with the map applied where its miss stage would apply the sky."""
import numpy as np
import pytest

import environment_ref as R
from helpers import make_mesh_oracle, make_mesh_tracer, mesh_inputs

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def W():
    import wavefront_path_tracer_amd as W
    return W


@pytest.fixture(scope="module")
def O():
    from oracle import oracle as O
    return O


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def assert_bits(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = g != w
    assert not bad.any(), f"{what}: {int(bad.sum())} values differ, first at {np.argwhere(bad)[0]}"


def make_map(w, h, seed=3):
    rng = np.random.default_rng(seed)
    m = rng.random((h, w, 3), dtype=np.float64).astype(F) * F(4.0)
    m[h // 2:, :, 1] *= F(0.25)  # some structure: a darker lower half in green
    return m


def probe_directions(n=100000, seed=5):
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, 3)).astype(F)
    d *= rng.uniform(0.01, 100.0, (n, 1)).astype(F)  # unnormalised lengths
    special = [(0, 1, 0), (0, -1, 0), (0, 0, -1), (0, 0, 1), (1, 0, 0), (-1, 0, 0), (0, 2, 0), (0, -3, 0),
               (1e-7, 1, 0), (-1e-7, 1, 0), (0, 0, 5), (-1e-6, 0, 1), (1e-6, 0, 1), (1e-30, 0.5, 1), (-1e-30, 0.5, 1),  # seam u = 0 / 1
               (0.3, 0.2, 1e-8), (1, 1, 1), (-1, -1, -1), (1, 0, 1), (-1, 0, -1)]
    return np.concatenate([np.asarray(special, F), d])


def test_device_atan2_equals_restatement(W):
    x = probe_directions()
    y, xx = x[:, 0].copy(), x[:, 2].copy()
    y = np.concatenate([y, F([0, -0.0, 0, -0.0, 1, -1, 3, -3])])
    xx = np.concatenate([xx, F([0, 0, -1, -1, 0, -0.0, 3, 3])])
    assert_bits(W.selftest_math(8, y, xx), R.atan2_(y, xx), "atan2_")


@pytest.mark.parametrize("w,h,intensity,rotation", [(1, 1, 2.5, 0.0), (3, 2, 1.0, 0.25), (64, 32, 0.5, 0.7), (2048, 1024, 1.0, 0.1),
                                                       (1025, 1024, 1.0, 0.0)])  # (a whole piece of the upload and a partial one)
def test_sample_environment_equals_restatement(W, w, h, intensity, rotation):
    pt = W.shirley_path_tracer(16, 16, flags=W.FLAG_ENVIRONMENT)
    m = make_map(w, h)
    pt.set_environment(m, intensity=intensity, rotation=rotation)
    d = probe_directions()
    assert_bits(pt.sample_environment(d), R.env_lookup(m, d, intensity, rotation), f"{w}x{h}")
    pt.close()


def lit_render(W, pt, m, spp, params=None):
    pt.set_environment(m, **(params or {}))
    pt.render(spp)
    return pt.accumulated()


@pytest.mark.parametrize("w,h", [(64, 64), (96, 54)])
@pytest.mark.parametrize("rng", ["dispatch", "pixel"])
def test_shirley_render_equals_restatement(W, O, w, h, rng):
    mode = W.RNG_DISPATCH if rng == "dispatch" else W.RNG_PIXEL
    m, params = make_map(64, 32), {"intensity": 1.5, "rotation": 0.3}
    pt = W.shirley_path_tracer(w, h, max_wavefronts=8, rng_mode=mode, flags=W.FLAG_ENVIRONMENT)
    got = lit_render(W, pt, m, 4, params)
    o = O.shirley_oracle(w, h, max_wavefronts=8, rng_mode=mode)
    want = R.render_with_environment(o, m, params, spp=4)
    assert_bits(got, want, f"shirley {w}x{h} {rng}")
    assert not np.array_equal(bits(got), bits(O.shirley_oracle(w, h, max_wavefronts=8, rng_mode=mode).render(4))), "the map changed nothing"
    pt.close()


@pytest.mark.parametrize("flags", [0, "NO_REFILL", "BINARY_BVH"])
def test_mesh_beyond_lds_equals_restatement(W, O, flags):
    w = h = 48
    f = W.FLAG_ENVIRONMENT | (getattr(W, "FLAG_" + flags) if flags else 0)
    m, params = make_map(32, 16, seed=7), {"intensity": 2.0, "rotation": 0.5}
    pt = make_mesh_tracer(W, w, h, 20000, max_wavefronts=8, flags=f)
    if not flags:
        assert pt.loop_kind == "refill"
    got = lit_render(W, pt, m, 2, params)
    o = make_mesh_oracle(O, mesh_inputs(O, w, h, 20000), w, h, max_wavefronts=8)
    assert_bits(got, R.render_with_environment(o, m, params, spp=2), f"mesh {flags}")
    pt.close()


def test_same_bits_across_loops_batches_and_shards(W):
    """(miss_floor 0: a band-sharded context counts only its own misses against the floor, so with a floor its loop may exit elsewhere)"""
    w, h, spp = 72, 48, 6
    m = make_map(128, 64, seed=11)
    base = None
    for flags, batch in [(0, 0), (W.FLAG_UNFUSED, 0), (W.FLAG_SPLIT_SHADE, 0), (W.FLAG_NO_GRAPH, 0), (0, 1), (0, 4), (0, 64)]:
        pt = W.shirley_path_tracer(w, h, max_wavefronts=8, miss_floor=0, rng_mode=W.RNG_PIXEL, flags=W.FLAG_ENVIRONMENT | flags, batch=batch)
        got = lit_render(W, pt, m, spp, {"intensity": 0.8})
        if base is None:
            base = got
        else:
            assert_bits(got, base, f"flags {flags} batch {batch}")
        pt.close()
    bands = []
    for r in range(3):
        pt = W.shirley_path_tracer(w, h, max_wavefronts=8, miss_floor=0, rng_mode=W.RNG_PIXEL, flags=W.FLAG_ENVIRONMENT, tile_rank=r,
                                   tile_world=3)
        bands.append(lit_render(W, pt, m, spp, {"intensity": 0.8}).reshape(-1, 8, w, 3))
        pt.close()
    full = np.zeros((h, w, 3), F)
    for r, b in enumerate(bands):
        for j in range(b.shape[0]):
            y0 = (j * 3 + r) * 8
            full[y0:y0 + 8] = b[j][:max(0, min(8, h - y0))]
    assert_bits(full.reshape(-1, 3), base, "three band-sharded contexts")


def test_flag_without_map_is_the_gradient_sky(W):
    w, h = 64, 40
    ref = W.shirley_path_tracer(w, h, max_wavefronts=8, flags=W.FLAG_AOV)
    ref.render(3)
    for clear in (False, True):
        pt = W.shirley_path_tracer(w, h, max_wavefronts=8, flags=W.FLAG_AOV | W.FLAG_ENVIRONMENT)
        if clear:
            pt.set_environment(make_map(8, 4))
            pt.render(2)
            pt.clear_environment()
        pt.render(3)
        assert_bits(pt.accumulated(), ref.accumulated(), f"image (clear={clear})")
        assert np.array_equal(pt.bounce_table(), ref.bounce_table())
        for name in ("albedo", "normal", "depth", "coverage"):
            assert_bits(pt.aov(name), ref.aov(name), name)
        pt.close()
    ref.close()


def test_miss_albedo_is_the_lookup_of_the_primary_direction(W, O):
    w = h = 32
    m = make_map(16, 8, seed=2)
    pt = W.shirley_path_tracer(w, h, max_wavefronts=4, flags=W.FLAG_AOV | W.FLAG_ENVIRONMENT)
    pt.set_environment(m, intensity=3.0)
    pt.render(2)
    o = O.shirley_oracle(w, h, max_wavefronts=4)
    gx, gy = (w + 7) // 8, (h + 7) // 8
    n_rays = gx * gy * 64
    alb = np.zeros((w * h, 3), F)
    for f in (1, 2):
        o.set_frame(f, 0)
        o.set_counters([0, 0, n_rays])
        o.generate_rays(gx, gy, True)
        o.extend(*O.workgroup_size_64(n_rays))
        c = o.counters()
        rays = o.rays(n_rays)
        miss = o.misses(int(c[0]))
        px = rays["pixel_idx"][miss].astype(np.int64)
        alb[px] = alb[px] + R.env_lookup(m, rays["direction"][miss, :3], 3.0)
    cov = pt.aov("coverage").reshape(-1)
    missed = cov == 0  # every sample missed: the albedo is the mean of the lookups
    assert missed.any()
    got = pt.aov("albedo").reshape(-1, 3)[missed]
    assert_bits(got, alb[missed] / F(2), "miss albedo")
    pt.close()


def test_set_map_resets_and_drops_graphs_and_history(W):
    w, h = 48, 32
    m1, m2 = make_map(32, 16, seed=1), make_map(32, 16, seed=2)
    pt = W.shirley_path_tracer(w, h, max_wavefronts=8, flags=W.FLAG_ENVIRONMENT | W.FLAG_DENOISE)
    pt.set_environment(m1)
    pt.render(3)  # captures a graph with m1 baked into its kernel arguments
    pt.denoise_temporal()
    pt.set_environment(m2)
    assert not pt.accumulated().any(), "setting a map restarts the accumulation"
    pt.render(3)
    assert_bits(pt.denoise_temporal(), pt.denoise(), "temporal after a new map = spatial")
    fresh = W.shirley_path_tracer(w, h, max_wavefronts=8, flags=W.FLAG_ENVIRONMENT | W.FLAG_DENOISE)
    fresh.set_environment(m2)
    fresh.render(3)
    assert_bits(pt.accumulated(), fresh.accumulated(), "after a second map (no stale graph)")
    fresh.close()
    pt.close()


def test_update_scene_keeps_the_map(W):
    w, h = 48, 32
    m = make_map(32, 16, seed=4)
    pt = W.shirley_path_tracer(w, h, max_wavefronts=8, flags=W.FLAG_ENVIRONMENT)
    pt.set_environment(m, intensity=2.0)
    pt.render(2)
    pt.update_scene(W.Scene.book_one_final(1))
    pt.render(2)
    fresh = W.shirley_path_tracer(w, h, max_wavefronts=8, flags=W.FLAG_ENVIRONMENT)
    fresh.set_environment(m, intensity=2.0)
    fresh.render(2)
    assert_bits(pt.accumulated(), fresh.accumulated(), "update_scene keeps the map")
    fresh.close()
    pt.close()


def test_refusals_leave_the_context_usable(W):
    w, h = 32, 24
    m = make_map(16, 8, seed=9)
    plain = W.shirley_path_tracer(w, h, max_wavefronts=4)
    with pytest.raises(W.WfptError) as e:
        plain.set_environment(m)
    assert e.value.status == -1
    plain.close()
    binned = W.shirley_path_tracer(w, h, max_wavefronts=4, rng_mode=W.RNG_PIXEL, flags=W.FLAG_ENVIRONMENT | W.FLAG_BINNING)
    if binned.loop_kind == "fused_binned":
        with pytest.raises(W.WfptError) as e:
            binned.set_environment(m)
        assert e.value.status == -4
    binned.close()
    pt = W.shirley_path_tracer(w, h, max_wavefronts=4, flags=W.FLAG_ENVIRONMENT)
    pt.set_environment(m, intensity=2.0)
    pt.render(2)
    want = pt.accumulated()
    bad = [(np.full((8, 4, 3), np.nan, F), {}), (-np.ones((8, 4, 3), F), {}), (np.full((8, 4, 3), np.inf, F), {}),
           (np.ones((1, 16385, 3), F), {}), (np.ones((8193, 1, 3), F), {}), (np.ones((0, 4, 3), F), {}),
           (m, {"intensity": -1.0}), (m, {"intensity": float("inf")}), (m, {"rotation": 1.0}), (m, {"rotation": -0.1})]
    for rgb, kw in bad:
        with pytest.raises(W.WfptError) as e:
            pt.set_environment(rgb, **kw)
        assert e.value.status == -1, (rgb.shape, kw)
    assert_bits(pt.accumulated(), want, "a refused call resets nothing")
    pt.render(2)
    fresh = W.shirley_path_tracer(w, h, max_wavefronts=4, flags=W.FLAG_ENVIRONMENT)
    fresh.set_environment(m, intensity=2.0)
    fresh.render(4)
    assert_bits(pt.accumulated(), fresh.accumulated(), "the previous map is kept")
    pt.clear_environment()
    with pytest.raises(W.WfptError) as e:
        pt.sample_environment(np.ones((4, 3), F))
    assert e.value.status == -1
    fresh.close()
    pt.close()
