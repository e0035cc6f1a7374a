"""shade, miss_kernel and the device-resident loops on inputs no shipped scene produces, against the oracle, 0 ulp.

The rays and scenes are those of helpers.py whose conditions tests/test_shade_edges_host.py asserts from the oracle alone. Every ray, material
or pixel class is declared finite or may-be-NaN: for finite ones the oracle's output is first shown NaN-free and then compared with the strict
assert_bit_equal; the NaN-aware assert_bits_or_nan is used for the may-be-NaN ones only (at most a quarter of a test's rays or pixels)."""
import numpy as np
import pytest

import environment_ref as R
import texture_ref as T
from conftest import assert_bit_equal
from helpers import (assert_bits_or_nan, closed_room_inputs, degenerate_radius_rays, fallback_wall, make_mesh_oracle, make_oracle, material_zoo,
                     ray_floats, shade_edge_mesh, shade_edge_rays)

pytestmark = pytest.mark.gpu
F = np.float32
CAMERA = ((0.0, 0.5, 12.0), (0.0, 0.0, 0.0), 60.0)


def fenced_equal(got, want, maybe_nan, what):
    """Rows declared finite: the oracle's hold no NaN, then bit for bit. Rows declared may-be-NaN (at most a quarter): NaN-aware."""
    got, want = np.ascontiguousarray(got, "<f4"), np.ascontiguousarray(want, "<f4")
    assert maybe_nan.mean() <= 0.25, f"{what}: {maybe_nan.mean():.3f} of the rows are may-be-NaN"
    assert not np.isnan(want[~maybe_nan]).any(), f"{what}: the oracle holds a NaN in a finite class"
    assert_bit_equal(got[~maybe_nan], want[~maybe_nan], what + " (finite classes)")
    assert_bits_or_nan(got[maybe_nan], want[maybe_nan], what + " (may-be-NaN classes)")


def zoo_pair(W, orc, w, h, with_nan=True, degenerate_radii=False, **kw):
    sp, mt = material_zoo(orc, with_nan, degenerate_radii)
    spo, nodes = orc.build_bvh(sp)
    cam, ip, vw = orc.camera(CAMERA[0], CAMERA[1], CAMERA[2], 0.0, 10.0, 0.1, 100.0, w, h)
    okw = {k: v for k, v in kw.items() if k in ("max_wavefronts", "miss_floor", "rng_mode")}
    o = orc.Oracle(w, h, spo, mt, nodes, cam, ip, vw, **okw)
    cc = W.CameraController(W.Camera(CAMERA[0], CAMERA[1]), CAMERA[2], 0.0, 10.0, 0.1, 100.0)
    pt = W.PathTracer(W.Scene(sp.view(W.SPHERE).copy(), mt.view(W.MATERIAL)), W.RenderParameters(cc, (w, h)), **kw)
    assert_bit_equal(pt.bvh_tree.nodes, nodes.view(W.BVH_NODE), "host BVH of the zoo")
    return sp, mt, o, pt


def run_chain(W, orc, pt, o, rays, maybe_nan, shade_stages, wavefronts=2, env=None):
    """write_rays, then per wavefront extend (counters and queues), shade (extension rays, image), miss_kernel (image), swap; accumulate.
    maybe_nan is per pixel. env = (map, params): the oracle's miss is replaced by the numpy restatement of the lookup, and the chain STOPS
    after the first miss_kernel (the oracle's image cannot carry the map's factor on; `wavefronts` is ignored)."""
    n = len(rays)
    pt.write_rays(rays); o.write_rays(rays.view(orc.RAY))
    pt.reset_image(); o.reset_image()
    pt.set_counters([0, 0, n]); o.set_counters([0, 0, n])
    n_rays = n
    for wave in range(wavefronts):
        ext = W.workgroup_size_64(n_rays)
        pt.extend_kernel.run(ext); o.extend(*ext)
        c = o.counters()
        assert np.array_equal(pt.read_counters()[:3], c[:3]), f"counters after extend {wave}"
        misses, hits = int(c[0]), int(c[1])
        assert_bit_equal(pt.hits(hits), o.hits(hits).view(W.HIT), f"hit queue {wave}")
        assert_bit_equal(pt.misses(misses), o.misses(misses), f"miss queue {wave}")
        cur = o.rays(n_rays)
        c[2] = 0
        pt.set_counters(c); o.set_counters(c)
        sh, ms = W.workgroup_size_64(hits), W.workgroup_size_64(misses)
        for k in shade_stages:
            k.run(sh)
        o.shade(*sh)
        assert int(pt.read_counters()[2]) == int(o.counters()[2]) == hits
        g, e = pt.extension_rays(hits), o.extension_rays(hits).view(W.RAY)
        assert np.array_equal(g["pixel_idx"], e["pixel_idx"])
        fenced_equal(ray_floats(g), ray_floats(e), maybe_nan[e["pixel_idx"]], f"extension rays {wave}")
        fenced_equal(pt.image(), o.image(), maybe_nan, f"image after shade {wave}")
        pt.miss_kernel.run(ms)
        if env is None:
            o.miss(*ms)
            want = o.image()
        else:
            m = cur[o.misses(misses)]
            want = o.image()
            with np.errstate(all="ignore"):
                want[m["pixel_idx"]] = want[m["pixel_idx"]] * R.env_lookup(env[0], m["direction"][:, :3], **env[1])
        fenced_equal(pt.image(), want, maybe_nan, f"image after miss {wave}")
        if env is not None:
            return
        pt.swap_ray_queues(); o.swap_ray_queues()
        n_rays = hits
        pt.set_counters([0, 0, hits, 0]); o.set_counters([0, 0, hits, 0])
    acc = W.workgroup_size_64(pt.n_pixels)
    pt.accumulate_kernel.run(acc); o.accumulate(*acc)
    fenced_equal(pt.accumulated(), o.accumulated(), maybe_nan, "accumulated")


@pytest.mark.parametrize("rng_mode", [0, 1])
@pytest.mark.parametrize("flags", ["0", "NO_LDS_SCENE"])
@pytest.mark.parametrize("stages", ["shade", "per-material"])
def test_edge_rays_through_shade_and_miss(gpu, orc, rng_mode, flags, stages):
    """The edge rays of shade_edge_rays (head-on, grazing, critical angle, direction lengths, origins, the aimed Lambertian fall-back) on the
    material zoo: extend, shade, miss_kernel, swap, and once more on the scattered rays (directions of length 1e-20 and 1e3, zero vectors
    from overflowed normalisations and near-zero fall-back candidates go through the walk again), then accumulate. Lengths 1e-3, 1e3 and
    1e-20 reach scatter(); 1e18 and 1e-30 cannot hit and reach miss_kernel only (helpers.shade_edge_rays)."""
    W = gpu
    w, h = 128, 64
    sp, mt, o, pt = zoo_pair(W, orc, w, h, rng_mode=rng_mode, flags=getattr(W, "FLAG_" + flags, 0))
    rays, cls, target, ray_nan = shade_edge_rays(W, sp, mt, w, h, 1, rng_mode, orc)
    maybe_nan = np.zeros(w * h, bool)
    maybe_nan[:len(rays)] = ray_nan  # pixel == ray index; the pixels no ray owns stay 1.0 on both sides
    pt.set_frame(W.GPUFrameBuffer.new(w, h, 1)); o.set_frame(1, 0)
    ks = [pt.shade_kernel] if stages == "shade" else [W.Kernel(k, pt) for k in ("shade_lambertian", "shade_metal", "shade_dielectric")]
    run_chain(W, orc, pt, o, rays, maybe_nan, ks)
    pt.close(); o.close()


@pytest.mark.parametrize("env_size", [None, (8, 4), (1, 1)])
def test_degenerate_rays_through_shade_and_miss(gpu, orc, env_size):
    """The NaN / inf / zero / denormal / 1e18 rays of test_extend_on_degenerate_rays, with unique pixels, continued through shade and
    miss_kernel: gradient sky, and WFPT_FLAG_ENVIRONMENT with an 8 x 4 and a 1 x 1 map. Rays whose direction holds a NaN, an infinity, or is
    zero are the may-be-NaN class (kinds 3, 10, 12 of 16: 3/16 of the rays; the oracle's sky is NaN for -inf only). What env_lookup reads
    for them (wfpt_device_math.h): a zero, NaN or infinite direction normalises to NaN components (0 * inf, inf * 0); atan2_ reads signs
    and magnitudes by comparisons, all false for a NaN, so phi = theta = 0, u = 0.5 + rotation, v = 0: an ordinary texel of row 0 and a
    finite result. Denormal directions and 1e-30 (kinds 5, 4: d.d underflows to 0) normalise to +-inf components (d * inf); atan2_(inf, inf)
    is inf / inf = NaN, so u, v, x0 and y0 are NaN: fmax(NaN, -1) = -1 makes column c0 = w - 1 and c1 = 0, fmax(NaN, 0) = 0 makes both rows 0,
    all inside the map (texel 0 of a 1 x 1 map), and the NaN weights make the result NaN. Under a map kinds 4 and 5 are may-be-NaN too,
    5/16 in all, so the map cases
    carry only every other such ray (the rest keep an ordinary direction)."""
    from test_gpu_parity import _odd_rays
    from helpers import inputs_for, make_tracer
    W = gpu
    w, h = 128, 64
    n = w * h
    o = make_oracle(orc, inputs_for(orc, "shirley", w, h), w, h)
    pt = make_tracer(W, "shirley", w, h, flags=W.FLAG_ENVIRONMENT if env_size else 0)
    rays = _odd_rays(W, n, 3)
    rays["pixel_idx"] = np.arange(n, dtype="<u4")
    kind = np.arange(n) % 16
    if env_size:  # keep the may-be-NaN share under a quarter: every other ray of kinds 4 and 5 gets an ordinary direction
        tame = np.isin(kind, (4, 5)) & ((np.arange(n) // 16) % 2 == 1)
        rays["direction"][tame, :3] = F([0.3, -0.5, 0.8])
        rays["inv_direction"][tame] = F(1.0) / F([0.3, -0.5, 0.8])
        kind = np.where(tame, 0, kind)
    maybe_nan = np.isin(kind, (3, 10, 12, 4, 5) if env_size else (3, 10, 12))
    env = None
    if env_size:
        m = (np.random.default_rng(9).random((env_size[1], env_size[0], 3)) * 3.0).astype(F)
        params = {"intensity": 1.5, "rotation": 0.25}
        pt.set_environment(m, **params)
        env = (m, params)
    pt.set_frame(W.GPUFrameBuffer.new(w, h, 1)); o.set_frame(1, 0)
    run_chain(W, orc, pt, o, rays, maybe_nan, [pt.shade_kernel], env=env)  # two wavefronts under the sky, one under a map
    pt.close(); o.close()


SPECIALS = F([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1e-39, 3.4028235e38, -3.4028235e38, 1.0, -1.0, 0.25])


def test_lookups_on_non_finite_input(gpu):
    """wfpt_sample_environment, wfpt_sample_texture (bilinear and nearest; 1 x 1, 3 x 2, 64 x 32) and atan2_ on every combination of +-0, +-inf,
    NaN, denormals and +-FLT_MAX, against the numpy restatements. Neither entry point refuses non-finite input; both clamp the texel
    coordinate as a float before it becomes an index. Environment: see test_degenerate_rays_through_shade_and_miss (NaN components read an
    ordinary texel of row 0 through atan2_'s comparisons, inf / inf reads row 0, columns w - 1 and 0). Texture: u' = u - floor(u) is NaN for NaN and +-inf (inf - inf) and 0 for +-FLT_MAX (an integer);
    nearest: fmax(floor(NaN), 0) = 0 reads column / row 0, a finite texel; bilinear: wrap_pair's fmax(NaN, -1) = -1 reads index n - 1 and 0,
    and the NaN weight makes the result NaN. A quarter of the probes at most are non-finite: the rest are ordinary directions / UVs."""
    W = gpu
    g = np.array(np.meshgrid(SPECIALS, SPECIALS, SPECIALS), F).reshape(3, -1).T
    yy, xx = g[:, 0].copy(), g[:, 1].copy()
    with np.errstate(all="ignore"):
        assert_bits_or_nan(W.selftest_math(8, yy, xx), R.atan2_(yy, xx), "atan2_ on specials")
    rng = np.random.default_rng(2)
    ordinary = rng.standard_normal((4 * len(g), 3)).astype(F)
    odd = ~np.isfinite(g).all(axis=1) | (np.abs(g) < 1e-30).all(axis=1) | (np.abs(g) > 1e30).any(axis=1)
    dirs = np.concatenate([g, ordinary])
    maybe = np.concatenate([odd, np.zeros(len(ordinary), bool)])
    pt = W.shirley_path_tracer(16, 16, flags=W.FLAG_ENVIRONMENT)
    for (w, h) in ((1, 1), (3, 2), (64, 32)):
        m = (rng.random((h, w, 3)) * 4.0).astype(F)
        pt.set_environment(m, intensity=2.0, rotation=0.3)
        with np.errstate(all="ignore"):
            want = R.env_lookup(m, dirs, 2.0, 0.3)
        fenced_equal(pt.sample_environment(dirs), want, maybe, f"environment {w}x{h}")
    pt.close()
    pt = W.shirley_path_tracer(16, 16, flags=W.FLAG_TEXTURES)
    g2 = np.array(np.meshgrid(SPECIALS, SPECIALS), F).reshape(2, -1).T
    uv = np.concatenate([g2, rng.uniform(-3, 3, (4 * len(g2), 2)).astype(F)])  # 0.62 of g2's rows are may-be-NaN: 1/8 of all
    maybe = np.concatenate([~(np.abs(g2) < 1e30).all(axis=1), np.zeros(4 * len(g2), bool)])  # FLT_MAX * 1.5 overflows under slot 1's scale
    for s, (w, h) in enumerate(((1, 1), (3, 2), (64, 32))):
        img = (rng.random((h, w, 3)) * 2.0).astype(F)
        for flt in ("bilinear", "nearest"):
            params = {"scale": (1.5, -2.0), "offset": (0.1, 7.0)} if s == 1 else {}
            pt.set_texture(s, img, filter=flt, **params)
            with np.errstate(all="ignore"):
                want = T.tex_lookup(img, uv[:, 0], uv[:, 1], filter=flt, **params)
            fenced_equal(pt.sample_texture(s, uv), want, maybe, f"texture {w}x{h} {flt}")
    pt.close()


# ------------------------------------------------------------------ the device-resident loops
LOOPS = [("0", 0, 0), ("NO_GRAPH", 0, 16), ("UNFUSED", 1, 1), ("SPLIT_SHADE", 0, 0), ("BINNING", 1, 16), ("NO_LDS_SCENE", 1, 0),
         ("NO_LDS_SCENE|NO_REFILL", 0, 16), ("0|AOV|DENOISE", 1, 1)]


def loop_flags(W, names):
    fl = 0
    for name in names.split("|"):
        fl |= getattr(W, "FLAG_" + name, 0)
    return fl


@pytest.mark.parametrize("names,rng_mode,batch", LOOPS)
@pytest.mark.parametrize("with_nan", [False, True])
def test_loops_on_the_material_zoo(gpu, orc, names, rng_mode, batch, with_nan):
    """Three samples of the zoo seen from outside through every loop. Finite materials: the oracle's image is NaN-free, strict. With the
    may-be-NaN materials (index 0, negative, inf, NaN) a pixel's class cannot be declared from the inputs (any path may meet such a sphere at
    any bounce), so the mask is "NaN in the oracle's image": at most a quarter, every other pixel strict. With AOV|DENOISE (batch 1) the
    luminance moments are compared too: wfpt_read_variance against denoise_ref's resolve of S1, S2 summed from the ORACLE's per-sample
    images, under the same fence."""
    W = gpu
    w, h, spp = 128, 72, 3
    sp, mt, o, pt = zoo_pair(W, orc, w, h, with_nan, rng_mode=rng_mode, max_wavefronts=8, flags=loop_flags(W, names), batch=batch)
    import denoise_ref as D
    s1, s2 = np.zeros(w * h, F), np.zeros(w * h, F)
    for s in range(spp):
        o.render_sample()
        with np.errstate(all="ignore"):
            L = D.luma(o.image())
            s1, s2 = s1 + L, s2 + L * L
    pt.render(spp)
    assert np.array_equal(pt.bounce_table(), o.bounce_table()) and np.array_equal(pt.totals(), o.totals())
    want = o.accumulated()
    maybe = np.isnan(want).any(axis=1)
    assert with_nan or not maybe.any()
    fenced_equal(pt.accumulated(), want, maybe, f"zoo {names}")
    if "DENOISE" in names:
        with np.errstate(all="ignore"):
            var = D.variance_resolve(s1, s2, spp)
        fenced_equal(pt.variance().reshape(-1), var.reshape(-1), maybe | np.isnan(var.reshape(-1)), f"variance {names}")
    pt.close(); o.close()


@pytest.mark.parametrize("names,rng_mode,batch", LOOPS)
@pytest.mark.parametrize("scene", ["closed-metal", "closed-glass", "centre"])
def test_loops_without_a_single_miss(gpu, orc, scene, names, rng_mode, batch):
    """The camera inside a closed sphere (metal of fuzz 0; glass; exactly at the centre): miss_floor 128 leaves at wavefront 0 with every
    pixel at 1.0 per sample and one table row; miss_floor 0 runs every wavefront full to max_wavefronts 1, 2 and 50 with zero misses in
    every row. All finite."""
    W = gpu
    w, h, spp = 64, 40, 2
    inputs = closed_room_inputs(orc, scene, w, h)
    pos = (0.0, 0.0, 0.0) if scene == "centre" else (0.5, 0.25, 1.0)
    cc = W.CameraController(W.Camera(pos, (0.5, 0.0, -1.0)), 70.0, 0.0, 10.0, 0.1, 100.0)
    for miss_floor, max_wavefronts in ((128, 50), (0, 1), (0, 2), (0, 50)):
        o = make_oracle(orc, inputs, w, h, max_wavefronts=max_wavefronts, miss_floor=miss_floor, rng_mode=rng_mode)
        want = o.render(spp)
        scn = W.Scene(inputs[0].view(W.SPHERE).copy(), inputs[1].view(W.MATERIAL))
        pt = W.PathTracer(scn, W.RenderParameters(cc, (w, h)), max_wavefronts=max_wavefronts, miss_floor=miss_floor, rng_mode=rng_mode,
                          flags=loop_flags(W, names), batch=batch)
        pt.render(spp)
        t = pt.bounce_table()
        assert np.array_equal(t, o.bounce_table()) and np.array_equal(pt.totals(), o.totals())
        assert (t[:, 2] == 0).all() and len(t) == (1 if miss_floor else max_wavefronts)
        assert not np.isnan(want).any()
        assert_bit_equal(pt.accumulated(), want, f"{scene} {names} floor {miss_floor} max {max_wavefronts}")
        if miss_floor:
            assert (pt.accumulated() == spp).all()
        pt.close(); o.close()


# ------------------------------------------------------------------ the mesh
@pytest.mark.parametrize("rng_mode", [0, 1])
@pytest.mark.parametrize("flags", ["0", "NO_LDS_SCENE"])
@pytest.mark.parametrize("stages", ["shade", "per-material"])
def test_edge_mesh_through_shade_and_miss(gpu, orc, rng_mode, flags, stages):
    """shade_edge_mesh (one triangle per ray: head-on from both faces, dot(n, -uv) at +-1, +-4, +-64 ulp-sized tilts of 0, the critical
    angle, direction lengths, the aimed fall-back with the triangle's normal = -rb') on the mesh in LDS and beyond it: the same chain as
    the spheres, two wavefronts and accumulate."""
    W = gpu
    w, h = 128, 64
    tris, mt, rays, cls, ray_nan = shade_edge_mesh(W, orc, w, h, 1, rng_mode)
    tb, nodes = orc.build_bvh_triangles(tris, 32)
    cam, ip, vw = orc.mesh_camera(w, h)
    o = make_mesh_oracle(orc, (tb, mt, nodes, cam, ip, vw), w, h, rng_mode=rng_mode)
    cc = W.CameraController(W.Camera((0.0, 0.0, 30.0), (0.0, 0.0, 0.0)), 40.0, 0.0, 10.0, 0.1, 100.0)
    scene = W.Scene(np.zeros(0, W.SPHERE), mt.view(W.MATERIAL), triangles=tris.view(W.TRIANGLE).copy())
    pt = W.PathTracer(scene, W.RenderParameters(cc, (w, h)), rng_mode=rng_mode, flags=getattr(W, "FLAG_" + flags, 0))
    assert_bit_equal(pt.bvh_tree.nodes, nodes.view(W.BVH_NODE), "host BVH of the edge mesh")
    maybe_nan = np.zeros(w * h, bool)
    maybe_nan[:len(rays)] = ray_nan
    pt.set_frame(W.GPUFrameBuffer.new(w, h, 1)); o.set_frame(1, 0)
    ks = [pt.shade_kernel] if stages == "shade" else [W.Kernel(k, pt) for k in ("shade_lambertian", "shade_metal", "shade_dielectric")]
    run_chain(W, orc, pt, o, rays, maybe_nan, ks)
    pt.close(); o.close()


@pytest.mark.parametrize("names,kind", [("0", "fused"), ("NO_GRAPH", "fused"), ("UNFUSED", "stages"), ("SPLIT_SHADE", None), ("BINNING", "fused_binned"),
                                        ("NO_LDS_SCENE", "refill"), ("NO_LDS_SCENE|NO_REFILL", None)])
@pytest.mark.parametrize("batch", [1, 16])
def test_aimed_fallback_through_the_loops(gpu, orc, names, kind, batch):
    """The Lambertian fall-back inside bounce_kernel (shade_hit / shade_record), bounce_binned_kernel and the refill loop's shade_rays_kernel:
    helpers.fallback_wall puts a wall with normal -rb(P, F) in front of the camera, so pixel P's first hit at frame F takes the fall-back
    (proved on the oracle's stages by test_shade_edges_host.test_wall_pixel_takes_the_fallback_at_its_frame); three samples (F = 2 is the
    second) are rendered and table, totals and image compared with the oracle, all finite. A sphere placed so that P's jittered primary ray
    meets it where the normal is -rb was not built: the sphere fall-back is covered by the stage API only
    (test_edge_rays_through_shade_and_miss)."""
    from test_shade_edges_host import WALL_FRAME, WALL_H, WALL_PIXEL, WALL_W, wall_oracle
    W = gpu
    tris, mt, o = wall_oracle(orc, max_wavefronts=4)
    _, _, pos, at = fallback_wall(orc, WALL_W, WALL_H, WALL_PIXEL, WALL_FRAME)
    cc = W.CameraController(W.Camera(pos, at), 60.0, 0.0, 10.0, 0.1, 100.0)
    scene = W.Scene(np.zeros(0, W.SPHERE), mt.view(W.MATERIAL), triangles=tris.view(W.TRIANGLE).copy())
    pt = W.PathTracer(scene, W.RenderParameters(cc, (WALL_W, WALL_H)), rng_mode=W.RNG_PIXEL, max_wavefronts=4, flags=loop_flags(W, names), batch=batch)
    if kind:
        assert pt.loop_kind == kind
    want = o.render(3)
    pt.render(3)
    assert not np.isnan(want).any()
    assert np.array_equal(pt.bounce_table(), o.bounce_table()) and np.array_equal(pt.totals(), o.totals())
    assert_bit_equal(pt.accumulated(), want, f"wall {names} batch {batch}")
    pt.close(); o.close()


@pytest.mark.parametrize("flags", ["0", "NO_LDS_SCENE", "UNFUSED"])
def test_zero_and_negative_radius(gpu, orc, flags):
    """wfpt_create accepts radius 0 and a negative radius and the device does with them what the reference's text does (include/wfpt.h,
    test_shade_edges_host.test_zero_and_negative_radius_in_the_oracle): rays aimed at both through extend, shade and miss, and a render of
    the zoo that holds them, against the oracle."""
    W = gpu
    w, h = 128, 64
    sp, mt, o, pt = zoo_pair(W, orc, w, h, True, True, rng_mode=W.RNG_PIXEL, max_wavefronts=6, flags=getattr(W, "FLAG_" + flags, 0))
    rays = degenerate_radius_rays(W, sp)
    pt.set_frame(W.GPUFrameBuffer.new(w, h, 1)); o.set_frame(1, 0)
    maybe_nan = np.zeros(w * h, bool)
    maybe_nan[3 * len(rays) // 4:len(rays)] = True  # aimed at the sphere of radius 0: a hit is at its centre, the normal 0 * inf
    run_chain(W, orc, pt, o, rays, maybe_nan, [pt.shade_kernel])
    pt.reset_progress(); o.reset_accumulated()
    want = o.render(2)  # the oracle's progress starts at frame 1 as well: the stage calls above do not advance it
    pt.render(2)
    maybe = np.isnan(want).any(axis=1)
    assert np.array_equal(pt.bounce_table(), o.bounce_table())
    fenced_equal(pt.accumulated(), want, maybe, f"zoo with radius 0 and -0.4, {flags}")
    pt.close(); o.close()
