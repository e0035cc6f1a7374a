"""First-hit AOVs (WFPT_FLAG_AOV, include/wfpt.h "AOVs") on the GPU.

The expected values are restated in numpy float32 from the oracle's own primary wavefronts, sample by sample, exactly as
orc_render_sample starts one: frame f, counters [0, 0, rays], generate_rays with the true-size rule, one extend. The
restatement follows the kernel's operation order (p = o + t d, normalize as v * (1 / sqrt(dot)), the sky colour of
miss_kernel, sums in ascending sample order), so every AOV is compared bit for bit.
"""
import numpy as np
import pytest

from helpers import inputs_for, make_mesh_oracle, make_mesh_tracer, make_oracle, make_tracer, mesh_inputs

pytestmark = pytest.mark.gpu

F = np.float32
MISS = 0xFFFFFFFF
NAMES = ("albedo", "normal", "depth", "coverage", "prim_id", "material_id")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_bits(got, want, what):
    g, w = bits(got), bits(np.asarray(want, got.dtype))
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = g != w
    if bad.ndim == 3:
        bad = bad.any(axis=2)
    assert not bad.any(), f"{what}: {int(bad.sum())} pixels differ, first at {np.argwhere(bad)[0]}: {got[tuple(np.argwhere(bad)[0])]} " \
                          f"vs {np.asarray(want)[tuple(np.argwhere(bad)[0])]}"


def normalize(v):
    inv = F(1.0) / np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    return v * inv[:, None]


def expected_aovs(O, o, w, h, n, prims, materials, triangles=False):
    """The resolved AOVs of n samples (frames 1 .. n) restated from the oracle's primary wavefronts."""
    gx, gy = (w + 7) // 8, (h + 7) // 8
    n_rays = gx * gy * 64
    ex = O.workgroup_size_64(n_rays)
    px_n = w * h
    alb, nrm = np.zeros((px_n, 3), F), np.zeros((px_n, 3), F)
    depth, hits = np.zeros(px_n, F), np.zeros(px_n, np.uint32)
    prim_id, mat_id = np.full(px_n, MISS, np.uint32), np.full(px_n, MISS, np.uint32)
    if triangles:
        e1, e2 = prims["e1"].astype(F), prims["e2"].astype(F)
        cr = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                       e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
        tri_normal = normalize(cr)
    for f in range(1, n + 1):
        o.set_frame(f, 0)
        o.set_counters([0, 0, n_rays])
        o.generate_rays(gx, gy, True)
        o.extend(*ex)
        c = o.counters()
        rays = o.rays(n_rays)
        hit = o.hits(int(c[1]))
        miss = o.misses(int(c[0]))
        # per pixel this sample: a hit or a miss (padding rays are neither)
        s_alb, s_nrm = np.zeros((px_n, 3), F), np.zeros((px_n, 3), F)
        s_t, s_hit = np.zeros(px_n, F), np.zeros(px_n, bool)
        s_prim = np.full(px_n, MISS, np.uint32)
        r = rays[hit["ray_idx"]]
        pix = r["pixel_idx"].astype(np.int64)
        t = hit["t"].astype(F)
        prim = hit["sphere_idx"].astype(np.int64)
        mat = (prims["material_idx"][prim]).astype(np.int64)
        s_alb[pix] = materials["albedo"][mat, :3].astype(F)
        if triangles:
            s_nrm[pix] = tri_normal[prim]
        else:
            o3, d3 = r["origin"][:, :3].astype(F), r["direction"][:, :3].astype(F)
            p = o3 + t[:, None] * d3
            s_nrm[pix] = normalize(p - prims["center"][prim, :3].astype(F))
        s_t[pix] = t
        s_hit[pix] = True
        s_prim[pix] = prim.astype(np.uint32)
        mr = rays[miss]
        mpix = mr["pixel_idx"].astype(np.int64)
        a = F(0.5) * (mr["direction"][:, 1].astype(F) + F(1.0))
        om = F(1.0) - a
        s_alb[mpix] = np.stack([om * F(1.0) + a * F(0.5), om * F(1.0) + a * F(0.7), om * F(1.0) + a * F(1.0)], axis=1)
        assert len(pix) + len(mpix) == px_n and not np.intersect1d(pix, mpix).size
        alb += s_alb
        nrm += s_nrm
        depth = np.where(s_hit, depth + s_t, depth)
        hits += s_hit.astype(np.uint32)
        if f == 1:
            prim_id = s_prim
            mat_id = np.where(s_hit, prims["material_idx"][np.where(s_hit, s_prim, 0)].astype(np.uint32), np.uint32(MISS))
    nf = F(n)
    out = {"albedo": alb / nf, "normal": nrm / nf,
           "depth": np.where(hits > 0, depth / np.maximum(hits, 1).astype(F), F(0)).astype(F),
           "coverage": hits.astype(F) / nf, "prim_id": prim_id, "material_id": mat_id}
    return {k: (v.reshape(h, w, 3) if v.ndim == 2 else v.reshape(h, w)) for k, v in out.items()}


def product_aovs(pt):
    return {k: pt.aov(k) for k in NAMES}


def assert_aovs(got, want, what):
    for k in NAMES:
        assert_bits(got[k], want[k], f"{what}: {k}")


@pytest.mark.parametrize("w,h", [(400, 225), (64, 64)])
@pytest.mark.parametrize("rng_mode", [0, 1])
@pytest.mark.parametrize("batch", [1, 2])
def test_shirley_aovs_match_the_oracle_primary_wavefronts(gpu, orc, w, h, rng_mode, batch):
    W = gpu
    spp = 3
    inputs = inputs_for(orc, "shirley", w, h)
    o = make_oracle(orc, inputs, w, h, rng_mode=rng_mode)
    want = expected_aovs(orc, o, w, h, spp, inputs[0], inputs[1])
    pt = make_tracer(W, "shirley", w, h, rng_mode=rng_mode, max_wavefronts=4, batch=batch, flags=W.FLAG_AOV)
    pt.render(spp)
    assert W.lib().wfpt_accumulated_samples(pt.handle) == spp
    got = product_aovs(pt)
    assert_aovs(got, want, f"shirley {w}x{h} rng {rng_mode} batch {batch}")
    assert got["coverage"].max() == 1.0
    pt.close(); o.close()


@pytest.mark.parametrize("flags", [0, "NO_REFILL", "BINARY_BVH", "EXACT_TRAVERSAL"])
def test_mesh_aovs_beyond_lds_match_the_oracle(gpu, orc, flags):
    """A random mesh too large for LDS: the refill loop (four-wide walk in the AOV pass), the fused bounce loop over HBM, the binary tree
    and the reference's exact walk. Triangle normals are the stored normalize(cross(e1, e2)), restated in the same order: bit-equal."""
    W = gpu
    w, h, n_tri, spp = 128, 96, 20000, 2
    fl = W.FLAG_AOV | (getattr(W, "FLAG_" + flags) if flags else 0)
    inputs = mesh_inputs(orc, w, h, n_tri, edge_scale=5.0)
    o = make_mesh_oracle(orc, inputs, w, h)
    want = expected_aovs(orc, o, w, h, spp, inputs[0], inputs[1], triangles=True)
    pt = make_mesh_tracer(W, w, h, n_tri, edge_scale=5.0, max_wavefronts=3, flags=fl)
    if flags == 0:
        assert pt.loop_kind == "refill"
    pt.render(spp)
    got = product_aovs(pt)
    assert_aovs(got, want, f"mesh {flags or 'default'}")
    assert 0.0 < got["coverage"].mean() < 1.0
    pt.close(); o.close()


def render_aovs(W, w, h, spp, **kw):
    pt = make_tracer(W, "shirley", w, h, max_wavefronts=4, **kw)
    pt.render(spp)
    out = (product_aovs(pt) if kw.get("flags", 0) & W.FLAG_AOV else None), pt.accumulated(), pt.bounce_table()
    pt.close()
    return out


def test_aovs_are_the_same_for_every_loop_and_batch(gpu):
    W = gpu
    w, h, spp = 100, 60, 20  # partial tiles in x and y; batches of 16 leave a remainder
    for rng_mode in (0, 1):
        ref, _, _ = render_aovs(W, w, h, spp, rng_mode=rng_mode, flags=W.FLAG_AOV)
        variants = [("UNFUSED", 0), ("SPLIT_SHADE", 0), ("NO_GRAPH", 0), ("EXACT_TRAVERSAL", 0), ("NO_LDS_SCENE", 0), (None, 1), (None, 16),
                    (None, 64)]
        if rng_mode == 1:
            variants.append(("BINNING", 0))
        for flag, batch in variants:
            fl = W.FLAG_AOV | (getattr(W, "FLAG_" + flag) if flag else 0)
            got, _, _ = render_aovs(W, w, h, spp, rng_mode=rng_mode, flags=fl, batch=batch)
            assert_aovs(got, ref, f"rng {rng_mode} flag {flag} batch {batch}")


def test_band_sharded_aovs_reassemble_to_the_whole_image(gpu):
    W = gpu
    w, h, spp, world = 96, 100, 3, 3
    ref, _, _ = render_aovs(W, w, h, spp, rng_mode=1, flags=W.FLAG_AOV)
    for name in NAMES:
        whole = np.zeros_like(ref[name])
        whole[...] = 0xAB if whole.dtype == np.uint32 else np.nan
        for rank in range(world):
            pt = make_tracer(W, "shirley", w, h, max_wavefronts=4, rng_mode=1, flags=W.FLAG_AOV, tile_rank=rank, tile_world=world)
            pt.render(spp)
            slab = pt.aov(name)
            for j in range(slab.shape[0] // 8):
                y0 = (j * world + rank) * 8
                rows = min(8, h - y0)
                whole[y0:y0 + rows] = slab[8 * j:8 * j + rows]
            pt.close()
        assert_bits(whole, ref[name], f"sharded {name}")


def test_aov_context_renders_the_same_image(gpu):
    """The AOV pass only reads the scene and writes its own sums: the beauty image and the bounce table do not change."""
    W = gpu
    for flags in (0, W.FLAG_UNFUSED):
        _, acc0, tab0 = render_aovs(W, 200, 120, 4, flags=flags)
        _, acc1, tab1 = render_aovs(W, 200, 120, 4, flags=flags | W.FLAG_AOV)
        assert_bits(acc1, acc0, f"accumulated, flags {flags}")
        assert np.array_equal(tab0, tab1)


def test_aov_ids_and_depth_match_the_stage_api_extend(gpu):
    """One sample's prim ids and depth against the same context's own stage-by-stage extend of that frame (64x64: the stage API's
    generate_rays covers 8 gx x 8 gy pixels, the true size here)."""
    W = gpu
    w, h = 64, 64
    pt = make_tracer(W, "shirley", w, h, max_wavefronts=4, flags=W.FLAG_AOV)
    pt.render(1)
    prim_id, depth = pt.aov("prim_id").reshape(-1), pt.aov("depth").reshape(-1)
    n = w * h
    pt.set_frame(W.GPUFrameBuffer.new(w, h, 1))
    pt.set_counters([0, 0, n])
    pt.generate_ray_kernel.run((w // 8, h // 8))
    pt.extend_kernel.run(W.workgroup_size_64(n))
    c = pt.read_counters()
    hits = pt.hits(int(c[1]))
    pix = pt.rays(n)["pixel_idx"][hits["ray_idx"]]
    want_prim = np.full(n, MISS, np.uint32)
    want_prim[pix] = hits["sphere_idx"]
    want_depth = np.zeros(n, F)
    want_depth[pix] = hits["t"]
    assert int(c[0]) + int(c[1]) == n and int(c[1]) > 0
    assert np.array_equal(prim_id, want_prim)
    assert_bits(depth, want_depth, "depth of one sample")
    pt.close()


def test_resets_and_errors(gpu):
    W = gpu
    pt = make_tracer(W, "shirley", 64, 48, max_wavefronts=3, flags=W.FLAG_AOV)
    pt.render(2)
    assert pt.aov("coverage").max() > 0 and pt.aov("albedo").max() > 0
    before = product_aovs(pt)
    W.lib().wfpt_reset_progress(pt.handle)
    for k in ("albedo", "normal", "depth", "coverage"):
        assert not bits(pt.aov(k)).any(), k  # n = 0: zeros
    assert (pt.aov("prim_id") == MISS).all() and (pt.aov("material_id") == MISS).all()
    pt.render(2)  # frames 1, 2 again: the same sums as before the reset
    assert_aovs(product_aovs(pt), before, "after wfpt_reset_progress")
    W.lib().wfpt_reset_accumulated(pt.handle)  # zeroes the sums (the sample count is the host's: unchanged)
    assert not bits(pt.aov("albedo")).any() and (pt.aov("prim_id") == MISS).all()
    # a viewport change zeroes them too
    pt.render(1)
    rp = pt.get_render_parameters()
    rp.set_viewport((40, 32))
    pt.update_render_parameters(rp)
    pt.update_buffers()
    assert pt.aov("albedo").shape == (32, 40, 3) and not bits(pt.aov("albedo")).any()
    ms, launches = pt.aov_timing()
    assert launches == 0
    pt.render_timed(3)
    ms, launches = pt.aov_timing()
    assert launches >= 1 and ms > 0.0
    # errors: an unknown AOV, a context without the flag
    L = W.lib()
    buf = np.zeros(64 * 48 * 3, "<f4")
    assert L.wfpt_read_aov(pt.handle, 6, W._p(buf), 10) == -1 and b"unknown AOV" in L.wfpt_last_error(pt.handle)
    assert L.wfpt_read_aov(pt.handle, -1, W._p(buf), 10) == -1
    assert L.wfpt_read_aov(pt.handle, 0, W._p(buf), 10 ** 9) == -1
    with pytest.raises(ValueError):
        pt.aov("velocity")
    pt.close()
    plain = make_tracer(W, "shirley", 64, 48, max_wavefronts=3)
    plain.render(1)
    with pytest.raises(W.WfptError, match="WFPT_FLAG_AOV"):
        plain.aov("albedo")
    assert L.wfpt_copy_aov_to_device(plain.handle, 0, W._p(buf), 4) == -1
    assert L.wfpt_aov_timing_ms(plain.handle, None, None) == -1
    plain.close()


def test_aov_to_tensor_gives_the_same_bits(gpu):
    torch = pytest.importorskip("torch")
    W = gpu
    pt = make_tracer(W, "shirley", 100, 60, max_wavefronts=3, flags=W.FLAG_AOV)
    pt.render(3)
    for k in NAMES:
        host = pt.aov(k)
        dt = torch.float32 if host.dtype == np.float32 else torch.int32
        t = torch.full(host.shape, -7, dtype=dt, device="cuda:0")
        pt.aov_to_tensor(k, t)
        got = t.cpu().numpy()
        assert np.array_equal(got.view(np.uint32), host.view(np.uint32)), k
    with pytest.raises(TypeError):
        pt.aov_to_tensor("albedo", torch.zeros((60, 100, 3), dtype=torch.float64, device="cuda:0"))
    with pytest.raises(ValueError):
        pt.aov_to_tensor("albedo", torch.zeros((60, 100), dtype=torch.float32, device="cuda:0"))
    with pytest.raises(ValueError):
        pt.aov_to_tensor("albedo", torch.zeros((100, 60, 3), dtype=torch.float32, device="cuda:0").transpose(0, 1))
    pt.close()
