"""CPU half of tests/test_gpu_shade_edges.py: the hand-made rays and scenes of helpers.py run through the ORACLE's extend -> shade -> miss, and
the conditions that make the GPU comparison mean something are asserted from the oracle's outputs alone: every ray of a hit class hits the
sphere it was built for, every class is populated, the aimed Lambertian fall-back is taken and not taken, refract()'s k and the grazing
cos_theta take both signs, finite classes hold no NaN, and may-be-NaN classes are at most a quarter. The counts are conditions, not measurements."""
import numpy as np
import pytest

import helpers as H

W_, H_ = 128, 64
FLOOR = 20


class _Layouts:  # shade_edge_rays only needs the RAY layout, which oracle and product share
    def __init__(self, orc):
        self.RAY = orc.RAY


def zoo_oracle(orc, rng_mode, with_nan=True, **kw):
    sp, mt = H.material_zoo(orc, with_nan)
    spo, nodes = orc.build_bvh(sp)
    cam, ip, vw = orc.camera((0.0, 0.5, 12.0), (0.0, 0.0, 0.0), 60.0, 0.0, 10.0, 0.1, 100.0, W_, H_)
    return sp, mt, spo, orc.Oracle(W_, H_, spo, mt, nodes, cam, ip, vw, rng_mode=rng_mode, **kw)


def test_assert_bits_or_nan_is_fenced():
    a = np.array([1.0, np.nan, -0.0], "<f4")
    b = a.copy()
    b.view(np.uint32)[1] ^= 0x80000001  # another NaN: sign and payload differ
    H.assert_bits_or_nan(a, b, "two NaNs")
    for bad in (np.array([1.0, 2.0, -0.0], "<f4"), np.array([1.0, np.nan, 0.0], "<f4"), np.array([np.nan, np.nan, -0.0], "<f4")):
        with pytest.raises(AssertionError):
            H.assert_bits_or_nan(a, bad, "NaN against a number, -0 against +0, a number against NaN")


def test_probe_shade_rb_is_shades_first_draw(orc):
    """The probe against orc_shade itself: a metal of fuzz 1 hit head-on leaves reflect(d, n) + rb in the extension ray."""
    sp, mt, spo, o = zoo_oracle(orc, orc.RNG_PIXEL)
    k = H.ZOO_NAMES.index("metal-fuzz1")
    rays = np.zeros(64, orc.RAY)
    rays["origin"][:] = (sp["center"][k, 0], 0.0, sp["center"][k, 2] + 2.0, 1.0)
    rays["direction"][:, 2] = -1.0
    with np.errstate(divide="ignore"):
        rays["inv_direction"] = np.float32(1.0) / rays["direction"][:, :3]
    rays["pixel_idx"] = np.arange(64) * 37
    o.set_frame(3, 0); o.reset_image(); o.write_rays(rays); o.set_counters([0, 0, 64])
    o.extend(1, 1)
    assert int(o.counters()[1]) == 64
    o.set_counters([0, 64, 0])
    o.shade(1, 1)
    ext = o.extension_rays(64)["direction"][:, :3]
    for i in (0, 5, 63):
        px = int(rays["pixel_idx"][i])
        rb = orc.probe_shade_rb(px % W_, px // W_, W_, 3, 0)
        assert np.array_equal(ext[i], (np.float32([0, 0, 1]) + np.float32(1.0) * rb).astype("<f4"))  # reflect((0,0,-1), (0,0,1)) = (0,0,1)


@pytest.mark.parametrize("rng_mode", [0, 1])
def test_edge_rays_meet_their_conditions(orc, rng_mode):
    sp, mt, spo, o = zoo_oracle(orc, rng_mode)
    rays, cls, target, maybe_nan = H.shade_edge_rays(_Layouts(orc), sp, mt, W_, H_, 1, rng_mode, orc)
    n = len(rays)
    assert len(np.unique(rays["pixel_idx"])) == n and (rays["origin"][:, 3] == 1).all() and (rays["direction"][:, 3] == 0).all()
    assert maybe_nan.mean() <= 0.25
    for name in H.EDGE_CLASSES:
        assert (cls == name).sum() >= FLOOR, name
    o.set_frame(1, 0); o.reset_image(); o.write_rays(rays); o.set_counters([0, 0, n])
    o.extend(*orc.workgroup_size_64(n))
    c = o.counters()
    n_hit, n_miss = int(c[1]), int(c[0])
    hits = o.hits(n_hit)
    got = np.full(n, -1)
    got[hits["ray_idx"]] = H.zoo_index_of(spo, sp)[hits["sphere_idx"]]
    wrong = np.flatnonzero(got != target)
    assert len(wrong) == 0, f"rays that do not meet their sphere: {[(i, cls[i]) for i in wrong[:8]]}"
    assert n_hit == (target >= 0).sum() and np.array_equal(hits["ray_idx"], np.arange(n_hit))  # hit index == ray index: the dispatch-keyed aim holds
    # what scatter() will see, from the oracle's queues
    nrm, uv, cos_theta, k = H.scatter_terms(o.rays(n), hits, spo, mt)
    hc = cls[hits["ray_idx"]]
    glass = hits["mat_type"] == 2
    kc = k[hc == "critical"]
    assert ((kc >= 0) & (np.abs(kc) < 1e-6)).sum() >= FLOOR and ((kc < 0) & (np.abs(kc) < 1e-6)).sum() >= FLOOR
    graze = glass & np.isin(hc, ["grazing_outside", "grazing_inside"])
    assert (cos_theta[graze] >= 0).sum() >= FLOOR and (cos_theta[graze] < 0).sum() >= FLOOR
    assert (np.abs(cos_theta[graze]) < 0.04).all()
    assert (cos_theta[glass & (hc == "head_on")] > 1).sum() >= FLOOR  # the clamp min(dot, 1) has work to do
    c[2] = 0
    o.set_counters(c)
    o.shade(*orc.workgroup_size_64(n_hit))
    ext = o.extension_rays(n_hit)
    took = (ext["direction"][:, :3].view(np.uint32) == nrm.view(np.uint32)).all(axis=1)
    fb = hc == "fallback"
    assert (took & fb).sum() >= FLOOR and (fb & ~took).sum() >= FLOOR and not (took & ~fb).any()
    lens = np.sqrt((ext["direction"][fb & ~took, :3].astype(np.float64) ** 2).sum(axis=1))
    assert (lens < 0.0015).sum() >= FLOOR  # aimed rays that stay just outside the threshold, not only far ones
    o.miss(*orc.workgroup_size_64(n_miss))
    finite_hit = ~maybe_nan[hits["ray_idx"]]
    assert not np.isnan(H.ray_floats(ext)[finite_hit]).any()
    assert not np.isnan(o.image()[:n][~maybe_nan]).any()
    o.close()


@pytest.mark.parametrize("scene", ["closed-metal", "closed-glass", "centre"])
def test_closed_rooms_have_no_misses(orc, scene):
    """A camera inside a closed sphere: no ray ever misses, so `misses < miss_floor` fires at wavefront 0 and with miss_floor 0 every
    wavefront runs full."""
    inputs = H.closed_room_inputs(orc, scene, 64, 40)
    o = H.make_oracle(orc, inputs, 64, 40, max_wavefronts=3, miss_floor=0)
    o.render(1)
    t = o.bounce_table()
    assert len(t) == 3 and (t[:, 2] == 0).all() and (t[:, 0] == 64 * 40).all() and (t[:, 1] == 64 * 40).all()
    assert not np.isnan(o.accumulated()).any()
    o.close()
    o = H.make_oracle(orc, inputs, 64, 40, max_wavefronts=3, miss_floor=128)
    o.render(2)
    assert len(o.bounce_table()) == 1 and (o.accumulated() == 2.0).all()
    o.close()


@pytest.mark.parametrize("with_nan", [False, True])
def test_zoo_renders_meet_the_nan_fence(orc, with_nan):
    sp, mt, spo, o = zoo_oracle(orc, orc.RNG_PIXEL, with_nan, max_wavefronts=8)
    img = o.render(2)
    frac = np.isnan(img).any(axis=1).mean()
    assert frac == 0 if not with_nan else frac <= 0.25
    t = o.bounce_table()
    assert t[0, 1] > 1000 and t[0, 2] > 500  # the camera sees the zoo and, between floor and ceiling, the sky
    o.close()


@pytest.mark.parametrize("rng_mode", [0, 1])
def test_edge_mesh_meets_its_conditions(orc, rng_mode):
    """The mesh variant: every ray hits its own triangle, the ulp-sized grazing tilts give dot(n, -uv) of both signs within 64 ulp-sized
    steps of 0 (|cos_theta| <= 64 * 2^-23), k takes both signs within 1e-6 of 0, the aimed fall-back is taken and not taken."""
    tris, mt, rays, cls, maybe_nan = H.shade_edge_mesh(_Layouts(orc), orc, W_, H_, 1, rng_mode)
    n = len(rays)
    assert maybe_nan.mean() <= 0.25 and len(np.unique(rays["pixel_idx"])) == n
    for name in H.MESH_CLASSES:
        assert (cls == name).sum() >= FLOOR, name
    tb, nodes = orc.build_bvh_triangles(tris, 32)
    cam, ip, vw = orc.mesh_camera(W_, H_)
    o = H.make_mesh_oracle(orc, (tb, mt, nodes, cam, ip, vw), W_, H_, rng_mode=rng_mode)
    o.set_frame(1, 0); o.reset_image(); o.write_rays(rays); o.set_counters([0, 0, n])
    o.extend(*orc.workgroup_size_64(n))
    c = o.counters()
    assert int(c[1]) == n and int(c[0]) == 0
    hits = o.hits(n)
    assert np.array_equal(hits["ray_idx"], np.arange(n)) and np.array_equal(H.mesh_index_of(tb, tris)[hits["sphere_idx"]], np.arange(n))
    nrm, uv, cos_theta, k = H.scatter_terms(o.rays(n), hits, None, mt, triangles=tb)
    g = cls == "grazing_ulp"
    assert (hits["mat_type"][g] == 2).all()
    assert (cos_theta[g] > 0).sum() >= FLOOR and (cos_theta[g] < 0).sum() >= FLOOR and (np.abs(cos_theta[g]) < 65 * 2.0 ** -23).all()
    for ulps in H.GRAZING_ULPS:  # each tilt size, from above and from below
        for sign in (1.0, -1.0):  # normalising the direction costs the tilt an ulp of its own value at most
            assert (np.abs(cos_theta[g] / np.float32(sign * ulps * 2.0 ** -23) - 1.0) < 1e-6).sum() >= 6
    kc = k[cls == "critical"]
    assert ((kc >= 0) & (np.abs(kc) < 1e-6)).sum() >= FLOOR and ((kc < 0) & (np.abs(kc) < 1e-6)).sum() >= FLOOR
    c[2] = 0
    o.set_counters(c)
    o.shade(*orc.workgroup_size_64(n))
    ext = o.extension_rays(n)
    took = (ext["direction"][:, :3].view(np.uint32) == nrm.view(np.uint32)).all(axis=1) & (hits["mat_type"] == 0)
    fb = cls == "fallback"
    assert (took & fb).sum() >= FLOOR and (fb & ~took).sum() >= FLOOR and not (took & ~fb).any()
    assert not np.isnan(H.ray_floats(ext)[~maybe_nan]).any()
    o.close()


WALL_PIXEL, WALL_FRAME, WALL_W, WALL_H = 37 * 96 + 41, 2, 96, 64


def wall_oracle(orc, **kw):
    tris, mt, pos, at = H.fallback_wall(orc, WALL_W, WALL_H, WALL_PIXEL, WALL_FRAME)
    tb, nodes = orc.build_bvh_triangles(tris, 32)
    cam, ip, vw = orc.camera(pos, at, 60.0, 0.0, 10.0, 0.1, 100.0, WALL_W, WALL_H)
    return tris, mt, H.make_mesh_oracle(orc, (tb, mt, nodes, cam, ip, vw), WALL_W, WALL_H, rng_mode=orc.RNG_PIXEL, **kw)


def test_wall_pixel_takes_the_fallback_at_its_frame(orc):
    """The proof behind test_aimed_fallback_through_the_loops: with the oracle's stages at frame WALL_FRAME every primary ray hits the wall and
    pixel WALL_PIXEL's extension ray is the normal bit for bit (the fall-back); at the other frames of the render it is not."""
    tris, mt, o = wall_oracle(orc)
    n = WALL_W * WALL_H
    for frame in (1, 2, 3):
        o.set_frame(frame, 0); o.reset_image(); o.set_counters([0, 0, n])
        o.generate_rays(WALL_W // 8, WALL_H // 8, False)
        o.extend(*orc.workgroup_size_64(n))
        c = o.counters()
        assert int(c[1]) == n
        hits = o.hits(n)
        nrm = H.scatter_terms(o.rays(n), hits, None, mt, triangles=orc.build_bvh_triangles(tris, 32)[0])[0]
        c[2] = 0
        o.set_counters(c)
        o.shade(*orc.workgroup_size_64(n))
        ext = o.extension_rays(n)
        took = (ext["direction"][:, :3].view(np.uint32) == nrm.view(np.uint32)).all(axis=1)
        at_pixel = ext["pixel_idx"] == WALL_PIXEL
        assert at_pixel.sum() == 1
        assert bool(took[at_pixel][0]) == (frame == WALL_FRAME), frame
    o.close()


def test_zero_and_negative_radius_in_the_oracle(orc):
    """What the reference's text does with them, as the oracle restates it: extend.wgsl:193 squares the radius and shade.wgsl:93 normalises
    p - centre without dividing by the radius, so a negative radius is the sphere of |radius| with an OUTWARD normal (not Shirley's hollow
    sphere); sphere.rs:23-24 gives it an inverted box, which the slab test (per-axis min / max of the two plane distances) reads like the
    proper one, but which does not widen its ancestors' boxes. Radius 0: the discriminant b b - a c is >= 0 only by rounding."""
    sp, mt = H.material_zoo(orc, True, degenerate_radii=True)
    spo, nodes = orc.build_bvh(sp)
    cam, ip, vw = orc.camera((0.0, 0.5, 12.0), (0.0, 0.0, 0.0), 60.0, 0.0, 10.0, 0.1, 100.0, W_, H_)
    o = orc.Oracle(W_, H_, spo, mt, nodes, cam, ip, vw)
    rays = H.degenerate_radius_rays(_Layouts(orc), sp)
    n = len(rays)
    o.set_frame(1, 0); o.write_rays(rays); o.set_counters([0, 0, n])
    o.extend(*orc.workgroup_size_64(n))
    hits = o.hits(int(o.counters()[1]))
    created = H.zoo_index_of(spo, sp)[hits["sphere_idx"]]
    neg, zero = len(sp) - 2, len(sp) - 1
    inside = hits["ray_idx"] < 3 * n // 4      # the first three quarters start inside the glass sphere, between radius 0.4 and 0.5
    assert (created[inside] == neg).sum() >= FLOOR, "the negative-radius sphere is hit like the sphere of |radius|"
    t = hits["t"][inside & (created == neg)]
    assert (np.abs(t - 0.05) < 1e-3).all()     # at distance 0.45 - 0.4 from the start
    assert (created == zero).sum() <= n // 8   # radius 0: a hit needs a discriminant of exactly 0
    o.close()
