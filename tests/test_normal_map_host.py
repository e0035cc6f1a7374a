"""Tangent-space normal maps (WFPT_FLAG_NORMAL_MAPS, include/wfpt.h "Normal maps") without a GPU: wfpt_mapped_normal_host -- steps B-F
compiled from the function the kernels call -- against the restatement (tests/normal_map_ref.py) bit for bit; the tangent against the
closed form on a sphere; the identity, unit-length and mirrored-UV properties; whole frames through the oracle against four mutations and
the flat map; the flag's create-time rules on device -1; the bench tool's legs and fields."""
import json
import os
import sys

import numpy as np
import pytest

import normal_map_ref as NM
import shading_normals_ref as S
import transport_ref
from conftest import assert_bit_equal
from helpers import assert_bits_or_nan
from test_ab_bench_host import COMMON_KEYS, ROOT, ab, load  # noqa: F401  (ab: the fixture)
from test_microfacet_host import create_message

F = np.float32
W_, H_, SPP, WAVES = 61, 37, 3, 4
SLOT = 1
BIND = {m: (SLOT, 1.0) for m in range(4)}


def built(orc):
    t, mt, n9, uv = NM.sphere_scene(orc)
    t, nodes = orc.build_bvh_triangles(t, 32)
    return t, mt, n9, uv, nodes


def oracle_of(orc, t, mt, nodes, **kw):
    cam, ip, vw = S.sphere_camera(orc, W_, H_)
    return orc.Oracle(W_, H_, np.zeros(1, orc.SPHERE), mt, nodes, cam, ip, vw, triangles=t, max_wavefronts=WAVES, **kw)


def scene_rows(orc, k, seed, strength, texel=None):
    """k uniformly drawn points on the scene's sphere: the inputs of steps B-F there (ng, ns, e1, e2, uv6, c, s) and the points"""
    t, mt, n9, uv = NM.sphere_scene(orc)
    rng = np.random.default_rng(seed)
    prim = rng.integers(0, 320, k)
    b = rng.dirichlet((1.0, 1.0, 1.0), k)
    tri = t[prim]
    p = (tri["v0"].astype(np.float64) + tri["e1"] * b[:, 1:2] + tri["e2"] * b[:, 2:3]).astype(F)
    ng = transport_ref.triangle_normal_area(tri)[0]
    ns = S.Normals(t, n9).at(prim, p)[0]
    rows = uv[tri["_pad"].astype(np.int64)]
    if texel is None:
        img = NM.tilt_map()
        c = img.reshape(-1, 3)[rng.integers(0, img.shape[0] * img.shape[1], k)]
    else:
        c = np.tile(np.asarray(texel, F), (k, 1))
    return (ng, ns, tri["e1"], tri["e2"], rows, c, np.full(k, strength, F)), p, prim


def test_the_scene_is_what_the_issue_says(orc):
    t, mt, n9, uv = NM.sphere_scene(orc)
    rows = uv[t["_pad"].astype(np.int64)].astype(np.float64)
    det = (rows[:, 2] - rows[:, 0]) * (rows[:, 5] - rows[:, 1]) - (rows[:, 4] - rows[:, 0]) * (rows[:, 3] - rows[:, 1])
    assert (det[:320] > 0).all(), "after the seam repair every sphere triangle has det > 0"
    assert det[320] > 0 and det[321] < 0, "the ground: planar UVs, then mirrored ones"
    for strength in (0.0, 1.0, 4.0):
        args, _, _ = scene_rows(orc, 20000, 6, strength)
        code = NM.mapped_normal(*args)[1]
        assert not np.isin(code, (2, 3)).any(), (strength, np.bincount(code))


# ---------------------------------------------------------------- bits
def edge_rows():
    """(args, may be NaN): det = 0, det < 0, equal UVs at all corners, T parallel to ns, a texel of (0.5, 0.5, 1), strength 0, z <= 0, NaN
    and inf in each input, a NaN ng"""
    rng = np.random.default_rng(9)
    k = 8

    def base():
        ng = np.tile((0.0, 0.0, 1.0), (k, 1)).astype(F)
        ns = (ng + 0.2 * rng.normal(size=(k, 3))).astype(F)
        ns /= np.linalg.norm(ns, axis=1)[:, None]
        e1 = np.tile((1.0, 0.0, 0.0), (k, 1)).astype(F) + (0.1 * rng.normal(size=(k, 3))).astype(F) * (1, 1, 0)
        e2 = np.tile((0.0, 1.0, 0.0), (k, 1)).astype(F) + (0.1 * rng.normal(size=(k, 3))).astype(F) * (1, 1, 0)
        uv = np.tile((0.0, 0.0, 1.0, 0.0, 0.0, 1.0), (k, 1)).astype(F) + (0.1 * rng.normal(size=(k, 6))).astype(F)
        c = (0.5 + 0.5 * rng.uniform(-0.6, 0.6, (k, 3))).astype(F)
        c[:, 2] = 0.9
        return [ng.astype(F), ns.astype(F), e1.astype(F), e2.astype(F), uv, c, np.ones(k, F)]

    parts, maybe, codes = [], [], []

    def add(a, nan=False, code=None):
        parts.append(a)
        maybe.append(np.full(k, nan))
        codes.append(code)

    a = base(); a[4][:, 2:4] = a[4][:, 4:6]; add(a, code=2)                      # det = 0: two corners share their UVs
    a = base(); a[4] = a[4][:, [0, 1, 4, 5, 2, 3]]; add(a, code=0)               # det < 0
    a = base(); a[4][:] = (0.25, 0.75) * 3; add(a, code=2)                       # equal UVs at all corners
    a = base(); a[4][:] = (0, 0, 1, 0, 0, 1); a[1][:] = (1, 0, 0); a[2][:] = (2, 0, 0); add(a, code=2)  # T = e1 parallel to ns: tt = 0
    a = base(); a[5][:] = (0.5, 0.5, 1.0); add(a, code=1)                        # a flat texel
    a = base(); a[6][:] = 0.0; add(a, code=1)                                    # strength 0
    a = base(); a[5][:, 2] = 0.5; a[1] = a[0].copy(); add(a, code=3)             # z = 0: m lies in the surface, dot(nm, ng) = 0
    a = base(); a[5][:, 2] = 0.1; a[1] = a[0].copy(); add(a, code=3)             # z < 0
    for slot in range(7):
        for bad in (np.nan, np.inf):
            a = base()
            if slot == 6:
                a[6][:] = bad
            else:
                a[slot][np.arange(k), np.arange(k) % a[slot].shape[1]] = bad
            add(a, nan=True)
    a = base(); a[0][:] = np.nan; add(a, nan=True, code=3)                       # a NaN ng: step F rejects, the answer is ns
    args = [np.concatenate([p[i] for p in parts]) for i in range(7)]
    return args, np.concatenate(maybe), codes, k


def test_host_function_equals_restatement_bit_for_bit(orc, wf):
    rng = np.random.default_rng(1)
    k = 3000
    ng = rng.normal(size=(k, 3)).astype(F)
    ng /= np.linalg.norm(ng, axis=1)[:, None]
    ns = (ng + 0.3 * rng.normal(size=(k, 3))).astype(F)
    ns /= np.linalg.norm(ns, axis=1)[:, None]
    random = [ng, ns, rng.normal(size=(k, 3)).astype(F), rng.normal(size=(k, 3)).astype(F), rng.uniform(-1, 2, (k, 6)).astype(F),
              rng.random((k, 3)).astype(F), rng.uniform(0, 4, k).astype(F)]
    parts = [random] + [list(scene_rows(orc, 1000, 20 + i, s)[0]) for i, s in enumerate((0.0, 1.0, 4.0))]
    args = [np.concatenate([p[i] for p in parts]) for i in range(7)]
    want, code = NM.mapped_normal(*args)
    assert len(want) >= 4000 and not np.isnan(want).any()
    assert (code == 0).sum() > 2000 and (code == 3).sum() > 500 and (code == 1).sum() >= 1000
    got = wf.mapped_normal_host(NM.host_rows(*args))
    assert_bit_equal(got[:, :3], want, "random and scene rows")
    assert np.array_equal(got[:, 3], code.astype(F))
    eargs, maybe, codes, k = edge_rows()
    want, code = NM.mapped_normal(*eargs)
    got = wf.mapped_normal_host(NM.host_rows(*eargs))
    assert_bits_or_nan(got[:, :3], want, "edge rows")
    assert np.array_equal(got[:, 3], code.astype(F)), "edge rows' codes"
    assert not np.isnan(want[~maybe]).any()
    for i, c in enumerate(codes):
        if c is not None:
            assert (code[i * k:(i + 1) * k] == c).all(), (i, c, code[i * k:(i + 1) * k])
    ident = np.concatenate([np.arange(4 * k, 6 * k)])
    assert_bit_equal(want[ident], eargs[1][ident], "the identity answers ns bit for bit")
    assert len(wf.mapped_normal_host(np.zeros((0, 22), F))) == 0
    with pytest.raises(ValueError):
        wf.mapped_normal_host(np.zeros((3, 21), F))


# ---------------------------------------------------------------- closed form and properties
def test_tangent_against_the_closed_form_on_a_sphere(orc):
    """texel (0.8, 0.5, 0.9): m = t x + ns z, so t is the part of the answer orthogonal to ns; the analytic dP/du of the spherical
    parameterisation is (-sin phi, 0, -cos phi) with phi = atan2(-z, x). Per-triangle tangents are off near the poles only."""
    args, p, prim = scene_rows(orc, 20000, 3, 1.0, texel=(0.8, 0.5, 0.9))
    n, code = NM.mapped_normal(*args)
    assert (code == 0).all()
    ns, n, p = args[1].astype(np.float64), n.astype(np.float64), p.astype(np.float64)
    t = n - ns * np.einsum("ij,ij->i", n, ns)[:, None]
    t /= np.linalg.norm(t, axis=1)[:, None]
    phi = np.arctan2(-p[:, 2], p[:, 0])
    want = np.stack([-np.sin(phi), np.zeros_like(phi), -np.cos(phi)], 1)
    cos = np.einsum("ij,ij->i", t, want)
    share = float((cos < 0.9).mean())
    print(f"closed form: median cosine {np.median(cos):.5f}, share below 0.9 {100 * share:.2f} %")
    assert np.median(cos) >= 0.999
    assert share <= 0.02


def test_identity_unit_length_and_mirrored_uvs(orc):
    for strength, texel in ((0.0, None), (1.0, (0.5, 0.5, 1.0)), (4.0, (0.5, 0.5, 0.75))):
        args, _, _ = scene_rows(orc, 2000, 5, strength, texel=texel)
        n, code = NM.mapped_normal(*args)
        assert (code == 1).all()
        assert_bit_equal(n, args[1], f"strength {strength}, texel {texel}: ns bit for bit")
    for strength in (1.0, 4.0):
        args, _, _ = scene_rows(orc, 5000, 7, strength)
        n, code = NM.mapped_normal(*args)
        assert (code == 0).all()
        length = np.linalg.norm(n.astype(np.float64), axis=1)
        assert np.abs(length - 1.0).max() <= 4 * np.finfo(F).eps, np.abs(length - 1.0).max()
    # a triangle and its copy with u -> 1 - u: the tilt along u flips, the tilt along v stays
    k = 64
    ng = np.tile((0.0, 0.0, 1.0), (k, 1)).astype(F)
    e1, e2 = np.tile((1.0, 0.0, 0.0), (k, 1)).astype(F), np.tile((0.0, 1.0, 0.0), (k, 1)).astype(F)
    uv = np.tile((0.0, 0.0, 1.0, 0.0, 0.0, 1.0), (k, 1)).astype(F)
    mirrored = uv.copy()
    mirrored[:, 0::2] = F(1) - uv[:, 0::2]
    c = (0.5 + 0.5 * np.random.default_rng(3).uniform(0.1, 0.6, (k, 3))).astype(F)
    a, ca = NM.mapped_normal(ng, ng, e1, e2, uv, c, 1.0)
    b, cb = NM.mapped_normal(ng, ng, e1, e2, mirrored, c, 1.0)
    assert (ca == 0).all() and (cb == 0).all()
    assert (a[:, 0] > 0).all() and np.array_equal(b[:, 0], -a[:, 0]), "along u the tilt is the opposite"
    assert (a[:, 1] > 0).all() and np.array_equal(b[:, 1], a[:, 1]) and np.array_equal(b[:, 2], a[:, 2]), "along v and n it is the same"


# ---------------------------------------------------------------- frames through the oracle
def test_mutations_change_the_frame_and_the_flat_map_does_not(orc):
    t, mt, n9, uv, nodes = built(orc)
    normals = S.Normals(t, n9)

    def frame(slots, bind=BIND, **mutations):
        nm = NM.Mapped(t, uv, slots, bind, normals, **mutations)
        return transport_ref.render(S.Shaded(oracle_of(orc, t, mt, nodes, rng_mode=1), nm, mt), spp=SPP)

    plain = transport_ref.render(S.Shaded(oracle_of(orc, t, mt, nodes, rng_mode=1), normals, mt), spp=SPP)
    assert_bit_equal(frame({SLOT: (NM.flat_map(), {"filter": "nearest"})}), plain, "the flat map is S.Shaded's frame")
    assert_bit_equal(frame({SLOT: (NM.tilt_map(), {})}, bind={m: (SLOT, 0.0) for m in range(4)}), plain, "strength 0 is S.Shaded's frame")
    tilt = {SLOT: (NM.tilt_map(), {})}
    want = frame(tilt)
    assert not np.array_equal(want.view(np.uint32), plain.view(np.uint32)), "the map changed nothing"
    for name in ("no_gram_schmidt", "ignore_sg", "swap_xy"):
        got = frame(tilt, **{name: True})
        assert not np.array_equal(got.view(np.uint32), want.view(np.uint32)), name
    # step F rejects nothing on this scene at strength 1 (test_the_scene_is_what_the_issue_says): its mutation is read at strength 16,
    # where normals tilted by 0.7 rad come to lie 84 degrees off ns and some leave the stored normal's hemisphere
    steep = {m: (SLOT, 16.0) for m in range(4)}
    assert not np.array_equal(frame(tilt, bind=steep, skip_f_test=True).view(np.uint32), frame(tilt, bind=steep).view(np.uint32)), "skip_f_test"


# ---------------------------------------------------------------- interface
def test_the_flag_needs_textures_and_shading_normals_and_inherits_the_refusals():
    """on device -1 an accepted combination ends at "no HIP device": wfpt_create checks its arguments before it selects a device"""
    import wavefront_path_tracer_amd as W
    assert W.FLAG_NORMAL_MAPS == 1 << 27
    base = W.FLAG_TEXTURES | W.FLAG_SHADING_NORMALS
    for missing in (0, W.FLAG_TEXTURES, W.FLAG_SHADING_NORMALS):
        assert create_message(W, W.FLAG_NORMAL_MAPS | missing, W.RNG_DISPATCH).startswith("wfpt_create: WFPT_FLAG_NORMAL_MAPS needs")
    full = base | W.FLAG_NORMAL_MAPS
    assert "no HIP device" in create_message(W, full, W.RNG_DISPATCH)
    connect = W.FLAG_EMISSION | W.FLAG_NEE
    for other in (W.FLAG_LIGHT_POWER, W.FLAG_ANALYTIC_LIGHTS):
        msg = create_message(W, full | connect | other, W.RNG_DISPATCH)
        assert "does not go with WFPT_FLAG_LIGHT_POWER or WFPT_FLAG_ANALYTIC_LIGHTS" in msg, msg
    needs = {"NEE": W.FLAG_EMISSION, "MIS": connect, "ENV_NEE": connect | W.FLAG_ENVIRONMENT, "ENV_MIS": connect | W.FLAG_ENVIRONMENT | W.FLAG_ENV_NEE,
             "ROUGH_DIELECTRIC": W.FLAG_MICROFACET}
    others = ["SPLIT_SHADE", "NO_GRAPH", "UNFUSED", "BINARY_BVH", "NO_REFILL", "NO_LDS_SCENE", "EXACT_TRAVERSAL", "NO_BINNING", "BINNING", "AOV",
              "DENOISE", "ENVIRONMENT", "EMISSION", "NEE", "ENV_NEE", "MIS", "ENV_MIS", "NO_TILE_LISTS", "RETIRE", "ADAPTIVE", "MICROFACET",
              "ROUGH_DIELECTRIC"]
    for name in others:
        flags = full | getattr(W, "FLAG_" + name) | needs.get(name, 0)
        msg = create_message(W, flags, W.RNG_PIXEL)
        assert "no HIP device" in msg, (name, msg)
        assert msg == create_message(W, flags & ~W.FLAG_NORMAL_MAPS, W.RNG_PIXEL), name


def test_the_bench_tool_keeps_its_legs_and_fields(ab, monkeypatch):
    """tests/test_ab_bench_host.py's check of the other tools, against this tool's own fixture"""
    with open(os.path.join(ROOT, "tests", "golden", "bench_tool_keys_normal_maps.json")) as f:
        want = json.load(f)["bench_normal_maps"]
    monkeypatch.delitem(sys.modules, "wavefront_path_tracer_amd", raising=False)
    mod = load("bench_normal_maps")
    assert "wavefront_path_tracer_amd" not in sys.modules  # the parent role needs no renderer
    args = mod.options().parse_args(want["argv"])
    legs = mod.legs(args)
    assert [leg[0] for leg in legs] == want["legs"] and mod.DIGITS == want["digits"]
    extras = want["keys"][len(COMMON_KEYS):]
    child = {"leg": "x", "loop": "refill", "frame_ms": [1.0, 2.0], **{k: 1.23456789 for k in reversed(extras)}, "frame": 0, "unknown": 1}
    line = ab.summarise({leg[0]: [child] for leg in legs}, args, mod.EXTRA_KEYS, mod.DIGITS)[want["legs"][-1]]
    assert list(line) == want["keys"]
    assert line[extras[0]] == round(1.23456789, want["digits"])
    assert [leg[0] for leg in mod.legs(mod.options().parse_args([]))] == want["legs"][1:], "no parent leg without --parent-root"
