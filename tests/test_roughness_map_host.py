"""Roughness maps (WFPT_FLAG_ROUGHNESS_MAPS, include/wfpt.h "Roughness maps") without a GPU: wfpt_hit_roughness_host -- steps R3-R4
compiled from the function the kernels call -- against the restatement (tests/roughness_map_ref.py) bit for bit; whole frames through the
oracle: the all-ones map, the all-zero map and four mutations of the stripe map; the conditions the issue puts on the reference; the
flag's create-time rule on device -1; the bench tool's legs and fields."""
import json
import os
import sys

import numpy as np
import pytest

import microfacet_ref as MF
import normal_map_ref as NM
import rough_dielectric_ref as RD
import roughness_map_ref as RM
import shading_normals_ref as S
import texture_ref as T
from conftest import assert_bit_equal
from test_ab_bench_host import COMMON_KEYS, ROOT, ab, load  # noqa: F401  (ab: the fixture)
from test_microfacet_host import create_message

F = np.float32
SPP, WAVES, FLOOR = 3, 4, 16
SLOT, CHANNEL = 2, 1
METAL, GLASS, ALPHA = 1, 2, 0.3
BOTH = {METAL: ALPHA, GLASS: ALPHA}
BIND = {METAL: (SLOT, CHANNEL, "linear"), GLASS: (SLOT, CHANNEL, "linear")}
STRIPES = {SLOT: (RM.stripe_map(), {})}

_built = {}


def built(orc):
    if "scene" not in _built:
        t, mt, n9, uv = NM.sphere_scene(orc)
        t, nodes = orc.build_bvh_triangles(t, 32)
        _built["scene"] = (t, mt, n9, uv, nodes)
    return _built["scene"]


def oracle_of(orc, w=61, h=37, **kw):
    t, mt, _, _, nodes = built(orc)
    cam, ip, vw = S.sphere_camera(orc, w, h)
    kw.setdefault("miss_floor", FLOOR)
    return orc.Oracle(w, h, np.zeros(1, orc.SPHERE), mt, nodes, cam, ip, vw, triangles=t, max_wavefronts=WAVES, **kw)


def render(orc, r):
    t, mt = built(orc)[:2]
    with MF.rough_weights(r):
        return T.render_with_textures(r, T.Textures(triangles=t, materials=mt), spp=SPP)


def mapped_frame(orc, slots=STRIPES, bind=BIND, alphas=BOTH, w=61, h=37, sample_alpha_m=False, **mutations):
    t, mt, _, uv, _ = built(orc)
    r = RM.RoughMapped(oracle_of(orc, w, h), t, mt, alphas, RM.Roughness(t, uv, slots, bind, **mutations), sample_alpha_m=sample_alpha_m)
    return render(orc, r), r


def assert_conditions(r, what):
    """the issue's conditions on the reference: at least 20 hits in each of the six classes, and RoughGlass.counts positive in all four cells"""
    print(what, r.classes, r.counts)
    assert all(v >= 20 for v in r.classes.values()), (what, r.classes)
    assert all(v > 0 for v in r.counts.values()), (what, r.counts)


# ---------------------------------------------------------------- bits
def edge_rows():
    """(alpha_m, c.rgb) rows with texel 0, 1, above 1, FLT_MAX and a denormal in every channel, under alpha 0, 1 and values between"""
    texels = np.array([0.0, 1.0, 1.25, np.finfo(F).max, 1e-40, np.nextafter(F(1), F(0)), np.nextafter(F(1), F(2)), 0.5], F)
    alphas = np.array([0.0, 1.0, 0.3, 1e-3, np.finfo(F).tiny], F)
    rows = []
    for a in alphas:
        for ch in range(3):
            for x in texels:
                c = np.array([0.25, 0.5, 0.75], F)
                c[ch] = x
                rows.append((a, *c))
    return np.array(rows, F)


def test_the_stripe_map_is_what_the_issue_says():
    img = RM.stripe_map()
    assert img.shape == (8, 16, 3) and img.dtype == F
    for ch in range(3):
        k = (np.arange(16) + ch) % 4
        col = img[:, :, ch]
        assert (col[:, k < 2] == 0).all() and ((col[:, k == 2] >= 1) & (col[:, k == 2] < 1.5)).all()
        assert ((col[:, k == 3] >= F(0.05)) & (col[:, k == 3] < 1)).all()
    rng = np.random.default_rng(9)
    low = rng.uniform(0.05, 1.0, (8, 16))
    assert np.array_equal(img[:, 3, 0], low[:, 3].astype(F)), "the U(0.05, 1) array is drawn first"


@pytest.mark.parametrize("remap", RM.REMAPS)
@pytest.mark.parametrize("channel", [0, 1, 2])
def test_host_function_equals_restatement_bit_for_bit(wf, channel, remap):
    rng = np.random.default_rng(3 + channel)
    rows = np.concatenate([np.concatenate([rng.random((4000, 1)), rng.uniform(0.0, 1.5, (4000, 3))], 1).astype(F), edge_rows()])
    alpha, r = RM.hit_roughness(rows[:, 0], rows[:, 1:], channel, remap)
    assert not np.isnan(alpha).any() and (r <= 1).all() and (alpha <= rows[:, 0]).all() and (alpha >= 0).all()
    assert (r == 1).sum() > 1000 and (alpha == 0).sum() >= 28
    got = wf.hit_roughness_host(rows, channel, remap)
    assert_bit_equal(got[:, 0], alpha, f"alpha_h, channel {channel}, {remap}")
    assert_bit_equal(got[:, 1], r, f"r, channel {channel}, {remap}")
    assert_bit_equal(wf.hit_roughness_host(rows, channel, RM.REMAPS.index(remap)), got, "the remap by value")
    assert len(wf.hit_roughness_host(np.zeros((0, 4), F), channel, remap)) == 0


def test_host_function_refuses_bad_arguments(wf):
    with pytest.raises(ValueError):
        wf.hit_roughness_host(np.zeros((3, 3), F))
    with pytest.raises(ValueError):
        wf.hit_roughness_host(np.zeros((3, 4), F), 1, "cubed")
    for channel, remap in ((3, 0), (0, 2)):
        with pytest.raises(wf.WfptError):
            wf.hit_roughness_host(np.zeros((3, 4), F), channel, remap)


# ---------------------------------------------------------------- frames through the oracle
def test_the_ones_map_the_zero_map_and_four_mutations(orc):
    t, mt = built(orc)[:2]
    rough = RD.RoughGlass(oracle_of(orc), t, mt, BOTH)
    # (nearest: a bilinear lookup of equal texels sums four weights, which need not round to exactly 1)
    ones, r = mapped_frame(orc, slots={SLOT: (RM.constant_map(1.0), {"filter": "nearest"})})
    assert_bit_equal(ones, render(orc, rough), "an all-ones map is RoughGlass's frame")
    assert r.sampled == rough.sampled and r.glass_sampled == rough.glass_sampled and r.counts == rough.counts
    smooth = RD.RoughGlass(oracle_of(orc), t, mt, {})
    zeros, r = mapped_frame(orc, slots={SLOT: (RM.constant_map(0.0), {})})
    assert_bit_equal(zeros, render(orc, smooth), "an all-zero map is the frame with no alpha set")
    assert r.sampled == 0 and r.glass_sampled == 0
    want, r = mapped_frame(orc)
    assert_conditions(r, "61x37 bilinear")
    bits = lambda a: np.ascontiguousarray(a, F).view(np.uint32)
    assert not np.array_equal(bits(want), bits(ones)) and not np.array_equal(bits(want), bits(zeros)), "the stripe map changed nothing"
    for name in ("wrong_channel", "no_clamp", "sample_alpha_m"):
        got, _ = mapped_frame(orc, **{name: True})
        assert not np.array_equal(bits(got), bits(want)), name
    squared = {m: (SLOT, CHANNEL, "squared") for m in BOTH}
    want2, _ = mapped_frame(orc, bind=squared)
    assert not np.array_equal(bits(want2), bits(want)), "squared is linear's frame"
    got, _ = mapped_frame(orc, bind=squared, no_square=True)
    assert not np.array_equal(bits(got), bits(want2)), "no_square"
    assert_bit_equal(got, want, "SQUARED not squaring is LINEAR")


@pytest.mark.parametrize("w,h,filter", [(61, 37, "nearest"), (64, 64, "bilinear"), (64, 64, "nearest")])
def test_the_conditions_on_the_reference(orc, w, h, filter):
    _, r = mapped_frame(orc, slots={SLOT: (RM.stripe_map(), {"filter": filter})}, w=w, h=h)
    assert_conditions(r, f"{w}x{h} {filter}")


# ---------------------------------------------------------------- interface
def test_the_flag_needs_textures_and_microfacet():
    """on device -1 an accepted combination ends at "no HIP device": wfpt_create checks its arguments before it selects a device"""
    import wavefront_path_tracer_amd as W
    assert W.FLAG_ROUGHNESS_MAPS == 1 << 28
    for present in (0, W.FLAG_TEXTURES, W.FLAG_MICROFACET, W.FLAG_MICROFACET | W.FLAG_ROUGH_DIELECTRIC):
        msg = create_message(W, W.FLAG_ROUGHNESS_MAPS | present, W.RNG_DISPATCH)
        assert msg.startswith("wfpt_create: WFPT_FLAG_ROUGHNESS_MAPS needs WFPT_FLAG_TEXTURES"), msg
        assert "WFPT_FLAG_MICROFACET" in msg
    full = W.FLAG_TEXTURES | W.FLAG_MICROFACET | W.FLAG_ROUGHNESS_MAPS
    assert "no HIP device" in create_message(W, full, W.RNG_DISPATCH)
    connect = W.FLAG_EMISSION | W.FLAG_NEE
    needs = {"NEE": W.FLAG_EMISSION, "MIS": connect, "LIGHT_POWER": connect, "ANALYTIC_LIGHTS": connect, "ENV_NEE": connect | W.FLAG_ENVIRONMENT,
             "ENV_MIS": connect | W.FLAG_ENVIRONMENT | W.FLAG_ENV_NEE, "NORMAL_MAPS": W.FLAG_SHADING_NORMALS}
    others = ["SPLIT_SHADE", "NO_GRAPH", "UNFUSED", "BINARY_BVH", "NO_REFILL", "NO_LDS_SCENE", "EXACT_TRAVERSAL", "NO_BINNING", "BINNING", "AOV",
              "DENOISE", "ENVIRONMENT", "EMISSION", "NEE", "ENV_NEE", "MIS", "ENV_MIS", "LIGHT_POWER", "ANALYTIC_LIGHTS", "NO_TILE_LISTS", "RETIRE",
              "ADAPTIVE", "SHADING_NORMALS", "ROUGH_DIELECTRIC", "NORMAL_MAPS"]
    for name in others:
        flags = full | getattr(W, "FLAG_" + name) | needs.get(name, 0)
        msg = create_message(W, flags, W.RNG_PIXEL)
        assert "no HIP device" in msg, (name, msg)
        assert msg == create_message(W, flags & ~W.FLAG_ROUGHNESS_MAPS, W.RNG_PIXEL), name


def test_the_bench_tool_keeps_its_legs_and_fields(ab, monkeypatch):
    """tests/test_ab_bench_host.py's check of the other tools, against this tool's own fixture"""
    with open(os.path.join(ROOT, "tests", "golden", "bench_tool_keys_roughness_maps.json")) as f:
        want = json.load(f)["bench_roughness_maps"]
    monkeypatch.delitem(sys.modules, "wavefront_path_tracer_amd", raising=False)
    mod = load("bench_roughness_maps")
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
