"""Emissive materials (WFPT_FLAG_EMISSION) without a GPU: the numpy restatement (tests/emission_ref.py) against answers known in closed form,
on the oracle; two mutation checks of the restatement itself; the ABI's constants and the Python-side argument checks."""
import os

import numpy as np
import pytest

import emission_ref as E
from emission_ref import COLOUR, furnace_inputs
import texture_ref as T
from helpers import closed_room_inputs, make_oracle

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W_, H_ = 40, 24


@pytest.fixture(scope="module")
def W():
    import wavefront_path_tracer_amd as W
    return W


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def room(orc, scene="closed-metal", **kw):
    inputs = closed_room_inputs(orc, scene, W_, H_)
    return inputs, make_oracle(orc, inputs, W_, H_, miss_floor=0, **kw)


@pytest.mark.parametrize("rng_mode", [0, 1])
def test_furnace_every_sample_is_the_colour(orc, rng_mode):
    n = 4
    inputs = furnace_inputs(orc, W_, H_)
    sp, mt = inputs[0], inputs[1]
    o = make_oracle(orc, inputs, W_, H_, max_wavefronts=6, miss_floor=0, rng_mode=rng_mode)
    r = E.render_with_emission(o, E.Emission({0: COLOUR}, spheres=sp, materials=mt), spp=n, parts=True)
    wall = int(np.flatnonzero(sp["radius"] == 5.0)[0])
    assert (r["first_prim"] == wall).all(), "a primary ray does not meet the emitter first (the oracle's hit queue)"
    e = np.asarray(COLOUR, F)
    for k in range(n):
        assert np.array_equal(bits(r["image"][k] + r["emitted"][k]), bits(np.broadcast_to(e, (W_ * H_, 3)))), f"sample {k}"
        assert not r["image"][k].any(), "the paths are dead"
    assert np.array_equal(bits(r["acc"]), bits(np.broadcast_to(F(n) * e, (W_ * H_, 3))))


def test_furnace_with_a_textured_emitter_is_texture_times_colour(orc):
    """The emission pass runs after the texture pass: (1 * tex) * e, exact for power-of-two texels."""
    inputs = furnace_inputs(orc, W_, H_)
    sp, mt = inputs[0], inputs[1]
    texel = np.asarray([[[0.5, 0.25, 2.0]]], F)
    tx = T.Textures(spheres=sp, materials=mt, slots={0: (texel, {"filter": "nearest"})}, bind={0: 0})
    o = make_oracle(orc, inputs, W_, H_, max_wavefronts=4, miss_floor=0)
    acc = E.render_with_emission(o, E.Emission({0: COLOUR}, spheres=sp, materials=mt), spp=2, tx=tx)
    want = F(2) * (texel[0, 0] * np.asarray(COLOUR, F))
    assert np.array_equal(bits(acc), bits(np.broadcast_to(want, acc.shape)))
    # mutation: with the emission pass in front of the texture pass the texture never reaches the light
    o = make_oracle(orc, inputs, W_, H_, max_wavefronts=4, miss_floor=0)
    wrong = E.render_with_emission(o, E.Emission({0: COLOUR}, spheres=sp, materials=mt, pass_first=True), spp=2, tx=tx)
    assert not np.array_equal(bits(wrong), bits(acc))


@pytest.mark.parametrize("scene", ["closed-metal", "centre"])
def test_black_body_is_the_plain_render(orc, scene):
    inputs, o = room(orc, scene, max_wavefronts=6)
    acc = E.render_with_emission(o, E.Emission({1: (0.0, 0.0, 0.0)}, spheres=inputs[0], materials=inputs[1]), spp=3)
    _, plain = room(orc, scene, max_wavefronts=6)
    assert np.array_equal(bits(acc), bits(plain.render(3)))
    # and in an open scene, with misses and the miss_floor exit
    sp, mt = orc.scene_book_one_final(1)
    sp, _ = orc.build_bvh(sp)
    o = orc.shirley_oracle(64, 40, max_wavefronts=5)
    acc = E.render_with_emission(o, E.Emission({}, spheres=sp, materials=mt), spp=2)
    assert np.array_equal(bits(acc), bits(orc.shirley_oracle(64, 40, max_wavefronts=5).render(2)))


def small_emitter(inputs):
    """The small Lambertian sphere of the closed rooms (material 1)."""
    return E.Emission({1: COLOUR}, spheres=inputs[0], materials=inputs[1])


def test_nothing_after_the_light(orc):
    inputs, o1 = room(orc, max_wavefronts=1)
    r1 = E.render_with_emission(o1, small_emitter(inputs), spp=2, parts=True)
    _, o8 = room(orc, max_wavefronts=8)
    r8 = E.render_with_emission(o8, small_emitter(inputs), spp=2, parts=True)
    lamp = int(np.flatnonzero(inputs[0]["material_idx"] == 1)[0])
    on_lamp = (r1["first_prim"] == lamp).all(axis=0)
    assert np.array_equal(r1["first_prim"], r8["first_prim"]) and 0 < on_lamp.sum() < on_lamp.size
    assert np.array_equal(bits(r1["acc"][on_lamp]), bits(r8["acc"][on_lamp]))
    assert np.array_equal(bits(r8["acc"][on_lamp]), bits(np.broadcast_to(F(2) * np.asarray(COLOUR, F), (int(on_lamp.sum()), 3))))
    assert not np.array_equal(bits(r1["acc"][~on_lamp]), bits(r8["acc"][~on_lamp])), "the other pixels do go on"
    # mutation: with thr left untouched the path goes on collecting albedos after the light
    em = small_emitter(inputs)
    em.keep_throughput = True
    _, o1 = room(orc, max_wavefronts=1)
    _, o8 = room(orc, max_wavefronts=8)
    w1, w8 = E.render_with_emission(o1, em, spp=2), E.render_with_emission(o8, em, spp=2)
    assert not np.array_equal(bits(w1[on_lamp]), bits(w8[on_lamp]))


def test_doubling_the_colour_doubles_the_light_exactly(orc):
    inputs, o = room(orc, max_wavefronts=8)
    a = E.render_with_emission(o, small_emitter(inputs), spp=2, parts=True)
    _, o = room(orc, max_wavefronts=8)
    twice = E.Emission({1: tuple(2.0 * c for c in COLOUR)}, spheres=inputs[0], materials=inputs[1])
    b = E.render_with_emission(o, twice, spp=2, parts=True)
    assert a["emitted"].any() and (a["emitted"] != 0).any(axis=2).mean() > 0.05, "the room is lit"
    assert np.array_equal(bits(b["emitted"]), bits(F(2) * a["emitted"]))
    assert np.array_equal(bits(b["image"]), bits(a["image"]))
    assert np.array_equal(b["first_prim"], a["first_prim"])


# ---------------------------------------------------------------- ABI and Python-side checks (no device)
def test_flag_and_symbols(W):
    hdr = open(os.path.join(ROOT, "include", "wfpt.h")).read()
    assert "WFPT_FLAG_EMISSION = 1u << 14" in hdr and W.FLAG_EMISSION == 1 << 14
    for name in ("wfpt_set_emission", "wfpt_get_emission", "wfpt_clear_emission", "wfpt_emission_timing_ms"):
        assert name in W.abi_symbols() and hasattr(W.lib(), name)
    assert "miss_floor = 0" in hdr.split("Emission (WFPT_FLAG_EMISSION)")[1].split("read-back")[0]


def test_python_argument_checks(W):
    assert list(W._emission_colour((0.5, 2, 0.25))) == [0.5, 2.0, 0.25]
    assert list(W._emission_colour(np.zeros(3))) == [0.0, 0.0, 0.0]
    for bad in ((1.0, 2.0), (1.0, 2.0, 3.0, 4.0), 1.0, (np.nan, 0.0, 0.0), (0.0, np.inf, 0.0), (0.0, 0.0, -1.0), [[1.0, 1.0, 1.0]]):
        with pytest.raises(ValueError):
            W._emission_colour(bad)
    assert W._material_index(3) == 3 and W._material_index(np.uint32(7)) == 7
    for bad in (-1, 1.5, 2 ** 32):
        with pytest.raises(ValueError):
            W._material_index(bad)
    # a null context is refused by the library itself, without a device
    rgb = (W.C.c_float * 3)(1.0, 1.0, 1.0)
    assert W.lib().wfpt_set_emission(None, 0, rgb) == -1
    assert W.lib().wfpt_get_emission(None, 0, rgb) == -1
    assert W.lib().wfpt_clear_emission(None) == -1
    assert W.lib().wfpt_emission_timing_ms(None, None, None) == -1
