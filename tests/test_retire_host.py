"""Path termination (WFPT_FLAG_RETIRE) without a GPU: the decision function of tests/retire_ref.py on hand-made rows, its stream against
the connect pass's, the restatement on the oracle (retiring dead paths changes no bit; Russian roulette changes no mean, and two
mutations of it do), the ABI's constants and the library's argument checks."""
import os

import numpy as np
import pytest

import emission_ref as E
import nee_ref as N
import retire_ref as RR
from helpers import make_oracle
from retire_ref import DEAD, ROULETTE, SURVIVES

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def W():
    import wavefront_path_tracer_amd as W
    return W


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def below(x):
    return np.nextafter(F(x), F(-np.inf))


# ---------------------------------------------------------------- the decision function
def hand_rows():
    """(t' rows, pixels): zeros of both signs, a NaN in every channel, maxima around q_min = 0.25 and around 1, large and tiny values"""
    nan, q = F(np.nan), F(0.25)
    rows = [(0.0, 0.0, 0.0), (-0.0, 0.0, -0.0), (-0.0, -0.0, -0.0), (0.0, 0.0, 1e-30), (0.0, -0.0, 0.5), (1e-45, 0.0, 0.0),
            (nan, 0.0, 0.0), (0.0, nan, 0.0), (0.0, 0.0, nan), (nan, 0.5, 0.25), (0.5, nan, 0.25), (0.5, 0.25, nan), (nan, nan, nan),
            (below(q), 0.1, 0.0), (q, 0.1, 0.0), (0.1, below(q), 0.2), (0.1, 0.2, q), (np.nextafter(q, F(1)), 0.0, 0.0),
            (below(1.0), 0.5, 0.5), (1.0, 0.5, 0.5), (0.5, np.nextafter(F(1), F(2)), 0.5), (0.5, 0.5, 8.0), (np.inf, 0.0, 0.0),
            (0.75, 0.5, 0.25), (0.3, 0.6, 0.9), (-0.5, -0.25, 0.0), (-0.5, -0.25, -0.125), (0.01, 0.02, 0.03)]
    t = np.asarray(rows, F)
    return t, (np.arange(len(t)) * 977 + 5).astype(np.uint32)


def test_dead_rows_and_nan_channels():
    t, pix = hand_rows()
    out, verdict, q, u = RR.decide(t, pix, 7, 0, roulette_start=RR.NO_ROULETTE)
    assert list(verdict[:6]) == [DEAD, DEAD, DEAD, SURVIVES, SURVIVES, SURVIVES], "-0 counts as zero, a denormal does not"
    assert (verdict[6:13] == SURVIVES).all(), "a NaN channel makes the dead test false"
    assert (verdict[13:] == SURVIVES).all()
    assert np.array_equal(bits(out), bits(t)) and not q.any() and not u.any(), "thr <- t' as before, nothing is drawn"
    # before roulette_start the same
    out2, verdict2, _, _ = RR.decide(t, pix, 7, 2, roulette_start=3, q_min=0.25)
    assert np.array_equal(verdict2, verdict) and np.array_equal(bits(out2), bits(t))


def test_roulette_probability_and_both_sides_of_q():
    t, pix = hand_rows()
    qm = F(0.25)
    for u_hand in (F(0.0), below(qm), qm, F(0.5), below(1.0)):
        out, verdict, q, u = RR.decide(t, pix, 7, 3, roulette_start=3, q_min=0.25, u=u_hand)
        assert list(verdict[:3]) == [DEAD] * 3 and not q[:3].any()
        # m just below and at q_min; a NaN maximum; a negative maximum: q = q_min. Elsewhere q = m.
        want_q = {13: qm, 14: qm, 15: qm, 16: qm, 17: np.nextafter(qm, F(1)), 6: qm, 12: qm, 25: qm, 26: qm, 27: qm, 23: F(0.75), 24: F(0.9),
                  18: below(1.0), 3: qm, 5: qm, 4: F(0.5), 7: qm, 8: qm}
        for i, v in want_q.items():
            assert q[i] == v, (i, q[i], v)
        # (nan, 0.5, 0.25): m = NaN from the first channel and no comparison replaces it; (0.5, nan, 0.25): the NaN is never greater
        assert q[9] == qm and q[10] == F(0.5) and q[11] == F(0.5)
        # m >= 1: survives untouched, nothing drawn
        for i in (19, 20, 21, 22):
            assert verdict[i] == SURVIVES and q[i] == 0 and u[i] == 0 and np.array_equal(bits(out[i]), bits(t[i])), i
        played = q > 0
        assert np.array_equal(u[played], np.full(int(played.sum()), u_hand))
        lives = played & (u_hand < q)
        assert np.array_equal(verdict[played], np.where(lives[played], SURVIVES, ROULETTE))
        with np.errstate(all="ignore"):
            assert np.array_equal(bits(out[lives]), bits(t[lives] / q[lives][:, None])), "three f32 divisions"
        assert not bits(out[played & ~lives]).any(), "+0 in every channel"
    # u == q retires, the float below it survives
    out, verdict, q, _ = RR.decide(t[23:24], pix[23:24], 7, 3, 3, 0.25, u=F(0.75))
    assert verdict[0] == ROULETTE
    out, verdict, q, _ = RR.decide(t[23:24], pix[23:24], 7, 3, 3, 0.25, u=below(0.75))
    assert verdict[0] == SURVIVES and np.array_equal(bits(out[0]), bits(t[23] / F(0.75)))
    # q_min = 1: every live row with m < 1 plays at q = 1 and survives untouched (u < 1 always)
    out, verdict, q, u = RR.decide(t, pix, 7, 3, 3, 1.0)
    assert (q[3:] == 0).all() and (verdict[3:] == SURVIVES).all() and np.array_equal(bits(out), bits(t))


def test_sample_rows_layout():
    t, pix = hand_rows()
    rows = RR.sample_rows(t, pix, 9, 4, roulette_start=0, q_min=0.25)
    out, verdict, q, u = RR.decide(t, pix, 9, 4, 0, 0.25)
    assert rows.shape == (len(t), 8) and not rows[:, 3].any() and not rows[:, 7].any()
    assert np.array_equal(rows[:, 2], verdict.astype(F)) and np.array_equal(bits(rows[:, 4:7]), bits(out))
    assert {0.0, 1.0, 2.0} == set(rows[:, 2])


# ---------------------------------------------------------------- the stream
def test_stream_is_the_steps_own_and_keyed_by_the_pixel():
    pix = np.arange(0, 4096, dtype=np.uint32)
    for frame, b in ((1, 0), (2, 3), (77, 49)):
        u = RR.termination_draw(pix, frame, b)
        u0, u1, u2 = N.connect_draws(pix, frame, b)
        assert (u >= 0).all() and (u < 1).all()
        for other in (u0, u1, u2):
            assert (u != other).mean() > 0.99, "the termination step draws the connect pass's numbers"
        assert abs(np.corrcoef(u, u0)[0, 1]) < 0.06
        assert 0.45 < u.mean() < 0.55
        assert (RR.termination_draw(pix, frame, b + 1) != u).mean() > 0.99 and (RR.termination_draw(pix, frame + 1, b) != u).mean() > 0.99


def test_draw_is_equal_across_rng_modes(orc):
    """The draws are a function of (pixel, frame, b) alone: the two RNG modes retire the same hits of the primary wavefront (whose hits are
    the same in both), although shade's own stream differs between them."""
    w, h = 40, 24
    inputs = RR.lamp_room_inputs(orc, w, h)
    em = E.Emission({1: RR.ROOM["e"]}, spheres=inputs[0], materials=inputs[1])
    seen = []
    for rng in (0, 1):
        o = RR.Retiring(make_oracle(orc, inputs, w, h, max_wavefronts=3, miss_floor=0, rng_mode=rng), roulette_start=0, q_min=0.9)
        r = E.render_with_emission(o, em, spp=2, parts=True, termination=o)
        seen.append((o.tables[0][1], o.tables[1][1], r["image"]))
    assert seen[0][0] == seen[1][0] and seen[0][1] == seen[1][1], "rays_in, hits of wavefront 1: the same paths were retired at b = 0"
    assert seen[0][0][0] > seen[0][0][1] + seen[0][0][2], "nothing was retired"
    assert not np.array_equal(bits(seen[0][2]), bits(seen[1][2])), "shade's own stream is the mode's"


# ---------------------------------------------------------------- the restatement on the oracle
@pytest.mark.parametrize("scene", ["lamp", "room"])
def test_retiring_dead_paths_changes_no_bit(orc, scene):
    """Roulette off, WFPT_RNG_PIXEL, miss_floor = 0: a dead path adds +0 wherever it ends, so the image is the unflagged one bit for bit,
    and the bounce rows show the retired slots."""
    w, h, spp = 48, 32, 3
    inputs = N.lamp_inputs(orc, w, h, mirror=True) if scene == "lamp" else RR.lamp_room_inputs(orc, w, h)
    colours = {1: N.LAMP["e"] if scene == "lamp" else RR.ROOM["e"]}
    em = E.Emission(colours, spheres=inputs[0], materials=inputs[1])

    def oracle():
        return make_oracle(orc, inputs, w, h, max_wavefronts=6, miss_floor=0, rng_mode=1)

    plain = E.render_with_emission(oracle(), em, spp=spp, parts=True)
    o = RR.Retiring(oracle(), roulette_start=RR.NO_ROULETTE)
    got = E.render_with_emission(o, em, spp=spp, parts=True, termination=o)
    for k in ("acc", "image", "emitted", "s1", "s2"):
        assert np.array_equal(bits(got[k]), bits(plain[k])), k
    t = o.bounce_table().astype(np.int64)
    assert (t[:, 1] + t[:, 2] < t[:, 0]).any(), "no row shows a retired slot"
    assert (t[1:, 0] == t[:-1, 1]).all(), "rays_in counts slots: the hits of the wavefront before"
    # with NEE on top: the same
    shadow = make_oracle(orc, inputs, w, h)
    plain = N.render_with_nee(oracle(), shadow, em, spp=spp, parts=True)
    o = RR.Retiring(oracle(), roulette_start=RR.NO_ROULETTE)
    got = N.render_with_nee(o, shadow, em, spp=spp, parts=True, termination=o)
    for k in ("acc", "image", "emitted"):
        assert np.array_equal(bits(got[k]), bits(plain[k])), k


def test_last_shade_of_the_loop_stays_as_it_is(orc):
    """Step 1: with max_wavefronts = 1 nothing is ever retired and nothing drawn."""
    w, h = 40, 24
    inputs = RR.lamp_room_inputs(orc, w, h)
    em = E.Emission({1: RR.ROOM["e"]}, spheres=inputs[0], materials=inputs[1])
    plain = E.render_with_emission(make_oracle(orc, inputs, w, h, max_wavefronts=1, miss_floor=0), em, spp=2)
    o = RR.Retiring(make_oracle(orc, inputs, w, h, max_wavefronts=1, miss_floor=0), roulette_start=0, q_min=0.5)
    assert np.array_equal(bits(E.render_with_emission(o, em, spp=2, termination=o)), bits(plain)) and o.retired == [[], []]


UNBIASED = {"w": 48, "h": 32, "spp": 16, "max_wavefronts": 12, "roulette_start": 1, "q_min": 0.25}


def room_sample_means(orc, **kw):
    """The image-mean luminance of every sample of the lamp room, rendered with emission alone"""
    w, h = UNBIASED["w"], UNBIASED["h"]
    inputs = RR.lamp_room_inputs(orc, w, h)
    em = E.Emission({1: RR.ROOM["e"]}, spheres=inputs[0], materials=inputs[1])
    o = make_oracle(orc, inputs, w, h, max_wavefronts=UNBIASED["max_wavefronts"], miss_floor=0, rng_mode=1)
    retiring = kw.pop("retire", True)
    if retiring:
        o = RR.Retiring(o, roulette_start=UNBIASED["roulette_start"], q_min=UNBIASED["q_min"], **kw)
    r = E.render_with_emission(o, em, spp=UNBIASED["spp"], parts=True, termination=o if retiring else None)
    v = (r["image"] + r["emitted"]).astype(np.float64)
    return (0.2126 * v[..., 0] + 0.7152 * v[..., 1] + 0.0722 * v[..., 2]).mean(axis=1)


def distance(a, b):
    """(mean(b) - mean(a)) in standard errors of the difference, from the two runs' own per-sample values"""
    se = np.sqrt(a.var(ddof=1) / len(a) + b.var(ddof=1) / len(b))
    return (b.mean() - a.mean()) / se


def test_roulette_is_unbiased_and_its_mutations_are_not(orc):
    """Aggressive roulette (from the second wavefront on, q_min = 0.25) in the closed lamp room at the same spp: the image-mean luminance
    moves by at most 4 standard errors of the difference (measured: +0.32), while a survivor not divided by q (-24.5) and a retired
    throughput left as t' (+147) each fall far outside."""
    base = room_sample_means(orc, retire=False)
    d = distance(base, room_sample_means(orc))
    d_nodiv = distance(base, room_sample_means(orc, no_divide=True))
    d_keep = distance(base, room_sample_means(orc, keep_retired=True))
    print(f"distances in standard errors: roulette {d:+.2f}, not divided {d_nodiv:+.2f}, retired thr kept {d_keep:+.2f}")
    assert abs(d) <= 4.0, d
    assert d_nodiv < -4.0, d_nodiv
    assert d_keep > 4.0, d_keep


# ---------------------------------------------------------------- ABI and argument checks (no device)
def test_flag_struct_and_symbols(W):
    hdr = open(os.path.join(ROOT, "include", "wfpt.h")).read()
    assert "WFPT_FLAG_RETIRE = 1u << 20" in hdr and W.FLAG_RETIRE == 1 << 20 and W.NO_ROULETTE == 0xFFFFFFFF
    for name in ("wfpt_termination_params_default", "wfpt_set_termination", "wfpt_get_termination", "wfpt_sample_termination"):
        assert name in W.abi_symbols() and hasattr(W.lib(), name)
    section = hdr.split("Path termination (WFPT_FLAG_RETIRE)")[1].split("read-back")[0]
    assert "0x85EBCA6Bu" in section and "sizeof(wfpt_termination_params) == 32" in section
    assert W.C.sizeof(W._TerminationParams) == 32
    p = W._TerminationParams()
    W.lib().wfpt_termination_params_default(W.C.byref(p))
    assert p.roulette_start == RR.DEFAULTS["roulette_start"] == 3 and p.q_min == F(RR.DEFAULTS["q_min"]) and not any(p._reserved)
    # no "retiring dead paths" left among the things not done
    assert "retiring dead paths" not in hdr and "retiring dead or" not in hdr


def test_null_context_is_refused(W):
    p = W._TerminationParams(3, 0.05)
    L = W.lib()
    assert L.wfpt_set_termination(None, W.C.byref(p)) == -1
    assert L.wfpt_get_termination(None, W.C.byref(p)) == -1
    assert L.wfpt_sample_termination(None, None, None, 1, 0, 0, None) == -1
    L.wfpt_termination_params_default(None)  # no-op
