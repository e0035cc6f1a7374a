"""Adaptive sampling (WFPT_FLAG_ADAPTIVE, include/wfpt.h "Adaptive sampling") without a GPU: the restatement tests/adaptive_ref.py itself --
the criterion on hand-made rows, the tile dilation's bit arithmetic against a naive loop, the masked render on the oracle and the two
mutations it must tell apart -- and the ABI's new names."""
import os

import numpy as np
import pytest

import adaptive_ref as A
import emission_ref as E

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W_, H_ = 69, 43
NAMES = ("wfpt_adaptive_params_default", "wfpt_set_adaptive", "wfpt_get_adaptive", "wfpt_set_active_mask", "wfpt_read_active_mask",
         "wfpt_adaptive_update", "wfpt_read_sample_counts", "wfpt_read_mean", "wfpt_copy_mean_to_device", "wfpt_render_adaptive")


@pytest.fixture(scope="module")
def W(wf):
    return wf


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---------------------------------------------------------------- the criterion
def test_criterion_on_hand_made_rows():
    p = {"min_samples": 4, "max_samples": 0, "threshold": 0.05, "luminance_floor": 0.01}
    nan, inf = F("nan"), F("inf")
    rows = [  # (s1, s2, n, unconverged, why)
        (1.5, 0.75, 3, True, "n below min_samples, zero variance"),
        (2.0, 1.0, 4, False, "zero variance converges exactly at min_samples: mu = 0.5, S2 / n = 0.25 = mu * mu"),
        (2.5, 1.0, 5, False, "d = 0.2 - 0.25 < 0 clamps to 0"),
        (4.0, 8.0, 4, True, "mu = 1, v = (2 - 1) / 4 = 0.25 > (0.05 * 1.01)^2"),
        (400.0, 400.0 + 0.8, 400, False, "mu = 1, v = 0.002 / 400 = 5e-6 <= 2.55e-3"),
        (nan, 1.0, 8, True, "NaN S1"),
        (1.0, nan, 8, True, "NaN S2"),
        (inf, inf, 8, True, "inf - inf is NaN"),
        (1.0, inf, 8, True, "infinite variance"),
        (0.0, 0.0, 0, True, "count 0: 0 / 0"),
        (0.0, 0.0, 4, False, "a black pixel: v = 0 <= (0.05 * 0.01)^2"),
    ]
    s1, s2, n = (np.array([r[k] for r in rows], t) for k, t in ((0, F), (1, F), (2, np.uint32)))
    got = A.criterion(s1, s2, n, p)
    for g, r in zip(got, rows):
        assert bool(g) == r[3], r
    # the maximum is no part of the criterion: next_mask applies it to the tile's word
    w, h = 8, 8
    s1 = np.full(64, 4.0, F); s2 = np.full(64, 8.0, F); cnt = np.full(64, 4, np.uint32)
    cnt[:8] = 6
    mask, n_active = A.next_mask(s1, s2, cnt, dict(p, max_samples=6, dilate=1), w, h)
    assert n_active == 56 and not mask[:8].any() and mask[8:].all(), "unconverged everywhere, the capped row is off although dilation reaches it"
    mask, n_active = A.next_mask(s1, s2, cnt, dict(p, max_samples=0, dilate=0), w, h)
    assert n_active == 64
    # and variance_resolve is wfpt_read_variance with the pixel's n
    assert A.variance_resolve([4.0], [8.0], [4])[0] == F(0.25) and A.variance_resolve([1.0], [1.0], [0])[0] == 0


def test_dilation_bit_arithmetic_equals_the_naive_loop():
    rng = np.random.default_rng(5)
    words = [0, A.ALL, 1, 1 << 7, 1 << 56, 1 << 63, 1 << 3, 1 << 59, 1 << 24, 1 << 31, 1 << 27]
    words += [int(x) for x in rng.integers(0, 2 ** 64, 200, dtype=np.uint64)]
    words += [int(x) & int(y) & int(z) for x, y, z in rng.integers(0, 2 ** 64, (200, 3), dtype=np.uint64)]  # sparse words
    for u in words:
        assert A.dilate_tile(u) == A.dilate_tile_naive(u), hex(u)
    assert A.dilate_tile(1) == 0x0303 and A.dilate_tile(1 << 7) == 0xC0C0 and A.dilate_tile(1 << 63) == 0xC0C0 << 48
    assert bin(A.dilate_tile(1 << 27)).count("1") == 9


def test_words_round_trip_and_tiling():
    rng = np.random.default_rng(6)
    for rank, world in ((0, 1), (0, 2), (1, 2), (2, 3)):
        rows = A.slab_rows(H_, rank, world)
        ins = A.inside(W_, H_, rank, world)
        assert len(ins) == rows * W_
        m = (rng.random(rows * W_) < 0.5) & ins
        words = A.to_words(m, W_, H_, rank, world)
        assert len(words) == ((W_ + 7) // 8) * (rows // 8 if world > 1 else (H_ + 7) // 8)
        assert np.array_equal(A.from_words(words, W_, H_, rank, world), m)
    # bit ly * 8 + lx of tile ty * tiles_x + tx
    m = np.zeros((H_, W_), bool)
    m[8 + 3, 16 + 5] = True
    words = A.to_words(m, W_, H_)
    assert words[1 * 9 + 2] == 1 << (3 * 8 + 5) and np.count_nonzero(words) == 1
    # the two ranks' rows interleave to the image's
    g0, g1 = A.global_rows(H_, 0, 2), A.global_rows(H_, 1, 2)
    both = np.sort(np.concatenate([g0, g1]))
    assert np.array_equal(both[both < H_], np.arange(H_))


def test_next_mask_is_the_same_sharded_or_not():
    """Dilation clipped to the tile: a band-sharded update needs no other rank's moments."""
    rng = np.random.default_rng(7)
    n = W_ * H_
    s1 = (rng.random(n) * 8).astype(F)
    s2 = (s1 * s1 / 8 + rng.random(n).astype(F) * 0.02).astype(F)
    cnt = rng.integers(6, 10, n).astype(np.uint32)
    p = {"min_samples": 8, "max_samples": 9, "threshold": 0.05, "luminance_floor": 0.01, "dilate": 1}
    whole, n_whole = A.next_mask(s1, s2, cnt, p, W_, H_)
    assert 0.1 * n < n_whole < 0.9 * n
    total = 0
    for rank in (0, 1):
        g = A.global_rows(H_, rank, 2)
        ok = g < H_
        take = lambda a: np.where(np.repeat(ok, W_), a.reshape(H_, W_)[np.minimum(g, H_ - 1)].reshape(-1), 0).astype(a.dtype)
        part, n_part = A.next_mask(take(s1), take(s2), take(cnt), p, W_, H_, rank, 2)
        assert np.array_equal(part.reshape(-1, W_)[ok], whole.reshape(H_, W_)[g[ok]])
        assert not part.reshape(-1, W_)[~ok].any()
        total += n_part
    assert total == n_whole


# ---------------------------------------------------------------- the masked render on the oracle
def shirley(orc, rng_mode, **kw):
    return orc.shirley_oracle(W_, H_, max_wavefronts=4, rng_mode=rng_mode, **kw)


def plain_emission(orc):
    sp, mt = orc.scene_book_one_final(1)
    sp, _ = orc.build_bvh(sp)
    return E.Emission({}, spheres=sp, materials=mt)


def checkerboard():
    y, x = np.mgrid[0:H_, 0:W_]
    return ((x + y) % 2 == 0).reshape(-1)


def test_all_active_mask_equals_the_oracles_own_render(orc):
    em = plain_emission(orc)
    for rng in (0, 1):
        want = shirley(orc, rng).render(2)
        o = A.Masked(shirley(orc, rng), A.all_active(W_, H_))
        r = E.render_with_emission(o, em, spp=2, parts=True)
        s = A.Sums(W_ * H_).add(r, A.all_active(W_, H_))
        assert np.array_equal(bits(s.acc), bits(want)), rng
        assert (s.count == 2).all()
        t = o.bounce_table().astype(np.int64)
        assert t[0, 0] == 9 * 6 * 64 and t[0, 1] + t[0, 2] == W_ * H_


def test_masked_pixels_keep_their_sums_and_slots(orc):
    em = plain_emission(orc)
    mask = checkerboard()
    o = A.Masked(shirley(orc, 1), mask)
    r = E.render_with_emission(o, em, spp=2, parts=True)
    s = A.Sums(W_ * H_)
    s.acc[:] = 7.0
    s.s1[:] = 3.0
    s.count[:] = 5
    s.add(r, mask)
    assert (s.acc[~mask] == 7.0).all() and (s.s1[~mask] == 3.0).all() and (s.count[~mask] == 5).all() and (s.count[mask] == 7).all()
    t = o.bounce_table().astype(np.int64)
    assert t[0, 0] == 9 * 6 * 64 and t[0, 1] + t[0, 2] == int(mask.sum()), "the masked slots are kept and neither hit nor miss"
    # pixel-keyed RNG: an active pixel's samples are those of the unmasked frame
    full = E.render_with_emission(shirley(orc, 1, miss_floor=0), em, spp=1, parts=True)
    part = E.render_with_emission(A.Masked(shirley(orc, 1, miss_floor=0), mask), em, spp=1, parts=True)
    assert np.array_equal(bits(part["image"][0][mask]), bits(full["image"][0][mask]))
    assert (part["image"][0][~mask] == 1.0).all(), "a masked pixel's throughput is never touched"


def test_two_mutations_are_detected(orc):
    """Marking masked rays by zeroing them without the inactive pixel, and dropping the masked slots from the queue: the bounce table (which
    tests/test_gpu_adaptive.py compares) tells both from the restatement, the first also by the throughput of the masked pixels."""
    em = plain_emission(orc)
    mask = checkerboard()

    def render(rng, **kw):
        o = A.Masked(shirley(orc, rng), mask, **kw)
        r = E.render_with_emission(o, em, spp=1, parts=True)
        return A.Sums(W_ * H_).add(r, mask).acc, o.bounce_table().astype(np.int64), r["image"][0]

    good, table, thr = render(0)
    assert (thr[~mask] == 1.0).all()
    # zeroed without the inactive pixel: the zero ray is traced and misses -- the bounce table counts it, and the sky lands on the
    # throughput of a pixel that was to be left alone (the hit queue, and so the active pixels, do not see it)
    bad, bad_table, bad_thr = render(0, zero_only=True)
    assert bad_table[0, 1] + bad_table[0, 2] == table[0, 1] + table[0, 2] + int((~mask).sum())
    assert not np.array_equal(bad_table, table) and (bad_thr[~mask] != 1.0).any()
    # dropped from the queue instead of kept: rays_in, n_in and the work items are no longer the unmasked frame's -- the bounce table shows
    # it. The image does not: a hit's position in the hit queue (shade's key under WFPT_RNG_DISPATCH) counts the hits before it, not the
    # slots, so compacting the slots leaves every draw where it was; the bounce table is what pins "slots are kept".
    bad, bad_table, _ = render(0, drop=True)
    assert bad_table[0, 0] == table[0, 0] - int((~mask).sum()) and bad_table[0, 1] + bad_table[0, 2] == table[0, 1] + table[0, 2]
    assert not np.array_equal(bad_table, table)
    assert np.array_equal(bits(bad), bits(good))


# ---------------------------------------------------------------- the ABI (no device)
def test_flag_struct_and_symbols(W):
    hdr = open(os.path.join(ROOT, "include", "wfpt.h")).read()
    assert "WFPT_FLAG_ADAPTIVE = 1u << 21" in hdr and W.FLAG_ADAPTIVE == 1 << 21
    for name in NAMES:
        assert name in W.abi_symbols() and hasattr(W.lib(), name), name
    section = hdr.split("Adaptive sampling (WFPT_FLAG_ADAPTIVE)")[1].split("read-back (blocking)")[0]
    for words in ("sizeof(wfpt_adaptive_params) == 32", "clipped to the tile", "gather of counts is out of scope", "0x0101010101010101"):
        assert words in section, words
    assert W.C.sizeof(W._AdaptiveParams) == 32
    p = W._AdaptiveParams()
    W.lib().wfpt_adaptive_params_default(W.C.byref(p))
    got = {k: getattr(p, k) for k in A.DEFAULTS}
    assert got == {k: (F(v) if isinstance(v, float) else v) for k, v in A.DEFAULTS.items()} and not any(p._reserved)
    assert W.ADAPTIVE_DEFAULTS == A.DEFAULTS


def test_null_context_is_refused(W):
    L = W.lib()
    p = W._AdaptiveParams(16, 0, 0.05, 0.01, 1)
    n = W.C.c_uint32(0)
    buf = np.zeros(16, np.uint8)
    ptr = buf.ctypes.data_as(W.C.c_void_p)
    assert L.wfpt_set_adaptive(None, W.C.byref(p)) == -1 and L.wfpt_get_adaptive(None, W.C.byref(p)) == -1
    assert L.wfpt_set_active_mask(None, ptr, 16) == -1 and L.wfpt_read_active_mask(None, ptr, 16) == -1
    assert L.wfpt_adaptive_update(None, W.C.byref(n)) == -1 and L.wfpt_render_adaptive(None, 1, 1, W.C.byref(n)) == -1
    assert L.wfpt_read_sample_counts(None, ptr, 4) == -1 and L.wfpt_read_mean(None, ptr, 4) == -1
    assert L.wfpt_copy_mean_to_device(None, ptr, 4) == -1
    L.wfpt_adaptive_params_default(None)  # no-op
