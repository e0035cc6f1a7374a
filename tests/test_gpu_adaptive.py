"""Adaptive sampling (WFPT_FLAG_ADAPTIVE, include/wfpt.h "Adaptive sampling") on the GPU.

Whole renders are compared bit for bit with tests/adaptive_ref.py: the restatement of the context's other flags (emission_ref, mis_ref,
env_mis_ref, texture_ref through emission_ref's tx) driven over an oracle wrapped in adaptive_ref.Masked, its per-sample values added to
the active pixels alone (adaptive_ref.Sums), and wfpt_adaptive_update against adaptive_ref.next_mask fed the context's own read-back. A
restatement depends on the scene, the size, the RNG mode, the masks and the parameters alone -- not on the loop or the batch -- so each is
computed once and shared. The shapes are tests/test_gpu_retire.py's: 69x43 (no multiple of 8: padding, masked and retired rays share a
queue; five 512-slot work items and a partial one), 3 spp per render call at batch = 2, max_wavefronts = 6."""
import numpy as np
import pytest

import adaptive_ref as A
import emission_ref as E
import env_mis_ref as X
import env_nee_ref as V
import mis_ref as M
import retire_ref as RR
import texture_ref as T
from helpers import make_oracle
from test_gpu_env_nee import ENV_PARAMS, LAMP_E, env_light, ground_tracer
from test_gpu_nee import assert_bits, light, mesh_inputs, mesh_tracer, shirley_scene
from test_gpu_retire import LOOP_KIND, LOOPS, MESH_LOOPS
from test_gpu_textures import apply as apply_textures
from test_gpu_textures import shirley_textures

pytestmark = pytest.mark.gpu

F = np.float32
SPP, BATCH, WAVEFRONTS = 3, 2, 6
W_, H_ = 69, 43
MESH_W, MESH_H = 96, 64
RETIRE = (1, 0.25)


@pytest.fixture(scope="module")
def W(gpu):
    return gpu


@pytest.fixture(scope="module")
def O(orc):
    return orc


def flags_of(W, *names):
    f = W.FLAG_ADAPTIVE
    for group in names:
        for n in (group.split("|") if group else []):
            f |= getattr(W, "FLAG_" + n)
    return f


# ---------------------------------------------------------------- the hand-made masks (one bool per pixel, row-major)
def hand_mask(name, w=W_, h=H_):
    y, x = np.mgrid[0:h, 0:w]
    if name == "checker":
        m = (x + y) % 2 == 0
    elif name == "tiles":  # one whole tile off, and eight consecutive tiles: slots 1024 .. 1535, a whole work item of the first launch
        tile = (y // 8) * ((w + 7) // 8) + x // 8
        m = ~((tile == 3) | ((tile >= 16) & (tile < 24)))
    elif name == "corner":  # a single active pixel, in the partial tile at the image's corner
        m = (x == w - 1) & (y == h - 1)
    elif name == "none":
        m = np.zeros((h, w), bool)
    elif name == "all":
        m = np.ones((h, w), bool)
    elif name == "blocks":  # two thirds of the pixels, in blocks that cut through the tiles
        m = (x // 5 + y // 3) % 3 != 0
    else:
        raise KeyError(name)
    return m.reshape(-1)


# ---------------------------------------------------------------- the cases: the context's other flags
CASES = {
    "alone": "",
    "retire": "EMISSION|NEE|MIS|RETIRE",
    "env": "ENVIRONMENT|EMISSION|NEE|ENV_NEE|ENV_MIS",
    "tex": "TEXTURES",
    "mesh": "",
}


class Ref:
    """The restatement of one flagged context: render(mask) adds SPP samples under a mask (frames continue from call to call, as the
    context's do), update(params) makes the next mask of the sums."""

    def __init__(self, O, case, rng, tile=(0, 1), miss_floor=None):
        self.O, self.case, self.rng, self.tile = O, case, rng, tile
        self.w, self.h = (MESH_W, MESH_H) if case == "mesh" else (W_, H_)
        self.miss_floor = miss_floor
        self.frame = 1
        self.sums = A.Sums(A.slab_rows(self.h, *tile) * self.w)
        self.mask = A.all_active(self.w, self.h, *tile)
        self.table = None

    def kw(self, **more):
        kw = dict(max_wavefronts=WAVEFRONTS, rng_mode=self.rng, tile_rank=self.tile[0], tile_world=self.tile[1])
        if self.miss_floor is not None:
            kw["miss_floor"] = self.miss_floor
        kw.update(more)
        return kw

    def render(self, mask=None, spp=SPP):
        O, case = self.O, self.case
        mask = self.mask if mask is None else np.asarray(mask, bool).reshape(-1) & A.inside(self.w, self.h, *self.tile)
        self.mask = mask
        common = dict(spp=spp, first_frame=self.frame, parts=True)
        if case == "env":
            inputs = V.ground_inputs(O, W_, H_, occluder=True, mirror=True, lamp=True)
            em = E.Emission({1: LAMP_E}, spheres=inputs[0], materials=inputs[1])
            o = A.Masked(make_oracle(O, inputs, W_, H_, **self.kw(miss_floor=0)), mask)
            r = X.render_with_env_mis(o, make_oracle(O, inputs, W_, H_), em, env_light(V.sun_map()), **common)
        elif case == "mesh":
            tris, mt, nodes, cam, ip, vw = mesh_inputs(O, MESH_W, MESH_H)
            o = A.Masked(O.Oracle(MESH_W, MESH_H, np.zeros(1, O.SPHERE), mt, nodes, cam, ip, vw, triangles=tris, **self.kw(miss_floor=16)), mask)
            r = E.render_with_emission(o, E.Emission({}, triangles=tris, materials=mt), **common)
        else:
            sp, mt, colours = shirley_scene(O)
            inner = O.shirley_oracle(W_, H_, **self.kw())
            if case == "retire":
                retiring = RR.Retiring(inner, roulette_start=RETIRE[0], q_min=RETIRE[1])
                o = A.Masked(retiring, mask)
                r = M.render_with_mis(o, O.shirley_oracle(W_, H_), E.Emission(colours, spheres=sp, materials=mt), termination=retiring, **common)
            elif case == "tex":
                slots, bind = shirley_textures(O, sp, mt)
                o = A.Masked(inner, mask)
                r = E.render_with_emission(o, E.Emission({}, spheres=sp, materials=mt), tx=T.Textures(spheres=sp, materials=mt, slots=slots, bind=bind),
                                           **common)
            else:
                o = A.Masked(inner, mask)
                r = E.render_with_emission(A.Local(o) if self.tile[1] > 1 else o, E.Emission({}, spheres=sp, materials=mt), **common)
        self.sums.add(r, mask)
        self.frame += spp
        self.table = o.bounce_table()
        return self

    def update(self, params):
        self.mask, n = A.next_mask(self.sums.s1, self.sums.s2, self.sums.count, params, self.w, self.h, *self.tile)
        return n


def tracer(W, O, case, loop="", rng=0, batch=BATCH, **kw):
    flags = kw.pop("flags", None)
    flags = flags_of(W, CASES[case], loop) if flags is None else flags
    if case == "env":
        inputs = V.ground_inputs(O, W_, H_, occluder=True, mirror=True, lamp=True)
        pt = ground_tracer(W, inputs, W_, H_, max_wavefronts=WAVEFRONTS, miss_floor=0, rng_mode=rng, flags=flags, batch=batch, **kw)
        pt.set_environment(V.sun_map(), **ENV_PARAMS)
        pt.set_emission(1, LAMP_E)
        return pt
    if case == "mesh":
        return mesh_tracer(W, MESH_W, MESH_H, max_wavefronts=WAVEFRONTS, miss_floor=16, rng_mode=rng, flags=flags, batch=batch, **kw)
    pt = W.shirley_path_tracer(W_, H_, max_wavefronts=WAVEFRONTS, rng_mode=rng, flags=flags, batch=batch, **kw)
    if case == "retire":
        light(pt, shirley_scene(O)[2])
        pt.set_termination(*RETIRE)
    if case == "tex":
        sp, mt, _ = shirley_scene(O)
        apply_textures(pt, *shirley_textures(O, sp, mt))
    return pt


def check(pt, ref, what):
    """accumulated, the counts, the moments (through variance(), the pixel's own n) and the last sample's bounce table"""
    assert_bits(pt.accumulated(), ref.sums.acc, what + ": accumulated")
    assert np.array_equal(pt.sample_counts().reshape(-1), ref.sums.count), what + ": sample counts"
    assert_bits(pt.variance().reshape(-1), ref.sums.variance(), what + ": variance")
    assert np.array_equal(pt.bounce_table(), ref.table), f"{what}: bounce table\n{pt.bounce_table()}\nvs\n{ref.table}"


_refs = {}


def masked_reference(O, case, rng, name):
    """one render of SPP samples under the hand-made mask `name`; "none": after a render with every pixel active"""
    key = (case, rng, name)
    if key not in _refs:
        ref = Ref(O, case, rng)
        if name == "none":
            ref.render(hand_mask("all", ref.w, ref.h))
        _refs[key] = ref.render(hand_mask(name, ref.w, ref.h))
    return _refs[key]


# ---------------------------------------------------------------- 1. a masked render against the restatement
@pytest.mark.parametrize("rng", [0, 1])
@pytest.mark.parametrize("loop", LOOPS)
def test_masked_render_equals_restatement(W, O, loop, rng):
    for name in ("checker", "tiles", "corner", "none"):
        ref = masked_reference(O, "alone", rng, name)
        pt = tracer(W, O, "alone", loop, rng)
        assert pt.loop_kind == LOOP_KIND[loop]
        what = f"{name} {loop} rng {rng}"
        if name == "none":
            pt.render(SPP)
            before, counts = pt.accumulated(), pt.sample_counts()
            assert (counts == SPP).all()
        pt.set_active_mask(hand_mask(name))
        pt.render(SPP)
        check(pt, ref, what)
        t = pt.bounce_table().astype(np.int64)
        assert t[0, 0] == 9 * 6 * 64, "the slots of the unmasked frame"
        assert t[0, 1] + t[0, 2] == int(hand_mask(name).sum()), what
        if name == "none":
            assert_bits(pt.accumulated(), before, what + ": accumulated was touched")
            assert np.array_equal(pt.sample_counts(), counts) and len(t) == 1 and not t[0, 1:].any(), t
        pt.close()


@pytest.mark.parametrize("rng", [0, 1])
@pytest.mark.parametrize("loop", MESH_LOOPS)
def test_masked_mesh_equals_restatement(W, O, loop, rng):
    """The 5 000-triangle mesh under one mask: the triangle forms of every loop, the four-wide and binary walks, refill on and off."""
    ref = masked_reference(O, "mesh", rng, "checker")
    pt = tracer(W, O, "mesh", loop, rng)
    pt.set_active_mask(hand_mask("checker", MESH_W, MESH_H))
    pt.render(SPP)
    check(pt, ref, f"mesh {loop} rng {rng}")
    pt.close()


# ---------------------------------------------------------------- 2. every pixel active: the unflagged frame
@pytest.mark.parametrize("loop", LOOPS)
def test_all_active_equals_the_unflagged_frame(W, O, loop):
    got = {}
    for flagged in (False, True):
        f = flags_of(W, loop) & ~(0 if flagged else W.FLAG_ADAPTIVE)
        pt = W.shirley_path_tracer(W_, H_, max_wavefronts=WAVEFRONTS, flags=f, batch=BATCH)
        pt.render(SPP)
        got[flagged] = (pt.accumulated(), pt.bounce_table())
        if flagged:
            assert (pt.sample_counts() == SPP).all() and pt.active_mask().all() and pt.active_mask().shape == (H_, W_)
            assert W.lib().wfpt_accumulated_samples(pt.handle) == SPP
        pt.close()
    assert_bits(got[True][0], got[False][0], f"{loop}: accumulated")
    assert np.array_equal(got[True][1], got[False][1])


# ---------------------------------------------------------------- 3. the update against the restatement
THRESHOLDS = (0.02, 0.05, 0.1, 0.2, 0.35, 0.5, 1.0, 2.0)
_updates = {}


def update_reference(O, dilate, max_samples):
    """Round 1 under the "blocks" mask (counts of 3 and 0), the update, round 2 under its mask. The threshold is chosen here, on the CPU:
    the candidate whose mask is closest to half of the pixels."""
    key = (dilate, max_samples)
    if key not in _updates:
        ref = Ref(O, "alone", 1).render(hand_mask("blocks"))
        min_samples = 3 if dilate else 2
        best = None
        for thr in THRESHOLDS:
            p = dict(min_samples=min_samples, max_samples=max_samples, threshold=thr, luminance_floor=0.01, dilate=dilate)
            _, n = A.next_mask(ref.sums.s1, ref.sums.s2, ref.sums.count, p, W_, H_)
            if best is None or abs(n - W_ * H_ / 2) < abs(best[1] - W_ * H_ / 2):
                best = (p, n)
        params = best[0]
        first = (ref.sums.acc.copy(), ref.sums.count.copy(), ref.sums.s1.copy(), ref.sums.s2.copy())
        n_active = ref.update(params)
        mask = ref.mask.copy()
        ref.render()
        _updates[key] = (params, first, mask, n_active, ref)
    return _updates[key]


@pytest.mark.parametrize("max_samples", [0, 3])
@pytest.mark.parametrize("dilate", [0, 1])
def test_update_equals_restatement(W, O, dilate, max_samples):
    params, first, mask, n_active, ref = update_reference(O, dilate, max_samples)
    n = W_ * H_
    assert 0.1 * n <= n_active <= 0.9 * n, f"the restatement's mask proves nothing: {n_active} of {n} active with {params}"
    assert n_active == int(mask.sum())
    pt = tracer(W, O, "alone", "", 1)
    pt.set_adaptive(**params)
    pt.set_active_mask(hand_mask("blocks"))
    pt.render(SPP)
    assert_bits(pt.accumulated(), first[0], "round 1")
    # next_mask fed the context's own read-back: the counts as they are, the moments as variance() shows them to be the restatement's
    counts = pt.sample_counts().reshape(-1)
    assert_bits(pt.variance().reshape(-1), A.variance_resolve(first[2], first[3], counts), "round 1: the moments")
    want_mask, want_n = A.next_mask(first[2], first[3], counts, params, W_, H_)
    assert want_n == n_active and np.array_equal(want_mask, mask)
    got_n = pt.adaptive_update()
    assert got_n == want_n, (got_n, want_n)
    assert np.array_equal(pt.active_mask().reshape(-1), want_mask), f"{int((pt.active_mask().reshape(-1) != want_mask).sum())} mask bits differ"
    pt.render(SPP)
    check(pt, ref, f"round 2, dilate {dilate}, max_samples {max_samples}")
    pt.close()


# ---------------------------------------------------------------- 4. batch sizes
def test_batch_sizes_give_the_same_bits(W, O):
    params = update_reference(O, 1, 0)[0]
    got = []
    for batch in (1, 3, 128):
        pt = tracer(W, O, "alone", "", 0, batch=batch)
        pt.set_adaptive(**params)
        pt.set_active_mask(hand_mask("blocks"))
        seen = []
        for _ in range(2):
            pt.render(SPP)
            n = pt.adaptive_update()
            seen.append((pt.accumulated(), pt.sample_counts(), pt.variance(), pt.active_mask(), n))
        got.append(seen)
        pt.close()
    for other, batch in zip(got[1:], (3, 128)):
        for a, b in zip(got[0], other):
            assert_bits(a[0], b[0], f"batch {batch}: accumulated")
            assert np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3]) and a[4] == b[4], f"batch {batch}"
            assert_bits(a[2], b[2], f"batch {batch}: variance")
    assert 0 < got[0][0][4] < W_ * H_


# ---------------------------------------------------------------- 5. composition with the other flags
@pytest.mark.parametrize("loop", ["", "UNFUSED", "NO_LDS_SCENE"])
@pytest.mark.parametrize("case", ["retire", "env", "tex"])
def test_composition_equals_restatement(W, O, case, loop):
    ref = masked_reference(O, case, 0, "checker")
    pt = tracer(W, O, case, loop, 0)
    pt.set_active_mask(hand_mask("checker"))
    pt.render(SPP)
    check(pt, ref, f"{case} {loop}")
    if case == "retire":
        t = pt.bounce_table().astype(np.int64)
        assert (t[1:, 1] + t[1:, 2] < t[1:, 0]).any(), "masked, padding and retired rays share a queue"
    pt.close()


# ---------------------------------------------------------------- 6. band sharding
def test_sharded_ranks_equal_restatement_and_interleave(W, O):
    params = dict(update_reference(O, 1, 0)[0])
    whole_mask = hand_mask("blocks")
    whole = tracer(W, O, "alone", "", 1, miss_floor=0)
    whole.set_adaptive(**params)
    whole.set_active_mask(whole_mask)
    whole.render(SPP)
    whole_n = whole.adaptive_update()
    whole_counts, whole_next, whole_acc = whole.sample_counts(), whole.active_mask(), whole.accumulated().reshape(H_, W_, 3)
    whole.close()
    total = 0
    for rank in (0, 1):
        g = A.global_rows(H_, rank, 2)
        ok = g < H_
        slab_mask = np.zeros((len(g), W_), bool)
        slab_mask[ok] = whole_mask.reshape(H_, W_)[g[ok]]
        ref = Ref(O, "alone", 1, tile=(rank, 2), miss_floor=0).render(slab_mask)
        pt = tracer(W, O, "alone", "", 1, miss_floor=0, tile_rank=rank, tile_world=2)
        assert pt.n_pixels == len(g) * W_
        pt.set_adaptive(**params)
        pt.set_active_mask(slab_mask)
        assert np.array_equal(pt.active_mask(), slab_mask)
        pt.render(SPP)
        check(pt, ref, f"rank {rank}")
        n = pt.adaptive_update()
        assert n == ref.update(params) and np.array_equal(pt.active_mask().reshape(-1), ref.mask), f"rank {rank}: the update"
        total += n
        # the rank's rows are the unsharded context's
        assert np.array_equal(pt.sample_counts()[ok], whole_counts[g[ok]]) and np.array_equal(pt.active_mask()[ok], whole_next[g[ok]])
        assert not pt.active_mask()[~ok].any() and not pt.sample_counts()[~ok].any()
        assert_bits(pt.accumulated().reshape(len(g), W_, 3)[ok], whole_acc[g[ok]], f"rank {rank}: accumulated")
        pt.render(SPP)
        check(pt, ref.render(), f"rank {rank}, round 2")
        pt.close()
    assert total == whole_n


# ---------------------------------------------------------------- 7. read-back
def test_mean_and_mask_read_back(W, O):
    import torch
    pt = tracer(W, O, "alone", "", 0)
    assert not pt.mean().any()
    pt.render(SPP)
    pt.set_active_mask(hand_mask("blocks"))
    assert np.array_equal(pt.active_mask().reshape(-1), hand_mask("blocks"))
    pt.render(SPP)
    pt.set_active_mask(hand_mask("none"))
    acc, count = pt.accumulated(), pt.sample_counts().reshape(-1)
    assert set(np.unique(count)) == {SPP, 2 * SPP}
    want = acc / count.astype(F)[:, None]
    assert_bits(pt.mean(), want, "mean")
    t = torch.zeros(W_ * H_ * 3, dtype=torch.float32, device="cuda:0")
    assert_bits(pt.mean_to_tensor(t).cpu().numpy().reshape(-1, 3), want, "mean_to_tensor")
    pt.reset_progress()
    pt.set_active_mask(hand_mask("corner"))
    pt.render(SPP)
    m = pt.mean()
    assert m[-1].any() and not m[:-1].any(), "0 where the count is 0"
    assert_bits(pt.mean_to_tensor(t).cpu().numpy().reshape(-1, 3), m, "mean_to_tensor with zero counts")
    for bad in (torch.zeros(5, device="cuda:0"), torch.zeros(W_ * H_ * 3, dtype=torch.float64, device="cuda:0")):
        with pytest.raises((ValueError, TypeError)):
            pt.mean_to_tensor(bad)
    pt.close()


# ---------------------------------------------------------------- 8. resets
@pytest.mark.parametrize("loop", ["", "NO_GRAPH", "UNFUSED"])
def test_resets_restore_the_mask_and_the_counts(W, O, loop):
    fresh = tracer(W, O, "alone", loop, 0)
    fresh.render(SPP)
    want = fresh.accumulated()
    fresh.close()
    pt = tracer(W, O, "alone", loop, 0)
    pt.render(SPP)  # (the captured graph has replayed once)
    ref = masked_reference(O, "alone", 0, "checker")

    def reset_by_progress():
        pt.reset_progress()

    def reset_by_camera():
        pt.render_parameters.set_viewport((61, 37))
        pt.update_buffers()
        assert pt.active_mask().shape == (37, 61) and pt.active_mask().all() and not pt.sample_counts().any()
        pt.render_parameters.set_viewport((W_, H_))
        pt.update_buffers()

    def reset_by_scene():
        pt.update_scene(pt.scene)

    for reset in (reset_by_progress, reset_by_camera, reset_by_scene):
        pt.set_active_mask(hand_mask("checker"))
        pt.render(SPP)
        assert not pt.active_mask().all() and (pt.sample_counts().reshape(-1)[~hand_mask("checker")] == pt.sample_counts().min()).all()
        reset()
        what = f"{loop} {reset.__name__}"
        assert pt.active_mask().all() and not pt.sample_counts().any() and not pt.accumulated().any(), what
        assert not pt.variance().any(), what
        pt.render(SPP)
        if reset is not reset_by_scene:  # (the rebuilt tree of the reordered spheres is another tree: the mask and the counts are what is checked)
            assert_bits(pt.accumulated(), want, what + ": the frame after the reset")
        assert (pt.sample_counts() == SPP).all()
        pt.reset_progress()
    # a new mask on a context whose graph has replayed: the graph holds the buffer, not its contents
    pt.set_active_mask(hand_mask("checker"))
    pt.render(SPP)
    check(pt, ref, f"{loop}: a mask set after the graph was captured")
    pt.close()


# ---------------------------------------------------------------- 9. refusals
def test_refusals_leave_the_context_as_it_was(W, O):
    for other in ("AOV", "DENOISE", "BINNING"):
        with pytest.raises(W.WfptError):
            W.shirley_path_tracer(64, 48, rng_mode=W.RNG_PIXEL, flags=W.FLAG_ADAPTIVE | getattr(W, "FLAG_" + other))
    pt = W.shirley_path_tracer(64, 48, max_wavefronts=3, rng_mode=W.RNG_PIXEL)
    with pytest.raises(W.WfptError):
        W.render_chunked(pt.scene, pt.render_parameters, 1, 2, flags=W.FLAG_ADAPTIVE)
    # every new call on an unflagged context
    import torch
    t = torch.zeros(64 * 48 * 3, dtype=torch.float32, device="cuda:0")
    calls = (lambda: pt.set_adaptive(), pt.adaptive, pt.adaptive_update, lambda: pt.set_active_mask(np.ones(64 * 48)), pt.active_mask,
             pt.sample_counts, pt.mean, lambda: pt.mean_to_tensor(t), lambda: pt.render_adaptive(4, 2), pt.variance)
    pt.render(1)
    before = pt.accumulated()
    for call in calls:
        with pytest.raises(W.WfptError):
            call()
    assert_bits(pt.accumulated(), before, "an unflagged context")
    pt.close()
    # bad parameters, a wrong mask length
    pt = tracer(W, O, "alone", "", 0)
    assert pt.adaptive() == {k: (float(F(v)) if isinstance(v, float) else v) for k, v in A.DEFAULTS.items()}
    good = dict(min_samples=3, max_samples=9, threshold=0.25, luminance_floor=0.5, dilate=0)
    pt.set_adaptive(**good)
    pt.set_active_mask(hand_mask("checker"))
    pt.render(SPP)
    before, counts, mask = pt.accumulated(), pt.sample_counts(), pt.active_mask()
    for bad in (dict(threshold=0.0), dict(threshold=-1.0), dict(threshold=float("nan")), dict(threshold=float("inf")),
                dict(luminance_floor=0.0), dict(luminance_floor=float("nan")), dict(luminance_floor=-float("inf")),
                dict(min_samples=1), dict(min_samples=0), dict(min_samples=8, max_samples=7), dict(min_samples=16, max_samples=2)):
        with pytest.raises(W.WfptError):
            pt.set_adaptive(**{**good, **bad})
    p = W._AdaptiveParams(3, 9, 0.25, 0.5, 0)
    p._reserved[1] = 1
    L = W.lib()
    assert L.wfpt_set_adaptive(pt.handle, W.C.byref(p)) == -1 and L.wfpt_set_adaptive(pt.handle, None) == -1
    assert L.wfpt_get_adaptive(pt.handle, None) == -1 and L.wfpt_render_adaptive(pt.handle, 4, 0, None) == -1
    for n in (W_ * H_ - 1, W_ * H_ + 1, 0):
        with pytest.raises(W.WfptError):
            pt.set_active_mask(np.ones(n))
    buf = np.zeros(W_ * H_ + 8, np.uint8)
    assert L.wfpt_read_active_mask(pt.handle, buf.ctypes.data_as(W.C.c_void_p), W_ * H_ + 1) == -1
    assert L.wfpt_set_active_mask(pt.handle, None, W_ * H_) == -1 and L.wfpt_read_sample_counts(pt.handle, None, 4) == -1
    assert L.wfpt_read_sample_counts(pt.handle, buf.ctypes.data_as(W.C.c_void_p), W_ * H_ + 1) == -1
    assert L.wfpt_read_mean(pt.handle, buf.ctypes.data_as(W.C.c_void_p), 3 * W_ * H_ + 1) == -1
    assert pt.adaptive() == {k: (float(F(v)) if isinstance(v, float) else v) for k, v in good.items()}
    assert_bits(pt.accumulated(), before, "a refused call touched the accumulation")
    assert np.array_equal(pt.sample_counts(), counts) and np.array_equal(pt.active_mask(), mask)
    assert W.lib().wfpt_accumulated_samples(pt.handle) == SPP
    # a successful set_adaptive neither resets nor drops anything, and the context renders on as before
    pt.set_adaptive(**dict(good, threshold=0.5))
    assert_bits(pt.accumulated(), before, "set_adaptive reset the accumulation")
    pt.render(SPP)
    ref = Ref(O, "alone", 0).render(hand_mask("checker")).render()
    check(pt, ref, "after the refused calls")
    pt.close()


# ---------------------------------------------------------------- 10. the convenience loop
def test_render_adaptive_stops_at_max_passes_or_when_nothing_is_active(W, O):
    pt = tracer(W, O, "alone", "", 0)
    pt.set_adaptive(min_samples=100)  # nothing converges within these passes
    n = pt.render_adaptive(7, 3)
    assert W.lib().wfpt_accumulated_samples(pt.handle) == 7 and (pt.sample_counts() == 7).all(), "3 + 3 + 1 passes"
    assert n == int(pt.active_mask().sum()) > 0
    pt.reset_progress()
    pt.set_adaptive(min_samples=4, threshold=1e6, luminance_floor=1.0)  # everything converges at min_samples
    n = pt.render_adaptive(64, 2)
    assert n == 0 and not pt.active_mask().any()
    assert W.lib().wfpt_accumulated_samples(pt.handle) == 4 and (pt.sample_counts() == 4).all(), "the second update: the first with n >= min_samples"
    pt.reset_progress()
    pt.set_adaptive(min_samples=2, threshold=1e6, luminance_floor=1.0)
    assert pt.render_adaptive(64, 2) == 0 and W.lib().wfpt_accumulated_samples(pt.handle) == 2, "it stops after the first update"
    assert pt.render_adaptive(0, 1) == 0
    pt.close()
