"""The per-tile candidate lists of the first fused launch (include/wfpt.h "Tile lists"; csrc/wfpt_tile_lists.h), checked without a GPU
through the host twin of the device builder:
  * conservative: every leaf whose margin-grown box a primary ray of the oracle hits is in that ray's tile record (or the tile has none);
  * not by falling back: at most a quarter of the tiles at 128x72 without a list; tight at the size bench.py times;
  * the list walk itself -- candidates in list order, both roots, the two-sided tie watch, one leaf-box verdict, the hand-over -- as a
    numpy model in float32, against the reference's own walk (Oracle.trace_bvh): same primitive, same distance bits;
  * the host twin under AddressSanitizer + UBSan, as a stand-alone program (tests/cpp/tile_lists_host.cpp)."""
import os
import subprocess

import numpy as np
import pytest

from helpers import adversarial_rays, inputs_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
HAND_OVER, NO_HIT = 0xFFFFFFFE, 0xFFFFFFFF


def case_inputs(O, kind, w, h):
    """(spheres, materials, nodes, camera, inv_proj, view) of a case; "pinhole": the book camera with defocus 0."""
    if kind == "pinhole":
        sp, mt, nodes = inputs_for(O, "shirley", w, h)[:3]
        return (sp, mt, nodes) + tuple(O.camera((13.0, 2.0, 3.0), (0.0, 0.0, 0.0), 20.0, 0.0, 10.0, 0.1, 100.0, w, h))
    return inputs_for(O, kind, w, h)


def oracle_primary_rays(O, inputs, w, h, frame):
    """generate_rays' output of one frame at true size, in slot order (slot >> 6 = the tile), with the padding lanes."""
    sp, mt, nodes, cam, ip, vw = inputs
    o = O.Oracle(w, h, sp, mt, nodes, cam, ip, vw)
    gx, gy = (w + 7) // 8, (h + 7) // 8
    o.set_frame(frame)
    o.generate_rays(gx, gy, true_size=True)
    rays = o.rays(gx * gy * 64)
    o.close()
    return rays


def leaves_of(ch):
    """(node indices, leaf words) of the leaves of a nodes_ch array, in node order."""
    lf, pc = ch[:, 3].view(np.uint32), ch[:, 7].view(np.uint32)
    idx = np.array([i for i in range(len(ch)) if i != 1 and pc[i] != 0])
    return idx, (lf[idx] | (pc[idx] << 16)).astype(np.uint32)


def boxes_hit(ch, idx, rays):
    """[ray, leaf]: does the ray (t >= 0) meet the margin-grown box? Slab test in float64."""
    o = rays["origin"][:, None, :3].astype(np.float64)
    d = rays["direction"][:, None, :3].astype(np.float64)
    lo = (ch[idx, 0:3].astype(np.float64) - ch[idx, 4:7].astype(np.float64))[None]
    hi = (ch[idx, 0:3].astype(np.float64) + ch[idx, 4:7].astype(np.float64))[None]
    with np.errstate(all="ignore"):
        t0, t1 = (lo - o) / d, (hi - o) / d
    t0 = np.where(np.isnan(t0), -np.inf, t0)  # (0 / 0: the origin lies on the plane of an axis the ray does not move along)
    t1 = np.where(np.isnan(t1), np.inf, t1)
    tmin, tmax = np.minimum(t0, t1).max(axis=2), np.maximum(t0, t1).min(axis=2)
    return tmax >= np.maximum(tmin, 0.0)


CASES = [("shirley", 128, 72), ("shirley", 64, 40), ("shirley", 60, 44), ("simple", 64, 64), ("pinhole", 128, 72), ("pinhole", 60, 44)]


@pytest.mark.parametrize("kind,w,h", CASES)
def test_every_leaf_a_primary_ray_reaches_is_in_its_tile_record(wf, orc, kind, w, h):
    inputs = case_inputs(orc, kind, w, h)
    nodes, cam, ip, vw = inputs[2:]
    ch = wf.nodes_ch(nodes, cam)
    rec = wf.tile_lists_host(nodes, cam, ip, vw, w, h)
    idx, words = leaves_of(ch)
    listed = (rec[:, :, None] == words[None, None, :]).any(axis=1)  # [tile, leaf]
    no_list = rec[:, 0] == wf.TILE_NO_LIST
    n_checked = 0
    for frame in range(1, 9):
        rays = oracle_primary_rays(orc, inputs, w, h, frame)
        tile = np.arange(len(rays)) >> 6
        live = rays["pixel_idx"] != orc.INACTIVE_PIXEL
        for s in range(0, len(rays), 2048):
            sl = slice(s, s + 2048)
            need = boxes_hit(ch, idx, rays[sl]) & live[sl, None]
            missing = need & ~listed[tile[sl]] & ~no_list[tile[sl], None]
            assert not missing.any(), (kind, w, h, frame, "ray slot, leaf:", np.argwhere(missing)[:4] + [s, 0])
            n_checked += int(need.sum())
    assert n_checked > 0
    if kind != "simple":  # (its five spheres: the root's children are all there is)
        assert not no_list.all()


def test_the_lists_do_not_pass_by_falling_back(wf, orc):
    """128x72: the union over 8 frames of the leaves the rays reach alone leaves 5 % of the tiles above the cap; a bound that pushes it
    past a quarter is too loose."""
    w, h = 128, 72
    nodes, cam, ip, vw = case_inputs(orc, "shirley", w, h)[2:]
    rec = wf.tile_lists_host(nodes, cam, ip, vw, w, h)
    frac = float((rec[:, 0] == wf.TILE_NO_LIST).mean())
    print(f"128x72: {frac:.3f} of the tiles without a list")
    assert frac <= 0.25


def test_tight_at_the_size_that_is_timed(wf, orc):
    """1920x1080, the book camera: the empirical union is 2.84 leaves per tile (maximum 11), 3.47 with 0.05 of padding."""
    w, h = 1920, 1080
    nodes, cam, ip, vw = case_inputs(orc, "shirley", w, h)[2:]
    rec = wf.tile_lists_host(nodes, cam, ip, vw, w, h)
    no_list = rec[:, 0] == wf.TILE_NO_LIST
    length = (rec[~no_list] != 0).sum(axis=1)
    print(f"1920x1080: mean list length {length.mean():.3f}, maximum {length.max()}, {no_list.mean():.5f} of the tiles without a list")
    assert length.mean() <= 4.5
    assert no_list.mean() <= 0.01


def test_records_are_well_formed(wf, orc):
    """Leaf words in ascending node order, then zeros; a tile without a list is the marker and zeros."""
    w, h = 64, 40
    nodes, cam, ip, vw = case_inputs(orc, "shirley", w, h)[2:]
    rec = wf.tile_lists_host(nodes, cam, ip, vw, w, h)
    idx, words = leaves_of(wf.nodes_ch(nodes, cam))
    order = {int(wd): k for k, wd in enumerate(words)}
    for r in rec:
        if r[0] == wf.TILE_NO_LIST:
            assert not r[1:].any()
            continue
        n = int((r != 0).sum())
        assert r[:n].all() and not r[n:].any()
        pos = [order[int(x)] for x in r[:n]]
        assert pos == sorted(set(pos))
    # sharded by bands: rank r of n holds the records of its own bands
    full = wf.tile_lists_host(nodes, cam, ip, vw, w, h).reshape(5, 8, -1)
    for rank in range(3):
        part = wf.tile_lists_host(nodes, cam, ip, vw, w, h, tile_rank=rank, tile_world=3)
        assert np.array_equal(part.reshape(-1, 8, 16), full[rank::3])


# ---------------------------------------------------------------- the list walk, as a numpy model in float32
def safe_region(spheres, nodes, cam):
    """wfpt_api.hip's safe_region (the ball of origins the free walks are proven for), a shade inside it."""
    reach = np.abs(cam["position"][0][:3]) + max(float(cam["defocus_radius"][0]), 0.0)
    keep = np.arange(len(nodes)) != 1
    extent = np.maximum(0.25 * reach, np.maximum(np.abs(nodes["aabb_min"][keep]).max(axis=0), np.abs(nodes["aabb_max"][keep]).max(axis=0)))
    c, r = spheres["center"][:, :3].astype(np.float64), np.abs(spheres["radius"].astype(np.float64))
    rest = np.arange(len(c)) != int(np.argmax(r)) if len(c) > 1 else np.ones(len(c), bool)
    centre = (0.5 * (c[rest].min(axis=0) + c[rest].max(axis=0))).astype(np.float32)
    margin = 0.875 * float(extent.min()) * 2.0 ** -17
    radius = float((np.sqrt(margin * r / (6.0 * 2.0 ** -24)) - np.linalg.norm(c - centre, axis=1)).min()) * 0.999
    return centre, (F(radius * radius) if radius > 0 else F(-1.0))


def list_walk(spheres, records, tile, rays, centre, r2):
    """trace_tile_list of wfpt_kernels.hip over `rays` (ray k reads records[tile[k]]): (t, primitive) with HAND_OVER where the ray goes
    to the reference's walk. Every operation in float32, in the kernel's order."""
    n = len(rays)
    o, d = rays["origin"][:, :3].astype(F), rays["direction"][:, :3].astype(F)
    sc, sr = spheres["center"][:, :3].astype(F), spheres["radius"].astype(F)
    a = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    nearest, best, best_leaf = np.full(n, F(1e30)), np.full(n, NO_HIT, np.uint32), np.zeros(n, np.uint32)
    f = o - centre
    far = (f[:, 0] * f[:, 0] + f[:, 1] * f[:, 1]) + f[:, 2] * f[:, 2] > r2
    eps = F(0.001)

    def near_tie(t):
        return np.abs(t - nearest) <= nearest * F(3.8146973e-6)

    def watch_and_take(t, act, idx):
        nonlocal nearest, best
        tie = act & (t > eps) & near_tie(t)
        nearest = np.where(tie, F(-1.0), nearest)
        best = np.where(tie, np.uint32(HAND_OVER), best)
        take = act & (t > eps) & (t < nearest)
        nearest = np.where(take, t, nearest)
        best = np.where(take, idx, best)
        return take

    with np.errstate(all="ignore"):
        for k in range(records.shape[1]):
            word = np.where(far, np.uint32(0), records[tile, k])
            first, count = word & 0xFFFF, word >> 16
            before = best.copy()
            for i in range(int(count.max()) if n else 0):
                act = i < count
                idx = np.where(act, first + i, 0).astype(np.uint32)
                oc = o - sc[idx]
                b = (d[:, 0] * oc[:, 0] + d[:, 1] * oc[:, 1]) + d[:, 2] * oc[:, 2]
                c = ((oc[:, 0] * oc[:, 0] + oc[:, 1] * oc[:, 1]) + oc[:, 2] * oc[:, 2]) - sr[idx] * sr[idx]
                disc = b * b - a * c
                act = act & (disc >= 0)
                sq = np.sqrt(np.where(act, disc, F(0.0)))
                took = watch_and_take((-b - sq) / a, act, idx)
                watch_and_take((-b + sq) / a, act & ~took, idx)
            best_leaf = np.where(best != before, word, best_leaf)
        # the verdict: the final hit's leaf box, recomputed from its primitives, under the reference's own test (ex:164-183)
        judged = best < HAND_OVER
        lo, hi = np.full((n, 3), F(np.inf)), np.full((n, 3), F(-np.inf))
        first, count = best_leaf & 0xFFFF, best_leaf >> 16
        for i in range(int(count[judged].max()) if judged.any() else 0):
            act = (judged & (i < count))[:, None]
            idx = np.where(act[:, 0], first + i, 0)
            lo = np.where(act, np.fmin(lo, sc[idx] - sr[idx, None]), lo)
            hi = np.where(act, np.fmax(hi, sc[idx] + sr[idx, None]), hi)
        inv = F(1.0) / d
        t0, t1 = (lo - o) * inv, (hi - o) * inv
        tmin, tmax = np.fmin(t0[:, 0], t1[:, 0]), np.fmax(t0[:, 0], t1[:, 0])
        for ax in (1, 2):
            tmin = np.fmax(np.fmin(t0[:, ax], t1[:, ax]), tmin)
            tmax = np.fmin(np.fmax(t0[:, ax], t1[:, ax]), tmax)
        fail = judged & ((tmin > tmax) | (tmax <= 0) | (tmin > nearest))
    best = np.where(fail | far, np.uint32(HAND_OVER), best)
    return nearest, best


def compare_with_the_reference_walk(O, inputs, w, h, rays, t, prim):
    sp, mt, nodes, cam, ip, vw = inputs
    o = O.Oracle(w, h, sp, mt, nodes, cam, ip, vw)
    handed = 0
    for k in range(len(rays)):
        if prim[k] == HAND_OVER:  # the kernel's retrace_reference is this walk
            handed += 1
            continue
        hit, out = o.trace_bvh(rays[k])
        if prim[k] == NO_HIT:
            assert not hit, (k, rays[k], out)
        else:
            assert hit and int(out["sphere_idx"]) == int(prim[k]) and F(out["t"]).view(np.uint32) == F(t[k]).view(np.uint32), (k, rays[k], out, t[k], prim[k])
    o.close()
    return handed


@pytest.mark.parametrize("kind,w,h", [("shirley", 64, 40), ("simple", 64, 64), ("pinhole", 60, 44)])
def test_list_walk_model_equals_the_reference_walk_on_primary_rays(wf, orc, kind, w, h):
    inputs = case_inputs(orc, kind, w, h)
    sp, _, nodes, cam, ip, vw = inputs
    rec = wf.tile_lists_host(nodes, cam, ip, vw, w, h)
    rays = oracle_primary_rays(orc, inputs, w, h, 1)
    tile = np.arange(len(rays)) >> 6
    keep = (rays["pixel_idx"] != orc.INACTIVE_PIXEL) & (rec[tile, 0] != wf.TILE_NO_LIST)
    assert keep.sum() > 500 or kind == "simple"
    rays, tile = rays[keep], tile[keep]
    centre, r2 = safe_region(sp, nodes, cam)
    t, prim = list_walk(sp, rec, tile, rays, centre, r2)
    handed = compare_with_the_reference_walk(orc, inputs, w, h, rays, t, prim)
    assert handed <= len(rays) // 100, "the model hands over more than a stray ray: it would prove nothing"


@pytest.mark.parametrize("kind", ["shirley", "simple"])
def test_list_walk_model_equals_the_reference_walk_on_adversarial_rays(wf, orc, kind):
    """helpers.adversarial_rays against ONE record that holds every leaf (no cap): whatever order the candidates come in, what the walk
    keeps is the reference's hit, or the ray is handed over."""
    w, h = 64, 64
    inputs = case_inputs(orc, kind, w, h)
    sp, _, nodes, cam = inputs[:4]
    _, words = leaves_of(wf.nodes_ch(nodes, cam))
    rays = adversarial_rays(wf, sp, nodes, 1200)
    centre, r2 = safe_region(sp, nodes, cam)
    t, prim = list_walk(sp, words[None, :], np.zeros(len(rays), np.int64), rays, centre, r2)
    handed = compare_with_the_reference_walk(orc, inputs, w, h, rays, t, prim)
    print(f"{kind}: {len(rays) - handed} of {len(rays)} adversarial rays compared, {handed} handed over")
    assert handed <= len(rays) // 2, "more than half of the rays handed over: too little compared"


# ---------------------------------------------------------------- the host twin under the sanitizers, as a program of its own
def test_host_twin_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "san_tile_lists")
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off"]
    cmd = ["g++", "-std=c++17", *san, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "tile_lists_host.cpp"),
           os.path.join(ROOT, "wavefront_path_tracer_amd", "csrc", "wfpt_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-4000:]
