"""Per-vertex shading normals (WFPT_FLAG_SHADING_NORMALS, include/wfpt.h "Shading normals") without a GPU: the restatement
(tests/shading_normals_ref.py) against the closed form of a sphere, against the plain oracle where the table is flat, and against three
mutations of itself; the OBJ loader's `vn` records; the host's normalisation of the table."""
import ctypes as C

import numpy as np
import pytest

import shading_normals_ref as S
import transport_ref
from conftest import assert_bit_equal

F = np.float32
W_, H_, SPP, WAVES = 61, 37, 3, 4


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def built(orc, emitter=False):
    t, mt, n9 = S.sphere_scene(orc, emitter=emitter)
    t, nodes = orc.build_bvh_triangles(t, 32)
    return t, mt, n9, nodes


def oracle_of(orc, t, mt, nodes, w=W_, h=H_, **kw):
    cam, ip, vw = S.sphere_camera(orc, w, h)
    return orc.Oracle(w, h, np.zeros(1, orc.SPHERE), mt, nodes, cam, ip, vw, triangles=t, max_wavefronts=WAVES, **kw)


def test_icosphere_is_wound_outward_and_inscribed():
    tri = S.icosphere(2)
    assert tri.shape == (320, 3, 3)
    assert np.allclose(np.linalg.norm(tri, axis=2), 1.0, atol=1e-12)
    out = np.einsum("ij,ij->i", np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), tri.mean(axis=1))
    assert (out > 0).all()


def test_closed_form_on_a_sphere(orc):
    """Corner normals = corner positions on the unit sphere: the interpolant of the positions is p itself, so ns = normalize(p) but for
    rounding (1.6e-7 in numpy float32); the stored normal is off by up to 0.17 there."""
    tri = S.icosphere(2)
    t = np.zeros(len(tri), orc.TRIANGLE)
    t["v0"], t["e1"], t["e2"] = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    t["_pad"] = np.arange(len(t))
    normals = S.Normals(t, tri.reshape(-1, 9))
    rng = np.random.default_rng(3)
    prim = rng.integers(0, len(t), 20000)
    b = rng.dirichlet((1.0, 1.0, 1.0), 20000)
    p = np.einsum("ij,ijk->ik", b, tri[prim]).astype(F)
    ns, fell = normals.at(prim, p)
    want = p.astype(np.float64) / np.linalg.norm(p.astype(np.float64), axis=1)[:, None]
    err = np.abs(ns - want).max()
    flat = np.abs(transport_ref.triangle_normal_area(t[prim])[0] - want).max()
    print(f"closed form: max |ns - normalize(p)| = {err:.3g}, the stored normal is off by up to {flat:.3g}")
    assert not fell.any()
    assert err <= 1e-5
    assert 0.1 < flat < 0.2


def test_steps_edge_rows(orc):
    """step 5's fall-backs, and step 1's den <= 0, in the restatement itself"""
    t = np.zeros(3, orc.TRIANGLE)
    t["v0"][:] = (0, 0, 0)
    t["e1"][:] = (1, 0, 0)
    t["e2"][:] = (0, 1, 0)
    t["e2"][2] = (2, 0, 0)  # degenerate: den = 0, the stored normal is NaN
    t["_pad"] = (0, 1, 2)
    n9 = np.zeros((3, 9), F)
    n9[0] = (0, 0, 1, 1, 0, 1, 0, 1, 1)
    n9[1] = (0, 0, -1, 0, 0, -1, 0, 0, -1)  # faces away from ng
    n9[2] = (0, 0, 1, 0, 0, 1, 0, 0, 1)
    nm = S.Normals(t, n9)
    ns, fell = nm.at([0, 0, 0], [(0, 0, 0), (1, 0, 0), (0, 1, 0)])
    assert not fell.any()
    assert np.abs(ns - nm.rows[0].reshape(3, 3)).max() < 2e-7, "corners give the corner normals (normalised once more)"
    ns, fell = nm.at([1, 0], [(0.25, 0.25, 0), (np.nan, 0, 0)])
    assert fell.all() and np.array_equal(ns, [(0, 0, 1), (0, 0, 1)])
    ns, fell = nm.at([2], [(0.5, 0, 0)])
    assert fell.all() and np.isnan(ns).all()
    ns, fell = S.Normals(t, np.zeros((3, 9), F)).at([0], [(0.25, 0.25, 0)])
    assert fell.all() and np.array_equal(ns, [(0, 0, 1)])


@pytest.mark.parametrize("rng_mode", [0, 1])
def test_flat_table_is_the_plain_oracle_bit_for_bit(orc, rng_mode):
    """An all-zero table: every hit falls back to the stored normal, so the restated scatter() must give the oracle's own extension rays
    for all three materials -- the restatement's frame is the oracle's."""
    t, mt, n9, nodes = built(orc)
    want = oracle_of(orc, t, mt, nodes, rng_mode=rng_mode).render(SPP)
    o = S.Shaded(oracle_of(orc, t, mt, nodes, rng_mode=rng_mode), S.Normals(t, np.zeros_like(n9)), mt)
    got = transport_ref.render(o, spp=SPP)
    assert_bit_equal(got, want, "flat table")
    hit = np.concatenate([np.array(tab)[:, 1] for tab in o.tables])
    assert hit.sum() > 3000, "the scene was hardly hit"


def test_mutations_change_the_frame(orc):
    t, mt, n9, nodes = built(orc)

    def frame(normals, **kw):
        return transport_ref.render(S.Shaded(oracle_of(orc, t, mt, nodes, rng_mode=1), normals, mt, **kw), spp=SPP)

    want = frame(S.Normals(t, n9))
    plain = oracle_of(orc, t, mt, nodes, rng_mode=1).render(SPP)
    assert not np.array_equal(want.view(np.uint32), plain.view(np.uint32)), "the table changed nothing"
    assert_bit_equal(frame(S.Normals(t, n9), keep_geometric=True), plain, "the stored normal kept in scatter is the plain frame")
    for name in ("keep_unnormalised", "swap_b"):
        got = frame(S.Normals(t, n9, **{name: True}))
        assert not np.array_equal(got.view(np.uint32), want.view(np.uint32)), name


def test_nee_receiver_normal_is_substituted(orc):
    """With the connect pass the shading normal is the receiver's normal too: the substitution changes the frame, and leaves
    transport_ref as it was."""
    import emission_ref as E
    import nee_ref as N
    t, mt, n9, nodes = built(orc, emitter=True)
    em = E.Emission({4: (8.0, 8.0, 8.0)}, triangles=t, materials=mt)
    nm = S.Normals(t, n9)

    def frame(substitute):
        o = S.Shaded(oracle_of(orc, t, mt, nodes, rng_mode=1, miss_floor=0), nm, mt)
        shadow = oracle_of(orc, t, mt, nodes, rng_mode=1)
        if not substitute:
            return N.render_with_nee(o, shadow, em, spp=2)
        with S.shading_receivers(nm):
            return N.render_with_nee(o, shadow, em, spp=2)

    keep = transport_ref.hit_normal
    a, b = frame(True), frame(False)
    assert transport_ref.hit_normal is keep
    assert not np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---------------------------------------------------------------- the host library: normalisation and the loader
def test_host_normalisation_equals_restatement(wf):
    rng = np.random.default_rng(5)
    n9 = rng.normal(size=(500, 9)).astype(F)
    n9[:50] *= F(1e-3)
    n9[50:100] *= F(1e6)
    n9[100] = 0
    n9[101, :3] = (1e30, 1e30, 0)      # l2 overflows: stored as zero
    n9[102, :3] = (1e-30, 0, 1e-30)    # l2 underflows to 0: stored as zero
    n9[103, :3] = (-0.0, 0.0, 3.0)
    n9[104, :3] = (1e-20, 0, 0)        # l2 is subnormal: still normalised
    out = np.zeros_like(n9)
    assert wf.lib().wfpt_normalize_triangle_normals(_p(n9), len(n9), _p(out)) == 0
    assert_bit_equal(out, S.normalize_rows(n9), "stored rows")
    assert not out[100].any() and not out[101, :3].any() and not out[102, :3].any()
    assert abs(out[104, 0] - 1) < 1e-4 and not out[104, 1:3].any()  # (a subnormal l2 keeps few bits)
    lens = np.delete(np.linalg.norm(out.reshape(-1, 3).astype(np.float64), axis=1), 3 * 104)
    assert (np.abs(lens[lens > 0] - 1) < 1e-6).all()
    for bad in (np.nan, np.inf, -np.inf):
        n9[7, 4] = bad
        assert wf.lib().wfpt_normalize_triangle_normals(_p(n9), len(n9), _p(out)) == -1


OBJ = """# a quad and two triangles
v 0 0 0
v 1 0 0
v 1 1 0
v 0 1 0
vt 0 0
vt 1 0
vt 1 1
vt 0 1
vn 0 0 1
vn 0 0 2
vn 1 0 1
vn 0 0 -1
f 1/1/1 2/2/2 3/3/3 4/4/1
f 1//1 -3//-3 3
f 1/1/4 2/2/4 3/3/-1
f 1 2 4
"""


def test_loader_reads_normals_swaps_winding_and_fills_gaps(wf, tmp_path):
    path = tmp_path / "n.obj"
    path.write_text(OBJ)
    scene, uv, n9 = wf.Scene.load_obj(str(path), uvs=True, normals=True)
    t = scene.triangles
    assert len(t) == 5 and n9.shape == (5, 9) and uv.shape == (5, 6)
    assert np.array_equal(t["_pad"], np.arange(5))
    # the fan of the quad: (1, 2, 3) and (1, 3, 4), with their t and n
    assert np.array_equal(n9[0], (0, 0, 1, 0, 0, 2, 1, 0, 1)) and np.array_equal(n9[1], (0, 0, 1, 1, 0, 1, 0, 0, 1))
    assert np.array_equal(uv[0], (0, 0, 1, 0, 1, 1)) and np.array_equal(uv[1], (0, 0, 1, 1, 0, 1))
    assert np.array_equal(t["e1"][0], (1, 0, 0)) and np.array_equal(t["e2"][0], (1, 1, 0))
    # i//n with negative indices (-3 of four = the second), and a corner without a vn: the face's own normal
    assert np.array_equal(n9[2], (0, 0, 1, 0, 0, 2, 0, 0, 1)) and not uv[2].any()
    # a face wound against its vn: e1 and e2 swapped, rows 1 and 2 swapped with them, in n9 and uv
    assert np.array_equal(t["e1"][3], (1, 1, 0)) and np.array_equal(t["e2"][3], (1, 0, 0))
    assert np.array_equal(n9[3], (0, 0, -1, 0, 0, -1, 0, 0, -1)) and np.array_equal(uv[3], (0, 0, 1, 1, 1, 0))
    assert np.cross(t["e1"][3], t["e2"][3])[2] < 0
    # plain `i` entries: the face's own normal at every corner
    assert np.array_equal(n9[4], (0, 0, 1) * 3)
    # without uvs the same triangles and normals; the plain loaders see the file as before
    scene2, n9b = wf.Scene.load_obj(str(path), normals=True)
    assert np.array_equal(n9b, n9) and np.array_equal(scene2.triangles, t)
    plain, uv_plain = wf.Scene.load_obj(str(path), uvs=True)
    assert np.array_equal(plain.triangles["e1"][3], (1, 0, 0)) and np.array_equal(uv_plain[3], (0, 0, 1, 0, 1, 1))
    assert len(wf.Scene.from_obj(str(path)).triangles) == 5
    # capacity and index errors
    n = C.c_uint32()
    assert wf.lib().wfpt_load_obj_normals(str(path).encode(), None, None, None, 0, C.byref(n), 0, 0) == 0 and n.value == 5
    small = np.zeros(2, wf.TRIANGLE)
    assert wf.lib().wfpt_load_obj_normals(str(path).encode(), _p(small), None, _p(np.zeros((2, 9), F)), 2, C.byref(n), 0, 0) == -1
    assert wf.lib().wfpt_load_obj_normals(str(path).encode(), _p(np.zeros(5, wf.TRIANGLE)), None, None, 5, C.byref(n), 0, 0) == -1
    bad = tmp_path / "bad.obj"
    bad.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nvn 0 0 1\nf 1//1 2//2 3//1\n")
    assert wf.lib().wfpt_load_obj_normals(str(bad).encode(), None, None, None, 0, C.byref(n), 0, 0) == -1


def test_loaded_normals_feed_the_restatement(wf, tmp_path):
    """an icosphere written with its vn records comes back with corner normals = corner positions and no winding swapped"""
    tri = S.icosphere(1)
    tri = tri.astype(F).astype(np.float64)  # what a float reads back from nine digits
    lines = [f"{k} {x:.9g} {y:.9g} {z:.9g}" for k in ("v", "vn") for x, y, z in tri.reshape(-1, 3).tolist()]
    lines += [f"f {3 * i + 1}//{3 * i + 1} {3 * i + 2}//{3 * i + 2} {3 * i + 3}//{3 * i + 3}" for i in range(len(tri))]
    path = tmp_path / "ico.obj"
    path.write_text("\n".join(lines) + "\n")
    scene, n9 = wf.Scene.load_obj(str(path), normals=True)
    assert_bit_equal(n9, tri.reshape(-1, 9).astype(F), "normals as the file gives them")
    assert_bit_equal(scene.triangles["v0"], tri[:, 0].astype(F), "v0")
    assert_bit_equal(scene.triangles["e1"], tri[:, 1].astype(F) - tri[:, 0].astype(F), "e1 (not swapped)")
