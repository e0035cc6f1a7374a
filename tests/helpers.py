"""Builders shared by the parity tests: the same scene / camera / parameters for oracle and product."""
import numpy as np


def shirley_inputs(O, width, height, seed=1):
    sp, mt = O.scene_book_one_final(seed)
    sp, nodes = O.build_bvh(sp)
    cam, ip, vw = O.shirley_camera(width, height)
    return sp, mt, nodes, cam, ip, vw


def simple_inputs(O, width, height):
    """scene.rs:12-46 (5 spheres, all three materials, nested dielectric) with the commented-out camera of
    main.rs:21-22: (0,0,1) looking at (0,0,-1); vfov 90, no defocus."""
    sp, mt = O.scene_new()
    sp, nodes = O.build_bvh(sp)
    cam, ip, vw = O.camera((0.0, 0.0, 1.0), (0.0, 0.0, -1.0), 90.0, 0.0, 10.0, 0.1, 100.0, width, height)
    return sp, mt, nodes, cam, ip, vw


def make_oracle(O, inputs, width, height, **kw):
    sp, mt, nodes, cam, ip, vw = inputs
    return O.Oracle(width, height, sp, mt, nodes, cam, ip, vw, **kw)


def make_tracer(W, kind, width, height, seed=1, **kw):
    """Product-side PathTracer on the same inputs (its own host code builds scene, BVH and camera)."""
    if kind == "shirley":
        return W.shirley_path_tracer(width, height, seed=seed, **kw)
    scene = W.Scene.new()
    cc = W.CameraController(W.Camera((0.0, 0.0, 1.0), (0.0, 0.0, -1.0)), 90.0, 0.0, 10.0, 0.1, 100.0)
    return W.PathTracer(scene, W.RenderParameters(cc, (width, height)), **kw)


def inputs_for(O, kind, width, height, seed=1):
    return shirley_inputs(O, width, height, seed) if kind == "shirley" else simple_inputs(O, width, height)


def sorted_rays(r):
    return np.sort(r, order=["pixel_idx"])


def mesh_inputs(O, width, height, n_triangles, edge_scale=1.0, seed=1, n_bins=32):
    """BASELINE config 5's triangle soup (optionally with longer edges so that small meshes get hit)."""
    tris, mt = O.scene_random_mesh(n_triangles, seed)
    if edge_scale != 1.0:
        tris["e1"] *= np.float32(edge_scale)
        tris["e2"] *= np.float32(edge_scale)
    tris, nodes = O.build_bvh_triangles(tris, n_bins)
    cam, ip, vw = O.mesh_camera(width, height)
    return tris, mt, nodes, cam, ip, vw


def make_mesh_oracle(O, inputs, width, height, **kw):
    tris, mt, nodes, cam, ip, vw = inputs
    return O.Oracle(width, height, np.zeros(1, O.SPHERE), mt, nodes, cam, ip, vw, triangles=tris, **kw)


def make_mesh_tracer(W, width, height, n_triangles, edge_scale=1.0, seed=1, n_bins=32, **kw):
    scene = W.Scene.random_mesh(n_triangles, seed)
    if edge_scale != 1.0:
        scene.triangles["e1"] *= np.float32(edge_scale)
        scene.triangles["e2"] *= np.float32(edge_scale)
    cc = W.CameraController(W.Camera((0.0, 0.0, 30.0), (0.0, 0.0, 0.0)), 40.0, 0.0, 10.0, 0.1, 100.0)
    return W.PathTracer(scene, W.RenderParameters(cc, (width, height)), mesh_bins=n_bins, **kw)


# ---- rays and a scene built to sit on the edges of the free walks' equivalence argument (tests/test_gpu_round3.py,
# tests/test_traversal_model.py)
def next_ulp(x, k):
    """x moved by k ulps (float32)."""
    x = np.float32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, np.float32(np.inf if k > 0 else -np.inf), dtype=np.float32)
    return x


def adversarial_rays(W, spheres, nodes, n_max):
    """Rays the conservative-box argument has to survive: head-on at the face centres of leaf and inner
    boxes (two direction components exactly zero: infinite inverses), origins exactly on the box planes at the tops / sides
    of spheres travelling along the plane (grazing), rays passing the centre of a sphere at r (1 +- k ulp) (near-tangent,
    where the exact test decides by the last bit), the same tilted by a few ulp, and rays towards pairs of spheres whose
    hits differ by a few ulp."""
    rays = []

    def add(o, d):
        rays.append((np.asarray(o, np.float32), np.asarray(d, np.float32)))

    axes = np.eye(3, dtype=np.float32)
    boxes = [(nd["aabb_min"], nd["aabb_max"]) for i, nd in enumerate(nodes) if i != 1]
    rng = np.random.default_rng(3)
    for lo, hi in boxes[: n_max // 40]:
        c = (lo + hi) * np.float32(0.5)
        for ax in range(3):
            for sgn in (-1.0, 1.0):
                o = c.copy()
                o[ax] = (hi[ax] + np.float32(3.0)) if sgn < 0 else (lo[ax] - np.float32(3.0))
                add(o, axes[ax] * np.float32(sgn))                       # head-on at the face centre, axis-parallel
                d = axes[ax] * np.float32(sgn)
                d[(ax + 1) % 3] = np.float32(1e-7)
                add(o, d)                                                 # almost axis-parallel: huge inverse
                e = c.copy()                                              # along an EDGE of the box, in the face plane
                e[ax] = hi[ax] if sgn > 0 else lo[ax]
                e[(ax + 1) % 3] = lo[(ax + 1) % 3] - np.float32(2.0)
                add(e, axes[(ax + 1) % 3])
    pick = rng.permutation(len(spheres))[: n_max // 60]
    for i in pick:
        c = spheres["center"][i][:3].astype(np.float32)
        r = np.float32(spheres["radius"][i])
        for ax in range(3):
            t_ax = (ax + 1) % 3
            for k in (-4, -2, -1, 0, 1, 2, 4):
                # origin on (or k ulp off) the plane that touches the sphere at its extreme point on axis `ax`, travelling in the plane
                o = c.copy()
                o[ax] = next_ulp(c[ax] + r, k)
                o[t_ax] = c[t_ax] - np.float32(2.0) * r - np.float32(1.0)
                add(o, axes[t_ax])
                d = axes[t_ax].copy()
                d[ax] = np.float32(k) * np.float32(1e-8)                  # tilted by next to nothing towards / away from the sphere
                add(o, d)
            # near-tangent in a random direction: pass the centre at distance r (1 + k 2^-23)
            u = rng.normal(size=3).astype(np.float32)
            u /= np.float32(np.linalg.norm(u))
            v = np.cross(u, rng.normal(size=3)).astype(np.float32)
            v /= np.float32(np.linalg.norm(v))
            for k in (-3, -1, 0, 1, 3):
                p = c + v * (r * (np.float32(1.0) + np.float32(k) * np.float32(2.0 ** -23)))
                add(p - u * np.float32(5.0), u)
    # neighbours: rays through the midpoints between close sphere pairs (two hits within a few ulp of each other are most
    # likely where spheres nearly touch or overlap)
    cs = spheres["center"][:, :3].astype(np.float64)
    for i in pick[:40]:
        dist = np.linalg.norm(cs - cs[i], axis=1)
        dist[i] = np.inf
        j = int(np.argmin(dist))
        m = ((cs[i] + cs[j]) * 0.5).astype(np.float32)
        for _ in range(4):
            u = rng.normal(size=3).astype(np.float32)
            u /= np.float32(np.linalg.norm(u))
            add(m - u * np.float32(4.0), u)
    rays = rays[:n_max]
    out = np.zeros(len(rays), W.RAY)
    for k, (o, d) in enumerate(rays):
        out["origin"][k, :3] = o
        out["origin"][k, 3] = 1.0
        out["direction"][k, :3] = d
    with np.errstate(all="ignore"):
        out["inv_direction"] = (np.float32(1.0) / out["direction"][:, :3]).astype("<f4")
    out["pixel_idx"] = np.arange(len(out), dtype="<u4") % 1024
    return out


def close_pairs_scene(orc):
    """A scene made for ties: pairs of spheres whose centres differ by 1-4 ulp (equal radii), nested and overlapping
    spheres, plus a ground sphere; BVH built by the oracle's builder."""
    rng = np.random.default_rng(11)
    sp = np.zeros(81, orc.SPHERE)
    mt = np.zeros(3, orc.MATERIAL)
    mt["albedo"][:] = (0.7, 0.6, 0.5, 1.0)
    mt["material_type"] = (0, 1, 2)
    mt["refract_index"][2] = 1.5
    sp["center"][0] = (0.0, -1000.0, 0.0, 1.0)
    sp["radius"][0] = 1000.0
    for k in range(40):
        c = rng.uniform(-6, 6, 3).astype(np.float32)
        c[1] = np.float32(abs(c[1]) * 0.3 + 0.5)
        r = np.float32(rng.uniform(0.2, 0.6))
        c2 = c.copy()
        c2[k % 3] = next_ulp(c2[k % 3], 1 + k % 4)
        sp["center"][1 + 2 * k, :3], sp["center"][2 + 2 * k, :3] = c, c2
        sp["radius"][1 + 2 * k] = r
        sp["radius"][2 + 2 * k] = r if k % 2 == 0 else next_ulp(r, 1)
    sp["center"][:, 3] = 1.0
    sp["material_idx"] = np.arange(len(sp)) % 3
    sp["material_type"] = np.arange(len(sp)) % 3
    return sp, mt


def adversarial_mesh(tris):
    """Mutates a TRIANGLE array (the same way for oracle and product) into a mesh made for the edges of the traversal argument:
    exact duplicates (two hits at bit-equal distances: the visit order decides, extend.wgsl:190-207), triangles that share an
    edge, and axis-aligned triangles whose boxes have no thickness."""
    n = len(tris)
    for k in range(0, min(200, n - 1), 2):
        tris["v0"][k + 1], tris["e1"][k + 1], tris["e2"][k + 1] = tris["v0"][k], tris["e1"][k], tris["e2"][k]
    for k in range(200, min(300, n - 1), 2):  # the second triangle completes the parallelogram: the diagonal is shared
        tris["v0"][k + 1] = tris["v0"][k] + tris["e1"][k] + tris["e2"][k]
        tris["e1"][k + 1], tris["e2"][k + 1] = -tris["e1"][k], -tris["e2"][k]
    for k in range(300, min(380, n)):
        ax = k % 3
        tris["e1"][k, ax] = 0.0
        tris["e2"][k, ax] = 0.0
    return tris


def adversarial_rays_mesh(W, tris, nodes, n_max):
    """Rays for a triangle mesh: at vertices, edge midpoints and centroids head-on and axis-parallel, in the planes of the boxes
    of flat triangles, along box edges of leaves and inner nodes, and a few ulp around each of them."""
    rays = []
    axes = np.eye(3, dtype=np.float32)

    def add(o, d):
        rays.append((np.asarray(o, np.float32), np.asarray(d, np.float32)))

    rng = np.random.default_rng(7)
    for k in range(min(len(tris), n_max // 40)):
        a = tris["v0"][k].astype(np.float32)
        b = (a + tris["e1"][k]).astype(np.float32)
        c = (a + tris["e2"][k]).astype(np.float32)
        nrm = np.cross(tris["e1"][k], tris["e2"][k]).astype(np.float32)
        ln = np.float32(np.linalg.norm(nrm))
        nrm = nrm / ln if ln > 0 else axes[k % 3]
        for p in (a, b, c, (a + b) * np.float32(0.5), (b + c) * np.float32(0.5), (a + b + c) / np.float32(3.0)):
            add(p + nrm * np.float32(4.0), -nrm)                       # head-on along the normal
            ax = int(np.argmax(np.abs(nrm)))
            o = p.copy()
            o[ax] += np.float32(5.0)
            add(o, -axes[ax])                                            # axis-parallel: two infinite inverses
        lo, hi = np.minimum(np.minimum(a, b), c), np.maximum(np.maximum(a, b), c)
        for ax in range(3):                                              # in the planes of the triangle's own box
            t_ax = (ax + 1) % 3
            for plane in (lo[ax], hi[ax]):
                o = (lo + hi) * np.float32(0.5)
                o[ax] = plane
                o[t_ax] = lo[t_ax] - np.float32(2.0)
                add(o, axes[t_ax])
                o2 = o.copy()
                o2[ax] = next_ulp(plane, int(rng.integers(-2, 3)))
                add(o2, axes[t_ax])
    for i, nd in enumerate(nodes[: n_max // 60]):
        if i == 1:
            continue
        lo, hi = nd["aabb_min"], nd["aabb_max"]
        c = (lo + hi) * np.float32(0.5)
        for ax in range(3):
            o = c.copy()
            o[ax] = hi[ax] + np.float32(3.0)
            add(o, -axes[ax])
            e = c.copy()
            e[ax] = hi[ax]
            e[(ax + 1) % 3] = lo[(ax + 1) % 3] - np.float32(2.0)
            add(e, axes[(ax + 1) % 3])
    rays = rays[:n_max]
    out = np.zeros(len(rays), W.RAY)
    for k, (o, d) in enumerate(rays):
        out["origin"][k, :3] = o
        out["origin"][k, 3] = 1.0
        out["direction"][k, :3] = d
    with np.errstate(all="ignore"):
        out["inv_direction"] = (np.float32(1.0) / out["direction"][:, :3]).astype("<f4")
    out["pixel_idx"] = np.arange(len(out), dtype="<u4") % 1024
    return out


def grazing_rays_mesh(W, tris, n_max, seed=11):
    """Rays for which Moeller-Trumbore is worst conditioned: within 1e-7 .. 1e-2 rad of a triangle's plane, passing
    an edge at -1e-3 .. +1e-3 (relative to the edge's length; negative = inside) as seen in the plane. The rounding slack of the
    primitive test grows like 1 / (cos(angle to the normal) * sin(angle between the edges)): such rays are where a hit could be reported
    for a ray that passes outside the triangle's box by more than the free walks' margin."""
    rng = np.random.default_rng(seed)
    rays = []
    per = max(n_max // 12, 1)
    for k in rng.permutation(len(tris))[:per]:
        a = tris["v0"][k].astype(np.float64)
        e1, e2 = tris["e1"][k].astype(np.float64), tris["e2"][k].astype(np.float64)
        nrm = np.cross(e1, e2)
        ln = np.linalg.norm(nrm)
        if ln == 0:
            continue
        nrm /= ln
        for (p0, ed) in ((a, e1), (a, e2), (a + e1, e2 - e1)):
            le = np.linalg.norm(ed)
            if le == 0:
                continue
            along = ed / le
            out = np.cross(along, nrm)                      # in the plane, perpendicular to the edge
            if np.dot(out, (a + (e1 + e2) / 3.0) - p0) > 0:  # make it point away from the triangle
                out = -out
            for _ in range(4):
                s = rng.uniform(0.05, 0.95)
                off = rng.choice([-1e-3, -1e-5, -1e-7, 0.0, 1e-7, 1e-5, 1e-3]) * le
                tilt = 10.0 ** rng.uniform(-7, -2) * rng.choice([-1.0, 1.0])
                phi = rng.uniform(0, 2 * np.pi)
                d_in_plane = np.cos(phi) * along + np.sin(phi) * out
                d = d_in_plane + tilt * nrm
                d /= np.linalg.norm(d)
                target = p0 + s * ed + off * out
                dist = rng.uniform(2.0, 40.0)
                rays.append(((target - d * dist).astype(np.float32), d.astype(np.float32)))
    rays = rays[:n_max]
    res = np.zeros(len(rays), W.RAY)
    for k, (o, d) in enumerate(rays):
        res["origin"][k, :3] = o
        res["origin"][k, 3] = 1.0
        res["direction"][k, :3] = d
    with np.errstate(all="ignore"):
        res["inv_direction"] = (np.float32(1.0) / res["direction"][:, :3]).astype("<f4")
    res["pixel_idx"] = np.arange(len(res), dtype="<u4") % 1024
    return res


# ---- shade, miss and the loops at the edges of scatter() (tests/test_shade_edges_host.py, tests/test_gpu_shade_edges.py)
def assert_bits_or_nan(a, b, what=""):
    """Bit equality of two float32 arrays, except that an element counts as equal where BOTH sides hold a NaN: x86 and gfx950 give a
    generated NaN different sign and payload bits. Only for inputs declared may-be-NaN; everything declared finite goes through
    conftest.assert_bit_equal after the oracle's side has been shown to hold no NaN."""
    a, b = np.ascontiguousarray(a, "<f4"), np.ascontiguousarray(b, "<f4")
    assert a.shape == b.shape, f"{what}: shape {a.shape} vs {b.shape}"
    bad = (a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))
    if bad.any():
        first = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {a.size} values differ; first at {first}: {a[first]!r} vs {b[first]!r}")


def ray_floats(r):
    """The twelve floats of RAY records as an (n, 11) float32 array (pixel_idx is compared apart)."""
    return np.concatenate([r["origin"], r["direction"], r["inv_direction"]], axis=1).astype("<f4")


# (name, material_type, albedo, fuzz, refract_index, may_be_nan): per type the values scatter() has branches or special arithmetic for
ZOO_MATERIALS = [
    ("lambert-black", 0, 0.0, 0.0, 0.0, False), ("lambert", 0, (0.7, 0.6, 0.5), 0.0, 0.0, False), ("lambert-2.0", 0, 2.0, 0.0, 0.0, False),
    ("metal-fuzz0", 1, (0.8, 0.7, 0.6), 0.0, 0.0, False), ("metal-fuzz0.5", 1, (0.8, 0.7, 0.6), 0.5, 0.0, False),
    ("metal-fuzz1", 1, (0.8, 0.7, 0.6), 1.0, 0.0, False), ("metal-fuzz4", 1, (0.8, 0.7, 0.6), 4.0, 0.0, False),
    ("glass-1.5", 2, 1.0, 0.0, 1.5, False), ("glass-1.0", 2, 1.0, 0.0, 1.0, False), ("glass-1/1.5", 2, 1.0, 0.0, 1.0 / 1.5, False),
    ("glass-1e-3", 2, 1.0, 0.0, 1e-3, False), ("glass-1e20", 2, 1.0, 0.0, 1e20, False),
    ("glass-0", 2, 1.0, 0.0, 0.0, True), ("glass-negative", 2, 1.0, 0.0, -1.5, True), ("glass-inf", 2, 1.0, 0.0, np.inf, True),
    ("glass-nan", 2, 1.0, 0.0, np.nan, True),
]
ZOO_NAMES = [m[0] for m in ZOO_MATERIALS]


def zoo_materials(orc, with_nan=True):
    mt = np.zeros(len(ZOO_MATERIALS), orc.MATERIAL)
    for k, (_, mtype, albedo, fuzz, ri, may_nan) in enumerate(ZOO_MATERIALS):
        mt["albedo"][k, :3] = albedo
        mt["albedo"][k, 3] = 1.0
        mt["fuzz"][k], mt["refract_index"][k], mt["material_type"][k] = fuzz, ri, mtype
        if may_nan and not with_nan:  # the finite zoo keeps the slot (same indices) but holds ordinary glass
            mt["refract_index"][k] = 1.5
    return mt


def material_zoo(orc, with_nan=True, degenerate_radii=False):
    """The material zoo as a sphere scene: every material of ZOO_MATERIALS on a sphere of radius 0.5 (a 4 x 4 grid at y = 0, 3 apart), one
    sphere of radius 1e-3 per material type behind the grid, and two of radius 1000 (the ground's size): a Lambertian floor whose top is
    at y = -3 and a glass ceiling whose bottom is at y = +3. Returns (spheres, materials) in creation order (the BVH build reorders a copy;
    zoo_index_of maps back)."""
    mt = zoo_materials(orc, with_nan)
    n = len(mt)
    sp = np.zeros(n + 5, orc.SPHERE)
    for k in range(n):
        sp["center"][k, :3] = (3.0 * (k % 4) - 4.5, 0.0, 3.0 * (k // 4) - 4.5)
        sp["radius"][k] = 0.5
        sp["material_idx"][k] = k
    for j, k in enumerate((1, 4, 7)):  # lambert, metal-fuzz0.5, glass-1.5
        sp["center"][n + j, :3] = (3.0 * j - 3.0, 0.0, 7.5)
        sp["radius"][n + j] = 1e-3
        sp["material_idx"][n + j] = k
    sp["center"][n + 3, :3], sp["radius"][n + 3], sp["material_idx"][n + 3] = (0.0, -1003.0, 0.0), 1000.0, 1
    sp["center"][n + 4, :3], sp["radius"][n + 4], sp["material_idx"][n + 4] = (0.0, 1003.0, 0.0), 1000.0, 7
    if degenerate_radii:  # the last two: Shirley's hollow glass (radius -0.4 inside the glass-1.5 sphere) and a Lambertian sphere of radius 0
        extra = np.zeros(2, orc.SPHERE)
        extra["center"][0, :3], extra["radius"][0], extra["material_idx"][0] = sp["center"][7, :3], -0.4, 7
        extra["center"][1, :3], extra["radius"][1], extra["material_idx"][1] = (0.0, 1.5, 1.5), 0.0, 1
        sp = np.concatenate([sp, extra])
    sp["center"][:, 3] = 1.0
    sp["material_type"] = mt["material_type"][sp["material_idx"]]
    return sp, mt


def zoo_index_of(built, created):
    """For each sphere of the BVH-ordered array `built` its index in `created` (centres are unique)."""
    key = {tuple(c): k for k, c in enumerate(created["center"][:, :3].tolist())}
    return np.array([key[tuple(c)] for c in built["center"][:, :3].tolist()], np.int64)


def shade_rng_key(idx, n_hits, width, rng_mode, pixel_idx, workgroup_size_64):
    """(px, py) that keys shade's RNG for hit `idx` of `n_hits` (sh:62-72): the dispatch's global_invocation_id in WFPT_RNG_DISPATCH, the
    ray's own pixel in WFPT_RNG_PIXEL."""
    if rng_mode == 1:
        return pixel_idx % width, pixel_idx // width
    gx, _ = workgroup_size_64(n_hits)
    wg, li = idx // 64, idx % 64
    return (wg % gx) * 8 + li % 8, (wg // gx) * 8 + li // 8


def _perp(u, rng):
    v = np.cross(u, rng.normal(size=3))
    return v / np.linalg.norm(v)


def _unit(rng):
    u = rng.normal(size=3)
    return u / np.linalg.norm(u)


def _tilted(u, angle, rng):
    return np.cos(angle) * u + np.sin(angle) * _perp(u, rng)


CRITICAL_COS = float(np.sqrt(1.0 - 1.0 / 2.25))  # inside glass of index 1.5: k = 1 - 2.25 (1 - cos^2) changes sign here
FALLBACK_TILTS = (0.0, 5e-4, 0.001 - 1e-6, 0.001 - 1e-7, 0.001 + 1e-7, 0.001 + 1e-6, 2e-3)
# geometry classes of shade_edge_rays: name -> may-be-NaN. The last two never hit (see shade_edge_rays) and sit at the end of the array.
EDGE_CLASSES = {"head_on": False, "grazing_outside": False, "grazing_inside": False, "critical": False, "len_1e-3": False, "len_1e3": False,
                "len_1e-20": False, "origin_inside": False, "origin_on_surface": False, "origin_1e4_away": False, "fallback": False,
                "len_1e18": False, "len_1e-30": True}


def shade_edge_rays(W, spheres, materials, w, h, frame, rng_mode, orc, per_class=160, seed=5):
    """One ray per pixel (unique pixel_idx = the ray's index, origin.w = 1, direction.w = 0), each built in float64 to hit a chosen sphere of
    material_zoo first, rounded to float32. `spheres` in creation order. Returns (rays, cls, target, maybe_nan): the class name, the
    intended sphere (creation index; -1 = built to miss) and the may-be-NaN flag of every ray.

      head_on            along the normal: dot(n, -uv) rounds to either side of 1, min(.., 1) clamps
      grazing_outside /  3e-3 .. 3e-2 rad off (1e-3 inside the big spheres) the tangent plane at the hit, arriving from outside (cos_theta >= 0) and from inside the same
      grazing_inside     sphere (cos_theta < 0). Ulp-sized tilts are out of a sphere's reach: the quadratic's discriminant b b - a c keeps
                         tilt^2 relative to b b, so a tilt below 2^-12 is rounded away and the ray hits or misses by chance; the mesh
                         (shade_edge_mesh, class grazing_ulp) carries those
      critical           from inside glass of index 1.5 at incidence stepping through the critical angle: k of refract() within 1e-6 of 0,
                         both signs (plus coarser steps)
      len_*              direction lengths 1e-3, 1e3, 1e-20 (a a is denormal) towards spheres of radius 0.5. Lengths 1e18 and 1e-30 cannot hit:
                         t = distance / length lies below the (0.001, ..) window for 1e18 unless the hit is 1e15 away, and for 1e-30
                         a = d.d underflows to 0 and t = -b / 0 is infinite. Both classes are built to MISS, are the last rays of the array
                         (so hit index == ray index for all others) and reach miss_kernel. An overflowing a = d.d (length >= 1.9e19) needs
                         a hit 1.9e16 away, where b b overflows first: normalize3's overflow side is reached by the second extend only
      origin_*           origin inside the sphere, on its surface heading inwards (the near root falls into the 0.001 window) and 1e4 away
                         from a sphere of radius 1000
      fallback           aimed at the Lambertian fall-back: for the ray's RNG key take rb from the oracle's probe and aim, along the normal,
                         at the surface point c - r rb' with rb' = rb tilted by FALLBACK_TILTS, so that length(nrm + rb) lands on both
                         sides of 0.001
    """
    rng = np.random.default_rng(seed)
    mat_of = spheres["material_idx"].astype(np.int64)
    nan_mat = np.array([m[5] for m in ZOO_MATERIALS])
    small = [k for k in range(len(spheres)) if spheres["radius"][k] == np.float32(0.5)]
    finite_small = [k for k in small if not nan_mat[mat_of[k]]]
    tiny = [k for k in range(len(spheres)) if spheres["radius"][k] < 0.01]
    big = [k for k in range(len(spheres)) if spheres["radius"][k] > 100.0]
    lambert = [k for k in small if materials["material_type"][mat_of[k]] == 0]
    glass15 = [k for k in small if ZOO_NAMES[mat_of[k]] == "glass-1.5"]
    out = []  # (class, target, origin, direction)

    def centre(k):
        return spheres["center"][k, :3].astype(np.float64), float(spheres["radius"][k])

    def normal_for(k):  # where on sphere k a ray may arrive: anywhere on the small ones, near the room's side on the two big ones
        c, r = centre(k)
        if r > 100.0:
            return _tilted(np.array([0.0, -np.sign(c[1]), 0.0]), rng.uniform(0, 0.004), rng)
        return _unit(rng)

    def gap(r):
        return min(1.5, 9.0 * r)

    for i in range(per_class):
        k = (small + tiny + big)[i % (len(small) + len(tiny) + len(big))]
        c, r = centre(k)
        n = normal_for(k)
        out.append(("head_on", k, c + n * (r + gap(r)), -n * rng.choice([1.0, 0.5, 2.0])))
    for i in range(per_class):
        k = (small + big)[i % (len(small) + len(big))]
        c, r = centre(k)
        n = normal_for(k)
        # the smallest angles each case resolves: from outside the origin's own rounding against the depth r (1 - cos(angle)) the ray dips
        # into the sphere (1e-3 rad misses now and then), from inside the chord 2 r sin(angle) against the 0.001 window
        ang = (3e-3, 1e-2, 3e-2)[i % 3]
        q = c + r * n
        d = np.cos(ang) * _perp(n, rng) - np.sin(ang) * n
        out.append(("grazing_outside", k, q - d * gap(r), d))
        ang = ((1e-3, 3e-3, 1e-2) if r > 100.0 else (1e-2, 2e-2, 3e-2))[i % 3]
        d = np.cos(ang) * _perp(n, rng) + np.sin(ang) * n          # from inside, leaving through q; half a chord back
        out.append(("grazing_inside", k, q - d * (r * np.sin(ang)), d))
    for i in range(2 * per_class):
        k = glass15[i % len(glass15)]
        c, r = centre(k)
        n = _unit(rng)
        step = rng.uniform(-6e-7, 6e-7) if i % 4 else (-1e-2, -1e-4, 1e-4, 1e-2)[(i // 4) % 4]
        ct = CRITICAL_COS + step
        d = ct * n + np.sqrt(1.0 - ct * ct) * _perp(n, rng)
        out.append(("critical", k, c + r * n - d * (r * ct), d))
    for name, scale in (("len_1e-3", 1e-3), ("len_1e3", 1e3), ("len_1e-20", 1e-20)):
        for i in range(per_class):
            k = small[i % len(small)]
            c, r = centre(k)
            n = _unit(rng)
            d = -_tilted(n, rng.uniform(0.0, 0.2), rng)
            out.append((name, k, c + n * (r + 1.5), d * scale))
    for i in range(per_class):
        k = (small + big)[i % (len(small) + len(big))]
        c, r = centre(k)
        out.append(("origin_inside", k, c + _unit(rng) * (0.3 * r), _unit(rng)))
        n = normal_for(k)
        out.append(("origin_on_surface", k, c + r * n, -_tilted(n, rng.uniform(0.0, 0.5), rng)))
        kb = big[i % len(big)]
        cb, rb_ = centre(kb)
        nb = _tilted(np.array([0.0, np.sign(cb[1]), 0.0]), rng.uniform(0, 0.004), rng)  # from outside the room, through the far side
        out.append(("origin_1e4_away", kb, cb + nb * 1e4, -nb))
    n_fb = per_class * 2
    base = len(out)
    n_hit = base + n_fb
    for i in range(n_fb):
        k = lambert[i % len(lambert)]
        c, r = centre(k)
        idx = base + i
        px, py = shade_rng_key(idx, n_hit, w, rng_mode, idx, orc.workgroup_size_64)
        rb = orc.probe_shade_rb(int(px), int(py), w, frame, 0).astype(np.float64)
        rb /= np.linalg.norm(rb)
        aim = _tilted(rb, FALLBACK_TILTS[i % len(FALLBACK_TILTS)], rng)
        out.append(("fallback", k, c - aim * (r + 1.5), aim))
    for name, scale in (("len_1e18", 1e18), ("len_1e-30", 1e-30)):
        for i in range(per_class // 2):
            k = small[i % len(small)]
            c, r = centre(k)
            n = _unit(rng)
            out.append((name, -1, c + n * (r + 1.5), -n * scale))
    assert len(out) <= w * h
    rays = np.zeros(len(out), W.RAY)
    for i, (_, _, o, d) in enumerate(out):
        rays["origin"][i, :3] = o
        rays["direction"][i, :3] = d
    rays["origin"][:, 3] = 1.0
    with np.errstate(all="ignore"):
        rays["inv_direction"] = (np.float32(1.0) / rays["direction"][:, :3]).astype("<f4")
    rays["pixel_idx"] = np.arange(len(out), dtype="<u4")
    cls = np.array([c for c, _, _, _ in out])
    target = np.array([t for _, t, _, _ in out], np.int64)
    maybe_nan = np.array([EDGE_CLASSES[c] for c in cls]) | np.where(target >= 0, nan_mat[mat_of[np.maximum(target, 0)]], False)
    return rays, cls, target, maybe_nan


def scatter_terms(rays, hits, spheres, materials, triangles=None):
    """What scatter() sees for each hit of a sphere scene (or of a mesh: triangles=, the normal is normalize(cross(e1, e2))), recomputed in float32 from the ORACLE's queues in the kernels' operation order:
    nrm, uv, the dielectric branch's cos_theta (before the clamp and the flip) and refract()'s k (NaN for other materials)."""
    from environment_ref import normalize3
    f = np.float32
    r = rays[hits["ray_idx"].astype(np.int64)]
    t = hits["t"].astype(f)
    s = (spheres if triangles is None else triangles)[hits["sphere_idx"].astype(np.int64)]
    if triangles is None:
        p = [r["origin"][:, a] + t * r["direction"][:, a] for a in range(3)]
        nrm = normalize3(*[p[a] - s["center"][:, a] for a in range(3)])
    else:
        a_, b_ = s["e1"], s["e2"]
        nrm = normalize3(a_[:, 1] * b_[:, 2] - a_[:, 2] * b_[:, 1], a_[:, 2] * b_[:, 0] - a_[:, 0] * b_[:, 2], a_[:, 0] * b_[:, 1] - a_[:, 1] * b_[:, 0])
    with np.errstate(all="ignore"):
        uv = normalize3(*[r["direction"][:, a] for a in range(3)])
        cos_theta = (nrm[0] * -uv[0] + nrm[1] * -uv[1]) + nrm[2] * -uv[2]
        ri = materials["refract_index"][s["material_idx"].astype(np.int64)].astype(f)
        front = np.fmin(cos_theta, f(1)) >= 0
        eta = np.where(front, f(1) / ri, ri).astype(f)
        sgn = np.where(front, f(1), f(-1))
        ct = (uv[0] * (nrm[0] * sgn) + uv[1] * (nrm[1] * sgn)) + uv[2] * (nrm[2] * sgn)
        k = f(1) - eta * eta * (f(1) - ct * ct)
    k = np.where(hits["mat_type"] == 2, k, f(np.nan)).astype(f)
    return np.stack(nrm, 1).astype(f), np.stack(uv, 1).astype(f), cos_theta.astype(f), k


def closed_room_inputs(orc, scene, w, h):
    """Scenes without a single miss: the camera inside a closed sphere of radius 5 that holds a small Lambertian one. closed-metal: fuzz 0;
    closed-glass: index 1.5 (total internal reflection or refraction into a second, enclosing metal sphere); centre: the camera exactly at
    the metal sphere's centre (every primary ray meets it head-on)."""
    sp = np.zeros(3, orc.SPHERE)
    mt = np.zeros(3, orc.MATERIAL)
    mt["albedo"][:] = (0.9, 0.8, 0.7, 1.0)
    mt["material_type"] = (1, 0, 2)
    mt["refract_index"][2] = 1.5
    sp["center"][:, 3] = 1.0
    sp["radius"] = (9.0, 0.5, 5.0) if scene == "closed-glass" else (5.0, 0.5, 0.25)
    sp["center"][1, :3] = (1.5, 0.0, -2.0)
    sp["center"][2, :3] = (0.0, 0.0, 0.0) if scene == "closed-glass" else (-1.5, 0.5, -2.0)
    sp["material_idx"] = (0, 1, 2)
    sp["material_type"] = mt["material_type"]
    sp, nodes = orc.build_bvh(sp)
    pos = (0.0, 0.0, 0.0) if scene == "centre" else (0.5, 0.25, 1.0)
    cam, ip, vw = orc.camera(pos, (0.5, 0.0, -1.0), 70.0, 0.0, 10.0, 0.1, 100.0, w, h)
    return sp, mt, nodes, cam, ip, vw


# ---- the same on a mesh: one small triangle per ray
MESH_CLASSES = {"head_on": False, "grazing_ulp": False, "critical": False, "len_1e-3": False, "len_1e3": False, "len_1e-20": False, "fallback": False}
GRAZING_ULPS = (1, 4, 64)


def _triangle(q, n, t1, size=0.6):
    """(v0, e1, e2) of a triangle with centroid q and cross(e1, e2) along n (t1 a unit tangent)."""
    t2 = np.cross(n, t1)
    e1, e2 = size * t1, size * t2
    return q - (e1 + e2) / 3.0, e1, e2


def shade_edge_mesh(W, orc, w, h, frame, rng_mode, per_class=60, with_nan=True, seed=9):
    """The mesh variant of shade_edge_rays: ray i is built to hit triangle i (edges chosen in float64, rounded to float32; centroids on a
    9 x 9 x 9 grid 2.5 apart, rays start 1.2 away, so no ray reaches another cell's triangle first), materials cycling through the zoo.
    Every ray hits, so hit index == ray index. Returns (triangles in creation order, materials, rays, cls, maybe_nan).

      head_on      against the stored normal from the front and from the back (the normal is never flipped)
      grazing_ulp  glass triangles lying exactly in the plane y = 0 (normal +y): the ray's direction is (cos phi, -s k 2^-23, sin phi) and its
                   origin 4 direction lengths back, at height 4 s k 2^-23 (exact in float32), for k = 1, 4, 64 and s = +-1 (from above: outside,
                   from below: inside): dot(n, -uv) = s k ulp-sized tilts of 0. A tilt of exactly 0 lies in the plane and cannot hit
      critical     from the back of glass of index 1.5 (eta = 1.5), incidence stepping through the critical angle
      len_*        direction lengths 1e-3, 1e3, 1e-20
      fallback     Lambertian triangles whose normal is -rb', rb' = the probe's rb for the ray's RNG key tilted by FALLBACK_TILTS, hit head-on
    """
    rng = np.random.default_rng(seed)
    mt = zoo_materials(orc, with_nan)
    nan_mat = np.array([m[5] for m in ZOO_MATERIALS])
    lambert = [k for k, m in enumerate(ZOO_MATERIALS) if m[1] == 0]
    glass = [k for k, m in enumerate(ZOO_MATERIALS) if m[1] == 2 and not m[5]]
    g15 = ZOO_NAMES.index("glass-1.5")
    plan = ([("grazing_ulp", i) for i in range(72)] + [("head_on", i) for i in range(per_class)] + [("critical", i) for i in range(2 * per_class)] +
            [(c, i) for c in ("len_1e-3", "len_1e3", "len_1e-20") for i in range(per_class)] + [("fallback", i) for i in range(2 * per_class + 20)])
    n = len(plan)
    assert n <= 729 and n <= w * h
    tris = np.zeros(n, orc.TRIANGLE)
    rays = np.zeros(n, W.RAY)
    mats = np.zeros(n, np.int64)
    for idx, (c, i) in enumerate(plan):
        # grazing triangles take the grid's middle layer (y = 0 exactly), the others the remaining cells in order
        cell = 4 * 81 + idx if c == "grazing_ulp" else (idx - 72 if idx - 72 < 4 * 81 else idx + 9)
        q = 2.5 * (np.array([cell % 9, cell // 81, (cell // 9) % 9], np.float64) - 4.0)
        if c == "grazing_ulp":
            nrm, t1 = np.array([0.0, 1.0, 0.0]), np.array([1.0, 0.0, 0.0])
            k, s_ = GRAZING_ULPS[i % 3], (1.0 if (i // 3) % 2 == 0 else -1.0)
            phi = rng.uniform(0, 2 * np.pi)
            d = np.array([np.cos(phi), -s_ * k * 2.0 ** -23, np.sin(phi)])
            o = q - 4.0 * d
            o[1] = 4.0 * s_ * k * 2.0 ** -23
            m = glass[i % len(glass)] if i % 4 else g15
        elif c == "fallback":
            px, py = shade_rng_key(idx, n, w, rng_mode, idx, orc.workgroup_size_64)
            rb = orc.probe_shade_rb(int(px), int(py), w, frame, 0).astype(np.float64)
            rb /= np.linalg.norm(rb)
            d = _tilted(rb, FALLBACK_TILTS[i % len(FALLBACK_TILTS)], rng)
            nrm, t1 = -d, _perp(d, rng)
            o = q - 1.2 * d
            m = lambert[i % len(lambert)]
        else:
            nrm = _unit(rng)
            t1 = _perp(nrm, rng)
            m = idx % len(ZOO_MATERIALS)
            if c == "head_on":
                d = -nrm if i % 2 == 0 else nrm
            elif c == "critical":
                m = g15
                step = rng.uniform(-2.5e-7, 2.5e-7) if i % 4 else (-1e-2, -1e-4, 1e-4, 1e-2)[(i // 4) % 4]
                ct = CRITICAL_COS + step
                d = ct * nrm + np.sqrt(1.0 - ct * ct) * t1
            else:
                d = -_tilted(nrm, rng.uniform(0.0, 0.3), rng)
            o = q - 1.2 * d
            d = d * {"len_1e-3": 1e-3, "len_1e3": 1e3, "len_1e-20": 1e-20}.get(c, 1.0)
        v0, e1, e2 = _triangle(q, nrm, t1)
        tris["v0"][idx], tris["e1"][idx], tris["e2"][idx] = v0, e1, e2
        rays["origin"][idx, :3], rays["direction"][idx, :3] = o, d
        mats[idx] = m
    tris["material_idx"] = mats
    tris["material_type"] = mt["material_type"][mats]
    rays["origin"][:, 3] = 1.0
    with np.errstate(all="ignore"):
        rays["inv_direction"] = (np.float32(1.0) / rays["direction"][:, :3]).astype("<f4")
    rays["pixel_idx"] = np.arange(n, dtype="<u4")
    cls = np.array([c for c, _ in plan])
    return tris, mt, rays, cls, nan_mat[mats] & with_nan


def mesh_index_of(built, created):
    """For each triangle of the BVH-ordered array `built` its index in `created` (v0 is unique)."""
    key = {tuple(c): k for k, c in enumerate(created["v0"].tolist())}
    return np.array([key[tuple(c)] for c in built["v0"].tolist()], np.int64)


def fallback_wall(orc, w, h, pixel, frame):
    """A scene whose pixel `pixel` takes the Lambertian fall-back at its first hit of frame `frame` in WFPT_RNG_PIXEL: a pair of triangles
    (one Lambertian quad, 40 x 40) 3 in front of a camera at the origin that looks along rb = the probe's first draw for (pixel, frame), with
    normal -rb. The wall fills the view and its normal is the same everywhere, so wherever the pixel's jittered primary ray lands,
    nrm + rb rounds to (almost) nothing. Returns (triangles, materials, camera position, look_at)."""
    rb = orc.probe_shade_rb(pixel % w, pixel // w, w, frame, 0).astype(np.float64)
    rb /= np.linalg.norm(rb)
    t1 = np.cross(rb, [0.0, 1.0, 0.0])
    t1 /= np.linalg.norm(t1)
    t2 = np.cross(-rb, t1)
    c = 3.0 * rb
    tris = np.zeros(2, orc.TRIANGLE)
    a = c - 20.0 * t1 - 20.0 * t2
    tris["v0"][0], tris["e1"][0], tris["e2"][0] = a, 40.0 * t1, 40.0 * t2              # cross(t1, t2) = -rb
    tris["v0"][1], tris["e1"][1], tris["e2"][1] = a + 40.0 * t1 + 40.0 * t2, -40.0 * t1, -40.0 * t2
    mt = np.zeros(1, orc.MATERIAL)
    mt["albedo"][0] = (0.8, 0.6, 0.4, 1.0)
    return tris, mt, (0.0, 0.0, 0.0), tuple(rb)


def degenerate_radius_rays(W, spheres, n=256, seed=4):
    """Rays for the last two spheres of material_zoo(degenerate_radii=True): the first three quarters start inside the glass sphere at distance
    0.45 from its centre and head for the centre (they meet the sphere of radius -0.4 after 0.05), the last quarter heads for the sphere of
    radius 0 from 2 away: a hit there is AT the centre, where normalize(p - centre) is 0 * inf, so that quarter is the may-be-NaN class."""
    rng = np.random.default_rng(seed)
    rays = np.zeros(n, W.RAY)
    for i in range(n):
        u = _unit(rng)
        c = spheres["center"][-2 if i < 3 * n // 4 else -1, :3].astype(np.float64)
        rays["origin"][i, :3] = c + u * (0.45 if i < 3 * n // 4 else 2.0)
        rays["direction"][i, :3] = -u
    rays["origin"][:, 3] = 1.0
    with np.errstate(all="ignore"):
        rays["inv_direction"] = (np.float32(1.0) / rays["direction"][:, :3]).astype("<f4")
    rays["pixel_idx"] = np.arange(n, dtype="<u4")
    return rays


def assert_second_trips(W, pt, batch_with, batch_without):
    """The premise of the second-trip tests, from the library's own numbers: `pt`'s segment count (its ray capacity over the segment size
    wfpt_build_info reports) is above the workgroups a segment-walking pass launches per sample at `batch_with`, so some workgroup walks
    a second segment, and within those at `batch_without`, so none does. The grid is consumer_grid's rule (csrc/wfpt_api.hip):
    min(segments, max(64, ceil(8 CUs / batch)))."""
    info = dict(kv.split("=") for kv in W.lib().wfpt_build_info().decode().split(";"))
    segments = pt.ray_capacity // int(info["chunk"])
    cus = W.device_info(0)["compute_units"]
    grid = {b: min(segments, max(64, -(-cus * 8 // b))) for b in (batch_with, batch_without)}
    assert segments > 64 and grid[batch_with] < segments == grid[batch_without], \
        f"{segments} segments, {grid} workgroups per sample: the premise of this test is gone"
