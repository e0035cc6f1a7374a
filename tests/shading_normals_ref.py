"""numpy float32 restatement of per-vertex shading normals (WFPT_FLAG_SHADING_NORMALS, include/wfpt.h "Shading normals"): the host's
normalisation of the table, steps 1-5 at a hit, shade.wgsl's scatter() about the shading normal, and a whole render driven through the
oracle's stages. The oracle scatters about the stored normal, so `Shaded` wraps it in the style of retire_ref.Retiring and
adaptive_ref.Masked: it notes the hits before shade() and, after the queue swap, rewrites the extension rays' directions (the origin and
the slot stay the oracle's) with scatter() restated about the shading normal. For the compositions with the connect pass,
`shading_receivers` substitutes transport_ref.hit_normal for the duration of a render. Every step is one IEEE f32 operation in the
header's order (pow, min and the first draw rb are the oracle's own statements of the library's), so the results are the device's bits."""
import contextlib
import ctypes as C

import numpy as np

import transport_ref
from nee_ref import jenkins_hash, rng_next_float
from transport_ref import BounceTables, dot3, f32, normalize3, triangle_normal_area

u32 = np.uint32


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# ---------------------------------------------------------------- the table as stored
def normalize_rows(n9):
    """wfpt_normalize_triangle_normals: each corner normal times 1 / sqrt(l2), l2 = (x x + y y) + z z; +0 where l2 is not a finite number
    above 0. n9 (n, 9) -> (n, 9)."""
    v = np.asarray(n9, f32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        l2 = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
        inv = f32(1) / np.sqrt(l2)
        out = v * inv[:, None]
    ok = (l2 > 0) & (l2 <= np.finfo(f32).max)
    return np.where(ok[:, None], out, f32(0)).astype(f32).reshape(-1, 9)


# ---------------------------------------------------------------- steps 1-5
def barycentrics(p, v0, e1, e2):
    """b0, b1, b2 of points p (k, 3) on the triangles (v0, e1, e2), as wfpt_device_math.h's triangle_uv forms them."""
    p, v0, e1, e2 = (np.asarray(a, f32) for a in (p, v0, e1, e2))
    w = p - v0
    with np.errstate(all="ignore"):
        d00, d01, d11, d20, d21 = dot3(e1, e1), dot3(e1, e2), dot3(e2, e2), dot3(w, e1), dot3(w, e2)
        den = d00 * d11 - d01 * d01
        ok = den > 0
        inv = f32(1) / np.where(ok, den, f32(1))
        b1 = np.where(ok, (d11 * d20 - d01 * d21) * inv, f32(0)).astype(f32)
        b2 = np.where(ok, (d00 * d21 - d01 * d20) * inv, f32(0)).astype(f32)
        b0 = (f32(1) - b1) - b2
    return b0.astype(f32), b1, b2


def shading_normal(triangles, rows, prim, p, keep_unnormalised=False, swap_b=False):
    """The shading normal of hits at p (k, 3) on triangles prim (k,) of `triangles` (the device's order, rows named by _pad) with the stored
    table rows (n, 9): (ns (k, 3), fell back (k,)). keep_unnormalised / swap_b: two mutations of tests/test_shading_normals_host.py (m used
    as it is; b1 and b2 exchanged)."""
    prim = np.asarray(prim, np.int64)
    p = np.asarray(p, f32).reshape(-1, 3)
    t = triangles[prim]
    ng = triangle_normal_area(t)[0]
    r = np.asarray(rows, f32).reshape(-1, 9)[t["_pad"].astype(np.int64)]
    n0, n1, n2 = r[:, 0:3], r[:, 3:6], r[:, 6:9]
    b0, b1, b2 = barycentrics(p, t["v0"], t["e1"], t["e2"])
    if swap_b:
        b1, b2 = b2, b1
    with np.errstate(all="ignore"):
        m = (n0 * b0[:, None] + n1 * b1[:, None]) + n2 * b2[:, None]
        l2 = dot3(m, m)
        ns = m * (f32(1) / np.sqrt(l2))[:, None]
        if keep_unnormalised:
            ns = m
        keep = (l2 > 0) & (l2 < np.inf) & (dot3(ns, ng) > 0)
    return np.where(keep[:, None], ns, ng).astype(f32), ~keep


class Normals:
    """What a context with a table holds: the triangles as the device holds them and the table as stored (normalised at the call)."""

    def __init__(self, triangles, n9, **mutations):
        self.triangles = triangles
        self.rows = normalize_rows(n9)
        self.mutations = mutations

    def at(self, prim, p):
        return shading_normal(self.triangles, self.rows, prim, p, **self.mutations)

    def sample_rows(self, p, prim):
        """wfpt_sample_shading_normal's rows for points p (k, 3) on triangles prim (k,): (ns.xyz | 1.0 where step 5 fell back)."""
        ns, fell = self.at(prim, p)
        return np.concatenate([ns, fell.astype(f32)[:, None]], 1).astype(f32)


def probe_rows(p, prim):
    """The rows wfpt_sample_shading_normal takes: (p.xyz | the triangle's index as the bits of the fourth float)."""
    rows = np.zeros((len(prim), 4), f32)
    rows[:, :3] = p
    rows[:, 3] = np.asarray(prim, u32).view(f32)
    return rows


# ---------------------------------------------------------------- scatter() about a given normal (shade.wgsl:93-151)
def _pow(x, y):
    from oracle import oracle as O
    x = np.ascontiguousarray(x, "<f4")
    y = np.ascontiguousarray(np.broadcast_to(f32(y), x.shape), "<f4")
    out = np.zeros_like(x)
    O.lib().orc_probe_pow(_p(x), _p(y), _p(out), x.size)
    return out


def _reflect(r, n):
    k = f32(2) * dot3(r, n)
    return r - k[:, None] * n


def scatter(nrm, rdir, mat_type, fuzz, refract_index, rb, u):
    """The extension direction of hits with normal nrm (k, 3) and incoming direction rdir (k, 3): metal reflect(rdir, nrm) + fuzz rb,
    dielectric reflect / refract by Schlick's reflectance against the draw u, everything else nrm + rb (nrm where that is shorter than
    0.001). rb (k, 3): shade's first draw, normalised (the oracle's probe); u (k,): the first draw of the same state as a float."""
    from oracle import oracle as O
    nrm, rdir, rb = (np.asarray(a, f32) for a in (nrm, rdir, rb))
    mat_type = np.asarray(mat_type, np.int64)
    fuzz, ri, u = np.asarray(fuzz, f32), np.asarray(refract_index, f32), np.asarray(u, f32)
    with np.errstate(all="ignore"):
        lam = nrm + rb
        lam = np.where((np.sqrt(dot3(lam, lam)) < f32(0.001))[:, None], nrm, lam)
        metal = _reflect(rdir, nrm) + fuzz[:, None] * rb
        uv = np.stack(normalize3(rdir[:, 0], rdir[:, 1], rdir[:, 2]), 1).astype(f32)
        cos_theta = O.probe_minmax(dot3(nrm, -uv), np.ones(len(nrm), f32))[0]
        front = cos_theta >= 0
        eta = np.where(front, f32(1) / ri, ri).astype(f32)
        norm = np.where(front[:, None], nrm, nrm * f32(-1)).astype(f32)
        cos_theta = np.where(front, cos_theta, cos_theta * f32(-1)).astype(f32)
        r0 = (f32(1) - eta) / (f32(1) + eta)
        r0 = r0 * r0
        reflectance = r0 + (f32(1) - r0) * _pow(f32(1) - cos_theta, 5.0)
        ct = dot3(uv, norm)
        k = f32(1) - eta * eta * (f32(1) - ct * ct)
        m = eta * ct + np.sqrt(k)
        refr = eta[:, None] * uv - m[:, None] * norm
        glass = np.where(((k >= 0) & ~(reflectance > u))[:, None], refr, _reflect(uv, norm))
    out = np.where((mat_type == 1)[:, None], metal, np.where((mat_type == 2)[:, None], glass, lam))
    return out.astype(f32)


def first_draw(px, py, width, frame):
    """rng_next_float of shade's state for the hit keyed by (px, py): init_rng, then one draw (sample_number = 0: no skip-ahead)."""
    s = jenkins_hash((np.asarray(px, u32) + np.asarray(py, u32) * u32(width)) ^ jenkins_hash(u32(frame)))
    return rng_next_float(s)[0]


# ---------------------------------------------------------------- the render
class Shaded(BounceTables):
    """An Oracle (or a wrapper around one) over a triangle scene whose shade scatters about the shading normal. normals: a Normals;
    materials: the scene's. keep_geometric: the mutation that leaves the oracle's own extension rays (the stored normal kept in scatter).
    Goes inside adaptive_ref.Local (the RNG key is the image's pixel), around or inside Masked / Retiring."""

    def __init__(self, o, normals, materials, keep_geometric=False):
        super().__init__(o)
        self.normals, self.materials = normals, materials
        self.keep_geometric = keep_geometric
        self.frame = 0
        self._noted = None

    def set_frame(self, frame, sample_number=0):
        assert sample_number == 0
        self.frame = frame
        self.o.set_frame(frame, sample_number)

    def shade(self, gx, gy):
        n_hit = min(int(self.o.counters()[1]), gx * gy * 64)
        hits = self.o.hits(n_hit)
        rays = self.o.rays()[hits["ray_idx"].astype(np.int64)]
        self._noted = (hits, rays)
        super().shade(gx, gy)

    def swap_ray_queues(self):
        from helpers import shade_rng_key
        from oracle import oracle as O
        self.o.swap_ray_queues()
        if self._noted is None or self.keep_geometric:
            return
        (hits, rays), self._noted = self._noted, None
        n = len(hits)
        if n == 0:
            return
        P, W_ = self.o.params, self.o.width
        prim = hits["sphere_idx"].astype(np.int64)
        org, d = rays["origin"][:, :3].astype(f32), rays["direction"][:, :3].astype(f32)
        pt = org + hits["t"].astype(f32)[:, None] * d  # sh:91
        ns, _ = self.normals.at(prim, pt)
        t = self.normals.triangles[prim]
        mat = self.materials[t["material_idx"].astype(np.int64)]
        pix = rays["pixel_idx"].astype(np.int64)
        key = [shade_rng_key(i, n, W_, P.rng_mode, int(pix[i]), O.workgroup_size_64) for i in range(n)]
        px, py = np.array([k[0] for k in key], np.int64), np.array([k[1] for k in key], np.int64)
        rb = np.stack([O.probe_shade_rb(int(x), int(y), W_, self.frame, 0) for x, y in zip(px, py)]).astype(f32)
        ext_dir = scatter(ns, d, hits["mat_type"], mat["fuzz"], mat["refract_index"], rb, first_draw(px, py, W_, self.frame))
        ext = self.o.rays(n)
        assert np.array_equal(ext["pixel_idx"], rays["pixel_idx"]), "extension ray h is not hit h's"
        ext["direction"][:, :3] = ext_dir
        with np.errstate(all="ignore"):
            ext["inv_direction"] = f32(1) / ext_dir
        self.o.write_rays(ext)


@contextlib.contextmanager
def shading_receivers(normals):
    """For the duration of a render, transport_ref.hit_normal -- the receiver normal of the connect pass -- is the shading normal."""
    keep = transport_ref.hit_normal

    def hit_normal(scene, prim, p):
        return normals.at(np.asarray(prim, np.int64), p)[0]

    transport_ref.hit_normal = hit_normal
    try:
        yield
    finally:
        transport_ref.hit_normal = keep


# ---------------------------------------------------------------- the scene of the tests
def icosphere(subdivisions=2, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """(corner positions (n, 3, 3) float64 of an icosphere's faces wound outward, inscribed in the sphere): 20 * 4^subdivisions faces."""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    v = np.array([(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1),
                  (-g, 0, -1), (-g, 0, 1)], np.float64)
    v /= np.linalg.norm(v, axis=1)[:, None]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4),
         (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    tri = v[np.array(f)]
    for _ in range(subdivisions):
        a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
        ab, bc, ca = ((x + y) / np.linalg.norm(x + y, axis=1)[:, None] for x, y in ((a, b), (b, c), (c, a)))
        tri = np.concatenate([np.stack(q, 1) for q in ((a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca))])
    return tri * radius + np.asarray(centre, np.float64)


def sphere_scene(orc, subdivisions=2, emitter=False):
    """The 20 * 4^subdivisions-triangle icosphere of radius 1 about the origin over a two-triangle ground at y = -1.25, materials by thirds
    of the sphere's faces: Lambertian (0), fuzzy metal (1), glass (2); the ground is Lambertian (3). emitter: a two-triangle lamp
    (material 4, Lambertian; the caller gives it its colour) above the sphere, facing down. Corner normals: the sphere's are its corner
    positions, the ground's and the lamp's are zero rows (flat). Returns (triangles in creation order with _pad = the row, materials,
    n9)."""
    tri = icosphere(subdivisions)
    n_s = len(tri)
    quads = [np.array([(-6.0, -1.25, -6.0), (-6.0, -1.25, 6.0), (6.0, -1.25, 6.0), (6.0, -1.25, -6.0)])]
    if emitter:
        quads.append(np.array([(-1.0, 2.5, -1.0), (1.0, 2.5, -1.0), (1.0, 2.5, 1.0), (-1.0, 2.5, 1.0)]))
    n = n_s + 2 * len(quads)
    t = np.zeros(n, orc.TRIANGLE)
    t["v0"][:n_s], t["e1"][:n_s], t["e2"][:n_s] = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    t["material_idx"][:n_s] = (np.arange(n_s) * 3) // n_s
    for k, q in enumerate(quads):
        for j, (a, b, c) in enumerate(((0, 1, 2), (0, 2, 3))):
            i = n_s + 2 * k + j
            t["v0"][i], t["e1"][i], t["e2"][i] = q[a], q[b] - q[a], q[c] - q[a]
            t["material_idx"][i] = 3 + k
    mt = np.zeros(5, orc.MATERIAL)
    mt["albedo"][:] = (0.5, 0.5, 0.5, 1.0)
    mt["albedo"][0, :3] = (0.75, 0.5, 0.25)
    mt["albedo"][1, :3] = (0.75, 0.75, 0.5)
    mt["albedo"][2, :3] = (1.0, 1.0, 1.0)
    mt["albedo"][3, :3] = (0.5, 0.75, 0.5)
    mt["material_type"] = (0, 1, 2, 0, 0)
    mt["fuzz"][1] = 0.25
    mt["refract_index"][2] = 1.5
    t["material_type"] = mt["material_type"][t["material_idx"]]
    t["_pad"] = np.arange(n, dtype=np.uint32)[::-1]  # row n - 1 - i belongs to triangle i: the rows are not the creation order
    n9 = np.zeros((n, 9), f32)
    n9[n - 1 - np.arange(n_s)] = (tri * 1.5).reshape(n_s, 9)  # (not unit length: the call normalises)
    return t, mt, n9


def sphere_camera(orc, w, h):
    return orc.camera((0.0, 1.0, 4.5), (0.0, -0.1, 0.0), 40.0, 0.0, 10.0, 0.1, 100.0, w, h)
