"""numpy float32 restatement of tangent-space normal maps (WFPT_FLAG_NORMAL_MAPS, include/wfpt.h "Normal maps"): steps A-F at a hit, and a
`Mapped` object with the `.at(prim, p)` interface of shading_normals_ref.Normals, so that S.Shaded, S.shading_receivers, microfacet_ref and
rough_dielectric_ref drive whole renders through the oracle with the mapped normal in the shading normal's place. Every step is one IEEE f32
operation in the header's order, so the results are the device's bits. The scene of the tests is here too: shading_normals_ref's icosphere
over a ground, with spherical corner UVs on the sphere, planar and mirrored UVs on the ground, and a small seeded map."""
import numpy as np

import shading_normals_ref as S
import texture_ref as T
from transport_ref import dot3, f32, triangle_normal_area

u32 = np.uint32
MUTATIONS = ("no_gram_schmidt", "ignore_sg", "swap_xy", "skip_f_test")


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1).astype(f32)


def mapped_normal(ng, ns, e1, e2, uv6, c, s, no_gram_schmidt=False, ignore_sg=False, swap_xy=False, skip_f_test=False):
    """Steps B-F for k hits: stored normals ng, shading normals ns, edges e1, e2 (k, 3 each), UV rows uv6 (k, 6), texels c (k, 3),
    strengths s (k,). Returns (n (k, 3), code (k,)): 0 mapped, 1 identity by step B, 2 no tangent frame, 3 rejected by step F. The
    keywords are the mutations of tests/test_normal_map_host.py."""
    ng, ns, e1, e2, uv6, c = (np.asarray(a, f32).reshape(-1, w) for a, w in ((ng, 3), (ns, 3), (e1, 3), (e2, 3), (uv6, 6), (c, 3)))
    s = np.broadcast_to(np.asarray(s, f32), (len(ng),)).astype(f32)
    one, two = f32(1), f32(2)
    with np.errstate(all="ignore"):
        # B.
        x = (two * c[:, 0] - one) * s
        y = (two * c[:, 1] - one) * s
        z = two * c[:, 2] - one
        if swap_xy:
            x, y = y, x
        identity = (x == 0) & (y == 0)
        # C.
        du1, dv1 = uv6[:, 2] - uv6[:, 0], uv6[:, 3] - uv6[:, 1]
        du2, dv2 = uv6[:, 4] - uv6[:, 0], uv6[:, 5] - uv6[:, 1]
        det = du1 * dv2 - du2 * dv1
        no_det = ~(det > 0) & ~(det < 0)
        sg = np.where(det > 0, one, -one).astype(f32)
        if ignore_sg:
            sg = np.ones_like(sg)
        Tn = ((e1 * dv2[:, None] - e2 * dv1[:, None]) * sg[:, None]).astype(f32)
        Bt = ((e2 * du1[:, None] - e1 * du2[:, None]) * sg[:, None]).astype(f32)
        # D.
        k = dot3(ns, Tn)
        tt = (Tn - ns * k[:, None]).astype(f32)
        if no_gram_schmidt:
            tt = Tn
        l2 = dot3(tt, tt)
        no_len = ~(l2 > 0) | ~(l2 < np.inf)
        t = (tt * (one / np.sqrt(l2))[:, None]).astype(f32)
        # E.
        bt = _cross(ns, t)
        bt = np.where((dot3(bt, Bt) < 0)[:, None], -bt, bt).astype(f32)
        # F.
        m = ((t * x[:, None] + bt * y[:, None]) + ns * z[:, None]).astype(f32)
        l2m = dot3(m, m)
        nm = (m * (one / np.sqrt(l2m))[:, None]).astype(f32)
        ok = (l2m > 0) & (l2m < np.inf)
        if not skip_f_test:
            ok = ok & (dot3(nm, ng) > 0)
    code = np.where(identity, 1, np.where(no_det | no_len, 2, np.where(ok, 0, 3))).astype(np.int64)
    return np.where((code == 0)[:, None], nm, ns).astype(f32), code


def host_rows(ng, ns, e1, e2, uv6, c, s):
    """The (k, 22) rows wfpt_mapped_normal_host takes."""
    k = len(np.asarray(ng).reshape(-1, 3))
    cols = [np.asarray(a, f32).reshape(k, -1) for a in (ng, ns, e1, e2, uv6, c)] + [np.broadcast_to(np.asarray(s, f32), (k,)).reshape(k, 1)]
    return np.ascontiguousarray(np.concatenate(cols, 1), f32)


class Mapped:
    """What a mapped context holds: the triangles as the device holds them (rows named by _pad), the UV table (n, 6) or None, the slots
    {slot: (img, params)} as texture_ref.Textures takes them, the bindings {material_idx: (slot, strength)}, and the table of corner
    normals as a shading_normals_ref.Normals over the same triangles, or None (ns is the stored normal then)."""

    def __init__(self, triangles, uv, slots, bind, normals=None, **mutations):
        self.triangles = triangles
        self.uv = None if uv is None else np.asarray(uv, f32).reshape(-1, 6)
        self.slots, self.bind = dict(slots), dict(bind)
        self.normals = normals
        self.mutations = mutations

    def at(self, prim, p):
        """(n (k, 3), code (k,)) of hits at p on triangles prim: codes 0-3 of mapped_normal, 4 where the material has no map."""
        prim = np.asarray(prim, np.int64).reshape(-1)
        p = np.asarray(p, f32).reshape(-1, 3)
        t = self.triangles[prim]
        ng = triangle_normal_area(t)[0]
        ns = self.normals.at(prim, p)[0] if self.normals is not None else ng
        out, code = np.array(ns, f32), np.full(len(prim), 4, np.int64)
        mat = t["material_idx"].astype(np.int64)
        rows = np.zeros((len(prim), 6), f32) if self.uv is None else self.uv[t["_pad"].astype(np.int64)]
        for m, (slot, strength) in self.bind.items():
            sel = mat == m
            if not sel.any():
                continue
            img, params = self.slots[slot]
            u, v = T.triangle_uv(p[sel], t["v0"][sel], t["e1"][sel], t["e2"][sel], rows[sel])  # A.
            c = T.tex_lookup(img, u, v, **params)
            out[sel], code[sel] = mapped_normal(ng[sel], ns[sel], t["e1"][sel], t["e2"][sel], rows[sel], c, f32(strength), **self.mutations)
        return out, code

    def sample_rows(self, p, prim):
        """wfpt_sample_normal_map's rows for points p on triangles prim: (n.xyz | code)."""
        n, code = self.at(prim, p)
        return np.concatenate([n, code.astype(f32)[:, None]], 1).astype(f32)


# ---------------------------------------------------------------- the scene of the tests
def spherical_uv(corners):
    """u = atan2(-z, x) / 2pi + 0.5, v = atan2(hypot(x, z), -y) / pi of corner positions (n, 3, 3) -> (n, 6) float64, with the seam
    repaired: in a triangle whose corner u span more than 0.5 the corners with u < 0.5 get u + 1."""
    x, y, z = corners[..., 0], corners[..., 1], corners[..., 2]
    u = np.arctan2(-z, x) / (2.0 * np.pi) + 0.5
    v = np.arctan2(np.hypot(x, z), -y) / np.pi
    seam = (u.max(axis=1) - u.min(axis=1)) > 0.5
    u = np.where(seam[:, None] & (u < 0.5), u + 1.0, u)
    return np.stack([u[:, 0], v[:, 0], u[:, 1], v[:, 1], u[:, 2], v[:, 2]], 1)


def sphere_scene(orc, emitter=False):
    """shading_normals_ref.sphere_scene plus the UV table: spherical UVs on the icosphere, planar UVs on the ground's first triangle
    (det > 0) and mirrored ones (u -> 1 - u, det < 0) on its second; a lamp's rows are zero. Returns (triangles in creation order,
    materials, n9, uv) -- uv's rows are named by _pad, as n9's."""
    t, mt, n9 = S.sphere_scene(orc, emitter=emitter)
    n = len(t)
    n_s = int((t["material_idx"] < 3).sum())
    v0 = t["v0"].astype(np.float64)
    corners = np.stack([v0, v0 + t["e1"], v0 + t["e2"]], 1)
    uv = np.zeros((n, 6))
    uv[:n_s] = spherical_uv(corners[:n_s])
    for j in range(2):
        c = corners[n_s + j]
        u, v = (c[:, 0] + 6.0) / 12.0, (6.0 - c[:, 2]) / 12.0
        if j == 1:
            u = 1.0 - u
        uv[n_s + j] = np.stack([u, v], 1).reshape(6)
    table = np.zeros((n, 6), f32)
    table[t["_pad"].astype(np.int64)] = uv.astype(f32)
    return t, mt, n9, table


def tilt_map(seed=4, w=16, h=8, max_tilt=0.7):
    """A seeded (h, w, 3) float32 map of unit vectors tilted up to max_tilt rad from +z, stored as 0.5 + 0.5 n."""
    rng = np.random.default_rng(seed)
    theta, phi = rng.uniform(0.0, max_tilt, (h, w)), rng.uniform(0.0, 2.0 * np.pi, (h, w))
    nrm = np.stack([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)], 2)
    return (0.5 + 0.5 * nrm).astype(f32)


def flat_map(w=4, h=2):
    """An all-(0.5, 0.5, 1) map: step B's identity at every texel."""
    img = np.zeros((h, w, 3), f32)
    img[:] = (0.5, 0.5, 1.0)
    return img


def probe_rows(p, prim):
    return S.probe_rows(p, prim)
