"""numpy float32 restatement of GGX microfacet metals (WFPT_FLAG_MICROFACET, include/wfpt.h "Microfacet metals"): the pass's own random
stream (step 0), steps 1-11 at a hit, the per-hit record of step 12 substituted into a whole render driven through the oracle's stages,
and a float64 midpoint quadrature of the directional albedo the estimator's mean must equal. The oracle reflects metal about the stored
normal and multiplies by the albedo, so `Rough` wraps it in the style of shading_normals_ref.Shaded: it samples the hits after extend(),
and after the queue swap rewrites the extension rays' directions with scatter() restated about m with fuzz +0 (about the shading normal
for the other hits, where a table of normals is set); `rough_weights` substitutes the weight for shade's albedo for the duration of a
transport_ref.render. Every step is one IEEE f32 operation in the header's order (sin and cos are the oracle's own statement of the
library's), so the results are the device's bits."""
import contextlib

import numpy as np

import shading_normals_ref as S
import transport_ref
from nee_ref import PI, jenkins_hash, rng_next_float, sincos
from transport_ref import dot3, f32, triangle_normal_area

u32 = np.uint32
MUTATIONS = {"no_G": False, "fresnel_on_cn": False, "no_warp": False}


# ---------------------------------------------------------------- step 0: the pass's own stream
def draws(pixel_idx, frame, b):
    """u1, u2 of the microfacet pass for pixels pixel_idx (x + y W) in the sample of frame `frame`, wavefront b."""
    s = jenkins_hash(np.asarray(pixel_idx, u32) ^ jenkins_hash(u32(frame)))
    s = jenkins_hash(s ^ u32((0xC2B2AE35 * (b + 1)) & 0xFFFFFFFF))
    u1, s = rng_next_float(s)
    u2, s = rng_next_float(s)
    return u1, u2


# ---------------------------------------------------------------- steps 1-11
def _normalize(v):
    inv = f32(1) / np.sqrt(dot3(v, v))
    return v * inv[:, None]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def sample(d, n, u1, u2, alpha, f0, **mutations):
    """Steps 1-11 for k hits: d, n, f0 (k, 3); u1, u2, alpha (k,). Returns m, weight (k, 3), cm (k,), fell (step 1 fell back: m, weight, cm
    are +0) and dead (step 10 left the weight at zero). mutations (tests/test_microfacet_host.py): no_G drops G, fresnel_on_cn takes the
    Fresnel term's cosine from the normal instead of the microfacet, no_warp drops step 6's warp of t2."""
    unknown = set(mutations) - set(MUTATIONS)
    if unknown:
        raise TypeError(f"sample() got unexpected keywords {sorted(unknown)}")
    mut = dict(MUTATIONS, **mutations)
    d, n, f0 = (np.asarray(a, f32).reshape(-1, 3) for a in (d, n, f0))
    u1, u2, alpha = (np.asarray(a, f32).reshape(-1) for a in (u1, u2, alpha))
    one, zero = f32(1), f32(0)
    with np.errstate(all="ignore"):
        wi = -_normalize(d)
        cn = dot3(n, wi)
        flip = cn < 0
        nf = np.where(flip[:, None], -n, n)
        cn = np.where(flip, -cn, cn)
        fell = ~(cn > 0)
        # 2.
        sg = np.where(nf[:, 2] >= 0, one, -one).astype(f32)
        a = -one / (sg + nf[:, 2])
        bb = (nf[:, 0] * nf[:, 1]) * a
        t = np.stack([one + ((sg * nf[:, 0]) * nf[:, 0]) * a, sg * bb, -(sg * nf[:, 0])], 1)
        bt = np.stack([bb, sg + (nf[:, 1] * nf[:, 1]) * a, -nf[:, 1]], 1)
        # 3-5.
        lx, ly, lz = dot3(t, wi), dot3(bt, wi), cn
        vh = _normalize(np.stack([alpha * lx, alpha * ly, lz], 1))
        l2 = vh[:, 0] * vh[:, 0] + vh[:, 1] * vh[:, 1]
        il = one / np.sqrt(l2)
        has = l2 > 0
        T1 = np.stack([np.where(has, -vh[:, 1] * il, one), np.where(has, vh[:, 0] * il, zero), np.zeros_like(l2)], 1).astype(f32)
        T2 = _cross(vh, T1)
        # 6-8.
        r = np.sqrt(u1)
        sn, cs = sincos((f32(2) * PI) * u2)
        t1, t2 = r * cs, r * sn
        s = f32(0.5) * (one + vh[:, 2])
        if not mut["no_warp"]:
            t2 = (one - s) * np.sqrt(np.fmax(zero, one - t1 * t1)) + s * t2
        h = np.sqrt(np.fmax(zero, (one - t1 * t1) - t2 * t2))
        nh = (t1[:, None] * T1 + t2[:, None] * T2) + h[:, None] * vh
        ml = _normalize(np.stack([alpha * nh[:, 0], alpha * nh[:, 1], np.fmax(zero, nh[:, 2])], 1))
        # 9.
        m = (ml[:, 0:1] * t + ml[:, 1:2] * bt) + ml[:, 2:3] * nf
        # 10.
        cm = dot3(wi, m)
        wo = (f32(2) * cm)[:, None] * m - wi
        co = dot3(nf, wo)
        dead = (~(cm > 0) | ~(co > 0)) & ~fell
        # 11.
        a2 = alpha * alpha
        G = (f32(2) * co) / (co + np.sqrt(a2 + (one - a2) * (co * co)))
        if mut["no_G"]:
            G = np.ones_like(G)
        f = one - (cn if mut["fresnel_on_cn"] else cm)
        f5 = ((f * f) * (f * f)) * f
        F = f0 + (one - f0) * f5[:, None]
        weight = F * G[:, None]
    gone = fell | dead
    weight = np.where(gone[:, None], zero, weight).astype(f32)
    m = np.where(fell[:, None], zero, m).astype(f32)
    cm = np.where(fell, zero, cm).astype(f32)
    return {"m": m, "weight": weight, "cm": cm, "fell": fell, "dead": dead}


def probe_rows(d, n, u1, u2, alpha, f0):
    """The rows wfpt_sample_microfacet takes: (d.xyz, n.xyz, u1, u2, alpha, F0.rgb)."""
    d, n, f0 = (np.asarray(a, f32).reshape(-1, 3) for a in (d, n, f0))
    k = len(d)
    cols = [np.broadcast_to(np.asarray(a, f32).reshape(-1), (k,))[:, None] for a in (u1, u2, alpha)]
    return np.ascontiguousarray(np.concatenate([d, n] + cols + [f0], 1), f32)


def sample_rows(rows, **mutations):
    """wfpt_sample_microfacet's answer for its rows: (m.xyz | 2.0 fell back, 1.0 dead, else 0.0 | weight.rgb | cm)."""
    rows = np.asarray(rows, f32).reshape(-1, 12)
    r = sample(rows[:, 0:3], rows[:, 3:6], rows[:, 6], rows[:, 7], rows[:, 8], rows[:, 9:12], **mutations)
    state = np.where(r["fell"], f32(2), np.where(r["dead"], f32(1), f32(0))).astype(f32)
    return np.concatenate([r["m"], state[:, None], r["weight"], r["cm"][:, None]], 1).astype(f32)


# ---------------------------------------------------------------- the quadrature
def cell_rows(alpha, cn, f0, k, seed):
    """k probe rows of one cell: the normal (0.36, -0.48, 0.8), the direction arriving at the cosine cn against it, uniform draws."""
    n = np.array([0.36, -0.48, 0.8])
    side = np.cross(n, [0.0, 0.0, 1.0])
    side /= np.linalg.norm(side)
    wi = cn * n + np.sqrt(1.0 - cn * cn) * side
    rng = np.random.default_rng(seed)
    u = rng.random((k, 2), dtype=np.float32)
    return probe_rows(np.tile(-1.7 * wi, (k, 1)), np.tile(n, (k, 1)), u[:, 0], u[:, 1], alpha, np.tile(f0, (k, 1)))


def directional_albedo(alpha, cn, f0, n_theta=1500, n_phi=3000):
    """The integral over the outgoing hemisphere of D F G1(wi) G1(wo) / (4 cn co) * co, per channel of f0, float64, midpoint rule in the
    polar angles of wo about the normal: what the mean of the estimator's weight F G1(wo) over the visible normals equals. D is the GGX
    distribution, G1 the separable Smith term of step 11, F Schlick's term on the cosine between wi and the half vector."""
    a2 = float(alpha) ** 2
    th = (np.arange(n_theta) + 0.5) * (0.5 * np.pi / n_theta)
    ph = (np.arange(n_phi) + 0.5) * (2.0 * np.pi / n_phi)
    st, ct = np.sin(th)[:, None], np.cos(th)[:, None]
    wo = np.stack([st * np.cos(ph)[None, :], st * np.sin(ph)[None, :], np.broadcast_to(ct, (n_theta, n_phi))], -1)
    wi = np.array([np.sqrt(1.0 - cn * cn), 0.0, cn])
    hv = wo + wi
    hv /= np.linalg.norm(hv, axis=-1, keepdims=True)
    ch, cm, co = hv[..., 2], hv @ wi, wo[..., 2]

    def g1(c):
        return 2.0 * c / (c + np.sqrt(a2 + (1.0 - a2) * c * c))

    D = a2 / (np.pi * (ch * ch * (a2 - 1.0) + 1.0) ** 2)
    base = D * g1(cn) * g1(co) / (4.0 * cn) * st  # (the co of the rendering equation cancels the BRDF's)
    f5 = (1.0 - cm) ** 5
    dw = (0.5 * np.pi / n_theta) * (2.0 * np.pi / n_phi)
    f0 = np.asarray(f0, np.float64)
    return np.array([np.sum(base * (c + (1.0 - c) * f5)) * dw for c in f0])


# ---------------------------------------------------------------- the render
class Rough(S.Shaded):
    """An Oracle (or a wrapper around one) over a triangle scene whose rough hits are shaded as the microfacet pass leaves them. triangles:
    the scene's, in the device's order; materials: the scene's; alphas: {material_idx: alpha}; normals: a shading_normals_ref.Normals where
    the context holds a table of corner normals as well (every hit then scatters about its shading normal), else None. Goes where Shaded
    goes: inside adaptive_ref.Local, around or inside Masked / Retiring. Use with rough_weights(self) around the render."""

    def __init__(self, o, triangles, materials, alphas, normals=None, **mutations):
        super().__init__(o, normals, materials)
        self.triangles = triangles
        self.alpha = np.zeros(len(materials), f32)
        for m, a in alphas.items():
            self.alpha[m] = a
        self.mutations = mutations
        self.cur = None
        self.sampled = 0

    def extend(self, gx, gy):
        super().extend(gx, gy)
        self.cur = None
        b = len(self.tables[-1]) - 1
        if b + 1 >= self.o.params.max_wavefronts:  # the pass does not run before the last wavefront's step
            return
        n_hit = int(self.o.counters()[1])
        if n_hit == 0:
            return
        hits = self.o.hits(n_hit)
        rays = self.o.rays()[hits["ray_idx"].astype(np.int64)]
        prim = hits["sphere_idx"].astype(np.int64)
        org, d = rays["origin"][:, :3].astype(f32), rays["direction"][:, :3].astype(f32)
        pt = org + hits["t"].astype(f32)[:, None] * d  # sh:91
        t = self.triangles[prim]
        midx = t["material_idx"].astype(np.int64)
        n = self.normals.at(prim, pt)[0] if self.normals is not None else triangle_normal_area(t)[0]
        alpha = np.where(t["material_type"] == 1, self.alpha[midx], f32(0)).astype(f32)
        rough = alpha > 0
        ok = np.zeros(n_hit, bool)
        m, weight = np.zeros((n_hit, 3), f32), np.zeros((n_hit, 3), f32)
        if rough.any():
            u1, u2 = draws(rays["pixel_idx"][rough], self.frame, b)
            f0 = np.asarray(self.materials["albedo"][midx[rough], :3], f32)
            r = sample(d[rough], n[rough], u1, u2, alpha[rough], f0, **self.mutations)
            ok[rough] = ~r["fell"]
            m[rough], weight[rough] = r["m"], r["weight"]
            self.sampled += int(ok.sum())
        self.cur = {"ok": ok, "m": m, "weight": weight, "n": n}

    def weights(self, alb):
        """shade's factor per hit of the wavefront extend() has just traced: the weight at a rough hit, the albedo `alb` elsewhere"""
        if self.cur is None:
            return alb
        assert len(alb) == len(self.cur["ok"]), "the wave's hits are not the ones extend() sampled"
        return np.where(self.cur["ok"][:, None], self.cur["weight"], alb).astype(f32)

    def swap_ray_queues(self):
        from helpers import shade_rng_key
        from oracle import oracle as O
        self.o.swap_ray_queues()
        noted, self._noted = self._noted, None
        cur, self.cur = self.cur, None
        if noted is None or cur is None:
            return
        hits, rays = noted
        n = len(hits)
        assert n == len(cur["ok"])
        sel = cur["ok"] | (self.normals is not None)
        if not sel.any():
            return
        P, W_ = self.o.params, self.o.width
        prim = hits["sphere_idx"].astype(np.int64)
        d = rays["direction"][:, :3].astype(f32)
        mat = self.materials[self.triangles[prim]["material_idx"].astype(np.int64)]
        pix = rays["pixel_idx"].astype(np.int64)
        key = [shade_rng_key(i, n, W_, P.rng_mode, int(pix[i]), O.workgroup_size_64) for i in range(n)]
        px, py = np.array([k[0] for k in key], np.int64), np.array([k[1] for k in key], np.int64)
        rb = np.stack([O.probe_shade_rb(int(x), int(y), W_, self.frame, 0) for x, y in zip(px, py)]).astype(f32)
        nrm = np.where(cur["ok"][:, None], cur["m"], cur["n"]).astype(f32)
        fuzz = np.where(cur["ok"], f32(0), mat["fuzz"]).astype(f32)
        ext_dir = S.scatter(nrm, d, hits["mat_type"], fuzz, mat["refract_index"], rb, S.first_draw(px, py, W_, self.frame))
        ext = self.o.rays(n)
        assert np.array_equal(ext["pixel_idx"], rays["pixel_idx"]), "extension ray h is not hit h's"
        ext["direction"][sel, :3] = ext_dir[sel]
        with np.errstate(all="ignore"):
            ext["inv_direction"][sel] = f32(1) / ext_dir[sel]
        self.o.write_rays(ext)


@contextlib.contextmanager
def rough_weights(rough):
    """For the duration of a render, the albedo transport_ref.render multiplies a hit's throughput by is rough.weights(albedo)."""
    keep = transport_ref._Wave

    class Wave(keep):
        @property
        def alb(self):
            return self._alb

        @alb.setter
        def alb(self, v):
            self._alb = rough.weights(np.asarray(v, f32))

    transport_ref._Wave = Wave
    try:
        yield
    finally:
        transport_ref._Wave = keep
