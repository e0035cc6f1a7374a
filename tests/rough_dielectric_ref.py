"""numpy float32 restatement of GGX rough dielectrics (WFPT_FLAG_ROUGH_DIELECTRIC, include/wfpt.h "Rough dielectrics"): the pass's own
random stream (step 0), steps 1-12 at a hit, the retyped per-hit record of step 13 substituted into a whole render driven through the
oracle's stages, and a float64 midpoint quadrature over the microfacet normals of the mean the estimator's weight must have. Steps 2-9 are
microfacet_ref.sample's (one statement for both features, as on the device); `RoughGlass` is microfacet_ref.Rough with the dielectric hits
sampled as well: after the queue swap their extension rays are scatter()'s METAL branch about the pseudo-normal h with fuzz +0, which is
what the retyped record makes the unchanged shade step compute. Every step is one IEEE f32 operation in the header's order (pow is the
oracle's own statement of the library's), so the results are the device's bits."""
import numpy as np

import microfacet_ref as MF
import shading_normals_ref as S
from nee_ref import jenkins_hash, rng_next_float
from transport_ref import dot3, f32

u32 = np.uint32
STREAM = 0x27D4EB2F
MUTATIONS = {"no_G": False, "eta_not_flipped_inside": False, "always_refract": False, "g_on_wrong_side": False}


# ---------------------------------------------------------------- step 0: the pass's own stream
def draws(pixel_idx, frame, b):
    """u1, u2, u3 of a rough glass hit for pixels pixel_idx (x + y W) in the sample of frame `frame`, wavefront b."""
    s = jenkins_hash(np.asarray(pixel_idx, u32) ^ jenkins_hash(u32(frame)))
    s = jenkins_hash(s ^ u32((STREAM * (b + 1)) & 0xFFFFFFFF))
    u1, s = rng_next_float(s)
    u2, s = rng_next_float(s)
    u3, s = rng_next_float(s)
    return u1, u2, u3


# ---------------------------------------------------------------- steps 1-12
def _g1(co, a2, one=f32(1), two=f32(2)):
    return (two * co) / (co + np.sqrt(a2 + (one - a2) * (co * co)))


def sample(d, n, u1, u2, u3, alpha, ior, albedo, **mutations):
    """Steps 1-12 for k hits: d, n, albedo (k, 3); u1, u2, u3, alpha, ior (k,). Returns h, weight, w (k, 3) -- w is the outgoing unit
    direction of step 11 --, fell (steps 1 or 11 fell back: h, weight are +0), dead (the weight is +0), refracted, inside and m.
    mutations (tests/test_rough_dielectric_host.py): no_G drops G; eta_not_flipped_inside keeps eta = 1 / ior from inside;
    always_refract ignores the Fresnel choice wherever refraction exists; g_on_wrong_side evaluates G on the cosine of the arm not taken."""
    unknown = set(mutations) - set(MUTATIONS)
    if unknown:
        raise TypeError(f"sample() got unexpected keywords {sorted(unknown)}")
    mut = dict(MUTATIONS, **mutations)
    d, n, albedo = (np.asarray(a, f32).reshape(-1, 3) for a in (d, n, albedo))
    k = len(d)
    u1, u2, u3, alpha, ior = (np.ascontiguousarray(np.broadcast_to(np.asarray(a, f32).reshape(-1), (k,))) for a in (u1, u2, u3, alpha, ior))
    one, zero, two = f32(1), f32(0), f32(2)
    with np.errstate(all="ignore"):
        # 1.
        uv = MF._normalize(d)
        wi = -uv
        cn = dot3(n, wi)
        inside = cn < 0
        nf = np.where(inside[:, None], -n, n)
        cn = np.where(inside, -cn, cn)
        eta = np.where(inside & (not mut["eta_not_flipped_inside"]), ior, one / ior).astype(f32)
        fell = ~(cn > 0)
        # 2-9. (microfacet_ref's steps 1-9 are these: the same flip, the same fall-back)
        m = MF.sample(d, n, u1, u2, alpha, np.zeros((k, 3), f32))["m"]
        # 10.
        cm = dot3(wi, m)
        dead10 = ~(cm > 0)
        r0 = (one - eta) / (one + eta)
        r0 = r0 * r0
        x = np.where(dead10 | fell, zero, one - np.fmin(cm, one)).astype(f32)  # (pow is not asked about the rows that never reach it)
        F = r0 + (one - r0) * S._pow(x, 5.0)
        ct = -cm
        kk = one - eta * eta * (one - ct * ct)
        # 11.
        reflects = ~(kk >= 0) | ((F > u3) & (not mut["always_refract"]))
        w_r = (two * cm)[:, None] * m - wi
        co_r = dot3(nf, w_r)
        mm = (one - eta * eta) / (np.sqrt(kk) + eta * cm)
        w_t = eta[:, None] * uv - mm[:, None] * m
        co_t = -dot3(nf, w_t)
        hv = (eta - one)[:, None] * uv - mm[:, None] * m
        l2 = dot3(hv, hv)
        h_t = hv * (one / np.sqrt(l2))[:, None]
        refracted = ~reflects & ~dead10 & ~fell
        fell = fell | (refracted & ~(l2 > 0))
        refracted = refracted & ~fell
        co = np.where(refracted, co_t, co_r)
        dead = (dead10 | ~(co > 0)) & ~fell
        # 12.
        a2 = alpha * alpha
        cg = np.where(kk >= 0, np.where(refracted, np.abs(co_r), np.abs(co_t)), co) if mut["g_on_wrong_side"] else co
        G = np.ones_like(co) if mut["no_G"] else _g1(cg, a2)
        weight = albedo * G[:, None]
    weight = np.where((fell | dead)[:, None], zero, weight).astype(f32)
    h = np.where(refracted[:, None], h_t, m)
    h = np.where(fell[:, None], zero, h).astype(f32)
    w = np.where(refracted[:, None], w_t, w_r).astype(f32)
    return {"h": h, "weight": weight, "w": w, "fell": fell, "dead": dead, "refracted": refracted, "inside": inside, "m": m, "uv": uv.astype(f32),
            "eta": eta}


def probe_rows(d, n, u1, u2, u3, alpha, ior, albedo):
    """The rows wfpt_sample_rough_dielectric takes: (d.xyz, n.xyz, u1, u2 | u3, alpha, ior, albedo.rgb, 0, 0)."""
    d, n, albedo = (np.asarray(a, f32).reshape(-1, 3) for a in (d, n, albedo))
    k = len(d)
    cols = [np.broadcast_to(np.asarray(a, f32).reshape(-1), (k,))[:, None] for a in (u1, u2, u3, alpha, ior)]
    return np.ascontiguousarray(np.concatenate([d, n] + cols + [albedo, np.zeros((k, 2), f32)], 1), f32)


def sample_row_parts(rows, **mutations):
    rows = np.asarray(rows, f32).reshape(-1, 16)
    return sample(rows[:, 0:3], rows[:, 3:6], rows[:, 6], rows[:, 7], rows[:, 8], rows[:, 9], rows[:, 10], rows[:, 11:14], **mutations)


def sample_rows(rows, **mutations):
    """wfpt_sample_rough_dielectric's answer for its rows: (h.xyz | 2.0 fell back, 1.0 dead, else 0.0), (weight.rgb | 1.0 refracted)."""
    r = sample_row_parts(rows, **mutations)
    state = np.where(r["fell"], f32(2), np.where(r["dead"], f32(1), f32(0))).astype(f32)
    return np.concatenate([r["h"], state[:, None], r["weight"], r["refracted"].astype(f32)[:, None]], 1).astype(f32)


def reflect_about(uv, h):
    """scatter()'s metal branch with fuzz +0 in f32: reflect(uv, h) + 0 rb, rb a unit vector"""
    uv, h = np.asarray(uv, f32), np.asarray(h, f32)
    return (uv - (f32(2) * dot3(uv, h))[:, None] * h).astype(f32)


def outgoing_f64(uv, m, eta, refracted):
    """steps 10-11's outgoing direction for the arm `refracted` names, evaluated in float64 from the float32 uv, m and eta"""
    uv, m, eta = np.asarray(uv, np.float64), np.asarray(m, np.float64), np.asarray(eta, np.float64)
    cm = -np.einsum("ij,ij->i", uv, m)
    w_r = uv + (2.0 * cm)[:, None] * m
    with np.errstate(all="ignore"):
        kk = 1.0 - eta * eta * (1.0 - cm * cm)
        w_t = eta[:, None] * uv - (eta * -cm + np.sqrt(kk))[:, None] * m
    return np.where(np.asarray(refracted)[:, None], w_t, w_r)


# ---------------------------------------------------------------- the quadrature
FACING = np.array([0.36, -0.48, 0.8])


def cell_rows(alpha, cn, inside, k, seed, ior=1.5, albedo=(1.0, 1.0, 1.0)):
    """k probe rows of one cell: the direction arrives at the cosine cn against the facing normal (0.36, -0.48, 0.8); from inside the
    stored normal is its negative. Uniform draws."""
    side = np.cross(FACING, [0.0, 0.0, 1.0])
    side /= np.linalg.norm(side)
    wi = cn * FACING + np.sqrt(1.0 - cn * cn) * side
    rng = np.random.default_rng(seed)
    u = rng.random((k, 3), dtype=np.float32)
    stored = -FACING if inside else FACING
    return probe_rows(np.tile(-1.7 * wi, (k, 1)), np.tile(stored, (k, 1)), u[:, 0], u[:, 1], u[:, 2], alpha, ior, np.tile(albedo, (k, 1)))


def directional_albedo_rt(alpha, cn, eta, n_theta=1200, n_phi=2400):
    """The mean of the estimator's weight at albedo 1, float64, midpoint rule over the microfacet normals m of the hemisphere about the
    facing normal: the integral of D(m) G1(wi) max(0, wi.m) / cn -- the density of visible normals, from the distribution D itself, no
    draw -- times F G1(co_r) 1(co_r > 0) + (1 - F) G1(co_t) 1(co_t > 0, k >= 0), F = 1 where k < 0 (total internal reflection)."""
    a2 = float(alpha) ** 2
    # (the polar angle's grid is uniform in s with tan(theta) = alpha tan(s): as dense about the pole as D is narrow; jac = d theta / d s)
    sg = (np.arange(n_theta) + 0.5) * (0.5 * np.pi / n_theta)
    th = np.arctan(float(alpha) * np.tan(sg))
    jac = (float(alpha) / np.cos(sg) ** 2 / (1.0 + a2 * np.tan(sg) ** 2))[:, None]
    ph = (np.arange(n_phi) + 0.5) * (2.0 * np.pi / n_phi)
    st, ctm = np.sin(th)[:, None], np.cos(th)[:, None]
    mx, my, mz = st * np.cos(ph)[None, :], st * np.sin(ph)[None, :], np.broadcast_to(ctm, (n_theta, n_phi))
    wx, wz = np.sqrt(1.0 - cn * cn), cn

    def g1(c):
        return 2.0 * c / (c + np.sqrt(a2 + (1.0 - a2) * c * c))

    D = a2 / (np.pi * (mz * mz * (a2 - 1.0) + 1.0) ** 2)
    cm = wx * mx + wz * mz
    vis = D * g1(cn) * np.maximum(0.0, cm) / cn * st * jac
    cmc = np.clip(cm, 0.0, 1.0)
    r0 = ((1.0 - eta) / (1.0 + eta)) ** 2
    kk = 1.0 - eta * eta * (1.0 - cmc * cmc)
    F = np.where(kk >= 0, r0 + (1.0 - r0) * (1.0 - cmc) ** 5, 1.0)
    co_r = 2.0 * cm * mz - wz  # dot(nf, (2 cm) m - wi)
    co_t = -(eta * -wz - (eta * -cm + np.sqrt(np.maximum(kk, 0.0))) * mz)  # -dot(nf, eta uv - (eta ct + sqrt k) m), uv = -wi
    with np.errstate(all="ignore"):
        refl = np.where(co_r > 0, g1(np.maximum(co_r, 1e-300)), 0.0)
        refr = np.where((co_t > 0) & (kk >= 0), g1(np.maximum(co_t, 1e-300)), 0.0)
    dw = (0.5 * np.pi / n_theta) * (2.0 * np.pi / n_phi)
    return float(np.sum(vis * (F * refl + (1.0 - F) * refr)) * dw)


# ---------------------------------------------------------------- the render
class RoughGlass(MF.Rough):
    """microfacet_ref.Rough whose extend() also samples the hits of dielectric primitives (material_type 2) of a material with an alpha
    above 0, and whose swap_ray_queues() scatters them as the retyped record makes shade scatter them: type 1 about h with fuzz +0. The
    metal hits stay Rough's. counts: the sampled glass hits by ("reflect" | "refract", "outside" | "inside")."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.glass = None
        self.glass_sampled = 0
        self.counts = {(arm, side): 0 for arm in ("reflect", "refract") for side in ("outside", "inside")}

    def extend(self, gx, gy):
        super().extend(gx, gy)  # (Rough's: the metal hits; self.cur is None where the pass does not run)
        self.glass = None
        if self.cur is None:
            return
        b = len(self.tables[-1]) - 1
        n_hit = len(self.cur["ok"])
        hits = self.o.hits(n_hit)
        rays = self.o.rays()[hits["ray_idx"].astype(np.int64)]
        t = self.triangles[hits["sphere_idx"].astype(np.int64)]
        midx = t["material_idx"].astype(np.int64)
        sel = (t["material_type"] == 2) & (self.alpha[midx] > 0)
        glass = np.zeros(n_hit, bool)
        if sel.any():
            u1, u2, u3 = draws(rays["pixel_idx"][sel], self.frame, b)
            mat = self.materials[midx[sel]]
            r = sample(rays["direction"][sel, :3].astype(f32), self.cur["n"][sel], u1, u2, u3, self.alpha[midx[sel]], mat["refract_index"],
                       np.asarray(mat["albedo"][:, :3], f32), **self.mutations)
            glass[sel] = ~r["fell"]
            self.cur["ok"][sel] = ~r["fell"]
            self.cur["m"][sel], self.cur["weight"][sel] = r["h"], r["weight"]
            live = ~r["fell"]
            self.glass_sampled += int(live.sum())
            for arm, a in (("reflect", ~r["refracted"]), ("refract", r["refracted"])):
                for side, s in (("outside", ~r["inside"]), ("inside", r["inside"])):
                    self.counts[(arm, side)] += int((live & a & s).sum())
        self.glass = glass

    def swap_ray_queues(self):
        if self._noted is not None and self.glass is not None and self.glass.any():
            hits, rays = self._noted
            assert len(hits) == len(self.glass)
            hits = hits.copy()
            hits["mat_type"][self.glass] = 1  # step 13: the record's type word
            self._noted = (hits, rays)
        self.glass = None
        super().swap_ray_queues()
