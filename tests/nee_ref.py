"""numpy float32 restatement of next-event estimation (WFPT_FLAG_NEE, include/wfpt.h "Next-event estimation"): emission_ref.render_with_emission
with the per-pixel connected flag, the gated emission add, and the connect pass between the emission pass and shade's albedo. Every step
is one IEEE f32 operation in the header's order (sin / cos are the oracle's own statement of the library's), so the results are the
device's bits. Occlusion comes from the oracle itself: a second Oracle over the same scene traces the shadow rays (write_rays, extend) and
its closest t is compared with dist * 0.999 -- no traversal is rewritten here."""
import ctypes as C

import numpy as np

from denoise_ref import luma
from environment_ref import env_lookup, normalize3, sky

f32 = np.float32
u32 = np.uint32
PI = f32(3.1415927)


# ---------------------------------------------------------------- the pass's own random stream (shade.wgsl's jenkins_hash, init_rng, rng_next_float)
def jenkins_hash(x):
    x = np.asarray(x, u32).copy()
    with np.errstate(over="ignore"):
        x += x << u32(10)
        x ^= x >> u32(6)
        x += x << u32(3)
        x ^= x >> u32(11)
        x += x << u32(15)
    return x


def rng_next_float(state):
    """(the draw, the next state): PCG-RXS-M-XS-32, then f32(word) * 2^-32 (one rounding each)."""
    with np.errstate(over="ignore"):
        s = state * u32(747796405) + u32(2891336453)
        word = ((s >> ((s >> u32(28)) + u32(4))) ^ s) * u32(277803737)
    word = (word >> u32(22)) ^ word
    return word.astype(f32) * f32(2.3283064365387e-10), s


def connect_draws(pixel_idx, frame, b):
    """u0, u1, u2 of the connect pass for pixels pixel_idx (x + y W) in the sample of frame `frame`, wavefront b."""
    s = jenkins_hash(np.asarray(pixel_idx, u32) ^ jenkins_hash(u32(frame)))
    s = jenkins_hash(s ^ u32((0x9E3779B9 * (b + 1)) & 0xFFFFFFFF))
    u0, s = rng_next_float(s)
    u1, s = rng_next_float(s)
    u2, s = rng_next_float(s)
    return u0, u1, u2


def sincos(x):
    from oracle import oracle as O
    x = np.ascontiguousarray(x, "<f4")
    s, c = np.zeros_like(x), np.zeros_like(x)
    O.lib().orc_probe_sincos(x.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p), x.size)
    return s, c


def dot3(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


class Lights:
    """The light list of an emission_ref.Emission: the primitives whose material emits, in primitive order; tx (texture_ref.Textures or None)
    modulates a textured light's colour at the sampled point."""

    def __init__(self, em, tx=None):
        self.em, self.tx = em, tx
        prims = em.prims()
        e = em.table[prims["material_idx"].astype(np.int64)]
        self.list = np.flatnonzero((e != 0).any(axis=1)).astype(np.int64)
        self.n = len(self.list)

    def sample(self, p, n, u0, u1, u2):
        """Steps 3 and 4 for receivers p (k, 3) with normals n (k, 3): a dict of q (k, 3), prim (k,), w (k, 3), dist (k,), e_q (k, 3), G (k,)
        and the mask `lit` of the samples that contribute if unoccluded. All-float32, the header's operation order."""
        em = self.em
        p, n = np.asarray(p, f32), np.asarray(n, f32)
        u0, u1, u2 = np.asarray(u0, f32), np.asarray(u1, f32), np.asarray(u2, f32)
        nf = f32(self.n)
        with np.errstate(all="ignore"):
            i = np.fmin(np.fmax(np.floor(u0 * nf), f32(0)), nf).astype(np.int64)
            prim = self.list[np.minimum(i, self.n - 1)]
            if em.triangles is None:
                s = em.spheres[prim]
                c = s["center"][:, :3].astype(f32)
                ra = np.abs(s["radius"].astype(f32))
                z = f32(1) - f32(2) * u1
                r = np.sqrt(np.fmax(f32(0), f32(1) - z * z))
                sn, cs = sincos((f32(2) * PI) * u2)
                q = np.stack([c[:, 0] + ra * (r * cs), c[:, 1] + ra * (r * sn), c[:, 2] + ra * z], 1)
                nl = (q - c) / ra[:, None]
                area = (f32(4) * PI) * (ra * ra)
            else:
                t = em.triangles[prim]
                v0, e1, e2 = t["v0"].astype(f32), t["e1"].astype(f32), t["e2"].astype(f32)
                su = np.sqrt(u1)
                b1, b2 = f32(1) - su, u2 * su
                q = (v0 + b1[:, None] * e1) + b2[:, None] * e2
                cr = [e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]]
                nl = np.stack(normalize3(*cr), 1).astype(f32)
                area = f32(0.5) * np.sqrt((cr[0] * cr[0] + cr[1] * cr[1]) + cr[2] * cr[2])
            v = q - p
            dist2 = dot3(v, v)
            dist = np.sqrt(dist2)
            w = v / dist[:, None]
            cos_s, cos_l = dot3(n, w), np.abs(dot3(nl, w))
            G = (((cos_s * cos_l) * area) * nf) / (PI * dist2)
            e_q = em.table[em.prims()["material_idx"][prim].astype(np.int64)].astype(f32)
            if self.tx is not None and len(prim):
                tex, bound = self.tx.factor(prim, q)
                e_q = np.where(bound[:, None], e_q * tex, e_q)
            lit = (area > 0) & (dist2 > 0) & (cos_s > 0) & (cos_l > 0)
        return {"q": q.astype(f32), "prim": prim, "w": w.astype(f32), "dist": dist.astype(f32), "e_q": e_q.astype(f32), "G": G.astype(f32),
                "lit": lit}


def occluded(shadow, p, w, dist):
    """The oracle's verdict for the shadow rays (p, w) of length dist: the closest hit of `shadow` (an Oracle over the scene with room
    for the rays) has t < dist * 0.999."""
    from oracle import oracle as O
    k = len(p)
    out = np.zeros(k, bool)
    if k == 0:
        return out
    assert k <= shadow.n_slots, (k, shadow.n_slots)
    rays = np.zeros(k, O.RAY)
    rays["origin"][:, :3] = p
    rays["origin"][:, 3] = 1.0
    rays["direction"][:, :3] = w
    with np.errstate(divide="ignore", invalid="ignore"):
        rays["inv_direction"] = f32(1.0) / rays["direction"][:, :3]
    rays["pixel_idx"] = np.arange(k)
    shadow.write_rays(rays)
    shadow.set_counters([0, 0, k])
    shadow.extend(*O.workgroup_size_64(k))
    hits = shadow.hits(int(shadow.counters()[1]))
    ridx = hits["ray_idx"].astype(np.int64)
    out[ridx] = hits["t"].astype(f32) < np.asarray(dist, f32)[ridx] * f32(0.999)
    return out


def render_with_nee(o, shadow, em, spp=1, first_frame=1, tx=None, env=None, env_params=None, parts=False, never_set_flag=False,
                    never_clear_flag=False):
    """emission_ref.render_with_emission with the connect pass. o: the Oracle that renders; shadow: a second Oracle over the same scene
    (any viewport with at least as many ray slots) that traces the shadow rays. With no light it is render_with_emission itself.
    never_set_flag / never_clear_flag: the two mutations of tests/test_nee_host.py (a diffuse hit leaves the flag 0: lights found after a
    diffuse bounce are counted twice; a non-diffuse hit leaves the flag as it was: a lamp seen in a mirror after a diffuse hit goes black)."""
    from oracle import oracle as O
    P = o.params
    assert P.tile_world == 1, "the restatement keys the connect stream by the oracle's pixel index: whole frames only"
    lights = Lights(em, tx)
    gx = (o.width + 7) // 8
    gy = (o.height + 7) // 8
    prims = em.prims()
    albedo = np.asarray(em.materials["albedo"][:, :3], f32)
    ep = dict(env_params or {})
    acc = np.zeros((o.n_pixels, 3), f32)
    s1, s2 = np.zeros(o.n_pixels, f32), np.zeros(o.n_pixels, f32)
    images, emitteds = [], []
    for k in range(spp):
        frame = first_frame + k
        o.set_frame(frame, 0)
        o.reset_image()
        o.set_counters([0, 0, gx * gy * 64])
        o.generate_rays(gx, gy, True)
        thr = o.image().copy()
        emitted = np.zeros_like(thr)
        flag = np.zeros(o.n_pixels, bool)
        ex, ey = O.workgroup_size_64(gx * gy * 64)
        for b in range(P.max_wavefronts):
            n_rays = int(o.counters()[2])
            o.extend(ex, ey)
            c = o.counters()
            n_miss, n_hit = int(c[0]), int(c[1])
            rays = o.rays(max(n_rays, 1))
            hits = o.hits(n_hit)
            ridx = hits["ray_idx"].astype(np.int64)
            hp = rays["pixel_idx"][ridx].astype(np.int64)
            prim = hits["sphere_idx"].astype(np.int64)
            if n_miss < P.miss_floor:
                break
            t = thr[hp]
            e, emits = em.colour(prim)
            org, d = rays["origin"][ridx, :3].astype(f32), rays["direction"][ridx, :3].astype(f32)
            pt = org + hits["t"].astype(f32)[:, None] * d  # sh:91, per component o + t d
            if tx is not None:  # the texture pass
                tex, bound = tx.factor(prim, pt)
                t = np.where(bound[:, None], t * tex, t)
            # the emission pass: thr * e only where the pixel's connected flag is 0 (always, with no light list)
            add = emits & ~flag[hp] if lights.n else emits
            emitted[hp[add]] = emitted[hp[add]] + t[add] * e[add]
            t = np.where(emits[:, None], f32(0), t)
            alb = albedo[prims["material_idx"][prim].astype(np.int64)]
            if lights.n:  # the connect pass
                mclass = prims["material_type"][prim].astype(np.int64)
                diffuse = ((mclass == 0) | (mclass > 2)) & ~emits
                if not never_clear_flag:
                    flag[hp[~diffuse]] = False
                if not never_set_flag:
                    flag[hp[diffuse]] = True
                dp, dpix = pt[diffuse], hp[diffuse]
                if em.triangles is None:
                    nrm = np.stack(normalize3(*[dp[:, a] - em.spheres["center"][prim[diffuse], a] for a in range(3)]), 1).astype(f32)
                else:
                    tr = em.triangles[prim[diffuse]]
                    a_, b_ = tr["e1"], tr["e2"]
                    nrm = np.stack(normalize3(a_[:, 1] * b_[:, 2] - a_[:, 2] * b_[:, 1], a_[:, 2] * b_[:, 0] - a_[:, 0] * b_[:, 2],
                                              a_[:, 0] * b_[:, 1] - a_[:, 1] * b_[:, 0]), 1).astype(f32)
                u0, u1, u2 = connect_draws(dpix, frame, b)
                s = lights.sample(dp, nrm, u0, u1, u2)
                lit = s["lit"]
                occ = np.zeros(len(dp), bool)
                occ[lit] = occluded(shadow, dp[lit], s["w"][lit], s["dist"][lit])
                ok = lit & ~occ
                with np.errstate(all="ignore"):
                    contrib = ((t[diffuse] * alb[diffuse]) * s["e_q"]) * s["G"][:, None]
                emitted[dpix[ok]] = emitted[dpix[ok]] + contrib[ok]
            thr[hp] = t * alb
            midx = o.misses(n_miss).astype(np.int64)
            mp = rays["pixel_idx"][midx].astype(np.int64)
            md = rays["direction"][midx, :3].astype(f32)
            thr[mp] = thr[mp] * (sky(md) if env is None else env_lookup(env, md, ep.get("intensity", 1.0), ep.get("rotation", 0.0)))
            o.set_counters([c[0], c[1], 0] + list(c[3:]))
            sx, sy = O.workgroup_size_64(n_hit)
            o.shade(sx, sy)
            n_ext = int(o.counters()[2])
            o.swap_ray_queues()
            ex, ey = O.workgroup_size_64(n_ext)
            o.set_counters([0, 0, n_ext])
        value = thr + emitted
        acc = acc + value
        L = luma(value)
        s1, s2 = s1 + L, s2 + L * L
        if parts:
            images.append(thr)
            emitteds.append(emitted)
    if not parts:
        return acc
    return {"acc": acc, "image": np.stack(images), "emitted": np.stack(emitteds), "s1": s1, "s2": s2}


# ---------------------------------------------------------------- the lamp scene
LAMP = {"ground_r": 100.0, "lamp_c": (0.0, 2.0, 0.0), "lamp_r": 0.25, "albedo": (0.5, 0.75, 0.25), "e": (16.0, 8.0, 32.0)}


def lamp_inputs(orc, w, h, lamp_r=LAMP["lamp_r"], blocker=False, mirror=False):
    """A large Lambertian ground sphere (material 0) under a small emitting sphere (material 1), seen from above at an angle; blocker: a
    Lambertian sphere (material 2) between lamp and ground; mirror: a fuzz-0 metal sphere (material 3) resting on the ground beside the
    lamp. Returns (spheres, materials, nodes, cam, inv_proj, view); the emitter's colour is LAMP["e"] for material 1."""
    n = 2 + int(blocker) + int(mirror)
    sp = np.zeros(n, orc.SPHERE)
    mt = np.zeros(4, orc.MATERIAL)
    mt["albedo"][:] = (0.5, 0.5, 0.5, 1.0)
    mt["albedo"][0, :3] = LAMP["albedo"]
    mt["albedo"][3, :3] = (1.0, 1.0, 1.0)
    mt["material_type"] = (0, 0, 0, 1)
    sp["center"][:, 3] = 1.0
    sp["center"][0, :3] = (0.0, -LAMP["ground_r"], 0.0)
    sp["radius"][0] = LAMP["ground_r"]
    sp["center"][1, :3] = LAMP["lamp_c"]
    sp["radius"][1] = lamp_r
    sp["material_idx"][:2] = (0, 1)
    k = 2
    if blocker:
        sp["center"][k, :3] = (0.0, 1.0, 0.0)
        sp["radius"][k] = 0.4
        sp["material_idx"][k] = 2
        k += 1
    if mirror:
        sp["center"][k, :3] = (-2.0, 0.7, 0.0)
        sp["radius"][k] = 0.7
        sp["material_idx"][k] = 3
    sp["material_type"] = mt["material_type"][sp["material_idx"]]
    sp, nodes = orc.build_bvh(sp)
    cam, ip, vw = orc.camera((0.0, 6.0, 8.0), (0.0, 0.0, 0.0), 40.0, 0.0, 10.0, 0.1, 100.0, w, h)
    return sp, mt, nodes, cam, ip, vw


def black_env():
    """a 1 x 1 zero environment map: every miss multiplies the throughput by 0"""
    return np.zeros((1, 1, 3), f32)
