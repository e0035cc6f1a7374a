"""numpy restatement of environment next-event estimation (WFPT_FLAG_ENV_NEE, include/wfpt.h "Environment next-event estimation"):
the map's sampling distribution (integer tables), the environment branch of the connect pass, and nee_ref.render_with_nee's loop with
the branch choice, the two extra draws and the gated miss. float32 in the header's operation order, float64 only in the two selections;
sin / cos are the oracle's own statement of the library's, the lookup is environment_ref's. Shadow rays are traced by a second oracle,
as nee_ref.occluded does, with "any hit" in place of the window."""
import numpy as np

from denoise_ref import luma
from environment_ref import env_lookup, normalize3
from nee_ref import Lights, connect_draws, dot3, jenkins_hash, occluded, rng_next_float, sincos

f32, f64, u32, u64 = np.float32, np.float64, np.uint32, np.uint64
PI = f32(3.1415927)
TWO_PI_SQ = f32(19.739209)


# ---------------------------------------------------------------- the sampling distribution
def weights(env):
    """(k (h, w) int64, M) of the map env (h, w, 3): the integer texel weights, or (None, M) for a black map."""
    env = np.asarray(env, f32)
    h, w = env.shape[:2]
    L = (f32(0.2126) * env[..., 0] + f32(0.7152) * env[..., 1]) + f32(0.0722) * env[..., 2]
    rows = [np.clip(np.arange(h) + d, 0, h - 1) for d in (-1, 0, 1)]
    cols = [(np.arange(w) + d) % w for d in (-1, 0, 1)]
    Lm = np.max([L[r][:, c] for r in rows for c in cols], axis=0).astype(f32)
    sy, _ = sincos(PI * ((np.arange(h).astype(f32) + f32(0.5)) / f32(h)))
    f = Lm * sy[:, None]
    M = f32(f.max())
    if not (M > 0 and np.isfinite(M)):
        return None, M
    k = np.ceil((f / M) * f32(65535.0)).astype(np.int64)
    k[(f > 0) & (k == 0)] = 1  # a quotient that underflows
    return k, M


class Distribution:
    """row (h, w) uint32, marg (h,) uint64 and total of a map; None-like (ok = False) for a black one."""

    def __init__(self, env):
        self.h, self.w = np.asarray(env).shape[:2]
        self.k, self.M = weights(env)
        self.ok = self.k is not None
        if self.ok:
            self.row = np.cumsum(self.k, axis=1).astype(u32)
            self.marg = np.cumsum(self.row[:, -1].astype(u64)).astype(u64)
            self.total = int(self.marg[-1])

    def select(self, u1, u2):
        """(y, x, k) for draws u1, u2 (float32 arrays): the two searches, float64 products, clamped into the tables."""
        u1, u2 = np.asarray(u1, f32), np.asarray(u2, f32)
        with np.errstate(invalid="ignore"):
            tr = np.floor(u1.astype(f64) * f64(self.total))
            T = np.where(tr >= 0, np.where(tr < f64(self.total), tr, f64(self.total - 1)), 0.0)
            T = np.where(np.isnan(tr), 0.0, T).astype(u64)
            y = np.searchsorted(self.marg, T, side="right")  # the first row with marg[y] > T
            R = self.row[y, -1].astype(np.int64)
            tc = np.floor(u2.astype(f64) * R.astype(f64))
            Cc = np.where(tc >= 0, np.where(tc < R, tc, R - 1), 0.0)
            Cc = np.where(np.isnan(tc), 0.0, Cc).astype(np.int64)
        x = np.array([np.searchsorted(self.row[yy], cc, side="right") for yy, cc in zip(y, Cc)], np.int64).reshape(y.shape)
        k = self.row[y, x].astype(np.int64) - np.where(x > 0, self.row[y, np.maximum(x - 1, 0)].astype(np.int64), 0)
        return y.astype(np.int64), x, k


class EnvLight:
    """The map as a light: env (h, w, 3), its parameters and its distribution. drop_st / drop_p: the two mutations of
    tests/test_env_nee_host.py (the pdf without its sine; Genv without the division by the share)."""

    def __init__(self, env, intensity=1.0, rotation=0.0, drop_st=False, drop_p=False):
        self.env, self.intensity, self.rotation = np.asarray(env, f32), intensity, rotation
        self.dist = Distribution(env)
        self.drop_st, self.drop_p = drop_st, drop_p

    def sample(self, n, u1, u2, u3, u4, share):
        """The environment branch for receivers with normals n (k, 3): a dict of w (k, 3), texel (k,), e (k, 3), G (k,) and `lit`."""
        d = self.dist
        n = np.asarray(n, f32).reshape(-1, 3)
        u3, u4 = np.asarray(u3, f32), np.asarray(u4, f32)
        y, x, k = d.select(u1, u2)
        fw, fh = f32(d.w), f32(d.h)
        with np.errstate(all="ignore"):
            u = (x.astype(f32) + u3) / fw
            v = (y.astype(f32) + u4) / fh
            theta = PI * v
            phi = (f32(2) * PI) * ((u - f32(0.5)) - f32(self.rotation))
            st, ct = sincos(theta)
            sp, cp = sincos(phi)
            wdir = np.stack([st * sp, ct, -(st * cp)], 1).astype(f32)
            P = k.astype(f32) / u64(d.total).astype(f32)
            pdf = ((P * fw) * fh) / (TWO_PI_SQ * st) if not self.drop_st else ((P * fw) * fh) / TWO_PI_SQ
            cos_s = dot3(n, wdir)
            e = env_lookup(self.env, wdir, self.intensity, self.rotation)
            G = (cos_s / PI) / (pdf * f32(share)) if not self.drop_p else (cos_s / PI) / pdf
            lit = (st > 0) & (cos_s > 0) & (pdf > 0)
        return {"w": wdir, "texel": y * d.w + x, "e": e.astype(f32), "G": G.astype(f32), "lit": lit, "st": st, "pdf": pdf}


def any_hit(shadow, p, w):
    """The oracle's verdict for the shadow rays (p, w) without a far end: its walk reports a hit. (nee_ref.occluded with an infinite
    length: t < inf * 0.999 holds for every hit.)"""
    return occluded(shadow, p, w, np.full(len(p), np.inf, f32))


def connect_draws5(pixel_idx, frame, b):
    """u0 .. u4 of the connect pass: nee_ref.connect_draws' stream, two draws further (only the environment branch uses them)."""
    s = jenkins_hash(np.asarray(pixel_idx, u32) ^ jenkins_hash(u32(frame)))
    s = jenkins_hash(s ^ u32((0x9E3779B9 * (b + 1)) & 0xFFFFFFFF))
    out = []
    for _ in range(5):
        u, s = rng_next_float(s)
        out.append(u)
    return out


def render_with_env_nee(o, shadow, em, light, share=0.5, spp=1, first_frame=1, tx=None, parts=False, never_gate_miss=False):
    """nee_ref.render_with_nee with the map as one more light. light: an EnvLight (its map also lights the ungated misses). With a black
    map it is render_with_nee itself. never_gate_miss: the mutation that counts the map twice after a diffuse bounce."""
    from nee_ref import render_with_nee
    from oracle import oracle as O
    if not light.dist.ok:
        return render_with_nee(o, shadow, em, spp=spp, first_frame=first_frame, tx=tx, env=light.env,
                               env_params={"intensity": light.intensity, "rotation": light.rotation}, parts=parts)
    P = o.params
    assert P.tile_world == 1, "the restatement keys the connect stream by the oracle's pixel index: whole frames only"
    lights = Lights(em, tx)
    p_eff = f32(share) if lights.n else f32(1)
    gx = (o.width + 7) // 8
    gy = (o.height + 7) // 8
    prims = em.prims()
    albedo = np.asarray(em.materials["albedo"][:, :3], f32)
    acc = np.zeros((o.n_pixels, 3), f32)
    s1, s2 = np.zeros(o.n_pixels, f32), np.zeros(o.n_pixels, f32)
    images, emitteds, values = [], [], []
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
            pt = org + hits["t"].astype(f32)[:, None] * d
            if tx is not None:
                tex, bound = tx.factor(prim, pt)
                t = np.where(bound[:, None], t * tex, t)
            add = emits & ~flag[hp]  # the emission pass, gated by the flag the step before left
            emitted[hp[add]] = emitted[hp[add]] + t[add] * e[add]
            t = np.where(emits[:, None], f32(0), t)
            alb = albedo[prims["material_idx"][prim].astype(np.int64)]
            # the connect pass
            mclass = prims["material_type"][prim].astype(np.int64)
            diffuse = ((mclass == 0) | (mclass > 2)) & ~emits
            flag[hp[~diffuse]] = False
            flag[hp[diffuse]] = True
            dp, dpix = pt[diffuse], hp[diffuse]
            if em.triangles is None:
                nrm = np.stack(normalize3(*[dp[:, a] - em.spheres["center"][prim[diffuse], a] for a in range(3)]), 1).astype(f32)
            else:
                tr = em.triangles[prim[diffuse]]
                a_, b_ = tr["e1"], tr["e2"]
                nrm = np.stack(normalize3(a_[:, 1] * b_[:, 2] - a_[:, 2] * b_[:, 1], a_[:, 2] * b_[:, 0] - a_[:, 0] * b_[:, 2],
                                          a_[:, 0] * b_[:, 1] - a_[:, 1] * b_[:, 0]), 1).astype(f32)
            u0, u1, u2, u3, u4 = connect_draws5(dpix, frame, b)
            to_env = np.ones(len(dp), bool) if not p_eff < 1 else u0 < p_eff
            with np.errstate(all="ignore"):
                base = t[diffuse] * alb[diffuse]
                # the environment branch
                ie = np.flatnonzero(to_env)
                s = light.sample(nrm[ie], u1[ie], u2[ie], u3[ie], u4[ie], p_eff)
                occ = np.zeros(len(ie), bool)
                occ[s["lit"]] = any_hit(shadow, dp[ie][s["lit"]], s["w"][s["lit"]])
                ok = s["lit"] & ~occ
                contrib = (base[ie] * s["e"]) * s["G"][:, None]
                emitted[dpix[ie][ok]] = emitted[dpix[ie][ok]] + contrib[ok]
                # the emitter branch
                il = np.flatnonzero(~to_env)
                if len(il):
                    q = f32(1) - p_eff
                    sl = lights.sample(dp[il], nrm[il], (u0[il] - p_eff) / q, u1[il], u2[il])
                    occ = np.zeros(len(il), bool)
                    occ[sl["lit"]] = occluded(shadow, dp[il][sl["lit"]], sl["w"][sl["lit"]], sl["dist"][sl["lit"]])
                    ok = sl["lit"] & ~occ
                    contrib = ((base[il] * sl["e_q"]) * sl["G"][:, None]) / q
                    emitted[dpix[il][ok]] = emitted[dpix[il][ok]] + contrib[ok]
            thr[hp] = t * alb
            midx = o.misses(n_miss).astype(np.int64)
            mp = rays["pixel_idx"][midx].astype(np.int64)
            md = rays["direction"][midx, :3].astype(f32)
            factor = env_lookup(light.env, md, light.intensity, light.rotation)
            if not never_gate_miss:  # the map is already counted where the pixel's connected flag is set
                factor = np.where(flag[mp][:, None], f32(0), factor)
            thr[mp] = thr[mp] * factor
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
            values.append(value)
    if not parts:
        return acc
    return {"acc": acc, "image": np.stack(images), "emitted": np.stack(emitteds), "value": np.stack(values), "s1": s1, "s2": s2}


# ---------------------------------------------------------------- scenes and maps
GROUND = {"r": 1000.0, "albedo": (0.5, 0.75, 0.25)}


def ground_inputs(orc, w, h, occluder=False, mirror=False, lamp=False, look_at=(0.0, 0.0, 0.0)):
    """One Lambertian sphere of radius 1000 as ground (material 0): it is convex, so every scattered ray misses -- one bounce, no
    interreflection. occluder: a Lambertian sphere (material 2) standing on it; mirror: a fuzz-0 metal sphere (material 3); lamp: a small
    sphere (material 1, to be given an emission colour) above the ground. The camera looks down at the ground at an angle (look_at
    (0, 3.5, 0) brings the horizon into the frame)."""
    n = 1 + int(occluder) + int(mirror) + int(lamp)
    sp = np.zeros(n, orc.SPHERE)
    mt = np.zeros(4, orc.MATERIAL)
    mt["albedo"][:] = (0.5, 0.5, 0.5, 1.0)
    mt["albedo"][0, :3] = GROUND["albedo"]
    mt["albedo"][3, :3] = (1.0, 1.0, 1.0)
    mt["material_type"] = (0, 0, 0, 1)
    sp["center"][:, 3] = 1.0
    sp["center"][0, :3] = (0.0, -GROUND["r"], 0.0)
    sp["radius"][0] = GROUND["r"]
    k = 1
    if lamp:
        sp["center"][k, :3] = (0.0, 2.0, 0.0)
        sp["radius"][k] = 0.25
        sp["material_idx"][k] = 1
        k += 1
    if occluder:
        sp["center"][k, :3] = (0.8, 0.5, 0.0)
        sp["radius"][k] = 0.5
        sp["material_idx"][k] = 2
        k += 1
    if mirror:
        sp["center"][k, :3] = (-1.5, 0.7, 0.0)
        sp["radius"][k] = 0.7
        sp["material_idx"][k] = 3
    sp["material_type"] = mt["material_type"][sp["material_idx"]]
    sp, nodes = orc.build_bvh(sp)
    cam, ip, vw = orc.camera((0.0, 6.0, 8.0), look_at, 40.0, 0.0, 10.0, 0.1, 100.0, w, h)
    return sp, mt, nodes, cam, ip, vw


def block_map(w=32, h=16, value=(40.0, 30.0, 20.0)):
    """Black but for a 2 x 2 block of texels at about 45 degrees elevation (rows h/4 - 1 and h/4), facing +x (columns 3w/4 - 1, 3w/4)."""
    env = np.zeros((h, w, 3), f32)
    env[h // 4 - 1:h // 4 + 1, 3 * w // 4 - 1:3 * w // 4 + 1] = value
    return env


def sun_map(w=16, h=8, seed=3):
    """A dim random sky with one texel 200 times brighter."""
    env = (np.random.default_rng(seed).random((h, w, 3)) * 0.2).astype(f32)
    env[h // 4, w // 3] = (60.0, 50.0, 40.0)
    return env


def irradiance(env, normal, intensity=1.0, rotation=0.0, n_theta=1024, n_phi=2048):
    """(3,) float64: the integral of env_lookup(w) cos / pi over the hemisphere about `normal`, by midpoint quadrature over the sphere
    of the restatement's own lookup."""
    th = (np.arange(n_theta) + 0.5) * np.pi / n_theta
    ph = (np.arange(n_phi) + 0.5) * 2 * np.pi / n_phi
    T, Ph = np.meshgrid(th, ph, indexing="ij")
    d = np.stack([np.sin(T) * np.cos(Ph), np.cos(T), np.sin(T) * np.sin(Ph)], -1).reshape(-1, 3)
    cos = np.clip(d @ np.asarray(normal, f64), 0.0, None)
    val = env_lookup(env, d.astype(f32), intensity, rotation).astype(f64)
    dw = (np.sin(T) * (np.pi / n_theta) * (2 * np.pi / n_phi)).reshape(-1)
    return (val * (cos * dw / np.pi)[:, None]).sum(axis=0)
