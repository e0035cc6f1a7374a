"""numpy restatement of environment next-event estimation (WFPT_FLAG_ENV_NEE, include/wfpt.h "Environment next-event estimation"):
the map's sampling distribution (integer tables), the environment branch of the connect pass, and transport_ref.render with the branch
choice, the two extra draws and the gated miss. float32 in the header's operation order, float64 only in the two selections; sin / cos
are the oracle's own statement of the library's, the lookup is environment_ref's. Shadow rays are traced by a second oracle, as
nee_ref.occluded does, with "any hit" in place of the window."""
import numpy as np

from environment_ref import env_lookup
from nee_ref import Lights, jenkins_hash, occluded, rng_next_float, sincos
from transport_ref import dot3, f32, render

f64, u32, u64 = np.float64, np.uint32, np.uint64
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


def render_with_env_nee(o, shadow, em, light, share=0.5, spp=1, first_frame=1, tx=None, parts=False, never_gate_miss=False, termination=None):
    """nee_ref.render_with_nee with the map as one more light (the loop's `env_connecting`: five draws, the map or an emitter by `share`,
    the gated miss). light: an EnvLight (its map also lights the ungated misses). With a black map the loop connects to the emitters
    alone and the map lights every miss: render_with_nee with that map. never_gate_miss: the mutation that counts the map twice after a
    diffuse bounce."""
    return render(o, shadow=shadow, em=em, tx=tx, lights=Lights(em, tx), env_light=light, share=share, termination=termination, spp=spp,
                  first_frame=first_frame, parts=parts, never_gate_miss=never_gate_miss)


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
