"""numpy float32 restatement of next-event estimation (WFPT_FLAG_NEE, include/wfpt.h "Next-event estimation"): the connect pass's random
stream, the light list with its sampler, densities and weights, and the occlusion test; transport_ref.render runs them with the per-pixel
connected flag, the gated emission add, and the connect pass between the emission pass and shade's albedo. Every step is one IEEE f32
operation in the header's order (sin / cos are the oracle's own statement of the library's), so the results are the device's bits.
Occlusion comes from the oracle itself: a second Oracle over the same scene traces the shadow rays (write_rays, extend) and its closest t
is compared with dist * 0.999 -- no traversal is rewritten here."""
import ctypes as C

import numpy as np

from transport_ref import dot3, f32, render, triangle_normal_area

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
            else:
                t = em.triangles[prim]
                v0, e1, e2 = t["v0"].astype(f32), t["e1"].astype(f32), t["e2"].astype(f32)
                su = np.sqrt(u1)
                b1, b2 = f32(1) - su, u2 * su
                q = (v0 + b1[:, None] * e1) + b2[:, None] * e2
            nl, area = self.normal_area(prim, q)
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

    def normal_area(self, prim, q):
        """(nl (k, 3), A (k,)) of the lights prim (k,) at their points q (k, 3), by the operations sample() uses: the same bits."""
        em = self.em
        with np.errstate(all="ignore"):
            if em.triangles is not None:
                return triangle_normal_area(em.triangles[prim])
            sp = em.spheres[prim]
            ra = np.abs(sp["radius"].astype(f32))
            return (q - sp["center"][:, :3].astype(f32)) / ra[:, None], (f32(4) * PI) * (ra * ra)

    def densities(self, p, s, nf=None):
        """(pl, pb, wl) of connect samples s = self.sample(p, n, ...) with s["n"] = n -- step 5 of "Multiple importance sampling". cos_s,
        cos_l, A and dist2 are recomputed (sample() does not return them). nf: the light count per sample, where it is not self.n."""
        nf = f32(self.n) if nf is None else nf
        with np.errstate(all="ignore"):
            nl, area = self.normal_area(s["prim"], s["q"])
            v = s["q"] - np.asarray(p, f32)
            dist2 = dot3(v, v)
            cos_s, cos_l = dot3(np.asarray(s["n"], f32), s["w"]), np.abs(dot3(nl, s["w"]))
            pb = cos_s / PI
            pl = dist2 / ((cos_l * area) * nf)
            wl = pl / (pl + pb)
        return pl.astype(f32), pb.astype(f32), wl.astype(f32)

    def hit_weight(self, o, ph, d, prim, pb_of_len=None, with_nf=True, nf=None):
        """The emission pass's weight for hits at ph on emitter `prim` (k,) of rays that left o with direction d (not normalised): a dict of
        pl, pb, wb, cos_l (k,), the header's operation order. pb_of_len / with_nf: the mutations of tests/test_mis_host.py. nf: the light
        count per hit, where it is not self.n."""
        o, ph, d = np.asarray(o, f32), np.asarray(ph, f32), np.asarray(d, f32)
        prim = np.asarray(prim, np.int64)
        nf = f32(1) if not with_nf else f32(self.n) if nf is None else nf
        with np.errstate(all="ignore"):
            v = ph - o
            dist2 = dot3(v, v)
            dist = np.sqrt(dist2)
            w = v / dist[:, None]
            nl, area = self.normal_area(prim, ph)
            cos_l = np.abs(dot3(nl, w))
            ln = np.sqrt(dot3(d, d))
            pb = ((f32(0.5) * ln) / PI) if pb_of_len is None else pb_of_len(ln)
            ok = (area > 0) & (dist2 > 0) & (cos_l > 0)
            pl = np.where(ok, dist2 / ((cos_l * area) * nf), f32(0)).astype(f32)
            wb = np.where(ok, pb / (pb + pl), f32(1)).astype(f32)
        return {"pl": pl, "pb": pb.astype(f32), "wb": wb, "cos_l": cos_l.astype(f32)}


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
                    never_clear_flag=False, termination=None):
    """transport_ref.render with the connect pass to the emitters (three draws) and the gated emission pass. o: the Oracle that renders;
    shadow: a second Oracle over the same scene (any viewport with at least as many ray slots) that traces the shadow rays. With no light
    the loop selects no connect pass and the emission pass `all`: emission_ref.render_with_emission.
    never_set_flag / never_clear_flag: the two mutations of tests/test_nee_host.py (a diffuse hit leaves the flag 0: lights found after a
    diffuse bounce are counted twice; a non-diffuse hit leaves the flag as it was: a lamp seen in a mirror after a diffuse hit goes black)."""
    return render(o, shadow=shadow, em=em, tx=tx, env=env, env_params=env_params, lights=Lights(em, tx), termination=termination, spp=spp,
                  first_frame=first_frame, parts=parts, never_set_flag=never_set_flag, never_clear_flag=never_clear_flag)


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
