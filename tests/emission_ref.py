"""numpy float32 restatement of emissive materials (WFPT_FLAG_EMISSION, include/wfpt.h "Emission"): a whole render driven through the
oracle's stages with the per-pixel throughput and the second per-sample plane kept here. It is texture_ref.render_with_textures with the
emission pass between the texture factor and shade's albedo; every step is one IEEE f32 operation, so the results are the device's bits."""
import numpy as np

from denoise_ref import luma
from environment_ref import env_lookup, sky

f32 = np.float32
COLOUR = (0.5, 2.0, 0.25)  # power-of-two channels: thr * e and the sums of a few samples are exact


class Emission:
    """What an emitting context holds: colours {material_idx: (r, g, b)}, and the scene's primitives as the device holds them (spheres or
    triangles) and materials. pass_first=True and keep_throughput=True are the two wrong orders the mutation checks of
    tests/test_emission_host.py use (emission before the texture pass; thr left as it was)."""

    def __init__(self, colours, spheres=None, triangles=None, materials=None, pass_first=False, keep_throughput=False):
        self.spheres, self.triangles, self.materials = spheres, triangles, materials
        self.table = np.zeros((len(materials), 3), f32)
        for m, c in dict(colours).items():
            self.table[int(m)] = np.asarray(c, f32)
        self.pass_first, self.keep_throughput = pass_first, keep_throughput

    def prims(self):
        return self.spheres if self.triangles is None else self.triangles

    def colour(self, prim):
        """(e (n, 3), emitter mask (n,)) of hits on primitives prim (n,)."""
        e = self.table[self.prims()["material_idx"][prim].astype(np.int64)]
        return e, (e != 0).any(axis=1)


def render_with_emission(o, em, spp=1, first_frame=1, tx=None, env=None, env_params=None, parts=False):
    """The oracle's per-sample loop (orc_render_sample) driven from Python with its own per-pixel throughput `thr` and `emitted`:
    generate_rays (thr = 1, emitted = 0), then per wavefront extend, the miss_floor exit, and at every hit
      thr <- thr * tex              where tx binds the material (the texture pass),
      emitted <- emitted + thr * e; thr <- +0      where the material emits (the emission pass),
      thr <- thr * albedo           (shade; the oracle's shade supplies the extension rays and the RNG),
    at every miss thr <- thr * sky (or the environment map env). The sample's value is thr + emitted; the values are summed in sample
    order. Returns the accumulated image (n_pixels x 3); with parts=True a dict with it ("acc"), the per-sample planes "image" and "emitted"
    (spp x n_pixels x 3), the luminance moments "s1", "s2" of the values, and per sample the primitive of the primary hit per pixel
    ("first_prim", -1 = a miss)."""
    from oracle import oracle as O
    p = o.params
    gx = (o.width + 7) // 8
    gy = ((o.height + 7) // 8 - p.tile_rank + p.tile_world - 1) // p.tile_world
    prims = em.prims()
    albedo = np.asarray(em.materials["albedo"][:, :3], f32)
    ep = dict(env_params or {})
    acc = np.zeros((o.n_pixels, 3), f32)
    s1, s2 = np.zeros(o.n_pixels, f32), np.zeros(o.n_pixels, f32)
    images, emitteds, firsts = [], [], []
    for k in range(spp):
        o.set_frame(first_frame + k, 0)
        o.reset_image()
        o.set_counters([0, 0, gx * gy * 64])
        o.generate_rays(gx, gy, True)
        thr = o.image().copy()
        emitted = np.zeros_like(thr)
        first = np.full(o.n_pixels, -1, np.int64)
        ex, ey = O.workgroup_size_64(gx * gy * 64)
        for b in range(p.max_wavefronts):
            n_rays = int(o.counters()[2])
            o.extend(ex, ey)
            c = o.counters()
            n_miss, n_hit = int(c[0]), int(c[1])
            rays = o.rays(max(n_rays, 1))
            hits = o.hits(n_hit)
            ridx = hits["ray_idx"].astype(np.int64)
            hp = rays["pixel_idx"][ridx].astype(np.int64)
            prim = hits["sphere_idx"].astype(np.int64)
            if b == 0:
                first[hp] = prim
            if n_miss < p.miss_floor:
                break
            t = thr[hp]
            e, emits = em.colour(prim)

            def emission_pass(t):
                emitted[hp[emits]] = emitted[hp[emits]] + t[emits] * e[emits]
                return t if em.keep_throughput else np.where(emits[:, None], f32(0), t)

            if em.pass_first:
                t = emission_pass(t)
            if tx is not None:
                org, d = rays["origin"][ridx, :3].astype(f32), rays["direction"][ridx, :3].astype(f32)
                tex, bound = tx.factor(prim, org + hits["t"].astype(f32)[:, None] * d)  # sh:91, per component o + t d
                t = np.where(bound[:, None], t * tex, t)
            if not em.pass_first:
                t = emission_pass(t)
            thr[hp] = t * albedo[prims["material_idx"][prim].astype(np.int64)]
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
            firsts.append(first)
    if not parts:
        return acc
    return {"acc": acc, "image": np.stack(images), "emitted": np.stack(emitteds), "s1": s1, "s2": s2, "first_prim": np.stack(firsts)}


def furnace_inputs(orc, w, h):
    """closed_room_inputs("centre") with the two small spheres moved behind the camera: the camera at the centre of one closed sphere of
    radius 5 (material 0), looking down -z, so that every primary ray meets that sphere first."""
    sp = np.zeros(3, orc.SPHERE)
    mt = np.zeros(3, orc.MATERIAL)
    mt["albedo"][:] = (0.9, 0.8, 0.7, 1.0)
    mt["material_type"] = (1, 0, 2)
    mt["refract_index"][2] = 1.5
    sp["center"][:, 3] = 1.0
    sp["radius"] = (5.0, 0.5, 0.25)
    sp["center"][1, :3] = (1.5, 0.0, 3.0)
    sp["center"][2, :3] = (-1.5, 0.5, 3.0)
    sp["material_idx"] = (0, 1, 2)
    sp["material_type"] = mt["material_type"]
    sp, nodes = orc.build_bvh(sp)
    cam, ip, vw = orc.camera((0.0, 0.0, 0.0), (0.5, 0.0, -1.0), 70.0, 0.0, 10.0, 0.1, 100.0, w, h)
    return sp, mt, nodes, cam, ip, vw
