"""The one wavefront loop of the light-transport restatements (textures, emission, NEE, MIS, their environment forms, light selection by
power, path termination): `render` drives the oracle's stages and keeps the throughput, the second plane, the connected flag and the
`origin` plane in numpy float32. Its passes are chosen once, before the loop, as the host chooses its launches in wfpt_api.hip
(enqueue_pre_shade, launch_emission_pass, launch_connect_pass, launch_miss_pass), and carry the same names: textured, emitting, connecting,
env_connecting, weighing, env_weighing; the emission kinds all / gated / weighed / weighed_env / weighed_power; the miss kinds sky / map /
gated / weighed. Every step is one IEEE f32 operation in the header's order, so the results are the device's bits. The feature modules
(environment_ref ... retire_ref) hold the pieces -- lookups, samplers, densities, weights, scenes -- and a few-line render_with_* each;
they take the primitives below from here, so `render` imports them when it is called."""
import numpy as np

from denoise_ref import luma

f32 = np.float32
INACTIVE_PIXEL = 0xFFFFFFFF
# the mutation checks of the host tests: every keyword render() accepts beyond its own, with the value that means "as the header says"
MUTATIONS = {"never_set_flag": False, "never_clear_flag": False, "no_wl": False, "no_wb": False, "no_nf": False, "pb_of_len": None,
             "never_gate_miss": False, "full_weight": False, "miss_pb_of_len": None, "miss_pe_without_p": False,
             "emission_plq_without_q": False}


# ---------------------------------------------------------------- primitives the restatements share
def normalize3(x, y, z):
    x, y, z = (np.asarray(v, f32) for v in (x, y, z))
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = f32(1.0) / np.sqrt((x * x + y * y) + z * z)
    return x * inv, y * inv, z * inv


def dot3(a, b):
    """of rows: a, b (k, 3)"""
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def dot3_components(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def is_diffuse(mclass):
    """the material classes whose hits the connect pass serves: Lambertian and every unknown class (shade treats those as Lambertian)"""
    return (mclass == 0) | (mclass > 2)


def prims_of(scene):
    """the primitives of an Emission or a Textures, as the device holds them"""
    return scene.spheres if scene.triangles is None else scene.triangles


def triangle_normal_area(t):
    e1, e2 = t["e1"].astype(f32), t["e2"].astype(f32)
    cr = [e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]]
    with np.errstate(all="ignore"):
        nl = np.stack(normalize3(*cr), 1).astype(f32)
        area = f32(0.5) * np.sqrt((cr[0] * cr[0] + cr[1] * cr[1]) + cr[2] * cr[2])
    return nl, area


def hit_normal(scene, prim, p):
    """The geometric normal of hits at p (k, 3) on primitives prim (k,): (p - c) normalised, or the triangle's."""
    if scene.triangles is None:
        return np.stack(normalize3(*[p[:, a] - scene.spheres["center"][prim, a] for a in range(3)]), 1).astype(f32)
    return triangle_normal_area(scene.triangles[prim])[0]


class BounceTables:
    """An Oracle (or a wrapper around one) that keeps, per sample, the rows (rays_in, hits, misses, shaded) wfpt_read_bounce_table gives."""

    def __init__(self, o):
        self.o = o
        self.tables = []

    def __getattr__(self, name):
        return getattr(self.o, name)

    def generate_rays(self, gx, gy, true_size=False):
        self.o.generate_rays(gx, gy, true_size)
        self.tables.append([])

    def extend(self, gx, gy):
        rays_in = int(self.o.counters()[2])
        self.o.extend(gx, gy)
        c = self.o.counters()
        self.tables[-1].append([rays_in, int(c[1]), int(c[0]), 0])

    def shade(self, gx, gy):
        self.tables[-1][-1][3] = 1
        self.o.shade(gx, gy)

    def bounce_table(self):
        """of the last sample"""
        return np.array(self.tables[-1], "<u4").reshape(-1, 4)


# ---------------------------------------------------------------- the loop
class _Sample:
    """what a sample keeps per pixel: thr, emitted, the connected flag, the `origin` plane"""

    def __init__(self, thr):
        self.thr, self.emitted = thr, np.zeros_like(thr)
        self.flag = np.zeros(len(thr), bool)
        self.origin = np.zeros((len(thr), 3), f32)


class _Wave:
    """what the passes of one wavefront read: b, frame, and per hit hp (pixel), prim, org, d, pt (o + t d), e, emits, alb"""


def render(o, *, shadow=None, em=None, tx=None, env=None, env_params=None, lights=None, env_light=None, share=0.5, weigh=False,
           termination=None, spp=1, first_frame=1, parts=False, aov=False, scatters=None, **mutations):
    """The oracle's per-sample loop (orc_render_sample) driven from Python with its own per-pixel throughput `thr` and `emitted`:
    generate_rays (thr = 1, emitted = 0), then per wavefront extend, the miss_floor exit, and at every hit, in the host's order,
      thr <- thr * tex                              where tx binds the material (the texture pass),
      emitted <- emitted + thr * e; thr <- +0       where em's material emits (the emission pass of the context's kind),
      emitted <- emitted + a light sample           at diffuse hits (the connect pass, which also sets the connected flag),
      thr <- thr * albedo                           (shade; the oracle's shade supplies the extension rays and the RNG),
    at every miss thr <- thr * the miss pass's factor, then the termination step on the hits' thr, shade, swap. The sample's value is
    thr + emitted; the values are summed in sample order.

    o: the Oracle that renders (or a wrapper: adaptive_ref.Masked, adaptive_ref.Local, retire_ref.Retiring). shadow: a second Oracle over
    the same scene that traces the shadow rays. em: an emission_ref.Emission; tx: a texture_ref.Textures; with neither, shade's albedo is
    read back from the oracle's own image. env, env_params: the map that lights the misses (None: the gradient sky). lights: a
    nee_ref.Lights (or light_power_ref.PowerLights); env_light: an env_nee_ref.EnvLight, whose map then lights the misses, with its share
    of the connect samples; weigh: the MIS flag of the context (WFPT_FLAG_MIS without a map, WFPT_FLAG_ENV_MIS with one). termination: a
    retire_ref.Retiring. scatters: a list that receives, per wavefront, (normal, direction) of every extension ray a diffuse hit produced.
    mutations: MUTATIONS' keywords.

    Returns the accumulated image (n_pixels x 3); with aov=True also the sum of the primary hits' tex * albedo (the miss factor of a primary
    miss); with parts=True a dict instead: "acc", the per-sample planes "image", "emitted" and "value" (spp x n_pixels x 3), the luminance
    moments "s1", "s2" of the values, per sample the primitive of the primary hit per pixel ("first_prim", -1 = a miss), and "stats"
    (counts of weighed hits and misses and of the connect samples that contributed)."""
    import env_mis_ref as X
    import env_nee_ref as V
    import nee_ref as N
    from environment_ref import env_lookup, sky
    from oracle import oracle as O
    unknown = set(mutations) - set(MUTATIONS)
    if unknown:
        raise TypeError(f"render() got unexpected keywords {sorted(unknown)}")
    mut = dict(MUTATIONS, **mutations)
    P = o.params
    scene = em if em is not None else tx
    if scene is not None:
        prims = prims_of(scene)
        albedo = np.asarray(scene.materials["albedo"][:, :3], f32)

    # ---- the context's kind, in the host's words
    textured, emitting = tx is not None, em is not None
    connecting = lights is not None and lights.n > 0  # to emitters
    env_connecting = env_light is not None and env_light.dist.ok  # to the map
    weighing = bool(weigh) and env_light is None and connecting
    env_weighing = bool(weigh) and env_connecting
    if env_light is not None:
        env, env_params = env_light.env, {"intensity": env_light.intensity, "rotation": env_light.rotation}
    ep = dict(env_params or {})
    p_eff = f32(share) if connecting else f32(1)  # the map's share of the connect samples
    q = f32(1) - p_eff
    assert not (connecting or env_connecting) or (emitting and shadow is not None)
    assert not (connecting or env_connecting or termination is not None) or P.tile_world == 1, \
        "the connect and termination streams are keyed by the oracle's pixel index: whole frames only"
    assert termination is None or scene is not None
    assert termination is not None or not hasattr(o, "retire"), "o is (or wraps) a Retiring that was not passed as termination="
    assert not aov or textured
    stats = {"weighed_misses": 0, "weighed_hits": 0, "env_samples": 0, "light_samples": 0}

    # ---- the texture pass
    def texture_pass(s, w, t):
        tex, bound = tx.factor(w.prim, w.pt)
        return np.where(bound[:, None], t * tex, t)

    # ---- the emission pass: thr * e where the pixel's connected flag is 0; where it is 1 nothing (gated) or (thr * e) * wb (weighed*)
    if not (connecting or env_connecting):
        emission_kind, wb_of = "all", None
    elif env_weighing:
        emission_kind = "weighed_env"  # pl * q in pl's place

        def wb_of(w, sel, origin):
            if mut["full_weight"]:
                return np.ones(int(sel.sum()), f32)
            return X.hit_weight_q(lights, origin, w.pt[sel], w.d[sel], w.prim[sel], f32(1) if mut["emission_plq_without_q"] else q)
    elif weighing:
        emission_kind = "weighed_power" if getattr(lights, "has_distribution", False) else "weighed"  # the lights' own nf or nfi

        def wb_of(w, sel, origin):
            if mut["no_wb"]:
                return np.ones(int(sel.sum()), f32)
            return lights.hit_weight(origin, w.pt[sel], w.d[sel], w.prim[sel], pb_of_len=mut["pb_of_len"], with_nf=not mut["no_nf"])["wb"]
    else:
        emission_kind, wb_of = "gated", None

    def emission_pass(s, w, t):
        flagged = np.zeros(len(w.hp), bool) if emission_kind == "all" else s.flag[w.hp]
        plain = w.emits & ~flagged
        s.emitted[w.hp[plain]] = s.emitted[w.hp[plain]] + t[plain] * w.e[plain]
        wgt = w.emits & flagged
        if wb_of is not None and wgt.any():
            assert np.array_equal(s.origin[w.hp[wgt]].view(np.uint32), w.org[wgt].view(np.uint32)), "origin is not the ray's origin"
            wb = wb_of(w, wgt, s.origin[w.hp[wgt]])
            s.emitted[w.hp[wgt]] = s.emitted[w.hp[wgt]] + (t[wgt] * w.e[wgt]) * wb[:, None]
            stats["weighed_hits"] += int(wgt.sum())
        return t if em.keep_throughput else np.where(w.emits[:, None], f32(0), t)

    # ---- the connect pass: the flag, the `origin` plane, and one light sample per diffuse hit
    def connect_emitters(s, w, base, dp, dpix, nrm):
        """three draws; ((t * alb) * e_q) * G, weighed by wl"""
        u0, u1, u2 = N.connect_draws(dpix, w.frame, w.b)
        sl = lights.sample(dp, nrm, u0, u1, u2)
        sl["n"] = nrm
        lit = sl["lit"]
        occ = np.zeros(len(dp), bool)
        occ[lit] = N.occluded(shadow, dp[lit], sl["w"][lit], sl["dist"][lit])
        ok = lit & ~occ
        with np.errstate(all="ignore"):
            contrib = (base * sl["e_q"]) * sl["G"][:, None]
            if weighing and not mut["no_wl"]:
                contrib = contrib * lights.densities(dp, sl)[2][:, None]
        s.emitted[dpix[ok]] = s.emitted[dpix[ok]] + contrib[ok]
        stats["light_samples"] += int(ok.sum())

    def connect_map_or_emitter(s, w, base, dp, dpix, nrm):
        """five draws; the map where u0 < its share ((t * alb) * e) * Genv weighed by we, any hit occludes; an emitter otherwise, with
        (u0 - p) / q as its u0, / q, weighed by plq / (plq + pb)"""
        u0, u1, u2, u3, u4 = V.connect_draws5(dpix, w.frame, w.b)
        to_env = np.ones(len(dp), bool) if not p_eff < 1 else u0 < p_eff
        weighed = env_weighing and not mut["full_weight"]
        with np.errstate(all="ignore"):
            ie = np.flatnonzero(to_env)
            se = env_light.sample(nrm[ie], u1[ie], u2[ie], u3[ie], u4[ie], p_eff)
            occ = np.zeros(len(ie), bool)
            occ[se["lit"]] = V.any_hit(shadow, dp[ie][se["lit"]], se["w"][se["lit"]])
            ok = se["lit"] & ~occ
            contrib = (base[ie] * se["e"]) * se["G"][:, None]
            if weighed:
                contrib = contrib * X.env_densities(se, nrm[ie], p_eff)[2][:, None]
            s.emitted[dpix[ie][ok]] = s.emitted[dpix[ie][ok]] + contrib[ok]
            stats["env_samples"] += int(ok.sum())
            il = np.flatnonzero(~to_env)
            if len(il):
                sl = lights.sample(dp[il], nrm[il], (u0[il] - p_eff) / q, u1[il], u2[il])
                sl["n"] = nrm[il]
                occ = np.zeros(len(il), bool)
                occ[sl["lit"]] = N.occluded(shadow, dp[il][sl["lit"]], sl["w"][sl["lit"]], sl["dist"][sl["lit"]])
                ok = sl["lit"] & ~occ
                contrib = ((base[il] * sl["e_q"]) * sl["G"][:, None]) / q
                if weighed:
                    pl, pb, _ = lights.densities(dp[il], sl)
                    plq = pl * q
                    contrib = contrib * (plq / (plq + pb))[:, None]
                s.emitted[dpix[il][ok]] = s.emitted[dpix[il][ok]] + contrib[ok]
                stats["light_samples"] += int(ok.sum())

    connect_sample = connect_map_or_emitter if env_connecting else connect_emitters if connecting else None

    def connect_pass(s, w, t):
        diffuse = is_diffuse(prims["material_type"][w.prim].astype(np.int64)) & ~w.emits
        if not mut["never_clear_flag"]:
            s.flag[w.hp[~diffuse]] = False
        if not mut["never_set_flag"]:
            s.flag[w.hp[diffuse]] = True
        dp, dpix = w.pt[diffuse], w.hp[diffuse]
        if weighing or env_weighing:
            s.origin[dpix] = dp
        nrm = hit_normal(em, w.prim[diffuse], dp)
        with np.errstate(all="ignore"):
            base = t[diffuse] * w.alb[diffuse]
        connect_sample(s, w, base, dp, dpix, nrm)
        return dpix, nrm

    # ---- the miss pass: the gradient sky or the map; the map gated by the connected flag; or weighed where the flag is set
    def miss_colour(md):
        return sky(md) if env is None else env_lookup(env, md, ep.get("intensity", 1.0), ep.get("rotation", 0.0))

    def miss_plain(s, mp, md):  # kinds "sky" and "map"
        s.thr[mp] = s.thr[mp] * miss_colour(md)

    def miss_gated(s, mp, md):  # the map is already counted where the pixel's connected flag is set
        factor = miss_colour(md)
        if not mut["never_gate_miss"]:
            factor = np.where(s.flag[mp][:, None], f32(0), factor)
        s.thr[mp] = s.thr[mp] * factor

    def miss_weighed(s, mp, md):
        factor = s.thr[mp] * miss_colour(md)
        g = s.flag[mp]
        if g.any() and not mut["full_weight"]:
            wb = X.miss_weight(env_light, md[g], p_eff, pb_of_len=mut["miss_pb_of_len"], with_p=not mut["miss_pe_without_p"])["wb"]
            factor[g] = factor[g] * wb[:, None]
        stats["weighed_misses"] += int(g.sum())
        s.thr[mp] = factor

    miss_pass = miss_weighed if env_weighing else miss_gated if env_connecting else miss_plain

    # ---- the samples
    gx = (o.width + 7) // 8
    gy = ((o.height + 7) // 8 - P.tile_rank + P.tile_world - 1) // P.tile_world
    acc = np.zeros((o.n_pixels, 3), f32)
    alb_sum = np.zeros((o.n_pixels, 3), f32)
    s1, s2 = np.zeros(o.n_pixels, f32), np.zeros(o.n_pixels, f32)
    images, emitteds, values, firsts = [], [], [], []
    for k in range(spp):
        frame = first_frame + k
        o.set_frame(frame, 0)
        o.reset_image()
        o.set_counters([0, 0, gx * gy * 64])
        o.generate_rays(gx, gy, True)
        s = _Sample(o.image().copy())
        first = np.full(o.n_pixels, -1, np.int64)
        pending = None  # (pixels, normals) of the previous wavefront's diffuse hits, for `scatters`
        ex, ey = O.workgroup_size_64(gx * gy * 64)
        for b in range(P.max_wavefronts):
            n_rays = int(o.counters()[2])
            o.extend(ex, ey)
            c = o.counters()
            n_miss, n_hit = int(c[0]), int(c[1])
            rays = o.rays(max(n_rays, 1))
            hits = o.hits(n_hit)
            ridx = hits["ray_idx"].astype(np.int64)
            w = _Wave()
            w.b, w.frame = b, frame
            w.hp = rays["pixel_idx"][ridx].astype(np.int64)
            w.prim = hits["sphere_idx"].astype(np.int64)
            w.org, w.d = rays["origin"][ridx, :3].astype(f32), rays["direction"][ridx, :3].astype(f32)
            w.pt = w.org + hits["t"].astype(f32)[:, None] * w.d  # sh:91, per component o + t d
            midx = o.misses(n_miss).astype(np.int64)
            mp = rays["pixel_idx"][midx].astype(np.int64)
            md = rays["direction"][midx, :3].astype(f32)
            if scene is not None:
                w.alb = albedo[prims["material_idx"][w.prim].astype(np.int64)]
            if b == 0:
                first[w.hp] = w.prim
                if aov:
                    tex, bound = tx.factor(w.prim, w.pt)
                    alb_sum[w.hp] = alb_sum[w.hp] + np.where(bound[:, None], tex * w.alb, w.alb)
                    alb_sum[mp] = alb_sum[mp] + miss_colour(md)
            if scatters is not None and pending is not None and n_rays:
                rp = rays["pixel_idx"][:n_rays].astype(np.int64)
                nrm_of = np.full((o.n_pixels, 3), np.nan, f32)
                nrm_of[pending[0]] = pending[1]
                sel = ~np.isnan(nrm_of[rp, 0])
                scatters.append((nrm_of[rp[sel]], rays["direction"][:n_rays, :3][sel].astype(f32)))
            if n_miss < P.miss_floor:
                break
            t = s.thr[w.hp]
            if emitting:
                w.e, w.emits = em.colour(w.prim)
                if em.pass_first:
                    t = emission_pass(s, w, t)
            if textured:
                t = texture_pass(s, w, t)
            if emitting and not em.pass_first:
                t = emission_pass(s, w, t)
            if connect_sample is not None:
                pending = connect_pass(s, w, t)
            if scene is not None:
                s.thr[w.hp] = t * w.alb
            miss_pass(s, mp, md)
            gone = None
            if termination is not None and b + 1 < P.max_wavefronts:
                gone = termination.retire(s.thr, w.hp, frame, b)  # by hit index = the extension ray's slot
            o.set_counters([c[0], c[1], 0] + list(c[3:]))
            sx, sy = O.workgroup_size_64(n_hit)
            o.shade(sx, sy)
            if scene is None:
                s.thr[w.hp] = o.image()[w.hp]
            n_ext = int(o.counters()[2])
            o.swap_ray_queues()
            if gone is not None and gone.any():  # the oracle's extend skips such rays
                ext = o.rays(n_ext)
                assert n_ext == len(gone)
                ext["pixel_idx"][gone] = INACTIVE_PIXEL
                o.write_rays(ext)
            ex, ey = O.workgroup_size_64(n_ext)
            o.set_counters([0, 0, n_ext])
        value = s.thr + s.emitted if emitting else s.thr
        acc = acc + value
        L = luma(value)
        s1, s2 = s1 + L, s2 + L * L
        if parts:
            images.append(s.thr)
            emitteds.append(s.emitted)
            values.append(value)
            firsts.append(first)
    if parts:
        return {"acc": acc, "image": np.stack(images), "emitted": np.stack(emitteds), "value": np.stack(values), "s1": s1, "s2": s2,
                "first_prim": np.stack(firsts), "stats": stats}
    return (acc, alb_sum) if aov else acc
