"""numpy float32 restatement of multiple importance sampling (WFPT_FLAG_MIS, include/wfpt.h "Multiple importance sampling") on nee_ref's
pieces: nee_ref.render_with_nee with the connect sample weighed by wl, the per-pixel `origin` plane, and the emission pass's weight wb where
the connected flag is 1. Every step is one IEEE f32 operation in the header's order; the shadow rays are traced through the second oracle,
exactly as nee_ref does."""
import numpy as np

import nee_ref as N
from denoise_ref import luma
from environment_ref import env_lookup, normalize3, sky
from nee_ref import PI, dot3, f32


def light_densities(lights, p, s):
    """(pl, pb, wl) of connect samples s = lights.sample(p, n, ...) -- the header's step 5. cos_s, cos_l, A and dist2 are recomputed here by
    the operations Lights.sample uses (it does not return them), so they carry the same bits. n is needed for cos_s: pass it in s["n"]."""
    em = lights.em
    nf = f32(lights.n)
    prim = s["prim"]
    with np.errstate(all="ignore"):
        if em.triangles is None:
            sp = em.spheres[prim]
            c = sp["center"][:, :3].astype(f32)
            ra = np.abs(sp["radius"].astype(f32))
            nl = (s["q"] - c) / ra[:, None]
            area = (f32(4) * PI) * (ra * ra)
        else:
            nl, area = triangle_normal_area(em.triangles[prim])
        v = s["q"] - np.asarray(p, f32)
        dist2 = dot3(v, v)
        cos_s, cos_l = dot3(np.asarray(s["n"], f32), s["w"]), np.abs(dot3(nl, s["w"]))
        pb = cos_s / PI
        pl = dist2 / ((cos_l * area) * nf)
        wl = pl / (pl + pb)
    return pl.astype(f32), pb.astype(f32), wl.astype(f32)


def triangle_normal_area(t):
    e1, e2 = t["e1"].astype(f32), t["e2"].astype(f32)
    cr = [e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]]
    with np.errstate(all="ignore"):
        nl = np.stack(normalize3(*cr), 1).astype(f32)
        area = f32(0.5) * np.sqrt((cr[0] * cr[0] + cr[1] * cr[1]) + cr[2] * cr[2])
    return nl, area


def hit_weight(lights, o, ph, d, prim, pb_of_len=None, with_nf=True):
    """The emission pass's weight for hits at ph on emitter `prim` (k,) of rays that left o with direction d (not normalised): a dict of
    pl, pb, wb, cos_l (k,), the header's operation order. pb_of_len / with_nf: the mutations of tests/test_mis_host.py."""
    em = lights.em
    o, ph, d = np.asarray(o, f32), np.asarray(ph, f32), np.asarray(d, f32)
    prim = np.asarray(prim, np.int64)
    nf = f32(lights.n) if with_nf else f32(1)
    with np.errstate(all="ignore"):
        v = ph - o
        dist2 = dot3(v, v)
        dist = np.sqrt(dist2)
        w = v / dist[:, None]
        if em.triangles is None:
            sp = em.spheres[prim]
            c = sp["center"][:, :3].astype(f32)
            ra = np.abs(sp["radius"].astype(f32))
            nl = (ph - c) / ra[:, None]
            area = (f32(4) * PI) * (ra * ra)
        else:
            nl, area = triangle_normal_area(em.triangles[prim])
        cos_l = np.abs(dot3(nl, w))
        ln = np.sqrt(dot3(d, d))
        pb = ((f32(0.5) * ln) / PI) if pb_of_len is None else pb_of_len(ln)
        ok = (area > 0) & (dist2 > 0) & (cos_l > 0)
        pl = np.where(ok, dist2 / ((cos_l * area) * nf), f32(0)).astype(f32)
        wb = np.where(ok, pb / (pb + pl), f32(1)).astype(f32)
    return {"pl": pl, "pb": pb.astype(f32), "wb": wb, "cos_l": cos_l.astype(f32)}


def hit_weight_rows(lights, rows):
    """wfpt_mis_hit_weight for rows (k, 8) of (o, d, t, primitive): (k, 4) of (pl, pb, wb, cos_l); a primitive that does not emit or is out
    of range (NaN included) answers (0, pb, 1, 0)."""
    rows = np.asarray(rows, f32)
    o, d, t, pf = rows[:, :3], rows[:, 3:6], rows[:, 6], rows[:, 7]
    n_prims = len(lights.em.prims())
    with np.errstate(all="ignore"):
        ph = o + t[:, None] * d
        inside = (pf >= 0) & (pf < f32(n_prims))
        prim = np.where(inside, pf, 0).astype(np.int64)
        emits = inside & np.isin(prim, lights.list)
        r = hit_weight(lights, o, ph, d, prim)
    out = np.stack([np.where(emits, r["pl"], f32(0)), r["pb"], np.where(emits, r["wb"], f32(1)), np.where(emits, r["cos_l"], f32(0))], 1)
    return out.astype(f32)


def sample_rows(lights, shadow, rows):
    """wfpt_sample_lights_mis for rows (k, 9) of (p, n, u0, u1, u2): (k, 12) of (q, primitive, (e_q G) wl, occluded, pl, pb, wl, 0)."""
    rows = np.asarray(rows, f32)
    p, n = rows[:, :3], rows[:, 3:6]
    s = lights.sample(p, n, rows[:, 6], rows[:, 7], rows[:, 8])
    s["n"] = n
    pl, pb, wl = light_densities(lights, p, s)
    lit = s["lit"]
    occ = np.zeros(len(rows), bool)
    occ[lit] = N.occluded(shadow, p[lit], s["w"][lit], s["dist"][lit])
    with np.errstate(all="ignore"):
        f = (s["e_q"] * s["G"][:, None]) * wl[:, None]
    z = f32(0)
    out = np.zeros((len(rows), 12), f32)
    out[:, :3] = s["q"]
    out[:, 3] = s["prim"].astype(f32)
    out[:, 4:7] = np.where(lit[:, None], f, z)
    out[:, 7] = occ
    out[:, 8], out[:, 9], out[:, 10] = np.where(lit, pl, z), np.where(lit, pb, z), np.where(lit, wl, z)
    return out


def render_with_mis(o, shadow, em, spp=1, first_frame=1, tx=None, env=None, env_params=None, parts=False, no_wl=False, no_wb=False,
                    no_nf=False, pb_of_len=None, scatters=None):
    """nee_ref.render_with_nee with the two weights. With no light it is that function itself. The mutations of tests/test_mis_host.py:
    no_wl (the connect sample at full weight), no_wb (the flagged emitter hit at full weight), no_nf (pl of the emission pass without the
    light count), pb_of_len (another density of the scatter from the direction's length). scatters: a list that receives, per wavefront,
    (normal, direction) of every extension ray a Lambertian non-emitter hit produced (the identity test's data)."""
    from oracle import oracle as O
    P = o.params
    assert P.tile_world == 1, "the restatement keys the connect stream by the oracle's pixel index: whole frames only"
    lights = N.Lights(em, tx)
    if lights.n == 0:
        return N.render_with_nee(o, shadow, em, spp=spp, first_frame=first_frame, tx=tx, env=env, env_params=env_params, parts=parts)
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
        origin = np.zeros((o.n_pixels, 3), f32)
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
            hp = rays["pixel_idx"][ridx].astype(np.int64)
            prim = hits["sphere_idx"].astype(np.int64)
            if scatters is not None and pending is not None and n_rays:
                rp = rays["pixel_idx"][:n_rays].astype(np.int64)
                nrm_of = np.full((o.n_pixels, 3), np.nan, f32)
                nrm_of[pending[0]] = pending[1]
                sel = ~np.isnan(nrm_of[rp, 0])
                scatters.append((nrm_of[rp[sel]], rays["direction"][:n_rays, :3][sel].astype(f32)))
            if n_miss < P.miss_floor:
                break
            t = thr[hp]
            e, emits = em.colour(prim)
            org, d = rays["origin"][ridx, :3].astype(f32), rays["direction"][ridx, :3].astype(f32)
            pt = org + hits["t"].astype(f32)[:, None] * d  # sh:91, per component o + t d
            if tx is not None:  # the texture pass
                tex, bound = tx.factor(prim, pt)
                t = np.where(bound[:, None], t * tex, t)
            # the emission pass: thr * e where the pixel's connected flag is 0, (thr * e) * wb where it is 1
            plain = emits & ~flag[hp]
            emitted[hp[plain]] = emitted[hp[plain]] + t[plain] * e[plain]
            wgt = emits & flag[hp]
            if wgt.any():
                assert np.array_equal(origin[hp[wgt]].view(np.uint32), org[wgt].view(np.uint32)), "origin is not the ray's origin"
                if no_wb:
                    wb = np.ones(int(wgt.sum()), f32)
                else:
                    wb = hit_weight(lights, origin[hp[wgt]], pt[wgt], d[wgt], prim[wgt], pb_of_len=pb_of_len, with_nf=not no_nf)["wb"]
                emitted[hp[wgt]] = emitted[hp[wgt]] + (t[wgt] * e[wgt]) * wb[:, None]
            t = np.where(emits[:, None], f32(0), t)
            alb = albedo[prims["material_idx"][prim].astype(np.int64)]
            # the connect pass
            mclass = prims["material_type"][prim].astype(np.int64)
            diffuse = ((mclass == 0) | (mclass > 2)) & ~emits
            flag[hp[~diffuse]] = False
            flag[hp[diffuse]] = True
            dp, dpix = pt[diffuse], hp[diffuse]
            origin[dpix] = dp
            if em.triangles is None:
                nrm = np.stack(normalize3(*[dp[:, a] - em.spheres["center"][prim[diffuse], a] for a in range(3)]), 1).astype(f32)
            else:
                nrm = triangle_normal_area(em.triangles[prim[diffuse]])[0]
            pending = (dpix, nrm)
            u0, u1, u2 = N.connect_draws(dpix, frame, b)
            s = lights.sample(dp, nrm, u0, u1, u2)
            s["n"] = nrm
            lit = s["lit"]
            occ = np.zeros(len(dp), bool)
            occ[lit] = N.occluded(shadow, dp[lit], s["w"][lit], s["dist"][lit])
            ok = lit & ~occ
            with np.errstate(all="ignore"):
                contrib = ((t[diffuse] * alb[diffuse]) * s["e_q"]) * s["G"][:, None]
                if not no_wl:
                    contrib = contrib * light_densities(lights, dp, s)[2][:, None]
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


# ---------------------------------------------------------------- the near-lamp scene
# An emitting sphere of radius 1 whose gap to the radius-1000 ground is 0.05 of its radius: under it the connect pass's 1 / dist2 is
# unbounded while half its samples lie on the lamp's far side; the scattered ray hits the lamp with high probability and a bounded weight.
NEAR = {"ground_r": 1000.0, "lamp_r": 1.0, "gap": 0.05, "albedo": (0.5, 0.75, 0.25), "e": (4.0, 2.0, 8.0)}


def near_lamp_inputs(orc, w, h, buried=False):
    """The radius-1000 Lambertian ground (material 0) under the near lamp (material 1), seen from above at an angle. Returns (spheres,
    materials, nodes, cam, inv_proj, view); the emitter's colour is NEAR["e"] for material 1. buried: a second sphere of material 1 deep
    inside the ground sphere. It lies below every ground point's tangent plane and no scattered ray can reach it, so it lights nothing:
    it only makes the light list two long (nf = 2), which the single lamp cannot."""
    sp = np.zeros(3 if buried else 2, orc.SPHERE)
    mt = np.zeros(2, orc.MATERIAL)
    mt["albedo"][:] = (0.5, 0.5, 0.5, 1.0)
    mt["albedo"][0, :3] = NEAR["albedo"]
    sp["center"][:, 3] = 1.0
    sp["center"][0, :3] = (0.0, -NEAR["ground_r"], 0.0)
    sp["radius"][0] = NEAR["ground_r"]
    sp["center"][1, :3] = (0.0, NEAR["lamp_r"] * (1.0 + NEAR["gap"]), 0.0)
    sp["radius"][1] = NEAR["lamp_r"]
    sp["material_idx"][:2] = (0, 1)
    if buried:
        sp["center"][2, :3] = (0.0, -0.5 * NEAR["ground_r"], 0.0)
        sp["radius"][2] = NEAR["lamp_r"]
        sp["material_idx"][2] = 1
    sp["material_type"] = mt["material_type"][sp["material_idx"]]
    sp, nodes = orc.build_bvh(sp)
    cam, ip, vw = orc.camera((0.0, 5.0, 7.0), (0.0, 0.0, 0.0), 40.0, 0.0, 10.0, 0.1, 100.0, w, h)
    return sp, mt, nodes, cam, ip, vw
