"""numpy restatement of multiple importance sampling between the environment map and the scatter (WFPT_FLAG_ENV_MIS, include/wfpt.h
"Environment multiple importance sampling") on the pieces of env_nee_ref, mis_ref and nee_ref: env_nee_ref.render_with_env_nee with the
map's connect sample weighed by we, the emitters' by wl (plq = pl * q), the `origin` plane, the emission pass's weight with plq, and the
miss weighed by wb where the connected flag is 1. float32 in the header's operation order; the shadow rays are traced by a second oracle."""
import numpy as np

import env_nee_ref as V
import mis_ref as M
import nee_ref as N
from denoise_ref import luma
from environment_ref import INV_2PI, INV_PI, atan2_, env_lookup, normalize3
from nee_ref import PI, dot3

f32, f64, u32, u64 = np.float32, np.float64, np.uint32, np.uint64
TWO_PI_SQ = V.TWO_PI_SQ


def miss_weight(light, dirs, share, pb_of_len=None, with_p=True):
    """The miss pass's weight for un-normalised directions dirs (k, 3) under the map `light` (an env_nee_ref.EnvLight) with effective share
    `share`: a dict of pe, pb, wb (k,) float32 and texel (k,) int64 = yt * w + xt. pb_of_len / with_p: the mutations of
    tests/test_env_mis_host.py (another density of the scatter from the direction's length; pe without the share)."""
    d = light.dist
    dirs = np.asarray(dirs, f32).reshape(-1, 3)
    fw, fh = f32(d.w), f32(d.h)
    with np.errstate(all="ignore"):
        ln = np.sqrt(dot3(dirs, dirs))
        pb = ((f32(0.5) * ln) / PI) if pb_of_len is None else pb_of_len(ln)
        nx, ny, nz = normalize3(dirs[:, 0], dirs[:, 1], dirs[:, 2])
        phi = atan2_(nx, -nz)
        st = np.sqrt(nx * nx + nz * nz)
        theta = atan2_(st, ny)
        u = phi * INV_2PI + (f32(0.5) + f32(light.rotation))
        u = u - np.floor(u)
        v = theta * INV_PI
        xt = np.fmin(np.fmax(np.floor(u * fw), f32(0)), fw - f32(1)).astype(np.int64)  # (fmax drops a NaN: texel 0)
        yt = np.fmin(np.fmax(np.floor(v * fh), f32(0)), fh - f32(1)).astype(np.int64)
        assert ((0 <= xt) & (xt < d.w) & (0 <= yt) & (yt < d.h)).all(), "an index outside the table"
        k = d.row[yt, xt].astype(np.int64) - np.where(xt > 0, d.row[yt, np.maximum(xt - 1, 0)].astype(np.int64), 0)
        P = k.astype(f32) / u64(d.total).astype(f32)
        pdf = ((P * fw) * fh) / (TWO_PI_SQ * st)
        ok = (st > 0) & (pdf > 0)
        pe = np.where(ok, pdf * f32(share) if with_p else pdf, f32(0)).astype(f32)
        wb = np.where(ok, pb / (pb + pe), f32(1)).astype(f32)
    return {"pe": pe, "pb": pb.astype(f32), "wb": wb, "texel": yt * d.w + xt, "st": st.astype(f32)}


def miss_weight_rows(light, dirs, share):
    """wfpt_env_mis_miss_weight: (k, 4) of (pe, pb, wb, f32(texel))."""
    m = miss_weight(light, dirs, share)
    return np.stack([m["pe"], m["pb"], m["wb"], m["texel"].astype(f32)], 1).astype(f32)


def env_densities(s, n, share):
    """(pe, pb, we) of the environment samples s = light.sample(n, ..., share): pe = pdf * p, pb = cos_s / pi, we = pe / (pe + pb)."""
    with np.errstate(all="ignore"):
        pe = s["pdf"] * f32(share)
        pb = dot3(np.asarray(n, f32).reshape(-1, 3), s["w"]) / PI
        we = pe / (pe + pb)
    return pe.astype(f32), pb.astype(f32), we.astype(f32)


def sample_rows(light, shadow, rows, share):
    """wfpt_sample_environment_light_mis for rows (k, 10) of (p, n, u1 .. u4): (k, 12) of (wdir, texel, (e Genv) we, occluded, pe, pb, we, 0)."""
    rows = np.asarray(rows, f32)
    p, n = rows[:, :3], rows[:, 3:6]
    s = light.sample(n, rows[:, 6], rows[:, 7], rows[:, 8], rows[:, 9], share)
    pe, pb, we = env_densities(s, n, share)
    lit = s["lit"]
    occ = np.zeros(len(rows), bool)
    if lit.any():
        occ[lit] = V.any_hit(shadow, p[lit], s["w"][lit])
    with np.errstate(all="ignore"):
        f = (s["e"] * s["G"][:, None]) * we[:, None]
    z = f32(0)
    out = np.zeros((len(rows), 12), f32)
    out[:, :3] = s["w"]
    out[:, 3] = s["texel"].astype(f32)
    out[:, 4:7] = np.where(lit[:, None], f, z)
    out[:, 7] = occ
    out[:, 8], out[:, 9], out[:, 10] = np.where(lit, pe, z), np.where(lit, pb, z), np.where(lit, we, z)
    return out


def hit_weight_q(lights, o, ph, d, prim, q):
    """mis_ref.hit_weight with plq = pl * q in place of pl (the emission pass of a context that weighs its map): wb (k,)."""
    em = lights.em
    o, ph, d = np.asarray(o, f32), np.asarray(ph, f32), np.asarray(d, f32)
    prim = np.asarray(prim, np.int64)
    nf = f32(lights.n)
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
            nl, area = M.triangle_normal_area(em.triangles[prim])
        cos_l = np.abs(dot3(nl, w))
        pb = (f32(0.5) * np.sqrt(dot3(d, d))) / PI
        ok = (area > 0) & (dist2 > 0) & (cos_l > 0)
        plq = (dist2 / ((cos_l * area) * nf)) * f32(q)
        wb = np.where(ok, pb / (pb + plq), f32(1)).astype(f32)
    return wb


def render_with_env_mis(o, shadow, em, light, share=0.5, spp=1, first_frame=1, tx=None, parts=False, full_weight=False, miss_pb_of_len=None,
                        miss_pe_without_p=False, emission_plq_without_q=False):
    """env_nee_ref.render_with_env_nee with the weights. With a black map it is that function itself (the flag does nothing). The
    mutations of tests/test_env_mis_host.py: full_weight (both strategies at full weight: every we, wl and wb is 1), miss_pb_of_len (another
    density of the scatter in the miss pass), miss_pe_without_p (the miss pass's pe without the share; the connect pass keeps it -- with
    both sides changed the weights would still sum to one), emission_plq_without_q (the emission pass's pl without q; the connect pass
    keeps it, for the same reason)."""
    from oracle import oracle as O
    if not light.dist.ok:
        return V.render_with_env_nee(o, shadow, em, light, share=share, spp=spp, first_frame=first_frame, tx=tx, parts=parts)
    P = o.params
    assert P.tile_world == 1, "the restatement keys the connect stream by the oracle's pixel index: whole frames only"
    lights = N.Lights(em, tx)
    p_eff = f32(share) if lights.n else f32(1)
    q = f32(1) - p_eff
    gx = (o.width + 7) // 8
    gy = (o.height + 7) // 8
    prims = em.prims()
    albedo = np.asarray(em.materials["albedo"][:, :3], f32)
    acc = np.zeros((o.n_pixels, 3), f32)
    s1, s2 = np.zeros(o.n_pixels, f32), np.zeros(o.n_pixels, f32)
    images, emitteds, values = [], [], []
    stats = {"weighed_misses": 0, "weighed_hits": 0, "env_samples": 0, "light_samples": 0}
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
            # the emission pass: thr * e where the pixel's connected flag is 0, (thr * e) * wb with plq = pl * q where it is 1
            plain = emits & ~flag[hp]
            emitted[hp[plain]] = emitted[hp[plain]] + t[plain] * e[plain]
            wgt = emits & flag[hp]
            if wgt.any():
                assert np.array_equal(origin[hp[wgt]].view(u32), org[wgt].view(u32)), "origin is not the ray's origin"
                if full_weight:
                    wb = np.ones(int(wgt.sum()), f32)
                else:
                    wb = hit_weight_q(lights, origin[hp[wgt]], pt[wgt], d[wgt], prim[wgt], f32(1) if emission_plq_without_q else q)
                emitted[hp[wgt]] = emitted[hp[wgt]] + (t[wgt] * e[wgt]) * wb[:, None]
                stats["weighed_hits"] += int(wgt.sum())
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
                nrm = M.triangle_normal_area(em.triangles[prim[diffuse]])[0]
            u0, u1, u2, u3, u4 = V.connect_draws5(dpix, frame, b)
            to_env = np.ones(len(dp), bool) if not p_eff < 1 else u0 < p_eff
            with np.errstate(all="ignore"):
                base = t[diffuse] * alb[diffuse]
                # the environment branch
                ie = np.flatnonzero(to_env)
                s = light.sample(nrm[ie], u1[ie], u2[ie], u3[ie], u4[ie], p_eff)
                occ = np.zeros(len(ie), bool)
                occ[s["lit"]] = V.any_hit(shadow, dp[ie][s["lit"]], s["w"][s["lit"]])
                ok = s["lit"] & ~occ
                contrib = (base[ie] * s["e"]) * s["G"][:, None]
                if not full_weight:
                    contrib = contrib * env_densities(s, nrm[ie], p_eff)[2][:, None]
                emitted[dpix[ie][ok]] = emitted[dpix[ie][ok]] + contrib[ok]
                stats["env_samples"] += int(ok.sum())
                # the emitter branch
                il = np.flatnonzero(~to_env)
                if len(il):
                    sl = lights.sample(dp[il], nrm[il], (u0[il] - p_eff) / q, u1[il], u2[il])
                    sl["n"] = nrm[il]
                    occ = np.zeros(len(il), bool)
                    occ[sl["lit"]] = N.occluded(shadow, dp[il][sl["lit"]], sl["w"][sl["lit"]], sl["dist"][sl["lit"]])
                    ok = sl["lit"] & ~occ
                    contrib = ((base[il] * sl["e_q"]) * sl["G"][:, None]) / q
                    if not full_weight:
                        pl, pb, _ = M.light_densities(lights, dp[il], sl)
                        plq = pl * q
                        contrib = contrib * (plq / (plq + pb))[:, None]
                    emitted[dpix[il][ok]] = emitted[dpix[il][ok]] + contrib[ok]
                    stats["light_samples"] += int(ok.sum())
            thr[hp] = t * alb
            midx = o.misses(n_miss).astype(np.int64)
            mp = rays["pixel_idx"][midx].astype(np.int64)
            md = rays["direction"][midx, :3].astype(f32)
            factor = thr[mp] * env_lookup(light.env, md, light.intensity, light.rotation)
            g = flag[mp]
            if g.any() and not full_weight:
                wb = miss_weight(light, md[g], p_eff, pb_of_len=miss_pb_of_len, with_p=not miss_pe_without_p)["wb"]
                factor[g] = factor[g] * wb[:, None]
            stats["weighed_misses"] += int(g.sum())
            thr[mp] = factor
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
    return {"acc": acc, "image": np.stack(images), "emitted": np.stack(emitteds), "value": np.stack(values), "s1": s1, "s2": s2, "stats": stats}


def soft_sky(w=16, h=8, seed=3):
    """env_nee_ref.sun_map without its sun: the dim random sky alone."""
    env = V.sun_map(w, h, seed)
    env[h // 4, w // 3] = (np.random.default_rng(seed).random((h, w, 3)) * 0.2).astype(f32)[h // 4, w // 3]
    return env
