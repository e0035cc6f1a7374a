"""numpy restatement of multiple importance sampling between the environment map and the scatter (WFPT_FLAG_ENV_MIS, include/wfpt.h
"Environment multiple importance sampling") on the pieces of env_nee_ref and nee_ref: the weights and row samplers, and
transport_ref.render with the map's connect sample weighed by we, the emitters' by wl (plq = pl * q), the `origin` plane, the emission
pass's weight with plq, and the miss weighed by wb where the connected flag is 1. float32 in the header's operation order; the shadow rays
are traced by a second oracle."""
import numpy as np

import env_nee_ref as V
import nee_ref as N
from environment_ref import INV_2PI, INV_PI, atan2_
from nee_ref import PI
from transport_ref import dot3, f32, normalize3, render

f64, u32, u64 = np.float64, np.uint32, np.uint64
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
    o, ph, d = np.asarray(o, f32), np.asarray(ph, f32), np.asarray(d, f32)
    prim = np.asarray(prim, np.int64)
    nf = f32(lights.n)
    with np.errstate(all="ignore"):
        v = ph - o
        dist2 = dot3(v, v)
        dist = np.sqrt(dist2)
        w = v / dist[:, None]
        nl, area = lights.normal_area(prim, ph)
        cos_l = np.abs(dot3(nl, w))
        pb = (f32(0.5) * np.sqrt(dot3(d, d))) / PI
        ok = (area > 0) & (dist2 > 0) & (cos_l > 0)
        plq = (dist2 / ((cos_l * area) * nf)) * f32(q)
        wb = np.where(ok, pb / (pb + plq), f32(1)).astype(f32)
    return wb


def render_with_env_mis(o, shadow, em, light, share=0.5, spp=1, first_frame=1, tx=None, parts=False, full_weight=False, miss_pb_of_len=None,
                        miss_pe_without_p=False, emission_plq_without_q=False, termination=None):
    """env_nee_ref.render_with_env_nee with the weights (the loop's `env_weighing`). With a black map the loop weighs nothing: it is that
    function itself (the flag does nothing). The mutations of tests/test_env_mis_host.py: full_weight (both strategies at full weight:
    every we, wl and wb is 1), miss_pb_of_len (another density of the scatter in the miss pass), miss_pe_without_p (the miss pass's pe
    without the share; the connect pass keeps it -- with both sides changed the weights would still sum to one), emission_plq_without_q
    (the emission pass's pl without q; the connect pass keeps it, for the same reason)."""
    return render(o, shadow=shadow, em=em, tx=tx, lights=N.Lights(em, tx), env_light=light, share=share, weigh=True, termination=termination,
                  spp=spp, first_frame=first_frame, parts=parts, full_weight=full_weight, miss_pb_of_len=miss_pb_of_len,
                  miss_pe_without_p=miss_pe_without_p, emission_plq_without_q=emission_plq_without_q)


def soft_sky(w=16, h=8, seed=3):
    """env_nee_ref.sun_map without its sun: the dim random sky alone."""
    env = V.sun_map(w, h, seed)
    env[h // 4, w // 3] = (np.random.default_rng(seed).random((h, w, 3)) * 0.2).astype(f32)[h // 4, w // 3]
    return env
