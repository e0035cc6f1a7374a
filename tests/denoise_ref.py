"""A numpy float32 restatement of the on-device denoiser (include/wfpt.h "Denoiser"): denoise_prepare_kernel and denoise_atrous_kernel
in their operation order. Every operation is an IEEE f32 operation on float32 arrays, so only exp, sqrt and pow may differ from the
kernels, by ulps.

Inputs are what the library's read-backs return for n >= 1 samples, as (h, w) / (h, w, 3) float32 arrays:
c = accumulated / n, the albedo, normal and depth AOVs, and v = wfpt_read_variance.
"""
import numpy as np

F = np.float32
DEFAULTS = {"iterations": 5, "sigma_luminance": 4.0, "sigma_normal": 128.0, "sigma_depth": 1.0, "sigma_albedo": 0.5}
H5 = (F(1.0 / 16.0), F(0.25), F(0.375), F(0.25), F(1.0 / 16.0))
K3 = (F(0.25), F(0.5), F(0.25))


def luma(c):
    return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


def shifted(a, dy, dx):
    """(a at (y + dy, x + dx), whether that pixel exists): a tap of every pixel at once."""
    h, w = a.shape[:2]
    out = np.zeros_like(a)
    valid = np.zeros((h, w), bool)
    if abs(dy) >= h or abs(dx) >= w:
        return out, valid
    ys, yd = slice(max(dy, 0), h + min(dy, 0)), slice(max(-dy, 0), h + min(-dy, 0))
    xs, xd = slice(max(dx, 0), w + min(dx, 0)), slice(max(-dx, 0), w + min(-dx, 0))
    out[yd, xd] = a[ys, xs]
    valid[yd, xd] = True
    return out, valid


def variance_resolve(s1, s2, n):
    """wfpt_read_variance from the moments S1, S2 of n samples."""
    if n == 0:
        return np.zeros_like(s1)
    nf = F(n)
    mu = s1 / nf
    return np.maximum(s2 / nf - mu * mu, F(0)) / nf


def prepare(c, albedo, normal, depth, variance, n):
    """denoise_prepare_kernel: (guide_nz (h, w, 4), guide_ag (h, w, 4), cv (h, w, 4))."""
    c, albedo, normal, z, v = (np.asarray(a, F) for a in (c, albedo, normal, depth, variance))
    h, w = z.shape
    with np.errstate(divide="ignore", invalid="ignore"):
        dot = (normal[..., 0] * normal[..., 0] + normal[..., 1] * normal[..., 1]) + normal[..., 2] * normal[..., 2]
        inv = F(1.0) / np.sqrt(dot)
        nhat = np.where((dot != 0)[..., None], normal * inv[..., None], F(0)).astype(F)
    grads = []
    for dy, dx in ((0, 1), (1, 0)):  # x, then y: the smaller step to an existing neighbour, 0 without one
        lo, lo_ok = shifted(z, -dy, -dx)
        hi, hi_ok = shifted(z, dy, dx)
        dl, dh = np.abs(lo - z), np.abs(hi - z)
        g = np.where(lo_ok & hi_ok, np.minimum(dl, dh), np.where(lo_ok, dl, np.where(hi_ok, dh, F(0))))
        grads.append(g.astype(F))
    grad = np.sqrt(grads[0] * grads[0] + grads[1] * grads[1])
    if n < 4:  # the population variance of L(c) over the clipped 7x7 window
        L = luma(c)
        s1, s2, m = np.zeros((h, w), F), np.zeros((h, w), F), np.zeros((h, w), F)
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                lq, ok = shifted(L, dy, dx)
                s1 = np.where(ok, s1 + lq, s1)
                s2 = np.where(ok, s2 + lq * lq, s2)
                m = np.where(ok, m + F(1), m)
        mu = s1 / m
        v = np.maximum(s2 / m - mu * mu, F(0))
    nz = np.concatenate([nhat, z[..., None]], axis=2).astype(F)
    ag = np.concatenate([albedo, grad[..., None]], axis=2).astype(F)
    cv = np.concatenate([c, v[..., None]], axis=2).astype(F)
    return nz, ag, cv


def atrous_pass(cv, nz, ag, step, sigma_luminance, sigma_normal, sigma_depth, sigma_albedo):
    """denoise_atrous_kernel at step `step`: the next (c, v)."""
    sl, sn, sz, sa = F(sigma_luminance), F(sigma_normal), F(sigma_depth), F(sigma_albedo)
    sa2 = sa * sa
    h, w = cv.shape[:2]
    lp = luma(cv)
    gs, gw = np.zeros((h, w), F), np.zeros((h, w), F)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            vq, ok = shifted(cv[..., 3], dy, dx)
            k = K3[dy + 1] * K3[dx + 1]
            gs = np.where(ok, gs + k * vq, gs)
            gw = np.where(ok, gw + k, gw)
    den_l = sl * np.sqrt(gs / gw) + F(1e-10)
    zscale = (sz * ag[..., 3]) * F(step)
    p_normal = (nz[..., :3] != 0).any(axis=2)
    sw = np.zeros((h, w), F)
    sc = np.zeros((h, w, 3), F)
    sv = np.zeros((h, w), F)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                cq, ok = shifted(cv, dy * step, dx * step)
                nq, _ = shifted(nz, dy * step, dx * step)
                aq, _ = shifted(ag, dy * step, dx * step)
                dl = np.abs(lp - luma(cq))
                dz = np.abs(nz[..., 3] - nq[..., 3])
                ar, ag_, ab = ag[..., 0] - aq[..., 0], ag[..., 1] - aq[..., 1], ag[..., 2] - aq[..., 2]
                da = (ar * ar + ag_ * ag_) + ab * ab
                den_z = zscale * np.sqrt(F(dx * dx + dy * dy)) + F(1e-3)
                e = (-(dl / den_l) - dz / den_z) - da / sa2
                q_normal = (nq[..., :3] != 0).any(axis=2)
                nd = (nz[..., 0] * nq[..., 0] + nz[..., 1] * nq[..., 1]) + nz[..., 2] * nq[..., 2]
                wn = np.where(p_normal & q_normal, np.power(np.maximum(nd, F(0)), sn),
                              np.where(p_normal == q_normal, F(1), F(0))).astype(F)
                wt = ((H5[dx + 2] * H5[dy + 2]) * np.exp(e).astype(F)) * wn
                sw = np.where(ok, sw + wt, sw)
                sc = np.where(ok[..., None], sc + wt[..., None] * cq[..., :3], sc)
                sv = np.where(ok, sv + (wt * wt) * cq[..., 3], sv)
    out = np.empty_like(cv)
    out[..., :3] = sc / sw[..., None]
    out[..., 3] = sv / (sw * sw)
    return out


def denoise(c, albedo, normal, depth, variance, n, **params):
    """wfpt_denoise: the last pass's colour (h, w, 3); n = samples accumulated (>= 1)."""
    p = {**DEFAULTS, **params}
    nz, ag, cv = prepare(c, albedo, normal, depth, variance, n)
    for i in range(int(p["iterations"])):
        cv = atrous_pass(cv, nz, ag, 1 << i, p["sigma_luminance"], p["sigma_normal"], p["sigma_depth"], p["sigma_albedo"])
    return cv[..., :3].copy()
