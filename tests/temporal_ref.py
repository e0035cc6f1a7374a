"""A numpy float32 restatement of temporal_prepare_kernel (include/wfpt.h "Temporal denoiser") past its projection: the taps, their
acceptance and the count-weighted blend, in the kernel's operation order. Prepare's part comes from tests/denoise_ref.py, so the
no-history pixels are prepare's bits.

Inputs, as (h, w[, k]) float32 arrays:
- `cur`: the current epoch's sums and read-backs: "sum" (accumulated), "s1", "s2" (the luminance moment sums), the AOVs "albedo",
  "normal", "depth", "coverage" and "material_id" (uint32), and n;
- `sealed`: what the sealed epoch's last call left, read right after it: temporal("color" / "moments" / "length") and that epoch's AOVs
  "normal", "depth", "coverage", "material_id";
- `motion`: the library's own MOTION read-back (x', y', z'); the projection itself is checked against float64 separately.
"""
import numpy as np

import denoise_ref as R

F = np.float32
NO_MOTION = F(-1e30)
DEFAULTS = {**R.DEFAULTS, "history_cap": 32.0, "depth_tolerance": 0.05, "normal_cos": 0.9}


def nhat(normal):
    """prepare's normalised normal: n * (1 / sqrt((x x + y y) + z z)), 0 where the sum is 0."""
    normal = np.asarray(normal, F)
    with np.errstate(divide="ignore", invalid="ignore"):
        dot = (normal[..., 0] * normal[..., 0] + normal[..., 1] * normal[..., 1]) + normal[..., 2] * normal[..., 2]
        inv = F(1.0) / np.sqrt(dot)
        return np.where((dot != 0)[..., None], normal * inv[..., None], F(0)).astype(F)


def taps(motion, width, height):
    """[(xt, yt, weight, inside)] of the four bilinear taps in the kernel's order."""
    mx, my = motion[..., 0].astype(F), motion[..., 1].astype(F)
    fx0, fy0 = np.floor(mx), np.floor(my)
    ok = (fx0 >= F(-1)) & (fx0 < F(width)) & (fy0 >= F(-1)) & (fy0 < F(height))
    fx, fy = mx - fx0, my - fy0
    x0 = np.where(ok, fx0, F(-8)).astype(np.int64)
    y0 = np.where(ok, fy0, F(-8)).astype(np.int64)
    one = F(1)
    weights = ((one - fx) * (one - fy), fx * (one - fy), (one - fx) * fy, fx * fy)
    out = []
    for k in range(4):
        xt, yt = x0 + (k & 1), y0 + (k >> 1)
        inside = ok & (xt >= 0) & (xt < width) & (yt >= 0) & (yt < height)
        out.append((np.clip(xt, 0, width - 1), np.clip(yt, 0, height - 1), weights[k].astype(F), inside))
    return out


def accepted(cur_nhat, cur_cov, cur_mat, sealed_nhat, sealed_depth, sealed_cov, sealed_mat, motion, depth_tolerance, normal_cos):
    """(h, w, 4) bool: which taps the kernel accepts, and the taps themselves."""
    h, w = cur_cov.shape
    hit = cur_cov > 0
    zp = motion[..., 2].astype(F)
    tol, ncos = F(depth_tolerance), F(normal_cos)
    tp = taps(motion, w, h)
    acc = np.zeros((h, w, 4), bool)
    for k, (xt, yt, _, inside) in enumerate(tp):
        cov_t, mat_t = sealed_cov[yt, xt], sealed_mat[yt, xt]
        n_t, z_t = sealed_nhat[yt, xt], sealed_depth[yt, xt]
        dot = (cur_nhat[..., 0] * n_t[..., 0] + cur_nhat[..., 1] * n_t[..., 1]) + cur_nhat[..., 2] * n_t[..., 2]
        ok_hit = (cov_t > 0) & (mat_t == cur_mat) & (np.abs(z_t - zp) <= tol * zp) & (dot >= ncos)
        acc[..., k] = inside & np.where(hit, ok_hit, cov_t == 0)
    return acc, tp


def temporal_prepare(cur, sealed, motion, history_cap=DEFAULTS["history_cap"], depth_tolerance=DEFAULTS["depth_tolerance"],
                     normal_cos=DEFAULTS["normal_cos"]):
    """The kernel's outputs: dict of "color" (h, w, 3), "moments" (h, w, 2), "length" (h, w), "cv" (h, w, 4) = pass 0's input, and
    prepare's guides "nz", "ag". `sealed` None = no sealed slot (no projection)."""
    n = int(cur["n"])
    nf = F(n)
    S = np.asarray(cur["sum"], F)
    s1, s2 = np.asarray(cur["s1"], F), np.asarray(cur["s2"], F)
    h, w = s1.shape
    c = S / nf
    var = R.variance_resolve(s1, s2, n)
    nz, ag, cv = R.prepare(c, cur["albedo"], cur["normal"], cur["depth"], var, n)
    color, length = cv[..., :3].copy(), np.full((h, w), nf, F)
    m1, m2 = s1 / nf, s2 / nf
    v = cv[..., 3].copy()
    if sealed is not None:
        acc, tp = accepted(nz[..., :3], np.asarray(cur["coverage"], F), np.asarray(cur["material_id"], np.uint32),
                           nhat(sealed["normal"]), np.asarray(sealed["depth"], F), np.asarray(sealed["coverage"], F),
                           np.asarray(sealed["material_id"], np.uint32), np.asarray(motion, F), depth_tolerance, normal_cos)
        sc, sl, sm = np.asarray(sealed["color"], F), np.asarray(sealed["length"], F), np.asarray(sealed["moments"], F)
        wsum = np.zeros((h, w), F)
        hc = np.zeros((h, w, 3), F)
        hl, hm1, hm2 = np.zeros((h, w), F), np.zeros((h, w), F), np.zeros((h, w), F)
        for k, (xt, yt, wt, _) in enumerate(tp):
            a = acc[..., k]
            wsum = np.where(a, wsum + wt, wsum)
            hc = np.where(a[..., None], hc + wt[..., None] * sc[yt, xt], hc)
            hl = np.where(a, hl + wt * sl[yt, xt], hl)
            hm1 = np.where(a, hm1 + wt * sm[yt, xt, 0], hm1)
            hm2 = np.where(a, hm2 + wt * sm[yt, xt, 1], hm2)
        hist = (wsum >= F(0.01)) & (F(history_cap) > F(0))
        with np.errstate(divide="ignore", invalid="ignore"):
            hh = np.minimum(hl / wsum, F(history_cap))
            L = hh + nf
            bc = (hh[..., None] * (hc / wsum[..., None]) + S) / L[..., None]
            b1 = (hh * (hm1 / wsum) + s1) / L
            b2 = (hh * (hm2 / wsum) + s2) / L
            d = b2 - b1 * b1
            bv = np.where(L < F(4), cv[..., 3] * (nf / L), np.where(d > 0, d, F(0)) / L)
        color = np.where(hist[..., None], bc, color).astype(F)
        length = np.where(hist, L, length).astype(F)
        m1, m2 = np.where(hist, b1, m1).astype(F), np.where(hist, b2, m2).astype(F)
        v = np.where(hist, bv, v).astype(F)
    cv = np.concatenate([color, v[..., None]], axis=2).astype(F)
    return {"color": color, "moments": np.stack([m1, m2], axis=2).astype(F), "length": length, "cv": cv, "nz": nz, "ag": ag}


def denoise_temporal(cur, sealed, motion, **params):
    """wfpt_denoise_temporal: the last pass's colour (h, w, 3)."""
    p = {**DEFAULTS, **params}
    out = temporal_prepare(cur, sealed, motion, p["history_cap"], p["depth_tolerance"], p["normal_cos"])
    cv = out["cv"]
    for i in range(int(p["iterations"])):
        cv = R.atrous_pass(cv, out["nz"], out["ag"], 1 << i, p["sigma_luminance"], p["sigma_normal"], p["sigma_depth"], p["sigma_albedo"])
    return cv[..., :3].copy()
