"""numpy float32 restatement of surface textures (WFPT_FLAG_TEXTURES) in the kernels' operation order: sphere_uv, triangle_uv and tex_lookup
of wfpt_device_math.h, and a whole textured render driven through the oracle's stages. Every step is one IEEE f32 operation (numpy float32
rounds each one as the device does with -ffp-contract=off), so the results are the device's bits."""
import numpy as np

from environment_ref import INV_2PI, INV_PI, atan2_
from transport_ref import dot3_components as dot3
from transport_ref import f32, normalize3, render

FILTERS = {"bilinear": 0, "nearest": 1}


def sphere_uv(p, centre):
    """(u, v) of points p (..., 3) on spheres with centres (..., 3): the normal scatter() uses, Shirley's get_sphere_uv."""
    p, c = np.asarray(p, f32), np.asarray(centre, f32)
    nx, ny, nz = normalize3(p[..., 0] - c[..., 0], p[..., 1] - c[..., 1], p[..., 2] - c[..., 2])
    u = atan2_(-nz, nx) * INV_2PI + f32(0.5)
    v = atan2_(np.sqrt(nx * nx + nz * nz), -ny) * INV_PI
    return u.astype(f32), v.astype(f32)


def triangle_uv(p, v0, e1, e2, uv6):
    """(u, v) of points p (..., 3) on triangles (v0, e1, e2) with corner UVs uv6 (..., 6) = u0 v0 u1 v1 u2 v2."""
    p, v0, e1, e2, uv6 = (np.asarray(a, f32) for a in (p, v0, e1, e2, uv6))
    wx, wy, wz = p[..., 0] - v0[..., 0], p[..., 1] - v0[..., 1], p[..., 2] - v0[..., 2]
    a = (e1[..., 0], e1[..., 1], e1[..., 2])
    b = (e2[..., 0], e2[..., 1], e2[..., 2])
    d00, d01, d11 = dot3(*a, *a), dot3(*a, *b), dot3(*b, *b)
    d20, d21 = dot3(wx, wy, wz, *a), dot3(wx, wy, wz, *b)
    den = d00 * d11 - d01 * d01
    ok = den > 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = f32(1) / np.where(ok, den, f32(1))
        b1 = np.where(ok, (d11 * d20 - d01 * d21) * inv, f32(0)).astype(f32)
        b2 = np.where(ok, (d00 * d21 - d01 * d20) * inv, f32(0)).astype(f32)
    b0 = (f32(1) - b1) - b2
    u = (uv6[..., 0] * b0 + uv6[..., 2] * b1) + uv6[..., 4] * b2
    v = (uv6[..., 1] * b0 + uv6[..., 3] * b1) + uv6[..., 5] * b2
    return u.astype(f32), v.astype(f32)


def _wrap_pair(c0, fn, n):
    with np.errstate(invalid="ignore"):
        k = np.fmin(np.fmax(c0, f32(-1)), fn - f32(1)).astype(np.int64)
    return np.where(k < 0, n - 1, k), np.where(k + 1 >= n, 0, k + 1)


def tex_lookup(img, u, v, scale=(1.0, 1.0), offset=(0.0, 0.0), filter="bilinear"):
    """The texture img (h, w, 3) float32 (row 0 = the top) at (u, v): (..., 3)."""
    img = np.asarray(img, f32)
    h, w = img.shape[:2]
    u, v = np.asarray(u, f32), np.asarray(v, f32)
    uu = u * f32(scale[0]) + f32(offset[0])
    vv = v * f32(scale[1]) + f32(offset[1])
    uu = uu - np.floor(uu)
    vv = vv - np.floor(vv)
    fw, fh = f32(w), f32(h)
    ry = f32(1) - vv
    if FILTERS.get(filter, filter) == 1:
        with np.errstate(invalid="ignore"):
            cx = np.fmin(np.fmax(np.floor(uu * fw), f32(0)), fw - f32(1)).astype(np.int64)
            cy = np.fmin(np.fmax(np.floor(ry * fh), f32(0)), fh - f32(1)).astype(np.int64)
        return img[cy, cx].astype(f32)
    x = uu * fw - f32(0.5)
    y = ry * fh - f32(0.5)
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = x - x0, y - y0
    c0, c1 = _wrap_pair(x0, fw, w)
    r0, r1 = _wrap_pair(y0, fh, h)
    t00, t10, t01, t11 = img[r0, c0], img[r0, c1], img[r1, c0], img[r1, c1]
    gx, gy = f32(1) - fx, f32(1) - fy
    w00, w10, w01, w11 = (gx * gy)[..., None], (fx * gy)[..., None], (gx * fy)[..., None], (fx * fy)[..., None]
    return (((t00 * w00 + t10 * w10) + t01 * w01) + t11 * w11).astype(f32)


class Textures:
    """What a textured context holds: slots {slot: (img, params)}, bindings {material_idx: slot}, the UV table (n, 6) or None, and the
    scene's primitives as the device holds them (spheres, or triangles with their rows in _pad) and materials."""

    def __init__(self, spheres=None, triangles=None, materials=None, slots=None, bind=None, uv=None):
        self.spheres, self.triangles = spheres, triangles
        self.materials = materials
        self.slots, self.bind = dict(slots or {}), dict(bind or {})
        self.uv = None if uv is None else np.asarray(uv, f32).reshape(-1, 6)

    def factor(self, prim, p):
        """(tex (n, 3), textured mask (n,)) for hits on primitives prim (n,) at points p (n, 3)."""
        prims = self.spheres if self.triangles is None else self.triangles
        mat = prims["material_idx"][prim].astype(np.int64)
        slot = np.array([self.bind.get(int(m), -1) for m in mat], np.int64) if len(mat) else np.zeros(0, np.int64)
        tex = np.ones((len(prim), 3), f32)
        if self.triangles is None:
            u, v = sphere_uv(p, self.spheres["center"][prim, :3])
        else:
            t = self.triangles[prim]
            rows = np.zeros((len(prim), 6), f32) if self.uv is None else self.uv[t["_pad"].astype(np.int64)]
            u, v = triangle_uv(p, t["v0"], t["e1"], t["e2"], rows)
        for s, (img, params) in self.slots.items():
            sel = slot == s
            if sel.any():
                tex[sel] = tex_lookup(img, u[sel], v[sel], **params)
        return tex, slot >= 0


def render_with_textures(o, tx, spp=1, first_frame=1, env=None, env_params=None, aov=False, termination=None):
    """transport_ref.render with the texture pass alone: at every hit thr <- (thr * tex) * albedo (thr * albedo where unbound), at every
    miss thr <- thr * sky (or the environment map). Returns the accumulated image (n_pixels x 3), and with aov=True also the sum of the
    primary hits' tex * albedo (the sky / map value of a primary miss)."""
    return render(o, tx=tx, env=env, env_params=env_params, termination=termination, spp=spp, first_frame=first_frame, aov=aov)
