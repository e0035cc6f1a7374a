"""numpy float32 restatement of the environment map (WFPT_FLAG_ENVIRONMENT) in the kernels' operation order: normalize3, atan2_ and the
bilinear lookup of wfpt_device_math.h, and a whole lit render driven through the oracle's stages with the map applied where miss_kernel would
colour a miss. Every step is one IEEE f32 operation (numpy float32 rounds each one as the device does with -ffp-contract=off), so the results
are the device's bits."""
import numpy as np

from transport_ref import f32, normalize3, render
INV_2PI = f32(0.15915494)
INV_PI = f32(0.31830988)
TAN_PI_8 = f32(0.41421356)
ATAN_HALF = (f32(4.636476040e-01), f32(5.012158688e-09))  # atan(1/2), pi/2, pi as hi + lo
PI_2 = (f32(1.570796371e+00), f32(-4.371138829e-08))
PI = (f32(3.141592741e+00), f32(-8.742277657e-08))
C3, C2, C1, C0 = f32(8.05374449538e-2), f32(1.38776856032e-1), f32(1.99777106478e-1), f32(3.33329491539e-1)


def atan2_(y, x):
    y, x = np.asarray(y, f32), np.asarray(x, f32)
    ax, ay = np.abs(x), np.abs(y)
    hi = np.where(ax > ay, ax, ay)
    lo = np.where(ax > ay, ay, ax)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        t = np.where(hi > 0, lo / np.where(hi > 0, hi, f32(1)), f32(0)).astype(f32)
        big = t > TAN_PI_8
        r = np.where(big, (f32(2) * lo - hi) / (f32(2) * hi + lo), t).astype(f32)
    z = r * r
    p = (((C3 * z - C2) * z + C1) * z - C0) * z
    a = p * r + r
    a = np.where(big, ATAN_HALF[0] + (ATAN_HALF[1] + a), a)
    a = np.where(ay > ax, PI_2[0] + (PI_2[1] - a), a)
    a = np.where(x < 0, PI[0] + (PI[1] - a), a)
    return np.where(y < 0, -a, a).astype(f32)


def env_uv(dirs, rotation=0.0):
    """(u, v) of the map for directions (..., 3)."""
    d = np.asarray(dirs, f32)
    nx, ny, nz = normalize3(d[..., 0], d[..., 1], d[..., 2])
    phi = atan2_(nx, -nz)
    theta = atan2_(np.sqrt(nx * nx + nz * nz), ny)
    u = phi * INV_2PI + (f32(0.5) + f32(rotation))
    u = u - np.floor(u)
    return u.astype(f32), (theta * INV_PI).astype(f32)


def env_lookup(env, dirs, intensity=1.0, rotation=0.0):
    """The map's value for directions (..., 3): env is H x W x 3 (or x 4) float32, row 0 = +y."""
    env = np.asarray(env, f32)
    h, w = env.shape[:2]
    u, v = env_uv(dirs, rotation)
    fw, fh = f32(w), f32(h)
    x = u * fw - f32(0.5)
    y = v * fh - f32(0.5)
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = x - x0, y - y0
    with np.errstate(invalid="ignore"):
        i0 = np.fmin(np.fmax(x0, f32(-1)), fw - f32(1)).astype(np.int64)
        r0 = np.fmin(np.fmax(y0, f32(0)), fh - f32(1)).astype(np.int64)
        r1 = np.fmin(np.fmax(y0 + f32(1), f32(0)), fh - f32(1)).astype(np.int64)
    c0 = np.where(i0 < 0, w - 1, i0)
    c1 = np.where(i0 + 1 >= w, 0, i0 + 1)
    t00, t10, t01, t11 = env[r0, c0, :3], env[r0, c1, :3], env[r1, c0, :3], env[r1, c1, :3]
    gx, gy = f32(1) - fx, f32(1) - fy
    w00, w10, w01, w11 = (gx * gy)[..., None], (fx * gy)[..., None], (gx * fy)[..., None], (fx * fy)[..., None]
    return ((((t00 * w00 + t10 * w10) + t01 * w01) + t11 * w11) * f32(intensity)).astype(f32)


def sky(dirs):
    """miss_kernel's gradient sky (mk:32-33) for directions (..., 3), the factor a miss applies without a map."""
    dy = np.asarray(dirs, f32)[..., 1]
    t = f32(0.5) * (dy + f32(1))
    om = f32(1) - t
    return np.stack([om * f32(1) + t * f32(0.5), om * f32(1) + t * f32(0.7), om * f32(1) + t * f32(1)], axis=-1).astype(f32)


def render_with_environment(o, env, params=None, spp=1, first_frame=1):
    """transport_ref.render with the map in place of the oracle's miss stage: at every miss the pixel's throughput is multiplied by the
    lookup (nothing touches it afterwards within the sample), and the samples are added to a float32 accumulator. The wrapper names no
    scene, so shade's albedo is the oracle's own. Returns the accumulated image (n_pixels x 3). env=None: the gradient sky (the oracle's
    own result)."""
    return render(o, env=env, env_params=params, spp=spp, first_frame=first_frame)
