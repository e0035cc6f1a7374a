"""numpy float32 restatement of the environment map (WFPT_FLAG_ENVIRONMENT) in the kernels' operation order: normalize3, atan2_ and the
bilinear lookup of wfpt_device_math.h, and a whole lit render driven through the oracle's stages with the map applied where miss_kernel would
colour a miss. Every step is one IEEE f32 operation (numpy float32 rounds each one as the device does with -ffp-contract=off), so the results
are the device's bits."""
import numpy as np

f32 = np.float32
INV_2PI = f32(0.15915494)
INV_PI = f32(0.31830988)
TAN_PI_8 = f32(0.41421356)
ATAN_HALF = (f32(4.636476040e-01), f32(5.012158688e-09))  # atan(1/2), pi/2, pi as hi + lo
PI_2 = (f32(1.570796371e+00), f32(-4.371138829e-08))
PI = (f32(3.141592741e+00), f32(-8.742277657e-08))
C3, C2, C1, C0 = f32(8.05374449538e-2), f32(1.38776856032e-1), f32(1.99777106478e-1), f32(3.33329491539e-1)


def normalize3(x, y, z):
    x, y, z = (np.asarray(v, f32) for v in (x, y, z))
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = f32(1.0) / np.sqrt((x * x + y * y) + z * z)
    return x * inv, y * inv, z * inv


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
    """The oracle's per-sample loop (orc_render_sample) driven from Python, with the map in place of its miss stage: generate_rays, then per
    wavefront extend, the miss_floor exit, shade, and -- instead of miss -- the pixel and direction of every miss are recorded; swap. Nothing
    touches a pixel's throughput after its miss within a sample, so the recorded pixels of image() are multiplied by the lookup at the end
    of the sample, and the sample is added to a float32 accumulator. Returns the accumulated image (n_pixels x 3). env=None: the gradient sky
    (the oracle's own result)."""
    from oracle import oracle as O
    params = dict(params or {})
    intensity, rotation = params.get("intensity", 1.0), params.get("rotation", 0.0)
    p = o.params
    gx = (o.width + 7) // 8
    gy = ((o.height + 7) // 8 - p.tile_rank + p.tile_world - 1) // p.tile_world
    acc = np.zeros((o.n_pixels, 3), f32)
    for k in range(spp):
        o.set_frame(first_frame + k, 0)
        o.reset_image()
        o.set_counters([0, 0, gx * gy * 64])
        o.generate_rays(gx, gy, True)
        ex, ey = O.workgroup_size_64(gx * gy * 64)
        pix, dirs = [], []
        for _ in range(p.max_wavefronts):
            n_rays = int(o.counters()[2])
            o.extend(ex, ey)
            c = o.counters()
            n_miss, n_hit = int(c[0]), int(c[1])
            if n_miss < p.miss_floor:
                break
            if n_miss:
                rays = o.rays(max(n_rays, 1))
                idx = o.misses(n_miss)
                pix.append(rays["pixel_idx"][idx].astype(np.int64))
                dirs.append(rays["direction"][idx, :3].astype(f32))
            o.set_counters([c[0], c[1], 0] + list(c[3:]))
            sx, sy = O.workgroup_size_64(n_hit)
            o.shade(sx, sy)
            n_ext = int(o.counters()[2])
            o.swap_ray_queues()
            ex, ey = O.workgroup_size_64(n_ext)
            o.set_counters([0, 0, n_ext])
        img = o.image().copy()
        if pix:
            px, d = np.concatenate(pix), np.concatenate(dirs)
            f = sky(d) if env is None else env_lookup(env, d, intensity, rotation)
            img[px] = img[px] * f
        acc = acc + img
    return acc
