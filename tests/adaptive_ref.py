"""numpy float32 restatement of adaptive sampling (WFPT_FLAG_ADAPTIVE, include/wfpt.h "Adaptive sampling"), on top of the existing
restatements: `Masked` wraps the Oracle a restatement drives (or another wrapper, such as retire_ref.Retiring) and, after generate_rays,
turns the rays of the pixels whose mask bit is clear into what the padding lanes of an odd-sized image are -- a zeroed ray with
pixel_idx = INACTIVE_PIXEL, its slot kept -- which the oracle's extend neither hits nor misses. `Sums` then adds the restatement's
per-sample values to the active pixels alone, and `criterion` / `dilate_tile` / `next_mask` restate wfpt_adaptive_update: every step one
IEEE f32 operation in the header's order, the dilation on the 64-bit word of one 8x8 tile."""
import numpy as np

from transport_ref import INACTIVE_PIXEL, BounceTables, f32

u32 = np.uint32
u64 = np.uint64
DEFAULTS = {"min_samples": 16, "max_samples": 0, "threshold": 0.05, "luminance_floor": 0.01, "dilate": 1}
COL0, COL7 = 0x0101010101010101, 0x8080808080808080
ALL = 0xFFFFFFFFFFFFFFFF


def params_of(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def luma(v):
    v = np.asarray(v, f32)
    return (f32(0.2126) * v[..., 0] + f32(0.7152) * v[..., 1]) + f32(0.0722) * v[..., 2]


def variance_resolve(s1, s2, count):
    """wfpt_read_variance on a flagged context: the variance of the mean's luminance with the pixel's own n, 0 where n == 0"""
    s1, s2, n = np.asarray(s1, f32), np.asarray(s2, f32), np.asarray(count, u32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        nf = n.astype(f32)
        mu = s1 / nf
        d = s2 / nf - mu * mu
        v = np.where(d > 0, d, f32(0)).astype(f32) / nf
    return np.where(n == 0, f32(0), v).astype(f32)


def criterion(s1, s2, count, params):
    """unconverged per pixel: the header's four lines. max(0, d) keeps a NaN d (d < 0 ? 0 : d), so a NaN anywhere fails `v <= tol * tol`
    and leaves the pixel unconverged; n == 0 gives 0 / 0."""
    p = params_of(**params)
    s1, s2, n = np.asarray(s1, f32), np.asarray(s2, f32), np.asarray(count, u32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        nf = n.astype(f32)
        mu = s1 / nf
        d = s2 / nf - mu * mu
        v = np.where(d < 0, f32(0), d).astype(f32) / nf
        tol = f32(p["threshold"]) * (mu + f32(p["luminance_floor"]))
        return ~((n >= u32(p["min_samples"])) & (v <= tol * tol))


def dilate_tile(word):
    """one pixel of dilation inside the 8x8 tile: the horizontal step, then the same step vertically (shifts of 8), in 64-bit arithmetic"""
    u = int(word) & ALL
    h = u | ((u << 1) & ALL & ~COL0) | ((u >> 1) & ~COL7)
    return (h | ((h << 8) & ALL) | (h >> 8)) & ALL


def dilate_tile_naive(word):
    """the same as a 2-D loop: bit ly * 8 + lx is set when any bit of its 3x3 neighbourhood, clipped to the tile, is"""
    u = int(word)
    out = 0
    for ly in range(8):
        for lx in range(8):
            hit = False
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    y, x = ly + dy, lx + dx
                    if 0 <= y < 8 and 0 <= x < 8 and (u >> (y * 8 + x)) & 1:
                        hit = True
            if hit:
                out |= 1 << (ly * 8 + lx)
    return out


# ---------------------------------------------------------------- the slab of a (band-sharded) context and its tiles
def slab_rows(h, tile_rank=0, tile_world=1):
    """rows of the context's slab: the whole image, or -- sharded -- whole 8-row bands (the last one may reach past the image)"""
    if tile_world <= 1:
        return h
    return (((h + 7) // 8 - tile_rank + tile_world - 1) // tile_world) * 8


def global_rows(h, tile_rank=0, tile_world=1):
    """the image row of every slab row"""
    r = np.arange(slab_rows(h, tile_rank, tile_world))
    return r if tile_world <= 1 else ((r // 8) * tile_world + tile_rank) * 8 + r % 8


def inside(w, h, tile_rank=0, tile_world=1):
    """per slab pixel: it lies inside the image"""
    return np.repeat(global_rows(h, tile_rank, tile_world) < h, w)


def to_words(per_pixel, w, h, tile_rank=0, tile_world=1):
    """a boolean per slab pixel -> one 64-bit word per 8x8 tile in generate_rays' tile order, bit ly * 8 + lx; lanes outside the slab clear"""
    rows = slab_rows(h, tile_rank, tile_world)
    tx, ty = (w + 7) // 8, (rows + 7) // 8
    a = np.zeros((ty * 8, tx * 8), bool)
    a[:rows, :w] = np.asarray(per_pixel, bool).reshape(rows, w)
    lanes = a.reshape(ty, 8, tx, 8).transpose(0, 2, 1, 3).reshape(ty * tx, 64)
    return np.packbits(lanes, axis=1, bitorder="little").view("<u8").reshape(-1)


def from_words(words, w, h, tile_rank=0, tile_world=1):
    rows = slab_rows(h, tile_rank, tile_world)
    tx, ty = (w + 7) // 8, (rows + 7) // 8
    lanes = np.unpackbits(np.ascontiguousarray(words, "<u8").view(np.uint8).reshape(ty * tx, 8), axis=1, bitorder="little").astype(bool)
    a = lanes.reshape(ty, tx, 8, 8).transpose(0, 2, 1, 3).reshape(ty * 8, tx * 8)
    return a[:rows, :w].reshape(-1)


def next_mask(s1, s2, count, params, w, h, tile_rank=0, tile_world=1):
    """wfpt_adaptive_update over a slab: (the next mask, one bool per slab pixel; n_active). Lanes outside the image are neither
    unconverged nor under the maximum."""
    p = params_of(**params)
    ins = inside(w, h, tile_rank, tile_world)
    n = np.asarray(count, u32)
    U = to_words(criterion(s1, s2, n, p) & ins, w, h, tile_rank, tile_world)
    under = to_words(((p["max_samples"] == 0) | (n < u32(p["max_samples"]))) & ins, w, h, tile_rank, tile_world)
    D = np.array([dilate_tile(x) for x in U], "<u8") if p["dilate"] else U
    words = D & under & to_words(ins, w, h, tile_rank, tile_world)
    mask = from_words(words, w, h, tile_rank, tile_world)
    return mask, int(mask.sum())


def all_active(w, h, tile_rank=0, tile_world=1):
    return inside(w, h, tile_rank, tile_world)


def local_pixel(pixel_idx, width, tile_rank=0, tile_world=1):
    """generate_rays' pixel_idx (x + y W of the image) -> the pixel's index in the context's slab"""
    pixel_idx = np.asarray(pixel_idx, np.int64)
    if tile_world <= 1:
        return pixel_idx
    y, x = pixel_idx // width, pixel_idx % width
    return ((y // 8 // tile_world) * 8 + y % 8) * width + x


# ---------------------------------------------------------------- the masked render
class Local:
    """A band-sharded Oracle as the restatements, which index their per-pixel arrays by the rays' pixel_idx, can drive it: rays() gives
    pixel_idx as the slab's own index. It goes outermost, around Masked."""

    def __init__(self, o):
        self.o = o

    def __getattr__(self, name):
        return getattr(self.o, name)

    def rays(self, n=None):
        P = self.o.params
        r = self.o.rays(n)
        live = r["pixel_idx"] != INACTIVE_PIXEL
        r["pixel_idx"][live] = local_pixel(r["pixel_idx"][live], self.o.width, P.tile_rank, P.tile_world).astype(u32)
        return r


class Masked(BounceTables):
    """An Oracle (or a wrapper around one) whose generate_rays obeys a mask: one bool per slab pixel, False = no ray. zero_only and drop
    are the two mutations of tests/test_adaptive_host.py: the masked rays zeroed but left with their pixel, and the masked slots dropped
    from the queue instead of kept. `bounce_table()` gives the last sample's rows (rays_in, hits, misses, shaded)."""

    def __init__(self, o, mask, zero_only=False, drop=False):
        super().__init__(o)
        self.mask = np.asarray(mask, bool).reshape(-1)
        self.zero_only, self.drop = zero_only, drop

    def local_pixel(self, pixel_idx):
        P = self.o.params
        return local_pixel(pixel_idx, self.o.width, P.tile_rank, P.tile_world)

    def generate_rays(self, gx, gy, true_size=False):
        o = self.o
        super().generate_rays(gx, gy, true_size)
        n = gx * gy * 64
        rays = o.rays(n)
        live = rays["pixel_idx"] != INACTIVE_PIXEL
        off = np.zeros(n, bool)
        off[live] = ~self.mask[self.local_pixel(rays["pixel_idx"][live])]
        if not off.any():
            return
        if self.drop:
            kept = rays[~off]
            o.write_rays(kept)
            c = o.counters()
            o.set_counters([c[0], c[1], len(kept)] + list(c[3:]))
            return
        pix = rays["pixel_idx"].copy()
        rays[off] = np.zeros((), rays.dtype)  # origin, direction and inverse direction: as the padding lanes have them
        rays["pixel_idx"] = pix if self.zero_only else np.where(off, u32(INACTIVE_PIXEL), pix)
        o.write_rays(rays)


class Sums:
    """`accumulated`, the luminance moments and the sample counts of a flagged context"""

    def __init__(self, n_pixels):
        self.acc = np.zeros((n_pixels, 3), f32)
        self.s1, self.s2 = np.zeros(n_pixels, f32), np.zeros(n_pixels, f32)
        self.count = np.zeros(n_pixels, u32)

    def add(self, parts, active):
        """the samples of a restatement's render (its parts=True dict) under the mask they were rendered with, in sample order"""
        a = np.asarray(active, bool).reshape(-1)
        for value in parts["value"]:
            L = luma(value)
            self.acc[a] = self.acc[a] + value[a]
            self.s1[a] = self.s1[a] + L[a]
            self.s2[a] = self.s2[a] + L[a] * L[a]
            self.count[a] += u32(1)
        return self

    def variance(self):
        return variance_resolve(self.s1, self.s2, self.count)

    def mean(self):
        with np.errstate(invalid="ignore", divide="ignore"):
            m = self.acc / self.count.astype(f32)[:, None]
        return np.where(self.count[:, None] == 0, f32(0), m).astype(f32)
