"""numpy float32 restatement of roughness maps (WFPT_FLAG_ROUGHNESS_MAPS, include/wfpt.h "Roughness maps"): steps R1-R5 at a hit, and
`RoughMapped`, rough_dielectric_ref.RoughGlass whose extend() samples every rough hit with its own alpha -- the material's times the
bound map's factor -- and leaves a hit whose alpha is not above 0 to the unchanged shade step. Every step is one IEEE f32 operation in the
header's order, so the results are the device's bits. The scene of the tests is normal_map_ref.sphere_scene; the test map is here."""
import numpy as np

import microfacet_ref as MF
import rough_dielectric_ref as RD
import shading_normals_ref as S
import texture_ref as T
from transport_ref import f32, triangle_normal_area

REMAPS = ("linear", "squared")
MUTATIONS = ("wrong_channel", "no_clamp", "no_square", "sample_alpha_m")
CLASSES = tuple((kind, texel) for kind in ("metal", "glass") for texel in ("zero", "above_one", "between"))


def hit_roughness(alpha_m, c, channel, remap, wrong_channel=False, no_clamp=False, no_square=False):
    """Steps R3-R4 for k hits: alphas alpha_m (k,), texels c (k, 3), one channel (0, 1, 2) and remap ("linear" | "squared" | 0 | 1) for
    all. Returns (alpha_h, r). The keywords are the mutations of tests/test_roughness_map_host.py."""
    alpha_m = np.asarray(alpha_m, f32).reshape(-1)
    c = np.asarray(c, f32).reshape(-1, 3)
    squared = remap in ("squared", 1)
    assert squared or remap in ("linear", 0), remap
    with np.errstate(all="ignore"):
        r = c[:, (channel + 1) % 3 if wrong_channel else channel]
        if not no_clamp:
            r = np.fmin(r, f32(1))
        if squared and not no_square:
            r = r * r
        return (alpha_m * r).astype(f32), r.astype(f32)


class Roughness:
    """What a context with roughness bindings holds beside its alphas: the triangles as the device holds them (rows named by _pad), the
    UV table (n, 6) or None, the slots {slot: (img, params)} as texture_ref.Textures takes them and the bindings
    {material_idx: (slot, channel, remap)}."""

    def __init__(self, triangles, uv, slots, bind, **mutations):
        unknown = set(mutations) - set(MUTATIONS)
        assert not unknown, unknown
        self.triangles = triangles
        self.uv = None if uv is None else np.asarray(uv, f32).reshape(-1, 6)
        self.slots, self.bind = dict(slots), dict(bind)
        self.mutations = {k: v for k, v in mutations.items() if k != "sample_alpha_m"}

    def at(self, prim, p, alpha_m):
        """(alpha_h (k,), r (k,), code (k,), texel (k,)) of hits at p on triangles prim whose step R1 alpha is alpha_m: the probe's codes 0-3;
        texel is the bound channel's value where a lookup happened, NaN elsewhere."""
        prim = np.asarray(prim, np.int64).reshape(-1)
        p = np.asarray(p, f32).reshape(-1, 3)
        alpha_m = np.asarray(alpha_m, f32).reshape(-1)
        t = self.triangles[prim]
        k = len(prim)
        rough = alpha_m > 0                                                     # R1.
        alpha = np.where(rough, alpha_m, f32(0)).astype(f32)
        r = np.where(rough, f32(1), f32(0)).astype(f32)
        code = np.where(rough, 1, 2).astype(np.int64)                           # R2.
        texel = np.full(k, np.nan, f32)
        mat = t["material_idx"].astype(np.int64)
        rows = np.zeros((k, 6), f32) if self.uv is None else self.uv[t["_pad"].astype(np.int64)]
        for m, (slot, channel, remap) in self.bind.items():
            sel = rough & (mat == m)
            if not sel.any():
                continue
            img, params = self.slots[slot]
            u, v = T.triangle_uv(p[sel], t["v0"][sel], t["e1"][sel], t["e2"][sel], rows[sel])  # R3.
            c = T.tex_lookup(img, u, v, **params)
            alpha[sel], r[sel] = hit_roughness(alpha_m[sel], c, channel, remap, **self.mutations)  # R3-R4.
            texel[sel] = np.asarray(c, f32).reshape(-1, 3)[:, channel]
            code[sel] = np.where(alpha[sel] > 0, 0, 3)
        return alpha, r, code, texel


def step_r1(triangles, alphas, glass):
    """alpha_m per triangle: the material's alpha where the triangle is a metal or, on a WFPT_FLAG_ROUGH_DIELECTRIC context (glass), a
    dielectric; +0 otherwise. alphas: (n_materials,) float32."""
    counts = (triangles["material_type"] == 1) | (glass & (triangles["material_type"] == 2))
    return np.where(counts, alphas[triangles["material_idx"].astype(np.int64)], f32(0)).astype(f32)


def sample_rows(rmap, alphas, p, prim, glass=True):
    """wfpt_sample_roughness_map's rows for points p on triangles prim (indices into rmap.triangles): (alpha_h | r | code | 0)."""
    prim = np.asarray(prim, np.int64).reshape(-1)
    alpha, r, code, _ = rmap.at(prim, p, step_r1(rmap.triangles[prim], np.asarray(alphas, f32), glass))
    return np.stack([alpha, r, code.astype(f32), np.zeros(len(prim), f32)], 1).astype(f32)


class RoughMapped(RD.RoughGlass):
    """rough_dielectric_ref.RoughGlass on a roughness-mapped context. rmap: a Roughness over the same triangles; glass: the context holds
    WFPT_FLAG_ROUGH_DIELECTRIC (False: the alphas of dielectrics are inert, microfacet_ref.Rough's rule); sample_alpha_m: the mutation
    that classifies by alpha_h and samples with alpha_m. classes: the hits that looked a texel up, by CLASSES."""

    def __init__(self, o, triangles, materials, alphas, rmap, normals=None, glass=True, sample_alpha_m=False):
        super().__init__(o, triangles, materials, alphas, normals)
        self.rmap, self.with_glass, self.sample_alpha_m = rmap, glass, sample_alpha_m
        self.classes = {c: 0 for c in CLASSES}

    def extend(self, gx, gy):
        S.Shaded.extend(self, gx, gy)
        self.cur = self.glass = None
        b = len(self.tables[-1]) - 1
        if b + 1 >= self.o.params.max_wavefronts:  # the pass does not run before the last wavefront's step
            return
        n_hit = int(self.o.counters()[1])
        if n_hit == 0:
            return
        hits = self.o.hits(n_hit)
        rays = self.o.rays()[hits["ray_idx"].astype(np.int64)]
        prim = hits["sphere_idx"].astype(np.int64)
        org, d = rays["origin"][:, :3].astype(f32), rays["direction"][:, :3].astype(f32)
        pt = org + hits["t"].astype(f32)[:, None] * d  # sh:91
        t = self.triangles[prim]
        midx = t["material_idx"].astype(np.int64)
        n = self.normals.at(prim, pt)[0] if self.normals is not None else triangle_normal_area(t)[0]
        alpha_m = step_r1(t, self.alpha, self.with_glass)
        alpha_h, _, _, texel = self.rmap.at(prim, pt, alpha_m)
        rough = alpha_h > 0                                                     # R5.
        alpha_s = alpha_m if self.sample_alpha_m else alpha_h
        for kind, type_ in (("metal", 1), ("glass", 2)):
            looked = ~np.isnan(texel) & (t["material_type"] == type_)
            self.classes[(kind, "zero")] += int((looked & (texel == 0)).sum())
            self.classes[(kind, "above_one")] += int((looked & (texel > 1)).sum())
            self.classes[(kind, "between")] += int((looked & (texel > 0) & (texel < 1)).sum())
        ok = np.zeros(n_hit, bool)
        m, weight = np.zeros((n_hit, 3), f32), np.zeros((n_hit, 3), f32)
        sel = rough & (t["material_type"] == 1)
        if sel.any():
            u1, u2 = MF.draws(rays["pixel_idx"][sel], self.frame, b)
            f0 = np.asarray(self.materials["albedo"][midx[sel], :3], f32)
            r = MF.sample(d[sel], n[sel], u1, u2, alpha_s[sel], f0)
            ok[sel] = ~r["fell"]
            m[sel], weight[sel] = r["m"], r["weight"]
            self.sampled += int((~r["fell"]).sum())
        glass = np.zeros(n_hit, bool)
        sel = rough & (t["material_type"] == 2)
        if sel.any():
            u1, u2, u3 = RD.draws(rays["pixel_idx"][sel], self.frame, b)
            mat = self.materials[midx[sel]]
            r = RD.sample(d[sel], n[sel], u1, u2, u3, alpha_s[sel], mat["refract_index"], np.asarray(mat["albedo"][:, :3], f32))
            live = ~r["fell"]
            glass[sel] = ok[sel] = live
            m[sel], weight[sel] = r["h"], r["weight"]
            self.glass_sampled += int(live.sum())
            for arm, a in (("reflect", ~r["refracted"]), ("refract", r["refracted"])):
                for side, s in (("outside", ~r["inside"]), ("inside", r["inside"])):
                    self.counts[(arm, side)] += int((live & a & s).sum())
        self.cur = {"ok": ok, "m": m, "weight": weight, "n": n}
        self.glass = glass


# ---------------------------------------------------------------- the maps of the tests
def stripe_map(seed=9, w=16, h=8):
    """A seeded (h, w, 3) float32 map: in channel ch, column x with k = (x + ch) % 4 holds exactly 0 for k < 2, U(1, 1.5) for k == 2 and
    U(0.05, 1) for k == 3. The two-column zero stripes make bilinear lookups land on exact zeros too."""
    rng = np.random.default_rng(seed)
    img = np.zeros((h, w, 3), f32)
    x = np.arange(w)
    for ch in range(3):
        low, high = rng.uniform(0.05, 1.0, (h, w)), rng.uniform(1.0, 1.5, (h, w))
        k = (x + ch) % 4
        img[:, :, ch] = np.where(k[None, :] < 2, 0.0, np.where(k[None, :] == 2, high, low))
    return img


def constant_map(value, w=4, h=2):
    img = np.zeros((h, w, 3), f32)
    img[:] = value
    return img


def probe_rows(p, prim):
    return S.probe_rows(p, prim)
