"""numpy restatement of light selection by power (WFPT_FLAG_LIGHT_POWER, include/wfpt.h "Light selection by power") on nee_ref's and
mis_ref's pieces: PowerLights is nee_ref.Lights with the light list's integer distribution (tables), the selection by it (sample: steps 3
and 4 with nfi = f32(total) / f32(k) in nf's place), and the densities and the hit weight with nfi in nf's place; transport_ref.render and
mis_ref's row samplers take it as their light list. Every step is one IEEE operation in the header's order (f64 in the selection alone)."""
import numpy as np

import mis_ref as M
import nee_ref as N
from denoise_ref import luma
from nee_ref import PI
from transport_ref import dot3, f32, render, triangle_normal_area

u64 = np.uint64


def light_areas(em, prim):
    """A of step 3 of "Next-event estimation" for primitives prim (k,), its operation order."""
    with np.errstate(all="ignore"):
        if em.triangles is None:
            ra = np.abs(em.spheres[prim]["radius"].astype(f32))
            return ((f32(4) * PI) * (ra * ra)).astype(f32)
        return triangle_normal_area(em.triangles[prim])[1].astype(f32)


class PowerLights(N.Lights):
    """nee_ref.Lights with the list's sampling distribution. has_distribution is False where the largest f is not a finite number above 0:
    such a list samples as nee_ref.Lights does. uniform_weight: the mutation of tests/test_light_power_host.py (the selection by power, the
    weight left at nf: the missing 1 / P)."""

    def __init__(self, em, tx=None, uniform_weight=False):
        super().__init__(em, tx)
        self.uniform_weight = uniform_weight
        t = self.tables() if self.n else None
        self.has_distribution = t is not None
        if t is not None:
            self.k, self.cdf, self.total, self.prim_k = t

    def weights(self):
        """f_i = L_i * A_i per light of the list, f32."""
        em = self.em
        e = em.table[em.prims()["material_idx"][self.list].astype(np.int64)].astype(f32)
        with np.errstate(all="ignore"):
            return (luma(e) * light_areas(em, self.list)).astype(f32)

    def tables(self):
        """(k (n_l,) uint32, cdf (n_l,) uint64, total, prim_k (n_prims,) uint32), or None where there is no distribution."""
        f = self.weights()
        pos = f > 0  # (a NaN is not)
        if not pos.any():
            return None
        m = f32(f[pos].max())
        if not (m > 0 and np.isfinite(m)):
            return None
        with np.errstate(all="ignore"):
            q = (np.where(pos, f, f32(0)) / m) * f32(65535.0)
        k = np.ceil(q).astype(np.uint32)
        k = np.where(pos & (k == 0), np.uint32(1), k)
        k = np.where(pos, k, np.uint32(0)).astype(np.uint32)
        cdf = np.cumsum(k.astype(u64), dtype=u64)
        prim_k = np.zeros(len(self.em.prims()), np.uint32)
        prim_k[self.list] = k
        return k, cdf, int(cdf[-1]), prim_k

    def select(self, u0):
        """(i, nfi) for draws u0 (k,): T = u64(floor(f64(u0) * f64(total))) clamped into [0, total - 1] (a NaN or negative product selects
        0), i the first index with cdf[i] > T, nfi = f32(total) / f32(k_i)."""
        u0 = np.asarray(u0, f32)
        ft = np.float64(self.total)
        with np.errstate(all="ignore"):
            tr = np.floor(u0.astype(np.float64) * ft)
        T = np.where(tr >= 0, np.where(tr < ft, tr, ft - 1), 0.0)  # (total < 2^53: the doubles are the integers)
        T = np.where(np.isnan(tr), 0.0, T).astype(u64)
        i = np.searchsorted(self.cdf, T, side="right").astype(np.int64)
        k = self.k[i]
        assert (k > 0).all()
        nfi = (np.full(len(i), self.total, u64).astype(f32) / k.astype(f32)).astype(f32)
        return i, nfi

    def sample(self, p, n, u0, u1, u2):
        """nee_ref.Lights.sample with the selection above and nfi in nf's place; the dict also holds nfi (k,)."""
        if not self.has_distribution:
            return super().sample(p, n, u0, u1, u2)
        i, nfi = self.select(u0)
        # the point, the normal, the area, the cosines and e_q are Lights.sample's own: a draw u0' that makes its floor(u0' nf) the light i
        s = super().sample(p, n, ((i.astype(np.float64) + 0.5) / self.n).astype(f32), u1, u2)
        assert np.array_equal(s["prim"], self.list[i])
        nf = f32(self.n)
        w = nf if self.uniform_weight else nfi
        with np.errstate(all="ignore"):
            # G = (((cos_s * cos_l) * A) * nfi) / (pi * dist2), from the same cos_s, cos_l, A, dist2 (recomputed as mis_ref does)
            nl, area = self.normal_area(s["prim"], s["q"])
            v = s["q"] - np.asarray(p, f32)
            dist2 = dot3(v, v)
            cos_s, cos_l = dot3(np.asarray(n, f32), s["w"]), np.abs(dot3(nl, s["w"]))
            s["G"] = ((((cos_s * cos_l) * area) * w) / (PI * dist2)).astype(f32)
        s["nfi"] = nfi
        return s

    def densities(self, p, s, nf=None):
        """nee_ref.Lights.densities with pl = dist2 / ((cos_l * A) * nfi), the sample's own nfi"""
        return super().densities(p, s, s["nfi"] if self.has_distribution else nf)

    def hit_weight(self, o, ph, d, prim, pb_of_len=None, with_nf=True, nf=None):
        """nee_ref.Lights.hit_weight with nfi = f32(total) / f32(prim_k[prim]) in nf's place; wb = 1 and pl = 0 where that k is 0."""
        if not self.has_distribution:
            return super().hit_weight(o, ph, d, prim, pb_of_len, with_nf, nf)
        prim = np.asarray(prim, np.int64)
        k = self.prim_k[prim]
        with np.errstate(all="ignore"):
            nfi = (np.full(len(prim), self.total, u64).astype(f32) / k.astype(f32)).astype(f32)
        r = super().hit_weight(o, ph, d, prim, pb_of_len, with_nf, nfi)
        r["pl"] = np.where(k == 0, f32(0), r["pl"]).astype(f32)
        r["wb"] = np.where(k == 0, f32(1), r["wb"]).astype(f32)
        return r

    def sample_rows(self, shadow, rows):
        """wfpt_sample_lights for rows (k, 9): (k, 8) of (q, primitive, e_q G, occluded)."""
        rows = np.asarray(rows, f32)
        s = self.sample(rows[:, :3], rows[:, 3:6], rows[:, 6], rows[:, 7], rows[:, 8])
        lit = s["lit"]
        occ = np.zeros(len(rows), bool)
        occ[lit] = N.occluded(shadow, rows[lit, :3], s["w"][lit], s["dist"][lit])
        out = np.zeros((len(rows), 8), f32)
        out[:, :3] = s["q"]
        out[:, 3] = s["prim"].astype(f32)
        with np.errstate(all="ignore"):
            out[:, 4:7] = np.where(lit[:, None], s["e_q"] * s["G"][:, None], f32(0))
        out[:, 7] = occ
        return out, s


def render_with_power(o, shadow, em, mis=False, tx=None, **kw):
    """nee_ref.render_with_nee (mis: mis_ref.render_with_mis) of a WFPT_FLAG_LIGHT_POWER context: transport_ref.render with PowerLights
    as its light list; the other keywords are theirs."""
    return render(o, shadow=shadow, em=em, tx=tx, lights=PowerLights(em, tx), weigh=mis, **kw)


def sample_rows_mis(lights, shadow, rows):
    """wfpt_sample_lights_mis on a flagged context: mis_ref.sample_rows, with lights' own densities."""
    return M.sample_rows(lights, shadow, rows)


def hit_weight_rows(lights, rows):
    """wfpt_mis_hit_weight on a flagged context: mis_ref.hit_weight_rows, with lights' own weight."""
    return M.hit_weight_rows(lights, rows)


# ---------------------------------------------------------------- the payoff scene
def indicator_inputs(orc, w, h, n_dim=63, seed=7, giant=False):
    """nee_ref's lamp scene with many dim lights: the radius-100 ground (material 0), one lamp of radius 0.5 (material 1) and n_dim spheres
    of radius 0.01 (material 2) scattered above the ground. giant: the last of them is a sphere of radius 2e19 centred 3e19 below the
    ground instead -- it encloses nothing and ra ra overflows. Returns (spheres, materials, nodes, cam, inv_proj, view)."""
    rng = np.random.default_rng(seed)
    sp = np.zeros(2 + n_dim, orc.SPHERE)
    mt = np.zeros(3, orc.MATERIAL)
    mt["albedo"][:] = (0.5, 0.5, 0.5, 1.0)
    mt["albedo"][0, :3] = N.LAMP["albedo"]
    sp["center"][:, 3] = 1.0
    sp["center"][0, :3] = (0.0, -N.LAMP["ground_r"], 0.0)
    sp["radius"][0] = N.LAMP["ground_r"]
    sp["center"][1, :3] = N.LAMP["lamp_c"]
    sp["radius"][1] = 0.5
    sp["material_idx"][:2] = (0, 1)
    sp["center"][2:, 0] = rng.uniform(-4.0, 4.0, n_dim)
    sp["center"][2:, 1] = rng.uniform(0.5, 3.0, n_dim)
    sp["center"][2:, 2] = rng.uniform(-4.0, 4.0, n_dim)
    sp["radius"][2:] = 0.01
    sp["material_idx"][2:] = 2
    if giant:
        sp["center"][-1, :3] = (0.0, -3e19, 0.0)
        sp["radius"][-1] = 2e19
    sp["material_type"] = mt["material_type"][sp["material_idx"]]
    sp, nodes = orc.build_bvh(sp)
    cam, ip, vw = orc.camera((0.0, 6.0, 8.0), (0.0, 0.0, 0.0), 40.0, 0.0, 10.0, 0.1, 100.0, w, h)
    return sp, mt, nodes, cam, ip, vw


INDICATOR_COLOURS = {1: (16.0, 16.0, 16.0), 2: (0.1, 0.1, 0.1)}
