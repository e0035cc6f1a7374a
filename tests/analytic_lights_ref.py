"""numpy float32 restatement of the analytic lights (WFPT_FLAG_ANALYTIC_LIGHTS, include/wfpt.h "Analytic lights"): point, spot and
directional lights beside the emitters of nee_ref.Lights, as one light list of N = n_l + n_a entries that transport_ref.render takes as
`lights=`. The emitter branch is nee_ref.Lights' own, with Nf = f32(N) wherever its nf stands; the analytic branch is the header's, one
IEEE f32 operation per step in its order. A directional sample has dist = +inf, with which nee_ref.occluded's t < dist * 0.999 is "any
hit": the oracle's extend is the walk with t_min = 0.001 and no far end. The host's normalisation of the directions (wfpt_set_lights) is
restated by `stored`."""
import numpy as np

import emission_ref as E
import mis_ref as M
import nee_ref as N
from transport_ref import dot3, f32, render

PI = N.PI
POINT, SPOT, DIRECTIONAL = 0, 1, 2
LIGHT = np.dtype([("position", "<f4", 3), ("type", "<u4"), ("direction", "<f4", 3), ("cos_inner", "<f4"),
                  ("colour", "<f4", 3), ("cos_outer", "<f4")])


def point(position, colour):
    l = np.zeros(1, LIGHT)
    l["position"], l["colour"], l["type"] = position, colour, POINT
    return l


def spot(position, direction, colour, cos_inner, cos_outer):
    l = point(position, colour)
    l["type"], l["direction"], l["cos_inner"], l["cos_outer"] = SPOT, direction, cos_inner, cos_outer
    return l


def directional(direction, colour):
    l = np.zeros(1, LIGHT)
    l["direction"], l["colour"], l["type"] = direction, colour, DIRECTIONAL
    return l


def stored(lights):
    """The lights as wfpt_set_lights stores them: the direction of a spot or directional light divided by
    len = sqrt((x x + y y) + z z), three divisions; a colour of -0 becomes +0; everything else as given."""
    out = np.array(np.atleast_1d(lights), LIGHT)
    d = out["direction"].astype(f32)
    with np.errstate(all="ignore"):
        ln = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        nd = d / ln[:, None]
    has_axis = out["type"] != POINT
    out["direction"] = np.where(has_axis[:, None], nd, d)
    out["colour"] = out["colour"] + f32(0)
    return out


class AnalyticLights:
    """The light list of a flagged context: the emitters of `em` (an emission_ref.Emission; its table all zero where no material emits)
    followed by the analytic lights `lights` (a LIGHT array as the caller hands it to wfpt_set_lights). The interface is nee_ref.Lights':
    n, sample, densities, hit_weight (and em, list for the row samplers of mis_ref).
    The mutations of tests/test_analytic_lights_host.py: nf_emitters_only (nf left at n_l), weigh_analytic (an analytic sample weighed by
    the balance heuristic against a density of its own making), sun_window (the sun's shadow ray ends at the distance to its unused
    position field), no_falloff (the spot's fall dropped)."""

    def __init__(self, em, lights=None, tx=None, nf_emitters_only=False, weigh_analytic=False, sun_window=False, no_falloff=False):
        self.em, self.tx = em, tx
        self.emitters = N.Lights(em, tx)
        self.list = self.emitters.list
        self.n_l = self.emitters.n
        self.lights = stored(lights) if lights is not None and len(lights) else np.zeros(0, LIGHT)
        self.n_a = len(self.lights)
        self.n = self.n_l + self.n_a
        self.nf = f32(self.n_l if nf_emitters_only else self.n)
        self.weigh_analytic, self.sun_window, self.no_falloff = weigh_analytic, sun_window, no_falloff

    # ---- selection
    def select(self, u0):
        """i (k,) in [0, N - 1]: min(u32(min(max(floor(u0 * Nf), 0), Nf)), N - 1), a NaN or negative u0 selects 0"""
        nf = f32(self.n)
        with np.errstate(all="ignore"):
            i = np.fmin(np.fmax(np.floor(np.asarray(u0, f32) * nf), f32(0)), nf).astype(np.int64)
        return np.minimum(i, self.n - 1)

    # ---- the analytic branch
    def sample_analytic(self, j, p, n):
        """lights j (k,) for receivers p, n (k, 3): the dict of nee_ref.Lights.sample, prim = -(1 + j)"""
        L = self.lights[j]
        c, a, e = L["position"].astype(f32), L["direction"].astype(f32), L["colour"].astype(f32)
        sun, is_spot = L["type"] == DIRECTIONAL, L["type"] == SPOT
        nf = self.nf
        with np.errstate(all="ignore"):
            v = c - p
            dist2 = dot3(v, v)
            dist = np.sqrt(dist2)
            wp = v / dist[:, None]
            w = np.where(sun[:, None], -a, wp).astype(f32)
            cos_s = dot3(n, w)
            cd = -dot3(a, wp)
            s = (cd - L["cos_outer"]) / (L["cos_inner"] - L["cos_outer"])
            s = np.where(s > 0, s, f32(0)).astype(f32)
            s = np.where(s < 1, s, f32(1)).astype(f32)
            fall = np.where(is_spot & (not self.no_falloff), (s * s) * (f32(3) - f32(2) * s), f32(1)).astype(f32)
            G = np.where(sun, (cos_s * nf) / PI, ((cos_s * fall) * nf) / (PI * dist2)).astype(f32)
            lit = (cos_s > 0) & (sun | ((dist2 > 0) & (fall > 0)))
        far = dist if self.sun_window else np.full(len(j), np.inf, f32)
        return {"q": np.where(sun[:, None], w, c).astype(f32), "prim": -(1 + j), "w": w, "dist": np.where(sun, far, dist).astype(f32),
                "e_q": e, "G": G, "lit": lit}

    # ---- nee_ref.Lights' interface
    def sample(self, p, n, u0, u1, u2):
        p, n = np.asarray(p, f32), np.asarray(n, f32)
        u1, u2 = np.asarray(u1, f32), np.asarray(u2, f32)
        k = len(p)
        i = self.select(u0)
        out = {"q": np.zeros((k, 3), f32), "prim": np.zeros(k, np.int64), "w": np.zeros((k, 3), f32), "dist": np.zeros(k, f32),
               "e_q": np.zeros((k, 3), f32), "G": np.zeros(k, f32), "lit": np.zeros(k, bool)}
        ie, ia = np.flatnonzero(i < self.n_l), np.flatnonzero(i >= self.n_l)
        if len(ie):
            # the point, the normal, the area, the cosines and e_q are Lights.sample's own: a draw u0' that makes its floor(u0' n_l) the light i
            s = self.emitters.sample(p[ie], n[ie], ((i[ie].astype(np.float64) + 0.5) / self.n_l).astype(f32), u1[ie], u2[ie])
            assert np.array_equal(s["prim"], self.list[i[ie]])
            with np.errstate(all="ignore"):  # G with Nf in nf's place, from the same cos_s, cos_l, A, dist2 (recomputed as light_power_ref does)
                nl, area = self.emitters.normal_area(s["prim"], s["q"])
                v = s["q"] - p[ie]
                dist2 = dot3(v, v)
                cos_s, cos_l = dot3(n[ie], s["w"]), np.abs(dot3(nl, s["w"]))
                s["G"] = ((((cos_s * cos_l) * area) * self.nf) / (PI * dist2)).astype(f32)
            for key in out:
                out[key][ie] = s[key]
        if len(ia):
            s = self.sample_analytic(i[ia] - self.n_l, p[ia], n[ia])
            for key in out:
                out[key][ia] = s[key]
        return out

    def densities(self, p, s, nf=None):
        """(pl, pb, wl): an emitter's with Nf; an analytic sample's pl = 0, pb = cos_s / pi, wl = 1"""
        p = np.asarray(p, f32)
        k = len(p)
        pl, pb, wl = np.zeros(k, f32), np.zeros(k, f32), np.ones(k, f32)
        an = s["prim"] < 0
        ie, ia = np.flatnonzero(~an), np.flatnonzero(an)
        if len(ie):
            sub = {key: np.asarray(val)[ie] for key, val in s.items()}
            pl[ie], pb[ie], wl[ie] = self.emitters.densities(p[ie], sub, self.nf if nf is None else nf)
        if len(ia):
            with np.errstate(all="ignore"):
                pb[ia] = dot3(np.asarray(s["n"], f32)[ia], s["w"][ia]) / PI
                if self.weigh_analytic:  # the mutation: as if the scatter could find the light, with the point light's 1 / dist2 as its density
                    v = s["q"][ia] - p[ia]
                    fake = f32(1) / dot3(v, v)
                    wl[ia] = fake / (fake + pb[ia])
        return pl, pb, wl

    def hit_weight(self, o, ph, d, prim, pb_of_len=None, with_nf=True, nf=None):
        """nee_ref.Lights.hit_weight with Nf in nf's place: the emission pass never sees an analytic light"""
        return self.emitters.hit_weight(o, ph, d, prim, pb_of_len, with_nf, self.nf if nf is None else nf)

    # ---- the row samplers
    def sample_rows(self, shadow, rows):
        """wfpt_sample_lights for rows (k, 9): (k, 8) of (q, primitive or -(1 + j), e_q G, occluded), and the samples"""
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

    def sample_rows_mis(self, shadow, rows):
        """wfpt_sample_lights_mis: mis_ref.sample_rows, with this list's densities"""
        return M.sample_rows(self, shadow, rows)

    def hit_weight_rows(self, rows):
        """wfpt_mis_hit_weight: mis_ref.hit_weight_rows, with Nf"""
        return M.hit_weight_rows(self, rows)


def no_emission(spheres=None, triangles=None, materials=None):
    """the Emission of a scene without an emitter: its table is zero"""
    return E.Emission({}, spheres=spheres, triangles=triangles, materials=materials)


def render_with_lights(o, shadow, em, lights, mis=False, tx=None, **kw):
    """transport_ref.render of a WFPT_FLAG_ANALYTIC_LIGHTS context: AnalyticLights as its light list (mis: the WFPT_FLAG_MIS context).
    lights: a LIGHT array, or an AnalyticLights (the host tests' mutations); the other keywords are render's."""
    al = lights if isinstance(lights, AnalyticLights) else AnalyticLights(em, lights, tx)
    return render(o, shadow=shadow, em=em, tx=tx, lights=al, weigh=mis, **kw)
