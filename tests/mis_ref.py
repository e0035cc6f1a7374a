"""numpy float32 restatement of multiple importance sampling (WFPT_FLAG_MIS, include/wfpt.h "Multiple importance sampling") on nee_ref's
pieces: the row samplers of wfpt_sample_lights_mis and wfpt_mis_hit_weight, and transport_ref.render with the connect sample weighed by wl,
the per-pixel `origin` plane, and the emission pass's weight wb where the connected flag is 1 (the densities and the weight are
nee_ref.Lights' methods, which a light list with its own nf overrides). Every step is one IEEE f32 operation in the header's order; the
shadow rays are traced through the second oracle, exactly as nee_ref does."""
import numpy as np

import nee_ref as N
from transport_ref import f32, render


def light_densities(lights, p, s):
    """(pl, pb, wl) of connect samples s = lights.sample(p, n, ...) with s["n"] = n -- the header's step 5, with the lights' own nf."""
    return lights.densities(p, s)


def hit_weight_rows(lights, rows):
    """wfpt_mis_hit_weight for rows (k, 8) of (o, d, t, primitive): (k, 4) of (pl, pb, wb, cos_l); a primitive that does not emit or is out
    of range (NaN included) answers (0, pb, 1, 0)."""
    rows = np.asarray(rows, f32)
    o, d, t, pf = rows[:, :3], rows[:, 3:6], rows[:, 6], rows[:, 7]
    n_prims = len(lights.em.prims())
    with np.errstate(all="ignore"):
        ph = o + t[:, None] * d
        inside = (pf >= 0) & (pf < f32(n_prims))
        prim = np.where(inside, pf, 0).astype(np.int64)
        emits = inside & np.isin(prim, lights.list)
        r = lights.hit_weight(o, ph, d, prim)
    out = np.stack([np.where(emits, r["pl"], f32(0)), r["pb"], np.where(emits, r["wb"], f32(1)), np.where(emits, r["cos_l"], f32(0))], 1)
    return out.astype(f32)


def sample_rows(lights, shadow, rows):
    """wfpt_sample_lights_mis for rows (k, 9) of (p, n, u0, u1, u2): (k, 12) of (q, primitive, (e_q G) wl, occluded, pl, pb, wl, 0)."""
    rows = np.asarray(rows, f32)
    p, n = rows[:, :3], rows[:, 3:6]
    s = lights.sample(p, n, rows[:, 6], rows[:, 7], rows[:, 8])
    s["n"] = n
    pl, pb, wl = light_densities(lights, p, s)
    lit = s["lit"]
    occ = np.zeros(len(rows), bool)
    occ[lit] = N.occluded(shadow, p[lit], s["w"][lit], s["dist"][lit])
    with np.errstate(all="ignore"):
        f = (s["e_q"] * s["G"][:, None]) * wl[:, None]
    z = f32(0)
    out = np.zeros((len(rows), 12), f32)
    out[:, :3] = s["q"]
    out[:, 3] = s["prim"].astype(f32)
    out[:, 4:7] = np.where(lit[:, None], f, z)
    out[:, 7] = occ
    out[:, 8], out[:, 9], out[:, 10] = np.where(lit, pl, z), np.where(lit, pb, z), np.where(lit, wl, z)
    return out


def render_with_mis(o, shadow, em, spp=1, first_frame=1, tx=None, env=None, env_params=None, parts=False, no_wl=False, no_wb=False,
                    no_nf=False, pb_of_len=None, scatters=None, termination=None):
    """nee_ref.render_with_nee with the two weights (the loop's `weighing`). With no light the loop selects no connect pass, so the flag
    does nothing. The mutations of tests/test_mis_host.py: no_wl (the connect sample at full weight), no_wb (the flagged emitter hit at
    full weight), no_nf (pl of the emission pass without the light count), pb_of_len (another density of the scatter from the direction's
    length). scatters: a list that receives, per wavefront, (normal, direction) of every extension ray a Lambertian non-emitter hit
    produced (the identity test's data)."""
    return render(o, shadow=shadow, em=em, tx=tx, env=env, env_params=env_params, lights=N.Lights(em, tx), weigh=True, termination=termination,
                  spp=spp, first_frame=first_frame, parts=parts, scatters=scatters, no_wl=no_wl, no_wb=no_wb, no_nf=no_nf, pb_of_len=pb_of_len)


# ---------------------------------------------------------------- the near-lamp scene
# An emitting sphere of radius 1 whose gap to the radius-1000 ground is 0.05 of its radius: under it the connect pass's 1 / dist2 is
# unbounded while half its samples lie on the lamp's far side; the scattered ray hits the lamp with high probability and a bounded weight.
NEAR = {"ground_r": 1000.0, "lamp_r": 1.0, "gap": 0.05, "albedo": (0.5, 0.75, 0.25), "e": (4.0, 2.0, 8.0)}


def near_lamp_inputs(orc, w, h, buried=False):
    """The radius-1000 Lambertian ground (material 0) under the near lamp (material 1), seen from above at an angle. Returns (spheres,
    materials, nodes, cam, inv_proj, view); the emitter's colour is NEAR["e"] for material 1. buried: a second sphere of material 1 deep
    inside the ground sphere. It lies below every ground point's tangent plane and no scattered ray can reach it, so it lights nothing:
    it only makes the light list two long (nf = 2), which the single lamp cannot."""
    sp = np.zeros(3 if buried else 2, orc.SPHERE)
    mt = np.zeros(2, orc.MATERIAL)
    mt["albedo"][:] = (0.5, 0.5, 0.5, 1.0)
    mt["albedo"][0, :3] = NEAR["albedo"]
    sp["center"][:, 3] = 1.0
    sp["center"][0, :3] = (0.0, -NEAR["ground_r"], 0.0)
    sp["radius"][0] = NEAR["ground_r"]
    sp["center"][1, :3] = (0.0, NEAR["lamp_r"] * (1.0 + NEAR["gap"]), 0.0)
    sp["radius"][1] = NEAR["lamp_r"]
    sp["material_idx"][:2] = (0, 1)
    if buried:
        sp["center"][2, :3] = (0.0, -0.5 * NEAR["ground_r"], 0.0)
        sp["radius"][2] = NEAR["lamp_r"]
        sp["material_idx"][2] = 1
    sp["material_type"] = mt["material_type"][sp["material_idx"]]
    sp, nodes = orc.build_bvh(sp)
    cam, ip, vw = orc.camera((0.0, 5.0, 7.0), (0.0, 0.0, 0.0), 40.0, 0.0, 10.0, 0.1, 100.0, w, h)
    return sp, mt, nodes, cam, ip, vw
