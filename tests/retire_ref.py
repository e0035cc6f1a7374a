"""numpy float32 restatement of path termination (WFPT_FLAG_RETIRE, include/wfpt.h "Path termination"), on top of the existing
restatements so that textures, emission, NEE and MIS compose: transport_ref.render takes a `Retiring` as its termination= (every
render_with_* passes the keyword on). Before the shade of every wavefront b with b + 1 < max_wavefronts (step 1), with t' = thr * albedo
formed, the loop hands it thr and the hits' pixels; `retire` applies steps 2 and 3 in place, and after the queue swap the loop sets
pixel_idx = INACTIVE_PIXEL on the retired hits' extension rays and writes them back with write_rays -- the oracle's extend skips such
rays. Every step is one IEEE f32 operation in the header's order."""
import numpy as np

from nee_ref import jenkins_hash, rng_next_float
from transport_ref import BounceTables, f32

u32 = np.uint32
NO_ROULETTE = 0xFFFFFFFF
DEAD, ROULETTE, SURVIVES = 0, 1, 2
DEFAULTS = {"roulette_start": 3, "q_min": 0.05}


def termination_draw(pixel_idx, frame, b):
    """u of the termination step for pixels pixel_idx (x + y W) in the sample of frame `frame`, wavefront b: a stream of the step's own."""
    s = jenkins_hash(np.asarray(pixel_idx, u32) ^ jenkins_hash(u32(frame)))
    s = jenkins_hash(s ^ u32((0x85EBCA6B * ((int(b) + 1) & 0xFFFFFFFF)) & 0xFFFFFFFF))
    u, _ = rng_next_float(s)
    return u


def decide(t, pixel_idx, frame, b, roulette_start=DEFAULTS["roulette_start"], q_min=DEFAULTS["q_min"], u=None, no_divide=False,
           keep_retired=False):
    """Steps 2 and 3 for rows t (n, 3) of t' = thr * albedo. Returns (thr' (n, 3), verdict (n,), q (n,), u (n,)); q and u are 0 where
    nothing is drawn. u: the draws to use instead of the stream's (hand-made rows). no_divide / keep_retired: the two mutations of
    tests/test_retire_host.py (the survivor not divided by q; the retired thr left as t')."""
    t = np.array(t, f32).reshape(-1, 3)
    n = len(t)
    pixel_idx = np.broadcast_to(np.asarray(pixel_idx, u32), (n,))
    out = t.copy()
    verdict = np.full(n, SURVIVES, np.int64)
    q_out, u_out = np.zeros(n, f32), np.zeros(n, f32)
    dead = (t[:, 0] == 0) & (t[:, 1] == 0) & (t[:, 2] == 0)  # (-0 == 0; a NaN channel compares false)
    verdict[dead] = DEAD
    if int(roulette_start) == NO_ROULETTE or int(b) < int(roulette_start):
        return out, verdict, q_out, u_out
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = t[:, 0].copy()
        m = np.where(t[:, 1] > m, t[:, 1], m)
        m = np.where(t[:, 2] > m, t[:, 2], m)
        q = np.where(m >= f32(q_min), m, f32(q_min)).astype(f32)  # (a NaN m gives q_min)
        plays = ~dead & ~(q >= f32(1))
        draws = termination_draw(pixel_idx, frame, b) if u is None else np.broadcast_to(np.asarray(u, f32), (n,))
        q_out[plays], u_out[plays] = q[plays], draws[plays]
        lives = plays & (draws < q)
        dies = plays & ~(draws < q)
        if not no_divide:
            out[lives] = t[lives] / q[lives][:, None]
        if not keep_retired:
            out[dies] = f32(0)
        verdict[dies] = ROULETTE
    return out, verdict, q_out, u_out


def sample_rows(thr, pixel_idx, frame, b, roulette_start=DEFAULTS["roulette_start"], q_min=DEFAULTS["q_min"]):
    """wfpt_sample_termination's rows: (q, u, verdict, 0, thr'.rgb, 0)."""
    out, verdict, q, u = decide(thr, pixel_idx, frame, b, roulette_start, q_min)
    rows = np.zeros((len(out), 8), f32)
    rows[:, 0], rows[:, 1], rows[:, 2] = q, u, verdict.astype(f32)
    rows[:, 4:7] = out
    return rows


# ---------------------------------------------------------------- the lamp room
ROOM = {"room_r": 5.0, "lamp_c": (1.5, 1.0, -2.0), "lamp_r": 1.0, "albedo": (0.5, 0.75, 0.25), "e": (4.0, 2.0, 8.0)}


def lamp_room_inputs(orc, w, h):
    """A closed sphere of fuzzy metal (material 0; a Lambertian wall would scatter about its outward normal, out of the room) lit from
    inside by an emitting sphere (material 1), the camera inside: next to no ray misses, so with miss_floor = 0 a path ends at the lamp,
    by roulette or at max_wavefronts. A smaller Lambertian sphere (material 2) stands in view. Returns (spheres, materials, nodes, cam, inv_proj, view); the emitter's colour is ROOM["e"] for material 1."""
    sp = np.zeros(3, orc.SPHERE)
    mt = np.zeros(3, orc.MATERIAL)
    mt["albedo"][:] = (0.5, 0.5, 0.5, 1.0)
    mt["albedo"][0, :3] = ROOM["albedo"]
    mt["albedo"][2, :3] = (0.75, 0.5, 0.5)
    mt["material_type"] = (1, 0, 0)
    mt["fuzz"][0] = 0.25
    sp["center"][:, 3] = 1.0
    sp["radius"] = (ROOM["room_r"], ROOM["lamp_r"], 0.5)
    sp["center"][1, :3] = ROOM["lamp_c"]
    sp["center"][2, :3] = (-1.0, -0.5, -2.5)
    sp["material_idx"] = (0, 1, 2)
    sp["material_type"] = mt["material_type"]
    sp, nodes = orc.build_bvh(sp)
    cam, ip, vw = orc.camera((0.5, 0.25, 1.0), (0.5, 0.0, -1.0), 70.0, 0.0, 10.0, 0.1, 100.0, w, h)
    return sp, mt, nodes, cam, ip, vw


class Retiring(BounceTables):
    """The termination step of a context, as transport_ref.render takes it (termination=), around the Oracle it renders with (o, whose
    bounce tables it keeps). roulette_start, q_min: the context's parameters; no_divide, keep_retired: decide()'s mutations. After a
    render, `tables` holds one bounce table per sample, rows (rays_in, hits, misses, shaded) as wfpt_read_bounce_table gives them, and
    `retired` the number of hits retired per sample and wavefront."""

    def __init__(self, o, roulette_start=DEFAULTS["roulette_start"], q_min=DEFAULTS["q_min"], no_divide=False, keep_retired=False):
        super().__init__(o)
        self.roulette_start, self.q_min = roulette_start, q_min
        self.no_divide, self.keep_retired = no_divide, keep_retired
        self.retired = []

    def generate_rays(self, gx, gy, true_size=False):
        super().generate_rays(gx, gy, true_size)
        self.retired.append([])

    def retire(self, thr, hp, frame, b):
        """Steps 2 and 3 on thr (n_pixels, 3), in place, for the hits of wavefront b at pixels hp -- the loop calls it where step 1 allows,
        after thr <- thr * albedo. Returns the mask of the retired hits."""
        out, verdict, _, _ = decide(thr[hp], hp, frame, b, self.roulette_start, self.q_min, no_divide=self.no_divide,
                                    keep_retired=self.keep_retired)
        thr[hp] = out
        gone = verdict != SURVIVES
        self.retired[-1].append(int(gone.sum()))
        return gone
