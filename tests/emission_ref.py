"""numpy float32 restatement of emissive materials (WFPT_FLAG_EMISSION, include/wfpt.h "Emission"): a whole render driven through the
oracle's stages by transport_ref.render, which keeps the per-pixel throughput and the second per-sample plane: the emission pass between
the texture factor and shade's albedo; every step is one IEEE f32 operation, so the results are the device's bits."""
import numpy as np

from transport_ref import f32, render

COLOUR = (0.5, 2.0, 0.25)  # power-of-two channels: thr * e and the sums of a few samples are exact


class Emission:
    """What an emitting context holds: colours {material_idx: (r, g, b)}, and the scene's primitives as the device holds them (spheres or
    triangles) and materials. pass_first=True and keep_throughput=True are the two wrong orders the mutation checks of
    tests/test_emission_host.py use (emission before the texture pass; thr left as it was)."""

    def __init__(self, colours, spheres=None, triangles=None, materials=None, pass_first=False, keep_throughput=False):
        self.spheres, self.triangles, self.materials = spheres, triangles, materials
        self.table = np.zeros((len(materials), 3), f32)
        for m, c in dict(colours).items():
            self.table[int(m)] = np.asarray(c, f32)
        self.pass_first, self.keep_throughput = pass_first, keep_throughput

    def prims(self):
        return self.spheres if self.triangles is None else self.triangles

    def colour(self, prim):
        """(e (n, 3), emitter mask (n,)) of hits on primitives prim (n,)."""
        e = self.table[self.prims()["material_idx"][prim].astype(np.int64)]
        return e, (e != 0).any(axis=1)


def render_with_emission(o, em, spp=1, first_frame=1, tx=None, env=None, env_params=None, parts=False, termination=None):
    """transport_ref.render with the emission pass of kind `all`: at every hit whose material emits emitted <- emitted + thr * e and
    thr <- +0, after the texture pass (where tx binds the material) and before shade's albedo. The sample's value is thr + emitted.
    Returns the accumulated image (n_pixels x 3); with parts=True the loop's dict."""
    return render(o, em=em, tx=tx, env=env, env_params=env_params, termination=termination, spp=spp, first_frame=first_frame, parts=parts)


def furnace_inputs(orc, w, h):
    """closed_room_inputs("centre") with the two small spheres moved behind the camera: the camera at the centre of one closed sphere of
    radius 5 (material 0), looking down -z, so that every primary ray meets that sphere first."""
    sp = np.zeros(3, orc.SPHERE)
    mt = np.zeros(3, orc.MATERIAL)
    mt["albedo"][:] = (0.9, 0.8, 0.7, 1.0)
    mt["material_type"] = (1, 0, 2)
    mt["refract_index"][2] = 1.5
    sp["center"][:, 3] = 1.0
    sp["radius"] = (5.0, 0.5, 0.25)
    sp["center"][1, :3] = (1.5, 0.0, 3.0)
    sp["center"][2, :3] = (-1.5, 0.5, 3.0)
    sp["material_idx"] = (0, 1, 2)
    sp["material_type"] = mt["material_type"]
    sp, nodes = orc.build_bvh(sp)
    cam, ip, vw = orc.camera((0.0, 0.0, 0.0), (0.5, 0.0, -1.0), 70.0, 0.0, 10.0, 0.1, 100.0, w, h)
    return sp, mt, nodes, cam, ip, vw
