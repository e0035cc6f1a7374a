"""Scenes whose staged copy needs between 64 and 80 KiB of LDS ("The launch layer").

Such a scene is still staged in LDS (upload_scene), but every launch over it asks for more dynamic LDS than a kernel may use by default:
it fails unless the context raised the limit of exactly that instantiation when the scene was uploaded. Each case here reaches other
instantiations (loop, box test, miss payload, AOV, texture, connect, MIS and power variants) and asserts that the render equals, bit
for bit, the same inputs rendered with WFPT_FLAG_NO_LDS_SCENE, whose loops the other files check against the oracle. Every material
is finite (no dielectric), so every pixel is compared and none is left out."""
import numpy as np
import pytest

import capacity_ref as R
from test_gpu_nee import assert_bits, mesh_tracer, random_tex, sphere_tracer

pytestmark = pytest.mark.gpu

F = np.float32
W_, H_, SPP = 60, 44, 2  # neither side a multiple of 8: the INACT extend variants run
N_SPHERES = 900          # small ones; + the ground and the lamp
N_TRIANGLES = 650
GROUND, LAMBERT, METAL, LAMP = 0, 1, 2, 3  # material indices of the sphere scene
LAMP_COLOUR = (8.0, 6.0, 4.0)
AOV_NAMES = ("albedo", "normal", "depth", "coverage", "prim_id", "material_id")


@pytest.fixture(scope="module")
def W(gpu):
    return gpu


def sphere_scene(W):
    """A Lambertian ground sphere, N_SPHERES small spheres (Lambertian and fuzzy metal in turn) at seeded positions above it and one
    sphere of radius 0.5 whose material the lit cases make an emitter."""
    rng = np.random.default_rng(7)
    n = N_SPHERES + 2
    sp = np.zeros(n, W.SPHERE)
    mt = np.zeros(4, W.MATERIAL)
    mt["albedo"][:] = (0.5, 0.5, 0.5, 1.0)
    mt["albedo"][LAMBERT, :3] = (0.7, 0.3, 0.2)
    mt["albedo"][METAL, :3] = (0.8, 0.8, 0.6)
    mt["material_type"] = (0, 0, 1, 0)
    mt["fuzz"][METAL] = 0.3
    sp["center"][:, 3] = 1.0
    sp["center"][0, :3], sp["radius"][0], sp["material_idx"][0] = (0.0, -100.0, 0.0), 100.0, GROUND
    sp["center"][1:-1, 0] = rng.uniform(-4.0, 4.0, N_SPHERES)
    sp["center"][1:-1, 1] = rng.uniform(0.2, 2.0, N_SPHERES)
    sp["center"][1:-1, 2] = rng.uniform(-4.0, 4.0, N_SPHERES)
    sp["radius"][1:-1] = 0.2
    sp["material_idx"][1:-1] = np.where(np.arange(N_SPHERES) % 2 == 0, LAMBERT, METAL)
    sp["center"][-1, :3], sp["radius"][-1], sp["material_idx"][-1] = (0.0, 2.0, 0.0), 0.5, LAMP
    sp["material_type"] = mt["material_type"][sp["material_idx"]]
    return sp, mt


def flags_of(W, names):
    f = 0
    for n in (names.split("|") if names else []):
        f |= getattr(W, "FLAG_" + n)
    return f


def assert_window(pt, n_prims, triangles):
    n_nodes = len(pt.bvh_tree.nodes)
    b = R.scene_lds_bytes(n_nodes, n_prims, triangles)
    assert R.in_lds_window(n_nodes, n_prims, triangles), \
        f"{n_prims} primitives, {n_nodes} nodes: {b} B staged (+ {R.K_EXTEND_LDS_OWN}) is not within 64 .. 80 KiB: the premise of this test is gone"


def dress(W, pt, names, lamp_material):
    """What the flags of a case need bound before they do anything: a seeded 4 x 2 map, a seeded texture on the lamp's material, the lamp"""
    flags = set(names.split("|")) if names else set()
    if "ENVIRONMENT" in flags:
        pt.set_environment((np.random.default_rng(3).random((2, 4, 3)) * 1.5).astype(F))
    if "TEXTURES" in flags:
        pt.set_texture(0, random_tex(8, 4, 5))
        pt.bind_texture(lamp_material, 0)
    if "EMISSION" in flags:
        pt.set_emission(lamp_material, LAMP_COLOUR)
        if "NEE" in flags:
            assert pt.nee_light_count() >= 1


def outputs(pt, names):
    flags = set(names.split("|")) if names else set()
    out = {"accumulated": pt.accumulated()}
    if "AOV" in flags:
        out.update({k: pt.aov(k) for k in AOV_NAMES})
    if "ADAPTIVE" in flags:
        out.update(variance=pt.variance(), sample_counts=pt.sample_counts(), mean=pt.mean())
    return out


def assert_same(got, want, what):
    assert got.keys() == want.keys()
    for k in got:
        if got[k].dtype == np.uint32:
            assert np.array_equal(got[k], want[k]), f"{what}: {k}"
        else:
            assert_bits(got[k], want[k], f"{what}: {k}")


def check(W, make, names, rng_mode, loop, n_prims, triangles, lamp_material):
    res = {}
    for lds in (True, False):
        pt = make(max_wavefronts=4, miss_floor=0, rng_mode=rng_mode, flags=flags_of(W, names) | (0 if lds else W.FLAG_NO_LDS_SCENE))
        if lds:
            assert_window(pt, n_prims, triangles)
        dress(W, pt, names, lamp_material)
        if lds:
            assert pt.loop_kind == loop, (names, pt.loop_kind)  # (after the map, texture and lamp: they take part in the choice)
        pt.render(SPP)
        res[lds] = outputs(pt, names)
        pt.close()
    assert np.any(res[True]["accumulated"] != 0)
    assert_same(res[True], res[False], f"{names or 'no flags'}: LDS-resident against HBM-resident")


NEE = "EMISSION|NEE"
SPHERE_CASES = [
    ("", 0, "fused"), ("UNFUSED", 0, "stages"), ("EXACT_TRAVERSAL", 0, "fused"),
    ("ENVIRONMENT", 0, "fused"), ("ENVIRONMENT|UNFUSED", 0, "stages"),
    ("RETIRE", 0, "fused"), ("RETIRE|UNFUSED", 0, "stages"), ("ADAPTIVE", 0, "fused"),
    ("BINNING", 1, "fused_binned"),
    ("AOV", 0, "fused"), ("AOV|ENVIRONMENT", 0, "fused"), ("AOV|TEXTURES", 0, "fused"), ("AOV|TEXTURES|ENVIRONMENT", 0, "fused"),
    (NEE, 0, "fused"), (NEE + "|TEXTURES", 0, "fused"), (NEE + "|MIS", 0, "fused"),
    (NEE + "|ENVIRONMENT|ENV_NEE", 0, "fused"), (NEE + "|ENVIRONMENT|ENV_NEE|ENV_MIS", 0, "fused"),
    (NEE + "|LIGHT_POWER", 0, "fused"), (NEE + "|LIGHT_POWER|MIS", 0, "fused"),
]


@pytest.mark.parametrize("names,rng_mode,loop", SPHERE_CASES, ids=[c[0] or "plain" for c in SPHERE_CASES])
def test_spheres_in_the_window_equal_the_hbm_resident_render(W, names, rng_mode, loop):
    inputs = sphere_scene(W)

    def make(**kw):
        return sphere_tracer(W, inputs, (0.0, 6.0, 8.0), (0.0, 0.0, 0.0), 40.0, W_, H_, **kw)
    check(W, make, names, rng_mode, loop, N_SPHERES + 2, False, LAMP)


@pytest.mark.parametrize("names", ["", NEE], ids=["plain", NEE])
def test_mesh_in_the_window_equals_the_hbm_resident_render(W, names):
    def make(**kw):
        return mesh_tracer(W, W_, H_, n=N_TRIANGLES, **kw)
    check(W, make, names, 0, "fused", N_TRIANGLES, True, 0)  # the mesh's first material (Lambertian, a third of the triangles) emits
