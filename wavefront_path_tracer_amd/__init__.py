"""wavefront_path_tracer_amd -- host-side mirror of the reference's API for ONE path:
the wavefront kernel chain generate_rays -> extend -> shade -> miss_kernel -> accumulate.

Everything here is a thin layer over the C ABI in include/wfpt.h (libwfpt.so: hand-written gfx950 HIP
kernels). Class and method names follow the reference (rchiaramo/wavefront_path_tracer @ 2024_10_08):

    Scene, Material, Sphere        wavefront_common/src/{scene,material,sphere}.rs
    BVHTree                        wavefront_common/src/bvh.rs
    Camera, CameraController       wavefront_common/src/{camera,camera_controller}.rs
    ProjectionMatrix               wavefront_common/src/projection_matrix.rs
    GPUFrameBuffer                 wavefront_common/src/gpu_structs.rs
    RenderParameters/RenderProgress wavefront_common/src/parameters.rs
    Kernel                         gpu_wavefront_pt/src/kernel.rs
    PathTracer                     gpu_wavefront_pt/src/path_tracer.rs

There is no CPU fallback: if libwfpt.so is missing or no MI355X is visible, device calls raise WfptError.
"""
import ctypes as C
import os

import numpy as np

from . import _build

__all__ = ["SPP", "SPF", "Scene", "BVHTree", "Camera", "CameraController", "ProjectionMatrix", "GPUFrameBuffer",
           "RenderParameters", "RenderProgress", "Kernel", "PathTracer", "WfptError", "workgroup_size_64",
           "RNG_DISPATCH", "RNG_PIXEL", "FLAG_SPLIT_SHADE", "FLAG_NO_GRAPH", "FLAG_UNFUSED", "FLAG_BINARY_BVH", "FLAG_NO_REFILL", "FLAG_NO_LDS_SCENE", "FLAG_EXACT_TRAVERSAL", "FLAG_NO_BINNING", "FLAG_BINNING", "FLAG_AOV", "AOVS", "FLAG_DENOISE", "DENOISE_DEFAULTS", "FLAG_ENVIRONMENT", "load_environment", "FLAG_TEXTURES", "MAX_TEXTURES", "load_texture", "FLAG_EMISSION", "FLAG_NEE", "FLAG_ENV_NEE", "FLAG_MIS", "FLAG_ENV_MIS", "FLAG_LIGHT_POWER", "FLAG_ANALYTIC_LIGHTS", "FLAG_SHADING_NORMALS", "FLAG_MICROFACET", "FLAG_ROUGH_DIELECTRIC", "FLAG_NORMAL_MAPS", "mapped_normal_host", "FLAG_ROUGHNESS_MAPS", "ROUGHNESS_REMAPS", "hit_roughness_host", "LIGHT", "LIGHT_POINT", "LIGHT_SPOT", "LIGHT_DIRECTIONAL", "MAX_LIGHTS", "FLAG_NO_TILE_LISTS", "TILE_LIST_CAP", "TILE_NO_LIST", "tile_lists_host", "nodes_ch", "TEMPORAL_DEFAULTS", "TEMPORAL_OUTPUTS", "STAGES", "lib", "build",
           "tonemap_rgb8", "selftest_math", "device_count"]

SPP = 10  # wavefront_common/src/parameters.rs:4
SPF = 1   # wavefront_common/src/parameters.rs:5

RNG_DISPATCH, RNG_PIXEL = 0, 1
LOOP_KINDS = ("stages", "fused", "fused_binned", "refill")  # wfpt_loop_kind
FLAG_SPLIT_SHADE, FLAG_NO_GRAPH, FLAG_UNFUSED, FLAG_BINARY_BVH, FLAG_NO_REFILL, FLAG_NO_LDS_SCENE, FLAG_EXACT_TRAVERSAL, FLAG_NO_BINNING, FLAG_BINNING = 1, 2, 4, 8, 16, 32, 64, 128, 256
FLAG_AOV = 1 << 10  # first-hit AOVs (include/wfpt.h "AOVs"); bit 9 is the retired WFPT_FLAG_TWO_CHAINS
FLAG_ENVIRONMENT = 1 << 12  # misses lit by an HDR environment map (include/wfpt.h "Environment map")
FLAG_TEXTURES = 1 << 13  # image textures on spheres and triangles (include/wfpt.h "Textures")
MAX_TEXTURES = 64  # WFPT_MAX_TEXTURES
TEXTURE_FILTERS = {"bilinear": 0, "nearest": 1}
FLAG_EMISSION = 1 << 14  # emissive materials (include/wfpt.h "Emission")
FLAG_NEE = 1 << 15  # shadow rays from diffuse hits to the emitters (include/wfpt.h "Next-event estimation"); needs FLAG_EMISSION
# the environment map as one more light of the connect pass (include/wfpt.h "Environment next-event estimation"); needs FLAG_ENVIRONMENT,
# FLAG_EMISSION and FLAG_NEE
FLAG_ENV_NEE = 1 << 16
FLAG_MIS = 1 << 17
# the map and the emitters weighed against the scatter (include/wfpt.h "Environment multiple importance sampling"); needs the four flags
# of FLAG_ENV_NEE, refused with FLAG_MIS
FLAG_ENV_MIS = 1 << 18
FLAG_NO_TILE_LISTS = 1 << 19  # the first fused launch walks the tree for every tile (include/wfpt.h "Tile lists")
FLAG_RETIRE = 1 << 20  # dead paths are retired and Russian roulette ends or re-weights the others (include/wfpt.h "Path termination")
NO_ROULETTE = 0xFFFFFFFF  # set_termination(roulette_start=NO_ROULETTE): dead paths alone are retired
# a per-pixel active mask, sample counts and moments, and the device pass that makes the next mask (include/wfpt.h "Adaptive sampling");
# refused with FLAG_AOV, FLAG_DENOISE and FLAG_BINNING
FLAG_ADAPTIVE = 1 << 21
# the connect pass selects its light in proportion to power, luminance times area (include/wfpt.h "Light selection by power"); needs
# FLAG_EMISSION and FLAG_NEE, refused with FLAG_ENV_NEE
FLAG_LIGHT_POWER = 1 << 22
# point, spot and directional lights for the connect pass (include/wfpt.h "Analytic lights"); needs FLAG_EMISSION and FLAG_NEE, refused with
# FLAG_ENV_NEE, FLAG_ENV_MIS and FLAG_LIGHT_POWER
FLAG_ANALYTIC_LIGHTS = 1 << 23
# per-vertex shading normals on triangle meshes (include/wfpt.h "Shading normals"); refused with FLAG_LIGHT_POWER and FLAG_ANALYTIC_LIGHTS
FLAG_SHADING_NORMALS = 1 << 24
# GGX microfacet metals on triangle meshes: a roughness per material (include/wfpt.h "Microfacet metals"); goes with every flag
FLAG_MICROFACET = 1 << 25
# GGX rough dielectrics on triangle meshes: the same roughness on a dielectric (include/wfpt.h "Rough dielectrics"); needs FLAG_MICROFACET
FLAG_ROUGH_DIELECTRIC = 1 << 26
# tangent-space normal maps on triangle meshes (include/wfpt.h "Normal maps"); needs FLAG_TEXTURES and FLAG_SHADING_NORMALS
FLAG_NORMAL_MAPS = 1 << 27
FLAG_ROUGHNESS_MAPS = 1 << 28
ROUGHNESS_REMAPS = ("linear", "squared")  # wfpt_roughness_remap, by value
LIGHT_POINT, LIGHT_SPOT, LIGHT_DIRECTIONAL = 0, 1, 2  # wfpt_light_type
MAX_LIGHTS = 1024  # WFPT_MAX_LIGHTS
ADAPTIVE_DEFAULTS = {"min_samples": 16, "max_samples": 0, "threshold": 0.05, "luminance_floor": 0.01, "dilate": 1}  # wfpt_adaptive_params_default
TILE_LIST_CAP, TILE_NO_LIST = 16, 0xFFFFFFFF
FLAG_DENOISE = 1 << 11  # luminance moments and the a-trous denoiser (include/wfpt.h "Denoiser"); implies FLAG_AOV
# wfpt_denoise_params_default: SVGF's iterations and sigmas, sigma_albedo chosen by tests/test_gpu_denoise.py's quality test
DENOISE_DEFAULTS = {"iterations": 5, "sigma_luminance": 4.0, "sigma_normal": 128.0, "sigma_depth": 1.0, "sigma_albedo": 0.5}
# wfpt_temporal_params_default: the spatial passes above plus the history (include/wfpt.h "Temporal denoiser"); history_cap chosen by a
# quality sweep, the rejection thresholds SVGF-style
TEMPORAL_DEFAULTS = {**DENOISE_DEFAULTS, "history_cap": 32.0, "depth_tolerance": 0.05, "normal_cos": 0.9}
# wfpt_temporal_out: name -> (value, channels)
TEMPORAL_OUTPUTS = {"color": (0, 3), "moments": (1, 2), "length": (2, 1), "motion": (3, 3)}
INACTIVE_PIXEL = 0xFFFFFFFF
# wfpt_aov: name -> (value, channels, numpy dtype of the resolved values)
AOV_ALBEDO, AOV_NORMAL, AOV_DEPTH, AOV_COVERAGE, AOV_PRIM_ID, AOV_MATERIAL_ID = 0, 1, 2, 3, 4, 5
AOVS = {"albedo": (AOV_ALBEDO, 3, "<f4"), "normal": (AOV_NORMAL, 3, "<f4"), "depth": (AOV_DEPTH, 1, "<f4"),
        "coverage": (AOV_COVERAGE, 1, "<f4"), "prim_id": (AOV_PRIM_ID, 1, "<u4"), "material_id": (AOV_MATERIAL_ID, 1, "<u4")}
# kernel.rs:32 loads shaders/{name}.wgsl; these are the stage names (path_tracer.rs:162,167,175,180,185)
STAGES = {"generate_rays": 0, "extend": 1, "shade": 2, "miss_kernel": 3, "accumulate": 4,
          "shade_lambertian": 5, "shade_metal": 6, "shade_dielectric": 7, "scan": 8,
          # fused launches of the device-resident loop (timing only; not dispatchable through Kernel)
          "bounce_first": 9, "bounce": 10, "bounce_last": 11, "compact": 12}
STAGE_COUNT = 13

SPHERE = np.dtype([("center", "<f4", 4), ("radius", "<f4"), ("material_idx", "<u4"),
                   ("material_type", "<u4"), ("_buffer", "<u4")])
MATERIAL = np.dtype([("albedo", "<f4", 4), ("fuzz", "<f4"), ("refract_index", "<f4"),
                     ("material_type", "<u4"), ("_buffer", "<u4")])
# wfpt_light: direction is the way the light travels (spot axis, sun direction); colour is the radiant intensity of a point or spot light and
# the irradiance on a facing surface of a directional one
LIGHT = np.dtype([("position", "<f4", 3), ("type", "<u4"), ("direction", "<f4", 3), ("cos_inner", "<f4"),
                  ("colour", "<f4", 3), ("cos_outer", "<f4")])
BVH_NODE = np.dtype([("aabb_min", "<f4", 3), ("left_first", "<u4"), ("aabb_max", "<f4", 3),
                     ("prim_count", "<u4")])
GPU_CAMERA = np.dtype([("position", "<f4", 4), ("pitch", "<f4"), ("yaw", "<f4"),
                       ("defocus_radius", "<f4"), ("focus_distance", "<f4")])
RAY = np.dtype([("origin", "<f4", 4), ("direction", "<f4", 4), ("inv_direction", "<f4", 3),
                ("pixel_idx", "<u4")])
HIT = np.dtype([("t", "<f4"), ("ray_idx", "<u4"), ("sphere_idx", "<u4"), ("mat_type", "<u4")])
# build extension (the reference has spheres only): vertex + two edges, 48 B
TRIANGLE = np.dtype([("v0", "<f4", 3), ("material_idx", "<u4"), ("e1", "<f4", 3), ("material_type", "<u4"),
                     ("e2", "<f4", 3), ("_pad", "<u4")])


OK, ERR_INVALID_ARGUMENT, ERR_HIP, ERR_OUT_OF_MEMORY, ERR_UNSUPPORTED, ERR_NO_DEVICE = 0, -1, -2, -3, -4, -5  # wfpt_status


class WfptError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"wfpt status {status}: {message}")
        self.status = status


class _Params(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("max_pixels", C.c_uint32),
                ("max_wavefronts", C.c_uint32), ("miss_floor", C.c_uint32), ("rng_mode", C.c_uint32),
                ("flags", C.c_uint32), ("tile_rank", C.c_uint32), ("tile_world", C.c_uint32),
                ("device", C.c_int32), ("batch", C.c_uint32)]


class _DenoiseParams(C.Structure):
    _fields_ = [("iterations", C.c_uint32), ("sigma_luminance", C.c_float), ("sigma_normal", C.c_float), ("sigma_depth", C.c_float),
                ("sigma_albedo", C.c_float), ("_reserved", C.c_uint32 * 3)]


class _EnvironmentParams(C.Structure):
    _fields_ = [("intensity", C.c_float), ("rotation", C.c_float), ("_reserved", C.c_uint32 * 6)]


class _TerminationParams(C.Structure):
    _fields_ = [("roulette_start", C.c_uint32), ("q_min", C.c_float), ("_reserved", C.c_uint32 * 6)]


class _AdaptiveParams(C.Structure):
    _fields_ = [("min_samples", C.c_uint32), ("max_samples", C.c_uint32), ("threshold", C.c_float), ("luminance_floor", C.c_float),
                ("dilate", C.c_uint32), ("_reserved", C.c_uint32 * 3)]


class _TextureParams(C.Structure):
    _fields_ = [("scale", C.c_float * 2), ("offset", C.c_float * 2), ("filter", C.c_uint32), ("_reserved", C.c_uint32 * 3)]


class _TemporalParams(C.Structure):
    _fields_ = [("spatial", _DenoiseParams), ("history_cap", C.c_float), ("depth_tolerance", C.c_float), ("normal_cos", C.c_float),
                ("_reserved", C.c_uint32 * 5)]


class GPUFrameBuffer(C.Structure):
    """wavefront_common/src/gpu_structs.rs:5-28"""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("frame", C.c_uint32),
                ("sample_number", C.c_uint32)]

    @classmethod
    def new(cls, width, height, frame):
        return cls(width, height, frame, 0)

    def into_array(self):
        return [self.width, self.height, self.frame, self.sample_number]

    def set_sample_number(self, sample_number):
        self.sample_number = sample_number


def build(force=False, verbose=False):
    return _build.build(force=force, verbose=verbose)


_lib = None


def _agree_on_hip_runtime():
    """libwfpt.so needs `libamdhip64.so.7`; a PyTorch ROCm wheel ships its own copy of that runtime (with its own HSA
    runtime beside it) under the same SONAME. One process can initialise the GPU through one HIP/HSA pair only: with the
    system copy mapped first, a later `import torch` would bring a second HSA runtime along and find "No HIP GPUs". So when a
    PyTorch ROCm wheel is installed (whether or not it has been, or ever will be, imported) the copy it ships is the one
    mapped first, by its file name: whichever of torch and this package loads first, both end up on the same runtime. Nothing
    of torch is imported or executed here; hosts without PyTorch (C, C++, Rust) are not concerned."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return  # its runtime is already mapped; libwfpt.so's NEEDED entry resolves to it by SONAME
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if not os.path.exists(cand):
        return
    # Only a copy that will actually SATISFY libwfpt.so's NEEDED entry may be mapped first: the dynamic loader matches by
    # DT_SONAME, so a wheel built against another HIP major version (another SONAME) would sit beside the system runtime
    # that libwfpt.so then pulls in -- two HIP/HSA pairs in one process, the very failure this function exists to avoid.
    try:
        want = [n for n in _elf_dynamic(os.environ.get("WFPT_LIB", _build.LIB_PATH))[1] if n.startswith("libamdhip64.so")]
        soname = _elf_dynamic(cand)[0]
    except (OSError, ValueError):
        return
    if not want or soname != want[0]:
        return  # a different runtime generation: leave the choice to the load order, as before
    try:
        C.CDLL(cand, mode=C.RTLD_GLOBAL)
    except OSError:
        pass  # fall back to the system runtime; `import torch` before this package still works as before


def _elf_dynamic(path):
    """(DT_SONAME, [DT_NEEDED ...]) of a 64-bit little-endian ELF shared object, read from the file (nothing is loaded)."""
    import struct
    with open(path, "rb") as f:
        head = f.read(64)
        if head[:4] != b"\x7fELF" or head[4] != 2 or head[5] != 1:
            raise ValueError("not a 64-bit little-endian ELF file")
        shoff, = struct.unpack_from("<Q", head, 0x28)
        shentsize, shnum = struct.unpack_from("<HH", head, 0x3A)
        f.seek(shoff)
        sections = [struct.unpack_from("<IIQQQQIIQQ", f.read(shentsize)) for _ in range(shnum)]
        dyn = next((sec for sec in sections if sec[1] == 6), None)  # SHT_DYNAMIC
        if dyn is None:
            raise ValueError("no dynamic section")
        strtab = sections[dyn[6]]  # sh_link: the string table of the dynamic section
        f.seek(strtab[4])
        strings = f.read(strtab[5])
        f.seek(dyn[4])
        raw = f.read(dyn[5])
    soname, needed = None, []
    for off in range(0, len(raw) - 15, 16):
        tag, val = struct.unpack_from("<qQ", raw, off)
        if tag == 0:
            break
        if tag in (1, 14):  # DT_NEEDED, DT_SONAME
            name = strings[val:strings.index(b"\0", val)].decode()
            if tag == 1:
                needed.append(name)
            else:
                soname = name
    return soname, needed


def _one_hip_runtime_mapped():
    """After libwfpt.so is loaded: the process must hold exactly one libamdhip64 (see _agree_on_hip_runtime)."""
    try:
        with open("/proc/self/maps") as f:
            paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    except OSError:
        return
    real = {os.path.realpath(x) for x in paths}
    if len(real) > 1:
        raise WfptError(-5, "two HIP runtimes are mapped into this process (" + ", ".join(sorted(real)) + "): the GPU can be "
                            "initialised through one of them only. Import torch before this package, or set LD_LIBRARY_PATH so "
                            "that libwfpt.so resolves libamdhip64 to the copy PyTorch ships")


def _lib_loaded():
    return _lib is not None


def lib():
    """Load libwfpt.so. Fails loudly when the HIP extension has not been built: nothing here can run without it."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("WFPT_LIB", _build.LIB_PATH)  # WFPT_LIB: tuning builds made with WFPT_EXTRA_FLAGS / WFPT_LIB_OUT
    if not os.path.exists(path):
        raise WfptError(-5, f"{path} is missing: run wavefront_path_tracer_amd.build() "
                            "(python -m wavefront_path_tracer_amd._build); there is no CPU fallback")
    _agree_on_hip_runtime()
    L = C.CDLL(path)
    _one_hip_runtime_mapped()
    vp, u32, i32, f32, sz = C.c_void_p, C.c_uint32, C.c_int, C.c_float, C.c_size_t
    sig = {
        "wfpt_scene_new": (u32, [vp, vp]),
        "wfpt_scene_book_one_final": (u32, [C.c_uint64, vp, vp, u32]),
        "wfpt_build_bvh": (i32, [vp, u32, vp, u32, C.POINTER(u32)]),
        "wfpt_build_bvh_triangles": (i32, [vp, u32, vp, u32, C.POINTER(u32), u32]),
        "wfpt_build_bvh_device": (i32, [vp, u32, vp, u32, C.POINTER(u32), i32, C.POINTER(f32)]),
        "wfpt_build_bvh_triangles_device": (i32, [vp, u32, vp, u32, C.POINTER(u32), u32, i32, C.POINTER(f32)]),
        "wfpt_load_obj": (i32, [C.c_char_p, vp, u32, C.POINTER(u32), u32, u32]),
        "wfpt_scene_random_mesh": (u32, [C.c_uint64, u32, vp, vp]),
        "wfpt_create_mesh": (vp, [C.POINTER(_Params), vp, u32, vp, u32, vp, u32, vp, vp, vp]),
        "wfpt_render_chunked": (i32, [C.POINTER(_Params), vp, u32, vp, u32, vp, u32, vp, vp, vp, u32, u32, vp]),
        "wfpt_render_chunked_mesh": (i32, [C.POINTER(_Params), vp, u32, vp, u32, vp, u32, vp, vp, vp, u32, u32, vp]),
        "wfpt_camera_new": (None, [vp, vp, C.POINTER(f32), C.POINTER(f32)]),
        "wfpt_view_transform": (None, [vp, f32, f32, vp]),
        "wfpt_p_inv": (None, [f32, f32, f32, f32, vp]),
        "wfpt_gpu_camera_new": (None, [vp, f32, f32, f32, f32, vp]),
        "wfpt_to_radians": (f32, [f32]),
        "wfpt_camera_controller_update": (None, [vp, C.POINTER(f32), C.POINTER(f32), vp, vp, f32, f32, f32]),
        "wfpt_workgroup_size_64": (None, [u32, C.POINTER(u32), C.POINTER(u32)]),
        "wfpt_stage_from_name": (i32, [C.c_char_p]),
        "wfpt_stage_name": (C.c_char_p, [i32]),
        "wfpt_device_count": (i32, []),
        "wfpt_create": (vp, [C.POINTER(_Params), vp, u32, vp, u32, vp, u32, vp, vp, vp]),
        "wfpt_destroy": (None, [vp]),
        "wfpt_update_scene": (i32, [vp, vp, u32, vp, u32]),
        "wfpt_update_scene_mesh": (i32, [vp, vp, u32, vp, u32, u32]),
        "wfpt_last_error": (C.c_char_p, [vp]),
        "wfpt_set_frame": (i32, [vp, C.POINTER(GPUFrameBuffer)]),
        "wfpt_update_render_parameters": (i32, [vp, u32, u32, vp, vp, vp]),
        "wfpt_set_counters": (i32, [vp, vp]),
        "wfpt_read_counters": (i32, [vp, vp]),
        "wfpt_reset_image": (i32, [vp]),
        "wfpt_reset_accumulated": (i32, [vp]),
        "wfpt_reset_progress": (i32, [vp]),
        "wfpt_clear_ray_queues": (i32, [vp]),
        "wfpt_swap_ray_queues": (i32, [vp]),
        "wfpt_kernel_run": (i32, [vp, i32, u32, u32]),
        "wfpt_kernel_timing_us": (f32, [vp, i32]),
        "wfpt_render_sample": (i32, [vp]),
        "wfpt_render": (i32, [vp, u32]),
        "wfpt_render_sample_timed": (i32, [vp, vp, vp]),
        "wfpt_render_timed": (i32, [vp, u32, vp, vp]),
        "wfpt_synchronize": (i32, [vp]),
        "wfpt_frame": (u32, [vp]),
        "wfpt_accumulated_samples": (u32, [vp]),
        "wfpt_progress": (f32, [vp, u32]),
        "wfpt_n_pixels": (u32, [vp]),
        "wfpt_ray_capacity": (u32, [vp]),
        "wfpt_read_accumulated": (i32, [vp, vp, sz]),
        "wfpt_read_image": (i32, [vp, vp, sz]),
        "wfpt_copy_accumulated_to_device": (i32, [vp, vp, sz]),
        "wfpt_comm_unique_id": (i32, [vp]),
        "wfpt_comm_init": (i32, [vp, vp, i32, i32]),
        "wfpt_gather_accumulated": (i32, [vp]),
        "wfpt_gather_accumulated_timed": (i32, [vp, C.POINTER(f32)]),
        "wfpt_loop_kind_of": (i32, [vp]),
        "wfpt_read_gathered": (i32, [vp, vp, sz]),
        "wfpt_comm_destroy": (i32, [vp]),
        "wfpt_read_rays": (i32, [vp, vp, u32]),
        "wfpt_read_extension_rays": (i32, [vp, vp, u32]),
        "wfpt_read_hits": (i32, [vp, vp, u32]),
        "wfpt_read_misses": (i32, [vp, vp, u32]),
        "wfpt_write_rays": (i32, [vp, vp, u32]),
        "wfpt_read_bounce_table": (i32, [vp, vp, u32, C.POINTER(u32)]),
        "wfpt_read_totals": (i32, [vp, vp]),
        "wfpt_read_wavefront_totals": (i32, [vp, vp, u32, C.POINTER(u32)]),
        "wfpt_device_info": (i32, [i32, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32), C.POINTER(C.c_uint64)]),
        "wfpt_tonemap_rgb8": (None, [vp, u32, u32, vp]),
        "wfpt_selftest_math": (i32, [i32, i32, vp, vp, vp, sz]),
        "wfpt_build_info": (C.c_char_p, []),
        "wfpt_save_ppm": (i32, [vp, C.c_char_p]),
        "wfpt_save_pfm": (i32, [vp, C.c_char_p]),
        "wfpt_save_png": (i32, [vp, C.c_char_p]),
        "wfpt_write_png_rgb8": (i32, [C.c_char_p, vp, u32, u32]),
        "wfpt_debug_extend_blocks_per_cu": (i32, [i32, u32]),
        "wfpt_debug_read_stamps": (i32, [vp, vp, i32]),
        "wfpt_debug_read_stamps_ex": (i32, [vp, i32, vp, i32]),
        "wfpt_debug_bvh4": (i32, [vp, u32, vp]),
        "wfpt_aov_channels": (i32, [i32]),
        "wfpt_read_aov": (i32, [vp, i32, vp, sz]),
        "wfpt_copy_aov_to_device": (i32, [vp, i32, vp, sz]),
        "wfpt_aov_timing_ms": (i32, [vp, C.POINTER(f32), C.POINTER(u32)]),
        "wfpt_denoise_params_default": (None, [C.POINTER(_DenoiseParams)]),
        "wfpt_denoise": (i32, [vp, C.POINTER(_DenoiseParams), vp, sz]),
        "wfpt_denoise_to_device": (i32, [vp, C.POINTER(_DenoiseParams), vp, sz]),
        "wfpt_read_variance": (i32, [vp, vp, sz]),
        "wfpt_denoise_timing_ms": (i32, [vp, C.POINTER(f32), C.POINTER(u32)]),
        "wfpt_set_frame_offset": (i32, [vp, u32]),
        "wfpt_frame_offset": (u32, [vp]),
        "wfpt_temporal_params_default": (None, [C.POINTER(_TemporalParams)]),
        "wfpt_denoise_temporal": (i32, [vp, C.POINTER(_TemporalParams), vp, sz]),
        "wfpt_denoise_temporal_to_device": (i32, [vp, C.POINTER(_TemporalParams), vp, sz]),
        "wfpt_read_temporal": (i32, [vp, i32, vp, sz]),
        "wfpt_reset_history": (i32, [vp]),
        "wfpt_temporal_timing_ms": (i32, [vp, C.POINTER(f32), C.POINTER(u32)]),
        "wfpt_environment_params_default": (None, [C.POINTER(_EnvironmentParams)]),
        "wfpt_set_environment": (i32, [vp, vp, u32, u32, C.POINTER(_EnvironmentParams)]),
        "wfpt_clear_environment": (i32, [vp]),
        "wfpt_sample_environment": (i32, [vp, vp, sz, vp]),
        "wfpt_texture_params_default": (None, [C.POINTER(_TextureParams)]),
        "wfpt_set_texture": (i32, [vp, u32, vp, u32, u32, C.POINTER(_TextureParams)]),
        "wfpt_clear_texture": (i32, [vp, u32]),
        "wfpt_bind_texture": (i32, [vp, u32, C.c_int32]),
        "wfpt_set_triangle_uvs": (i32, [vp, vp, u32]),
        "wfpt_sample_texture": (i32, [vp, u32, vp, sz, vp]),
        "wfpt_texture_timing_ms": (i32, [vp, C.POINTER(f32), C.POINTER(u32)]),
        "wfpt_load_obj_uv": (i32, [C.c_char_p, vp, vp, u32, C.POINTER(u32), u32, u32]),
        "wfpt_load_obj_normals": (i32, [C.c_char_p, vp, vp, vp, u32, C.POINTER(u32), u32, u32]),
        "wfpt_normalize_triangle_normals": (i32, [vp, u32, vp]),
        "wfpt_set_triangle_normals": (i32, [vp, vp, u32]),
        "wfpt_get_triangle_normals": (i32, [vp, vp, u32, C.POINTER(u32)]),
        "wfpt_sample_shading_normal": (i32, [vp, vp, sz, vp]),
        "wfpt_shading_normal_timing_ms": (i32, [vp, C.POINTER(f32), C.POINTER(u32)]),
        "wfpt_set_roughness": (i32, [vp, u32, f32]),
        "wfpt_get_roughness": (i32, [vp, u32, C.POINTER(f32)]),
        "wfpt_clear_roughness": (i32, [vp]),
        "wfpt_sample_microfacet": (i32, [vp, vp, sz, vp]),
        "wfpt_microfacet_timing_ms": (i32, [vp, C.POINTER(f32), C.POINTER(u32)]),
        "wfpt_sample_rough_dielectric": (i32, [vp, vp, sz, vp]),
        "wfpt_bind_normal_map": (i32, [vp, u32, C.c_int32, f32]),
        "wfpt_get_normal_map": (i32, [vp, u32, C.POINTER(C.c_int32), C.POINTER(f32)]),
        "wfpt_sample_normal_map": (i32, [vp, vp, sz, vp]),
        "wfpt_mapped_normal_host": (i32, [vp, sz, vp]),
        "wfpt_bind_roughness_map": (i32, [vp, u32, C.c_int32, u32, u32]),
        "wfpt_get_roughness_map": (i32, [vp, u32, C.POINTER(C.c_int32), C.POINTER(u32), C.POINTER(u32)]),
        "wfpt_sample_roughness_map": (i32, [vp, vp, sz, vp]),
        "wfpt_hit_roughness_host": (i32, [vp, u32, u32, sz, vp]),
        "wfpt_set_emission": (i32, [vp, u32, C.POINTER(f32)]),
        "wfpt_get_emission": (i32, [vp, u32, C.POINTER(f32)]),
        "wfpt_clear_emission": (i32, [vp]),
        "wfpt_emission_timing_ms": (i32, [vp, C.POINTER(f32), C.POINTER(u32)]),
        "wfpt_nee_light_count": (i32, [vp]),
        "wfpt_nee_timing_ms": (i32, [vp, C.POINTER(f32), C.POINTER(u32)]),
        "wfpt_sample_lights": (i32, [vp, vp, sz, vp]),
        "wfpt_set_environment_share": (i32, [vp, f32]),
        "wfpt_environment_share": (f32, [vp]),
        "wfpt_read_environment_distribution": (i32, [vp, vp, vp]),
        "wfpt_read_light_distribution": (i32, [vp, vp, vp]),
        "wfpt_set_lights": (i32, [vp, vp, u32]),
        "wfpt_get_lights": (i32, [vp, vp, u32, C.POINTER(u32)]),
        "wfpt_analytic_light_count": (i32, [vp]),
        "wfpt_sample_environment_light": (i32, [vp, vp, sz, vp]),
        "wfpt_sample_lights_mis": (i32, [vp, vp, sz, vp]),
        "wfpt_mis_hit_weight": (i32, [vp, vp, sz, vp]),
        "wfpt_sample_environment_light_mis": (i32, [vp, vp, sz, vp]),
        "wfpt_env_mis_miss_weight": (i32, [vp, vp, sz, vp]),
        "wfpt_termination_params_default": (None, [C.POINTER(_TerminationParams)]),
        "wfpt_set_termination": (i32, [vp, C.POINTER(_TerminationParams)]),
        "wfpt_get_termination": (i32, [vp, C.POINTER(_TerminationParams)]),
        "wfpt_sample_termination": (i32, [vp, vp, vp, u32, u32, sz, vp]),
        "wfpt_adaptive_params_default": (None, [C.POINTER(_AdaptiveParams)]),
        "wfpt_set_adaptive": (i32, [vp, C.POINTER(_AdaptiveParams)]),
        "wfpt_get_adaptive": (i32, [vp, C.POINTER(_AdaptiveParams)]),
        "wfpt_set_active_mask": (i32, [vp, vp, sz]),
        "wfpt_read_active_mask": (i32, [vp, vp, sz]),
        "wfpt_adaptive_update": (i32, [vp, C.POINTER(u32)]),
        "wfpt_read_sample_counts": (i32, [vp, vp, sz]),
        "wfpt_read_mean": (i32, [vp, vp, sz]),
        "wfpt_copy_mean_to_device": (i32, [vp, vp, sz]),
        "wfpt_render_adaptive": (i32, [vp, u32, u32, C.POINTER(u32)]),
        "wfpt_tile_lists_host": (i32, [vp, u32, vp, vp, vp, u32, u32, u32, u32, vp, u32]),
        "wfpt_debug_nodes_ch": (i32, [vp, u32, vp, vp]),
        "wfpt_debug_read_tile_lists": (i32, [vp, vp, C.POINTER(u32)]),
        "wfpt_tile_lists_timing_ms": (i32, [vp, C.POINTER(f32), C.POINTER(u32)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)  # AttributeError here = the library does not export what wfpt.h declares
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


ABI_SYMBOLS = None  # filled lazily by abi_symbols()


def abi_symbols():
    """Every function include/wfpt.h declares (parsed from the header)."""
    import re
    hdr = os.path.join(_build.ROOT, "include", "wfpt.h")
    text = open(hdr).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(wfpt_[a-z0-9_]+)\s*\(", text)))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- tile lists (include/wfpt.h "Tile lists"): the host twin of the device builder, no GPU needed
def nodes_ch(nodes, gpu_camera):
    """The margin-grown (centre | left_first), (half-extent | prim_count) boxes a context of this tree and camera walks: float32
    [n_nodes, 8] (the two index words as their bits)."""
    out = np.zeros((len(nodes), 8), np.float32)
    st = lib().wfpt_debug_nodes_ch(_p(nodes), len(nodes), _p(gpu_camera), _p(out))
    if st != 0:
        raise WfptError(st, lib().wfpt_last_error(None).decode())
    return out


def tile_lists_host(nodes, gpu_camera, inv_proj, view, width, height, tile_rank=0, tile_world=1):
    """The per-tile candidate lists of the first fused launch, computed on the host: uint32 [tiles, TILE_LIST_CAP] records (leaf words
    `left_first | prim_count << 16` in ascending node order, then 0; record[0] == TILE_NO_LIST: the tile keeps no list)."""
    ch = nodes_ch(nodes, gpu_camera)
    gx, bands = (width + 7) // 8, (height + 7) // 8
    gy = (bands - tile_rank + tile_world - 1) // tile_world if bands > tile_rank else 0
    out = np.zeros((gx * gy, TILE_LIST_CAP), np.uint32)
    inv_proj, view = np.ascontiguousarray(inv_proj, np.float32), np.ascontiguousarray(view, np.float32)
    st = lib().wfpt_tile_lists_host(_p(ch), len(nodes), _p(gpu_camera), _p(inv_proj), _p(view), width, height, tile_rank, tile_world,
                                    _p(out), gx * gy)
    if st != 0:
        raise WfptError(st, "wfpt_tile_lists_host: invalid argument")
    return out


def mapped_normal_host(rows):
    """Steps B-F of include/wfpt.h "Normal maps" on the host (no GPU), from the function the kernels call. rows: (n, 22) float32 of
    (ng.xyz, ns.xyz, e1.xyz, e2.xyz, u0 v0 u1 v1 u2 v2, c.rgb, strength); returns (n, 4) float32 of (n.xyz, code 0..3)."""
    a = np.ascontiguousarray(rows, "<f4")
    if a.ndim != 2 or a.shape[1] != 22:
        raise ValueError(f"mapped_normal_host: expected rows of 22 floats, got shape {a.shape}")
    out = np.zeros((a.shape[0], 4), "<f4")
    st = lib().wfpt_mapped_normal_host(_p(a), a.shape[0], _p(out))
    if st != 0:
        raise WfptError(st, "wfpt_mapped_normal_host: invalid argument")
    return out


def _remap_value(remap):
    if isinstance(remap, str):
        if remap not in ROUGHNESS_REMAPS:
            raise ValueError(f"remap must be one of {ROUGHNESS_REMAPS}, got {remap!r}")
        return ROUGHNESS_REMAPS.index(remap)
    return int(remap)


def hit_roughness_host(rows, channel=1, remap="linear"):
    """Steps R3-R4 of include/wfpt.h "Roughness maps" on the host (no GPU), from the function the kernels call. rows: (n, 4) float32 of
    (alpha_m, c.r, c.g, c.b); channel 0, 1 or 2 and remap "linear" or "squared" for all rows; returns (n, 2) float32 of (alpha_h, r)."""
    a = np.ascontiguousarray(rows, "<f4")
    if a.ndim != 2 or a.shape[1] != 4:
        raise ValueError(f"hit_roughness_host: expected rows of 4 floats, got shape {a.shape}")
    out = np.zeros((a.shape[0], 2), "<f4")
    st = lib().wfpt_hit_roughness_host(_p(a), int(channel), _remap_value(remap), a.shape[0], _p(out))
    if st != 0:
        raise WfptError(st, "wfpt_hit_roughness_host: invalid argument")
    return out


def device_count():
    return lib().wfpt_device_count()


def comm_unique_id():
    """Rank 0: a fresh RCCL unique id (128 bytes) to hand to every rank's PathTracer.comm_init."""
    buf = np.zeros(128, np.uint8)
    st = lib().wfpt_comm_unique_id(_p(buf))
    if st != 0:
        raise WfptError(st, lib().wfpt_last_error(None).decode())
    return buf.tobytes()


def device_info(device=0):
    """CU count, memory clock (kHz), memory bus width (bits), memory bytes of HIP device `device`."""
    cu, clk, width, mem = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint64()
    st = lib().wfpt_device_info(device, C.byref(cu), C.byref(clk), C.byref(width), C.byref(mem))
    if st != 0:
        raise WfptError(st, lib().wfpt_last_error(None).decode())
    return {"compute_units": cu.value, "memory_clock_khz": clk.value, "memory_bus_width_bits": width.value,
            "total_memory_bytes": mem.value}


def workgroup_size_64(x):
    """path_tracer.rs:282-289"""
    gx, gy = C.c_uint32(), C.c_uint32()
    lib().wfpt_workgroup_size_64(x, C.byref(gx), C.byref(gy))
    return gx.value, gy.value


def tonemap_rgb8(accumulated, n_samples):
    a = np.ascontiguousarray(accumulated, "<f4").reshape(-1)
    out = np.zeros(a.size, np.uint8)
    lib().wfpt_tonemap_rgb8(_p(a), a.size // 3, n_samples, _p(out))
    return out.reshape(-1, 3)


def write_png(path, rgb8, width, height):
    """An (height, width, 3) uint8 image as a PNG file (wfpt_write_png_rgb8; no compression library)."""
    a = np.ascontiguousarray(rgb8, np.uint8)
    if a.size != 3 * width * height:
        raise ValueError("rgb8 must hold width * height RGB pixels")
    st = lib().wfpt_write_png_rgb8(os.fsencode(path), _p(a), width, height)
    if st != 0:
        raise WfptError(st, f"cannot write {path}")


def load_environment(path):
    """An HDR environment map as an (h, w, 3) float32 array, row 0 = top: Radiance .hdr (RGBE, "-Y h +X w", flat or new-style RLE
    scanlines) or .pfm (colour "PF", either byte order; PFM stores rows bottom-up)."""
    data = open(path, "rb").read()
    if data[:2] in (b"PF", b"Pf"):
        return _read_pfm(data)
    if data[:2] == b"#?":
        return _read_hdr(data)
    raise ValueError(f"load_environment: {path} is neither a Radiance .hdr nor a .pfm file")


def _read_pfm(data):
    fields, pos = [], 0
    while len(fields) < 4:  # "PF", width, height, scale, separated by whitespace
        while data[pos:pos + 1].isspace():
            pos += 1
        end = pos
        while not data[end:end + 1].isspace():
            end += 1
        fields.append(data[pos:end].decode("ascii"))
        pos = end
    pos += 1  # the single whitespace character before the raster
    if fields[0] != "PF":
        raise ValueError("load_environment: only colour PFM (PF) maps are supported")
    w, h, scale = int(fields[1]), int(fields[2]), float(fields[3])
    a = np.frombuffer(data, "<f4" if scale < 0 else ">f4", count=w * h * 3, offset=pos)
    return np.ascontiguousarray(a.reshape(h, w, 3)[::-1].astype("<f4"))


def _read_hdr(data):
    pos = 0
    while True:  # header lines up to the empty one
        end = data.index(b"\n", pos)
        line = data[pos:end].strip()
        pos = end + 1
        if not line:
            break
        if line.startswith(b"FORMAT=") and line != b"FORMAT=32-bit_rle_rgbe":
            raise ValueError(f"load_environment: unsupported .hdr format {line!r}")
    end = data.index(b"\n", pos)
    res = data[pos:end].split()
    pos = end + 1
    if len(res) != 4 or res[0] != b"-Y" or res[2] != b"+X":
        raise ValueError(f"load_environment: only '-Y h +X w' .hdr maps are supported, not {data[pos:end]!r}")
    h, w = int(res[1]), int(res[3])
    buf = np.frombuffer(data, np.uint8, offset=pos)
    rgbe = np.zeros((h, w, 4), np.uint8)
    i = 0
    for y in range(h):
        if 8 <= w < 32768 and buf[i] == 2 and buf[i + 1] == 2 and (int(buf[i + 2]) << 8 | int(buf[i + 3])) == w and not buf[i + 2] & 0x80:
            i += 4  # new-style RLE: four channel runs, each packed as (count > 128: a run of count - 128 copies | count: literals)
            for ch in range(4):
                x = 0
                while x < w:
                    n = int(buf[i])
                    i += 1
                    if n > 128:
                        n -= 128
                        rgbe[y, x:x + n, ch] = buf[i]
                        i += 1
                    else:
                        rgbe[y, x:x + n, ch] = buf[i:i + n]
                        i += n
                    x += n
        else:  # flat scanline
            rgbe[y] = buf[i:i + 4 * w].reshape(w, 4)
            i += 4 * w
    e = rgbe[..., 3].astype(np.int32)
    scale = np.where(e > 0, np.ldexp(1.0, e - 136), 0.0)  # mantissa / 256 * 2^(e - 128)
    return (rgbe[..., :3].astype(np.float64) * scale[..., None]).astype("<f4")


def load_texture(path):
    """A texture image as an (h, w, 3) float32 array of linear RGB, row 0 = the top: 8-bit PNG (grey, RGB or RGBA, non-interlaced) or binary
    PPM (P6), decoded from sRGB; or PFM / Radiance .hdr, linear as stored (the environment map's readers)."""
    data = open(path, "rb").read()
    if data[:8] == b"\x89PNG\r\n\x1a\n":
        return _srgb_to_linear(_read_png(data))
    if data[:2] == b"P6":
        return _srgb_to_linear(_read_ppm(data))
    if data[:2] in (b"PF", b"Pf"):
        return _read_pfm(data)
    if data[:2] == b"#?":
        return _read_hdr(data)
    raise ValueError(f"load_texture: {path} is not a PNG, PPM (P6), PFM or Radiance .hdr file")


def _srgb_to_linear(rgb8):
    c = rgb8.astype(np.float64) / 255.0
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4).astype("<f4")


def _read_ppm(data):
    fields, pos = [], 0
    while len(fields) < 4:  # "P6", width, height, maxval; comments run to the end of their line
        while data[pos:pos + 1].isspace():
            pos += 1
        if data[pos:pos + 1] == b"#":
            pos = data.index(b"\n", pos) + 1
            continue
        end = pos
        while end < len(data) and not data[end:end + 1].isspace():
            end += 1
        fields.append(data[pos:end].decode("ascii"))
        pos = end
    pos += 1
    w, h, maxval = int(fields[1]), int(fields[2]), int(fields[3])
    if maxval != 255:
        raise ValueError("load_texture: only 8-bit PPM files (maxval 255) are supported")
    return np.frombuffer(data, np.uint8, count=w * h * 3, offset=pos).reshape(h, w, 3)


def _png_unfilter(raw, w, ch):
    """The five scanline filters of PNG (spec 9.2) undone for a whole image: raw (h, 1 + w * ch) uint8 -> (h, w, ch) uint8. A pixel depends
    on its reconstructed left, upper and upper-left neighbours only, so every anti-diagonal x + y = d depends on earlier diagonals alone:
    the image is reconstructed one diagonal at a time, each as one vector step over its pixels (h + w steps, not h * w * ch)."""
    h = raw.shape[0]
    filt = raw[:, 0].astype(np.int32)
    if (filt > 4).any():
        raise ValueError(f"load_texture: unknown PNG filter type {int(filt.max())}")
    line = raw[:, 1:].reshape(h, w, ch).astype(np.int32)
    rec = np.zeros((h + 1, w + 1, ch), np.int32)  # row 0 and column 0: the zero neighbours outside the image
    for d in range(h + w - 1):
        y = np.arange(max(0, d - w + 1), min(h, d + 1))
        x = d - y
        a, b, c = rec[y + 1, x], rec[y, x + 1], rec[y, x]  # left, up, upper left
        pa, pb, pc = np.abs(b - c), np.abs(a - c), np.abs(a + b - 2 * c)
        paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
        f = filt[y][:, None]
        pred = np.where(f == 1, a, np.where(f == 2, b, np.where(f == 3, (a + b) >> 1, np.where(f == 4, paeth, 0))))
        rec[y + 1, x + 1] = (line[y, x] + pred) & 255
    return rec[1:, 1:].astype(np.uint8)


def _read_png(data):
    import struct
    import zlib
    pos, idat, w = 8, [], None
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        pos += 12 + n
        if kind == b"IHDR":
            w, h, depth, ctype, _, _, interlace = struct.unpack(">IIBBBBB", body)
            if depth != 8 or ctype not in (0, 2, 6) or interlace:
                raise ValueError("load_texture: only 8-bit, non-interlaced grey, RGB or RGBA PNG files are supported")
        elif kind == b"IDAT":
            idat.append(body)
        elif kind == b"IEND":
            break
    if w is None:
        raise ValueError("load_texture: PNG without IHDR")
    ch = {0: 1, 2: 3, 6: 4}[ctype]
    raw = np.frombuffer(zlib.decompress(b"".join(idat)), np.uint8).reshape(h, 1 + w * ch)
    img = _png_unfilter(raw, w, ch)
    if ch == 1:
        img = np.repeat(img, 3, axis=2)
    return np.ascontiguousarray(img[..., :3])


def _emission_colour(rgb):
    """rgb as the (3 x c_float) array wfpt_set_emission takes; ValueError unless it is three finite floats >= 0 (what the library accepts)."""
    a = np.asarray(rgb, "<f4")
    if a.shape != (3,):
        raise ValueError(f"set_emission: expected 3 floats (r, g, b), got shape {a.shape}")
    if not (np.isfinite(a).all() and (a >= 0).all()):
        raise ValueError(f"set_emission: the colour must be finite and >= 0, got {a.tolist()}")
    return (C.c_float * 3)(*a.tolist())


def _material_index(material_idx):
    m = int(material_idx)
    if m != material_idx or not 0 <= m < 2 ** 32:
        raise ValueError(f"material_idx must be an integer in 0..2^32-1, got {material_idx!r}")
    return m


def selftest_math(op, a, b=None, device=0):
    a = np.ascontiguousarray(a, "<f4")
    out = np.zeros_like(a)
    bb = None if b is None else np.ascontiguousarray(b, "<f4")
    st = lib().wfpt_selftest_math(device, op, _p(a), None if bb is None else _p(bb), _p(out), a.size)
    if st != 0:
        raise WfptError(st, lib().wfpt_last_error(None).decode())
    return out


# ------------------------------------------------------------------------------------------------
# wavefront_common data model
# ------------------------------------------------------------------------------------------------
class Scene:
    """wavefront_common/src/scene.rs: `spheres` and `materials` in the reference's 32-byte layouts."""

    def __init__(self, spheres, materials, triangles=None):
        self.spheres = np.ascontiguousarray(spheres, SPHERE)
        self.materials = np.ascontiguousarray(materials, MATERIAL)
        self.triangles = None if triangles is None else np.ascontiguousarray(triangles, TRIANGLE)  # build extension

    @classmethod
    def from_obj(cls, path, materials=None, material_idx=0):
        """Build extension (README.md:25): the triangles of a Wavefront OBJ file, all with one material
        (default: Lambertian 0.7 grey, like the mesh scene's first material)."""
        if materials is None:
            materials = np.zeros(1, MATERIAL)
            materials["albedo"][0] = (0.7, 0.7, 0.7, 1.0)
        materials = np.ascontiguousarray(materials, MATERIAL)
        n = C.c_uint32()
        st = lib().wfpt_load_obj(os.fsencode(path), None, 0, C.byref(n), 0, 0)
        if st != 0 or n.value == 0:
            raise WfptError(st or ERR_INVALID_ARGUMENT, f"cannot read triangles from {path}")
        tris = np.zeros(n.value, TRIANGLE)
        mtype = int(materials["material_type"][material_idx])
        st = lib().wfpt_load_obj(os.fsencode(path), _p(tris), len(tris), C.byref(n), material_idx, mtype)
        if st != 0:
            raise WfptError(st, f"cannot read triangles from {path}")
        return cls(np.zeros(0, SPHERE), materials, triangles=tris)

    @classmethod
    def load_obj(cls, path, materials=None, material_idx=0, uvs=False, normals=False):
        """from_obj; with uvs=True returns (scene, uv) -- the (n, 6) float32 UV rows u0 v0 u1 v1 u2 v2 of the triangles in file order (each
        triangle's _pad names its row), for PathTracer.set_triangle_uvs. With normals=True returns (scene, normals), or (scene, uv, normals)
        with uvs=True too -- the (n, 9) float32 rows of corner normals as the file gives them (a corner without one: the face's own), for
        PathTracer.set_triangle_normals; a face wound against its normals has its winding swapped (wfpt_load_obj_normals)."""
        if normals:
            if materials is None:
                materials = np.zeros(1, MATERIAL)
                materials["albedo"][0] = (0.7, 0.7, 0.7, 1.0)
            materials = np.ascontiguousarray(materials, MATERIAL)
            n = C.c_uint32()
            st = lib().wfpt_load_obj_normals(os.fsencode(path), None, None, None, 0, C.byref(n), 0, 0)
            if st != 0 or n.value == 0:
                raise WfptError(st or ERR_INVALID_ARGUMENT, f"cannot read triangles from {path}")
            tris, uv, n9 = np.zeros(n.value, TRIANGLE), np.zeros((n.value, 6), "<f4"), np.zeros((n.value, 9), "<f4")
            mtype = int(materials["material_type"][material_idx])
            st = lib().wfpt_load_obj_normals(os.fsencode(path), _p(tris), _p(uv), _p(n9), len(tris), C.byref(n), material_idx, mtype)
            if st != 0:
                raise WfptError(st, f"cannot read triangles from {path}")
            scene = cls(np.zeros(0, SPHERE), materials, triangles=tris)
            return (scene, uv, n9) if uvs else (scene, n9)
        if not uvs:
            return cls.from_obj(path, materials, material_idx)
        if materials is None:
            materials = np.zeros(1, MATERIAL)
            materials["albedo"][0] = (0.7, 0.7, 0.7, 1.0)
        materials = np.ascontiguousarray(materials, MATERIAL)
        n = C.c_uint32()
        st = lib().wfpt_load_obj_uv(os.fsencode(path), None, None, 0, C.byref(n), 0, 0)
        if st != 0 or n.value == 0:
            raise WfptError(st or ERR_INVALID_ARGUMENT, f"cannot read triangles from {path}")
        tris, uv = np.zeros(n.value, TRIANGLE), np.zeros((n.value, 6), "<f4")
        mtype = int(materials["material_type"][material_idx])
        st = lib().wfpt_load_obj_uv(os.fsencode(path), _p(tris), _p(uv), len(tris), C.byref(n), material_idx, mtype)
        if st != 0:
            raise WfptError(st, f"cannot read triangles from {path}")
        return cls(np.zeros(0, SPHERE), materials, triangles=tris), uv

    @classmethod
    def random_mesh(cls, n_triangles, seed=1):
        """BASELINE config 5's seeded triangle soup (build extension: the reference has no triangle type)."""
        tr, mt = np.zeros(n_triangles, TRIANGLE), np.zeros(3, MATERIAL)
        lib().wfpt_scene_random_mesh(seed, n_triangles, _p(tr), _p(mt))
        return cls(np.zeros(0, SPHERE), mt, tr)

    @classmethod
    def new(cls):
        """scene.rs:12-46"""
        sp, mt = np.zeros(5, SPHERE), np.zeros(5, MATERIAL)
        n = lib().wfpt_scene_new(_p(sp), _p(mt))
        return cls(sp[:n], mt[:n])

    @classmethod
    def book_one_final(cls, seed=1):
        """scene.rs:48-107, seeded (the reference draws from an unseeded thread_rng)."""
        sp, mt = np.zeros(512, SPHERE), np.zeros(512, MATERIAL)
        n = lib().wfpt_scene_book_one_final(seed, _p(sp), _p(mt), 512)
        if n == 0:
            raise WfptError(-1, "wfpt_scene_book_one_final failed")
        return cls(sp[:n].copy(), mt[:n].copy())


class BVHTree:
    """wavefront_common/src/bvh.rs:143-210"""

    def __init__(self, num_primitives):
        self.capacity = 2 * max(int(num_primitives), 1)
        self.nodes = np.zeros(0, BVH_NODE)

    def build_bvh_tree(self, spheres, device=None):
        """Reorders `spheres` (a SPHERE array) in place, like the reference."""
        if not (isinstance(spheres, np.ndarray) and spheres.dtype == SPHERE and spheres.flags.c_contiguous):
            raise TypeError("spheres must be a contiguous SPHERE array (it is reordered in place)")
        nodes = np.zeros(self.capacity, BVH_NODE)
        n = C.c_uint32()
        if device is None:
            st = lib().wfpt_build_bvh(_p(spheres), len(spheres), _p(nodes), len(nodes), C.byref(n))
        else:  # build extension: the same builder on HIP device `device`, same bytes out
            ms = C.c_float()
            st = lib().wfpt_build_bvh_device(_p(spheres), len(spheres), _p(nodes), len(nodes), C.byref(n), device, C.byref(ms))
            self.device_ms = ms.value
        if st != 0:
            raise WfptError(st, "wfpt_build_bvh failed: " + lib().wfpt_last_error(None).decode())
        self.nodes = nodes[:n.value].copy()

    def build_bvh_tree_triangles(self, triangles, n_bins=32, device=None):
        """Build extension: the same builder over a TRIANGLE array (reordered in place), n_bins bins per axis."""
        if not (isinstance(triangles, np.ndarray) and triangles.dtype == TRIANGLE and triangles.flags.c_contiguous):
            raise TypeError("triangles must be a contiguous TRIANGLE array (it is reordered in place)")
        nodes = np.zeros(self.capacity, BVH_NODE)
        n = C.c_uint32()
        if device is None:
            st = lib().wfpt_build_bvh_triangles(_p(triangles), len(triangles), _p(nodes), len(nodes), C.byref(n), n_bins)
        else:
            ms = C.c_float()
            st = lib().wfpt_build_bvh_triangles_device(_p(triangles), len(triangles), _p(nodes), len(nodes), C.byref(n), n_bins,
                                                       device, C.byref(ms))
            self.device_ms = ms.value
        if st != 0:
            raise WfptError(st, "wfpt_build_bvh_triangles failed: " + lib().wfpt_last_error(None).decode())
        self.nodes = nodes[:n.value].copy()


class Camera:
    """wavefront_common/src/camera.rs"""

    def __init__(self, look_from, look_at):
        self.position = np.asarray(look_from, "<f4").copy()
        la = np.asarray(look_at, "<f4")
        pitch, yaw = C.c_float(), C.c_float()
        lib().wfpt_camera_new(_p(self.position), _p(la), C.byref(pitch), C.byref(yaw))
        self.pitch, self.yaw = pitch.value, yaw.value

    @classmethod
    def book_one_final_camera(cls):
        """camera.rs:26-30"""
        return cls((13.0, 2.0, 3.0), (0.0, 0.0, 0.0))

    def get_camera(self):
        return self.position, self.pitch, self.yaw

    def view_transform(self):
        """camera.rs:41-69: 16 floats, column-major."""
        view = np.zeros(16, "<f4")
        lib().wfpt_view_transform(_p(self.position), self.pitch, self.yaw, _p(view))
        return view


class CameraController:
    """wavefront_common/src/camera_controller.rs:8-158"""

    def __init__(self, camera, vfov, defocus_angle, focus_distance, z_near, z_far, speed=4.0, sensitivity=0.1):
        L = lib()
        self.camera = camera
        self._vfov_rad = L.wfpt_to_radians(vfov)
        self.defocus_angle_rad = L.wfpt_to_radians(defocus_angle)
        self.focus_distance = focus_distance
        self.z_near, self.z_far = z_near, z_far
        self.speed, self.sensitivity = speed, sensitivity
        self._amounts = np.zeros(6, "<f4")  # forward, backward, right, left, up, down
        self._rotate = np.zeros(2, "<f4")   # horizontal, vertical

    def copy(self):
        """The reference's controller is `Copy`; hosts edit a copy and hand it to update_camera_controller."""
        other = CameraController.__new__(CameraController)
        other.__dict__.update(self.__dict__)
        cam = Camera.__new__(Camera)
        cam.position, cam.pitch, cam.yaw = self.camera.position.copy(), self.camera.pitch, self.camera.yaw
        other.camera, other._amounts, other._rotate = cam, self._amounts.copy(), self._rotate.copy()
        return other

    def vfov_rad(self):
        return self._vfov_rad

    def set_vfov(self, vfov):
        self._vfov_rad = lib().wfpt_to_radians(vfov)

    def dof(self):
        return self.defocus_angle_rad, self.focus_distance

    def set_defocus_angle(self, defocus_angle):
        self.defocus_angle_rad = lib().wfpt_to_radians(defocus_angle)

    def set_focus_distance(self, focus_distance):
        self.focus_distance = focus_distance

    def process_mouse(self, delta):
        """camera_controller.rs:74-77"""
        self._rotate[:] = delta

    def _press(self, slot, direction):
        self._amounts[slot] = 1.0 if direction == 1 else 0.0

    def move_forward(self, direction):  # camera_controller.rs:95-101
        self._press(0, direction)

    def move_backwards(self, direction):  # :103-109
        self._press(1, direction)

    def move_right(self, direction):  # :111-117
        self._press(2, direction)

    def move_left(self, direction):  # :119-125
        self._press(3, direction)

    def move_up(self, direction):  # :79-85
        self._press(4, direction)

    def move_down(self, direction):  # :87-93
        self._press(5, direction)

    def update_camera(self, dt):
        """camera_controller.rs:125-158"""
        pitch, yaw = C.c_float(self.camera.pitch), C.c_float(self.camera.yaw)
        lib().wfpt_camera_controller_update(_p(self.camera.position), C.byref(pitch), C.byref(yaw), _p(self._amounts),
                                            _p(self._rotate), self.speed, self.sensitivity, dt)
        self.camera.pitch, self.camera.yaw = pitch.value, yaw.value

    def get_clip_planes(self):
        return self.z_near, self.z_far

    def get_GPU_camera(self):
        """camera_controller.rs:66-68, 173-185"""
        cam = np.zeros(1, GPU_CAMERA)
        lib().wfpt_gpu_camera_new(_p(self.camera.position), self.camera.pitch, self.camera.yaw,
                                  self.defocus_angle_rad, self.focus_distance, _p(cam))
        return cam

    def get_view_matrix(self):
        return self.camera.view_transform()


class ProjectionMatrix:
    """wavefront_common/src/projection_matrix.rs"""

    def __init__(self, vfov_rad, aspect_ratio, z_near, z_far):
        self.vfov_rad, self.aspect_ratio, self.z_near, self.z_far = vfov_rad, aspect_ratio, z_near, z_far

    def p_inv(self):
        out = np.zeros(16, "<f4")
        lib().wfpt_p_inv(self.vfov_rad, self.aspect_ratio, self.z_near, self.z_far, _p(out))
        return out


class RenderParameters:
    """wavefront_common/src/parameters.rs:7-58"""

    def __init__(self, camera_controller, viewport_size):
        self._camera_controller = camera_controller
        self._viewport_size = tuple(viewport_size)
        self._resized = False
        self._camera_changed = False

    def changed(self):
        return self._resized or self._camera_changed

    def resized(self):
        return self._resized

    def camera_changed(self):
        return self._camera_changed

    def set_viewport(self, size):
        self._viewport_size = tuple(size)
        self._resized = True

    def viewport_size(self):
        return self._viewport_size

    def reset(self):
        self._resized = False
        self._camera_changed = False

    def camera_controller(self):
        return self._camera_controller

    def update_camera_controller(self, camera_controller):
        self._camera_controller = camera_controller
        self._camera_changed = True


class RenderProgress:
    """wavefront_common/src/parameters.rs:61-101"""

    def __init__(self):
        self.frame = 0
        self._accumulated_samples = 0

    def get_next_frame(self, rp):
        w, h = rp.viewport_size()
        self.frame += 1
        return GPUFrameBuffer.new(w, h, self.frame)

    def incr_accumulated_samples(self, delta):
        self._accumulated_samples += delta

    def reset(self):
        self._accumulated_samples = 0
        self.frame = 0

    def progress(self):
        return self._accumulated_samples / SPP

    def accumulated_samples(self):
        return self._accumulated_samples


# ------------------------------------------------------------------------------------------------
# kernel-stage API and the wavefront loop
# ------------------------------------------------------------------------------------------------
class Kernel:
    """gpu_wavefront_pt/src/kernel.rs: `Kernel::new(name, ...)`, `run((gx, gy))`, `get_timing()`.

    The reference binds buffers explicitly; here the context owns them (path_tracer.rs:53-128) and the
    stage name selects the binding table of SURVEY.md section 2.2."""

    def __init__(self, name, path_tracer):
        stage = lib().wfpt_stage_from_name(name.encode())
        if stage < 0 or stage >= STAGES["scan"]:
            # kernel.rs:36 unwraps the shader read and panics on an unknown name
            raise WfptError(-1, f"no such kernel stage: {name!r}")
        self.name, self.stage, self._pt = name, stage, path_tracer

    def run(self, workgroup_size):
        gx, gy = workgroup_size
        self._pt._check(lib().wfpt_kernel_run(self._pt.handle, self.stage, gx, gy))

    def get_timing(self):
        """Running mean (microseconds) of the last <= 10 dispatches (query_gpu.rs:26-43)."""
        return lib().wfpt_kernel_timing_us(self._pt.handle, self.stage)


class PathTracer:
    """gpu_wavefront_pt/src/path_tracer.rs. `new` builds the BVH (reordering scene.spheres, path_tracer.rs:117-118)
    and uploads everything; `run()` is the reference's host-driven loop over the five Kernels with blocking
    counter read-backs; `render(spp)` is the same loop resident on the device (no host synchronisation)."""

    def __init__(self, scene, rp, max_window_size=0, max_wavefronts=50, miss_floor=128, rng_mode=RNG_DISPATCH,
                 flags=0, tile_rank=0, tile_world=1, device=0, spp=SPP, batch=0, mesh_bins=32, device_bvh=False, bvh=None):
        """`bvh`: a BVHTree the caller built itself over scene.spheres / scene.triangles AS THEY ARE (the C ABI takes any tree in bvh.rs's
        layout: siblings at (2k, 2k + 1), at most 63 levels); default: built here like path_tracer.rs:117-118 does."""
        L = lib()
        self.handle = None
        self.scene = scene
        self.render_parameters = rp
        self.render_progress = RenderProgress()
        self.spp = spp
        self.max_wavefronts, self.miss_floor = max_wavefronts, miss_floor
        if bvh is not None:
            pass
        elif scene.triangles is not None:
            bvh = BVHTree(len(scene.triangles))
            bvh.build_bvh_tree_triangles(scene.triangles, mesh_bins, device=device if device_bvh else None)
        else:
            bvh = BVHTree(len(scene.spheres))
            bvh.build_bvh_tree(scene.spheres, device=device if device_bvh else None)  # path_tracer.rs:117-118
        self.bvh_tree = bvh
        cc = rp.camera_controller()
        w, h = rp.viewport_size()
        self.width, self.height = w, h
        z_near, z_far = cc.get_clip_planes()
        ar = np.float32(w) / np.float32(h)
        proj = ProjectionMatrix(cc.vfov_rad(), ar, z_near, z_far).p_inv()  # path_tracer.rs:135-138
        view = cc.get_view_matrix()
        cam = cc.get_GPU_camera()
        self._params = _Params(w, h, max_window_size, max_wavefronts, miss_floor, rng_mode, flags,
                               tile_rank, tile_world, device, batch)
        if scene.triangles is not None:
            self.handle = L.wfpt_create_mesh(C.byref(self._params), _p(scene.triangles), len(scene.triangles),
                                             _p(scene.materials), len(scene.materials), _p(bvh.nodes), len(bvh.nodes),
                                             _p(cam), _p(proj), _p(view))
        else:
            self.handle = L.wfpt_create(C.byref(self._params), _p(scene.spheres), len(scene.spheres),
                                        _p(scene.materials), len(scene.materials), _p(bvh.nodes), len(bvh.nodes),
                                        _p(cam), _p(proj), _p(view))
        if not self.handle:
            raise WfptError(-2, L.wfpt_last_error(None).decode())
        self.n_pixels = L.wfpt_n_pixels(self.handle)
        self.ray_capacity = L.wfpt_ray_capacity(self.handle)
        # path_tracer.rs:158-186
        self.generate_ray_kernel = Kernel("generate_rays", self)
        self.extend_kernel = Kernel("extend", self)
        self.shade_kernel = Kernel("shade", self)
        self.miss_kernel = Kernel("miss_kernel", self)
        self.accumulate_kernel = Kernel("accumulate", self)
        self.last_wavefronts = 0

    # ---- plumbing
    def _check(self, status):
        if status != 0:
            raise WfptError(status, lib().wfpt_last_error(self.handle).decode())

    def close(self):
        if self.handle:
            lib().wfpt_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- reference API
    def progress(self):
        return self.render_progress.progress()

    def get_render_parameters(self):
        return self.render_parameters

    def update_render_parameters(self, render_parameters):
        self.render_parameters = render_parameters

    def resize(self, rp):
        self.update_render_parameters(rp)

    def update_buffers(self):
        """path_tracer.rs:240-277"""
        rp = self.render_parameters
        if not rp.changed():
            return
        cc = rp.camera_controller()
        w, h = rp.viewport_size()
        z_near, z_far = cc.get_clip_planes()
        proj = ProjectionMatrix(cc.vfov_rad(), np.float32(w) / np.float32(h), z_near, z_far).p_inv()
        view = cc.get_view_matrix()
        cam = cc.get_GPU_camera()
        self._check(lib().wfpt_update_render_parameters(self.handle, w, h, _p(cam), _p(proj), _p(view)))
        self.width, self.height = w, h
        self.n_pixels = lib().wfpt_n_pixels(self.handle)
        rp.reset()
        self.render_progress.reset()

    def update_scene(self, scene, mesh_bins=32):
        """Build extension (dynamic scenes): replaces the scene of this live context. The BVH is rebuilt on the device
        (reordering scene.spheres / scene.triangles in place, like PathTracer::new does, path_tracer.rs:117-118) and the
        accumulation restarts at frame 1 (update_buffers, path_tracer.rs:240-277)."""
        if scene.triangles is not None:
            self._check(lib().wfpt_update_scene_mesh(self.handle, _p(scene.triangles), len(scene.triangles), _p(scene.materials),
                                                     len(scene.materials), mesh_bins))
        else:
            self._check(lib().wfpt_update_scene(self.handle, _p(scene.spheres), len(scene.spheres), _p(scene.materials),
                                                len(scene.materials)))
        self.scene = scene
        self.bvh_tree = None  # the new tree exists on the device only (the primitives above were reordered to match it)
        self.render_progress.reset()

    def set_frame(self, frame):
        self._check(lib().wfpt_set_frame(self.handle, C.byref(frame)))

    def set_counters(self, values):
        a = np.zeros(16, "<u4")
        a[:len(values)] = values
        self._check(lib().wfpt_set_counters(self.handle, _p(a)))

    def read_counters(self):
        a = np.zeros(16, "<u4")
        self._check(lib().wfpt_read_counters(self.handle, _p(a)))
        return a

    def reset_image(self):
        self._check(lib().wfpt_reset_image(self.handle))

    def reset_accumulated(self):
        self._check(lib().wfpt_reset_accumulated(self.handle))

    def reset_progress(self):
        """RenderProgress::reset + accumulation clear: the next sample is frame 1 again."""
        self._check(lib().wfpt_reset_progress(self.handle))
        self.render_progress.reset()

    def clear_ray_queues(self):
        self._check(lib().wfpt_clear_ray_queues(self.handle))

    def swap_ray_queues(self):
        self._check(lib().wfpt_swap_ray_queues(self.handle))

    def run(self):
        """path_tracer.rs:279-371, host-driven, one sample (SPF = 1) per call until `spp` are accumulated."""
        self.update_buffers()
        if self.render_progress.accumulated_samples() < self.spp:
            frame = self.render_progress.get_next_frame(self.render_parameters)
            for sample_number in range(SPF):
                frame.set_sample_number(sample_number)
                self.set_frame(frame)                                    # :296-297
                self.reset_image()                                       # :305-306
                self.clear_ray_queues()                                  # :309-310
                width, height = self.render_parameters.viewport_size()
                self.set_counters([0, 0, width * height])                # :313-316
                self.generate_ray_kernel.run((width // 8, height // 8))  # :318
                wavefront = 0
                extend_size = workgroup_size_64(width * height)          # :322
                while wavefront < self.max_wavefronts:                   # :323
                    self.extend_kernel.run(extend_size)                  # :325
                    counter = self.read_counters()                       # :327-328
                    num_misses, num_hits = int(counter[0]), int(counter[1])
                    if num_misses < self.miss_floor:                     # :332
                        break
                    counter[2] = 0                                       # :335-336
                    self.set_counters(counter)
                    self.shade_kernel.run(workgroup_size_64(num_hits))   # :339
                    self.miss_kernel.run(workgroup_size_64(num_misses))  # :340
                    num_extension = int(self.read_counters()[2])         # :343-345
                    self.swap_ray_queues()                               # :348
                    extend_size = workgroup_size_64(num_extension)       # :350
                    self.set_counters([0, 0, num_extension, 0])          # :352
                    wavefront += 1
                self.last_wavefronts = wavefront
                self.accumulate_kernel.run(workgroup_size_64(width * height))  # :362
                self.render_progress.incr_accumulated_samples(1)         # :363
                frame.set_sample_number(self.render_progress.accumulated_samples())
                self.set_frame(frame)                                    # :366-367

    # ---- device-resident loop
    def render_sample(self):
        self._check(lib().wfpt_render_sample(self.handle))

    def render(self, spp):
        self._check(lib().wfpt_render(self.handle, spp))

    def render_sample_timed(self):
        ms = np.zeros(STAGE_COUNT, "<f4")
        launches = np.zeros(STAGE_COUNT, "<u4")
        self._check(lib().wfpt_render_sample_timed(self.handle, _p(ms), _p(launches)))
        return ms, launches

    def render_timed(self, n_samples):
        """Like render(n_samples) (same batching) with hipEvent pairs around every launch: (ms, launches) per stage."""
        ms = np.zeros(STAGE_COUNT, "<f4")
        launches = np.zeros(STAGE_COUNT, "<u4")
        self._check(lib().wfpt_render_timed(self.handle, n_samples, _p(ms), _p(launches)))
        return ms, launches

    def synchronize(self):
        self._check(lib().wfpt_synchronize(self.handle))

    # ---- first-hit AOVs (contexts created with FLAG_AOV)
    def _aov_shape(self, name):
        if name not in AOVS:
            raise ValueError(f"unknown AOV {name!r}: one of {sorted(AOVS)}")
        which, ch, dtype = AOVS[name]
        rows = self.n_pixels // self.width
        return which, ((rows, self.width, 3) if ch == 3 else (rows, self.width)), dtype

    def aov(self, name):
        """The resolved AOV `name` (see AOVS) as (h, w, 3) or (h, w): float32, uint32 for the ids. A sharded context holds its own bands."""
        which, shape, dtype = self._aov_shape(name)
        a = np.zeros(shape, dtype)
        self._check(lib().wfpt_read_aov(self.handle, which, _p(a), a.size))
        return a

    def aov_to_tensor(self, name, tensor):
        """Writes AOV `name` into a caller's contiguous device tensor (torch float32 or int32 / uint32 for the ids, as many elements as
        aov(name) has) on the context's device, resolved by the GPU (the same bits as aov(name)). Returns the tensor."""
        which, shape, dtype = self._aov_shape(name)
        n = int(np.prod(shape))
        want = ("float32",) if dtype == "<f4" else ("int32", "uint32")
        dt = str(getattr(tensor, "dtype", "")).replace("torch.", "")
        if dt not in want:
            raise TypeError(f"aov_to_tensor({name!r}): tensor dtype {dt or type(tensor).__name__} is not {' or '.join(want)}")
        if tensor.numel() != n:
            raise ValueError(f"aov_to_tensor({name!r}): tensor has {tensor.numel()} elements, the AOV {n} {shape}")
        if not tensor.is_contiguous():
            raise ValueError(f"aov_to_tensor({name!r}): tensor is not contiguous")
        if getattr(tensor, "device", None) is None or tensor.device.type != "cuda" or tensor.device.index != self._params.device:
            raise ValueError(f"aov_to_tensor({name!r}): tensor must live on this context's device (cuda:{self._params.device})")
        self._check(lib().wfpt_copy_aov_to_device(self.handle, which, C.c_void_p(tensor.data_ptr()), 4 * n))
        return tensor

    def _timing(self, entry):
        """(milliseconds, count) as one of the wfpt_*_timing_ms entry points reports them."""
        ms, n = C.c_float(0.0), C.c_uint32(0)
        self._check(entry(self.handle, C.byref(ms), C.byref(n)))
        return float(ms.value), int(n.value)

    def aov_timing(self):
        """(milliseconds, launches) of the AOV launches of every timed render since creation (apart from render_timed's stage times)."""
        return self._timing(lib().wfpt_aov_timing_ms)

    # ---- denoiser (contexts created with FLAG_DENOISE)
    def variance(self):
        """(h, w) float32: the variance of each pixel's n-sample mean luminance, from the per-pixel moments (0 before any sample)."""
        a = np.zeros((self.n_pixels // self.width, self.width), "<f4")
        self._check(lib().wfpt_read_variance(self.handle, _p(a), a.size))
        return a

    @staticmethod
    def _denoise_params(params):
        unknown = set(params) - set(DENOISE_DEFAULTS)
        if unknown:
            raise TypeError(f"unknown denoise parameter(s) {sorted(unknown)}: one of {sorted(DENOISE_DEFAULTS)}")
        v = {**DENOISE_DEFAULTS, **params}
        return _DenoiseParams(int(v["iterations"]), v["sigma_luminance"], v["sigma_normal"], v["sigma_depth"], v["sigma_albedo"])

    def denoise(self, **params):
        """(h, w, 3) float32: the denoised mean colour (not a sum). Parameters as DENOISE_DEFAULTS; iterations=0 gives accumulated / n."""
        p = self._denoise_params(params)
        a = np.zeros((self.n_pixels // self.width, self.width, 3), "<f4")
        self._check(lib().wfpt_denoise(self.handle, C.byref(p), _p(a), a.size))
        return a

    def denoise_to_tensor(self, tensor, **params):
        """Writes denoise(**params) into a caller's contiguous float32 device tensor of h * w * 3 elements on the context's device (the
        same bits as denoise()). Returns the tensor."""
        p = self._denoise_params(params)
        n = self.n_pixels * 3
        dt = str(getattr(tensor, "dtype", "")).replace("torch.", "")
        if dt != "float32":
            raise TypeError(f"denoise_to_tensor: tensor dtype {dt or type(tensor).__name__} is not float32")
        if tensor.numel() != n:
            raise ValueError(f"denoise_to_tensor: tensor has {tensor.numel()} elements, the image {n}")
        if not tensor.is_contiguous():
            raise ValueError("denoise_to_tensor: tensor is not contiguous")
        if getattr(tensor, "device", None) is None or tensor.device.type != "cuda" or tensor.device.index != self._params.device:
            raise ValueError(f"denoise_to_tensor: tensor must live on this context's device (cuda:{self._params.device})")
        self._check(lib().wfpt_denoise_to_device(self.handle, C.byref(p), C.c_void_p(tensor.data_ptr()), 4 * n))
        return tensor

    # ---- tile lists (include/wfpt.h "Tile lists")
    def read_tile_lists(self):
        """The context's per-tile candidate lists as uint32 [tiles, TILE_LIST_CAP] (blocking; see tile_lists_host), or None where
        the context keeps none (its first launch walks the tree for every tile)."""
        n = C.c_uint32(0)
        self._check(lib().wfpt_debug_read_tile_lists(self.handle, None, C.byref(n)))
        if n.value == 0:
            return None
        out = np.zeros((n.value, TILE_LIST_CAP), np.uint32)
        self._check(lib().wfpt_debug_read_tile_lists(self.handle, _p(out), C.byref(n)))
        return out

    def tile_lists_timing(self):
        """(milliseconds of the last build of the tile lists on the device, builds since creation)."""
        return self._timing(lib().wfpt_tile_lists_timing_ms)

    def denoise_timing(self):
        """(milliseconds of the last denoise call's launches, denoise calls since creation)."""
        return self._timing(lib().wfpt_denoise_timing_ms)

    # ---- temporal denoiser (contexts created with FLAG_DENOISE; include/wfpt.h "Temporal denoiser")
    def set_frame_offset(self, offset):
        """The device-resident loop's RNG frame offset: the next samples render frames wfpt_frame() + 1 + offset, ... (uint32). An
        interactive host sets it to the samples rendered so far after each camera move, so a new pose does not replay the random streams
        of the last one. No reset clears it; run() (the stage API) ignores it."""
        self._check(lib().wfpt_set_frame_offset(self.handle, int(offset) & 0xFFFFFFFF))

    @property
    def frame_offset(self):
        return int(lib().wfpt_frame_offset(self.handle))

    @staticmethod
    def _temporal_params(params):
        unknown = set(params) - set(TEMPORAL_DEFAULTS)
        if unknown:
            raise TypeError(f"unknown temporal denoise parameter(s) {sorted(unknown)}: one of {sorted(TEMPORAL_DEFAULTS)}")
        v = {**TEMPORAL_DEFAULTS, **params}
        spatial = PathTracer._denoise_params({k: v[k] for k in DENOISE_DEFAULTS})
        return _TemporalParams(spatial, v["history_cap"], v["depth_tolerance"], v["normal_cos"])

    def denoise_temporal(self, **params):
        """(h, w, 3) float32: the denoised mean colour with the reprojected history of earlier epochs blended in. Parameters as
        TEMPORAL_DEFAULTS; history_cap=0 gives denoise()'s bits."""
        p = self._temporal_params(params)
        a = np.zeros((self.n_pixels // self.width, self.width, 3), "<f4")
        self._check(lib().wfpt_denoise_temporal(self.handle, C.byref(p), _p(a), a.size))
        return a

    def denoise_temporal_to_tensor(self, tensor, **params):
        """Writes denoise_temporal(**params) into a caller's contiguous float32 device tensor of h * w * 3 elements on the context's device
        (the same bits). Returns the tensor."""
        p = self._temporal_params(params)
        n = self.n_pixels * 3
        dt = str(getattr(tensor, "dtype", "")).replace("torch.", "")
        if dt != "float32":
            raise TypeError(f"denoise_temporal_to_tensor: tensor dtype {dt or type(tensor).__name__} is not float32")
        if tensor.numel() != n:
            raise ValueError(f"denoise_temporal_to_tensor: tensor has {tensor.numel()} elements, the image {n}")
        if not tensor.is_contiguous():
            raise ValueError("denoise_temporal_to_tensor: tensor is not contiguous")
        if getattr(tensor, "device", None) is None or tensor.device.type != "cuda" or tensor.device.index != self._params.device:
            raise ValueError(f"denoise_temporal_to_tensor: tensor must live on this context's device (cuda:{self._params.device})")
        self._check(lib().wfpt_denoise_temporal_to_device(self.handle, C.byref(p), C.c_void_p(tensor.data_ptr()), 4 * n))
        return tensor

    def temporal(self, name):
        """State of the last temporal call, float32: "color" (h, w, 3) c before the passes, "moments" (h, w, 2) (m1, m2), "length" (h, w)
        the history length L, "motion" (h, w, 3) (x', y', z'), (-1e30, -1e30, 0) where there was no projection."""
        if name not in TEMPORAL_OUTPUTS:
            raise KeyError(f"unknown temporal output {name!r}: one of {sorted(TEMPORAL_OUTPUTS)}")
        which, ch = TEMPORAL_OUTPUTS[name]
        h = self.n_pixels // self.width
        a = np.zeros((h, self.width, ch) if ch > 1 else (h, self.width), "<f4")
        self._check(lib().wfpt_read_temporal(self.handle, which, _p(a), a.size))
        return a

    def reset_history(self):
        """The next denoise_temporal() call has no history."""
        self._check(lib().wfpt_reset_history(self.handle))

    def temporal_timing(self):
        """(milliseconds of the last temporal call's launches, temporal calls since creation)."""
        return self._timing(lib().wfpt_temporal_timing_ms)

    # ---- environment map (contexts created with FLAG_ENVIRONMENT; include/wfpt.h "Environment map")
    def set_environment(self, rgb, intensity=1.0, rotation=0.0):
        """Lights every miss with the map `rgb`, an (h, w, 3) float32 array (row 0 = up, column w/2 faces -z; finite, >= 0), times
        `intensity`, turned by `rotation` (in turns, [0, 1)). Restarts the accumulation like a scene update."""
        a = np.ascontiguousarray(rgb, "<f4")
        if a.ndim != 3 or a.shape[2] != 3:
            raise ValueError(f"set_environment: expected an (h, w, 3) array, got shape {a.shape}")
        p = _EnvironmentParams(float(intensity), float(rotation))
        self._check(lib().wfpt_set_environment(self.handle, _p(a), a.shape[1], a.shape[0], C.byref(p)))
        self._env_shape = (a.shape[0], a.shape[1])

    def clear_environment(self):
        """Back to the gradient sky (restarts the accumulation)."""
        self._check(lib().wfpt_clear_environment(self.handle))
        self._env_shape = None

    def _probe(self, fn, name, rows, in_width, out_width, *leading):
        """A device probe: fn(handle, *leading, rows, n, out) with `rows` as (n, in_width) float32; returns out, (n, out_width) float32."""
        a = np.ascontiguousarray(rows, "<f4")
        if a.ndim != 2 or a.shape[1] != in_width:
            raise ValueError(f"{name}: expected rows of {in_width} floats, got shape {a.shape}")
        out = np.zeros((a.shape[0], out_width), "<f4")
        self._check(fn(self.handle, *leading, _p(a), a.shape[0], _p(out)))
        return out

    def sample_environment(self, dirs):
        """(n, 3) float32: the map's value (with its intensity) in each of the (n, 3) directions, looked up on the device."""
        return self._probe(lib().wfpt_sample_environment, "sample_environment", np.asarray(dirs, "<f4").reshape(-1, 3), 3, 3)

    # ---- textures (contexts created with FLAG_TEXTURES; include/wfpt.h "Textures")
    def set_texture(self, slot, rgb, scale=(1.0, 1.0), offset=(0.0, 0.0), filter="bilinear"):
        """Puts the (h, w, 3) float32 image `rgb` (linear, row 0 = the top; finite, >= 0) in texture slot `slot`, with the UV transform
        u' = u * scale + offset and the filter "bilinear" or "nearest". Restarts the accumulation like a scene update."""
        a = np.ascontiguousarray(rgb, "<f4")
        if a.ndim != 3 or a.shape[2] != 3:
            raise ValueError(f"set_texture: expected an (h, w, 3) array, got shape {a.shape}")
        if filter not in TEXTURE_FILTERS:
            raise ValueError(f"set_texture: filter must be one of {sorted(TEXTURE_FILTERS)}")
        p = _TextureParams((C.c_float * 2)(*scale), (C.c_float * 2)(*offset), TEXTURE_FILTERS[filter])
        self._check(lib().wfpt_set_texture(self.handle, slot, _p(a), a.shape[1], a.shape[0], C.byref(p)))

    def clear_texture(self, slot):
        """Empties the slot and unbinds the materials bound to it."""
        self._check(lib().wfpt_clear_texture(self.handle, slot))

    def bind_texture(self, material_idx, slot):
        """Material `material_idx` is textured by slot `slot` (which must hold a texture); None or -1 unbinds it."""
        self._check(lib().wfpt_bind_texture(self.handle, material_idx, -1 if slot is None else slot))

    def set_triangle_uvs(self, uv):
        """The UV table: (n, 6) rows u0 v0 u1 v1 u2 v2; a triangle uses the row its _pad names. None clears it."""
        if uv is None:
            self._check(lib().wfpt_set_triangle_uvs(self.handle, None, 0))
            return
        a = np.ascontiguousarray(uv, "<f4").reshape(-1, 6)
        self._check(lib().wfpt_set_triangle_uvs(self.handle, _p(a), a.shape[0]))

    def sample_texture(self, slot, uv):
        """(n, 3) float32: the texture of slot `slot` at each of the (n, 2) UVs, looked up on the device."""
        return self._probe(lib().wfpt_sample_texture, "sample_texture", np.asarray(uv, "<f4").reshape(-1, 2), 2, 3, slot)

    def texture_timing(self):
        """(milliseconds, launches) of the texture launches of every timed render since creation (apart from render_timed's stage times)."""
        return self._timing(lib().wfpt_texture_timing_ms)

    # ---- shading normals (triangle contexts created with FLAG_SHADING_NORMALS; include/wfpt.h "Shading normals")
    def set_triangle_normals(self, n):
        """The table of corner normals: (n, 9) rows of the normals of corners 0, 1, 2 (finite; normalised as stored); a triangle uses the
        row its _pad names. None clears it. Restarts the accumulation like a scene update."""
        if n is None:
            self._check(lib().wfpt_set_triangle_normals(self.handle, None, 0))
        else:
            a = np.ascontiguousarray(n, "<f4").reshape(-1, 9)
            self._check(lib().wfpt_set_triangle_normals(self.handle, _p(a), a.shape[0]))
        self.render_progress.reset()

    def triangle_normals(self):
        """The table as stored, (n, 9) float32 (n = 0: none is set)."""
        n = C.c_uint32(0)
        self._check(lib().wfpt_get_triangle_normals(self.handle, None, 0, C.byref(n)))
        out = np.zeros((int(n.value), 9), "<f4")
        if len(out):
            self._check(lib().wfpt_get_triangle_normals(self.handle, _p(out), len(out), C.byref(n)))
        return out

    def sample_shading_normal(self, rows):
        """The shading normal for caller-supplied hits, computed on the device. rows: (n, 4) float32 of (p.xyz, the triangle's index in the
        device's order as the BITS of the fourth float); returns (n, 4) float32 of (ns.xyz, 1.0 where it fell back to the stored normal)."""
        return self._probe(lib().wfpt_sample_shading_normal, "sample_shading_normal", rows, 4, 4)

    def shading_normal_timing(self):
        """(milliseconds, launches) of the shading-normal launches of every timed render since creation (apart from render_timed's stage times)."""
        return self._timing(lib().wfpt_shading_normal_timing_ms)

    # ---- microfacet metals (triangle contexts created with FLAG_MICROFACET; include/wfpt.h "Microfacet metals")
    def set_roughness(self, material_idx, alpha):
        """Material `material_idx` gets the GGX roughness `alpha` in [0, 1]: its metal primitives are shaded as rough conductors. 0 makes it
        an ordinary material again. Restarts the accumulation like a scene update."""
        self._check(lib().wfpt_set_roughness(self.handle, _material_index(material_idx), float(alpha)))
        self.render_progress.reset()

    def get_roughness(self, material_idx):
        """The roughness of material `material_idx` (0.0: none)."""
        out = C.c_float(0.0)
        self._check(lib().wfpt_get_roughness(self.handle, _material_index(material_idx), C.byref(out)))
        return float(out.value)

    def clear_roughness(self):
        """Every material back to roughness 0."""
        self._check(lib().wfpt_clear_roughness(self.handle))
        self.render_progress.reset()

    def sample_microfacet(self, rows):
        """The microfacet pass's sampler for caller-supplied hits, computed on the device. rows: (n, 12) float32 of (d.xyz, n.xyz, u1, u2,
        alpha, F0.rgb); returns (n, 8) float32 of (m.xyz, 2.0 where the hit fell back to its plain shading / 1.0 where the weight is zero /
        else 0.0, weight.rgb, cm)."""
        return self._probe(lib().wfpt_sample_microfacet, "sample_microfacet", rows, 12, 8)

    def sample_rough_dielectric(self, rows):
        """The rough-dielectric sampler of a FLAG_ROUGH_DIELECTRIC context for caller-supplied hits, computed on the device. rows: (n, 16)
        float32 of (d.xyz, n.xyz, u1, u2, u3, alpha, ior, albedo.rgb, 0, 0); returns (n, 8) float32 of (h.xyz, 2.0 where the hit fell back
        to its plain shading / 1.0 where the weight is zero / else 0.0, weight.rgb, 1.0 refracted / 0.0 reflected)."""
        return self._probe(lib().wfpt_sample_rough_dielectric, "sample_rough_dielectric", rows, 16, 8)

    def microfacet_timing_ms(self):
        """(milliseconds, launches) of the microfacet launches of every timed render since creation (apart from render_timed's stage times)."""
        return self._timing(lib().wfpt_microfacet_timing_ms)

    # ---- normal maps (triangle contexts created with FLAG_NORMAL_MAPS; include/wfpt.h "Normal maps")
    def bind_normal_map(self, material_idx, slot, strength=1.0):
        """Material `material_idx` takes the texture of slot `slot` (linear texels, rgb = 0.5 + 0.5 * the tangent-space normal, green = +v)
        as its normal map at `strength` (finite, >= 0); None or -1 unbinds it. Restarts the accumulation like a scene update."""
        self._check(lib().wfpt_bind_normal_map(self.handle, _material_index(material_idx), -1 if slot is None else slot, float(strength)))
        self.render_progress.reset()

    def normal_map(self, material_idx):
        """(slot, strength) of the material's normal-map binding; (None, 0.0) where it has none."""
        slot, strength = C.c_int32(-1), C.c_float(0.0)
        self._check(lib().wfpt_get_normal_map(self.handle, _material_index(material_idx), C.byref(slot), C.byref(strength)))
        return (None if slot.value < 0 else int(slot.value)), float(strength.value)

    def sample_normal_map(self, rows):
        """The mapped normal for caller-supplied hits, computed on the device. rows: (n, 4) float32 of (p.xyz, the triangle's index in the
        device's order as the BITS of the fourth float); returns (n, 4) float32 of (n.xyz, code): 0 mapped, 1 identity, 2 no tangent
        frame, 3 rejected, 4 the material has no map, 5 an index outside the scene."""
        return self._probe(lib().wfpt_sample_normal_map, "sample_normal_map", rows, 4, 4)

    # ---- roughness maps (triangle contexts created with FLAG_ROUGHNESS_MAPS; include/wfpt.h "Roughness maps")
    def bind_roughness_map(self, material_idx, slot, channel=1, remap="linear"):
        """Material `material_idx` takes channel `channel` (0, 1, 2 = r, g, b) of the texture of slot `slot` as its roughness map: a hit
        is sampled with set_roughness' alpha times min(texel, 1), squared first where remap is "squared" (glTF's perceptual roughness).
        None or -1 unbinds it. Restarts the accumulation like a scene update."""
        self._check(lib().wfpt_bind_roughness_map(self.handle, _material_index(material_idx), -1 if slot is None else slot, int(channel),
                                                  _remap_value(remap)))
        self.render_progress.reset()

    def get_roughness_map(self, material_idx):
        """(slot, channel, remap) of the material's roughness binding; (None, 0, "linear") where it has none."""
        slot, channel, remap = C.c_int32(-1), C.c_uint32(0), C.c_uint32(0)
        self._check(lib().wfpt_get_roughness_map(self.handle, _material_index(material_idx), C.byref(slot), C.byref(channel), C.byref(remap)))
        return (None if slot.value < 0 else int(slot.value)), int(channel.value), ROUGHNESS_REMAPS[remap.value]

    def sample_roughness_map(self, rows):
        """The per-hit alpha for caller-supplied hits, computed on the device. rows: (n, 4) float32 of (p.xyz, the triangle's index in the
        device's order as the BITS of the fourth float); returns (n, 4) float32 of (alpha_h, r, code, 0): 0 mapped, 1 the material has no
        roughness binding, 2 its alpha is not above 0, 3 mapped and alpha_h is not above 0, 5 an index outside the scene."""
        return self._probe(lib().wfpt_sample_roughness_map, "sample_roughness_map", rows, 4, 4)

    # ---- emission (contexts created with FLAG_EMISSION; include/wfpt.h "Emission")
    def set_emission(self, material_idx, rgb):
        """Material `material_idx` emits the colour `rgb` (3 floats, finite, >= 0) and ends the paths that hit it; all zeros makes it an
        ordinary material again. Restarts the accumulation like a scene update."""
        self._check(lib().wfpt_set_emission(self.handle, _material_index(material_idx), _emission_colour(rgb)))
        self.render_progress.reset()

    def emission(self, material_idx):
        """The (3,) float32 emission colour of material `material_idx` (zeros: not an emitter)."""
        out = (C.c_float * 3)()
        self._check(lib().wfpt_get_emission(self.handle, _material_index(material_idx), out))
        return np.array(out[:], "<f4")

    def clear_emission(self):
        """No material emits."""
        self._check(lib().wfpt_clear_emission(self.handle))
        self.render_progress.reset()

    def emission_timing(self):
        """(milliseconds, launches) of the emission launches of every timed render since creation (apart from render_timed's stage times)."""
        return self._timing(lib().wfpt_emission_timing_ms)

    # ---- next-event estimation (contexts created with FLAG_EMISSION | FLAG_NEE; include/wfpt.h "Next-event estimation")
    def nee_light_count(self):
        """The number of emitting primitives (the light list the connect pass samples), 0 with none."""
        n = lib().wfpt_nee_light_count(self.handle)
        if n < 0:
            self._check(n)
        return int(n)

    def nee_timing(self):
        """(milliseconds, launches) of the connect launches of every timed render since creation (apart from render_timed's stage times)."""
        return self._timing(lib().wfpt_nee_timing_ms)

    def sample_lights(self, rows):
        """The connect pass's light sample for caller-supplied receivers, computed on the device. rows: (n, 9) float32 of (p.xyz, n.xyz,
        u0, u1, u2); returns (n, 8) float32 of (q.xyz, the light's primitive index, the unoccluded factor e_q * G per channel, occluded 0/1)."""
        return self._probe(lib().wfpt_sample_lights, "sample_lights", rows, 9, 8)

    # ---- light selection by power (contexts created with FLAG_EMISSION | FLAG_NEE | FLAG_LIGHT_POWER; include/wfpt.h "Light selection by power")
    def light_distribution(self):
        """(light_prims, cdf) of the light list's sampling distribution: light_prims (n_l,) uint32, the emitting primitives in list order,
        and cdf (n_l,) uint64, the inclusive prefix sums of their integer weights. Raises while the list has no distribution."""
        n = self.nee_light_count()
        prims, cdf = np.zeros(n, "<u4"), np.zeros(n, "<u8")
        self._check(lib().wfpt_read_light_distribution(self.handle, _p(prims), _p(cdf)))
        return prims, cdf

    # ---- analytic lights (contexts created with FLAG_EMISSION | FLAG_NEE | FLAG_ANALYTIC_LIGHTS; include/wfpt.h "Analytic lights")
    def set_lights(self, lights):
        """The context's point, spot and directional lights: a LIGHT array (or None / empty: none). Directions are normalised at the call.
        Restarts the accumulation like a scene update."""
        a = np.zeros(0, LIGHT) if lights is None else np.ascontiguousarray(lights, LIGHT).reshape(-1)
        self._check(lib().wfpt_set_lights(self.handle, _p(a) if len(a) else None, len(a)))
        self.render_progress.reset()

    def lights(self):
        """The analytic lights as stored (directions normalised): a LIGHT array."""
        out = np.zeros(self.analytic_light_count(), LIGHT)
        n = C.c_uint32(0)
        self._check(lib().wfpt_get_lights(self.handle, _p(out) if len(out) else None, len(out), C.byref(n)))
        return out[:int(n.value)]

    get_lights = lights

    def analytic_light_count(self):
        """The number of analytic lights, 0 with none."""
        n = lib().wfpt_analytic_light_count(self.handle)
        if n < 0:
            self._check(n)
        return int(n)

    # ---- environment next-event estimation (contexts created with FLAG_ENVIRONMENT | FLAG_EMISSION | FLAG_NEE | FLAG_ENV_NEE)
    def set_environment_share(self, share):
        """The probability, in (0, 1], with which a diffuse hit connects to the map rather than to an emitter (0.5 by default; with no
        emitter every hit connects to the map). Restarts the accumulation."""
        self._check(lib().wfpt_set_environment_share(self.handle, float(share)))

    def environment_share(self):
        return float(lib().wfpt_environment_share(self.handle))

    def environment_distribution(self):
        """(row, marg) of the map's sampling distribution: row (h, w) uint32, the prefix sums of the integer texel weights along each row,
        and marg (h,) uint64, the prefix sums of the row totals. Raises while no map with a distribution is set."""
        h, w = getattr(self, "_env_shape", None) or (1, 1)
        row, marg = np.zeros((h, w), "<u4"), np.zeros(h, "<u8")
        self._check(lib().wfpt_read_environment_distribution(self.handle, _p(row), _p(marg)))
        return row, marg

    def sample_environment_light(self, rows):
        """The connect pass's sample of the map (its environment branch with p = 1) for caller-supplied receivers, computed on the device.
        rows: (n, 10) float32 of (p.xyz, n.xyz, u1, u2, u3, u4); returns (n, 8) float32 of (wdir.xyz, the texel index y * w + x, the
        unoccluded factor e * Genv per channel, occluded 0/1)."""
        return self._probe(lib().wfpt_sample_environment_light, "sample_environment_light", rows, 10, 8)

    # ---- multiple importance sampling (contexts created with FLAG_EMISSION | FLAG_NEE | FLAG_MIS; include/wfpt.h "Multiple importance sampling")
    def sample_lights_mis(self, rows):
        """The connect pass's weighed light sample for caller-supplied receivers, computed on the device. rows: (n, 9) float32 as for
        sample_lights; returns (n, 12) float32 of (q.xyz, the light's primitive index, (e_q * G) * wl per channel, occluded 0/1, pl, pb, wl, 0)."""
        return self._probe(lib().wfpt_sample_lights_mis, "sample_lights_mis", rows, 9, 12)

    def mis_hit_weight(self, rows):
        """The emission pass's weight for caller-supplied hits, computed on the device. rows: (n, 8) float32 of (o.xyz, d.xyz, t, the
        primitive index); returns (n, 4) float32 of (pl, pb, wb, cos_l)."""
        return self._probe(lib().wfpt_mis_hit_weight, "mis_hit_weight", rows, 8, 4)

    # ---- environment multiple importance sampling (FLAG_ENV_NEE's four flags | FLAG_ENV_MIS; include/wfpt.h "Environment multiple importance sampling")
    def sample_environment_light_mis(self, rows):
        """The connect pass's weighed sample of the map, with the context's effective share p, for caller-supplied receivers, computed on
        the device. rows: (n, 10) float32 as for sample_environment_light; returns (n, 12) float32 of (wdir.xyz, the texel index
        y * w + x, (e * Genv) * we per channel, occluded 0/1, pe, pb, we, 0)."""
        return self._probe(lib().wfpt_sample_environment_light_mis, "sample_environment_light_mis", rows, 10, 12)

    def env_mis_miss_weight(self, dirs):
        """The miss pass's weight for caller-supplied un-normalised directions, computed on the device. dirs: (n, 3) float32; returns
        (n, 4) float32 of (pe, pb, wb, the texel index yt * w + xt)."""
        return self._probe(lib().wfpt_env_mis_miss_weight, "env_mis_miss_weight", dirs, 3, 4)

    # ---- path termination (contexts created with FLAG_RETIRE; include/wfpt.h "Path termination")
    def set_termination(self, roulette_start=3, q_min=0.05):
        """Russian roulette from wavefront `roulette_start` on (NO_ROULETTE: never) with the survival probability's floor `q_min`, in
        (0, 1]. Restarts the accumulation."""
        p = _TerminationParams(int(roulette_start) & 0xFFFFFFFF, float(q_min))
        self._check(lib().wfpt_set_termination(self.handle, C.byref(p)))
        self.render_progress.reset()

    def termination(self):
        """(roulette_start, q_min) of the context."""
        p = _TerminationParams()
        self._check(lib().wfpt_get_termination(self.handle, C.byref(p)))
        return int(p.roulette_start), float(p.q_min)

    def sample_termination(self, thr, pixel_idx, frame, b):
        """The termination step for caller-supplied hits of wavefront `b` of the sample with frame `frame`, computed on the device.
        thr: (n, 3) float32 of t' = thr * albedo; pixel_idx: (n,) uint32; returns (n, 8) float32 of (q, u, verdict, 0, thr'.rgb, 0) with
        verdict 0 = retired dead, 1 = retired by roulette, 2 = survives."""
        thr = np.ascontiguousarray(thr, "<f4").reshape(-1, 3)
        pix = np.ascontiguousarray(pixel_idx, "<u4").reshape(-1)
        if len(pix) != len(thr):
            raise ValueError("sample_termination: thr and pixel_idx differ in length")
        out = np.zeros((len(thr), 8), "<f4")
        self._check(lib().wfpt_sample_termination(self.handle, _p(thr), _p(pix), int(frame) & 0xFFFFFFFF, int(b) & 0xFFFFFFFF, len(thr), _p(out)))
        return out

    # ---- adaptive sampling (contexts created with FLAG_ADAPTIVE; include/wfpt.h "Adaptive sampling")
    def set_adaptive(self, **params):
        """The update's parameters, as ADAPTIVE_DEFAULTS (those not named keep their defaults). Neither resets the accumulation nor drops
        the graphs."""
        unknown = set(params) - set(ADAPTIVE_DEFAULTS)
        if unknown:
            raise TypeError(f"unknown adaptive parameter(s) {sorted(unknown)}: one of {sorted(ADAPTIVE_DEFAULTS)}")
        v = {**ADAPTIVE_DEFAULTS, **params}
        p = _AdaptiveParams(int(v["min_samples"]), int(v["max_samples"]), float(v["threshold"]), float(v["luminance_floor"]), int(v["dilate"]))
        self._check(lib().wfpt_set_adaptive(self.handle, C.byref(p)))

    def adaptive(self):
        """The context's update parameters as a dict like ADAPTIVE_DEFAULTS."""
        p = _AdaptiveParams()
        self._check(lib().wfpt_get_adaptive(self.handle, C.byref(p)))
        return {"min_samples": int(p.min_samples), "max_samples": int(p.max_samples), "threshold": float(p.threshold),
                "luminance_floor": float(p.luminance_floor), "dilate": int(p.dilate)}

    def adaptive_update(self):
        """Computes the next active mask from the moments on the device; returns the number of active pixels (blocking)."""
        n = C.c_uint32(0)
        self._check(lib().wfpt_adaptive_update(self.handle, C.byref(n)))
        return int(n.value)

    def set_active_mask(self, mask):
        """A caller's mask: one value per pixel of the context (any shape of n_pixels elements), non-zero = active."""
        m = np.ascontiguousarray(np.asarray(mask) != 0, np.uint8).reshape(-1)
        self._check(lib().wfpt_set_active_mask(self.handle, _p(m), m.size))

    def active_mask(self):
        """(h, w) bool: the pixels the next render adds samples to. A sharded context holds its own bands."""
        m = np.zeros(self.n_pixels, np.uint8)
        self._check(lib().wfpt_read_active_mask(self.handle, _p(m), m.size))
        return m.reshape(self.n_pixels // self.width, self.width).astype(bool)

    def sample_counts(self):
        """(h, w) uint32: the samples added to each pixel since the last reset."""
        a = np.zeros((self.n_pixels // self.width, self.width), "<u4")
        self._check(lib().wfpt_read_sample_counts(self.handle, _p(a), a.size))
        return a

    def mean(self):
        """(n_pixels, 3) float32: accumulated / count per pixel, 0 where the count is 0."""
        a = np.zeros((self.n_pixels, 3), "<f4")
        self._check(lib().wfpt_read_mean(self.handle, _p(a), a.size))
        return a

    def mean_to_tensor(self, tensor):
        """Writes mean() into a caller's contiguous float32 device tensor of n_pixels * 3 elements on the context's device, resolved by
        the GPU (the same bits as mean()). Returns the tensor."""
        n = self.n_pixels * 3
        dt = str(getattr(tensor, "dtype", "")).replace("torch.", "")
        if dt != "float32":
            raise TypeError(f"mean_to_tensor: tensor dtype {dt or type(tensor).__name__} is not float32")
        if tensor.numel() != n:
            raise ValueError(f"mean_to_tensor: tensor has {tensor.numel()} elements, the image {n}")
        if not tensor.is_contiguous():
            raise ValueError("mean_to_tensor: tensor is not contiguous")
        if getattr(tensor, "device", None) is None or tensor.device.type != "cuda" or tensor.device.index != self._params.device:
            raise ValueError(f"mean_to_tensor: tensor must live on this context's device (cuda:{self._params.device})")
        self._check(lib().wfpt_copy_mean_to_device(self.handle, C.c_void_p(tensor.data_ptr()), 4 * n))
        return tensor

    def render_adaptive(self, max_passes, interval):
        """render(interval) and adaptive_update() in turn until no pixel is active or max_passes sample passes are done; returns the
        number of pixels still active."""
        n = C.c_uint32(0)
        self._check(lib().wfpt_render_adaptive(self.handle, int(max_passes), int(interval), C.byref(n)))
        return int(n.value)

    # ---- read-back
    def accumulated(self):
        a = np.zeros((self.n_pixels, 3), "<f4")
        self._check(lib().wfpt_read_accumulated(self.handle, _p(a), a.size))
        return a

    def image(self):
        a = np.zeros((self.n_pixels, 3), "<f4")
        self._check(lib().wfpt_read_image(self.handle, _p(a), a.size))
        return a

    def copy_accumulated_to_device(self, device_ptr, n_bytes):
        self._check(lib().wfpt_copy_accumulated_to_device(self.handle, C.c_void_p(device_ptr), n_bytes))

    # ---- multi-GPU gather (RCCL behind the C ABI)
    def comm_init(self, unique_id, rank, world):
        """Collective over all ranks: joins the RCCL communicator named by `unique_id` (128 bytes from comm_unique_id())."""
        buf = np.frombuffer(bytes(unique_id), np.uint8).copy()
        self._check(lib().wfpt_comm_init(self.handle, _p(buf), rank, world))

    def gather_accumulated(self):
        """Every rank: its slab goes to rank 0 over xGMI (asynchronous on the context's stream)."""
        self._check(lib().wfpt_gather_accumulated(self.handle))

    def gather_accumulated_timed(self):
        """The same gather, blocking; returns its duration on this rank in milliseconds (hipEvents on the context's stream)."""
        ms = C.c_float(0.0)
        self._check(lib().wfpt_gather_accumulated_timed(self.handle, C.byref(ms)))
        return float(ms.value)

    @property
    def loop_kind(self):
        """Which loop render() enqueues: "stages", "fused", "fused_binned" or "refill" (wfpt_loop_kind_of)."""
        k = lib().wfpt_loop_kind_of(self.handle)
        if k < 0:
            self._check(k)
        return LOOP_KINDS[k]

    def gathered(self):
        """Rank 0: the assembled (width * height, 3) accumulated frame."""
        a = np.zeros((self.width * self.height, 3), "<f4")
        self._check(lib().wfpt_read_gathered(self.handle, _p(a), a.size))
        return a

    def rays(self, n):
        a = np.zeros(n, RAY)
        self._check(lib().wfpt_read_rays(self.handle, _p(a), n))
        return a

    def extension_rays(self, n):
        a = np.zeros(n, RAY)
        self._check(lib().wfpt_read_extension_rays(self.handle, _p(a), n))
        return a

    def write_rays(self, rays):
        a = np.ascontiguousarray(rays, RAY)
        self._check(lib().wfpt_write_rays(self.handle, _p(a), len(a)))

    def hits(self, n):
        a = np.zeros(n, HIT)
        self._check(lib().wfpt_read_hits(self.handle, _p(a), n))
        return a

    def misses(self, n):
        a = np.zeros(n, "<u4")
        self._check(lib().wfpt_read_misses(self.handle, _p(a), n))
        return a

    def save_ppm(self, path):
        """8-bit P6 of sqrt(accumulated / samples), the display shader's tone map (display_shader.wgsl:50-52)."""
        self._check(lib().wfpt_save_ppm(self.handle, os.fsencode(path)))

    def save_png(self, path):
        """The tone-mapped frame (display_shader.wgsl:50-52) as an 8-bit RGB PNG."""
        self._check(lib().wfpt_save_png(self.handle, os.fsencode(path)))

    def save_pfm(self, path):
        """Linear float32 PFM of accumulated / samples."""
        self._check(lib().wfpt_save_pfm(self.handle, os.fsencode(path)))

    def bounce_table(self):
        t = np.zeros((64, 4), "<u4")
        n = C.c_uint32()
        self._check(lib().wfpt_read_bounce_table(self.handle, _p(t), 64, C.byref(n)))
        return t[:n.value].copy()

    def totals(self):
        t = np.zeros(3, "<u8")
        self._check(lib().wfpt_read_totals(self.handle, _p(t)))
        return t

    def wavefront_totals(self):
        """(rays traced, hits, misses) per wavefront, summed over every sample rendered by the device-resident loop."""
        t = np.zeros((64, 3), "<u8")
        n = C.c_uint32()
        self._check(lib().wfpt_read_wavefront_totals(self.handle, _p(t), 64, C.byref(n)))
        return t[:n.value].copy()


def render_chunked(scene, rp, spp, chunks, max_wavefronts=50, miss_floor=128, rng_mode=RNG_PIXEL, flags=0, device=0, batch=0,
                   mesh_bins=32):
    """wfpt_render_chunked: the frame as `chunks` band-interleaved slabs rendered one after the other on one GPU (README.md:20),
    assembled on the host; returns the accumulated (width * height, 3) image. Builds the BVH like PathTracer does."""
    L = lib()
    cc = rp.camera_controller()
    w, h = rp.viewport_size()
    z_near, z_far = cc.get_clip_planes()
    proj = ProjectionMatrix(cc.vfov_rad(), np.float32(w) / np.float32(h), z_near, z_far).p_inv()
    view, cam = cc.get_view_matrix(), cc.get_GPU_camera()
    params = _Params(w, h, 0, max_wavefronts, miss_floor, rng_mode, flags, 0, 1, device, batch)
    out = np.zeros((w * h, 3), "<f4")
    if scene.triangles is not None:
        bvh = BVHTree(len(scene.triangles))
        bvh.build_bvh_tree_triangles(scene.triangles, mesh_bins)
        st = L.wfpt_render_chunked_mesh(C.byref(params), _p(scene.triangles), len(scene.triangles), _p(scene.materials), len(scene.materials),
                                        _p(bvh.nodes), len(bvh.nodes), _p(cam), _p(proj), _p(view), spp, chunks, _p(out))
    else:
        bvh = BVHTree(len(scene.spheres))
        bvh.build_bvh_tree(scene.spheres)
        st = L.wfpt_render_chunked(C.byref(params), _p(scene.spheres), len(scene.spheres), _p(scene.materials), len(scene.materials),
                                   _p(bvh.nodes), len(bvh.nodes), _p(cam), _p(proj), _p(view), spp, chunks, _p(out))
    if st != 0:
        raise WfptError(st, L.wfpt_last_error(None).decode())
    return out


def shirley_path_tracer(width, height, seed=1, **kw):
    """main.rs:17-36: seeded Shirley scene, book camera (13,2,3)->origin, vfov 20, defocus 0.6, focus 10."""
    scene = Scene.book_one_final(seed)
    cc = CameraController(Camera.book_one_final_camera(), 20.0, 0.6, 10.0, 0.1, 100.0, 4.0, 0.1)
    return PathTracer(scene, RenderParameters(cc, (width, height)), **kw)


def mesh_path_tracer(width, height, n_triangles, seed=1, **kw):
    """BASELINE config 5: seeded triangle soup, camera (0,0,30) -> origin, vfov 40, no defocus."""
    scene = Scene.random_mesh(n_triangles, seed)
    cc = CameraController(Camera((0.0, 0.0, 30.0), (0.0, 0.0, 0.0)), 40.0, 0.0, 10.0, 0.1, 100.0)
    return PathTracer(scene, RenderParameters(cc, (width, height)), **kw)
