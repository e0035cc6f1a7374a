"""Surface textures (WFPT_FLAG_TEXTURES) without a GPU: the ABI's layout, wfpt_load_obj_uv, UV rows through the BVH builder, the texture
readers, the numpy restatement's self-check against the oracle (tests/texture_ref.py) and its UV sanity, and the texture kernels' resources
(hipcc cross-compiles)."""
import ctypes as C
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

import texture_ref as T

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def W():
    import wavefront_path_tracer_amd as W
    return W


# ---------------------------------------------------------------- ABI
def test_texture_params_layout_and_constants(W):
    P = W._TextureParams
    assert C.sizeof(P) == 32 and P.offset.offset == 8 and P.filter.offset == 16 and P._reserved.offset == 20
    hdr = open(os.path.join(ROOT, "include", "wfpt.h")).read()
    assert "WFPT_FLAG_TEXTURES = 1u << 13" in hdr and W.FLAG_TEXTURES == 1 << 13
    assert re.search(r"#define WFPT_MAX_TEXTURES 64u", hdr) and W.MAX_TEXTURES == 64
    assert "sizeof(wfpt_texture_params) == 32" in hdr
    p = P()
    W.lib().wfpt_texture_params_default(C.byref(p))
    assert list(p.scale) == [1.0, 1.0] and list(p.offset) == [0.0, 0.0] and p.filter == 0 and list(p._reserved) == [0, 0, 0]


# ---------------------------------------------------------------- OBJ with texture coordinates
OBJ = """# a quad, a triangle with i/t/n, one with negative indices, one without texture indices
v 0 0 0
v 1 0 0
v 1 1 0
v 0 1 0
vt 0.0 0.0
vt 1.0 0.0
vt 1.0 1.0 0.0
vt 0.0 1.0
vn 0 0 1
f 1/1 2/2 3/3 4/4
f 1/1/1 3/3/1 4/4/1
f -4/-4 -3/-3 -2/-2
f 1 2 3
f 2//1 3//1 4//1
"""


def load_uv(W, path):
    n = C.c_uint32()
    assert W.lib().wfpt_load_obj_uv(os.fsencode(path), None, None, 0, C.byref(n), 0, 0) == 0
    tris, uv = np.zeros(n.value, W.TRIANGLE), np.zeros((n.value, 6), F)
    assert W.lib().wfpt_load_obj_uv(os.fsencode(path), W._p(tris), W._p(uv), n.value, C.byref(n), 2, 1) == 0
    return tris, uv


def test_load_obj_uv(W, tmp_path):
    p = tmp_path / "m.obj"
    p.write_text(OBJ)
    tris, uv = load_uv(W, p)
    assert len(tris) == 6  # the quad fans into two
    assert list(tris["_pad"]) == list(range(6))
    assert (tris["material_idx"] == 2).all() and (tris["material_type"] == 1).all()
    want = F([[0, 0, 1, 0, 1, 1],   # quad, fan 1-2-3
              [0, 0, 1, 1, 0, 1],   # quad, fan 1-3-4
              [0, 0, 1, 1, 0, 1],   # i/t/n
              [0, 0, 1, 0, 1, 1],   # negative: vertices 1 2 3, texcoords 1 2 3
              [0, 0, 0, 0, 0, 0],   # no /t
              [0, 0, 0, 0, 0, 0]])  # i//n
    assert np.array_equal(uv, want), uv
    # the geometry is wfpt_load_obj's, except for the row numbers
    ref = W.Scene.from_obj(str(p))
    assert np.array_equal(ref.triangles["v0"], tris["v0"]) and np.array_equal(ref.triangles["e2"], tris["e2"])
    assert (ref.triangles["_pad"] == 0).all()
    scene, uv2 = W.Scene.load_obj(str(p), uvs=True)
    assert np.array_equal(uv2, uv) and list(scene.triangles["_pad"]) == list(range(6))


def test_load_obj_uv_refusals(W, tmp_path):
    n = C.c_uint32()
    bad = tmp_path / "bad.obj"
    bad.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nf 1/2 2/1 3/1\n")  # texture index beyond the vt records
    assert W.lib().wfpt_load_obj_uv(os.fsencode(bad), None, None, 0, C.byref(n), 0, 0) == W.ERR_INVALID_ARGUMENT
    ok = tmp_path / "ok.obj"
    ok.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
    tris = np.zeros(1, W.TRIANGLE)
    assert W.lib().wfpt_load_obj_uv(os.fsencode(ok), W._p(tris), None, 1, C.byref(n), 0, 0) == W.ERR_INVALID_ARGUMENT  # rows needed


def test_rows_survive_the_bvh_builder(W):
    scene = W.Scene.random_mesh(3000, seed=4)
    tris = scene.triangles.copy()
    tris["_pad"] = np.arange(len(tris), dtype=np.uint32)[::-1]
    orig = tris.copy()
    bvh = W.BVHTree(len(tris))
    bvh.build_bvh_tree_triangles(tris, 32)
    assert not np.array_equal(tris["v0"], orig["v0"]), "the builder reordered nothing: the test shows nothing"
    back = orig[len(orig) - 1 - tris["_pad"].astype(np.int64)]  # the row names the triangle it was written for
    assert np.array_equal(back.view(np.uint8), tris.view(np.uint8))


# ---------------------------------------------------------------- readers
def srgb(c8):
    c = c8.astype(np.float64) / 255.0
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4).astype(F)


def test_png_round_trip_from_the_library(W, tmp_path):
    img = np.random.default_rng(1).integers(0, 256, (9, 13, 3), dtype=np.uint8)
    p = tmp_path / "t.png"
    W.write_png(str(p), img, 13, 9)
    got = W.load_texture(str(p))
    assert got.dtype == np.float32 and got.shape == (9, 13, 3) and np.array_equal(got, srgb(img))


def png_chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xffffffff)


def write_png_filtered(path, img, ctype):
    """A PNG whose scanlines cycle through the five filter types (the library's writer uses filter 0 only)."""
    h, w, ch = img.shape
    raw = bytearray()
    prev = np.zeros(w * ch, np.int32)
    for y in range(h):
        f = y % 5
        line = img[y].reshape(-1).astype(np.int32)
        left = np.concatenate([np.zeros(ch, np.int32), line[:-ch]])
        upleft = np.concatenate([np.zeros(ch, np.int32), prev[:-ch]])
        if f == 0:
            pred = np.zeros_like(line)
        elif f == 1:
            pred = left
        elif f == 2:
            pred = prev
        elif f == 3:
            pred = (left + prev) >> 1
        else:
            pa, pb, pc = np.abs(prev - upleft), np.abs(left - upleft), np.abs(left + prev - 2 * upleft)
            pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, prev, upleft))
        raw += bytes([f]) + ((line - pred) & 255).astype(np.uint8).tobytes()
        prev = line
    with open(path, "wb") as fh:
        fh.write(b"\x89PNG\r\n\x1a\n" + png_chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, ctype, 0, 0, 0)) +
                 png_chunk(b"IDAT", zlib.compress(bytes(raw))) + png_chunk(b"IEND", b""))


@pytest.mark.parametrize("ctype,ch", [(0, 1), (2, 3), (6, 4)])
def test_png_filters_and_colour_types(W, tmp_path, ctype, ch):
    img = np.random.default_rng(ctype).integers(0, 256, (11, 7, ch), dtype=np.uint8)
    p = tmp_path / "f.png"
    write_png_filtered(p, img, ctype)
    want = np.repeat(img, 3, axis=2) if ch == 1 else img[..., :3]
    assert np.array_equal(W.load_texture(str(p)), srgb(want))


def reference_unfilter(raw, w, ch):
    """The filters undone byte by byte, as PNG's specification writes them (9.2)."""
    h = raw.shape[0]
    out = np.zeros((h, w * ch), np.int32)
    prev = [0] * (w * ch)
    for y in range(h):
        f, line, cur = int(raw[y, 0]), [int(v) for v in raw[y, 1:]], [0] * (w * ch)
        for x in range(w * ch):
            a, b, c = (cur[x - ch] if x >= ch else 0), prev[x], (prev[x - ch] if x >= ch else 0)
            p = a + b - c
            paeth = a if abs(p - a) <= abs(p - b) and abs(p - a) <= abs(p - c) else (b if abs(p - b) <= abs(p - c) else c)
            cur[x] = (line[x] + (0, a, b, (a + b) >> 1, paeth)[f]) & 255
        out[y] = cur
        prev = cur
    return out.astype(np.uint8).reshape(h, w, ch)


@pytest.mark.parametrize("w,h,ch", [(211, 67, 3), (64, 150, 4), (1, 9, 3), (300, 1, 1)])
def test_png_unfilter_mixed_filters(W, w, h, ch):
    """Random filter bytes per row over random data: the whole-image reconstruction equals the byte-by-byte one."""
    rng = np.random.default_rng(w * h + ch)
    raw = np.concatenate([rng.integers(0, 5, (h, 1), dtype=np.uint8), rng.integers(0, 256, (h, w * ch), dtype=np.uint8)], axis=1)
    assert np.array_equal(W._png_unfilter(raw, w, ch), reference_unfilter(raw, w, ch))
    with pytest.raises(ValueError):
        bad = raw.copy()
        bad[0, 0] = 5
        W._png_unfilter(bad, w, ch)


def test_ppm_and_pfm(W, tmp_path):
    img = np.random.default_rng(2).integers(0, 256, (5, 6, 3), dtype=np.uint8)
    p = tmp_path / "t.ppm"
    p.write_bytes(b"P6\n# a comment\n6 5\n255\n" + img.tobytes())
    assert np.array_equal(W.load_texture(str(p)), srgb(img))
    lin = np.random.default_rng(3).random((4, 3, 3)).astype(F)
    q = tmp_path / "t.pfm"
    q.write_bytes(b"PF\n3 4\n-1.0\n" + np.ascontiguousarray(lin[::-1], "<f4").tobytes())
    assert np.array_equal(W.load_texture(str(q)), lin)
    with pytest.raises(ValueError):
        (tmp_path / "x.bin").write_bytes(b"nothing")
        W.load_texture(str(tmp_path / "x.bin"))


# ---------------------------------------------------------------- the restatement
def test_restatement_without_textures_is_the_oracle():
    """render_with_textures with nothing bound drives the oracle's stages into its own image, bit for bit: the driver itself is right."""
    from oracle import oracle as O
    want = O.shirley_oracle(40, 24, max_wavefronts=6).render(2)
    sp, mt = O.scene_book_one_final(1)
    sp, _ = O.build_bvh(sp)
    got = T.render_with_textures(O.shirley_oracle(40, 24, max_wavefronts=6), T.Textures(spheres=sp, materials=mt), spp=2)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_restatement_with_a_texture_changes_the_image():
    from oracle import oracle as O
    sp, mt = O.scene_book_one_final(1)
    sp, _ = O.build_bvh(sp)
    tx = T.Textures(spheres=sp, materials=mt, slots={0: (np.full((2, 2, 3), 0.5, F), {})}, bind={0: 0})
    a = T.render_with_textures(O.shirley_oracle(40, 24, max_wavefronts=6), tx, spp=1)
    b = O.shirley_oracle(40, 24, max_wavefronts=6).render(1)
    assert not np.array_equal(a, b) and (a <= b).all()


def test_triangle_corners_give_the_corner_uvs():
    rng = np.random.default_rng(6)
    v0, e1, e2 = (rng.standard_normal((50, 3)).astype(F) for _ in range(3))
    uv = rng.random((50, 6)).astype(F)
    for k, p in enumerate([v0, v0 + e1, v0 + e2]):
        u, v = T.triangle_uv(p, v0, e1, e2, uv)
        assert np.allclose(u, uv[:, 2 * k], atol=2e-4) and np.allclose(v, uv[:, 2 * k + 1], atol=2e-4)
    u, v = T.triangle_uv(v0, v0, v0 * 0, v0 * 0, uv)  # degenerate: b1 = b2 = 0
    assert np.array_equal(u, uv[:, 0]) and np.array_equal(v, uv[:, 1])


def test_sphere_poles_and_seam():
    c = np.zeros((1, 3), F)
    u, v = T.sphere_uv(F([[0, -2, 0]]), c)
    assert v[0] == 0  # -y pole
    u, v = T.sphere_uv(F([[0, 3, 0]]), c)
    assert abs(v[0] - 1) <= 1e-6  # +y pole
    u, v = T.sphere_uv(F([[1, 0, 0]]), c)
    assert u[0] == F(0.5) and abs(v[0] - 0.5) <= 1e-6  # +x, the equator
    u, v = T.sphere_uv(F([[0, 0, -1], [0, 0, 1], [-1, 0, 1e-7], [-1, 0, -1e-7]]), c)
    assert abs(u[0] - 0.75) <= 1e-6 and abs(u[1] - 0.25) <= 1e-6
    assert u[2] <= 1e-6 and u[3] >= 1 - 1e-6  # either side of the seam at -x


def test_lookup_wraps_and_filters():
    img = np.random.default_rng(7).random((4, 5, 3)).astype(F)
    u = F([0.1, 1.1, -0.9, 7.1])  # the same point, repeated
    v = F([0.3, 0.3, -1.7, 2.3])
    for flt in ("bilinear", "nearest"):
        got = T.tex_lookup(img, u, v, filter=flt)
        assert np.allclose(got, got[0], atol=1e-5)
    # texel centres: bilinear reads one texel; row 0 is the top (v near 1)
    x, y = 2, 0
    got = T.tex_lookup(img, F([(x + 0.5) / 5]), F([1 - (y + 0.5) / 4]))
    assert np.allclose(got[0], img[y, x], atol=1e-6)
    assert np.array_equal(T.tex_lookup(img, F([0.999]), F([0.001]), filter="nearest")[0], img[3, 4])
    # scale and offset
    assert np.allclose(T.tex_lookup(img, F([0.05]), F([0.3]), scale=(2, 1), offset=(0.0, 0)),
                       T.tex_lookup(img, F([0.1]), F([0.3])), atol=1e-6)


# ---------------------------------------------------------------- kernels
def test_texture_kernel_resources(tmp_path):
    """texture_kernel and the textured AOV kernels use no scratch; the texture pass stays within 64 vector registers."""
    from wavefront_path_tracer_amd import _build
    out = tmp_path / "wfpt_kernels.s"
    flags = [f for f in _build.FLAGS if f not in ("-shared", "-fPIC")]
    cmd = [_build.hipcc()] + flags + ["--offload-device-only", "-S", "-I" + os.path.join(ROOT, "include"), "-I" + _build.CSRC, "-o", str(out),
                                      os.path.join(_build.CSRC, "wfpt_kernels.hip")]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-3000:]
    asm = open(out).read()
    md = {m.group(1): {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\n", m.group(2))}
          for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size:", asm, re.S)}
    tex = next(m for n, m in md.items() if "texture_kernel" in n)
    assert tex["private_segment_fixed_size"] == 0 and tex["vgpr_count"] <= 64 and tex.get("agpr_count", 0) == 0, tex
    aov = {n: m for n, m in md.items() if "aov_tex_kernel" in n}
    assert len(aov) == 24, sorted(aov)
    assert all(m["private_segment_fixed_size"] == 0 for m in aov.values()), aov
