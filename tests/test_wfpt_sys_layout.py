"""The #[repr(C)] structs of wfpt-sys/src/lib.rs have the byte layout include/wfpt.h asserts for their C twins.

tests/test_abi.py checks that the crate is what tools/gen_wfpt_sys.py makes of the header; this checks what the generator made: every
field's offset and every struct's size, computed from the Rust declarations (all fields are 4-byte scalars, arrays of them or structs of
them), against the header's WFPT_LAYOUT_ASSERT sizeof / offsetof values -- a field the generator dropped shows up as a wrong size."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALAR_BYTES = {"f32": 4, "u32": 4, "i32": 4}


def rust_layouts():
    src = open(os.path.join(ROOT, "wfpt-sys", "src", "lib.rs")).read()
    structs = {name: re.findall(r"pub (\w+): ([^,]+),", body) for name, body in re.findall(r"pub struct (wfpt_\w+) \{(.*?)\n\}", src, re.S)}
    layouts = {}

    def size_of(t):
        m = re.fullmatch(r"\[(\w+); (\d+)\]", t.strip())
        if m:
            return size_of(m.group(1)) * int(m.group(2))
        t = t.strip()
        if t in SCALAR_BYTES:
            return SCALAR_BYTES[t]
        return layout(t)[0]

    def layout(name):
        if name not in layouts:
            off, offsets = 0, {}
            for field, t in structs[name]:
                offsets[field] = off
                off += size_of(t)
            layouts[name] = (off, offsets)
        return layouts[name]

    return {n: layout(n) for n in structs if structs[n] and not structs[n][0][0].startswith("_private")}


def header_asserts():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wfpt.h")).read(), flags=re.S)
    out = {}
    for body in re.findall(r"WFPT_LAYOUT_ASSERT\((.*?),\s*\"", text, re.S):
        m = re.search(r"sizeof\((wfpt_\w+)\) == (\d+)", body)
        if m:
            out[m.group(1)] = (int(m.group(2)), {f: int(v) for f, v in re.findall(r"offsetof\(" + m.group(1) + r", (\w+)\) == (\d+)", body)})
    return out


def test_every_asserted_struct_has_its_c_layout_in_rust():
    rust, want = rust_layouts(), header_asserts()
    assert "wfpt_texture_params" in want and "wfpt_environment_params" in want
    for name, (size, offsets) in want.items():
        assert name in rust, f"{name} is missing from wfpt-sys"
        got_size, got_offsets = rust[name]
        assert got_size == size, f"{name}: {got_size} bytes in Rust, {size} in C"
        for field, off in offsets.items():
            assert got_offsets.get(field) == off, f"{name}.{field}: offset {got_offsets.get(field)} in Rust, {off} in C"


def test_texture_params_and_filters_in_rust():
    rust = rust_layouts()
    size, offsets = rust["wfpt_texture_params"]
    assert size == 32 and offsets["scale"] == 0 and offsets["offset"] == 8 and offsets["filter"] == 16 and offsets["_reserved"] == 20
    src = open(os.path.join(ROOT, "wfpt-sys", "src", "lib.rs")).read()
    assert "pub const WFPT_TEXTURE_BILINEAR: c_int = 0;" in src and "pub const WFPT_TEXTURE_NEAREST: c_int = 1;" in src
