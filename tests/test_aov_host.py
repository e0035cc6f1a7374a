"""First-hit AOVs (WFPT_FLAG_AOV) without a GPU: the ABI declares and exports them, every aov_kernel variant compiles to gfx950 without
scratch, and on a box without a device the Python calls fail loudly."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("wfpt_aov_channels", "wfpt_read_aov", "wfpt_copy_aov_to_device", "wfpt_aov_timing_ms")


def test_header_and_library_carry_the_aov_abi(wf):
    declared = wf.abi_symbols()
    L = wf.lib()
    for name in NEW:
        assert name in declared and hasattr(L, name), name
    hdr = open(os.path.join(ROOT, "include", "wfpt.h")).read()
    assert re.search(r"WFPT_FLAG_AOV = 1u << 10\b", hdr)
    assert not re.search(r"= 1u << 9\b", hdr)  # bit 9 stays retired (WFPT_FLAG_TWO_CHAINS)
    assert "WFPT_STAGE_COUNT = 13" in hdr  # callers size their stage arrays by it
    for k, v in (("ALBEDO", 0), ("NORMAL", 1), ("DEPTH", 2), ("COVERAGE", 3), ("PRIM_ID", 4), ("MATERIAL_ID", 5)):
        assert f"WFPT_AOV_{k} = {v}," in hdr
        assert getattr(wf, f"AOV_{k}") == v
    assert wf.FLAG_AOV == 1 << 10
    assert [L.wfpt_aov_channels(i) for i in range(-1, 7)] == [0, 3, 3, 1, 1, 1, 1, 0]
    assert {k: v[1] for k, v in wf.AOVS.items()} == {"albedo": 3, "normal": 3, "depth": 1, "coverage": 1, "prim_id": 1, "material_id": 1}


def test_aov_calls_without_a_context_are_refused(wf):
    L = wf.lib()
    buf = np.zeros(4, "<f4")
    assert L.wfpt_read_aov(None, 0, wf._p(buf), 1) == -1
    assert L.wfpt_copy_aov_to_device(None, 0, wf._p(buf), 4) == -1
    assert L.wfpt_aov_timing_ms(None, None, None) == -1


@pytest.fixture(scope="module")
def device_asm(tmp_path_factory):
    """wfpt_kernels.hip compiled for gfx950 to assembly, the way tests/test_kernel_resources.py does it."""
    from wavefront_path_tracer_amd import _build
    out = tmp_path_factory.mktemp("isa_aov") / "wfpt_kernels.s"
    flags = [f for f in _build.FLAGS if f not in ("-shared", "-fPIC")]
    cmd = [_build.hipcc()] + flags + ["--offload-device-only", "-S", "-I" + os.path.join(ROOT, "include"), "-I" + _build.CSRC, "-o", str(out),
                                      os.path.join(_build.CSRC, "wfpt_kernels.hip")]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-3000:]
    return open(out).read()


def test_every_aov_kernel_variant_runs_without_scratch(device_asm):
    """Spheres / triangles x LDS-resident (32- and 64-bit trail) / HBM x exact or not: 12 instantiations, and the resolve kernel."""
    found = {}
    for m in re.finditer(r"\.name:\s+(\S*aov_(?:resolve_)?kernel\S*)\n(.*?)\.wavefront_size:", device_asm, re.S):
        found[m.group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\n", m.group(2))}
    variants = [n for n in found if "aov_kernel" in n]
    assert len(variants) == 12 and any("aov_resolve_kernel" in n for n in found), sorted(found)
    for name, md in found.items():
        assert md["private_segment_fixed_size"] == 0, (name, md)
        assert md.get("agpr_count", 0) == 0, (name, md)
        assert md["vgpr_count"] <= 128, (name, md)  # at least 4 waves per SIMD: two 512-thread workgroups per CU


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="only meaningful on a box without a GPU")
def test_no_gpu_means_aov_contexts_fail_loudly(wf):
    assert wf.device_count() == 0
    with pytest.raises(wf.WfptError):
        wf.shirley_path_tracer(64, 64, flags=wf.FLAG_AOV)
