"""What the compiler makes of the middle fused launch of WFPT_FLAG_RETIRE contexts (bounce_kernel<kBounceMiddleRetire>), checked without a
GPU as tests/test_kernel_resources.py checks the unflagged launches: the termination step must not cost the launch its 8 waves per SIMD
(<= 64 vector, <= 80 scalar registers), it must not touch scratch, and its LDS walk must still be the hand-written loop."""
import re

from test_kernel_resources import body, device_asm, metadata  # noqa: F401  (device_asm: the fixture, compiled once for this module)

FRAG = "bounce_kernelILi3EjLi0ELb1ELb0E"  # MODE = 3, 32-bit trail, spheres, scene in LDS, default walk (both miss payloads)


def test_retire_launch_keeps_eight_waves_per_simd(device_asm):
    names = re.findall(r"\.name:\s+(\S*" + re.escape(FRAG) + r"\S*)\n", device_asm)
    assert len(names) == 2, names  # ENV = false, true
    for name in names:
        md = metadata(device_asm, name)
        assert md["vgpr_count"] <= 64, (name, md)
        assert md["sgpr_count"] <= 80, (name, md)
        assert md["private_segment_fixed_size"] == 0, (name, md)
        assert md.get("agpr_count", 0) == 0, (name, md)


def test_retire_launch_walks_with_the_hand_written_loop(device_asm):
    text = body(device_asm, FRAG)
    m = re.search(r"^\.Lwfpt_loop\d+:\n(.*?)^\.Lwfpt_end\d+:", text, re.S | re.M)
    assert m, "the LDS walk of this kernel does not contain descend_asm's loop"
    ops = re.findall(r"^\t([a-z_0-9]+)", m.group(1), re.M)
    valu = [o for o in ops if o.startswith("v_")]
    lds = [o for o in ops if o.startswith("ds_")]
    assert len(valu) <= 52 and len(lds) == 7 and sum(1 for o in valu if o == "v_fma_f32") == 18, (len(valu), len(lds))


def test_the_unflagged_fragments_still_name_the_unflagged_launches(device_asm):
    """MODE is the first template argument: the fragments tests/test_kernel_resources.py looks kernels up by never match MODE = 3."""
    for frag in ("bounce_kernelILi1EjLi0ELb1ELb0E", "refill_kernelILi1ELi1EE"):
        names = re.findall(r"\.name:\s+(\S*" + re.escape(frag) + r"\S*)\n", device_asm)
        assert names and all("ILi3E" not in n for n in names), names
    assert re.search(r"\.name:\s+\S*refill_kernelILi3ELi1EE", device_asm) and re.search(r"\.name:\s+\S*shade_retire_kernel", device_asm)
    assert re.search(r"\.name:\s+\S*shade_rays_retire_kernel", device_asm)
