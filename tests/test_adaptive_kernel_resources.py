"""What the compiler makes of the first fused launch of WFPT_FLAG_ADAPTIVE contexts (bounce_kernel<kBounceFirstMasked>), checked without a
GPU as tests/test_kernel_resources.py checks the unflagged first launch: the mask word must not cost the launch its 8 waves per SIMD
(<= 64 vector, <= 80 scalar registers, the unflagged first launch's scratch allowance), and its LDS walk must still be the hand-written
loop. The fragments the two existing resource tests look kernels up by must keep naming the unflagged kernels."""
import re

from test_kernel_resources import KERNELS, body, device_asm, metadata  # noqa: F401  (device_asm: the fixture, compiled once for this module)

FRAG = "bounce_kernelILi4EjLi0ELb1ELb0E"  # MODE = 4, 32-bit trail, spheres, scene in LDS, default walk (both miss payloads)
UNFLAGGED_FIRST = "bounce_kernelILi0EjLi0ELb1ELb0E"


def names_of(asm, frag):
    return re.findall(r"\.name:\s+(\S*" + re.escape(frag) + r"\S*)\n", asm)


def test_masked_first_launch_keeps_eight_waves_per_simd(device_asm):
    _, scratch = KERNELS[UNFLAGGED_FIRST]
    names = names_of(device_asm, FRAG)
    assert len(names) == 2, names  # ENV = false, true
    for name in names:
        md = metadata(device_asm, name)
        assert md["vgpr_count"] <= 64, (name, md)
        assert md["sgpr_count"] <= 80, (name, md)
        assert md["private_segment_fixed_size"] <= scratch, (name, md)
        assert md.get("agpr_count", 0) == 0, (name, md)


def test_masked_first_launch_walks_with_the_hand_written_loop(device_asm):
    text = body(device_asm, FRAG)
    m = re.search(r"^\.Lwfpt_loop\d+:\n(.*?)^\.Lwfpt_end\d+:", text, re.S | re.M)
    assert m, "the LDS walk of this kernel does not contain descend_asm's loop"
    ops = re.findall(r"^\t([a-z_0-9]+)", m.group(1), re.M)
    valu = [o for o in ops if o.startswith("v_")]
    lds = [o for o in ops if o.startswith("ds_")]
    assert len(valu) <= 52 and len(lds) == 7 and sum(1 for o in valu if o == "v_fma_f32") == 18, (len(valu), len(lds))


def test_the_mask_word_arrives_through_the_scalar_path(device_asm):
    """The tile's word is wave-uniform: more 64-bit scalar loads than the unflagged first launch (the table's address, the word), and no
    64-bit vector load more."""
    def loads(frag, op):
        return len(re.findall(r"^\t" + op + r"\b", body(device_asm, frag), re.M))
    assert loads(FRAG, "s_load_dwordx2") > loads(UNFLAGGED_FIRST, "s_load_dwordx2")
    assert loads(FRAG, "global_load_dwordx2") == loads(UNFLAGGED_FIRST, "global_load_dwordx2")


def test_the_unflagged_fragments_still_name_the_unflagged_launches(device_asm):
    """MODE is the first template argument: the fragments tests/test_kernel_resources.py and tests/test_retire_kernel_resources.py look
    kernels up by never match MODE = 4, and the other generate and accumulate kernels keep their names beside the masked ones."""
    for frag in list(KERNELS) + ["bounce_kernelILi3EjLi0ELb1ELb0E"]:
        names = names_of(device_asm, frag)
        assert names and all("bounce_kernelILi4E" not in n for n in names), names
    for kernel in ("generate_rays_kernel", "generate_dense_kernel", "accumulate_kernel", "accumulate_moments_kernel", "accumulate_emission_kernel",
                   "accumulate_emission_moments_kernel"):
        assert len(names_of(device_asm, kernel + "E")) == 1, kernel
    for kernel in ("generate_rays_masked_kernel", "generate_dense_masked_kernel", "accumulate_masked_kernel", "accumulate_emission_masked_kernel",
                   "adaptive_update_kernel", "mean_resolve_kernel"):
        assert len(names_of(device_asm, kernel)) == 1, kernel
    assert len(names_of(device_asm, "bounce_kernelILi4E")) == 24  # trail x primitive x residency x walk x miss payload, as MODE 0
    assert len(names_of(device_asm, "bounce_kernelILi4E")) == len(names_of(device_asm, "bounce_kernelILi0E"))
