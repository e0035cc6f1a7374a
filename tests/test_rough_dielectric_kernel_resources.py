"""What the compiler makes of the kernels of WFPT_FLAG_ROUGH_DIELECTRIC contexts (rough_glass_kernel<NORMALS>, rough_glass_sample_kernel),
checked without a GPU as tests/test_microfacet_kernel_resources.py checks its kernels: both instantiations of the pass and the probe
exist, none touches scratch, none uses an AGPR. Their register counts are printed, not fixed: DESIGN.md 9u quotes them."""
import re

from test_kernel_resources import device_asm, metadata  # noqa: F401  (device_asm: the fixture, compiled once for this module)
from test_microfacet_kernel_resources import names_of

PASS = re.compile(r"rough_glass_kernelILb(\d)EE")  # NORMALS


def test_both_passes_are_there_and_spill_nothing(device_asm):
    names = names_of(device_asm, "rough_glass_kernel")
    assert len(names) == 2, names
    assert sorted(PASS.search(n).group(1) for n in names) == ["0", "1"], names
    for name in names:
        md = metadata(device_asm, name)
        print("rough_glass_kernel<NORMALS =", PASS.search(name).group(1), ">: vgpr", md["vgpr_count"], "sgpr", md["sgpr_count"])
        assert md["private_segment_fixed_size"] == 0, (name, md)
        assert md.get("agpr_count", 0) == 0, (name, md)
    assert all(n.endswith("EvNS_14MicrofacetArgsE") for n in names), "the microfacet pass's argument block"


def test_the_probe_is_there_and_spills_nothing(device_asm):
    names = names_of(device_asm, "rough_glass_sample_kernel")
    assert len(names) == 1, names
    md = metadata(device_asm, names[0])
    print("rough_glass_sample_kernel: vgpr", md["vgpr_count"], "sgpr", md["sgpr_count"])
    assert md["private_segment_fixed_size"] == 0 and md.get("agpr_count", 0) == 0, md
