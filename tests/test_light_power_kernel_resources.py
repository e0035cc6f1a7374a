"""What the compiler makes of the kernels of WFPT_FLAG_LIGHT_POWER contexts (connect_power_kernel, emission_weighed_power_kernel,
mis_weight_power_kernel and the three kernels that build the distribution), checked without a GPU as tests/test_retire_kernel_resources.py
checks its launch: none of them may touch scratch. The connect kernels carry no register bound (no min-waves launch bound, as their
unflagged twins): their counts beside the twins' are DESIGN.md 9p's table, printed here."""
import re

from test_kernel_resources import device_asm, metadata  # noqa: F401  (device_asm: the fixture, compiled once for this module)

POWER = re.compile(r"connect_power_kernelI(\w)Li(\d)ELb(\d)ELb(\d)ELb(\d)ELb(\d)E")  # Trail, PRIM, LDS_SCENE, EXACT, TEX, MIS


def test_every_power_connect_kernel_is_there_and_spills_nothing(device_asm):
    names = sorted(set(re.findall(r"\.name:\s+(\S*connect_power_kernel\S*)\n", device_asm)))
    twins = set(re.findall(r"\.name:\s+(\S*connect_kernel\S*)\n", device_asm))
    assert len(names) == 48 and len(twins) == 96, (len(names), len(twins))  # 12 walks x TEX x MIS; the twins also x ENVS
    print("trail prim lds exact tex mis: vgpr sgpr (twin vgpr sgpr)")
    for name in names:
        trail, prim, lds, exact, tex, mis = POWER.search(name).groups()
        twin = [t for t in twins if f"connect_kernelI{trail}Li{prim}ELb{lds}ELb{exact}ELb{tex}ELb0ELb{mis}E" in t]
        assert len(twin) == 1, (name, twin)
        md, tw = metadata(device_asm, name), metadata(device_asm, twin[0])
        print(trail, prim, lds, exact, tex, mis, ":", md["vgpr_count"], md["sgpr_count"], "(", tw["vgpr_count"], tw["sgpr_count"], ")")
        assert md["private_segment_fixed_size"] == 0, (name, md)
        assert md.get("agpr_count", 0) == 0, (name, md)
        assert tw["private_segment_fixed_size"] == 0, (twin[0], tw)


def test_the_other_new_kernels_spill_nothing(device_asm):
    for frag in ("emission_weighed_power_kernel", "mis_weight_power_kernel", "light_weight_kernel", "light_quantise_kernel", "light_scan_kernel"):
        md = metadata(device_asm, frag)
        assert md["private_segment_fixed_size"] == 0 and md.get("agpr_count", 0) == 0, (frag, md)
    # the weighed emission kernel next to its unflagged twin (emission_kernel<kEmitWeighed>): one table load and a division more
    md, tw = metadata(device_asm, "emission_weighed_power_kernel"), metadata(device_asm, "emission_kernelILi2EE")
    print("emission_weighed_power_kernel", md["vgpr_count"], md["sgpr_count"], "emission_kernel<kEmitWeighed>", tw["vgpr_count"], tw["sgpr_count"])
    assert md["vgpr_count"] <= 64, md  # a consumer kernel of 256 threads: 8 waves per SIMD, as its twin
