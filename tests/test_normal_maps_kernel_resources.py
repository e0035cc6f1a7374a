"""What the compiler makes of the kernels of mapped WFPT_FLAG_NORMAL_MAPS contexts (shading_nmap_kernel, microfacet_nmap_kernel,
rough_glass_nmap_kernel, nmap_sample_kernel, connect_nmap_kernel, aov_nmap_kernel), checked without a GPU as
tests/test_shading_normals_kernel_resources.py checks its kernels: every instantiation exists, none touches scratch, none uses an AGPR.
The register counts are printed beside those of the kernels they stand in for (DESIGN.md 9v's table) and carry no bound of their own."""
import re

from test_kernel_resources import device_asm, metadata  # noqa: F401  (device_asm: the fixture, compiled once for this module)
from test_shading_normals_kernel_resources import names_of

CONNECT = re.compile(r"connect_nmap_kernelI(\w)Li(\d)ELb(\d)ELb(\d)ELb(\d)ELb(\d)ELb(\d)E")  # Trail, PRIM, LDS_SCENE, EXACT, TEX, ENVS, MIS
AOV = re.compile(r"aov_nmap_kernelI(\w)Li(\d)ELb(\d)ELb(\d)ELb(\d)ELb(\d)E")  # Trail, PRIM, LDS_SCENE, EXACT, ENV, TEX
TWINS = {"shading_nmap_kernel": "shading_normal_kernel", "microfacet_nmap_kernel": "microfacet_kernelILb1EE",
         "rough_glass_nmap_kernel": "rough_glass_kernelILb1EE", "nmap_sample_kernel": "shading_sample_kernel"}


def spills_nothing(asm, name):
    md = metadata(asm, name)
    assert md["private_segment_fixed_size"] == 0, (name, md)
    assert md.get("agpr_count", 0) == 0, (name, md)
    return md


def test_the_record_passes_and_the_probe_spill_nothing(device_asm):
    for kernel, twin in TWINS.items():
        names = names_of(device_asm, kernel)
        assert len(names) == 1, (kernel, names)
        md, tw = spills_nothing(device_asm, names[0]), metadata(device_asm, twin)
        print(kernel, ": vgpr", md["vgpr_count"], "sgpr", md["sgpr_count"], "(", twin, tw["vgpr_count"], tw["sgpr_count"], ")")


def test_every_nmap_connect_kernel_is_there_and_spills_nothing(device_asm):
    names = names_of(device_asm, "connect_nmap_kernel")
    twins = set(names_of(device_asm, "connect_shading_kernel"))
    assert len(names) == 48, len(names)  # triangles only: 6 walks x TEX x ENVS x MIS
    assert len({CONNECT.search(n).groups() for n in names}) == 48
    print("trail lds exact tex envs mis: vgpr sgpr (connect_shading_kernel vgpr sgpr)")
    for name in names:
        trail, prim, lds, exact, tex, envs, mis = CONNECT.search(name).groups()
        assert prim == "1", name
        twin = [t for t in twins if f"connect_shading_kernelI{trail}Li1ELb{lds}ELb{exact}ELb{tex}ELb{envs}ELb{mis}E" in t]
        assert len(twin) == 1, (name, twin)
        md, tw = spills_nothing(device_asm, name), metadata(device_asm, twin[0])
        print(trail, lds, exact, tex, envs, mis, ":", md["vgpr_count"], md["sgpr_count"], "(", tw["vgpr_count"], tw["sgpr_count"], ")")
    assert all("ConnectArgsENS_9NmapSceneE" in n for n in names), "ConnectArgs stays as it is: the tables are a second argument"


def test_every_nmap_aov_kernel_is_there_and_spills_nothing(device_asm):
    names = names_of(device_asm, "aov_nmap_kernel")
    assert len(names) == 24, len(names)  # triangles only: 6 walks x ENV x TEX
    assert len({AOV.search(n).groups() for n in names}) == 24
    print("trail lds exact env tex: vgpr sgpr (aov_shading_kernel vgpr sgpr)")
    for name in names:
        trail, prim, lds, exact, env, tex = AOV.search(name).groups()
        assert prim == "1", name
        md = spills_nothing(device_asm, name)
        tw = metadata(device_asm, f"aov_shading_kernelI{trail}Li1ELb{lds}ELb{exact}ELb{env}ELb{tex}E")
        print(trail, lds, exact, env, tex, ":", md["vgpr_count"], md["sgpr_count"], "(", tw["vgpr_count"], tw["sgpr_count"], ")")


def test_the_existing_families_keep_their_counts(device_asm):
    """no new kernel's name contains an existing kernel's: the counts the other resource tests assert by substring are what they were"""
    for kernel, n in (("shading_normal_kernel", 1), ("connect_shading_kernel", 48), ("aov_shading_kernel", 24), ("microfacet_kernel", 2),
                      ("rough_glass_kernel", 2), ("shading_sample_kernel", 1), ("microfacet_sample_kernel", 1), ("rough_glass_sample_kernel", 1)):
        assert len(names_of(device_asm, kernel)) == n, (kernel, names_of(device_asm, kernel))
