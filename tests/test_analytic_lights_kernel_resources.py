"""What the compiler makes of the connect kernels of WFPT_FLAG_ANALYTIC_LIGHTS contexts (connect_analytic_kernel), checked without a GPU
as tests/test_light_power_kernel_resources.py checks its kernels: every instantiation exists, none touches scratch, none uses an AGPR.
They carry no register bound (no min-waves launch bound, as their unflagged twins): their counts beside the twins' are DESIGN.md 9q's
table, printed here."""
import re

from test_kernel_resources import device_asm, metadata  # noqa: F401  (device_asm: the fixture, compiled once for this module)

ANALYTIC = re.compile(r"connect_analytic_kernelI(\w)Li(\d)ELb(\d)ELb(\d)ELb(\d)ELb(\d)E")  # Trail, PRIM, LDS_SCENE, EXACT, TEX, MIS


def test_every_analytic_connect_kernel_is_there_and_spills_nothing(device_asm):
    names = sorted(set(re.findall(r"\.name:\s+(\S*connect_analytic_kernel\S*)\n", device_asm)))
    twins = set(re.findall(r"\.name:\s+(\S*connect_kernel\S*)\n", device_asm))
    assert len(names) == 48, len(names)  # 12 walks x TEX x MIS
    assert len({ANALYTIC.search(n).groups() for n in names}) == 48
    print("trail prim lds exact tex mis: vgpr sgpr (twin vgpr sgpr)")
    for name in names:
        trail, prim, lds, exact, tex, mis = ANALYTIC.search(name).groups()
        twin = [t for t in twins if f"connect_kernelI{trail}Li{prim}ELb{lds}ELb{exact}ELb{tex}ELb0ELb{mis}E" in t]
        assert len(twin) == 1, (name, twin)
        md, tw = metadata(device_asm, name), metadata(device_asm, twin[0])
        print(trail, prim, lds, exact, tex, mis, ":", md["vgpr_count"], md["sgpr_count"], "(", tw["vgpr_count"], tw["sgpr_count"], ")")
        assert md["private_segment_fixed_size"] == 0, (name, md)
        assert md.get("agpr_count", 0) == 0, (name, md)


def test_the_table_takes_the_second_argument(device_asm):
    """ConnectArgs stays as it is: the new kernels take it unchanged and the light table behind it, as connect_power_kernel takes its
    distribution."""
    names = set(re.findall(r"\.name:\s+(\S*connect_analytic_kernel\S*)\n", device_asm))
    assert names and all(n.endswith("EEvNS_11ConnectArgsENS_10LightTableE") for n in names), sorted(names)[:2]
