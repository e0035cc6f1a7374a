"""What the compiler makes of the kernels of WFPT_FLAG_SHADING_NORMALS contexts (shading_normal_kernel, connect_shading_kernel,
aov_shading_kernel), checked without a GPU as tests/test_analytic_lights_kernel_resources.py checks its kernels: every instantiation
exists, none touches scratch, none uses an AGPR. The connect and AOV twins carry no register bound, as the kernels they are twins of:
their counts beside those are DESIGN.md 9r's table, printed here."""
import re

from test_kernel_resources import device_asm, metadata  # noqa: F401  (device_asm: the fixture, compiled once for this module)

CONNECT = re.compile(r"connect_shading_kernelI(\w)Li(\d)ELb(\d)ELb(\d)ELb(\d)ELb(\d)ELb(\d)E")  # Trail, PRIM, LDS_SCENE, EXACT, TEX, ENVS, MIS
AOV = re.compile(r"aov_shading_kernelI(\w)Li(\d)ELb(\d)ELb(\d)ELb(\d)ELb(\d)E")  # Trail, PRIM, LDS_SCENE, EXACT, ENV, TEX


def names_of(asm, kernel):
    return sorted(set(re.findall(r"\.name:\s+(\S*" + kernel + r"\S*)\n", asm)))


def test_the_pass_and_its_probe_spill_nothing(device_asm):
    for kernel in ("shading_normal_kernel", "shading_sample_kernel"):
        names = names_of(device_asm, kernel)
        assert len(names) == 1, names
        md = metadata(device_asm, names[0])
        print(kernel, ": vgpr", md["vgpr_count"], "sgpr", md["sgpr_count"])
        assert md["private_segment_fixed_size"] == 0 and md.get("agpr_count", 0) == 0, md
    md = metadata(device_asm, "shading_normal_kernel")
    assert md["vgpr_count"] <= 64, "the pass is a gather and a store: it should run at full occupancy"


def test_every_shading_connect_kernel_is_there_and_spills_nothing(device_asm):
    names = names_of(device_asm, "connect_shading_kernel")
    twins = set(names_of(device_asm, "connect_kernel"))
    assert len(names) == 48, len(names)  # triangles only: 6 walks x TEX x ENVS x MIS
    assert len({CONNECT.search(n).groups() for n in names}) == 48
    print("trail lds exact tex envs mis: vgpr sgpr (twin vgpr sgpr)")
    for name in names:
        trail, prim, lds, exact, tex, envs, mis = CONNECT.search(name).groups()
        assert prim == "1", name
        twin = [t for t in twins if f"connect_kernelI{trail}Li1ELb{lds}ELb{exact}ELb{tex}ELb{envs}ELb{mis}E" in t]
        assert len(twin) == 1, (name, twin)
        md, tw = metadata(device_asm, name), metadata(device_asm, twin[0])
        print(trail, lds, exact, tex, envs, mis, ":", md["vgpr_count"], md["sgpr_count"], "(", tw["vgpr_count"], tw["sgpr_count"], ")")
        assert md["private_segment_fixed_size"] == 0, (name, md)
        assert md.get("agpr_count", 0) == 0, (name, md)
    assert all(n.endswith("EEvNS_11ConnectArgsEPK15HIP_vector_typeIfLj4EE") for n in names), "ConnectArgs stays as it is: the rows are a second argument"


def test_every_shading_aov_kernel_is_there_and_spills_nothing(device_asm):
    names = names_of(device_asm, "aov_shading_kernel")
    assert len(names) == 24, len(names)  # triangles only: 6 walks x ENV x TEX
    assert len({AOV.search(n).groups() for n in names}) == 24
    print("trail lds exact env tex: vgpr sgpr (aov_tex_kernel / aov_kernel / aov_env_kernel vgpr sgpr)")
    for name in names:
        trail, prim, lds, exact, env, tex = AOV.search(name).groups()
        assert prim == "1", name
        if tex == "1":
            twin = f"aov_tex_kernelI{trail}Li1ELb{lds}ELb{exact}ELb{env}E"
        else:
            twin = f"aov_{'env_' if env == '1' else ''}kernelI{trail}Li1ELb{lds}ELb{exact}E"
        md, tw = metadata(device_asm, name), metadata(device_asm, twin)
        print(trail, lds, exact, env, tex, ":", md["vgpr_count"], md["sgpr_count"], "(", tw["vgpr_count"], tw["sgpr_count"], ")")
        assert md["private_segment_fixed_size"] == 0, (name, md)
        assert md.get("agpr_count", 0) == 0, (name, md)
