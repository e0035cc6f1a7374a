"""What the compiler makes of the kernels of roughness-mapped WFPT_FLAG_ROUGHNESS_MAPS contexts (microfacet_rmap_kernel,
rough_glass_rmap_kernel, rmap_sample_kernel), checked without a GPU as tests/test_normal_maps_kernel_resources.py checks its kernels:
each exists exactly once, none touches scratch, none uses an AGPR. The register counts are printed beside those of the kernels they stand
in for (DESIGN.md 9w's table) and carry no bound of their own."""
from test_kernel_resources import device_asm, metadata  # noqa: F401  (device_asm: the fixture, compiled once for this module)
from test_normal_maps_kernel_resources import spills_nothing
from test_shading_normals_kernel_resources import names_of

TWINS = {"microfacet_rmap_kernel": ("microfacet_kernelILb0EE", "microfacet_kernelILb1EE", "microfacet_nmap_kernel"),
         "rough_glass_rmap_kernel": ("rough_glass_kernelILb0EE", "rough_glass_kernelILb1EE", "rough_glass_nmap_kernel"),
         "rmap_sample_kernel": ("nmap_sample_kernel",)}


def test_the_record_passes_and_the_probe_spill_nothing(device_asm):
    for kernel, twins in TWINS.items():
        names = names_of(device_asm, kernel)
        assert len(names) == 1, (kernel, names)
        md = spills_nothing(device_asm, names[0])
        beside = ", ".join(f"{t} {metadata(device_asm, t)['vgpr_count']} {metadata(device_asm, t)['sgpr_count']}" for t in twins)
        print(kernel, ": vgpr", md["vgpr_count"], "sgpr", md["sgpr_count"], "(", beside, ")")
    assert all("MicrofacetArgsENS_9RmapSceneE" in names_of(device_asm, k)[0] for k in ("microfacet_rmap_kernel", "rough_glass_rmap_kernel")), \
        "MicrofacetArgs stays as it is: the tables are a second argument"


def test_the_existing_families_keep_their_counts(device_asm):
    """no new kernel's name contains an existing kernel's: the counts the other resource tests assert by substring are what they were"""
    for kernel, n in (("shading_normal_kernel", 1), ("microfacet_kernel", 2), ("rough_glass_kernel", 2), ("shading_nmap_kernel", 1),
                      ("microfacet_nmap_kernel", 1), ("rough_glass_nmap_kernel", 1), ("nmap_sample_kernel", 1), ("connect_nmap_kernel", 48),
                      ("aov_nmap_kernel", 24), ("connect_shading_kernel", 48), ("aov_shading_kernel", 24), ("shading_sample_kernel", 1),
                      ("microfacet_sample_kernel", 1), ("rough_glass_sample_kernel", 1)):
        assert len(names_of(device_asm, kernel)) == n, (kernel, names_of(device_asm, kernel))
