"""How the first fused launch hands out its work items (csrc/wfpt_first_schedule.h), checked without a GPU:
tests/cpp/first_schedule_host.cpp runs the header's rule as the kernel applies it -- item counts around the multiples of the grid and the
259 200 items of the frame bench.py times, grids of 1, 7 and 1024 workgroups, every share of the sweep -- as a stand-alone program under
AddressSanitizer + UBSan: the static items of all workgroups and the dynamic range cover the items exactly once, a workgroup's items
ascend, share 0 leaves nothing static."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_first_schedule_rule_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "san_first_schedule")
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    cmd = ["g++", "-std=c++17", "-Wall", *san, "-I", os.path.join(ROOT, "wavefront_path_tracer_amd", "csrc"),
           os.path.join(ROOT, "tests", "cpp", "first_schedule_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-4000:]


def test_the_shipped_share_is_one_of_the_sweep():
    """The macro's default in wfpt_kernels.h is a share the host program covers."""
    import re
    text = open(os.path.join(ROOT, "wavefront_path_tracer_amd", "csrc", "wfpt_kernels.h")).read()
    num = int(re.search(r"#define WFPT_FIRST_STATIC_SHARE_NUM (\d+)", text).group(1))
    den = int(re.search(r"#define WFPT_FIRST_STATIC_SHARE_DEN (\d+)", text).group(1))
    assert (num, den) in [(0, 1), (1, 2), (3, 4), (7, 8), (15, 16), (1, 1), (1, 16), (1, 8), (1, 4), (3, 8), (5, 8)] or num == 0
