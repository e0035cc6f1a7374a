"""What one draw from the fused launches' work counter buys (csrc/wfpt_ticket_chunks.h), checked without a
GPU: tests/cpp/chunk_schedule_host.cpp runs the rule as bounce_kernel applies it -- behind the first launch's static range and over a
middle launch's tickets; grids of 1, 7 and 1024 workgroups; ranges around 0, 1, the chunk length, the tail and tail + one chunk per
workgroup, the 259 200 items of the frame bench.py times and the 65 535 x 64 of the largest launch; chunk lengths 1 .. 16; 0, 1 and 4 tail
rounds; static shares 0 and 1/2; three orders in which the workgroups finish -- as a stand-alone program under AddressSanitizer + UBSan:
every item is taken exactly once, a workgroup's items ascend, an item follows without a draw exactly inside a chunk, the draws that find
something number chunks + singles, chunk length 1 is the rule as it was, draw for draw, and the 32-bit products are exact."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wavefront_path_tracer_amd", "csrc")


def test_chunk_rule_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "san_chunk_schedule")
    san = ["-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    cmd = ["g++", "-std=c++17", "-Wall", *san, "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "chunk_schedule_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-4000:]


def test_the_shipped_constants_are_covered_by_the_host_program():
    """The macros' defaults in wfpt_kernels.h: chunk lengths and tail rounds the host program runs."""
    text = open(os.path.join(CSRC, "wfpt_kernels.h")).read()
    for name in ("WFPT_FIRST_CHUNK", "WFPT_BOUNCE_CHUNK"):
        assert int(re.search(r"#define " + name + r" (\d+)", text).group(1)) in (1, 2, 4, 8, 16), name
    for name in ("WFPT_FIRST_TAIL_ROUNDS", "WFPT_BOUNCE_TAIL_ROUNDS"):
        assert int(re.search(r"#define " + name + r" (\d+)", text).group(1)) in (0, 1, 4), name
