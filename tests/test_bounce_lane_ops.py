"""Scalars parked in vector lanes by the fused bounce launches, checked without a GPU (hipcc cross-compiles, exactly as
tests/test_kernel_resources.py compiles): bounce_kernel is bound by vector-ALU issue, a scalar the register allocator cannot keep in the 80
scalar registers of eight waves per SIMD goes into a lane of a vector register, and every later use is a v_readlane_b32 -- a vector
instruction at half rate (profiles/r03_microbench_valu.txt). Up to round 9 every field of the argument block was loaded before the work-item
loop and held across shade, walk and compaction; since round 10 an item reads the block where it uses it
(bounce_args_here). This file counts v_readlane_b32 + v_writelane_b32 inside the work-item loop -- the largest region closed by a backward
branch -- of the bounce kernels of the LDS-resident sphere scene and holds each to a budget below what its parent commit (2dddeb3) had.

The counts include wave_offsets' four v_readlane_b32 (its prefix sums' read-out, not spills) in every kernel that traces."""
import re

import pytest

from test_kernel_resources import body, device_asm, metadata  # noqa: F401  (device_asm: the module-scoped fixture, compiled as there)

LANE_OPS = ("v_readlane_b32", "v_writelane_b32")

# mangled fragment: (what it is, lane ops in the work-item loop at the parent commit 2dddeb3, budget)
# The budgets are what the kernels have now plus a margin of 4 for the allocator's mood; each is strictly below its parent count.
KERNELS = {
    "bounce_kernelILi1EjLi0ELb1ELb0ELb0E": ("bounce_kernel<middle>", 110, 26),
    "bounce_kernelILi0EjLi0ELb1ELb0ELb0E": ("bounce_kernel<first>", 72, 24),
    "bounce_kernelILi3EjLi0ELb1ELb0ELb0E": ("bounce_kernel<middle, retire>", 107, 28),
    "bounce_kernelILi4EjLi0ELb1ELb0ELb0E": ("bounce_kernel<first, masked>", 75, 24),
    "bounce_kernelILi2EjLi0ELb0ELb0ELb0E": ("bounce_kernel<last>", 6, 2),
    "bounce_kernelILi1EjLi0ELb1ELb0ELb1E": ("bounce_kernel<middle>, environment", 63, 14),
    "bounce_kernelILi0EjLi0ELb1ELb0ELb1E": ("bounce_kernel<first>, environment", 49, 14),
    "bounce_kernelILi3EjLi0ELb1ELb0ELb1E": ("bounce_kernel<middle, retire>, environment", 75, 14),
    "bounce_kernelILi4EjLi0ELb1ELb0ELb1E": ("bounce_kernel<first, masked>, environment", 51, 14),
}
# (bounce_kernel<last>, environment -- bounce_kernelILi2EjLi0ELb0ELb0ELb1E -- had none at the parent commit and has none now: nothing to cut)


def item_loop(text):
    """The lines of the largest region of a kernel's text that a backward branch closes: label ... branch to that label."""
    lines = text.split("\n")
    labels = {m.group(1): i for i, l in enumerate(lines) if (m := re.match(r"^(\.LBB\d+_\d+):", l))}
    best = (0, 0)
    for i, l in enumerate(lines):
        m = re.match(r"^\t(?:s_cbranch_\w+|s_branch)\s+(\.LBB\d+_\d+)", l)
        if m and m.group(1) in labels and labels[m.group(1)] < i and i - labels[m.group(1)] > best[1] - best[0]:
            best = (labels[m.group(1)], i)
    return lines[best[0]:best[1] + 1]


def ops(lines):
    return [m.group(1) for l in lines if (m := re.match(r"^\t([a-z_0-9]+)", l))]


def test_budgets_are_below_the_parent_counts():
    for frag, (what, parent, budget) in KERNELS.items():
        assert budget < parent, what
    assert KERNELS["bounce_kernelILi1EjLi0ELb1ELb0ELb0E"][1] == 110 and KERNELS["bounce_kernelILi0EjLi0ELb1ELb0ELb0E"][1] == 72


@pytest.mark.parametrize("frag", sorted(KERNELS))
def test_item_loop_keeps_its_scalars_out_of_vector_lanes(device_asm, frag):
    what, parent, budget = KERNELS[frag]
    lines = item_loop(body(device_asm, frag))
    loop = ops(lines)
    assert len(loop) > 200, (what, "the work-item loop was not found")
    if "ILi2E" not in frag:  # the launches that trace: the region found is the one that holds the hand-written walk
        assert any(l.startswith(".Lwfpt_loop") for l in lines), what
    lane = sum(1 for o in loop if o in LANE_OPS)
    print(f"{what}: {lane} lane ops in the work-item loop (parent {parent}, budget {budget}), {sum(1 for o in loop if o.startswith('v_'))} vector, "
          f"{sum(1 for o in loop if o.startswith('s_load'))} s_load")
    assert lane <= budget, (what, lane, budget, parent)


@pytest.mark.parametrize("frag", sorted(KERNELS))
def test_arguments_are_read_through_the_scalar_path(device_asm, frag):
    """The item's reads of the argument block are s_load instructions inside the loop, and a pointer taken from the block is still known to
    be global memory: no flat_ access anywhere in the kernel."""
    what = KERNELS[frag][0]
    text = body(device_asm, frag)
    loop = ops(item_loop(text))
    assert sum(1 for o in loop if o.startswith("s_load")) >= 4, what
    assert not [o for o in ops(text.split("\n")) if o.startswith("flat_")], what
