"""The scalar work of the pair kernels' ray loop (render_pair7_kernel, render_pair_kernel<6>): hipcc's ISA, compiled
from the product source with the build flags (device code only, no GPU), with the compile and the helpers of
tests/test_pair_kernel_registers.py.

The ray loop reads per ray only what a ray can change.  What the launch decides -- the kind of the list's cuboid, whether a depth is a
path's last, where the list's records lie -- is a template parameter, one launch field or a compile-time offset, and two counts say so:
the scalar loads at loop depth 4 (the ray loop's own blocks: the launch fields and the list's records; the walk's loads are deeper) and
the scalar instructions at depth >= 4 other than loads, waits and no-ops.

PARENT: the counts of commit c25739d, the last one before this change, from the same compile of that commit.  A count must stay below
its parent's, and within SLACK of what this change left (the allowance tests/test_pair7_kernel_registers.py gives the allocator)."""
import pytest

from test_pair_kernel_registers import PAIR, body_of, compiled, instructions_by_loop_depth, one  # noqa: F401  (compiled: the fixture)

PAIR7 = "_ZN4rtgo19render_pair7_kernelE"
SLACK = 8
#                  s_load* at depth 4, scalar instructions at depth >= 4
PARENT = {"pair7": (12, 1304), "pair6": (12, 1304)}   # commit c25739d
CHANGE = {"pair7": (11, 869), "pair6": (11, 869)}
NOT_COUNTED = ("s_waitcnt", "s_nop", "s_load")


def counts(ins):
    loads = sum(1 for d, op in ins if d == 4 and op.startswith("s_load"))
    scalar = sum(1 for d, op in ins if d >= 4 and op.startswith("s_") and not op.startswith(NOT_COUNTED))
    return loads, scalar


@pytest.mark.parametrize("which", ["pair7", "pair6"])
def test_ray_loop_scalar_loads_and_scalar_instructions(compiled, which):
    remarks, asm = compiled
    ins = list(instructions_by_loop_depth(body_of(asm, one(remarks, PAIR7 if which == "pair7" else PAIR % 6))))
    assert max(d for d, _ in ins) >= 4, "no loop nest found"
    loads, scalar = counts(ins)
    print("%s: s_load* at loop depth 4: %d (parent %d), scalar instructions at depth >= 4: %d (parent %d)" %
          (which, loads, PARENT[which][0], scalar, PARENT[which][1]))
    assert scalar > 400, scalar   # (the loop was found)
    assert loads < PARENT[which][0], (loads, PARENT[which])
    assert scalar < PARENT[which][1], (scalar, PARENT[which])
    assert loads <= CHANGE[which][0] + SLACK, (loads, CHANGE[which])
    assert scalar <= CHANGE[which][1] + SLACK, (scalar, CHANGE[which])
