"""The wave votes of the pair kernels' ray loop (render_pair7_kernel, render_pair_kernel<6>): hipcc's ISA, compiled
from the product source with the build flags (device code only, no GPU), with the compile and the helpers of
tests/test_pair_kernel_registers.py.

hipcc lowers __ballot of a combination of compares by turning the lane mask into a 0/1 vector register and comparing it back --
`v_cndmask_b32 v, 0, 1, <mask>` and `v_cmp_ne_u32 vcc, 0, v` ahead of every vote -- and keeps bools that live across a loop as 0/1
integers.  The pair kernels' ray loop carries its predicates as lane masks instead (Pred<true>, rtgo_device.h), which needs neither; two
counts at loop depth >= 4 (the ray loop and the walk inside it) say so.

PARENT: the counts of commit e99ffe2, the last one before this change, from the same compile of that commit.  A count must stay below its
parent's, and within SLACK of what this change left.  What is left: the near leaf of fast_pair, which keeps the bool (as masks its
predicates cost render_pair7_kernel more SGPR spills than tests/test_pair7_kernel_registers.py allows), the quadrics' branches of
leaf_test, and the lock-step loop's own `active`.  The generic kernels keep the bool everywhere: one of them is held to its parent's counts
exactly."""
import re

import pytest

from test_pair_kernel_registers import PAIR, body_of, compiled, one  # noqa: F401  (compiled: the fixture)

PAIR7 = "_ZN4rtgo19render_pair7_kernelE"
GENERIC = "_ZN4rtgo13render_kernelILb1ELb0ELi6ELb0ELb0ELb1ELb0ELb0EE"   # path, fast walk, 6 waves, lock-step, frames: the kernel the pair kernels stand in for
SLACK = 2
#          v_cndmask_b32 v, 0, 1, <mask>;  v_cmp_ne_u32 vcc, 0, v      (at loop depth >= 4)
PARENT = {"pair7": (27, 25), "pair6": (27, 25), "generic": (21, 23)}   # commit e99ffe2
CHANGE = {"pair7": (11, 8), "pair6": (11, 8)}
SYMBOL = {"pair7": PAIR7, "pair6": PAIR % 6, "generic": GENERIC}


def lines_by_loop_depth(body):
    """(loop depth, instruction text without its comment) of every instruction, the depth from the assembler's block comments"""
    depth = 0
    for line in body[1:]:
        m = re.match(r"^(\.LBB\w+:|; %bb\.\d+:)(.*)$", line)
        if m:
            d = re.search(r"Depth=(\d+)", m.group(2))
            depth = int(d.group(1)) if d else 0
        elif line.startswith("\t") and not line.strip().startswith((".", ";")):
            yield depth, line.split(";")[0].strip()


def counts(compiled, which):
    remarks, asm = compiled
    ins = [text for d, text in lines_by_loop_depth(body_of(asm, one(remarks, SYMBOL[which]))) if d >= 4]
    assert len(ins) > 1000, len(ins)   # (the loop was found)
    to_vector = sum(1 for text in ins if re.match(r"v_cndmask_b32\w*\s+v\d+, 0, 1, ", text))
    and_back = sum(1 for text in ins if re.match(r"v_cmp_ne_u32\w*\s+vcc, 0, v\d+", text))
    return to_vector, and_back


@pytest.mark.parametrize("which", ["pair7", "pair6"])
def test_ray_loop_votes_on_lane_masks(compiled, which):
    to_vector, and_back = counts(compiled, which)
    print("%s at loop depth >= 4: v_cndmask_b32 v, 0, 1, mask: %d (parent %d), v_cmp_ne_u32 vcc, 0, v: %d (parent %d)" %
          (which, to_vector, PARENT[which][0], and_back, PARENT[which][1]))
    assert to_vector < PARENT[which][0], (to_vector, PARENT[which])
    assert and_back < PARENT[which][1], (and_back, PARENT[which])
    assert to_vector <= CHANGE[which][0] + SLACK, (to_vector, CHANGE[which])
    assert and_back <= CHANGE[which][1] + SLACK, (and_back, CHANGE[which])


def test_generic_kernel_keeps_its_votes(compiled):
    assert counts(compiled, "generic") == PARENT["generic"]
