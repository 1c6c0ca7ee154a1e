"""Register budget of the 7-waves pair kernel, render_pair7_kernel (render_pair_kernel<6>'s body under WPE = 7):
hipcc's resource remarks and the ISA, compiled from the product source with the build flags (device code only, no GPU), with the compile
and the helpers of tests/test_pair_kernel_registers.py.

Seven waves per SIMD leave a wave 512 / 7 -> 72 VGPRs (granule 8).  The kernel must fit them without scratch and without VGPR spills, and
its ray loop must be the 6-waves kernel's: what the tighter budget costs is SGPR spills into VGPR lanes, and those must stay where they
are today -- no more of them, and none inside the pass loop or the ray loop (loop depth >= 3), the rule render_pair_kernel<6> is held to.

SGPR_SPILLS is the count of today's compile: 12 values held across the work queue and the strip loop, 27 lane moves at loop depths 0 to 2.
They are kept and pinned, count and depth; re-deriving those values where they are used (params_here, opaque_lane, s_cam) is left open
(profiles/r09a/README.md)."""
import os
import re

import pytest

from test_pair_kernel_registers import PAIR, body_of, compiled, instructions_by_loop_depth, one  # noqa: F401  (compiled: the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIR7 = "_ZN4rtgo19render_pair7_kernelE"
SGPR_SPILLS = 12
LANE_MOVES = ("v_readlane_b32", "v_writelane_b32")
# the two ray loops are the same source under the same switches; the allocator may place a copy or two differently under 72 registers
RAY_LOOP_SLACK = 8


def vector_in_ray_loop(ins):
    return sum(1 for d, op in ins if d >= 4 and op.startswith(("v_", "ds_", "global_", "buffer_", "flat_")))


def test_seven_waves_pair_kernel_resources(compiled):
    remarks, _ = compiled
    r = remarks[one(remarks, PAIR7)]
    print(r)
    assert int(r["VGPRs"]) <= 72, r
    assert int(r["ScratchSize [bytes/lane]"]) == 0, r
    assert int(r["VGPRs Spill"]) == 0, r
    assert int(r["Occupancy [waves/SIMD]"]) == 7, r
    assert int(r["SGPRs Spill"]) <= SGPR_SPILLS, r


def test_seven_waves_pair_kernel_lane_moves_stay_outside_the_pass_loop(compiled):
    # loop depths of the lock-step kernel: 1 the work queue, 2 the units of a strip, 3 the passes of a unit, 4 the ray loop, 5+ the walk
    remarks, asm = compiled
    ins = list(instructions_by_loop_depth(body_of(asm, one(remarks, PAIR7))))
    assert max(d for d, _ in ins) >= 4, "no loop nest found"
    lane_moves = [(d, op) for d, op in ins if op in LANE_MOVES]
    print("lane moves by loop depth:", sorted(lane_moves))
    assert [m for m in lane_moves if m[0] >= 3] == [], lane_moves


def test_seven_waves_ray_loop_is_the_six_waves_one(compiled):
    remarks, asm = compiled
    seven = vector_in_ray_loop(list(instructions_by_loop_depth(body_of(asm, one(remarks, PAIR7)))))
    six = vector_in_ray_loop(list(instructions_by_loop_depth(body_of(asm, one(remarks, PAIR % 6)))))
    print("vector instructions at loop depth >= 4: 7 waves %d, 6 waves %d" % (seven, six))
    assert six > 1000, six
    assert abs(seven - six) <= RAY_LOOP_SLACK, (seven, six)


def test_pair_template_keeps_its_two_instantiations(compiled):
    remarks, _ = compiled
    assert sorted(n for n in remarks if "render_pair_kernel" in n) == sorted([one(remarks, PAIR % 5), one(remarks, PAIR % 6)])
    assert len([n for n in remarks if "render_pair7_kernel" in n]) == 1, sorted(remarks)


def test_header_documents_the_seven_waves_bit():
    with open(os.path.join(ROOT, "include", "rtgo.h")) as f:
        text = f.read()
    assert re.search(r"bit 9\b[^\n]*seven waves per SIMD", text), "rtgo.h: last_variant bit 9"
