"""Compile-time budget of render_slab7_kernel (render_pair7_kernel's body with cuboid_slab in cuboid_range's place, for the room and for both
leaves): hipcc's resource remarks, its inlining remarks and the ISA, compiled from the product source with the build
flags (device code only, no GPU), with the helpers of tests/test_pair_kernel_registers.py.

What the kernel was admitted on: it fits seven waves per SIMD (72 VGPRs) without scratch and without VGPR spills; no SGPR is spilled
into VGPR lanes inside the pass loop or the ray loop (loop depth >= 3); its SGPR spills stay at the count of its first good compile (3:
values held across the work queue and the strip loop); its ray loop (loop depth >= 4) holds at least 150 vector instructions fewer than
render_pair7_kernel's in the same compile -- 150 is what the issue-slot budget of DESIGN 3.3 needs for a gain above the A/B gate; and
the one form of the cuboid test in it is the slab's: no instantiation of cuboid_range is inlined into it, by hipcc's own account."""
import os
import re
import subprocess

import pytest

from test_pair_kernel_registers import body_of, instructions_by_loop_depth, one

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIR7 = "_ZN4rtgo19render_pair7_kernelE"
SLAB7 = "_ZN4rtgo19render_slab7_kernelE"
SGPR_SPILLS = 3
LANE_MOVES = ("v_readlane_b32", "v_writelane_b32")
RAY_LOOP_SAVING = 150


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """(resource remarks by kernel, the ISA's lines, the inlining remarks as (callee, caller) pairs)"""
    import sys
    sys.path.insert(0, ROOT)
    from raytracingo_amd import _build
    out = str(tmp_path_factory.mktemp("isa") / "rtgo_device.s")
    flags = [f for f in _build.HIP_FLAGS if f != "-shared"]
    res = subprocess.run([_build.HIPCC] + flags + ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", "-Rpass=inline", "-o", out,
                          os.path.join(_build.PKG, "csrc", "rtgo_capi.hip")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    remarks, inlined, name = {}, set(), None
    for line in res.stderr.splitlines():
        m = re.search(r"remark: '(\S+)' inlined into '(\S+)'", line)
        if m:
            inlined.add((m.group(1), m.group(2)))
            continue
        m = re.search(r"remark: +(.+?): (\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        key, value = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            name = value
            remarks[name] = {}
        elif name is not None:
            remarks[name][key] = value
    with open(out) as f:
        asm = f.read().split("\n")
    return remarks, asm, inlined


def vector_in_ray_loop(ins):
    return sum(1 for d, op in ins if d >= 4 and op.startswith(("v_", "ds_", "global_", "buffer_", "flat_")))


def reached_from(inlined, fragment):
    """every function into which a function whose name holds `fragment` ends up inlined, directly or through its callers"""
    seen = set()
    todo = [callee for callee, _ in inlined if fragment in callee]
    while todo:
        f = todo.pop()
        for callee, caller in inlined:
            if callee == f and caller not in seen:
                seen.add(caller)
                todo.append(caller)
    return seen


def test_slab_kernel_resources(compiled):
    remarks, _, _ = compiled
    r = remarks[one(remarks, SLAB7)]
    print(r)
    assert int(r["VGPRs"]) <= 72, r
    assert int(r["ScratchSize [bytes/lane]"]) == 0, r
    assert int(r["VGPRs Spill"]) == 0, r
    assert int(r["Occupancy [waves/SIMD]"]) == 7, r
    assert int(r["SGPRs Spill"]) <= SGPR_SPILLS, r


def test_slab_kernel_lane_moves_stay_outside_the_pass_loop(compiled):
    # loop depths of the lock-step kernel: 1 the work queue, 2 the units of a strip, 3 the passes of a unit, 4 the ray loop, 5+ the walk
    remarks, asm, _ = compiled
    ins = list(instructions_by_loop_depth(body_of(asm, one(remarks, SLAB7))))
    assert max(d for d, _ in ins) >= 4, "no loop nest found"
    lane_moves = [(d, op) for d, op in ins if op in LANE_MOVES]
    print("lane moves by loop depth:", sorted(lane_moves))
    assert [m for m in lane_moves if m[0] >= 3] == [], lane_moves


def test_slab_ray_loop_is_shorter_than_the_pair_kernels(compiled):
    remarks, asm, _ = compiled
    slab = vector_in_ray_loop(list(instructions_by_loop_depth(body_of(asm, one(remarks, SLAB7)))))
    pair = vector_in_ray_loop(list(instructions_by_loop_depth(body_of(asm, one(remarks, PAIR7)))))
    print("vector instructions at loop depth >= 4: slab %d, pair %d" % (slab, pair))
    assert pair > 1000, pair
    assert slab <= pair - RAY_LOOP_SAVING, (slab, pair)


def test_no_cuboid_range_in_the_slab_kernel(compiled):
    remarks, _, inlined = compiled
    slab, pair = one(remarks, SLAB7), one(remarks, PAIR7)
    range_in = reached_from(inlined, "cuboid_range")
    assert pair in range_in, "the inlining remarks do not show cuboid_range in render_pair7_kernel: the check below would prove nothing"
    assert slab not in range_in
    assert slab in reached_from(inlined, "cuboid_slab")
    assert pair not in reached_from(inlined, "cuboid_slab")


def test_one_slab_kernel_and_no_pair_in_its_name(compiled):
    # (tests/test_pair7_kernel_registers.py counts the pair kernels by the substring "render_pair")
    remarks, _, _ = compiled
    names = [n for n in remarks if "render_slab" in n]
    assert names == [one(remarks, SLAB7)], names
    assert "render_pair" not in names[0]


def test_header_documents_the_slab_bit():
    with open(os.path.join(ROOT, "include", "rtgo.h")) as f:
        text = f.read()
    assert re.search(r"bit 10\b[^\n]*slab", text), "rtgo.h: last_variant bit 10"
