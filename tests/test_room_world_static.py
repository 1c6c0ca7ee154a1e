"""Compile-time account of render_roomw_kernel (render_unit16_kernel's body with the room's slab test steered in world axes -- ROOMW,
room_world in rtgo_device.h): hipcc's resource remarks and the ISA, one device-only compile of the product source with
the build flags (no GPU), with the helpers of tests/test_unit16_kernel_static.py.  Everything is held against render_unit16_kernel of the
same compile.

What the kernel was admitted on: seven waves per SIMD (at most 72 VGPRs) without scratch, VGPR spills or SGPR spills -- id and noid now
live across the room's face test and the light's test, and that must not cost the seventh wave; no lane moves at the ray loop's depth;
and a shorter ray loop: at least 30 vector instructions fewer (the source says 36 and 3 reciprocals; six are left to the compiler's
scheduling moves), at least 3 v_rcp_f32 fewer, fewer scalar-memory instructions.

Both kernels are UNIT16: no pass loop, the ray loop is at loop depth 3 (tests/test_unit16_kernel_static.py)."""
import os
import re

import pytest

from test_pair_kernel_registers import body_of, one
from test_unit16_kernel_static import LANE_MOVES, ROOT, UNIT16, VECTOR, compiled, lines_by_loop_depth   # noqa: F401 (compiled: the fixture)

ROOMW = "_ZN4rtgo19render_roomw_kernelE"
RAY_LOOP = 3
PROFILE = os.path.join(ROOT, "profiles", "r28a")


def counts(asm, symbol):
    ins = list(lines_by_loop_depth(body_of(asm, symbol)))
    loop = [(op, l) for d, op, l in ins if d >= RAY_LOOP]
    return {"deepest loop": max(d for d, _, _ in ins), "instructions": len(ins),
            "vector in the ray loop": sum(1 for op, _ in loop if op.startswith(VECTOR)),
            "scalar in the ray loop": sum(1 for op, _ in loop if op.startswith("s_")),
            "scalar memory in the ray loop": sum(1 for op, _ in loop if op.startswith(("s_load_", "s_buffer_load_"))),
            "v_rcp_f32 in the ray loop": sum(1 for op, _ in loop if op.startswith("v_rcp_f32")),
            "lane moves in the ray loop": sum(1 for op, _ in loop if op in LANE_MOVES)}


@pytest.fixture(scope="module")
def both(compiled):
    remarks, asm = compiled
    new, old = one(remarks, ROOMW), one(remarks, UNIT16)
    c_new, c_old = counts(asm, new), counts(asm, old)
    print("%-32s %22s %22s" % ("", "render_roomw_kernel", "render_unit16_kernel"))
    for key in ("VGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill", "Occupancy [waves/SIMD]"):
        print("%-32s %22s %22s" % (key, remarks[new][key], remarks[old][key]))
    for key in c_new:
        print("%-32s %22d %22d" % (key, c_new[key], c_old[key]))
    return remarks[new], remarks[old], c_new, c_old


def test_resources(both):
    r, _, _, _ = both
    assert int(r["VGPRs"]) <= 72, r
    assert int(r["ScratchSize [bytes/lane]"]) == 0, r
    assert int(r["VGPRs Spill"]) == 0, r
    assert int(r["SGPRs Spill"]) == 0, r
    assert int(r["Occupancy [waves/SIMD]"]) == 7, r


def test_no_lane_moves_in_the_ray_loop(both):
    _, _, c, c_old = both
    assert c["deepest loop"] >= RAY_LOOP and c["vector in the ray loop"] > 1000, "the ray loop is not where it is looked for"
    assert c_old["deepest loop"] == c["deepest loop"], (c, c_old)
    assert c["lane moves in the ray loop"] == 0, c


def test_the_ray_loop_lost_the_frame_transform(both):
    _, _, c, c_old = both
    assert c["vector in the ray loop"] <= c_old["vector in the ray loop"] - 30, (c, c_old)
    assert c["v_rcp_f32 in the ray loop"] <= c_old["v_rcp_f32 in the ray loop"] - 3, (c, c_old)
    assert c["scalar memory in the ray loop"] < c_old["scalar memory in the ray loop"], (c, c_old)


def test_one_new_kernel_and_its_name(compiled):
    # (tests/test_unit16_kernel_static.py, test_slab7_kernel_registers.py and test_pair7_kernel_registers.py count their kernels by name)
    remarks, _ = compiled
    names = [n for n in remarks if "roomw" in n]
    assert names == [one(remarks, ROOMW)], names
    assert not any(s in names[0] for s in ("unit16", "slab", "pair"))


def test_recorded_asm_diff_says_every_other_function_is_the_parents():
    """tools/kernel_asm_diff.py, the parent's device assembly against this change's, as recorded with the profile: every function of the
    parent identical -- render_unit16_kernel and the build kernels included -- and one function new"""
    with open(os.path.join(PROFILE, "asm_diff.txt")) as f:
        text = f.read()
    m = re.search(r"functions: (\d+) and (\d+); in one only: (\d+); identical: (\d+); different: (\d+)", text)
    assert m, text[:400]
    a, b, only, same, diff = map(int, m.groups())
    assert (b, only, same, diff) == (a + 1, 1, a, 0), text[:400]
    assert re.search(r"only in one: _ZN4rtgo19render_roomw_kernelE", text), text[:400]


def test_header_documents_bit_12_and_the_knob():
    with open(os.path.join(ROOT, "include", "rtgo.h")) as f:
        text = f.read()
    assert re.search(r"bit 12\b[^\n]*render_roomw_kernel", text) and "RTGO_NO_ROOMW" in text, "rtgo.h: last_variant bit 12"
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    assert re.search(r"bit 12\b[^\n]*render_roomw_kernel", text) and "RTGO_NO_ROOMW" in text, "INTEGRATION.md: last_variant bit 12"
