"""Compile-time account of render_unit16_kernel (render_slab7_kernel's body with what a launch of 16 samples per pixel in workgroups of
256 threads fixes compiled in -- UNIT16, rtgo_render_body.inc): hipcc's resource remarks and the ISA, one device-only
compile of the product source with the build flags (no GPU), with the helpers of tests/test_pair_kernel_registers.py.  Everything is
held against render_slab7_kernel of the same compile.

What the kernel was admitted on: seven waves per SIMD (72 VGPRs) without scratch and without VGPR spills; no more SGPR spills than the
slab kernel; no lane moves at loop depth >= 3; the in-order sample sum as DPP row broadcasts folded into the additions (16 per channel:
48 v_add_f32_dpp with row_newbcast) and its three ds_bpermute_b32 gone (the seed fetch keeps its one); the generic unsigned divisions by
the samples per pass gone (one v_mul_hi_u32 each, three sites); and a shorter ray loop, vector and scalar.

Loop depths.  The slab kernel's nest is 1 the work queue, 2 the units of a strip, 3 the passes of a unit, 4 the ray loop, 5+ the walk.
UNIT16 has one pass, so its pass loop is gone and its ray loop is at depth 3 where hipcc drops the loop (it does).  The counts "at loop
depth >= 4" are therefore taken twice: literally, and ray loop against ray loop (the new kernel's depth >= 3 against the slab kernel's
depth >= 4), which is the comparison that says something and the stricter one -- the new kernel's count at depth >= 3 holds its count at
depth >= 4."""
import os
import re
import subprocess

import pytest

from test_pair_kernel_registers import body_of, instructions_by_loop_depth, one

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLAB7 = "_ZN4rtgo19render_slab7_kernelE"
UNIT16 = "_ZN4rtgo20render_unit16_kernelE"
LANE_MOVES = ("v_readlane_b32", "v_writelane_b32")
VECTOR = ("v_", "ds_", "global_", "buffer_", "flat_")


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """(resource remarks by kernel, the ISA's lines)"""
    import sys
    sys.path.insert(0, ROOT)
    from raytracingo_amd import _build
    out = str(tmp_path_factory.mktemp("isa") / "rtgo_device.s")
    flags = [f for f in _build.HIP_FLAGS if f != "-shared"]
    res = subprocess.run([_build.HIPCC] + flags + ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", "-o", out,
                          os.path.join(_build.PKG, "csrc", "rtgo_capi.hip")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    remarks, name = {}, None
    for line in res.stderr.splitlines():
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
    return remarks, asm


def lines_by_loop_depth(body):
    """(loop depth, mnemonic, the whole line) of every instruction: instructions_by_loop_depth with the operands kept"""
    depth = 0
    for line in body[1:]:
        m = re.match(r"^(\.LBB\w+:|; %bb\.\d+:)(.*)$", line)
        if m:
            d = re.search(r"Depth=(\d+)", m.group(2))
            depth = int(d.group(1)) if d else 0
        elif line.startswith("\t") and not line.strip().startswith((".", ";")):
            yield depth, line.split()[0], line.strip()


def counts(asm, symbol):
    body = body_of(asm, symbol)
    ins = list(lines_by_loop_depth(body))
    assert [(d, op) for d, op, _ in ins] == list(instructions_by_loop_depth(body))
    c = {"deepest loop": max(d for d, _, _ in ins), "instructions": len(ins)}
    for at in (3, 4):
        c["vector at depth >= %d" % at] = sum(1 for d, op, _ in ins if d >= at and op.startswith(VECTOR))
        c["scalar at depth >= %d" % at] = sum(1 for d, op, _ in ins if d >= at and op.startswith("s_"))
    c["vector"] = sum(1 for _, op, _ in ins if op.startswith(VECTOR))
    c["scalar"] = sum(1 for _, op, _ in ins if op.startswith("s_"))
    c["v_add_f32_dpp row_newbcast"] = sum(1 for _, op, l in ins if op == "v_add_f32_dpp" and "row_newbcast" in l)
    c["v_mov_b32_dpp"] = sum(1 for _, op, _ in ins if op == "v_mov_b32_dpp")
    c["ds_bpermute_b32"] = sum(1 for _, op, _ in ins if op == "ds_bpermute_b32")
    c["v_mul_hi_u32"] = sum(1 for _, op, _ in ins if op == "v_mul_hi_u32")
    c["ds_read / ds_write"] = sum(1 for _, op, _ in ins if op.startswith(("ds_read", "ds_write")))
    c["s_waitcnt"] = sum(1 for _, op, _ in ins if op == "s_waitcnt")
    c["lane moves at depth >= 3"] = sum(1 for d, op, _ in ins if d >= 3 and op in LANE_MOVES)
    return c


@pytest.fixture(scope="module")
def both(compiled):
    remarks, asm = compiled
    new, slab = one(remarks, UNIT16), one(remarks, SLAB7)
    c_new, c_slab = counts(asm, new), counts(asm, slab)
    print("%-32s %22s %22s" % ("", "render_unit16_kernel", "render_slab7_kernel"))
    for key in ("VGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill", "Occupancy [waves/SIMD]"):
        print("%-32s %22s %22s" % (key, remarks[new][key], remarks[slab][key]))
    for key in c_new:
        print("%-32s %22d %22d" % (key, c_new[key], c_slab[key]))
    return remarks[new], remarks[slab], c_new, c_slab


def test_resources(both):
    r, r_slab, _, _ = both
    assert int(r["VGPRs"]) <= 72, r
    assert int(r["ScratchSize [bytes/lane]"]) == 0, r
    assert int(r["VGPRs Spill"]) == 0, r
    assert int(r["Occupancy [waves/SIMD]"]) == 7, r
    assert int(r["SGPRs Spill"]) <= int(r_slab["SGPRs Spill"]), (r, r_slab)


def test_no_lane_moves_from_the_pass_loop_inwards(both):
    _, _, c, _ = both
    assert c["deepest loop"] >= 3, "no loop nest found"
    assert c["lane moves at depth >= 3"] == 0, c


def test_sample_sum_is_row_broadcast_additions(both):
    _, _, c, c_slab = both
    assert c["v_add_f32_dpp row_newbcast"] >= 48, c
    assert c["ds_bpermute_b32"] <= c_slab["ds_bpermute_b32"] - 3, (c, c_slab)
    assert c["ds_bpermute_b32"] >= 1, "the seed fetch is a lane exchange"


def test_no_generic_division_by_the_samples_per_pass(both):
    _, _, c, c_slab = both
    assert c["v_mul_hi_u32"] <= c_slab["v_mul_hi_u32"] - 3, (c, c_slab)


def test_ray_loop_is_shorter_than_the_slab_kernels(both):
    _, _, c, c_slab = both
    assert c_slab["deepest loop"] >= 4 and c_slab["vector at depth >= 4"] > 1000, c_slab
    # literally ...
    assert c["vector at depth >= 4"] < c_slab["vector at depth >= 4"], (c, c_slab)
    assert c["scalar at depth >= 4"] < c_slab["scalar at depth >= 4"], (c, c_slab)
    # ... and ray loop against ray loop: the new kernel's is one level up where its pass loop is gone
    shift = c_slab["deepest loop"] - c["deepest loop"]
    assert shift in (0, 1), (c, c_slab)
    at = "depth >= %d" % (4 - shift)
    assert c["vector at " + at] > 1000, "the ray loop is not where it is looked for"
    assert c["vector at " + at] < c_slab["vector at depth >= 4"], (c, c_slab)
    assert c["scalar at " + at] < c_slab["scalar at depth >= 4"], (c, c_slab)


def test_one_unit16_kernel_and_no_slab_or_pair_in_its_name(compiled):
    # (tests/test_slab7_kernel_registers.py and tests/test_pair7_kernel_registers.py count their kernels by those substrings)
    remarks, _ = compiled
    names = [n for n in remarks if "unit16" in n]
    assert names == [one(remarks, UNIT16)], names
    assert "render_slab" not in names[0] and "render_pair" not in names[0]


def test_header_documents_the_unit16_bit():
    with open(os.path.join(ROOT, "include", "rtgo.h")) as f:
        text = f.read()
    assert re.search(r"bit 11\b[^\n]*render_unit16_kernel", text), "rtgo.h: last_variant bit 11"
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    assert re.search(r"bit 11\b[^\n]*render_unit16_kernel", text) and "RTGO_NO_UNIT16" in text, "INTEGRATION.md: last_variant bit 11"
