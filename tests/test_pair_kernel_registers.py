"""Register budgets of the pair kernels, render_pair_kernel<6> and <5> (path mode over a flat scene whose fast-walk tree is a root over
two certified cuboid leaves: cornell): hipcc's resource remarks and the ISA, compiled from the product source with the
build flags (device code only, no GPU), as tests/test_bench_kernel_registers.py does for the kernel they stand in for.

The 6-waves one is the bench launch and keeps the bench kernel's budget: 80 VGPRs without scratch, no more SGPR spills, no lane moves in
the pass and ray loops.  The 5-waves one serves a band share of it and is held to render_kernel<true, false, 5, false, false, true> of
the same compile."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIR = "_ZN4rtgo18render_pair_kernelILi%dEE"
FLAT5 = "_ZN4rtgo13render_kernelILb1ELb0ELi5ELb0ELb0ELb1ELb0ELb0EE"
SGPR_SPILL_CEILING = 4


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    import sys
    sys.path.insert(0, ROOT)
    from raytracingo_amd import _build
    out = str(tmp_path_factory.mktemp("isa") / "rtgo_device.s")
    flags = [f for f in _build.HIP_FLAGS if f != "-shared"]
    res = subprocess.run([_build.HIPCC] + flags + ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", "-o", out,
                          os.path.join(_build.PKG, "csrc", "rtgo_capi.hip")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    remarks = {}
    name = None
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


def one(remarks, prefix):
    mine = [n for n in remarks if n.startswith(prefix)]
    assert len(mine) == 1, sorted(remarks)
    return mine[0]


def body_of(asm, symbol):
    start = next(i for i, l in enumerate(asm) if l.startswith(symbol + ":"))
    end = next(i for i in range(start, len(asm)) if asm[i].startswith(".Lfunc_end"))
    return asm[start:end]


def instructions_by_loop_depth(body):
    """(loop depth, mnemonic) of every instruction, the depth from the assembler's block comments"""
    depth = 0
    for line in body[1:]:
        m = re.match(r"^(\.LBB\w+:|; %bb\.\d+:)(.*)$", line)
        if m:
            d = re.search(r"Depth=(\d+)", m.group(2))
            depth = int(d.group(1)) if d else 0
        elif line.startswith("\t") and not line.strip().startswith((".", ";")):
            yield depth, line.split()[0]


def test_exactly_two_pair_kernels(compiled):
    remarks, _ = compiled
    assert sorted(n for n in remarks if "render_pair_kernel" in n) == sorted([one(remarks, PAIR % 5), one(remarks, PAIR % 6)])


def test_six_waves_pair_kernel_resources(compiled):
    remarks, _ = compiled
    r = remarks[one(remarks, PAIR % 6)]
    assert int(r["VGPRs"]) <= 80, r
    assert int(r["ScratchSize [bytes/lane]"]) == 0, r
    assert int(r["VGPRs Spill"]) == 0, r
    assert int(r["Occupancy [waves/SIMD]"]) == 6, r
    assert int(r["SGPRs Spill"]) <= SGPR_SPILL_CEILING, r


def test_six_waves_pair_kernel_no_lane_moves_in_the_pass_loop(compiled):
    # loop depths of the lock-step kernel: 1 the work queue, 2 the units of a strip, 3 the passes of a unit, 4 the ray loop, 5+ the walk
    remarks, asm = compiled
    ins = list(instructions_by_loop_depth(body_of(asm, one(remarks, PAIR % 6))))
    assert max(d for d, _ in ins) >= 4, "no loop nest found"
    lane_moves = [(d, op) for d, op in ins if op in ("v_readlane_b32", "v_writelane_b32")]
    assert [m for m in lane_moves if m[0] >= 3] == [], lane_moves


def test_five_waves_pair_kernel_resources(compiled):
    remarks, _ = compiled
    r, base = remarks[one(remarks, PAIR % 5)], remarks[one(remarks, FLAT5)]
    assert int(r["Occupancy [waves/SIMD]"]) == 5, r
    assert int(r["ScratchSize [bytes/lane]"]) <= int(base["ScratchSize [bytes/lane]"]), (r, base)
    assert int(r["VGPRs Spill"]) <= int(base["VGPRs Spill"]), (r, base)


def test_header_documents_the_variant_bit():
    with open(os.path.join(ROOT, "include", "rtgo.h")) as f:
        text = f.read()
    assert re.search(r"bit 8\b[^\n]*two-leaf tree", text), "rtgo.h: last_variant bit 8"
