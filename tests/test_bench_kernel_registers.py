"""Register budget of the bench kernel, the 6-waves-per-SIMD path kernel over flat scenes (render_kernel<true, false, 6, false, false,
true>): hipcc's resource remarks and the kernel's ISA, compiled from the product source with the build flags (device code only, no GPU).

The kernel fits 80 VGPRs at 6 waves per SIMD without scratch.  It reads the launch parameters through params_here (scalar loads where
they are used) instead of holding them from the kernel's start; held, they overflowed the 102 SGPRs of a wave into VGPR lanes, and every
save and restore was a VALU instruction (v_writelane_b32 / v_readlane_b32), inside the ray loop too.  DESIGN section 3.2 has the numbers."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "_ZN4rtgo13render_kernelILb1ELb0ELi6ELb0ELb0ELb1ELb0ELb0EE"
# the remaining spills: the workgroup index and the wave's index in it (one save at the start, one restore for the seed pass at the end),
# the queue's static-strip offset and the strip's row (one restore, resp. one save and one restore, per unit); none in the pass loop
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
    mine = [n for n in remarks if n.startswith(KERNEL)]
    assert len(mine) == 1, sorted(remarks)
    with open(out) as f:
        asm = f.read().split("\n")
    start = next(i for i, l in enumerate(asm) if l.startswith(mine[0] + ":"))
    end = next(i for i in range(start, len(asm)) if asm[i].startswith(".Lfunc_end"))
    return remarks[mine[0]], asm[start:end]


def instructions_by_loop_depth(body):
    """(loop depth, mnemonic) of every instruction, the depth from the assembler's block comments ("Loop Header: Depth=N",
    "in Loop: Header=... Depth=N"); a block without one is outside every loop"""
    depth = 0
    for line in body[1:]:
        m = re.match(r"^(\.LBB\w+:|; %bb\.\d+:)(.*)$", line)
        if m:
            d = re.search(r"Depth=(\d+)", m.group(2))
            depth = int(d.group(1)) if d else 0
        elif line.startswith("\t") and not line.strip().startswith((".", ";")):
            yield depth, line.split()[0]


def test_bench_kernel_resources(compiled):
    r, _ = compiled
    assert int(r["VGPRs"]) <= 80, r
    assert int(r["ScratchSize [bytes/lane]"]) == 0, r
    assert int(r["VGPRs Spill"]) == 0, r
    assert int(r["Occupancy [waves/SIMD]"]) == 6, r
    assert int(r["SGPRs Spill"]) <= SGPR_SPILL_CEILING, r


def test_bench_kernel_no_lane_moves_in_the_pass_loop(compiled):
    # loop depths of the lock-step kernel: 1 the work queue, 2 the units of a strip, 3 the passes of a unit, 4 the ray loop, 5+ the walk
    _, body = compiled
    ins = list(instructions_by_loop_depth(body))
    assert max(d for d, _ in ins) >= 5, "no loop nest found"
    lane_moves = [(d, op) for d, op in ins if op in ("v_readlane_b32", "v_writelane_b32")]
    assert len(lane_moves) <= 2 * SGPR_SPILL_CEILING, lane_moves
    assert [m for m in lane_moves if m[0] >= 3] == [], lane_moves
