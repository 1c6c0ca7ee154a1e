"""Budgets of the two kernels of rtgo_whitted_set_instances_device (rtgo_whitted_inst_update.h): hipcc's resource remarks, compiled from
the product source with the build flags (device code only, no GPU), as tests/test_whitted_build_batch_kernel_registers.py reads them.

inst_prepare_kernel carries a 3x4 matrix and its inverse in double and inst_gather_kernel four float4: neither has a reason to touch
scratch, to spill or to need a dynamic stack.  inst_prepare_kernel's static LDS is its 256 records at 15 dwords and the mesh table,
256 x 12 dwords."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = "_ZN4rtgo7whitted"
PREPARE, GATHER = W + "19inst_prepare_kernelE", W + "18inst_gather_kernelE"


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    import sys
    sys.path.insert(0, ROOT)
    from raytracingo_amd import _build
    out = str(tmp_path_factory.mktemp("isa") / "rtgo_device.s")
    flags = [f for f in _build.HIP_FLAGS if f != "-shared"]
    res = subprocess.run([_build.HIPCC] + flags + ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", "-o", out,
                          os.path.join(_build.PKG, "csrc", "rtgo_capi.hip")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    found = {}
    name = None
    for line in res.stderr.splitlines():
        m = re.search(r"remark: +(.+?): (\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        key, value = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            name = value
            found[name] = {}
        elif name is not None:
            found[name][key] = value
    return found


def one(remarks, prefix):
    mine = [n for n in remarks if n.startswith(prefix)]
    assert len(mine) == 1, (prefix, sorted(remarks))
    return remarks[mine[0]]


@pytest.mark.parametrize("kernel", [PREPARE, GATHER])
def test_no_scratch_no_spills_no_dynamic_stack(remarks, kernel):
    r = one(remarks, kernel)
    print(kernel, sorted(r.items()))
    assert int(r["ScratchSize [bytes/lane]"]) == 0, r
    assert int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, r
    assert r["Dynamic Stack"] == "False", r


def test_the_prepare_kernel_stages_records_at_an_odd_stride_and_the_mesh_table(remarks):
    assert int(one(remarks, PREPARE)["LDS Size [bytes/block]"]) == 4 * (256 * 15 + 256 * 12)
    assert int(one(remarks, GATHER)["LDS Size [bytes/block]"]) == 0
