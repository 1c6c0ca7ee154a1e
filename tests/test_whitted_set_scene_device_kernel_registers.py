"""Budgets of the three kernels of rtgo_whitted_set_scene_device (rtgo_whitted_mesh_device.h): hipcc's resource remarks, compiled from
the product source with the build flags (device code only, no GPU), as tests/test_whitted_instances_device_kernel_registers.py reads
them.

mesh_check_kernel and mesh_check_final_kernel stream dwords and carry a box, a word of fault bits and a material index; mesh_pack_kernel
copies dwords: none has a reason to touch scratch, to spill or to need a dynamic stack.  The two check kernels' static LDS is
reduce_bounds' six rows of 1024 floats and the two words the fault bits and the largest material index are gathered in; the pack kernel
declares none."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = "_ZN4rtgo7whitted"
CHECK, FINAL, PACK = W + "17mesh_check_kernelE", W + "23mesh_check_final_kernelE", W + "16mesh_pack_kernelE"


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


@pytest.mark.parametrize("kernel", [CHECK, FINAL, PACK])
def test_no_scratch_no_spills_no_dynamic_stack(remarks, kernel):
    r = one(remarks, kernel)
    print(kernel, sorted(r.items()))
    assert int(r["ScratchSize [bytes/lane]"]) == 0, r
    assert int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, r
    assert r["Dynamic Stack"] == "False", r


def test_static_lds_is_what_the_kernels_declare(remarks):
    declared = 4 * (6 * 1024 + 2)   # s_red[6][kMeshCheckThreads] and s_words[2]
    assert int(one(remarks, CHECK)["LDS Size [bytes/block]"]) == declared
    assert int(one(remarks, FINAL)["LDS Size [bytes/block]"]) == declared
    assert int(one(remarks, PACK)["LDS Size [bytes/block]"]) == 0
