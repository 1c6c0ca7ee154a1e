"""Budgets of the batched build kernels of rtgo_whitted_big.h (rtgo_whitted_set_scene, rtgo_whitted_rebuild_meshes): hipcc's resource
remarks, compiled from the product source with the build flags (device code only, no GPU), as tests/test_pair_kernel_registers.py reads
them.

big_build_batch_kernel runs build_kernel's body (whitted::build_structure) and big_sah_batch_kernel sah_kernel's (whitted::sah_structure),
one workgroup per structure of a table: each may use no more VGPRs than the kernel whose body it runs, in this same compile, and has
neither scratch nor spills; each keeps that kernel's static LDS, so the two stay two kernels with their own dynamic LDS sizes.

The three single-structure kernels keep the figures of the commit before the batched builds, read from a compile of that commit with the
same flags:

    kernel         VGPRs  scratch  static LDS
    build_kernel      48        0     24 592
    sah_kernel        61        0         32
    refit_kernel      49        0     24 576

build_kernel and sah_kernel became thin callers of the shared bodies.  sah_kernel's instruction stream differs from that commit's in
scheduling and in the order of its static LDS variables only; build_kernel's also by the prefix sum that numbers the Morton records in
node order, where an atomicAdd numbered them in arrival order (profiles/r13a/asm_diff.txt).  build_kernel comes out at 47 VGPRs,
sah_kernel at 61; refit_kernel is instruction-identical.  So the VGPR figures are held as ceilings (refit_kernel's as an equality),
scratch and static LDS as equalities."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = "_ZN4rtgo7whitted"
BUILD, SAH, REFIT = W + "12build_kernelE", W + "10sah_kernelE", W + "12refit_kernelE"
BUILD_BATCH, SAH_BATCH = W + "22big_build_batch_kernelE", W + "20big_sah_batch_kernelE"
OFFSETS, PACK = W + "24big_batch_offsets_kernelE", W + "23big_pack_records_kernelE"
PARENT = {BUILD: (48, 0, 24592), SAH: (61, 0, 32), REFIT: (49, 0, 24576)}   # VGPRs, scratch bytes per lane, static LDS bytes


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


def figures(r):
    return int(r["VGPRs"]), int(r["ScratchSize [bytes/lane]"]), int(r["LDS Size [bytes/block]"])


def test_exactly_the_intended_batched_kernels(remarks):
    batched = sorted(n for n in remarks if re.search(r"big_\w*(batch|pack)\w*kernel", n))
    assert [n[:n.index("kernelE") + 7] for n in batched] == sorted([BUILD_BATCH, SAH_BATCH, OFFSETS, PACK]), batched


@pytest.mark.parametrize("batched,body", [(BUILD_BATCH, BUILD), (SAH_BATCH, SAH)])
def test_a_batched_kernel_stays_within_the_kernel_whose_body_it_runs(remarks, batched, body):
    b, k = one(remarks, batched), one(remarks, body)
    print(batched, figures(b), body, figures(k))
    assert int(b["VGPRs"]) <= int(k["VGPRs"]), (b, k)
    assert int(b["AGPRs"]) == 0 and int(b["ScratchSize [bytes/lane]"]) == 0, b
    assert int(b["VGPRs Spill"]) == 0 and int(b["SGPRs Spill"]) == 0, b
    assert b["Dynamic Stack"] == "False", b
    assert int(b["LDS Size [bytes/block]"]) == int(k["LDS Size [bytes/block]"]), (b, k)
    assert int(b["Occupancy [waves/SIMD]"]) >= int(k["Occupancy [waves/SIMD]"]), (b, k)


@pytest.mark.parametrize("helper", [OFFSETS, PACK])
def test_the_helpers_are_small(remarks, helper):
    r = one(remarks, helper)
    assert int(r["VGPRs"]) <= 32 and int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, r


@pytest.mark.parametrize("kernel", [BUILD, SAH, REFIT])
def test_the_single_structure_kernels_keep_their_figures(remarks, kernel):
    r = one(remarks, kernel)
    vgprs, scratch, lds = PARENT[kernel]
    print(kernel, figures(r), "before:", PARENT[kernel])
    assert int(r["VGPRs"]) <= vgprs, r
    assert int(r["ScratchSize [bytes/lane]"]) == scratch and int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, r
    assert int(r["LDS Size [bytes/block]"]) == lds, r
    if kernel == REFIT:
        assert int(r["VGPRs"]) == vgprs, r
