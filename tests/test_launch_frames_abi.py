"""rtgo_launch_frames without a GPU: the entry is declared, exported and bound, the ABI's sizes and version stand, the batched kernels
(render_frames_kernel, six instantiations) fit their register budgets without scratch, and the command line has the flag.

The register check compiles the product source's device code with the build flags and reads hipcc's resource remarks only, as
test_bench_kernel_registers.py does."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# render_frames_kernel<PATH, WPE, FRAMES>: path mode over scenes with quadrics / over flat scenes, distributed mode; at 4 and at 5 waves
BATCHED = [(path, wpe, frames) for (path, frames) in ((True, False), (True, True), (False, False)) for wpe in (4, 5)]
VGPR_BUDGET = {4: 128, 5: 96}


@pytest.fixture(scope="module")
def capi():
    from raytracingo_amd import _build, capi as m
    _build.build_all()
    m.load()
    return m


def test_entry_is_declared_exported_and_bound(capi):
    src = open(os.path.join(ROOT, "include", "rtgo.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+rtgo_launch_frames\s*\(\s*rtgo_ctx\s*\*\s*\w+\s*,\s*const\s+rtgo_frame\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*\)\s*;", code)
    assert "bit 7" in src   # rtgo_stats::last_variant documents the batched launches' bit
    assert "rtgo_launch_frames" in capi.SYMBOLS
    assert capi.load().rtgo_launch_frames is not None
    assert callable(getattr(capi.Context, "launch_frames", None))


def test_abi_sizes_and_version_stand(capi):
    assert C.sizeof(capi.Frame) == 64 and C.sizeof(capi.Stats) == 104
    assert capi.load().rtgo_abi_version() == 6
    src = open(os.path.join(ROOT, "include", "rtgo.h")).read()
    assert re.search(r"#define\s+RTGO_ABI_VERSION\s+6\b", src)


def test_host_entries_are_exported(capi):
    from raytracingo_amd import scene
    L = scene.load()
    assert L.rtgo_host_render_batched is not None and L.rtgo_host_render_multi_batched is not None
    assert callable(scene.host_render_batched) and callable(scene.host_render_multi_batched)


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    from raytracingo_amd import _build
    out = str(tmp_path_factory.mktemp("isa") / "rtgo_device.s")
    flags = [f for f in _build.HIP_FLAGS if f != "-shared"]
    res = subprocess.run([_build.HIPCC] + flags + ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", "-o", out,
                          os.path.join(_build.PKG, "csrc", "rtgo_capi.hip")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    found, name = {}, None
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


@pytest.mark.parametrize("path,wpe,frames", BATCHED)
def test_batched_kernel_resources(remarks, path, wpe, frames):
    mangled = "_ZN4rtgo20render_frames_kernelILb%dELi%dELb%dEEE" % (path, wpe, frames)
    mine = [n for n in remarks if n.startswith(mangled)]
    assert len(mine) == 1, sorted(n for n in remarks if "render_frames_kernel" in n)
    r = remarks[mine[0]]
    print(mine[0], r)
    assert int(r["ScratchSize [bytes/lane]"]) == 0, r
    assert int(r["VGPRs Spill"]) == 0, r
    assert int(r["VGPRs"]) <= VGPR_BUDGET[wpe], r
    assert int(r["Occupancy [waves/SIMD]"]) == wpe, r


def test_no_other_batched_instantiation(remarks):
    assert len([n for n in remarks if "render_frames_kernel" in n]) == len(BATCHED)


def test_cli_lists_the_flag(capi):
    exe = os.path.join(ROOT, "raytracingo_amd", "rtgo_engine")
    r = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert "--frames-per-launch" in r.stdout + r.stderr
