"""Register budgets of the whitted render kernels, the single-subframe instantiations and their FRAMES forms (rtgo_whitted_launch_frames:
several lanes per pixel, render_tile_subframes): hipcc's resource remarks for the product source under the build flags (device code only,
no GPU), as tests/test_pair_kernel_registers.py reads them.

Every instantiation: at most 128 VGPRs, no scratch, no VGPR spill, 4 waves per SIMD -- one 1024-thread workgroup per CU.  The
single-subframe kernels may not rise above what they had before the FRAMES switch existed; the FRAMES forms get the same ceiling.

VGPRs read from this compile (single-subframe kernel before the switch / with it / its FRAMES form):
    render_kernel<kAllInL2>             124 / 124 / 120
    render_kernel<kRecordsInLds>        124 / 124 / 120
    render_kernel<kAllInLds>            128 / 128 / 128
    render_inst_kernel<false, false>    117 / 117 / 113
    render_inst_kernel<true, false>     120 / 120 / 116
    render_inst_kernel<false, true>     128 / 128 / 127
    render_inst_kernel<true, true>      128 / 128 / 128
Scratch and VGPR spills are 0 and the occupancy is 4 in all fourteen (seven before).  Before the switch the kernels' names had no third (render_kernel:
second) template argument: _ZN4rtgo7whitted13render_kernelILi<MODE>EEE..., _ZN4rtgo7whitted18render_inst_kernelILb<TOP>ELb<CLUSTERED>EEE..."""
import pytest

from test_pair_kernel_registers import compiled, one   # noqa: F401  (compiled: the module's fixture)

MESH = "_ZN4rtgo7whitted13render_kernelILi%dELb%dEEE"
INST = "_ZN4rtgo7whitted18render_inst_kernelILb%dELb%dELb%dEEE"
# (name pattern, template arguments ahead of FRAMES, the single-subframe kernel's VGPRs before the FRAMES switch)
KERNELS = [(MESH, (0,), 124), (MESH, (1,), 124), (MESH, (2,), 128),
           (INST, (0, 0), 117), (INST, (1, 0), 120), (INST, (0, 1), 128), (INST, (1, 1), 128)]
CEILING = 128


@pytest.mark.parametrize("frames", [0, 1])
@pytest.mark.parametrize("pattern,args,before", KERNELS)
def test_whitted_render_kernel_resources(compiled, pattern, args, before, frames):
    remarks, _ = compiled
    r = remarks[one(remarks, pattern % (args + (frames,)))]
    print(pattern % (args + (frames,)), r)
    assert int(r["VGPRs"]) <= (CEILING if frames else before), r
    assert int(r["ScratchSize [bytes/lane]"]) == 0, r
    assert int(r["VGPRs Spill"]) == 0, r
    assert int(r["Occupancy [waves/SIMD]"]) == 4, r


def test_no_other_whitted_render_kernel(compiled):
    remarks, _ = compiled
    mine = sorted(n for n in remarks if n.startswith(("_ZN4rtgo7whitted13render_kernelI", "_ZN4rtgo7whitted18render_inst_kernelI")))
    assert mine == sorted(one(remarks, pattern % (args + (frames,))) for pattern, args, _ in KERNELS for frames in (0, 1))
