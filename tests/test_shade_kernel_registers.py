"""Register budgets of shade_rays_kernel (rtgo_shade_rays), its four instantiations <PATH, SCENE_IN_LDS>: hipcc's resource remarks for the
product source under the build flags (device code only, no GPU), as tests/test_pair_kernel_registers.py reads them.

Every instantiation: at most 128 VGPRs, no scratch, no VGPR spill, at least 4 waves per SIMD -- what a 1024-lane workgroup needs to be
resident at all, and what the host sizes the grid by.

VGPRs read from this compile (no scratch, no spill): <path, global> 93 and <path, LDS> 86 at 5 waves per SIMD, <distributed, global> 111
and <distributed, LDS> 108 at 4.  Both modes keep the level records in registers: with them in LDS distributed mode took 92 / 85 VGPRs,
but the 80 bytes a lane more halved the waves the stacks leave a CU room for, and it was the slower form."""
import pytest

from test_pair_kernel_registers import compiled, one   # noqa: F401  (compiled: the module's fixture)

SHADE = "_ZN4rtgo17shade_rays_kernelILb%dELb%dEEE"
KINDS = [(1, 0), (1, 1), (0, 0), (0, 1)]   # <PATH, SCENE_IN_LDS>


@pytest.mark.parametrize("path,in_lds", KINDS)
def test_shade_kernel_resources(compiled, path, in_lds):
    remarks, _ = compiled
    r = remarks[one(remarks, SHADE % (path, in_lds))]
    print(SHADE % (path, in_lds), r)
    assert int(r["VGPRs"]) <= 128, r
    assert int(r["ScratchSize [bytes/lane]"]) == 0, r
    assert int(r["VGPRs Spill"]) == 0, r
    assert int(r["Occupancy [waves/SIMD]"]) >= 4, r


def test_exactly_four_shade_kernels(compiled):
    remarks, _ = compiled
    mine = sorted(n for n in remarks if "shade_rays_kernel" in n)
    assert mine == sorted(one(remarks, SHADE % k) for k in KINDS)
