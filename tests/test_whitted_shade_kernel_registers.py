"""Register budgets of whitted_shade_kernel (rtgo_whitted_shade_rays), one instantiation per kind of walk: hipcc's resource remarks for the
product source under the build flags (device code only, no GPU), as tests/test_pair_kernel_registers.py reads them.

Every instantiation: at most 128 VGPRs, no scratch, no VGPR spill, at least 4 waves per SIMD -- four of its 256-lane workgroups per CU,
what the host sizes the grid by.

VGPRs read from this compile: kTraceMesh 111, kTraceInst 106, kTraceInstLds 106, kTraceClustered 121, kTraceClusteredLds 121."""
import pytest

from test_pair_kernel_registers import compiled, one   # noqa: F401  (compiled: the module's fixture)

SHADE = "_ZN4rtgo7whitted20whitted_shade_kernelILi%dEEE"
KINDS = [0, 1, 2, 3, 4]   # kTraceMesh, kTraceInst, kTraceInstLds, kTraceClustered, kTraceClusteredLds


@pytest.mark.parametrize("kind", KINDS)
def test_whitted_shade_kernel_resources(compiled, kind):
    remarks, _ = compiled
    r = remarks[one(remarks, SHADE % kind)]
    print(SHADE % kind, r)
    assert int(r["VGPRs"]) <= 128, r
    assert int(r["ScratchSize [bytes/lane]"]) == 0, r
    assert int(r["VGPRs Spill"]) == 0, r
    assert int(r["Occupancy [waves/SIMD]"]) >= 4, r


def test_exactly_five_whitted_shade_kernels(compiled):
    remarks, _ = compiled
    mine = sorted(n for n in remarks if "whitted_shade_kernel" in n)
    assert mine == sorted(one(remarks, SHADE % kind) for kind in KINDS)
