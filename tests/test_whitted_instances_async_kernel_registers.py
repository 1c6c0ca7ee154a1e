"""Budgets of the two kernels of rtgo_whitted_refit_instances_device_async (rtgo_whitted_inst_update.h): hipcc's resource remarks,
compiled from the product source with the build flags (device code only, no GPU), as
tests/test_whitted_instances_device_kernel_registers.py reads them.

inst_commit_kernel moves two flat streams and four float4 per lane, inst_refit_gated_kernel is refit_kernel behind five scalar loads:
neither has a reason to touch scratch, to spill or to need a dynamic stack.  The commit stages nothing (its copies are coalesced as they
stand), so its LDS is 0; the gated refit's is refit_structure's reduction array, 6 x kBuildThreads floats.

The kernels the new call runs unchanged or shares a body with -- refit_kernel, inst_prepare_kernel, inst_gather_kernel -- must compile as
they did: PARENT holds their remarks from a compile of the commit before this call was added."""
import pytest

from test_whitted_instances_device_kernel_registers import GATHER, PREPARE, W, one, remarks   # noqa: F401 (remarks: the fixture)

COMMIT, GATED = W + "18inst_commit_kernelE", W + "23inst_refit_gated_kernelE"
REFIT = W + "12refit_kernelE"
K_BUILD_THREADS = 1024

PARENT = {
    REFIT: {"TotalSGPRs": "35", "VGPRs": "49", "AGPRs": "0", "ScratchSize [bytes/lane]": "0", "Dynamic Stack": "False", "Occupancy [waves/SIMD]": "8",
            "SGPRs Spill": "0", "VGPRs Spill": "0", "LDS Size [bytes/block]": "24576"},
    PREPARE: {"TotalSGPRs": "42", "VGPRs": "74", "AGPRs": "0", "ScratchSize [bytes/lane]": "0", "Dynamic Stack": "False", "Occupancy [waves/SIMD]": "5",
              "SGPRs Spill": "0", "VGPRs Spill": "0", "LDS Size [bytes/block]": "27648"},
    GATHER: {"TotalSGPRs": "16", "VGPRs": "20", "AGPRs": "0", "ScratchSize [bytes/lane]": "0", "Dynamic Stack": "False", "Occupancy [waves/SIMD]": "8",
             "SGPRs Spill": "0", "VGPRs Spill": "0", "LDS Size [bytes/block]": "0"},
}


@pytest.mark.parametrize("kernel", [COMMIT, GATED])
def test_no_scratch_no_spills_no_dynamic_stack(remarks, kernel):
    r = one(remarks, kernel)
    print(kernel, sorted(r.items()))
    assert int(r["ScratchSize [bytes/lane]"]) == 0, r
    assert int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, r
    assert r["Dynamic Stack"] == "False", r


def test_the_commit_stages_nothing_and_the_gated_refit_holds_the_reduction_array(remarks):
    assert int(one(remarks, COMMIT)["LDS Size [bytes/block]"]) == 0
    assert int(one(remarks, GATED)["LDS Size [bytes/block]"]) == 4 * 6 * K_BUILD_THREADS


@pytest.mark.parametrize("kernel", sorted(PARENT))
def test_the_kernels_it_shares_compile_as_before(remarks, kernel):
    assert one(remarks, kernel) == PARENT[kernel]
