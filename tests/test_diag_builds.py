"""Every diagnostic flag set still compiles (device side, syntax only): the probe types of csrc/rtgo_probes.h have a real and an
empty definition each, and only the empty ones are compiled by the product build."""
import os
import subprocess

import pytest

from raytracingo_amd import _build

SRC = os.path.join(_build.PKG, "csrc", "rtgo_capi.hip")
DIAG_FLAGS = ["-DRTGO_TIMELINE", "-DRTGO_STREAM_STATS", "-DRTGO_FAST_COUNTERS=1", "-DRTGO_FAST_COUNTERS=2", "-DRTGO_CMPWALK", "-DRTGO_WHITTED_TIMING"]


@pytest.mark.parametrize("flag", DIAG_FLAGS)
def test_diagnostic_build_compiles(flag):
    cmd = [_build.HIPCC] + [f for f in _build.HIP_FLAGS if f != "-shared"] + [flag, "--cuda-device-only", "-fsyntax-only", SRC]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-4000:]
