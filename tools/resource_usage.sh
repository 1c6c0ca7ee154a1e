#!/bin/bash
# developer tool: VGPRs / spills / scratch / occupancy / LDS of every kernel of librtgo_hip.so (hipcc remarks), one line per kernel
root="$(cd "$(dirname "$0")/.." && pwd)"
out="$(mktemp)"
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-slp-vectorize -mllvm -amdgpu-atomic-optimizer-strategy=None "$@" \
  --cuda-device-only -S -Rpass-analysis=kernel-resource-usage -o "$out" "$root/raytracingo_amd/csrc/rtgo_capi.hip" 2>&1 |
  grep -E "Function Name|VGPRs:|Spill:|ScratchSize|Occupancy|LDS Size" | sed -E 's/.*remark: +//; s/ \[-Rpass.*//; s/Function Name: _ZN4rtgo[0-9]*/@/; s/EvNS_12LaunchParams.*//; s/(render_pair7_kernel)ENS_12LaunchParams.*/\1/;s/EPKNS_6PrimIn.*//; s/EvNS_11TraceParams.*//; s/EvNS0_15TraceRaysParams.*//; s/EvNS0_15ShadeRaysParams.*//' |
  tr '\n' ' ' | tr '@' '\n'; echo
rm -f "$out"
