#!/usr/bin/env bash
# Resource usage (VGPRs / spills / occupancy) of the kernels that trace:
#   tools/vgprs.sh [spt_kernel.hip | spt_guide.hip] [extra hipcc flags]   (no file: both)
cd "$(dirname "$0")/../small-pathtracer_amd/csrc"
files="spt_kernel.hip spt_guide.hip"
case "$1" in *.hip) files="$1"; shift ;; esac
for f in $files; do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off \
    -fhip-fp32-correctly-rounded-divide-sqrt -fno-slp-vectorize --offload-device-only -S \
    -o /tmp/vgprs.s "$f" -Rpass-analysis=kernel-resource-usage "$@" 2>&1 |
    grep -E "Function Name|    VGPRs:|TotalSGPRs|Occupancy|Spill" | sed 's/ \[-Rpass.*//; s/.*remark: *//' |
    paste - - - - - - | grep -E "render_kernel|guide_kernel" |
    sed 's/Function Name: _ZN3spt13render_kernelINS_4Topo//; s/Function Name: _ZN3spt12//'
done
