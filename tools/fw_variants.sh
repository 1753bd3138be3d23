#!/bin/bash
# tools/fw_variants.sh "name|flags" ... -- on the GPU box: the wide fused kernels (build/fw_conv_13 .. 23.o) rebuilt with extra flags as a scratch
# library under variants/ (tools/variant.sh; the repo's own build is not touched), timed with tools/fw_dev.py --no-check $FW_DEV_ARGS
for spec in "$@"; do
    name=${spec%%|*}; flags=${spec#*|}
    "$(dirname "$0")"/variant.sh "fw_$name" "fw_conv_13 fw_conv_15 fw_conv_17 fw_conv_19 fw_conv_21 fw_conv_23" "$flags" \
        bash -c "timeout -k 10 200 python tools/fw_dev.py --no-check $FW_DEV_ARGS 2>&1 | grep -v amdgpu.ids" || exit 1
done
