#!/bin/bash
# Per-kernel VGPRs / scratch / occupancy of HIP sources (dev tool).
# usage: scripts/regs.sh FILE.hip [FILE.hip ...]
#   e.g. the megakernel's two render units, from concurrent-raytracer-go_amd/:
#   ../scripts/regs.sh csrc/rt_kernel.hip csrc/rt_stream.hip
for f in "$@"; do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -munsafe-fp-atomics -x hip -c "$f" \
    -o /tmp/regs.o -Rpass-analysis=kernel-resource-usage 2>&1 |
    grep -E "Function Name|VGPRs:|ScratchSize|Occupancy" | sed -E 's/.*remark: [^ ]+ +//; s/ \[-Rpass.*//' | paste - - - -
done
