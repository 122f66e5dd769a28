#!/bin/bash
# device assembly of every csrc/*.hip, for proving that a refactor changed no
# kernel: tools/device_asm.sh OUTDIR [extra hipcc flags] -> OUTDIR/<name>.s
# Run it on two checkouts and `diff -r` the two OUTDIRs, or compare them
# function by function with tools/asm_diff.py. Lines with the
# compiler's per-translation-unit __hip_cuid_<hash> symbol are dropped.
set -e -o pipefail
OUTDIR=$(mkdir -p "$1" && cd "$1" && pwd); shift
cd "$(dirname "$0")/../adaptive-mcmc_amd/csrc"
FLAGS=$(make -s --no-print-directory flags)
pids=()
for src in *.hip; do
  ${HIPCC:-/opt/rocm/bin/hipcc} $FLAGS "$@" --offload-device-only -S "$src" -o - \
    | grep -v __hip_cuid_ > "$OUTDIR/${src%.hip}.s" &
  pids+=($!)
done
for p in "${pids[@]}"; do wait "$p"; done
