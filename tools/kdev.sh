#!/bin/bash
# Fast inspection build of the fused-MLP units (default model instances only,
# -DNR_MLP_DEV): per-kernel registers/spills, and the gfx950 ISA in /tmp/<unit>_dev.s.
#   tools/kdev.sh [UNIT ...] [-- HIPCC_FLAGS]   UNIT: mlp_fp32, mlp_16, mlp_dw, mlp_pack
# Without a unit, every csrc/mlp_*.hip that holds kernels is built.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
SRC=$ROOT/robust-nerf_amd/csrc
UNITS=()
while [ $# -gt 0 ] && [ "$1" != "--" ]; do UNITS+=("$1"); shift; done
[ "$1" = "--" ] && shift
[ ${#UNITS[@]} -gt 0 ] || UNITS=(mlp_fp32 mlp_16 mlp_dw mlp_pack)
FLAGS="-O3 -std=c++17 --offload-arch=gfx950 -munsafe-fp-atomics -ffp-contract=off -DNR_MLP_DEV -I$ROOT/include -I$SRC"
for U in "${UNITS[@]}"; do
  echo "== $U"
  /opt/rocm/bin/hipcc $FLAGS -fPIC -c $SRC/$U.hip -o /tmp/${U}_dev.o "$@"
  "$ROOT/tools/kres.sh" /tmp/${U}_dev.o
  /opt/rocm/bin/hipcc $FLAGS --cuda-device-only -S $SRC/$U.hip -o /tmp/${U}_dev.s "$@"
done
