#!/bin/bash
# Per-kernel register / spill / LDS usage of built HIP objects
# (default: every fused-MLP unit of the library build, build/mlp*.o).
#   tools/kres.sh [OBJECT ...]
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
[ $# -gt 0 ] || set -- "$ROOT"/robust-nerf_amd/build/mlp*.o
for OBJ in "$@"; do
  TMP=$(mktemp -d)
  cp "$OBJ" "$TMP/k.o"
  ( cd "$TMP"
    /opt/rocm/lib/llvm/bin/llvm-objdump --offloading k.o > /dev/null
    [ -f k.o.0.hipv4-amdgcn-amd-amdhsa--gfx950 ] || exit 0   # a unit without kernels
    /opt/rocm/lib/llvm/bin/llvm-readelf --notes k.o.0.hipv4-amdgcn-amd-amdhsa--gfx950 |
      grep -E "^\s+\.name:|\.vgpr_count|\.agpr_count|spill_count|group_segment_fixed_size" | grep -v args |
      sed 's/  */ /g' | paste -d' ' - - - - - - | sed 's/_ZN2nr//' | cut -c1-220 )
  rm -rf "$TMP"
done
