#!/bin/bash
# Build A/B variants of the v10 KMeans kernel into variants/libalink_hip_<name>.so (the in-tree lib's other
# objects + a variant kmeans_v10.o), for tools/kmeans_ab.py.  Run after `python build_native.py`.
#   timing   : -DKM10_TIMING=1 (per-workgroup stamps and per-role wait sums; tools/kmeans_wg_timing.py).
#              `... timing` builds only this one
#   pfd      : -DKM10_PFD=1 (the ALINK_KMEANS_V10_PFD L2 prefetch A/B; `... pfd` builds only this one)
# `... NAME "FLAGS"` builds one variant with any other compile flags.
set -e
cd "$(dirname "$0")/.."
mkdir -p variants
build_var() {
  name=$1; flags=$2; d=build/variants/$name
  mkdir -p "$d"
  cp alink_amd/ops/csrc/kmeans_v10.hip alink_amd/ops/csrc/kmeans_tile.h alink_amd/ops/csrc/kmeans_v10_body.h "$d/"
  (cd "$d" && /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -mcode-object-version=5 $flags \
      -c kmeans_v10.hip -o kmeans_v10.o)
  objs=$(ls build/hip/*.o | grep -v kmeans_v10)
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "variants/libalink_hip_$name.so" $objs "$d/kmeans_v10.o"
}
[ "$1" = timing ] && { build_var timing "-DKM10_TIMING=1"; exit 0; }
[ "$1" = pfd ] && { build_var pfd "-DKM10_PFD=1"; exit 0; }
[ -n "$1" ] && { build_var "$1" "$2"; exit 0; }
build_var timing "-DKM10_TIMING=1"
build_var pfd "-DKM10_PFD=1"
