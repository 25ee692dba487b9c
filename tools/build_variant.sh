#!/bin/bash
# Build an A/B variant of libdruidgpu.so: tools/build_variant.sh NAME [-DFOO ...]
# Every source the Makefile builds, with the extra flags, into incubator-druid_amd/lib/variants/NAME.
# DG_CSRC=dir builds the sources of another directory (a patched copy of csrc/, for a variant that is an
# edit and not a flag; the headers include ../../include/druidgpu.h, so copy include/ beside it as well).
# Load the result with DRUID_AMD_LIB=incubator-druid_amd/lib/variants/NAME/libdruidgpu.so.
set -e
name=$1; shift
root="$(cd "$(dirname "$0")/.." && pwd)"
src="${DG_CSRC:-$root/incubator-druid_amd/csrc}"
out="$root/incubator-druid_amd/lib/variants/$name"
mkdir -p "$out/obj"
H="/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 -Wno-unused-value -Wno-unused-result -I$root/include $*"
pids=()
for f in "$src"/*.hip; do
  $H -c -x hip "$f" -o "$out/obj/$(basename "${f%.hip}").o" & pids+=($!)
done
for f in "$src"/*.cpp; do
  $H -c "$f" -o "$out/obj/$(basename "${f%.cpp}").o" & pids+=($!)
done
for p in "${pids[@]}"; do wait "$p"; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$out/libdruidgpu.so" "$out"/obj/*.o
echo "$out/libdruidgpu.so"
