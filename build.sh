#!/usr/bin/env bash
# Builds libdtk_hip.so (gfx950) in-tree.  hipcc cross-compiles without a GPU.
set -euo pipefail
cd "$(dirname "$0")"
SRC=detikzify_amd/csrc
OUT=detikzify_amd/lib
mkdir -p "$OUT" build
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
OBJCOPY=${OBJCOPY:-$("$(dirname "$(command -v "$HIPCC")")/hipconfig" -l)/llvm-objcopy}      # the toolchain's own (hipconfig -l: its clang directory)
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -fvisibility=hidden -Wall -Wno-unused-function -Wno-unused-variable"
UNITS="kernels_decode kernels_decode_mv kernels_batch_decode kernels_batch_gemm kernels_batch_ks kernels_batch_mx kernels_batched kernels_sample_mb kernels_cfg kernels_spec kernels_top dtk_api dtk_ops"

if [ "$(cat build/.flags 2>/dev/null)" != "$FLAGS" ]; then rm -f build/*.o; mkdir -p build; echo "$FLAGS" > build/.flags; fi
# an object is stale when its source or any header is newer: every header under csrc/ and the public one
stale() {
  [ ! -f "$1" ] && return 0
  local h
  for h in "$2" $SRC/*.h include/dtk.h; do [ "$h" -nt "$1" ] && return 0; done
  return 1
}
pids=()
objs=()
for f in $UNITS; do
  objs+=(build/$f.o)
  if stale build/$f.o $SRC/$f.hip; then
    if [ $f = dtk_ops ]; then
      # a unit without device code: the id symbol hipcc gives every HIP unit (__hip_cuid_*, exported whatever the visibility flag
      # says) is made local, so the library exports what it exported before the test entry points had a unit of their own
      ( $HIPCC $FLAGS -c $SRC/$f.hip -o build/$f.o && $OBJCOPY -w -L '__hip_cuid_*' build/$f.o ) &
    else
      $HIPCC $FLAGS -c $SRC/$f.hip -o build/$f.o &
    fi
    pids+=($!)
  fi
done
# the run loop of a batch (host code only; same flags so the exports stay include/dtk.h's)
objs+=(build/dtk_engine.o)
if [ ! -f build/dtk_engine.o ] || [ $SRC/dtk_engine.cpp -nt build/dtk_engine.o ] || [ include/dtk.h -nt build/dtk_engine.o ]; then
  $HIPCC $FLAGS -x c++ -pthread -c $SRC/dtk_engine.cpp -o build/dtk_engine.o &
  pids+=($!)
fi
for p in "${pids[@]:-}"; do [ -n "$p" ] && wait "$p"; done
$HIPCC --offload-arch=gfx950 -shared -fPIC -o $OUT/libdtk_hip.so "${objs[@]}" -pthread
echo "built $OUT/libdtk_hip.so"
