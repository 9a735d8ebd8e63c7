#!/bin/bash
# Build the MI355X encoder library in-tree: hmp3_amd/libhmp3amd.so (gfx950 only).
# The translation units, their compilers and their flags come from csrc/hx_units.tab, with the measurements behind the flags.
# -ffp-contract=off: the kernels must not fuse multiply-adds (bit-exactness against the oracle).
# HX_EXTRA: extra compiler flags (e.g. -DHX_PROFILE); HX_ALLOC_EXTRA: the same for the allocator kernels only; HX_LIBNAME: build a variant library next to the product
# (objects go to a directory of their own, so variants can be built side by side).
set -e
cd "$(dirname "$0")/csrc"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
LIB=${HX_LIBNAME:-libhmp3amd.so}
OBJ=$(mktemp -d /tmp/hxbuild.XXXXXX)
trap 'rm -rf "$OBJ"' EXIT
TAB=hx_units.tab
ILP="-mllvm -amdgpu-sched-strategy=iterative-ilp"
ALLOC_SCHED="${HX_ALLOC_SCHED-$ILP}"
NOLICM="${HX_NOLICM--mllvm -disable-machine-licm}"
# build id = hash of the kernel / host sources and of the flags that change the generated code
BUILD_ID=$( (LC_ALL=C; cat *.hip *.inc *.h *.cpp $TAB ../build.sh; $HIPCC --version; echo "${HX_OPT:--O3} $HX_EXTRA ${HX_ALLOC_OPT:--O2} $HX_ALLOC_EXTRA $ALLOC_SCHED $NOLICM $HX_FRONT_EXTRA $HX_PACK_EXTRA") | sha256sum | cut -c1-16)
FLAGS="-DHX_BUILD_ID=\"$BUILD_ID\" --offload-arch=gfx950 $HX_EXTRA -fPIC -ffp-contract=off -fno-fast-math -std=c++17 -Wall -Wno-unused-variable -Wno-unused-but-set-variable -Wno-unused-value -Wno-unused-result"
pids=()
while read -r unit cc group own; do
  case "$unit" in ''|'#'*) continue ;; esac
  if [ $cc = g++ ]; then
    g++ $own -fPIC -ffp-contract=off -std=c++17 -Wno-unused-result -D__HIP_PLATFORM_AMD__ -I"$(dirname "$(dirname "$HIPCC")")/include" -c $unit.cpp -o $OBJ/$unit.cpp.o & pids+=($!)
    continue
  fi
  # the table's default flags, each replaced by its override where one is set
  own=${own/-O3/${HX_OPT:--O3}}
  own=${own/-mllvm -disable-machine-licm/$NOLICM}
  case $group in
    front) own="$own $HX_FRONT_EXTRA" ;;
    pack)  own="$own $HX_PACK_EXTRA" ;;
    alloc) own=${own/-O2/${HX_ALLOC_OPT:--O2}}; own="${own/$ILP/$ALLOC_SCHED} $HX_ALLOC_EXTRA" ;;
  esac
  $HIPCC $FLAGS $own -c $unit.hip -o $OBJ/$unit.hip.o & pids+=($!)
done < $TAB
# (every compiler is waited for before a failure ends the script: the EXIT trap removes the object directory)
rc=0
for p in "${pids[@]}"; do wait $p || rc=1; done
[ $rc -eq 0 ] || { echo "build failed" >&2; exit 1; }
$HIPCC --offload-arch=gfx950 -shared -o ../$LIB $OBJ/*.o
[ -n "$HX_LIBNAME" ] || g++ -O2 -std=c++17 -Wall ../cli/hmp3amd.cpp -o ../hmp3amd -L.. -lhmp3amd -Wl,-rpath,'$ORIGIN' -Wl,-rpath,/opt/rocm/lib
echo built hmp3_amd/$LIB build_id=$BUILD_ID
