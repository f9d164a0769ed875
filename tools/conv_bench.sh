#!/bin/bash
# Build conv_bench variants (knock-out masks) here; run them on the GPU with RUN=1.  Each variant links
# tools/conv_bench.cpp against the library's own conv dispatch and kernels (csrc/Makefile target conv_objs:
# conv.o, conv_bwd.o and one object per row of conv_inst.hip's table), built with -DSDP_KO=<mask> and EXTRA.
# TAG=<name>: name the (single) build conv_bench_<name> instead of by its mask (e.g. EXTRA=-DSDP_TIMING TAG=T)
set -eu
cd "$(dirname "$0")/.."
mkdir -p tools/_cb
SRC=simultaneous-diffusion-for-pointclouds_amd/csrc
if [ "${RUN:-0}" = 0 ]; then
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 ${EXTRA:-} -c tools/conv_bench.cpp -o tools/_cb/main.o
  H=$(python3 -c "import sys; sys.path.insert(0, 'simultaneous-diffusion-for-pointclouds_amd'); from sdp import _build; print(_build.conv_source_hash())")
  for ko in ${KOS:-0 1 2 4 8 16}; do
    t=${TAG:-$ko}
    make -B -C $SRC -j${JOBS:-8} OBJDIR=$PWD/tools/_cb/obj_$t EXTRA="-DSDP_KO=$ko ${EXTRA:-}" conv_objs > tools/_cb/build_$t.log 2>&1 \
      || { tail -30 tools/_cb/build_$t.log; exit 1; }
    /opt/rocm/bin/hipcc --offload-arch=gfx950 tools/_cb/main.o tools/_cb/obj_$t/*.o -o tools/_cb/conv_bench_$t
    rm -rf tools/_cb/obj_$t
    echo "$H ${EXTRA:-}" > tools/_cb/conv_bench_$t.hash     # the conv sources (and extra flags) it was built from
  done
else
  for ko in ${KOS:-0 1 2 4 8 16}; do
    echo "KO=$ko"
    timeout -k 5 60 tools/_cb/conv_bench_$ko 256 256 32 512 ${B:-4} 1 20 ${MODE:-1}
    timeout -k 5 60 tools/_cb/conv_bench_$ko 128 128 64 1024 ${B:-4} 1 20 ${MODE:-1}
  done
fi
