#!/bin/bash
# variant build of the library with compile-time options (phase timers -DDIGAT_GEMM_TIMERS / -DDIGAT_SPARSE_TIMERS / -DDIGAT_CF_TIMERS,
# the #ifndef DIGAT_* tuning defaults): tools/exp/build_variant.sh <name> [-Dflags...]  ->  tools/exp/lib_<name>.so
set -e
cd "$(dirname "$0")/../.."
NAME=$1; shift
hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-slp-vectorize -shared -fPIC "$@" -o tools/exp/lib_$NAME.so digat_amd/csrc/digat_kernels.hip
echo tools/exp/lib_$NAME.so
