#!/bin/bash
# Experiment build (no GPU needed): libsdrk.so whose fft4096.hip is compiled with -DSDRK_F4K_TIMELINE — both loops of the
# flagship kernel, grid-stride and ticketed, then leave one 16-byte record per frame (real-time counter at the issue of the
# frame's loads, frame, workgroup) in the buffer sdrk_f4k_timeline() names.  Every other object is the product's.
#   experiments/f4k_order/build.sh      -> sdr-iq-visualizer_amd/lib_f4ktl/libsdrk.so
# Read it with experiments/f4k_order/timeline.py (SDRK_LIB points the package at this library).
set -e
cd "$(dirname "$0")/../../sdr-iq-visualizer_amd/csrc"
make -s -j8
mkdir -p ../build_f4ktl ../lib_f4ktl
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fno-slp-vectorize -ffp-contract=on -Wall -Wno-unused-function \
    -DSDRK_F4K_TIMELINE -c fft4096.hip -o ../build_f4ktl/fft4096.o
OBJS=$(ls ../build/*.o | grep -v '/fft4096\.o$')
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -pthread -o ../lib_f4ktl/libsdrk.so $OBJS ../build_f4ktl/fft4096.o
ls -la ../lib_f4ktl/libsdrk.so
