#!/bin/bash
# builds tools/variants/libmpgan_<name>.so: the product library with other settings of the development switches of the
# F16F6 K loop (mpgan_conv_f6.hip) and the small-channel kernels (mpgan_conv_small.hip).  Only these two units are
# compiled per variant; every other object is the product build's (the Makefile's list).
set -e
cd "$(dirname "$0")/../multi-pass-gan_amd/csrc"
OUT=../../tools/variants
mkdir -p $OUT
make -j4
SWITCHED="mpgan_conv_f6 mpgan_conv_small"
OBJS=$(make -s print-objs)
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-function -fno-slp-vectorize -fno-vectorize -I../../include -I."
build() {  # name, extra flags ("@slp" among them: build WITH the SLP / loop vectorisers, i.e. packed fp32 allowed)
  name=$1; shift
  local F="$FLAGS" args=() objs="$OBJS" u
  for a in "$@"; do if [ "$a" = "@slp" ]; then F="${FLAGS/-fno-slp-vectorize -fno-vectorize/}"; else args+=("$a"); fi; done
  set -- "${args[@]}"
  FLAGS_USED="$F"
  for u in $SWITCHED; do
    /opt/rocm/bin/hipcc $F "$@" -c $u.hip -o $OUT/${u}_$name.o
    objs="${objs/$u.o/$OUT/${u}_$name.o}"
  done
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $objs -o $OUT/libmpgan_$name.so
  for u in $SWITCHED; do rm $OUT/${u}_$name.o; done
}
for spec in "$@"; do
  name=${spec%%:*}; flags=${spec#*:}
  build $name $flags &
done
wait
ls -la $OUT
