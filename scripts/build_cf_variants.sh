#!/bin/bash
# Experimental libcep builds whose closed-form partition units (cf_kernels.hip
# CF_UNIT 9-14) are compiled with extra macros; every other object is the
# in-tree build's.  usage: scripts/build_cf_variants.sh <name>:"<macros>" ...
set -e
cd "$(dirname "$0")/../flink-siddhi_amd"
make -s -j8 >/dev/null
mkdir -p exp
for spec in "$@"; do
  name=${spec%%:*}; flags=${spec#*:}
  objs=""
  for o in build/frontend.o build/engine.o build/operator.o build/kernels.o build/reorder.o build/keymap.o \
           build/hot.o build/mq_kernels.o build/filter.o build/cf_u1.o build/cf_u2.o build/cf_u3.o build/cf_u4.o \
           build/cf_u5.o build/cf_u6.o build/cf_u7.o build/cf_u8.o build/cf_u15.o build/cf_u16.o build/cf_u17.o \
           build/cf_u18.o build/cf_u19.o build/cf_u20.o; do objs="$objs $o"; done
  for u in 9 10 11 12 13 14; do
    /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC $flags -DCF_UNIT=$u --offload-arch=gfx950 -c csrc/cf_kernels.hip -o exp/cf_u$u.$name.o &
    objs="$objs exp/cf_u$u.$name.o"
  done
  wait
  /opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 $objs -o exp/libcep_$name.so
  rm -f exp/cf_u*.$name.o
  echo "built exp/libcep_$name.so ($flags)"
done
