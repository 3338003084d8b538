#!/bin/bash
# Builds an A/B copy of libulg.so with extra preprocessor definitions for
# the cBIC scorer's objects, csrc/cbic*.hip (the other objects come from
# urlearning-cpp_amd/build/):
#   scripts/build_variant.sh NAME "-DFOO=1 -DBAR"  -> urlearning-cpp_amd/ablib/NAME/libulg_NAME.so (travels to the GPU box; *.o and *.so stay out of git)
set -eu
cd "$(dirname "$0")/.."
NAME=$1; DEFS=${2:-}
OUT=urlearning-cpp_amd/ablib/$NAME
mkdir -p $OUT
FLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -Xarch_host -mpopcnt -Xarch_host -mbmi2 -Wall -Wno-unused-function -Wno-unused-result"
CBIC=""; PIDS=""
for src in urlearning-cpp_amd/csrc/cbic*.hip; do
  obj=$OUT/$(basename $src .hip).o
  rm -f $obj
  /opt/rocm/bin/hipcc $FLAGS $DEFS -c -o $obj $src &
  PIDS="$PIDS $!"
  CBIC="$CBIC $obj"
done
for pid in $PIDS; do wait $pid; done  # a failed compile stops the script (set -e)
OBJS=$(ls urlearning-cpp_amd/build/*.o | grep -v -e '/cbic[a-z_]*\.o$' -e '_ru\.o$')
/opt/rocm/bin/hipcc $FLAGS -shared -o $OUT/libulg_$NAME.so $CBIC $OBJS
echo $OUT/libulg_$NAME.so
