#!/bin/bash
# a variant of the library that differs in ONE source file's compile flags -> tools/out/libzebra_NAME.so
#   tools/build_variant.sh NAME "-DZT_SOMETHING=1 ..." [source.hip, default tppr_stream.hip]
#   (run it with tools/exp/bench_lib.py tools/out/libzebra_NAME.so <bench.py args>)
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
NAME=${1:?name}; FLAGS=$2; SRC=${3:-tppr_stream.hip}
cd $R/zebra_amd/csrc
O=$R/tools/out
mkdir -p $O
FP=""; case $SRC in tppr_stream.hip|tppr_prune.hip) FP="-ffp-contract=off";; esac
hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC $FP $FLAGS -I$R/zebra_amd/csrc -c $SRC -o $O/v_$NAME.o
L=$R/zebra_amd/lib
OBJS=$(ls $L/*.o | grep -v "/${SRC%.hip}.o\|test_hooks.o")
hipcc --offload-arch=gfx950 -shared -fPIC -o $O/libzebra_$NAME.so $O/v_$NAME.o $OBJS -ldl -lrt
# the same library under the product's file name in a directory of its own, with the test hooks linked against it: what
# ZT_TEST_LIB=tools/out/NAME/libzebra_amd.so (tests/conftest.py) loads -- the hooks resolve against THIS build
mkdir -p $O/$NAME
cp $O/libzebra_$NAME.so $O/$NAME/libzebra_amd.so
hipcc --offload-arch=gfx950 -shared -fPIC -o $O/$NAME/libzebra_amd_testhooks.so $L/test_hooks.o -L$O/$NAME -lzebra_amd -Wl,-rpath,'$ORIGIN'
echo $O/libzebra_$NAME.so
