#!/bin/bash
# diagnostic builds of libamh.so with compile-time switches of one source
# file: tools/build_variants.sh SRC "name:-DFLAG ..." ... -> lib/var_<name>/libamh.so
# (select one at run time with AMH_LIB_PATH).  The compile flags are the
# Makefile's (its `flags` target), so a variant differs from the release
# build by its own defines only.
set -e
cd "$(dirname "$0")/../adaptive-mcmc_amd/csrc"
SRC=$1; shift
OUT=../lib
FLAGS=$(make -s --no-print-directory flags)
base=$(basename $SRC .hip)
for v in "$@"; do
  name=${v%%:*}; defs=${v#*:}
  mkdir -p $OUT/var_$name
  /opt/rocm/bin/hipcc $FLAGS $defs -c $SRC -o $OUT/var_$name/v.o
  objs=$(ls $OUT/*.o | grep -v "/$base.o")
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $OUT/var_$name/libamh.so $OUT/var_$name/v.o $objs
  echo built $name
done
