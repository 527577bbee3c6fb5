#!/bin/bash
# Builds an alternative libtopsy_splat (extra compiler defines) next to the product library, for A/B measurements:
#   tools/build_variant.sh <suffix> -DTSP_HDEAL=4 ...   ->  topsy_amd/libtopsy_splat_<suffix>.so  (select it with TOPSY_SPLAT_LIB)
# The sources and flags are the Makefile's; the objects go to a directory of their own, removed afterwards.
set -e
SUF=$1; shift
ROOT=$(cd $(dirname $0)/.. && pwd)
make -C $ROOT/topsy_amd/csrc -j8 OBJDIR=build_$SUF OUT=../libtopsy_splat_$SUF.so EXTRA="$*"
rm -rf $ROOT/topsy_amd/csrc/build_$SUF
echo built topsy_amd/libtopsy_splat_$SUF.so
