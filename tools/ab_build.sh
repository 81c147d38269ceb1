#!/bin/bash
# A/B variant of libmpcqp.so: the Makefile builds the given sources again with
# extra flags (its own flag line, per-file flags included, plus EXTRA) and
# links them with copies of the product objects (make first).  With no source
# given the whole library is built with the flags.
#   bash tools/ab_build.sh TAG "-DFLAG=1" quad_box.hip [more.hip ...]
# -> model_predictive_control_amd/lib/variants/libmpcqp_TAG.so (select it with
# MPCQP_LIB=...).
set -e
TAG=$1; FLAGS=$2; shift 2
ROOT=$(cd "$(dirname "$0")/.." && pwd)
LIB=$ROOT/model_predictive_control_amd/lib
VOBJ=$LIB/variants/obj_$TAG
rm -rf $VOBJ
mkdir -p $VOBJ
if [ $# -gt 0 ]; then
  cp -p $LIB/obj/*.o $VOBJ/
  for src in "$@"; do rm -f $VOBJ/$src.o; done
fi
make -C $ROOT/model_predictive_control_amd/csrc -j8 OBJDIR=../lib/variants/obj_$TAG \
  OUT=../lib/variants/libmpcqp_$TAG.so EXTRA="$FLAGS"
rm -rf $VOBJ
echo "built $LIB/variants/libmpcqp_$TAG.so"
