#!/bin/bash
# Build a variant of libdpc_render.so into scratch/<name>/ with extra compiler flags (timing experiments, stamps):
#   tools/build_variant.sh <name> [extra hipcc flags...]        e.g.  tools/build_variant.sh abl -DDPC_ABLATE
#   SRC_REV=<git rev> tools/build_variant.sh <name> ...         builds the sources of that commit instead of the working tree
# The build is the Makefile's (its sources and per-file flags) on a copy of csrc/ and include/ under scratch/<name>/src;
# the extra flags reach every hipcc call.  The variant is loaded by pointing dpc.render._native.LIB_PATH (or
# DPC_RENDER_LIB) at it; never shipped as the product.
set -e
name=$1; shift
root=$(cd "$(dirname "$0")/.." && pwd)
out=$root/scratch/$name
tmp=$out/src
rm -rf $tmp; mkdir -p $tmp
if [ -n "$SRC_REV" ]; then
  git -C $root archive $SRC_REV pytorch-unsup-pc_amd/csrc include | tar -x -C $tmp
else
  mkdir -p $tmp/pytorch-unsup-pc_amd
  cp -r $root/pytorch-unsup-pc_amd/csrc $tmp/pytorch-unsup-pc_amd/
  cp -r $root/include $tmp/
  make -s -C $tmp/pytorch-unsup-pc_amd/csrc clean
fi
make -C $tmp/pytorch-unsup-pc_amd/csrc -j8 HIPCC="/opt/rocm/bin/hipcc $*"
mv $tmp/pytorch-unsup-pc_amd/csrc/libdpc_render.so $out/
rm -rf $tmp
echo "built $out/libdpc_render.so"
