#!/bin/bash
# A/B of a kernel change on ONE box (boxes of the pool differ by +-3 %): builds the library of the last COMMIT beside the working
# tree's, as csrc/exp/head.so.  Then, in one gpurun call:
#   bash tools/kernel_times.sh head $PWD/3d-.../csrc/exp/head.so && bash tools/kernel_times.sh new ''
set -e
root=$(cd "$(dirname "$0")/.." && pwd)
pkg=3d-gaussian-splatting-for-novel-view-synthesis_amd
tmp=$(mktemp -d)
git -C $root archive HEAD $pkg/csrc include | tar -x -C $tmp          # the whole of HEAD's csrc/ and include/, whatever files they hold
make -s -C $tmp/$pkg/csrc libgsplat_mi355x.so          # HEAD's own Makefile: whatever sources the library has there
mkdir -p $root/$pkg/csrc/exp
cp $tmp/$pkg/csrc/libgsplat_mi355x.so $root/$pkg/csrc/exp/head.so
rm -rf $tmp
echo "built $pkg/csrc/exp/head.so from $(git -C $root rev-parse --short HEAD)"
