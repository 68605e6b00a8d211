#!/bin/bash
# A/B of a change that also touches the Python side, on ONE box (boxes of the pool differ by +-3 %): a whole checkout of a commit
# (default: the last one) beside the working tree, as exp/parent_tree, with its product library built -- tools/build_head_lib.sh's
# method for more than the library.  Then, in one GPU call:  python tools/filter3d_time.py --baseline-tree exp/parent_tree
set -e
root=$(cd "$(dirname "$0")/.." && pwd)
rev=${1:-HEAD}
pkg=3d-gaussian-splatting-for-novel-view-synthesis_amd
dst=$root/exp/parent_tree
rm -rf "$dst"
mkdir -p "$dst"
git -C "$root" archive "$rev" $pkg include oracle bench.py | tar -x -C "$dst"
make -s -C "$dst/$pkg/csrc" libgsplat_mi355x.so          # that commit's own Makefile: whatever sources the library has there
echo "built exp/parent_tree from $(git -C "$root" rev-parse --short "$rev")"
