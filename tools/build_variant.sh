#!/bin/bash
# Build an experimental libfrequensee.so into tools/tmp/<name>/ (git-ignored; travels to the GPU box):
#   bash tools/build_variant.sh n1 "-DFS_CHILD_ORDER=1"
# then on the GPU box: bash tools/ab_builds.sh n1 ...
# Everything goes through the Makefile, which owns the file lists.  Diagnostic builds whose device-side debug symbols are
# shared by all kernels (-DFS_WAVE_TIMELINE, -DFS_TRAV_STATS) take its `onefile` target: fs_kernels_all.hip in place of the
# four units it includes.  In that unit the narrow fused frame kernel walks NodeQ4 records, bound by its own launcher —
# correct, but not the product's record format (the 48-byte node view): such a build is for counting and timelines, not
# for rates.
set -e
name=$1; shift
mkdir -p tools/tmp/$name
flags="$*"
target=lib
if [[ "$flags" == *FS_WAVE_TIMELINE* || "$flags" == *FS_TRAV_STATS* ]]; then target=onefile; fi
make -s -C audio-pathtracer_amd/csrc -j8 $target OBJ=build_$name OUT=../../tools/tmp/$name EXTRA="$flags"
echo built tools/tmp/$name
