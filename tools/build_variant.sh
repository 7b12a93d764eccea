#!/bin/bash
# Diagnostic variant of the library with extra compile definitions (A/B measurements; never shipped):
#   tools/build_variant.sh <name> -DFOO=1 ...  ->  ab_libs/libitsd_hip_<name>.so (ab_libs/ travels to the
# GPU box with the snapshot; objects stay in build_diag/<name>/, which does not).
# build.py's build() compiles it, with the product's flags; --force recompiles every object, and a failed
# compile raises before the link, so no object of an earlier build reaches the variant.
set -e
cd "$(dirname "$0")/.."
PKG=inference-time-scaling-for-diffusion-models-beyond-scaling-denoising-steps_amd
name=$1; shift
mkdir -p ab_libs
rm -f ab_libs/libitsd_hip_$name.so
python $PKG/build.py --force --obj-dir build_diag/$name --out ab_libs/libitsd_hip_$name.so "$@" > /dev/null
echo ab_libs/libitsd_hip_$name.so
