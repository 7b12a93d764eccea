#!/bin/bash
# Diagnostic build with in-kernel phase stamps (conv.hip ITSD_STAMPS) and the compile-time ablations
# (ITSD_DIAG): ab_libs/libitsd_hip_stamps.so (ab_libs/ travels to the GPU box; build_diag/ does not).
# Never shipped; tools/stamps.py and tools/census.py --lib load it explicitly.
# build.py's build() compiles it, with the product's flags.
set -e
cd "$(dirname "$0")/.."
PKG=inference-time-scaling-for-diffusion-models-beyond-scaling-denoising-steps_amd
OUT=${1:-ab_libs}
mkdir -p "$OUT"
python $PKG/build.py --force --obj-dir build_diag --out "$OUT/libitsd_hip_stamps.so" -DITSD_STAMPS -DITSD_DIAG > /dev/null
echo $OUT/libitsd_hip_stamps.so
