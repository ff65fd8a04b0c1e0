#!/bin/bash
# builds scripts/ubench/<name> from scripts/ubench/<src>.hip (gfx950 .s kept under /tmp/lab for inspection)
#   build_lab.sh [src [out [extra hipcc flags...]]]
SRC=${1:-gemm_lab}; OUT=${2:-$SRC}; shift; shift
R=$(cd "$(dirname "$0")/../.." && pwd)
mkdir -p /tmp/lab/$OUT && cd /tmp/lab/$OUT && hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffast-math -fno-finite-math-only "$@" -I $R/videollama2_amd/csrc -I $R/scripts/ubench $R/scripts/ubench/$SRC.hip -o $R/scripts/ubench/$OUT -save-temps 2>&1 | grep -v "warning: argument unused\|implicit conversion\|float u1\|~$\|warning generated" | head -30
