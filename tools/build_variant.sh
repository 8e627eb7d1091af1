#!/bin/bash
# Build a variant of the kernel library for A/B runs (U3D_LIB_PATH=<out> python bench.py ...):
#   tools/build_variant.sh <out.so> <file.hip[,file2.hip...]> <extra hipcc flags...>
#   e.g.  tools/build_variant.sh tools/bin/libu3d_ald40.so spconv.hip -DU3D_GMM_ALD40
# The named sources are recompiled with the extra flags, every other object comes from the in-tree build.  The flags of each
# source and the object list are csrc/build.py's (command(), SOURCES): nothing about the compilation is repeated here.
set -e
R=$(cd "$(dirname "$0")/.." && pwd); OUT=$(realpath -m "$1"); shift
cd "$R" && python -m unidet3d_amd.csrc.build --variant "$OUT" "$@"
ls -la "$OUT"
