#!/bin/bash
# A/B variant of the library: scripts/ab_build.sh <name> "<extra -D flags>" [all | <tu>]  -> ab/libpq_<name>.so
# The experiment switches of csrc/experiments.h need -DPQ_EXPERIMENTS as well (a product build never sets it).
# Default: only suite.hip (the job-grid kernels bench.py times) is rebuilt with the flags; `all` rebuilds every TU.  The other
# objects are the product build's (run `make -C polars_quant_amd/csrc` first); the TU list is the Makefile's.
# `ab/` is git-ignored; delete it after use (it travels with every push of the tree to the GPU box).
set -e
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
cd "$ROOT/polars_quant_amd/csrc"
TUS=$(sed -n 's/^SRCS *:= *//p' Makefile | sed 's/\.hip//g')
TMP=$(mktemp -d /tmp/ab_$1.XXXXXX)
mkdir -p "$ROOT/ab"
F="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -Wall -Wno-unused-function -Wno-bitwise-instead-of-logical -Wno-parentheses"
if [ "$3" = all ]; then
  for f in $TUS; do mkdir -p "$TMP/$(dirname $f)"; /opt/rocm/bin/hipcc $F $2 -c $f.hip -o $TMP/$f.o & done; wait
  OBJS=""; for f in $TUS; do OBJS="$OBJS $TMP/$f.o"; done
else
  TU=${3:-suite}   # the one TU to rebuild with the flags (default: suite.hip)
  mkdir -p "$TMP/$(dirname $TU)"
  /opt/rocm/bin/hipcc $F $2 -c $TU.hip -o $TMP/$TU.o
  OBJS=""; for f in $TUS; do if [ $f = $TU ]; then OBJS="$OBJS $TMP/$TU.o"; else OBJS="$OBJS $f.o"; fi; done
fi
/opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -o "$ROOT/ab/libpq_$1.so" $OBJS -ldl
rm -rf "$TMP"
