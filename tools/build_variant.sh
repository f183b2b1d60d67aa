#!/bin/bash
# build_variant.sh NAME "EXTRA HIPCC FLAGS" -- an alternative build of libofdmrx.so for A/B runs
# (MODEM_AMD_LIB=modem_amd/lib/variants/libofdmrx_NAME.so).  In the environment, PERFILE_<stem>="flags" adds flags to one file and
# SRC_<stem>=path (from the repository root) replaces one source file
# (e.g. SRC_k_polar=tools/experiments/variants/k_polar_level9_in_registers.hip).
# The files and their flags are those of modem_amd/csrc/Makefile: this runs it with another object directory (under /tmp) and
# another name for the library; only the .so lands in-tree (git-ignored).
set -e
NAME=$1; FLAGS=$2
R=$(cd "$(dirname "$0")/.." && pwd)
for v in ${!SRC_@}; do export "$v=$R/${!v}"; done
make -B -j16 -C "$R/modem_amd/csrc" lib O="/tmp/variant_$NAME" LIB="../lib/variants/libofdmrx_$NAME.so" EXTRA="$FLAGS" > /dev/null
echo "built modem_amd/lib/variants/libofdmrx_$NAME.so"
