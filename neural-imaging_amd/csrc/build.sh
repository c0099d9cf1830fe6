#!/bin/bash
# Build libnimg.so for gfx950 (MI355X) in-tree.  Usage: neural-imaging_amd/csrc/build.sh [make variables, e.g. EXTRA=-DX]
set -e
cd "$(dirname "$0")"
JOBS=${MAX_JOBS:-$(nproc)}          # nproc counts the whole host, not this job's share of it: at most 16 compilers at once
[ "$JOBS" -gt 16 ] && JOBS=16
make -j"$JOBS" "$@"
