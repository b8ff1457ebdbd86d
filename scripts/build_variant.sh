#!/bin/bash
# Build the engine library of git revision REV (WT: the working tree) into
# foundationdb_amd/variants/libfdbcs_<NAME>.so (same-box A/B of kernel changes: bench.py loads it with
# FDBCS_LIB=...), with EXTRA compiler flags (e.g. EXTRA=-DFDBCS_RUN_PROBES=7).  The sources are the
# working tree's list (foundationdb_amd/build.py); a file REV does not have becomes empty, so a
# revision from before a source was added still builds.  Usage:
#   [EXTRA=...] bash scripts/build_variant.sh <rev> <name>
set -eu
cd "$(dirname "$0")/.."
REV=$1; NAME=$2
TMP=$(mktemp -d)
C=foundationdb_amd/csrc
mkdir -p $TMP/$C $TMP/include foundationdb_amd/variants
SOURCES=$(python3 -c "from foundationdb_amd import build; print(' '.join(build.SOURCES))")
FILES=$(python3 -c "from foundationdb_amd import build as b; print(' '.join(['$C/' + f for f in b.SOURCES + b.HEADERS] + [b.PUBLIC_HEADER]))")
for f in $FILES; do
  if [ "$REV" = "WT" ]; then cp $f $TMP/$f; else git show $REV:$f > $TMP/$f 2>/dev/null || : > $TMP/$f; fi
done
H=/opt/rocm/bin/hipcc
OBJS=
for f in $SOURCES; do
  case $f in
    *.hip) $H -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function -mllvm -disable-promote-alloca-to-lds \
             ${EXTRA:-} -c $TMP/$C/$f -o $TMP/$f.o ;;
    *) $H -O3 -std=c++17 -fPIC -Wall ${EXTRA:-} -c $TMP/$C/$f -o $TMP/$f.o ;;
  esac
  OBJS="$OBJS $TMP/$f.o"
done
$H --offload-arch=gfx950 -shared -fPIC -o foundationdb_amd/variants/libfdbcs_$NAME.so $OBJS
rm -rf $TMP
echo foundationdb_amd/variants/libfdbcs_$NAME.so
