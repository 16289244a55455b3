#!/bin/bash
# Build a library variant for same-box A/Bs:  tools/build_variant.sh <name> <file.hip>[,<file2.hip>...] [-Dmacro ...]
# -> build/var/liblfi_<name>.so = the tree's objects with the named files recompiled under the extra flags (picked with LFI_LIB_PATH).
# The source list and each file's flags are the Makefile's own (its print-srcs / print-flags targets).
set -eu
NAME=$1; SRCS=$2; shift 2
ROOT=$(cd "$(dirname "$0")/.." && pwd)
CSRC=$ROOT/lets_face_it_amd/csrc
make -C $CSRC -j4 > /dev/null
mkdir -p $ROOT/build/var
for SRC in ${SRCS//,/ }; do
  FLAGS=$(make -s -C $CSRC print-flags SRC=$SRC)
  # (LFI_SLP=1: with the SLP vectoriser, which the Makefile switches off for the encoder's units - the determinism chase of round 5)
  [ -n "${LFI_SLP:-}" ] && FLAGS=${FLAGS//-fno-slp-vectorize/}
  hipcc $FLAGS "$@" -c $CSRC/$SRC -o $ROOT/build/var/${NAME}_${SRC%.hip}.o
done
OBJS=""
for SRC in $(make -s -C $CSRC print-srcs); do
  case ",$SRCS," in
    *",$SRC,"*) OBJS="$OBJS $ROOT/build/var/${NAME}_${SRC%.hip}.o" ;;
    *) OBJS="$OBJS $ROOT/build/csrc/${SRC%.hip}.o" ;;
  esac
done
hipcc --offload-arch=gfx950 -shared -fPIC -o $ROOT/build/var/liblfi_$NAME.so $OBJS
echo "built build/var/liblfi_$NAME.so"
