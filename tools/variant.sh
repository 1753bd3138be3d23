#!/bin/bash
# tools/variant.sh NAME "STEM ..." "EXTRA FLAGS" [COMMAND...]   (COMMAND: on the GPU box)
# A/B builds that leave the repo's own build alone: the objects of blur_algorithms_amd/csrc/build are COPIED to variants/NAME/, the listed
# objects (fx_conv_11, ff_u16_conv_7, engine, bx_box ...; a trailing .hip is accepted) are rebuilt there by the csrc Makefile with its own
# flags for them and the extra flags after, variants/NAME/libblur_amd.so is linked, and COMMAND runs with BLUR_AMD_LIB pointing at it
# (blur_algorithms_amd/_lib.py).  variants/ is git-ignored.
set -e
ROOT=${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}
NAME=$1; STEMS=$2; EXTRA=$3; shift 3
SRC=$ROOT/blur_algorithms_amd/csrc
OUT=$ROOT/variants/$NAME
mkdir -p "$OUT"
cp -p "$SRC"/build/*.o "$OUT"/
OBJS=""
for s in $STEMS; do OBJS="$OBJS $OUT/${s%.hip}.o"; done
rm -f $OBJS
make -C "$SRC" -j8 BUILD="$OUT" EXTRA="$EXTRA" $OBJS
make -C "$SRC" BUILD="$OUT" OUT="$OUT/libblur_amd.so"
echo "=== variant $NAME ($STEMS: $EXTRA)"
if [ $# -gt 0 ]; then (cd "$ROOT" && BLUR_AMD_LIB="$OUT/libblur_amd.so" "$@"); fi
