#!/bin/bash
# Build abl/<name>.so: the current objects with some sources recompiled under extra -D flags
# (dev tool for interleaved A/B via TT2_LIB).  Default: every GEMM unit (csrc/gemm*.hip) -- they
# share headers and knobs, and TT2_PHASE changes the probe record width for the probe state and
# every probed kernel alike, so they are recompiled together.  VAR_SRC names other sources
# (base names, space separated).
#   [VAR_SRC="layernorm batchnorm attention"] tools/build_variant.sh <name> -DFOO=1 ...
set -euo pipefail
NAME=$1; shift
ROOT=$(cd "$(dirname "$0")/.." && pwd)
PKG=$ROOT/transformer-tacotron2_amd
python "$PKG/build_lib.py" > /dev/null
mkdir -p "$ROOT/abl"
TMP=$(mktemp -d)
VARIED=()
if [ -n "${VAR_SRC:-}" ]; then
  for s in $VAR_SRC; do
    f="$PKG/csrc/$s.hip"; [ -f "$f" ] || f="$PKG/csrc/$s.cpp"
    [ -f "$f" ] || { echo "no source $s in csrc/" >&2; exit 2; }
    VARIED+=("$(basename "$f")")
  done
else
  for f in "$PKG"/csrc/gemm*.hip; do VARIED+=("$(basename "$f")"); done
fi
OBJS=()
PIDS=()
for f in "$PKG"/csrc/*.hip "$PKG"/csrc/*.cpp; do
  b=$(basename "$f")
  if [[ " ${VARIED[*]} " == *" $b "* ]]; then
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -I"$ROOT/include" -I"$PKG/csrc" \
      -Wno-unused-result "$@" -c "$f" -o "$TMP/$b.o" &
    PIDS+=($!)
    OBJS+=("$TMP/$b.o")
  else
    OBJS+=("$PKG/build/$b.o")
  fi
done
for p in "${PIDS[@]}"; do wait "$p"; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$ROOT/abl/$NAME.so" "${OBJS[@]}"
rm -rf "$TMP"
echo "abl/$NAME.so"
