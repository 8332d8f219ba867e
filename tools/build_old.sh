#!/bin/bash
# abl/<name>.so: the current library with one source file as of commit <rev> (dev tool for
# interleaved A/B via TT2_LIB).   tools/build_old.sh <name> <rev> <csrc file, e.g. batchnorm.hip>
# The file must exist under the same name, with the same entry points, in both commits: a
# revision from before gemm.hip was split into gemm_*.hip cannot be mixed in for the GEMM (its
# gemm.hip defines what the gemm_*.o objects define too; the link reports duplicate symbols), and
# likewise a revision from before attention.hip was split into attention_*.hip for the attention,
# or from before norm.hip and misc.hip were split (layernorm, batchnorm, reduce, embed, loss,
# optim, repack, comm_standin) for those.
# For that A/B build the old commit's whole library in a worktree.
set -euo pipefail
NAME=$1; REV=$2; FILE=$3
ROOT=$(cd "$(dirname "$0")/.." && pwd)
P=$ROOT/transformer-tacotron2_amd
python "$P/build_lib.py" > /dev/null
TMP=$(mktemp -d)
git -C "$ROOT" show "$REV:transformer-tacotron2_amd/csrc/$FILE" > "$P/csrc/_old_$FILE"
# the file's per-file flags from build_lib.py (attention*.hip: MFMA results in arch VGPRs), so the
# A/B differs in the source only
EXTRA=$(cd "$P" && python -c "import build_lib; print(' '.join(build_lib.extra_flags('$FILE')))")
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -I"$ROOT/include" -I"$P/csrc" -Wno-unused-result \
  $EXTRA -c "$P/csrc/_old_$FILE" -o "$TMP/old.o" || { rm -f "$P/csrc/_old_$FILE"; exit 1; }
rm -f "$P/csrc/_old_$FILE"
mkdir -p "$ROOT/abl"
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$ROOT/abl/$NAME.so" $(ls "$P"/build/*.o | grep -v "/$FILE.o") "$TMP/old.o"
rm -rf "$TMP"
echo "abl/$NAME.so"
