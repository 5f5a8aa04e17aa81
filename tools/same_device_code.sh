#!/bin/bash
# Here (no GPU): is the device code of the working tree the same as that of git revision REV (default HEAD)?  Each .hip file of the
# library is compiled to gfx950 assembly at both, with the Makefile's FLAGS, and the two compared without the lines that name the
# per-compilation __hip_cuid_ symbol.  The first question of a kernel change that is meant to change nothing: an empty diff covers
# behaviour and speed of every kernel at once.     bash tools/same_device_code.sh [REV [EXTRA flags]]
set -u
R=$(cd "$(dirname "$0")/.." && pwd); C=ken-burns-effect_amd/csrc
REV=${1:-HEAD}; EXTRA=${2:-}
T=$(mktemp -d); trap 'rm -rf "$T"' EXIT
mkdir -p $T/rev $T/out && git -C $R archive $REV $C include | tar -x -C $T/rev || exit 2
HIPCC=${HIPCC:-$(command -v hipcc || echo /opt/rocm/bin/hipcc)}
FLAGS=$(sed -n "s/^FLAGS *?= *//p" $R/$C/Makefile | sed "s/ -shared//")
asm_of() { ( cd $1/$C && $HIPCC --offload-arch=gfx950 $FLAGS -Wno-unused-command-line-argument $EXTRA --cuda-device-only -S $2.hip -o - ) | grep -v __hip_cuid_ > $3; }
fail=0
for f in $R/$C/*.hip; do
  k=$(basename $f .hip)
  asm_of $T/rev $k $T/out/$k.rev.s & asm_of $R $k $T/out/$k.tree.s & wait
  if [ -s $T/out/$k.tree.s ] && cmp -s $T/out/$k.rev.s $T/out/$k.tree.s; then echo "$k.hip: identical ($(wc -l < $T/out/$k.tree.s) lines of assembly)"
  else echo "$k.hip: DIFFERS"; diff $T/out/$k.rev.s $T/out/$k.tree.s | head -20; fail=1; fi
done
exit $fail
