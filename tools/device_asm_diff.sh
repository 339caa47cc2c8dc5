#!/bin/sh
# Device-code gate for host-side / helper refactors: compile every csrc/*.hip of two trees to gfx950 device assembly, with the
# Makefile's flags and again with -DMG_AB_BUILD, and compare.  Lines naming __hip_cuid_ differ between any two builds and are
# dropped; everything else (instructions, kernel descriptors, symbol names) must be byte-identical.  Runs the compiler only.
#   tools/device_asm_diff.sh <tree A> <tree B> [file.hip ...]      exit 0 = identical
set -u
A=$(cd "$1" && pwd) && B=$(cd "$2" && pwd) || exit 2
shift 2
OUT=${OUT:-$(mktemp -d)}
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -S --cuda-device-only"
[ $# -gt 0 ] || set -- $(cd "$B/moviigen1.1_amd/csrc" && ls *.hip)
bad=0
for f in "$@"; do
    for cfg in prod ab; do
        [ $cfg = ab ] && D=-DMG_AB_BUILD || D=
        for t in A B; do
            eval "tree=\$$t"
            s=$OUT/$t.$cfg.${f%.hip}.s
            [ -s "$s" ] && [ -n "${REUSE:-}" ] && [ $t = A ] && continue      # REUSE=1 OUT=dir: keep tree A's assembly between runs
            (cd "$tree/moviigen1.1_amd/csrc" && ${HIPCC:-/opt/rocm/bin/hipcc} $FLAGS $D "$f" -o - 2>/dev/null | grep -v __hip_cuid_ > "$s") &
        done
        wait
        if [ -s "$OUT/A.$cfg.${f%.hip}.s" ] && cmp -s "$OUT/A.$cfg.${f%.hip}.s" "$OUT/B.$cfg.${f%.hip}.s"; then r=identical; else r=DIFFERENT; bad=1; fi
        echo "$f $cfg $r"
    done
done
exit $bad
