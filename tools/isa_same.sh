#!/bin/bash
# is the gfx950 code of one source file the same as at an earlier commit?  (device-side compile to assembly, twice, ~1 min; no GPU)
#   tools/isa_same.sh net_gated.hip [rev]      rev defaults to HEAD~1
# The file is compiled once from rev (its own include/ and csrc/, in a temp dir) and once from the working tree.  Per function
# (kernels and the device functions that stay calls) the text is compared without comments, directives (the __hip_cuid_ symbol is
# one) and the function's number in local labels; registers and scratch are tools/kres.sh's.  Under a function that DIFFERS: the
# mnemonics whose instruction count changed, old -> new, the floating-point ones on a line of their own.
set -euo pipefail
cd "$(dirname "$0")/.."
src=$1 rev=${2:-HEAD~1}
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
mkdir -p "$tmp/old" "$tmp/f_old" "$tmp/f_new"
git archive "$rev" include golds-rl-gym_amd/csrc | tar -x -C "$tmp/old"

asm() {     # $1 = root of a tree, $2 = output .s
    (cd "$1/golds-rl-gym_amd" && /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -I../include -I/opt/rocm/include \
        --cuda-device-only -w -S "csrc/$src" -o "$2")
}
functions() {     # $1 = .s, $2 = directory: one file per function, named by its symbol
    awk -v d="$2" '
        /^\t\.type\t.*,@function/ { split($2, a, ","); f = d "/" a[1]; printf "" > f; next }
        /^\.Lfunc_end/ { f = ""; next }
        f == "" || /^[ \t]*;/ || /^[A-Za-z_]/ { next }
        /^[ \t]*\./ && !/^\.LBB/ { next }
        { sub(/[ \t]*;.*$/, ""); gsub(/\.LBB[0-9]+_/, ".LBB_"); print > f }' "$1"
}
asm "$tmp/old" "$tmp/old.s"
asm . "$tmp/new.s"
functions "$tmp/old.s" "$tmp/f_old"
functions "$tmp/new.s" "$tmp/f_new"
name() { (c++filt "$1" 2>/dev/null || echo "$1") | sed 's/^void //; s/grl:://g; s/(.*//' | cut -c1-90; }
counts() { awk '!/:$/ { print $1 }' "$1" | sed -E "$2" | sort | uniq -c | awk '{ print $2, $1 }'; }     # instructions per mnemonic, labels left out
changed() { join -a1 -a2 -e0 -o 0,1.2,2.2 <(counts "$1" "$3") <(counts "$2" "$3") | awk '$2 != $3'; }     # mnemonic, count in $1, count in $2
fp='(_f64|_f32)(_e32|_e64|_dpp|_sdwa)?$|^v_rcp|^v_rsq|^v_sqrt|^v_div_|^v_fma'
bare='s/_(e32|e64|dpp|sdwa)$//'
for f in "$tmp"/f_new/*; do
    s=$(basename "$f")
    if [ ! -f "$tmp/f_old/$s" ]; then echo "new        $(name "$s")"
    elif cmp -s "$f" "$tmp/f_old/$s"; then echo "identical  $(name "$s")  ($(wc -l < "$f") lines)"
    else
        echo "DIFFERS    $(name "$s")  ($(diff "$tmp/f_old/$s" "$f" | grep -c '^[<>]' || true) of $(wc -l < "$f") lines)"
        # which mnemonics changed their count, old -> new; the floating-point ones apart: they are the arithmetic
        changed "$tmp/f_old/$s" "$f" '' | awk -v fp="$fp" '$1 !~ fp' > "$tmp/int"
        changed "$tmp/f_old/$s" "$f" '' | awk -v fp="$fp" '$1 ~ fp' > "$tmp/enc"
        changed "$tmp/f_old/$s" "$f" "$bare" | awk -v fp="$fp" '$1 ~ fp' > "$tmp/fp"
        echo "           counts: $(awk '{ printf "%s %s->%s  ", $1, $2, $3 }' "$tmp/int")"
        echo "           floating-point counts, the encoding's suffix left out: $(awk '{ printf "%s %s->%s  ", $1, $2, $3 } END { if (!NR) printf "none differs" }' "$tmp/fp")"
        [ -s "$tmp/enc" ] && echo "           floating-point encodings: $(awk '{ printf "%s %s->%s  ", $1, $2, $3 }' "$tmp/enc")"
    fi
done
for f in "$tmp"/f_old/*; do
    s=$(basename "$f")
    [ -f "$tmp/f_new/$s" ] || echo "gone       $(name "$s")"
done
