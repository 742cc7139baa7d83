#!/bin/bash
# Are the MfccKernel<...> instantiations of the working tree the machine code of another revision's?  Needs no GPU.
#   usage: profiles/micro/mfcc_isa_diff.sh [base revision, default HEAD]
# Compiles feat_kernels.hip of both trees to gfx950 assembly with the Makefile's flags, cuts every MfccKernel function out of the
# two listings (label to end of function, plus its .amdhsa_ kernel descriptor: registers, LDS, scratch) and diffs them.  Exit status 0 and
# "identical" when nothing differs.
set -euo pipefail
BASE="${1:-HEAD}"
ROOT="$(cd "$(dirname "$0")/../.." && pwd)"
TMP="$(mktemp -d)"
trap 'rm -rf "$TMP"' EXIT
mkdir -p "$TMP/base" "$TMP/new"
git -C "$ROOT" archive "$BASE" rhasspy_speech_amd/csrc include | tar -x -C "$TMP/base"
cp -r "$ROOT/rhasspy_speech_amd" "$ROOT/include" "$TMP/new/"
FL="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-function -Wno-unused-result -ffp-contract=off -fno-slp-vectorize -fno-vectorize"
for v in base new; do
  (cd "$TMP/$v/rhasspy_speech_amd/csrc" && hipcc $FL --offload-device-only -S -o "$TMP/$v.s" feat_kernels.hip)
  # function bodies and kernel descriptors of the MfccKernel instantiations, in name order; compiler-numbered local labels differ
  # between two translation units that hold different sets of functions, so they are renumbered per function and the comments dropped
  awk '
    /^_ZN2rs10MfccKernel[A-Za-z0-9_]*:/ { name = $1; keep = 1; n = 0; delete lab }
    /^\.amdhsa_kernel _ZN2rs10MfccKernel/ { name = $2 ":desc"; keep = 2 }
    keep == 1 && /^\.Lfunc_end/ { keep = 0 }
    keep {
      line = $0
      sub(/[ \t]*;.*$/, "", line)      # (comments carry the number of the function in its translation unit)
      if (line == "") next
      while (match(line, /\.LBB[0-9]+_[0-9]+/)) {
        l = substr(line, RSTART, RLENGTH)
        if (!(l in lab)) lab[l] = "L" n++
        line = substr(line, 1, RSTART - 1) lab[l] substr(line, RSTART + RLENGTH)
      }
      print name "\t" line
    }
    keep == 2 && /^\.end_amdhsa_kernel/ { keep = 0 }
  ' "$TMP/$v.s" | sort -s -t "$(printf '\t')" -k1,1 > "$TMP/$v.mfcc"
done
echo "MfccKernel instantiations: $(cut -f1 "$TMP/new.mfcc" | grep -v ':desc' | sort -u | wc -l), $(grep -vc ':desc' "$TMP/new.mfcc") lines of code"
if diff "$TMP/base.mfcc" "$TMP/new.mfcc" > "$TMP/diff.txt"; then echo "identical"; else head -80 "$TMP/diff.txt"; echo "DIFFERENT: $(wc -l < "$TMP/diff.txt") diff lines"; exit 1; fi
