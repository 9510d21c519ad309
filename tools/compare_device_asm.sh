#!/bin/bash
# Is the gfx950 device code of every build.SOURCES file the same as at a git revision (no GPU needed)?
#   tools/compare_device_asm.sh [REV=HEAD] [JOBS=8]
# Each tree in turn (REV's, then the working tree's csrc/ + include/) is unpacked into the SAME temporary directory -- hipcc
# derives a symbol of every compilation unit from the file's path and the command line -- and each file is compiled from inside
# csrc/ with the flags of occdepth_amd/build.py plus --cuda-device-only -S.  The two .s files are compared with cmp.
# Prints one line per file; exit status 0 = all identical.
set -u
rev=${1:-HEAD}; jobs=${2:-8}
root=$(git -C "$(dirname "$(readlink -f "$0")")" rev-parse --show-toplevel) || exit 2
hipcc=$(command -v hipcc || echo /opt/rocm/bin/hipcc)
read -r arch flags sources < <(cd "$root" && python3 -c "
from occdepth_amd import build
print(build.ARCH, ','.join(build.FLAGS), ' '.join(build.SOURCES))") || exit 2
tmp=$(mktemp -d) || exit 2
trap 'rm -rf "$tmp"' EXIT
for side in base new; do
  mkdir -p "$tmp/tree" "$tmp/$side"
  if [ $side = base ]; then git -C "$root" archive "$rev" occdepth_amd/csrc include; else tar -c -C "$root" occdepth_amd/csrc include; fi \
    | tar -x -C "$tmp/tree" || exit 2
  (cd "$tmp/tree/occdepth_amd/csrc" && printf '%s\n' $sources | xargs -P "$jobs" -I{} \
     "$hipcc" --offload-arch="$arch" ${flags//,/ } -x hip --cuda-device-only -S {} -o {}.s 2>"$tmp/$side/log")
  mv "$tmp/tree/occdepth_amd/csrc/"*.s "$tmp/$side/" 2>/dev/null
  rm -rf "$tmp/tree"
done
bad=0
for s in $sources; do
  if [ -s "$tmp/base/$s.s" ] && cmp -s "$tmp/base/$s.s" "$tmp/new/$s.s"; then echo "identical  $s"; else echo "DIFFERS    $s"; bad=1; fi
done
[ $bad = 0 ] || grep -h "error" "$tmp/base/log" "$tmp/new/log" | head -20
exit $bad
