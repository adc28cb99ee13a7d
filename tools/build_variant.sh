#!/bin/bash
# Build a variant of libomr_gpu.so into tfhe-omr_amd/build/var_<name>.so (run on the CPU;
# tools/bench_variants.sh times every var_*.so on the GPU box).
#   tools/build_variant.sh <name> [--patch FILE]... [-DMACRO=VALUE ...]
# The sources are copied to a scratch tree under tfhe-omr_amd/build/, the patches (unified diffs
# against the repository root, e.g. the timing-only ablations of tools/variants/) are applied
# there, and the project's own Makefile builds it with the -D flags passed as EXTRA.
set -e
name=$1; shift
patches=()
extra=()
while [ $# -gt 0 ]; do
  case $1 in
    --patch) patches+=("$(realpath "$2")"); shift 2 ;;
    *) extra+=("$1"); shift ;;
  esac
done
root=$(cd "$(dirname "$0")/.." && pwd)
tree=$root/tfhe-omr_amd/build/var_${name}_src
rm -rf "$tree"
mkdir -p "$tree"
tar -C "$root" --exclude=tfhe-omr_amd/build --exclude='*.so' -cf - tfhe-omr_amd include | tar -C "$tree" -xf -
for p in "${patches[@]}"; do
  if ! patch -d "$tree" -p1 --forward --fuzz=0 < "$p"; then
    echo "build_variant: $p does not apply to the current sources" >&2
    exit 1
  fi
done
make -C "$tree/tfhe-omr_amd" -j4 EXTRA="${extra[*]}"
cp "$tree/tfhe-omr_amd/libomr_gpu.so" "$root/tfhe-omr_amd/build/var_$name.so"
echo "built tfhe-omr_amd/build/var_$name.so (${patches[*]} ${extra[*]})"
