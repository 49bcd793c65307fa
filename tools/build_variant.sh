#!/bin/bash
# Build the bf16 library with extra compile flags into abvar_<name>/ (git-ignored; travels to the
# GPU box for same-box A/Bs:  STF_LIB=$GRAFT_REPO_ROOT/abvar_<name>/libstfunet_hip.so).
#   bash tools/build_variant.sh <name> "<extra hipcc flags>"
set -e
name=$1; flags=$2
root=$(cd "$(dirname "$0")/.." && pwd)
tmp=$(mktemp -d /tmp/stfvar.XXXX)
# the same layout as the repository, so the sources' relative includes and the Makefile's paths hold
mkdir -p "$tmp/stf-unet_amd/csrc" "$tmp/stf-unet_amd/stfunet" "$tmp/include" "$root/abvar_$name"
cp "$root"/stf-unet_amd/csrc/*.hip "$root"/stf-unet_amd/csrc/*.h "$root"/stf-unet_amd/csrc/Makefile "$tmp/stf-unet_amd/csrc/"
cp "$root/include/stfunet.h" "$tmp/include/"
make -C "$tmp/stf-unet_amd/csrc" -j8 "CXXFLAGS=--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -Wno-unused-variable $flags" ../stfunet/libstfunet_hip.so > "$tmp/build.log" 2>&1 || { tail -20 "$tmp/build.log"; exit 1; }
cp "$tmp/stf-unet_amd/stfunet/libstfunet_hip.so" "$root/abvar_$name/"
rm -rf "$tmp"
echo "built abvar_$name/libstfunet_hip.so ($flags)"
