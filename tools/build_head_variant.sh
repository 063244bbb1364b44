# Build the committed (HEAD or $2) render kernel as raytracinginaweekend_amd/librtw_$1.so for A/B runs
# (extra compiler flags, e.g. -DRTW_QUEUES=32, from $RTW_VARIANT_FLAGS).  rtw_device.hip and rtw_parts.hip, which
# share the partition records' launchers, come from that commit with its own include/; the other objects are this
# tree's build.
set -e
cd "$(dirname "$0")/../raytracinginaweekend_amd/csrc"
rev=${2:-HEAD}
src=$(mktemp -d)
trap 'rm -rf "$src"' EXIT
git -C ../.. archive "$rev" include raytracinginaweekend_amd/csrc | tar -x -C "$src"
flags="-O3 -fPIC -std=c++17 -ffp-contract=off -fno-fast-math --offload-arch=gfx950 -fhip-fp32-correctly-rounded-divide-sqrt -munsafe-fp-atomics -fno-slp-vectorize"
/opt/rocm/bin/hipcc $flags $RTW_VARIANT_FLAGS -c -x hip "$src/raytracinginaweekend_amd/csrc/rtw_device.hip" -o build/ab_tmp.o
/opt/rocm/bin/hipcc $flags -c -x hip "$src/raytracinginaweekend_amd/csrc/rtw_parts.hip" -o build/ab_parts.o
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../librtw_$1.so build/ab_tmp.o build/ab_parts.o build/scene_builder.o \
  build/demo_worlds.o build/rtw_common.o build/rtw_sort.o build/rtw_sah.o build/rtw_multi.o build/rtw_denoise.o build/rtw_check.o
