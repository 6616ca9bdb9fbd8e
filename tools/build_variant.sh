# builds stm32f4_sdr_gps_amd/lib/libgpsx_b.so -- a LAB build (-DGPSX_LAB: the only kind that may carry variants of the kernels)
# -- from the matrix-core grid sources of the working tree (k_acq_mx.hip, k_acq_mx_byte.hip, k_acq_mxw.hip over gpsx_mx_parts.hpp;
# -DMX_VARIANT_B is defined for an #ifdef'd alternative, if a source carries one) for same-box A/B timings -- boxes differ by +-3 %:
#   git stash; bash tools/build_variant.sh; git stash pop; make -C stm32f4_sdr_gps_amd/csrc      # B = HEAD, A = working tree
#   bash tools/gpu_validate.sh ab   (on the GPU box: alternates A and B through $GPSX_LIB of tools/bench_grid_kernel.py)
# VARIANT_DEFS: the variant's own -D flags (default none)
set -e
cd "$(dirname "$0")/../stm32f4_sdr_gps_amd/csrc"
F="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -fhip-fp32-correctly-rounded-divide-sqrt -ffp-contract=off -fno-fast-math -Wno-unused-function -DGPSX_LAB"
DEFS="${VARIANT_DEFS:-}"
MX="k_acq_mx k_acq_mx_byte k_acq_mxw"   # all three as the variant: an object left out here would be missing from the link
MX_B=""
for src in $MX; do
  /opt/rocm/bin/hipcc $F -fno-slp-vectorize -DMX_VARIANT_B $DEFS -c $src.hip -o ../build/${src}_b.o
  MX_B="$MX_B ../build/${src}_b.o"
done
/opt/rocm/bin/hipcc $F $DEFS -c gpsx_api.hip -o ../build/gpsx_api_b.o
OBJS=$(ls ../build/*.o | grep -v -E "/(k_acq_mx|k_acq_mx_byte|k_acq_mxw|gpsx_api)\.o$" | grep -v _b.o | grep -v _lab.o)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../lib/libgpsx_b.so $OBJS $MX_B ../build/gpsx_api_b.o -Wl,-rpath,/opt/rocm/lib -Wl,--no-undefined -ldl
echo built ../lib/libgpsx_b.so
