// How do an MFMA stream and a VALU stream share one SIMD on gfx950?  k_acq_mx keeps two waves per SIMD: one issues the FP4
// MFMAs of a pass, the other the clip/square/root/search instructions of the previous pass.  This micro-benchmark times both
// streams (s_memtime, shader cycles), alone and together, for VALU streams of different instruction classes and different
// distances between dependent instructions.
// Build: hipcc --offload-arch=gfx950 -O3 issue_mix.hip -o issue_mix ; run on the GPU box.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <vector>

#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)

typedef unsigned int u32;
typedef unsigned long long u64;
typedef float v16f __attribute__((ext_vector_type(16)));
typedef int v8i __attribute__((ext_vector_type(8)));

constexpr int kMfmaPerIter = 32;    // 8 accumulators x 4

// VALU stream: kValuPerIter instructions per iteration over ILP independent registers (dependent distance = ILP)
// OP 0: v_mul_f32 (2-cycle class)  1: v_max_i32 (4-cycle class)  2: v_sqrt_f32  3: the epilogue's mix per hypothesis
template <int OP, int ILP, int kValuPerIter>
__device__ __forceinline__ void valu_iter(float (&x)[8], float c)
{
  float2 cp = make_float2(c, c);
  asm volatile("" : "+v"(cp));
#pragma unroll
  for (int i = 0; i < kValuPerIter; i++) {
    float &r = x[i % ILP];
    if (OP == 0)
      asm volatile("v_mul_f32 %0, %0, %1" : "+v"(r) : "v"(c));
    else if (OP == 1)
      asm volatile("v_max_i32 %0, %0, %1" : "+v"(r) : "v"(c));
    else if (OP == 2)
      asm volatile("v_sqrt_f32 %0, %0" : "+v"(r));
    else if (OP == 3)
      asm volatile("v_lshl_or_b32 %0, %0, 1, %1" : "+v"(r) : "v"(c));
    else if (OP == 4) {   // packed f32: two values per lane and instruction (register pairs x[0:1], x[2:3], ..)
      float2 &rp = reinterpret_cast<float2 *>(x)[(i % ILP) % 4];
      asm volatile("v_pk_mul_f32 %0, %0, %1" : "+v"(rp) : "v"(cp));
    } else if (OP == 5) {
      float2 &rp = reinterpret_cast<float2 *>(x)[(i % ILP) % 4];
      asm volatile("v_pk_fma_f32 %0, %0, %1, %1" : "+v"(rp) : "v"(cp));
    } else if (OP == 6) {
      float2 &rp = reinterpret_cast<float2 *>(x)[(i % ILP) % 4];
      asm volatile("v_pk_add_f32 %0, %0, %1" : "+v"(rp) : "v"(cp));
    } else if (OP == 7)
      asm volatile("v_mul_f32_e64 %0, %0, |%1| clamp" : "+v"(r) : "v"(c));
    else if (OP == 8)
      asm volatile("v_max3_u32 %0, %0, %1, %1" : "+v"(r) : "v"(c));
    else if (OP == 9)
      asm volatile("v_pk_add_u16 %0, %0, %1 clamp" : "+v"(r) : "v"(c));
    else if (OP == 10)
      asm volatile("v_perm_b32 %0, %0, %1, %1" : "+v"(r) : "v"(c));
    else if (OP == 11)
      asm volatile("v_or3_b32 %0, %0, %1, %1" : "+v"(r) : "v"(c));
    else if (OP == 12)
      asm volatile("v_cvt_pkrtz_f16_f32 %0, %0, %1" : "+v"(r) : "v"(c));
    else if (OP == 13)
      asm volatile("v_pk_max_f16 %0, %0, %1" : "+v"(r) : "v"(c));
    else if (OP == 14)   // (distance >= 2: the dot instructions need a wait state before a dependent read)
      asm volatile("v_dot2_f32_f16 %0, %1, %1, %0" : "+v"(r) : "v"(c));
    else if (OP == 15)
      asm volatile("v_dot2c_f32_f16 %0, %1, %1" : "+v"(r) : "v"(c));
  }
}

// ---- the epilogue group of k_acq_mx<0> as a literal instruction sequence (OP 16..19) -----------------------------------------
// Eight hypotheses on eight register pairs (I in v64..71, Q in v72..79), two groups per loop iteration, the whole loop in one asm
// statement on fixed registers (all of them clobbered).  The inputs are small, so the radius test never fires; its branches are there.
//   OP 16  (a) the order the compiler gave the group-tested code: v_mul, v_mul, v_add per hypothesis, the test threaded through
//   OP 17  (b) phase order -- 16 clip-squares, 8 sums, the test, 8 roots, 8 fmas, 8 keys, the chains -- with test and branches
//   OP 18  (c) phase order without them (the trusted path)
//   OP 19  (d) as (c) with an s_nop 0 in front of each later phase (what an empty asm statement between the phases leaves)
#define G_MUL(d, s) "v_mul_f32_e64 v" #d ", v" #s ", |v" #s "| clamp\n"
#define G_ADD(d, a, b) "v_add_f32_e32 v" #d ", v" #a ", v" #b "\n"
#define G_SQRT(d) "v_sqrt_f32_e32 v" #d ", v" #d "\n"
#define G_FMA(d) "v_fmamk_f32 v" #d ", v" #d ", 0x46000002, v112\n"
#define G_KEY(d, s, code) "v_lshl_or_b32 v" #d ", v" #s ", 6, " #code "\n"
#define G_MAX3(d, a, b) "v_max3_u32 v" #d ", v" #d ", v" #a ", v" #b "\n"
#define G_ADD3(d, a, b) "v_add3_u32 v" #d ", v" #a ", v" #d ", v" #b "\n"
#define G_BRANCH "v_cmp_lt_u32_e32 vcc, s20, v113\ns_mov_b64 s[22:23], -1\ns_cbranch_vccnz 2f\ns_andn2_b64 vcc, exec, s[22:23]\ns_cbranch_vccnz 2f\n"
#define G_HYP(i, I, Q) G_MUL(88, I) G_MUL(89, Q) G_ADD(i, 89, 88)
#define G_TODAY                                                                                                                  \
  G_HYP(80, 64, 72) G_HYP(81, 65, 73) G_HYP(82, 66, 74) G_MUL(88, 67) G_MUL(89, 75) "v_max_u32_e32 v113, v80, v81\n"              \
  G_ADD(83, 89, 88) G_MAX3(113, 82, 83) G_HYP(84, 68, 76) G_HYP(85, 69, 77) G_MAX3(113, 84, 85) G_HYP(86, 70, 78)                 \
  G_HYP(87, 71, 79) G_MAX3(113, 86, 87) G_BRANCH                                                                                  \
  G_SQRT(80) G_SQRT(81) G_SQRT(82) G_SQRT(83) G_FMA(80) G_FMA(81) G_FMA(82) G_SQRT(84) G_SQRT(85) G_SQRT(86) G_SQRT(87)           \
  G_FMA(83) G_FMA(84) G_FMA(85) G_FMA(86) G_FMA(87) "2:\n"                                                                        \
  G_KEY(96, 80, 59) G_KEY(97, 84, 43) G_MAX3(104, 96, 97) G_KEY(96, 81, 58) G_KEY(97, 85, 42) G_MAX3(105, 96, 97)                 \
  G_KEY(96, 82, 57) G_KEY(97, 86, 41) G_MAX3(106, 96, 97) G_KEY(96, 83, 56) G_KEY(97, 87, 40)                                     \
  G_ADD3(108, 80, 84) G_ADD3(109, 81, 85) G_ADD3(110, 82, 86) G_MAX3(107, 96, 97) G_ADD3(111, 83, 87)
#define G_SQUARES                                                                                                                \
  G_MUL(80, 64) G_MUL(88, 72) G_MUL(81, 65) G_MUL(89, 73) G_MUL(82, 66) G_MUL(90, 74) G_MUL(83, 67) G_MUL(91, 75)                 \
  G_MUL(84, 68) G_MUL(92, 76) G_MUL(85, 69) G_MUL(93, 77) G_MUL(86, 70) G_MUL(94, 78) G_MUL(87, 71) G_MUL(95, 79)
#define G_SUMS G_ADD(80, 80, 88) G_ADD(81, 81, 89) G_ADD(82, 82, 90) G_ADD(83, 83, 91) G_ADD(84, 84, 92) G_ADD(85, 85, 93) G_ADD(86, 86, 94) G_ADD(87, 87, 95)
#define G_TEST "v_max_u32_e32 v113, v80, v81\n" G_MAX3(113, 82, 83) G_MAX3(113, 84, 85) G_MAX3(113, 86, 87) G_BRANCH
#define G_ROOTS G_SQRT(80) G_SQRT(81) G_SQRT(82) G_SQRT(83) G_SQRT(84) G_SQRT(85) G_SQRT(86) G_SQRT(87)
#define G_FMAS G_FMA(80) G_FMA(81) G_FMA(82) G_FMA(83) G_FMA(84) G_FMA(85) G_FMA(86) G_FMA(87)
#define G_KEYS G_KEY(96, 80, 59) G_KEY(97, 81, 58) G_KEY(98, 82, 57) G_KEY(99, 83, 56) G_KEY(100, 84, 43) G_KEY(101, 85, 42) G_KEY(102, 86, 41) G_KEY(103, 87, 40)
#define G_CHAINS G_MAX3(104, 96, 100) G_ADD3(108, 80, 84) G_MAX3(105, 97, 101) G_ADD3(109, 81, 85) G_MAX3(106, 98, 102) G_ADD3(110, 82, 86) G_MAX3(107, 99, 103) G_ADD3(111, 83, 87)
#define G_NOP "s_nop 0\n"
#define G_PHASED_TEST G_SQUARES G_SUMS G_TEST G_ROOTS G_FMAS "2:\n" G_KEYS G_CHAINS
#define G_PHASED G_SQUARES G_SUMS G_ROOTS G_FMAS G_KEYS G_CHAINS
#define G_PHASED_NOPS G_SQUARES G_NOP G_SUMS G_NOP G_ROOTS G_NOP G_FMAS G_NOP G_KEYS G_NOP G_CHAINS
constexpr int kGroupsPerIter = 2;
template <int ARM>
__device__ __forceinline__ float group_loop(int iters)
{
  u32 n = (u32)__builtin_amdgcn_readfirstlane(iters);
  float sink;
#define G_LOOP(BODY)                                                                                                               \
  asm volatile("v_mov_b32 v64, 0x3c23d70a\nv_mov_b32 v65, 0x3c343958\nv_mov_b32 v66, 0x3c449ba6\nv_mov_b32 v67, 0x3c54fdf4\n"      \
               "v_mov_b32 v68, 0x3c656042\nv_mov_b32 v69, 0x3c75c28f\nv_mov_b32 v70, 0x3c83126f\nv_mov_b32 v71, 0x3c8b4396\n"      \
               "v_mov_b32 v72, v71\nv_mov_b32 v73, v70\nv_mov_b32 v74, v69\nv_mov_b32 v75, v68\nv_mov_b32 v76, v67\n"               \
               "v_mov_b32 v77, v66\nv_mov_b32 v78, v65\nv_mov_b32 v79, v64\nv_mov_b32 v112, 0x4b000000\ns_mov_b32 s20, 0x3c7fffff\n" \
               "v_mov_b32 v104, 0\nv_mov_b32 v105, 0\nv_mov_b32 v106, 0\nv_mov_b32 v107, 0\n"                                       \
               "v_mov_b32 v108, 0\nv_mov_b32 v109, 0\nv_mov_b32 v110, 0\nv_mov_b32 v111, 0\n"                                       \
               "1:\n" BODY BODY "s_sub_u32 %1, %1, 1\ns_cmp_lg_u32 %1, 0\ns_cbranch_scc1 1b\n"                                      \
               "v_xor_b32 v104, v104, v105\nv_xor_b32 v106, v106, v107\nv_xor_b32 v108, v108, v109\nv_xor_b32 v110, v110, v111\n"   \
               "v_xor_b32 v104, v104, v106\nv_xor_b32 v108, v108, v110\nv_xor_b32 %0, v104, v108\n"                                 \
               : "=v"(sink), "+s"(n)                                                                                               \
               :                                                                                                                   \
               : "v64", "v65", "v66", "v67", "v68", "v69", "v70", "v71", "v72", "v73", "v74", "v75", "v76", "v77", "v78", "v79", "v80",  \
                 "v81", "v82", "v83", "v84", "v85", "v86", "v87", "v88", "v89", "v90", "v91", "v92", "v93", "v94", "v95", "v96", "v97",  \
                 "v98", "v99", "v100", "v101", "v102", "v103", "v104", "v105", "v106", "v107", "v108", "v109", "v110", "v111", "v112",   \
                 "v113", "s20", "s22", "s23", "vcc", "scc", "memory")
  if constexpr (ARM == 0)
    G_LOOP(G_TODAY);
  else if constexpr (ARM == 1)
    G_LOOP(G_PHASED_TEST);
  else if constexpr (ARM == 2)
    G_LOOP(G_PHASED);
  else
    G_LOOP(G_PHASED_NOPS);
#undef G_LOOP
  return sink;
}

template <int OP, int ILP, int VPI, bool WITH_MFMA, bool WITH_VALU>
__global__ __launch_bounds__(512, 1) void k_mix(u32 *out, int iters, float c)
{
  __shared__ u32 pad[30000];   // > 80 KB: one workgroup per CU
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  pad[tid] = tid;
  __syncthreads();
  const int role = wave >> 2;
  u64 t0 = 0, t1 = 0;
  float sink = 0.f;
  if (role == 0) {
    if (WITH_MFMA) {
      v16f acc[8];
      for (int a = 0; a < 8; a++)
        for (int r = 0; r < 16; r++)
          acc[a][r] = 0.f;
      v8i fa = {(int)pad[lane] * 0x11111111, 0x2a2a2a2a, 0x02a0020a, (int)pad[lane + 64], 0, 0, 0, 0};
      v8i fb = {0x2a2a2a2a, (int)pad[lane + 3] * 0x01010101, 0x02a0020a, 0x22222222, 0, 0, 0, 0};
      asm volatile("" : "+v"(fa), "+v"(fb));
      t0 = __builtin_amdgcn_s_memtime();
#pragma unroll 1
      for (int it = 0; it < iters; it++) {
#pragma unroll
        for (int k = 0; k < kMfmaPerIter; k++)
          acc[k & 7] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(fa, fb, acc[k & 7], 4, 4, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
      }
      asm volatile("s_nop 0" ::: "memory");
      for (int a = 0; a < 8; a++)
        for (int r = 0; r < 16; r++)
          sink += acc[a][r];
      asm volatile("" : "+v"(sink));
      t1 = __builtin_amdgcn_s_memtime();
    }
  } else {
    if (WITH_VALU) {
      float x[8];
      for (int i = 0; i < 8; i++)
        x[i] = 1.0f + 0.001f * (float)(lane + i);
      t0 = __builtin_amdgcn_s_memtime();
      if constexpr (OP >= 16) {
        x[0] = group_loop<OP - 16>(iters);
      } else {
#pragma unroll 1
        for (int it = 0; it < iters; it++)
          valu_iter<OP, ILP, VPI>(x, c);
      }
      for (int i = 0; i < 8; i++)
        sink += x[i];
      asm volatile("" : "+v"(sink));
      t1 = __builtin_amdgcn_s_memtime();
    }
  }
  if (lane == 0) {
    out[(blockIdx.x * 8 + wave) * 2] = (u32)(t1 - t0);
    out[(blockIdx.x * 8 + wave) * 2 + 1] = __float_as_uint(sink);
  }
}

template <int OP, int ILP, int VPI>
static int run(const char *name, int n_wg, int iters)
{
  u32 *d_out;
  CHECK(hipMalloc(&d_out, (size_t)n_wg * 16 * sizeof(u32)));
  std::vector<u32> h(n_wg * 16);
  auto mean = [&](int role, double per) {
    double s = 0;
    int cnt = 0;
    for (int b = 0; b < n_wg; b++)
      for (int w = 4 * role; w < 4 * role + 4; w++) {
        s += h[(b * 8 + w) * 2];
        cnt++;
      }
    return s / cnt / per;
  };
  printf("%-30s dep. distance %d, %d per MFMA:", name, ILP, VPI / kMfmaPerIter);
  for (int rep = 0; rep < 2; rep++) {
    hipLaunchKernelGGL((k_mix<OP, ILP, VPI, false, true>), dim3(n_wg), dim3(512), 0, 0, d_out, iters, 1.0f);
    CHECK(hipDeviceSynchronize());
  }
  CHECK(hipMemcpy(h.data(), d_out, h.size() * 4, hipMemcpyDeviceToHost));
  printf("  alone %5.2f cyc/VALU,", mean(1, (double)iters * VPI));
  hipLaunchKernelGGL((k_mix<OP, ILP, VPI, true, false>), dim3(n_wg), dim3(512), 0, 0, d_out, iters, 1.0f);
  CHECK(hipDeviceSynchronize());
  CHECK(hipMemcpy(h.data(), d_out, h.size() * 4, hipMemcpyDeviceToHost));
  printf(" %5.1f cyc/MFMA |", mean(0, (double)iters * kMfmaPerIter));
  hipLaunchKernelGGL((k_mix<OP, ILP, VPI, true, true>), dim3(n_wg), dim3(512), 0, 0, d_out, iters, 1.0f);
  CHECK(hipDeviceSynchronize());
  CHECK(hipMemcpy(h.data(), d_out, h.size() * 4, hipMemcpyDeviceToHost));
  const double m = mean(0, (double)iters * kMfmaPerIter), v = mean(1, (double)iters * VPI);
  printf(" together %5.2f cyc/VALU (stream %6.0f cyc/iter), %5.1f cyc/MFMA (stream %6.0f cyc/iter)", v, v * VPI, m, m * kMfmaPerIter);
  if (OP >= 16)
    printf(" | %6.1f cyc/group", v * VPI / kGroupsPerIter);
  printf("\n");
  CHECK(hipFree(d_out));
  return 0;
}

int main()
{
  setvbuf(stdout, nullptr, _IONBF, 0);
  hipDeviceProp_t prop;
  CHECK(hipGetDeviceProperties(&prop, 0));
  printf("device %s CUs=%d; one MFMA wave + one VALU wave per SIMD; an iteration = %d MFMAs | VPI VALU instructions\n", prop.gcnArchName,
         prop.multiProcessorCount, kMfmaPerIter);
  const int n_wg = 256, it = 200;
  run<0, 1, 192>("v_mul_f32 (2-cycle class)", n_wg, it);
  run<0, 2, 192>("v_mul_f32 (2-cycle class)", n_wg, it);
  run<0, 4, 192>("v_mul_f32 (2-cycle class)", n_wg, it);
  run<0, 8, 192>("v_mul_f32 (2-cycle class)", n_wg, it);
  run<0, 8, 384>("v_mul_f32 (2-cycle class)", n_wg, it);
  run<1, 1, 192>("v_max_i32 (4-cycle class)", n_wg, it);
  run<1, 2, 192>("v_max_i32 (4-cycle class)", n_wg, it);
  run<1, 4, 192>("v_max_i32 (4-cycle class)", n_wg, it);
  run<1, 8, 192>("v_max_i32 (4-cycle class)", n_wg, it);
  run<1, 8, 64>("v_max_i32 (4-cycle class)", n_wg, it);
  run<1, 8, 128>("v_max_i32 (4-cycle class)", n_wg, it);
  run<1, 8, 256>("v_max_i32 (4-cycle class)", n_wg, it);
  run<2, 1, 64>("v_sqrt_f32", n_wg, it);
  run<2, 8, 64>("v_sqrt_f32", n_wg, it);
  run<3, 1, 192>("v_lshl_or_b32 (VOP3)", n_wg, it);
  run<3, 8, 192>("v_lshl_or_b32 (VOP3)", n_wg, it);
  run<4, 4, 192>("v_pk_mul_f32 (2 values/lane)", n_wg, it);
  run<5, 4, 192>("v_pk_fma_f32 (2 values/lane)", n_wg, it);
  run<6, 4, 192>("v_pk_add_f32 (2 values/lane)", n_wg, it);
  run<6, 4, 96>("v_pk_add_f32 (2 values/lane)", n_wg, it);
  run<7, 8, 192>("v_mul_f32 |x| clamp (VOP3)", n_wg, it);
  run<8, 8, 192>("v_max3_u32", n_wg, it);
  run<9, 8, 192>("v_pk_add_u16 clamp", n_wg, it);
  run<10, 8, 192>("v_perm_b32", n_wg, it);
  run<11, 8, 192>("v_or3_b32", n_wg, it);
  run<12, 8, 192>("v_cvt_pkrtz_f16_f32", n_wg, it);
  run<13, 8, 192>("v_pk_max_f16", n_wg, it);
  run<14, 8, 192>("v_dot2_f32_f16", n_wg, it);
  run<15, 8, 192>("v_dot2c_f32_f16", n_wg, it);
  // the epilogue group of k_acq_mx<0>, two groups per iteration (VPI = their vector instructions; "dep. distance" does not apply);
  // every arm twice: the spread of a repeated line is what a difference between arms has to beat
  for (int rep = 0; rep < 2; rep++) {
    run<16, 8, 120>("group (a) today's order, test", n_wg, it);
    run<17, 8, 120>("group (b) phase order, test", n_wg, it);
    run<18, 8, 112>("group (c) phase order, no test", n_wg, it);
    run<19, 8, 112>("group (d) = (c) + s_nop per phase", n_wg, it);
  }
  return 0;
}
