// Operand-layout check for the single-block grid's one-pass anchor: the mixed call
//      v_mfma_scale_f32_32x32x64_f8f6f4   A = E2M1 (FP4) chips {0, 1} at scale 2^-13,   B = E3M2 (BF6) integers -8..8 at scale 2^1
// before any kernel relies on it (as mfma_fp4_corr.hip part 1 did for the FP4 x FP4 call).
//   A (M x K, rows = PRN)  lane (m = lane & 31, h = lane >> 5): 32 nibbles, k = 32 h + j at bit 4 j of four dwords (pinned in round 2)
//   B (K x N, cols = q)    HYPOTHESIS: lane (n, h): 32 six-bit codes, k = 32 h + j at bit 6 j of six dwords (LSB first, codes straddle
//                          dwords), dwords 6, 7 ignored; format code blgp = 3 (E3M2; 2 would be E2M3); scale_b byte 0 with opsel_b = 0
// Part 1  every lane x every element position x each of the 17 values, one MFMA per case, blgp 3 and (for contrast) 2
// Part 2  chained accumulation: 16 k-steps x 17 passes of random 17-valued B into one accumulator with a non-zero start;
//         scales with all four bytes equal and with only byte 0 set (pins which byte the opsel = 0 call reads)
// Part 3  the kernel's way of feeding B: ONE packed six-bit stream per vector, lane (n, h) of fragment f takes the 192 bits at bit
//         6 (32 (f + h) + n) with seven dword reads and six v_alignbit_b32 -- a Toeplitz product against the CPU
// Transposed arm (parts 1T, 2T, 3T): the same three parts with the operands swapped -- A = the E3M2 vector (cbsz 3, the same six
//         dwords per lane, dwords 6, 7 ignored, its scale on the A side), B = the FP4 chips (blgp 4, 2^-13 on the B side) -- so
//         that D comes out transposed: register i of lane l = D[row (i & 3) + 8 (i >> 2) + 4 (l >> 5)][col l & 31], rows = the
//         vector's columns (chip offsets), the lane = the PRN
// Every part must print 0 mismatches for the hypothesis; the program's exit status says so.
// Build: hipcc --offload-arch=gfx950 -O3 mfma_fp6_anchor.hip -o mfma_fp6_anchor
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../stm32f4_sdr_gps_amd/csrc/gpsx_anchor_codes.hpp"

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); exit(1); } } while (0)

typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));
typedef unsigned int u32;

constexpr float kStart = 3.0f;       // accumulator start of every case: on the result's 2^-12 grid, every sum stays below 2^24 of it

// One wave per case: acc = start; n_step MFMAs over a[case][step][lane][4] and b[case][step][lane][6]; out[case][lane][16].
// TR: the operands swapped (b as A with format code BLGP in cbsz, a as B), the scales with them
template <int BLGP, bool TR = false>
__global__ __launch_bounds__(64) void k_cases(const u32 *a, const u32 *b, float *out, int n_step, u32 scale_a, u32 scale_b)
{
  const int lane = threadIdx.x, cs = blockIdx.x;
  v16f acc;
  for (int r = 0; r < 16; r++)
    acc[r] = kStart;
  for (int s = 0; s < n_step; s++) {
    const u32 *pa = a + ((size_t)(cs * n_step + s) * 64 + lane) * 4;
    const u32 *pb = b + ((size_t)(cs * n_step + s) * 64 + lane) * 6;
    const v8i fa = {(int)pa[0], (int)pa[1], (int)pa[2], (int)pa[3], 0, 0, 0, 0};
    const v8i fb = {(int)pb[0], (int)pb[1], (int)pb[2], (int)pb[3], (int)pb[4], (int)pb[5], -1, -1};   // dwords 6, 7 must not matter
    if constexpr (TR)
      acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(fb, fa, acc, BLGP, 4, 0, scale_b, 0, scale_a);
    else
      acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(fa, fb, acc, 4, BLGP, 0, scale_a, 0, scale_b);
  }
  for (int r = 0; r < 16; r++)
    out[((size_t)cs * 64 + lane) * 16 + r] = acc[r];
}

constexpr int kStreamDwords = 384 + 8;   // 2048 six-bit codes + slack for the seventh dword of the last window

// Part 3: one workgroup of 8 waves, wave w owns q-tiles w, w + 8, w + 16, w + 24; out[q][prn] = sum_c chip[prn][c] * val[q + c].
// TR: the fragment is A, the chips are B: lane (n, h) then holds PRN n at chip offsets 32 tile + (r & 3) + 8 (r >> 2) + 4 h
template <bool TR>
__global__ __launch_bounds__(512) void k_toeplitz(const u32 *stream, const u32 *chips /* [16][64 lanes][4] */, float *out, u32 scale_a, u32 scale_b)
{
  __shared__ u32 s6[kStreamDwords];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 31, h = lane >> 5;
  for (int i = tid; i < kStreamDwords; i += 512)
    s6[i] = stream[i];
  __syncthreads();
  const int sh = (6 * n) & 31;
  for (int j = 0; j < 4; j++) {
    const int tile = wave + 8 * j;
    v16f acc;
    for (int r = 0; r < 16; r++)
      acc[r] = kStart;
    for (int kappa = 0; kappa < 16; kappa++) {
      const int f = tile + 2 * kappa + h;                // window starts at code 32 f + n, bit 6 (32 f + n)
      const u32 *w = &s6[6 * f + ((6 * n) >> 5)];
      u32 d[7];
      for (int i = 0; i < 7; i++)
        d[i] = w[i];
      v8i fb = {0, 0, 0, 0, 0, 0, 0, 0};
      for (int i = 0; i < 6; i++)
        fb[i] = (int)__builtin_amdgcn_alignbit(d[i + 1], d[i], sh);      // ({hi, lo} >> sh)[31:0]; sh = 0 passes d[i]
      const u32 *pa = chips + ((size_t)kappa * 64 + lane) * 4;
      const v8i fa = {(int)pa[0], (int)pa[1], (int)pa[2], (int)pa[3], 0, 0, 0, 0};
      if constexpr (TR)
        acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(fb, fa, acc, 3, 4, 0, scale_b, 0, scale_a);
      else
        acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(fa, fb, acc, 4, 3, 0, scale_a, 0, scale_b);
    }
    for (int r = 0; r < 16; r++) {
      const int sub = (r & 3) + 8 * (r >> 2) + 4 * h;
      if constexpr (TR)
        out[(size_t)(32 * tile + sub) * 32 + n] = acc[r];
      else
        out[(size_t)(32 * tile + n) * 32 + sub] = acc[r];
    }
  }
}

static float e2m3_value(int code)      // what blgp = 2 would make of the same six bits
{
  const int e = (code >> 3) & 3, m = code & 7;
  const float mag = e == 0 ? m / 8.f : (float)(1 << (e - 1)) * (1.f + m / 8.f);
  return (code & 32) ? -mag : mag;
}

// Packs 32 six-bit codes LSB first into six dwords.
static void pack6(const uint8_t *codes, u32 *dw)
{
  memset(dw, 0, 24);
  for (int j = 0; j < 32; j++)
    for (int bit = 0; bit < 6; bit++)
      if (codes[j] >> bit & 1)
        dw[(6 * j + bit) >> 5] |= 1u << ((6 * j + bit) & 31);
}

struct Cases {
  int n_case, n_step;
  std::vector<uint8_t> chip;   // [case][step][32 m][64 k]  0 / 1
  std::vector<uint8_t> code;   // [case][step][64 k][32 n]  six-bit codes
};

static long run_cases(const Cases &c, int blgp, u32 scale_a, u32 scale_b, double mult, const char *what, bool transposed = false)
{
  const size_t n_ms = (size_t)c.n_case * c.n_step;
  std::vector<u32> a(n_ms * 64 * 4, 0), b(n_ms * 64 * 6, 0);
  for (size_t ms = 0; ms < n_ms; ms++)
    for (int lane = 0; lane < 64; lane++) {
      const int r = lane & 31, h = lane >> 5;
      uint8_t codes[32];
      for (int j = 0; j < 32; j++) {
        if (c.chip[(ms * 32 + r) * 64 + 32 * h + j])
          a[(ms * 64 + lane) * 4 + (j >> 3)] |= 2u << (4 * (j & 7));      // FP4 code 2 = 1.0
        codes[j] = c.code[(ms * 64 + 32 * h + j) * 32 + r];
      }
      pack6(codes, &b[(ms * 64 + lane) * 6]);
    }
  u32 *d_a, *d_b;
  float *d_out;
  CHECK(hipMalloc(&d_a, a.size() * 4));
  CHECK(hipMalloc(&d_b, b.size() * 4));
  CHECK(hipMalloc(&d_out, (size_t)c.n_case * 64 * 16 * 4));
  CHECK(hipMemcpy(d_a, a.data(), a.size() * 4, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(d_b, b.data(), b.size() * 4, hipMemcpyHostToDevice));
  if (transposed && blgp == 3)
    hipLaunchKernelGGL((k_cases<3, true>), dim3(c.n_case), dim3(64), 0, 0, d_a, d_b, d_out, c.n_step, scale_a, scale_b);
  else if (transposed)
    hipLaunchKernelGGL((k_cases<2, true>), dim3(c.n_case), dim3(64), 0, 0, d_a, d_b, d_out, c.n_step, scale_a, scale_b);
  else if (blgp == 3)
    hipLaunchKernelGGL(k_cases<3>, dim3(c.n_case), dim3(64), 0, 0, d_a, d_b, d_out, c.n_step, scale_a, scale_b);
  else
    hipLaunchKernelGGL(k_cases<2>, dim3(c.n_case), dim3(64), 0, 0, d_a, d_b, d_out, c.n_step, scale_a, scale_b);
  CHECK(hipDeviceSynchronize());
  std::vector<float> out((size_t)c.n_case * 64 * 16);
  CHECK(hipMemcpy(out.data(), d_out, out.size() * 4, hipMemcpyDeviceToHost));
  CHECK(hipFree(d_a));
  CHECK(hipFree(d_b));
  CHECK(hipFree(d_out));
  long bad = 0;
  for (int cs = 0; cs < c.n_case; cs++)
    for (int lane = 0; lane < 64; lane++)
      for (int r = 0; r < 16; r++) {
        // D[row][col]: register r of lane l holds row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31; rows belong to A
        const int sub = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        const int n = transposed ? sub : lane & 31, m = transposed ? lane & 31 : sub;
        double want = 0;
        for (int s = 0; s < c.n_step; s++) {
          const size_t ms = (size_t)cs * c.n_step + s;
          for (int k = 0; k < 64; k++) {
            const int code = c.code[(ms * 64 + k) * 32 + n];
            want += c.chip[(ms * 32 + m) * 64 + k] * (blgp == 3 ? (double)gpsx_e3m2_value(code) : (double)e2m3_value(code));
          }
        }
        want = want * mult + kStart;
        const float got = out[((size_t)cs * 64 + lane) * 16 + r];
        if (got != (float)want) {
          if (bad < 4)
            printf("  mismatch case %d col %d row %d: got %.6f want %.6f\n", cs, n, m, got, want);
          bad++;
        }
      }
  printf("%s: %ld mismatches of %d\n", what, bad, c.n_case * 64 * 16);
  return bad;
}

int main()
{
  setvbuf(stdout, nullptr, _IONBF, 0);
  hipDeviceProp_t prop;
  CHECK(hipGetDeviceProperties(&prop, 0));
  printf("device %s CUs=%d\n", prop.gcnArchName, prop.multiProcessorCount);
  printf("E3M2 codes of 8 - S, S = 0..16:");
  for (int s = 0; s <= 16; s++)
    printf(" %d", kGpsxAnchorCode[s]);
  printf("\n");
  srand(20261018);
  const u32 kA = 0x72727272u, kB = 0x80808080u;          // E8M0 114 = 2^-13, 128 = 2^1
  const double mult = 1.0 / 4096.0;                      // 2^-13 * 2^1
  long hyp_bad = 0;

  // ---- part 1: 17 values x 32 element positions; every lane (n, h) carries its own value at that position -----------------
  Cases p1;
  p1.n_case = 17 * 32;
  p1.n_step = 1;
  p1.chip.resize((size_t)p1.n_case * 32 * 64);
  p1.code.assign((size_t)p1.n_case * 64 * 32, 0);
  for (auto &x : p1.chip)
    x = rand() & 1;
  for (int cs = 0; cs < p1.n_case; cs++) {
    const int vi = cs % 17, j = cs / 17;
    for (int h = 0; h < 2; h++)
      for (int n = 0; n < 32; n++)
        p1.code[((size_t)cs * 64 + 32 * h + j) * 32 + n] = kGpsxAnchorCode[(vi + n + 7 * h) % 17];
  }
  hyp_bad += run_cases(p1, 3, kA, kB, mult, "part 1 blgp 3 (E3M2), 17 values x 32 positions x 64 lanes, bit 6 j LSB first");
  run_cases(p1, 2, kA, kB, mult, "part 1 blgp 2 (E2M3) on the same bits, for contrast");

  // ---- part 2: chained accumulation, 16 k-steps x 17 passes, random values of the 17 -------------------------------------------
  Cases p2;
  p2.n_case = 8;
  p2.n_step = 16 * 17;
  p2.chip.resize((size_t)p2.n_case * p2.n_step * 32 * 64);
  p2.code.resize((size_t)p2.n_case * p2.n_step * 64 * 32);
  for (auto &x : p2.chip)
    x = rand() & 1;
  for (size_t i = 0; i < p2.code.size(); i++)
    p2.code[i] = kGpsxAnchorCode[i < (size_t)p2.n_step * 64 * 32 ? (rand() % 2) * 16 : rand() % 17];    // case 0: only the extremes +-8
  hyp_bad += run_cases(p2, 3, kA, kB, mult, "part 2 chained 272 MFMAs, scale bytes all equal (0x72727272, 0x80808080)");
  hyp_bad += run_cases(p2, 3, 0x7F7F7F72u, 0x7F7F7F80u, mult, "part 2 chained 272 MFMAs, scale in byte 0 only, opsel 0");
  run_cases(p2, 3, 0x727F7F7Fu, 0x807F7F7Fu, mult, "part 2 scale in byte 3 only, opsel 0 (expected to MISMATCH)");

  // ---- the transposed arm of parts 1 and 2: E3M2 as A (cbsz 3), chips as B (blgp 4), each scale with its operand ----------------
  hyp_bad += run_cases(p1, 3, kA, kB, mult, "part 1T cbsz 3 (E3M2 as A) x blgp 4, 17 values x 32 positions x 64 lanes, D transposed", true);
  run_cases(p1, 2, kA, kB, mult, "part 1T cbsz 2 (E2M3 as A) on the same bits, for contrast", true);
  hyp_bad += run_cases(p2, 3, kA, kB, mult, "part 2T chained 272 MFMAs, 2^1 on the A side, 2^-13 on the B side, bytes all equal", true);
  hyp_bad += run_cases(p2, 3, 0x7F7F7F72u, 0x7F7F7F80u, mult, "part 2T chained 272 MFMAs, scale in byte 0 only, opsel 0", true);

  // ---- part 3: one packed stream, windows by funnel shift ---------------------------------------------------------------------
  {
    std::vector<int> sums(2048 + 64, 0);
    for (int k = 0; k < 2048; k++)
      sums[k] = k < 40 ? (k & 1) * 16 : rand() % 17;       // 0 and 16 adjacent at the front
    std::vector<u32> stream(kStreamDwords, 0);
    for (int k = 0; k < 2048; k++) {
      const u32 code = kGpsxAnchorCode[sums[k]];
      for (int bit = 0; bit < 6; bit++)
        if (code >> bit & 1)
          stream[(6 * k + bit) >> 5] |= 1u << ((6 * k + bit) & 31);
    }
    std::vector<uint8_t> chip(32 * 1024);
    for (int p = 0; p < 32; p++)
      for (int c = 0; c < 1024; c++)
        chip[p * 1024 + c] = c < 1023 ? rand() & 1 : 0;
    std::vector<u32> a(16 * 64 * 4, 0);
    for (int kappa = 0; kappa < 16; kappa++)
      for (int lane = 0; lane < 64; lane++)
        for (int j = 0; j < 32; j++)
          if (chip[(lane & 31) * 1024 + 64 * kappa + 32 * (lane >> 5) + j])
            a[(kappa * 64 + lane) * 4 + (j >> 3)] |= 2u << (4 * (j & 7));
    u32 *d_s, *d_a;
    float *d_out;
    CHECK(hipMalloc(&d_s, stream.size() * 4));
    CHECK(hipMalloc(&d_a, a.size() * 4));
    CHECK(hipMalloc(&d_out, 1024 * 32 * 4));
    CHECK(hipMemcpy(d_s, stream.data(), stream.size() * 4, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_a, a.data(), a.size() * 4, hipMemcpyHostToDevice));
    for (int tr = 0; tr < 2; tr++) {
      CHECK(hipMemset(d_out, 0, 1024 * 32 * 4));
      if (tr)
        hipLaunchKernelGGL(k_toeplitz<true>, dim3(1), dim3(512), 0, 0, d_s, d_a, d_out, kA, kB);
      else
        hipLaunchKernelGGL(k_toeplitz<false>, dim3(1), dim3(512), 0, 0, d_s, d_a, d_out, kA, kB);
      CHECK(hipDeviceSynchronize());
      std::vector<float> out(1024 * 32);
      CHECK(hipMemcpy(out.data(), d_out, out.size() * 4, hipMemcpyDeviceToHost));
      long bad = 0;
      for (int q = 0; q < 1024; q++)
        for (int p = 0; p < 32; p++) {
          double want = 0;
          for (int c = 0; c < 1024; c++)
            want += chip[p * 1024 + c] * (8 - sums[q + c]);
          want = want * mult + kStart;
          if (out[q * 32 + p] != (float)want) {
            if (bad < 4)
              printf("  mismatch q %d prn %d: got %.6f want %.6f\n", q, p, out[q * 32 + p], want);
            bad++;
          }
        }
      printf("part 3%s Toeplitz from one packed stream, 7 dwords + 6 alignbit per fragment%s: %ld mismatches of %d\n", tr ? "T" : "",
             tr ? ", the fragment as A" : "", bad, 1024 * 32);
      hyp_bad += bad;
    }
  }
  printf(hyp_bad == 0 ? "LAYOUT PINNED: blgp 3 / cbsz 3, code j at bit 6 j LSB first, scale byte 0 (opsel 0), D transposes with the operands\n" : "LAYOUT NOT PINNED\n");
  return hyp_bad == 0 ? 0 : 1;
}
