// gpsx_anchor_codes.hpp -- the one-pass anchor of the single-block grid kernel (k_acq_mx<0>): the block sums S_0[k] in 0..16 of
// the first sample offset as ONE matrix operand, E3M2 (the six-bit "BF6" of v_mfma_scale_f32_32x32x64_f8f6f4: 1 sign, 3 exponent
// bits at bias 3, 2 mantissa bits, no infinities), which holds every integer in -8..8 exactly.  The vector holds 8 - S_0[k] at B
// scale 2^1; against chips in {0, 1} the pass adds
//      2 * sum_c chip[c] * (8 - S_0[q + c]) = -2 M_0(q) + 16 * 512 = -2 M_0(q) + 8192     (every C/A code has 512 ones),
// so the accumulator's start value is the two-pass anchor's less 8192.
// Pure host C++ (no HIP): tests/test_single_block_anchor_codes.py compiles it with g++; tools/microbench/mfma_fp6_anchor.hip pins
// the operand layout on the device with the same table.
#pragma once
#include <stdint.h>

// E3M2 code of 8 - S for S = 0..16: +8 = e 6 m 0, 7..4 = e 5 m 3..0, 3 = e 4 m 2, 2 = e 4 m 0, 1 = e 3 m 0, 0; negatives set bit 5
constexpr uint8_t kGpsxAnchorCode[17] = {24, 23, 22, 21, 20, 18, 16, 12, 0, 44, 48, 50, 52, 53, 54, 55, 56};

// The same code by arithmetic, as the kernel computes it per block sum: |v| >= 4 sits in the two top binades (16 + |v|), the four
// small magnitudes come from a byte table.
constexpr uint32_t gpsx_anchor_code(int s)
{
  const int v = 8 - s;
  const uint32_t m = (uint32_t)(v < 0 ? -v : v);
  return (m >= 4u ? 16u + m : (0x12100C00u >> (8u * m)) & 0xFFu) | (v < 0 ? 32u : 0u);
}
constexpr bool gpsx_anchor_codes_agree(int s = 0) { return s > 16 || (gpsx_anchor_code(s) == kGpsxAnchorCode[s] && gpsx_anchor_codes_agree(s + 1)); }
static_assert(gpsx_anchor_codes_agree(), "gpsx_anchor_code() is the table");

// Value of a six-bit E3M2 code (subnormals at exponent field 0: m / 16).
constexpr float gpsx_e3m2_value(int code)
{
  const int e = (code >> 2) & 7, m = code & 3;
  const float mag = e == 0 ? m / 16.f : (e >= 3 ? (float)(1 << (e - 3)) : 1.f / (float)(1 << (3 - e))) * (1.f + m / 4.f);
  return (code & 32) ? -mag : mag;
}

// The accumulator start of k_acq_mx<0> per (PRN, Doppler-wiped stream): pop_d = pop(D) of the quirk terms, as in the two-pass
// form, whose start is pop_d + 8192 - 8184 (its passes add -2 M); the one-pass anchor adds -2 M + 8192.
constexpr int kGpsxAnchorChipOnes = 512;                                   // ones per C/A code period, every PRN
constexpr int kGpsxAnchorPassBias = 16 * kGpsxAnchorChipOnes;              // 8192: what the "8 -" adds through the chips
constexpr int gpsx_start_two_pass(int pop_d) { return pop_d + 8192 - 8184; }
constexpr int gpsx_start_one_pass(int pop_d) { return gpsx_start_two_pass(pop_d) - kGpsxAnchorPassBias; }
