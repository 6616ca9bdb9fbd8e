// gpsx_fold_codes.hpp -- the single-block grid kernel (k_acq_mx<0>) without the extra K step of the quirk terms.
// That step adds  c1022 * ca(q) + c1021 * cb(q)  to the accumulator of (chip offset q, PRN): PRN flags times per-offset deltas.
// Chips 1022 and 1021 are columns of the main GEMM already, where they meet v[q + 1022] and v[q + 1021] of the pass's vector
// v[k] = -2 (d[k + 1] - d[k])  (d = the pass's plane bits, circular in 1023; sample offsets 9..15: impulses -1 / +1 at entries
// 1021 / 1022 of the first period).  Both steps run at B scale 2^0 against chips that are FP4 1.0, so the term rides in those two
// columns: they meet  f22(q) = v[q + 1022] + ca(q)  and  f21(q) = v[q + 1021] + cb(q)  instead.  With a = d[q - 2], b = d[q - 1]
// (circular: d[-1] = d[1022], d[-2] = d[1021]):
//      passes                    q        f22            f21
//      early (offsets 1..7)      any      2 b - 1        -2 (b - a)          (v[q + 1021] as it is)
//      late  (offsets 9..15)     >= 2     0              2 a - 1
//      late                      1        0              2 a                 (a = d[1022])
//      late                      0        2 b            -2 (b - a) - 1      (b = d[1022], a = d[1021])
// Every value lies in -3..3: exact as an E2M1 code.  A pair is one byte, the code chip 1021 meets in its low nibble, chip 1022's
// in the high one: nibbles 5 and 6 of the fourth dword of the fragment that holds chips 992..1023, bits 20..27.
// Pure host C++ (no HIP): tests/test_single_block_fold_codes.py compiles it with g++.
#pragma once
#include <stdint.h>

constexpr int kGpsxFoldShift = 20;                        // a pair's place in the fragment dword
constexpr uint32_t kGpsxFoldMask = 0xFFu << kGpsxFoldShift;

// E2M1 (FP4) code of an integer in -4..4: magnitudes 0 1 2 3 4 -> codes 0 2 4 5 6, bit 3 the sign
constexpr uint32_t gpsx_e2m1_code(int v)
{
  const uint32_t m = (uint32_t)(v < 0 ? -v : v);
  return ((0x65420u >> (4u * m)) & 0xFu) | (v < 0 ? 8u : 0u);
}

// Value of a four-bit E2M1 code: 1 sign, 2 exponent bits at bias 1, 1 mantissa bit, subnormal 0.5, no infinities
constexpr float gpsx_e2m1_value(int code)
{
  const int e = (code >> 1) & 3, m = code & 1;
  const float mag = e == 0 ? 0.5f * (float)m : (float)(1 << (e - 1)) * (1.f + 0.5f * (float)m);
  return (code & 8) ? -mag : mag;
}

// What chip 1022 / chip 1021 of a PRN meet at chip offset q in a pass that carries the quirk terms (a = d[q - 2], b = d[q - 1])
constexpr int gpsx_fold_f22(bool late, int q, int a, int b) { return !late ? 2 * b - 1 : (q == 0 ? 2 * b : 0); }
constexpr int gpsx_fold_f21(bool late, int q, int a, int b)
{
  return !late ? -2 * (b - a) : (q >= 2 ? 2 * a - 1 : (q == 1 ? 2 * a : -2 * (b - a) - 1));
}
constexpr uint32_t gpsx_fold_pair(bool late, int q, int a, int b)
{
  return gpsx_e2m1_code(gpsx_fold_f21(late, q, a, b)) | (gpsx_e2m1_code(gpsx_fold_f22(late, q, a, b)) << 4);
}
