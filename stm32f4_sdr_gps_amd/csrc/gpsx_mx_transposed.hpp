// gpsx_mx_transposed.hpp -- the index maps of the single-block grid kernel's transposed accumulator tile (k_acq_mx<0>).
// There the Toeplitz fragment is the A operand of the MFMA and the chips are B, so D = A x B comes out with chip offsets in the rows
// and PRNs in the columns: lane l of a wave holds ONE PRN, l & 31, and register r of its tile j the chip offset
//      q = 32 (q0_tile + 2 j) + (r & 3) + 8 (r >> 2) + 4 h,      h = l >> 5,   q0_tile = 8 (wave >> 1) + (wave & 1)
// (tools/microbench/mfma_fp4_corr.hip and mfma_fp6_anchor.hip pin that layout on the device).  A lane's 64 hypotheses of a sample
// offset are numbered by the local index 16 j + r; its running maximum goes by LOCAL keys (magnitude << 6) | (63 - local index), a
// compile-time constant per register, and is turned into the global key (magnitude << 11) | (2047 - byte offset) once per lane and
// sample offset.  For a fixed (wave, h) the chip offset grows with the local index, so among equal magnitudes the larger local
// key is the smaller byte offset, as with the global keys: the reference's tie rule (the first maximum wins) survives the change.
// Pure host C++ (no HIP): tests/test_single_block_transposed_maps.py compiles it with g++.
#pragma once
#include <stdint.h>

constexpr int kGpsxMxtLocals = 64;                         // hypotheses of a lane per sample offset: 4 tiles x 16 registers
constexpr int kGpsxMxtKeyShift = 6;                        // a local key's magnitude field starts here
constexpr int kGpsxKeyShift = 11;                          // a global key's

constexpr int gpsx_mxt_q0_tile(int wave) { return 8 * (wave >> 1) + (wave & 1); }
// row of D in register r of lane half h: the chip offset within the tile
constexpr int gpsx_mxt_row(int h, int r) { return (r & 3) + 8 * (r >> 2) + 4 * h; }
constexpr int gpsx_mxt_q(int wave, int h, int j, int r) { return 32 * (gpsx_mxt_q0_tile(wave) + 2 * j) + gpsx_mxt_row(h, r); }
constexpr int gpsx_mxt_local(int j, int r) { return 16 * j + r; }
constexpr uint32_t gpsx_mxt_code(int j, int r) { return (uint32_t)(kGpsxMxtLocals - 1 - gpsx_mxt_local(j, r)); }
constexpr uint32_t gpsx_mxt_local_key(uint32_t bits, int j, int r) { return (bits << kGpsxMxtKeyShift) | gpsx_mxt_code(j, r); }
// the chip offset of local index `local` from the lane's first one, q_first = gpsx_mxt_q(wave, h, 0, 0) = 32 q0_tile + 4 h:
// 64 j + 8 (r >> 2) + (r & 3) are bit fields of 16 j + r moved into place
constexpr int gpsx_mxt_q_of_local(int q_first, int local)
{
  return q_first + ((local & 48) << 2) + ((local & 12) << 1) + (local & 3);
}
// From a lane's winning local key to the global key.  Whatever a magnitude carries above its low 21 bits (the small path's root is
// the f32 pattern 0x4B000000 + magnitude) is the same in all keys of a lane and leaves the 32-bit word in the shift.
constexpr uint32_t gpsx_mxt_global_key(uint32_t local_key, int q_first, int half)
{
  const int local = (int)((local_key & (kGpsxMxtLocals - 1)) ^ (kGpsxMxtLocals - 1));
  const int q = gpsx_mxt_q_of_local(q_first, local);
  return ((local_key >> kGpsxMxtKeyShift) << kGpsxKeyShift) | (uint32_t)(2047 - (2 * q + half));
}
// The epilogue's trust limit (mxt_epilogue).  The small path's root bits are kGpsxMxtRootBias + magnitude; they are
// taken for all 64 hypotheses of a lane without a radius test, and the lane's winning local key is compared once with the local key
// of (magnitude kGpsxMxtTrustRadius, code 0), mod 2^32 as the keys themselves are.  Magnitudes stay below 2^14 (11 585 at the most),
// so a local key is monotone in (magnitude, code): winner >= limit <=> some hypothesis of the lane has magnitude >= 1024.
constexpr uint32_t kGpsxMxtRootBias = 0x4B000000u;         // the f32 pattern of 2^23: what the rounding fma leaves above the root
constexpr int kGpsxMxtTrustRadius = 1024;                  // the small path is used below it (and proven below 1182)
constexpr int kGpsxMxtHotRadius = 768;                     // a winner from here on sends the wave's NEXT epilogue down the careful path
constexpr uint32_t gpsx_mxt_limit_key(int radius) { return (kGpsxMxtRootBias + (uint32_t)radius) << kGpsxMxtKeyShift; }
constexpr uint32_t gpsx_mxt_trust_limit_key() { return gpsx_mxt_limit_key(kGpsxMxtTrustRadius); }
constexpr uint32_t gpsx_mxt_hot_limit_key() { return gpsx_mxt_limit_key(kGpsxMxtHotRadius); }
// the 8-PRN sharding group a lane's results belong to (the lane is the PRN)
constexpr int gpsx_mxt_group(int lane) { return (lane & 31) >> 3; }
