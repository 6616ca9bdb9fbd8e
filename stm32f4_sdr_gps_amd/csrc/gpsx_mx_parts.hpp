// gpsx_mx_parts.hpp -- what the matrix-core grid kernels share: k_acq_mx<MODE> (k_acq_mx.hip, k_acq_mx_byte.hip) and the weighted
// k_acq_mxw / k_acq_wmx_ms (k_acq_mxw.hip).  The grid: the fine (16368-phase) sweep with the correlations on the matrix cores.
//
// Same contract as k_acq / k_acq_poly: per (search, PRN, Doppler, replica bit shift) the triplet correlation_search
// (PM/GPS/gps_misc.c:155-191) returns, bit for bit; same preamble (capture -> LDS, carrier wipe-off K3), same
// per-hypothesis corrections of the reference's quirks and the same magnitude.  What changes is where the sums
//      M_t0(q) = sum_c chip_p[c] * S_t0[q + c],   S_t0[k] = pop(D[16 k + t0, +16)),   sample offset s = 16 q + t0
// come from.  In the polyphase form (k_acq_poly.hip)  M_{t0+1}(q) - M_t0(q) = sum_c chip_p[c] * e_t0[q + c]  with
// e_t0[k] = d_t0[k + 1] - d_t0[k] in {-1, 0, +1},  d_t0[k] = D(16 k + t0): for the 32 PRNs of a workgroup and the 1023
// chip offsets q that is a GEMM   C[p][q] += A[p][c] * B[c][q],   A = chips (32 x 1024),  B = the TOEPLITZ matrix
// B[c][q] = e[(q + c) mod 1023]  of ONE 1023-element vector -- and C, kept in the accumulator registers from one sample
// offset to the next, IS M_t0.  Operands are MX-FP4 (E2M1: 0, +-1, 2, 3, 4 exact; block scale E8M0 2^0 or 2^2),
// v_mfma_scale_f32_32x32x64_f8f6f4 accumulates in f32: every partial sum is an integer below 2^24, so the result is
// exact whatever the order (tools/microbench/mfma_fp4_corr.hip checks layouts and exactness on the device).
// M for the first offset takes two passes: S = (S & 3) + 4 (S >> 2), both parts FP4-exact, the second at a block scale -- or,
// in the single-block form, ONE pass with the vector as E3M2 (six-bit codes, the same MFMA rate): 8 - S, every integer in -8..8
// exact (gpsx_anchor_codes.hpp; tools/microbench/mfma_fp6_anchor.hip checks that operand's layout on the device).
//
// Data movement: B never exists.  The nibble vector (2048 entries: one period + its wrap-around) sits in LDS in eight
// copies, copy c starting at nibble c, so that lane (n, h) of tile (Q, kappa) -- column q = 32 Q + n, chips
// 64 kappa + 32 h .. + 31 -- finds its 32 nibbles dword-aligned at dword 4 (Q + 2 kappa + h) + n / 8 of copy n % 8, bank
// conflict free.  Tile (Q, kappa) reads what (Q - 2, kappa + 1) reads: a wave owns q-tiles Q0, Q0 + 2, Q0 + 4, Q0 + 6
// and walks the anti-diagonals f = Q + 2 kappa, 19 fragment loads for 64 MFMAs per stream.
//
// Nothing linear is left to the vector ALU.  What the reference's quirks add to a popcount is linear in chip bits
// (DESIGN.md 4.1), so it rides in the same accumulators: the accumulator of (q, PRN p) holds, after the pass of sample
// offset t0, exactly  cnt(q, t0, p) - 8184  -- the number gps_correlation8 clips and squares:
//   * the vector carries -2 e (values 0, +-2), the accumulators start at pop(D) + 8192 - 8184 (or at -2^20 for byte offsets
//     outside the search window: they clip to zero by themselves);
//   * odd byte offsets skip the replica word at the wrap (quirk Q3), a popcount against chips (1021 - q, 1022 - q): two
//     impulses of -1 / +1 in the vector at entries 1021 and 1022 (not in their wrap-around copies) per step;
//   * the terms "PRN flag x per-offset value" (chip 1022: quirk Q5 and the tail word of Q3; chip 1021: the tail word) are
//     one more K step of the GEMM: A column 0 of lane half 0 = chip 1022 of the PRN, of half 1 = chip 1021, B = the
//     per-offset deltas (0, +-1, +-2) read as one byte per lane -- in the single-block form they ride in chip columns 1021 / 1022
//     of the main GEMM instead (MxFold, gpsx_fold_codes.hpp);
//   * at the switch from even to odd byte offsets (t0 = 8) every such term jumps; that one step is patched into the
//     accumulators by the vector ALU (mx_half_switch).
// The epilogue of a sample offset is then: clip, square, add, correctly rounded root, truncate, (add the running sum of
// earlier blocks,) pack the key, max, sum.
//
// A workgroup = 8 waves = one (search, Doppler) pair x 32 PRNs (four 8-PRN sharding units) x all 16 sample offsets.
// Lane layout, by form:
//   * the walk, store, split and byte-phase forms (k_acq_mx<1..5>) and the weighted kernels: chips = A, fragment = B.  Lane (n, h)
//     of a wave holds, per tile, column q = 32 Q + n for the 16 PRNs p = (r & 3) + 8 (r >> 2) + 4 h, r = 0..15 -- the per-offset
//     work (corrections, window test) is shared by 16 hypotheses; every lane folds its 16 results per sample offset into its own
//     LDS slots (MxShared::part), reduced once at the end.
//   * the single-block form (k_acq_mx<0>), where the fold and the anchor left no per-offset work inside the steps: fragment = A,
//     chips = B (mx_mfma<true>), each block scale with its operand -- the TRANSPOSED tile (gpsx_mx_transposed.hpp).  Lane (n, h)
//     holds PRN n, and register r of tile j the chip offset 32 (q0_tile + 2 j) + (r & 3) + 8 (r >> 2) + 4 h: a sample offset's
//     maximum and sum are register chains of the lane, two LDS atomics per wave, and the result slots (k_acq_mx.hip:
//     MxSingleShared::part) one word per (bit shift, field, lane half, PRN).  Its LDS block ends with MxSharedCore.
// The matrix pipe and the vector ALU of a SIMD are separate: waves 0..3 and 4..7 (one of each per SIMD) run half a step apart,
// one group's MFMA pass under the other's epilogue, with one barrier per step.
//
// Forms (k_acq_mx<MODE>; all in k_acq_mx.hip but 4, in k_acq_mx_byte.hip): 0 single block, one workgroup per cluster (the headline
// sweep); 3 / 1 a workgroup walks the blocks of its search, running sums as 16- / 24-bit records through HBM scratch; 2 a workgroup
// per (cluster, block), magnitudes out for k_acq_vals_search; 4 the byte-phase grid (sample offsets 0 and 8, each started directly
// from its own block sums; one persistent workgroup per CU runs its clusters as ONE software pipeline: mx_byte_pipe); 5 small
// launches: 2 / 4 / 8 workgroups per cluster, each started directly at its own sample offset (mx_direct_terms: every quirk term as
// a start value), results merged through global planes.
#pragma once
#if !defined(GPSX_LAB) && defined(MX_VARIANT_B)
#error "variants of the matrix-core grid kernels for same-box A/B timing build with -DGPSX_LAB only: tools/build_variant.sh"
#endif
#include <cstdlib>

#include "gpsx_anchor_codes.hpp"
#include "gpsx_device.hpp"
#include "gpsx_fold_codes.hpp"
#include "gpsx_kernels.hpp"

namespace gpsx {

namespace {

typedef int v8i __attribute__((ext_vector_type(8)));
typedef int v4i __attribute__((ext_vector_type(4)));
typedef float v16f __attribute__((ext_vector_type(16)));

constexpr int kMxThreads = 512;
constexpr int kMxTiles = 4;            // q-tiles (32 chip offsets each) per wave
constexpr int kCopyDwords = 260;       // one shifted copy of the nibble vector: 256 dwords + slack; 260 = 4 (mod 32): the 32
                                       // lanes of a fragment read (copy n % 8, dword n / 8 + ..) hit 32 different banks
constexpr int kVecDwords = 258;        // dwords of copy 0 that the shifted copies are cut from
constexpr int kPlaneWordsMx = 66;      // polyphase bit plane: 1023 bits + circular extension to 2112
constexpr u32 kScaleOne = 0x7F7F7F7Fu;   // E8M0 127 = 2^0
// The accumulators hold (cnt - 8184) / 8192: the A operand's block scale is 2^-13 (E8M0 114).  A power of two changes no
// rounding anywhere, and it puts every in-window value inside (-1, 1), where one v_mul_f32 c, |c| with the clamp modifier
// IS the reference's clip-and-square (mx_clip_square).
constexpr u32 kScaleA = 0x72727272u;
constexpr float kAccScale = 1.0f / 8192.0f;
constexpr float kUnscaleSq = 67108864.0f;   // 2^26: scaled squares -> integers
constexpr u32 kScaleEight = 0x82828282u; // E8M0 130 = 2^3
constexpr u32 kScaleTwo = 0x80808080u;   // E8M0 128 = 2^1

// (MxSharedCore: everything but the result slots -- the single-block form, whose slots are its own, ends its block here)
struct MxSharedCore {
  uint16_t x[1024];                      // raw IF block (sign plane)
  u32 d[2][514];                         // wiped I / Q streams (word 511 = wrap-around copy, then zero pad)
  u32 plane[2][16][kPlaneWordsMx];       // d_t0 for the 16 sample offsets, circularly extended
  u32 base[2][kCopyDwords];              // nibble vector of the pass in preparation (copy 0), I / Q
  u32 e8[2][2][8][kCopyDwords];          // [buffer][stream][copy][dword]
  u32 corr[2][2][2][128];                // [buffer][stream][chip 1022 / chip 1021 term][q / 8]: FP4 codes of the step's deltas
  v4i chips_a[16][2][32];                // A fragments: [kappa][h][PRN] = 32 FP4 chips 64 kappa + 32 h ..
  u32 chip_t[1032];                      // chip_t[c + 1]: bit p = chip c of PRN p of this cluster; [0] = chip -1 = 0
  u32 ones[2];                           // pop(D) per stream
  u32 t_lut[768];                        // [0, 512): 9 adjacent bits -> FP4 codes of -2 (bit k+1 - bit k), k = 0..7;
                                         // [512, 768): 8 bits -> FP4 codes of 2 bit - 1 (mx_fill_tables)
};
struct MxShared : MxSharedCore {
  alignas(16) u32 part[8][32][2][32];              // (packed best key, sum) per bit shift, PRN and lane of the wave half that holds the
                                         // PRN: every lane folds its own results in with LDS atomics (no return value, no
                                         // conflicts), the 32 lanes meet once, when the workgroup writes its triplets
};

// The single-block form alone (k_acq_mx<0>; behind MxShared in its LDS block): the quirk terms of a recurrence pass as code pairs
// for chip columns 1021 / 1022 of the main GEMM instead of sh.corr and the extra K step (gpsx_fold_codes.hpp)
struct MxFold {
  u32 pair[2][2][1024];                  // [buffer][stream][q]: the pair of chip offset q where the fragment dword has it, bits 20..27
  v4i lut[2][32];                        // [late][plane bits 4 j - 2 .. 4 j + 2] -> the pairs of q = 4 j .. 4 j + 3, q >= 2
};

// The single-block form alone: the chip operand of a lane -- chips_a[kappa][h][PRN] of its own (PRN, h), kappa < kMxChipsResident --
// in registers for the whole cluster.  With the transposed tile a lane's B operand is 32 chips of ONE PRN and K half per kappa: the
// same 4 dwords in the anchor pass and in all fifteen recurrence passes, of every tile and both streams.  The anchor pass reads
// them from LDS as it always did, a step ahead of their first MFMA (mx_anchor_step), and they stay; the recurrence passes read no
// chips (mx_pass_step<.., RES>).  k[] IS the a[] of the passes' steps: an entry at or beyond kMxChipsResident is requested by every
// pass a step ahead of its use, as in the other forms, and lives no longer than that.  The passes are unrolled over the
// anti-diagonal, so every k[] is indexed by a constant: registers, never memory.
// 16 = all of them: k_acq_mx<0> at 16 compiles without scratch inside the 256 registers that two waves per SIMD leave a wave.
constexpr int kMxChipsResident = 16;
static_assert(kMxChipsResident >= 0 && kMxChipsResident <= 16 && kMxChipsResident % 4 == 0, "whole quads of kappa");
struct MxChipRegs {
  v4i k[16];
};

__device__ __forceinline__ v8i widen(v4i x) { return v8i{x.x, x.y, x.z, x.w, 0, 0, 0, 0}; }

__device__ __forceinline__ u32 lds_byte(const u32 *words, int byte_index)
{
  return (words[byte_index >> 2] >> ((byte_index & 3) * 8)) & 0xFFu;
}

// 8 bits -> 8 nibbles (bit k -> bit 4 k)
__device__ __forceinline__ u32 spread8(u32 x)
{
  u32 t = (x | (x << 12)) & 0x000F000Fu;
  t = (t | (t << 6)) & 0x03030303u;
  t = (t | (t << 3)) & 0x11111111u;
  return t;
}

__device__ __forceinline__ int wrap1023(int i)   // i < 3 * 1023
{
  i = i >= 2 * kChips ? i - 2 * kChips : i;
  return i >= kChips ? i - kChips : i;
}

// bits [pos, pos + 9) of a plane
__device__ __forceinline__ u32 plane_bits9(const u32 *pl, int pos)
{
  return __builtin_amdgcn_alignbit(pl[(pos >> 5) + 1], pl[pos >> 5], (u32)(pos & 31)) & 0x1FFu;
}

// ---- per cluster: decode, the PRN set's tables -------------------------------------------------------------------------------
// cluster = (search, Doppler bin, set of 32 PRN slots), the set running fastest
struct MxCluster {
  int set, sd, dopp, search;
};
__device__ __forceinline__ MxCluster mx_decode_cluster(int cluster, int n_sets, int n_dopp)
{
  const int set = cluster % n_sets, sd = cluster / n_sets;
  return MxCluster{set, sd, sd % n_dopp, sd / n_dopp};
}
// the carrier NCO's step per 32-sample word in Doppler bin `dopp`
__device__ __forceinline__ u32 mx_step_word(int dopp, int if_hz, int dopp_min_hz, int dopp_step_hz)
{
  const float freq_hz = (float)(if_hz + dopp_min_hz + dopp * dopp_step_hz);   // PM/GPS/acquisition.c:285-289
  return nco_step_per_word(freq_hz);
}
// mx_a [set][16][2][32][4] -> the A fragments (all the weighted kernels read of the tables); with mx_t [set][1032] -> chip_t
__device__ __forceinline__ void mx_load_chips_a(MxSharedCore &sh, const u32 *__restrict__ mx_a, int set, int tid)
{
  const u32 *src_a = mx_a + (size_t)set * (16 * 2 * 32 * 4);
  u32 *dst_a = reinterpret_cast<u32 *>(&sh.chips_a[0][0][0]);
  for (int i = tid; i < 16 * 2 * 32 * 4; i += kMxThreads)
    dst_a[i] = src_a[i];
}
__device__ __forceinline__ void mx_load_tables(MxSharedCore &sh, const u32 *__restrict__ mx_a, const u32 *__restrict__ mx_t, int set, int tid)
{
  mx_load_chips_a(sh, mx_a, set, tid);
  const u32 *src_t = mx_t + (size_t)set * 1032;
  for (int i = tid; i < 1032; i += kMxThreads)
    sh.chip_t[i] = src_t[i];
}

// ---- per block: capture -> LDS, wipe-off, polyphase planes -------------------------------------------------------------
// (in two parts: the block's load goes out together with the cluster's tables -- one global-memory latency, not two)
__device__ __forceinline__ void mx_load_block(MxSharedCore &sh, const uint8_t *blk, int if_format, int tid)
{
  for (int i = tid; i < 1024; i += kMxThreads)
    sh.x[i] = i < kWords16 ? load_sign16(blk, i, if_format) : (uint16_t)0;
  if (tid < 2)
    sh.ones[tid] = 0;
}
// the wipe-off and the wrap word: all that the vectors of sample offset 0 (and a direct start's) read of a block
// WRAP_IN_PLACE: the thread of word 511 makes the wrap word itself, from the stream's word 0 as it recomputes it (the NCO's
// phase at word 0 is 0) -- no barrier and no second step for it; the caller's next barrier publishes everything
template <bool WRAP_IN_PLACE = false>
__device__ __forceinline__ void mx_wipe_stream(MxSharedCore &sh, u32 step_word, int tid, int lane)
{
  {
    const u32 *x32 = reinterpret_cast<const u32 *>(sh.x);
    u32 ones_i = 0, ones_q = 0;
    for (int w = tid; w < 514; w += kMxThreads) {
      u32 vi = 0, vq = 0;
      if (w < kWords32) {
        const u32 quad = (step_word * (u32)w) >> 30;
        vi = carrier_i(quad) ^ x32[w];
        vq = carrier_q(quad) ^ x32[w];
      }
      ones_i += __popc(vi);
      ones_q += __popc(vq);
      if (WRAP_IN_PLACE && w == 511) {   // samples 16352..16367 are zero, then the stream wraps to sample 0
        vi = (carrier_i(0u) ^ x32[0]) << 16;
        vq = (carrier_q(0u) ^ x32[0]) << 16;
      }
      sh.d[0][w] = vi;
      sh.d[1][w] = vq;
    }
    ones_i = wave_sum_to_lane63(ones_i);   // (DPP: no lane-address constants to keep in -- or spill from -- registers)
    ones_q = wave_sum_to_lane63(ones_q);
    if (lane == 63) {
      atomicAdd(&sh.ones[0], ones_i);
      atomicAdd(&sh.ones[1], ones_q);
    }
  }
  if constexpr (!WRAP_IN_PLACE) {
    __syncthreads();
    if (tid < 2)
      sh.d[tid][511] = sh.d[tid][0] << 16;   // samples 16352..16367 are zero, then the stream wraps to sample 0
    // (the caller's next barrier publishes the wrap word)
  }
}
// word w >= 32 of a circularly extended plane: the 32 bits from position 32 w mod 1023 of the 1023-bit period in words 0..31
__device__ __forceinline__ u32 mx_plane_ext_word(const u32 *pl, int w)
{
  const int pos = 32 * w - (w >= 64 ? 2 * kChips : kChips);
  const int lo = pos >> 5;
  u32 v = __builtin_amdgcn_alignbit(lo < 31 ? pl[lo + 1] : 0u, pl[lo], (u32)(pos & 31));
  if (pos + 32 > kChips) {   // the period ends inside the word: its first bits follow
    const int k = kChips - pos;
    v = (v & ((1u << k) - 1u)) | (pl[0] << k);
  }
  return v;
}
__device__ void mx_wipe_block(MxShared &sh, u32 step_word, int tid, int lane)
{
  mx_wipe_stream(sh, step_word, tid, lane);
  __syncthreads();
  // plane[iq][t0] bit i = D(16 (i mod 1023) + t0), i < 2112.  First period: word w of offset t0 takes bit t0 and bit 16 + t0
  // of the stream words 16 w .. 16 w + 15 (bit 1023 = D(16368 + t0) is the wrap-around copy in word 511: D(t0), as it has
  // to be); the 16 threads of a word read the same 16 addresses (LDS broadcast).
  for (int m = tid; m < 2 * 32 * 16; m += kMxThreads) {
    const int t0 = m & 15, w = (m >> 4) & 31, iq = m >> 9;
    const u32 *src = &sh.d[iq][16 * w];
    u32 bits = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) {
      const u32 sk = src[k];
      bits |= ((sk >> t0) & 1u) << (2 * k);
      bits |= ((sk >> (16 + t0)) & 1u) << (2 * k + 1);
    }
    sh.plane[iq][t0][w] = bits;
  }
  __syncthreads();
  // circular extension: word w >= 32 = the 32 bits from position 32 w mod 1023 of the 1023-bit period
  for (int m = tid; m < 2 * 16 * (kPlaneWordsMx - 32); m += kMxThreads) {
    const int w = 32 + m % (kPlaneWordsMx - 32);
    const int r = m / (kPlaneWordsMx - 32);
    sh.plane[r >> 4][r & 15][w] = mx_plane_ext_word(sh.plane[r >> 4][r & 15], w);
  }
  // (the caller's next barrier publishes the planes)
}

// FP4 (E2M1) code of a small integer: 0, +-1, +-2, +-3, +-4 (and 6)
__device__ __forceinline__ u32 fp4_code(int v)
{
  const u32 m = (u32)(v < 0 ? -v : v);
  return ((0x0765420u >> (4u * (m > 5u ? 5u : m))) & 0xFu) | (v < 0 ? 8u : 0u);   // |v|: 0 1 2 3 4 6 -> 0 2 4 5 6 7
}

// The vector builders' lookup tables (once per workgroup): what they replace is the bit -> nibble spreading, a dozen
// vector instructions per dword of the vectors -- and the vectors are built once per sample offset next to the MFMA passes,
// by waves that have better things to do.
__device__ void mx_fill_tables(MxSharedCore &sh, int tid, int nthreads = kMxThreads)
{
  for (int w = tid; w < 512; w += nthreads) {
    const u32 cur = (u32)w & 0xFFu, nxt = ((u32)w >> 1) & 0xFFu;
    const u32 plus = spread8(nxt & ~cur), minus = spread8(cur & ~nxt);   // e = +1 -> -2 (code C), e = -1 -> +2 (code 4)
    sh.t_lut[w] = (plus << 2) | (plus << 3) | (minus << 2);
  }
  for (int x = tid; x < 256; x += nthreads)
    sh.t_lut[512 + x] = (spread8((u32)x) << 1) | (spread8(~(u32)x & 0xFFu) * 0xAu);   // +1 -> code 2, -1 -> code A
}

// ---- per pass: the nibble vector, copy 0 (phase 1), then its eight shifted copies (phase 2) --------------------------------
// pass 0: -2 (S_0 & 3), pass 1: -(S_0 >> 2) at scale 2^3, pass p >= 2 (producing sample offset t0 = p - 1 from plane
// p - 2): -2 e_{p-2}, plus the wrap-word impulses when t0 is 9..15; and the byte vectors of the extra K step.
__device__ void mx_vector_phase1(MxShared &sh, int pass, int buf, int tid)
{
  const int t0 = pass - 1;
  // nibbles 0 .. 2055 are ever read (dword 4 * 62 + 3 + 3 of copy 7): 258 dwords of copy 0; then the 2 x 128 dword pairs of
  // the extra K step
  for (int m = tid; m < 2 * kVecDwords + 2 * 128; m += kMxThreads) {
    if (m < 2 * kVecDwords) {
      const int iq = m >= kVecDwords, dw = m - iq * kVecDwords;
      u32 packed = 0;
      if (pass < 2) {
        const u32 *dd = sh.d[iq];
#pragma unroll
        for (int e = 0; e < 8; e++) {
          const int k = wrap1023(8 * dw + e);
          const int pos = 16 * k;
          const u32 sum = pop16(__builtin_amdgcn_alignbit(dd[(pos >> 5) + 1], dd[pos >> 5], (u32)(pos & 31)));
          // pass 0: -2 (S & 3) = 0, -2, -4, -6 -> codes 0, C, E, F;  pass 1: -(S >> 2) = 0 .. -4 -> codes 0, A, C, D, E
          const u32 code = pass == 0 ? (0xFEC0u >> (4u * (sum & 3u))) & 0xFu : (0xEDCA0u >> (4u * (sum >> 2))) & 0xFu;
          packed |= code << (4 * e);
        }
      } else {
        const u32 w = plane_bits9(sh.plane[iq][pass - 2], 8 * dw);
        packed = sh.t_lut[w];
        if (dw == 127 && t0 >= 9) {
          // entries 1021 / 1022 (nibbles 5 / 6 of this dword, first period only): the skipped wrap word's coefficients
          // alpha_b = b on chip 1021 - q and beta_b = const - b on chip 1022 - q move by +1 / -1 per step; they are
          // subtracted from the count: -1 / +1 here
          const u32 cur = w & 0xFFu, nxt = (w >> 1) & 0xFFu;
          const int e5 = (int)((nxt >> 5) & 1u) - (int)((cur >> 5) & 1u), e6 = (int)((nxt >> 6) & 1u) - (int)((cur >> 6) & 1u);
          packed = (packed & ~0x0FF00000u) | (fp4_code(-2 * e5 - 1) << 20) | (fp4_code(-2 * e6 + 1) << 24);
        }
      }
      sh.base[iq][dw] = packed;
    } else {
      // extra K step: deltas of  c1022 * A'(q)  and  c1021 * B'(q)  (see mx_half_switch for the terms themselves), eight
      // chip offsets per dword:
      //   t0 = 1..7, 9..15:  A_b = 2 pop(byte_o & low_b) - b grows by 2 D(8 o + b) - 1 = 2 d[q] - 1
      //   t0 = 9..15, q > 0: the tail word (o - 2, o - 1) of odd offsets, whose bit b is d[q - 1]: A' += 1 - 2 d[q - 1]
      //                      (together 2 (d[q] - d[q - 1])), B' grows by 2 d[q - 1] - 1
      const int mm = m - 2 * kVecDwords;
      const int iq = mm >> 7, dw = mm & 127;
      u32 ca = 0, cb = 0;
      if (pass >= 2 && t0 != 8) {
        const u32 *pl = sh.plane[iq][pass - 2];
        // bits 8 dw - 1 .. 8 dw + 7 of the plane (bit -1 = 0): d[q] = bit k + 1, d[q - 1] = bit k for the eight q of this dword
        const u32 w = dw ? plane_bits9(pl, 8 * dw - 1) : (pl[0] << 1) & 0x1FFu;
        const u32 exist = dw == 127 ? 0x0FFFFFFFu : 0xFFFFFFFFu;   // q = 1023 does not exist
        if (t0 < 8) {
          ca = sh.t_lut[512 + (w >> 1)] & exist;
        } else {
          const u32 diff = sh.t_lut[w];                             // -2 (d - dm)
          ca = (diff ^ ((diff & 0x44444444u) << 1)) & exist;        // 2 (d - dm): the sign bit of the non-zero codes flips
          cb = sh.t_lut[512 + (w & 0xFFu)] & exist;                     // 2 dm - 1
          if (dw == 0) {                                            // q = 0 has no tail word: A' grows by 2 d - 1, B' stays
            ca = (ca & ~0xFu) | ((w & 2u) ? 0x2u : 0xAu);
            cb &= ~0xFu;
          }
        }
      }
      sh.corr[buf][iq][0][dw] = ca;
      sh.corr[buf][iq][1][dw] = cb;
    }
  }
}

__device__ void mx_vector_phase2(MxShared &sh, int buf, int tid)
{
  for (int m = tid; m < 2 * 256; m += kMxThreads) {
    const int iq = m >> 8, j = m & 255;
    const u32 lo = sh.base[iq][j], hi = sh.base[iq][j + 1];
#pragma unroll
    for (int c = 0; c < 8; c++)
      sh.e8[buf][iq][c][j] = c ? __builtin_amdgcn_alignbit(hi, lo, 4u * (u32)c) : lo;
  }
}

// ---- one MFMA pass: acc[stream][tile] += chips x Toeplitz(vector) -------------------------------------------------------
typedef __attribute__((address_space(3))) const u32 lds_cu32;

// an LDS address the compiler cannot see through: what is added to it afterwards are small constants that fit the DS
// instructions' offset fields (left alone it rebuilds "variable part + offset of the array in the LDS block + 32 s" with a
// v_add per load: the array's offset does not fit the 8-bit dword offsets of ds_read2_b32)
__device__ __forceinline__ lds_cu32 *lds_opaque(const u32 *p)
{
  u32 a = (u32)(size_t)(lds_cu32 *)p;
  asm volatile("" : "+v"(a));
  return (lds_cu32 *)(size_t)a;
}
__device__ __forceinline__ v4i lds_frag(lds_cu32 *w, int dw)   // four dwords, dword aligned only
{
  return v4i{(int)w[dw], (int)w[dw + 1], (int)w[dw + 2], (int)w[dw + 3]};
}

// ---- the vector of pass p_vec >= 2 in one phase ------------------------------------------------------------------------
// Same values as mx_vector_phase1 + phase2 (which build the first two vectors, before the loop), without the copy-0 round
// trip through LDS: thread (stream, j) looks up dwords j and j + 1 of copy 0 itself and writes dword j of the eight shifted
// copies; thread (stream, term, dw) one dword of the extra K step's vectors.  512 threads, three dependent LDS accesses.
// dword 127 of a vector, sample offsets 9..15: the wrap word's impulses at entries 1021 / 1022 (see mx_vector_phase1)
__device__ __forceinline__ u32 mx_patch_wrap(u32 packed, u32 w9, bool patch)
{
  const u32 i5 = 1u + ((w9 >> 6) & 1u) - ((w9 >> 5) & 1u), i6 = 1u + ((w9 >> 7) & 1u) - ((w9 >> 6) & 1u);   // e + 1
  const u32 c5 = (0xDA2u >> (4u * i5)) & 0xFu;   // -2 e - 1 = 1, -1, -3 -> codes 2, A, D
  const u32 c6 = (0xA25u >> (4u * i6)) & 0xFu;   // -2 e + 1 = 3, 1, -1 -> codes 5, 2, A
  const u32 patched = (packed & ~0x0FF00000u) | (c5 << 20) | (c6 << 24);
  return patch ? patched : packed;
}

// FOLD (the single-block form): in place of the extra K step's vectors thread (stream, j) writes the code pairs of chip offsets
// 4 j .. 4 j + 3 (MxFold): one table look-up by the five plane bits they depend on; q = 0 and q = 1 of sample offsets 9..15 have
// pairs of their own.  (Sample offset 8, the half switch: its pass reads no pairs.)
template <bool FOLD = false>
__device__ __forceinline__ void mx_vector_build(MxSharedCore &sh, int p_vec, int tid, MxFold *fold = nullptr)
{
  const int t0 = p_vec - 1, buf = p_vec & 1;
  const bool late = t0 >= 9;
  const int iq = tid >> 8, j = tid & 255, which = (tid >> 7) & 1, dwc = tid & 127;
  const u32 *pl = sh.plane[iq][p_vec - 2];
  // 17 plane bits from 8 j: the 9-bit windows of dwords j and j + 1
  const u32 x = __builtin_amdgcn_alignbit(pl[(j >> 2) + 1], pl[j >> 2], 8u * (u32)(j & 3));
  u32 cw = 0, v = 0;
  if constexpr (!FOLD) {
    // bits 8 dwc - 1 .. 8 dwc + 7 (bit -1 = 0) for the extra K step: d[q] = bit k + 1, d[q - 1] = bit k of the dword's eight q
    const int pos = dwc ? 8 * dwc - 1 : 0;
    const u32 y = __builtin_amdgcn_alignbit(pl[(pos >> 5) + 1], pl[pos >> 5], (u32)(pos & 31));
    cw = (dwc ? y : y << 1) & 0x1FFu;
  }
  u32 lo = sh.t_lut[x & 0x1FFu], hi = sh.t_lut[(x >> 8) & 0x1FFu];
  // term 0: A' deltas: 2 d - 1 before the half switch, 2 (d - dm) after it; term 1: B' deltas 2 dm - 1 (after it only)
  if constexpr (!FOLD)
    v = sh.t_lut[which ? 512u + (cw & 0xFFu) : (late ? cw : 512u + (cw >> 1))];
  if (late) {
    lo = mx_patch_wrap(lo, x & 0x1FFu, j == 127);
    hi = mx_patch_wrap(hi, (x >> 8) & 0x1FFu, j == 126);
    if constexpr (!FOLD) {
      if (which == 0)
        v ^= (v & 0x44444444u) << 1;                       // -2 (d - dm) -> 2 (d - dm): the sign of the non-zero codes
      if (dwc == 0)                                        // q = 0 has no tail word: A' grows by 2 d - 1, B' stays
        v = (v & ~0xFu) | (which ? 0u : ((cw & 2u) ? 0x2u : 0xAu));
    }
  }
  if constexpr (!FOLD) {
    v &= dwc == 127 ? 0x0FFFFFFFu : 0xFFFFFFFFu;           // q = 1023 does not exist
    if ((which && !late) || t0 == 8)
      v = 0;
    sh.corr[buf][iq][which][dwc] = v;
  } else {
    // plane bits 4 j - 2 .. 4 j + 2, from the circular extension (at + 1023): bits i and i + 1 are d[q - 2] and d[q - 1] of
    // q = 4 j + i.  (q = 1023 does not exist: its pair meets an accumulator that clips to zero whatever is added.)
    const int pos = 4 * j + kChips - 2;
    const u32 z = __builtin_amdgcn_alignbit(pl[(pos >> 5) + 1], pl[pos >> 5], (u32)(pos & 31)) & 31u;
    v4i pr = fold->lut[late][z];
    if (late && j == 0) {
      pr.x = (int)(gpsx_fold_pair(true, 0, (int)(z & 1u), (int)((z >> 1) & 1u)) << kGpsxFoldShift);
      pr.y = (int)(gpsx_fold_pair(true, 1, (int)((z >> 1) & 1u), (int)((z >> 2) & 1u)) << kGpsxFoldShift);
    }
    *reinterpret_cast<v4i *>(&fold->pair[buf][iq][4 * j]) = pr;
  }
  u32 *dst = &sh.e8[buf][iq][0][j];
#pragma unroll
  for (int c = 0; c < 8; c++)
    dst[c * kCopyDwords] = c ? __builtin_amdgcn_alignbit(hi, lo, 4u * (u32)c) : lo;
}

// One anti-diagonal of a pass (fragment Q0 + 2 S): request the fragments of the next one, then the MFMAs of this one.
// The sched_group_barriers pin that order -- the DS reads first, (8 MFMAs = 260 cycles ahead of their use) -- which the
// scheduler, short of registers, would otherwise turn into "requested one MFMA before the wait": the LDS is kept busy by
// the four waves of the other role, a wave that waits for it at every step loses a third of the matrix pipe's time.
//
// FOLD (the single-block form, MxFold): chips 992..1023 -- kappa = 15, lane half 1 -- sit in the fragment of steps S = 15..18, where
// tile S - 15 alone is at kappa = 15.  Its MFMAs go last in the step, and in front of them the lane's code pair of that tile
// (requested a step ahead, with the fragments) replaces bits 20..27 of the fragment's fourth dword in place: one v_bfi_b32 per
// stream, issued under the other tiles' MFMAs.  mask = 0 (lane half 0; a pass without quirk terms) leaves the dword as it is.
struct MxFoldRegs {
  lds_cu32 *w;                           // pair[buffer][0][q of tile 0]: tile j at + 64 j, the Q stream at + 1024
  u32 mask, pi, pq;
};
// One MFMA of a pass: chips x fragment.  TR (the single-block form, gpsx_mx_transposed.hpp): the fragment is the A operand and the
// chips are B, each block scale with its operand -- the same registers, the tile transposed: chip offsets in the rows, one PRN per lane.
template <bool TR, u32 SCALE_C>
__device__ __forceinline__ v16f mx_mfma(v4i chips, v4i frag, v16f acc, u32 scale_f)
{
  if constexpr (TR)
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(widen(frag), widen(chips), acc, 4, 4, 0, scale_f, 0, SCALE_C);
  else
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(widen(chips), widen(frag), acc, 4, 4, 0, SCALE_C, 0, scale_f);
}
// (FOLD is the single-block form's instantiation, and the transposed one; RES: a[] is MxChipRegs::k, filled for kappa < RES)
template <int S, int NT, u32 SCALE_A = kScaleA, bool FOLD = false, int RES = 0>
__device__ __forceinline__ void mx_pass_step(lds_cu32 *wi, lds_cu32 *wq, const v4i *ca, v4i (&a)[16], v4i &fi, v4i &fq,
                                             v16f (&acc)[2][NT], u32 scale_b, MxFoldRegs *fold = nullptr)
{
  constexpr int kSteps = 16 + NT - 1;
  constexpr bool more = S + 1 < kSteps;
  constexpr bool pair_next = FOLD && more && S + 1 >= 15, patched = FOLD && S >= 15;
  constexpr bool chips_next = more && S + 1 < 16 && S + 1 >= RES;
  v4i fi_next = fi, fq_next = fq;
  u32 pi_next = 0, pq_next = 0;
  if constexpr (more) {
    fi_next = lds_frag(wi, 8 * (S + 1));
    fq_next = lds_frag(wq, 8 * (S + 1));
    if constexpr (chips_next)
      a[S + 1] = ca[(S + 1) * 64];                         // chips_a[S + 1][h][n]
    if constexpr (pair_next) {
      pi_next = fold->w[64 * (S + 1 - 15)];
      pq_next = fold->w[64 * (S + 1 - 15) + 1024];
    }
  }
  constexpr int j_lo = S - 15 > 0 ? S - 15 : 0, j_hi = S < NT - 1 ? S : NT - 1;
#pragma unroll
  for (int j = j_lo + (patched ? 1 : 0); j <= j_hi; j++) {
    acc[0][j] = mx_mfma<FOLD, SCALE_A>(a[S - j], fi, acc[0][j], scale_b);
    acc[1][j] = mx_mfma<FOLD, SCALE_A>(a[S - j], fq, acc[1][j], scale_b);
  }
  if constexpr (patched) {
    fi.w = (int)((fold->mask & fold->pi) | (~fold->mask & (u32)fi.w));
    fq.w = (int)((fold->mask & fold->pq) | (~fold->mask & (u32)fq.w));
    acc[0][j_lo] = mx_mfma<FOLD, SCALE_A>(a[15], fi, acc[0][j_lo], scale_b);
    acc[1][j_lo] = mx_mfma<FOLD, SCALE_A>(a[15], fq, acc[1][j_lo], scale_b);
  }
  if constexpr (more) {
    __builtin_amdgcn_sched_group_barrier(0x100, (chips_next ? 5 : 4) + (pair_next ? 2 : 0), 0);   // DS reads
    if constexpr (patched) {
      __builtin_amdgcn_sched_group_barrier(0x008, 2 * (j_hi - j_lo), 0);    // MFMAs of the tiles below kappa = 15
      __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);                    // the two patches
      __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);                    // MFMAs of tile S - 15
    } else {
      __builtin_amdgcn_sched_group_barrier(0x008, 2 * (j_hi - j_lo + 1), 0);   // MFMAs
    }
  }
  __builtin_amdgcn_sched_barrier(0);
  fi = fi_next;
  fq = fq_next;
  if constexpr (FOLD) {
    fold->pi = pi_next;
    fold->pq = pq_next;
  }
  if constexpr (more)
    mx_pass_step<S + 1, NT, SCALE_A, FOLD, RES>(wi, wq, ca, a, fi, fq, acc, scale_b, fold);
}

// The same without a second set of fragment registers (the walk forms, whose prefetched sums leave none): the I fragment of the
// next anti-diagonal is requested INTO the registers of this one's as soon as its MFMAs have been issued, under the Q stream's
// MFMAs, the Q fragment under the next step's I MFMAs -- four MFMAs (130 cycles) of cover each instead of eight; the A fragment
// (registers of its own) a whole step ahead.
template <int S, int NT>
__device__ __forceinline__ void mx_pass_step_inplace(lds_cu32 *wi, lds_cu32 *wq, const v4i *ca, v4i (&a)[16], v4i &fi, v4i &fq,
                                                     v16f (&acc)[2][NT], u32 scale_b)
{
  constexpr int kSteps = 16 + NT - 1;
  constexpr bool more = S + 1 < kSteps;
  if constexpr (more && S + 1 < 16)
    a[S + 1] = ca[(S + 1) * 64];                           // chips_a[S + 1][h][n]
  constexpr int j_lo = S - 15 > 0 ? S - 15 : 0, j_hi = S < NT - 1 ? S : NT - 1;
#pragma unroll
  for (int j = j_lo; j <= j_hi; j++)
    acc[0][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(widen(a[S - j]), widen(fi), acc[0][j], 4, 4, 0, kScaleA, 0, scale_b);
  if constexpr (more)
    fi = lds_frag(wi, 8 * (S + 1));
#pragma unroll
  for (int j = j_lo; j <= j_hi; j++)
    acc[1][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(widen(a[S - j]), widen(fq), acc[1][j], 4, 4, 0, kScaleA, 0, scale_b);
  if constexpr (more)
    fq = lds_frag(wq, 8 * (S + 1));
  if constexpr (more) {
    if constexpr (S + 1 < 16)
      __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                 // DS read: the A fragment
    __builtin_amdgcn_sched_group_barrier(0x008, j_hi - j_lo + 1, 0);     // MFMAs, I
    __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);                   // DS reads: the next I fragment
    __builtin_amdgcn_sched_group_barrier(0x008, j_hi - j_lo + 1, 0);     // MFMAs, Q
    __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);                   // DS reads: the next Q fragment
  }
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (more)
    mx_pass_step_inplace<S + 1, NT>(wi, wq, ca, a, fi, fq, acc, scale_b);
}

// AHEAD = false (the walk forms): mx_pass_step_inplace
// NT = q-tiles of this call (q0_tile + 2 j, j < NT): four everywhere but in the byte-phase form, which works in tile pairs
// SCALE_A: the A operand's block scale (the weighted extension keeps plain integers in its accumulators: 2^0; AHEAD only)
// FOLD: no extra K step; with_corr says whether the pairs of fold_pair (MxFold::pair[buf]) are patched in (mx_pass_step)
// RES > 0 (the single-block form): the steps' a[] is chips->k, filled for kappa < RES; the pass reads the others from LDS as it goes
template <bool AHEAD, int NT, u32 SCALE_A = kScaleA, bool FOLD = false, int RES = 0>
__device__ __forceinline__ void mx_pass(const MxSharedCore &sh, int buf, int lane, int q0_tile, v16f (&acc)[2][NT],
                                        u32 scale_b, v4i a_corr, bool with_corr, const u32 *fold_pair = nullptr,
                                        MxChipRegs *chips = nullptr)
{
  static_assert(!FOLD || (AHEAD && NT == kMxTiles), "the fold is the single-block form's");
  static_assert(RES == 0 || (FOLD && RES <= kMxChipsResident), "resident chips are the single-block form's");
  const int n = lane & 31, h = lane >> 5;
  const u32 *e8 = &sh.e8[buf][0][0][0];
  lds_cu32 *wi = lds_opaque(e8 + (n & 7) * kCopyDwords + 4 * (q0_tile + h) + (n >> 3));
  lds_cu32 *wq = lds_opaque(e8 + (8 + (n & 7)) * kCopyDwords + 4 * (q0_tile + h) + (n >> 3));
  const v4i *ca = &sh.chips_a[0][h][n];
  v4i a[16];
  if constexpr (AHEAD) {
    v4i fi = lds_frag(wi, 0), fq = lds_frag(wq, 0);
    if constexpr (RES == 0)
      a[0] = ca[0];
    if constexpr (FOLD) {
      MxFoldRegs fold{lds_opaque(fold_pair + 32 * q0_tile + n), h && with_corr ? kGpsxFoldMask : 0u, 0u, 0u};
      if constexpr (RES > 0)
        mx_pass_step<0, NT, SCALE_A, true, RES>(wi, wq, ca, chips->k, fi, fq, acc, scale_b, &fold);
      else
        mx_pass_step<0, NT, SCALE_A, true>(wi, wq, ca, a, fi, fq, acc, scale_b, &fold);
    } else {
      mx_pass_step<0, NT, SCALE_A>(wi, wq, ca, a, fi, fq, acc, scale_b);
    }
  } else {
    static_assert(SCALE_A == kScaleA, "the in-place walk is the sign-only grid's");
    v4i fi = lds_frag(wi, 0), fq = lds_frag(wq, 0);
    a[0] = ca[0];
    mx_pass_step_inplace<0, NT>(wi, wq, ca, a, fi, fq, acc, scale_b);
  }
  if (!FOLD && with_corr) {   // wave-uniform
    // the extra K step: only column 0 of each lane half of A is set (chip 1022 / chip 1021 of the PRN), so only the first
    // nibble of a lane's B window counts: the step's delta for (stream, term h, q)
    // (dword q >> 3 = 4 (q0_tile + 2 j) + n / 8 of the term's vector: one address, constant offsets per tile and stream)
    lds_cu32 *cw = lds_opaque(&sh.corr[buf][0][h][4 * q0_tile + (n >> 3)]);
#pragma unroll
    for (int j = 0; j < NT; j++) {
      // (nibble q & 7 of dword q >> 3 moved to nibble 0; what is left above it meets zero columns of A)
      const v4i gi = v4i{(int)(cw[8 * j] >> (4 * (n & 7))), 0, 0, 0};
      const v4i gq = v4i{(int)(cw[8 * j + 2 * 128] >> (4 * (n & 7))), 0, 0, 0};
      acc[0][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(widen(a_corr), widen(gi), acc[0][j], 4, 4, 0, kScaleA, 0,
                                                                   kScaleOne);
      acc[1][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(widen(a_corr), widen(gq), acc[1][j], 4, 4, 0, kScaleA, 0,
                                                                   kScaleOne);
    }
  }
}

// gps_correlation8's magnitude (PM/GPS/gps_misc.c:106-118) on the centred counts as the accumulators hold them (exact
// integers / 8192 in f32): one-sided clip and square in one instruction, the f32 sum of the two, the correctly rounded root
// (v_sqrt_f32 + the neighbour test, as mag8_fast), truncation.
__device__ __forceinline__ u32 root_trunc(float e);
// max(c, 0)^2 for |c| < 1 (and 0 for any c <= -1): c |c| clamped to [0, 1].  The product of the exact count with itself,
// rounded once: what (float)(I * I) is -- at 2^-26.
__device__ __forceinline__ float mx_clip_square(float c)
{
  // (v_mul_f32 c, |c| clamp: the median with 0 and 1 folds into the multiplication's clamp bit)
  return __builtin_amdgcn_fmed3f(c * __builtin_fabsf(c), 0.0f, 1.0f);
}
__device__ __forceinline__ float clip_square_sum(float ci, float cq)   // (I^2 + Q^2) / 2^26
{
  return mx_clip_square(ci) + mx_clip_square(cq);
}
__device__ __forceinline__ u32 mag8_f32(float ci, float cq)
{
  return root_trunc(clip_square_sum(ci, cq) * kUnscaleSq);
}

// (int) of the correctly rounded f32 root
__device__ __forceinline__ u32 root_trunc(float e)
{
  float r = __builtin_amdgcn_sqrtf(e);
  const float r_dn = __uint_as_float(__float_as_uint(r) - 1u);
  const float r_up = __uint_as_float(__float_as_uint(r) + 1u);
  const float res_dn = __builtin_fmaf(-r_dn, r, e);
  const float res_up = __builtin_fmaf(-r_up, r, e);
  r = res_dn <= 0.0f ? r_dn : r;
  r = res_up > 0.0f ? r_up : r;
  return (u32)(int)r;
}

// ---- the rounding mode of an epilogue ---------------------------------------------------------------------------------------
// The small-radius path wants floor(root) as an integer in the low mantissa bits of an f32: with the f32 rounding mode at
// "toward zero" that is ONE v_fma_f32 behind the root -- root * 2^13 (1 + 2^-22) + 2^23 -- where round-to-nearest took an add of
// 1/2 in front of the root (so that the approximate root of a square does not land below it) and an add of 2^23 - 1/2 behind
// it.  The factor is the guard: v_sqrt_f32 is good to one ulp (2^-23 relative), so root (1 + 2^-23) <= x <= root (1 + 1.5 *
// 2^-22), never below the true root, and below the next integer as long as 1.5 * 2^-22 < 1 / (2 (m + 1)^2): m + 1 < 1182, the
// small path ends at 1024.  Everything else on that path is exact in any mode (integers < 2^24 at a power-of-two scale).
// The exact path -- (float)(I * I), the f32 sum, the correctly rounded root -- is the reference's arithmetic and runs in
// round-to-nearest: it switches the mode back for its own instructions (its inputs and results go through the switching
// asm statements, so none of them can be scheduled outside the pair).  MODE.FP_ROUND[1:0]: 0 = nearest even, 3 = toward zero.
constexpr float kRootGuard = 8192.001953125f;   // 2^13 (1 + 2^-22): scaled root -> root, nudged up past v_sqrt_f32's ulp
__device__ __forceinline__ void mx_round_toward_zero()
{
  asm volatile("s_setreg_imm32_b32 hwreg(HW_REG_MODE, 0, 2), 3\n\ts_nop 1" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}
__device__ __forceinline__ void mx_round_to_nearest()
{
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_setreg_imm32_b32 hwreg(HW_REG_MODE, 0, 2), 0\n\ts_nop 1" ::: "memory");
}
// 0x4B000000 + floor(root of e * 2^26), e * 2^26 < 2^20 an integer; needs mx_round_toward_zero()
__device__ __forceinline__ u32 root_bits_small(float e)
{
  return __float_as_uint(__builtin_fmaf(__builtin_amdgcn_sqrtf(e), kRootGuard, 8388608.0f));
}
// the exact path of N hypotheses, in round-to-nearest whatever the mode around it
template <int N>
__device__ __forceinline__ void mx_roots_exact(float (&ci)[N], float (&cq)[N], u32 (&mag)[N])
{
  static_assert(N == 4 || N == 8, "group size");
  if constexpr (N == 8)
    asm volatile("s_setreg_imm32_b32 hwreg(HW_REG_MODE, 0, 2), 0\n\ts_nop 1"
                 : "+v"(ci[0]), "+v"(ci[1]), "+v"(ci[2]), "+v"(ci[3]), "+v"(ci[4]), "+v"(ci[5]), "+v"(ci[6]), "+v"(ci[7]),
                   "+v"(cq[0]), "+v"(cq[1]), "+v"(cq[2]), "+v"(cq[3]), "+v"(cq[4]), "+v"(cq[5]), "+v"(cq[6]), "+v"(cq[7]));
  else
    asm volatile("s_setreg_imm32_b32 hwreg(HW_REG_MODE, 0, 2), 0\n\ts_nop 1"
                 : "+v"(ci[0]), "+v"(ci[1]), "+v"(ci[2]), "+v"(ci[3]), "+v"(cq[0]), "+v"(cq[1]), "+v"(cq[2]), "+v"(cq[3]));
#pragma unroll
  for (int i = 0; i < N; i++)
    mag[i] = mag8_f32(ci[i], cq[i]);
  if constexpr (N == 8)
    asm volatile("s_setreg_imm32_b32 hwreg(HW_REG_MODE, 0, 2), 3\n\ts_nop 1"
                 : "+v"(mag[0]), "+v"(mag[1]), "+v"(mag[2]), "+v"(mag[3]), "+v"(mag[4]), "+v"(mag[5]), "+v"(mag[6]), "+v"(mag[7]));
  else
    asm volatile("s_setreg_imm32_b32 hwreg(HW_REG_MODE, 0, 2), 3\n\ts_nop 1"
                 : "+v"(mag[0]), "+v"(mag[1]), "+v"(mag[2]), "+v"(mag[3]));
}

constexpr float kOutside = -1048576.0f * kAccScale;   // start value (scaled) of hypotheses outside the search window: stays
                                                      // below -1, clips to 0

// Start of a block: every accumulator = the part of  cnt - 8184  that does not depend on the code (even byte offsets)
// (ones: pop(D) of the two streams -- sh.ones, or the other block's pair in the pipelined byte-phase form)
// (pass_bias: what the first offset's passes add beyond -2 M -- 0, or kGpsxAnchorPassBias for the one-pass anchor)
template <int NT>
__device__ __forceinline__ void mx_init_acc(const u32 *ones, int lane, int q0_tile, v16f (&acc)[2][NT], int win_start,
                                            int win_stop, int pass_bias = 0)
{
  const int n = lane & 31;
  const float base_i = (float)((int)ones[0] + 8192 - kHalf - pass_bias) * kAccScale,
              base_q = (float)((int)ones[1] + 8192 - kHalf - pass_bias) * kAccScale;
#pragma unroll
  for (int j = 0; j < NT; j++) {
    const int q = 32 * (q0_tile + 2 * j) + n;
    const int o = 2 * q;
    const bool in_win = q < kChips && o >= win_start && o < win_stop;
#pragma unroll
    for (int r = 0; r < 16; r++) {
      acc[0][j][r] = in_win ? base_i : base_i + kOutside;
      acc[1][j][r] = in_win ? base_q : base_q + kOutside;
    }
  }
}

// After the pass of sample offset 8 (the first odd byte offset, b = 0), before its epilogue: every quirk term jumps.
//   cnt = C0 + c1022 A_b(q)                                                                    even offsets o = 2 q
//   cnt = C0 + c1022 A_b(q) - [pop(W) + chip[1021 - q] alpha_b + chip[1022 - q] beta_b]        odd offsets o = 2 q + 1
//            - T(q) [pop(P) + c1021 (b - 2 pop(P & low_b)) + c1022 (16 - b - 2 pop(P & high_b))]
// A_b = 2 pop(byte_o & low_b) - b (quirk Q5); W = data bytes (2045, 0), the word at the wrap; P = data bytes (o - 2, o - 1),
// T = [q > 0]: the two replica words odd offsets skip (quirk Q3); alpha_b = b, beta_b = 16 - 2 pop(W) - b because the low
// byte of W (data byte 2045, never mixed) is zero.  At b = 0: A = 0, alpha = 0.
template <int NT>
__device__ __forceinline__ void mx_half_switch(const MxShared &sh, int lane, int q0_tile, v16f (&acc)[2][NT], int win_start,
                                               int win_stop)
{
  const int n = lane & 31, h = lane >> 5;
  const u32 *d_i = sh.d[0], *d_q = sh.d[1];
  const u32 wrap_i = (d_i[0] & 0xFFu) << 8, wrap_q = (d_q[0] & 0xFFu) << 8;
  const float beta0_i = (float)(16 - 2 * (int)__popc(wrap_i)) * kAccScale, beta0_q = (float)(16 - 2 * (int)__popc(wrap_q)) * kAccScale;
  const int popw_i = (int)__popc(wrap_i), popw_q = (int)__popc(wrap_q);
  const u32 f22 = sh.chip_t[1022 + 1] >> (4 * h);
#pragma unroll
  for (int j = 0; j < NT; j++) {
    const int q = 32 * (q0_tile + 2 * j) + n;
    const bool exists = q < kChips;
    const int qc = exists ? q : 0;
    const bool in0 = exists && 2 * q >= win_start && 2 * q < win_stop;
    const bool in1 = exists && 2 * q + 1 >= win_start && 2 * q + 1 < win_stop;
    // A_7 of the even offset goes, A_0 = 0 of the odd one comes
    int fa_i = -(2 * (int)__popc(lds_byte(d_i, 2 * qc) & 0x7Fu) - 7);
    int fa_q = -(2 * (int)__popc(lds_byte(d_q, 2 * qc) & 0x7Fu) - 7);
    int fk_i = -popw_i, fk_q = -popw_q;
    if (q > 0 && exists) {
      const u32 prev_i = lds_byte(d_i, 2 * qc - 1) | (lds_byte(d_i, 2 * qc) << 8);
      const u32 prev_q = lds_byte(d_q, 2 * qc - 1) | (lds_byte(d_q, 2 * qc) << 8);
      fk_i -= (int)__popc(prev_i);
      fk_q -= (int)__popc(prev_q);
      fa_i -= 16 - 2 * (int)__popc(prev_i);
      fa_q -= 16 - 2 * (int)__popc(prev_q);
    }
    float fkf_i = (float)fk_i * kAccScale, fkf_q = (float)fk_q * kAccScale;
    if (in0 != in1) {   // the window edge falls between the two byte offsets of this chip offset
      fkf_i += in1 ? -kOutside : kOutside;
      fkf_q += in1 ? -kOutside : kOutside;
    }
    const float faf_i = (float)fa_i * kAccScale, faf_q = (float)fa_q * kAccScale;
    const u32 w1 = sh.chip_t[(exists ? kChips - 1 - q : 0) + 1] >> (4 * h);   // chip 1022 - q of the lane's PRNs
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int pb = (r & 3) + 8 * (r >> 2);
      const float c22 = (float)((f22 >> pb) & 1u), c1 = (float)((w1 >> pb) & 1u);
      acc[0][j][r] += fkf_i + c22 * faf_i - c1 * beta0_i;
      acc[1][j][r] += fkf_q + c22 * faf_q - c1 * beta0_q;
    }
  }
}

// The single-block form's epilogue (n_ms == 1: what the headline sweep runs).  A wave that has its SIMD's vector ALU to
// itself issues an instruction every ~6.5 cycles whatever the instruction (tools/microbench/issue_mix.hip), so what counts
// here is their number: per hypothesis 2 clip-squares, 1 add, 5/8 for the group's radius test, the root of the scaled sum,
// 1 fma that (in round-toward-zero mode, root_bits_small) leaves floor(root) as an integer in the low mantissa bits, the
// key, and 1/2 + 1/2 for the running maximum and sum of its PRN (two tiles at a time: v_max3_u32 / v_add3_u32).
//   The f32 pattern of that fma is 0x4B000000 + floor(root): shifted left by 11 the exponent bits fall off the key; the
//   sums carry 0x4B000000 per term, four terms per PRN and sample offset: they start at -4 x 0x4B000000 (mod 2^32).
//   (Tried: taking the small path on trust and checking the best keys afterwards -- one test per 64 hypotheses, a second round
//   on the exact path for the PRN groups that show a radius >= 1024 -- saves the 5/8: 1 % faster on noise, 2.5 % slower
//   on the strong test signal, same-box A/B; not kept.  The transposed single-block form, where a lane is one PRN, does it per
//   wave with a predictor for the strong signal -- mxt_epilogue, k_acq_mx.hip: 7 instructions per hypothesis + 3 per lane and
//   sample offset on the trusted path, these 7 5/8 on its careful path.)
constexpr u32 kRootBias = 0x4B000000u;
template <int NT>
__device__ __forceinline__ void mx_epilogue_single(MxShared &sh, int lane, const u32 (&kq)[NT], int t0,
                                                   const v16f (&acc)[2][NT], int slots = -1)
{
  // (slots: which eighth of sh.part takes the results -- the bit shift's own, unless the pipelined byte-phase form says otherwise)
  const int n = lane & 31, h = lane >> 5;
  const int b = t0 & 7, half = t0 >> 3;
  u32 *slot = &sh.part[slots < 0 ? b : slots][4 * h][0][n];
  u32 best[16], total[16];
  // key = (magnitude << 11) | (2047 - byte offset), byte offset = 2 q + half: kq = 2047 - 2 q is the lane's own constant
  // (>= 1), the wave-uniform half comes off it here, once per tile
  u32 kqh[NT];
#pragma unroll
  for (int j = 0; j < NT; j++)
    kqh[j] = kq[j] - (u32)half;
#pragma unroll
  for (int r = 0; r < 16; r++) {
    best[r] = 0;
    total[r] = 0u - (u32)NT * kRootBias;   // (one biased term per tile and PRN)
  }
  mx_round_toward_zero();
#pragma unroll
  for (int jp = 0; jp < NT; jp += 2) {
#pragma unroll
    for (int r0 = 0; r0 < 16; r0 += 4) {
      // eight hypotheses: two tiles x four PRNs
      float ev[8];
      u32 e_max = 0;
#pragma unroll
      for (int i = 0; i < 8; i++) {
        ev[i] = clip_square_sum(acc[0][jp + (i >> 2)][r0 + (i & 3)], acc[1][jp + (i >> 2)][r0 + (i & 3)]);
        e_max = max(e_max, __float_as_uint(ev[i]));
      }
      const bool small = __builtin_amdgcn_ballot_w64(e_max >= 0x3C800000u /* 2^20 / 2^26 as f32 */) == 0;
      u32 bits[8];
      if (__builtin_expect(small, 1)) {
#pragma unroll
        for (int i = 0; i < 8; i++)
          bits[i] = root_bits_small(ev[i]);
      } else {
        float ci[8], cq[8];
#pragma unroll
        for (int i = 0; i < 8; i++) {
          ci[i] = acc[0][jp + (i >> 2)][r0 + (i & 3)];
          cq[i] = acc[1][jp + (i >> 2)][r0 + (i & 3)];
        }
        mx_roots_exact<8>(ci, cq, bits);
#pragma unroll
        for (int i = 0; i < 8; i++)
          bits[i] += kRootBias;
      }
#pragma unroll
      for (int rr = 0; rr < 4; rr++) {
        const int r = r0 + rr;
        const u32 k0 = (bits[rr] << 11) | kqh[jp], k1 = (bits[4 + rr] << 11) | kqh[jp + 1];
        best[r] = max(max(best[r], k0), k1);
        total[r] = total[r] + bits[rr] + bits[4 + rr];
      }
      // (pinned in program order: left alone, the compiler sinks all 64 chains to the end and spills)
#pragma unroll
      for (int rr = 0; rr < 4; rr++)
        asm volatile("" : "+v"(best[r0 + rr]), "+v"(total[r0 + rr]));
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  mx_round_to_nearest();
#pragma unroll
  for (int r = 0; r < 16; r++) {
    const int p_off = ((r & 3) + 8 * (r >> 2)) * 64;   // PRN (r & 3) + 8 (r >> 2) + 4 h: 2 x 32 words per PRN
    atomicMax(slot + p_off, best[r]);
    atomicAdd(slot + p_off + 32, total[r]);
  }
}

// max of a 64-bit value over the eight adjacent lanes of a PRN's bit shifts (quad permutes, then the mirrored half)
__device__ __forceinline__ unsigned long long mx_max8_u64(unsigned long long v)
{
  u32 lo = (u32)v, hi = (u32)(v >> 32);
#define MX_MAX8(ctrl)                                                                           \
  {                                                                                             \
    const u32 lo2 = (u32)__builtin_amdgcn_mov_dpp((int)lo, ctrl, 0xF, 0xF, true);               \
    const u32 hi2 = (u32)__builtin_amdgcn_mov_dpp((int)hi, ctrl, 0xF, 0xF, true);               \
    const bool g = hi2 > hi || (hi2 == hi && lo2 > lo);                                         \
    lo = g ? lo2 : lo;                                                                          \
    hi = g ? hi2 : hi;                                                                          \
  }
  MX_MAX8(0xB1)    // quad_perm [1, 0, 3, 2]
  MX_MAX8(0x4E)    // quad_perm [2, 3, 0, 1]
  MX_MAX8(0x141)   // row_half_mirror
#undef MX_MAX8
  return ((unsigned long long)hi << 32) | lo;
}

constexpr int kMxSingle = 0, kMxWalk = 1, kMxStore = 2, kMxWalk16 = 3, kMxByte = 4, kMxSplit = 5;   // k_acq_mx's MODE

}  // namespace

// One kernel per form; kMxByte is a specialisation in a file of its own (k_acq_mx_byte.hip), every other MODE the primary
// template (k_acq_mx.hip).
#define GPSX_K_ACQ_MX_PARAMS                                                                                                          \
  const AcqParams prm, int cluster_lo, const uint8_t *__restrict__ if_blocks, const u32 *__restrict__ mx_a,                             \
      const u32 *__restrict__ mx_t, gpsx_peak_t *__restrict__ peaks, u32 *__restrict__ energy, u32 *__restrict__ flags
template <int MODE>
__global__ __launch_bounds__(kMxThreads, 1) void k_acq_mx(GPSX_K_ACQ_MX_PARAMS);
template <>
__global__ __launch_bounds__(kMxThreads, 1) void k_acq_mx<kMxByte>(GPSX_K_ACQ_MX_PARAMS);
// (launch_acq_mx's AcqForm::kMxByte)
void launch_acq_mx_byte(hipStream_t s, unsigned grid, const AcqParams &prm, int cluster_lo, const uint8_t *d_if, const uint32_t *d_mx_a,
                        const uint32_t *d_mx_t);

}  // namespace gpsx
