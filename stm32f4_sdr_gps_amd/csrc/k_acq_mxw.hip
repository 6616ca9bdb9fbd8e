// k_acq_mxw.hip -- the weighted two-bit grids on the matrix cores: k_acq_mxw (one block) and k_acq_wmx_ms (n_ms blocks summed
// non-coherently), on the parts of the sign-only matrix-core grid (gpsx_mx_parts.hpp).
#include "gpsx_mx_parts.hpp"

namespace gpsx {

// =============================================================================================================================
// EXTENSION, not in the reference: the weighted two-bit grid (include/gpsx.h gpsx_acq_grid_weighted, k_acq_weighted.hip for the
// definition) on the matrix cores -- the same Toeplitz GEMM, with values where the sign-only grid has bits.
//   v(n) in {0, +-1, +-3}: the wiped sample's sign x its magnitude weight; the sixteen samples the carrier NCO never mixes: 0
//   I(16 q + t0) = sum_c s[c] S_t0[(q + c) mod 1023],  s = 1 - 2 chip,  S_t0[k] = sum of v over the window [16 k + t0, +16)
//                = T - 2 sum_c chip[c] S_t0[q + c],    T = sum of all v (every sample sits in exactly one window)
// A = chips (FP4 1.0, the tables of the sign-only grid, at block scale 2^0: the accumulators hold plain integers), start value T:
//   * sample offset 0 in THREE passes: y = -S_0 in [-48, 48] = y0 + 4 y1 + 16 y2 with balanced base-4 digits in [-2, 2]
//     (|y2| <= 3), the vector carries 2 y_i (FP4-exact: 0, +-2, +-4, +-6) at block scales 2^0, 2^2, 2^4;
//   * every further offset in one: S_{t0+1}[k] - S_t0[k] = v_t0(k + 1) - v_t0(k) in {0, +-1, +-2, +-3, +-4, +-6} (a difference
//     of 5 does not exist) with v_t0(i) = v(16 i + t0), i mod 1023, and v_t0(1022) = 0 (the unmixed samples, whatever t0):
//     the vector carries its negative at block scale 2^1.
// Every partial sum is an integer below 2^24 at a power-of-two scale: exact in f32 in any order, like the sign-only grid.
// The epilogue is this grid's own: no clipping (the correlation is signed), floor(sqrt(I^2 + Q^2)) exactly, the first fine phase
// reaching the maximum, the sum.  Work split, pipelining of the two roles and the result slots are k_acq_mx<0>'s.
namespace {

struct MxwShared {
  MxShared s;
  u32 mag[514];                     // the capture's magnitude plane, laid out as s.d (zero in the sign-only mode)
  u32 mplane[16][kPlaneWordsMx];    // polyphase magnitude planes, as s.plane
  int wsum[2];                      // sum over the mixed samples of (2 d - 1) m, per stream
};
constexpr int kWPasses = 18;                 // 3 for the first offset + 15 recurrence steps
constexpr u32 kScaleFour = 0x81818181u;      // 2^2
constexpr u32 kScaleSixteen = 0x83838383u;   // 2^4

__device__ __forceinline__ void mxw_write_copies(u32 *dst, u32 lo, u32 hi)
{
#pragma unroll
  for (int c = 0; c < 8; c++)
    dst[c * kCopyDwords] = c ? __builtin_amdgcn_alignbit(hi, lo, 4u * (u32)c) : lo;
}

// digit `which` of the first offset's chip sums (thread (stream, j): entries 8 j .. 8 j + 15 of copy 0 -> dword j of the copies)
__device__ __forceinline__ void mxw_build_start(MxwShared &shw, int which, int buf, int tid)
{
  const int iq = tid >> 8, j = tid & 255;
  const u32 *dd = shw.s.d[iq], *mm = shw.mag;
  u32 w2[2] = {0, 0};
#pragma unroll
  for (int e = 0; e < 16; e++) {
    const int k = wrap1023(8 * j + e);
    const u32 x = (dd[k >> 1] >> (16 * (k & 1))) & 0xFFFFu, m = (mm[k >> 1] >> (16 * (k & 1))) & 0xFFFFu;
    int y = -((2 * (int)__popc(x) - 16) + 2 * (2 * (int)__popc(x & m) - (int)__popc(m)));
    y = k == kChips - 1 ? 0 : y;                       // window 1022 = the sixteen unmixed samples
    const int y0 = ((y + 2) & 3) - 2, r1 = (y - y0) >> 2;
    const int y1 = ((r1 + 2) & 3) - 2, y2 = (r1 - y1) >> 2;
    const int digit = which == 0 ? y0 : which == 1 ? y1 : y2;
    w2[e >> 3] |= fp4_code(2 * digit) << (4 * (e & 7));
  }
  mxw_write_copies(&shw.s.e8[buf][iq][0][j], w2[0], w2[1]);
}

// the vector that takes the accumulators from sample offset t0 to t0 + 1: entry k = v_t0(k) - v_t0(k + 1).
// Lookup table (in the sign-only grid's t_lut, which this kernel does not use otherwise): (sign, magnitude) pairs of five
// consecutive samples -- ten bits, sample i in bits 2 i, 2 i + 1 -- -> the FP4 codes of their four differences
__device__ __forceinline__ int mxw_val2(u32 sm) { return ((sm & 1u) ? 1 : -1) * ((sm & 2u) ? 3 : 1); }
__device__ void mxw_fill_table(MxShared &sh, int tid)
{
  uint16_t *lut = reinterpret_cast<uint16_t *>(sh.t_lut);
  static_assert(sizeof(sh.t_lut) >= 1024 * sizeof(uint16_t), "difference table fits");
  for (int i = tid; i < 1024; i += kMxThreads) {
    u32 codes = 0;
#pragma unroll
    for (int k = 0; k < 4; k++)
      codes |= fp4_code(mxw_val2(((u32)i >> (2 * k)) & 3u) - mxw_val2(((u32)i >> (2 * k + 2)) & 3u)) << (4 * k);
    lut[i] = (uint16_t)codes;
  }
}
// 16 bits -> the even bit positions of 32
__device__ __forceinline__ u32 spread16(u32 x)
{
  x = (x | (x << 8)) & 0x00FF00FFu;
  x = (x | (x << 4)) & 0x0F0F0F0Fu;
  x = (x | (x << 2)) & 0x33333333u;
  return (x | (x << 1)) & 0x55555555u;
}
__device__ __forceinline__ void mxw_build_step(MxwShared &shw, int t0, int buf, int tid)
{
  const int iq = tid >> 8, j = tid & 255;
  const u32 *pl = shw.s.plane[iq][t0], *mp = shw.mplane[t0];
  const uint16_t *lut = reinterpret_cast<const uint16_t *>(shw.s.t_lut);
  const u32 sx = __builtin_amdgcn_alignbit(pl[(j >> 2) + 1], pl[j >> 2], 8u * (u32)(j & 3));   // plane bits 8 j .. 8 j + 31
  const u32 mx = __builtin_amdgcn_alignbit(mp[(j >> 2) + 1], mp[j >> 2], 8u * (u32)(j & 3));
  const u32 z_lo = spread16(sx & 0xFFFFu) | (spread16(mx & 0xFFFFu) << 1);                      // samples 0..15 of the window
  const u32 z_hi = ((sx >> 16) & 1u) | (((mx >> 16) & 1u) << 1);                                // sample 16
  u32 w2[2];
  w2[0] = (u32)lut[z_lo & 0x3FFu] | ((u32)lut[(z_lo >> 8) & 0x3FFu] << 16);
  w2[1] = (u32)lut[(z_lo >> 16) & 0x3FFu] | ((u32)lut[(z_lo >> 24) | ((z_hi & 3u) << 8)] << 16);
  // entries 1021, 1022 (dword 127, nibbles 5 and 6) and their wrap-around copies 2044, 2045 (dword 255, nibbles 4 and 5: 1023 is
  // odd) touch the unmixed samples, v(1022) = 0: they are v(1021) - 0 and 0 - v(0).  Every thread works the two codes out (four
  // broadcast reads) and patches by selection: a branch here put 300 instructions with dependent LDS reads on two waves' paths
  {
    const u32 c1 = fp4_code(mxw_val2(((pl[31] >> 29) & 1u) | (((mp[31] >> 29) & 1u) << 1)));
    const u32 c2 = fp4_code(-mxw_val2((pl[0] & 1u) | ((mp[0] & 1u) << 1)));
    const u32 at127 = (c1 << 20) | (c2 << 24), at255 = (c1 << 16) | (c2 << 20);
#pragma unroll
    for (int k = 0; k < 2; k++) {
      const int dword = j + k;
      u32 w = w2[k];
      w = dword == 127 ? (w & ~0x0FF00000u) | at127 : w;
      w = dword == 255 ? (w & ~0x00FF0000u) | at255 : w;
      w2[k] = w;
    }
  }
  mxw_write_copies(&shw.s.e8[buf][iq][0][j], w2[0], w2[1]);
}

__device__ __forceinline__ u32 mxw_root_exact(int i, int q)
{
  const u64 e = (u64)((long long)i * i) + (u64)((long long)q * q);
  u64 r = (u64)__builtin_sqrt((double)e);
  r = r * r > e ? r - 1 : r;
  r = (r + 1) * (r + 1) <= e ? r + 1 : r;
  return (u32)r;
}

// floor(sqrt(E)) for E = I^2 + Q^2 < 2^24 - 2 (an integer, exact in f32), in eight instructions: v_sqrt_f32 is good to one ulp,
// at most 2^-12 below 4096, and sqrt(E + 2) - sqrt(E) = 2 / (sqrt(E + 2) + sqrt(E)) > 2^-12 there: the root of E + 2 as the
// hardware returns it is not below floor(sqrt(E)) =: r and stays below r + 2 -- its truncation is r or r + 1, and
// (E + 2) - (r + 1)^2 < 2 (exact) tells which.  The + 2 rides in the first multiply-add.
__device__ __forceinline__ u32 mxw_root_small(float fi, float fq)
{
  const float e2 = __builtin_fmaf(fi, fi, __builtin_fmaf(fq, fq, 2.0f));
  const u32 r = (u32)__builtin_amdgcn_sqrtf(e2);
  const float rf = (float)r;
  return __builtin_fmaf(-rf, rf, e2) < 2.0f ? r - 1u : r;
}

// the epilogue of sample offset t0: 64 hypotheses per lane into the slots of bit shift t0 & 7 (byte offset 2 q + (t0 >> 3))
template <bool ALL_SMALL>
__device__ __forceinline__ void mxw_epilogue_body(MxShared &sh, int lane, int q0_tile, int t0, const v16f (&acc)[2][kMxTiles],
                                                  const bool (&small)[kMxTiles])
{
  const int n = lane & 31, h = lane >> 5;
  u32 key_lo[kMxTiles];
#pragma unroll
  for (int j = 0; j < kMxTiles; j++)
    key_lo[j] = (u32)(2047 - (2 * (32 * (q0_tile + 2 * j) + n) + (t0 >> 3)));
  const bool last_exists = 32 * (q0_tile + 2 * (kMxTiles - 1)) + n < kChips;   // chip offset 1023 (tile 31, lane 31) does not exist
  u32 *slot = &sh.part[t0 & 7][4 * h][0][n];
  if constexpr (ALL_SMALL) {
    // two PRNs (eight hypotheses) at a time, stage by stage: eight independent instructions between dependent ones -- a vector
    // instruction behind the one it depends on waits out its latency, next to the other wave's MFMAs even longer
#pragma unroll
    for (int r = 0; r < 16; r += 2) {
      float e2[8], rf[8];
      u32 root[8];
#pragma unroll
      for (int i = 0; i < 8; i++)
        e2[i] = __builtin_fmaf(acc[1][i & 3][r + (i >> 2)], acc[1][i & 3][r + (i >> 2)], 2.0f);
#pragma unroll
      for (int i = 0; i < 8; i++)
        e2[i] = __builtin_fmaf(acc[0][i & 3][r + (i >> 2)], acc[0][i & 3][r + (i >> 2)], e2[i]);
#pragma unroll
      for (int i = 0; i < 8; i++)
        rf[i] = __builtin_amdgcn_sqrtf(e2[i]);
#pragma unroll
      for (int i = 0; i < 8; i++)
        root[i] = (u32)rf[i];
#pragma unroll
      for (int i = 0; i < 8; i++)
        rf[i] = (float)root[i];
#pragma unroll
      for (int i = 0; i < 8; i++)
        rf[i] = __builtin_fmaf(-rf[i], rf[i], e2[i]);
#pragma unroll
      for (int i = 0; i < 8; i++)
        root[i] = rf[i] < 2.0f ? root[i] - 1u : root[i];
      root[3] = last_exists ? root[3] : 0u;
      root[7] = last_exists ? root[7] : 0u;
      asm volatile("" : "+v"(root[0]), "+v"(root[1]), "+v"(root[2]), "+v"(root[3]), "+v"(root[4]), "+v"(root[5]), "+v"(root[6]), "+v"(root[7]));
#pragma unroll
      for (int k = 0; k < 2; k++) {
        u32 best = 0, total = 0;
#pragma unroll
        for (int j = 0; j < kMxTiles; j++) {
          const u32 key = (root[4 * k + j] << 11) | key_lo[j];
          best = key > best ? key : best;
          total += root[4 * k + j];
        }
        const int p = ((r + k) & 3) + 8 * ((r + k) >> 2);
        atomicMax(&slot[p * 64], best);
        atomicAdd(&slot[p * 64 + 32], total);
      }
    }
    return;
  }
#pragma unroll
  for (int r = 0; r < 16; r++) {
    u32 best = 0, total = 0;
#pragma unroll
    for (int j = 0; j < kMxTiles; j++) {
      const float fi = acc[0][j][r], fq = acc[1][j][r];     // (plain integers: the A operand's block scale is 2^0 here)
      u32 m;
      if (small[j])
        m = mxw_root_small(fi, fq);
      else
        m = mxw_root_exact((int)fi, (int)fq);
      if (j == kMxTiles - 1)
        m = last_exists ? m : 0u;
      const u32 key = (m << 11) | key_lo[j];
      best = key > best ? key : best;
      total += m;
    }
    const int p = (r & 3) + 8 * (r >> 2);              // PRN p + 4 h of the cluster
    atomicMax(&slot[p * 64], best);
    atomicAdd(&slot[p * 64 + 32], total);
  }
}
// max(m, |a|, |b|) in ONE instruction (the source modifiers of v_max3_f32; written out because fmaxf() on fabsf() compiles to a
// canonicalising v_max_f32 |x|, |x| per operand in front of the maximum: 3.5 instructions per pair instead of one)
__device__ __forceinline__ float mxw_max_abs(float m, float a, float b)
{
  asm("v_max3_f32 %0, |%1|, |%2|, %0" : "+v"(m) : "v"(a), "v"(b));
  return m;
}
__device__ __forceinline__ void mxw_epilogue(MxShared &sh, int lane, int q0_tile, int t0, const v16f (&acc)[2][kMxTiles])
{
  // (wave-uniform) every |I|, |Q| of the wave's 64 x 64 hypotheses below 2896: I^2 + Q^2 + 2 < 2^24 -- all but the tiles next to a
  // strong satellite's peak
  float lim[kMxTiles];
#pragma unroll
  for (int j = 0; j < kMxTiles; j++)
    lim[j] = 0.0f;
#pragma unroll
  for (int r = 0; r < 16; r++)
#pragma unroll
    for (int j = 0; j < kMxTiles; j++)   // (four independent chains)
      lim[j] = mxw_max_abs(lim[j], acc[0][j][r], acc[1][j][r]);
  const float top = __builtin_fmaxf(__builtin_fmaxf(lim[0], lim[1]), __builtin_fmaxf(lim[2], lim[3]));
  bool small[kMxTiles];
  if (__builtin_amdgcn_ballot_w64(top >= 2896.0f) == 0) {
    mxw_epilogue_body<true>(sh, lane, q0_tile, t0, acc, small);
  } else {
#pragma unroll
    for (int j = 0; j < kMxTiles; j++)
      small[j] = __builtin_amdgcn_ballot_w64(lim[j] >= 2896.0f) == 0;
    mxw_epilogue_body<false>(sh, lane, q0_tile, t0, acc, small);
  }
}

// a cluster's start, before its first block: the 32 PRNs' chips, the result slots zeroed, the difference table
__device__ __forceinline__ void mxw_cluster_start(MxShared &sh, const u32 *__restrict__ mx_a, int set, int tid)
{
  mx_load_chips_a(sh, mx_a, set, tid);
  for (int i = tid; i < 8 * 32 * 2 * 32 / 4; i += kMxThreads)
    reinterpret_cast<uint4 *>(&sh.part[0][0][0][0])[i] = make_uint4(0, 0, 0, 0);
  mxw_fill_table(sh, tid);
}

// one block into the workgroup: the two bit planes, the wipe-off, the magnitude planes, the streams' totals, the first two vectors
// (the preamble of every block, in both kernels); the caller's LDS writes before it are ordered by its first barrier
__device__ __forceinline__ void mxw_block_start(MxwShared &shw, const uint8_t *blk, int use_magnitude, u32 step_word, int tid, int lane)
{
  MxShared &sh = shw.s;
  mx_load_block(sh, blk, GPSX_IF_2BIT_SM, tid);
  for (int w = tid; w < 514; w += kMxThreads) {
    u32 m = 0;
    if (use_magnitude && w < 512) {
#pragma unroll
      for (int hh = 0; hh < 2; hh++) {
        const int w16 = 2 * w + hh;
        if (w16 < kWords16) {
          const uint16_t *p = reinterpret_cast<const uint16_t *>(blk) + 2 * w16;
          m |= even_bits16(((u32)p[0] | ((u32)p[1] << 16)) >> 1) << (16 * hh);
        }
      }
    }
    shw.mag[w] = m;
  }
  if (tid < 2)
    shw.wsum[tid] = 0;
  __syncthreads();
  if (tid == 0)
    shw.mag[511] |= shw.mag[0] << 16;                    // the stream wraps to sample 0 (as s.d's word 511)
  mx_wipe_block(sh, step_word, tid, lane);
  // ---- magnitude planes (first period), the weighted part of the streams' totals, the first two vectors -----------------------
  for (int m = tid; m < 32 * 16; m += kMxThreads) {
    const int t0 = m & 15, w = m >> 4;
    const u32 *src = &shw.mag[16 * w];
    u32 bits = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) {
      const u32 sk = src[k];
      bits |= ((sk >> t0) & 1u) << (2 * k);
      bits |= ((sk >> (16 + t0)) & 1u) << (2 * k + 1);
    }
    shw.mplane[t0][w] = bits;
  }
  {
    int part_i = 0, part_q = 0;
    for (int w = tid; w < kWords32; w += kMxThreads) {
      const u32 m = shw.mag[w];
      part_i += 2 * (int)__popc(sh.d[0][w] & m) - (int)__popc(m);
      part_q += 2 * (int)__popc(sh.d[1][w] & m) - (int)__popc(m);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      part_i += __shfl_xor(part_i, off);
      part_q += __shfl_xor(part_q, off);
    }
    if (lane == 0) {
      atomicAdd(&shw.wsum[0], part_i);
      atomicAdd(&shw.wsum[1], part_q);
    }
  }
  mxw_build_start(shw, 0, 0, tid);
  mxw_build_start(shw, 1, 1, tid);
  __syncthreads();
  for (int m = tid; m < 16 * (kPlaneWordsMx - 32); m += kMxThreads) {   // circular extension, as mx_wipe_block's
    const int w = 32 + m % (kPlaneWordsMx - 32);
    const int r = m / (kPlaneWordsMx - 32);
    const u32 *pl = shw.mplane[r];
    const int pos = 32 * w - (w >= 64 ? 2 * kChips : kChips);
    const int lo = pos >> 5;
    u32 v = __builtin_amdgcn_alignbit(lo < 31 ? pl[lo + 1] : 0u, pl[lo], (u32)(pos & 31));
    if (pos + 32 > kChips) {
      const int k = kChips - pos;
      v = (v & ((1u << k) - 1u)) | (pl[0] << k);
    }
    shw.mplane[r][w] = v;
  }
}

}  // namespace

__global__ __launch_bounds__(kMxThreads, 1) void k_acq_mxw(const uint8_t *__restrict__ if_blocks, int stride_blocks, int n_prn,
                                                           const u32 *__restrict__ mx_a, int if_hz, int dopp_min_hz, int dopp_step_hz,
                                                           int n_dopp, int use_magnitude, gpsx_peak_t *__restrict__ peaks)
{
  __shared__ MxwShared shw;
  MxShared &sh = shw.s;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int role = wave >> 2;                            // waves w and w + 4 share a SIMD: half a step apart
  const int q0_tile = 8 * (wave >> 1) + (wave & 1);      // this wave owns q-tiles q0_tile + 2 j
  const MxCluster c = mx_decode_cluster((int)blockIdx.x, (n_prn + 31) / 32, n_dopp);
  const int set = c.set, dopp = c.dopp, search = c.search;
  const u32 step_word = mx_step_word(dopp, if_hz, dopp_min_hz, dopp_step_hz);
  const uint8_t *blk = if_blocks + (size_t)search * stride_blocks * GPSX_BYTES_PER_MS_2BIT;

  mxw_cluster_start(sh, mx_a, set, tid);
  mxw_block_start(shw, blk, use_magnitude, step_word, tid, lane);
  v16f acc[2][kMxTiles];
  {
    const float t_i = (float)(2 * (int)sh.ones[0] - 32 * kWords32 + 2 * shw.wsum[0]);
    const float t_q = (float)(2 * (int)sh.ones[1] - 32 * kWords32 + 2 * shw.wsum[1]);
#pragma unroll
    for (int j = 0; j < kMxTiles; j++)
#pragma unroll
      for (int r = 0; r < 16; r++) {
        acc[0][j][r] = t_i;
        acc[1][j][r] = t_q;
      }
  }
  const v4i no_corr = v4i{0, 0, 0, 0};
  // steps of two halves, as mx_unit (k_acq_mx.hip): role 0 runs pass p, then the epilogue of the offset pass p - 1 finished; role 1 the
  // epilogue first, then the pass; one barrier per step.  The vector of pass p + 1 is built during step p by role 0 alone
  // (k_acq_wmx_ms runs this schedule with its own epilogue: one shared loop changed both kernels' main loops, EXPERIMENTS.md)
#pragma unroll 1
  for (int hs = 0; hs <= 2 * kWPasses; hs++) {
    if ((hs & 1) == 0)
      __syncthreads();
    const int x = hs - role;
    const bool active = x >= 0 && x < 2 * kWPasses;
    const int p = x >> 1;
    if (active && (x & 1) == 0)
      mx_pass<true, kMxTiles, kScaleOne>(sh, p & 1, lane, q0_tile, acc, p == 0 ? kScaleOne : p == 1 ? kScaleFour : p == 2 ? kScaleSixteen : kScaleTwo,
                                         no_corr, false);
    if (active && (x & 1) && p >= 2)
      mxw_epilogue(sh, lane, q0_tile, p - 2, acc);
    // the vector of the NEXT step's pass, by the waves of role 0 alone, behind their epilogue: they are the ones that wait at the
    // step's barrier (role 1's epilogue runs beside a pass and takes half as long again); the buffer was last read in the
    // previous step
    if (role == 0 && (hs & 1)) {
      const int p_vec = (hs >> 1) + 1;
      if (p_vec == 2) {
        mxw_build_start(shw, 2, 0, tid);
        mxw_build_start(shw, 2, 0, tid + 256);
      } else if (p_vec > 2 && p_vec < kWPasses) {
        mxw_build_step(shw, p_vec - 3, p_vec & 1, tid);
        mxw_build_step(shw, p_vec - 3, p_vec & 1, tid + 256);
      }
    }
  }
  __syncthreads();
  // ---- one triplet per (search, PRN, Doppler): the eight bit shifts' slots (32 lanes each) meet here --------------------------
  {
    const int which = tid >> 8, p = (tid >> 3) & 31, b = tid & 7;
    const int slot = 32 * set + p;
    const u32 *row = sh.part[b][p][which];
    u32 k = 0, t = 0;
#pragma unroll
    for (int l = 0; l < 32; l++) {
      const u32 v = row[(l + tid) & 31];
      k = v > k ? v : k;
      t += v;
    }
    const size_t idx = ((size_t)search * n_prn + slot) * n_dopp + dopp;
    if (which == 0) {   // (wave-uniform: waves 0..3; a PRN's eight bit shifts are eight adjacent lanes)
      const u32 max_val = k >> 11, fine = 8u * (2047u - (k & 2047u)) + (u32)b;
      unsigned long long key = max_val ? ((unsigned long long)max_val << 14) | (unsigned long long)(16383u - fine) : 0ull;
      key = mx_max8_u64(key);
      if (b == 0 && slot < n_prn) {
        peaks[idx].max_val = (u32)(key >> 14);
        peaks[idx].phase = key ? 16383u - (u32)(key & 16383u) : 0u;
      }
    } else {
      t += __shfl_xor(t, 1);
      t += __shfl_xor(t, 2);
      t += __shfl_xor(t, 4);
      if (b == 0 && slot < n_prn) {
        peaks[idx].sum = t;
        peaks[idx].avr = t / (u32)kSamples;
      }
    }
  }
}

void launch_acq_mxw(hipStream_t s, const uint8_t *d_if_blocks, int n_search, int stride_blocks, int n_prn, const uint32_t *d_mx_a,
                    int if_hz, int dopp_min_hz, int dopp_step_hz, int n_dopp, int use_magnitude, gpsx_peak_t *d_peaks)
{
  const int n_sets = (n_prn + 31) / 32;
  hipLaunchKernelGGL(k_acq_mxw, dim3((unsigned)(n_search * n_dopp * n_sets)), dim3(kMxThreads), 0, s, d_if_blocks, stride_blocks,
                     n_prn, d_mx_a, if_hz, dopp_min_hz, dopp_step_hz, n_dopp, use_magnitude, d_peaks);
}

// =============================================================================================================================
// EXTENSION, not in the reference: the weighted grid over n_ms blocks summed non-coherently (include/gpsx.h
// gpsx_acq_grid_weighted_ms):  E(tau) = sum_b floor(sqrt(I_b(tau)^2 + Q_b(tau)^2)),  then max / first phase / sum of E.
// Form: k_acq_mxw's workgroup (a cluster: search, Doppler bin, 32 PRNs) walks the search's blocks -- per block the same
// preamble (mxw_block_start), passes and exact roots as the single-block kernel.  A block's roots go into running sums E kept
// in HBM (u32: 128 x 69375 < 2^24): record layout per wave [sample offset][tile][quad of PRN rows][lane] as uint4, one
// contiguous kilobyte per wave instruction; the first block reads none, the last writes none and folds E instead -- into
// 64-bit keys (E << 14 | 16383 - tau: E needs up to 24 bits, the single-block kernel's 32-bit keys hold 21) and u32 sums, one
// slot per (PRN, lane) in the LDS of the single-block kernel's result slots.  Records are requested half a tile ahead.
namespace {

constexpr int kWmsRecsPerWave = 16 * 64;    // uint4 per (sample offset, wave): 4 tiles x 4 quads x 64 lanes

// half a tile's records (quads 2 hh, 2 hh + 1 of tile j: eight PRN rows) of this lane
__device__ __forceinline__ void wmxms_request(const uint4 *__restrict__ rec, int half, int lane, uint4 (&r)[2])
{
#pragma unroll
  for (int c = 0; c < 2; c++)
    r[c] = rec[(half * 2 + c) * 64 + lane];
}

// the epilogue of sample offset t0 in halves of a tile (eight PRN rows): the next half's records are requested before this
// one's roots (nothing is held across the MFMA pass: 8 more registers there spilled)
__device__ __forceinline__ void wmxms_epilogue(MxShared &sh, int lane, int q0_tile, int t0, const v16f (&acc)[2][kMxTiles],
                                               uint4 *__restrict__ rec, bool first, bool last)
{
  asm volatile("" : "+v"(lane));   // (its addresses are worked out here, not hoisted into registers held across the passes)
  uint4 pre[2];
  if (!first)
    wmxms_request(rec, 0, lane, pre);
  const int n = lane & 31, h = lane >> 5;
  const bool last_exists = 32 * (q0_tile + 2 * (kMxTiles - 1)) + n < kChips;   // chip offset 1023 does not exist
  // result slots (last block): u64 keys [32 PRNs][32 lanes] in the first 8 KB of s.part, u32 sums behind them
  unsigned long long *key_slot = reinterpret_cast<unsigned long long *>(&sh.part[0][0][0][0]) + 4 * h * 32 + n;
  u32 *sum_slot = &sh.part[0][0][0][0] + 2048 + 4 * h * 32 + n;
#pragma unroll
  for (int hf = 0; hf < 2 * kMxTiles; hf++) {
    const int j = hf >> 1, r0 = 8 * (hf & 1);
    uint4 nxt[2];
    if (!first && hf + 1 < 2 * kMxTiles)
      wmxms_request(rec, hf + 1, lane, nxt);
    float lim = 0.0f;
#pragma unroll
    for (int r = r0; r < r0 + 8; r++)
      lim = mxw_max_abs(lim, acc[0][j][r], acc[1][j][r]);
    const bool small = __builtin_amdgcn_ballot_w64(lim >= 2896.0f) == 0;
    u32 e[8];
    if (small) {
#pragma unroll
      for (int i = 0; i < 8; i++)
        e[i] = mxw_root_small(acc[0][j][r0 + i], acc[1][j][r0 + i]);
    } else {
#pragma unroll
      for (int i = 0; i < 8; i++)
        e[i] = mxw_root_exact((int)acc[0][j][r0 + i], (int)acc[1][j][r0 + i]);
    }
    const bool exists = j < kMxTiles - 1 || last_exists;
#pragma unroll
    for (int i = 0; i < 8; i++)
      e[i] = exists ? e[i] : 0u;
    if (!first) {
#pragma unroll
      for (int c = 0; c < 2; c++) {
        e[4 * c + 0] += pre[c].x;
        e[4 * c + 1] += pre[c].y;
        e[4 * c + 2] += pre[c].z;
        e[4 * c + 3] += pre[c].w;
      }
    }
    if (!last) {
#pragma unroll
      for (int c = 0; c < 2; c++)
        rec[(hf * 2 + c) * 64 + lane] = make_uint4(e[4 * c], e[4 * c + 1], e[4 * c + 2], e[4 * c + 3]);
    } else {
      const int q = 32 * (q0_tile + 2 * j) + n;
      const unsigned long long low = exists ? (unsigned long long)(16383 - (16 * q + t0)) : 0ull;
#pragma unroll
      for (int i = 0; i < 8; i++) {
        const int r = r0 + i, p = (r & 3) + 8 * (r >> 2);  // PRN p + 4 h of the cluster
        const unsigned long long key = exists ? ((unsigned long long)e[i] << 14) | low : 0ull;
        atomicMax(&key_slot[p * 32], key);
        atomicAdd(&sum_slot[p * 32], e[i]);
      }
    }
    if (!first && hf + 1 < 2 * kMxTiles) {
#pragma unroll
      for (int c = 0; c < 2; c++)
        pre[c] = nxt[c];
    }
  }
}

}  // namespace

__global__ __launch_bounds__(kMxThreads, 1) void k_acq_wmx_ms(const uint8_t *__restrict__ if_blocks, int stride_blocks, int n_ms, int n_prn,
                                                              const u32 *__restrict__ mx_a, int if_hz, int dopp_min_hz, int dopp_step_hz,
                                                              int n_dopp, int use_magnitude, int cluster_lo, uint4 *__restrict__ scratch,
                                                              gpsx_peak_t *__restrict__ peaks)
{
  __shared__ MxwShared shw;
  MxShared &sh = shw.s;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int role = wave >> 2;
  const int q0_tile = 8 * (wave >> 1) + (wave & 1);
  const MxCluster c = mx_decode_cluster(cluster_lo + (int)blockIdx.x, (n_prn + 31) / 32, n_dopp);
  const int set = c.set, dopp = c.dopp, search = c.search;
  const u32 step_word = mx_step_word(dopp, if_hz, dopp_min_hz, dopp_step_hz);
  // this workgroup's running sums: [sample offset][wave] slices of kWmsRecsPerWave records
  uint4 *const recs = scratch + (size_t)blockIdx.x * (16 * 8 * kWmsRecsPerWave) + (size_t)wave * kWmsRecsPerWave;

  mxw_cluster_start(sh, mx_a, set, tid);
  const v4i no_corr = v4i{0, 0, 0, 0};
#pragma unroll 1
  for (int b = 0; b < n_ms; b++) {
    const bool first = b == 0, last = b == n_ms - 1;
    if (!first)
      __syncthreads();   // (the previous block's passes and vectors are done with the planes)
    // (the preamble's addresses derive from an opaque copy of the thread index: hoisted out of the block loop they stayed live
    //  across every pass and spilled)
    int tid_b = tid, lane_b = lane;
    asm volatile("" : "+v"(tid_b), "+v"(lane_b));
    mxw_block_start(shw, if_blocks + ((size_t)search * stride_blocks + b) * GPSX_BYTES_PER_MS_2BIT, use_magnitude, step_word, tid_b, lane_b);
    v16f acc[2][kMxTiles];
    {
      const float t_i = (float)(2 * (int)sh.ones[0] - 32 * kWords32 + 2 * shw.wsum[0]);
      const float t_q = (float)(2 * (int)sh.ones[1] - 32 * kWords32 + 2 * shw.wsum[1]);
  #pragma unroll
      for (int j = 0; j < kMxTiles; j++)
  #pragma unroll
        for (int r = 0; r < 16; r++) {
          acc[0][j][r] = t_i;
          acc[1][j][r] = t_q;
        }
    }
    // k_acq_mxw's schedule of passes, epilogues and vector builds (its own copy: one shared loop changed both kernels' main loops)
#pragma unroll 1
    for (int hs = 0; hs <= 2 * kWPasses; hs++) {
      if ((hs & 1) == 0)
        __syncthreads();
      const int x = hs - role;
      const bool active = x >= 0 && x < 2 * kWPasses;
      const int p = x >> 1;
      if (active && (x & 1) == 0)
        mx_pass<true, kMxTiles, kScaleOne>(sh, p & 1, lane, q0_tile, acc, p == 0 ? kScaleOne : p == 1 ? kScaleFour : p == 2 ? kScaleSixteen : kScaleTwo,
                                           no_corr, false);
      if (active && (x & 1) && p >= 2)
        wmxms_epilogue(sh, lane, q0_tile, p - 2, acc, recs + (size_t)(p - 2) * 8 * kWmsRecsPerWave, first, last);
      if (role == 0 && (hs & 1)) {
        const int p_vec = (hs >> 1) + 1;
        int tv = tid;
        asm volatile("" : "+v"(tv));
        if (p_vec == 2) {
          mxw_build_start(shw, 2, 0, tv);
          mxw_build_start(shw, 2, 0, tv + 256);
        } else if (p_vec > 2 && p_vec < kWPasses) {
          mxw_build_step(shw, p_vec - 3, p_vec & 1, tv);
          mxw_build_step(shw, p_vec - 3, p_vec & 1, tv + 256);
        }
      }
    }
  }
  __syncthreads();
  // ---- one record per (search, PRN, Doppler): the 32 lanes' slots of each PRN ------------------------------------------------
  {
    const int p = tid >> 4, i = tid & 15;                  // 16 threads per PRN, two slots each
    const unsigned long long *keys = reinterpret_cast<const unsigned long long *>(&sh.part[0][0][0][0]) + p * 32;
    const u32 *sums = &sh.part[0][0][0][0] + 2048 + p * 32;
    unsigned long long k = keys[i] > keys[i + 16] ? keys[i] : keys[i + 16];
    u32 t = sums[i] + sums[i + 16];
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) {
      const u32 lo = __shfl_xor((u32)k, off), hi = __shfl_xor((u32)(k >> 32), off);
      const unsigned long long o = ((unsigned long long)hi << 32) | lo;
      k = o > k ? o : k;
      t += __shfl_xor(t, off);
    }
    const int slot = 32 * set + p;
    if (i == 0 && slot < n_prn) {
      gpsx_peak_t pk;
      pk.max_val = (u32)(k >> 14);
      pk.phase = pk.max_val ? 16383u - (u32)(k & 16383u) : 0u;
      pk.sum = t;
      pk.avr = t / (u32)kSamples;
      peaks[((size_t)search * n_prn + slot) * n_dopp + dopp] = pk;
    }
  }
}

void launch_acq_mxw_ms(hipStream_t s, const uint8_t *d_if_blocks, int stride_blocks, int n_ms, int n_prn, const uint32_t *d_mx_a, int if_hz,
                       int dopp_min_hz, int dopp_step_hz, int n_dopp, int use_magnitude, int cluster_lo, int n_clusters, void *d_scratch,
                       gpsx_peak_t *d_peaks)
{
  hipLaunchKernelGGL(k_acq_wmx_ms, dim3((unsigned)n_clusters), dim3(kMxThreads), 0, s, d_if_blocks, stride_blocks, n_ms, n_prn, d_mx_a,
                     if_hz, dopp_min_hz, dopp_step_hz, n_dopp, use_magnitude, cluster_lo, static_cast<uint4 *>(d_scratch), d_peaks);
}

}  // namespace gpsx
