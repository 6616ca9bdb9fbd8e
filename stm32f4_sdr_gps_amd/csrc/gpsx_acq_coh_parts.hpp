// gpsx_acq_coh_parts.hpp -- the parts the coherent weighted grid's kernels share: k_acq_coh.hip (one window per search,
// gpsx_acq_grid_weighted_coh) and k_acq_hyb.hip (n_seg windows per search, their magnitudes summed: gpsx_acq_grid_weighted_hyb).
// The pre-sum of a window's blocks into polyphase int8 planes, the exact root, the record, the Toeplitz rows and the MFMA pass
// of the matrix-core form, the int16 rows and the v_dot2 loop of the vector form.  k_acq_coh.hip's header comment has the algebra.
#pragma once
#include "gpsx_device.hpp"

namespace gpsx {

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));
typedef short v2s __attribute__((ext_vector_type(2)));

// word w of block `blk`'s sign and magnitude planes (32 samples; w < 511: only the mixed words are read)
__device__ __forceinline__ void coh_planes(const uint8_t *blk, int w, u32 &s, u32 &m)
{
  const uint16_t *p = reinterpret_cast<const uint16_t *>(blk) + 4 * w;
  const u32 lo = (u32)p[0] | ((u32)p[1] << 16), hi = (u32)p[2] | ((u32)p[3] << 16);
  s = even_bits16(lo) | (even_bits16(hi) << 16);
  m = even_bits16(lo >> 1) | (even_bits16(hi >> 1) << 16);
}

// the pre-sum: mt[stream][t][k] = M(16 k + t) = sum_b v_b(16 k + t) wiped, int8; k = 1022 (the unmixed samples) and the pad k = 1023: 0.
// Word w of block b is mixed with the NCO's quadrant (acc_b + w step32) >> 30, acc_b = 511 b step32 (mod 2^32).
__device__ __forceinline__ void coh_presum(int8_t (&mt)[2][16][1024], const uint8_t *blk0, int n_coh, u32 step_word, int use_magnitude,
                                           int tid, int n_threads)
{
  for (int w = tid; w < 512; w += n_threads) {
    int mi[32], mq[32];
#pragma unroll
    for (int k = 0; k < 32; k++)
      mi[k] = mq[k] = 0;
    if (w < kWords32) {
#pragma unroll 1
      for (int b = 0; b < n_coh; b++) {
        u32 sg, mg;
        coh_planes(blk0 + (size_t)b * GPSX_BYTES_PER_MS_2BIT, w, sg, mg);
        mg = use_magnitude ? mg : 0u;
        const u32 quad = (step_word * (u32)(kWords32 * b + w)) >> 30;
        const u32 di = sg ^ carrier_i(quad), dq = sg ^ carrier_q(quad);
#pragma unroll
        for (int k = 0; k < 32; k++) {
          const int wt = 1 + 2 * (int)((mg >> k) & 1u);
          mi[k] += ((di >> k) & 1u) ? wt : -wt;
          mq[k] += ((dq >> k) & 1u) ? wt : -wt;
        }
      }
    }
    // sample 32 w + k -> mt[k % 16][2 w + k / 16]: one 16-bit store per (stream, t)
#pragma unroll
    for (int t = 0; t < 16; t++) {
      *reinterpret_cast<uint16_t *>(&mt[0][t][2 * w]) = (uint16_t)((mi[t] & 0xFF) | ((mi[t + 16] & 0xFF) << 8));
      *reinterpret_cast<uint16_t *>(&mt[1][t][2 * w]) = (uint16_t)((mq[t] & 0xFF) | ((mq[t + 16] & 0xFF) << 8));
    }
  }
}

// floor(sqrt(I^2 + Q^2)) exactly for |I|, |Q| < 2^20: the f32 root of the f32 sum is within 0.25 of the true root (relative error
// below 2^-21.5), so its truncation is r - 1, r or r + 1, and the 64-bit squares tell which
__device__ __forceinline__ u32 coh_root(int i, int q)
{
  const u64 e = (u64)((long long)i * i) + (u64)((long long)q * q);
  const float fi = (float)i, fq = (float)q;
  u32 r = (u32)__builtin_amdgcn_sqrtf(__builtin_fmaf(fi, fi, fq * fq));
  r = (u64)r * r > e ? r - 1u : r;
  r = (u64)(r + 1u) * (r + 1u) <= e ? r + 1u : r;
  return r;
}

__device__ __forceinline__ unsigned long long coh_key(u32 m, int tau)
{
  return ((unsigned long long)m << 14) | (unsigned long long)(16383 - tau);
}

// a (search, PRN, Doppler) record from its key (m << 14 | 16383 - tau, the first tau reaching the maximum) and its sum
__device__ __forceinline__ void coh_record(gpsx_peak_t *peak, unsigned long long key, u32 sum)
{
  gpsx_peak_t pk;
  pk.max_val = (u32)(key >> 14);
  pk.phase = pk.max_val ? 16383u - (u32)(key & 0x3FFFu) : 0u;
  pk.sum = sum;
  pk.avr = sum / (u32)kSamples;
  *peak = pk;
}

// ---- matrix cores -------------------------------------------------------------------------------------------------------------
constexpr int kCohThreads = 512;
constexpr int kCohTiles = 4;        // q-tiles (32 chip offsets) per wave: wave w owns tiles 4 w .. 4 w + 3
constexpr int kCopyDw = 520;        // one shifted copy of a B row: 2046 entries (1023 doubled) + zeros; 520 = 8 (mod 32)
constexpr int kCohPasses = 17;      // 2 for sample offset 0, one per further offset

// B rows in four copies, copy c starting at entry c: lane (n, h) of diagonal f = Q + kappa reads entries 32 f + 16 h + n .. + 15 --
// copy n % 4, four dwords from 8 f + 4 h + n / 4 (32 lanes on 32 banks)
struct CohMxShared {
  v4i chips[32][2][32];             // [kappa][h][PRN]: the signs of chips 32 kappa + 16 h .. + 15 as int8 (+1 / -1; chip 1023: 0)
  u32 rows[2][2][4][kCopyDw];       // [buffer][stream][copy][dword]
  int8_t mt[2][16][1024];           // the pre-summed planes, polyphase
  int16_t s0[2][1024];              // S_0 per stream
  unsigned long long best[32][32];  // [PRN][lane]: running best key of the lanes that hold the PRN
  u32 total[32][32];
};

// entry k (< 1023) of stream st's row of pass p: the high / low digit of S_0 (p = 0 / 1), S_{t0+1} - S_t0 for t0 = p - 2
__device__ __forceinline__ int coh_row_val(const CohMxShared &sh, int p, int st, int k)
{
  if (p >= 2) {
    const int8_t *row = sh.mt[st][p - 2];
    return (int)row[k == kChips - 1 ? 0 : k + 1] - (int)row[k];
  }
  const int s = sh.s0[st][k], lo = ((s + 8) & 15) - 8;
  return p == 0 ? (s - lo) >> 4 : lo;
}

__device__ __forceinline__ void coh_build_rows(CohMxShared &sh, int p, int buf, int tid)
{
  for (int i = tid; i < 2 * kCopyDw; i += kCohThreads) {
    const int st = i / kCopyDw, d = i % kCopyDw;
    u32 w2[2] = {0u, 0u};
#pragma unroll
    for (int e = 0; e < 8; e++) {
      const int x = 4 * d + e;
      const int v = x < 2 * kChips ? coh_row_val(sh, p, st, x >= kChips ? x - kChips : x) : 0;
      w2[e >> 2] |= ((u32)v & 0xFFu) << (8 * (e & 3));
    }
#pragma unroll
    for (int c = 0; c < 4; c++)
      sh.rows[buf][st][c][d] = c ? __builtin_amdgcn_alignbyte(w2[1], w2[0], (u32)c) : w2[0];
  }
}

// one pass: acc[stream][j] += chips x Toeplitz(row) for the wave's four q-tiles; per kappa one A fragment, one new B fragment per
// stream (tile j at kappa reads diagonal q0 + j + kappa: what tile j + 1 read at kappa - 1), eight MFMAs
__device__ __forceinline__ void coh_pass(const CohMxShared &sh, int buf, int q0, int n, int h, v16i (&acc)[2][kCohTiles])
{
  const u32 *rw0 = &sh.rows[buf][0][n & 3][4 * h + (n >> 2)], *rw1 = &sh.rows[buf][1][n & 3][4 * h + (n >> 2)];
  auto frag = [&](const u32 *rw, int f) {
    const u32 *p = rw + 8 * f;
    return v4i{(int)p[0], (int)p[1], (int)p[2], (int)p[3]};
  };
  v4i b[2][4];
#pragma unroll
  for (int j = 0; j < 3; j++) {
    b[0][j] = frag(rw0, q0 + j);
    b[1][j] = frag(rw1, q0 + j);
  }
#pragma unroll 1
  for (int kb = 0; kb < 32; kb += 4) {
#pragma unroll
    for (int kk = 0; kk < 4; kk++) {
      const int kappa = kb + kk;
      const v4i a = sh.chips[kappa][h][n];
      b[0][(kk + 3) & 3] = frag(rw0, q0 + 3 + kappa);
      b[1][(kk + 3) & 3] = frag(rw1, q0 + 3 + kappa);
#pragma unroll
      for (int st = 0; st < 2; st++)
#pragma unroll
        for (int j = 0; j < kCohTiles; j++)
          acc[st][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b[st][(kk + j) & 3], acc[st][j], 0, 0, 0);
    }
  }
}

// ---- vector ALU -------------------------------------------------------------------------------------------------------------
constexpr int kCohVThreads = 256;
constexpr int kCohVG = 8;           // PRNs per workgroup
constexpr int kVRowDw = 1028;       // one row of S_t0 as int16: 2046 entries (1023 doubled) + zeros

struct CohVecShared {
  int8_t mt[2][16][1024];
  u32 rows[2][kVRowDw];             // [stream]: entries 2 d, 2 d + 1 in dword d
  u32 chips[kCohVG][512];           // per PRN: chips 2 i, 2 i + 1 as int16 +1 / -1 (chip 1023: 0)
  unsigned long long best[kCohVG];
  u32 total[kCohVG];
};

__device__ __forceinline__ unsigned long long coh_wave_max_u64(unsigned long long v)
{
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const u32 lo = __shfl_xor((u32)v, off), hi = __shfl_xor((u32)(v >> 32), off);
    const unsigned long long o = ((unsigned long long)hi << 32) | lo;
    v = o > v ? o : v;
  }
  return v;
}

// the chip signs of the workgroup's eight PRNs: chips 2 i, 2 i + 1 as int16 x 2
__device__ __forceinline__ void coh_vec_chips(CohVecShared &sh, const uint8_t *chips_all, const uint8_t *prns, int n_prn, int group, int tid)
{
  for (int i = tid; i < kCohVG * 512; i += kCohVThreads) {
    const int g = i >> 9, c2 = i & 511, p = group * kCohVG + g;
    u32 word = 0;
    if (p < n_prn) {
      const uint8_t *ch = chips_all + (size_t)prns[p] * 1024;
#pragma unroll
      for (int e = 0; e < 2; e++) {
        const int c = 2 * c2 + e;
        word |= (c < kChips ? (ch[c] ? 0xFFFFu : 0x0001u) : 0u) << (16 * e);
      }
    }
    sh.chips[g][c2] = word;
  }
}


}  // namespace

}  // namespace gpsx
