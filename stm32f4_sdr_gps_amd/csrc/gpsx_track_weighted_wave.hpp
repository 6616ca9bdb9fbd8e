// gpsx_track_weighted_wave.hpp -- the weighted two-bit E/P/L correlators of one block for the channels of a wave, as device
// functions shared by k_track_epl_weighted (open loop: a (block, channel group) grid, k_track_weighted.hip) and the closed loops
// k_track_wloop and k_track_wsync (the blocks one after the other inside the kernel, k_track_loop_weighted.hip and
// k_track_loop_weighted_sync.hip; what those two share beyond the correlators is gpsx_track_wloop_parts.hpp).  The formulation -- two planes,
// pop(y) + 2 pop(y & m), the circular table with Late at the window's first bit, stream word 511 staged as zero and taken back,
// pop(m) per block -- is described in front of k_track_epl_weighted.
#pragma once
#include "gpsx_track_wave.hpp"

namespace gpsx {
namespace trkweighted {

constexpr int kMixed = 32 * kWords32;   // 16352 samples the NCO loop mixes

// tau = (int)code_phase_fine reduced to [0, 16368); false: not finite or |phase| >= 2^24 (the channel is treated like a bad PRN)
__device__ __forceinline__ bool weighted_tau(float phase, int &tau)
{
  tau = 0;
  if (!(__builtin_fabsf(phase) < 16777216.0f))
    return false;
  const int t = (int)phase % kSamples;
  tau = t < 0 ? t + kSamples : t;
  return true;
}

// a block's two planes, by the whole workgroup of 256: 32 samples = four 16-bit words of sign/magnitude pairs; stream word 511
// (the sixteen unmixed samples, weight 0) is zero in both.  The caller synchronises.
__device__ __forceinline__ void stage_planes(const uint8_t *__restrict__ block, int use_magnitude, u32 *s_x, u32 *s_m)
{
  const uint16_t *src = reinterpret_cast<const uint16_t *>(block);
  for (int w = threadIdx.x; w < 512; w += 256) {
    u32 s = 0, m = 0;
    if (w < kWords32) {
      const uint16_t *p = src + 4 * w;
      const u32 lo = (u32)p[0] | ((u32)p[1] << 16), hi = (u32)p[2] | ((u32)p[3] << 16);
      s = even_bits16(lo) | (even_bits16(hi) << 16);
      m = use_magnitude ? even_bits16(lo >> 1) | (even_bits16(hi >> 1) << 16) : 0u;
    }
    s_x[w] = s;
    s_m[w] = m;
  }
}

// One block of Early / Prompt / Late for the n_here (>= 1) channels of a wave, in two steps.  Lane 4 c + k (k = 0 / 1 / 2 = Early /
// Prompt / Late, k = 3 idles) carries channel c's validated PRN (0: a bad channel), tau, the NCO step per word and the accumulator
// at the start of THIS block.
// Step 1, all 64 lanes: the counts over stream words 0 .. 511 -> lane 4 c + k: (count_I | count_Q << 16), count = pop(y) + 2 pop(y & m),
// and the block's pop(m).
__device__ __forceinline__ u32 wave_counts(const u32 *s_x, const u32 *s_m, const uint2 *s_carrier, int lane, int n_here, int prn, int tau,
                                           int spacing, u32 step, u32 acc_b, const u32 *__restrict__ rep_all, u32 &pop_m_out)
{
  using namespace trkwave;
  const int c_l = lane >> 2;
  // Late's window starts at table bit t_l; tap k's (2 - k) x spacing bits further on
  const u32 t_l = (u32)(2 * kSamples - tau - spacing) % (u32)kSamples;
  const u32 info = ((u32)prn << 14) | t_l;

  // this lane's eight words of both planes (the same for every channel of the wave) and the block's pop(m)
  const u32 lane4 = 4u * (u32)lane;
  u32 x[8], m[8];
#pragma unroll
  for (int it = 0; it < 2; it++) {
    const uint4 x4 = *reinterpret_cast<const uint4 *>(&s_x[lane4 + 256 * it]);
    const uint4 m4 = *reinterpret_cast<const uint4 *>(&s_m[lane4 + 256 * it]);
    x[4 * it] = x4.x; x[4 * it + 1] = x4.y; x[4 * it + 2] = x4.z; x[4 * it + 3] = x4.w;
    m[4 * it] = m4.x; m[4 * it + 1] = m4.y; m[4 * it + 2] = m4.z; m[4 * it + 3] = m4.w;
  }
  u32 pop_m = 0;
#pragma unroll
  for (int u = 0; u < 8; u++)
    pop_m += (u32)__popc(m[u]);
  pop_m_out = wave_sum_u32(pop_m);

  const int xor16 = (lane ^ 16) << 2, xor32 = (lane ^ 32) << 2;
  const u32 sh_p = (u32)spacing, sh_e = 2u * (u32)spacing;
  u32 sums = 0;   // lane 4 c + k: (count_I | count_Q << 16), count = pop(y) + 2 pop(y & m) over stream words 0 .. 511

#pragma unroll 1
  for (int c = 0; c < n_here; c++) {
    const u32 acc0 = (u32)__builtin_amdgcn_readlane((int)acc_b, 4 * c);
    const u32 stp = (u32)__builtin_amdgcn_readlane((int)step, 4 * c);
    const u32 inf = (u32)__builtin_amdgcn_readlane((int)info, 4 * c);
    uint2 cw[8];   // carrier words: word w sees NCO phase acc + w step
    {
      u32 acc = acc0 + stp * lane4;
#pragma unroll
      for (int it = 0; it < 2; it++) {
#pragma unroll
        for (int u = 0; u < 4; u++) {
          cw[4 * it + u] = *reinterpret_cast<const uint2 *>(reinterpret_cast<const char *>(s_carrier) + ((acc >> 27) & 0x18u));
          acc += stp;
        }
        acc += stp * 252u;
      }
    }
    const u32 t0 = inf & 0x3FFFu, sh = t0 & 31u;
    const u32 *row = rep_all + (size_t)(inf >> 14) * kTrackRepStride + (t0 >> 5);
    u32 cs[3][2] = {{0, 0}, {0, 0}, {0, 0}}, cm[3][2] = {{0, 0}, {0, 0}, {0, 0}};   // [Late, Prompt, Early][I, Q]
#pragma unroll
    for (int it = 0; it < 2; it++) {
      const u32 *p = row + lane4 + 256 * it;
      const TrkW4 t4 = *reinterpret_cast<const TrkW4 *>(p);
      const TrkW2 t2 = *reinterpret_cast<const TrkW2 *>(p + 4);
      const u32 t[6] = {t4.w[0], t4.w[1], t4.w[2], t4.w[3], t2.w[0], t2.w[1]};
      u32 a[5];
#pragma unroll
      for (int u = 0; u < 5; u++)
        a[u] = __builtin_amdgcn_alignbit(t[u + 1], t[u], sh);
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int j = 4 * it + u;
#pragma unroll
        for (int k = 0; k < 3; k++) {
          const u32 r = k == 0 ? a[u] : __builtin_amdgcn_alignbit(a[u + 1], a[u], k == 1 ? sh_p : sh_e);
          const u32 yi = __builtin_amdgcn_bitop3_b32(x[j], cw[j].x, r, 0x96), yq = __builtin_amdgcn_bitop3_b32(x[j], cw[j].y, r, 0x96);
          cs[k][0] = bcnt_acc(yi, cs[k][0]);
          cs[k][1] = bcnt_acc(yq, cs[k][1]);
          cm[k][0] = bcnt_acc(yi & m[j], cm[k][0]);
          cm[k][1] = bcnt_acc(yq & m[j], cm[k][1]);
        }
      }
    }
    u32 pk[3];
#pragma unroll
    for (int k = 0; k < 3; k++)
      pk[k] = (cs[k][0] + 2u * cm[k][0]) | ((cs[k][1] + 2u * cm[k][1]) << 16);
    const u32 p_l = pk[0], p_p = pk[1], p_e = pk[2];
    // wave_epl's transposing reduction: lane class (lane & 3) = 0 / 1 / 2 / 3 ends with Early / Prompt / Late / Late
    const bool odd = lane & 1, upper = lane & 2;
    u32 ab = (odd ? p_p : p_e) + dpp_get<0xB1>(odd ? p_e : p_p);   // quad_perm [1,0,3,2]
    u32 cc = p_l + dpp_get<0xB1>(p_l);
    u32 v = (upper ? cc : ab) + dpp_get<0x4E>(upper ? ab : cc);    // quad_perm [2,3,0,1]
    v += dpp_get<0x124>(v);                                        // row_ror:4
    v += dpp_get<0x128>(v);                                        // row_ror:8
    v += (u32)__builtin_amdgcn_ds_bpermute(xor16, (int)v);
    v += (u32)__builtin_amdgcn_ds_bpermute(xor32, (int)v);
    sums = c_l == c ? v : sums;
  }

  return sums;
}

// Step 2, the lanes that hold a (channel, tap): stream word 511 is zero in both planes, the loop counted pop(carrier ^ r) there --
// take it back -- and centre: I and Q of tap k, exact (zeros for a bad channel)
__device__ __forceinline__ void finish_tap(const uint2 *s_carrier, int lane, int prn, int tau, int spacing, u32 step, u32 acc_b,
                                           const u32 *__restrict__ rep_all, u32 sums, u32 pop_m, int &res_i, int &res_q)
{
  const int k_l = lane & 3;
  const u32 t_l = (u32)(2 * kSamples - tau - spacing) % (u32)kSamples;
  const u32 t_k = t_l + (u32)((2 - (k_l < 3 ? k_l : 2)) * spacing);
  u32 total = sums;
  {
    const u32 *rw = rep_all + (size_t)prn * kTrackRepStride + (t_k >> 5) + kWords32;
    const u32 r = __builtin_amdgcn_alignbit(rw[1], rw[0], t_k & 31u);
    const uint2 c511 = s_carrier[(acc_b + step * (u32)kWords32) >> 30];
    total -= (u32)__popc(c511.x ^ r) + ((u32)__popc(c511.y ^ r) << 16);
  }
  const int bias = kMixed + 2 * (int)pop_m;
  res_i = 2 * (int)(total & 0xFFFFu) - bias;
  res_q = 2 * (int)(total >> 16) - bias;
  if (prn == 0)
    res_i = res_q = 0;   // a bad channel: zeros
}

}  // namespace trkweighted
}  // namespace gpsx
