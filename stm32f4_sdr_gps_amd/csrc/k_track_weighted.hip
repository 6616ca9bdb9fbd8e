// k_track_weighted.hip -- EXTENSION, not in the reference: Early / Prompt / Late I and Q on WEIGHTED two-bit samples, for many
// channels and K consecutive 1 ms blocks per launch (include/gpsx.h gpsx_track_epl_weighted).  The sample, carrier
// and replica definitions are the weighted grids' (k_acq_coh.hip), so a grid record hands over to a channel state exactly.
//
// The shape is k_track_epl_wave's (gpsx_track_wave.hpp): a wave per channel, `cpw` channels per wave one after the other, the
// data words stay in the lane that mixed them, x ^ carrier ^ replica is one v_bitop3_b32, the replica window is cut from the
// circular bit-stream table d_trk_rep with funnel shifts, v_bcnt_u32_b32 accumulates with its own addend and one transposing DPP
// reduction finishes.  What differs:
//  * Two planes.  With y = x ^ carrier ^ r (a set bit: wiped sample x replica = +1) and m the magnitude word, the correlation over
//    the N = 16352 mixed samples is  sum (2 y - 1)(1 + 2 m) = 2 (pop(y) + 2 pop(y & m)) - N - 2 pop(m).  A lane keeps pop(y) and
//    pop(y & m) apart while it counts (at most 8 x 32 each) and packs pop(y) + 2 pop(y & m) <= 768 for I and Q into one word for
//    the reduction: a channel's total is at most 3 x 16352 + 32 < 2^16.  pop(m) belongs to the block, not to the channel.
//  * The table IS the circular replica of this definition, and it holds two periods and a bit: with Late at the window's first
//    bit t_l = (-(tau + spacing)) mod 16368, Prompt sits `spacing` and Early 2 x spacing bits further on for every tau -- the
//    wrap of tau +- spacing is the reduction of t_l and nothing else.  2 x 15 < 32: the six-word read covers every spacing.
//  * No quirk terms.  Stream word 511 (the sixteen unmixed samples, weight 0) is staged as zero in both planes; what the loop
//    counted there, pop(carrier ^ r), is taken back per (channel, tap) after the loop.
//  * K blocks.  acc_b = acc + b x 511 x step32 is a closed form, so (block, channel group) units are independent: blockIdx.y is the
//    block.  The state is read by every block's unit, so the accumulator a call leaves is written where nothing else can be reading
//    it: by the kernel itself at K = 1, by k_track_weighted_advance behind it on the stream otherwise.
#include "gpsx_track_wave.hpp"
#include "gpsx_track_weighted_plan.hpp"

namespace gpsx {

namespace {

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

}  // namespace

__global__ __launch_bounds__(256) void k_track_epl_weighted(const uint8_t *__restrict__ if_blocks, int if_hz, int use_magnitude, int spacing,
                                                            gpsx_trk_state_t *__restrict__ st, int n_ch, int cpw,
                                                            const u32 *__restrict__ rep_all, int32_t *__restrict__ iq_out,
                                                            u32 *__restrict__ bad_prn, int write_accum)
{
  using namespace trkwave;
  __shared__ __attribute__((aligned(16))) u32 s_x[512], s_m[512];
  __shared__ uint2 s_carrier[4];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int blk = blockIdx.y;
  const int ch0 = ((int)blockIdx.x * 4 + wave) * cpw;

  // ---- the block's two planes, once per workgroup: 32 samples = four 16-bit words of sign/magnitude pairs ---------------------
  if (threadIdx.x < 4)
    s_carrier[threadIdx.x] = uint2{carrier_i(threadIdx.x), carrier_q(threadIdx.x)};
  {
    const uint16_t *src = reinterpret_cast<const uint16_t *>(if_blocks + (size_t)blk * GPSX_BYTES_PER_MS_2BIT);
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
  __syncthreads();
  if (ch0 >= n_ch)   // (wave-uniform: an idle wave of the last workgroup)
    return;
  const int n_here = min(cpw, n_ch - ch0);

  // ---- per (channel, tap): lane 4 c + k, k = 0 / 1 / 2 = Early / Prompt / Late (k = 3 idles) ----------------------------------
  const int c_l = lane >> 2, k_l = lane & 3;
  const bool mine = c_l < n_here && k_l < 3;
  const int ch_l = ch0 + (c_l < n_here ? c_l : 0);
  const gpsx_trk_state_t state = st[ch_l];
  int tau;
  const bool phase_ok = weighted_tau(state.code_phase_fine, tau);
  const bool reporter = mine && k_l == 0 && blk == 0;
  int prn = track_prn(state.prn, bad_prn, reporter);
  if (!phase_ok) {
    if (reporter && bad_prn && state.prn != kTrackPadPrn)
      *bad_prn = 1u;
    prn = 0;
  }
  const u32 step = nco_step_per_word((float)if_hz + state.if_freq_offset_hz);
  const u32 acc_b = state.if_freq_accum + (u32)blk * (u32)kWords32 * step;
  // Late's window starts at table bit t_l; this lane's tap (2 - k) x spacing bits further on
  const u32 t_l = (u32)(2 * kSamples - tau - spacing) % (u32)kSamples;
  const u32 t_k = t_l + (u32)((2 - (k_l < 3 ? k_l : 2)) * spacing);
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
  pop_m = wave_sum_u32(pop_m);

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

  if (!mine)
    return;
  // stream word 511 is zero in both planes: the loop counted pop(carrier ^ r) there -- take it back
  u32 total = sums;
  {
    const u32 *rw = rep_all + (size_t)prn * kTrackRepStride + (t_k >> 5) + kWords32;
    const u32 r = __builtin_amdgcn_alignbit(rw[1], rw[0], t_k & 31u);
    const uint2 c511 = s_carrier[(acc_b + step * (u32)kWords32) >> 30];
    total -= (u32)__popc(c511.x ^ r) + ((u32)__popc(c511.y ^ r) << 16);
  }
  const int bias = kMixed + 2 * (int)pop_m;
  int res_i = 2 * (int)(total & 0xFFFFu) - bias, res_q = 2 * (int)(total >> 16) - bias;
  if (prn == 0)
    res_i = res_q = 0;   // a bad channel: six zeros per block
  int32_t *out = iq_out + ((size_t)blk * (size_t)n_ch + (size_t)ch_l) * 6 + 2 * k_l;   // (IE,QE) (IP,QP) (IL,QL)
  out[0] = res_i;
  out[1] = res_q;
  if (write_accum && k_l == 0)
    st[ch_l].if_freq_accum = acc_b + step * (u32)kWords32;
}

// the accumulator a K-block call leaves, K >= 2: acc + K x 511 x step32, behind the correlators on the stream
__global__ __launch_bounds__(256) void k_track_weighted_advance(int if_hz, gpsx_trk_state_t *__restrict__ st, int n_ch, u32 n_blocks)
{
  const int ch = blockIdx.x * blockDim.x + threadIdx.x;
  if (ch >= n_ch)
    return;
  const u32 step = nco_step_per_word((float)if_hz + st[ch].if_freq_offset_hz);
  st[ch].if_freq_accum += n_blocks * (u32)kWords32 * step;
}

void launch_track_epl_weighted(hipStream_t s, const uint8_t *d_if_blocks_2bit, int n_blocks, int if_hz, int use_magnitude, int spacing,
                               gpsx_trk_state_t *d_st, int n_ch, const uint32_t *d_trk_rep, int32_t *d_iq, uint32_t *d_bad_prn)
{
  if (n_ch <= 0 || n_blocks <= 0)
    return;
  const TrackWeightedPlan p = plan_track_weighted(n_ch, n_blocks);   // channels per wave and workgroups: gpsx_track_weighted_plan.hpp
  hipLaunchKernelGGL(k_track_epl_weighted, dim3(p.groups, (unsigned)n_blocks), dim3(256), 0, s, d_if_blocks_2bit, if_hz, use_magnitude,
                     spacing, d_st, n_ch, p.cpw, d_trk_rep, d_iq, d_bad_prn, n_blocks == 1 ? 1 : 0);
  if (n_blocks > 1)
    hipLaunchKernelGGL(k_track_weighted_advance, dim3((unsigned)(((long)n_ch + 255) / 256)), dim3(256), 0, s, if_hz, d_st, n_ch,
                       (u32)n_blocks);
}

}  // namespace gpsx
