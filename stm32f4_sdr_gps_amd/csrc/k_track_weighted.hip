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
#include "gpsx_track_weighted_plan.hpp"
#include "gpsx_track_weighted_wave.hpp"

namespace gpsx {

__global__ __launch_bounds__(256) void k_track_epl_weighted(const uint8_t *__restrict__ if_blocks, int if_hz, int use_magnitude, int spacing,
                                                            gpsx_trk_state_t *__restrict__ st, int n_ch, int cpw,
                                                            const u32 *__restrict__ rep_all, int32_t *__restrict__ iq_out,
                                                            u32 *__restrict__ bad_prn, int write_accum)
{
  using namespace trkweighted;
  __shared__ __attribute__((aligned(16))) u32 s_x[512], s_m[512];
  __shared__ uint2 s_carrier[4];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int blk = blockIdx.y;
  const int ch0 = ((int)blockIdx.x * 4 + wave) * cpw;

  // ---- the block's two planes, once per workgroup (gpsx_track_weighted_wave.hpp) ----------------------------------------------
  if (threadIdx.x < 4)
    s_carrier[threadIdx.x] = uint2{carrier_i(threadIdx.x), carrier_q(threadIdx.x)};
  stage_planes(if_blocks + (size_t)blk * GPSX_BYTES_PER_MS_2BIT, use_magnitude, s_x, s_m);
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

  u32 pop_m;
  const u32 sums = wave_counts(s_x, s_m, s_carrier, lane, n_here, prn, tau, spacing, step, acc_b, rep_all, pop_m);
  if (!mine)
    return;
  int res_i, res_q;   // a bad channel: six zeros per block
  finish_tap(s_carrier, lane, prn, tau, spacing, step, acc_b, rep_all, sums, pop_m, res_i, res_q);
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
