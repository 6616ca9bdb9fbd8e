// k_track_loop_weighted.hip -- EXTENSION, not in the reference: a closed DLL / Costas PLL / FLL on WEIGHTED two-bit samples, the
// channel state resident in HBM (include/gpsx.h gpsx_track_loop_weighted).
//
// One launch advances every channel by K blocks: per block the weighted E/P/L correlators of gpsx_track_weighted_wave.hpp (the
// device function k_track_epl_weighted launches: the same integers), int32 window sums kept in the lanes, and at the end of every
// coherent window of n_coh blocks the loop arithmetic of the header's definition -- every float operation one IEEE single
// operation in the order written there (this file is built with -ffp-contract=off and correctly rounded division like the rest),
// the arctangent as glibc <= 2.40 computes it (gpsx_libm.hpp).
//
// Lanes: k_track_loop's.  Lane 4 c + k of a wave holds channel c of the wave (k = 0 / 1 / 2 = Early / Prompt / Late in the
// correlators); all four lanes of a quad carry the channel's whole state and run the loop redundantly -- they all need the new tau
// and carrier for the next window's correlators, and a broadcast would cost what the arithmetic does.
// Blocks: the loop is a recurrence in time, so the blocks run one after the other inside the kernel; the workgroup stages block
// b's two planes into LDS buffer b & 1 and meets at ONE barrier per block.  A wave that has passed barrier b + 1 knows that every
// wave has finished reading block b's buffer, which is the one block b + 2 is staged into.  Every wave of a workgroup reaches
// every barrier: a wave without channels (the last workgroup's) stages, waits and skips the work -- it never leaves the loop.
// HBM traffic per launch: K x 4 KB of samples per workgroup (L2 hits after the first), 40 B of state in and out per channel, 36 B
// per (window, channel).
#include <hip/hip_runtime.h>

#include <cstddef>

#include "gpsx_device.hpp"
#include "gpsx_kernels.hpp"
#include "gpsx_libm.hpp"
#include "gpsx_track_loop_weighted_plan.hpp"
#include "gpsx_track_weighted_wave.hpp"

namespace gpsx {

namespace {

template <int K>
__device__ __forceinline__ int quad_get(int v)   // lane k of this lane's quad
{
  return __builtin_amdgcn_update_dpp(0, v, K | (K << 2) | (K << 4) | (K << 6), 0xF, 0xF, true);
}

constexpr float kCyclesPerRadian = 0.15915494f;
constexpr float kSpan = 16368.0f;

}  // namespace

__global__ __launch_bounds__(256, 4) void k_track_wloop(const uint8_t *__restrict__ if_blocks, int n_blocks, int if_hz, gpsx_wloop_cfg_t cfg,
                                                     gpsx_wloop_state_t *__restrict__ st, int n_ch, int cpw,
                                                     const u32 *__restrict__ rep_all, gpsx_wloop_rec_t *__restrict__ rec,
                                                     u32 *__restrict__ bad_prn)
{
  using namespace trkweighted;
  __shared__ __attribute__((aligned(16))) u32 s_x[2][512], s_m[2][512];   // this and the next block's planes
  __shared__ uint2 s_carrier[4];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int c_l = lane >> 2, k_l = lane & 3;
  const int ch0 = ((int)blockIdx.x * 4 + wave) * cpw;
  const int n_here = ch0 < n_ch ? min(cpw, n_ch - ch0) : 0;   // 0: an idle wave of the last workgroup still stages and waits
  const bool in_wave = c_l < n_here;
  const bool mine = in_wave && k_l < 3;
  const int ch_l = in_wave ? ch0 + c_l : (n_here ? ch0 : 0);  // (always a channel below n_ch)
  const int use_magnitude = cfg.weights == GPSX_WEIGHTS_SIGN_MAGNITUDE;
  const int n_coh = cfg.n_coh;
  const float T = (float)n_coh * 0.001f;
  const float dll_c2t = cfg.dll_c2 * T, pll_c2t = cfg.pll_c2 * T;

  if (threadIdx.x < 4)
    s_carrier[threadIdx.x] = uint2{carrier_i(threadIdx.x), carrier_q(threadIdx.x)};   // (visible after the first block's barrier)

  // the state in registers: everything but prn (its validated value is all the loop needs) and the reserved word
  struct Live { float code_phase_fine, if_freq_offset_hz; u32 if_freq_accum; float dll_err, pll_err; int prev_ip, prev_qp; u32 n_updates; };
  static_assert(sizeof(Live) == 32 && sizeof(gpsx_wloop_state_t) == 40 && offsetof(gpsx_wloop_state_t, code_phase_fine) == 4 &&
                offsetof(gpsx_wloop_state_t, n_updates) == 32, "gpsx_wloop_state_t layout");
  Live s = {};
  int prn_ok = 0;   // the validated PRN; 0: outside 1 .. 210 (reported here); -1: a padding channel (never reported)
  if (n_here) {
    const int raw = st[ch_l].prn;
    __builtin_memcpy(&s, &st[ch_l].code_phase_fine, sizeof s);
    prn_ok = raw == kTrackPadPrn ? -1 : track_prn(raw, bad_prn, mine && k_l == 0);
  }

  // what the window's correlators use: fixed at the window's start
  int tau = 0, prn = 0;
  u32 step = 0;
  auto begin_window = [&]() {
    const bool phase_ok = weighted_tau(s.code_phase_fine, tau);
    prn = phase_ok && prn_ok > 0 ? prn_ok : 0;
    if (!phase_ok && mine && k_l == 0 && bad_prn && prn_ok >= 0)
      *bad_prn = 1u;
    step = nco_step_per_word((float)if_hz + s.if_freq_offset_hz);
  };
  begin_window();
  int sum_i = 0, sum_q = 0;   // lane 4 c + k: tap k's window sums
  int in_win = 0, window = 0;

#pragma unroll 1
  for (int b = 0; b < n_blocks; b++) {
    stage_planes(if_blocks + (size_t)b * GPSX_BYTES_PER_MS_2BIT, use_magnitude, s_x[b & 1], s_m[b & 1]);
    __syncthreads();
    if (!n_here)   // (wave-uniform)
      continue;
    u32 pop_m;
    const u32 counts = wave_counts(s_x[b & 1], s_m[b & 1], s_carrier, lane, n_here, prn, tau, cfg.spacing, step, s.if_freq_accum, rep_all, pop_m);
    int res_i = 0, res_q = 0;
    if (mine)
      finish_tap(s_carrier, lane, prn, tau, cfg.spacing, step, s.if_freq_accum, rep_all, counts, pop_m, res_i, res_q);
    sum_i += res_i;
    sum_q += res_q;
    s.if_freq_accum += step * (u32)kWords32;
    if (++in_win < n_coh)   // (uniform over the launch)
      continue;

    // ---- the window's end: the quad gathers its six sums, every lane of it runs the loop ---------------------------------------
    const int IE = quad_get<0>(sum_i), QE = quad_get<0>(sum_q), IP = quad_get<1>(sum_i), QP = quad_get<1>(sum_q);
    const int IL = quad_get<2>(sum_i), QL = quad_get<2>(sum_q);
    if (prn != 0) {   // (a bad channel: floats and loop memory stay as they were)
      // DLL
      const long long e2 = (long long)IE * IE + (long long)QE * QE, l2 = (long long)IL * IL + (long long)QL * QL;
      float d = 0.0f;
      if (e2 + l2 != 0)
        d = (float)(e2 - l2) / (float)(e2 + l2);
      float phase = s.code_phase_fine - (cfg.dll_c1 * (d - s.dll_err) + dll_c2t * d);
      if (phase < 0.0f)
        phase = phase + kSpan;
      else if (phase >= kSpan)
        phase = phase - kSpan;
      s.code_phase_fine = phase;
      s.dll_err = d;
      // Costas PLL, in cycles
      float p;
      if (IP == 0)
        p = QP > 0 ? 0.25f : (QP < 0 ? -0.25f : 0.0f);
      else
        p = gpsx_libm::atanf_fdlibm((float)QP / (float)IP) * kCyclesPerRadian;
      // FLL, in Hz
      float fe = 0.0f;
      if (cfg.fll_c != 0.0f && s.n_updates > 0) {
        const long long cross = (long long)s.prev_ip * QP - (long long)s.prev_qp * IP;
        const long long dot = (long long)s.prev_ip * IP + (long long)s.prev_qp * QP;
        if (dot != 0)
          fe = gpsx_libm::atanf_fdlibm((float)cross / (float)dot) * kCyclesPerRadian / T;
      }
      s.if_freq_offset_hz = s.if_freq_offset_hz - ((cfg.pll_c1 * (p - s.pll_err) + pll_c2t * p) + cfg.fll_c * fe);
      s.pll_err = p;
      s.prev_ip = IP;
      s.prev_qp = QP;
      s.n_updates++;
    }
    if (in_wave && k_l == 0) {
      gpsx_wloop_rec_t r;
      r.iq[0] = IE; r.iq[1] = QE; r.iq[2] = IP; r.iq[3] = QP; r.iq[4] = IL; r.iq[5] = QL;
      r.code_phase_fine = s.code_phase_fine;
      r.if_freq_offset_hz = s.if_freq_offset_hz;
      r.if_freq_accum = s.if_freq_accum;
      rec[(size_t)window * (size_t)n_ch + (size_t)ch_l] = r;
    }
    window++;
    in_win = 0;
    sum_i = sum_q = 0;
    begin_window();   // tau, validity and step of the next window, in registers
  }
  if (in_wave && k_l == 0)
    __builtin_memcpy(&st[ch_l].code_phase_fine, &s, sizeof s);
}

void launch_track_loop_weighted(hipStream_t s, const uint8_t *d_if_blocks_2bit, int n_blocks, int if_hz, const gpsx_wloop_cfg_t &cfg,
                                gpsx_wloop_state_t *d_st, int n_ch, const uint32_t *d_trk_rep, gpsx_wloop_rec_t *d_rec,
                                uint32_t *d_bad_prn)
{
  if (n_ch <= 0 || n_blocks <= 0)
    return;
  const TrackLoopWeightedPlan p = plan_track_loop_weighted(n_ch);   // gpsx_track_loop_weighted_plan.hpp
  hipLaunchKernelGGL(k_track_wloop, dim3(p.groups), dim3(256), 0, s, d_if_blocks_2bit, n_blocks, if_hz, cfg, d_st, n_ch, p.cpw, d_trk_rep,
                     d_rec, d_bad_prn);
}

}  // namespace gpsx
