// gpsx_track_wloop_parts.hpp -- what the two closed loops on weighted two-bit samples share beyond the correlators of
// gpsx_track_weighted_wave.hpp: k_track_wloop (k_track_loop_weighted.hip) and k_track_wsync (k_track_loop_weighted_sync.hip), and the
// carrier-aided instances of the same two bodies beside them (k_track_waid_loop, k_track_waid_sync).  The
// lanes' places, the loop state in registers, a window's start and -- the ONE copy of it -- the DLL / Costas PLL / FLL update.
// That update is exact arithmetic: every float operation one IEEE single operation in the order written (both files are built with
// -ffp-contract=off and correctly rounded division), the arctangent gpsx_libm.hpp's; tests/weighted_loop_ref.py restates it and is
// compared bit for bit.  Regroup nothing.
// Not shared, on purpose: the per-block body (stage, barrier, wave_counts, finish_tap) and the window bookkeeping around it (windows
// uniform over the launch in one kernel, per lane and resident in the state in the other), and the two rules in which the kernels
// differ at a window's start, which each passes to begin_window at its call.
// The kernels' block loops are, instruction for instruction, what they were before this header (tools/kernel_isa_diff.py).  That
// shaped two things: the lanes' predicates are functions of Lanes' integers, not stored flags, and begin_window takes a callable.
#pragma once
#include <cstddef>

#include "gpsx_libm.hpp"
#include "gpsx_track_weighted_wave.hpp"

namespace gpsx {
namespace trkwloop {
using namespace trkweighted;

template <int K>
__device__ __forceinline__ int quad_get(int v)   // lane k of this lane's quad
{
  return __builtin_amdgcn_update_dpp(0, v, K | (K << 2) | (K << 4) | (K << 6), 0xF, 0xF, true);
}

constexpr float kCyclesPerRadian = 0.15915494f, kSpan = 16368.0f;

// the loop state in registers, in every lane of a quad: gpsx_wloop_state_t without prn (validated at the load) and the reserved word
struct Live { float code_phase_fine, if_freq_offset_hz; u32 if_freq_accum; float dll_err, pll_err; int prev_ip, prev_qp; u32 n_updates; };
static_assert(sizeof(Live) == 32 && sizeof(gpsx_wloop_state_t) == 40 && offsetof(gpsx_wloop_state_t, code_phase_fine) == 4 &&
              offsetof(gpsx_wloop_state_t, n_updates) == 32, "gpsx_wloop_state_t layout");

// a window's gains and its length T in seconds; dll_c2 * T and pll_c2 * T are formed where they are used (k_track_wloop's are launch
// constants: the compiler hoists them out of its block loop)
struct Gains { float dll_c1, dll_c2, pll_c1, pll_c2, fll_c, T; };

// the window's end for a good channel: its six sums -> code phase, carrier offset and loop memory.  Aided (the k_track_waid_*
// kernels; include/gpsx.h gpsx_track_loop_weighted_aided): the carrier offset the window's correlators ran with -- read before the
// carrier step below -- feeds the code's slide forward, one product per window, ahead of the wrap.  code_per_hz == 0: no term, the
// unaided bytes.  Without Aided the parameter is not read and the function is what it was.
template <bool Aided = false>
__device__ __forceinline__ void window_update(Live &s, const Gains &g, int IE, int QE, int IP, int QP, int IL, int QL, float code_per_hz = 0.0f)
{
  // DLL
  const long long e2 = (long long)IE * IE + (long long)QE * QE, l2 = (long long)IL * IL + (long long)QL * QL;
  float d = 0.0f;
  if (e2 + l2 != 0)
    d = (float)(e2 - l2) / (float)(e2 + l2);
  float phase = s.code_phase_fine - (g.dll_c1 * (d - s.dll_err) + (g.dll_c2 * g.T) * d);
  if constexpr (Aided)
    if (code_per_hz != 0.0f)
      phase = phase - (code_per_hz * s.if_freq_offset_hz) * g.T;
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
  if (g.fll_c != 0.0f && s.n_updates > 0) {
    const long long cross = (long long)s.prev_ip * QP - (long long)s.prev_qp * IP;
    const long long dot = (long long)s.prev_ip * IP + (long long)s.prev_qp * QP;
    if (dot != 0)
      fe = gpsx_libm::atanf_fdlibm((float)cross / (float)dot) * kCyclesPerRadian / g.T;
  }
  s.if_freq_offset_hz = s.if_freq_offset_hz - ((g.pll_c1 * (p - s.pll_err) + (g.pll_c2 * g.T) * p) + g.fll_c * fe);
  s.pll_err = p;
  s.prev_ip = IP;
  s.prev_qp = QP;
  s.n_updates++;
}

// Where a lane stands: lane 4 c + k of a wave holds channel c of the wave (k = 0 / 1 / 2 = Early / Prompt / Late, k = 3 idles); wave w
// of workgroup g serves channels (4 g + w) cpw .. + cpw - 1 below n_ch (gpsx_track_loop_weighted_plan.hpp).
struct Lanes {
  int lane, c_l, k_l;
  int n_here;   // the wave's channels; 0: an idle wave of the last workgroup still stages and waits
  int ch_l;     // the quad's channel; beyond the wave's channels: its first (always a channel below n_ch)
  __device__ __forceinline__ bool in_wave() const { return c_l < n_here; }        // this lane's quad has a channel
  __device__ __forceinline__ bool mine() const { return in_wave() && k_l < 3; }   // ... and this lane a tap of it
};

__device__ __forceinline__ Lanes lanes_of(int n_ch, int cpw)
{
  Lanes l;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  l.lane = threadIdx.x & 63;
  l.c_l = l.lane >> 2;
  l.k_l = l.lane & 3;
  const int ch0 = ((int)blockIdx.x * 4 + wave) * cpw;
  l.n_here = ch0 < n_ch ? min(cpw, n_ch - ch0) : 0;
  l.ch_l = l.in_wave() ? ch0 + l.c_l : (l.n_here ? ch0 : 0);
  return l;
}

// the four carrier words, by the workgroup's first four threads (visible after the first block's barrier)
__device__ __forceinline__ void fill_carrier(uint2 *s_carrier)
{
  if (threadIdx.x < 4)
    s_carrier[threadIdx.x] = uint2{carrier_i(threadIdx.x), carrier_q(threadIdx.x)};
}

// A channel's loop state into registers.  Returns the validated PRN; 0: outside 1 .. 210 (reported here); -1: a padding channel.
__device__ __forceinline__ int load_state(const gpsx_wloop_state_t *st, const Lanes &l, u32 *bad_prn, Live &s)
{
  const int raw = st->prn;
  __builtin_memcpy(&s, &st->code_phase_fine, sizeof s);
  return raw == kTrackPadPrn ? -1 : track_prn(raw, bad_prn, l.mine() && l.k_l == 0);
}

// what a window's correlators use, fixed at its start (prn == 0: a bad channel, or no channel -- nothing but the accumulator moves)
struct Window { int tau = 0, prn = 0; u32 step = 0; };

// A window's start: tau from the code phase, the kernel's own rule, the NCO step from the carrier offset.  `rule(phase_ok)` sets
// w.prn and reports an unusable phase (weighted_tau): which lanes keep a PRN and which channels are reported is the kernel's to say.
template <typename Rule>
__device__ __forceinline__ void begin_window(Window &w, const Live &s, int if_hz, Rule rule)
{
  rule(weighted_tau(s.code_phase_fine, w.tau));
  w.step = nco_step_per_word((float)if_hz + s.if_freq_offset_hz);
}

}  // namespace trkwloop
}  // namespace gpsx
