// k_track_loop_weighted.hip -- EXTENSION, not in the reference: a closed DLL / Costas PLL / FLL on WEIGHTED two-bit samples, the
// channel state resident in HBM (include/gpsx.h gpsx_track_loop_weighted).
//
// One launch advances every channel by K blocks: per block the weighted E/P/L correlators of gpsx_track_weighted_wave.hpp (the
// device function k_track_epl_weighted launches: the same integers), int32 window sums kept in the lanes, and at the end of every
// coherent window of n_coh blocks the loop arithmetic of the header's definition -- every float operation one IEEE single
// operation in the order written there (this file is built with -ffp-contract=off and correctly rounded division like the rest),
// the arctangent as glibc <= 2.40 computes it (gpsx_libm.hpp): gpsx_track_wloop_parts.hpp, shared with k_track_wsync, like the lanes.
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

#include "gpsx_device.hpp"
#include "gpsx_kernels.hpp"
#include "gpsx_track_loop_weighted_plan.hpp"
#include "gpsx_track_weighted_wave.hpp"
#include "gpsx_track_wloop_parts.hpp"

namespace gpsx {

#define GPSX_WLOOP_KERNEL k_track_wloop
#define GPSX_WLOOP_AIDED 0
#include "k_track_loop_weighted_kernel.inc"
#undef GPSX_WLOOP_KERNEL
#undef GPSX_WLOOP_AIDED

// the same text with the carrier aiding clause (include/gpsx.h gpsx_track_loop_weighted_aided)
#define GPSX_WLOOP_KERNEL k_track_waid_loop
#define GPSX_WLOOP_AIDED 1
#include "k_track_loop_weighted_kernel.inc"
#undef GPSX_WLOOP_KERNEL
#undef GPSX_WLOOP_AIDED

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

void launch_track_loop_weighted_aided(hipStream_t s, const uint8_t *d_if_blocks_2bit, int n_blocks, int if_hz, const gpsx_wloop_cfg_t &cfg,
                                      float code_per_hz, gpsx_wloop_state_t *d_st, int n_ch, const uint32_t *d_trk_rep, gpsx_wloop_rec_t *d_rec,
                                      uint32_t *d_bad_prn)
{
  if (n_ch <= 0 || n_blocks <= 0)
    return;
  const TrackLoopWeightedPlan p = plan_track_loop_weighted(n_ch);   // the unaided launch's plan
  hipLaunchKernelGGL(k_track_waid_loop, dim3(p.groups), dim3(256), 0, s, d_if_blocks_2bit, n_blocks, if_hz, cfg, d_st, n_ch, p.cpw, d_trk_rep,
                     d_rec, d_bad_prn, code_per_hz);
}

}  // namespace gpsx
