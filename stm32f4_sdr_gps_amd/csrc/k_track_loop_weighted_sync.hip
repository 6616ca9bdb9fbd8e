// k_track_loop_weighted_sync.hip -- EXTENSION, not in the reference: the closed loop on WEIGHTED two-bit samples with a 20 ms bit
// synchroniser per channel and windows aligned with every channel's own bit edge (include/gpsx.h gpsx_track_loop_weighted_sync;
// DESIGN.md 4.6.3).
//
// k_track_wloop's shape (k_track_loop_weighted.hip): lane 4 c + k of a wave holds channel c of the wave, the blocks run one after
// the other, the workgroup stages block b's planes into LDS buffer b & 1 and meets at ONE barrier per block that every wave
// reaches; the correlators are gpsx_track_weighted_wave.hpp's, the same integers; the loop update, the lanes' places, the state load
// and a window's start are gpsx_track_wloop_parts.hpp's, the same code.  What differs:
//  * the open window (six sums, its length) and the synchroniser's words come from the state and go back to it, so a launch may
//    be cut anywhere;
//  * a window's end is a per-lane condition (the mode's n_coh reached, or a locked channel's bit edge).  The update code is skipped
//    with one wave-uniform test when no channel of the wave ends a window at this block and runs under the lanes' mask otherwise;
//    the search's decision (once per 20 (sync_bits + 1) blocks) likewise;
//  * the search arrays (base[20][2], e[20]: 320 B per channel) stay in HBM / L2 and are updated in place by the quad's Prompt lane,
//    whose correlator result IS the block's prompt: one candidate per block (the prefix form), 16 B in and 16 B out, for channels
//    in SEARCH only;
//  * a record is three 16-byte stores by the quad's lanes 0 .. 2, and a slot in which no window ended gets the empty pattern.
#include <hip/hip_runtime.h>

#include <cstddef>

#include "gpsx_device.hpp"
#include "gpsx_kernels.hpp"
#include "gpsx_track_loop_weighted_plan.hpp"
#include "gpsx_track_weighted_wave.hpp"
#include "gpsx_track_wloop_parts.hpp"

namespace gpsx {

namespace {

static_assert(sizeof(gpsx_wsync_cfg_t) == 68 && offsetof(gpsx_wsync_cfg_t, search) == 16 && offsetof(gpsx_wsync_cfg_t, lock) == 36 &&
              offsetof(gpsx_wsync_cfg_t, sync_bits) == 56, "gpsx_wsync_cfg_t layout");
static_assert(sizeof(gpsx_wsync_state_t) == 448 && offsetof(gpsx_wsync_state_t, win_iq) == 40 && offsetof(gpsx_wsync_state_t, win_n) == 64 &&
              offsetof(gpsx_wsync_state_t, ms_count) == 68 && offsetof(gpsx_wsync_state_t, mode) == 72 && offsetof(gpsx_wsync_state_t, edge) == 76 &&
              offsetof(gpsx_wsync_state_t, bit_ip) == 80 && offsetof(gpsx_wsync_state_t, search_n) == 84 &&
              offsetof(gpsx_wsync_state_t, prev_best_p1) == 88 && offsetof(gpsx_wsync_state_t, sync_rounds) == 92 &&
              offsetof(gpsx_wsync_state_t, p_i) == 96 && offsetof(gpsx_wsync_state_t, last_best_e) == 104 &&
              offsetof(gpsx_wsync_state_t, last_opp_e) == 112 && offsetof(gpsx_wsync_state_t, zero) == 120 &&
              offsetof(gpsx_wsync_state_t, base) == 128 && offsetof(gpsx_wsync_state_t, e) == 288, "gpsx_wsync_state_t layout");
static_assert(sizeof(gpsx_wsync_rec_t) == 48 && offsetof(gpsx_wsync_rec_t, end_block) == 36 && offsetof(gpsx_wsync_rec_t, flags) == 40 &&
              offsetof(gpsx_wsync_rec_t, bit_ip) == 44, "gpsx_wsync_rec_t layout");

struct alignas(4) Rec16 { u32 w[4]; };   // a third of a record at a dword-aligned address: one global_store_dwordx4

}  // namespace

#define GPSX_WSYNC_KERNEL k_track_wsync
#define GPSX_WSYNC_AIDED 0
#include "k_track_loop_weighted_sync_kernel.inc"
#undef GPSX_WSYNC_KERNEL
#undef GPSX_WSYNC_AIDED

// the same text with the carrier aiding clause (include/gpsx.h gpsx_track_loop_weighted_sync_aided)
#define GPSX_WSYNC_KERNEL k_track_waid_sync
#define GPSX_WSYNC_AIDED 1
#include "k_track_loop_weighted_sync_kernel.inc"
#undef GPSX_WSYNC_KERNEL
#undef GPSX_WSYNC_AIDED

void launch_track_loop_weighted_sync(hipStream_t s, const uint8_t *d_if_blocks_2bit, int n_blocks, int if_hz, const gpsx_wsync_cfg_t &cfg,
                                     gpsx_wsync_state_t *d_st, int n_ch, const uint32_t *d_trk_rep, gpsx_wsync_rec_t *d_rec,
                                     uint32_t *d_bad_prn)
{
  if (n_ch <= 0 || n_blocks <= 0)
    return;
  const TrackLoopWeightedPlan p = plan_track_loop_weighted(n_ch);   // the same shape as k_track_wloop's (gpsx_track_loop_weighted_plan.hpp)
  hipLaunchKernelGGL(k_track_wsync, dim3(p.groups), dim3(256), 0, s, d_if_blocks_2bit, n_blocks, if_hz, cfg, d_st, n_ch, p.cpw, d_trk_rep,
                     d_rec, d_bad_prn);
}

void launch_track_loop_weighted_sync_aided(hipStream_t s, const uint8_t *d_if_blocks_2bit, int n_blocks, int if_hz, const gpsx_wsync_cfg_t &cfg,
                                           float code_per_hz, gpsx_wsync_state_t *d_st, int n_ch, const uint32_t *d_trk_rep,
                                           gpsx_wsync_rec_t *d_rec, uint32_t *d_bad_prn)
{
  if (n_ch <= 0 || n_blocks <= 0)
    return;
  const TrackLoopWeightedPlan p = plan_track_loop_weighted(n_ch);   // the unaided launch's plan
  hipLaunchKernelGGL(k_track_waid_sync, dim3(p.groups), dim3(256), 0, s, d_if_blocks_2bit, n_blocks, if_hz, cfg, d_st, n_ch, p.cpw, d_trk_rep,
                     d_rec, d_bad_prn, code_per_hz);
}

}  // namespace gpsx
