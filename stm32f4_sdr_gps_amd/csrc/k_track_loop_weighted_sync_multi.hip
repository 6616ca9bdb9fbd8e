// k_track_loop_weighted_sync_multi.hip -- EXTENSION, not in the reference: the weighted loop with bit sync for MANY RECEIVERS in one
// launch, one IF stream each (include/gpsx.h gpsx_track_loop_weighted_sync_multi).
//
// k_track_waid_sync's text (k_track_loop_weighted_sync_kernel.inc, included here a third time: the block loop, the correlators,
// window_update<true>, the search, the decision and the record stores are that one copy) with other PLACES.  A workgroup of four
// waves is one receiver: it stages only that receiver's block into its two LDS plane buffers, keeps the one barrier per block, and
// its wave w serves the receiver's slots w cpw .. + cpw - 1 below ch_per_rx (cpw = ceil(ch_per_rx / 4): 64 slots fill four waves of
// sixteen quads).  Channel r ch_per_rx + j is slot j of receiver r: the states and the records are the single-stream call's arrays,
// so the lanes' channel index counts over all receivers and the record pitch is n_rx ch_per_rx -- the n_ch the text is given --
// while the lanes are bounded by ch_per_rx.  One instance: the aided text; a factor of 0 gives the unaided bytes by
// window_update's own clause.
#include <hip/hip_runtime.h>

#include <cstddef>

#include "gpsx_device.hpp"
#include "gpsx_kernels.hpp"
#include "gpsx_track_loop_weighted_plan.hpp"
#include "gpsx_track_weighted_wave.hpp"
#include "gpsx_track_wloop_parts.hpp"

namespace gpsx {

namespace {

static_assert(sizeof(gpsx_wsync_state_t) == 448 && sizeof(gpsx_wsync_rec_t) == 48 && sizeof(gpsx_wsync_cfg_t) == 68, "the sync loop's layouts");
static_assert(sizeof(gpsx_wmulti_t) == 16 && offsetof(gpsx_wmulti_t, rx_stride_blocks) == 8, "gpsx_wmulti_t layout");
static_assert(kTrackPadPrn == GPSX_PRN_NONE, "GPSX_PRN_NONE names the kernels' padding PRN");

struct alignas(4) Rec16 { u32 w[4]; };   // a third of a record at a dword-aligned address: one global_store_dwordx4

}  // namespace

namespace trkwloop {

// lanes_of for a receiver per workgroup: wave w serves slots w cpw .. + cpw - 1 below ch_per_rx of receiver blockIdx.x; ch_l is the
// channel's index over all receivers.  Beyond the wave's slots: its first; an idle wave: the receiver's first (always a channel).
__device__ __forceinline__ Lanes lanes_of_rx(int ch_per_rx, int cpw)
{
  Lanes l;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  l.lane = threadIdx.x & 63;
  l.c_l = l.lane >> 2;
  l.k_l = l.lane & 3;
  const int slot0 = wave * cpw, first = (int)blockIdx.x * ch_per_rx;   // (n_rx ch_per_rx <= INT32_MAX: the host checks)
  l.n_here = slot0 < ch_per_rx ? min(cpw, ch_per_rx - slot0) : 0;
  l.ch_l = first + (l.in_wave() ? slot0 + l.c_l : (l.n_here ? slot0 : 0));
  return l;
}

}  // namespace trkwloop

#define GPSX_WSYNC_KERNEL k_track_wsync_multi
#define GPSX_WSYNC_AIDED 1
#define GPSX_WSYNC_MULTI 1
#include "k_track_loop_weighted_sync_kernel.inc"
#undef GPSX_WSYNC_KERNEL
#undef GPSX_WSYNC_AIDED
#undef GPSX_WSYNC_MULTI

void launch_track_loop_weighted_sync_multi(hipStream_t s, const uint8_t *d_if_blocks_2bit, int n_blocks, int if_hz, const gpsx_wsync_cfg_t &cfg,
                                           float code_per_hz, int n_rx, int ch_per_rx, int rx_stride_blocks, gpsx_wsync_state_t *d_st,
                                           const uint32_t *d_trk_rep, gpsx_wsync_rec_t *d_rec, uint32_t *d_bad_prn)
{
  if (n_rx <= 0 || ch_per_rx <= 0 || ch_per_rx > kTrackLoopWeightedMultiMaxSlots || n_blocks <= 0)
    return;
  const TrackLoopWeightedPlan p = plan_track_loop_weighted_multi(n_rx, ch_per_rx);
  hipLaunchKernelGGL(k_track_wsync_multi, dim3(p.groups), dim3(256), 0, s, d_if_blocks_2bit, n_blocks, if_hz, cfg, d_st, n_rx * ch_per_rx, p.cpw,
                     d_trk_rep, d_rec, d_bad_prn, code_per_hz, ch_per_rx, (size_t)rx_stride_blocks * GPSX_BYTES_PER_MS_2BIT);
}

}  // namespace gpsx
