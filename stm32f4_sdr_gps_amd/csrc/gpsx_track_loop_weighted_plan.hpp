// gpsx_track_loop_weighted_plan.hpp -- the launch shape of k_track_wloop (k_track_loop_weighted.hip) and of k_track_wsync
// (k_track_loop_weighted_sync.hip), which takes the same plan: how many channels a wave serves one after the other and how many
// workgroups that takes.  The blocks run one after the other inside the kernel (the loop
// is a recurrence in time), so there is no block dimension to spread over: the shape depends on n_ch alone.  Pure host C++ (no
// HIP): tests/test_track_loop_weighted_plan.py compiles it with g++ and checks the shapes the GPU tests run.
#pragma once

namespace gpsx {

constexpr int kTrackLoopWeightedMaxCpw = 16;   // both kernels: lanes 4 c + k carry channel c's values, sixteen channels fill a wave

struct TrackLoopWeightedPlan {
  int cpw;           // channels per wave, 1 .. 16; wave w of workgroup g serves channels (4 g + w) cpw .. + cpw - 1 below n_ch
  unsigned groups;   // workgroups of four waves
};

// channels per wave: as many as leave ~4 workgroups per CU (launch_track_loop's rule), 16 at most
inline TrackLoopWeightedPlan plan_track_loop_weighted(int n_ch)
{
  long cpw = (long)n_ch / (4 * 256 * 4);
  cpw = cpw < 1 ? 1 : (cpw > kTrackLoopWeightedMaxCpw ? kTrackLoopWeightedMaxCpw : cpw);
  const unsigned groups = (unsigned)(((long)n_ch + 4 * cpw - 1) / (4 * cpw));
  return TrackLoopWeightedPlan{(int)cpw, groups};
}

// k_track_wsync_multi (k_track_loop_weighted_sync_multi.hip): one workgroup of four waves per receiver, wave w serves the receiver's
// slots w cpw .. + cpw - 1 below ch_per_rx.  Four waves of sixteen quads: 64 slots at most.  ch_per_rx outside 1 .. 64 or n_rx < 1:
// {0, 0}, no launch.  tests/test_track_loop_weighted_multi_plan.py checks it as the plan above is checked.
constexpr int kTrackLoopWeightedMultiMaxSlots = 4 * kTrackLoopWeightedMaxCpw;

inline TrackLoopWeightedPlan plan_track_loop_weighted_multi(int n_rx, int ch_per_rx)
{
  if (n_rx < 1 || ch_per_rx < 1 || ch_per_rx > kTrackLoopWeightedMultiMaxSlots)
    return TrackLoopWeightedPlan{0, 0u};
  return TrackLoopWeightedPlan{(ch_per_rx + 3) / 4, (unsigned)n_rx};
}

}  // namespace gpsx
