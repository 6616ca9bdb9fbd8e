// gpsx_track_weighted_plan.hpp -- the launch shape of k_track_epl_weighted (k_track_weighted.hip): how many channels a wave serves
// one after the other and how many workgroups that takes.  Pure host C++ (no HIP): tests/test_track_weighted_plan.py compiles it
// with g++ and checks the shapes the GPU tests run, so that what they claim to cover is what the launcher launches.
#pragma once

namespace gpsx {

constexpr int kTrackWeightedMaxCpw = 16;   // lanes 4 c + k carry channel c's values: sixteen channels fill a wave

struct TrackWeightedPlan {
  int cpw;             // channels per wave, 1 .. 16; wave w of workgroup g serves channels (4 g + w) cpw .. + cpw - 1 below n_ch
  unsigned groups;     // workgroups of four waves along x (the blocks are along y)
  bool spread_bound;   // cpw was set by ceil(n_ch / 4), not by the launch size: few channels, many blocks
};

// channels per wave: as many as leave ~4 workgroups per CU over the (block, channel group) units, 16 at most, and no more than
// spread the channels over a workgroup's four waves
inline TrackWeightedPlan plan_track_weighted(int n_ch, int n_blocks)
{
  long cpw = (long)n_ch * n_blocks / (4 * 256 * 4);
  const long spread = ((long)n_ch + 3) / 4;
  const bool spread_bound = cpw > spread && spread <= kTrackWeightedMaxCpw;
  cpw = cpw > spread ? spread : cpw;
  cpw = cpw < 1 ? 1 : (cpw > kTrackWeightedMaxCpw ? kTrackWeightedMaxCpw : cpw);
  const unsigned groups = (unsigned)(((long)n_ch + 4 * cpw - 1) / (4 * cpw));
  return TrackWeightedPlan{(int)cpw, groups, spread_bound};
}

}  // namespace gpsx
