// k_acq_hyb.hip -- EXTENSION, not in the reference: the weighted two-bit grid over n_seg coherent windows of n_coh blocks each,
// the windows' magnitudes summed (include/gpsx.h gpsx_acq_grid_weighted_hyb).
//
//   segment j of a search: exactly k_acq_coh.hip's window starting at block j * n_coh of the search -- the NCO accumulator from 0
//   at the segment's first block, chained through its n_coh blocks; I_j(tau), Q_j(tau) exact; m_j = floor(sqrt(I_j^2 + Q_j^2))
//   E(tau) = sum_j m_j(tau)   (n_seg <= 128: E < 2^28)
//   per (search, PRN, Doppler): max E, the first tau reaching it, sum E mod 2^32 (the record of gpsx_acq_grid_weighted_ms).
// Two kernels, records identical bit for bit; the window's parts are k_acq_coh.hip's (gpsx_acq_coh_parts.hpp):
//   k_acq_hyb_mx   matrix cores, a workgroup per cluster (search, Doppler bin, 32 PRNs).  Per segment the pre-sum, S_0 and the 17
//                  int8 passes of k_acq_coh_mx; a pass's exact roots are added into the cluster's u32 running sums in HBM scratch
//                  (k_acq_wmx_ms's layout: [sample offset][wave][tile][quad of PRN rows][lane] as uint4, a kilobyte per wave
//                  instruction).  The first segment writes without reading, the last reads, adds and folds into the LDS slots
//                  without writing.  Half of a sample offset's sums (four half tiles, 32 registers) are requested before the pass
//                  whose epilogue adds them, every further half tile's four half tiles ahead of its roots.
//   k_acq_hyb_vec  vector ALU, a workgroup per (search, Doppler bin, 8 PRNs): sample offset outer, segments inner, a thread's
//                  4 chip offsets x 8 PRNs of E in registers -- no scratch; a segment's pre-sum is redone per sample offset
//                  (a row S_t0 needs all sixteen polyphase planes), beside 32 768 v_dot2_i32_i16 per thread and offset.
#include "gpsx_device.hpp"
#include "gpsx_kernels.hpp"
#include "gpsx_acq_coh_parts.hpp"

namespace gpsx {

namespace {

// (the chip signs and S_0 below are k_acq_coh_mx's preamble, the rows and the v_dot2 loop further down k_acq_coh_vec's: written out
//  there -- called as functions they changed those kernels' code)
// the cluster's chip signs: A fragments of the 32 PRNs of set `set`
__device__ __forceinline__ void coh_mx_chips(CohMxShared &sh, const uint8_t *chips_all, const uint8_t *prns, int n_prn, int set, int tid)
{
  for (int i = tid; i < 32 * 2 * 32 * 4; i += kCohThreads) {
    const int dw = i & 3, p = (i >> 2) & 31, hh = (i >> 7) & 1, kappa = i >> 8;
    const int slot = 32 * set + p;
    u32 word = 0;
    if (slot < n_prn) {
      const uint8_t *ch = chips_all + (size_t)prns[slot] * 1024;
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const int c = 32 * kappa + 16 * hh + 4 * dw + e;
        word |= (c < kChips ? (ch[c] ? 0xFFu : 0x01u) : 0u) << (8 * e);
      }
    }
    reinterpret_cast<u32 *>(&sh.chips[0][0][0])[i] = word;
  }
}

// S_0 of both streams from the planes
__device__ __forceinline__ void coh_mx_s0(CohMxShared &sh, int tid)
{
  for (int i = tid; i < 2 * 1024; i += kCohThreads) {
    const int st = i >> 10, k = i & 1023;
    int s = 0;
#pragma unroll
    for (int t = 0; t < 16; t++)
      s += sh.mt[st][t][k];
    sh.s0[st][k] = (int16_t)s;
  }
}

constexpr int kHybRecsPerWave = 16 * 64;    // uint4 per (sample offset, wave): 4 tiles x 4 quads of PRN rows x 64 lanes

// half a tile's running sums (registers 8 (half & 1) .. + 7 of tile half / 2) of this lane
__device__ __forceinline__ void hyb_request(const uint4 *rec, int half, int lane, uint4 (&r)[2])
{
#pragma unroll
  for (int c = 0; c < 2; c++)
    r[c] = rec[(half * 2 + c) * 64 + lane];
}

constexpr int kHybAhead = 4;                // half tiles of running sums requested before the pass whose epilogue adds them

// sample offset t0's roots of this segment into the running sums, in halves of a tile; `pre`: the first kHybAhead halves' sums,
// requested before the pass; half hf + kHybAhead is requested before half hf takes its roots.  first: nothing is read; last:
// nothing is written, E goes into the PRNs' slots of this lane (k_acq_coh_mx's slots)
__device__ __forceinline__ void hyb_epilogue(CohMxShared &sh, int q0, int lane, int t0, const v16i (&acc)[2][kCohTiles], uint4 *rec,
                                             uint4 (&pre)[kHybAhead + 1][2], bool first, bool last)
{
  const int n = lane & 31, h = lane >> 5;
#pragma unroll
  for (int hf = 0; hf < 2 * kCohTiles; hf++) {
    const int j = hf >> 1, r0 = 8 * (hf & 1);
    if (!first && hf + kHybAhead < 2 * kCohTiles)
      hyb_request(rec, hf + kHybAhead, lane, pre[(hf + kHybAhead) % (kHybAhead + 1)]);
    const int q = 32 * (q0 + j) + n;
    const bool exists = q < kChips;                    // (chip offset 1023 does not exist: tile 31, lane 31)
    u32 e[8];
#pragma unroll
    for (int i = 0; i < 8; i++)
      e[i] = exists ? coh_root(acc[0][j][r0 + i], acc[1][j][r0 + i]) : 0u;
    if (!first) {
      const uint4 (&have)[2] = pre[hf % (kHybAhead + 1)];
#pragma unroll
      for (int c = 0; c < 2; c++) {
        e[4 * c + 0] += have[c].x;
        e[4 * c + 1] += have[c].y;
        e[4 * c + 2] += have[c].z;
        e[4 * c + 3] += have[c].w;
      }
    }
    if (!last) {
#pragma unroll
      for (int c = 0; c < 2; c++)
        rec[(hf * 2 + c) * 64 + lane] = make_uint4(e[4 * c], e[4 * c + 1], e[4 * c + 2], e[4 * c + 3]);
    } else {
#pragma unroll
      for (int i = 0; i < 8; i++) {
        const int r = r0 + i, p = (r & 3) + 8 * (r >> 2) + 4 * h;   // the MFMA's row of register r in lane half h
        atomicMax(&sh.best[p][n], exists ? coh_key(e[i], 16 * q + t0) : 0ull);
        atomicAdd(&sh.total[p][n], e[i]);
      }
    }
  }
}

// sample offset t0's rows from the planes: S_t0[k] = sum_u (u >= t0 ? mt[u][k] : mt[u][k + 1])
__device__ __forceinline__ void coh_vec_rows(CohVecShared &sh, int t0, int tid)
{
  for (int i = tid; i < 2 * kVRowDw; i += kCohVThreads) {
    const int st = i / kVRowDw, d = i % kVRowDw;
    u32 word = 0;
#pragma unroll
    for (int e = 0; e < 2; e++) {
      const int x = 2 * d + e;
      int s = 0;
      if (x < 2 * kChips) {
        const int k = x >= kChips ? x - kChips : x, k1 = k == kChips - 1 ? 0 : k + 1;
#pragma unroll
        for (int u = 0; u < 16; u++)
          s += sh.mt[st][u][u >= t0 ? k : k1];
      }
      word |= ((u32)s & 0xFFFFu) << (16 * e);
    }
    sh.rows[st][d] = word;
  }
}

// the correlations of the rows: thread tid owns chip offsets q = tid + 256 j, two chips per step
__device__ __forceinline__ void coh_vec_correlate(const CohVecShared &sh, int tid, int (&acc)[4][2][kCohVG])
{
#pragma unroll
  for (int j = 0; j < 4; j++)
#pragma unroll
    for (int st = 0; st < 2; st++)
#pragma unroll
      for (int g = 0; g < kCohVG; g++)
        acc[j][st][g] = 0;
  u32 prev[4][2];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int q = min(tid + 256 * j, kChips - 1);
    prev[j][0] = sh.rows[0][q >> 1];
    prev[j][1] = sh.rows[1][q >> 1];
  }
#pragma unroll 2
  for (int c2 = 0; c2 < 512; c2++) {
    v2s win[4][2];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int q = min(tid + 256 * j, kChips - 1);
#pragma unroll
      for (int st = 0; st < 2; st++) {
        const u32 nxt = sh.rows[st][(q >> 1) + c2 + 1];
        win[j][st] = __builtin_bit_cast(v2s, __builtin_amdgcn_alignbit(nxt, prev[j][st], 16u * (u32)(q & 1)));
        prev[j][st] = nxt;
      }
    }
#pragma unroll
    for (int g = 0; g < kCohVG; g++) {
      const v2s cw = __builtin_bit_cast(v2s, sh.chips[g][c2]);   // (wave-uniform address: one broadcast read)
#pragma unroll
      for (int j = 0; j < 4; j++) {
        acc[j][0][g] = __builtin_amdgcn_sdot2(win[j][0], cw, acc[j][0][g], false);
        acc[j][1][g] = __builtin_amdgcn_sdot2(win[j][1], cw, acc[j][1][g], false);
      }
    }
  }
}

}  // namespace

__global__ __launch_bounds__(kCohThreads, 1) void k_acq_hyb_mx(const uint8_t *__restrict__ if_blocks, int stride_blocks, int n_coh, int n_seg,
                                                               int n_prn, const uint8_t *__restrict__ chips_all,
                                                               const uint8_t *__restrict__ prns, int if_hz, int dopp_min_hz, int dopp_step_hz,
                                                               int n_dopp, int use_magnitude, int cluster_lo, uint4 *scratch,
                                                               gpsx_peak_t *__restrict__ peaks)
{
  __shared__ CohMxShared sh;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = lane & 31, h = lane >> 5, q0 = kCohTiles * wave;
  const int n_sets = (n_prn + 31) / 32;
  const int cluster = cluster_lo + (int)blockIdx.x;
  const int set = cluster % n_sets, sd = cluster / n_sets, dopp = sd % n_dopp, search = sd / n_dopp;
  const u32 step_word = nco_step_per_word((float)(if_hz + dopp_min_hz + dopp * dopp_step_hz));
  const uint8_t *blk0 = if_blocks + (size_t)search * stride_blocks * GPSX_BYTES_PER_MS_2BIT;
  // this workgroup's running sums: [sample offset][wave] slices of kHybRecsPerWave records
  uint4 *const recs = scratch + (size_t)blockIdx.x * (16 * 8 * kHybRecsPerWave) + (size_t)wave * kHybRecsPerWave;

  coh_mx_chips(sh, chips_all, prns, n_prn, set, tid);
  for (int i = tid; i < 32 * 32; i += kCohThreads) {
    (&sh.best[0][0])[i] = 0;
    (&sh.total[0][0])[i] = 0;
  }
#pragma unroll 1
  for (int seg = 0; seg < n_seg; seg++) {
    const bool first = seg == 0, last = seg == n_seg - 1;
    __syncthreads();                // (the previous segment's passes are done with the planes and rows)
    // ---- the segment's planes from its own first block, the accumulator from 0; S_0; the first row ---------------------------
    coh_presum(sh.mt, blk0 + (size_t)seg * n_coh * GPSX_BYTES_PER_MS_2BIT, n_coh, step_word, use_magnitude, tid, kCohThreads);
    __syncthreads();
    coh_mx_s0(sh, tid);
    __syncthreads();
    coh_build_rows(sh, 0, 0, tid);
    // ---- k_acq_coh_mx's 17 passes; the epilogue of sample offset p - 1 behind pass p ------------------------------------------
    v16i acc[2][kCohTiles];
#pragma unroll
    for (int st = 0; st < 2; st++)
#pragma unroll
      for (int j = 0; j < kCohTiles; j++)
#pragma unroll
        for (int r = 0; r < 16; r++)
          acc[st][j][r] = 0;
#pragma unroll 1
    for (int p = 0; p < kCohPasses; p++) {
      __syncthreads();
      if (p + 1 < kCohPasses)
        coh_build_rows(sh, p + 1, (p + 1) & 1, tid);
      uint4 *const rec = recs + (size_t)(p ? p - 1 : 0) * 8 * kHybRecsPerWave;
      uint4 pre[kHybAhead + 1][2] = {};
      if (p && !first) {
#pragma unroll
        for (int hf = 0; hf < kHybAhead; hf++)
          hyb_request(rec, hf, lane, pre[hf]);
      }
      coh_pass(sh, p & 1, q0, n, h, acc);
      if (p == 0) {
#pragma unroll
        for (int st = 0; st < 2; st++)
#pragma unroll
          for (int j = 0; j < kCohTiles; j++)
            acc[st][j] <<= 4;
      } else {
        hyb_epilogue(sh, q0, lane, p - 1, acc, rec, pre, first, last);
      }
    }
  }
  __syncthreads();
  // ---- one record per (search, PRN, Doppler): the PRN's 32 lane slots --------------------------------------------------------
  if (tid < 32 && 32 * set + tid < n_prn) {
    unsigned long long k = 0;
    u32 t = 0;
    for (int l = 0; l < 32; l++) {
      const int ll = (l + tid) & 31;
      const unsigned long long v = sh.best[tid][ll];
      k = v > k ? v : k;
      t += sh.total[tid][ll];
    }
    coh_record(&peaks[((size_t)search * n_prn + 32 * set + tid) * n_dopp + dopp], k, t);
  }
}

__global__ __launch_bounds__(kCohVThreads) void k_acq_hyb_vec(const uint8_t *__restrict__ if_blocks, int stride_blocks, int n_coh, int n_seg,
                                                              int n_prn, const uint8_t *__restrict__ chips_all,
                                                              const uint8_t *__restrict__ prns, int if_hz, int dopp_min_hz, int dopp_step_hz,
                                                              int n_dopp, int use_magnitude, gpsx_peak_t *__restrict__ peaks)
{
  __shared__ CohVecShared sh;
  const int tid = threadIdx.x;
  const int n_groups = (n_prn + kCohVG - 1) / kCohVG;
  const int group = (int)blockIdx.x % n_groups, dopp = ((int)blockIdx.x / n_groups) % n_dopp, search = (int)blockIdx.x / (n_groups * n_dopp);
  const u32 step_word = nco_step_per_word((float)(if_hz + dopp_min_hz + dopp * dopp_step_hz));
  const uint8_t *blk0 = if_blocks + (size_t)search * stride_blocks * GPSX_BYTES_PER_MS_2BIT;

  coh_vec_chips(sh, chips_all, prns, n_prn, group, tid);
  if (tid < kCohVG) {
    sh.best[tid] = 0;
    sh.total[tid] = 0;
  }
  unsigned long long best[kCohVG];
  u32 total[kCohVG];
#pragma unroll
  for (int g = 0; g < kCohVG; g++) {
    best[g] = 0;
    total[g] = 0;
  }
#pragma unroll 1
  for (int t0 = 0; t0 < 16; t0++) {
    u32 e_sum[4][kCohVG];
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
      for (int g = 0; g < kCohVG; g++)
        e_sum[j][g] = 0;
#pragma unroll 1
    for (int seg = 0; seg < n_seg; seg++) {
      // (the planes are free: every thread passed the barrier behind the previous step's rows, which were their last readers)
      coh_presum(sh.mt, blk0 + (size_t)seg * n_coh * GPSX_BYTES_PER_MS_2BIT, n_coh, step_word, use_magnitude, tid, kCohVThreads);
      __syncthreads();              // (the planes are written / the previous step's rows are read)
      coh_vec_rows(sh, t0, tid);
      __syncthreads();
      int acc[4][2][kCohVG];
      coh_vec_correlate(sh, tid, acc);
#pragma unroll
      for (int j = 0; j < 4; j++)
#pragma unroll
        for (int g = 0; g < kCohVG; g++)
          e_sum[j][g] += coh_root(acc[j][0][g], acc[j][1][g]);
    }
    // ---- this offset's sums into the PRNs' running best / sum ------------------------------------------------------------------
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int q = tid + 256 * j;
      if (q >= kChips)
        continue;
#pragma unroll
      for (int g = 0; g < kCohVG; g++) {
        const unsigned long long key = coh_key(e_sum[j][g], 16 * q + t0);
        best[g] = key > best[g] ? key : best[g];
        total[g] += e_sum[j][g];
      }
    }
  }
#pragma unroll
  for (int g = 0; g < kCohVG; g++) {
    const unsigned long long b = coh_wave_max_u64(best[g]);
    const u32 t = wave_sum_to_lane63(total[g]);
    if ((tid & 63) == 63) {
      atomicMax(&sh.best[g], b);
      atomicAdd(&sh.total[g], t);
    }
  }
  __syncthreads();
  if (tid < kCohVG && group * kCohVG + tid < n_prn)
    coh_record(&peaks[((size_t)search * n_prn + group * kCohVG + tid) * n_dopp + dopp], sh.best[tid], sh.total[tid]);
}

void launch_acq_hyb_mx(hipStream_t s, const uint8_t *d_if_blocks, int stride_blocks, int n_coh, int n_seg, int n_prn,
                       const uint8_t *d_chips_all, const uint8_t *d_prns, int if_hz, int dopp_min_hz, int dopp_step_hz, int n_dopp,
                       int use_magnitude, int cluster_lo, int n_clusters, void *d_scratch, gpsx_peak_t *d_peaks)
{
  hipLaunchKernelGGL(k_acq_hyb_mx, dim3((unsigned)n_clusters), dim3(kCohThreads), 0, s, d_if_blocks, stride_blocks, n_coh, n_seg, n_prn,
                     d_chips_all, d_prns, if_hz, dopp_min_hz, dopp_step_hz, n_dopp, use_magnitude, cluster_lo,
                     static_cast<uint4 *>(d_scratch), d_peaks);
}

void launch_acq_hyb_vec(hipStream_t s, const uint8_t *d_if_blocks, int n_search, int stride_blocks, int n_coh, int n_seg, int n_prn,
                        const uint8_t *d_chips_all, const uint8_t *d_prns, int if_hz, int dopp_min_hz, int dopp_step_hz, int n_dopp,
                        int use_magnitude, gpsx_peak_t *d_peaks)
{
  hipLaunchKernelGGL(k_acq_hyb_vec, dim3((unsigned)(n_search * n_dopp * ((n_prn + kCohVG - 1) / kCohVG))), dim3(kCohVThreads), 0, s,
                     d_if_blocks, stride_blocks, n_coh, n_seg, n_prn, d_chips_all, d_prns, if_hz, dopp_min_hz, dopp_step_hz, n_dopp,
                     use_magnitude, d_peaks);
}

}  // namespace gpsx
