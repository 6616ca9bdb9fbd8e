// k_acq_coh.hip -- EXTENSION, not in the reference: the weighted two-bit grid over n_coh blocks integrated COHERENTLY
// (include/gpsx.h gpsx_acq_grid_weighted_coh).
//
//   block b of a search: the weighted values of gpsx_acq_grid_weighted (v in {0, +-1, +-3}), wiped by the reference's NCO started
//   from acc_b = b * 511 * step32 -- the accumulator one block leaves to the next (PM/GPS/gps_misc.c:244-274, chained)
//   I(tau) = sum_b sum_n vI_b[n] c[((n - tau) mod 16368) / 16],  Q likewise,  m(tau) = floor(sqrt(I^2 + Q^2)) exactly
//   per (search, PRN, Doppler): max m, the first tau reaching it, sum m mod 2^32 (the record of gpsx_acq_grid_weighted_ms).
// The C/A code repeats every block, so the correlation of the n_coh blocks is ONE correlation of their sum: a workgroup adds the
// wiped blocks sample by sample into M_I, M_Q in [-3 n_coh, 3 n_coh] (int8 in LDS; nothing goes through HBM) and correlates that.
//   I(16 q + t0) = sum_c s[c] S_t0[(q + c) mod 1023],  s = 1 - 2 chip (0 for chip 1023),  S_t0[k] = sum_{j < 16} M(16 k + t0 + j)
// M is kept polyphase: mt[t][k] = M(16 k + t), k < 1023 (k = 1022: the sixteen unmixed samples, 0), so a sample offset's rows are
// contiguous.  Two kernels, records identical bit for bit:
//   k_acq_coh_mx   matrix cores, a workgroup per cluster (search, Doppler bin, 32 PRNs): the Toeplitz GEMM of k_acq_mxw on
//                  v_mfma_i32_32x32x32_i8 -- A = the 32 PRNs' signs (+-1 int8, no start value), B[c][q] = the row entry q + c.
//                  Offset 0 in two passes (S_0 = 16 hi + lo, |hi| <= 60, |lo| <= 8: the accumulators are shifted left by four
//                  between them), every further offset in one on S_{t0+1}[k] - S_t0[k] = M(16 (k + 1) + t0) - M(16 k + t0),
//                  |.| <= 6 n_coh <= 120: int8.  Exact int32 accumulators (|I| <= 3 x 16352 x 20 = 981 120).
//   k_acq_coh_vec  vector ALU, a workgroup per (search, Doppler bin, 8 PRNs): per sample offset the two rows of S_t0 as int16
//                  (|S| <= 960) and v_dot2_i32_i16, two chips per instruction.  No matrix cores.
// Neither needs scratch memory.
#include "gpsx_device.hpp"
#include "gpsx_kernels.hpp"
#include "gpsx_acq_coh_parts.hpp"

namespace gpsx {

namespace {

// sample offset t0's 64 hypotheses per lane (4 tiles x 16 PRNs) into the PRNs' slots of this lane
__device__ __forceinline__ void coh_epilogue(CohMxShared &sh, int q0, int n, int h, int t0, const v16i (&acc)[2][kCohTiles])
{
#pragma unroll
  for (int r = 0; r < 16; r++) {
    unsigned long long best = 0;
    u32 total = 0;
#pragma unroll
    for (int j = 0; j < kCohTiles; j++) {
      const int q = 32 * (q0 + j) + n;                 // (chip offset 1023 does not exist: tile 31, lane 31)
      const u32 m = q < kChips ? coh_root(acc[0][j][r], acc[1][j][r]) : 0u;
      const unsigned long long key = q < kChips ? coh_key(m, 16 * q + t0) : 0ull;
      best = key > best ? key : best;
      total += m;
    }
    const int p = (r & 3) + 8 * (r >> 2) + 4 * h;    // the MFMA's row of register r in lane half h
    atomicMax(&sh.best[p][n], best);
    atomicAdd(&sh.total[p][n], total);
  }
}

}  // namespace

__global__ __launch_bounds__(kCohThreads, 1) void k_acq_coh_mx(const uint8_t *__restrict__ if_blocks, int stride_blocks, int n_coh, int n_prn,
                                                               const uint8_t *__restrict__ chips_all, const uint8_t *__restrict__ prns,
                                                               int if_hz, int dopp_min_hz, int dopp_step_hz, int n_dopp, int use_magnitude,
                                                               gpsx_peak_t *__restrict__ peaks)
{
  __shared__ CohMxShared sh;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = lane & 31, h = lane >> 5, q0 = kCohTiles * wave;
  const int n_sets = (n_prn + 31) / 32;
  const int cluster = (int)blockIdx.x;
  const int set = cluster % n_sets, sd = cluster / n_sets, dopp = sd % n_dopp, search = sd / n_dopp;
  const u32 step_word = nco_step_per_word((float)(if_hz + dopp_min_hz + dopp * dopp_step_hz));
  const uint8_t *blk0 = if_blocks + (size_t)search * stride_blocks * GPSX_BYTES_PER_MS_2BIT;

  // ---- the cluster's chip signs, the result slots, the pre-summed planes ----------------------------------------------------
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
  for (int i = tid; i < 32 * 32; i += kCohThreads) {
    (&sh.best[0][0])[i] = 0;
    (&sh.total[0][0])[i] = 0;
  }
  coh_presum(sh.mt, blk0, n_coh, step_word, use_magnitude, tid, kCohThreads);
  __syncthreads();
  for (int i = tid; i < 2 * 1024; i += kCohThreads) {
    const int st = i >> 10, k = i & 1023;
    int s = 0;
#pragma unroll
    for (int t = 0; t < 16; t++)
      s += sh.mt[st][t][k];
    sh.s0[st][k] = (int16_t)s;
  }
  __syncthreads();
  coh_build_rows(sh, 0, 0, tid);

  // ---- 17 passes, one barrier each: the row of pass p + 1 is built into the other buffer before pass p's MFMAs ---------------
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
    coh_pass(sh, p & 1, q0, n, h, acc);
    if (p == 0) {
#pragma unroll
      for (int st = 0; st < 2; st++)
#pragma unroll
        for (int j = 0; j < kCohTiles; j++)
          acc[st][j] <<= 4;
    } else {
      coh_epilogue(sh, q0, n, h, p - 1, acc);
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

__global__ __launch_bounds__(kCohVThreads) void k_acq_coh_vec(const uint8_t *__restrict__ if_blocks, int stride_blocks, int n_coh, int n_prn,
                                                              const uint8_t *__restrict__ chips_all, const uint8_t *__restrict__ prns,
                                                              int if_hz, int dopp_min_hz, int dopp_step_hz, int n_dopp, int use_magnitude,
                                                              gpsx_peak_t *__restrict__ peaks)
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
  coh_presum(sh.mt, blk0, n_coh, step_word, use_magnitude, tid, kCohVThreads);

  unsigned long long best[kCohVG];
  u32 total[kCohVG];
#pragma unroll
  for (int g = 0; g < kCohVG; g++) {
    best[g] = 0;
    total[g] = 0;
  }
#pragma unroll 1
  for (int t0 = 0; t0 < 16; t0++) {
    __syncthreads();                // (the planes are written / the previous offset's rows are read)
    // ---- this offset's rows: S_t0[k] = sum_u (u >= t0 ? mt[u][k] : mt[u][k + 1]) ------------------------------------------------
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
    __syncthreads();
    // ---- the correlations: thread tid owns chip offsets q = tid + 256 j, two chips per step -----------------------------------
    int acc[4][2][kCohVG];
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
    // ---- this offset's magnitudes into the PRNs' running best / sum ------------------------------------------------------------
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int q = tid + 256 * j;
      if (q >= kChips)
        continue;
#pragma unroll
      for (int g = 0; g < kCohVG; g++) {
        const u32 m = coh_root(acc[j][0][g], acc[j][1][g]);
        const unsigned long long key = coh_key(m, 16 * q + t0);
        best[g] = key > best[g] ? key : best[g];
        total[g] += m;
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

void launch_acq_coh(hipStream_t s, bool mx, const uint8_t *d_if_blocks, int n_search, int stride_blocks, int n_coh, int n_prn,
                    const uint8_t *d_chips_all, const uint8_t *d_prns, int if_hz, int dopp_min_hz, int dopp_step_hz, int n_dopp,
                    int use_magnitude, gpsx_peak_t *d_peaks)
{
  if (mx)
    hipLaunchKernelGGL(k_acq_coh_mx, dim3((unsigned)(n_search * n_dopp * ((n_prn + 31) / 32))), dim3(kCohThreads), 0, s, d_if_blocks,
                       stride_blocks, n_coh, n_prn, d_chips_all, d_prns, if_hz, dopp_min_hz, dopp_step_hz, n_dopp, use_magnitude, d_peaks);
  else
    hipLaunchKernelGGL(k_acq_coh_vec, dim3((unsigned)(n_search * n_dopp * ((n_prn + kCohVG - 1) / kCohVG))), dim3(kCohVThreads), 0, s,
                       d_if_blocks, stride_blocks, n_coh, n_prn, d_chips_all, d_prns, if_hz, dopp_min_hz, dopp_step_hz, n_dopp,
                       use_magnitude, d_peaks);
}

}  // namespace gpsx
