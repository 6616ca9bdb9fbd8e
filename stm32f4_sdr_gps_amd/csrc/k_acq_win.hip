// k_acq_win.hip -- EXTENSION, not in the reference: the weighted two-bit grid's energy in a WINDOW around each predicted satellite
// (include/gpsx.h gpsx_acq_window_weighted).
//
//   per (receiver r, PRN index p): gpsx_wpred's record names a code phase and a Doppler; the window is the 2 W + 1 phases
//   (c + j) mod 16368, j = -W .. W, around c = rint(code_phase) and the 2 D + 1 bins around dc = rint((f_hz - dopp_min) / dopp_step),
//   clipped to the lattice.  Per bin E(tau) is k_acq_hyb.hip's, evaluated at the window's phases only:
//   segment j = k_acq_coh.hip's window from block j * n_coh of the search (the NCO from 0 there, chained through its n_coh blocks),
//   I_j(tau), Q_j(tau) exact, m_j = floor(sqrt(I_j^2 + Q_j^2)), E = sum_j m_j.
//   Record: max E over the window, the numerically smallest tau reaching it, and the mean of the window's phases further than
//   `guard` from that tau, scaled by 16368 into the grids' `sum` (floor(S_far * 16368 / |F|) mod 2^32).
// One workgroup of 256 threads per (receiver, PRN index, k = 0 .. 2 D), bin dc - D + k.  Per segment the pre-sum of
// gpsx_acq_coh_parts.hpp puts the polyphase int8 planes into LDS; per sample offset t0 the int16 rows S_t0 (k_acq_coh_vec's, built
// once for t0 = 0 and then updated: S_t0[k] = S_(t0-1)[k] - M(16 k + t0 - 1) + M(16 (k + 1) + t0 - 1)) and v_dot2_i32_i16 against the
// PRN's chip pairs.  At most 256 window phases share a sample offset, so a thread owns one; where there are fewer, P = 2 .. 64
// adjacent lanes share a phase's 512 chip pairs (pair c2 goes to lane c2 % P: adjacent lanes read adjacent dwords) and add their
// parts by butterflies.  The exact roots are added into E[2 W + 1] in LDS, every entry by its one owner.  No HBM scratch, no
// global atomics, no scratch memory.
#include "gpsx_device.hpp"
#include "gpsx_kernels.hpp"
#include "gpsx_acq_coh_parts.hpp"

namespace gpsx {

namespace {

constexpr int kWinThreads = 256;
constexpr int kWinMaxPhases = 2 * 2047 + 1;
constexpr long long kWinMaxGroups = ((1ll << 32) - 1) / kWinThreads;      // workgroups per launch
constexpr u32 kWinSearched = GPSX_ACQ_WINDOW_SEARCHED, kWinSkipped = GPSX_ACQ_WINDOW_SKIPPED, kWinBad = GPSX_ACQ_WINDOW_BAD,
              kWinOffLattice = GPSX_ACQ_WINDOW_OFF_LATTICE, kWinClipped = GPSX_ACQ_WINDOW_CLIPPED;

struct WinPrns {
  u64 w[8];                         // PRN index p: byte p & 7 of word p >> 3
};

struct WinShared {
  int8_t mt[2][16][1024];           // the segment's pre-summed planes, polyphase
  u32 rows[2][kVRowDw];             // [stream]: S_t0, entries 2 d, 2 d + 1 in dword d (1023 entries doubled, then zeros)
  u32 chips[512];                   // chips 2 i, 2 i + 1 as int16 +1 / -1 (chip 1023: 0)
  u32 e[kWinMaxPhases + 1];         // E of window phase j + W
  unsigned long long best[kWinThreads / 64];
  unsigned long long far_sum[kWinThreads / 64];
  u32 far_n[kWinThreads / 64];
};

__device__ __forceinline__ u64 win_wave_sum_u64(u64 v)
{
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const u32 lo = __shfl_xor((u32)v, off), hi = __shfl_xor((u32)(v >> 32), off);
    v += ((u64)hi << 32) | lo;
  }
  return v;
}

// the two entries of row dword d (entry x: S[x mod 1023], x < 2046) at sample offset 0
__device__ __forceinline__ u32 win_row_first(const int8_t (&mt)[16][1024], int d)
{
  u32 word = 0;
#pragma unroll
  for (int e = 0; e < 2; e++) {
    const int x = 2 * d + e;
    int s = 0;
    if (x < 2 * kChips) {
      const int k = x >= kChips ? x - kChips : x;
#pragma unroll
      for (int u = 0; u < 16; u++)
        s += mt[u][k];
    }
    word |= ((u32)s & 0xFFFFu) << (16 * e);
  }
  return word;
}

// ... moved on from sample offset t0 - 1 to t0: sample 16 k + t0 - 1 leaves entry k, sample 16 (k + 1) + t0 - 1 enters
__device__ __forceinline__ u32 win_row_next(const int8_t (&plane)[1024], int d, u32 word)
{
  u32 out = 0;
#pragma unroll
  for (int e = 0; e < 2; e++) {
    const int x = 2 * d + e;
    int s = (int)(int16_t)(word >> (16 * e));
    if (x < 2 * kChips) {
      const int k = x >= kChips ? x - kChips : x, k1 = k == kChips - 1 ? 0 : k + 1;
      s += (int)plane[k1] - (int)plane[k];
    }
    out |= ((u32)s & 0xFFFFu) << (16 * e);
  }
  return out;
}

}  // namespace

__global__ __launch_bounds__(kWinThreads) void k_acq_win(const uint8_t *__restrict__ if_blocks, int stride_blocks, int n_coh, int n_seg,
                                                         int half_width, int half_bins, int guard, u32 need_flags, u32 skip_flags, int rx_lo,
                                                         int n_prn, WinPrns prns, const uint8_t *__restrict__ chips_all, int if_hz,
                                                         int dopp_min_hz, int dopp_step_hz, int n_dopp, int use_magnitude,
                                                         const gpsx_wpred_t *__restrict__ pred, gpsx_peak_t *__restrict__ peaks,
                                                         gpsx_acq_window_rep_t *__restrict__ rep)
{
  __shared__ WinShared sh;
  const int tid = threadIdx.x;
  const int n_k = 2 * half_bins + 1;
  const int k = (int)(blockIdx.x % (u32)n_k), p = (int)((blockIdx.x / (u32)n_k) % (u32)n_prn);
  const int r = rx_lo + (int)(blockIdx.x / ((u32)n_k * (u32)n_prn));
  const size_t row = (size_t)r * n_prn + p;

  // ---- steps 0 - 2: selection, centre, bins (one record: every lane reads it, the values are uniform) ------------------------------
  const u32 rec_flags = pred[row].flags;
  const double code_phase = pred[row].code_phase, f_hz = pred[row].f_hz;
  u32 flags;
  int c = 0, d0 = 0, d1 = -1, dc = 0;
  if ((rec_flags & need_flags) != need_flags || (rec_flags & skip_flags) != 0u) {
    flags = kWinSkipped;
  } else if (!(code_phase >= 0.0 && code_phase <= 16368.0) || !(f_hz - f_hz == 0.0)) {   // (a NaN fails the first, an infinity either)
    flags = kWinBad;
  } else {
    c = (int)__builtin_rint(code_phase);
    c = c == kSamples ? 0 : c;
    const double x = (f_hz - (double)dopp_min_hz) / (double)dopp_step_hz;
    if (__builtin_fabs(x) > 1073741824.0) {
      flags = kWinOffLattice;
    } else {
      dc = (int)__builtin_rint(x);
      d0 = max(dc - half_bins, 0);
      d1 = min(dc + half_bins, n_dopp - 1);
      flags = d0 > d1 ? kWinOffLattice : kWinSearched | (dc - half_bins < 0 || dc + half_bins > n_dopp - 1 ? kWinClipped : 0u);
    }
  }
  const bool searched = (flags & kWinSearched) != 0u;
  if (!searched) {
    d0 = 0;
    d1 = -1;
  }

  // ---- step 5: the row's unsearched records, spread over its workgroups; the report from the first ---------------------------------
  gpsx_peak_t *const out = peaks + row * (size_t)n_dopp;
  for (int d = k * kWinThreads + tid; d < n_dopp; d += n_k * kWinThreads)
    if (d < d0 || d > d1)
      out[d] = gpsx_peak_t{0u, 0u, 0u, 0u};
  if (k == 0 && tid == 0 && rep) {
    gpsx_acq_window_rep_t o;
    o.flags = flags;
    o.first_bin = searched ? d0 : 0;
    o.n_bins = searched ? d1 - d0 + 1 : 0;
    o.centre = searched ? c : 0;
    rep[row] = o;
  }
  const int dopp = dc - half_bins + k;
  if (!searched || dopp < d0 || dopp > d1)
    return;

  // ---- step 3: E over the window's phases ---------------------------------------------------------------------------------------------
  const int n_win = 2 * half_width + 1;
  const int prn = (int)((prns.w[p >> 3] >> ((p & 7) * 8)) & 0xFFu);
  const u32 step_word = nco_step_per_word((float)(int)((u32)if_hz + (u32)dopp_min_hz + (u32)dopp * (u32)dopp_step_hz));
  const uint8_t *blk0 = if_blocks + (size_t)r * stride_blocks * GPSX_BYTES_PER_MS_2BIT;
  {
    const uint8_t *ch = chips_all + (size_t)prn * 1024;
    for (int i = tid; i < 512; i += kWinThreads) {
      u32 word = 0;
#pragma unroll
      for (int e = 0; e < 2; e++) {
        const int cc = 2 * i + e;
        word |= (cc < kChips ? (ch[cc] ? 0xFFFFu : 0x0001u) : 0u) << (16 * e);
      }
      sh.chips[i] = word;
    }
  }
  for (int i = tid; i < n_win; i += kWinThreads)
    sh.e[i] = 0u;
  // lanes per phase: the most phases one sample offset holds is (2 W) / 16 + 1; P = 256 / (that, rounded up to a power of two), <= 64
  int lg_p = 0;
  {
    const int most = (2 * half_width) / 16 + 1;
    int span = 1;
    while (span < most)
      span <<= 1;
    while ((span << lg_p) < kWinThreads && lg_p < 6)
      lg_p++;
  }
  const int n_part = 1 << lg_p, part = tid & (n_part - 1), m = tid >> lg_p;

#pragma unroll 1
  for (int seg = 0; seg < n_seg; seg++) {
    // (the planes are free: every thread passed the barrier behind the previous segment's last offset)
    coh_presum(sh.mt, blk0 + (size_t)seg * n_coh * GPSX_BYTES_PER_MS_2BIT, n_coh, step_word, use_magnitude, tid, kWinThreads);
    __syncthreads();
#pragma unroll 1
    for (int t0 = 0; t0 < 16; t0++) {
      for (int i = tid; i < 2 * kVRowDw; i += kWinThreads) {
        const int st = i / kVRowDw, d = i % kVRowDw;
        sh.rows[st][d] = t0 == 0 ? win_row_first(sh.mt[st], d) : win_row_next(sh.mt[st][t0 - 1], d, sh.rows[st][d]);
      }
      __syncthreads();
      // this offset's window phases: j = -W + first + 16 m, first = (t0 - c + W) mod 16
      const int first = (t0 - c + half_width) & 15;
      const int j = first + 16 * m;                    // (as an index into E: j + W of the definition)
      const bool mine = j < n_win;
      int tau = c + j - half_width;
      tau = tau < 0 ? tau + kSamples : tau >= kSamples ? tau - kSamples : tau;
      const int q = mine ? tau >> 4 : 0;               // (a lane without a phase runs along on offset 0: the butterflies need it)
      const u32 *r0 = &sh.rows[0][q >> 1], *r1 = &sh.rows[1][q >> 1];
      const u32 odd = 16u * (u32)(q & 1);
      int acc_i = 0, acc_q = 0;
#pragma unroll 4
      for (int c2 = part; c2 < 512; c2 += n_part) {
        const v2s cw = __builtin_bit_cast(v2s, sh.chips[c2]);
        const v2s wi = __builtin_bit_cast(v2s, __builtin_amdgcn_alignbit(r0[c2 + 1], r0[c2], odd));
        const v2s wq = __builtin_bit_cast(v2s, __builtin_amdgcn_alignbit(r1[c2 + 1], r1[c2], odd));
        acc_i = __builtin_amdgcn_sdot2(wi, cw, acc_i, false);
        acc_q = __builtin_amdgcn_sdot2(wq, cw, acc_q, false);
      }
      for (int off = 1; off < n_part; off <<= 1) {
        acc_i += __shfl_xor(acc_i, off);
        acc_q += __shfl_xor(acc_q, off);
      }
      if (mine && part == 0)
        sh.e[j] += coh_root(acc_i, acc_q);
      __syncthreads();              // (the rows are read; E's entry is written)
    }
  }

  // ---- step 4: the record -----------------------------------------------------------------------------------------------------------
  unsigned long long best = 0;
  for (int j = tid; j < n_win; j += kWinThreads) {
    int tau = c + j - half_width;
    tau = tau < 0 ? tau + kSamples : tau >= kSamples ? tau - kSamples : tau;
    const unsigned long long key = coh_key(sh.e[j], tau);
    best = key > best ? key : best;
  }
  best = coh_wave_max_u64(best);
  if ((tid & 63) == 0)
    sh.best[tid >> 6] = best;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < kWinThreads / 64; w++)
    best = sh.best[w] > best ? sh.best[w] : best;
  const u32 max_val = (u32)(best >> 14);
  const int phase = max_val ? 16383 - (int)(best & 0x3FFFu) : 0;
  u64 far_sum = 0;
  u32 far_n = 0;
  for (int j = tid; j < n_win; j += kWinThreads) {
    int tau = c + j - half_width;
    tau = tau < 0 ? tau + kSamples : tau >= kSamples ? tau - kSamples : tau;
    const int dd = tau > phase ? tau - phase : phase - tau, dist = min(dd, kSamples - dd);
    if (dist > guard) {
      far_sum += sh.e[j];
      far_n++;
    }
  }
  far_sum = win_wave_sum_u64(far_sum);
  far_n = (u32)win_wave_sum_u64(far_n);
  if ((tid & 63) == 0) {
    sh.far_sum[tid >> 6] = far_sum;
    sh.far_n[tid >> 6] = far_n;
  }
  __syncthreads();
  if (tid == 0) {
    u64 s = 0;
    u32 n = 0;
#pragma unroll
    for (int w = 0; w < kWinThreads / 64; w++) {
      s += sh.far_sum[w];
      n += sh.far_n[w];
    }
    coh_record(&out[dopp], best, n ? (u32)(s * (u64)kSamples / (u64)n) : 0u);
  }
}

void launch_acq_win(hipStream_t s, const gpsx_acq_window_t &cfg, const uint8_t *d_if_blocks, int n_rx, int stride_blocks, int n_prn,
                    const uint8_t *prns, const uint8_t *d_chips_all, int if_hz, int dopp_min_hz, int dopp_step_hz, int n_dopp, int use_magnitude,
                    const gpsx_wpred_t *d_pred, gpsx_peak_t *d_peaks, gpsx_acq_window_rep_t *d_rep)
{
  // (no checks of its own: gpsx_api_wtrack.hip's acq_window() is the one list of what a launch needs and refuses with a text before it comes here)
  WinPrns list = {};
  for (int p = 0; p < n_prn; p++)
    list.w[p >> 3] |= (u64)prns[p] << ((p & 7) * 8);
  // a launch's THREADS are counted in 32 bits (the runtime refuses more than 2^32 - 1): at most 2^24 - 1 workgroups of 256, receivers in chunks
  // (a receiver has at most 64 x 65 workgroups, so a chunk holds 4032 receivers at least)
  const long long per_rx = (long long)n_prn * (2 * cfg.half_bins + 1);
  const int chunk = (int)std::max(1ll, std::min((long long)n_rx, (long long)kWinMaxGroups / per_rx));
  for (int lo = 0; lo < n_rx; lo += chunk) {
    const int n = std::min(chunk, n_rx - lo);
    hipLaunchKernelGGL(k_acq_win, dim3((unsigned)((long long)n * per_rx)), dim3(kWinThreads), 0, s, d_if_blocks, stride_blocks, cfg.n_coh,
                       cfg.n_seg, cfg.half_width, cfg.half_bins, cfg.guard, cfg.need_flags, cfg.skip_flags, lo, n_prn, list, d_chips_all, if_hz,
                       dopp_min_hz, dopp_step_hz, n_dopp, use_magnitude, d_pred, d_peaks, d_rep);
  }
}

}  // namespace gpsx
