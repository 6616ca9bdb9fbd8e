// k_wpred.hip -- EXTENSION, not in the reference: prediction and hot hand-over, the stage behind the navigation filter that computes
// every banked satellite's elevation, pseudorange, code phase and Doppler at the loop's next block from the filter's state and hands
// the visible ones that no slot tracks to free slots (include/gpsx.h gpsx_wpred).
//
// k_wacq's geometry: one wave per receiver, four receivers per 256-thread workgroup; no LDS, no barrier, no scratch.  Every lane reads
// the receiver's 384-byte filter state (one address for the wave) and keeps x^ and the two 4 x 4 blocks of P that the variances need.
// Lane p is PRN index p for steps 2 - 4: its bank record, three passes of one FP64 satellite evaluation each (gpsx_wsolve_parts.hpp:
// sat_at_clock, az_el, klobuchar, saastamoinen) under #pragma unroll 1, the observables and the two variances -- that is where the
// time goes.  Lane j is slot j for steps 5 - 7, as in k_wacq: which PRNs a kept slot holds, the candidates' ranks (by elevation, a
// loop of shuffles) and the slots they go to are ballots, popcounts of masks and shuffles from a wave-uniform lane; the states of a
// slot that is handed over or evicted are written by the wave together, 8 bytes per lane.  Every ballot and shuffle runs under
// wave-uniform control flow: a wave whose receiver does not exist, or whose state is not a filter's, leaves as a whole (the state is
// one for the wave); the loops around them have wave-uniform bounds; lane-dependent conditions are selects or lane-local branches
// without a cross-lane operation inside.  The lane-local loops are bounded: three passes, Kepler at 30 steps, the geodetic fixed
// point at 30.
#include <hip/hip_runtime.h>

#include <cstddef>

#include "gpsx_device.hpp"
#include "gpsx_kernels.hpp"
#include "gpsx_wsolve_parts.hpp"

namespace gpsx {
using namespace wsolve;

namespace {

static_assert(sizeof(gpsx_wpred_cfg_t) == 128 && offsetof(gpsx_wpred_cfg_t, mps_per_hz) == 64 && offsetof(gpsx_wpred_cfg_t, el_min_rad) == 72 &&
              offsetof(gpsx_wpred_cfg_t, max_sigma_m) == 80 && offsetof(gpsx_wpred_cfg_t, max_sigma_hz) == 88 && offsetof(gpsx_wpred_cfg_t, ch_per_rx) == 96 &&
              offsetof(gpsx_wpred_cfg_t, lead_blocks) == 100 && offsetof(gpsx_wpred_cfg_t, evict_after_blocks) == 104 &&
              offsetof(gpsx_wpred_cfg_t, handover) == 108 && offsetof(gpsx_wpred_cfg_t, reserved) == 112, "gpsx_wpred_cfg_t layout");
static_assert(sizeof(gpsx_wpred_t) == 64 && offsetof(gpsx_wpred_t, slot) == 4 && offsetof(gpsx_wpred_t, tx_ms) == 8 && offsetof(gpsx_wpred_t, pr_m) == 16 &&
              offsetof(gpsx_wpred_t, code_phase) == 24 && offsetof(gpsx_wpred_t, f_hz) == 32 && offsetof(gpsx_wpred_t, el) == 40 &&
              offsetof(gpsx_wpred_t, az) == 48 && offsetof(gpsx_wpred_t, sigma_m) == 56 && offsetof(gpsx_wpred_t, sigma_hz) == 60, "gpsx_wpred_t layout");
static_assert(sizeof(gpsx_wpred_rx_t) == 64 && offsetof(gpsx_wpred_rx_t, week) == 2 && offsetof(gpsx_wpred_rx_t, t_ms) == 4 &&
              offsetof(gpsx_wpred_rx_t, n_have) == 8 && offsetof(gpsx_wpred_rx_t, n_dropped) == 13 && offsetof(gpsx_wpred_rx_t, zero) == 14 &&
              offsetof(gpsx_wpred_rx_t, visible_mask) == 16 && offsetof(gpsx_wpred_rx_t, have_mask) == 24 && offsetof(gpsx_wpred_rx_t, assigned_mask) == 32 &&
              offsetof(gpsx_wpred_rx_t, free_mask) == 56, "gpsx_wpred_rx_t layout");
static_assert(sizeof(gpsx_wkf_state_t) == 384 && offsetof(gpsx_wkf_state_t, P) == 64 && offsetof(gpsx_wkf_state_t, rcv_ms) == 352 &&
              offsetof(gpsx_wkf_state_t, week) == 360 && offsetof(gpsx_wkf_state_t, flags) == 364, "gpsx_wkf_state_t layout");
static_assert(sizeof(gpsx_wsync_state_t) == 448 && offsetof(gpsx_wsync_state_t, loop) == 0 && offsetof(gpsx_wloop_state_t, prn) == 0 &&
              offsetof(gpsx_wloop_state_t, code_phase_fine) == 4 && offsetof(gpsx_wloop_state_t, if_freq_offset_hz) == 8 &&
              offsetof(gpsx_wloop_state_t, if_freq_accum) == 12, "gpsx_wsync_state_t layout");
static_assert(sizeof(gpsx_wlock_state_t) == 128 && offsetof(gpsx_wlock_state_t, blocks_seen) == 0 && offsetof(gpsx_wlock_state_t, flags) == 80 &&
              sizeof(gpsx_wnav_state_t) == 64 && sizeof(gpsx_wobs_state_t) == 80 && sizeof(gpsx_weph_state_t) == 192, "the four stage states");

constexpr int kSyncWords = 56;                                      // 8-byte words of a sync state
constexpr int kLockWords = 16, kNavWords = 8, kObsWords = 10;       // ... of the other four: 16 + 8 + 10 + 24 = 58 lanes
constexpr int kEphWords = 24;

// the place of element (i, j) of a symmetric 8 x 8 in its upper triangle, row by row (gpsx_wkf_state_t.P)
__device__ __forceinline__ constexpr int tri(int i, int j) { return i <= j ? i * (17 - i) / 2 + (j - i) : j * (17 - j) / 2 + (i - j); }
__device__ __forceinline__ u64 below(int lane) { return (1ull << lane) - 1ull; }   // the lanes under this one (lane 0 .. 63)

}  // namespace

// PRN numbers by value, eight per word (n_prn <= 64): lane p's is a select among eight scalars, never an indexed copy
struct WpredPrns { u64 w[8]; };

__global__ __launch_bounds__(256) void k_wpred(gpsx_wpred_cfg_t cfg, int n_rx, int n_prn, WpredPrns prns, const gpsx_wkf_state_t *__restrict__ kf,
                                               const gpsx_weph_t *__restrict__ bank, gpsx_wsync_state_t *sync, gpsx_wlock_state_t *lock,
                                               gpsx_wnav_state_t *nav, gpsx_wobs_state_t *obs, gpsx_weph_state_t *eph,
                                               gpsx_wpred_rx_t *__restrict__ rx, gpsx_wpred_t *__restrict__ pred)
{
  const int lane = (int)threadIdx.x & 63;
  const int r = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
  if (r >= n_rx)          // (the whole wave: r is the same in its 64 lanes)
    return;
  const int ch = cfg.ch_per_rx;
  const bool is_prn = lane < n_prn;

  // 0 the filter's state, the same in every lane
  const gpsx_wkf_state_t *sp = kf + r;
  double x[8], pp[10], pv[16], vv[10];      // x^; P's upper-left, upper-right and lower-right 4 x 4 blocks
  bool sane = true;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    x[i] = sp->x[i];
    sane = sane && finite(x[i]);
  }
  bool diag = true;
#pragma unroll
  for (int i = 0; i < 8; i++)
#pragma unroll
    for (int k = i; k < 8; k++) {
      const double v = sp->P[tri(i, k)];
      sane = sane && finite(v);
      if (i == k)
        diag = diag && v > 0.0;
      if (k < 4)
        pp[tri(i, k) - (i == 0 ? 0 : (i == 1 ? 4 : (i == 2 ? 8 : 12)))] = v;
      else if (i >= 4)
        vv[tri(i - 4, k - 4) - (i == 4 ? 0 : (i == 5 ? 4 : (i == 6 ? 8 : 12)))] = v;
      else
        pv[i * 4 + (k - 4)] = v;
    }
  long long T = sp->rcv_ms;
  int week = sp->week;
  const u32 sflags = sp->flags;
  sane = sane && (sflags & ~GPSX_WKF_STATE_INIT) == 0 && T >= 0 && T < kWeekMs;
  const bool inited = (sflags & GPSX_WKF_STATE_INIT) != 0;
  sane = sane && (!inited || diag);
  if (!sane || !inited) {   // (the whole wave: the state is one for its 64 lanes)
    if (pred && is_prn) {
      gpsx_wpred_t o = {};
      pred[(size_t)r * (size_t)n_prn + (size_t)lane] = o;
    }
    if (lane == 0) {
      gpsx_wpred_rx_t o = {};
      o.flags = (uint16_t)(!sane ? GPSX_WPRED_RX_BAD : GPSX_WPRED_RX_NOT_INIT);
      rx[r] = o;
    }
    return;
  }

  // 1 the epoch: T, x^, P^ without the q terms (the upper-left block; the lower-right one stays)
  T += (long long)cfg.lead_blocks;
  if (T >= kWeekMs) {
    T -= kWeekMs;
    week += 1;
  }
  const double dt = (double)cfg.lead_blocks * 1e-3;
#pragma unroll
  for (int i = 0; i < 4; i++)
    x[i] = x[i] + dt * x[4 + i];
  {
    double np_[10];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int k = i; k < 4; k++) {
        const int at = tri(i, k) - (i == 0 ? 0 : (i == 1 ? 4 : (i == 2 ? 8 : 12)));
        const int av = tri(i, k) - (i == 0 ? 0 : (i == 1 ? 4 : (i == 2 ? 8 : 12)));      // (the same place in the lower-right block's triangle)
        np_[at] = (pp[at] + dt * (pv[i * 4 + k] + pv[k * 4 + i])) + (dt * dt) * vv[av];
      }
#pragma unroll
    for (int i = 0; i < 10; i++)
      pp[i] = np_[i];
  }
  double ion[8];
  choose_ion(cfg.ion, ion);
  double lat, lon, hgt;
  geodetic(x[0], x[1], x[2], lat, lon, hgt);
  const double tow = (double)T / 1000.0;

  // 2 the satellite and the range: lane p is PRN index p
  const gpsx_weph_t e = bank[(size_t)r * (size_t)n_prn + (size_t)(is_prn ? lane : 0)];
  const bool have = is_prn && (e.flags & GPSX_WEPH_VALID) != 0;
  bool good = have && e.svh == 0;
  double pr = 72.0 * kMs, el = 0.0, az = 0.0, l0 = 0.0, l1 = 0.0, l2 = 0.0;
  SatState s = {};
  const double kk = kOmegaE / kC;
#pragma unroll 1
  for (int pass = 0; pass < 3; pass++) {
    if (good) {            // (lane-local: no cross-lane operation in here)
      good = sat_at_clock(e, ((double)T - pr / kMs) / 1000.0, s);
      if (good) {
        l0 = s.px - x[0];
        l1 = s.py - x[1];
        l2 = s.pz - x[2];
        const double range = sqrt(l0 * l0 + l1 * l1 + l2 * l2);
        const double rn = sqrt(s.px * s.px + s.py * s.py + s.pz * s.pz);
        const double rho = range + kOmegaE * (s.px * x[1] - s.py * x[0]) / kC;
        good = !(range == 0.0) && !(rn < kRe) && !(rho <= 0.0);
        if (good) {
          l0 /= range;
          l1 /= range;
          l2 /= range;
          az_el(l0, l1, l2, lat, lon, hgt, az, el);
          const double dion = klobuchar(tow, ion, lat, lon, hgt, az, el);
          const double dtrp = saastamoinen(lat, hgt, el, 0.7);
          pr = (rho + dion + dtrp + x[3] - kC * s.clk) + kC * e.tgd;
        }
      }
    }
  }

  // 3 the observables, 4 the flags
  const double u = pr / kMs, q = floor(u);
  const double code_phase = (u - q) * 16368.0;
  const double a0 = -l0 - kk * s.py, a1 = -l1 + kk * s.px, a2 = -l2;
  const double f_hz = ((a0 * x[4] + a1 * x[5] + a2 * x[6] + x[7]) +
                       (l0 * s.vx + l1 * s.vy + l2 * s.vz + kk * (s.vx * x[1] - s.vy * x[0]) - kC * s.rate)) / cfg.mps_per_hz;
  double s_pr, s_f;
  {
    const double h0 = -l0, h1 = -l1, h2 = -l2;
    const double t0 = (pp[0] * h0 + pp[1] * h1 + pp[2] * h2) + pp[3];
    const double t1 = (pp[1] * h0 + pp[4] * h1 + pp[5] * h2) + pp[6];
    const double t2 = (pp[2] * h0 + pp[5] * h1 + pp[7] * h2) + pp[8];
    const double t3 = (pp[3] * h0 + pp[6] * h1 + pp[8] * h2) + pp[9];
    s_pr = h0 * t0 + h1 * t1 + h2 * t2 + t3;
    const double u0 = (vv[0] * a0 + vv[1] * a1 + vv[2] * a2) + vv[3];
    const double u1 = (vv[1] * a0 + vv[4] * a1 + vv[5] * a2) + vv[6];
    const double u2 = (vv[2] * a0 + vv[5] * a1 + vv[7] * a2) + vv[8];
    const double u3 = (vv[3] * a0 + vv[6] * a1 + vv[8] * a2) + vv[9];
    s_f = (a0 * u0 + a1 * u1 + a2 * u2 + u3) / (cfg.mps_per_hz * cfg.mps_per_hz);
  }
  const float sigma_m = (float)sqrt(s_pr), sigma_hz = (float)sqrt(s_f);
  const bool predicted = good && finite(pr) && finite(code_phase) && finite(f_hz) && finite(el) && finite(az) && finite(s_pr) && finite(s_f) &&
                         finite((double)sigma_m) && finite((double)sigma_hz) && __builtin_fabs(q) < 4503599627370496.0;
  const bool visible = predicted && el >= cfg.el_min_rad;
  const bool certain = predicted && s_pr <= cfg.max_sigma_m * cfg.max_sigma_m && s_f <= cfg.max_sigma_hz * cfg.max_sigma_hz;
  long long tx_ms = 0;
  if (predicted) {
    tx_ms = (T - (long long)q) % kWeekMs;
    if (tx_ms < 0)
      tx_ms += kWeekMs;
  }
  const u64 word = lane < 8 ? prns.w[0] : lane < 16 ? prns.w[1] : lane < 24 ? prns.w[2] : lane < 32 ? prns.w[3] :
                   lane < 40 ? prns.w[4] : lane < 48 ? prns.w[5] : lane < 56 ? prns.w[6] : prns.w[7];
  const int my_prn = (int)((word >> ((lane & 7) * 8)) & 0xFFull);

  // 5 slots: lane j is slot j
  const bool is_slot = lane < ch;
  const size_t ch0 = (size_t)r * (size_t)ch;
  const int slot_prn = is_slot ? sync[ch0 + lane].loop.prn : GPSX_PRN_NONE;
  const bool holds = is_slot && slot_prn != GPSX_PRN_NONE;
  bool evicted = false;
  if (cfg.evict_after_blocks > 0) {     // (then lock is not null: the host checked)
    const gpsx_wlock_state_t *ls = lock + ch0 + (is_slot ? lane : 0);
    const long long seen = ls->blocks_seen;
    const u32 lflags = ls->flags;
    evicted = holds && (lflags & GPSX_WLOCK_CODE) == 0 && seen >= (long long)cfg.evict_after_blocks;
  }
  const bool kept = holds && !evicted;
  const u64 kept_mask = __ballot(kept), evicted_mask = __ballot(evicted), free_before = __ballot(is_slot && !kept);

  // 6 candidates: VISIBLE and CERTAIN and held by no kept slot, ranked by elevation (equal: the lower index), the k-th to the k-th free slot
  bool tracked = false;
#pragma unroll 1
  for (int j = 0; j < ch; j++) {
    const int v = __shfl(slot_prn, j, 64);
    tracked = tracked || (((kept_mask >> j) & 1ull) != 0 && v == my_prn);
  }
  tracked = tracked && is_prn;
  const bool cand = visible && certain && !tracked;
  const u64 cand_mask = __ballot(cand);
  int rank = 0;
#pragma unroll 1
  for (int p = 0; p < n_prn; p++) {
    const double eq = __shfl(el, p, 64);
    rank += (((cand_mask >> p) & 1ull) != 0 && (eq > el || (eq == el && p < lane))) ? 1 : 0;
  }
  const bool hand = cfg.handover != 0;      // (wave-uniform)
  const int n_free = __popcll(free_before);
  const bool assigned = hand && cand && rank < n_free;
  const bool dropped = hand && cand && !assigned;
  int slot = -1;
  if (assigned) {                        // the rank-th set bit of free_before (no cross-lane operation in here)
    u64 m = free_before;
    for (int i = 0; i < rank; i++)
      m &= m - 1ull;
    slot = __ffsll((long long)m) - 1;
  }
  const u64 assigned_mask =
      hand ? __ballot(is_slot && ((free_before >> lane) & 1ull) != 0 && __popcll(free_before & below(lane)) < __popcll(cand_mask)) : 0ull;
  const u64 tracked_mask = __ballot(tracked), visible_mask = __ballot(visible), have_mask = __ballot(have), dropped_mask = __ballot(dropped);

  // 7 the hand-over: the states of every slot that is handed over or evicted, the wave together
  const float phase_f = (float)code_phase, freq_f = (float)f_hz;
  u64 todo = hand ? (assigned_mask | evicted_mask) : 0ull;      // (wave-uniform: ballots)
#pragma unroll 1
  while (todo != 0) {
    const int j = __ffsll((long long)todo) - 1;
    todo &= todo - 1ull;
    const u64 from = __ballot(assigned && slot == j);       // the candidate that goes there: one lane, or none
    const int src = from != 0 ? __ffsll((long long)from) - 1 : 0;
    const int h_prn = __shfl(my_prn, src, 64);
    const u32 h_phase = (u32)__shfl((int)__float_as_uint(phase_f), src, 64);
    const u32 h_freq = (u32)__shfl((int)__float_as_uint(freq_f), src, 64);
    const u64 w0 = from != 0 ? ((u64)h_phase << 32) | (u64)(u32)h_prn : (u64)(u32)GPSX_PRN_NONE;
    const u64 w1 = from != 0 ? (u64)h_freq : 0ull;          // (if_freq_accum, the high half: 0)
    const size_t c = ch0 + (size_t)j;
    if (lane < kSyncWords)
      reinterpret_cast<u64 *>(sync + c)[lane] = lane == 0 ? w0 : lane == 1 ? w1 : 0ull;
    u64 *dst = nullptr;
    if (lane < kLockWords)
      dst = lock ? reinterpret_cast<u64 *>(lock + c) + lane : nullptr;
    else if (lane < kLockWords + kNavWords)
      dst = nav ? reinterpret_cast<u64 *>(nav + c) + (lane - kLockWords) : nullptr;
    else if (lane < kLockWords + kNavWords + kObsWords)
      dst = obs ? reinterpret_cast<u64 *>(obs + c) + (lane - kLockWords - kNavWords) : nullptr;
    else if (lane < kLockWords + kNavWords + kObsWords + kEphWords)
      dst = eph ? reinterpret_cast<u64 *>(eph + c) + (lane - kLockWords - kNavWords - kObsWords) : nullptr;
    if (dst)
      *dst = 0ull;
  }

  // 8 the records
  if (pred && is_prn) {
    gpsx_wpred_t o = {};
    o.flags = (have ? GPSX_WPRED_HAVE_EPH : 0u) | (predicted ? GPSX_WPRED_PREDICTED : 0u) | (visible ? GPSX_WPRED_VISIBLE : 0u) |
              (certain ? GPSX_WPRED_CERTAIN : 0u) | (tracked ? GPSX_WPRED_TRACKED : 0u) | (assigned ? GPSX_WPRED_ASSIGNED : 0u) |
              (dropped ? GPSX_WPRED_DROPPED : 0u);
    o.slot = slot;
    if (predicted) {
      o.tx_ms = tx_ms;
      o.pr_m = pr;
      o.code_phase = code_phase;
      o.f_hz = f_hz;
      o.el = el;
      o.az = az;
      o.sigma_m = sigma_m;
      o.sigma_hz = sigma_hz;
    }
    pred[(size_t)r * (size_t)n_prn + (size_t)lane] = o;
  }
  if (lane == 0) {
    const u32 n_assigned = (u32)__popcll(assigned_mask), n_evicted = (u32)__popcll(evicted_mask), n_dropped = (u32)__popcll(dropped_mask);
    gpsx_wpred_rx_t o = {};
    o.flags = (uint16_t)(GPSX_WPRED_RX_PREDICTED | (n_assigned ? GPSX_WPRED_RX_ASSIGNED : 0u) | (n_evicted ? GPSX_WPRED_RX_EVICTED : 0u) |
                         (n_dropped ? GPSX_WPRED_RX_FULL : 0u));
    o.week = (int16_t)week;
    o.t_ms = (int32_t)T;
    o.n_have = (uint8_t)__popcll(have_mask);
    o.n_visible = (uint8_t)__popcll(visible_mask);
    o.n_tracked = (uint8_t)__popcll(tracked_mask);
    o.n_assigned = (uint8_t)n_assigned;
    o.n_evicted = (uint8_t)n_evicted;
    o.n_dropped = (uint8_t)n_dropped;
    o.visible_mask = visible_mask;
    o.have_mask = have_mask;
    o.assigned_mask = assigned_mask;
    o.evicted_mask = evicted_mask;
    o.kept_mask = kept_mask;
    o.free_mask = free_before & ~assigned_mask;
    rx[r] = o;
  }
}

void launch_wpred(hipStream_t s, const gpsx_wpred_cfg_t &cfg, int n_rx, int n_prn, const uint8_t *prns, const gpsx_wkf_state_t *d_kf_state,
                  const gpsx_weph_t *d_bank, gpsx_wsync_state_t *d_sync_st, gpsx_wlock_state_t *d_lock_st, gpsx_wnav_state_t *d_nav_st,
                  gpsx_wobs_state_t *d_obs_st, gpsx_weph_state_t *d_eph_st, gpsx_wpred_rx_t *d_rx, gpsx_wpred_t *d_pred)
{
  // (no checks of its own: gpsx_api_wtrack.hip's wpred() is the one list of what a launch needs and refuses with a text before it comes here)
  WpredPrns list = {};
  for (int p = 0; p < n_prn; p++)
    list.w[p >> 3] |= (u64)prns[p] << ((p & 7) * 8);
  hipLaunchKernelGGL(k_wpred, dim3(((unsigned)n_rx + 3u) / 4u), dim3(256), 0, s, cfg, n_rx, n_prn, list, d_kf_state, d_bank, d_sync_st, d_lock_st, d_nav_st,
                     d_obs_st, d_eph_st, d_rx, d_pred);
}

}  // namespace gpsx
