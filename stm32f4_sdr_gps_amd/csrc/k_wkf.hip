// k_wkf.hip -- EXTENSION, not in the reference: every receiver's navigation filter -- position, clock term, velocity and clock drift
// carried from launch to launch in a resident state -- from the weighted chain's observables and ephemeris records, on the device
// (include/gpsx.h gpsx_wkf).
//
// k_wfix's lane layout: one slot per lane; a receiver is a group of W lanes, W the smallest power of two >= ch_per_rx, so a wave holds
// 64 / W receivers and a workgroup of 256 lanes 256 / W.  Every lane of a group reads its receiver's 384-byte state and runs the
// prediction (x-, P- in three 4 x 4 blocks).  Once per lane: the slot's observable and ephemeris record, the satellite at the transmit
// time its own clock reads (position, analytic velocity, clock offset and rate), the pseudorange row at x- (Sagnac, elevation,
// Klobuchar, Saastamoinen, the variance terms) and the Doppler row, the millisecond repair (a repaired slot is evaluated once more at
// the corrected transmit time: a lane-local loop of two passes at most), the gate against h P- h^T + sig2.  Once per group: the
// 10 + 4 sums of each of the two 4 x 4 information blocks and the two NIS sums by xor-butterflies of width W, six masks from ballots,
// then in every lane, unrolled and in registers, nothing indexed by a run-time value: (P-)^-1 by a Cholesky factorisation, + I, P+ by
// a second one, x+ = x- + P+ g.  The group's first lane writes the record and the state.  FP64 on the vector ALU; 390 VGPRs (one wave
// per SIMD, as k_wfix), 106 SGPRs, no LDS, no scratch (build.py check_wkf).
// The parts it shares with k_wfix, k_wfde and k_wvel are gpsx_wsolve_parts.hpp's; tri and spd_inverse are this file's.
//
// Every cross-lane operation runs under wave-uniform control flow: there is no branch around a ballot or a shuffle -- the six
// ballots and every group_sum (a butterfly of width w, w the launch's) stand at the kernel's top level, the sums in loops that are
// unrolled -- a lane without a row adds zeros, a group that does not run (out of range, BAD, not initialised) computes on zeros and
// masks its result; nothing returns before the last shuffle.  The lane-local loops are bounded: the repair's two passes, Kepler at
// 30 steps, the geodetic fixed point at 30.  Every store is an ordinary vector store.
#include <hip/hip_runtime.h>

#include <cstddef>

#include "gpsx_device.hpp"
#include "gpsx_kernels.hpp"
#include "gpsx_wsolve_parts.hpp"

namespace gpsx {
using namespace wsolve;

namespace {

static_assert(sizeof(gpsx_wkf_cfg_t) == 176 && offsetof(gpsx_wkf_cfg_t, mps_per_hz) == 64 && offsetof(gpsx_wkf_cfg_t, sig_pr_m) == 72 &&
              offsetof(gpsx_wkf_cfg_t, sig_dop_mps) == 80 && offsetof(gpsx_wkf_cfg_t, gate) == 88 && offsetof(gpsx_wkf_cfg_t, q_acc) == 96 &&
              offsetof(gpsx_wkf_cfg_t, q_clk_f) == 104 && offsetof(gpsx_wkf_cfg_t, q_clk_g) == 112 && offsetof(gpsx_wkf_cfg_t, p0_pos) == 120 &&
              offsetof(gpsx_wkf_cfg_t, p0_drift) == 144 && offsetof(gpsx_wkf_cfg_t, ch_per_rx) == 152 && offsetof(gpsx_wkf_cfg_t, max_coast) == 156 &&
              offsetof(gpsx_wkf_cfg_t, reserved) == 160, "gpsx_wkf_cfg_t layout");
static_assert(sizeof(gpsx_wkf_state_t) == 384 && offsetof(gpsx_wkf_state_t, P) == 64 && offsetof(gpsx_wkf_state_t, rcv_ms) == 352 &&
              offsetof(gpsx_wkf_state_t, week) == 360 && offsetof(gpsx_wkf_state_t, flags) == 364 && offsetof(gpsx_wkf_state_t, n_starved) == 368 &&
              offsetof(gpsx_wkf_state_t, n_init) == 372 && offsetof(gpsx_wkf_state_t, n_lost) == 376 && offsetof(gpsx_wkf_state_t, reserved) == 380,
              "gpsx_wkf_state_t layout");
static_assert(sizeof(gpsx_wkf_t) == 240 && offsetof(gpsx_wkf_t, n_pr) == 4 && offsetof(gpsx_wkf_t, n_dop) == 8 && offsetof(gpsx_wkf_t, n_starved) == 12 &&
              offsetof(gpsx_wkf_t, pr_mask) == 16 && offsetof(gpsx_wkf_t, dop_mask) == 24 && offsetof(gpsx_wkf_t, rej_pr_mask) == 32 &&
              offsetof(gpsx_wkf_t, rej_dop_mask) == 40 && offsetof(gpsx_wkf_t, plus_mask) == 48 && offsetof(gpsx_wkf_t, minus_mask) == 56 &&
              offsetof(gpsx_wkf_t, rr) == 64 && offsetof(gpsx_wkf_t, clk_m) == 88 && offsetof(gpsx_wkf_t, vel) == 96 &&
              offsetof(gpsx_wkf_t, cdrift_mps) == 120 && offsetof(gpsx_wkf_t, geo) == 128 && offsetof(gpsx_wkf_t, enu) == 152 &&
              offsetof(gpsx_wkf_t, sigma) == 176 && offsetof(gpsx_wkf_t, nis_pr) == 208 && offsetof(gpsx_wkf_t, nis_dop) == 216 &&
              offsetof(gpsx_wkf_t, rcv_ms) == 224 && offsetof(gpsx_wkf_t, week) == 232 && offsetof(gpsx_wkf_t, reserved) == 236, "gpsx_wkf_t layout");

// the place of element (i, j) of a symmetric 8 x 8 in its upper triangle, row by row
__device__ __forceinline__ constexpr int tri(int i, int j) { return i <= j ? i * (17 - i) / 2 + (j - i) : j * (17 - j) / 2 + (i - j); }

// the header's INV, in place: a <- a^-1, false if a pivot fails the rule.  Unrolled, every index a constant: registers.
__device__ __forceinline__ bool spd_inverse(double (&a)[36])
{
  double m[36];
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 8; j++) {   // L[i][k], k < i, takes N's place at tri(k, i)
    const double njj = a[tri(j, j)];
    double p = njj;
#pragma unroll
    for (int k = 0; k < j; k++)
      p -= a[tri(k, j)] * a[tri(k, j)];
    ok = ok && (j == 0 ? p > 0.0 : p > kPivot * njj);
    const double ljj = sqrt(p);
    a[tri(j, j)] = ljj;
#pragma unroll
    for (int i = j + 1; i < 8; i++) {
      double t = a[tri(j, i)];
#pragma unroll
      for (int k = 0; k < j; k++)
        t -= a[tri(k, i)] * a[tri(k, j)];
      a[tri(j, i)] = t / ljj;
    }
  }
#pragma unroll
  for (int j = 0; j < 8; j++) {   // M[i][j], j <= i, at m[tri(j, i)]
    m[tri(j, j)] = 1.0 / a[tri(j, j)];
#pragma unroll
    for (int i = j + 1; i < 8; i++) {
      double t = a[tri(j, i)] * m[tri(j, j)];
#pragma unroll
      for (int k = j + 1; k < i; k++)
        t += a[tri(k, i)] * m[tri(j, k)];
      m[tri(j, i)] = -t / a[tri(i, i)];
    }
  }
#pragma unroll
  for (int i = 0; i < 8; i++)
#pragma unroll
    for (int j = i; j < 8; j++) {
      double t = m[tri(i, j)] * m[tri(j, j)];
#pragma unroll
      for (int k = j + 1; k < 8; k++)
        t += m[tri(i, k)] * m[tri(j, k)];
      a[tri(i, j)] = t;
    }
  return ok;
}

}  // namespace

__global__ __launch_bounds__(256) void k_wkf(gpsx_wkf_cfg_t cfg, const gpsx_wobs_t *obs, const gpsx_weph_t *eph, const gpsx_wlock_t *lock,
                                             const gpsx_wfix_t *fix, const gpsx_wvel_t *vel, int n_rx, int n_blocks, int w, int log2w,
                                             gpsx_wkf_state_t *state, gpsx_wkf_t *kf, u32 *bad_state)
{
  const Lane ln = lane_of(w, log2w, n_rx, cfg.ch_per_rx);
  const int j = ln.j, base = ln.base;
  const long long r = ln.r;
  const bool in_rx = ln.in_rx, slot = ln.slot;
  const size_t at = ln.at;

  // ---- the receiver's state, in every lane of its group; what kind of call this is for it ----
  double x[8], P[36];
#pragma unroll
  for (int i = 0; i < 8; i++)
    x[i] = 0.0;
#pragma unroll
  for (int i = 0; i < 36; i++)
    P[i] = 0.0;
  long long rcv_ms = 0;
  int week = 0;
  u32 sflags = 0, n_starved = 0, n_init = 0, n_lost = 0;
  enum { kOut, kBad, kNotInit, kInit, kRun };
  int kind = kOut;
  if (in_rx) {
    const gpsx_wkf_state_t *sp = state + r;
    bool sane = true;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      x[i] = sp->x[i];
      sane = sane && finite(x[i]);
    }
#pragma unroll
    for (int i = 0; i < 36; i++) {
      P[i] = sp->P[i];
      sane = sane && finite(P[i]);
    }
    rcv_ms = sp->rcv_ms;
    week = sp->week;
    sflags = sp->flags;
    n_starved = sp->n_starved;
    n_init = sp->n_init;
    n_lost = sp->n_lost;
    sane = sane && (sflags & ~GPSX_WKF_STATE_INIT) == 0 && rcv_ms >= 0 && rcv_ms < kWeekMs;
    if (sflags & GPSX_WKF_STATE_INIT) {
#pragma unroll
      for (int i = 0; i < 8; i++)
        sane = sane && P[tri(i, i)] > 0.0;
    }
    kind = !sane ? kBad : ((sflags & GPSX_WKF_STATE_INIT) ? kRun : kNotInit);
  }
  if (kind == kBad && j == 0 && bad_state)
    *bad_state = 1u;
  if (kind == kNotInit && fix) {
    const gpsx_wfix_t *p = fix + r;
    if (p->flags & GPSX_WFIX_FIX) {
      const double u = 1000.0 * (p->rx_tow_s - p->dtr_s), m = rint(u);
      if (__builtin_fabs(m) < 9007199254740992.0) {
        rcv_ms = (long long)m;
        week = p->week;
        if (rcv_ms >= kWeekMs) {
          rcv_ms -= kWeekMs;
          week += 1;
        }
        if (rcv_ms < 0) {
          rcv_ms += kWeekMs;
          week -= 1;
        }
        if (rcv_ms >= 0 && rcv_ms < kWeekMs) {
          x[0] = p->rr[0];
          x[1] = p->rr[1];
          x[2] = p->rr[2];
          x[3] = kMs * (m - u);
          if (vel && (vel[r].flags & GPSX_WVEL_VEL)) {
            x[4] = vel[r].vel[0];
            x[5] = vel[r].vel[1];
            x[6] = vel[r].vel[2];
            x[7] = kC * vel[r].drift_s_s;
          }
#pragma unroll
          for (int i = 0; i < 8; i++)
            P[tri(i, i)] = i < 3 ? cfg.p0_pos * cfg.p0_pos : (i == 3 ? cfg.p0_clk * cfg.p0_clk : (i < 7 ? cfg.p0_vel * cfg.p0_vel : cfg.p0_drift * cfg.p0_drift));
          n_starved = 0;
          n_init += 1u;
          kind = kInit;
        }
      }
    }
  }
  const bool run = kind == kRun;

  // ---- the time base, the prediction (a group that does not run: on zeros, masked at the end) ----
  if (run) {
    rcv_ms += (long long)n_blocks;
    if (rcv_ms >= kWeekMs) {
      rcv_ms -= kWeekMs;
      week += 1;
    }
    const double dt = (double)n_blocks * 1e-3, t3 = dt * dt * dt / 3.0, t2 = dt * dt / 2.0;
#pragma unroll
    for (int i = 0; i < 4; i++)
      x[i] = x[i] + dt * x[4 + i];
    double pp[10];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int k = i; k < 4; k++)
        pp[tri(i, k) - (i == 0 ? 0 : (i == 1 ? 4 : (i == 2 ? 8 : 12)))] =
            (P[tri(i, k)] + dt * (P[tri(i, 4 + k)] + P[tri(k, 4 + i)])) + (dt * dt) * P[tri(4 + i, 4 + k)];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int k = 0; k < 4; k++)
        P[tri(i, 4 + k)] = P[tri(i, 4 + k)] + dt * P[tri(4 + i, 4 + k)];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int k = i; k < 4; k++)
        P[tri(i, k)] = pp[tri(i, k) - (i == 0 ? 0 : (i == 1 ? 4 : (i == 2 ? 8 : 12)))];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const double qpp = i < 3 ? cfg.q_acc * t3 : cfg.q_clk_f * dt + cfg.q_clk_g * t3;
      const double qpv = (i < 3 ? cfg.q_acc : cfg.q_clk_g) * t2, qvv = (i < 3 ? cfg.q_acc : cfg.q_clk_g) * dt;
      P[tri(i, i)] += qpp;
      P[tri(i, 4 + i)] += qpv;
      P[tri(4 + i, 4 + i)] += qvv;
    }
  }

  // ---- the lane's records ----
  gpsx_wobs_t o = {};
  gpsx_weph_t e = {};
  bool may_pr = false, may_dop = false;
  if (slot && run) {
    o = obs[at];
    e = eph[at];
    const bool usable = (o.flags & GPSX_WOBS_VALID) != 0 && (e.flags & GPSX_WEPH_VALID) != 0 && e.svh == 0;
    const u32 lf = lock ? lock[at].flags : (GPSX_WLOCK_CODE | GPSX_WLOCK_CARRIER);
    may_pr = usable && (lf & GPSX_WLOCK_CODE) != 0;
    may_dop = usable && (lf & GPSX_WLOCK_CARRIER) != 0 && __builtin_fabsf(o.if_freq_offset_hz) <= 3.402823466e+38f;
  }
  double ion[8];
  choose_ion(cfg.ion, ion);
  double lat, lon, hgt;
  geodetic(x[0], x[1], x[2], lat, lon, hgt);
  const double tow = (double)rcv_ms / 1000.0;

  // ---- the satellite and the two rows at x-; a repaired slot once more at its corrected transmit time (lane-local) ----
  bool prow = false, drow = false, k_out = false;
  double v = 0.0, sig2 = 0.0, h0 = 0.0, h1 = 0.0, h2 = 0.0, y = 0.0, a0 = 0.0, a1 = 0.0, a2 = 0.0;
  int k_ms = 0;
#pragma unroll 1
  for (int pass = 0; pass < 2; pass++) {
    prow = false;
    drow = false;
    SatState s = {};
    bool sat = false;
    const long long tx_ms = o.tx_ms + (long long)k_ms;
    if (may_pr || may_dop)
      sat = sat_at_clock(e, ((double)tx_ms - (double)o.code_phase_fine / 16368.0) / 1000.0, s);
    double l0 = s.px - x[0], l1 = s.py - x[1], l2 = s.pz - x[2];
    const double range = sqrt(l0 * l0 + l1 * l1 + l2 * l2);
    if (sat && !(range == 0.0)) {
      l0 /= range;
      l1 /= range;
      l2 /= range;
      const double kk = kOmegaE / kC;
      if (may_dop) {
        a0 = -l0 - kk * s.py;
        a1 = -l1 + kk * s.px;
        a2 = -l2;
        y = cfg.mps_per_hz * (double)o.if_freq_offset_hz - (l0 * s.vx + l1 * s.vy + l2 * s.vz + kk * (s.vx * x[1] - s.vy * x[0]) - kC * s.rate);
        y = y - (a0 * x[4] + a1 * x[5] + a2 * x[6] + x[7]);
        drow = true;
      }
      const double rn = sqrt(s.px * s.px + s.py * s.py + s.pz * s.pz);
      const double rho = range + kOmegaE * (s.px * x[1] - s.py * x[0]) / kC;
      double az, el;
      az_el(l0, l1, l2, lat, lon, hgt, az, el);
      if (may_pr && !(rn < kRe) && !(rho <= 0.0) && !(el < 0.0)) {
        const double pr = 299792458e-3 * ((double)fold_ms(rcv_ms - tx_ms) + (double)o.code_phase_fine / 16368.0);
        double dion, dtrp;
        const double var = pr_model(tow, ion, lat, lon, hgt, az, el, s.svar, dion, dtrp);
        v = (pr - kC * e.tgd) - (rho + dion + dtrp + x[3] - kC * s.clk);
        sig2 = var + cfg.sig_pr_m * cfg.sig_pr_m;
        h0 = -l0;
        h1 = -l1;
        h2 = -l2;
        prow = true;
      }
    }
    if (pass == 0 && prow && (o.flags & GPSX_WOBS_AMBIGUOUS)) {
      const double q = rint(v / kMs);
      if (!(__builtin_fabs(q) <= 1.0))   // (a NaN too)
        k_out = true;
      else if (q != 0.0) {
        k_ms = (int)q;
        continue;
      }
    }
    break;
  }

  // ---- the gate: each row against h P- h^T + sig2 ----
  const double gg = cfg.gate * cfg.gate;
  double s_pr, s_dop;
  {
    const double t0 = (P[tri(0, 0)] * h0 + P[tri(0, 1)] * h1 + P[tri(0, 2)] * h2) + P[tri(0, 3)];
    const double t1 = (P[tri(1, 0)] * h0 + P[tri(1, 1)] * h1 + P[tri(1, 2)] * h2) + P[tri(1, 3)];
    const double t2 = (P[tri(2, 0)] * h0 + P[tri(2, 1)] * h1 + P[tri(2, 2)] * h2) + P[tri(2, 3)];
    const double t3 = (P[tri(3, 0)] * h0 + P[tri(3, 1)] * h1 + P[tri(3, 2)] * h2) + P[tri(3, 3)];
    s_pr = (h0 * t0 + h1 * t1 + h2 * t2 + t3) + sig2;
    const double u0 = (P[tri(4, 4)] * a0 + P[tri(4, 5)] * a1 + P[tri(4, 6)] * a2) + P[tri(4, 7)];
    const double u1 = (P[tri(5, 4)] * a0 + P[tri(5, 5)] * a1 + P[tri(5, 6)] * a2) + P[tri(5, 7)];
    const double u2 = (P[tri(6, 4)] * a0 + P[tri(6, 5)] * a1 + P[tri(6, 6)] * a2) + P[tri(6, 7)];
    const double u3 = (P[tri(7, 4)] * a0 + P[tri(7, 5)] * a1 + P[tri(7, 6)] * a2) + P[tri(7, 7)];
    s_dop = (a0 * u0 + a1 * u1 + a2 * u2 + u3) + cfg.sig_dop_mps * cfg.sig_dop_mps;
  }
  const bool pr_ok = prow && !k_out && finite(v) && finite(s_pr) && !(v * v > gg * s_pr);
  const bool dop_ok = drow && finite(y) && finite(s_dop) && !(y * y > gg * s_dop);
  const u64 group_bits = ln.group_bits;
  const u64 pr_mask = (__ballot(pr_ok) >> base) & group_bits, dop_mask = (__ballot(dop_ok) >> base) & group_bits;
  const u64 rej_pr = (__ballot(prow && !pr_ok) >> base) & group_bits, rej_dop = (__ballot(drow && !dop_ok) >> base) & group_bits;
  const u64 plus_mask = (__ballot(k_ms > 0) >> base) & group_bits, minus_mask = (__ballot(k_ms < 0) >> base) & group_bits;

  // ---- the information sums: 10 + 4 per block, the two NIS ----
  const double wp = pr_ok ? 1.0 : 0.0, wd = dop_ok ? 1.0 : 0.0;
  const double hp[4] = {pr_ok ? h0 : 0.0, pr_ok ? h1 : 0.0, pr_ok ? h2 : 0.0, wp}, hd[4] = {dop_ok ? a0 : 0.0, dop_ok ? a1 : 0.0, dop_ok ? a2 : 0.0, wd};
  const double sp2 = pr_ok ? sig2 : 1.0, sd2 = cfg.sig_dop_mps * cfg.sig_dop_mps, vp = pr_ok ? v : 0.0, vd = dop_ok ? y : 0.0;
  double info[36], gvec[8];
#pragma unroll
  for (int i = 0; i < 36; i++)
    info[i] = 0.0;
#pragma unroll
  for (int i = 0; i < 4; i++) {
#pragma unroll
    for (int k = i; k < 4; k++) {
      info[tri(i, k)] = group_sum((hp[i] * hp[k]) / sp2, w);
      info[tri(4 + i, 4 + k)] = group_sum((hd[i] * hd[k]) / sd2, w);
    }
    gvec[i] = group_sum((hp[i] * vp) / sp2, w);
    gvec[4 + i] = group_sum((hd[i] * vd) / sd2, w);
  }
  const double nis_pr = group_sum(pr_ok ? v * v / s_pr : 0.0, w);
  const double nis_dop = group_sum(dop_ok ? y * y / s_dop : 0.0, w);   // (the last shuffle)

  // ---- the update, in every lane: L = (P-)^-1 + I, P+ = L^-1, x+ = x- + P+ g ----
  const int n_pr = __popcll(pr_mask), n_dop = __popcll(dop_mask);
  const bool any = n_pr + n_dop > 0;
  double A[36];
#pragma unroll
  for (int i = 0; i < 36; i++)
    A[i] = P[i];
  bool ok = spd_inverse(A);
#pragma unroll
  for (int i = 0; i < 36; i++)
    A[i] += info[i];
  ok = spd_inverse(A) && ok;
  if (run && any) {
    double dx[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
      double t = A[tri(i, 0)] * gvec[0];
#pragma unroll
      for (int k = 1; k < 8; k++)
        t += A[tri(i, k)] * gvec[k];
      dx[i] = t;
    }
#pragma unroll
    for (int i = 0; i < 8; i++)
      x[i] = x[i] + dx[i];
#pragma unroll
    for (int i = 0; i < 36; i++)
      P[i] = A[i];
  }

  // ---- starvation, steering, the record and the state, by the group's first lane ----
  if (in_rx && j == 0) {
    u32 flags = kind == kBad ? GPSX_WKF_BAD : (kind == kNotInit ? GPSX_WKF_NOT_INIT : (kind == kInit ? GPSX_WKF_INIT : 0u));
    if (run) {
      flags = any ? GPSX_WKF_UPDATED : GPSX_WKF_COAST;
      n_starved = n_pr == 0 ? n_starved + 1u : 0u;
      if ((any && !ok) || n_starved > (u32)cfg.max_coast)
        flags = GPSX_WKF_LOST;
      else {
        if (x[3] > kMs / 2.0) {
          x[3] -= kMs;
          rcv_ms -= 1;
          if (rcv_ms < 0) {
            rcv_ms += kWeekMs;
            week -= 1;
          }
          flags |= GPSX_WKF_STEERED;
        } else if (x[3] < -kMs / 2.0) {
          x[3] += kMs;
          rcv_ms += 1;
          if (rcv_ms >= kWeekMs) {
            rcv_ms -= kWeekMs;
            week += 1;
          }
          flags |= GPSX_WKF_STEERED;
        }
        if (plus_mask | minus_mask)
          flags |= GPSX_WKF_REPAIRED;
        if (rej_pr | rej_dop)
          flags |= GPSX_WKF_REJECTED;
      }
    }
    gpsx_wkf_t out = {};
    if (flags & (GPSX_WKF_INIT | GPSX_WKF_UPDATED | GPSX_WKF_COAST)) {
      double glat, glon, ghgt;
      geodetic(x[0], x[1], x[2], glat, glon, ghgt);
      double east, north, up;
      to_enu(glat, glon, x[4], x[5], x[6], east, north, up);
      bool fin = finite(glat) && finite(glon) && finite(ghgt) && finite(east) && finite(north) && finite(up) && finite(nis_pr) && finite(nis_dop);
      float sg[8];
#pragma unroll
      for (int i = 0; i < 8; i++) {
        sg[i] = (float)sqrt(P[tri(i, i)]);
        fin = fin && finite(x[i]) && finite((double)sg[i]);
      }
#pragma unroll
      for (int i = 0; i < 36; i++)
        fin = fin && finite(P[i]);
      if (!fin)
        flags = kind == kInit ? GPSX_WKF_NOT_INIT : GPSX_WKF_LOST;
      else {
        if (run) {
          out.n_pr = n_pr;
          out.n_dop = n_dop;
          out.n_starved = n_starved;
          out.pr_mask = pr_mask;
          out.dop_mask = dop_mask;
          out.rej_pr_mask = rej_pr;
          out.rej_dop_mask = rej_dop;
          out.plus_mask = plus_mask;
          out.minus_mask = minus_mask;
          out.nis_pr = nis_pr;
          out.nis_dop = nis_dop;
        }
        out.rr[0] = x[0];
        out.rr[1] = x[1];
        out.rr[2] = x[2];
        out.clk_m = x[3];
        out.vel[0] = x[4];
        out.vel[1] = x[5];
        out.vel[2] = x[6];
        out.cdrift_mps = x[7];
        out.geo[0] = glat;
        out.geo[1] = glon;
        out.geo[2] = ghgt;
        out.enu[0] = east;
        out.enu[1] = north;
        out.enu[2] = up;
#pragma unroll
        for (int i = 0; i < 8; i++)
          out.sigma[i] = sg[i];
        out.rcv_ms = rcv_ms;
        out.week = week;
      }
    }
    out.flags = flags;
    kf[r] = out;
    if (flags & (GPSX_WKF_INIT | GPSX_WKF_UPDATED | GPSX_WKF_COAST | GPSX_WKF_LOST)) {
      gpsx_wkf_state_t st = {};
      if (flags & GPSX_WKF_LOST) {
        st.n_init = n_init;
        st.n_lost = n_lost + 1u;
      } else {
#pragma unroll
        for (int i = 0; i < 8; i++)
          st.x[i] = x[i];
#pragma unroll
        for (int i = 0; i < 36; i++)
          st.P[i] = P[i];
        st.rcv_ms = rcv_ms;
        st.week = week;
        st.flags = GPSX_WKF_STATE_INIT;
        st.n_starved = n_starved;
        st.n_init = n_init;
        st.n_lost = n_lost;
      }
      state[r] = st;
    }
  }
}

void launch_wkf(hipStream_t s, const gpsx_wkf_cfg_t &cfg, const gpsx_wobs_t *d_obs, const gpsx_weph_t *d_eph, const gpsx_wlock_t *d_lock,
                const gpsx_wfix_t *d_fix, const gpsx_wvel_t *d_vel, int n_rx, int n_blocks, gpsx_wkf_state_t *d_state, gpsx_wkf_t *d_kf,
                uint32_t *d_bad_state)
{
  if (n_rx < 1 || n_rx > (1 << 20) || cfg.ch_per_rx < 1 || cfg.ch_per_rx > 64 || n_blocks < 1 || n_blocks > 4096)
    return;
  const Geometry g = geometry_of(n_rx, cfg.ch_per_rx);
  hipLaunchKernelGGL(k_wkf, dim3(g.grid), dim3(256), 0, s, cfg, d_obs, d_eph, d_lock, d_fix, d_vel, n_rx, n_blocks, g.w, g.log2w, d_state, d_kf,
                     d_bad_state);
}

}  // namespace gpsx
