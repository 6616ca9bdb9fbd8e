// k_wfix.hip -- EXTENSION, not in the reference: every receiver's position fix from the weighted chain's observables and ephemeris
// records, on the device (include/gpsx.h gpsx_wfix).
//
// One slot per lane; a receiver is a group of W lanes, W the smallest power of two >= ch_per_rx, so a wave holds 64 / W receivers and
// a workgroup of 256 lanes 256 / W.  Once per lane: the slot's 32-byte observable and 256-byte ephemeris record, the pseudorange (the
// host helper's serial scan for the reference slot, run by every lane of the group on values fetched with __shfl: bit-exact), the
// satellite's state at its transmit time -- csrc/gpsx_pvt.cpp's solve(), which keeps it outside the iteration too.  Per iteration: the
// lane's row, residual and variance; the 10 + 4 sums of the symmetric 4 x 4 normal system (and the sum of squared residuals) reduced by
// xor-butterflies of width W; rows and used_mask from a ballot; the Cholesky solve and the inverse's position block in every lane,
// unrolled, nothing indexed by a run-time value.  FP64 on the vector ALU, no LDS, no scratch (build.py check_wfix).
//
// Every cross-lane operation runs under wave-uniform control flow: the pass loop's condition is "a group of this wave is not
// finished", from a ballot, eleven passes at most (ten iterations and the pass that takes the residuals at the final x); a group that
// is finished masks its own updates; nothing returns before the last shuffle.  The lane-local loops are bounded: Kepler at 30 steps as
// on the host, the geodetic fixed point at 30 (a finite position needs about five).
//
// gpsx_wsolve_parts.hpp has what is shared: the constants and models, the lane geometry, the satellite at its transmit time, azimuth
// and elevation, the row's model terms.  The reference scan, the sums, the Cholesky solve and the record's fill are this file's own
// text: shared, they cost 0.4 us at 64 slots per receiver (EXPERIMENTS.md, "One parts header for the solver kernels").
#include <hip/hip_runtime.h>

#include <cstddef>

#include "gpsx_device.hpp"
#include "gpsx_kernels.hpp"
#include "gpsx_wsolve_parts.hpp"

namespace gpsx {
using namespace wsolve;

static_assert(sizeof(gpsx_wfix_cfg_t) == 96 && offsetof(gpsx_wfix_cfg_t, ion) == 8 && offsetof(gpsx_wfix_cfg_t, ch_per_rx) == 72 &&
              offsetof(gpsx_wfix_cfg_t, min_sats) == 76 && offsetof(gpsx_wfix_cfg_t, reserved0) == 80, "gpsx_wfix_cfg_t layout");

__global__ __launch_bounds__(256) void k_wfix(gpsx_wfix_cfg_t cfg, const gpsx_wobs_t *obs, const gpsx_weph_t *eph, const gpsx_wlock_t *lock,
                                              const gpsx_wfix_t *prev, int n_rx, int w, int log2w, gpsx_wfix_t *fix, double *pr_out)
{
  const Lane ln = lane_of(w, log2w, n_rx, cfg.ch_per_rx);
  const int j = ln.j, base = ln.base;
  const long long r = ln.r;
  const bool in_rx = ln.in_rx, slot = ln.slot;
  const size_t at = ln.at;

  // ---- the lane's records; the receiver's start point (read before anything is written: prev may be fix) ----
  gpsx_wobs_t o = {};
  gpsx_weph_t e = {};
  bool usable = false;
  if (slot) {
    o = obs[at];
    e = eph[at];
    usable = (o.flags & GPSX_WOBS_VALID) != 0 && (e.flags & GPSX_WEPH_VALID) != 0;
    if (lock)
      usable = usable && (lock[at].flags & GPSX_WLOCK_CODE) != 0;
  }
  double x0 = 0.0, x1 = 0.0, x2 = 0.0, x3 = 0.0;
  if (in_rx && prev) {
    const gpsx_wfix_t *p = prev + r;
    if (p->flags & GPSX_WFIX_FIX) {
      x0 = p->rr[0];
      x1 = p->rr[1];
      x2 = p->rr[2];
    }
  }

  // ---- gpsx_wobs_pseudoranges over the usable slots: its serial scan, in every lane of the group ----
  int ref = -1, count = 0, week = 0;
  long long ref_tx = 0;
  float ref_ph = 0.0f;
#pragma unroll 1
  for (int k = 0; k < w; k++) {
    const int src = base + k;
    const long long tx_k = __shfl(o.tx_ms, src);
    const float ph_k = __shfl(o.code_phase_fine, src);
    const int us_k = __shfl((int)usable, src), week_k = __shfl(e.week, src);
    if (us_k) {
      count++;
      if (ref < 0 || (double)fold_ms(tx_k - ref_tx) - ((double)ph_k - (double)ref_ph) / 16368.0 > 0.0) {
        ref = k;
        ref_tx = tx_k;
        ref_ph = ph_k;
        week = week_k;
      }
    }
  }
  double pr = 0.0, rx_tow = 0.0;
  if (ref >= 0) {
    if (usable)
      pr = 299792458e-3 * ((double)fold_ms(ref_tx - o.tx_ms) + ((double)o.code_phase_fine - (double)ref_ph) / 16368.0 + cfg.offset_ms);
    const double rx = ((double)ref_tx - (double)ref_ph / 16368.0 + cfg.offset_ms) / 1000.0;
    rx_tow = rx >= 604800.0 ? rx - 604800.0 : (rx < 0.0 ? rx + 604800.0 : rx);
  }
  const bool time_ok = finite(rx_tow);
  if (!time_ok)
    rx_tow = 0.0;
  if (slot && pr_out)
    pr_out[at] = finite(pr) ? pr : 0.0;

  // ---- the observation time, the satellite at its transmit time (satposs) ----
  const GTime t_obs = obs_time(week, rx_tow);
  const double tow = tow_of(t_obs);
  double px = 0.0, py = 0.0, pz = 0.0, clk = 0.0, svar = 0.0;
  bool cand = false;   // the solver has a satellite record for this slot (health and all)
  if (usable)
    cand = sat_at_transmit(e, t_obs, pr, px, py, pz, clk, svar);
  const bool healthy = e.svh == 0;
  const double tgd = kC * e.tgd;
  const double rn = sqrt(px * px + py * py + pz * pz);
  double ion_sq = 0.0;
#pragma unroll
  for (int i = 0; i < 8; i++)
    ion_sq += cfg.ion[i] * cfg.ion[i];
  double ion[8];
#pragma unroll
  for (int i = 0; i < 8; i++)
    ion[i] = ion_sq <= 0.0 ? kIonDefault[i] : cfg.ion[i];

  // ---- estpos / rescode ----
  const u64 group_bits = group_mask(w);
  u32 flags = 0;
  int mode = 0;   // 0: iterating, 1: converged, the residuals at the final x are due, 2: finished
  if (!in_rx)
    mode = 2;
  else if (!time_ok) {
    flags = GPSX_WFIX_NONFINITE;
    mode = 2;
  } else if (count < cfg.min_sats) {
    flags = GPSX_WFIX_TOO_FEW;
    mode = 2;
  }
  int n_used = 0, n_iter = 0;
  u64 used_mask = 0;
  double q00 = 0.0, q11 = 0.0, q22 = 0.0, q01 = 0.0, q12 = 0.0, q02 = 0.0, rms = 0.0, lat_out = 0.0, lon_out = 0.0, hgt_out = 0.0;

#pragma unroll 1
  for (int pass = 0; pass <= kMaxIter; pass++) {
    if (__ballot(mode != 2) == 0ull)   // (wave-uniform)
      break;
    double lat, lon, hgt;
    geodetic(x0, x1, x2, lat, lon, hgt);
    // the lane's row
    bool row = cand && mode != 2 && !(rn < kRe);
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, y = 0.0, v = 0.0;
    if (row) {
      double l0 = px - x0, l1 = py - x1, l2 = pz - x2;
      const double range = sqrt(l0 * l0 + l1 * l1 + l2 * l2);
      l0 /= range;
      l1 /= range;
      l2 /= range;
      const double rho = range + kOmegaE * (px * x1 - py * x0) / kC;
      row = !(rho <= 0.0);
      double az, el;
      az_el(l0, l1, l2, lat, lon, hgt, az, el);
      row = row && !(el < 0.0) && healthy;
      if (row) {
        double dion, dtrp;
        const double var = pr_model(tow, ion, lat, lon, hgt, az, el, svar, dion, dtrp);
        v = (pr - tgd) - (rho + dion + dtrp + x3 - kC * clk);
        const double sig = sqrt(var);
        a0 = -l0 / sig;
        a1 = -l1 / sig;
        a2 = -l2 / sig;
        a3 = 1.0 / sig;
        y = v / sig;
      }
    }
    const u64 rows = (__ballot(row) >> base) & group_bits;
    const bool counted = mode == 1 ? (row && ((used_mask >> j) & 1ull)) : row;
    const double vv = counted ? v : 0.0;
    const double n00 = group_sum(a0 * a0, w), n10 = group_sum(a1 * a0, w), n11 = group_sum(a1 * a1, w), n20 = group_sum(a2 * a0, w),
                 n21 = group_sum(a2 * a1, w), n22 = group_sum(a2 * a2, w), n30 = group_sum(a3 * a0, w), n31 = group_sum(a3 * a1, w),
                 n32 = group_sum(a3 * a2, w), n33 = group_sum(a3 * a3, w), b0 = group_sum(a0 * y, w), b1 = group_sum(a1 * y, w),
                 b2 = group_sum(a2 * y, w), b3 = group_sum(a3 * y, w), ss = group_sum(vv * vv, w);

    // Cholesky N = L L^T, M = L^-1, dx = M^T M b, Q = M^T M; computed by every lane, used by the groups that iterate
    const double p0 = n00, l00 = sqrt(p0), l10 = n10 / l00, l20 = n20 / l00, l30 = n30 / l00;
    const double p1 = n11 - l10 * l10, l11 = sqrt(p1), l21 = (n21 - l20 * l10) / l11, l31 = (n31 - l30 * l10) / l11;
    const double p2 = n22 - l20 * l20 - l21 * l21, l22 = sqrt(p2), l32 = (n32 - l30 * l20 - l31 * l21) / l22;
    const double p3 = n33 - l30 * l30 - l31 * l31 - l32 * l32, l33 = sqrt(p3);
    const double m00 = 1.0 / l00, m11 = 1.0 / l11, m22 = 1.0 / l22, m33 = 1.0 / l33;
    const double m10 = -(l10 * m00) / l11, m20 = -(l20 * m00 + l21 * m10) / l22, m21 = -(l21 * m11) / l22;
    const double m30 = -(l30 * m00 + l31 * m10 + l32 * m20) / l33, m31 = -(l31 * m11 + l32 * m21) / l33, m32 = -(l32 * m22) / l33;
    const double y0 = m00 * b0, y1 = m10 * b0 + m11 * b1, y2 = m20 * b0 + m21 * b1 + m22 * b2, y3 = m30 * b0 + m31 * b1 + m32 * b2 + m33 * b3;
    const double d0 = m00 * y0 + m10 * y1 + m20 * y2 + m30 * y3, d1 = m11 * y1 + m21 * y2 + m31 * y3, d2 = m22 * y2 + m32 * y3, d3 = m33 * y3;
    const bool sums_ok = finite(n00) && finite(n10) && finite(n11) && finite(n20) && finite(n21) && finite(n22) && finite(n30) && finite(n31) &&
                         finite(n32) && finite(n33) && finite(b0) && finite(b1) && finite(b2) && finite(b3);

    if (mode == 1) {   // the residuals at the final x
      rms = sqrt(ss / (double)n_used);
      lat_out = lat;
      lon_out = lon;
      hgt_out = hgt;
      flags = GPSX_WFIX_FIX;
      mode = 2;
    } else if (mode == 0) {
      n_iter = pass + 1;
      n_used = __popcll(rows);
      used_mask = rows;
      if (n_used < cfg.min_sats) {
        flags = GPSX_WFIX_TOO_FEW;
        mode = 2;
      } else if (!sums_ok) {
        flags = GPSX_WFIX_NONFINITE;
        mode = 2;
      } else if (!(p0 > 0.0 && p1 > kPivot * n11 && p2 > kPivot * n22 && p3 > kPivot * n33)) {
        flags = GPSX_WFIX_SINGULAR;
        mode = 2;
      } else if (!(finite(d0) && finite(d1) && finite(d2) && finite(d3))) {
        flags = GPSX_WFIX_NONFINITE;
        mode = 2;
      } else {
        x0 += d0;
        x1 += d1;
        x2 += d2;
        x3 += d3;
        if (d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3 < 1E-8) {
          q00 = m00 * m00 + m10 * m10 + m20 * m20 + m30 * m30;
          q11 = m11 * m11 + m21 * m21 + m31 * m31;
          q22 = m22 * m22 + m32 * m32;
          q01 = m10 * m11 + m20 * m21 + m30 * m31;
          q12 = m21 * m22 + m31 * m32;
          q02 = m20 * m22 + m30 * m32;
          mode = 1;
        } else if (pass + 1 == kMaxIter) {
          flags = GPSX_WFIX_NO_CONV;
          mode = 2;
        }
      }
    }
  }

  // ---- the receiver's record, by the group's first lane ----
  if (in_rx && j == 0) {
    gpsx_wfix_t out = {};
    const float f0 = (float)q00, f1 = (float)q11, f2 = (float)q22, f3 = (float)q01, f4 = (float)q12, f5 = (float)q02;
    const double dtr = x3 / kC;
    if (flags == GPSX_WFIX_FIX && !(finite(x0) && finite(x1) && finite(x2) && finite(dtr) && finite(lat_out) && finite(lon_out) && finite(hgt_out) &&
                                    finite(rms) && finite((double)f0) && finite((double)f1) && finite((double)f2) && finite((double)f3) &&
                                    finite((double)f4) && finite((double)f5)))
      flags = GPSX_WFIX_NONFINITE;
    out.flags = flags;
    out.n_used = n_used;
    out.n_iter = n_iter;
    out.ref_slot = ref;
    out.used_mask = used_mask;
    out.rx_tow_s = rx_tow;
    out.week = week;
    if (flags == GPSX_WFIX_FIX) {
      out.rr[0] = x0;
      out.rr[1] = x1;
      out.rr[2] = x2;
      out.dtr_s = dtr;
      out.geo[0] = lat_out;
      out.geo[1] = lon_out;
      out.geo[2] = hgt_out;
      out.qr[0] = f0;
      out.qr[1] = f1;
      out.qr[2] = f2;
      out.qr[3] = f3;
      out.qr[4] = f4;
      out.qr[5] = f5;
      out.resid_rms_m = rms;
    }
    fix[r] = out;
  }
}

void launch_wfix(hipStream_t s, const gpsx_wfix_cfg_t &cfg, const gpsx_wobs_t *d_obs, const gpsx_weph_t *d_eph, const gpsx_wlock_t *d_lock,
                 const gpsx_wfix_t *d_prev, int n_rx, gpsx_wfix_t *d_fix, double *d_pr_m)
{
  if (n_rx < 1 || n_rx > (1 << 20) || cfg.ch_per_rx < 1 || cfg.ch_per_rx > 64)
    return;
  const Geometry g = geometry_of(n_rx, cfg.ch_per_rx);
  hipLaunchKernelGGL(k_wfix, dim3(g.grid), dim3(256), 0, s, cfg, d_obs, d_eph, d_lock, d_prev, n_rx, g.w, g.log2w, d_fix, d_pr_m);
}

}  // namespace gpsx
