// k_wvel.hip -- EXTENSION, not in the reference: every receiver's velocity and clock drift from the weighted chain's carrier frequencies,
// ephemeris records and position fixes, on the device (include/gpsx.h gpsx_wvel).
//
// k_wfix's lane layout: one slot per lane; a receiver is a group of W lanes, W the smallest power of two >= ch_per_rx, so a wave holds
// 64 / W receivers and a workgroup of 256 lanes 256 / W.  Once per lane: the slot's 32-byte observable and 256-byte ephemeris record,
// the satellite's position, velocity and clock rate at the transmit time its own clock reads (no pseudorange, no reference slot), the
// lane's row and right-hand side.  Once per group: the 10 + 4 sums of the symmetric 4 x 4 normal system by xor-butterflies of width W,
// the rows' mask from a ballot, the Cholesky solve and the inverse's velocity block in every lane, unrolled; then the residuals at the
// solution and their sum of squares by one more butterfly.  The model is linear: one solve, no iteration, no atmosphere, no geodetic
// fixed point.  FP64 on the vector ALU, no LDS, no scratch (build.py check_wvel).
//
// Every cross-lane operation runs under wave-uniform control flow: there is no branch around a ballot or a shuffle, a lane without a
// row adds zeros, and nothing returns before the last shuffle.  The only lane-local loop is Kepler's, bounded at 30 steps.
// gpsx_wsolve_parts.hpp has the constants, the small helpers and the lane geometry; everything else is this file's own text, which
// keeps the kernel instruction for instruction what it was (a shared part moved it by 0.4 % at 4 slots per receiver).
#include <hip/hip_runtime.h>

#include <cstddef>

#include "gpsx_device.hpp"
#include "gpsx_kernels.hpp"
#include "gpsx_wsolve_parts.hpp"

namespace gpsx {
using namespace wsolve;

static_assert(sizeof(gpsx_wvel_cfg_t) == 32 && offsetof(gpsx_wvel_cfg_t, ch_per_rx) == 8 && offsetof(gpsx_wvel_cfg_t, min_sats) == 12 &&
              offsetof(gpsx_wvel_cfg_t, reserved) == 16, "gpsx_wvel_cfg_t layout");
static_assert(sizeof(gpsx_wvel_t) == 112 && offsetof(gpsx_wvel_t, n_used) == 4 && offsetof(gpsx_wvel_t, used_mask) == 8 &&
              offsetof(gpsx_wvel_t, vel) == 16 && offsetof(gpsx_wvel_t, drift_s_s) == 40 && offsetof(gpsx_wvel_t, enu) == 48 &&
              offsetof(gpsx_wvel_t, qv) == 72 && offsetof(gpsx_wvel_t, resid_rms_mps) == 96 && offsetof(gpsx_wvel_t, reserved) == 104,
              "gpsx_wvel_t layout");

__global__ __launch_bounds__(256) void k_wvel(gpsx_wvel_cfg_t cfg, const gpsx_wobs_t *obs, const gpsx_weph_t *eph, const gpsx_wlock_t *lock,
                                              const gpsx_wfix_t *fix, int n_rx, int w, int log2w, gpsx_wvel_t *vel)
{
  const Lane ln = lane_of(w, log2w, n_rx, cfg.ch_per_rx);
  const int j = ln.j, base = ln.base;
  const long long r = ln.r;
  const bool in_rx = ln.in_rx, slot = ln.slot;
  const size_t at = ln.at;

  // ---- the receiver's fix, the lane's records ----
  bool fixed = false;
  u64 fix_mask = 0;
  double r0 = 0.0, r1 = 0.0, r2 = 0.0, lat = 0.0, lon = 0.0;
  if (in_rx) {
    const gpsx_wfix_t *p = fix + r;
    fixed = (p->flags & GPSX_WFIX_FIX) != 0;
    if (fixed) {
      fix_mask = p->used_mask;
      r0 = p->rr[0];
      r1 = p->rr[1];
      r2 = p->rr[2];
      lat = p->geo[0];
      lon = p->geo[1];
    }
  }
  gpsx_wobs_t o = {};
  gpsx_weph_t e = {};
  bool cand = false;
  if (slot && ((fix_mask >> j) & 1ull)) {
    o = obs[at];
    e = eph[at];
    cand = (o.flags & GPSX_WOBS_VALID) != 0 && (e.flags & GPSX_WEPH_VALID) != 0 && e.svh == 0 &&
           __builtin_fabsf(o.if_freq_offset_hz) <= 3.402823466e+38f;
    if (lock)
      cand = cand && (lock[at].flags & GPSX_WLOCK_CARRIER) != 0;
  }

  // ---- the satellite at the transmit time its clock reads: position, velocity, clock rate ----
  double px = 0.0, py = 0.0, pz = 0.0, vx = 0.0, vy = 0.0, vz = 0.0, rate = 0.0;
  bool sat = false;
  if (cand) {
    const double t_sv = ((double)o.tx_ms - (double)o.code_phase_fine / 16368.0) / 1000.0;
    const double toc = (double)(((e.toc_time - 315964800ll) % 604800ll + 604800ll) % 604800ll) + e.toc_sec;
    double tc = fold_s(t_sv - toc);
    tc -= clock_poly(e, tc);
    tc -= clock_poly(e, tc);
    const double t = t_sv - clock_poly(e, tc);
    const double tk = fold_s(t - e.toes);
    if (__builtin_fabs(tk) <= 7201.0 && e.A > 0.0) {
      const double n0 = sqrt(kMu / (e.A * e.A * e.A)) + e.deln;
      const double mean = e.M0 + n0 * tk;
      double ecc = mean, was = 0.0;
      int n = 0;
      for (; __builtin_fabs(ecc - was) > 1E-14 && n < 30; n++) {
        was = ecc;
        ecc -= (ecc - e.e * sin(ecc) - mean) / (1.0 - e.e * cos(ecc));
      }
      if (n < 30) {
        const double se = sin(ecc), ce = cos(ecc);
        const double root = sqrt(1.0 - e.e * e.e), den = 1.0 - e.e * ce;
        double u = atan2(root * se, ce - e.e) + e.omg;
        double rad = e.A * den;
        double inc = e.i0 + e.idot * tk;
        const double s2 = sin(2.0 * u), c2 = cos(2.0 * u);
        const double ed = n0 / den;              // E'
        const double nud = ed * root / den;      // nu'
        const double ud = nud * (1.0 + 2.0 * (e.cus * c2 - e.cuc * s2));
        const double rd = e.A * e.e * ed * se + 2.0 * nud * (e.crs * c2 - e.crc * s2);
        const double id = e.idot + 2.0 * nud * (e.cis * c2 - e.cic * s2);
        const double od = e.OMGd - kOmegaE;
        u += e.cus * s2 + e.cuc * c2;
        rad += e.crs * s2 + e.crc * c2;
        inc += e.cis * s2 + e.cic * c2;
        const double su = sin(u), cu = cos(u), si = sin(inc), ci = cos(inc);
        const double xo = rad * cu, yo = rad * su;
        const double xd = rd * cu - rad * ud * su, yd = rd * su + rad * ud * cu;
        const double node = e.OMG0 + od * tk - kOmegaE * e.toes;
        const double sn = sin(node), cn = cos(node);
        px = xo * cn - yo * ci * sn;
        py = xo * sn + yo * ci * cn;
        pz = yo * si;
        vx = xd * cn - yd * ci * sn + yo * id * si * sn - od * py;
        vy = xd * sn + yd * ci * cn - yo * id * si * cn + od * px;
        vz = yd * si + yo * id * ci;
        rate = e.f1 + 2.0 * e.f2 * fold_s(t - toc) - 2.0 * sqrt(kMu * e.A) * e.e * ce * ed / (kC * kC);
        sat = true;
      }
    }
  }

  // ---- the lane's row ----
  double l0 = px - r0, l1 = py - r1, l2 = pz - r2;
  const double sq = l0 * l0 + l1 * l1 + l2 * l2;   // (counts among the sums: not finite -> NONFINITE)
  const double range = sqrt(sq);
  const bool row = sat && !(range == 0.0);
  const bool wild = row && !finite(sq);
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, y = 0.0;
  if (row) {
    l0 /= range;
    l1 /= range;
    l2 /= range;
    const double k = kOmegaE / kC;
    y = cfg.mps_per_hz * (double)o.if_freq_offset_hz - (l0 * vx + l1 * vy + l2 * vz + k * (vx * r1 - vy * r0) - kC * rate);
    a0 = -l0 - k * py;
    a1 = -l1 + k * px;
    a2 = -l2;
    a3 = 1.0;
  }
  const u64 group_bits = ln.group_bits;
  const u64 rows = (__ballot(row) >> base) & group_bits;
  const u64 wilds = (__ballot(wild) >> base) & group_bits;
  const double n00 = group_sum(a0 * a0, w), n10 = group_sum(a1 * a0, w), n11 = group_sum(a1 * a1, w), n20 = group_sum(a2 * a0, w),
               n21 = group_sum(a2 * a1, w), n22 = group_sum(a2 * a2, w), n30 = group_sum(a3 * a0, w), n31 = group_sum(a3 * a1, w),
               n32 = group_sum(a3 * a2, w), n33 = group_sum(a3 * a3, w), b0 = group_sum(a0 * y, w), b1 = group_sum(a1 * y, w),
               b2 = group_sum(a2 * y, w), b3 = group_sum(a3 * y, w);

  // Cholesky N = L L^T, M = L^-1, x = M^T M b, Q = M^T M; in every lane
  const double p0 = n00, l00 = sqrt(p0), l10 = n10 / l00, l20 = n20 / l00, l30 = n30 / l00;
  const double p1 = n11 - l10 * l10, l11 = sqrt(p1), l21 = (n21 - l20 * l10) / l11, l31 = (n31 - l30 * l10) / l11;
  const double p2 = n22 - l20 * l20 - l21 * l21, l22 = sqrt(p2), l32 = (n32 - l30 * l20 - l31 * l21) / l22;
  const double p3 = n33 - l30 * l30 - l31 * l31 - l32 * l32, l33 = sqrt(p3);
  const double m00 = 1.0 / l00, m11 = 1.0 / l11, m22 = 1.0 / l22, m33 = 1.0 / l33;
  const double m10 = -(l10 * m00) / l11, m20 = -(l20 * m00 + l21 * m10) / l22, m21 = -(l21 * m11) / l22;
  const double m30 = -(l30 * m00 + l31 * m10 + l32 * m20) / l33, m31 = -(l31 * m11 + l32 * m21) / l33, m32 = -(l32 * m22) / l33;
  const double y0 = m00 * b0, y1 = m10 * b0 + m11 * b1, y2 = m20 * b0 + m21 * b1 + m22 * b2, y3 = m30 * b0 + m31 * b1 + m32 * b2 + m33 * b3;
  const double x0 = m00 * y0 + m10 * y1 + m20 * y2 + m30 * y3, x1 = m11 * y1 + m21 * y2 + m31 * y3, x2 = m22 * y2 + m32 * y3, x3 = m33 * y3;
  const double v = row ? y - (a0 * x0 + a1 * x1 + a2 * x2 + a3 * x3) : 0.0;
  const double ss = group_sum(v * v, w);   // (the last shuffle)

  // ---- the receiver's record, by the group's first lane ----
  if (in_rx && j == 0) {
    const int n_used = __popcll(rows);
    const bool sums_ok = wilds == 0ull && finite(n00) && finite(n10) && finite(n11) && finite(n20) && finite(n21) && finite(n22) && finite(n30) &&
                         finite(n31) && finite(n32) && finite(n33) && finite(b0) && finite(b1) && finite(b2) && finite(b3);
    const double sp = sin(lat), cp = cos(lat), sl = sin(lon), cl = cos(lon);
    const double east = -sl * x0 + cl * x1;
    const double north = -sp * cl * x0 - sp * sl * x1 + cp * x2;
    const double up = cp * cl * x0 + cp * sl * x1 + sp * x2;
    const double drift = x3 / kC, rms = sqrt(ss / (double)n_used);
    const float f0 = (float)(m00 * m00 + m10 * m10 + m20 * m20 + m30 * m30), f1 = (float)(m11 * m11 + m21 * m21 + m31 * m31),
                f2 = (float)(m22 * m22 + m32 * m32), f3 = (float)(m10 * m11 + m20 * m21 + m30 * m31), f4 = (float)(m21 * m22 + m31 * m32),
                f5 = (float)(m20 * m22 + m30 * m32);
    u32 flags;
    if (!fixed)
      flags = GPSX_WVEL_NO_FIX;
    else if (n_used < cfg.min_sats)
      flags = GPSX_WVEL_TOO_FEW;
    else if (!sums_ok)
      flags = GPSX_WVEL_NONFINITE;
    else if (!(p0 > 0.0 && p1 > kPivot * n11 && p2 > kPivot * n22 && p3 > kPivot * n33))
      flags = GPSX_WVEL_SINGULAR;
    else if (!(finite(x0) && finite(x1) && finite(x2) && finite(drift) && finite(east) && finite(north) && finite(up) && finite(rms) &&
               finite((double)f0) && finite((double)f1) && finite((double)f2) && finite((double)f3) && finite((double)f4) && finite((double)f5)))
      flags = GPSX_WVEL_NONFINITE;
    else
      flags = GPSX_WVEL_VEL;
    gpsx_wvel_t out = {};
    out.flags = flags;
    out.n_used = n_used;
    out.used_mask = rows;
    if (flags == GPSX_WVEL_VEL) {
      out.vel[0] = x0;
      out.vel[1] = x1;
      out.vel[2] = x2;
      out.drift_s_s = drift;
      out.enu[0] = east;
      out.enu[1] = north;
      out.enu[2] = up;
      out.qv[0] = f0;
      out.qv[1] = f1;
      out.qv[2] = f2;
      out.qv[3] = f3;
      out.qv[4] = f4;
      out.qv[5] = f5;
      out.resid_rms_mps = rms;
    }
    vel[r] = out;
  }
}

void launch_wvel(hipStream_t s, const gpsx_wvel_cfg_t &cfg, const gpsx_wobs_t *d_obs, const gpsx_weph_t *d_eph, const gpsx_wlock_t *d_lock,
                 const gpsx_wfix_t *d_fix, int n_rx, gpsx_wvel_t *d_vel)
{
  if (n_rx < 1 || n_rx > (1 << 20) || cfg.ch_per_rx < 1 || cfg.ch_per_rx > 64)
    return;
  const Geometry g = geometry_of(n_rx, cfg.ch_per_rx);
  hipLaunchKernelGGL(k_wvel, dim3(g.grid), dim3(256), 0, s, cfg, d_obs, d_eph, d_lock, d_fix, n_rx, g.w, g.log2w, d_vel);
}

}  // namespace gpsx
