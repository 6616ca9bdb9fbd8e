// k_wfde.hip -- EXTENSION, not in the reference: every receiver's position fix with the ambiguous millisecond repaired and faulty
// slots detected and excluded, on the device (include/gpsx.h gpsx_wfde).
//
// k_wfix's lane layout and solver, with a loop over ROUNDS around the pass loop: one slot per lane, a receiver a group of W lanes,
// W the smallest power of two >= ch_per_rx.  A round is gpsx_wfix's definition on the group's active slots with tx_ms + k_j: the
// serial scan for the reference slot, the pseudoranges, the satellites at their transmit times (the 256-byte ephemeris record is
// read again in every round, not kept in registers), then at most eleven passes.  Round 0 of a group that repairs runs on the
// unambiguous slots, the ambiguous ones ride along as probes -- they form their row at every x but enter no sum -- and give their
// k_j from the residual at the final x.  Every other round ends in the test of T = sum y^2 against the Wilson-Hilferty limit and,
// where it fails, in the exclusion of the slot with the largest w^2 = y^2 / (1 - h_jj): an arg-max butterfly on (value, slot).
//
// k_wfix.hip's solver text is repeated here, not shared: k_wfix must keep its instruction stream, and helpers change code
// generation in this file's neighbours.  The arithmetic that gpsx_wfix defines is written operation for operation as there, so
// with repair = 0 and max_excl = 0 the fix records and pseudoranges are k_wfix's bytes.
//
// Every cross-lane operation runs under wave-uniform control flow: the round loop and the pass loop both run while a ballot says
// "a group of this wave is not finished"; a group that is finished masks its own updates (groups of one wave routinely sit in
// different rounds); nothing returns before the last shuffle.  Every loop is bounded: max_excl + 2 rounds of at most eleven passes,
// Kepler at 30 steps, the geodetic fixed point at 30.  FP64 on the vector ALU, no LDS, no scratch (build.py check_wfde).
#include <hip/hip_runtime.h>

#include <cstddef>

#include "gpsx_device.hpp"
#include "gpsx_kernels.hpp"

namespace gpsx {

namespace {

static_assert(sizeof(gpsx_wfde_cfg_t) == 128 && offsetof(gpsx_wfde_cfg_t, fix) == 0 && offsetof(gpsx_wfde_cfg_t, z_global) == 96 &&
              offsetof(gpsx_wfde_cfg_t, max_excl) == 104 && offsetof(gpsx_wfde_cfg_t, repair) == 108 && offsetof(gpsx_wfde_cfg_t, reserved) == 112,
              "gpsx_wfde_cfg_t layout");
static_assert(sizeof(gpsx_wfde_t) == 64 && offsetof(gpsx_wfde_t, n_rounds) == 4 && offsetof(gpsx_wfde_t, n_excluded) == 8 &&
              offsetof(gpsx_wfde_t, dof) == 12 && offsetof(gpsx_wfde_t, excl_mask) == 16 && offsetof(gpsx_wfde_t, plus_mask) == 24 &&
              offsetof(gpsx_wfde_t, minus_mask) == 32 && offsetof(gpsx_wfde_t, t_stat) == 40 && offsetof(gpsx_wfde_t, t_limit) == 48 &&
              offsetof(gpsx_wfde_t, reserved) == 56, "gpsx_wfde_t layout");
static_assert(sizeof(gpsx_wfix_t) == 128 && sizeof(gpsx_wobs_t) == 32 && sizeof(gpsx_weph_t) == 256 && sizeof(gpsx_wlock_t) == 64,
              "the records this stage reads and writes");

constexpr double kC = 299792458.0;
constexpr double kPi = 3.1415926535897932;
constexpr double kMu = 3.9860050E14;
constexpr double kOmegaE = 7.2921151467E-5;
constexpr double kRe = 6378137.0;
constexpr double kFe = 1.0 / 298.257223563;
constexpr int kMaxIter = 10;
constexpr double kPivot = 1E-10;   // a pivot at or below this share of its diagonal element is round-off: SINGULAR
constexpr double kMsM = 299792.458;   // one millisecond of range
constexpr long long kWeekMs = 604800000, kHalfMs = kWeekMs / 2;

__device__ const double kUra[15] = {2.4, 3.4, 4.85, 6.85, 9.65, 13.65, 24.0, 48.0, 96.0, 192.0, 384.0, 768.0, 1536.0, 3072.0, 6144.0};
__device__ const double kIonDefault[8] = {0.1118E-07, -0.7451E-08, -0.5961E-07, 0.1192E-06, 0.1167E+06, -0.2294E+06, -0.1311E+06, 0.1049E+07};

struct GTime { long long time; double sec; };

__device__ __forceinline__ bool finite(double v) { return __builtin_fabs(v) <= 1.7976931348623157e308; }   // (a NaN fails it)
__device__ __forceinline__ long long fold(long long d) { return ((d + kHalfMs) % kWeekMs + kWeekMs) % kWeekMs - kHalfMs; }
__device__ __forceinline__ double time_diff(GTime a, GTime b) { return (double)(a.time - b.time) + a.sec - b.sec; }
__device__ __forceinline__ GTime time_add(GTime t, double sec)   // no carry into t.time, as the host's
{
  t.sec += sec;
  const double whole = floor(t.sec);
  t.sec += whole;
  t.sec -= whole;
  return t;
}
__device__ __forceinline__ double clock_poly(const gpsx_weph_t &e, double t) { return e.f0 + e.f1 * t + e.f2 * t * t; }
__device__ __forceinline__ double sat_clock_bias(const gpsx_weph_t &e, GTime when)
{
  double t = time_diff(when, GTime{e.toc_time, e.toc_sec});
  t -= clock_poly(e, t);
  t -= clock_poly(e, t);
  return clock_poly(e, t);
}

// ecef2pos as the host has it (what it does at the origin included), its fixed point bounded
__device__ __forceinline__ void geodetic(double x, double y, double zr, double &lat, double &lon, double &hgt)
{
  const double e2 = kFe * (2.0 - kFe), r2 = x * x + y * y;
  double v = kRe, z = zr, zk = 0.0;
  for (int it = 0; __builtin_fabs(z - zk) >= 1E-4 && it < 30; it++) {
    zk = z;
    const double sp = z / sqrt(r2 + z * z);
    v = kRe / sqrt(1.0 - e2 * sp * sp);
    z = zr + v * e2 * sp;
  }
  lat = r2 > 1E-12 ? atan(z / sqrt(r2)) : (zr > 0.0 ? kPi / 2.0 : -kPi / 2.0);
  lon = r2 > 1E-12 ? atan2(y, x) : 0.0;
  hgt = sqrt(r2 + z * z) - v;
}

__device__ __forceinline__ double klobuchar(double tow, const double *ion, double lat, double lon, double hgt, double az, double el)
{
  if (hgt < -1E3 || el <= 0)
    return 0.0;
  const double psi = 0.0137 / (el / kPi + 0.11) - 0.022;
  double phi = lat / kPi + psi * cos(az);
  phi = phi > 0.416 ? 0.416 : (phi < -0.416 ? -0.416 : phi);
  const double lam = lon / kPi + psi * sin(az) / cos(phi * kPi);
  phi += 0.064 * cos((lam - 1.617) * kPi);
  double tt = 43200.0 * lam + tow;
  tt -= floor(tt / 86400.0) * 86400.0;
  const double slant = 1.0 + 16.0 * pow(0.53 - el / kPi, 3.0);
  double amp = ion[0] + phi * (ion[1] + phi * (ion[2] + phi * ion[3]));
  double per = ion[4] + phi * (ion[5] + phi * (ion[6] + phi * ion[7]));
  amp = amp < 0.0 ? 0.0 : amp;
  per = per < 72000.0 ? 72000.0 : per;
  const double x = 2.0 * kPi * (tt - 50400.0) / per;
  return kC * slant * (__builtin_fabs(x) < 1.57 ? 5E-9 + amp * (1.0 + x * x * (-0.5 + x * x / 24.0)) : 5E-9);
}

__device__ __forceinline__ double saastamoinen(double lat, double h, double el, double humidity)
{
  if (h < -100.0 || 1E4 < h || el <= 0)
    return 0.0;
  const double hgt = h < 0.0 ? 0.0 : h;
  const double pres = 1013.25 * pow(1.0 - 2.2557E-5 * hgt, 5.2568);
  const double temp = 15.0 - 6.5E-3 * hgt + 273.16;
  const double e = 6.108 * humidity * exp((17.15 * temp - 4684.0) / (temp - 38.45));
  const double z = kPi / 2.0 - el;
  const double dry = 0.0022768 * pres / (1.0 - 0.00266 * cos(2.0 * lat) - 0.00028 * hgt / 1E3) / cos(z);
  const double wet = 0.002277 * (1255.0 / temp + 0.05) * e / cos(z);
  return dry + wet;
}

// the sum over a group's w lanes, in every one of them (the same bits in each: an addition commutes)
__device__ __forceinline__ double group_sum(double v, int w)
{
  for (int m = 1; m < w; m <<= 1)   // (w is the launch's: wave-uniform)
    v += __shfl_xor(v, m);
  return v;
}

}  // namespace

__global__ __launch_bounds__(256) void k_wfde(gpsx_wfde_cfg_t fc, const gpsx_wobs_t *obs, const gpsx_weph_t *eph, const gpsx_wlock_t *lock,
                                              const gpsx_wfix_t *prev, int n_rx, int w, int log2w, gpsx_wfix_t *fix, gpsx_wfde_t *fde,
                                              double *pr_out)
{
  const gpsx_wfix_cfg_t &cfg = fc.fix;
  const int lane = (int)(threadIdx.x & 63u);
  const long long g = (long long)blockIdx.x * 256 + (long long)threadIdx.x;
  const int j = (int)(g & (long long)(w - 1));
  const long long r = g >> log2w;
  const int base = lane & ~(w - 1);
  const bool in_rx = r < (long long)n_rx;
  const bool slot = in_rx && j < cfg.ch_per_rx;
  const size_t at = slot ? (size_t)r * (size_t)cfg.ch_per_rx + (size_t)j : 0;
  const u64 group_bits = (w == 64 ? ~0ull : ((1ull << w) - 1ull));

  // ---- the lane's observable, the sets U, A and C; the receiver's start point (read before anything is written: prev may be fix) ----
  gpsx_wobs_t o = {};
  bool usable = false;
  if (slot) {
    o = obs[at];
    usable = (o.flags & GPSX_WOBS_VALID) != 0 && (eph[at].flags & GPSX_WEPH_VALID) != 0;
    if (lock)
      usable = usable && (lock[at].flags & GPSX_WLOCK_CODE) != 0;
  }
  const bool ambig = usable && (o.flags & GPSX_WOBS_AMBIGUOUS) != 0;
  const int n_u = __popcll((__ballot(usable) >> base) & group_bits), n_a = __popcll((__ballot(ambig) >> base) & group_bits);
  const bool do_repair = in_rx && fc.repair != 0 && n_a > 0 && n_u - n_a >= cfg.min_sats;
  u32 modifiers = in_rx && n_a > 0 && !do_repair ? GPSX_WFDE_UNRESOLVED : 0u;
  double sx0 = 0.0, sx1 = 0.0, sx2 = 0.0;   // the next round's start
  if (in_rx && prev) {
    const gpsx_wfix_t *p = prev + r;
    if (p->flags & GPSX_WFIX_FIX) {
      sx0 = p->rr[0];
      sx1 = p->rr[1];
      sx2 = p->rr[2];
    }
  }
  double ion_sq = 0.0;
#pragma unroll
  for (int i = 0; i < 8; i++)
    ion_sq += cfg.ion[i] * cfg.ion[i];
  double ion[8];
#pragma unroll
  for (int i = 0; i < 8; i++)
    ion[i] = ion_sq <= 0.0 ? kIonDefault[i] : cfg.ion[i];

  // ---- what the rounds carry: the lane's millisecond correction and exclusion, the group's verdict, its last round's record ----
  int kj = 0;
  bool excl = false, done = !in_rx;
  int n_stat = 0, n_rounds = 0, dof = 0;
  u32 verdict = GPSX_WFDE_NOFIX;
  double t_stat = 0.0, t_limit = 0.0;
  u32 flags = 0;
  int n_used = 0, n_iter = 0, ref = -1, week = 0;
  u64 used_mask = 0;
  double x0 = 0.0, x1 = 0.0, x2 = 0.0, x3 = 0.0, rx_tow = 0.0, pr = 0.0;
  double q00 = 0.0, q11 = 0.0, q22 = 0.0, q01 = 0.0, q12 = 0.0, q02 = 0.0, rms = 0.0, lat_out = 0.0, lon_out = 0.0, hgt_out = 0.0;

#pragma unroll 1
  for (int round = 0; round < fc.max_excl + 2; round++) {
    if (__ballot(!done) == 0ull)   // (wave-uniform)
      break;
    const bool repairing = !done && do_repair && round == 0;
    const bool probe = repairing && ambig;                      // rides along: a row at every x, in no sum
    const bool act = !done && usable && !excl && !probe;        // the round's active set
    const bool live = act || probe;
    const long long tx = o.tx_ms + (long long)kj;
    gpsx_weph_t e = {};
    if (live)
      e = eph[at];

    // ---- gpsx_wobs_pseudoranges over the active slots: its serial scan, in every lane of the group ----
    int ref_r = -1, count = 0, week_r = 0;
    long long ref_tx = 0;
    float ref_ph = 0.0f;
#pragma unroll 1
    for (int k = 0; k < w; k++) {
      const int src = base + k;
      const long long tx_k = __shfl(tx, src);
      const float ph_k = __shfl(o.code_phase_fine, src);
      const int us_k = __shfl((int)act, src), week_k = __shfl(e.week, src);
      if (us_k) {
        count++;
        if (ref_r < 0 || (double)fold(tx_k - ref_tx) - ((double)ph_k - (double)ref_ph) / 16368.0 > 0.0) {
          ref_r = k;
          ref_tx = tx_k;
          ref_ph = ph_k;
          week_r = week_k;
        }
      }
    }
    double pr_r = 0.0, rx_tow_r = 0.0;
    if (ref_r >= 0) {
      if (live)
        pr_r = 299792458e-3 * ((double)fold(ref_tx - tx) + ((double)o.code_phase_fine - (double)ref_ph) / 16368.0 + cfg.offset_ms);
      const double rx = ((double)ref_tx - (double)ref_ph / 16368.0 + cfg.offset_ms) / 1000.0;
      rx_tow_r = rx >= 604800.0 ? rx - 604800.0 : (rx < 0.0 ? rx + 604800.0 : rx);
    }
    const bool time_ok = finite(rx_tow_r);
    if (!time_ok)
      rx_tow_r = 0.0;

    // ---- the observation time, the satellite at its transmit time (satposs) ----
    const int whole = (int)rx_tow_r;
    const GTime t_obs = {315964800ll + 604800ll * (long long)week_r + (long long)whole, rx_tow_r - (double)whole};
    const double tow = (double)((t_obs.time - 315964800ll) - (long long)(int)((t_obs.time - 315964800ll) / 604800ll) * 604800ll) + t_obs.sec;
    double px = 0.0, py = 0.0, pz = 0.0, clk = 0.0, svar = 0.0;
    bool cand = false;   // the solver has a satellite record for this slot (health and all)
    if (live && __builtin_fabs(time_diff(GTime{e.toe_time, e.toe_sec}, t_obs)) <= 7201.0) {
      GTime t = time_add(t_obs, -pr_r / kC);
      t = time_add(t, -sat_clock_bias(e, t));
      if (e.A <= 0.0) {
        cand = true;
        clk = sat_clock_bias(e, t);   // (clk == 0: "no precise clock")
      } else {
        double tk = time_diff(t, GTime{e.toe_time, e.toe_sec});
        const double mean = e.M0 + (sqrt(kMu / (e.A * e.A * e.A)) + e.deln) * tk;
        double ecc = mean, was = 0.0;
        int n = 0;
        for (; __builtin_fabs(ecc - was) > 1E-14 && n < 30; n++) {
          was = ecc;
          ecc -= (ecc - e.e * sin(ecc) - mean) / (1.0 - e.e * cos(ecc));
        }
        if (n < 30) {
          const double se = sin(ecc), ce = cos(ecc);
          double u = atan2(sqrt(1.0 - e.e * e.e) * se, ce - e.e) + e.omg;
          double rad = e.A * (1.0 - e.e * ce);
          double inc = e.i0 + e.idot * tk;
          const double s2 = sin(2.0 * u), c2 = cos(2.0 * u);
          u += e.cus * s2 + e.cuc * c2;
          rad += e.crs * s2 + e.crc * c2;
          inc += e.cis * s2 + e.cic * c2;
          const double xo = rad * cos(u), yo = rad * sin(u), ci = cos(inc);
          const double node = e.OMG0 + (e.OMGd - kOmegaE) * tk - kOmegaE * e.toes;
          const double sn = sin(node), cn = cos(node);
          px = xo * cn - yo * ci * sn;
          py = xo * sn + yo * ci * cn;
          pz = yo * sin(inc);
          tk = time_diff(t, GTime{e.toc_time, e.toc_sec});
          clk = clock_poly(e, tk) - 2.0 * sqrt(kMu * e.A) * e.e * se / (kC * kC);
          const double ura = (e.sva < 0 || e.sva > 14) ? 6144.0 : kUra[e.sva];
          svar = ura * ura;
          cand = true;
          if (clk == 0.0)
            clk = sat_clock_bias(e, t);
        }
      }
    }
    const bool healthy = e.svh == 0;
    const double tgd = kC * e.tgd;
    const double rn = sqrt(px * px + py * py + pz * pz);

    // ---- the round's record starts; estpos / rescode ----
    int mode = 0;   // 0: iterating, 1: converged, the residuals at the final x are due, 2: finished
    if (done)
      mode = 2;
    else {
      flags = 0;
      n_used = 0;
      n_iter = 0;
      used_mask = 0;
      q00 = q11 = q22 = q01 = q12 = q02 = rms = lat_out = lon_out = hgt_out = 0.0;
      x0 = sx0;
      x1 = sx1;
      x2 = sx2;
      x3 = 0.0;
      ref = ref_r;
      week = week_r;
      rx_tow = rx_tow_r;
      pr = act ? pr_r : 0.0;
      if (!time_ok) {
        flags = GPSX_WFIX_NONFINITE;
        mode = 2;
      } else if (count < cfg.min_sats) {
        flags = GPSX_WFIX_TOO_FEW;
        mode = 2;
      }
    }
    // the residual pass's yield: the lane's residual and w^2, the group's T, counted rows and whether a slot can be named
    double v_fin = 0.0, w2 = 0.0, t_sum = 0.0;
    bool row_fin = false, name_ok = false;
    int n_cnt = 0;

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
        double az = 0.0, el = kPi / 2.0;
        if (hgt > -kRe) {
          const double sp = sin(lat), cp = cos(lat), sl = sin(lon), cl = cos(lon);
          const double east = -sl * l0 + cl * l1;
          const double north = -sp * cl * l0 - sp * sl * l1 + cp * l2;
          const double up = cp * cl * l0 + cp * sl * l1 + sp * l2;
          az = east * east + north * north < 1E-12 ? 0.0 : atan2(east, north);
          if (az < 0.0)
            az += 2 * kPi;
          el = asin(up);
        }
        row = row && !(el < 0.0) && healthy;
        if (row) {
          const double dion = klobuchar(tow, ion, lat, lon, hgt, az, el);
          const double dtrp = saastamoinen(lat, hgt, el, 0.7);
          const double v_ion = (dion * 0.5) * (dion * 0.5);
          const double sin_el = sin(el);
          const double v_trp = (0.3 / (sin_el + 0.1)) * (0.3 / (sin_el + 0.1));
          const double ev = 0.003 * 0.003;
          const double v_meas = ev * (ev + ev / sin_el);
          v = (pr_r - tgd) - (rho + dion + dtrp + x3 - kC * clk);
          const double sig = sqrt(v_meas + svar + v_ion + v_trp);
          a0 = -l0 / sig;
          a1 = -l1 / sig;
          a2 = -l2 / sig;
          a3 = 1.0 / sig;
          y = v / sig;
        }
      }
      const u64 rows = (__ballot(row && act) >> base) & group_bits;
      // what enters the sums: the active rows; in the residual pass those of used_mask, "the rows counted"
      const bool counted = row && act && (mode != 1 || ((used_mask >> j) & 1ull) != 0);
      if (!counted) {
        a0 = 0.0;
        a1 = 0.0;
        a2 = 0.0;
        a3 = 0.0;
        y = 0.0;
      }
      const double vv = counted ? v : 0.0;
      const double n00 = group_sum(a0 * a0, w), n10 = group_sum(a1 * a0, w), n11 = group_sum(a1 * a1, w), n20 = group_sum(a2 * a0, w),
                   n21 = group_sum(a2 * a1, w), n22 = group_sum(a2 * a2, w), n30 = group_sum(a3 * a0, w), n31 = group_sum(a3 * a1, w),
                   n32 = group_sum(a3 * a2, w), n33 = group_sum(a3 * a3, w), b0 = group_sum(a0 * y, w), b1 = group_sum(a1 * y, w),
                   b2 = group_sum(a2 * y, w), b3 = group_sum(a3 * y, w), ss = group_sum(vv * vv, w), tt = group_sum(y * y, w);

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
      const bool pivots_ok = p0 > 0.0 && p1 > kPivot * n11 && p2 > kPivot * n22 && p3 > kPivot * n33;

      if (mode == 1) {   // the residuals at the final x; the test's T and every counted slot's w^2 = y^2 / (1 - |M a|^2)
        rms = sqrt(ss / (double)n_used);
        lat_out = lat;
        lon_out = lon;
        hgt_out = hgt;
        flags = GPSX_WFIX_FIX;
        mode = 2;
        v_fin = v;
        row_fin = row;
        t_sum = tt;
        n_cnt = __popcll(rows & used_mask);
        name_ok = sums_ok && pivots_ok;
        const double h0 = m00 * a0, h1 = m10 * a0 + m11 * a1, h2 = m20 * a0 + m21 * a1 + m22 * a2, h3 = m30 * a0 + m31 * a1 + m32 * a2 + m33 * a3;
        const double rest = 1.0 - (h0 * h0 + h1 * h1 + h2 * h2 + h3 * h3);
        w2 = counted && rest > 1E-10 ? y * y / rest : 0.0;
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
        } else if (!pivots_ok) {
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

    // ---- the round's record is complete: gpsx_wfix's rule for a result that is not finite ----
    if (!done && flags == GPSX_WFIX_FIX) {
      const float f0 = (float)q00, f1 = (float)q11, f2 = (float)q22, f3 = (float)q01, f4 = (float)q12, f5 = (float)q02;
      if (!(finite(x0) && finite(x1) && finite(x2) && finite(x3 / kC) && finite(lat_out) && finite(lon_out) && finite(hgt_out) && finite(rms) &&
            finite((double)f0) && finite((double)f1) && finite((double)f2) && finite((double)f3) && finite((double)f4) && finite((double)f5)))
        flags = GPSX_WFIX_NONFINITE;
    }
    const bool fixed = !done && flags == GPSX_WFIX_FIX;

    // ---- the slot to name: the largest w^2 > 0 of the group, the lowest slot among equals (every lane of the wave takes part) ----
    double best = fixed && !repairing && finite(w2) && w2 > 0.0 ? w2 : 0.0;
    int best_j = j;
    for (int m = 1; m < w; m <<= 1) {   // (w is the launch's: wave-uniform)
      const double other = __shfl_xor(best, m);
      const int other_j = __shfl_xor(best_j, m);
      if (other > best || (other == best && other_j < best_j)) {
        best = other;
        best_j = other_j;
      }
    }

    // ---- the round's decision, the same in every lane of the group ----
    if (!done) {
      n_rounds++;
      if (repairing) {
        if (!fixed)
          modifiers |= GPSX_WFDE_UNRESOLVED;
        else if (probe && row_fin) {
          const double kd = rint(v_fin / kMsM);
          if (!finite(v_fin) || __builtin_fabs(kd) > 1.0)
            excl = true;
          else
            kj = (int)kd;
        }
      } else if (!fixed) {
        verdict = GPSX_WFDE_NOFIX;
        dof = 0;
        t_stat = 0.0;
        t_limit = 0.0;
        done = true;
      } else {
        dof = n_cnt - 4;
        if (dof < 1) {
          verdict = GPSX_WFDE_UNCHECKED;
          t_stat = 0.0;
          t_limit = 0.0;
          done = true;
        } else {
          const double dd = (double)dof;
          const double t = 1.0 - 2.0 / (9.0 * dd) + fc.z_global * sqrt(2.0 / (9.0 * dd));
          t_limit = dd * t * t * t;
          t_stat = finite(t_sum) ? t_sum : 0.0;
          if (finite(t_sum) && t_sum <= t_limit) {
            verdict = GPSX_WFDE_PASSED;
            done = true;
          } else if (n_stat == fc.max_excl || n_cnt - 1 < cfg.min_sats || !name_ok || !(best > 0.0)) {
            verdict = GPSX_WFDE_FAULT;
            done = true;
          } else {
            if (j == best_j)
              excl = true;
            n_stat++;
          }
        }
      }
      sx0 = fixed ? x0 : 0.0;
      sx1 = fixed ? x1 : 0.0;
      sx2 = fixed ? x2 : 0.0;
    }
  }

  // ---- the masks; the receiver's two records, by the group's first lane; every slot's pseudorange ----
  const u64 excl_mask = (__ballot(excl) >> base) & group_bits, plus_mask = (__ballot(kj == 1) >> base) & group_bits,
            minus_mask = (__ballot(kj == -1) >> base) & group_bits;
  if (slot && pr_out)
    pr_out[at] = finite(pr) ? pr : 0.0;
  if (in_rx && j == 0) {
    gpsx_wfix_t out = {};
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
      out.dtr_s = x3 / kC;
      out.geo[0] = lat_out;
      out.geo[1] = lon_out;
      out.geo[2] = hgt_out;
      out.qr[0] = (float)q00;
      out.qr[1] = (float)q11;
      out.qr[2] = (float)q22;
      out.qr[3] = (float)q01;
      out.qr[4] = (float)q12;
      out.qr[5] = (float)q02;
      out.resid_rms_m = rms;
    }
    fix[r] = out;
    gpsx_wfde_t rec = {};
    rec.flags = verdict | modifiers | (excl_mask != 0 ? GPSX_WFDE_EXCLUDED : 0u) | ((plus_mask | minus_mask) != 0 ? GPSX_WFDE_REPAIRED : 0u);
    rec.n_rounds = n_rounds;
    rec.n_excluded = __popcll(excl_mask);
    rec.dof = dof;
    rec.excl_mask = excl_mask;
    rec.plus_mask = plus_mask;
    rec.minus_mask = minus_mask;
    rec.t_stat = t_stat;
    rec.t_limit = t_limit;
    fde[r] = rec;
  }
}

void launch_wfde(hipStream_t s, const gpsx_wfde_cfg_t &cfg, const gpsx_wobs_t *d_obs, const gpsx_weph_t *d_eph, const gpsx_wlock_t *d_lock,
                 const gpsx_wfix_t *d_prev, int n_rx, gpsx_wfix_t *d_fix, gpsx_wfde_t *d_fde, double *d_pr_m)
{
  if (n_rx < 1 || n_rx > (1 << 20) || cfg.fix.ch_per_rx < 1 || cfg.fix.ch_per_rx > 64 || cfg.max_excl < 0 || cfg.max_excl > 8)
    return;
  int w = 1, log2w = 0;
  while (w < cfg.fix.ch_per_rx) {
    w <<= 1;
    log2w++;
  }
  const unsigned long long lanes = (unsigned long long)n_rx << log2w;   // at most 2^26
  hipLaunchKernelGGL(k_wfde, dim3((unsigned)((lanes + 255ull) / 256ull)), dim3(256), 0, s, cfg, d_obs, d_eph, d_lock, d_prev, n_rx, w, log2w, d_fix,
                     d_fde, d_pr_m);
}

}  // namespace gpsx
