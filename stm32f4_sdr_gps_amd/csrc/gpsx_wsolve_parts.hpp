// gpsx_wsolve_parts.hpp -- what the solver kernels at the weighted chain's end share, one slot per lane and a receiver a group of W
// lanes in all four: k_wfix and k_wfde (position), k_wvel (velocity), k_wkf (the filter).  Here: the constants and tables, the time
// arithmetic, the models (geodetic, Klobuchar, Saastamoinen), the lane and launch geometry, Kepler's equation and the two satellite
// evaluations on it, the pseudorange row's model terms, the 4 x 4 normal system's sums and its factorisation, the gpsx_wfix_t
// record's fill, the ENU rotation; the layout of the records all four read, once.  A kernel keeps the asserts on its own cfg, state
// and output structs, its loops under #pragma unroll 1, every ballot and every shuffle but those of group_sum below -- so that a
// kernel file with group_sum reads as one argument on wave-uniform control flow -- its rows' residuals, its flags and what it does
// with a result.  k_wkf's tri and spd_inverse have one user and are k_wkf.hip's.
//
// Not every kernel takes every part: a part whose sharing moved a kernel's time out of the parent's own spread is that kernel's own
// text again (measured, EXPERIMENTS.md "One parts header for the solver kernels").  The reference-slot scan is in k_wfix.hip and
// k_wfde.hip (shared, it cost k_wfde 1 % at 64 slots); the sums, the solve and the record's fill are k_wfde's from here and
// k_wfix.hip's own (0.4 us at 64 slots); k_wvel takes the small helpers and the geometry only and stays instruction for instruction
// what it was, so the satellite at its clock's reading is here for k_wkf and in k_wvel.hip.
//
// Every part is __device__ __forceinline__, its arithmetic operation for operation what the four files had, nothing indexed by a
// run-time value but the two tables.  -ffp-contract=off -fno-fast-math: the same operations in the same order are the same bits
// whatever registers hold them (profiles/r26_wsolve_parts_isa.txt, profiles/r26_wsolve_parts_bytes.txt).
#pragma once
#include <cstddef>
#include "gpsx_device.hpp"
namespace gpsx {
namespace wsolve {

static_assert(sizeof(gpsx_wobs_t) == 32 && sizeof(gpsx_weph_t) == 256 && sizeof(gpsx_wlock_t) == 64 && sizeof(gpsx_wvel_t) == 112,
              "the records the solvers read");
static_assert(sizeof(gpsx_wfix_t) == 128 && offsetof(gpsx_wfix_t, n_used) == 4 && offsetof(gpsx_wfix_t, n_iter) == 8 &&
              offsetof(gpsx_wfix_t, ref_slot) == 12 && offsetof(gpsx_wfix_t, used_mask) == 16 && offsetof(gpsx_wfix_t, rr) == 24 &&
              offsetof(gpsx_wfix_t, dtr_s) == 48 && offsetof(gpsx_wfix_t, rx_tow_s) == 56 && offsetof(gpsx_wfix_t, geo) == 64 &&
              offsetof(gpsx_wfix_t, qr) == 88 && offsetof(gpsx_wfix_t, resid_rms_m) == 112 && offsetof(gpsx_wfix_t, week) == 120 &&
              offsetof(gpsx_wfix_t, reserved) == 124, "gpsx_wfix_t layout");

constexpr double kC = 299792458.0;
constexpr double kMs = 299792.458;   // c per millisecond
constexpr double kPi = 3.1415926535897932;
constexpr double kMu = 3.9860050E14;
constexpr double kOmegaE = 7.2921151467E-5;
constexpr double kRe = 6378137.0;
constexpr double kFe = 1.0 / 298.257223563;
constexpr int kMaxIter = 10;
constexpr double kPivot = 1E-10;   // a pivot at or below this share of its diagonal element is round-off: SINGULAR
constexpr double kHalfWeek = 302400.0, kWeek = 604800.0;
constexpr long long kWeekMs = 604800000, kHalfMs = kWeekMs / 2;

static __device__ const double kUra[15] = {2.4, 3.4, 4.85, 6.85, 9.65, 13.65, 24.0, 48.0, 96.0, 192.0, 384.0, 768.0, 1536.0, 3072.0, 6144.0};
static __device__ const double kIonDefault[8] = {0.1118E-07, -0.7451E-08, -0.5961E-07, 0.1192E-06, 0.1167E+06, -0.2294E+06, -0.1311E+06, 0.1049E+07};

struct GTime { long long time; double sec; };

__device__ __forceinline__ bool finite(double v) { return __builtin_fabs(v) <= 1.7976931348623157e308; }   // (a NaN fails it)
__device__ __forceinline__ long long fold_ms(long long d) { return ((d + kHalfMs) % kWeekMs + kWeekMs) % kWeekMs - kHalfMs; }
__device__ __forceinline__ double fold_s(double d) { return d > kHalfWeek ? d - kWeek : (d < -kHalfWeek ? d + kWeek : d); }
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

// ---- the geometry: one slot per lane, a receiver a group of w = 2^log2w lanes, 256 lanes a workgroup ---------------------------------
// j: the lane's slot of its receiver r; base: the group's first lane in the wave; at: the slot's record (0 where there is none)
struct Lane {
  int j, base;
  long long r;
  bool in_rx, slot;
  size_t at;
  u64 group_bits;
};
__device__ __forceinline__ u64 group_mask(int w) { return w == 64 ? ~0ull : ((1ull << w) - 1ull); }   // (a group's lanes, shifted to bit 0)
__device__ __forceinline__ Lane lane_of(int w, int log2w, int n_rx, int ch_per_rx)
{
  Lane l;
  const int lane = (int)(threadIdx.x & 63u);
  const long long g = (long long)blockIdx.x * 256 + (long long)threadIdx.x;
  l.j = (int)(g & (long long)(w - 1));
  l.r = g >> log2w;
  l.base = lane & ~(w - 1);
  l.in_rx = l.r < (long long)n_rx;
  l.slot = l.in_rx && l.j < ch_per_rx;
  l.at = l.slot ? (size_t)l.r * (size_t)ch_per_rx + (size_t)l.j : 0;
  l.group_bits = (w == 64 ? ~0ull : ((1ull << w) - 1ull));
  return l;
}
// the launch's: w the smallest power of two >= ch_per_rx (1..64), the grid for n_rx (1..2^20) groups
struct Geometry {
  int w, log2w;
  unsigned grid;
};
inline Geometry geometry_of(int n_rx, int ch_per_rx)
{
  Geometry g = {1, 0, 0};
  while (g.w < ch_per_rx) {
    g.w <<= 1;
    g.log2w++;
  }
  const unsigned long long lanes = (unsigned long long)n_rx << g.log2w;   // at most 2^26
  g.grid = (unsigned)((lanes + 255ull) / 256ull);
  return g;
}

// the Klobuchar coefficients of a launch: cfg's, the default table where cfg's are all zero
__device__ __forceinline__ void choose_ion(const double (&cfg_ion)[8], double (&ion)[8])
{
  double ion_sq = 0.0;
#pragma unroll
  for (int i = 0; i < 8; i++)
    ion_sq += cfg_ion[i] * cfg_ion[i];
#pragma unroll
  for (int i = 0; i < 8; i++)
    ion[i] = ion_sq <= 0.0 ? kIonDefault[i] : cfg_ion[i];
}

// ---- the satellite ----------------------------------------------------------------------------------------------------------------
// Kepler's equation from the mean anomaly, 30 steps at most as on the host; false: not converged
__device__ __forceinline__ bool kepler(double mean, double e, double &ecc)
{
  ecc = mean;
  double was = 0.0;
  int n = 0;
  for (; __builtin_fabs(ecc - was) > 1E-14 && n < 30; n++) {
    was = ecc;
    ecc -= (ecc - e * sin(ecc) - mean) / (1.0 - e * cos(ecc));
  }
  return n < 30;
}

// the observation time of a receiver time of week, and its time of week as satposs counts it
__device__ __forceinline__ GTime obs_time(int week, double rx_tow)
{
  const int whole = (int)rx_tow;
  return GTime{315964800ll + 604800ll * (long long)week + (long long)whole, rx_tow - (double)whole};
}
__device__ __forceinline__ double tow_of(GTime t)
{
  return (double)((t.time - 315964800ll) - (long long)(int)((t.time - 315964800ll) / 604800ll) * 604800ll) + t.sec;
}

// satposs for one slot: position, clock and variance at the transmit time of pseudorange pr observed at t_obs (k_wfix, k_wfde).
// -> the solver has a satellite record for this slot (health and all); the outputs are written only then, and only where set
__device__ __forceinline__ bool sat_at_transmit(const gpsx_weph_t &e, GTime t_obs, double pr, double &px, double &py, double &pz, double &clk,
                                                double &svar)
{
  bool cand = false;
  if (__builtin_fabs(time_diff(GTime{e.toe_time, e.toe_sec}, t_obs)) <= 7201.0) {
    GTime t = time_add(t_obs, -pr / kC);
    t = time_add(t, -sat_clock_bias(e, t));
    if (e.A <= 0.0) {
      cand = true;
      clk = sat_clock_bias(e, t);   // (clk == 0: "no precise clock")
    } else {
      double tk = time_diff(t, GTime{e.toe_time, e.toe_sec});
      const double mean = e.M0 + (sqrt(kMu / (e.A * e.A * e.A)) + e.deln) * tk;
      double ecc;
      if (kepler(mean, e.e, ecc)) {
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
  return cand;
}

// the satellite at the transmit time t_sv its own clock reads (k_wvel, k_wkf): position, analytic velocity, clock offset and rate,
// variance.  -> there is one; the outputs are written only then
struct SatState {
  double px, py, pz, vx, vy, vz, rate, clk, svar;
};
__device__ __forceinline__ bool sat_at_clock(const gpsx_weph_t &e, double t_sv, SatState &s)
{
  const double toc = (double)(((e.toc_time - 315964800ll) % 604800ll + 604800ll) % 604800ll) + e.toc_sec;
  double tc = fold_s(t_sv - toc);
  tc -= clock_poly(e, tc);
  tc -= clock_poly(e, tc);
  const double t = t_sv - clock_poly(e, tc);
  const double tk = fold_s(t - e.toes);
  if (__builtin_fabs(tk) <= 7201.0 && e.A > 0.0) {
    const double n0 = sqrt(kMu / (e.A * e.A * e.A)) + e.deln;
    const double mean = e.M0 + n0 * tk;
    double ecc;
    if (kepler(mean, e.e, ecc)) {
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
      s.px = xo * cn - yo * ci * sn;
      s.py = xo * sn + yo * ci * cn;
      s.pz = yo * si;
      s.vx = xd * cn - yd * ci * sn + yo * id * si * sn - od * s.py;
      s.vy = xd * sn + yd * ci * cn - yo * id * si * cn + od * s.px;
      s.vz = yd * si + yo * id * ci;
      const double tcl = fold_s(t - toc);
      s.rate = e.f1 + 2.0 * e.f2 * tcl - 2.0 * sqrt(kMu * e.A) * e.e * ce * ed / (kC * kC);
      s.clk = clock_poly(e, tcl) - 2.0 * sqrt(kMu * e.A) * e.e * se / (kC * kC);
      const double ura = (e.sva < 0 || e.sva > 14) ? 6144.0 : kUra[e.sva];
      s.svar = ura * ura;
      return true;
    }
  }
  return false;
}

// ---- the rows -----------------------------------------------------------------------------------------------------------------------
// a vector in the east / north / up frame at (lat, lon)
__device__ __forceinline__ void to_enu(double lat, double lon, double v0, double v1, double v2, double &east, double &north, double &up)
{
  const double sp = sin(lat), cp = cos(lat), sl = sin(lon), cl = cos(lon);
  east = -sl * v0 + cl * v1;
  north = -sp * cl * v0 - sp * sl * v1 + cp * v2;
  up = cp * cl * v0 + cp * sl * v1 + sp * v2;
}

// azimuth and elevation of the unit line of sight l at (lat, lon, hgt); below the Earth's centre: the zenith
__device__ __forceinline__ void az_el(double l0, double l1, double l2, double lat, double lon, double hgt, double &az, double &el)
{
  az = 0.0;
  el = kPi / 2.0;
  if (hgt > -kRe) {
    double east, north, up;
    to_enu(lat, lon, l0, l1, l2, east, north, up);
    az = east * east + north * north < 1E-12 ? 0.0 : atan2(east, north);
    if (az < 0.0)
      az += 2 * kPi;
    el = asin(up);
  }
}

// the pseudorange row's model: the two delays; -> the variance of measurement, ephemeris (svar), ionosphere and troposphere
__device__ __forceinline__ double pr_model(double tow, const double *ion, double lat, double lon, double hgt, double az, double el, double svar,
                                           double &dion, double &dtrp)
{
  dion = klobuchar(tow, ion, lat, lon, hgt, az, el);
  dtrp = saastamoinen(lat, hgt, el, 0.7);
  const double v_ion = (dion * 0.5) * (dion * 0.5);
  const double sin_el = sin(el);
  const double v_trp = (0.3 / (sin_el + 0.1)) * (0.3 / (sin_el + 0.1));
  const double ev = 0.003 * 0.003;
  const double v_meas = ev * (ev + ev / sin_el);
  return v_meas + svar + v_ion + v_trp;
}

// ---- the symmetric 4 x 4 normal system of a group: N = sum a a^T, b = sum a y over its lanes (a lane without a row passes zeros) --------
struct Normal {
  double n00, n10, n11, n20, n21, n22, n30, n31, n32, n33, b0, b1, b2, b3;
};
__device__ __forceinline__ Normal normal_sums(double a0, double a1, double a2, double a3, double y, int w)
{
  Normal s;
  s.n00 = group_sum(a0 * a0, w);
  s.n10 = group_sum(a1 * a0, w);
  s.n11 = group_sum(a1 * a1, w);
  s.n20 = group_sum(a2 * a0, w);
  s.n21 = group_sum(a2 * a1, w);
  s.n22 = group_sum(a2 * a2, w);
  s.n30 = group_sum(a3 * a0, w);
  s.n31 = group_sum(a3 * a1, w);
  s.n32 = group_sum(a3 * a2, w);
  s.n33 = group_sum(a3 * a3, w);
  s.b0 = group_sum(a0 * y, w);
  s.b1 = group_sum(a1 * y, w);
  s.b2 = group_sum(a2 * y, w);
  s.b3 = group_sum(a3 * y, w);
  return s;
}
__device__ __forceinline__ bool sums_ok(const Normal &s)
{
  return finite(s.n00) && finite(s.n10) && finite(s.n11) && finite(s.n20) && finite(s.n21) && finite(s.n22) && finite(s.n30) && finite(s.n31) &&
         finite(s.n32) && finite(s.n33) && finite(s.b0) && finite(s.b1) && finite(s.b2) && finite(s.b3);
}

// Cholesky N = L L^T (pivots p), M = L^-1, the solution d = M^T M b; computed by every lane whatever the sums are, judged by
// sums_ok and pivots_ok
struct Solve {
  double p0, p1, p2, p3, m00, m10, m11, m20, m21, m22, m30, m31, m32, m33, d0, d1, d2, d3;
};
__device__ __forceinline__ Solve solve(const Normal &s)
{
  Solve r;
  const double l00 = sqrt(s.n00), l10 = s.n10 / l00, l20 = s.n20 / l00, l30 = s.n30 / l00;
  r.p0 = s.n00;
  r.p1 = s.n11 - l10 * l10;
  const double l11 = sqrt(r.p1), l21 = (s.n21 - l20 * l10) / l11, l31 = (s.n31 - l30 * l10) / l11;
  r.p2 = s.n22 - l20 * l20 - l21 * l21;
  const double l22 = sqrt(r.p2), l32 = (s.n32 - l30 * l20 - l31 * l21) / l22;
  r.p3 = s.n33 - l30 * l30 - l31 * l31 - l32 * l32;
  const double l33 = sqrt(r.p3);
  r.m00 = 1.0 / l00;
  r.m11 = 1.0 / l11;
  r.m22 = 1.0 / l22;
  r.m33 = 1.0 / l33;
  r.m10 = -(l10 * r.m00) / l11;
  r.m20 = -(l20 * r.m00 + l21 * r.m10) / l22;
  r.m21 = -(l21 * r.m11) / l22;
  r.m30 = -(l30 * r.m00 + l31 * r.m10 + l32 * r.m20) / l33;
  r.m31 = -(l31 * r.m11 + l32 * r.m21) / l33;
  r.m32 = -(l32 * r.m22) / l33;
  const double y0 = r.m00 * s.b0, y1 = r.m10 * s.b0 + r.m11 * s.b1, y2 = r.m20 * s.b0 + r.m21 * s.b1 + r.m22 * s.b2,
               y3 = r.m30 * s.b0 + r.m31 * s.b1 + r.m32 * s.b2 + r.m33 * s.b3;
  r.d0 = r.m00 * y0 + r.m10 * y1 + r.m20 * y2 + r.m30 * y3;
  r.d1 = r.m11 * y1 + r.m21 * y2 + r.m31 * y3;
  r.d2 = r.m22 * y2 + r.m32 * y3;
  r.d3 = r.m33 * y3;
  return r;
}
__device__ __forceinline__ bool pivots_ok(const Normal &s, const Solve &r)
{
  return r.p0 > 0.0 && r.p1 > kPivot * s.n11 && r.p2 > kPivot * s.n22 && r.p3 > kPivot * s.n33;
}
// the first three unknowns' block of Q = M^T M: the diagonal, then (0,1), (1,2), (0,2) -- the order of the records' q arrays
struct QBlock {
  double q00, q11, q22, q01, q12, q02;
};
__device__ __forceinline__ QBlock q_block(const Solve &r)
{
  QBlock q;
  q.q00 = r.m00 * r.m00 + r.m10 * r.m10 + r.m20 * r.m20 + r.m30 * r.m30;
  q.q11 = r.m11 * r.m11 + r.m21 * r.m21 + r.m31 * r.m31;
  q.q22 = r.m22 * r.m22 + r.m32 * r.m32;
  q.q01 = r.m10 * r.m11 + r.m20 * r.m21 + r.m30 * r.m31;
  q.q12 = r.m21 * r.m22 + r.m31 * r.m32;
  q.q02 = r.m20 * r.m22 + r.m30 * r.m32;
  return q;
}

// ---- the gpsx_wfix_t record -----------------------------------------------------------------------------------------------------------
// what a fix carries; gpsx_wfix's rule: a FIX of which any of it is not finite is NONFINITE
struct FixResult {
  double x0, x1, x2, x3, lat, lon, hgt, rms;
  QBlock q;
};
__device__ __forceinline__ bool fix_finite(const FixResult &f)
{
  return finite(f.x0) && finite(f.x1) && finite(f.x2) && finite(f.x3 / kC) && finite(f.lat) && finite(f.lon) && finite(f.hgt) && finite(f.rms) &&
         finite((double)(float)f.q.q00) && finite((double)(float)f.q.q11) && finite((double)(float)f.q.q22) && finite((double)(float)f.q.q01) &&
         finite((double)(float)f.q.q12) && finite((double)(float)f.q.q02);
}
__device__ __forceinline__ gpsx_wfix_t fix_record(u32 flags, int n_used, int n_iter, int ref, u64 used_mask, double rx_tow, int week, const FixResult &f)
{
  gpsx_wfix_t out = {};
  out.flags = flags;
  out.n_used = n_used;
  out.n_iter = n_iter;
  out.ref_slot = ref;
  out.used_mask = used_mask;
  out.rx_tow_s = rx_tow;
  out.week = week;
  if (flags == GPSX_WFIX_FIX) {
    out.rr[0] = f.x0;
    out.rr[1] = f.x1;
    out.rr[2] = f.x2;
    out.dtr_s = f.x3 / kC;
    out.geo[0] = f.lat;
    out.geo[1] = f.lon;
    out.geo[2] = f.hgt;
    out.qr[0] = (float)f.q.q00;
    out.qr[1] = (float)f.q.q11;
    out.qr[2] = (float)f.q.q22;
    out.qr[3] = (float)f.q.q01;
    out.qr[4] = (float)f.q.q12;
    out.qr[5] = (float)f.q.q02;
    out.resid_rms_m = f.rms;
  }
  return out;
}

}  // namespace wsolve
}  // namespace gpsx
