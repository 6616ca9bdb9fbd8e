// k_wsnap.hip -- EXTENSION, not in the reference: snapshot fixes, the stage behind a weighted grid that turns a receiver's peak records,
// an ephemeris bank and a coarse prior into a position, a common bias and a corrected time of week: coarse-time navigation with five
// unknowns (include/gpsx.h gpsx_wsnap).
//
// k_wacq's geometry: one wave per receiver, four receivers per 256-thread workgroup; no LDS, no barrier, no scratch.  Step 1 is
// k_wacq's text: a row's bins strided over the lanes, a 64-bit key (max_val, ~bin) reduced by a butterfly, lane p keeps row p's.
// From step 2 on lane p is PRN index p, as in k_wpred: its bank record and, per pass of the solver, three passes of one FP64
// satellite evaluation (gpsx_wsolve_parts.hpp: sat_at_clock, az_el, pr_model) under #pragma unroll 1 -- that is where the time goes.
// The first pass of the solver stands at the prior, so its evaluation is step 2's: the candidates, the reference (ranked by
// elevation with a loop of shuffles, named by a ballot) and the milliseconds N_p are taken there, under `pass == 0`, and the
// evaluation's text exists once.  The twenty sums of the 5 x 5 normal system and the residuals' are group_sum's butterflies over
// the wave; the factorisation runs in every lane on constant indices.  Every ballot and shuffle runs under wave-uniform control flow:
// a wave whose receiver does not exist or has no prior leaves as a whole; `mode` and `pass` are the same in the 64 lanes (they follow
// from ballots and from sums that are the same bits in every lane); lane-dependent conditions are selects or lane-local branches
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

static_assert(sizeof(gpsx_wsnap_cfg_t) == 128 && offsetof(gpsx_wsnap_cfg_t, el_min_rad) == 64 && offsetof(gpsx_wsnap_cfg_t, epoch_offset_s) == 72 &&
              offsetof(gpsx_wsnap_cfg_t, max_resid_m) == 80 && offsetof(gpsx_wsnap_cfg_t, det_num) == 88 && offsetof(gpsx_wsnap_cfg_t, min_peak) == 96 &&
              offsetof(gpsx_wsnap_cfg_t, min_sats) == 100 && offsetof(gpsx_wsnap_cfg_t, reserved) == 104, "gpsx_wsnap_cfg_t layout");
static_assert(sizeof(gpsx_wsnap_prior_t) == 48 && offsetof(gpsx_wsnap_prior_t, week) == 4 && offsetof(gpsx_wsnap_prior_t, rr) == 8 &&
              offsetof(gpsx_wsnap_prior_t, tow_s) == 32 && offsetof(gpsx_wsnap_prior_t, reserved) == 40, "gpsx_wsnap_prior_t layout");
static_assert(sizeof(gpsx_wsnap_t) == 128 && offsetof(gpsx_wsnap_t, week) == 4 && offsetof(gpsx_wsnap_t, n_detected) == 8 &&
              offsetof(gpsx_wsnap_t, ref) == 12 && offsetof(gpsx_wsnap_t, used_mask) == 16 && offsetof(gpsx_wsnap_t, rr) == 24 &&
              offsetof(gpsx_wsnap_t, b_m) == 48 && offsetof(gpsx_wsnap_t, dt_s) == 56 && offsetof(gpsx_wsnap_t, tow_s) == 64 &&
              offsetof(gpsx_wsnap_t, geo) == 72 && offsetof(gpsx_wsnap_t, resid_rms_m) == 96 && offsetof(gpsx_wsnap_t, qr) == 104, "gpsx_wsnap_t layout");
static_assert(sizeof(gpsx_wsnap_sv_t) == 48 && offsetof(gpsx_wsnap_sv_t, n_ms) == 4 && offsetof(gpsx_wsnap_sv_t, phase) == 8 &&
              offsetof(gpsx_wsnap_sv_t, dopp_hz) == 12 && offsetof(gpsx_wsnap_sv_t, el) == 16 && offsetof(gpsx_wsnap_sv_t, resid_m) == 32 &&
              offsetof(gpsx_wsnap_sv_t, reserved) == 40, "gpsx_wsnap_sv_t layout");
static_assert(sizeof(gpsx_peak_t) == 16 && offsetof(gpsx_peak_t, max_val) == 0 && offsetof(gpsx_peak_t, phase) == 4 && offsetof(gpsx_peak_t, sum) == 8,
              "gpsx_peak_t layout");

constexpr u32 kPhases = 16368u;

struct alignas(4) Quad { u32 a, b, c, d; };   // a record at a dword-aligned address: one global_load_dwordx4

// the place of element (i, j), i >= j, of the 5 x 5 lower triangle, row by row
__device__ __forceinline__ constexpr int low(int i, int j) { return i * (i + 1) / 2 + j; }

}  // namespace

__global__ __launch_bounds__(256) void k_wsnap(gpsx_wsnap_cfg_t cfg, int n_rx, int n_prn, int n_dopp, int dopp_min_hz, int dopp_step_hz, int bank_stride,
                                               const gpsx_peak_t *__restrict__ peaks, const gpsx_weph_t *__restrict__ bank,
                                               const gpsx_wsnap_prior_t *__restrict__ prior, gpsx_wsnap_t *__restrict__ snap,
                                               gpsx_wsnap_sv_t *__restrict__ sv)
{
  const int lane = (int)threadIdx.x & 63;
  const int r = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
  if (r >= n_rx)          // (the whole wave: r is the same in its 64 lanes)
    return;
  const bool is_prn = lane < n_prn;

  // 0 the prior, the same in every lane
  const gpsx_wsnap_prior_t pri = prior[r];
  const bool have_prior = pri.flags == GPSX_WSNAP_PRIOR_HAVE && pri.reserved[0] == 0u && pri.reserved[1] == 0u && finite(pri.rr[0]) &&
                          finite(pri.rr[1]) && finite(pri.rr[2]) && finite(pri.tow_s) && pri.tow_s >= 0.0 && pri.tow_s < kWeek && pri.week >= 0 &&
                          pri.week <= 32767;
  if (!have_prior) {      // (the whole wave: the prior is one for its 64 lanes)
    if (sv && is_prn) {
      gpsx_wsnap_sv_t o = {};
      sv[(size_t)r * (size_t)n_prn + (size_t)lane] = o;
    }
    if (lane == 0) {
      gpsx_wsnap_t o = {};
      o.flags = GPSX_WSNAP_NO_PRIOR;
      snap[r] = o;
    }
    return;
  }

  // 1 the best record per PRN: lane p keeps row p's key (k_wacq's step 1)
  const gpsx_peak_t *rows = peaks + (size_t)r * (size_t)n_prn * (size_t)n_dopp;
  u64 key = 0;            // (below every record's: a key's low word is ~bin >= 2^31)
  auto wave_key = [](u64 k) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const u64 o = (u64)__shfl_xor((long long)k, m, 64);
      k = o > k ? o : k;
    }
    return k;
  };
#pragma unroll 1
  for (int p = 0; p < n_prn; p += 2) {
    const bool two = p + 1 < n_prn;                        // (wave-uniform; a last odd row is read twice)
    const gpsx_peak_t *row0 = rows + (size_t)p * (size_t)n_dopp, *row1 = rows + (size_t)(two ? p + 1 : p) * (size_t)n_dopp;
    u64 k0 = 0, k1 = 0;
#pragma unroll 1
    for (int d0 = lane; d0 < n_dopp; d0 += 4 * 64) {     // (lane-dependent by one turn at most; no cross-lane operation in here)
      u32 v0[4], v1[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const bool in = d0 + 64 * u < n_dopp;
        v0[u] = in ? row0[d0 + 64 * u].max_val : 0u;
        v1[u] = in ? row1[d0 + 64 * u].max_val : 0u;
      }
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const bool in = d0 + 64 * u < n_dopp;
        const u64 lo = (u64)(0xFFFFFFFFu - (u32)(d0 + 64 * u));
        const u64 a = in ? ((u64)v0[u] << 32) | lo : 0ull, b = in ? ((u64)v1[u] << 32) | lo : 0ull;
        k0 = a > k0 ? a : k0;
        k1 = b > k1 ? b : k1;
      }
    }
    k0 = wave_key(k0);
    k1 = wave_key(k1);
    key = lane == p ? k0 : (two && lane == p + 1 ? k1 : key);
  }
  const u32 M = is_prn ? (u32)(key >> 32) : 0u;
  const u32 bin = is_prn ? 0xFFFFFFFFu - (u32)key : 0u;
  const Quad best = *reinterpret_cast<const Quad *>(rows + (is_prn ? (size_t)lane * (size_t)n_dopp + bin : 0));
  const u32 tau = is_prn ? best.b : 0u, S = best.c;
  const int dopp_hz = is_prn ? (int)((u32)dopp_min_hz + bin * (u32)dopp_step_hz) : 0;   // (inside int32: the host checked both ends of the grid)
  const bool detected = is_prn && M >= (cfg.min_peak > 1u ? cfg.min_peak : 1u) &&
                        (u64)M * (u64)kPhases * (u64)cfg.det_den >= (u64)cfg.det_num * (u64)S;
  const int n_detected = __popcll(__ballot(detected));

  // 2 the bank: lane p is PRN index p
  const gpsx_weph_t e = bank[(size_t)r * (size_t)bank_stride + (size_t)(is_prn ? lane : 0)];
  const bool have = is_prn && (e.flags & GPSX_WEPH_VALID) != 0;
  const bool sel = detected && have && e.svh == 0;
  double ion[8];
  choose_ion(cfg.ion, ion);
  const double kk = kOmegaE / kC;
  const double t0 = pri.tow_s + cfg.epoch_offset_s;
  const double s_frac = (double)tau / 16368.0;

  // the unknowns, what steps 2 and 3 leave, what the passes leave
  double x0 = pri.rr[0], x1 = pri.rr[1], x2 = pri.rr[2], x3 = 0.0, x4 = 0.0;
  bool cand = false;
  int n_cand = 0, ref = -1, n_ms = 0;
  double z = 0.0, el_c = 0.0, az_c = 0.0, resid = 0.0;
  u32 flags = 0;
  int mode = 0;   // 0: iterating, 1: converged, the residuals at the final unknowns are due, 2: finished
  int n_used = 0, n_iter = 0;
  u64 used_mask = 0;
  double q00 = 0.0, q11 = 0.0, q22 = 0.0, q01 = 0.0, q12 = 0.0, q02 = 0.0, rms = 0.0, lat_out = 0.0, lon_out = 0.0, hgt_out = 0.0;

#pragma unroll 1
  for (int pass = 0; pass <= kMaxIter; pass++) {
    if (__ballot(mode != 2) == 0ull)   // (wave-uniform)
      break;
    double lat, lon, hgt;
    geodetic(x0, x1, x2, lat, lon, hgt);
    const double T = 1000.0 * (t0 + x4), tow = T / 1000.0;      // (gpsx_wpred's step 2 with a double T)

    // EVAL((x0, x1, x2), T) in the lanes that may have a row
    bool good = pass == 0 ? sel : cand;
    double pr = 72.0 * kMs, el = 0.0, az = 0.0, l0 = 0.0, l1 = 0.0, l2 = 0.0, var = 0.0;
    SatState s = {};
#pragma unroll 1
    for (int k = 0; k < 3; k++) {
      if (good) {            // (lane-local: no cross-lane operation in here)
        good = sat_at_clock(e, (T - pr / kMs) / 1000.0, s);
        if (good) {
          l0 = s.px - x0;
          l1 = s.py - x1;
          l2 = s.pz - x2;
          const double range = sqrt(l0 * l0 + l1 * l1 + l2 * l2);
          const double rn = sqrt(s.px * s.px + s.py * s.py + s.pz * s.pz);
          const double rho = range + kOmegaE * (s.px * x1 - s.py * x0) / kC;
          good = !(range == 0.0) && !(rn < kRe) && !(rho <= 0.0);
          if (good) {
            l0 /= range;
            l1 /= range;
            l2 /= range;
            az_el(l0, l1, l2, lat, lon, hgt, az, el);
            double dion, dtrp;
            var = pr_model(tow, ion, lat, lon, hgt, az, el, s.svar, dion, dtrp);
            pr = (rho + dion + dtrp - kC * s.clk) + kC * e.tgd;
          }
        }
      }
    }
    const double rd = l0 * s.vx + l1 * s.vy + l2 * s.vz + kk * (s.vx * x1 - s.vy * x0) - kC * s.rate;
    good = good && finite(pr) && finite(el) && finite(az) && finite(rd) && finite(var) && __builtin_fabs(pr) < 1E12;

    if (pass == 0) {       // (wave-uniform) steps 2 and 3: the candidates, the reference, the milliseconds
      cand = good && el >= cfg.el_min_rad;
      const u64 cand_mask = __ballot(cand);
      n_cand = __popcll(cand_mask);
      el_c = cand ? el : 0.0;
      az_c = cand ? az : 0.0;
      if (n_cand < cfg.min_sats) {
        flags = GPSX_WSNAP_TOO_FEW;
        mode = 2;
      } else {
        int rank = 0;
#pragma unroll 1
        for (int p = 0; p < n_prn; p++) {
          const double eq = __shfl(el, p, 64);
          rank += (((cand_mask >> p) & 1ull) != 0 && (eq > el || (eq == el && p < lane))) ? 1 : 0;
        }
        ref = __ffsll((long long)__ballot(cand && rank == 0)) - 1;   // (one lane: the ranks of the candidates are a permutation)
        const double pr_ref = __shfl(pr, ref, 64), s_ref = __shfl(s_frac, ref, 64);
        const double n_ref = rint(pr_ref / kMs - s_ref);
        const double b0 = (n_ref + s_ref) * kMs - pr_ref;
        const double n_p = rint((pr + b0) / kMs - s_frac);
        z = (n_p + s_frac) * kMs;
        n_ms = cand ? (int)n_p : 0;   // (|pr| < 1e12 and so is b0's: far inside int32)
      }
    }

    // the lane's row
    const bool row = cand && good && !(el < 0.0) && mode != 2;
    double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, y = 0.0, v = 0.0;
    if (row) {
      v = z - (pr + x3);
      const double sig = sqrt(var);
      a[0] = -l0 / sig;
      a[1] = -l1 / sig;
      a[2] = -l2 / sig;
      a[3] = 1.0 / sig;
      a[4] = rd / sig;
      y = v / sig;
    }
    const u64 rows_mask = __ballot(row);
    const bool counted = mode == 1 ? (row && ((used_mask >> lane) & 1ull) != 0) : row;
    const double vv = counted ? v : 0.0;
    double n[15], g[5];
#pragma unroll
    for (int i = 0; i < 5; i++) {
#pragma unroll
      for (int j = 0; j <= i; j++)
        n[low(i, j)] = group_sum(a[i] * a[j], 64);
    }
#pragma unroll
    for (int i = 0; i < 5; i++)
      g[i] = group_sum(a[i] * y, 64);
    const double ss = group_sum(vv * vv, 64);
    bool sums_ok = true;
#pragma unroll
    for (int i = 0; i < 15; i++)
      sums_ok = sums_ok && finite(n[i]);
#pragma unroll
    for (int i = 0; i < 5; i++)
      sums_ok = sums_ok && finite(g[i]);

    // Cholesky N = L L^T, M = L^-1, dx = M^T M g; computed by every lane whatever the sums are, used by the wave that iterates
    double l[15], m[15], pv[5], w[5], dx[5];
    bool pivots = true;
#pragma unroll
    for (int j = 0; j < 5; j++) {
      double pj = n[low(j, j)];
#pragma unroll
      for (int k = 0; k < j; k++)
        pj = pj - l[low(j, k)] * l[low(j, k)];
      pv[j] = pj;
      pivots = pivots && (j == 0 ? pj > 0.0 : pj > kPivot * n[low(j, j)]);
      l[low(j, j)] = sqrt(pj);
#pragma unroll
      for (int i = j + 1; i < 5; i++) {
        double tt = n[low(i, j)];
#pragma unroll
        for (int k = 0; k < j; k++)
          tt = tt - l[low(i, k)] * l[low(j, k)];
        l[low(i, j)] = tt / l[low(j, j)];
      }
    }
#pragma unroll
    for (int j = 0; j < 5; j++)
      m[low(j, j)] = 1.0 / l[low(j, j)];
#pragma unroll
    for (int i = 1; i < 5; i++) {
#pragma unroll
      for (int j = 0; j < i; j++) {
        double tt = l[low(i, j)] * m[low(j, j)];
#pragma unroll
        for (int k = j + 1; k < i; k++)
          tt = tt + l[low(i, k)] * m[low(k, j)];
        m[low(i, j)] = -tt / l[low(i, i)];
      }
    }
#pragma unroll
    for (int i = 0; i < 5; i++) {
      double tt = m[low(i, 0)] * g[0];
#pragma unroll
      for (int k = 1; k <= i; k++)
        tt = tt + m[low(i, k)] * g[k];
      w[i] = tt;
    }
#pragma unroll
    for (int j = 0; j < 5; j++) {
      double tt = m[low(j, j)] * w[j];
#pragma unroll
      for (int i = j + 1; i < 5; i++)
        tt = tt + m[low(i, j)] * w[i];
      dx[j] = tt;
    }

    if (mode == 1) {   // the residuals at the final unknowns
      rms = sqrt(ss / (double)n_used);
      resid = vv;
      lat_out = lat;
      lon_out = lon;
      hgt_out = hgt;
      flags = rms > cfg.max_resid_m ? GPSX_WSNAP_RESID : GPSX_WSNAP_FIX;
      mode = 2;
    } else if (mode == 0) {
      n_iter = pass + 1;
      n_used = __popcll(rows_mask);
      used_mask = rows_mask;
      if (n_used < cfg.min_sats) {
        flags = GPSX_WSNAP_TOO_FEW;
        mode = 2;
      } else if (!sums_ok) {
        flags = GPSX_WSNAP_NONFINITE;
        mode = 2;
      } else if (!pivots) {
        flags = GPSX_WSNAP_SINGULAR;
        mode = 2;
      } else if (!(finite(dx[0]) && finite(dx[1]) && finite(dx[2]) && finite(dx[3]) && finite(dx[4]))) {
        flags = GPSX_WSNAP_NONFINITE;
        mode = 2;
      } else {
        x0 += dx[0];
        x1 += dx[1];
        x2 += dx[2];
        x3 += dx[3];
        x4 += dx[4];
        const double ms4 = 1000.0 * dx[4];
        if (dx[0] * dx[0] + dx[1] * dx[1] + dx[2] * dx[2] + dx[3] * dx[3] + ms4 * ms4 < 1E-8) {
          q00 = m[low(0, 0)] * m[low(0, 0)] + m[low(1, 0)] * m[low(1, 0)] + m[low(2, 0)] * m[low(2, 0)] + m[low(3, 0)] * m[low(3, 0)] +
                m[low(4, 0)] * m[low(4, 0)];
          q11 = m[low(1, 1)] * m[low(1, 1)] + m[low(2, 1)] * m[low(2, 1)] + m[low(3, 1)] * m[low(3, 1)] + m[low(4, 1)] * m[low(4, 1)];
          q22 = m[low(2, 2)] * m[low(2, 2)] + m[low(3, 2)] * m[low(3, 2)] + m[low(4, 2)] * m[low(4, 2)];
          q01 = m[low(1, 0)] * m[low(1, 1)] + m[low(2, 0)] * m[low(2, 1)] + m[low(3, 0)] * m[low(3, 1)] + m[low(4, 0)] * m[low(4, 1)];
          q12 = m[low(2, 1)] * m[low(2, 2)] + m[low(3, 1)] * m[low(3, 2)] + m[low(4, 1)] * m[low(4, 2)];
          q02 = m[low(2, 0)] * m[low(2, 2)] + m[low(3, 0)] * m[low(3, 2)] + m[low(4, 0)] * m[low(4, 2)];
          mode = 1;
        } else if (pass + 1 == kMaxIter) {
          flags = GPSX_WSNAP_NO_CONV;
          mode = 2;
        }
      }
    }
  }

  // 6 the records
  const float f0 = (float)q00, f1 = (float)q11, f2 = (float)q22, f3 = (float)q01, f4 = (float)q12, f5 = (float)q02;
  double tow = pri.tow_s;
  int week = pri.week;
  bool solved = flags == GPSX_WSNAP_FIX || flags == GPSX_WSNAP_RESID;
  if (solved) {
    tow = pri.tow_s + x4;
    if (tow >= kWeek) {
      tow -= kWeek;
      week += 1;
    } else if (tow < 0.0) {
      tow += kWeek;
      week -= 1;
    }
    if (!(finite(x0) && finite(x1) && finite(x2) && finite(x3) && finite(x4) && finite(tow) && tow >= 0.0 && tow < kWeek && finite(lat_out) && finite(lon_out) && finite(hgt_out) &&
          finite(rms) && finite((double)f0) && finite((double)f1) && finite((double)f2) && finite((double)f3) && finite((double)f4) &&
          finite((double)f5))) {
      flags = GPSX_WSNAP_NONFINITE;
      solved = false;
      tow = pri.tow_s;
      week = pri.week;
    }
  }
  if (sv && is_prn) {
    const bool used = ((used_mask >> lane) & 1ull) != 0;
    gpsx_wsnap_sv_t o = {};
    o.flags = (detected ? GPSX_WSNAP_SV_DETECTED : 0u) | (have ? GPSX_WSNAP_SV_HAVE_EPH : 0u) | (cand ? GPSX_WSNAP_SV_CANDIDATE : 0u) |
              (used ? GPSX_WSNAP_SV_USED : 0u) | (lane == ref ? GPSX_WSNAP_SV_REFERENCE : 0u);
    o.n_ms = ref >= 0 ? n_ms : 0;
    o.phase = tau;
    o.dopp_hz = dopp_hz;
    o.el = el_c;
    o.az = az_c;
    o.resid_m = solved && used && finite(resid) ? resid : 0.0;
    sv[(size_t)r * (size_t)n_prn + (size_t)lane] = o;
  }
  if (lane == 0) {
    gpsx_wsnap_t o = {};
    o.flags = flags;
    o.week = week;
    o.n_detected = (uint8_t)n_detected;
    o.n_candidates = (uint8_t)n_cand;
    o.n_used = (uint8_t)n_used;
    o.n_iter = (uint8_t)n_iter;
    o.ref = ref;
    o.used_mask = used_mask;
    o.tow_s = tow;
    if (solved) {
      o.rr[0] = x0;
      o.rr[1] = x1;
      o.rr[2] = x2;
      o.b_m = x3;
      o.dt_s = x4;
      o.geo[0] = lat_out;
      o.geo[1] = lon_out;
      o.geo[2] = hgt_out;
      o.resid_rms_m = rms;
      o.qr[0] = f0;
      o.qr[1] = f1;
      o.qr[2] = f2;
      o.qr[3] = f3;
      o.qr[4] = f4;
      o.qr[5] = f5;
    }
    snap[r] = o;
  }
}

void launch_wsnap(hipStream_t s, const gpsx_wsnap_cfg_t &cfg, int n_rx, int n_prn, int dopp_min_hz, int dopp_step_hz, int n_dopp,
                  const gpsx_peak_t *d_peaks, const gpsx_weph_t *d_bank, int bank_stride, const gpsx_wsnap_prior_t *d_prior, gpsx_wsnap_t *d_snap,
                  gpsx_wsnap_sv_t *d_sv)
{
  // (no checks of its own: gpsx_api_wtrack.hip's wsnap() is the one list of what a launch needs and refuses with a text before it comes here)
  hipLaunchKernelGGL(k_wsnap, dim3(((unsigned)n_rx + 3u) / 4u), dim3(256), 0, s, cfg, n_rx, n_prn, n_dopp, dopp_min_hz, dopp_step_hz, bank_stride,
                     d_peaks, d_bank, d_prior, d_snap, d_sv);
}

}  // namespace gpsx
