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
// A round's parts are gpsx_wsolve_parts.hpp's -- satellite, azimuth and elevation, model terms as k_wfix.hip calls them; the sums,
// the Cholesky solve and the record's fill operation for operation what k_wfix.hip writes out -- so with repair = 0 and max_excl = 0
// the fix records and pseudoranges are k_wfix's bytes.  The reference scan is this file's own text: shared, it cost 1 % at 64 slots
// per receiver (EXPERIMENTS.md, "One parts header for the solver kernels").
//
// Every cross-lane operation runs under wave-uniform control flow: the round loop and the pass loop both run while a ballot says
// "a group of this wave is not finished"; the scan (w steps of shuffles, w the launch's) runs once per round and normal_sums
// and group_sum (butterflies of width w) once per pass, each outside every branch of its loop's body; a group that is finished masks
// its own updates (groups of one wave routinely sit in different rounds); nothing returns before the last shuffle.  Every loop is
// bounded: max_excl + 2 rounds of at most eleven passes, Kepler at 30 steps, the geodetic fixed point at 30.  FP64 on the vector
// ALU, no LDS, no scratch (build.py check_wfde).
#include <hip/hip_runtime.h>

#include <cstddef>

#include "gpsx_device.hpp"
#include "gpsx_kernels.hpp"
#include "gpsx_wsolve_parts.hpp"

namespace gpsx {
using namespace wsolve;

static_assert(sizeof(gpsx_wfde_cfg_t) == 128 && offsetof(gpsx_wfde_cfg_t, fix) == 0 && offsetof(gpsx_wfde_cfg_t, z_global) == 96 &&
              offsetof(gpsx_wfde_cfg_t, max_excl) == 104 && offsetof(gpsx_wfde_cfg_t, repair) == 108 && offsetof(gpsx_wfde_cfg_t, reserved) == 112,
              "gpsx_wfde_cfg_t layout");
static_assert(sizeof(gpsx_wfde_t) == 64 && offsetof(gpsx_wfde_t, n_rounds) == 4 && offsetof(gpsx_wfde_t, n_excluded) == 8 &&
              offsetof(gpsx_wfde_t, dof) == 12 && offsetof(gpsx_wfde_t, excl_mask) == 16 && offsetof(gpsx_wfde_t, plus_mask) == 24 &&
              offsetof(gpsx_wfde_t, minus_mask) == 32 && offsetof(gpsx_wfde_t, t_stat) == 40 && offsetof(gpsx_wfde_t, t_limit) == 48 &&
              offsetof(gpsx_wfde_t, reserved) == 56, "gpsx_wfde_t layout");

// what a round's reference scan yields (gpsx_wobs_pseudoranges over the active slots)
struct RefScan {
  int ref, count, week;   // the reference slot (-1: none), the active slots, the reference's week
  double pr, rx_tow;      // the lane's pseudorange (0 where not live), the receiver's time of week (0 where !time_ok)
  bool time_ok;
};

__global__ __launch_bounds__(256) void k_wfde(gpsx_wfde_cfg_t fc, const gpsx_wobs_t *obs, const gpsx_weph_t *eph, const gpsx_wlock_t *lock,
                                              const gpsx_wfix_t *prev, int n_rx, int w, int log2w, gpsx_wfix_t *fix, gpsx_wfde_t *fde,
                                              double *pr_out)
{
  const gpsx_wfix_cfg_t &cfg = fc.fix;
  const Lane ln = lane_of(w, log2w, n_rx, cfg.ch_per_rx);
  const int j = ln.j, base = ln.base;
  const long long r = ln.r;
  const bool in_rx = ln.in_rx, slot = ln.slot;
  const size_t at = ln.at;
  const u64 group_bits = ln.group_bits;

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
  double ion[8];
  choose_ion(cfg.ion, ion);

  // ---- what the rounds carry: the lane's millisecond correction and exclusion, the group's verdict, its last round's record ----
  int kj = 0;
  bool excl = false, done = !in_rx;
  int n_stat = 0, n_rounds = 0, dof = 0;
  u32 verdict = GPSX_WFDE_NOFIX;
  double t_stat = 0.0, t_limit = 0.0;
  u32 flags = 0;
  int n_used = 0, n_iter = 0, ref = -1, week = 0;
  u64 used_mask = 0;
  double rx_tow = 0.0, pr = 0.0;
  FixResult f = {};

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
    RefScan sc = {-1, 0, 0, 0.0, 0.0, false};
    long long ref_tx = 0;
    float ref_ph = 0.0f;
#pragma unroll 1
    for (int k = 0; k < w; k++) {
      const int src = base + k;
      const long long tx_k = __shfl(tx, src);
      const float ph_k = __shfl(o.code_phase_fine, src);
      const int us_k = __shfl((int)act, src), week_k = __shfl(e.week, src);
      if (us_k) {
        sc.count++;
        if (sc.ref < 0 || (double)fold_ms(tx_k - ref_tx) - ((double)ph_k - (double)ref_ph) / 16368.0 > 0.0) {
          sc.ref = k;
          ref_tx = tx_k;
          ref_ph = ph_k;
          sc.week = week_k;
        }
      }
    }
    if (sc.ref >= 0) {
      if (live)
        sc.pr = 299792458e-3 * ((double)fold_ms(ref_tx - tx) + ((double)o.code_phase_fine - (double)ref_ph) / 16368.0 + cfg.offset_ms);
      const double rx = ((double)ref_tx - (double)ref_ph / 16368.0 + cfg.offset_ms) / 1000.0;
      sc.rx_tow = rx >= 604800.0 ? rx - 604800.0 : (rx < 0.0 ? rx + 604800.0 : rx);
    }
    sc.time_ok = finite(sc.rx_tow);
    if (!sc.time_ok)
      sc.rx_tow = 0.0;
    const double pr_r = sc.pr;

    // ---- the observation time, the satellite at its transmit time (satposs) ----
    const GTime t_obs = obs_time(sc.week, sc.rx_tow);
    const double tow = tow_of(t_obs);
    double px = 0.0, py = 0.0, pz = 0.0, clk = 0.0, svar = 0.0;
    bool cand = false;   // the solver has a satellite record for this slot (health and all)
    if (live)
      cand = sat_at_transmit(e, t_obs, pr_r, px, py, pz, clk, svar);
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
      f = FixResult{};
      f.x0 = sx0;
      f.x1 = sx1;
      f.x2 = sx2;
      ref = sc.ref;
      week = sc.week;
      rx_tow = sc.rx_tow;
      pr = act ? pr_r : 0.0;
      if (!sc.time_ok) {
        flags = GPSX_WFIX_NONFINITE;
        mode = 2;
      } else if (sc.count < cfg.min_sats) {
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
      geodetic(f.x0, f.x1, f.x2, lat, lon, hgt);
      // the lane's row
      bool row = cand && mode != 2 && !(rn < kRe);
      double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, y = 0.0, v = 0.0;
      if (row) {
        double l0 = px - f.x0, l1 = py - f.x1, l2 = pz - f.x2;
        const double range = sqrt(l0 * l0 + l1 * l1 + l2 * l2);
        l0 /= range;
        l1 /= range;
        l2 /= range;
        const double rho = range + kOmegaE * (px * f.x1 - py * f.x0) / kC;
        row = !(rho <= 0.0);
        double az, el;
        az_el(l0, l1, l2, lat, lon, hgt, az, el);
        row = row && !(el < 0.0) && healthy;
        if (row) {
          double dion, dtrp;
          const double var = pr_model(tow, ion, lat, lon, hgt, az, el, svar, dion, dtrp);
          v = (pr_r - tgd) - (rho + dion + dtrp + f.x3 - kC * clk);
          const double sig = sqrt(var);
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
      const Normal ns = {group_sum(a0 * a0, w), group_sum(a1 * a0, w), group_sum(a1 * a1, w), group_sum(a2 * a0, w), group_sum(a2 * a1, w),
                         group_sum(a2 * a2, w), group_sum(a3 * a0, w), group_sum(a3 * a1, w), group_sum(a3 * a2, w), group_sum(a3 * a3, w),
                         group_sum(a0 * y, w),  group_sum(a1 * y, w),  group_sum(a2 * y, w),  group_sum(a3 * y, w)};
      const double ss = group_sum(vv * vv, w), tt = group_sum(y * y, w);
      const Solve sv = solve(ns);   // computed by every lane, used by the groups that iterate
      const bool ok_sums = sums_ok(ns), ok_pivots = pivots_ok(ns, sv);

      if (mode == 1) {   // the residuals at the final x; the test's T and every counted slot's w^2 = y^2 / (1 - |M a|^2)
        f.rms = sqrt(ss / (double)n_used);
        f.lat = lat;
        f.lon = lon;
        f.hgt = hgt;
        flags = GPSX_WFIX_FIX;
        mode = 2;
        v_fin = v;
        row_fin = row;
        t_sum = tt;
        n_cnt = __popcll(rows & used_mask);
        name_ok = ok_sums && ok_pivots;
        const double h0 = sv.m00 * a0, h1 = sv.m10 * a0 + sv.m11 * a1, h2 = sv.m20 * a0 + sv.m21 * a1 + sv.m22 * a2,
                     h3 = sv.m30 * a0 + sv.m31 * a1 + sv.m32 * a2 + sv.m33 * a3;
        const double rest = 1.0 - (h0 * h0 + h1 * h1 + h2 * h2 + h3 * h3);
        w2 = counted && rest > 1E-10 ? y * y / rest : 0.0;
      } else if (mode == 0) {
        n_iter = pass + 1;
        n_used = __popcll(rows);
        used_mask = rows;
        if (n_used < cfg.min_sats) {
          flags = GPSX_WFIX_TOO_FEW;
          mode = 2;
        } else if (!ok_sums) {
          flags = GPSX_WFIX_NONFINITE;
          mode = 2;
        } else if (!ok_pivots) {
          flags = GPSX_WFIX_SINGULAR;
          mode = 2;
        } else if (!(finite(sv.d0) && finite(sv.d1) && finite(sv.d2) && finite(sv.d3))) {
          flags = GPSX_WFIX_NONFINITE;
          mode = 2;
        } else {
          f.x0 += sv.d0;
          f.x1 += sv.d1;
          f.x2 += sv.d2;
          f.x3 += sv.d3;
          if (sv.d0 * sv.d0 + sv.d1 * sv.d1 + sv.d2 * sv.d2 + sv.d3 * sv.d3 < 1E-8) {
            f.q = q_block(sv);
            mode = 1;
          } else if (pass + 1 == kMaxIter) {
            flags = GPSX_WFIX_NO_CONV;
            mode = 2;
          }
        }
      }
    }

    // ---- the round's record is complete: gpsx_wfix's rule for a result that is not finite ----
    if (!done && flags == GPSX_WFIX_FIX && !fix_finite(f))
      flags = GPSX_WFIX_NONFINITE;
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
          const double kd = rint(v_fin / kMs);
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
      sx0 = fixed ? f.x0 : 0.0;
      sx1 = fixed ? f.x1 : 0.0;
      sx2 = fixed ? f.x2 : 0.0;
    }
  }

  // ---- the masks; the receiver's two records, by the group's first lane; every slot's pseudorange ----
  const u64 excl_mask = (__ballot(excl) >> base) & group_bits, plus_mask = (__ballot(kj == 1) >> base) & group_bits,
            minus_mask = (__ballot(kj == -1) >> base) & group_bits;
  if (slot && pr_out)
    pr_out[at] = finite(pr) ? pr : 0.0;
  if (in_rx && j == 0) {
    fix[r] = fix_record(flags, n_used, n_iter, ref, used_mask, rx_tow, week, f);
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
  const Geometry g = geometry_of(n_rx, cfg.fix.ch_per_rx);
  hipLaunchKernelGGL(k_wfde, dim3(g.grid), dim3(256), 0, s, cfg, d_obs, d_eph, d_lock, d_prev, n_rx, g.w, g.log2w, d_fix, d_fde, d_pr_m);
}

}  // namespace gpsx
