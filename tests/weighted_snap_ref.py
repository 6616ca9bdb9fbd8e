"""A CPU restatement of the weighted chain's snapshot fixes (include/gpsx.h gpsx_wsnap), for the tests: a weighted grid's peak records,
an ephemeris bank and one prior per receiver in, one record per receiver and one per (receiver, PRN index) out.  Written from the
header's text on the parts the neighbours have: weighted_acq_ref's steps 1 and 2 (Python integers), weighted_pred_ref.one_pass -- the
satellite at its clock's reading (weighted_kf_ref.satellites), the line of sight, azimuth and elevation, the two delays -- with a
double T, weighted_fix_ref's ecef2pos and variance terms.  The sums run in the butterfly's order (pairs of neighbours, six rounds over
64 lanes), the 5 x 5 factorisation in the header's order, every operation a single np.float64 one.  What is exact: detection, the
candidates' and the reference's choice, the milliseconds N_p, the masks and flags of receivers whose decisions are clear of round-off.
What is not: everything behind a sine -- numpy's libm is not the device's.  Nothing of the library's kernel code is included or imported."""
import numpy as np

import weighted_acq_ref as Q
import weighted_eph_ref as E
import weighted_fix_ref as F
import weighted_pred_ref as P

F_FIX, F_RESID, F_TOO_FEW, F_SINGULAR, F_NO_CONV, F_NONFINITE, F_NO_PRIOR = 1, 2, 4, 8, 16, 32, 64      # GPSX_WSNAP_*
PRIOR_HAVE = 1
SV_DETECTED, SV_HAVE_EPH, SV_CANDIDATE, SV_USED, SV_REFERENCE = 1, 2, 4, 8, 16                          # GPSX_WSNAP_SV_*
CFG_DTYPE = np.dtype([("ion", "<f8", (8,)), ("el_min_rad", "<f8"), ("epoch_offset_s", "<f8"), ("max_resid_m", "<f8"), ("det_num", "<i4"),
                      ("det_den", "<i4"), ("min_peak", "<u4"), ("min_sats", "<i4"), ("reserved", "<i4", (6,))])
PRIOR_DTYPE = np.dtype([("flags", "<u4"), ("week", "<i4"), ("rr", "<f8", (3,)), ("tow_s", "<f8"), ("reserved", "<u4", (2,))])
SNAP_DTYPE = np.dtype([("flags", "<u4"), ("week", "<i4"), ("n_detected", "u1"), ("n_candidates", "u1"), ("n_used", "u1"), ("n_iter", "u1"),
                       ("ref", "<i4"), ("used_mask", "<u8"), ("rr", "<f8", (3,)), ("b_m", "<f8"), ("dt_s", "<f8"), ("tow_s", "<f8"),
                       ("geo", "<f8", (3,)), ("resid_rms_m", "<f8"), ("qr", "<f4", (6,))])
SV_DTYPE = np.dtype([("flags", "<u4"), ("n_ms", "<i4"), ("phase", "<u4"), ("dopp_hz", "<i4"), ("el", "<f8"), ("az", "<f8"), ("resid_m", "<f8"),
                     ("reserved", "<u4", (2,))])
assert CFG_DTYPE.itemsize == 128 and PRIOR_DTYPE.itemsize == 48 and SNAP_DTYPE.itemsize == 128 and SV_DTYPE.itemsize == 48
PEAK_DTYPE, EPH_DTYPE = Q.PEAK_DTYPE, E.EPH_DTYPE
MS, C_LIGHT, OMEGA_E, WEEK_S = P.MS, P.C_LIGHT, P.OMEGA_E, 604800.0
MAX_ITER, PIVOT, LANES = F.MAX_ITER, F.PIVOT, 64
f8 = np.float64


def make_cfg(epoch_offset_s, el_min_rad=0.0873, max_resid_m=1000.0, det=(4, 1), min_peak=0, min_sats=5, ion=None):
    """the library's gpsx_wsnap_cfg_t as a one-element array"""
    cfg = np.zeros(1, CFG_DTYPE)
    for name, v in (("el_min_rad", el_min_rad), ("epoch_offset_s", epoch_offset_s), ("max_resid_m", max_resid_m), ("det_num", det[0]),
                    ("det_den", det[1]), ("min_peak", min_peak), ("min_sats", min_sats)):
        cfg[name] = v
    if ion is not None:
        cfg["ion"][0] = ion
    return cfg


def make_prior(rr, week, tow_s, flags=PRIOR_HAVE):
    """gpsx_wsnap_prior_t records from rr [n, 3]"""
    rr = np.asarray(rr, np.float64).reshape(-1, 3)
    out = np.zeros(len(rr), PRIOR_DTYPE)
    out["flags"], out["week"], out["rr"], out["tow_s"] = flags, week, rr, tow_s
    return out


def prior_ok(p):
    """step 0 on one record"""
    return (int(p["flags"]) == PRIOR_HAVE and not p["reserved"].any() and bool(np.isfinite(p["rr"]).all()) and bool(np.isfinite(p["tow_s"]))
            and 0.0 <= float(p["tow_s"]) < WEEK_S and 0 <= int(p["week"]) <= 32767)


def butterfly(v):
    """the sum of 64 lanes' values in the butterfly's order: in round m lane l adds lane l ^ m's, m = 1, 2, 4, 8, 16, 32"""
    v = np.asarray(v, np.float64)
    assert v.shape == (LANES,)
    for _ in range(6):
        v = v[0::2] + v[1::2]
    return f8(v[0])


def evaluate(e, sel, x, T, ion):
    """EVAL((x_0, x_1, x_2), T / 1000) for the records e [n] in the lanes sel -> dict(good, pr, los [n, 3], el, az, rd, var, geo, passes)"""
    n = len(e)
    xh = np.array([x[0], x[1], x[2], 0.0])
    geo = tuple(float(v[0]) for v in F._geodetic(xh[None, :3]))
    good, pr, passes = sel.copy(), np.full(n, 72.0 * MS), []
    for _ in range(3):
        d = P.one_pass(e, T, pr, xh, geo, ion)
        good = good & d["good"]
        pr = np.where(good, d["pr"], pr)
        passes.append(d)
    d = passes[-1]
    los, vs, el, az = d["los"], d["vs"], d["el"], d["az"]
    kk = OMEGA_E / C_LIGHT
    rd = los[:, 0] * vs[:, 0] + los[:, 1] * vs[:, 1] + los[:, 2] * vs[:, 2] + kk * (vs[:, 0] * xh[1] - vs[:, 1] * xh[0]) - C_LIGHT * d["rate"]
    sva = e["sva"]
    ura = np.where((sva < 0) | (sva > 14), 6144.0, F.URA[np.clip(sva, 0, 14)])
    v_ion = (d["dion"] * 0.5) * (d["dion"] * 0.5)
    sin_el = np.sin(el)
    v_trp = (0.3 / (sin_el + 0.1)) * (0.3 / (sin_el + 0.1))
    ev = 0.003 * 0.003
    var = ev * (ev + ev / sin_el) + ura * ura + v_ion + v_trp
    good = good & np.isfinite(pr) & np.isfinite(el) & np.isfinite(az) & np.isfinite(rd) & np.isfinite(var) & (np.abs(pr) < 1E12)
    return dict(good=good, pr=pr, los=los, el=el, az=az, rd=rd, var=var, geo=geo, passes=passes)


def _low(i, j):
    return i * (i + 1) // 2 + j


def cholesky5(n, g):
    """the header's factorisation of the 5 x 5 system: n [15] (the lower triangle, row by row), g [5] -> pivots ok, dx [5], qr [6], the
    pivots' shares p_k / N_kk (p_0 itself)"""
    lo, m, ok, shares = [f8(0.0)] * 15, [f8(0.0)] * 15, True, []
    for j in range(5):
        pj = n[_low(j, j)]
        for k in range(j):
            pj = pj - lo[_low(j, k)] * lo[_low(j, k)]
        ok = ok and bool(pj > 0.0 if j == 0 else pj > PIVOT * n[_low(j, j)])
        shares.append(float(pj) if j == 0 else float(pj / n[_low(j, j)]))
        lo[_low(j, j)] = np.sqrt(pj)
        for i in range(j + 1, 5):
            t = n[_low(i, j)]
            for k in range(j):
                t = t - lo[_low(i, k)] * lo[_low(j, k)]
            lo[_low(i, j)] = t / lo[_low(j, j)]
    for j in range(5):
        m[_low(j, j)] = f8(1.0) / lo[_low(j, j)]
    for i in range(1, 5):
        for j in range(i):
            t = lo[_low(i, j)] * m[_low(j, j)]
            for k in range(j + 1, i):
                t = t + lo[_low(i, k)] * m[_low(k, j)]
            m[_low(i, j)] = -t / lo[_low(i, i)]
    w, dx = [], []
    for i in range(5):
        t = m[_low(i, 0)] * g[0]
        for k in range(1, i + 1):
            t = t + m[_low(i, k)] * g[k]
        w.append(t)
    for j in range(5):
        t = m[_low(j, j)] * w[j]
        for i in range(j + 1, 5):
            t = t + m[_low(i, j)] * w[i]
        dx.append(t)
    M = lambda i, j: m[_low(i, j)]      # noqa: E731
    q = [M(0, 0) * M(0, 0) + M(1, 0) * M(1, 0) + M(2, 0) * M(2, 0) + M(3, 0) * M(3, 0) + M(4, 0) * M(4, 0),
         M(1, 1) * M(1, 1) + M(2, 1) * M(2, 1) + M(3, 1) * M(3, 1) + M(4, 1) * M(4, 1),
         M(2, 2) * M(2, 2) + M(3, 2) * M(3, 2) + M(4, 2) * M(4, 2),
         M(1, 0) * M(1, 1) + M(2, 0) * M(2, 1) + M(3, 0) * M(3, 1) + M(4, 0) * M(4, 1),
         M(2, 1) * M(2, 2) + M(3, 1) * M(3, 2) + M(4, 1) * M(4, 2),
         M(2, 0) * M(2, 2) + M(3, 0) * M(3, 2) + M(4, 0) * M(4, 2)]
    return ok, np.array(dx, np.float64), np.array(q, np.float64), shares


def _pad(v):
    out = np.zeros(LANES)
    out[:len(v)] = v
    return out


def solve(c, e, detected, tau, prior, trace=None):
    """steps 2 - 6 for one receiver: c the cfg record, e [n_prn] its bank records, detected [n_prn] bools, tau [n_prn] the code phases in
    samples (the records' integers; a test may pass fractions), prior one PRIOR_DTYPE record that step 0 passed
    -> dict(flags, week, n_candidates, n_used, n_iter, ref, used_mask, x [5], tow_s, geo, qr, rms, have, cand, n_ms, el, az, resid)"""
    n_prn = len(e)
    ion = np.array(c["ion"], np.float64)
    ion = F.ION_DEFAULT if float((ion * ion).sum()) <= 0.0 else ion
    min_sats, el_min = int(c["min_sats"]), float(c["el_min_rad"])
    have = (e["flags"] & E.F_VALID) != 0
    sel = np.asarray(detected, bool) & have & (e["svh"] == 0)
    t0 = f8(prior["tow_s"]) + f8(c["epoch_offset_s"])
    s_frac = np.asarray(tau, np.float64) / 16368.0
    x = np.array([prior["rr"][0], prior["rr"][1], prior["rr"][2], 0.0, 0.0], np.float64)
    out = dict(flags=0, week=int(prior["week"]), n_candidates=0, n_used=0, n_iter=0, ref=-1, used_mask=0, x=x, tow_s=float(prior["tow_s"]),
               geo=np.zeros(3), qr=np.zeros(6, np.float32), rms=0.0, have=have, cand=np.zeros(n_prn, bool), n_ms=np.zeros(n_prn, np.int64),
               el=np.zeros(n_prn), az=np.zeros(n_prn), resid=np.zeros(n_prn))
    tr = dict(passes=[], margins={})
    if trace is not None:
        trace.append(tr)
    mode, cand, z, q, mask, n_used = 0, np.zeros(n_prn, bool), np.zeros(n_prn), np.zeros(6), np.zeros(n_prn, bool), 0
    with np.errstate(all="ignore"):
        for p in range(MAX_ITER + 1):
            if mode == 2:
                break
            T = f8(1000.0) * (t0 + x[4])
            d = evaluate(e, sel if p == 0 else cand, x, T, ion)
            good, pr, el = d["good"], d["pr"], d["el"]
            if p == 0:
                cand = good & (el >= el_min)
                out["cand"], out["n_candidates"] = cand, int(cand.sum())
                out["el"], out["az"] = np.where(cand, el, 0.0), np.where(cand, d["az"], 0.0)
                tr["el0"], tr["good0"], tr["sel"] = el.copy(), good.copy(), sel.copy()
                tr["pass0"], tr["pr0"] = d["passes"][0], pr.copy()
                if out["n_candidates"] < min_sats:
                    out["flags"], mode = F_TOO_FEW, 2
                    continue
                ref = min(np.flatnonzero(cand), key=lambda k: (-float(el[k]), int(k)))
                n_ref = np.rint(pr[ref] / MS - s_frac[ref])
                b0 = (n_ref + s_frac[ref]) * MS - pr[ref]
                u = (pr + b0) / MS - s_frac
                n_p = np.rint(u)
                z = (n_p + s_frac) * MS
                out["ref"], out["n_ms"] = int(ref), np.where(cand, n_p, 0.0).astype(np.int64)
                tr["u"], tr["b0"] = u.copy(), float(b0)
            row = cand & good & ~(el < 0.0)
            v = np.where(row, z - (pr + x[3]), 0.0)
            sig = np.sqrt(d["var"])
            a = np.stack([-d["los"][:, 0] / sig, -d["los"][:, 1] / sig, -d["los"][:, 2] / sig, 1.0 / sig, d["rd"] / sig], 0)
            a = np.where(row[None, :], a, 0.0)
            y = np.where(row, v / sig, 0.0)
            counted = row & mask if mode == 1 else row
            vv = np.where(counted, v, 0.0)
            n = [f8(0.0)] * 15
            for i in range(5):
                for j in range(i + 1):
                    n[_low(i, j)] = butterfly(_pad(a[i] * a[j]))
            g = [butterfly(_pad(a[i] * y)) for i in range(5)]
            ss = butterfly(_pad(vv * vv))
            sums_ok = bool(np.isfinite(n).all() and np.isfinite(g).all())
            ok, dx, qn, shares = cholesky5(n, g)
            tr["passes"].append(dict(x=x.copy(), el=el.copy(), row=row.copy(), v=v.copy(), shares=shares, dx=dx.copy(), good=good.copy()))
            if mode == 1:
                out["rms"] = float(np.sqrt(ss / f8(n_used)))
                out["resid"], out["geo"] = vv.copy(), np.array(d["geo"])
                out["flags"] = F_RESID if out["rms"] > float(c["max_resid_m"]) else F_FIX
                mode = 2
            else:
                out["n_iter"], n_used, mask = p + 1, int(row.sum()), row.copy()
                out["n_used"], out["used_mask"] = n_used, sum(1 << int(k) for k in np.flatnonzero(row))
                if n_used < min_sats:
                    out["flags"], mode = F_TOO_FEW, 2
                elif not sums_ok:
                    out["flags"], mode = F_NONFINITE, 2
                elif not ok:
                    out["flags"], mode = F_SINGULAR, 2
                elif not np.isfinite(dx).all():
                    out["flags"], mode = F_NONFINITE, 2
                else:
                    x = x + dx
                    ms4 = f8(1000.0) * dx[4]
                    if dx[0] * dx[0] + dx[1] * dx[1] + dx[2] * dx[2] + dx[3] * dx[3] + ms4 * ms4 < 1E-8:
                        q, mode = qn, 1
                    elif p + 1 == MAX_ITER:
                        out["flags"], mode = F_NO_CONV, 2
        out["x"] = x
        if out["flags"] in (F_FIX, F_RESID):
            tow, week = f8(prior["tow_s"]) + x[4], int(prior["week"])
            if tow >= WEEK_S:
                tow, week = tow - WEEK_S, week + 1
            elif tow < 0.0:
                tow, week = tow + WEEK_S, week - 1
            qf = q.astype(np.float32)
            if (np.isfinite(x).all() and np.isfinite(tow) and 0.0 <= tow < WEEK_S and np.isfinite(out["geo"]).all() and np.isfinite(out["rms"])
                    and np.isfinite(qf).all()):
                out["tow_s"], out["week"], out["qr"] = float(tow), week, qf
            else:
                out["flags"] = F_NONFINITE
        tr["max_resid_m"] = float(c["max_resid_m"])
    return out


def snap(cfg, prns, dopp_min_hz, dopp_step_hz, peaks, bank, bank_stride, prior, want_sv=True, trace=None, tau=None):
    """gpsx_wsnap on peaks [n_rx][n_prn][n_dopp], the bank ([n_rx][n_prn] with bank_stride n_prn, [n_prn] or [1][n_prn] with 0) and
    prior [n_rx] -> (SNAP_DTYPE [n_rx], SV_DTYPE [n_rx][n_prn] or None).  tau [n_rx][n_prn]: code phases that replace the records'
    integers (fractions of a sample: what no record can hold), for the tests of the method itself.  trace (a list): per receiver the
    dict solve() fills, or None for a receiver without a prior"""
    c = np.asarray(cfg, CFG_DTYPE).reshape(1)[0]
    n_rx, n_prn, n_dopp = peaks.shape
    assert len(prns) == n_prn and bank_stride in (0, n_prn) and len(prior) == n_rx
    bank = np.asarray(bank, EPH_DTYPE).reshape(-1, n_prn)
    dcfg = dict(min_peak=int(c["min_peak"]), det_num=int(c["det_num"]), det_den=int(c["det_den"]))
    out, sv = np.zeros(n_rx, SNAP_DTYPE), np.zeros((n_rx, n_prn), SV_DTYPE)
    for r in range(n_rx):
        if not prior_ok(prior[r]):
            out[r]["flags"] = F_NO_PRIOR
            if trace is not None:
                trace.append(None)
            continue
        best = [Q.best_record(peaks[r, p]) for p in range(n_prn)]
        det = np.array([Q.detected(m, s, dcfg) for _, m, s, _ in best])
        phases = np.array([t for _, _, _, t in best], np.float64) if tau is None else np.asarray(tau[r], np.float64)
        o = solve(c, bank[r if bank_stride else 0], det, phases, prior[r], trace)
        w = out[r]
        w["flags"], w["week"], w["n_detected"], w["n_candidates"], w["n_used"], w["n_iter"] = o["flags"], o["week"], int(det.sum()), o["n_candidates"], o["n_used"], o["n_iter"]
        w["ref"], w["used_mask"], w["tow_s"] = o["ref"], o["used_mask"], o["tow_s"]
        solved = o["flags"] in (F_FIX, F_RESID)
        if solved:
            w["rr"], w["b_m"], w["dt_s"], w["geo"], w["resid_rms_m"], w["qr"] = o["x"][:3], o["x"][3], o["x"][4], o["geo"], o["rms"], o["qr"]
        for p in range(n_prn):
            used = (o["used_mask"] >> p) & 1
            s = sv[r, p]
            s["flags"] = ((SV_DETECTED if det[p] else 0) | (SV_HAVE_EPH if o["have"][p] else 0) | (SV_CANDIDATE if o["cand"][p] else 0) |
                          (SV_USED if used else 0) | (SV_REFERENCE if p == o["ref"] else 0))
            s["n_ms"], s["phase"], s["dopp_hz"] = (o["n_ms"][p] if o["ref"] >= 0 else 0), best[p][3], dopp_min_hz + best[p][0] * dopp_step_hz
            s["el"], s["az"] = o["el"][p], o["az"][p]
            s["resid_m"] = o["resid"][p] if solved and used and np.isfinite(o["resid"][p]) else 0.0
    return out, (sv if want_sv else None)


def to_fix(snap_rec):
    """gpsx_wsnap_to_fix on one record -> FIX_DTYPE item, or None without FIX"""
    if int(snap_rec["flags"]) != F_FIX:
        return None
    f = np.zeros(1, F.FIX_DTYPE)
    dtr = f8(snap_rec["b_m"]) / f8(299792458.0)
    f["flags"], f["n_used"], f["n_iter"], f["ref_slot"], f["used_mask"] = F.F_FIX, snap_rec["n_used"], snap_rec["n_iter"], snap_rec["ref"], snap_rec["used_mask"]
    f["rr"], f["dtr_s"], f["rx_tow_s"], f["geo"], f["qr"] = snap_rec["rr"], dtr, f8(snap_rec["tow_s"]) + dtr, snap_rec["geo"], snap_rec["qr"]
    f["resid_rms_m"], f["week"] = snap_rec["resid_rms_m"], snap_rec["week"]
    return f[0]
