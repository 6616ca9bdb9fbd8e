"""A CPU restatement of the weighted path's fixes with millisecond repair and fault detection / exclusion (include/gpsx.h gpsx_wfde), for
the tests: the header's definition in np.float64 on weighted_fix_ref's functions, every receiver of a launch at once -- each receiver
sits in its own round, as the groups of a wave do, and a receiver that is finished is masked.  A round here is weighted_fix_ref.run's
body on an active set with tx_ms + k; with repair = 0 and max_excl = 0 it performs run's operations in run's order, so its records are
run's byte for byte.  Written from the header's text; nothing of the library's code is included or imported.

Beside the records it returns every decision's margin, per receiver: |T - limit| / limit of each test, the relative gap between the best
and the second-best w^2 of each exclusion, |v / L - k| of each repair (the decision flips at 0.5).  Where all of these are >= 1e-6 the
device, whose libm differs from glibc by about 1e-6 m, must take the same decisions (min_margin)."""
import numpy as np

import weighted_eph_ref as E
import weighted_fix_ref as F
import weighted_obs_ref as O

PASSED, UNCHECKED, FAULT, NOFIX, EXCLUDED, REPAIRED, UNRESOLVED = 1, 2, 4, 8, 16, 32, 64
VERDICTS = PASSED | UNCHECKED | FAULT | NOFIX
CFG_DTYPE = np.dtype([("fix", F.CFG_DTYPE), ("z_global", "<f8"), ("max_excl", "<i4"), ("repair", "<i4"), ("reserved", "<i4", (4,))])
FDE_DTYPE = np.dtype([("flags", "<u4"), ("n_rounds", "<i4"), ("n_excluded", "<i4"), ("dof", "<i4"), ("excl_mask", "<u8"), ("plus_mask", "<u8"),
                      ("minus_mask", "<u8"), ("t_stat", "<f8"), ("t_limit", "<f8"), ("reserved", "<u8")])
assert CFG_DTYPE.itemsize == 128 and FDE_DTYPE.itemsize == 64
MS_M = 299792.458      # one millisecond of range
MARGIN = 1e-6


def make_cfg(offset_ms, ch_per_rx, min_sats=4, ion=None, z_global=3.09, max_excl=2, repair=1):
    cfg = np.zeros(1, CFG_DTYPE)
    cfg["fix"] = F.make_cfg(offset_ms, ch_per_rx, min_sats, ion)
    cfg["z_global"], cfg["max_excl"], cfg["repair"] = z_global, max_excl, repair
    return cfg


def _bits(mask):
    """bool [n_rx, ch] -> uint64 [n_rx]"""
    return (mask.astype(np.uint64) << np.arange(mask.shape[1], dtype=np.uint64)).sum(1, dtype=np.uint64)


def limit(dof, z):
    """the Wilson-Hilferty chi-square quantile, in doubles as the header writes it"""
    dof = np.asarray(dof, np.float64)
    t = 1.0 - 2.0 / (9.0 * dof) + z * np.sqrt(2.0 / (9.0 * dof))
    return dof * t * t * t


def _leverage(N, a):
    """the header's factorisation of N [n, 4, 4] once more, for M = L^-1: -> pivots ok [n], h_jj = |M a_j|^2 [n, ch] for a [n, ch, 4]"""
    n = lambda i, j: N[:, i, j]      # noqa: E731
    p0 = n(0, 0)
    l00 = np.sqrt(p0)
    l10, l20, l30 = n(1, 0) / l00, n(2, 0) / l00, n(3, 0) / l00
    p1 = n(1, 1) - l10 * l10
    l11 = np.sqrt(p1)
    l21, l31 = (n(2, 1) - l20 * l10) / l11, (n(3, 1) - l30 * l10) / l11
    p2 = n(2, 2) - l20 * l20 - l21 * l21
    l22 = np.sqrt(p2)
    l32 = (n(3, 2) - l30 * l20 - l31 * l21) / l22
    p3 = n(3, 3) - l30 * l30 - l31 * l31 - l32 * l32
    l33 = np.sqrt(p3)
    m00, m11, m22, m33 = 1.0 / l00, 1.0 / l11, 1.0 / l22, 1.0 / l33
    m10 = -(l10 * m00) / l11
    m20, m21 = -(l20 * m00 + l21 * m10) / l22, -(l21 * m11) / l22
    m30, m31, m32 = -(l30 * m00 + l31 * m10 + l32 * m20) / l33, -(l31 * m11 + l32 * m21) / l33, -(l32 * m22) / l33
    c = lambda m: m[:, None]      # noqa: E731
    a0, a1, a2, a3 = (a[..., i] for i in range(4))
    h0 = c(m00) * a0
    h1 = c(m10) * a0 + c(m11) * a1
    h2 = c(m20) * a0 + c(m21) * a1 + c(m22) * a2
    h3 = c(m30) * a0 + c(m31) * a1 + c(m32) * a2 + c(m33) * a3
    ok = (p0 > 0.0) & (p1 > F.PIVOT * n(1, 1)) & (p2 > F.PIVOT * n(2, 2)) & (p3 > F.PIVOT * n(3, 3)) & np.isfinite(N).all((1, 2))
    return ok, h0 * h0 + h1 * h1 + h2 * h2 + h3 * h3


def _round(c, S, k, probe, start, go):
    """One round for the receivers of `go` (the others: finished, every mask of theirs empty): gpsx_wfix's steps 1 - 7 on the active
    set S [n_rx, ch] with tx_ms + k, started at `start` [n_rx, 3]; the slots of `probe` ride along -- their pseudorange against S's
    reference slot, their satellite, their row at every x -- and enter no sum.
    -> dict(fix: FIX_DTYPE records, pr, and from the residual pass: v, row (probes included), counted, y, T, n_counted, name_ok, w2)"""
    n_rx, ch = S.shape
    min_sats, offset_ms, ion, e = c["min_sats"], c["offset_ms"], c["ion"], c["eph"]
    S, probe = S & go[:, None], probe & go[:, None]
    live = S | probe
    obs = c["obs"].copy()
    obs["tx_ms"] = c["obs"]["tx_ms"].astype(np.int64) + k
    out = np.zeros(n_rx, F.FIX_DTYPE)
    with np.errstate(all="ignore"):
        _, ref, rx_tow = F.pseudoranges(obs, S, offset_ms)
        have = ref >= 0
        tx, ph = obs["tx_ms"].astype(np.int64), obs["code_phase_fine"].astype(np.float64)
        at = (np.arange(n_rx), np.maximum(ref, 0))
        ref_tx, ref_ph = tx[at], ph[at]
        pr = 299792458e-3 * (F._fold(ref_tx[:, None] - tx).astype(np.float64) + (ph - ref_ph[:, None]) / 16368.0 + offset_ms)
        pr = np.where(live & have[:, None], pr, 0.0)
        time_ok = np.isfinite(rx_tow)
        rx_tow = np.where(time_ok, rx_tow, 0.0)
        pr_out = np.where(np.isfinite(pr) & S, pr, 0.0)
        week = np.where(have, e["week"][at], 0).astype(np.int64)
        whole_s = np.trunc(rx_tow).astype(np.int64)
        whole = (F.UNIX_TO_GPS + 604800 * week + whole_s)[:, None]
        sec = (rx_tow - whole_s.astype(np.float64))[:, None]
        s = whole[:, 0] - F.UNIX_TO_GPS
        tow = (s - (np.trunc(s / 604800).astype(np.int64)) * 604800).astype(np.float64) + sec[:, 0]
        sat_ok, pos, clk, var = F._satellites(e, live, whole, sec, pr)
        healthy, tgd = e["svh"] == 0, F.C_LIGHT * e["tgd"]

        x = np.zeros((n_rx, 4))
        x[:, :3] = start
        flags = np.zeros(n_rx, np.uint32)
        mode = np.zeros(n_rx, np.int64)      # 0: iterating, 1: converged, residuals due, 2: finished
        mode[~go] = 2
        bad_time = go & ~time_ok
        flags[bad_time], mode[bad_time] = F.F_NONFINITE, 2
        few = go & time_ok & (S.sum(1) < min_sats)
        flags[few], mode[few] = F.F_TOO_FEW, 2
        n_used, n_iter, mask = np.zeros(n_rx, np.int64), np.zeros(n_rx, np.int64), np.zeros((n_rx, ch), bool)
        q, rms, geo = np.zeros((n_rx, 6)), np.zeros(n_rx), np.zeros((n_rx, 3))
        fin = dict(v=np.zeros((n_rx, ch)), row=np.zeros((n_rx, ch), bool), counted=np.zeros((n_rx, ch), bool), y=np.zeros((n_rx, ch)),
                   T=np.zeros(n_rx), n_counted=np.zeros(n_rx, np.int64), name_ok=np.zeros(n_rx, bool), w2=np.zeros((n_rx, ch)))
        for p in range(F.MAX_ITER + 1):
            if (mode == 2).all():
                break
            row_all, a, y, v, g = F._rows(x, sat_ok, pos, clk, var, healthy, tgd, pr, tow, ion)
            row_all &= (mode != 2)[:, None]
            row = row_all & S
            counted = row & np.where((mode == 1)[:, None], mask, True)
            a, y = np.where(counted[..., None], a, 0.0), np.where(counted, y, 0.0)
            N = np.einsum("rci,rcj->rij", a, a)
            b = np.einsum("rci,rc->ri", a, y)
            ok, dx, qn = F._cholesky(N, b)
            # the groups whose residuals were due
            due = mode == 1
            vv = np.where(counted, v, 0.0)
            rms[due] = np.sqrt((vv * vv).sum(1) / n_used)[due]
            for k3 in range(3):
                geo[due, k3] = g[k3][due]
            flags[due], mode[due] = F.F_FIX, 2
            if due.any():
                piv, h = _leverage(N, a)
                rest = 1.0 - h
                w2 = np.where(counted & (rest > 1E-10), y * y / np.where(rest > 1E-10, rest, 1.0), 0.0)
                fin["v"][due], fin["row"][due], fin["counted"][due], fin["y"][due] = v[due], row_all[due], counted[due], y[due]
                fin["T"][due], fin["n_counted"][due], fin["name_ok"][due], fin["w2"][due] = (y * y).sum(1)[due], counted.sum(1)[due], piv[due], w2[due]
            # the groups that iterate
            it = (mode == 0) & ~due
            n_iter[it] = p + 1
            n_used[it] = row.sum(1)[it]
            mask[it] = row[it]
            sums_ok = np.isfinite(N).all((1, 2)) & np.isfinite(b).all(1)
            dx_ok = np.isfinite(dx).all(1)
            few = it & (n_used < min_sats)
            nonf = it & ~few & ~sums_ok
            sing = it & ~few & sums_ok & ~ok
            nonf |= it & ~few & sums_ok & ok & ~dx_ok
            step = it & ~few & sums_ok & ok & dx_ok
            flags[few], flags[nonf], flags[sing] = F.F_TOO_FEW, F.F_NONFINITE, F.F_SINGULAR
            mode[few | nonf | sing] = 2
            x[step] += dx[step]
            conv = step & ((dx * dx).sum(1) < 1E-8)
            q[conv] = qn[conv]
            mode[conv] = 1
            late = step & ~conv & (p + 1 == F.MAX_ITER)
            flags[late], mode[late] = F.F_NO_CONV, 2
        fixed = flags == F.F_FIX
        dtr = x[:, 3] / F.C_LIGHT
        qf = q.astype(np.float32)
        bad = fixed & ~(np.isfinite(x[:, :3]).all(1) & np.isfinite(dtr) & np.isfinite(geo).all(1) & np.isfinite(rms) & np.isfinite(qf).all(1))
        flags[bad] = F.F_NONFINITE
        fixed &= ~bad
    out["flags"], out["n_used"], out["n_iter"], out["ref_slot"], out["rx_tow_s"], out["week"] = flags, n_used, n_iter, ref, rx_tow, week
    out["used_mask"] = _bits(mask)
    out["rr"][fixed], out["dtr_s"][fixed], out["geo"][fixed] = x[fixed, :3], dtr[fixed], geo[fixed]
    out["qr"][fixed], out["resid_rms_m"][fixed] = qf[fixed], rms[fixed]
    return dict(fin, fix=out, pr=pr_out)


def run(cfg, obs, eph, n_rx, lock=None, prev=None):
    """gpsx_wfde on obs / eph (/ lock) [n_rx * ch_per_rx] and prev [n_rx]
    -> (FIX_DTYPE [n_rx], FDE_DTYPE [n_rx], pr_m [n_rx * ch_per_rx], margins: per receiver dict(test=[..], gap=[..], repair=[..]))"""
    cfg = np.asarray(cfg, CFG_DTYPE).reshape(1)[0]
    fx = cfg["fix"]
    ch, min_sats = int(fx["ch_per_rx"]), int(fx["min_sats"])
    z, max_excl, repair = float(cfg["z_global"]), int(cfg["max_excl"]), int(cfg["repair"])
    ion = np.array(fx["ion"], np.float64)
    c = dict(obs=np.ascontiguousarray(obs, O.OBS_DTYPE).reshape(n_rx, ch), eph=np.ascontiguousarray(eph, E.EPH_DTYPE).reshape(n_rx, ch),
             min_sats=min_sats, offset_ms=float(fx["offset_ms"]), ion=F.ION_DEFAULT if float((ion * ion).sum()) <= 0.0 else ion)
    U = ((c["obs"]["flags"] & O.F_VALID) != 0) & ((c["eph"]["flags"] & E.F_VALID) != 0)
    if lock is not None:
        U &= (np.ascontiguousarray(lock).view(F.LOCK_DTYPE).reshape(n_rx, ch)["flags"] & F.LOCK_CODE) != 0
    A = U & ((c["obs"]["flags"] & O.F_AMBIGUOUS) != 0)
    do_repair = (repair != 0) & A.any(1) & ((U & ~A).sum(1) >= min_sats)
    modifiers = np.where(A.any(1) & ~do_repair, UNRESOLVED, 0).astype(np.uint32)
    start = np.zeros((n_rx, 3))
    if prev is not None:
        prev = np.ascontiguousarray(prev, F.FIX_DTYPE).reshape(n_rx)
        warm = (prev["flags"] & F.F_FIX) != 0
        start[warm] = prev["rr"][warm]
    k, excl = np.zeros((n_rx, ch), np.int64), np.zeros((n_rx, ch), bool)
    done = np.zeros(n_rx, bool)
    n_stat, n_rounds, dof = np.zeros(n_rx, np.int64), np.zeros(n_rx, np.int64), np.zeros(n_rx, np.int64)
    verdict = np.full(n_rx, NOFIX, np.uint32)
    t_stat, t_limit = np.zeros(n_rx), np.zeros(n_rx)
    fix, pr = np.zeros(n_rx, F.FIX_DTYPE), np.zeros((n_rx, ch))
    margins = [dict(test=[], gap=[], repair=[]) for _ in range(n_rx)]
    for rnd in range(max_excl + 2):
        if done.all():
            break
        go = ~done
        repairing = go & do_repair & (rnd == 0)
        probe = A & repairing[:, None]
        S = U & ~excl & ~probe
        res = _round(c, S, k, probe, start, go)
        fix[go], pr[go] = res["fix"][go], res["pr"][go]
        fixed = go & (res["fix"]["flags"] == F.F_FIX)
        n_rounds[go] += 1
        start[go] = np.where(fixed[go, None], res["fix"]["rr"][go], 0.0)
        for r in np.flatnonzero(go):
            if repairing[r]:
                if not fixed[r]:
                    modifiers[r] |= UNRESOLVED
                    continue
                for j in np.flatnonzero(probe[r] & res["row"][r]):
                    v = float(res["v"][r, j])
                    kd = float(np.rint(v / MS_M))
                    if not np.isfinite(v) or abs(kd) > 1.0:
                        excl[r, j] = True
                    else:
                        k[r, j] = int(kd)
                    if np.isfinite(v):
                        margins[r]["repair"].append(abs(v / MS_M - kd))
                continue
            if not fixed[r]:
                verdict[r], dof[r], t_stat[r], t_limit[r], done[r] = NOFIX, 0, 0.0, 0.0, True
                continue
            n_cnt = int(res["n_counted"][r])
            dof[r] = n_cnt - 4
            if dof[r] < 1:
                verdict[r], t_stat[r], t_limit[r], done[r] = UNCHECKED, 0.0, 0.0, True
                continue
            T = float(res["T"][r])
            t_limit[r] = float(limit(int(dof[r]), z))
            t_stat[r] = T if np.isfinite(T) else 0.0
            if np.isfinite(T):
                margins[r]["test"].append(abs(T - t_limit[r]) / t_limit[r])
            if np.isfinite(T) and T <= t_limit[r]:
                verdict[r], done[r] = PASSED, True
                continue
            w2 = np.where(np.isfinite(res["w2"][r]) & (res["w2"][r] > 0.0), res["w2"][r], 0.0)
            best = int(np.argmax(w2))      # (the first of equals: the lowest slot)
            if n_stat[r] == max_excl or n_cnt - 1 < min_sats or not res["name_ok"][r] or not w2[best] > 0.0:
                verdict[r], done[r] = FAULT, True
                continue
            second = float(np.delete(w2, best).max()) if ch > 1 else 0.0
            margins[r]["gap"].append((float(w2[best]) - second) / float(w2[best]))
            excl[r, best] = True
            n_stat[r] += 1
    assert done.all()
    fde = np.zeros(n_rx, FDE_DTYPE)
    fde["excl_mask"], fde["plus_mask"], fde["minus_mask"] = _bits(excl), _bits(k == 1), _bits(k == -1)
    fde["flags"] = verdict | modifiers | np.where(excl.any(1), EXCLUDED, 0).astype(np.uint32) | np.where((k != 0).any(1), REPAIRED, 0).astype(np.uint32)
    fde["n_rounds"], fde["n_excluded"], fde["dof"], fde["t_stat"], fde["t_limit"] = n_rounds, excl.sum(1), dof, t_stat, t_limit
    return fix, fde, pr.reshape(-1), margins


def min_margin(m):
    """the smallest distance of a receiver's decisions from flipping: its tests, its exclusions' gaps, its repairs (which flip at 0.5)"""
    return min(m["test"] + m["gap"] + [0.5 - f for f in m["repair"]] + [np.inf])
