"""CPU restatements of the two stages that close the weighted chain's loop (include/gpsx.h), for the tests.  gpsx_wbank, exact: a
launch's ephemeris records and the slots' PRNs in, the bank updated in place, the merged records and one report record per receiver
out; every decision is a Python integer, records are moved whole.  gpsx_wpred: the filter's state and the bank in, one record per
(receiver, PRN index) and per receiver out, hand-overs written into the slots' states; the header's definition in np.float64 on
weighted_kf_ref's satellite, weighted_fix_ref's models and weighted_acq_ref's hand-over state, the slot decisions in Python
integers, the two casts explicit np.float32.  What is not exact there is everything behind a sine: numpy's libm is not the device's.
Nothing of the library's kernel code is included or imported."""
import numpy as np

import weighted_acq_ref as Q
import weighted_eph_ref as E
import weighted_fix_ref as F
import weighted_kf_ref as R
import weighted_lock_ref as L
import weighted_sync_ref as Y

PRN_NONE = -2147483648                                   # GPSX_PRN_NONE
F_VALID, F_NEW = E.F_VALID, E.F_NEW
EPH_DTYPE = E.EPH_DTYPE
BANK_CFG_DTYPE = np.dtype([("ch_per_rx", "<i4"), ("reserved", "<i4", (3,))])
BANK_DTYPE = np.dtype([("stored_mask", "<u8"), ("have_mask", "<u8"), ("from_bank_mask", "<u8"), ("n_stored", "<u2"), ("n_have", "<u2"),
                       ("n_from_bank", "<u2"), ("zero", "<u2")])
assert BANK_CFG_DTYPE.itemsize == 16 and BANK_DTYPE.itemsize == 32 and EPH_DTYPE.itemsize == 256 and Y.STATE_DTYPE.itemsize == 448


def bank_cfg_record(ch_per_rx, reserved=(0, 0, 0)):
    """the library's gpsx_wbank_cfg_t as a one-element array"""
    out = np.zeros(1, BANK_CFG_DTYPE)
    out["ch_per_rx"], out["reserved"] = ch_per_rx, reserved
    return out


def empty_bank(n_rx, n_prn):
    return np.zeros((n_rx, n_prn), EPH_DTYPE)


def stored_form(rec):
    """what step 2 stores of a slot's record: every byte but flags = VALID"""
    out = np.array(rec, EPH_DTYPE)
    out["flags"] = F_VALID
    return out


def bank(ch, prns, slot_prns, eph, bank, want_out=True, trace=None):
    """gpsx_wbank on eph [n_rx * ch] (read only), the slots' PRNs slot_prns [n_rx * ch] (the sync states' loop.prn) and bank
    [n_rx][n_prn], which is changed in place -> (BANK_DTYPE [n_rx], merged EPH_DTYPE [n_rx * ch] or None).  trace (a list): per receiver
    a dict of the integers the decisions were taken on -- index [p_j or None per slot], offers [slots], winner {p: slot}, stored [p],
    refused [p: a winner older than the bank's], from_bank [slots]"""
    prns = [int(v) for v in prns]
    n_prn = len(prns)
    n_rx = len(bank)
    assert len(eph) == n_rx * ch and len(slot_prns) == n_rx * ch and bank.shape == (n_rx, n_prn) and len(set(prns)) == n_prn
    rep = np.zeros(n_rx, BANK_DTYPE)
    out = eph.copy() if want_out else None
    for r in range(n_rx):
        c0 = r * ch
        # 1 offer
        index = [prns.index(int(slot_prns[c0 + j])) if int(slot_prns[c0 + j]) in prns else None for j in range(ch)]
        valid = [(int(eph["flags"][c0 + j]) & F_VALID) != 0 for j in range(ch)]
        offers = [j for j in range(ch) if index[j] is not None and valid[j]]
        # 2 store
        winner = {}
        for j in offers:                                   # ascending slots: only a strictly greater toe_time displaces
            p = index[j]
            if p not in winner or int(eph["toe_time"][c0 + j]) > int(eph["toe_time"][c0 + winner[p]]):
                winner[p] = j
        stored, refused = [], []
        for p, j in sorted(winner.items()):
            if (int(bank["flags"][r, p]) & F_VALID) == 0 or int(eph["toe_time"][c0 + j]) >= int(bank["toe_time"][r, p]):
                bank[r, p] = stored_form(eph[c0 + j])
                stored.append(p)
            else:
                refused.append(p)
        have = [p for p in range(n_prn) if (int(bank["flags"][r, p]) & F_VALID) != 0]
        # 3 merge
        from_bank = [j for j in range(ch) if not valid[j] and index[j] is not None and index[j] in have]
        if want_out:
            for j in from_bank:
                out[c0 + j] = bank[r, index[j]]
        # 4 report
        mask = lambda bits: sum(1 << b for b in bits)       # noqa: E731
        o = rep[r]
        o["stored_mask"], o["have_mask"], o["from_bank_mask"] = mask(stored), mask(have), mask(from_bank)
        o["n_stored"], o["n_have"], o["n_from_bank"] = len(stored), len(have), len(from_bank)
        if trace is not None:
            trace.append(dict(index=index, offers=offers, winner=winner, stored=stored, refused=refused, have=have, from_bank=from_bank))
    return rep, out


# ---- gpsx_wpred ---------------------------------------------------------------------------------------------------------------------------
P_HAVE_EPH, P_PREDICTED, P_VISIBLE, P_CERTAIN, P_TRACKED, P_ASSIGNED, P_DROPPED = 1, 2, 4, 8, 16, 32, 64      # GPSX_WPRED_*
RX_PREDICTED, RX_NOT_INIT, RX_BAD, RX_ASSIGNED, RX_EVICTED, RX_FULL = 1, 2, 4, 8, 16, 32                      # GPSX_WPRED_RX_*
PRED_CFG_DTYPE = np.dtype([("ion", "<f8", (8,)), ("mps_per_hz", "<f8"), ("el_min_rad", "<f8"), ("max_sigma_m", "<f8"), ("max_sigma_hz", "<f8"),
                           ("ch_per_rx", "<i4"), ("lead_blocks", "<i4"), ("evict_after_blocks", "<i4"), ("handover", "<i4"), ("reserved", "<i4", (4,))])
PRED_DTYPE = np.dtype([("flags", "<u4"), ("slot", "<i4"), ("tx_ms", "<i8"), ("pr_m", "<f8"), ("code_phase", "<f8"), ("f_hz", "<f8"), ("el", "<f8"),
                       ("az", "<f8"), ("sigma_m", "<f4"), ("sigma_hz", "<f4")])
PRED_RX_DTYPE = np.dtype([("flags", "<u2"), ("week", "<i2"), ("t_ms", "<i4"), ("n_have", "u1"), ("n_visible", "u1"), ("n_tracked", "u1"),
                          ("n_assigned", "u1"), ("n_evicted", "u1"), ("n_dropped", "u1"), ("zero", "<u2"), ("visible_mask", "<u8"), ("have_mask", "<u8"),
                          ("assigned_mask", "<u8"), ("evicted_mask", "<u8"), ("kept_mask", "<u8"), ("free_mask", "<u8")])
assert PRED_CFG_DTYPE.itemsize == 128 and PRED_DTYPE.itemsize == 64 and PRED_RX_DTYPE.itemsize == 64
MS, C_LIGHT, OMEGA_E, RE, PI, WEEK_MS = R.MS, R.C_LIGHT, R.OMEGA_E, R.RE, R.PI, R.WEEK_MS
F32 = np.float32


def pred_cfg(ch_per_rx, mps_per_hz, el_min_rad=0.0873, max_sigma_m=300.0, max_sigma_hz=12.5, lead_blocks=0, evict_after_blocks=0, handover=1,
             ion=None):
    """the library's gpsx_wpred_cfg_t as a one-element array"""
    cfg = np.zeros(1, PRED_CFG_DTYPE)
    for name, v in (("mps_per_hz", mps_per_hz), ("el_min_rad", el_min_rad), ("max_sigma_m", max_sigma_m), ("max_sigma_hz", max_sigma_hz),
                    ("ch_per_rx", ch_per_rx), ("lead_blocks", lead_blocks), ("evict_after_blocks", evict_after_blocks), ("handover", handover)):
        cfg[name] = v
    if ion is not None:
        cfg["ion"][0] = ion
    return cfg


def epoch(st, lead_blocks):
    """steps 0 and 1 on one filter state -> (kind, T, week, x^ [8], P^ upper-left block [4, 4], P_vv [4, 4]); kind: "bad", "not_init" or "run" """
    x, P = np.array(st["x"], np.float64), np.array(st["P"], np.float64)
    flags, rcv = int(st["flags"]), int(st["rcv_ms"])
    inited = (flags & R.S_INIT) != 0
    bad = (flags & ~R.S_INIT) != 0 or rcv < 0 or rcv >= WEEK_MS or not np.isfinite(x).all() or not np.isfinite(P).all()
    bad = bad or (inited and not all(P[R.tri(i, i)] > 0.0 for i in range(8)))
    if bad or not inited:
        return ("bad" if bad else "not_init"), 0, 0, None, None, None
    T, week = rcv + int(lead_blocks), int(st["week"])
    if T >= WEEK_MS:
        T, week = T - WEEK_MS, week + 1
    dt = float(lead_blocks) * 1e-3
    xh = x.copy()
    for i in range(4):
        xh[i] = x[i] + dt * x[4 + i]
    pp, vv = np.zeros((4, 4)), np.zeros((4, 4))
    for i in range(4):
        for k in range(4):
            a, b = min(i, k), max(i, k)
            pp[i, k] = (P[R.tri(a, b)] + dt * (P[R.tri(a, 4 + b)] + P[R.tri(b, 4 + a)])) + (dt * dt) * P[R.tri(4 + a, 4 + b)]
            vv[i, k] = P[R.tri(4 + i, 4 + k)]
    return "run", T, week, xh, pp, vv


def one_pass(e, T, pr, xh, geo, ion):
    """one pass of step 2 for the records e [n] at the pseudoranges pr [n] -> dict(good, pr (the next), ps, vs, rate, los, el, az, tk, rho,
    dion, dtrp), everything [n] or [n, 3]"""
    lat, lon, hgt = geo
    tx = (float(T) - pr / MS)                    # (handed to R.satellites as tx_ms with a zero phase: t_sv = tx / 1000, the header's)
    sat, ps, vs, rate, clk, _, tk = R.satellites(e, tx, np.zeros(len(pr)), np.ones(len(pr), bool))
    los = ps - xh[None, :3]
    rng = np.sqrt(los[:, 0] * los[:, 0] + los[:, 1] * los[:, 1] + los[:, 2] * los[:, 2])
    rn = np.sqrt(ps[:, 0] * ps[:, 0] + ps[:, 1] * ps[:, 1] + ps[:, 2] * ps[:, 2])
    rho = rng + OMEGA_E * (ps[:, 0] * xh[1] - ps[:, 1] * xh[0]) / C_LIGHT
    good = sat & ~(rng == 0.0) & ~(rn < RE) & ~(rho <= 0.0)
    los = los / rng[:, None]
    sp, cp, sl, cl = np.sin(lat), np.cos(lat), np.sin(lon), np.cos(lon)
    east = -sl * los[:, 0] + cl * los[:, 1]
    north = -sp * cl * los[:, 0] - sp * sl * los[:, 1] + cp * los[:, 2]
    up = cp * cl * los[:, 0] + cp * sl * los[:, 1] + sp * los[:, 2]
    az = np.where(east * east + north * north < 1E-12, 0.0, np.arctan2(east, north))
    az = np.where(az < 0.0, az + 2 * PI, az)
    el = np.arcsin(up)
    if not hgt > -RE:
        az, el = np.zeros(len(pr)), np.full(len(pr), PI / 2.0)
    dion = F._klobuchar(float(T) / 1000.0, ion, lat, lon, hgt, az, el)
    dtrp = F._saastamoinen(lat, hgt, el)
    nxt = (rho + dion + dtrp + xh[3] - C_LIGHT * clk) + C_LIGHT * e["tgd"]
    return dict(good=good, pr=nxt, ps=ps, vs=vs, rate=rate, los=los, el=el, az=az, tk=tk, rho=rho, dion=dion, dtrp=dtrp)


def _quad(M, h):
    """sum_i h_i (sum_j M_ij h_j) over a 4 x 4 block with h [n, 3] and a fourth element of 1, in gpsx_wkf step 8's order"""
    t = [(M[i, 0] * h[:, 0] + M[i, 1] * h[:, 1] + M[i, 2] * h[:, 2]) + M[i, 3] for i in range(4)]
    return h[:, 0] * t[0] + h[:, 1] * t[1] + h[:, 2] * t[2] + t[3]


def predict(cfg, prns, kf_state, bank, sync, lock=None, nav=None, obs=None, eph=None, want_pred=True, trace=None):
    """gpsx_wpred on the filter states [n_rx], the bank [n_rx][n_prn] (both read only) and the slots' states [n_rx * ch_per_rx] (lock ..
    eph: None for a NULL pointer), which are changed in place -> (PRED_RX_DTYPE [n_rx], PRED_DTYPE [n_rx][n_prn] or None).  trace (a
    list): per receiver a dict -- kind, and for a receiver that runs: T, xh, the three passes' dicts, u, q, s_pr, s_f [n_prn], candidates
    [PRN indices in rank order], holds / evicted / kept / free [slots, before the call], assigned {PRN index: slot}, written [slots]"""
    c = np.asarray(cfg, PRED_CFG_DTYPE).reshape(1)[0]
    ch, lead, evict, hand = int(c["ch_per_rx"]), int(c["lead_blocks"]), int(c["evict_after_blocks"]), int(c["handover"]) != 0
    mps = float(c["mps_per_hz"])
    ion = np.array(c["ion"], np.float64)
    ion = F.ION_DEFAULT if float((ion * ion).sum()) <= 0.0 else ion
    prns = [int(v) for v in prns]
    n_prn, n_rx = len(prns), len(kf_state)
    assert bank.shape == (n_rx, n_prn) and len(sync) == n_rx * ch and (evict == 0 or lock is not None)
    rx = np.zeros(n_rx, PRED_RX_DTYPE)
    pred = np.zeros((n_rx, n_prn), PRED_DTYPE)
    for r in range(n_rx):
        kind, T, week, xh, pp, vv = epoch(kf_state[r], lead)
        if kind != "run":
            rx[r]["flags"] = RX_BAD if kind == "bad" else RX_NOT_INIT
            if trace is not None:
                trace.append(dict(kind=kind))
            continue
        c0 = r * ch
        e = bank[r]
        with np.errstate(all="ignore"):
            geo = tuple(float(v[0]) for v in F._geodetic(xh[None, :3]))
            have = (e["flags"] & F_VALID) != 0
            good = have & (e["svh"] == 0)
            pr = np.full(n_prn, 72.0 * MS)
            passes = []
            for _ in range(3):
                d = one_pass(e, T, pr, xh, geo, ion)
                good = good & d["good"]
                pr = np.where(good, d["pr"], pr)
                passes.append(d)
            d = passes[-1]
            los, ps, vs = d["los"], d["ps"], d["vs"]
            u = pr / MS
            q = np.floor(u)
            code_phase = (u - q) * 16368.0
            kk = OMEGA_E / C_LIGHT
            a = np.stack([-los[:, 0] - kk * ps[:, 1], -los[:, 1] + kk * ps[:, 0], -los[:, 2]], -1)
            f_hz = ((a[:, 0] * xh[4] + a[:, 1] * xh[5] + a[:, 2] * xh[6] + xh[7]) +
                    (los[:, 0] * vs[:, 0] + los[:, 1] * vs[:, 1] + los[:, 2] * vs[:, 2] + kk * (vs[:, 0] * xh[1] - vs[:, 1] * xh[0]) - C_LIGHT * d["rate"])) / mps
            s_pr = _quad(pp, -los)
            s_f = _quad(vv, a) / (mps * mps)
            sig_m, sig_hz = np.sqrt(s_pr).astype(F32), np.sqrt(s_f).astype(F32)
            el, az = d["el"], d["az"]
            predicted = good & np.isfinite(pr) & np.isfinite(code_phase) & np.isfinite(f_hz) & np.isfinite(el) & np.isfinite(az) & np.isfinite(s_pr) & \
                np.isfinite(s_f) & np.isfinite(sig_m) & np.isfinite(sig_hz) & (np.abs(q) < 4503599627370496.0)
            visible = predicted & (el >= float(c["el_min_rad"]))
            certain = predicted & (s_pr <= float(c["max_sigma_m"]) * float(c["max_sigma_m"])) & (s_f <= float(c["max_sigma_hz"]) * float(c["max_sigma_hz"]))
        # 5 slots, 6 candidates: integers
        holds = [j for j in range(ch) if int(sync["loop"]["prn"][c0 + j]) != PRN_NONE]
        evicted = [j for j in holds if evict > 0 and (int(lock["flags"][c0 + j]) & L.F_CODE) == 0 and int(lock["blocks_seen"][c0 + j]) >= evict]
        kept = [j for j in holds if j not in evicted]
        free = [j for j in range(ch) if j not in kept]
        kept_prns = {int(sync["loop"]["prn"][c0 + j]) for j in kept}
        tracked = [p for p in range(n_prn) if prns[p] in kept_prns]
        cands = sorted((p for p in range(n_prn) if visible[p] and certain[p] and p not in tracked), key=lambda p: (-float(el[p]), p))
        assigned = dict(zip(cands, free)) if hand else {}
        dropped = cands[len(free):] if hand else []
        written = sorted(set(assigned.values()) | set(evicted)) if hand else []
        for j in written:
            who = [p for p, slot in assigned.items() if slot == j]
            if who:
                sync[c0 + j] = Q.handover_state(prns[who[0]], F32(code_phase[who[0]]), F32(f_hz[who[0]]))
            else:
                sync[c0 + j] = Q.handover_state(PRN_NONE)
            for other in (lock, nav, obs, eph):
                if other is not None:
                    other[c0 + j] = np.zeros(1, other.dtype)[0]
        mask = lambda bits: sum(1 << int(b) for b in bits)       # noqa: E731
        o = rx[r]
        o["flags"] = RX_PREDICTED | (RX_ASSIGNED if assigned else 0) | (RX_EVICTED if evicted else 0) | (RX_FULL if dropped else 0)
        o["week"], o["t_ms"] = week, T
        o["n_have"], o["n_visible"], o["n_tracked"] = int(have.sum()), int(visible.sum()), len(tracked)
        o["n_assigned"], o["n_evicted"], o["n_dropped"] = len(assigned), len(evicted), len(dropped)
        o["visible_mask"], o["have_mask"] = mask(np.flatnonzero(visible)), mask(np.flatnonzero(have))
        o["assigned_mask"], o["evicted_mask"], o["kept_mask"] = mask(assigned.values()), mask(evicted), mask(kept)
        o["free_mask"] = mask(j for j in free if j not in assigned.values())
        for p in range(n_prn):
            w = pred[r, p]
            w["flags"] = ((P_HAVE_EPH if have[p] else 0) | (P_PREDICTED if predicted[p] else 0) | (P_VISIBLE if visible[p] else 0) |
                          (P_CERTAIN if certain[p] else 0) | (P_TRACKED if p in tracked else 0) | (P_ASSIGNED if p in assigned else 0) |
                          (P_DROPPED if p in dropped else 0))
            w["slot"] = assigned.get(p, -1)
            if predicted[p]:
                w["tx_ms"] = (T - int(q[p])) % WEEK_MS
                w["pr_m"], w["code_phase"], w["f_hz"], w["el"], w["az"], w["sigma_m"], w["sigma_hz"] = pr[p], code_phase[p], f_hz[p], el[p], az[p], sig_m[p], sig_hz[p]
        if trace is not None:
            trace.append(dict(kind=kind, T=T, week=week, xh=xh, pp=pp, vv=vv, passes=passes, good=good, u=u, q=q, s_pr=s_pr, s_f=s_f, el=el, predicted=predicted,
                              visible=visible, certain=certain, candidates=cands, holds=holds, evicted=evicted, kept=kept, free=free, tracked=tracked,
                              assigned=assigned, dropped=dropped, written=written))
    return rx, (pred if want_pred else None)
