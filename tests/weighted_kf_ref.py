"""A CPU restatement of the weighted path's navigation filter (include/gpsx.h gpsx_wkf), for the tests: the header's definition in
np.float64, every receiver of a launch at once (arrays [n_rx, ch_per_rx]).  Written from the header's text; the pieces whose definition
is gpsx_wfix's (ecef2pos, Klobuchar, Saastamoinen, the URA table) are weighted_fix_ref's; nothing of the library's code is included or
imported.  What is exact: the time base, the pseudoranges (int64 and single double operations), the candidates, the masks and the flags
of receivers whose decisions are clear of round-off.  What is not: everything behind a sine -- numpy's libm is not the device's -- and the
information sums, which are added here in numpy's order."""
import numpy as np

import weighted_eph_ref as E
import weighted_fix_ref as F
import weighted_obs_ref as O
import weighted_vel_ref as V

F_INIT, F_NOT_INIT, F_UPDATED, F_COAST, F_LOST, F_BAD, F_REPAIRED, F_REJECTED, F_STEERED = 1, 2, 4, 8, 16, 32, 64, 128, 256
S_INIT = 1
LOCK_CODE, LOCK_CARRIER = 1, 2
CFG_DTYPE = np.dtype([("ion", "<f8", (8,)), ("mps_per_hz", "<f8"), ("sig_pr_m", "<f8"), ("sig_dop_mps", "<f8"), ("gate", "<f8"), ("q_acc", "<f8"),
                      ("q_clk_f", "<f8"), ("q_clk_g", "<f8"), ("p0_pos", "<f8"), ("p0_clk", "<f8"), ("p0_vel", "<f8"), ("p0_drift", "<f8"),
                      ("ch_per_rx", "<i4"), ("max_coast", "<i4"), ("reserved", "<i4", (4,))])
STATE_DTYPE = np.dtype([("x", "<f8", (8,)), ("P", "<f8", (36,)), ("rcv_ms", "<i8"), ("week", "<i4"), ("flags", "<u4"), ("n_starved", "<u4"),
                        ("n_init", "<u4"), ("n_lost", "<u4"), ("reserved", "<u4")])
KF_DTYPE = np.dtype([("flags", "<u4"), ("n_pr", "<i4"), ("n_dop", "<i4"), ("n_starved", "<u4"), ("pr_mask", "<u8"), ("dop_mask", "<u8"),
                     ("rej_pr_mask", "<u8"), ("rej_dop_mask", "<u8"), ("plus_mask", "<u8"), ("minus_mask", "<u8"), ("rr", "<f8", (3,)),
                     ("clk_m", "<f8"), ("vel", "<f8", (3,)), ("cdrift_mps", "<f8"), ("geo", "<f8", (3,)), ("enu", "<f8", (3,)), ("sigma", "<f4", (8,)),
                     ("nis_pr", "<f8"), ("nis_dop", "<f8"), ("rcv_ms", "<i8"), ("week", "<i4"), ("reserved", "<i4")])
assert CFG_DTYPE.itemsize == 176 and STATE_DTYPE.itemsize == 384 and KF_DTYPE.itemsize == 240

C_LIGHT, MU, OMEGA_E, PIVOT, PI, RE = F.C_LIGHT, F.MU, F.OMEGA_E, F.PIVOT, F.PI, F.RE
MS = 299792.458
WEEK_MS = F.WEEK_MS
UNIX_TO_GPS = 315964800


def make_cfg(ch_per_rx, mps_per_hz=V.L1CA, sig_pr_m=3.0, sig_dop_mps=0.1, gate=5.0, q_acc=1.0, q_clk_f=0.04, q_clk_g=0.4,
             p0=(30.0, 30.0, 10.0, 500.0), max_coast=10, ion=None):
    cfg = np.zeros(1, CFG_DTYPE)
    for name, v in (("mps_per_hz", mps_per_hz), ("sig_pr_m", sig_pr_m), ("sig_dop_mps", sig_dop_mps), ("gate", gate), ("q_acc", q_acc),
                    ("q_clk_f", q_clk_f), ("q_clk_g", q_clk_g), ("p0_pos", p0[0]), ("p0_clk", p0[1]), ("p0_vel", p0[2]), ("p0_drift", p0[3]),
                    ("ch_per_rx", ch_per_rx), ("max_coast", max_coast)):
        cfg[name] = v
    if ion is not None:
        cfg["ion"][0] = ion
    return cfg


def tri(i, j):
    """the place of element (i, j) of a symmetric 8 x 8 in its upper triangle, row by row"""
    i, j = min(i, j), max(i, j)
    return i * (17 - i) // 2 + (j - i)


def full(P):
    """[n, 36] -> [n, 8, 8]"""
    out = np.zeros(P.shape[:-1] + (8, 8))
    for i in range(8):
        for j in range(8):
            out[..., i, j] = P[..., tri(i, j)]
    return out


def inverse(a):
    """the header's INV on a [n, 36] -> ok [n], the inverse [n, 36], shares [n, 8] (p_0 itself, then p_j / N_jj)"""
    a = a.copy()
    n = a.shape[0]
    m, ok, shares = np.zeros((n, 36)), np.ones(n, bool), np.zeros((n, 8))
    for j in range(8):
        njj = a[:, tri(j, j)].copy()
        p = njj.copy()
        for k in range(j):
            p = p - a[:, tri(k, j)] * a[:, tri(k, j)]
        ok &= (p > 0.0) if j == 0 else (p > PIVOT * njj)
        shares[:, j] = p if j == 0 else p / njj
        ljj = np.sqrt(p)
        a[:, tri(j, j)] = ljj
        for i in range(j + 1, 8):
            t = a[:, tri(j, i)].copy()
            for k in range(j):
                t = t - a[:, tri(k, i)] * a[:, tri(k, j)]
            a[:, tri(j, i)] = t / ljj
    for j in range(8):
        m[:, tri(j, j)] = 1.0 / a[:, tri(j, j)]
        for i in range(j + 1, 8):
            t = a[:, tri(j, i)] * m[:, tri(j, j)]
            for k in range(j + 1, i):
                t = t + a[:, tri(k, i)] * m[:, tri(j, k)]
            m[:, tri(j, i)] = -t / a[:, tri(i, i)]
    for i in range(8):
        for j in range(i, 8):
            t = m[:, tri(i, j)] * m[:, tri(j, j)]
            for k in range(j + 1, 8):
                t = t + m[:, tri(i, k)] * m[:, tri(j, k)]
            a[:, tri(i, j)] = t
    return ok, a, shares


def predict(x, P, dt, cfg):
    """step 3 on x [n, 8], P [n, 36] -> x-, P-"""
    x, Pn = x.copy(), P.copy()
    t3, t2 = dt * dt * dt / 3.0, dt * dt / 2.0
    for i in range(4):
        x[:, i] = x[:, i] + dt * x[:, 4 + i]
    for i in range(4):
        for k in range(i, 4):
            Pn[:, tri(i, k)] = (P[:, tri(i, k)] + dt * (P[:, tri(i, 4 + k)] + P[:, tri(k, 4 + i)])) + (dt * dt) * P[:, tri(4 + i, 4 + k)]
    for i in range(4):
        for k in range(4):
            Pn[:, tri(i, 4 + k)] = P[:, tri(i, 4 + k)] + dt * P[:, tri(4 + i, 4 + k)]
    qa, qf, qg = float(cfg["q_acc"]), float(cfg["q_clk_f"]), float(cfg["q_clk_g"])
    for i in range(4):
        qpp = qa * t3 if i < 3 else qf * dt + qg * t3
        qpv, qvv = (qa if i < 3 else qg) * t2, (qa if i < 3 else qg) * dt
        Pn[:, tri(i, i)] += qpp
        Pn[:, tri(i, 4 + i)] += qpv
        Pn[:, tri(4 + i, 4 + i)] += qvv
    return x, Pn


def _fold(d):
    return np.where(d > 302400.0, d - 604800.0, np.where(d < -302400.0, d + 604800.0, d))


def _poly(e, t):
    return e["f0"] + e["f1"] * t + e["f2"] * t * t


def satellites(e, tx_ms, phase, cand):
    """step 5: gpsx_wvel's step 2 at tx_ms, with the clock offset and the URA variance -> sat, ps [..., 3], vs [..., 3], rate, clk, svar,
    tk (of every candidate slot, NaN elsewhere: for the tests' margins)"""
    t_sv = (tx_ms.astype(np.float64) - phase.astype(np.float64) / 16368.0) / 1000.0
    toc = ((e["toc_time"] - UNIX_TO_GPS) % 604800).astype(np.float64) + e["toc_sec"]
    tc = _fold(t_sv - toc)
    tc = tc - _poly(e, tc)
    tc = tc - _poly(e, tc)
    t = t_sv - _poly(e, tc)
    tk = _fold(t - e["toes"])
    A, ecc_ = e["A"], e["e"]
    orbiting = cand & (np.abs(tk) <= 7201.0) & (A > 0.0)
    n0 = np.sqrt(MU / (A * A * A)) + e["deln"]
    mean = e["M0"] + n0 * tk
    ecc, was, n = mean.copy(), np.zeros(mean.shape), np.zeros(mean.shape, np.int64)
    for _ in range(30):
        go = orbiting & (np.abs(ecc - was) > 1E-14) & (n < 30)
        if not go.any():
            break
        was = np.where(go, ecc, was)
        ecc = np.where(go, ecc - (ecc - ecc_ * np.sin(ecc) - mean) / (1.0 - ecc_ * np.cos(ecc)), ecc)
        n = n + go
    sat = orbiting & (n < 30)
    se, ce = np.sin(ecc), np.cos(ecc)
    root, den = np.sqrt(1.0 - ecc_ * ecc_), 1.0 - ecc_ * ce
    u = np.arctan2(root * se, ce - ecc_) + e["omg"]
    rad = A * den
    inc = e["i0"] + e["idot"] * tk
    s2, c2 = np.sin(2.0 * u), np.cos(2.0 * u)
    ed = n0 / den
    nud = ed * root / den
    ud = nud * (1.0 + 2.0 * (e["cus"] * c2 - e["cuc"] * s2))
    rd = A * ecc_ * ed * se + 2.0 * nud * (e["crs"] * c2 - e["crc"] * s2)
    idot = e["idot"] + 2.0 * nud * (e["cis"] * c2 - e["cic"] * s2)
    od = e["OMGd"] - OMEGA_E
    u = u + (e["cus"] * s2 + e["cuc"] * c2)
    rad = rad + (e["crs"] * s2 + e["crc"] * c2)
    inc = inc + (e["cis"] * s2 + e["cic"] * c2)
    su, cu, si, ci = np.sin(u), np.cos(u), np.sin(inc), np.cos(inc)
    xo, yo = rad * cu, rad * su
    xd, yd = rd * cu - rad * ud * su, rd * su + rad * ud * cu
    node = e["OMG0"] + od * tk - OMEGA_E * e["toes"]
    sn, cn = np.sin(node), np.cos(node)
    px, py, pz = xo * cn - yo * ci * sn, xo * sn + yo * ci * cn, yo * si
    vx = xd * cn - yd * ci * sn + yo * idot * si * sn - od * py
    vy = xd * sn + yd * ci * cn - yo * idot * si * cn + od * px
    vz = yd * si + yo * idot * ci
    tcl = _fold(t - toc)
    rate = e["f1"] + 2.0 * e["f2"] * tcl - 2.0 * np.sqrt(MU * A) * ecc_ * ce * ed / (C_LIGHT * C_LIGHT)
    clk = _poly(e, tcl) - 2.0 * np.sqrt(MU * A) * ecc_ * se / (C_LIGHT * C_LIGHT)
    sva = e["sva"]
    ura = np.where((sva < 0) | (sva > 14), 6144.0, F.URA[np.clip(sva, 0, 14)])
    z = lambda a: np.where(sat, a, 0.0)      # noqa: E731
    return sat, np.stack([z(px), z(py), z(pz)], -1), np.stack([z(vx), z(vy), z(vz)], -1), z(rate), z(clk), z(ura * ura), np.where(cand, tk, np.nan)


def rows(x, rcv_ms, obs, e, k_ms, may_pr, may_dop, cfg, ion):
    """steps 5 and 6 at x- [n, 8] with tx_ms + k_ms -> dict(prow, v, sig2, h [n, ch, 3], drow, y, a [n, ch, 3], el, tk)"""
    tx = obs["tx_ms"].astype(np.int64) + k_ms
    ph = obs["code_phase_fine"]
    sat, ps, vs, rate, clk, svar, tk = satellites(e, tx, ph, may_pr | may_dop)
    lat, lon, hgt = F._geodetic(x[:, :3])
    tow = rcv_ms.astype(np.float64) / 1000.0
    los = ps - x[:, None, :3]
    rng = np.sqrt(los[..., 0] * los[..., 0] + los[..., 1] * los[..., 1] + los[..., 2] * los[..., 2])
    geom = sat & ~(rng == 0.0)
    los = los / rng[..., None]
    kk = OMEGA_E / C_LIGHT
    x0, x1 = x[:, None, 0], x[:, None, 1]
    a = np.stack([-los[..., 0] - kk * ps[..., 1], -los[..., 1] + kk * ps[..., 0], -los[..., 2]], -1)
    f = obs["if_freq_offset_hz"].astype(np.float64)
    y = float(cfg["mps_per_hz"]) * f - (los[..., 0] * vs[..., 0] + los[..., 1] * vs[..., 1] + los[..., 2] * vs[..., 2]
                                        + kk * (vs[..., 0] * x1 - vs[..., 1] * x0) - C_LIGHT * rate)
    y = y - (a[..., 0] * x[:, None, 4] + a[..., 1] * x[:, None, 5] + a[..., 2] * x[:, None, 6] + x[:, None, 7])
    drow = geom & may_dop
    rn = np.sqrt(ps[..., 0] * ps[..., 0] + ps[..., 1] * ps[..., 1] + ps[..., 2] * ps[..., 2])
    rho = rng + OMEGA_E * (ps[..., 0] * x1 - ps[..., 1] * x0) / C_LIGHT
    sp, cp, sl, cl = (fn(v)[:, None] for v in (lat, lon) for fn in (np.sin, np.cos))
    east = -sl * los[..., 0] + cl * los[..., 1]
    north = -sp * cl * los[..., 0] - sp * sl * los[..., 1] + cp * los[..., 2]
    up = cp * cl * los[..., 0] + cp * sl * los[..., 1] + sp * los[..., 2]
    az = np.where(east * east + north * north < 1E-12, 0.0, np.arctan2(east, north))
    az = np.where(az < 0.0, az + 2 * PI, az)
    el = np.arcsin(up)
    above = (hgt > -RE)[:, None]
    az, el = np.where(above, az, 0.0), np.where(above, el, PI / 2.0)
    prow = geom & may_pr & ~(rn < RE) & ~(rho <= 0.0) & ~(el < 0.0)
    pr = 299792458e-3 * (F._fold(rcv_ms[:, None] - tx).astype(np.float64) + ph.astype(np.float64) / 16368.0)
    lat2, lon2, hgt2 = lat[:, None], lon[:, None], hgt[:, None]
    dion = F._klobuchar(tow[:, None], ion, lat2, lon2, hgt2, az, el)
    dtrp = F._saastamoinen(lat2, hgt2, el)
    v_ion = (dion * 0.5) * (dion * 0.5)
    sin_el = np.sin(el)
    v_trp = (0.3 / (sin_el + 0.1)) * (0.3 / (sin_el + 0.1))
    ev = 0.003 * 0.003
    v_meas = ev * (ev + ev / sin_el)
    v = (pr - C_LIGHT * e["tgd"]) - (rho + dion + dtrp + x[:, None, 3] - C_LIGHT * clk)
    sig2 = (v_meas + svar + v_ion + v_trp) + float(cfg["sig_pr_m"]) * float(cfg["sig_pr_m"])
    return dict(prow=prow, v=v, sig2=sig2, h=-los, drow=drow, y=y, a=a, el=el, tk=tk)


def _gate_s(P, h, off, extra):
    """s = sum_i h_i (sum_j P_ij h_j) + extra over the 4 x 4 block at `off`, h [n, ch, 3] with a fourth element of 1"""
    t = []
    for i in range(4):
        t.append((P[:, None, tri(off + i, off)] * h[..., 0] + P[:, None, tri(off + i, off + 1)] * h[..., 1] + P[:, None, tri(off + i, off + 2)] * h[..., 2])
                 + P[:, None, tri(off + i, off + 3)])
    return (h[..., 0] * t[0] + h[..., 1] * t[1] + h[..., 2] * t[2] + t[3]) + extra


def _mask(b, ch):
    return (b.astype(np.uint64) << np.arange(ch, dtype=np.uint64)).sum(1, dtype=np.uint64)


def run(cfg, obs, eph, state, n_rx, n_blocks, lock=None, fix=None, vel=None, detail=None):
    """gpsx_wkf on obs / eph (/ lock) [n_rx * ch_per_rx], the states [n_rx] and fix / vel [n_rx] (or None)
    -> (KF_DTYPE [n_rx], the states after, the code: 0 or -22 when a state was BAD).  detail: a dict that receives the decisions'
    quantities (gate ratios v^2 / (gate^2 s), the rint arguments, the pivot shares, the elevations of the rows, tk of every candidate slot
    at the transmit time that counts, x+_3 as step 11 finds it, step 2's u of the receivers it initialises)"""
    c = np.asarray(cfg, CFG_DTYPE).reshape(1)[0]
    ch = int(c["ch_per_rx"])
    ion = np.array(c["ion"], np.float64)
    ion = F.ION_DEFAULT if float((ion * ion).sum()) <= 0.0 else ion
    obs = np.ascontiguousarray(obs, O.OBS_DTYPE).reshape(n_rx, ch)
    e = np.ascontiguousarray(eph, E.EPH_DTYPE).reshape(n_rx, ch)
    st = np.ascontiguousarray(state, STATE_DTYPE).reshape(n_rx).copy()
    out = np.zeros(n_rx, KF_DTYPE)
    with np.errstate(all="ignore"):
        inited = (st["flags"] & S_INIT) != 0
        bad = ((st["flags"] & ~np.uint32(S_INIT)) != 0) | (st["rcv_ms"] < 0) | (st["rcv_ms"] >= WEEK_MS) | ~np.isfinite(st["x"]).all(1) | \
            ~np.isfinite(st["P"]).all(1)
        diag = np.stack([st["P"][:, tri(i, i)] for i in range(8)], -1)
        bad |= inited & ~(diag > 0.0).all(1)
        run_ = inited & ~bad
        x, P = st["x"].copy(), st["P"].copy()
        rcv, week = st["rcv_ms"].astype(np.int64).copy(), st["week"].astype(np.int64).copy()
        n_starved, n_init, n_lost = st["n_starved"].astype(np.int64), st["n_init"].astype(np.int64), st["n_lost"].astype(np.int64)

        # ---- step 2: initialisation ----
        init, init_u = np.zeros(n_rx, bool), np.full(n_rx, np.nan)
        if fix is not None:
            fx = np.ascontiguousarray(fix, F.FIX_DTYPE).reshape(n_rx)
            cand = ~inited & ~bad & ((fx["flags"] & F.F_FIX) != 0)
            u = 1000.0 * (fx["rx_tow_s"] - fx["dtr_s"])
            m = np.rint(u)
            cand &= np.abs(m) < 9007199254740992.0
            mi = np.where(cand, m, 0.0).astype(np.int64)
            wk = fx["week"].astype(np.int64)
            over = mi >= WEEK_MS
            mi, wk = np.where(over, mi - WEEK_MS, mi), np.where(over, wk + 1, wk)
            under = mi < 0
            mi, wk = np.where(under, mi + WEEK_MS, mi), np.where(under, wk - 1, wk)
            cand &= (mi >= 0) & (mi < WEEK_MS)
            xi = np.zeros((n_rx, 8))
            xi[:, :3], xi[:, 3] = fx["rr"], MS * (m - u)
            if vel is not None:
                vl = np.ascontiguousarray(vel, V.VEL_DTYPE).reshape(n_rx)
                hv = (vl["flags"] & V.F_VEL) != 0
                xi[hv, 4:7], xi[hv, 7] = vl["vel"][hv], (C_LIGHT * vl["drift_s_s"])[hv]
            Pi = np.zeros((n_rx, 36))
            for i in range(8):
                p0 = float(c[("p0_pos", "p0_pos", "p0_pos", "p0_clk", "p0_vel", "p0_vel", "p0_vel", "p0_drift")[i]])
                Pi[:, tri(i, i)] = p0 * p0
            x[cand], P[cand], rcv[cand], week[cand] = xi[cand], Pi[cand], mi[cand], wk[cand]
            n_starved[cand] = 0
            n_init[cand] = (n_init[cand] + 1) % (1 << 32)
            init, init_u = cand, np.where(cand, u, np.nan)

        # ---- steps 1 and 3: the time base, the prediction ----
        rcv = np.where(run_, rcv + n_blocks, rcv)
        over = run_ & (rcv >= WEEK_MS)
        rcv, week = np.where(over, rcv - WEEK_MS, rcv), np.where(over, week + 1, week)
        xm, Pm = predict(x, P, float(n_blocks) * 1e-3, c)
        xm, Pm = np.where(run_[:, None], xm, x), np.where(run_[:, None], Pm, P)

        # ---- steps 4 - 7: the rows, the repair ----
        usable = run_[:, None] & ((obs["flags"] & O.F_VALID) != 0) & ((e["flags"] & E.F_VALID) != 0) & (e["svh"] == 0)
        may_pr, may_dop = usable.copy(), usable & np.isfinite(obs["if_freq_offset_hz"])
        if lock is not None:
            lf = np.ascontiguousarray(lock).view(F.LOCK_DTYPE).reshape(n_rx, ch)["flags"]
            may_pr &= (lf & LOCK_CODE) != 0
            may_dop &= (lf & LOCK_CARRIER) != 0
        r0 = rows(xm, rcv, obs, e, np.zeros((n_rx, ch), np.int64), may_pr, may_dop, c, ion)
        amb = r0["prow"] & ((obs["flags"] & O.F_AMBIGUOUS) != 0)
        q = np.rint(r0["v"] / MS)
        k_out = amb & ~(np.abs(q) <= 1.0)
        k_ms = np.where(amb & ~k_out, np.nan_to_num(q), 0.0).astype(np.int64)
        again = k_ms != 0
        r1 = rows(xm, rcv, obs, e, k_ms, may_pr, may_dop, c, ion)
        R = {k: np.where(again[..., None] if r0[k].ndim == 3 else again, r1[k], r0[k]) for k in r0}
        prow, drow, v, y = R["prow"], R["drow"], R["v"], R["y"]

        # ---- step 8: the gate ----
        gg = float(c["gate"]) * float(c["gate"])
        sd2 = float(c["sig_dop_mps"]) * float(c["sig_dop_mps"])
        hz = np.where(prow[..., None], R["h"], 0.0)
        az_ = np.where(drow[..., None], R["a"], 0.0)
        v, sig2 = np.where(prow, v, 0.0), np.where(prow, R["sig2"], 0.0)
        y = np.where(drow, y, 0.0)
        s_pr, s_dop = _gate_s(Pm, hz, 0, sig2), _gate_s(Pm, az_, 4, sd2)
        pr_ok = prow & ~k_out & np.isfinite(v) & np.isfinite(s_pr) & ~(v * v > gg * s_pr)
        dop_ok = drow & np.isfinite(y) & np.isfinite(s_dop) & ~(y * y > gg * s_dop)

        # ---- step 9: the update ----
        hp = np.concatenate([np.where(pr_ok[..., None], hz, 0.0), pr_ok[..., None].astype(np.float64)], -1)
        hd = np.concatenate([np.where(dop_ok[..., None], az_, 0.0), dop_ok[..., None].astype(np.float64)], -1)
        sp2, vp, vd = np.where(pr_ok, sig2, 1.0), np.where(pr_ok, v, 0.0), np.where(dop_ok, y, 0.0)
        info, g = np.zeros((n_rx, 36)), np.zeros((n_rx, 8))
        for i in range(4):
            for k in range(i, 4):
                info[:, tri(i, k)] = ((hp[..., i] * hp[..., k]) / sp2).sum(1)
                info[:, tri(4 + i, 4 + k)] = ((hd[..., i] * hd[..., k]) / sd2).sum(1)
            g[:, i] = ((hp[..., i] * vp) / sp2).sum(1)
            g[:, 4 + i] = ((hd[..., i] * vd) / sd2).sum(1)
        nis_pr = np.where(pr_ok, v * v / s_pr, 0.0).sum(1)
        nis_dop = np.where(dop_ok, y * y / s_dop, 0.0).sum(1)
        n_pr, n_dop = pr_ok.sum(1), dop_ok.sum(1)
        any_ = (n_pr + n_dop) > 0
        ok1, A, sh1 = inverse(Pm)
        ok2, Pp, sh2 = inverse(A + info)
        ok = ok1 & ok2
        dx = np.zeros((n_rx, 8))
        for i in range(8):
            t = Pp[:, tri(i, 0)] * g[:, 0]
            for k in range(1, 8):
                t = t + Pp[:, tri(i, k)] * g[:, k]
            dx[:, i] = t
        upd = run_ & any_
        xp, Pp = np.where(upd[:, None], xm + dx, xm), np.where(upd[:, None], Pp, Pm)

        # ---- steps 10 - 12 ----
        flags = np.where(bad, F_BAD, np.where(init, F_INIT, np.where(run_, np.where(any_, F_UPDATED, F_COAST), F_NOT_INIT))).astype(np.int64)
        n_starved = np.where(run_, np.where(n_pr == 0, (n_starved + 1) % (1 << 32), 0), n_starved)
        lost = run_ & ((any_ & ~ok) | (n_starved > int(c["max_coast"])))
        live = run_ & ~lost
        x3_pre = np.where(live, xp[:, 3], np.nan)
        up_, dn_ = live & (xp[:, 3] > MS / 2.0), live & (xp[:, 3] < -MS / 2.0)
        xp[:, 3] = np.where(up_, xp[:, 3] - MS, np.where(dn_, xp[:, 3] + MS, xp[:, 3]))
        rcv = np.where(up_, rcv - 1, np.where(dn_, rcv + 1, rcv))
        under, over = up_ & (rcv < 0), dn_ & (rcv >= WEEK_MS)
        rcv = np.where(under, rcv + WEEK_MS, np.where(over, rcv - WEEK_MS, rcv))
        week = np.where(under, week - 1, np.where(over, week + 1, week))
        plus, minus = _mask(k_ms > 0, ch), _mask(k_ms < 0, ch)
        rej_pr, rej_dop = _mask(prow & ~pr_ok, ch), _mask(drow & ~dop_ok, ch)
        flags = np.where(live & (up_ | dn_), flags | F_STEERED, flags)
        flags = np.where(live & ((plus | minus) != 0), flags | F_REPAIRED, flags)
        flags = np.where(live & ((rej_pr | rej_dop) != 0), flags | F_REJECTED, flags)
        flags = np.where(lost, F_LOST, flags)
        lat, lon, hgt = F._geodetic(xp[:, :3])
        sp, cp, sl, cl = np.sin(lat), np.cos(lat), np.sin(lon), np.cos(lon)
        enu = np.stack([-sl * xp[:, 4] + cl * xp[:, 5], -sp * cl * xp[:, 4] - sp * sl * xp[:, 5] + cp * xp[:, 6],
                        cp * cl * xp[:, 4] + cp * sl * xp[:, 5] + sp * xp[:, 6]], -1)
        sg = np.sqrt(np.stack([Pp[:, tri(i, i)] for i in range(8)], -1)).astype(np.float32)
        fin = np.isfinite(lat) & np.isfinite(lon) & np.isfinite(hgt) & np.isfinite(enu).all(1) & np.isfinite(nis_pr) & np.isfinite(nis_dop) & \
            np.isfinite(xp).all(1) & np.isfinite(sg).all(1) & np.isfinite(Pp).all(1)
        solved = (init | live) & fin
        flags = np.where(init & ~fin, F_NOT_INIT, np.where(live & ~fin, F_LOST, flags))
        lost |= live & ~fin
    out["flags"] = flags
    for name, val in (("n_pr", n_pr), ("n_dop", n_dop), ("n_starved", n_starved), ("pr_mask", _mask(pr_ok, ch)), ("dop_mask", _mask(dop_ok, ch)),
                      ("rej_pr_mask", rej_pr), ("rej_dop_mask", rej_dop), ("plus_mask", plus), ("minus_mask", minus), ("nis_pr", nis_pr),
                      ("nis_dop", nis_dop)):
        w = solved & run_
        out[name][w] = val[w]
    s = solved
    out["rr"][s], out["clk_m"][s], out["vel"][s], out["cdrift_mps"][s] = xp[s, :3], xp[s, 3], xp[s, 4:7], xp[s, 7]
    out["geo"][s], out["enu"][s], out["sigma"][s] = np.stack([lat, lon, hgt], -1)[s], enu[s], sg[s]
    out["rcv_ms"][s], out["week"][s] = rcv[s], week[s]
    st["x"][s], st["P"][s], st["rcv_ms"][s], st["week"][s] = xp[s], Pp[s], rcv[s], week[s]
    st["flags"][s], st["n_starved"][s], st["n_init"][s], st["reserved"][s] = S_INIT, n_starved[s], n_init[s], 0
    if lost.any():
        keep_init, keep_lost = st["n_init"][lost].copy(), (n_lost[lost] + 1) % (1 << 32)
        st[lost] = np.zeros(int(lost.sum()), STATE_DTYPE)
        st["n_init"][lost], st["n_lost"][lost] = keep_init, keep_lost
    if detail is not None:
        with np.errstate(all="ignore"):
            detail.update(gate_pr=np.where(prow & ~k_out, v * v / (gg * s_pr), np.nan), gate_dop=np.where(drow, y * y / (gg * s_dop), np.nan),
                          rint_arg=np.where(amb, r0["v"] / MS, np.nan), el=np.where(R["prow"] | (may_pr & ~R["prow"]), R["el"], np.nan),
                          shares=np.where((run_ & any_)[:, None], np.minimum(sh1, sh2), np.nan), pr_ok=pr_ok, dop_ok=dop_ok, prow=prow, drow=drow,
                          v=v, y=y, s_pr=s_pr, s_dop=s_dop, xm=xm, Pm=Pm, tk=R["tk"], x3_pre=x3_pre, init_u=init_u, may_pr=may_pr, may_dop=may_dop,
                          pivot_failed=run_ & any_ & ~ok, starved_out=run_ & (n_starved > int(c["max_coast"])), not_finite=(init | run_) & ~fin)
    return out, st, (-22 if bad.any() else 0)
