"""A CPU restatement of the weighted path's velocity fixes (include/gpsx.h gpsx_wvel), for the tests: the header's definition in
np.float64, every receiver of a launch at once (arrays [n_rx, ch_per_rx]; Kepler's loop runs over the whole array with a mask of the
elements still in it).  Written from the header's text and IS-GPS-200 table 20-IV; nothing of the library's code is included or
imported.  What is exact: the candidates, the rows, the masks and the flags of receivers whose decisions are clear of round-off.  What is
not: everything behind a sine -- numpy's libm is not the device's -- and the sums of the normal system, which are added here in numpy's
order."""
import numpy as np

import weighted_eph_ref as E
import weighted_fix_ref as F
import weighted_obs_ref as O

F_VEL, F_NO_FIX, F_TOO_FEW, F_SINGULAR, F_NONFINITE = 1, 2, 4, 8, 16
LOCK_CARRIER = 2
L1CA = -0.19029367279836487      # GPSX_WVEL_L1CA
L1CA_WLOOP = L1CA * 1022.0 / 1023.0      # GPSX_WVEL_L1CA_WLOOP: the weighted loops rest at fd (1 + 1/1022)
CFG_DTYPE = np.dtype([("mps_per_hz", "<f8"), ("ch_per_rx", "<i4"), ("min_sats", "<i4"), ("reserved", "<i4", (4,))])
VEL_DTYPE = np.dtype([("flags", "<u4"), ("n_used", "<i4"), ("used_mask", "<u8"), ("vel", "<f8", (3,)), ("drift_s_s", "<f8"), ("enu", "<f8", (3,)),
                      ("qv", "<f4", (6,)), ("resid_rms_mps", "<f8"), ("reserved", "<u8")])
assert CFG_DTYPE.itemsize == 32 and VEL_DTYPE.itemsize == 112 and abs(L1CA + 299792458.0 / 1575.42e6) < 1e-16

C_LIGHT, MU, OMEGA_E, PIVOT = F.C_LIGHT, F.MU, F.OMEGA_E, F.PIVOT
UNIX_TO_GPS = 315964800


def make_cfg(ch_per_rx, min_sats=4, mps_per_hz=L1CA):
    cfg = np.zeros(1, CFG_DTYPE)
    cfg["mps_per_hz"], cfg["ch_per_rx"], cfg["min_sats"] = mps_per_hz, ch_per_rx, min_sats
    return cfg


def _fold(d):
    return np.where(d > 302400.0, d - 604800.0, np.where(d < -302400.0, d + 604800.0, d))


def _poly(e, t):
    return e["f0"] + e["f1"] * t + e["f2"] * t * t


def satellites(e, obs, cand):
    """step 2 on records e and observables obs of any one shape, cand the slots to evaluate
    -> sat (the slot has a satellite), pos [..., 3], vel [..., 3], the clock rate, t (the transmit time in GPS time, s of week)"""
    t_sv = (obs["tx_ms"].astype(np.float64) - obs["code_phase_fine"].astype(np.float64) / 16368.0) / 1000.0
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
    rate = e["f1"] + 2.0 * e["f2"] * _fold(t - toc) - 2.0 * np.sqrt(MU * A) * ecc_ * ce * ed / (C_LIGHT * C_LIGHT)
    z = lambda a: np.where(sat, a, 0.0)      # noqa: E731
    return sat, np.stack([z(px), z(py), z(pz)], -1), np.stack([z(vx), z(vy), z(vz)], -1), z(rate), t


def _cholesky(N, b):
    """step 4's factorisation, once: N [n, 4, 4], b [n, 4] -> ok [n] (the pivot rule on p_k and N_kk, as the kernel has it), x [n, 4], the
    inverse's six qv [n, 6], shares [n, 4] (p_0 itself, then the same p_k over N_kk: what the tests hold the margins to)"""
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
    y0 = m00 * b[:, 0]
    y1 = m10 * b[:, 0] + m11 * b[:, 1]
    y2 = m20 * b[:, 0] + m21 * b[:, 1] + m22 * b[:, 2]
    y3 = m30 * b[:, 0] + m31 * b[:, 1] + m32 * b[:, 2] + m33 * b[:, 3]
    x = np.stack([m00 * y0 + m10 * y1 + m20 * y2 + m30 * y3, m11 * y1 + m21 * y2 + m31 * y3, m22 * y2 + m32 * y3, m33 * y3], -1)
    q = np.stack([m00 * m00 + m10 * m10 + m20 * m20 + m30 * m30, m11 * m11 + m21 * m21 + m31 * m31, m22 * m22 + m32 * m32,
                  m10 * m11 + m20 * m21 + m30 * m31, m21 * m22 + m31 * m32, m20 * m22 + m30 * m32], -1)
    ok = (p0 > 0.0) & (p1 > PIVOT * n(1, 1)) & (p2 > PIVOT * n(2, 2)) & (p3 > PIVOT * n(3, 3))
    return ok, x, q, np.stack([p0, p1 / n(1, 1), p2 / n(2, 2), p3 / n(3, 3)], -1)


def system(cfg, obs, eph, fix, n_rx, lock=None):
    """steps 1 - 4 up to the sums -> dict(fixed [n_rx], row [n_rx, ch], a [n_rx, ch, 4], y [n_rx, ch], wild [n_rx], N, b, pivots [n_rx, 4]
    (p_k / N_kk; p_0 itself), x [n_rx, 4], q [n_rx, 6], ok [n_rx])"""
    cfg = np.asarray(cfg, CFG_DTYPE).reshape(1)[0]
    ch = int(cfg["ch_per_rx"])
    obs = np.ascontiguousarray(obs, O.OBS_DTYPE).reshape(n_rx, ch)
    e = np.ascontiguousarray(eph, E.EPH_DTYPE).reshape(n_rx, ch)
    fix = np.ascontiguousarray(fix, F.FIX_DTYPE).reshape(n_rx)
    fixed = (fix["flags"] & F.F_FIX) != 0
    in_mask = ((fix["used_mask"][:, None] >> np.arange(ch, dtype=np.uint64)[None, :]) & np.uint64(1)) != 0
    cand = fixed[:, None] & in_mask & ((obs["flags"] & O.F_VALID) != 0) & ((e["flags"] & E.F_VALID) != 0) & (e["svh"] == 0)
    cand &= np.isfinite(obs["if_freq_offset_hz"])
    if lock is not None:
        cand &= (np.ascontiguousarray(lock).view(F.LOCK_DTYPE).reshape(n_rx, ch)["flags"] & LOCK_CARRIER) != 0
    sat, ps, vs, rate, _ = satellites(e, obs, cand)
    rr = np.where(fixed[:, None], fix["rr"], 0.0)[:, None, :]
    los = ps - rr
    sq = los[..., 0] * los[..., 0] + los[..., 1] * los[..., 1] + los[..., 2] * los[..., 2]
    rho = np.sqrt(sq)
    row = sat & ~(rho == 0.0)
    wild = (row & ~np.isfinite(sq)).any(1)
    los = los / rho[..., None]
    k = OMEGA_E / C_LIGHT
    f = obs["if_freq_offset_hz"].astype(np.float64)
    y = float(cfg["mps_per_hz"]) * f - (los[..., 0] * vs[..., 0] + los[..., 1] * vs[..., 1] + los[..., 2] * vs[..., 2]
                                        + k * (vs[..., 0] * rr[..., 1] - vs[..., 1] * rr[..., 0]) - C_LIGHT * rate)
    a = np.stack([-los[..., 0] - k * ps[..., 1], -los[..., 1] + k * ps[..., 0], -los[..., 2], np.ones(rho.shape)], -1)
    a, y = np.where(row[..., None], a, 0.0), np.where(row, y, 0.0)
    N = np.einsum("rci,rcj->rij", a, a)
    b = np.einsum("rci,rc->ri", a, y)
    ok, x, q, L = _cholesky(N, b)
    return dict(fixed=fixed, row=row, a=a, y=y, wild=wild, N=N, b=b, pivots=L, x=x, q=q, ok=ok, geo=fix["geo"])


def run(cfg, obs, eph, fix, n_rx, lock=None):
    """gpsx_wvel on obs / eph (/ lock) [n_rx * ch_per_rx] and fix [n_rx] -> VEL_DTYPE [n_rx]"""
    c = np.asarray(cfg, CFG_DTYPE).reshape(1)[0]
    ch, min_sats = int(c["ch_per_rx"]), int(c["min_sats"])
    out = np.zeros(n_rx, VEL_DTYPE)
    with np.errstate(all="ignore"):
        s = system(cfg, obs, eph, fix, n_rx, lock)
        row, x = s["row"], s["x"]
        n_used = row.sum(1)
        v = np.where(row, s["y"] - np.einsum("rci,ri->rc", s["a"], x), 0.0)
        rms = np.sqrt((v * v).sum(1) / n_used)
        lat, lon = np.where(s["fixed"], s["geo"][:, 0], 0.0), np.where(s["fixed"], s["geo"][:, 1], 0.0)
        sp, cp, sl, cl = np.sin(lat), np.cos(lat), np.sin(lon), np.cos(lon)
        enu = np.stack([-sl * x[:, 0] + cl * x[:, 1], -sp * cl * x[:, 0] - sp * sl * x[:, 1] + cp * x[:, 2],
                        cp * cl * x[:, 0] + cp * sl * x[:, 1] + sp * x[:, 2]], -1)
        drift = x[:, 3] / C_LIGHT
        qf = s["q"].astype(np.float32)
        sums_ok = ~s["wild"] & np.isfinite(s["N"]).all((1, 2)) & np.isfinite(s["b"]).all(1)
        res_ok = np.isfinite(x).all(1) & np.isfinite(drift) & np.isfinite(enu).all(1) & np.isfinite(rms) & np.isfinite(qf).all(1)
    flags = np.where(~s["fixed"], F_NO_FIX, np.where(n_used < min_sats, F_TOO_FEW, np.where(~sums_ok, F_NONFINITE, np.where(
        ~s["ok"], F_SINGULAR, np.where(~res_ok, F_NONFINITE, F_VEL))))).astype(np.uint32)
    good = flags == F_VEL
    out["flags"], out["n_used"] = flags, n_used
    out["used_mask"] = (row.astype(np.uint64) << np.arange(ch, dtype=np.uint64)).sum(1, dtype=np.uint64)
    out["vel"][good], out["drift_s_s"][good], out["enu"][good] = x[good, :3], drift[good], enu[good]
    out["qv"][good], out["resid_rms_mps"][good] = qf[good], rms[good]
    return out
