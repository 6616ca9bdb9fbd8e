"""A CPU restatement of the weighted path's position fixes (include/gpsx.h gpsx_wfix), for the tests: the header's definition in
np.float64, every receiver of a launch at once (arrays [n_rx, ch_per_rx]; a loop that the definition runs per slot or per receiver
runs here over the whole array with a mask of the elements still in it, which gives each element what its own loop would).  Written
from the header's text and the models (IS-GPS-200 table 20-IV, Klobuchar, Saastamoinen, RTKLIB's variance terms); nothing of the
library's code is included or imported.  What is exact: the usable slots, the pseudoranges, ref_slot, rx_tow_s, week (integer and
single double operations).  What is not: everything behind a sine -- numpy's libm is not the device's -- and the sums of the normal
system, which are added here in numpy's order."""
import numpy as np

import weighted_eph_ref as E
import weighted_obs_ref as O

F_FIX, F_TOO_FEW, F_SINGULAR, F_NO_CONV, F_NONFINITE = 1, 2, 4, 8, 16
LOCK_CODE = 1
CFG_DTYPE = np.dtype([("offset_ms", "<f8"), ("ion", "<f8", (8,)), ("ch_per_rx", "<i4"), ("min_sats", "<i4"), ("reserved0", "<i4"),
                      ("reserved1", "<i4"), ("reserved2", "<i4"), ("reserved3", "<i4")])
FIX_DTYPE = np.dtype([("flags", "<u4"), ("n_used", "<i4"), ("n_iter", "<i4"), ("ref_slot", "<i4"), ("used_mask", "<u8"), ("rr", "<f8", (3,)),
                      ("dtr_s", "<f8"), ("rx_tow_s", "<f8"), ("geo", "<f8", (3,)), ("qr", "<f4", (6,)), ("resid_rms_m", "<f8"), ("week", "<i4"),
                      ("reserved", "<i4")])
LOCK_DTYPE = np.dtype([("flags", "<u4"), ("rest", "<u4", (15,))])      # gpsx_wlock_t: only its flags matter here
assert CFG_DTYPE.itemsize == 96 and FIX_DTYPE.itemsize == 128 and LOCK_DTYPE.itemsize == 64

C_LIGHT = 299792458.0
PI = 3.1415926535897932
MU = 3.9860050E14
OMEGA_E = 7.2921151467E-5
RE = 6378137.0
FE = 1.0 / 298.257223563
MAX_ITER = 10
PIVOT = 1E-10
WEEK_MS = 604_800_000
UNIX_TO_GPS = 315964800
URA = np.array([2.4, 3.4, 4.85, 6.85, 9.65, 13.65, 24.0, 48.0, 96.0, 192.0, 384.0, 768.0, 1536.0, 3072.0, 6144.0])
ION_DEFAULT = np.array([0.1118E-07, -0.7451E-08, -0.5961E-07, 0.1192E-06, 0.1167E+06, -0.2294E+06, -0.1311E+06, 0.1049E+07])


def make_cfg(offset_ms, ch_per_rx, min_sats=4, ion=None):
    cfg = np.zeros(1, CFG_DTYPE)
    cfg["offset_ms"], cfg["ch_per_rx"], cfg["min_sats"] = offset_ms, ch_per_rx, min_sats
    if ion is not None:
        cfg["ion"][0] = ion
    return cfg


def _fold(d):
    return (d + WEEK_MS // 2) % WEEK_MS - WEEK_MS // 2


def _time_add(sec, d):
    """the solver's time_add on the fraction alone: it never carries into the whole second"""
    sec = sec + d
    whole = np.floor(sec)
    sec = sec + whole
    return sec - whole


def _clock_poly(e, t):
    return e["f0"] + e["f1"] * t + e["f2"] * t * t


def _clock_bias(e, whole, sec):
    t = (whole - e["toc_time"]).astype(np.float64) + sec - e["toc_sec"]
    t = t - _clock_poly(e, t)
    t = t - _clock_poly(e, t)
    return _clock_poly(e, t)


def pseudoranges(obs, usable, offset_ms):
    """gpsx_wobs_pseudoranges over the usable slots of every receiver: obs, usable [n_rx, ch] -> (pr_m [n_rx, ch], ref_slot [n_rx],
    rx_tow_s [n_rx]), before the stage's finite rule"""
    n_rx, ch = usable.shape
    tx, ph = obs["tx_ms"].astype(np.int64), obs["code_phase_fine"].astype(np.float64)
    ref, ref_tx, ref_ph = np.full(n_rx, -1), np.zeros(n_rx, np.int64), np.zeros(n_rx)
    for k in range(ch):
        d = _fold(tx[:, k] - ref_tx).astype(np.float64) - (ph[:, k] - ref_ph) / 16368.0
        take = usable[:, k] & ((ref < 0) | (d > 0.0))
        ref[take], ref_tx[take], ref_ph[take] = k, tx[take, k], ph[take, k]
    have = ref >= 0
    pr = 299792458e-3 * (_fold(ref_tx[:, None] - tx).astype(np.float64) + (ph - ref_ph[:, None]) / 16368.0 + offset_ms)
    pr = np.where(usable & have[:, None], pr, 0.0)
    rx = (ref_tx.astype(np.float64) - ref_ph / 16368.0 + offset_ms) / 1000.0
    rx = np.where(rx >= 604800.0, rx - 604800.0, np.where(rx < 0.0, rx + 604800.0, rx))
    return pr, ref, np.where(have, rx, 0.0)


def _geodetic(x):
    """ecef2pos of x [n, 3] -> lat, lon, hgt [n]; the fixed point bounded at 30 steps"""
    e2 = FE * (2.0 - FE)
    r2 = x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]
    v, z, zk = np.full(len(x), RE), x[:, 2].copy(), np.zeros(len(x))
    for _ in range(30):
        go = np.abs(z - zk) >= 1E-4
        if not go.any():
            break
        zk = np.where(go, z, zk)
        sp = z / np.sqrt(r2 + z * z)
        vn = RE / np.sqrt(1.0 - e2 * sp * sp)
        zn = x[:, 2] + vn * e2 * sp
        v, z = np.where(go, vn, v), np.where(go, zn, z)
    far = r2 > 1E-12
    lat = np.where(far, np.arctan(z / np.sqrt(np.where(far, r2, 1.0))), np.where(x[:, 2] > 0.0, PI / 2.0, -PI / 2.0))
    lon = np.where(far, np.arctan2(x[:, 1], x[:, 0]), 0.0)
    return lat, lon, np.sqrt(r2 + z * z) - v


def _klobuchar(tow, ion, lat, lon, hgt, az, el):
    psi = 0.0137 / (el / PI + 0.11) - 0.022
    phi = lat / PI + psi * np.cos(az)
    phi = np.where(phi > 0.416, 0.416, np.where(phi < -0.416, -0.416, phi))
    lam = lon / PI + psi * np.sin(az) / np.cos(phi * PI)
    phi = phi + 0.064 * np.cos((lam - 1.617) * PI)
    tt = 43200.0 * lam + tow
    tt = tt - np.floor(tt / 86400.0) * 86400.0
    slant = 1.0 + 16.0 * np.power(0.53 - el / PI, 3.0)
    amp = ion[0] + phi * (ion[1] + phi * (ion[2] + phi * ion[3]))
    per = ion[4] + phi * (ion[5] + phi * (ion[6] + phi * ion[7]))
    amp = np.where(amp < 0.0, 0.0, amp)
    per = np.where(per < 72000.0, 72000.0, per)
    x = 2.0 * PI * (tt - 50400.0) / per
    d = C_LIGHT * slant * np.where(np.abs(x) < 1.57, 5E-9 + amp * (1.0 + x * x * (-0.5 + x * x / 24.0)), 5E-9)
    return np.where((hgt < -1E3) | (el <= 0), 0.0, d)


def _saastamoinen(lat, h, el, humidity=0.7):
    hgt = np.where(h < 0.0, 0.0, h)
    pres = 1013.25 * np.power(np.abs(1.0 - 2.2557E-5 * hgt), 5.2568)      # (the base is positive wherever the result is used)
    temp = 15.0 - 6.5E-3 * hgt + 273.16
    e = 6.108 * humidity * np.exp((17.15 * temp - 4684.0) / (temp - 38.45))
    z = PI / 2.0 - el
    dry = 0.0022768 * pres / (1.0 - 0.00266 * np.cos(2.0 * lat) - 0.00028 * hgt / 1E3) / np.cos(z)
    wet = 0.002277 * (1255.0 / temp + 0.05) * e / np.cos(z)
    return np.where((h < -100.0) | (1E4 < h) | (el <= 0), 0.0, dry + wet)


def _satellites(e, usable, whole, sec, pr):
    """every slot's satellite at its transmit time: e the records [n_rx, ch], (whole [n_rx, 1], sec [n_rx, 1]) the observation time
    -> cand (the solver has a satellite record for the slot), pos [n_rx, ch, 3], clk, var"""
    cand = usable & (np.abs((e["toe_time"] - whole).astype(np.float64) + e["toe_sec"] - sec) <= 7201.0)
    t_sec = _time_add(np.broadcast_to(sec, pr.shape), -pr / C_LIGHT)
    t_sec = _time_add(t_sec, -_clock_bias(e, whole, t_sec))
    tk = (whole - e["toe_time"]).astype(np.float64) + t_sec - e["toe_sec"]
    A, ecc_ = e["A"], e["e"]
    orbiting = cand & (A > 0.0)
    mean = e["M0"] + (np.sqrt(MU / (A * A * A)) + e["deln"]) * tk
    ecc, was, n = mean.copy(), np.zeros(mean.shape), np.zeros(mean.shape, np.int64)
    for _ in range(30):
        go = orbiting & (np.abs(ecc - was) > 1E-14) & (n < 30)
        if not go.any():
            break
        was = np.where(go, ecc, was)
        ecc = np.where(go, ecc - (ecc - ecc_ * np.sin(ecc) - mean) / (1.0 - ecc_ * np.cos(ecc)), ecc)
        n = n + go
    settled = n < 30
    se, ce = np.sin(ecc), np.cos(ecc)
    u = np.arctan2(np.sqrt(1.0 - ecc_ * ecc_) * se, ce - ecc_) + e["omg"]
    rad = A * (1.0 - ecc_ * ce)
    inc = e["i0"] + e["idot"] * tk
    s2, c2 = np.sin(2.0 * u), np.cos(2.0 * u)
    u = u + (e["cus"] * s2 + e["cuc"] * c2)
    rad = rad + (e["crs"] * s2 + e["crc"] * c2)
    inc = inc + (e["cis"] * s2 + e["cic"] * c2)
    xo, yo, ci = rad * np.cos(u), rad * np.sin(u), np.cos(inc)
    node = e["OMG0"] + (e["OMGd"] - OMEGA_E) * tk - OMEGA_E * e["toes"]
    sn, cn = np.sin(node), np.cos(node)
    pos = np.stack([xo * cn - yo * ci * sn, xo * sn + yo * ci * cn, yo * np.sin(inc)], -1)
    tc = (whole - e["toc_time"]).astype(np.float64) + t_sec - e["toc_sec"]
    clk = _clock_poly(e, tc) - 2.0 * np.sqrt(MU * A) * ecc_ * se / (C_LIGHT * C_LIGHT)
    sva = e["sva"]
    ura = np.where((sva < 0) | (sva > 14), 6144.0, URA[np.clip(sva, 0, 14)])
    clk = np.where(clk == 0.0, _clock_bias(e, whole, t_sec), clk)
    good = orbiting & settled
    pos = np.where(good[..., None], pos, 0.0)      # (A <= 0: a satellite at the centre; not settled: no satellite -- no row either way)
    return cand & (settled | ~orbiting), pos, np.where(good, clk, 0.0), np.where(good, ura * ura, 0.0)


def _rows(x, sat_ok, pos, clk, var, healthy, tgd, pr, tow, ion):
    """rescode at x [n_rx, 4] -> row [n_rx, ch], a [n_rx, ch, 4] (weighted), y (weighted), v (unweighted), geo"""
    lat, lon, hgt = _geodetic(x[:, :3])
    rn = np.sqrt(pos[..., 0] * pos[..., 0] + pos[..., 1] * pos[..., 1] + pos[..., 2] * pos[..., 2])
    row = sat_ok & ~(rn < RE)
    los = pos - x[:, None, :3]
    rng = np.sqrt(los[..., 0] * los[..., 0] + los[..., 1] * los[..., 1] + los[..., 2] * los[..., 2])
    los = los / rng[..., None]
    rho = rng + OMEGA_E * (pos[..., 0] * x[:, None, 1] - pos[..., 1] * x[:, None, 0]) / C_LIGHT
    row = row & ~(rho <= 0.0)
    sp, cp, sl, cl = (f(a)[:, None] for a in (lat, lon) for f in (np.sin, np.cos))
    east = -sl * los[..., 0] + cl * los[..., 1]
    north = -sp * cl * los[..., 0] - sp * sl * los[..., 1] + cp * los[..., 2]
    up = cp * cl * los[..., 0] + cp * sl * los[..., 1] + sp * los[..., 2]
    az = np.where(east * east + north * north < 1E-12, 0.0, np.arctan2(east, north))
    az = np.where(az < 0.0, az + 2 * PI, az)
    el = np.arcsin(up)
    above = (hgt > -RE)[:, None]
    az, el = np.where(above, az, 0.0), np.where(above, el, PI / 2.0)
    row = row & ~(el < 0.0) & healthy
    lat2, lon2, hgt2 = lat[:, None], lon[:, None], hgt[:, None]
    dion = _klobuchar(tow[:, None], ion, lat2, lon2, hgt2, az, el)
    dtrp = _saastamoinen(lat2, hgt2, el)
    v_ion = (dion * 0.5) * (dion * 0.5)
    sin_el = np.sin(el)
    v_trp = (0.3 / (sin_el + 0.1)) * (0.3 / (sin_el + 0.1))
    ev = 0.003 * 0.003
    v_meas = ev * (ev + ev / sin_el)
    v = (pr - tgd) - (rho + dion + dtrp + x[:, None, 3] - C_LIGHT * clk)
    sig = np.sqrt(v_meas + var + v_ion + v_trp)
    a = np.concatenate([-los / sig[..., None], (1.0 / sig)[..., None]], -1)
    a = np.where(row[..., None], a, 0.0)
    return row, a, np.where(row, v / sig, 0.0), np.where(row, v, 0.0), (lat, lon, hgt)


def _cholesky(N, b):
    """the 4 x 4 system by the header's factorisation: N [n, 4, 4], b [n, 4] -> pivots ok [n], dx [n, 4], the inverse's six qr [n, 6]"""
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
    dx = np.stack([m00 * y0 + m10 * y1 + m20 * y2 + m30 * y3, m11 * y1 + m21 * y2 + m31 * y3, m22 * y2 + m32 * y3, m33 * y3], -1)
    q = np.stack([m00 * m00 + m10 * m10 + m20 * m20 + m30 * m30, m11 * m11 + m21 * m21 + m31 * m31, m22 * m22 + m32 * m32,
                  m10 * m11 + m20 * m21 + m30 * m31, m21 * m22 + m31 * m32, m20 * m22 + m30 * m32], -1)
    ok = (p0 > 0.0) & (p1 > PIVOT * n(1, 1)) & (p2 > PIVOT * n(2, 2)) & (p3 > PIVOT * n(3, 3))
    return ok, dx, q


def run(cfg, obs, eph, n_rx, lock=None, prev=None):
    """gpsx_wfix on obs / eph (/ lock) [n_rx * ch_per_rx] and prev [n_rx] -> (FIX_DTYPE [n_rx], pr_m [n_rx * ch_per_rx])"""
    cfg = np.asarray(cfg, CFG_DTYPE).reshape(1)[0]
    ch, min_sats, offset_ms = int(cfg["ch_per_rx"]), int(cfg["min_sats"]), float(cfg["offset_ms"])
    ion = np.array(cfg["ion"], np.float64)
    ion = ION_DEFAULT if float((ion * ion).sum()) <= 0.0 else ion
    obs = np.ascontiguousarray(obs, O.OBS_DTYPE).reshape(n_rx, ch)
    e = np.ascontiguousarray(eph, E.EPH_DTYPE).reshape(n_rx, ch)
    out = np.zeros(n_rx, FIX_DTYPE)
    with np.errstate(all="ignore"):
        usable = ((obs["flags"] & O.F_VALID) != 0) & ((e["flags"] & E.F_VALID) != 0)
        if lock is not None:
            usable &= (np.ascontiguousarray(lock).view(LOCK_DTYPE).reshape(n_rx, ch)["flags"] & LOCK_CODE) != 0
        pr, ref, rx_tow = pseudoranges(obs, usable, offset_ms)
        time_ok = np.isfinite(rx_tow)
        rx_tow = np.where(time_ok, rx_tow, 0.0)
        pr_out = np.where(np.isfinite(pr), pr, 0.0)
        week = np.where(ref >= 0, e["week"][np.arange(n_rx), np.maximum(ref, 0)], 0).astype(np.int64)
        whole_s = np.trunc(rx_tow).astype(np.int64)
        whole = (UNIX_TO_GPS + 604800 * week + whole_s)[:, None]
        sec = (rx_tow - whole_s.astype(np.float64))[:, None]
        s = whole[:, 0] - UNIX_TO_GPS
        tow = (s - (np.trunc(s / 604800).astype(np.int64)) * 604800).astype(np.float64) + sec[:, 0]
        sat_ok, pos, clk, var = _satellites(e, usable, whole, sec, pr)
        healthy, tgd = e["svh"] == 0, C_LIGHT * e["tgd"]

        x = np.zeros((n_rx, 4))
        if prev is not None:
            prev = np.ascontiguousarray(prev, FIX_DTYPE).reshape(n_rx)
            warm = (prev["flags"] & F_FIX) != 0
            x[warm, :3] = prev["rr"][warm]
        flags = np.zeros(n_rx, np.uint32)
        mode = np.zeros(n_rx, np.int64)      # 0: iterating, 1: converged, residuals due, 2: finished
        flags[~time_ok], mode[~time_ok] = F_NONFINITE, 2
        few = time_ok & (usable.sum(1) < min_sats)
        flags[few], mode[few] = F_TOO_FEW, 2
        n_used, n_iter, mask = np.zeros(n_rx, np.int64), np.zeros(n_rx, np.int64), np.zeros((n_rx, ch), bool)
        q, rms, geo = np.zeros((n_rx, 6)), np.zeros(n_rx), np.zeros((n_rx, 3))
        for p in range(MAX_ITER + 1):
            if (mode == 2).all():
                break
            row, a, y, v, g = _rows(x, sat_ok, pos, clk, var, healthy, tgd, pr, tow, ion)
            row &= (mode != 2)[:, None]
            a, y = np.where(row[..., None], a, 0.0), np.where(row, y, 0.0)
            N = np.einsum("rci,rcj->rij", a, a)
            b = np.einsum("rci,rc->ri", a, y)
            ok, dx, qn = _cholesky(N, b)
            # the groups whose residuals were due
            due = mode == 1
            vv = np.where(row & mask, v, 0.0)
            rms[due] = np.sqrt((vv * vv).sum(1) / n_used)[due]
            for k in range(3):
                geo[due, k] = g[k][due]
            flags[due], mode[due] = F_FIX, 2
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
            flags[few], flags[nonf], flags[sing] = F_TOO_FEW, F_NONFINITE, F_SINGULAR
            mode[few | nonf | sing] = 2
            x[step] += dx[step]
            conv = step & ((dx * dx).sum(1) < 1E-8)
            q[conv] = qn[conv]
            mode[conv] = 1
            late = step & ~conv & (p + 1 == MAX_ITER)
            flags[late], mode[late] = F_NO_CONV, 2
        fixed = flags == F_FIX
        dtr = x[:, 3] / C_LIGHT
        qf = q.astype(np.float32)
        bad = fixed & ~(np.isfinite(x[:, :3]).all(1) & np.isfinite(dtr) & np.isfinite(geo).all(1) & np.isfinite(rms) & np.isfinite(qf).all(1))
        flags[bad] = F_NONFINITE
        fixed &= ~bad
    out["flags"], out["n_used"], out["n_iter"], out["ref_slot"], out["rx_tow_s"], out["week"] = flags, n_used, n_iter, ref, rx_tow, week
    out["used_mask"] = (mask.astype(np.uint64) << np.arange(ch, dtype=np.uint64)).sum(1, dtype=np.uint64)
    out["rr"][fixed], out["dtr_s"][fixed], out["geo"][fixed] = x[fixed, :3], dtr[fixed], geo[fixed]
    out["qr"][fixed], out["resid_rms_m"][fixed] = qf[fixed], rms[fixed]
    return out, pr_out.reshape(-1)
