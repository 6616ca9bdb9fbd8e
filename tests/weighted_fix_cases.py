"""What the CPU and GPU tests of the weighted chain's position fixes share (include/gpsx.h gpsx_wfix): receivers at a handful of sites
under skies of 4 to 12 satellites, their gpsx_wobs_t / gpsx_weph_t records built on the CPU in milliseconds (no IF stream), the glue to
the library's four-satellite pntpos, and the bounds.  Test infrastructure; nothing here is product code.

A sky is the union of pvt_chain.pick_satellites(rx, tow, 4, seed) over consecutive seeds, `sat` renumbered (that function is only ever
called with n = 4: its azimuth rule makes larger n take minutes).  An ephemeris record is weighted_eph_ref.decode of
pvt_chain.subframe_payloads of the quantised row: what gpsx_weph gives for that broadcast.  An observable is the transmit time on the
satellite's clock of what arrives at t_rx: T = 1000 (t_rx - tau + dts) ms, tx_ms = ceil(T), code_phase_fine = float32((tx_ms - T) 16368)."""
import ctypes as C
import functools
import math

import numpy as np

import pvt_chain as pc
import weighted_eph_ref as E
import weighted_fix_ref as F
import weighted_obs_ref as O
from pvt_types import CLIGHT, UNIX2GPS, Eph, GTime, Nav, Obsd, Sol, geodetic_to_ecef

MUNICH = (48.1374, 11.5755, 520.0)      # weighted_pvt_cases' receiver
SITES = {"munich": MUNICH, "sydney": (-33.8688, 151.2093, 58.0), "taveuni": (-16.85, 179.95, 20.0), "quito": (-0.18, -78.47, 2850.0)}
# (the southern hemisphere, the date line, the equator at 2850 m)
SEEDS = tuple(s for s in range(29, 99) if s != 56)      # every one checked at every site: pick_satellites returns within 0.25 s
TOW = 388800 + 30 * 37 + 25.0
OFFSET_MS = 68.802
OBS_FLAGS = O.F_PHASE | O.F_EDGE | O.F_TOW | O.F_CONFIRMED | O.F_VALID


def site_ecef(name):
    return geodetic_to_ecef(*SITES[name])


@functools.lru_cache(maxsize=None)
def sky(site, n_sats, seed0):
    """n_sats satellites above `site`: the quartets of SEEDS[seed0], SEEDS[seed0 + 1], ... (the index wraps) one after the other,
    renumbered 1 .. n_sats -> ((raw integers, quantised row), ...)"""
    rx, out, seed = site_ecef(site), [], seed0
    while len(out) < n_sats:
        for raw, row in pc.pick_satellites(rx, TOW, 4, seed=SEEDS[seed % len(SEEDS)]):
            if len(out) < n_sats:
                out.append((raw, dict(row, sat=len(out) + 1)))
        seed += 1
    return tuple(out)


def eph_record(raw, tow1=None):
    """the VALID gpsx_weph_t of one broadcast: decode of the three subframes' payloads (tow1: subframe 1's HOW count)"""
    pay = pc.subframe_payloads(raw)
    words = [[int("".join(str(b) for b in w), 2) for w in pay[k]] for k in (1, 2, 3)]
    rec = np.zeros(1, E.EPH_DTYPE)
    for k, v in E.decode(words, int(TOW // 6) - 4 if tow1 is None else tow1).items():
        rec[k] = v
    rec["flags"], rec["n_sets"], rec["have"] = E.F_VALID, 1, 7
    return rec


def observable(row, rx, t_rx, noise_m=0.0):
    """the VALID gpsx_wobs_t of one satellite at the receiver instant t_rx (seconds of the week)"""
    tau, dts, _ = pc.travel_time(row, rx, np.array([t_rx]))
    T = 1000.0 * (t_rx - (float(tau[0]) + noise_m / CLIGHT) + float(dts[0]))
    tx_ms = math.ceil(T)
    o = np.zeros(1, O.OBS_DTYPE)
    o["tx_ms"], o["code_phase_fine"], o["flags"] = tx_ms, np.float32((tx_ms - T) * 16368.0), OBS_FLAGS
    return o


@functools.lru_cache(maxsize=None)
def _receiver(site, n_sats, seed0):
    rx = site_ecef(site)
    sats = sky(site, n_sats, seed0)
    obs = np.concatenate([observable(row, rx, TOW) for _, row in sats])
    eph = np.concatenate([eph_record(raw) for raw, _ in sats])
    return obs, eph


def receiver(site, n_sats, seed0=0, noise=None):
    """(observables [n_sats], ephemeris records [n_sats]) of a receiver at `site`; noise: metres added to each pseudorange"""
    obs, eph = (a.copy() for a in _receiver(site, n_sats, seed0))
    if noise is not None:
        rx = site_ecef(site)
        obs = np.concatenate([observable(row, rx, TOW, float(m)) for (_, row), m in zip(sky(site, n_sats, seed0), noise)])
    return obs, eph


def pack(receivers, ch_per_rx):
    """[(obs [n], eph [n])] -> the launch's arrays [n_rx * ch_per_rx], each receiver's records in its first slots, the rest zero"""
    obs, eph = np.zeros((len(receivers), ch_per_rx), O.OBS_DTYPE), np.zeros((len(receivers), ch_per_rx), E.EPH_DTYPE)
    for r, (o, e) in enumerate(receivers):
        obs[r, :len(o)], eph[r, :len(e)] = o, e
    return obs.reshape(-1), eph.reshape(-1)


# ---- the library's own four-satellite path: gpsx_wobs_pseudoranges + gpsx_weph_to_eph + pntpos -----------------------------------------
def pntpos_fix(lib, obs, eph, offset_ms, start=None):
    """weighted_pvt_cases.position's glue with a start point -> dict(rr, dtr, qr, rx_tow_s, pr) or None when pntpos finds no fix"""
    from stm32f4_sdr_gps_amd import capi
    lib.pntpos.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.pntpos.restype = C.c_int
    lib.gpsx_wobs_pseudoranges.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.POINTER(C.c_double)]
    lib.gpsx_weph_to_eph.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    obs, eph = np.ascontiguousarray(obs, O.OBS_DTYPE), np.ascontiguousarray(eph, E.EPH_DTYPE)
    n = len(obs)
    assert 1 <= n <= 4
    pr, rx = np.zeros(n), C.c_double(0.0)
    assert lib.gpsx_wobs_pseudoranges(obs.ctypes.data, n, float(offset_ms), pr.ctypes.data, C.byref(rx)) == n
    ephs, nav = np.zeros(n, capi.EPH_DTYPE), Nav()
    nav.n = n
    for k in range(n):
        assert lib.gpsx_weph_to_eph(eph[k:k + 1].ctypes.data, k + 1, ephs[k:k + 1].ctypes.data) == 0
        nav.eph[k] = C.cast(ephs[k:k + 1].ctypes.data, C.POINTER(Eph))
    whole, od = int(rx.value), (Obsd * n)()
    for k in range(n):
        od[k].time = GTime(UNIX2GPS + 604800 * int(ephs["week"][0]) + whole, rx.value - whole)
        od[k].sat, od[k].rcv, od[k].code[0], od[k].P[0] = k + 1, 1, 1, float(pr[k])
    sol = Sol()
    if start is not None:
        sol.rr[0], sol.rr[1], sol.rr[2] = (float(v) for v in start)
    if lib.pntpos(od, n, C.byref(nav), C.byref(sol)) != 1:
        return None
    return dict(rr=np.array(list(sol.rr)[:3]), dtr=float(sol.dtr[0]), qr=np.array(list(sol.qr), np.float32), rx_tow_s=rx.value, pr=pr)


# ---- scenarios --------------------------------------------------------------------------------------------------------------------
GDOP_MAX = 20.0


def gdop(site, sats):
    """the geometric dilution of precision of `sats` at `site`, from the true geometry: sqrt(trace((H^T H)^-1)), H's rows (-los, 1)"""
    rx = site_ecef(site)
    los = np.stack([pc.sat_state(row, np.array([TOW - 0.07]))[0][0] - rx for _, row in sats])
    H = np.concatenate([-los / np.linalg.norm(los, axis=1, keepdims=True), np.ones((len(sats), 1))], 1)
    return float(np.sqrt(np.trace(np.linalg.inv(H.T @ H))))


@functools.lru_cache(maxsize=None)
def quartets(n=32):
    """n four-satellite receivers: the sites in turn, a seed of their own each; a quartet whose GDOP exceeds GDOP_MAX is passed over.
    Why: test (a) holds two eliminations of one normal system to 1e-6 m, and their round-off grows with the system's condition number,
    about GDOP^2 -- at a GDOP of several hundred (four satellites can nearly share a cone) it is micrometres for any pair of correct
    solvers, and a receiver would refuse such a sky anyway.  The rule looks at the true geometry alone, not at either solver."""
    names, out, k = sorted(SITES), [], 0
    while len(out) < n:
        site = names[k % len(names)]
        if gdop(site, sky(site, 4, k)) <= GDOP_MAX:
            out.append((site, k))
        k += 1
    return tuple(out)


def big_skies(n_sats, n=10):
    """n receivers under n_sats satellites: the sites in turn"""
    names = sorted(SITES)
    return [(names[k % len(names)], 3 * k) for k in range(n)]


NOISE_SEED, NOISE_M, NOISE_RX = 2024, 3.0, 64


def noisy(n_rx=NOISE_RX):
    """n_rx twelve-satellite receivers with seeded Gaussian pseudorange noise of NOISE_M metres -> [(site, obs, eph)]"""
    rng = np.random.default_rng(NOISE_SEED)
    names = sorted(SITES)
    return [(names[k % len(names)],) + receiver(names[k % len(names)], 12, 3 * k + 2, noise=rng.normal(0.0, NOISE_M, 12)) for k in range(n_rx)]


# ---- the GPU tests' launches: slot mixes and receivers that cannot be fixed -------------------------------------------------------------
SHAPES_CH, SHAPES_RX = (1, 3, 4, 5, 8, 12, 33, 64), (1, 2, 17, 67)
KINDS = ("clean", "obs_invalid", "eph_invalid", "zero_pair", "unhealthy", "below_horizon", "a_zero", "toe_far", "lock_masked", "duplicate",
         "nan_element", "first_and_last")


@functools.lru_cache(maxsize=None)
def _below_horizon(site):
    """(observable, record) of a satellite that `site` has below its horizon: one of the antipodal sky's, with the observable its
    signal would give if the earth were not in the way"""
    lat, lon, _ = SITES[site]
    far = geodetic_to_ecef(-lat, lon + 180.0 if lon < 0 else lon - 180.0, 0.0)
    rx = site_ecef(site)
    for raw, row in pc.pick_satellites(far, TOW, 4, seed=SEEDS[0]):
        if float(pc.travel_time(row, rx, np.array([TOW]))[2][0]) < -0.2:
            return observable(row, rx, TOW), eph_record(raw)
    raise AssertionError(site)


def launch_case(ch, n_rx):
    """one launch of the GPU tests: receiver r is of KINDS[(r + ch) % 12], its satellites (twelve at most) start at slot r % ch and wrap, the
    rest of its slots are all-zero pairs; a spoiled slot is the first, the last or one between, in turn
    -> dict(obs, eph, lock (None when no receiver is lock_masked), kinds [n_rx], spoiled [n_rx] (slot lists))"""
    names = sorted(SITES)
    obs, eph = np.zeros((n_rx, ch), O.OBS_DTYPE), np.zeros((n_rx, ch), E.EPH_DTYPE)
    lock = np.zeros((n_rx, ch), F.LOCK_DTYPE)
    lock["flags"] = F.LOCK_CODE
    kinds, spoiled, masked = [], [], False
    for r in range(n_rx):
        site, kind = names[(r + ch) % len(names)], KINDS[(r + ch) % len(KINDS)]
        n = min(ch, 12)
        o, e = receiver(site, n, 3 * (r % 20))
        slots = [(r + k) % ch for k in range(n)]
        if kind == "duplicate" and ch >= 4:      # four slots, two of them the same satellite
            slots, o, e = slots[:4], o[[0, 1, 2, 2]], e[[0, 1, 2, 2]]
        obs[r, slots], eph[r, slots] = o, e
        at = [(0, ch - 1, ch // 2)[r % 3]] if kind != "first_and_last" else sorted({0, ch - 1})
        if kind in ("clean", "duplicate"):
            at = []
        for p in at:
            if p not in slots:      # a spoiled slot holds a satellite: move one there
                q = slots[-1]
                obs[r, p], eph[r, p] = obs[r, q], eph[r, q]
                obs[r, q], eph[r, q] = 0, 0
                slots = slots[:-1] + [p]
            k = kind if kind != "first_and_last" else ("unhealthy", "toe_far")[p != 0]
            if k == "obs_invalid":
                obs["flags"][r, p] &= ~np.uint32(O.F_VALID)
            elif k == "eph_invalid":
                eph["flags"][r, p] = 0
            elif k == "zero_pair":
                obs[r, p], eph[r, p] = 0, 0
            elif k == "unhealthy":
                eph["svh"][r, p] = 1
            elif k == "below_horizon":
                obs[r, p], eph[r, p] = _below_horizon(site)
            elif k == "a_zero":
                eph["A"][r, p] = 0.0
            elif k == "toe_far":
                eph["toe_time"][r, p] += 7300
            elif k == "lock_masked":
                lock["flags"][r, p], masked = 0, True
            elif k == "nan_element":
                eph["crc"][r, p] = np.nan
        kinds.append(kind)
        spoiled.append(at)
    return dict(obs=obs.reshape(-1), eph=eph.reshape(-1), lock=lock.reshape(-1) if masked else None, kinds=kinds, spoiled=spoiled)


def compare(got, got_pr, want, want_pr, bound=None):
    """a launch's records against the restatement's as the issue orders it: exact flags, n_used, used_mask, ref_slot, week; bitwise
    pr_m and rx_tow_s; n_iter within one; rr, c dtr_s, geo[2], resid_rms_m / 2 within the position bound, geo[0..1] within it / 6.3e6,
    qr 1e-5 relative -> the per-field maxima of the differences (measured before anything is asserted)"""
    bound = POSITION_BOUND_M if bound is None else bound
    fixed = (want["flags"] & F.F_FIX) != 0
    dq = np.abs(got["qr"][fixed] - want["qr"][fixed]) / np.maximum(np.abs(want["qr"][fixed]), 1e-30)
    worst = {"rr_m": float(np.linalg.norm(got["rr"] - want["rr"], axis=1).max()), "cdt_m": float(np.abs(got["dtr_s"] - want["dtr_s"]).max() * CLIGHT),
             "height_m": float(np.abs(got["geo"][:, 2] - want["geo"][:, 2]).max()), "latlon_rad": float(np.abs(got["geo"][:, :2] - want["geo"][:, :2]).max()),
             "resid_rms_m": float(np.abs(got["resid_rms_m"] - want["resid_rms_m"]).max()), "qr_rel": float(dq.max()) if dq.size else 0.0,
             "n_iter": int(np.abs(got["n_iter"] - want["n_iter"]).max())}
    for f in ("flags", "n_used", "used_mask", "ref_slot", "week", "reserved"):
        assert (got[f] == want[f]).all(), (f, np.flatnonzero(got[f] != want[f])[:8], got[f][got[f] != want[f]][:8], want[f][got[f] != want[f]][:8])
    assert got["rx_tow_s"].tobytes() == want["rx_tow_s"].tobytes(), "rx_tow_s"
    assert got_pr is None or got_pr.tobytes() == want_pr.tobytes(), "pr_m"
    assert np.isfinite(got["rr"]).all() and np.isfinite(got["geo"]).all() and np.isfinite(got["qr"]).all() and np.isfinite(got["resid_rms_m"]).all()
    off = np.flatnonzero(np.abs(got["n_iter"] - want["n_iter"]) > 1)
    assert off.size == 0, (worst, "receivers", off[:8], "n_iter", got["n_iter"][off][:8], want["n_iter"][off][:8], "flags", want["flags"][off][:8])
    assert max(worst["rr_m"], worst["cdt_m"], worst["height_m"], worst["resid_rms_m"] / 2.0) <= bound, worst
    assert worst["latlon_rad"] <= bound / 6.3e6 and worst["qr_rel"] <= 1e-5, worst
    unfixed = ~fixed
    for f in ("rr", "dtr_s", "geo", "qr", "resid_rms_m"):
        assert not got[f][unfixed].any(), (f, "not zero without FIX")
    return worst


def fix_error(fix, site):
    return float(np.linalg.norm(np.asarray(fix["rr"], np.float64) - site_ecef(site)))


# ---- bounds -----------------------------------------------------------------------------------------------------------------------
# (b) MEASURED["pntpos_m"]: the largest distance from the true receiver that the library's pntpos shows on four-satellite subsets (slots
#     0 .. 3 and the last four) of big_skies(5), big_skies(8) and big_skies(12), noise-free.  What it is made of: the float32 code phase
#     (half an ulp at 16 368 samples is 0.009 m of range) and the five passes of travel_time's fixed point, times the geometry.
# (c) MEASURED["noise_median_m"]: the median error of noisy()'s 64 receivers with all twelve satellites and with each one's first four.
#     Measured: pntpos 1.385 / 0.999 / 2.079 m at 5 / 8 / 12 satellites; medians 5.025 m (twelve) and 19.347 m (four).
MEASURED = {"pntpos_m": 2.0786, "noise_median_m": (5.025, 19.347)}
BOUNDS = {"noise_free_m": 2.0 * MEASURED["pntpos_m"]}
# the device against the restatement: 8 x the largest |d rr| measured on one MI355X over every receiver of tests/test_gpu_weighted_fix.py
# (profiles/r19_weighted_fix_parity.json), capped at 1e-4 m -- both stop at a step below 1e-4 m of an iteration that contracts by orders
# of magnitude per step, so two correct implementations one iteration apart are closer than that
PARITY_MEASURED_M = 7.63e-7
PARITY_CAP_M = 1e-4
POSITION_BOUND_M = PARITY_CAP_M if PARITY_MEASURED_M is None else min(8.0 * PARITY_MEASURED_M, PARITY_CAP_M)
