"""What the CPU and GPU tests of the weighted chain's solvers at the edges of their input space share (include/gpsx.h gpsx_wfix, gpsx_wfde,
gpsx_wvel; tests/test_weighted_edge_reference.py, tests/test_gpu_weighted_edges.py): receivers across the week, across the orbit and
across the globe.  weighted_fix_cases draws every receiver at one instant (tk = -2465 s), with e <= 0.012, f2 = tgd = sva = 0 and
toc = toe, at four sites between 34 S and 48 N; here tk runs to either end of the ephemeris' span, e to 0.4, the clock has every term and
an epoch of its own, and the sites reach both Klobuchar clamps and both troposphere cut-offs.  Test infrastructure; nothing here is
product code.

The picker (pick) is pvt_chain.pick_satellites' rejection with `toes` given and the wider draws; a row goes through pvt_chain.quantize and
subframe_payloads (with toc put into the raw integers) and weighted_eph_ref.decode, so a record is what gpsx_weph gives for that
broadcast.  The truth (sat_state, travel_time, observable, doppler) is this module's own: dts(t) = f0 + f1 (t - toc) + f2 (t - toc)^2 +
relativity, every difference of times folded into +- half a week, the L1 code showing t + dts - tgd, and an atmosphere with the cut-offs
of the header's step 4 (no troposphere below -100 m or above 10 km; Klobuchar's clamp at +- 0.416 semicircles).  An observable is
T = 1000 (t_rx - tau + dts - tgd) ms, tx_ms = ceil(T) mod one week, code_phase_fine = float32((ceil(T) - T) 16368); the milliseconds are
taken from the fraction of t_rx alone, so T keeps its last digits late in the week."""
import functools
import json
import math
import os
import time

import numpy as np

import pvt_chain as pc
import weighted_eph_ref as E
import weighted_fde_ref as D
import weighted_fix_cases as W
import weighted_fix_ref as F
import weighted_obs_ref as O
import weighted_vel_cases as K
import weighted_vel_ref as V
from pvt_types import CLIGHT, OMGE, geodetic_to_ecef

WEEK_S, WEEK_MS = 604800.0, 604_800_000
OFFSET_MS = W.OFFSET_MS
SITES = {"munich": W.MUNICH,                   # the control
         "arctic": (84.0, -40.0, 10.0),        # Klobuchar's clamp at +0.416
         "pole": (-89.9, 0.0, 2835.0),         # the clamp at -0.416; longitude conditioned by 1 / cos(lat)
         "high": (-0.18, -78.47, 12000.0),     # above 10 km: no troposphere
         "deadsea": (31.5, 35.5, -430.0)}      # below -100 m: no troposphere
VELOCITY, DRIFT = K.VELOCITIES[1], K.DRIFTS[1]      # every receiver moves at 36 m/s and drifts by 1e-6 s/s
BUILD_SECONDS = {}      # what building cost, per cached item (printed by the reference test)


def site_ecef(name):
    return geodetic_to_ecef(*SITES[name])


def fold(d):
    """a difference of times of the week into [-302 400, 302 400)"""
    return (np.asarray(d, np.float64) + 302400.0) % WEEK_S - 302400.0


# ---- the truth ------------------------------------------------------------------------------------------------------------------------
def sat_state(row, t):
    """ECEF position and clock offset of satellite `row` at GPS time of week t (array): pvt_chain.sat_state's orbit at the folded
    tk, the polynomial about the row's own toc with the quadratic term, the relativistic term"""
    t = np.asarray(t, np.float64)
    pos, rel = pc.sat_state(dict(row, f0=0.0, f1=0.0, f2=0.0), row["toes"] + fold(t - row["toes"]))
    tc = fold(t - row["toc"])
    return pos, row["f0"] + row["f1"] * tc + row["f2"] * tc * tc + rel


def troposphere(geo, el):
    """pvt_chain's Saastamoinen with the cut-offs of the header's step 4"""
    if geo[2] < -100.0 or geo[2] > 1e4:
        return np.zeros_like(el)
    return pc._saastamoinen(geo, el)


def travel_time(row, rx, t_rx, atmosphere=True):
    """pvt_chain.travel_time on this module's satellite and atmosphere -> (tau, dts at transmission, elevation, azimuth)"""
    t_rx = np.asarray(t_rx, np.float64)
    geo = pc._geodetic(rx)
    tau = np.full_like(t_rx, 0.075)
    for _ in range(5):
        pos, dts = sat_state(row, t_rx - tau)
        th = OMGE * tau
        rot = np.stack([np.cos(th) * pos[..., 0] + np.sin(th) * pos[..., 1], -np.sin(th) * pos[..., 0] + np.cos(th) * pos[..., 1], pos[..., 2]], -1)
        az, el = pc._azel(rx, geo, rot)
        rng = np.linalg.norm(rot - rx, axis=-1)
        if atmosphere:
            rng = rng + pc._klobuchar(t_rx, geo, az, el) + troposphere(geo, el)      # (Klobuchar's clamp is in pvt_chain's)
        tau = rng / CLIGHT
    return tau, dts, el, az


def observable(row, rx, t_rx, noise_m=0.0):
    """the VALID gpsx_wobs_t of one satellite at the receiver instant t_rx (seconds of the week; past 604 800 the transmit time wraps)"""
    tau, dts, _, _ = travel_time(row, rx, np.array([t_rx]))
    whole = math.floor(t_rx)
    part = 1000.0 * ((t_rx - whole) - (float(tau[0]) + noise_m / CLIGHT) + float(dts[0]) - row["tgd0"])
    up = math.ceil(part)
    o = np.zeros(1, O.OBS_DTYPE)
    o["tx_ms"], o["code_phase_fine"], o["flags"] = (1000 * whole + up) % WEEK_MS, np.float32((up - part) * 16368.0), W.OBS_FLAGS
    return o


def doppler(row, rx0, t, v=VELOCITY, drift=DRIFT):
    """weighted_vel_cases.doppler's central difference on this module's travel time, for a receiver that passes rx0 at t with velocity v
    (the two instants' distances from t are taken as the doubles they are)"""
    rx0, v = np.asarray(rx0, np.float64), np.asarray(v, np.float64)
    g, s = [], []
    for h in (-K.H_S, K.H_S):
        s.append((t + h) - t)
        tau, dts, _, _ = travel_time(row, rx0 + v * s[-1], np.array([t + h]), atmosphere=False)
        g.append(float(tau[0]) - float(dts[0]) + drift * s[-1])
    return np.float32(-pc.F_L1 * (g[1] - g[0]) / (s[1] - s[0]))


# ---- the picker -------------------------------------------------------------------------------------------------------------------------
def pick(rx, t, toes, n, seed, min_el_deg=25.0):
    """n <= 4 satellites above min_el_deg at ECEF rx at time of week t, spread in azimuth as pvt_chain.pick_satellites spreads them, with
    the broadcast's epoch `toes` given: e uniform in [0, 0.4] (the first satellite's exactly 0), sva 0 .. 15, tgd0 ~ N(0, 2e-8 s) and
    f2 ~ N(0, 1.5e-15 s/s^2) (both cut at what eight bits carry), toc = toes - 16 k with k in 0 .. 450 (not below the week's start)
    -> [(raw integers, quantised row with `toc`)]"""
    assert 1 <= n <= 4 and toes % 16 == 0 and 0 <= toes < WEEK_S
    rng = np.random.default_rng(seed)
    geo = pc._geodetic(rx)
    out = []
    while len(out) < n:
        row = dict(sat=0, iode=int(rng.integers(1, 255)), iodc=0, sva=int(rng.integers(0, 16)), svh=0, week=pc.WEEK,
                   A=26559710.0 + rng.normal(0, 3e3), e=0.0 if not out else float(rng.uniform(0.0, 0.4)), i0=0.96 + rng.normal(0, 0.02),
                   OMG0=float(rng.uniform(-math.pi, math.pi)), omg=float(rng.uniform(-math.pi, math.pi)),
                   M0=float(rng.uniform(-math.pi, math.pi)), deln=float(rng.normal(4.5e-9, 5e-10)),
                   OMGd=float(rng.normal(-8.0e-9, 3e-10)), idot=float(rng.normal(0, 2e-10)),
                   crc=float(rng.normal(220, 60)), crs=float(rng.normal(0, 60)), cuc=float(rng.normal(0, 3e-6)),
                   cus=float(rng.normal(6e-6, 3e-6)), cic=float(rng.normal(0, 1e-7)), cis=float(rng.normal(0, 1e-7)),
                   toes=float(toes), f0=float(rng.normal(0, 2e-4)), f1=float(rng.normal(0, 5e-12)),
                   f2=float(np.clip(rng.normal(0, 1.5e-15), -3.4e-15, 3.4e-15)), tgd0=float(np.clip(rng.normal(0, 2e-8), -5.8e-8, 5.8e-8)))
        k = int(rng.integers(0, min(450, int(toes) // 16) + 1))
        row["iodc"] = row["iode"]
        pos, _ = pc.sat_state(row, np.array([toes + float(fold(t - toes))]))
        az, el = pc._azel(rx, geo, pos)
        if math.degrees(el[0]) < min_el_deg:
            continue
        if any(abs((az[0] - a + math.pi) % (2 * math.pi) - math.pi) < 2 * math.pi / (n + 2) for _, _, a in out):
            continue
        raw, q = pc.quantize(row)
        raw["toc"], q["toc"] = (int(toes) - 16 * k) // 16, float(int(toes) - 16 * k)
        out.append((raw, q, float(az[0])))
    return [(raw, q) for raw, q, _ in out]


def eph_record(raw, t):
    """weighted_fix_cases.eph_record with subframe 1's hand-over count a few subframes before t"""
    return W.eph_record(raw, max(0, int(t // 6) - 4) % 100800)


def shift_weeks(eph, weeks):
    """records whose week, toe_time, toc_time and ttr_time are `weeks` whole weeks later"""
    out = eph.copy()
    out["week"] += weeks
    for f in ("toe_time", "toc_time", "ttr_time"):
        out[f] += 604800 * weeks
    return out


# ---- the receivers ------------------------------------------------------------------------------------------------------------------
# name -> (site, receive time in seconds of the week, ((toes, seed, satellites taken), ...)).  A solved receiver is named by what its
# satellites' tk = t - toes are: a time t = 16 k + 0.5 puts toes at t - 7200.5, t + 3599.5, t - 0.5 (tk about +7200.4, -3599.6, +0.4 at
# transmission: the near side of the 7201 s limit by half a second against 0.09 s of travel time, clock and reference-slot offset), a time
# t = 16 k + 15.5 at t + 7200.5, t - 3599.5, t + 0.5.  One second later (far_plus) or earlier (far_minus) the first satellite's
# |toe - t| = 7201.5 gives no row; the rest of that receiver is good.  Every (site, t, toes, seed) below is checked to return within a
# second by tests/test_weighted_edge_reference.py.
def _spans(t, plus):
    return ((t - 7200.5, 4), (t + 3599.5, 4), (t - 0.5, 4)) if plus else ((t + 7200.5, 4), (t - 3599.5, 4), (t + 0.5, 4))


_BASE = {"munich": 100000, "arctic": 216000, "pole": 350000, "high": 450000, "deadsea": 550000}      # multiples of 16
RECEIVERS = {}
_seed = 1000
for _site, _b in _BASE.items():
    for _plus in (True, False):
        _t = _b + (0.5 if _plus else 15.5)
        RECEIVERS[f"{_site}_{'plus' if _plus else 'minus'}"] = (_site, _t, tuple((toes, _seed + 7 * i, n) for i, (toes, n) in enumerate(_spans(_t, _plus))))
        _seed += 31
for _name, _t, _first in (("near_plus", 132000 + 0.5, 132000 - 7200), ("far_plus", 132000 + 1.5, 132000 - 7200),
                          ("near_minus", 164000 - 0.5, 164000 + 7200), ("far_minus", 164000 - 1.5, 164000 + 7200)):
    RECEIVERS[_name] = ("munich", _t, ((_first, _seed, 1), (_first + (3600 if "plus" in _name else -3600), _seed + 1, 4),
                                       (16 * int(_t // 16), _seed + 12, 4), (_first + (7200 if "plus" in _name else -7200), _seed + 3, 3)))
    _seed += 31
for _name, _site, _t, _toes in (("t_30", "munich", 30.0, (0, 7200, 3600)), ("t_half_before", "arctic", 302399.9, (302400, 298800, 309584)),
                                ("t_half_after", "pole", 302400.1, (302400, 306000, 295216)), ("t_week_end", "high", 604798.8, (604784, 601200, 597600))):
    RECEIVERS[_name] = (_site, _t, tuple((toes, _seed + 7 * i, 4) for i, toes in enumerate(_toes)))
    _seed += 31
# t_sv within 50 ms of either side of the week's end; in straddle_b three satellites are on the next week's broadcast (toes = 0): too
# few for gpsx_wfix, whose observation time wraps to the start of the records' week, and rows for gpsx_wvel, which folds; prev_week
# stands at 1800 s on the previous week's broadcast: tk = +5400 s through the fold
RECEIVERS["straddle_a"] = ("munich", 604800.075, ((601200, _seed, 4), (601200, _seed + 1, 4), (601200, _seed + 2, 4)))
RECEIVERS["straddle_b"] = ("arctic", 604800.078, ((0, _seed + 3, 3), (601200, _seed + 4, 4), (601200, _seed + 5, 4), (601200, _seed + 9, 1)))
RECEIVERS["prev_week"] = ("munich", 1800.0, ((601200, _seed + 6, 4), (601200, _seed + 7, 4), (601200, _seed + 8, 4)))
SHIFTS = {"shift_m522": -522, "shift_m1": -1, "shift_p1": 1, "shift_p500": 500}      # copies of munich_plus, whole weeks away
SYNTHETIC = ("synthetic_before", "synthetic_after")      # transmit milliseconds set by hand around 604 800 000: pseudoranges only
SOLVED = tuple(n for n in RECEIVERS if not n.startswith(("straddle", "prev_week"))) + tuple(SHIFTS)
NOT_SOLVED_BY_WFIX = ("straddle_a", "straddle_b", "prev_week") + SYNTHETIC      # (the restatement says what they end in)
# the launches' order: kinds in turn, so that neighbours in a wave differ in what their lanes do
ORDER = ("munich_plus", "straddle_a", "pole_minus", "far_plus", "shift_m522", "t_30", "arctic_plus", "synthetic_before", "high_minus", "near_minus",
         "prev_week", "t_half_before", "deadsea_plus", "shift_p1", "pole_plus", "far_minus", "t_week_end", "straddle_b", "munich_minus", "shift_m1",
         "arctic_minus", "near_plus", "synthetic_after", "t_half_after", "high_plus", "shift_p500", "deadsea_minus")
assert sorted(ORDER) == sorted(tuple(RECEIVERS) + tuple(SHIFTS) + SYNTHETIC)


@functools.lru_cache(maxsize=None)
def sky(name):
    """the receiver's satellites, renumbered 1 .. -> ((raw integers, row), ...); the slowest pick's seconds go to BUILD_SECONDS"""
    site, t, picks = RECEIVERS[name]
    rx, out, slowest = site_ecef(site), [], 0.0
    for toes, seed, n in picks:
        t0 = time.perf_counter()
        got = pick(rx, t, toes, 4, seed)[:n]
        slowest = max(slowest, time.perf_counter() - t0)
        out += [(raw, dict(row, sat=len(out) + i + 1)) for i, (raw, row) in enumerate(got)]
    BUILD_SECONDS["pick " + name] = slowest
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _receiver(name):
    if name in SHIFTS:
        base = _receiver("munich_plus")
        return dict(base, name=name, eph=shift_weeks(base["eph"], SHIFTS[name]))
    if name in SYNTHETIC:      # munich_plus' records (toes around 100 000 s: no candidate at the week's end, whatever the pseudoranges)
        base = _receiver("munich_plus")
        obs = base["obs"].copy()
        rng = np.random.default_rng(77 + SYNTHETIC.index(name))
        late = rng.integers(604_799_900, 604_799_999, 12)
        early = rng.integers(0, 31, 12)
        # before: every slot before the week's end but two in the middle, the latest of all first -- ref_slot moves across the end;
        # after: the first slot after the end, then the sides in turn
        obs["tx_ms"] = np.where(np.isin(np.arange(12), (5, 9)), early, late) if name == "synthetic_before" else np.where(np.arange(12) % 2 == 0, early, late)
        obs["code_phase_fine"] = rng.uniform(0.0, 16367.0, 12).astype(np.float32)
        return dict(base, name=name, obs=obs, rows=None, fix=no_fix_record())
    site, t, _ = RECEIVERS[name]
    rx, sats = site_ecef(site), sky(name)
    obs = np.concatenate([observable(row, rx, t) for _, row in sats])
    obs["if_freq_offset_hz"] = [doppler(row, rx, t) for _, row in sats]
    eph = np.concatenate([eph_record(raw, t) for raw, _ in sats])
    if name == "prev_week":
        eph = shift_weeks(eph, -1)
    return dict(name=name, site=site, t=t, rows=tuple(row for _, row in sats), obs=obs, eph=eph)


def no_fix_record():
    fix = np.zeros(1, F.FIX_DTYPE)
    fix["flags"] = F.F_TOO_FEW
    return fix


def receiver(name, n=12):
    """dict(name, site, t, rows, obs [n], eph [n]): the receiver's first n satellites (copies)"""
    r = _receiver(name)
    return dict(r, obs=r["obs"][:n].copy(), eph=r["eph"][:n].copy(), rows=None if r["rows"] is None else r["rows"][:n])


def noisy(name, noise_m, ms=None):
    """the twelve-satellite receiver with noise_m metres added per pseudorange; ms {slot: d}: tx_ms moved by d and flagged AMBIGUOUS"""
    r = receiver(name)
    rx = site_ecef(r["site"])
    dop = r["obs"]["if_freq_offset_hz"].copy()
    r["obs"] = np.concatenate([observable(row, rx, r["t"], float(m)) for row, m in zip(r["rows"], noise_m)])
    r["obs"]["if_freq_offset_hz"] = dop
    for slot, d in (ms or {}).items():
        r["obs"]["tx_ms"][slot] += d
        r["obs"]["flags"][slot] |= O.F_AMBIGUOUS
    return r


# ---- the launches -------------------------------------------------------------------------------------------------------------------
SHAPES = ((8, len(ORDER)), (12, len(ORDER)), (33, 17))


@functools.lru_cache(maxsize=None)
def launch_case(ch, n_rx):
    """One launch: receiver r is ORDER[r], its satellites (twelve at most) start at slot r % ch and wrap (a copy whole weeks away sits in
    munich_plus' slots, so that its bytes can be munich_plus'), the rest of its slots are all-zero pairs.  `fix` holds what gpsx_wvel stands on when it is given directly: the true site with every filled slot in used_mask
    (a synthetic receiver: a record without FIX).
    -> dict(obs, eph, fix, names, slots [n_rx] (slot of satellite k), cfg (gpsx_wfix's), vcfg (gpsx_wvel's))"""
    t0 = time.perf_counter()
    obs, eph = np.zeros((n_rx, ch), O.OBS_DTYPE), np.zeros((n_rx, ch), E.EPH_DTYPE)
    fix = np.zeros(n_rx, F.FIX_DTYPE)
    names, slots_of = ORDER[:n_rx], []
    for r, name in enumerate(names):
        rec = receiver(name, min(ch, 12))
        start = names.index("munich_plus") if name in SHIFTS else r      # (a copy in its original's slots: the same lanes, the same sums)
        slots = [(start + k) % ch for k in range(len(rec["obs"]))]
        obs[r, slots], eph[r, slots] = rec["obs"], rec["eph"]
        fix[r] = (no_fix_record() if name in SYNTHETIC else K.fix_record(site_ecef(rec["site"]), slots))[0]
        slots_of.append(slots)
    BUILD_SECONDS[f"launch {ch} x {n_rx}"] = time.perf_counter() - t0
    return dict(obs=obs.reshape(-1), eph=eph.reshape(-1), fix=fix, names=names, slots=slots_of, cfg=F.make_cfg(OFFSET_MS, ch), vcfg=V.make_cfg(ch))


@functools.lru_cache(maxsize=None)
def want_fix(ch, n_rx, warm=False):
    """the restatement's (fix records, pr_m) of a launch; warm: from a previous fix 30 km off the cold one"""
    case = launch_case(ch, n_rx)
    cold = F.run(case["cfg"], case["obs"], case["eph"], n_rx)
    if not warm:
        return cold
    return F.run(case["cfg"], case["obs"], case["eph"], n_rx, prev=warm_start(cold[0]))


def warm_start(cold):
    prev = cold.copy()
    prev["rr"][(prev["flags"] & F.F_FIX) != 0] += np.array([3.0, -2.0, 1.0]) * (30e3 / math.sqrt(14.0))      # 30 km
    return prev


@functools.lru_cache(maxsize=None)
def want_vel(ch, n_rx):
    case = launch_case(ch, n_rx)
    return V.run(case["vcfg"], case["obs"], case["eph"], case["fix"], n_rx)


def fix_pivot_shares(cfg, obs, eph, n_rx, fix):
    """the weighted normal system of gpsx_wfix's step 6 at each record's own solution, over the rows of its used_mask, by
    weighted_fix_ref's functions -> p_k / N_kk [n_rx, 4] (p_0 itself first), as weighted_vel_ref._cholesky gives them"""
    c = np.asarray(cfg, F.CFG_DTYPE).reshape(1)[0]
    ch = int(c["ch_per_rx"])
    o, e = np.ascontiguousarray(obs, O.OBS_DTYPE).reshape(n_rx, ch), np.ascontiguousarray(eph, E.EPH_DTYPE).reshape(n_rx, ch)
    with np.errstate(all="ignore"):
        usable = ((o["flags"] & O.F_VALID) != 0) & ((e["flags"] & E.F_VALID) != 0)
        pr, _, _ = F.pseudoranges(o, usable, float(c["offset_ms"]))
        whole_s = np.trunc(fix["rx_tow_s"]).astype(np.int64)
        whole = (F.UNIX_TO_GPS + 604800 * fix["week"].astype(np.int64) + whole_s)[:, None]
        sec = (fix["rx_tow_s"] - whole_s)[:, None]
        sat_ok, pos, clk, var = F._satellites(e, usable, whole, sec, pr)
        x = np.concatenate([fix["rr"], (fix["dtr_s"] * F.C_LIGHT)[:, None]], 1)
        row, a, y, _, _ = F._rows(x, sat_ok, pos, clk, var, e["svh"] == 0, F.C_LIGHT * e["tgd"], pr, whole_s + sec[:, 0], F.ION_DEFAULT)
        used = ((fix["used_mask"][:, None] >> np.arange(ch, dtype=np.uint64)[None, :]) & np.uint64(1)) != 0
        a = np.where((row & used)[..., None], a, 0.0)
        return V._cholesky(np.einsum("rci,rcj->rij", a, a), np.einsum("rci,rc->ri", a, np.where(row & used, y, 0.0)))[3]


def fix_decisions_clear(ch, n_rx, warm=False):
    """every solved receiver's system in the restatement has pivot shares >= 1e-7 (1e3 x the rule's 1e-10), so the device, whose sums
    differ in the last digits, decides alike -> the smallest share"""
    case, (fix, _) = launch_case(ch, n_rx), want_fix(ch, n_rx, warm)
    shares = fix_pivot_shares(case["cfg"], case["obs"], case["eph"], n_rx, fix)
    solved = (fix["flags"] & F.F_FIX) != 0
    assert (shares[solved, 0] > 0.0).all() and (shares[solved, 1:] >= 1e-7).all(), [(case["names"][r], shares[r]) for r in np.flatnonzero(solved) if not (shares[r, 1:] >= 1e-7).all()]
    return float(shares[solved, 1:].min())


# ---- what the census of tests/test_weighted_edge_reference.py reads: inputs and true geometry, no solver ------------------------------------
@functools.lru_cache(maxsize=None)
def geometry(name):
    """per satellite of a physical receiver, from the truth alone: tk at transmission (folded), e, sva, elevation, azimuth, Klobuchar's
    latitude before its clamp (semicircles) and its phase x (the day arm is |x| < 1.57), toc - toe -> dict of arrays [12]"""
    site, t, _ = RECEIVERS[name]
    rx = site_ecef(site)
    geo = pc._geodetic(rx)
    out = {k: [] for k in ("tk", "e", "sva", "el", "az", "phi_raw", "x", "toc_minus_toe", "tc", "mean")}
    for raw, row in sky(name):
        tau, _, el, az = (float(a[0]) for a in travel_time(row, rx, np.array([t])))
        tk = float(fold(t - tau - row["toes"]))
        psi = 0.0137 / (el / math.pi + 0.11) - 0.022
        raw_phi = geo[0] / math.pi + psi * math.cos(az)
        phi = min(max(raw_phi, -0.416), 0.416)
        lam = geo[1] / math.pi + psi * math.sin(az) / math.cos(phi * math.pi)
        phi += 0.064 * math.cos((lam - 1.617) * math.pi)
        per = max(F.ION_DEFAULT[4] + phi * (F.ION_DEFAULT[5] + phi * (F.ION_DEFAULT[6] + phi * F.ION_DEFAULT[7])), 72000.0)
        x = 2.0 * math.pi * ((43200.0 * lam + t) % 86400.0 - 50400.0) / per
        for k, v in (("tk", tk), ("e", row["e"]), ("sva", raw["sva"]), ("el", el), ("az", az), ("phi_raw", raw_phi), ("x", x),
                     ("toc_minus_toe", row["toc"] - row["toes"]), ("tc", float(fold(t - tau - row["toc"]))),
                     ("mean", row["M0"] + (math.sqrt(F.MU / row["A"] ** 3) + row["deln"]) * tk)):
            out[k].append(v)
    return {k: np.array(v) for k, v in out.items()}


def kepler_trips(mean, e):
    """the trip count of the restatements' Kepler loop (weighted_fix_ref._satellites, weighted_vel_ref.satellites: from E = M, until a
    step moves E by at most 1e-14, thirty at most) for arrays of mean anomaly and eccentricity"""
    ecc, was, n = mean.copy(), np.zeros(mean.shape), np.zeros(mean.shape, np.int64)
    for _ in range(30):
        go = (np.abs(ecc - was) > 1E-14) & (n < 30)
        if not go.any():
            break
        was = np.where(go, ecc, was)
        ecc = np.where(go, ecc - (ecc - e * np.sin(ecc) - mean) / (1.0 - e * np.cos(ecc)), ecc)
        n = n + go
    return n


def wave_trip_spreads(ch, n_rx):
    """per 64-lane wave of a launch (a receiver is a group of W lanes, W the smallest power of two >= ch_per_rx; slot = lane in group)
    the largest minus the smallest Kepler trip count over the lanes that hold a physical receiver's satellite"""
    w = 1
    while w < ch:
        w *= 2
    case, waves = launch_case(ch, n_rx), {}
    for r, name in enumerate(case["names"]):
        base = "munich_plus" if name in SHIFTS else name
        if base in SYNTHETIC:
            continue
        g = geometry(base)
        trips = kepler_trips(g["mean"], g["e"])
        for k, slot in enumerate(case["slots"][r]):
            waves.setdefault((r * w + slot) // 64, []).append(int(trips[k]))
    return {wave: max(t) - min(t) for wave, t in waves.items()}


# ---- fault detection and exclusion ---------------------------------------------------------------------------------------------------
FDE_NAMES = ("munich_plus", "munich_minus", "arctic_plus", "arctic_minus", "pole_plus", "pole_minus", "near_plus", "near_minus")
FDE_SEED, FDE_NOISE_M, FDE_FAULT_M = 2026, 2.0, 300.0
FDE_SVA_MAX = 5      # a fault is put on a satellite whose broadcast sigma is at most 13.65 m: under sva 12 (1536 m) 300 m is no fault at all


@functools.lru_cache(maxsize=None)
def fde_draws():
    """per receiver of FDE_NAMES (either tk extreme at the control and both polar sites, the limit's near side) under 2 m of seeded noise:
    a 300 m fault on one slot, and one slot a millisecond off and AMBIGUOUS, the slot the first, the last or the middle one, in turn, of
    those whose sva is at most FDE_SVA_MAX (chosen from the records, not from a solver)
    -> [dict(name, kind, slot, d, obs, eph)], 16 draws"""
    out = []
    for i, name in enumerate(FDE_NAMES):
        for kind in ("fault", "ms"):
            rng = np.random.default_rng([FDE_SEED, i, kind == "ms"])
            sharp = [k for k, row in enumerate(receiver(name)["eph"]["sva"]) if row <= FDE_SVA_MAX]
            noise, slot = rng.normal(0.0, FDE_NOISE_M, 12), (sharp[0], sharp[-1], sharp[len(sharp) // 2])[(i + (kind == "ms")) % 3]
            d = int(rng.choice((-1, 1)))
            if kind == "fault":
                noise[slot] += FDE_FAULT_M
            r = noisy(name, noise, {slot: d} if kind == "ms" else None)
            out.append(dict(name=name, kind=kind, slot=slot, d=d, obs=r["obs"], eph=r["eph"], site=r["site"]))
    return out


def fde_cfg(ch=12, **kw):
    return D.make_cfg(OFFSET_MS, ch, **kw)


@functools.lru_cache(maxsize=None)
def fde_kept():
    """the draws whose every margin in the restatement is at least weighted_fde_ref.MARGIN and whose restatement finds what was
    injected -> ([draw], (fix, fde, pr, margins) of the kept draws packed into one twelve-slot launch)"""
    draws = fde_draws()
    obs, eph = W.pack([(d["obs"], d["eph"]) for d in draws], 12)
    _, fde, _, margins = D.run(fde_cfg(), obs, eph, len(draws))
    kept = [d for r, d in enumerate(draws) if D.min_margin(margins[r]) >= D.MARGIN and fde_found(d, fde[r])]
    obs, eph = W.pack([(d["obs"], d["eph"]) for d in kept], 12)
    return kept, D.run(fde_cfg(), obs, eph, len(kept))


def fde_found(draw, fde):
    """the record names the injected slot and nothing else"""
    if draw["kind"] == "fault":
        return int(fde["excl_mask"]) == 1 << draw["slot"] and int(fde["plus_mask"]) == 0 and int(fde["minus_mask"]) == 0
    plus, minus = ((1 << draw["slot"], 0) if draw["d"] < 0 else (0, 1 << draw["slot"]))
    return int(fde["excl_mask"]) == 0 and int(fde["plus_mask"]) == plus and int(fde["minus_mask"]) == minus


# ---- comparison ---------------------------------------------------------------------------------------------------------------------
PARITY_ENV = "GPSX_WEDGE_PARITY_JSON"      # a path: every labelled comparison records its maxima there (how the profile is written)


def record_parity(label, stage, worst, fields, names=None):
    path = os.environ.get(PARITY_ENV)
    if not path or label is None:
        return
    doc = json.load(open(path)) if os.path.exists(path) else {"launches": {}}
    doc["launches"][label] = dict(worst, stage=stage, largest=max(worst[k] for k in fields), **({"worst_receiver": names} if names else {}))
    doc["what"] = ("largest |device - restatement| per compared launch of tests/test_gpu_weighted_edges.py, one MI355X: fix and fde in metres (rr, c dtr, "
                   "height, latitude and longitude as ground distance, resid_rms_m / 2), vel in m/s (vel, enu, c drift, resid_rms_mps); written by "
                   "weighted_edge_cases under $" + PARITY_ENV)
    for st in ("fix", "fde", "vel"):
        got = [v["largest"] for v in doc["launches"].values() if v["stage"] == st]
        if got:
            doc["largest_" + st] = max(got)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)


FIX_FIELDS = ("rr_m", "cdt_m", "height_m", "lat_m", "lon_m", "half_resid_rms_m")


def compare(got, got_pr, want, want_pr, bound=None, label=None, stage="fix", names=None):
    """weighted_fix_cases.compare's order and fields -- exact flags, n_used, used_mask, ref_slot, week, reserved; bitwise rx_tow_s and
    pr_m; n_iter within one; rr, c dtr_s, height and resid_rms_m / 2 within the position bound; qr 1e-5 relative; nothing non-finite;
    zeros without FIX -- with latitude and longitude as ground distance (|dlat| 6.4e6, |dlon| cos(lat) 6.4e6 metres) against the same
    bound: at 89.9 S two correct solvers 1e-6 m apart differ by 1e-10 rad of longitude
    -> the per-field maxima (measured, and with a label recorded under $GPSX_WEDGE_PARITY_JSON, before anything is asserted)"""
    bound = FIX_BOUND_M if bound is None else bound
    fixed = (want["flags"] & F.F_FIX) != 0
    dq = np.abs(got["qr"][fixed] - want["qr"][fixed]) / np.maximum(np.abs(want["qr"][fixed]), 1e-30)
    d_rr = np.linalg.norm(got["rr"] - want["rr"], axis=1)
    worst = {"rr_m": float(d_rr.max()), "cdt_m": float(np.abs(got["dtr_s"] - want["dtr_s"]).max() * CLIGHT),
             "height_m": float(np.abs(got["geo"][:, 2] - want["geo"][:, 2]).max()),
             "lat_m": float(np.abs(got["geo"][:, 0] - want["geo"][:, 0]).max() * 6.4e6),
             "lon_m": float((np.abs(got["geo"][:, 1] - want["geo"][:, 1]) * np.cos(want["geo"][:, 0])).max() * 6.4e6),
             "half_resid_rms_m": float(np.abs(got["resid_rms_m"] - want["resid_rms_m"]).max() / 2.0), "qr_rel": float(dq.max()) if dq.size else 0.0,
             "n_iter": int(np.abs(got["n_iter"] - want["n_iter"]).max())}
    record_parity(label, stage, worst, FIX_FIELDS, None if names is None else names[int(np.argmax(d_rr))])
    for f in ("flags", "n_used", "used_mask", "ref_slot", "week", "reserved"):
        bad = np.flatnonzero(got[f] != want[f])
        assert bad.size == 0, (f, bad[:8], names and [names[b] for b in bad[:8]], got[f][bad][:8], want[f][bad][:8])
    assert got["rx_tow_s"].tobytes() == want["rx_tow_s"].tobytes(), "rx_tow_s"
    assert got_pr is None or got_pr.tobytes() == want_pr.tobytes(), "pr_m"
    assert np.isfinite(got["rr"]).all() and np.isfinite(got["geo"]).all() and np.isfinite(got["qr"]).all() and np.isfinite(got["resid_rms_m"]).all()
    assert worst["n_iter"] <= 1, (worst, np.flatnonzero(np.abs(got["n_iter"] - want["n_iter"]) > 1)[:8])
    assert max(worst[k] for k in FIX_FIELDS) <= bound and worst["qr_rel"] <= 1e-5, worst
    for f in ("rr", "dtr_s", "geo", "qr", "resid_rms_m"):
        assert not got[f][~fixed].any(), (f, "not zero without FIX")
    return worst


def compare_vel(got, want, label=None, names=None):
    """weighted_vel_cases.compare under this module's bound, recorded under $GPSX_WEDGE_PARITY_JSON"""
    worst = K.compare(got, want, bound=np.inf)
    record_parity(label, "vel", worst, ("vel_mps", "enu_mps", "cdrift_mps", "resid_rms_mps"),
                  None if names is None else names[int(np.argmax(np.abs(got["vel"] - want["vel"]).max(1)))])
    return K.compare(got, want, bound=VEL_BOUND_MPS)


# ---- bounds -----------------------------------------------------------------------------------------------------------------------
# MEASURED on the CPU (tests/test_weighted_edge_reference.py prints them; its bounds are 2 x these):
#   truth_m: the largest distance of the restatement's fix from the true site over the solved receivers of the launches 8 x 27 and 12 x 27,
#     noise-free.  What it is made of: the float32 code phase (half an ulp at 16 368 samples is 0.009 m of range) through the geometry.
#   sat_vel_mps, sat_clock_rate: weighted_vel_ref.satellites' velocity and clock rate against central differences (+- 0.5 s) of this
#     module's sat_state over every satellite of every receiver, e up to 0.4 and |tk| up to 7200.6 s.  What it is made of: the difference
#     quotient's truncation (jerk x h^2 / 6, larger at perigee of an eccentric orbit) and cancellation.
# Measured: 0.3122 m (t_half_after, eight satellites); satellite velocity 1.7652e-5 m/s (against 2.95e-6 at e <= 0.012), clock rate
# 8.475e-19 s/s; the injected 36 m/s and 1e-6 s/s come back within 2.222e-2 m/s and 1.915e-2 m/s of c drift (arctic_plus and munich_minus,
# eight satellites), the size weighted_vel_cases measured for 7.5 km/s receivers, because the terms of second order in 1 / c go with the
# square of the range rate and an orbit of e = 0.4 doubles it
MEASURED = {"truth_m": 0.31225, "sat_vel_mps": 1.7653e-5, "sat_clock_rate": 8.475e-19}
# the device against the restatement: 8 x the largest difference measured on one MI355X over every launch of tests/test_gpu_weighted_edges.py
# (profiles/r23_weighted_edges_parity.json, written under $GPSX_WEDGE_PARITY_JSON), under weighted_fix_cases' and weighted_vel_cases' caps
# and for their reasons
# Measured: fix 2.0862e-7 m (height, t_half_after from 30 km off, eight slots), fde 1.1630e-7 m (rr, pole_plus with a slot a millisecond off),
# vel 3.5982e-11 m/s (vel, pole_minus, eight slots) -- all below what weighted_fix_cases (7.63e-7 m), weighted_fde_cases (1.0325e-6 m) and
# weighted_vel_cases (9.131e-8 m/s) measured at their one instant
PARITY_MEASURED = {"fix_m": 2.0862e-7, "fde_m": 1.1630e-7, "vel_mps": 3.5982e-11}


def _bound(measured, cap):
    return cap if measured is None else min(8.0 * measured, cap)


FIX_BOUND_M = _bound(PARITY_MEASURED["fix_m"], W.PARITY_CAP_M)
FDE_BOUND_M = _bound(PARITY_MEASURED["fde_m"], W.PARITY_CAP_M)
VEL_BOUND_MPS = _bound(PARITY_MEASURED["vel_mps"], K.PARITY_CAP_MPS)
