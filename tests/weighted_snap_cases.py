"""The fabricated receivers of the snapshot fixes' tests (include/gpsx.h gpsx_wsnap; restated in tests/weighted_snap_ref.py): one row per
clause of the definition, each with a predicate on the outcome's own numbers; launches of any shape that hold the rows where they fit
and seeded random receivers elsewhere; the noise-free skies with their prior errors; the clearance that makes an exact comparison of
the device's integers with the restatement's fair; the comparison itself; the IF scenario; the smoke fixture.
tests/test_weighted_snap_reference.py asserts the predicates on the restatement, tests/test_gpu_weighted_snap.py on the device's bytes.

Two sources of code phases.  The rows and the random receivers take theirs from the restatement's own model at the true point and
instant (model_phases: any bank serves, the week's end included); what they test is decisions and bytes.  The skies and the scenario
take theirs from the synthesiser's truth (pvt_chain.travel_time, five passes of its own fixed point, its own geodetic and delays):
what they test is the method's error.

Clauses with a case of their own instead of a table row (a cfg, a prior or phases that the table's launch cannot hold): a candidate
below the horizon (below_horizon_case: el < 0, no row); rho <= 0 (rho_case: an orbit and a prior of 1e13 m, the prior perpendicular to
the satellite in the xy-plane, where the Sagnac term outweighs the range); an exact tie of rint in N_p (tie_case: CPU only, with
fractional phases chosen so that (pr + b0) / ms - s ends in exactly .5 -- no record's integer phase produces that on two libms at
once, so on the device decisions_clear keeps receivers that come near one out of the comparison).  NONFINITE has no constructed case:
it needs a sum or a dx that is not finite although every row's pr, el, az, rd and var are and |pr| < 1e12 (the routes there go through
orbit rates of 1e160 and would not be the same on two libms), or a |dt_s| beyond a week."""
import functools
import json
import os
from collections import namedtuple

import numpy as np

import pvt_chain as pc
import weighted_fix_cases as W
import weighted_snap_ref as S

N_PRN, N_DOPP = 10, 5                  # the canonical shape: what the predicates are proven at
PRNS = [11, 12, 13, 14, 15, 16, 17, 18, 19, 20]      # index p: Munich's sky's satellite p (0 .. 7), the one below the horizon (8), none (9)
DOPP_MIN_HZ, DOPP_STEP_HZ = -1000, 500
WEEK = pc.WEEK
EPOCH_S = 0.004
EL_MIN = 0.5236                        # 30 degrees: the sky's satellites stand at 28.0 .. 79.7, two of them under it
UNDER, ABOVE = (1, 2), (0, 3, 4, 5, 6, 7)
MAX_RESID_M = 1000.0
SEED_1_5_1 = 2                         # launch(1, 5, 1, seed=2): its one receiver has all five satellites detected and reaches FIX
MEAN, STRONG, WEAK = 300, 6000, 1000   # a record's mean over the phases; a detected peak (20 x); a noise row's (3.3 x)
PRIOR_OFF_M, PRIOR_OFF_S = (12000.0, -9000.0, 7000.0), -10.0
Row = namedtuple("Row", "name build check")      # build() -> receiver dict; check(outcome dict) -> bool


def table_cfg(**kw):
    return S.make_cfg(EPOCH_S, **dict(dict(el_min_rad=EL_MIN, max_resid_m=MAX_RESID_M, det=(4, 1), min_peak=0, min_sats=5), **kw))


# ---- receivers ---------------------------------------------------------------------------------------------------------------------------
def model_phases(bank_row, rr, t_s):
    """the code phases (samples, fractions and all) the restatement's own model gives the bank's satellites at the point rr and the
    instant t_s, and the milliseconds below them -> (tau [n], N [n], good [n])"""
    e = np.asarray(bank_row, S.EPH_DTYPE)
    have = ((e["flags"] & S.E.F_VALID) != 0)
    with np.errstate(all="ignore"):
        d = S.evaluate(e, have, np.asarray(rr, np.float64), np.float64(1000.0) * np.float64(t_s), S.F.ION_DEFAULT)
    u = np.where(d["good"], d["pr"], 0.0) / S.MS
    return (u - np.floor(u)) * 16368.0, np.floor(u).astype(np.int64), d["good"]


def whole(tau):
    """phases rounded to whole samples, inside 0 .. 16367: the grids' resolution"""
    return np.rint(tau).astype(np.int64) % 16368


def peak_rows(rng, taus, strong, bins=None, n_dopp=N_DOPP):
    """records [n_prn][n_dopp]: every row noise (max_val around WEAK at random phases, sum = 16368 MEAN: 3.3 x the mean, not detected at
    4 / 1), the PRNs of `strong` with a peak of STRONG at phase taus[p] in bin bins[p]"""
    n = len(taus)
    out = np.zeros((n, n_dopp), S.PEAK_DTYPE)
    out["max_val"] = rng.integers(WEAK - 50, WEAK + 50, (n, n_dopp))
    out["phase"] = rng.integers(0, 16368, (n, n_dopp))
    out["sum"], out["avr"] = 16368 * MEAN, MEAN
    for p in range(n):
        if strong[p]:
            b = int(bins[p]) if bins is not None else int(rng.integers(0, n_dopp))
            out["max_val"][p, b], out["phase"][p, b] = STRONG, int(taus[p])
    return out


@functools.lru_cache(maxsize=None)
def _munich_bank():
    bank = np.zeros(N_PRN, S.EPH_DTYPE)
    for p, (raw, _) in enumerate(W.sky("munich", 8, 0)):
        bank[p] = W.eph_record(raw)[0]
    bank[8] = W._below_horizon("munich")[1][0]
    return bank


def receiver(bank, rr_true, t_true, prior_rr, prior_tow, week=WEEK, strong=None, seed=0, shift=0, n_dopp=N_DOPP):
    """one receiver: the bank's satellites seen from rr_true at the instant t_true + EPOCH_S (model_phases, whole samples, all moved by
    `shift` samples: the common bias takes it), the PRNs of `strong` (default: every one with a VALID record) detected"""
    rng = np.random.default_rng([32, seed])
    tau, n_ms, good = model_phases(bank, rr_true, t_true + EPOCH_S)
    taus = (whole(tau) + shift) % 16368
    strong = good if strong is None else np.asarray(strong, bool)
    return dict(bank=np.array(bank, S.EPH_DTYPE), peaks=peak_rows(rng, taus, strong, n_dopp=n_dopp), prior=S.make_prior(prior_rr, week, prior_tow)[0],
                rr=np.asarray(rr_true, np.float64), t=float(t_true), taus=taus)


def munich(strong=None, off_m=PRIOR_OFF_M, off_s=PRIOR_OFF_S, seed=0, shift=0, bank=None):
    """the base receiver: Munich at weighted_fix_cases' instant, the prior 16 km and 10 s off"""
    rr = W.site_ecef("munich")
    return receiver(_munich_bank() if bank is None else bank, rr, W.TOW, rr + np.asarray(off_m), W.TOW + off_s, strong=strong, seed=seed, shift=shift)


def _with(rec, **ch):
    for k, v in ch.items():
        if k == "prior":
            for f, val in v.items():
                rec["prior"][f] = val
        elif k == "bank":
            for p, fields in v.items():
                if fields is None:
                    rec["bank"][p] = np.zeros(1, S.EPH_DTYPE)[0]
                elif isinstance(fields, int):
                    rec["bank"][p] = rec["bank"][fields]
                    rec["peaks"][p] = rec["peaks"][fields]
                else:
                    for f, val in fields.items():
                        rec["bank"][p][f] = val
        elif k == "peak":                # {p: dict(max_val=, sum=, phase=)} on the PRN's strongest record
            for p, fields in v.items():
                b = int(np.argmax(rec["peaks"]["max_val"][p]))
                for f, val in fields.items():
                    rec["peaks"][f][p, b] = val
        elif k == "phase_plus":          # {p: samples added to the PRN's peak's phase}
            for p, d in v.items():
                b = int(np.argmax(rec["peaks"]["max_val"][p]))
                rec["peaks"]["phase"][p, b] = (int(rec["peaks"]["phase"][p, b]) + d) % 16368
    return rec


def _only(*ps):
    return [p in ps for p in range(N_PRN)]


def _shift_to(p, target):
    """Munich with every phase moved so that satellite p's lands on `target`"""
    base = munich()
    return munich(shift=(target - int(base["taus"][p])) % 16368)


@functools.lru_cache(maxsize=None)
def _week_end():
    import weighted_edge_cases as X
    r = X.receiver("t_week_end")
    bank = np.zeros(N_PRN, S.EPH_DTYPE)
    bank[:8] = r["eph"][:8]
    return X.site_ecef(r["site"]), bank


def week_end():
    """the truth 1.2 s behind the week's end, the prior's clock 3 s slow of it in the week before... and the other way round: the prior
    2 s into the new week, the truth 1.2 s before it began -- dt_s = -3.2 takes tow_s below 0"""
    rr, bank = _week_end()
    return receiver(bank, rr, 604798.8, rr + np.asarray(PRIOR_OFF_M), 2.0, week=WEEK + 1)


def week_end_up():
    """the prior 3 s before the week's end, the truth 1.5 s after it: tow_s + dt_s >= 604800"""
    rr, bank = _week_end()
    return receiver(bank, rr, 604801.5, rr + np.asarray(PRIOR_OFF_M), 604797.0, week=WEEK)


FL = lambda o: int(o["snap"]["flags"])      # noqa: E731
SV = lambda o, p: int(o["sv"][p]["flags"])      # noqa: E731
ALL = S.SV_DETECTED | S.SV_HAVE_EPH | S.SV_CANDIDATE | S.SV_USED
MASK = lambda ps: sum(1 << p for p in ps)      # noqa: E731


def _err(o):
    return float(np.linalg.norm(o["snap"]["rr"] - o["rec"]["rr"]))


def _zero_but_flag(o):
    return o["snap"].tobytes()[4:] == bytes(124) and not o["sv"].tobytes().strip(b"\0")


def _fixed(o, used=ABOVE, bound_m=60.0, bound_s=0.05):
    """FIX on exactly these PRNs, within what whole-sample phases allow of the truth"""
    return (FL(o) == S.F_FIX and int(o["snap"]["used_mask"]) == MASK(used) and int(o["snap"]["n_used"]) == len(used) and _err(o) < bound_m
            and abs(float(o["snap"]["dt_s"]) - (o["rec"]["t"] - float(o["rec"]["prior"]["tow_s"]) + _wrap(o))) < bound_s
            and float(o["snap"]["resid_rms_m"]) < 30.0 and all(SV(o, p) & ~S.SV_REFERENCE == ALL for p in used))


def _wrap(o):
    d = o["rec"]["t"] - float(o["rec"]["prior"]["tow_s"])
    return -604800.0 if d > 302400.0 else (604800.0 if d < -302400.0 else 0.0)


ROWS = [
    Row("FIX: six satellites over el_min_rad, two under it, one below the horizon, one without a record", lambda: munich(),
        lambda o: _fixed(o) and int(o["snap"]["n_detected"]) == 9 and int(o["snap"]["n_candidates"]) == 6 and int(o["snap"]["ref"]) == 3
        and SV(o, 3) == ALL | S.SV_REFERENCE and all(SV(o, p) == S.SV_DETECTED | S.SV_HAVE_EPH for p in UNDER + (8,)) and SV(o, 9) == 0
        and int(o["snap"]["week"]) == WEEK and abs(float(o["snap"]["tow_s"]) - W.TOW) < 0.05 and 2 <= int(o["snap"]["n_iter"]) <= 6),
    Row("NO_PRIOR: no HAVE flag", lambda: _with(munich(), prior=dict(flags=0)), lambda o: FL(o) == S.F_NO_PRIOR and _zero_but_flag(o)),
    Row("NO_PRIOR: a flag bit beyond HAVE", lambda: _with(munich(), prior=dict(flags=3)), lambda o: FL(o) == S.F_NO_PRIOR and _zero_but_flag(o)),
    Row("NO_PRIOR: an rr that is not finite", lambda: _with(munich(), prior=dict(rr=(1.0, np.nan, 2.0))), lambda o: FL(o) == S.F_NO_PRIOR and _zero_but_flag(o)),
    Row("NO_PRIOR: a tow_s that is not finite", lambda: _with(munich(), prior=dict(tow_s=np.inf)), lambda o: FL(o) == S.F_NO_PRIOR and _zero_but_flag(o)),
    Row("NO_PRIOR: tow_s = 604800", lambda: _with(munich(), prior=dict(tow_s=604800.0)), lambda o: FL(o) == S.F_NO_PRIOR and _zero_but_flag(o)),
    Row("NO_PRIOR: week = -1", lambda: _with(munich(), prior=dict(week=-1)), lambda o: FL(o) == S.F_NO_PRIOR and _zero_but_flag(o)),
    Row("NO_PRIOR: week = 32768", lambda: _with(munich(), prior=dict(week=32768)), lambda o: FL(o) == S.F_NO_PRIOR and _zero_but_flag(o)),
    Row("NO_PRIOR: a reserved word", lambda: _with(munich(), prior=dict(reserved=(0, 1))), lambda o: FL(o) == S.F_NO_PRIOR and _zero_but_flag(o)),
    Row("detection at the threshold", lambda: _with(munich(), peak={3: dict(max_val=4 * MEAN, sum=16368 * MEAN)}),
        lambda o: _fixed(o) and (SV(o, 3) & S.SV_DETECTED) != 0),
    Row("detection one below the threshold", lambda: _with(munich(), peak={3: dict(max_val=4 * MEAN - 1, sum=16368 * MEAN)}),
        lambda o: _fixed(o, (0, 4, 5, 6, 7)) and SV(o, 3) == S.SV_HAVE_EPH and int(o["snap"]["n_detected"]) == 8 and int(o["snap"]["ref"]) == 7),
    Row("a PRN detected without an ephemeris", lambda: _with(munich(strong=[True] * N_PRN), bank={0: None}),
        lambda o: _fixed(o, (3, 4, 5, 6, 7)) and SV(o, 0) == S.SV_DETECTED and SV(o, 9) == S.SV_DETECTED and int(o["snap"]["n_detected"]) == 10),
    Row("an unhealthy satellite", lambda: _with(munich(), bank={3: dict(svh=1)}),
        lambda o: _fixed(o, (0, 4, 5, 6, 7)) and SV(o, 3) == S.SV_DETECTED | S.SV_HAVE_EPH and float(o["sv"][3]["el"]) == 0.0),
    Row("A <= 0: the pass fails", lambda: _with(munich(), bank={4: dict(A=0.0)}),
        lambda o: _fixed(o, (0, 3, 5, 6, 7)) and SV(o, 4) == S.SV_DETECTED | S.SV_HAVE_EPH),
    Row("|ps| < Re: the pass fails", lambda: _with(munich(), bank={4: dict(A=5.0e6)}),
        lambda o: _fixed(o, (0, 3, 5, 6, 7)) and SV(o, 4) == S.SV_DETECTED | S.SV_HAVE_EPH),
    Row("|tk| > 7201: the pass fails", lambda: _with(munich(), bank={5: dict(toes=float(_munich_bank()[5]["toes"]) - 14400.0)}),
        lambda o: _fixed(o, (0, 3, 4, 6, 7)) and SV(o, 5) == S.SV_DETECTED | S.SV_HAVE_EPH),
    Row("exactly min_sats", lambda: munich(strong=_only(0, 3, 4, 5, 6, 1, 8)),
        lambda o: _fixed(o, (0, 3, 4, 5, 6), bound_m=150.0) and int(o["snap"]["n_candidates"]) == 5),
    Row("one fewer than min_sats: TOO_FEW", lambda: munich(strong=_only(0, 3, 4, 5, 1, 2, 8)),
        lambda o: FL(o) == S.F_TOO_FEW and int(o["snap"]["n_candidates"]) == 4 and int(o["snap"]["n_iter"]) == 0 and int(o["snap"]["ref"]) == -1
        and int(o["snap"]["n_detected"]) == 7 and o["snap"].tobytes()[16:64] == bytes(48) and float(o["snap"]["tow_s"]) == float(o["rec"]["prior"]["tow_s"])
        and all(SV(o, p) == S.SV_DETECTED | S.SV_HAVE_EPH | S.SV_CANDIDATE for p in (0, 3, 4, 5))),
    Row("tau = 0", lambda: _shift_to(4, 0), lambda o: _fixed(o) and int(o["sv"][4]["phase"]) == 0),
    Row("tau = 16367", lambda: _shift_to(6, 16367), lambda o: _fixed(o) and int(o["sv"][6]["phase"]) == 16367),
    Row("a reference tie in el: the lower index", lambda: _with(munich(strong=_only(0, 3, 4, 5, 6, 7, 9)), bank={9: 3}),
        lambda o: _fixed(o, ABOVE + (9,)) and int(o["snap"]["ref"]) == 3 and float(o["sv"][9]["el"]) == float(o["sv"][3]["el"])
        and SV(o, 9) == ALL and int(o["sv"][9]["n_ms"]) == int(o["sv"][3]["n_ms"])),
    Row("one z_p 110 km off: RESID, the numbers stay", lambda: _with(munich(), phase_plus={5: 6000}),
        lambda o: FL(o) == S.F_RESID and float(o["snap"]["resid_rms_m"]) > 10.0 * MAX_RESID_M and int(o["snap"]["n_used"]) == 6
        and np.abs(o["snap"]["rr"]).max() > 1e6 and np.abs(o["sv"]["resid_m"]).max() > 1e4),
    Row("three code phases 55 to 150 km off: ten passes do not settle, NO_CONV", lambda: _with(munich(), phase_plus={5: 8100, 0: -7000, 7: 3000}),
        lambda o: FL(o) == S.F_NO_CONV and int(o["snap"]["n_iter"]) == 10 and int(o["snap"]["n_used"]) == 6 and o["snap"].tobytes()[24:64] == bytes(40)
        and o["snap"].tobytes()[72:] == bytes(56) and float(o["snap"]["tow_s"]) == float(o["rec"]["prior"]["tow_s"])),
    Row("a prior 300 km off, outside what step 3 resolves: wrong milliseconds, RESID", lambda: munich(off_m=(0.0, 0.0, 300000.0)),
        lambda o: FL(o) == S.F_RESID and float(o["snap"]["resid_rms_m"]) > 10.0 * MAX_RESID_M
        and any(int(o["sv"][p]["n_ms"]) != int(o["truth_n"][p]) + int(o["sv"][3]["n_ms"]) - int(o["truth_n"][3]) for p in ABOVE)),
    Row("coincident satellites: SINGULAR", lambda: _with(munich(strong=_only(0, 3, 4, 5, 6, 7, 9)), bank={0: 3, 4: 3, 5: 3, 6: 3, 7: 3, 9: 3}),
        lambda o: FL(o) == S.F_SINGULAR and int(o["snap"]["n_iter"]) == 1 and int(o["snap"]["n_used"]) == 7 and o["snap"].tobytes()[24:64] == bytes(40)
        and o["snap"].tobytes()[72:] == bytes(56)),
    Row("the week's end: tow_s + dt_s < 0", week_end,
        lambda o: FL(o) == S.F_FIX and int(o["snap"]["week"]) == WEEK and abs(float(o["snap"]["tow_s"]) - 604798.8) < 0.05 and _err(o) < 60.0
        and float(o["snap"]["dt_s"]) < -3.0),
    Row("the week's end: tow_s + dt_s >= 604800", week_end_up,
        lambda o: FL(o) == S.F_FIX and int(o["snap"]["week"]) == WEEK + 1 and abs(float(o["snap"]["tow_s"]) - 1.5) < 0.05 and _err(o) < 60.0
        and float(o["snap"]["dt_s"]) > 4.0),
]
assert len({r.name for r in ROWS}) == len(ROWS)


# ---- launches ------------------------------------------------------------------------------------------------------------------------------
class Launch:
    """n_rx receivers on a list of n_prn PRNs and n_dopp bins: prns (uint8), peaks [n_rx][n_prn][n_dopp], bank [n_rx][n_prn] (shared: [1][n_prn],
    bank_stride 0), prior [n_rx], rows [the Row a receiver holds, or None], recs [the receiver dicts]"""


def _random_receiver(rng, n_prn, n_dopp, shared_bank=None):
    """a receiver at one of the four sites (Munich under a shared bank) under 5 .. 12 satellites at random indices of the list, the prior up
    to 30 km and 20 s off; every ninth without a prior, every seventh with too few satellites, records unhealthy or missing among them"""
    if shared_bank is not None:
        site, bank = "munich", shared_bank
    else:
        site = sorted(W.SITES)[int(rng.integers(0, 4))]
        n_sats = int(rng.integers(5, min(n_prn, 12) + 1)) if n_prn >= 5 else n_prn
        sats = W.sky(site, 12, 3 * int(rng.integers(0, 4)))[:n_sats]
        bank = np.zeros(n_prn, S.EPH_DTYPE)
        for (raw, _), p in zip(sats, rng.permutation(n_prn)[:n_sats]):
            bank[p] = W.eph_record(raw)[0]
    rr = W.site_ecef(site)
    t = W.TOW + float(rng.uniform(-300.0, 300.0))
    direction = rng.normal(0.0, 1.0, 3)
    off = direction / np.linalg.norm(direction) * float(rng.uniform(0.0, 30000.0))
    bank = bank.copy()
    kind = int(rng.integers(0, 63))
    strong = ((bank["flags"] & S.E.F_VALID) != 0) | (rng.integers(0, 6, n_prn) == 0)
    if kind % 7 == 0:
        strong &= rng.integers(0, 2, n_prn) == 0
    if kind % 5 == 0:
        bank["svh"][int(rng.integers(0, n_prn))] = 1
    rec = receiver(bank, rr, t, rr + off, t + float(rng.uniform(-20.0, 20.0)), strong=strong, seed=int(rng.integers(0, 1 << 30)), n_dopp=n_dopp)
    if kind % 9 == 0:
        rec["prior"]["flags"] = 0
    return rec


def launch(n_rx, n_prn=N_PRN, n_dopp=N_DOPP, seed=0, shared=False, rows=True):
    """the rows in the first receivers where the shape holds them (not under a shared bank: a row's bank is its own), seeded random
    receivers behind them and in every other shape"""
    rng = np.random.default_rng([32, seed, n_rx, n_prn, n_dopp, int(shared)])
    la = Launch()
    la.n_rx, la.n_prn, la.n_dopp, la.bank_stride = n_rx, n_prn, n_dopp, 0 if shared else n_prn
    extra = [q for q in range(21, 100)]
    la.prns = np.array((PRNS + extra)[:n_prn] if n_prn >= N_PRN else extra[:n_prn], np.uint8)
    la.peaks, la.prior = np.zeros((n_rx, n_prn, n_dopp), S.PEAK_DTYPE), np.zeros(n_rx, S.PRIOR_DTYPE)
    shared_bank = None
    if shared:
        shared_bank = np.zeros(n_prn, S.EPH_DTYPE)
        src = _munich_bank()
        for k, p in enumerate(rng.permutation(n_prn)[:min(n_prn, 9)]):
            shared_bank[p] = src[k]
    la.bank = shared_bank[None].copy() if shared else np.zeros((n_rx, n_prn), S.EPH_DTYPE)
    la.rows, la.recs = [], []
    fits = rows and not shared and n_prn >= N_PRN and n_dopp == N_DOPP
    for r in range(n_rx):
        row = ROWS[r] if fits and r < len(ROWS) else None
        if row is not None:
            rec = row.build()
            la.peaks[r, :N_PRN], la.bank[r, :N_PRN], la.prior[r] = rec["peaks"], rec["bank"], rec["prior"]
            if n_prn > N_PRN:
                la.peaks[r, N_PRN:] = peak_rows(rng, np.zeros(n_prn - N_PRN, np.int64), np.zeros(n_prn - N_PRN, bool))
        else:
            rec = _random_receiver(rng, n_prn, n_dopp, shared_bank)
            la.peaks[r], la.prior[r] = rec["peaks"], rec["prior"]
            if not shared:
                la.bank[r] = rec["bank"]
        la.rows.append(row)
        la.recs.append(rec)
    return la


def run(la, cfg=None, want_sv=True):
    """the restatement on a launch -> (snap, sv, trace)"""
    trace = []
    snap, sv = S.snap(table_cfg() if cfg is None else cfg, la.prns, DOPP_MIN_HZ, DOPP_STEP_HZ, la.peaks, la.bank, la.bank_stride, la.prior, want_sv=want_sv,
                      trace=trace)
    return snap, sv, trace


def outcome(la, r, snap, sv, trace):
    rec = la.recs[r]
    _, truth_n, _ = model_phases(rec["bank"], rec["rr"], rec["t"] + EPOCH_S)
    return dict(snap=snap[r], sv=sv[r, :N_PRN], trace=trace[r], rec=rec, truth_n=truth_n)


def below_horizon_case():
    """(launch of one receiver, cfg): el_min_rad = -1.5, so the satellite below the horizon is a CANDIDATE -- and el < 0 leaves it without a row"""
    la = launch(1, rows=False)
    rec = munich()
    la.peaks[0], la.bank[0], la.prior[0], la.recs, la.rows = rec["peaks"], rec["bank"], rec["prior"], [rec], [None]
    return la, table_cfg(el_min_rad=-1.5)


def below_horizon_check(snap, sv):
    return (int(snap[0]["flags"]) == S.F_FIX and int(snap[0]["n_candidates"]) == 9 and int(snap[0]["n_used"]) == 8 and int(snap[0]["used_mask"]) == 0xFF
            and int(sv[0, 8]["flags"]) == S.SV_DETECTED | S.SV_HAVE_EPH | S.SV_CANDIDATE and float(sv[0, 8]["el"]) < -0.2 and float(sv[0, 8]["resid_m"]) == 0.0)


def _one(rec):
    la = launch(1, rows=False)
    la.peaks[0], la.bank[0], la.prior[0], la.recs, la.rows = rec["peaks"], rec["bank"], rec["prior"], [rec], [None]
    return la


RHO_SAT = 4


def rho_case(mirrored=False):
    """(launch of one receiver, cfg): satellite 4 on an orbit of A = 1e13 m, the prior 1e13 m out, perpendicular to the satellite in the
    xy-plane on the side where we (ps_x x_1 - ps_y x_0) / c is negative: rho <= 0 and the pass fails.  mirrored: the other side, where the
    same satellite's pass does not fail -- so it is this rule and no other"""
    rec = munich()
    rec["bank"][RHO_SAT]["A"] = 1e13
    with np.errstate(all="ignore"):
        d = S.evaluate(rec["bank"], np.arange(N_PRN) == RHO_SAT, np.array([1e13, 0.0, 0.0]), np.float64(1000.0) * (np.float64(rec["prior"]["tow_s"]) + np.float64(EPOCH_S)),
                       S.F.ION_DEFAULT)
    ps = d["passes"][0]["ps"][RHO_SAT]
    rr = np.array([ps[1], -ps[0], 0.0]) * (-1.0 if mirrored else 1.0)
    rec["prior"]["rr"] = rr / np.linalg.norm(rr) * 1e13
    return _one(rec), table_cfg()


def rho_check(sv, trace, mirrored=False):
    """the satellite is DETECTED | HAVE_EPH without CANDIDATE because rho <= 0: it has a position outside the Earth, a range, and the sign"""
    p0 = trace[0]["pass0"]
    ps = p0["ps"][RHO_SAT]
    there = float(np.linalg.norm(ps)) > S.P.RE and bool(np.isfinite(ps).all()) and bool(trace[0]["sel"][RHO_SAT])
    if mirrored:
        return there and float(p0["rho"][RHO_SAT]) > 0.0 and bool(p0["good"][RHO_SAT])
    return (there and float(p0["rho"][RHO_SAT]) < -1e11 and not bool(p0["good"][RHO_SAT])
            and int(sv[0, RHO_SAT]["flags"]) == S.SV_DETECTED | S.SV_HAVE_EPH and int(sv[0, RHO_SAT]["n_ms"]) == 0)


def tie_case():
    """CPU only -> (launch, cfg, tau [1][n_prn], want {PRN index: N_p}): Munich with the model's fractional phases, and for every candidate
    but the reference a phase moved so that (pr + b0) / ms - s is k + 0.5 in exactly that double; rint takes it to the even neighbour:
    down where k is even, up where it is odd"""
    la, cfg = _one(munich()), table_cfg()
    rec = la.recs[0]
    tau, _, _ = model_phases(rec["bank"], rec["rr"], rec["t"] + EPOCH_S)
    trace = []
    snap, _ = S.snap(cfg, la.prns, DOPP_MIN_HZ, DOPP_STEP_HZ, la.peaks, la.bank, la.bank_stride, la.prior, trace=trace, tau=tau[None])
    t, ref, want = trace[0], int(snap[0]["ref"]), {}
    for p in ABOVE:
        if p == ref:
            continue
        w = (t["pr0"][p] + np.float64(t["b0"])) / S.MS
        k = np.floor(w - 0.5)
        c = np.float64((w - (k + 0.5)) * 16368.0)
        for c in [c] + [f(c, n) for n in range(1, 200) for f in (_up, _down)]:
            if 0.0 <= c < 16368.0 and w - c / 16368.0 == k + 0.5:
                tau[p], want[p] = c, int(k) if int(k) % 2 == 0 else int(k) + 1
                break
    return la, cfg, tau[None], want


def _up(c, n):
    for _ in range(n):
        c = np.nextafter(c, np.inf)
    return c


def _down(c, n):
    for _ in range(n):
        c = np.nextafter(c, -np.inf)
    return c


# the launches of tests/test_gpu_weighted_snap.py's sweep: (n_rx, n_prn, n_dopp, shared bank, d_sv, seed).  Four receivers a workgroup: a
# second one from 5 on, 65 at 257; the PRN lanes end at 64 and two rows are read a turn (odd and even n_prn); a row's bins are strided
# over 64 lanes (1 and 21 bins).  The seeds: the restatement alone leaves at most 5 % of each out (tests/test_weighted_snap_reference.py
# checks every one of them on the CPU), and the one-receiver launch at n_prn = 5 reaches FIX
GPU_SHAPES = [(0, N_PRN, N_DOPP, False, True, 1),      # n_rx 0: the table (len(ROWS) receivers), the canonical shape
              (0, N_PRN, N_DOPP, False, False, 1),
              (1, 5, 1, False, True, SEED_1_5_1),
              (2, 8, 21, True, True, 1),
              (5, 33, 21, False, True, 1),
              (5, 64, 1, True, False, 1),
              (257, 8, 1, False, True, 1),
              (257, 12, 21, True, True, 1),
              (40, 64, 21, False, True, 1)]
GPU_OTHER = [(40, 33, 21, False, True, 4), (-9, N_PRN, N_DOPP, False, True, 0)]      # the second call's launch; the table + 9 (n_rx -9)


def gpu_launch(shape):
    """-> (launch, cfg, whether it is the table) of one GPU_SHAPES / GPU_OTHER entry"""
    n_rx, n_prn, n_dopp, shared, _, seed = shape
    table = n_rx <= 0
    la = launch(len(ROWS) - n_rx if table else n_rx, n_prn, n_dopp, seed=seed, shared=shared, rows=table)
    return la, (table_cfg() if table else table_cfg(el_min_rad=0.0873)), table


# ---- clearance: what makes an exact comparison of the integers fair -------------------------------------------------------------------------
PARITY_ENV = "GPSX_WSNAP_PARITY_JSON"      # a path: every labelled compare() records its maxima there (how the profile is written)
PARITY_CAP_M = 1e-4                        # weighted_fix_cases' cap
ANGLE_CLEAR, TIE_CLEAR, RESID_CLEAR, CONV_CLEAR, PIVOT_CLEAR = 1e-9, 1e-9, 1e-3, 1.1, 10.0
MAX_LEFT_OUT = 0.05


def _receiver_clear(t):
    """one receiver's trace against the thresholds (see decisions_clear)"""
    if t is None:
        return True
    ok = True
    el0 = t["el0"][t["good0"]]
    ok &= bool((np.abs(el0 - t["el_min"]) > ANGLE_CLEAR).all())
    if "u" in t:
        cand = t["good0"] & (t["el0"] >= t["el_min"])
        u = t["u"][cand]
        ok &= bool((0.5 - np.abs(u - np.rint(u)) > TIE_CLEAR).all())
        top = np.sort(t["el0"][cand])[::-1]
        ok &= len(top) < 2 or top[0] - top[1] > ANGLE_CLEAR or t.get("tie_is_exact", False)
    for k, ps in enumerate(t["passes"]):
        rows = ps["row"] | (ps["good"] & (np.abs(ps["el"]) <= ANGLE_CLEAR))
        ok &= bool((np.abs(ps["el"][rows]) > ANGLE_CLEAR).all())
        if ps["row"].sum() >= 5 and k < len(t["passes"]) - 1 or (k == len(t["passes"]) - 1 and t["flags"] not in (S.F_FIX, S.F_RESID)):
            sh = ps["shares"]
            ok &= all(not np.isfinite(s) or abs(np.log10(max(s, 1e-300) / S.PIVOT)) > np.log10(PIVOT_CLEAR) for s in sh[1:]) or sh[0] <= 0.0
            dx = ps["dx"]
            if np.isfinite(dx).all():
                norm = float(dx[0] * dx[0] + dx[1] * dx[1] + dx[2] * dx[2] + dx[3] * dx[3] + (1000.0 * dx[4]) ** 2)
                ok &= norm == 0.0 or abs(np.log10(max(norm, 1e-300) / 1e-8)) > np.log10(CONV_CLEAR)
    if t["flags"] in (S.F_FIX, S.F_RESID):
        ok &= abs(t["rms"] / t["max_resid_m"] - 1.0) > RESID_CLEAR
    return bool(ok)


def decisions_clear(la, cfg, snap, trace):
    """every decision of a launch that the device takes on doubles stands clear of its threshold in the restatement: el against
    el_min_rad at the prior and against 0 in every pass (1e-9 rad: 2 cm of a 2e7 m range), the two highest candidates' elevations
    against each other unless they are the same bits (the reference's choice), (pr + b0) / ms - s against a tie of rint (1e-9 ms: 0.3 mm of range),
    the pivots' shares against 1e-10 (a factor 10), the step's squared length against 1e-8 (a factor 1.1: two correct
    implementations stand 1e-9 m apart when the step is 1e-4 m long, 1e-5 of it), resid_rms_m against max_resid_m (1e-3 relative) -> the receivers that are NOT clear"""
    c = np.asarray(cfg, S.CFG_DTYPE).reshape(1)[0]
    out = []
    for r in range(la.n_rx):
        t = trace[r]
        if t is not None:
            t["el_min"], t["flags"], t["rms"] = float(c["el_min_rad"]), int(snap[r]["flags"]), float(snap[r]["resid_rms_m"])
            cand = t["good0"] & (t["el0"] >= t["el_min"])
            top = np.argsort(-t["el0"] - 10.0 * cand)[:2] if cand.sum() >= 2 else []
            t["tie_is_exact"] = len(top) == 2 and float(t["el0"][top[0]]) == float(t["el0"][top[1]])
        if not _receiver_clear(t):
            out.append(la.rows[r].name if la.rows[r] is not None else r)
    return out


# ---- the device against the restatement ---------------------------------------------------------------------------------------------------
SNAP_INT_FIELDS = ("flags", "week", "n_detected", "n_candidates", "n_used", "n_iter", "ref", "used_mask")
SV_INT_FIELDS = ("flags", "n_ms", "phase", "dopp_hz", "reserved")


def _record_parity(label, worst, n):
    path = os.environ.get(PARITY_ENV)
    if not path or label is None:
        return
    doc = json.load(open(path)) if os.path.exists(path) else {"launches": {}}
    doc["launches"][str(label)] = dict(worst, solved=n)
    doc["what"] = ("largest |device - restatement| in rr (m), b_m (m), 1000 m/s x dt_s (m), tow_s (s), geo, resid_rms_m, el / az (rad), resid_m and the float "
                   "qr (relative) per compared launch of tests/test_gpu_weighted_snap.py, one MI355X; written by weighted_snap_cases.compare under $" + PARITY_ENV)
    doc["largest_m"] = max(max(w["rr_m"], w["b_m"], w["dt_m"]) for w in doc["launches"].values())
    doc["cap_m"] = PARITY_CAP_M
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)


def compare(got, got_sv, want, want_sv, skip=(), label=None):
    """a launch's records against the restatement's: every integer field, flag, mask and N_p equal; rr, b_m and 1000 m/s x dt_s within
    PARITY_CAP_M; tow_s within the cap over 1000 m/s; geo[2], resid_rms_m and resid_m within 10 x the cap (they follow rr through the
    geometry), geo[0..1], el and az within the cap over 6.3e6 m x 50; qr 1e-4 relative; records without a solution byte for byte;
    nothing non-finite.  skip: receivers left out (decisions_clear's).  -> the per-field maxima (measured and, with a label, recorded
    under $GPSX_WSNAP_PARITY_JSON, before anything is asserted)"""
    keep = np.array([r not in skip for r in range(len(want))])
    g, w = got[keep], want[keep]
    for f in ("rr", "b_m", "dt_s", "tow_s", "geo", "resid_rms_m", "qr"):
        assert np.isfinite(got[f]).all(), f
    solved = (w["flags"] & (S.F_FIX | S.F_RESID)) != 0
    gs, ws = g[solved], w[solved]
    mx = lambda a: float(np.abs(a).max()) if a.size else 0.0      # noqa: E731
    worst = {"rr_m": mx(gs["rr"] - ws["rr"]), "b_m": mx(gs["b_m"] - ws["b_m"]), "dt_m": 1000.0 * mx(gs["dt_s"] - ws["dt_s"]), "tow_s": mx(gs["tow_s"] - ws["tow_s"]),
             "height_m": mx(gs["geo"][:, 2] - ws["geo"][:, 2]), "latlon_rad": mx(gs["geo"][:, :2] - ws["geo"][:, :2]),
             "resid_rms_m": mx(gs["resid_rms_m"] - ws["resid_rms_m"]),
             "qr_rel": mx((gs["qr"].astype(np.float64) - ws["qr"]) / np.maximum(np.abs(ws["qr"].astype(np.float64)), 1e-30))}
    if got_sv is not None:
        gv, wv = got_sv[keep], want_sv[keep]
        for f in ("el", "az", "resid_m"):
            assert np.isfinite(got_sv[f]).all(), f
        daz = np.abs(gv["az"] - wv["az"])
        worst.update({"el_rad": mx(gv["el"] - wv["el"]), "az_rad": mx(np.minimum(daz, 2 * S.P.PI - daz)), "resid_m": mx(gv["resid_m"] - wv["resid_m"])})
    _record_parity(label, worst, int(solved.sum()))
    for f in SNAP_INT_FIELDS:
        bad = np.flatnonzero(g[f] != w[f])
        assert bad.size == 0, (label, f, np.flatnonzero(keep)[bad][:8], g[f][bad][:8], w[f][bad][:8])
    assert g[~solved].tobytes() == w[~solved].tobytes(), "records without a solution"
    assert max(worst["rr_m"], worst["b_m"], worst["dt_m"]) <= PARITY_CAP_M and worst["tow_s"] <= PARITY_CAP_M / 1000.0, (label, worst)
    assert max(worst["height_m"], worst["resid_rms_m"]) <= 10.0 * PARITY_CAP_M and worst["latlon_rad"] <= PARITY_CAP_M / 6.3e6 * 50.0, (label, worst)
    assert worst["qr_rel"] <= 1e-4, (label, worst)
    if got_sv is not None:
        for f in SV_INT_FIELDS:
            bad = np.argwhere(gv[f] != wv[f])
            assert bad.size == 0, (label, f, bad[:8])
        assert max(worst["el_rad"], worst["az_rad"]) <= PARITY_CAP_M / 6.3e6 * 50.0 and worst["resid_m"] <= 10.0 * PARITY_CAP_M, (label, worst)
    return worst


# ---- the method's error: noise-free skies against the synthesiser's truth ----------------------------------------------------------------------
SKY_SATS = (5, 8, 12)
PRIOR_KM, PRIOR_S = (10.0, 50.0, 100.0), (-60.0, -20.0, 20.0, 60.0)
DIRECTION_SEED = 5
LIMIT_M = 150000.0                     # step 3's: half a millisecond of combined error in a range difference
# MEASURED, each on the CPU against pvt_chain.travel_time's truth (tests/test_weighted_snap_reference.py prints them):
#   exact_m / exact_s: the largest position and time error over the four sites x 5 / 8 / 12 satellites x the twelve prior errors with the
#     truth's own fractional phases -- the two models' difference (five passes against three, two ecef2pos) and round-off;
#   whole_m / whole_s: the same with the phases rounded to whole samples (a sample is 18.3 m of range), the error the stage really has;
#   scenario_m / scenario_s: the IF scenario's (six satellites through the two-bit front end, 8 blocks, 1 x 8 hybrid grid).
MEASURED = {"exact_m": 3.6428e-4, "exact_s": 1.4278e-7, "whole_m": 93.119, "whole_s": 0.016172, "scenario_m": 530.55, "scenario_s": 0.12639}
BOUNDS = {"noise_free_m": None, "noise_free_s": None, "whole_m": None, "whole_s": None, "scenario_m": None, "scenario_s": None}


def _set_bounds():
    if MEASURED["exact_m"] is not None:
        BOUNDS["noise_free_m"], BOUNDS["noise_free_s"] = 2.0 * MEASURED["exact_m"], 2.0 * MEASURED["exact_s"]
    for k in ("whole", "scenario"):
        if MEASURED[k + "_m"] is not None:
            BOUNDS[k + "_m"], BOUNDS[k + "_s"] = 1.5 * MEASURED[k + "_m"], 1.5 * MEASURED[k + "_s"]


def truth_phases(site, n_sats, seed0, t_s):
    """the synthesiser's truth for a sky at the instant t_s: (bank [n], fractional phases in samples, whole milliseconds, rows)"""
    rx = W.site_ecef(site)
    sats = W.sky(site, n_sats, seed0)
    bank = np.concatenate([W.eph_record(raw) for raw, _ in sats])
    lag = np.array([float(tau[0] - dts[0]) for tau, dts, _ in (pc.travel_time(row, rx, np.array([t_s])) for _, row in sats)])
    u = lag * 1000.0
    return bank, (u - np.floor(u)) * 16368.0, np.floor(u).astype(np.int64), [row for _, row in sats]


def prior_errors():
    """the twelve (offset vector in m, offset in s) of the noise-free runs: 10 / 50 / 100 km in a seeded direction each, +-20 / 60 s"""
    rng = np.random.default_rng(DIRECTION_SEED)
    out = []
    for km in PRIOR_KM:
        for s in PRIOR_S:
            d = rng.normal(0.0, 1.0, 3)
            out.append((d / np.linalg.norm(d) * km * 1000.0, s))
    return out


def difference_error_m(site, rows, t_s, off_m, off_s):
    """the combined error of the prior in a range difference, from the synthesiser's geometry alone: the largest over the satellites p of
    |(rho_p - rho_ref)(prior point, prior time) - (rho_p - rho_ref)(truth)|, rho the travel time's range and clock and ref the satellite
    that stands highest over the prior point (no atmosphere: the synthesiser's troposphere is not defined 100 km up, and it is metres)"""
    def lag(rr, t):
        out = [pc.travel_time(row, rr, np.array([t]), atmosphere=False) for row in rows]
        return np.array([float(tau[0] - dts[0]) for tau, dts, _ in out]) * S.C_LIGHT, np.array([float(el[0]) for _, _, el in out])
    rx = np.asarray(W.site_ecef(site), np.float64)
    at_prior, el = lag(rx + np.asarray(off_m, np.float64), float(t_s) + float(off_s))
    d = at_prior - lag(rx, float(t_s))[0]
    return float(np.abs(d - d[int(np.argmax(el))]).max())


def sky_run(site, n_sats, seed0, off_m, off_s, exact, cfg=None):
    """one noise-free receiver through the restatement -> (snap record, sv records, truth's whole milliseconds)"""
    t = W.TOW
    bank, tau, n_ms, _ = truth_phases(site, n_sats, seed0, t + EPOCH_S)
    peaks = peak_rows(np.random.default_rng(1), whole(tau), np.ones(n_sats, bool), n_dopp=1)
    prior = S.make_prior(W.site_ecef(site) + off_m, WEEK, t + off_s)
    cfg = S.make_cfg(EPOCH_S, el_min_rad=0.0873, max_resid_m=MAX_RESID_M) if cfg is None else cfg
    snap, sv = S.snap(cfg, list(range(1, n_sats + 1)), 0, 500, peaks[None], bank[None], n_sats, prior, tau=tau[None] if exact else None)
    return snap[0], sv[0], n_ms


def sky_errors(snap, site):
    return float(np.linalg.norm(snap["rr"] - W.site_ecef(site))), abs(float(snap["tow_s"]) - W.TOW)


# ---- the IF scenario: six satellites through the two-bit front end, eight blocks, a 1 x 8 hybrid grid ---------------------------------------------
SCEN_SEED, SCEN_BLOCKS, SCEN_GRID = 50, 8, (-5000, 500, 21)      # (seed 50: pick_satellites returns six within 0.2 s; most seeds take minutes)
SCEN_OFF_M, SCEN_OFF_S = (30000.0, -28000.0, 28565.7), 20.0       # 50 km


@functools.lru_cache(maxsize=None)
def scenario():
    """dict(prns, blocks [8][4092], bank [6], prior [1], cfg, truth_n [6]: the whole milliseconds of the truth's travel times at the middle
    of the eight blocks, first: the synthesiser's (Doppler, code delay) per satellite at block 0)"""
    import weighted_pvt_cases as PV
    sats = pc.pick_satellites(PV.RX, PV.TOW0, 6, seed=SCEN_SEED)
    blocks, first = pc.make_if_from_orbits(SCEN_BLOCKS, sats, PV.RX, PV.TOW0, amp=PV.AMPLITUDE, noise_amp=PV.NOISE_AMP, seed=PV.NOISE_SEED, cycle=PV.CYCLE,
                                           two_bit=True, mag_threshold=PV.MAG_THRESHOLD)
    bank = np.concatenate([W.eph_record(raw) for raw, _ in sats])
    lag = np.array([float(tau[0] - dts[0]) for tau, dts, _ in (pc.travel_time(row, PV.RX, np.array([PV.TOW0 + EPOCH_S])) for _, row in sats)])
    prior = S.make_prior(np.asarray(PV.RX, np.float64) + np.asarray(SCEN_OFF_M), WEEK, PV.TOW0 + SCEN_OFF_S)
    return dict(prns=np.array([row["sat"] for _, row in sats], np.uint8), blocks=blocks, bank=bank, prior=prior, first=first,
                cfg=S.make_cfg(EPOCH_S, el_min_rad=0.0873, max_resid_m=MAX_RESID_M, det=(4, 1), min_sats=5), truth_n=np.floor(lag * 1000.0).astype(np.int64),
                rr=np.asarray(PV.RX, np.float64), t=float(PV.TOW0))


def scenario_check(sc, snap, sv):
    """FIX, all six used, the milliseconds the truth's (N_p - N_ref against the travel times': the common bias may hold whole
    milliseconds) -> (position error in m, time error in s)"""
    assert int(snap["flags"]) == S.F_FIX and int(snap["n_used"]) == 6 and int(snap["used_mask"]) == 63, (snap, sv)
    ref = int(snap["ref"])
    assert [int(v) - int(sv["n_ms"][ref]) for v in sv["n_ms"]] == [int(v) - int(sc["truth_n"][ref]) for v in sc["truth_n"]], (sv["n_ms"], sc["truth_n"])
    return float(np.linalg.norm(snap["rr"] - sc["rr"])), abs(float(snap["tow_s"]) - sc["t"])


# ---- the smoke fixture ----------------------------------------------------------------------------------------------------------------------------
def smoke_case():
    """the smoke run's launch: every row and seven random receivers behind them, a second workgroup and more"""
    return launch(len(ROWS) + 7, seed=32)


def write_smoke(path):
    """tests/golden/wsnap_smoke.npz: the launch and the restatement's answer"""
    la = smoke_case()
    cfg = table_cfg()
    snap, sv, trace = run(la, cfg)
    unclear = decisions_clear(la, cfg, snap, trace)
    skip = np.array([r for r in range(la.n_rx) if (la.rows[r].name if la.rows[r] is not None else r) in unclear], np.int32)
    np.savez_compressed(path, cfg=cfg, prns=la.prns, dopp=np.array([DOPP_MIN_HZ, DOPP_STEP_HZ], np.int32), peaks=la.peaks, bank=la.bank, prior=la.prior,
                        snap=snap, sv=sv, skip=skip)


_set_bounds()
