"""The fabricated receivers of the tests of the two stages that close the weighted chain's loop (include/gpsx.h gpsx_wbank, gpsx_wpred;
restated in tests/weighted_pred_ref.py): per stage one row per clause of the definition, each with a predicate on the outcome's own
numbers, and launches of any shape that hold the rows where they fit and seeded random receivers elsewhere.  The bank's records are
random bytes (NaN patterns among the doubles included): the stage moves records and never evaluates them, so any byte it changes or
mixes up shows.  The prediction's receivers stand in Munich under weighted_fix_cases' sky (and at the week's end under
weighted_edge_cases'), with filter states made by hand; below the table: the closure with the filter's own rows, the clearance that
makes a byte-for-byte comparison with the device fair (and the re-seeding that keeps it), the comparison itself with its measured
parity bound, and the physics on weighted_pvt_cases' IF stream.  tests/test_weighted_pred_reference.py asserts the predicates on the
restatements, tests/test_gpu_weighted_pred.py on the device's bytes."""
from collections import namedtuple

import numpy as np

import weighted_pred_ref as P

CH, N_PRN = 4, 5                       # the canonical shape: what the predicates are proven at
PRNS = [3, 7, 19, 30, 210]
UNLISTED = 5
V, VN, NEW_ONLY = P.F_VALID, P.F_VALID | P.F_NEW, P.F_NEW

Slot = namedtuple("Slot", "prn flags toe ttr", defaults=(0, 0))
Row = namedtuple("Row", "name slots bank check")      # slots: [Slot]; bank: {PRN index: (toe, ttr)}; check(outcome) -> bool
Outcome = namedtuple("Outcome", "eph bank_before bank_after out rep trace")   # one receiver's: [ch], [n_prn], [n_prn], [ch], item, dict


def record(rng, flags, toe=0, ttr=0):
    """one EPH_DTYPE record of random bytes with these flags, toe_time and ttr_time"""
    rec = np.frombuffer(rng.bytes(P.EPH_DTYPE.itemsize), P.EPH_DTYPE).copy()
    rec["flags"], rec["toe_time"], rec["ttr_time"] = flags, toe, ttr
    return rec[0]


def _same(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def _is_stored(o, p, j):
    """bank entry p is slot j's record with flags = VALID, and the report says so"""
    return _same(o.bank_after[p], P.stored_form(o.eph[j])) and (int(o.rep["stored_mask"]) >> p) & 1 == 1 and (int(o.rep["have_mask"]) >> p) & 1 == 1


def _kept(o, p):
    """bank entry p is what it was, and not reported as stored"""
    return _same(o.bank_after[p], o.bank_before[p]) and (int(o.rep["stored_mask"]) >> p) & 1 == 0


def _own(o, j):
    return _same(o.out[j], o.eph[j]) and (int(o.rep["from_bank_mask"]) >> j) & 1 == 0


def _banked(o, j, p):
    return _same(o.out[j], o.bank_after[p]) and (int(o.rep["from_bank_mask"]) >> j) & 1 == 1 and int(o.out[j]["flags"]) == V


E = Slot(P.PRN_NONE, 0)              # an empty slot
BIG = (1 << 32) + 1                  # toe_times that differ in the high word only from small ones: the comparison is on 64 bits

ROWS = [
    Row("NEW enters", [Slot(3, VN, 1000, 11), E, E, E], {},
        lambda o: _is_stored(o, 0, 0) and int(o.bank_after[0]["flags"]) == V and int(o.rep["n_stored"]) == 1 and int(o.rep["n_have"]) == 1 and _own(o, 0)),
    Row("VALID without NEW enters an empty entry", [E, Slot(7, V, 1000, 11), E, E], {},
        lambda o: _is_stored(o, 1, 1) and int(o.rep["stored_mask"]) == 2 and _own(o, 1)),
    Row("an older toe is refused", [Slot(3, VN, 999, 50), E, E, E], {0: (1000, 11)},
        lambda o: _kept(o, 0) and int(o.rep["have_mask"]) == 1 and int(o.rep["n_stored"]) == 0 and _own(o, 0) and o.trace["refused"] == [0]),
    Row("an equal toe refreshes", [Slot(3, V, 1000, 77), E, E, E], {0: (1000, 11)},
        lambda o: _is_stored(o, 0, 0) and int(o.bank_after[0]["ttr_time"]) == 77 and int(o.bank_before[0]["ttr_time"]) == 11),
    Row("a newer toe replaces", [Slot(3, V, 1001, 5), E, E, E], {0: (1000, 11)},
        lambda o: _is_stored(o, 0, 0) and int(o.bank_after[0]["toe_time"]) == 1001),
    Row("toe_time is compared as a signed 64-bit number: newer", [Slot(3, V, 3), Slot(7, V, BIG), E, E], {0: (-5, 0), 1: (2, 0)},
        lambda o: _is_stored(o, 0, 0) and _is_stored(o, 1, 1)),
    Row("toe_time is compared as a signed 64-bit number: older", [Slot(3, V, -5), Slot(7, V, 2), E, E], {0: (3, 0), 1: (BIG, 0)},
        lambda o: _kept(o, 0) and _kept(o, 1) and o.trace["refused"] == [0, 1]),
    Row("two slots with one PRN, the later slot newer", [Slot(19, V, 100, 1), E, Slot(19, VN, 200, 2), E], {},
        lambda o: _is_stored(o, 2, 2) and o.trace["winner"] == {2: 2} and int(o.rep["n_stored"]) == 1),
    Row("two slots with one PRN, the earlier slot newer", [Slot(19, V, BIG, 1), E, Slot(19, VN, 200, 2), E], {},
        lambda o: _is_stored(o, 2, 0) and o.trace["winner"] == {2: 0}),
    Row("two slots with one PRN at equal toe: the lowest slot", [E, Slot(30, V, 100, 1), E, Slot(30, V, 100, 2)], {},
        lambda o: _is_stored(o, 3, 1) and int(o.bank_after[3]["ttr_time"]) == 1 and not _same(o.eph[1], o.eph[3])),
    Row("an unlisted PRN and GPSX_PRN_NONE are ignored", [Slot(UNLISTED, VN, 1000), Slot(P.PRN_NONE, V, 1000), Slot(0, V, 1000), Slot(-3, V, 9)], {},
        lambda o: int(o.rep["stored_mask"]) == 0 and int(o.rep["have_mask"]) == 0 and not o.bank_after["flags"].any() and all(_own(o, j) for j in range(4))),
    Row("an invalid slot keeps the bank's entry", [Slot(3, 0, 5000), Slot(7, NEW_ONLY, 5000), E, E], {0: (1000, 11), 1: (1000, 12)},
        lambda o: _kept(o, 0) and _kept(o, 1) and _banked(o, 0, 0) and _banked(o, 1, 1) and int(o.rep["n_from_bank"]) == 2),
    Row("merge: a VALID record of its own stays, even an older one", [Slot(3, V, 999, 50), Slot(UNLISTED, 0, 7), E, E], {0: (1000, 11)},
        lambda o: _own(o, 0) and _own(o, 1) and not _same(o.out[0], o.bank_after[0])),
    Row("merge: the bank's record where the slot has none", [Slot(210, 0), E, E, E], {4: (1000, 11)},
        lambda o: _banked(o, 0, 4) and int(o.rep["from_bank_mask"]) == 1),
    Row("merge: neither has one", [Slot(3, 0, 44), Slot(7, NEW_ONLY, 45), E, E], {2: (1000, 11)},
        lambda o: _own(o, 0) and _own(o, 1) and int(o.rep["from_bank_mask"]) == 0 and int(o.rep["have_mask"]) == 4),
    Row("merge: the record another slot stored in this call", [Slot(19, 0), Slot(19, VN, 300, 9), E, Slot(19, 0)], {2: (200, 1)},
        lambda o: _is_stored(o, 2, 1) and _banked(o, 0, 2) and _banked(o, 3, 2) and _own(o, 1) and _same(o.out[0], P.stored_form(o.eph[1]))),
    Row("every slot offers, every entry is replaced", [Slot(3, V, 10), Slot(7, V, 10), Slot(19, VN, 10), Slot(30, V, 10)], {0: (1, 0), 1: (10, 0), 3: (9, 0)},
        lambda o: int(o.rep["stored_mask"]) == 0b1111 and int(o.rep["have_mask"]) == 0b1111 and int(o.rep["from_bank_mask"]) == 0),
]
assert len({r.name for r in ROWS}) == len(ROWS)


class Launch:
    """n_rx receivers of ch slots on a list of n_prn PRNs: prns (uint8), slot_prns [n_rx * ch], eph [n_rx * ch], bank [n_rx][n_prn],
    rows [the Row a receiver holds, or None]"""


def _random_receiver(rng, ch, prns):
    """slots and a bank of every kind, seeded: listed PRNs (some twice), unlisted ones and empty slots, records with and without VALID
    and NEW, toe_times drawn from a few values so that older, equal and newer meet"""
    n_prn = len(prns)
    unlisted = [q for q in range(1, 211) if q not in prns] or [0]
    slots = []
    for _ in range(ch):
        kind = rng.integers(0, 10)
        prn = P.PRN_NONE if kind == 0 else int(rng.choice(unlisted)) if kind == 1 else int(prns[rng.integers(0, n_prn)])
        slots.append(Slot(prn, int(rng.choice([0, V, V, VN, NEW_ONLY])), int(rng.choice([-7, 100, 200, 200, 300, BIG])), int(rng.integers(0, 1 << 40))))
    bank = {p: (int(rng.choice([100, 200, 300])), int(rng.integers(0, 1 << 40))) for p in range(n_prn) if rng.integers(0, 2)}
    return slots, bank


def launch(n_rx, n_prn=N_PRN, ch=CH, seed=0):
    """the rows in the first receivers where the shape holds them (the canonical list first, further slots empty or on PRNs of the
    list's extension, further bank entries random), seeded random receivers behind them and in every other shape"""
    rng = np.random.default_rng([seed, n_rx, n_prn, ch])
    la = Launch()
    more = [q for q in range(1, 211) if q not in PRNS and q != UNLISTED]
    la.n_rx, la.n_prn, la.ch = n_rx, n_prn, ch
    la.prns = np.array((PRNS + more)[:n_prn] if n_prn >= N_PRN else more[:n_prn], np.uint8)
    la.slot_prns, la.eph, la.bank, la.rows = np.zeros(n_rx * ch, np.int32), np.zeros(n_rx * ch, P.EPH_DTYPE), P.empty_bank(n_rx, n_prn), []
    fits = ch >= CH and n_prn >= N_PRN
    for r in range(n_rx):
        row = ROWS[r] if fits and r < len(ROWS) else None
        if row is not None:
            slots, bank = list(row.slots), dict(row.bank)
            extra = [int(q) for q in la.prns[N_PRN:]]
            for _ in range(ch - CH):
                slots.append(Slot(int(rng.choice(extra)) if extra and rng.integers(0, 2) else P.PRN_NONE, int(rng.choice([0, V, VN])), int(rng.choice([100, 200])), 3))
            for p in range(N_PRN, n_prn):
                if rng.integers(0, 2):
                    bank[p] = (int(rng.choice([100, 200])), 4)
        else:
            slots, bank = _random_receiver(rng, ch, [int(q) for q in la.prns])
        la.rows.append(row)
        for j, s in enumerate(slots):
            la.slot_prns[r * ch + j] = s.prn
            la.eph[r * ch + j] = record(rng, s.flags, s.toe, s.ttr)
        for p, (toe, ttr) in bank.items():
            la.bank[r, p] = record(rng, V, toe, ttr)
    return la


def sync_states(la):
    """the sync states the call reads loop.prn from: random bytes but for that field (nothing else of them may matter)"""
    import weighted_sync_ref as Y
    rng = np.random.default_rng(la.n_rx * 64 + la.ch)
    st = np.frombuffer(rng.bytes(la.n_rx * la.ch * Y.STATE_DTYPE.itemsize), Y.STATE_DTYPE).copy()
    st["loop"]["prn"] = la.slot_prns
    return st


def run(la, want_out=True):
    """the restatement on a launch -> (rep, out, bank after, trace); the launch's own arrays stay as they are"""
    bank, trace = la.bank.copy(), []
    rep, out = P.bank(la.ch, la.prns, la.slot_prns, la.eph, bank, want_out=want_out, trace=trace)
    return rep, out, bank, trace


def outcome(la, r, rep, out, bank_after, trace):
    c = slice(r * la.ch, (r + 1) * la.ch)
    return Outcome(la.eph[c], la.bank[r], bank_after[r], out[c], rep[r], trace[r])


def smoke_case():
    """the smoke run's launch: every row and as many random receivers again, at a shape with a second workgroup, odd slot and list sizes"""
    return launch(2 * len(ROWS) + 1, 7, 5, seed=28)


def write_smoke(path):
    """tests/golden/wpred_smoke.npz: the bank's launch and the restatement's answer; the prediction table (every row, five random
    receivers behind them) with the restatement's records and states"""
    la = smoke_case()
    rep, out, bank, _ = run(la)
    lp = pred_launch(len(PRED_ROWS) + 5)
    cfg = pred_cfg()
    rx, pred, after, _ = pred_run(lp, cfg)
    np.savez_compressed(path, ch=np.int32(la.ch), prns=la.prns, sync=sync_states(la), eph=la.eph, bank_before=la.bank, bank_after=bank, out=out, rep=rep,
                        p_cfg=cfg, p_prns=lp.prns, p_kf=lp.kf, p_bank=lp.bank, p_rx=rx, p_pred=pred,
                        **{"p_" + k + "_before": v for k, v in lp.states.items()}, **{"p_" + k + "_after": v for k, v in after.items()})


# ==== gpsx_wpred: prediction and hot hand-over ================================================================================================
import functools  # noqa: E402
import json  # noqa: E402
import os  # noqa: E402

import weighted_acq_cases as AC  # noqa: E402
import weighted_fix_cases as W  # noqa: E402
import weighted_kf_ref as R  # noqa: E402
import weighted_lock_ref as L  # noqa: E402
import weighted_vel_ref as VR  # noqa: E402

P_CH, P_N_PRN = 6, 10                  # the canonical shape of the prediction table
P_PRNS = [11, 12, 13, 14, 15, 16, 17, 18, 19, 20]      # index p: the sky's satellite p (0 .. 7), the one below the horizon (8), none (9)
OTHER = (101, 102, 103, 104, 105, 106)                   # PRNs the list lacks
EVICT = 1000
EL_MIN = 0.5236                        # 30 degrees: the sky's satellites stand at 28.0 .. 79.7, two of them under it
TABLE_CFG = dict(el_min_rad=EL_MIN, max_sigma_m=30.0, max_sigma_hz=2.0, lead_blocks=7, evict_after_blocks=EVICT)
WEEK = 2290
PRow = namedtuple("PRow", "name build check")      # build() -> receiver dict; check(outcome dict) -> bool


def pred_cfg(ch=P_CH, handover=1, **kw):
    return P.pred_cfg(ch, VR.L1CA_WLOOP, handover=handover, **dict(TABLE_CFG, **kw))


def kf_state(rr, rcv_ms, b=12.0, vel=(3.0, -2.0, 1.0), d=150.0, sig=(5.0, 10.0, 0.1, 0.2), week=WEEK):
    """an initialised filter state: position rr, clock term b, velocity, drift (150 m/s, an oscillator 0.5 ppm off: it moves every
    satellite's frequency by -788 Hz, away from 0, where the floats a hand-over casts to lie too close for any clearance); P = diag(sig_pos^2 x 3, sig_clk^2, sig_vel^2 x 3,
    sig_drift^2) with a little correlation between each position axis and its velocity"""
    st = np.zeros(1, R.STATE_DTYPE)
    st["x"][0] = [rr[0], rr[1], rr[2], b, vel[0], vel[1], vel[2], d]
    for i in range(8):
        st["P"][0, R.tri(i, i)] = (sig[0], sig[0], sig[0], sig[1], sig[2], sig[2], sig[2], sig[3])[i] ** 2
    for i in range(4):
        st["P"][0, R.tri(i, 4 + i)] = 0.1 * (sig[0] if i < 3 else sig[1]) * (sig[2] if i < 3 else sig[3])
    st["rcv_ms"], st["week"], st["flags"] = rcv_ms, week, R.S_INIT
    return st[0]


@functools.lru_cache(maxsize=None)
def _munich_bank():
    bank = np.zeros(P_N_PRN, P.EPH_DTYPE)
    for p, (raw, _) in enumerate(W.sky("munich", 8, 0)):
        bank[p] = W.eph_record(raw)[0]
    bank[8] = W._below_horizon("munich")[1][0]
    return bank


def munich(slots=(), lock=None, **state_kw):
    """the base receiver: Munich, the sky's eight satellites at indices 0 .. 7, one below the horizon at 8, nothing at 9; slots:
    {slot: PRN}; lock: {slot: (flags, blocks_seen)}"""
    return dict(state=kf_state(W.site_ecef("munich"), int(W.TOW * 1000), **state_kw), bank=_munich_bank().copy(), slots=dict(slots), lock=dict(lock or {}))


def _with(rec, **changes):
    for k, v in changes.items():
        if k == "state_x":
            rec["state"]["x"][v[0]] = v[1]
        elif k == "state_P":
            rec["state"]["P"][R.tri(v[0], v[0])] = v[1]
        elif k == "state_flags":
            rec["state"]["flags"] = v
        elif k == "bank":
            for p, fields in v.items():
                if fields is None:
                    rec["bank"][p] = np.zeros(1, P.EPH_DTYPE)[0]
                elif isinstance(fields, int):
                    rec["bank"][p] = rec["bank"][fields]
                else:
                    for f, val in fields.items():
                        rec["bank"][p][f] = val
        elif k == "rcv_ms":
            rec["state"]["rcv_ms"] = v
    return rec


def _toes(p=0):
    return float(_munich_bank()[p]["toes"])


@functools.lru_cache(maxsize=None)
def _week_end():
    import weighted_edge_cases as X
    r = X.receiver("t_week_end")
    bank = np.zeros(P_N_PRN, P.EPH_DTYPE)
    bank[:8] = r["eph"][:8]
    return X.site_ecef(r["site"]), bank


def week_end():
    rr, bank = _week_end()
    return dict(state=kf_state(rr, R.WEEK_MS - 3), bank=bank.copy(), slots={}, lock={})


def _phase_on_the_seam():
    """Munich with the clock term chosen so that satellite 3's code phase is 2e-4 samples under 16368: its float cast is 16368.0f.  The row
    re-seeds itself (reseed() would move the clock): the drift in steps until the receiver stands clear, the clock solved again each time"""
    cfg = pred_cfg(1, evict_after_blocks=0, handover=0)
    sync = AC.empty_states(1)["sync"]
    for k in range(RESEED_TRIES if PARITY_MEASURED_M is not None else 1):
        rec, target = munich(d=150.0 + 0.0137 * k), None
        for _ in range(4):
            tr = []
            _, pred = P.predict(cfg, P_PRNS, np.array([rec["state"]]), rec["bank"][None], sync, trace=tr)
            u = float(tr[0]["u"][3])
            target = np.floor(u) + 1.0 - 1.2e-8 if target is None else target
            rec["state"]["x"][3] += (target - u) * P.MS
        tr = []
        _, pred = P.predict(cfg, P_PRNS, np.array([rec["state"]]), rec["bank"][None], sync, trace=tr)
        if _receiver_clear(tr[0], rec["bank"], pred[0], cfg[0], PARITY_BOUND_M, PARITY_BOUND_MPS):
            break
    return rec


FLAGS = lambda o, p: int(o["pred"][p]["flags"])      # noqa: E731
ALL4 = P.P_HAVE_EPH | P.P_PREDICTED | P.P_VISIBLE | P.P_CERTAIN
UNDER = (1, 2)                         # the sky's satellites between the horizon and EL_MIN
ABOVE = (0, 3, 4, 5, 6, 7)             # ... and above it, by index; by elevation: 3, 7, 6, 0, 4, 5


def _untouched(o):
    return all(o["after"][k].tobytes() == o["before"][k].tobytes() for k in o["after"])


PRED_ROWS = [
    PRow("NOT_INIT", lambda: _with(munich({0: OTHER[0]}), state_flags=0),
         lambda o: int(o["rx"]["flags"]) == P.RX_NOT_INIT and not o["pred"].tobytes().strip(b"\0") and _untouched(o)
         and o["rx"].tobytes()[2:] == bytes(62)),
    PRow("BAD: an x that is not finite", lambda: _with(munich(), state_x=(2, np.nan)),
         lambda o: int(o["rx"]["flags"]) == P.RX_BAD and not o["pred"].tobytes().strip(b"\0") and _untouched(o)),
    PRow("BAD: a P_ii <= 0", lambda: _with(munich(), state_P=(5, 0.0)),
         lambda o: int(o["rx"]["flags"]) == P.RX_BAD and not o["pred"].tobytes().strip(b"\0") and _untouched(o)),
    PRow("an empty bank", lambda: _with(munich({1: OTHER[1]}), bank={p: None for p in range(P_N_PRN)}),
         lambda o: int(o["rx"]["flags"]) == P.RX_PREDICTED and int(o["rx"]["n_have"]) == 0 and not o["pred"]["flags"].any() and (o["pred"]["slot"] == -1).all()
         and _untouched(o) and int(o["rx"]["t_ms"]) == int(W.TOW * 1000) + 7),
    PRow("svh != 0", lambda: _with(munich(), bank={3: dict(svh=1)}),
         lambda o: FLAGS(o, 3) == P.P_HAVE_EPH and float(o["pred"][3]["pr_m"]) == 0.0 and FLAGS(o, 7) & P.P_ASSIGNED and int(o["pred"][7]["slot"]) == 0),
    PRow("|tk| > 7201", lambda: _with(munich(), rcv_ms=int(round((_toes() + 7201.6) * 1000))),
         lambda o: all(FLAGS(o, p) == P.P_HAVE_EPH for p in range(8)) and all(abs(float(t)) > 7201.3 for t in o["trace"]["passes"][0]["tk"][:8])),
    PRow("|tk| just inside 7201", lambda: _with(munich(), rcv_ms=int(round((_toes() + 7200.6) * 1000))),
         lambda o: all(FLAGS(o, p) & P.P_PREDICTED for p in range(8)) and all(7200.3 < abs(float(t)) < 7200.8 for t in o["trace"]["passes"][2]["tk"][:8])),
    PRow("a satellite below the horizon", lambda: munich(),
         lambda o: FLAGS(o, 8) == P.P_HAVE_EPH | P.P_PREDICTED | P.P_CERTAIN and float(o["pred"][8]["el"]) < -0.2
         and float(o["trace"]["passes"][2]["dion"][8]) == 0.0 and float(o["trace"]["passes"][2]["dtrp"][8]) == 0.0 and float(o["pred"][8]["pr_m"]) > 2.5e7),
    PRow("above the horizon but under el_min_rad", lambda: munich(),
         lambda o: all(FLAGS(o, p) == P.P_HAVE_EPH | P.P_PREDICTED | P.P_CERTAIN and 0.3 < float(o["pred"][p]["el"]) < EL_MIN for p in UNDER)
         and int(o["rx"]["visible_mask"]) == sum(1 << p for p in ABOVE)),
    PRow("s_pr over its limit", lambda: munich(sig=(40.0, 10.0, 0.1, 0.2)),
         lambda o: all(FLAGS(o, p) == P.P_HAVE_EPH | P.P_PREDICTED | P.P_VISIBLE for p in ABOVE) and float(o["pred"][0]["sigma_m"]) > 35.0
         and float(o["pred"][0]["sigma_hz"]) < 1.5 and int(o["rx"]["n_assigned"]) == 0 and _untouched(o)),
    PRow("s_f over its limit", lambda: munich(sig=(5.0, 10.0, 0.6, 0.2)),
         lambda o: all(FLAGS(o, p) == P.P_HAVE_EPH | P.P_PREDICTED | P.P_VISIBLE for p in ABOVE) and float(o["pred"][0]["sigma_hz"]) > 2.5
         and float(o["pred"][0]["sigma_m"]) < 15.0 and int(o["rx"]["n_assigned"]) == 0),
    PRow("both under their limits: six satellites to six free slots, by elevation", lambda: munich(),
         lambda o: all(FLAGS(o, p) == ALL4 | P.P_ASSIGNED for p in ABOVE) and [int(o["pred"][p]["slot"]) for p in (3, 7, 6, 0, 4, 5)] == [0, 1, 2, 3, 4, 5]
         and float(o["pred"][0]["sigma_m"]) < 15.0 and float(o["pred"][0]["sigma_hz"]) < 1.5 and int(o["rx"]["free_mask"]) == 0),
    PRow("every PRN TRACKED", lambda: munich({j: P_PRNS[p] for j, p in enumerate(ABOVE)}),
         lambda o: all(FLAGS(o, p) == ALL4 | P.P_TRACKED for p in ABOVE) and int(o["rx"]["n_tracked"]) == 6 and int(o["rx"]["n_assigned"]) == 0
         and int(o["rx"]["kept_mask"]) == 63 and _untouched(o)),
    PRow("a full receiver", lambda: munich({j: OTHER[j] for j in (0, 1, 2, 4, 5)}),
         lambda o: FLAGS(o, 3) == ALL4 | P.P_ASSIGNED and int(o["pred"][3]["slot"]) == 3 and all(FLAGS(o, p) == ALL4 | P.P_DROPPED for p in (0, 4, 5, 6, 7))
         and int(o["rx"]["flags"]) == P.RX_PREDICTED | P.RX_ASSIGNED | P.RX_FULL and int(o["rx"]["n_dropped"]) == 5),
    PRow("the three eviction boundaries", lambda: munich({0: OTHER[0], 1: OTHER[1], 2: OTHER[2], 3: OTHER[3], 4: OTHER[4], 5: OTHER[5]},
                                                         {0: (L.F_CODE, EVICT + 5), 1: (0, EVICT - 1), 2: (0, EVICT), 3: (L.F_CARRIER, EVICT + 1), 4: (L.F_CODE, 0),
                                                          5: (0, 0)}),
         lambda o: int(o["rx"]["evicted_mask"]) == 0b001100 and int(o["rx"]["kept_mask"]) == 0b110011 and int(o["pred"][3]["slot"]) == 2
         and int(o["pred"][7]["slot"]) == 3 and int(o["rx"]["n_dropped"]) == 4),
    PRow("an evicted slot left empty and one reused", lambda: _with(munich({0: OTHER[0], 1: P_PRNS[7], 2: OTHER[2], 3: P_PRNS[0], 4: P_PRNS[4], 5: P_PRNS[5]},
                                                                        {0: (0, EVICT), 2: (0, EVICT + 7), 1: (L.F_CODE, 5000)}), bank={6: None}),
         lambda o: int(o["rx"]["evicted_mask"]) == 0b000101 and int(o["pred"][3]["slot"]) == 0 and int(o["rx"]["assigned_mask"]) == 1
         and int(o["after"]["sync"]["loop"]["prn"][2]) == P.PRN_NONE and int(o["after"]["sync"]["loop"]["prn"][0]) == P_PRNS[3]
         and int(o["rx"]["free_mask"]) == 0b000100 and not o["after"]["lock"][2].tobytes().strip(b"\0")),
    PRow("two candidates with bit-equal elevation: the index decides", lambda: _with(munich({j: OTHER[j] for j in (1, 2, 3, 4, 5)}), bank={9: 3}),
         lambda o: float(o["pred"][9]["el"]) == float(o["pred"][3]["el"]) and FLAGS(o, 3) == ALL4 | P.P_ASSIGNED and FLAGS(o, 9) == ALL4 | P.P_DROPPED
         and o["pred"][9].tobytes()[8:] == o["pred"][3].tobytes()[8:]),
    PRow("T crosses the week's end through lead_blocks, tx_ms folds below 0", week_end,
         lambda o: int(o["rx"]["t_ms"]) == 4 and int(o["rx"]["week"]) == WEEK + 1 and int(o["rx"]["n_visible"]) >= 4
         and all(R.WEEK_MS - 120 < int(w["tx_ms"]) < R.WEEK_MS - 50 for w in o["pred"] if int(w["flags"]) & P.P_PREDICTED)),
    PRow("a code_phase whose float cast is 16368.0f", _phase_on_the_seam,
         lambda o: float(o["pred"][3]["code_phase"]) < 16368.0 and np.float32(o["pred"][3]["code_phase"]) == np.float32(16368.0)
         and float(o["after"]["sync"]["loop"]["code_phase_fine"][0]) == 16368.0 and int(o["pred"][3]["slot"]) == 0),
]
assert len({r.name for r in PRED_ROWS}) == len(PRED_ROWS)
SEAM_ROW = "a code_phase whose float cast is 16368.0f"


def _random_pred_receiver(rng, ch, n_prn):
    """a Munich receiver of any shape: the sky's satellites at random indices of the list, slots on listed, unlisted and no PRNs, lock states
    around the eviction rule; every third one moved off Munich by kilometres, some not initialised"""
    rr = W.site_ecef("munich") + rng.normal(0.0, 3000.0, 3) * (rng.integers(0, 3) == 0)
    st = kf_state(rr, int(W.TOW * 1000) + int(rng.integers(0, 5000)), b=float(rng.normal(0, 1e4)), vel=tuple(rng.normal(0, 10.0, 3)), d=float(rng.normal(150.0, 2.0)),
                  sig=(float(rng.choice([3.0, 8.0, 40.0])), 10.0, float(rng.choice([0.05, 0.1, 0.6])), 0.2))
    if rng.integers(0, 12) == 0:
        st["flags"] = 0
    bank = np.zeros(n_prn, P.EPH_DTYPE)
    src = _munich_bank()
    for p in range(n_prn):
        if rng.integers(0, 3):
            bank[p] = src[int(rng.integers(0, 9))]
    return st, bank


def pred_launch(n_rx, n_prn=P_N_PRN, ch=P_CH, seed=0, skip=(), clear=True):
    """the prediction rows in the first receivers where the shape holds them, seeded random receivers elsewhere -> Launch with prns,
    kf [n_rx], bank [n_rx][n_prn], states {sync, lock, nav, obs, eph: [n_rx * ch]} (random bytes but for the fields the stage reads),
    rows; skip: row names left out (their place is taken by a random receiver)"""
    rng = np.random.default_rng([28, seed, n_rx, n_prn, ch])
    la = Launch()
    la.n_rx, la.n_prn, la.ch = n_rx, n_prn, ch
    extra = [q for q in range(21, 100)]
    la.prns = np.array((P_PRNS + extra)[:n_prn] if n_prn >= P_N_PRN else extra[:n_prn], np.uint8)
    la.kf, la.bank, la.rows = np.zeros(n_rx, R.STATE_DTYPE), P.empty_bank(n_rx, n_prn), []
    la.states = {k: np.frombuffer(rng.bytes(n_rx * ch * d.itemsize), d).copy() for k, d in P.Q.STATE_DTYPES.items()}
    la.states["sync"]["loop"]["prn"] = P.PRN_NONE
    la.states["lock"]["flags"], la.states["lock"]["blocks_seen"] = L.F_CODE, 0
    fits = ch >= P_CH and n_prn >= P_N_PRN
    for r in range(n_rx):
        row = PRED_ROWS[r] if fits and r < len(PRED_ROWS) and PRED_ROWS[r].name not in skip else None
        la.rows.append(row)
        c0 = r * ch
        if row is not None:
            rec = row.build()
            la.kf[r], la.bank[r, :P_N_PRN] = rec["state"], rec["bank"]
            for j, prn in rec["slots"].items():
                la.states["sync"]["loop"]["prn"][c0 + j] = prn
            for j, (fl, seen) in rec["lock"].items():
                la.states["lock"]["flags"][c0 + j], la.states["lock"]["blocks_seen"][c0 + j] = fl, seen
        else:
            la.kf[r], la.bank[r] = _random_pred_receiver(rng, ch, n_prn)
            for j in range(ch):
                kind = int(rng.integers(0, 4))
                la.states["sync"]["loop"]["prn"][c0 + j] = P.PRN_NONE if kind == 0 else int(rng.choice(OTHER)) if kind == 1 else int(la.prns[rng.integers(0, n_prn)])
                la.states["lock"]["flags"][c0 + j] = int(rng.choice([0, L.F_CODE, L.F_CARRIER]))
                la.states["lock"]["blocks_seen"][c0 + j] = int(rng.choice([0, EVICT - 1, EVICT, EVICT + 1, 1 << 40]))
    # (while the parity bound is the cap nothing that is handed over can stand clear of it: re-seeding starts with the measurement)
    la.reseeded = [reseed(la.kf[r], la.bank[r], la.prns) if clear and PARITY_MEASURED_M is not None and not (la.rows[r] is not None and la.rows[r].name == SEAM_ROW)
                   else 0 for r in range(n_rx)]
    return la


def pred_run(la, cfg, nulls=(), want_pred=True):
    """the restatement on a launch -> (rx, pred, {name: states after}, trace); the launch's own arrays stay as they are"""
    st = {k: None if k in nulls else v.copy() for k, v in la.states.items()}
    trace = []
    rx, pred = P.predict(cfg, la.prns, la.kf, la.bank, st["sync"], st["lock"], st["nav"], st["obs"], st["eph"], want_pred=want_pred, trace=trace)
    return rx, pred, st, trace


def pred_outcome(la, r, rx, pred, after, trace):
    c = slice(r * la.ch, (r + 1) * la.ch)
    return dict(rx=rx[r], pred=pred[r], after={k: v[c] for k, v in after.items() if v is not None}, before={k: v[c] for k, v in la.states.items() if after[k] is not None},
                trace=trace[r])


# ---- closure: the prediction fed back to the filter's and the velocity solver's rows ------------------------------------------------------
def closure(la, cfg, rx, pred, trace):
    """for every PREDICTED (receiver, PRN): an observable made of the record's tx_ms and its double code_phase, at gpsx_wkf's row at the same
    x^ (weighted_kf_ref.rows with rcv_ms = T, evaluated in doubles: the phase is not cast to float) -> the largest |v| (m), and with the
    record's f_hz the largest |y - a . x^_v| (m/s); both are zero but for the fourth pass that was not made and round-off"""
    c = np.asarray(cfg, P.PRED_CFG_DTYPE).reshape(1)[0]
    kcfg = R.make_cfg(1, mps_per_hz=float(c["mps_per_hz"]), sig_pr_m=0.0)[0]
    ion = np.array(c["ion"], np.float64)
    ion = P.F.ION_DEFAULT if float((ion * ion).sum()) <= 0.0 else ion
    worst_v, worst_y, n = 0.0, 0.0, 0
    for r in range(la.n_rx):
        if trace[r]["kind"] != "run":
            continue
        for p in np.flatnonzero((pred[r]["flags"] & P.P_PREDICTED) != 0):
            w = pred[r, p]
            obs = np.zeros((1, 1), np.dtype([("tx_ms", "<i8"), ("code_phase_fine", "<f8"), ("if_freq_offset_hz", "<f8")]))
            obs["tx_ms"], obs["code_phase_fine"], obs["if_freq_offset_hz"] = w["tx_ms"], w["code_phase"], w["f_hz"]
            with np.errstate(all="ignore"):
                d = R.rows(trace[r]["xh"][None, :], np.array([trace[r]["T"]], np.int64), obs, la.bank[r, p:p + 1][None, :], np.zeros((1, 1), np.int64),
                           np.ones((1, 1), bool), np.ones((1, 1), bool), kcfg, ion)
            v = float(d["v"][0, 0])
            if float(d["el"][0, 0]) < 0.0:      # (below the horizon the filter forms no row; its v is still the model's)
                assert not d["prow"][0, 0]
            worst_v, worst_y, n = max(worst_v, abs(v)), max(worst_y, abs(float(d["y"][0, 0]))), n + 1
    return worst_v, worst_y, n


# ---- clearance: what makes a byte-for-byte comparison with the device fair ----------------------------------------------------------------
PARITY_ENV = "GPSX_WPRED_PARITY_JSON"      # a path: every labelled compare() records its maxima there (how the profile is written)
PARITY_CAP_M, PARITY_CAP_MPS = 1e-4, 1e-6
# profiles/r28_weighted_pred_parity.json, one MI355X: "largest_m": 8.528943176773665e-09, "largest_mps": 1.1238623970771973e-12
PARITY_MEASURED_M = 8.5290e-9      # largest |device - restatement| of pr_m and code_phase x 18.3 m over every compared launch; None: not measured, the cap holds
PARITY_MEASURED_MPS = 1.1239e-12   # ... of f_hz x |mps_per_hz|
PARITY_BOUND_M = PARITY_CAP_M if PARITY_MEASURED_M is None else min(8.0 * PARITY_MEASURED_M, PARITY_CAP_M)
PARITY_BOUND_MPS = PARITY_CAP_MPS if PARITY_MEASURED_MPS is None else min(8.0 * PARITY_MEASURED_MPS, PARITY_CAP_MPS)
M_PER_SAMPLE = P.MS / 16368.0          # 18.3 m
CLEAR = 1e3


def _float_margin(v):
    """the distance of the double v from the nearest boundary between two floats' rounding intervals"""
    f = np.float32(v)
    lo, hi = np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))
    return min(abs(float(v) - (float(f) + float(lo)) / 2.0), abs(float(v) - (float(f) + float(hi)) / 2.0))


def _receiver_clear(t, bank_row, pred_row, c, bound_m, bound_mps):
    """one receiver's trace against the thresholds (see decisions_clear)"""
    mps = abs(float(c["mps_per_hz"]))
    ang = CLEAR * bound_m / 2.0e7
    ok = True
    for p in range(len(bank_row)):
        if not (int(bank_row[p]["flags"]) & P.F_VALID and int(bank_row[p]["svh"]) == 0):
            continue
        ok &= abs(abs(float(t["passes"][0]["tk"][p])) - 7201.0) > 1e-3
        if not t["predicted"][p]:
            continue
        el, u = float(t["el"][p]), float(t["u"][p])
        ok &= abs(el) > ang and abs(el - float(c["el_min_rad"])) > ang
        ok &= abs(float(t["s_pr"][p]) / float(c["max_sigma_m"]) ** 2 - 1.0) > CLEAR * 1e-5 and abs(float(t["s_f"][p]) / float(c["max_sigma_hz"]) ** 2 - 1.0) > CLEAR * 1e-5
        ok &= min(u - np.floor(u), np.floor(u) + 1.0 - u) * P.MS > CLEAR * bound_m
        if t["visible"][p] and t["certain"][p]:      # (whatever the slots are: it may be handed over)
            ok &= _float_margin(pred_row[p]["code_phase"]) * M_PER_SAMPLE > CLEAR * bound_m and _float_margin(pred_row[p]["f_hz"]) * mps > CLEAR * bound_mps
    able = [p for p in range(len(bank_row)) if t["visible"][p] and t["certain"][p]]
    for a in range(len(able)):
        for b in range(a + 1, len(able)):
            same = bank_row[able[a]].tobytes() == bank_row[able[b]].tobytes()
            ok &= same or abs(float(t["el"][able[a]]) - float(t["el"][able[b]])) > ang
    return bool(ok)


def decisions_clear(la, cfg, pred, trace, bound_m=None, bound_mps=None):
    """every decision of a launch that the device takes on doubles stands at least CLEAR x the parity bound from its threshold in the
    restatement: el against 0 and el_min_rad (the angle's bound: the position bound over the range), the two variances against
    their limits (relative: the float sigmas' 1e-5), the elevations of any two satellites of one receiver that could be candidates
    against each other unless their records are the same bytes, u against floor(u) and floor(u) + 1, tk against 7201 (1e-3 s), and
    the two floats of every satellite that could be handed over against the boundaries of their rounding intervals
    -> the receivers that are NOT clear (a row's name, or the receiver's number)"""
    bound_m = PARITY_BOUND_M if bound_m is None else bound_m
    bound_mps = PARITY_BOUND_MPS if bound_mps is None else bound_mps
    c = np.asarray(cfg, P.PRED_CFG_DTYPE).reshape(1)[0]
    return [la.rows[r].name if la.rows[r] is not None else r for r in range(la.n_rx)
            if trace[r]["kind"] == "run" and not _receiver_clear(trace[r], la.bank[r], pred[r], c, bound_m, bound_mps)]


RESEED_TRIES = 400


def reseed(state, bank_row, prns):
    """a receiver that does not stand clear is re-seeded, not tolerated: its clock term moves in steps of 0.731 m (0.04 samples of code
    phase for every satellite) and its drift in steps of 0.0137 m/s (0.07 Hz), neither of which a row's predicate can see, until it
    does -> the number of steps"""
    cfg = pred_cfg(1, handover=0, evict_after_blocks=0)
    c = cfg[0]
    if not int(state["flags"]) & R.S_INIT or not np.isfinite(state["x"]).all():
        return 0
    sync = AC.empty_states(1)["sync"]
    b0, d0 = float(state["x"][3]), float(state["x"][7])
    for k in range(RESEED_TRIES):
        state["x"][3], state["x"][7] = b0 + 0.731 * k, d0 + 0.0137 * k
        tr = []
        _, pred = P.predict(cfg, prns, np.array([state]), bank_row[None], sync, trace=tr)
        if tr[0]["kind"] != "run" or _receiver_clear(tr[0], bank_row, pred[0], c, PARITY_BOUND_M, PARITY_BOUND_MPS):
            return k
    return RESEED_TRIES


# ---- the device against the restatement ---------------------------------------------------------------------------------------------------
PRED_INT_FIELDS = ("flags", "slot", "tx_ms")


def _record_parity(label, worst, n):
    path = os.environ.get(PARITY_ENV)
    if not path or label is None:
        return
    doc = json.load(open(path)) if os.path.exists(path) else {"launches": {}}
    doc["launches"][str(label)] = dict(worst, predicted=n)
    doc["what"] = ("largest |device - restatement| in pr_m and code_phase x 18.3 m (m), f_hz x |mps_per_hz| (m/s), el and az (rad) and the float "
                   "sigmas (relative) per compared launch of tests/test_gpu_weighted_pred.py, one MI355X; written by weighted_pred_cases.compare "
                   "under $" + PARITY_ENV)
    doc["largest_m"] = max(max(w["pr_m"], w["code_phase_m"]) for w in doc["launches"].values())
    doc["largest_mps"] = max(w["f_mps"] for w in doc["launches"].values())
    doc["cap_m"], doc["bound_m"] = PARITY_CAP_M, min(8.0 * doc["largest_m"], PARITY_CAP_M)
    doc["cap_mps"], doc["bound_mps"] = PARITY_CAP_MPS, min(8.0 * doc["largest_mps"], PARITY_CAP_MPS)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)


def compare(got_rx, got_pred, want_rx, want_pred, mps_per_hz, label=None, bound_m=None, bound_mps=None):
    """a launch's records against the restatement's: the receiver records byte for byte (they hold integers only); per (receiver, PRN)
    flags, slot and tx_ms equal, pr_m and code_phase x 18.3 m within the position bound, f_hz x |mps_per_hz| within the velocity bound,
    el and az within the position bound over the range (2e7 m), the float sigmas 1e-5 relative; nothing non-finite
    -> the per-field maxima (measured, and with a label recorded under $GPSX_WPRED_PARITY_JSON, before anything is asserted)"""
    bound_m = PARITY_BOUND_M if bound_m is None else bound_m
    bound_mps = PARITY_BOUND_MPS if bound_mps is None else bound_mps
    for f in ("pr_m", "code_phase", "f_hz", "el", "az", "sigma_m", "sigma_hz"):
        assert np.isfinite(got_pred[f]).all(), f
    on = (want_pred["flags"] & P.P_PREDICTED) != 0
    g, w = got_pred[on], want_pred[on]
    mx = lambda a: float(np.abs(a).max()) if a.size else 0.0      # noqa: E731
    daz = np.abs(g["az"] - w["az"])
    worst = {"pr_m": mx(g["pr_m"] - w["pr_m"]), "code_phase_m": mx(g["code_phase"] - w["code_phase"]) * M_PER_SAMPLE,
             "f_mps": mx(g["f_hz"] - w["f_hz"]) * abs(float(mps_per_hz)), "el_rad": mx(g["el"] - w["el"]), "az_rad": mx(np.minimum(daz, 2 * P.PI - daz)),
             "sigma_rel": max(mx((g[f].astype(np.float64) - w[f]) / np.maximum(np.abs(w[f]), 1e-30)) for f in ("sigma_m", "sigma_hz"))}
    _record_parity(label, worst, int(on.sum()))
    assert got_rx.tobytes() == want_rx.tobytes(), (label, [r for r in range(len(got_rx)) if got_rx[r].tobytes() != want_rx[r].tobytes()][:4], got_rx[:2], want_rx[:2])
    for f in PRED_INT_FIELDS:
        bad = np.argwhere(got_pred[f] != want_pred[f])
        assert bad.size == 0, (label, f, bad[:8])
    assert got_pred[~on].tobytes() == want_pred[~on].tobytes(), "records without a prediction"
    assert max(worst["pr_m"], worst["code_phase_m"]) <= bound_m and max(worst["el_rad"], worst["az_rad"]) <= bound_m / 2.0e7 * 50.0, (label, worst)
    assert worst["f_mps"] <= bound_mps and worst["sigma_rel"] <= 1e-5, (label, worst)
    return worst


# ---- physics: the stream of weighted_pvt_cases, the restatements all the way ----------------------------------------------------------------
# MEASURED, each on the CPU (tests/test_weighted_pred_reference.py prints them; a GPU-side repeat is bounded at 1.5 x these):
#   pred_phase_samples, pred_freq_hz: the largest error, over the stream's four satellites and the two instants (blocks 24 576 and 25 000), of the
#     predicted transmit time at sample 0 (in samples) and of f_hz against the synthesiser's own truth (weighted_pvt_cases.lag_s, doppler_at
#     x 1023 / 1022: the loops' unit).
#   repull_phase_samples, repull_freq_hz: slot 2 handed PRN 4 by gpsx_wpred at block 24 576 and tracked for the last 424 blocks: the difference of its
#     final code_phase_fine and if_freq_offset_hz from the undisturbed channel's.
MEASURED = {"pred_phase_samples": 2.08781, "pred_freq_hz": 0.336946, "repull_phase_samples": 0.0625, "repull_freq_hz": 0.564942}
STREAM_PRNS = [31, 4, 1, 2, 5, 3, 210]      # the list of the stream's tests: its four PRNs (1, 3, 4, 5) among others


def stream_filter_cfgs():
    """weighted_kf_cases.if_cfgs() with initial standard deviations that say what gpsx_wvel's record is worth on this stream (0.07 m/s,
    weighted_kf_cases.MEASURED): 0.5 m/s and 1 m/s of drift instead of the defaults' 10 and 500, which are a prior for a filter started
    from nothing.  CERTAIN reads P: a prior of 500 m/s of drift is 2630 Hz of not knowing, and nothing would be handed over at INIT"""
    import weighted_kf_cases as K
    fcfg, vcfg, _ = K.if_cfgs()
    return fcfg, vcfg, R.make_cfg(4, mps_per_hz=VR.L1CA_WLOOP, p0=(30.0, 30.0, 0.5, 1.0))


def stream_on_restatements():
    """weighted_pvt_cases' stream through the cached restatement chain (MOVING gains) with the bank and the filter behind every launch
    -> dict(flags: the filter's per launch, at: {block: (filter state, bank [1][n_prn])} for blocks 24 576 and 25 000, chain, end: the
    chain's states at the end, reps: the bank's reports per launch)"""
    import weighted_kf_cases as K
    import weighted_pvt_cases as S
    chain, end = S.chain_on_restatements("moving")
    fcfg, vcfg, kcfg = stream_filter_cfgs()
    state, prev, bank = np.zeros(1, R.STATE_DTYPE), None, P.empty_bank(1, len(STREAM_PRNS))
    flags, at, reps = [], {}, []
    slot_prns = np.array(S.PRNS, np.int32)
    for first, n, _, _, obs, eph in chain:
        rep, merged = P.bank(4, STREAM_PRNS, slot_prns, eph, bank)
        fix = P.F.run(fcfg, obs, merged, 1, prev=prev)[0]
        prev = fix
        vel = VR.run(vcfg, obs, merged, fix, 1)
        rec, state, rc = R.run(kcfg, obs, merged, state, 1, n, None, fix, vel)
        assert rc == 0
        flags.append(int(rec["flags"][0]))
        reps.append(rep)
        at[first + n] = (state.copy(), bank.copy())
    return dict(flags=flags, at=at, chain=chain, end=end, reps=reps)


def stream_cfg(handover=0):
    return P.pred_cfg(4, VR.L1CA_WLOOP, el_min_rad=0.0873, max_sigma_m=300.0, max_sigma_hz=12.5, lead_blocks=0, evict_after_blocks=0, handover=handover)


def prediction_errors(pred, t_ms):
    """a receiver's records on STREAM_PRNS against the synthesiser's truth at the block that starts at t_ms -> (the four satellites' errors of the
    transmit time at sample 0 in samples, of f_hz in Hz)"""
    import weighted_pvt_cases as S
    block = int(t_ms) - int(round(S.TOW0 * 1000.0))
    d_phase, d_freq = [], []
    for (_, row), prn in zip(S.sats(), S.PRNS):
        w = pred[STREAM_PRNS.index(prn)]
        assert int(w["flags"]) & P.P_PREDICTED, prn
        d_phase.append(((float(int(w["tx_ms"])) - float(w["code_phase"]) / 16368.0) - S.truth_tx_ms(row, block)) * 16368.0)
        d_freq.append(float(w["f_hz"]) - S.doppler_at(row, block) * 1023.0 / 1022.0)
    return np.array(d_phase), np.array(d_freq), block
