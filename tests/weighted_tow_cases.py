"""The fabricated receivers of the tests of the time-of-week aiding (include/gpsx.h gpsx_wtow; restated in tests/weighted_tow_ref.py): one
row per clause of the definition, each with a predicate on the outcome's own numbers, and launches of any shape that hold the rows
where they fit and seeded random receivers elsewhere.  The observable states, the sync states, the observables and gpsx_wpred's records
are written as bytes -- no prediction is computed: the stage reads four fields of a record and evaluates nothing, so every decision is
exact and the device is compared byte for byte, with no clearance margin.  A predicate reads the launch's resolve and rearm from the
outcome: the table is run under all four pairs.  tests/test_weighted_tow_reference.py asserts the predicates on the restatement,
tests/test_gpu_weighted_tow.py on the device's bytes."""
from collections import namedtuple

import numpy as np

import weighted_obs_ref as O
import weighted_pred_ref as P
import weighted_sync_ref as Y
import weighted_tow_ref as T

CH, N_PRN = 4, 5                       # the canonical shape: what the predicates are proven at
PRNS = [3, 7, 19, 30, 210]
UNLISTED = 5
W = O.WEEK_MS
PE = O.F_PHASE | O.F_EDGE
AMB, TOW, CONF = O.F_AMBIGUOUS, O.F_TOW, O.F_CONFIRMED
BASE = 389_934_920                     # a multiple of 20: the transmit millisecond at the edge of block Z in most rows
MAX_SIGMA, MAX_RESID, MAX_AGE = 30.0, 8.0, 40
BIG = 1 << 62
NAN = float("nan")

Row = namedtuple("Row", "name slots check rx_flags", defaults=(P.RX_PREDICTED,))      # slots: [dict] (slot()); check(outcome) -> bool
Outcome = namedtuple("Outcome", "t rx sb sa yb ya ob oa resolve rearm")                # one receiver's: records, states / sync / obs before and after


def tx_for(b, z, m=0, base=BASE):
    """the tx for which step 3 finds Tz' = base + m at a state with blocks_seen b and edge_block z"""
    return (base + m + b - z) % W


def slot(prn=None, b=25000, z=24613, age=10, phase=5000.0, flags=PE, tz=0, m=0, k=0, cp=None, sigma=5.0, pflags=P.P_PREDICTED | P.P_HAVE_EPH, tx=None, mode=2,
         **state):
    """one slot: a running chain at block b with its edge at block z, its newest window `age` blocks old, and the prediction of its PRN:
    code_phase cp (half a sample from the loop's by default), tx_ms such that the edge of block z falls m ms off the 20 ms grid after a
    millisecond step of k; **state overrides fields of the observable state"""
    st = dict(blocks_seen=b, last_bit_end_p1=b - 3, chain_first_p1=b - 403, edge_block=z, tx_ms_at_edge=tz, last_win_end_p1=b - age, last_phase=phase,
              last_freq=-1234.5, flags=flags, n_wraps=1, n_anchor=2, n_mismatch=3, n_break=4, reserved=0)
    st.update(state)
    return dict(prn=prn, state=st, mode=mode,
                pred=dict(flags=pflags, tx_ms=(tx_for(st["blocks_seen"], st["edge_block"], m) - k) % W if tx is None else tx,
                          code_phase=phase + 0.5 if cp is None else cp, sigma_m=sigma))


E = dict(prn=P.PRN_NONE)               # an empty slot
FL = lambda o, j: int(o.t[j]["flags"])      # noqa: E731
_same = lambda a, b: np.asarray(a).tobytes() == np.asarray(b).tobytes()      # noqa: E731


def untouched(o, j):
    return _same(o.sa[j], o.sb[j]) and _same(o.ya[j], o.yb[j]) and (o.oa is None or _same(o.oa[j], o.ob[j]))


def record(o, j, flags, p=None, tx=0, m=-1, shift=0):
    t = o.t[j]
    return (int(t["flags"]), int(t["tx_ms"]), int(t["m"]), int(t["shift"]), int(t["zero"])) == (flags, tx, m, shift, 0) and (p is None or int(t["prn_index"]) == p)


def aided(o, j, z, tz, extra=0, keeps=PE):
    """slot j was anchored: edge_block z, tx_ms_at_edge tz, TOW set, AMBIGUOUS cleared under resolve, every other byte of the state kept,
    and the observable patched where there is one"""
    a, b = o.sa[j], o.sb[j]
    want = b.copy()
    want["edge_block"], want["tx_ms_at_edge"] = z, tz
    want["flags"] = (int(b["flags"]) | TOW) & (~AMB if o.resolve else ~0)
    ok = _same(a, want) and FL(o, j) == T.T_AIDED | extra and int(a["flags"]) & keeps == keeps and _same(o.ya[j], o.yb[j])
    if o.oa is not None:
        w = o.ob[j].copy()
        w["tx_ms"], w["flags"] = (tz + int(b["blocks_seen"]) - z) % W, int(want["flags"]) | O.F_VALID
        ok = ok and _same(o.oa[j], w)
    return bool(ok) and (int(o.rx["aided_mask"]) >> j) & 1 == 1 and (int(o.rx["valid_after_mask"]) >> j) & 1 == 1


def _grid(o, j, m, amb, mode=2):
    """what step 4 makes of a slot at m with or without AMBIGUOUS (its sync state in `mode`), under the launch's resolve and rearm"""
    z, b = 24613, 25000
    if m in (1, 19) and amb and o.resolve:
        s = -1 if m == 1 else 1
        return aided(o, j, z + s, BASE + m + s, T.T_SHIFTED) and record(o, j, T.T_AIDED | T.T_SHIFTED, j, tx_for(b, z, m), m, s)
    rearmed = T.T_REARMED if o.rearm and mode != 0 else 0
    return record(o, j, T.T_OFF_GRID | rearmed, j, tx_for(b, z, m), m) and _same(o.sa[j], o.sb[j]) and (o.oa is None or _same(o.oa[j], o.ob[j]))


def _rearm(o, j, mode):
    want = o.yb[j].copy()
    if o.rearm and mode != 0:
        want["mode"], want["search_n"], want["prev_best_p1"] = 0, 0, 0
    return _same(o.ya[j], want) and bool(FL(o, j) & T.T_REARMED) == bool(o.rearm and mode != 0) and bool(FL(o, j) & T.T_OFF_GRID) and _same(o.sa[j], o.sb[j])


f32_above = lambda v: float(np.nextafter(np.float32(v), np.float32(np.inf)))      # noqa: E731

ROWS = [
    Row("NO_PRED", [slot(), slot(), E, slot(prn=UNLISTED)],
        lambda o: all(record(o, j, T.T_NO_PRED, 0, 0, 0) and float(o.t[j]["resid"]) == 0.0 and untouched(o, j) for j in range(4))
        and int(o.rx["flags"]) == T.RX_NO_PRED and o.rx.tobytes()[2:] == bytes(62), P.RX_NOT_INIT),
    Row("EMPTY and UNLISTED", [E, slot(prn=UNLISTED), slot(prn=0), slot(prn=-3)],
        lambda o: record(o, 0, T.T_EMPTY, -1) and all(record(o, j, T.T_UNLISTED, -1) for j in (1, 2, 3)) and all(untouched(o, j) for j in range(4))
        and o.rx.tobytes() == bytes(64)),
    Row("BAD: a flag bit gpsx_wobs does not know, reserved != 0", [slot(flags=PE | 32), slot(flags=PE | (1 << 31)), slot(reserved=1), slot()],
        lambda o: all(record(o, j, T.T_BAD, j) and untouched(o, j) for j in range(3)) and aided(o, 3, 24613, BASE) and int(o.rx["valid_after_mask"]) == 8),
    Row("BAD: a count outside 0 .. 2^62", [slot(blocks_seen=-1, last_win_end_p1=0), slot(last_bit_end_p1=BIG + 1), slot(chain_first_p1=-5), slot(last_win_end_p1=BIG + 1)],
        lambda o: all(record(o, j, T.T_BAD, j) and untouched(o, j) for j in range(4)) and int(o.rx["valid_after_mask"]) == 0),
    Row("BAD: edge_block and tx_ms_at_edge", [slot(z=BIG + 1), slot(z=-BIG - 1), slot(tz=W), slot(tz=-1)],
        lambda o: all(record(o, j, T.T_BAD, j) and untouched(o, j) for j in range(4))),
    Row("BAD: last_phase outside [0, 16368) under PHASE; without PHASE it is not looked at", [slot(phase=16368.0), slot(phase=NAN), slot(phase=-0.5), slot(phase=16368.0, flags=O.F_EDGE)],
        lambda o: all(record(o, j, T.T_BAD, j) and untouched(o, j) for j in range(3)) and record(o, 3, T.T_WAITING, 3) and untouched(o, 3)),
    Row("WAITING", [slot(flags=O.F_EDGE | TOW), slot(flags=O.F_PHASE | TOW), slot(flags=0), slot(flags=AMB | CONF)],
        lambda o: all(record(o, j, T.T_WAITING, j) and untouched(o, j) for j in range(4)) and int(o.rx["valid_after_mask"]) == 0),
    Row("STALE, and the age exactly at the limit", [slot(age=MAX_AGE + 1), slot(age=MAX_AGE), slot(age=-7), slot(b=BIG, z=BIG - 387, age=BIG)],
        lambda o: record(o, 0, T.T_STALE, 0) and untouched(o, 0) and aided(o, 1, 24613, BASE) and aided(o, 2, 24613, BASE) and record(o, 3, T.T_STALE, 3)),
    Row("UNCERTAIN", [slot(pflags=P.P_HAVE_EPH), slot(sigma=f32_above(MAX_SIGMA)), slot(sigma=MAX_SIGMA), slot(pflags=0, sigma=1e9)],
        lambda o: all(record(o, j, T.T_UNCERTAIN, j) and untouched(o, j) and float(o.t[j]["resid"]) == 0.0 for j in (0, 1, 3)) and aided(o, 2, 24613, BASE)),
    Row("d either side of +8184 and of -8184: the millisecond turns, the residual changes sign",
        [slot(phase=16000.0, cp=7816.0), slot(phase=16000.0, cp=float(np.nextafter(7816.0, 0.0))), slot(phase=100.0, cp=8284.0), slot(phase=100.0, cp=float(np.nextafter(8284.0, 9000.0)))],
        lambda o: [float(o.t[j]["resid"]) for j in range(4)] == [8184.0, -8184.0, -8184.0, 8184.0] and all(record(o, j, T.T_INCONSISTENT, j) and untouched(o, j) for j in range(4))
        and int(o.rx["n_inconsistent"]) == 4),
    Row("k = -1, 0 and +1", [slot(phase=2.0, cp=16365.0, k=-1), slot(phase=5000.0, cp=4997.25), slot(phase=16366.0, cp=2.5, k=1), E],
        lambda o: [float(o.t[j]["resid"]) for j in range(3)] == [5.0, 2.75, -4.5] and all(aided(o, j, 24613, BASE) for j in range(3))
        and [int(o.t[j]["tx_ms"]) for j in range(3)] == [tx_for(25000, 24613)] * 3 and [int(o.t[j]["m"]) for j in range(3)] == [0, 0, 0]),
    Row("|rho| at the limit, just over it, a NaN and an infinite code_phase",
        [slot(cp=5000.0 - MAX_RESID), slot(cp=float(np.nextafter(5000.0 - MAX_RESID, 0.0))), slot(cp=NAN), slot(cp=float("-inf"))],
        lambda o: aided(o, 0, 24613, BASE) and float(o.t[0]["resid"]) == MAX_RESID and all(record(o, j, T.T_INCONSISTENT, j) and untouched(o, j) for j in (1, 2, 3))
        and o.t[2]["resid"].tobytes() == T.QUIET_NAN.tobytes() and float(o.t[3]["resid"]) == float("inf")),
    Row("tx folds below 0 and at W; a tx_ms outside the week is taken modulo W",
        [slot(phase=2.0, cp=16365.0, tx=0, z=25000 - 399), slot(phase=16366.0, cp=2.5, tx=W - 1, z=25000 - 400), slot(tx=tx_for(25000, 24613) - 3 * W),
         slot(tx=(1 << 63) - 1, z=25000 - ((1 << 63) - 1) % W % 20)],
        lambda o: record(o, 0, T.T_AIDED, 0, W - 1, 0) and int(o.sa[0]["tx_ms_at_edge"]) == W - 400 and record(o, 1, T.T_AIDED, 1, 0, 0)
        and int(o.sa[1]["tx_ms_at_edge"]) == W - 400 and aided(o, 2, 24613, BASE) and record(o, 3, T.T_AIDED, 3, ((1 << 63) - 1) % W, 0)),
    Row("B and Z near 2^62, a negative Z", [slot(b=BIG, z=BIG - 387), slot(b=BIG - 1, z=BIG), slot(b=100, z=-287, chain_first_p1=1), slot(b=50, z=-BIG, chain_first_p1=1)],
        lambda o: aided(o, 0, BIG - 387, BASE) and aided(o, 1, BIG, BASE) and aided(o, 2, -287, BASE) and aided(o, 3, -BIG, BASE)
        and int(o.t[1]["tx_ms"]) == BASE - 1),
    Row("m = 0, with and without AMBIGUOUS", [slot(flags=PE | AMB), slot(), slot(flags=PE | AMB | CONF), E],
        lambda o: aided(o, 0, 24613, BASE) and aided(o, 1, 24613, BASE) and aided(o, 2, 24613, BASE, keeps=PE | CONF)
        and bool(int(o.sa[0]["flags"]) & AMB) == (not o.resolve) and int(o.rx["n_aided"]) == 3 and int(o.rx["n_shifted"]) == 0),
    Row("m = 1 and 19 with AMBIGUOUS: the other nearest block start under resolve", [slot(m=1, flags=PE | AMB), slot(m=19, flags=PE | AMB), slot(m=1, flags=PE | AMB, mode=0), E],
        lambda o: _grid(o, 0, 1, True) and _grid(o, 1, 19, True) and _grid(o, 2, 1, True, 0) and int(o.rx["shifted_mask"]) == (7 if o.resolve else 0)
        and int(o.rx["off_grid_mask"]) == (0 if o.resolve else 7)),
    Row("m = 1 and 19 without AMBIGUOUS: OFF_GRID", [slot(m=1), slot(m=19), slot(m=19, flags=PE | CONF), E],
        lambda o: _grid(o, 0, 1, False) and _grid(o, 1, 19, False) and _grid(o, 2, 19, False) and int(o.rx["n_off_grid"]) == 3),
    Row("m = 2, 10 and 18: OFF_GRID whatever the flags", [slot(m=2, flags=PE | AMB), slot(m=10), slot(m=18, flags=PE | AMB), slot(m=10, flags=PE | TOW, tz=BASE + 10)],
        lambda o: _grid(o, 0, 2, True) and _grid(o, 1, 10, False) and _grid(o, 2, 18, True) and _grid(o, 3, 10, False) and int(o.rx["valid_after_mask"]) == 8),
    Row("rearm with mode 0, 1 and 2", [slot(m=7, mode=0), slot(m=7, mode=1), slot(m=7, mode=2), slot(mode=2)],
        lambda o: _rearm(o, 0, 0) and _rearm(o, 1, 1) and _rearm(o, 2, 2) and aided(o, 3, 24613, BASE)
        and bool(int(o.rx["flags"]) & T.RX_REARMED) == bool(o.rearm) and int(o.rx["flags"]) & T.RX_OFF_GRID),
    Row("TOW set and agreeing", [slot(flags=PE | TOW, tz=BASE), slot(flags=PE | TOW | CONF | AMB, tz=BASE), slot(flags=PE | TOW | AMB, tz=BASE, m=1), E],
        lambda o: record(o, 0, T.T_AGREES, 0, tx_for(25000, 24613), 0) and untouched(o, 0)
        and record(o, 1, T.T_AGREES, 1, tx_for(25000, 24613), 0) and int(o.sa[1]["flags"]) == (PE | TOW | CONF | (0 if o.resolve else AMB))
        and int(o.sa[1]["edge_block"]) == 24613 and int(o.sa[1]["tx_ms_at_edge"]) == BASE
        and (o.oa is None or (_same(o.oa[1], o.ob[1]) if not o.resolve else int(o.oa[1]["flags"]) == PE | TOW | CONF | O.F_VALID and int(o.oa[1]["tx_ms"]) == BASE + 387))
        # agreeing only after the shift: Tz stays, Z moves
        and (record(o, 2, T.T_AGREES | T.T_SHIFTED, 2, tx_for(25000, 24613, 1), 1, -1) and int(o.sa[2]["edge_block"]) == 24612 and int(o.sa[2]["tx_ms_at_edge"]) == BASE
             and int(o.sa[2]["flags"]) == PE | TOW and (o.oa is None or int(o.oa[2]["tx_ms"]) == BASE + 388) if o.resolve else _grid(o, 2, 1, True))
        and int(o.rx["valid_after_mask"]) == 7),
    Row("TOW set and disagreeing: the HOW stands", [slot(flags=PE | TOW, tz=BASE + 20), slot(flags=PE | TOW | AMB, tz=BASE - 20), slot(flags=PE | TOW | AMB, tz=BASE + 1, m=1),
                                                    slot(flags=PE | TOW | CONF, tz=0)],
        lambda o: all(FL(o, j) & ~T.T_SHIFTED == T.T_DISAGREES and untouched(o, j) for j in (0, 1, 3))
        and (FL(o, 2) == T.T_DISAGREES | T.T_SHIFTED and int(o.t[2]["shift"]) == -1 if o.resolve else FL(o, 2) & T.T_OFF_GRID) and _same(o.sa[2], o.sb[2])
        and int(o.rx["disagrees_mask"]) == (15 if o.resolve else 11) and int(o.rx["valid_after_mask"]) == 15),
    Row("CONFIRMED and the counters are kept; four slots on one PRN read one record", [slot(prn=3, flags=PE | CONF), slot(prn=3, flags=PE | CONF | AMB), slot(prn=3),
                                                                                       slot(prn=3, flags=PE | TOW | CONF, tz=BASE)],
        lambda o: aided(o, 0, 24613, BASE, keeps=PE | CONF) and aided(o, 1, 24613, BASE, keeps=PE | CONF) and aided(o, 2, 24613, BASE)
        and [int(o.t[j]["prn_index"]) for j in range(4)] == [0, 0, 0, 0] and FL(o, 3) == T.T_AGREES and untouched(o, 3)
        and all(int(o.sa[j][f]) == int(o.sb[j][f]) for j in range(4) for f in ("n_wraps", "n_anchor", "n_mismatch", "n_break"))),
]
assert len({r.name for r in ROWS}) == len(ROWS)


class Launch:
    """n_rx receivers of ch slots on a list of n_prn PRNs: prns (uint8), pred_rx [n_rx], pred [n_rx][n_prn], sync, states, obs [n_rx * ch],
    rows [the Row a receiver holds, or None]"""


def _fill(la, r, slots):
    """a receiver's slots into the launch's arrays: states, sync fields and the prediction record of each slot's PRN"""
    prns = [int(q) for q in la.prns]
    for j, s in enumerate(slots):
        at = r * la.ch + j
        prn = s.get("prn")
        prn = prns[j % len(prns)] if prn is None else prn      # (the canonical rows: slot j tracks PRN index j)
        la.sync["loop"]["prn"][at] = prn
        if "state" not in s:
            continue
        la.sync["mode"][at] = s["mode"]
        for name, v in s["state"].items():
            la.states[name][at] = v
        if prn in prns:
            w = la.pred[r, prns.index(prn)]
            for name, v in s["pred"].items():
                w[name] = v


def _random_slots(rng, ch, prns):
    """slots of every kind, seeded: empty, unlisted and listed ones; states good, bad, waiting and stale; predictions with every outcome of
    steps 2 .. 5 drawn from the values the rows use"""
    unlisted = [q for q in range(1, 211) if q not in prns] or [0]
    slots, used = [], set()
    for _ in range(ch):
        kind = int(rng.integers(0, 12))
        if kind == 0:
            slots.append(E)
            continue
        free = [q for q in prns if q not in used]
        prn = int(rng.choice(unlisted)) if kind == 1 or not free else int(rng.choice(free))      # (one slot per PRN: each has its own record)
        used.add(prn)
        b = int(rng.choice([25000, 424, BIG, int(rng.integers(0, 1 << 40))]))
        z = b - int(rng.integers(-3, 3000))
        flags = int(rng.choice([PE, PE, PE | AMB, PE | AMB, PE | TOW, PE | TOW | AMB, PE | TOW | CONF, O.F_PHASE, O.F_EDGE, PE | 64]))
        m = int(rng.choice([0, 0, 0, 1, 19, 1, 19, 2, 10, 18]))
        k = int(rng.choice([-1, 0, 0, 1]))
        phase = float(np.float32(rng.uniform(0.0, 9.0) if k < 0 else rng.uniform(16359.0, 16367.9) if k > 0 else rng.uniform(10.0, 16350.0)))
        cp = (phase + float(rng.choice([0.5, -3.0, 7.99, 8.01, -8.0, 100.0]))) - 16368.0 * k
        s = slot(prn, b, z, int(rng.choice([0, 3, MAX_AGE, MAX_AGE + 1])), phase, flags, 0, m, k, cp if rng.integers(0, 30) else NAN,
                 float(rng.choice([4.0, MAX_SIGMA, f32_above(MAX_SIGMA)])), int(rng.choice([3, 3, 3, 1])), None, int(rng.integers(0, 3)))
        if flags & TOW:      # an anchor that agrees (before or after the shift) or does not
            s["state"]["tx_ms_at_edge"] = (BASE + int(rng.choice([0, 0, m, 20, -20]))) % W
        if rng.integers(0, 25) == 0:
            s["state"]["reserved"] = 7
        slots.append(s)
    return slots


def launch(n_rx, n_prn=N_PRN, ch=CH, seed=0):
    """the rows in the first receivers where the shape holds them, seeded random receivers behind them and in every other shape; every
    byte no row sets is random (states of empty slots, unused prediction records, the observables, the sync states but for the fields read)"""
    rng = np.random.default_rng([29, seed, n_rx, n_prn, ch])
    la = Launch()
    more = [q for q in range(1, 211) if q not in PRNS and q != UNLISTED]
    la.n_rx, la.n_prn, la.ch = n_rx, n_prn, ch
    la.prns = np.array((PRNS + more)[:n_prn] if n_prn >= N_PRN else more[:n_prn], np.uint8)
    draw = lambda n, d: np.frombuffer(rng.bytes(n * d.itemsize), d).copy()      # noqa: E731
    la.pred_rx, la.pred = draw(n_rx, P.PRED_RX_DTYPE), draw(n_rx * n_prn, P.PRED_DTYPE).reshape(n_rx, n_prn)
    la.sync, la.states, la.obs = draw(n_rx * ch, Y.STATE_DTYPE), draw(n_rx * ch, O.STATE_DTYPE), draw(n_rx * ch, O.OBS_DTYPE)
    la.rows = []
    fits = ch >= CH and n_prn >= N_PRN
    for r in range(n_rx):
        row = ROWS[r] if fits and r < len(ROWS) else None
        la.rows.append(row)
        if row is not None:
            slots = list(row.slots) + [E] * (ch - CH)
            la.pred_rx["flags"][r] = row.rx_flags
        else:
            slots = _random_slots(rng, ch, [int(q) for q in la.prns])
            la.pred_rx["flags"][r] = int(rng.choice([P.RX_PREDICTED] * 7 + [P.RX_NOT_INIT, P.RX_BAD, P.RX_PREDICTED | P.RX_ASSIGNED | P.RX_FULL]))
        _fill(la, r, slots)
    return la


def cfg(ch=CH, resolve=1, rearm=0, **kw):
    return T.make_cfg(ch, **dict(dict(max_sigma_m=MAX_SIGMA, max_resid_samples=MAX_RESID, max_age_blocks=MAX_AGE), resolve=resolve, rearm=rearm, **kw))


def run(la, c, with_obs=True):
    """the restatement on a launch -> (tow, tow_rx, sync after, states after, obs after or None); the launch's own arrays stay as they are"""
    sync, states, obs = la.sync.copy(), la.states.copy(), la.obs.copy() if with_obs else None
    tow, tow_rx = T.run(c, la.prns, la.pred_rx, la.pred, sync, states, obs)
    return tow, tow_rx, sync, states, obs


def outcome(la, r, c, tow, tow_rx, sync, states, obs):
    s = slice(r * la.ch, (r + 1) * la.ch)
    return Outcome(tow[s], tow_rx[r], la.states[s], states[s], la.sync[s], sync[s], la.obs[s], None if obs is None else obs[s], int(c["resolve"][0]), int(c["rearm"][0]))


def smoke_case():
    """the smoke run's launch: every row and as many random receivers again, at a shape with a second workgroup and odd slot and list sizes"""
    return launch(2 * len(ROWS) + 1, 7, 5, seed=29), cfg(5, resolve=1, rearm=1)


def write_smoke(path):
    """tests/golden/wtow_smoke.npz: the launch's fabricated inputs and the restatement's records, states and observables"""
    la, c = smoke_case()
    tow, tow_rx, sync, states, obs = run(la, c)
    np.savez_compressed(path, cfg=c, prns=la.prns, pred_rx=la.pred_rx, pred=la.pred, sync_before=la.sync, states_before=la.states, obs_before=la.obs,
                        tow=tow, tow_rx=tow_rx, sync_after=sync, states_after=states, obs_after=obs)


# ---- physics: the stream of weighted_pvt_cases, the restatements all the way ----------------------------------------------------------------
# MEASURED on the CPU (tests/test_weighted_tow_reference.py prints them; the GPU-side repeat is bounded at 1.5 x resid_samples):
#   resid_samples: the largest |rho| over the stream's four slots at block 25 000, the loop's code phase against gpsx_wpred's
#   sigma_m: the largest sigma_m of those four predictions
MEASURED = {"resid_samples": 0.0502251, "sigma_m": 5.03097}
STREAM = dict(max_sigma_m=300.0, max_resid_samples=8.0, max_age_blocks=40, resolve=1)      # 8 samples = 150 m: between the measured residual and the 8184 where the millisecond turns
EDGE_GUARD = 512.0
