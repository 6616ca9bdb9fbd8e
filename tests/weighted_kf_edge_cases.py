"""What the CPU and GPU tests of the navigation filter at the edges of its input space share (include/gpsx.h gpsx_wkf;
tests/test_weighted_kf_edge_reference.py, tests/test_gpu_weighted_kf_edges.py).  weighted_kf_cases.launch_case draws every receiver at one
instant (tk = -2465 s, e <= 0.012, f2 = tgd = sva = 0, toc = toe, four mid-latitude sites), 1000 blocks a launch, lock records that are
all or nothing, cfg.ion all zero and one kind of BAD state.  Here: weighted_edge_cases' receivers carried forward as tracks (tk to either
end of the span and across the 7201 s limit between two launches, e to 0.4, every clock term, both Klobuchar clamps, both troposphere
cut-offs, the week's start, middle and end, records whole weeks away), clocks steered in both directions across the week's end, both
wraps of the initialisation, lock records per slot, slots that give one row of the two, every BAD, LOST and NOT_INIT variety of the
header's steps 0, 2, 9 and 12, 1 / 7 / 4096 blocks a launch, max_coast = 0 and a set of ionosphere coefficients.  Test infrastructure;
nothing here is product code.

A case is a dict(cfg, ch, n_rx, n_blocks, obs [launch][n_rx * ch], eph, lock (or None), fix [launch] -> [n_rx], vel [n_rx], poke
{launch: [(receiver, function)]}, repair {launch: [receivers]}, names, truth [launch][receiver] -> (t, rx) or None); finish() adds what
the restatement gives, launch after launch: want, states, codes, details."""
import functools
import json
import math
import os

import numpy as np

import pvt_chain as pc
import weighted_edge_cases as X
import weighted_eph_ref as E
import weighted_fix_cases as W
import weighted_fix_ref as F
import weighted_kf_cases as C
import weighted_kf_ref as K
import weighted_obs_ref as O
import weighted_vel_ref as V

WEEK_MS = K.WEEK_MS


# ---- tracks of weighted_edge_cases' receivers --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _track(name, n_launch, n_blocks, t0, drift):
    r = X.receiver("munich_plus" if name in X.SHIFTS else name)
    rx0 = X.site_ecef(r["site"])
    t0 = r["t"] if t0 is None else t0
    v = np.asarray(X.VELOCITY, np.float64)
    out = []
    for t in C.epoch_times(t0, drift, n_launch, n_blocks):
        rx = rx0 + v * (t - t0)
        obs = np.concatenate([X.observable(row, rx, t) for row in r["rows"]])
        obs["if_freq_offset_hz"] = [X.doppler(row, rx, t, X.VELOCITY, drift) for row in r["rows"]]
        out.append(dict(t=t, rx=rx, obs=obs))
    return tuple(out)


def track(name, n_launch=4, n_blocks=500, t0=None, drift=X.DRIFT):
    """weighted_edge_cases.receiver(name)'s twelve satellites seen from a receiver that leaves the site at t0 (None: the receiver's own
    instant) at X.VELOCITY, its clock gaining `drift` seconds per second, as weighted_kf_cases.track has it: true time advances by
    n_blocks ms / (1 + drift) per launch.  A SHIFTS copy is munich_plus' track with its records whole weeks away
    -> ([dict(t, rx, obs [12])] per launch, eph [12]); copies"""
    eps = _track("munich_plus" if name in X.SHIFTS else name, n_launch, n_blocks, t0, float(drift))
    return [dict(e, obs=e["obs"].copy()) for e in eps], X.receiver(name)["eph"].copy()


def week_of(name):
    """the week the receiver's clock is in: weighted_edge_cases' records' (prev_week's records are the week before's)"""
    return pc.WEEK + X.SHIFTS.get(name, 0)


# ---- the restatement over a case ----------------------------------------------------------------------------------------------------------
def apply_pokes(case, k, st, before):
    """launch k's repairs and pokes on the states `st` [n_rx], in place: a repaired receiver gets `before`'s state (the states as they
    were ahead of the pokes), a poked one what its function writes -> the states ahead of them (a copy), or `before` if launch k has
    neither"""
    if k not in case["poke"] and k not in case["repair"]:
        return before
    was = st.copy()
    for r in case["repair"].get(k, ()):
        st[r] = before[r]
    for r, fn in case["poke"].get(k, ()):
        fn(st, r)
    return was


def finish(case):
    """the restatement on the case's launches, from zeroed states -> the case with want, states (after each launch), codes, details"""
    n_rx = case["n_rx"]
    state, before = np.zeros(n_rx, K.STATE_DTYPE), None
    want, states, codes, details = [], [], [], []
    for k in range(len(case["obs"])):
        before = apply_pokes(case, k, state, before)
        d = {}
        rec, state, rc = K.run(case["cfg"], case["obs"][k], case["eph"], state, n_rx, case["n_blocks"], case["lock"], case["fix"][k], case["vel"], detail=d)
        want.append(rec)
        states.append(state.copy())
        codes.append(rc)
        details.append(d)
    return dict(case, want=want, states=states, codes=codes, details=details)


def _empty(ch, n_rx, n_launch, n_blocks, **cfg_kw):
    lock = np.zeros((n_rx, ch), F.LOCK_DTYPE)
    lock["flags"] = C.LOCK_BOTH
    vel = np.zeros(n_rx, V.VEL_DTYPE)
    vel["flags"] = V.F_TOO_FEW
    fix = np.zeros((n_launch, n_rx), F.FIX_DTYPE)
    fix["flags"] = F.F_TOO_FEW
    return dict(cfg=K.make_cfg(ch, **cfg_kw), cfg_kw=cfg_kw, ch=ch, n_rx=n_rx, n_blocks=n_blocks, obs=np.zeros((n_launch, n_rx, ch), O.OBS_DTYPE),
                eph=np.zeros((n_rx, ch), E.EPH_DTYPE), lock=lock, fix=fix, vel=vel, poke={}, repair={}, names=[],
                truth=[[None] * n_rx for _ in range(n_launch)])


def _flat(case, lock=True):
    n = len(case["obs"])
    return finish(dict(case, obs=case["obs"].reshape(n, -1), eph=case["eph"].reshape(-1), lock=case["lock"].reshape(-1) if lock else None))


def _place(case, r, eps, eph, slots, week, dtr_s=0.0, fix_at=None, vel=None):
    """receiver r of a case under construction: the track's first len(slots) satellites in `slots`, a FIX record at the true site in the
    launches of fix_at (None: every one: an initialised receiver never reads it), a velocity record if given"""
    n = len(slots)
    case["eph"][r, slots] = eph[:n]
    for k, ep in enumerate(eps):
        case["obs"][k, r, slots] = ep["obs"][:n]
        case["truth"][k][r] = (ep["t"], ep["rx"])
        if fix_at is None or k in fix_at:
            case["fix"][k, r] = C.fix_record(ep["rx"], slots, ep["t"], week, dtr_s)[0]
    if vel is not None:
        case["vel"][r] = vel[0]


# ---- edge launches ------------------------------------------------------------------------------------------------------------------------
NAMES = tuple(n for n in X.ORDER if n not in X.SYNTHETIC)      # 21 physical receivers and the four copies whole weeks away
PHYSICAL = tuple(n for n in NAMES if n not in X.SHIFTS)
SHAPES = ((8, len(NAMES)), (12, len(NAMES)), (33, 17))
EDGE_LAUNCHES, EDGE_BLOCKS = 4, 500


@functools.lru_cache(maxsize=None)
def edge_case(ch, n_rx):
    """Four launches of 500 blocks, built like weighted_edge_cases.launch_case: receiver r is NAMES[r], so different kinds are neighbours
    in a wave; its satellites (twelve at most) start at slot r % ch and wrap (a copy whole weeks away sits in munich_plus' slots, so that
    its bytes can be munich_plus'); INIT from a FIX record at the true site (every fourth receiver's clock 0.3 ms fast in it), every
    second receiver (and every copy, as munich_plus) is offered a velocity record; no lock records"""
    names = NAMES[:n_rx]
    case = _empty(ch, n_rx, EDGE_LAUNCHES, EDGE_BLOCKS)
    for r, name in enumerate(names):
        eps, eph = track(name, EDGE_LAUNCHES, EDGE_BLOCKS)
        start = names.index("munich_plus") if name in X.SHIFTS else r
        slots = [(start + k) % ch for k in range(min(ch, 12))]
        _place(case, r, eps, eph, slots, week_of(name), dtr_s=3e-4 if r % 4 == 1 else 0.0,
               vel=C.vel_record(X.VELOCITY, X.DRIFT) if r % 2 == 0 or name in X.SHIFTS else None)
    case["names"] = list(names)
    return _flat(case, lock=False)


# ---- steering and the week's wraps ----------------------------------------------------------------------------------------------------------
# name -> (GPS time at the end of launch 0, drift, the launch in which every slot is cut or None, (t, dtr_s) of the FIX record or None:
# the true time, the week's number added to the records' week in it).  t_week_end's sky, 1000 blocks a launch.
#   up:    the clock reads 604 797 000 ms at INIT, b = +0.4975 ms and grows by 1e-3 ms a launch: above ms / 2 in launch 3, whose step 1
#          has just wrapped rcv_ms to 0 in week + 1 -- step 11 takes it back to 604 799 999 in the week before
#   down:  the mirror image: 604 796 999 ms, b = -0.4975 ms, step 11 wraps 604 799 999 + 1 to 0 in week + 1
#   coast: `up` with no usable slot in launch 3: the prediction alone crosses (COAST | STEERED)
#   init_over:  rx_tow_s = 604 799.9996: m = W, so rcv_ms = 0 in week + 1 (b = +0.4 ms)
#   init_under: rx_tow_s - dtr_s = 0.002 - 0.003 in the week after: m = -1, so rcv_ms = 604 799 999 in the records' week
STEER_LAUNCHES, STEER_BLOCKS, STEER_AT = 7, 1000, 3
STEER = {"up": (604796.9995025, 1e-6, None, None, 0), "down": (604796.9994975, -1e-6, None, None, 0), "coast": (604796.9995025, 1e-6, STEER_AT, None, 0),
         "init_over": (604799.9996, 1e-6, None, None, 0), "init_under": (604799.999, -1e-6, None, (-0.001, 0.003), 1)}


@functools.lru_cache(maxsize=None)
def steer_case():
    ch, names = 12, tuple(STEER)
    case = _empty(ch, len(names), STEER_LAUNCHES, STEER_BLOCKS)
    for r, name in enumerate(names):
        t0, drift, cut, rec, dweek = STEER[name]
        eps, eph = track("t_week_end", STEER_LAUNCHES, STEER_BLOCKS, t0, drift)
        slots = [(r + k) % ch for k in range(12)]
        _place(case, r, eps, eph, slots, pc.WEEK, fix_at=(0,) if rec else None, vel=C.vel_record(X.VELOCITY, drift))
        if rec:
            case["fix"][0, r] = C.fix_record(eps[0]["rx"], slots, rec[0], pc.WEEK + dweek, rec[1])[0]
        if cut is not None:
            case["obs"]["flags"][cut, r] &= ~np.uint32(O.F_VALID)
    case["names"] = list(names)
    return _flat(case, lock=False)


# ---- slot edges -----------------------------------------------------------------------------------------------------------------------------
SLOT_KINDS = ("plain", "code_only", "carrier_only", "mixed", "freq_not_finite", "unhealthy", "a_zero", "a_small", "cut_all")
MIXED_LOCK = (1, 2, 3, 0, 1, 2, 3, 3)      # CODE | CARRIER per slot: pr_mask 0xd5, dop_mask 0xe6
FREQ_INF, FREQ_NAN, SVH_SLOT, A_ZERO_SLOT, A_SMALL_SLOT, A_SMALL = 2, 5, 1, 3, 6, 6e6
# a broadcast set that is not the default one (alpha 1.5 x, beta moved): the solution moves by 1.5 m
ION = (0.1677E-07, -0.1118E-07, -0.8942E-07, 0.1788E-06, 0.1290E+06, -0.2294E+06, -0.0655E+06, 0.1049E+07)
SLOT_LAUNCHES = 5
# (n_blocks, max_coast, ion): the second has max_coast = 0 -- a launch without a pseudorange row is LOST at once
SLOT_CASES = ((1000, 2, ION), (1000, 0, None), (1, 2, None), (7, 2, None), (4096, 2, None))


@functools.lru_cache(maxsize=None)
def slot_case(n_blocks, max_coast, ion):
    """Five launches of 2 x 9 eight-slot receivers on weighted_kf_cases' tracks (four sites, both drifts), receiver r of
    SLOT_KINDS[r % 9]: lock records with CODE alone (no Doppler row), CARRIER alone (UPDATED on Doppler rows while n_starved counts up
    to LOST, then INIT again from the record offered in every launch), MIXED_LOCK; if_freq_offset_hz +Inf and NaN in two slots; svh = 1;
    A = 0 (no satellite); A = 6e6 (|ps| < Re: a Doppler row without a pseudorange row); every slot cut from the second launch on"""
    ch, n_rx = 8, 2 * len(SLOT_KINDS)
    sites = sorted(W.SITES)
    case = _empty(ch, n_rx, SLOT_LAUNCHES, n_blocks, max_coast=max_coast, ion=ion)
    for r in range(n_rx):
        kind, drift = SLOT_KINDS[r % len(SLOT_KINDS)], (1e-6, -1e-6)[r % 2]
        eps, eph = C.track(sites[r % 4], 8, 3 * (r % 3), C.VELOCITY, drift, SLOT_LAUNCHES, n_blocks)
        slots = [(r + k) % ch for k in range(8)]
        _place(case, r, eps, eph, slots, int(eph["week"][0]), dtr_s=(0.0, 3e-4)[r % 2], vel=C.vel_record(C.VELOCITY, drift) if r % 2 == 0 else None)
        if kind == "code_only":
            case["lock"]["flags"][r] = K.LOCK_CODE
        elif kind == "carrier_only":
            case["lock"]["flags"][r] = K.LOCK_CARRIER
        elif kind == "mixed":
            case["lock"]["flags"][r] = MIXED_LOCK
        elif kind == "freq_not_finite":
            case["obs"]["if_freq_offset_hz"][:, r, FREQ_INF], case["obs"]["if_freq_offset_hz"][:, r, FREQ_NAN] = np.inf, np.nan
        elif kind == "unhealthy":
            case["eph"]["svh"][r, SVH_SLOT] = 1
        elif kind == "a_zero":
            case["eph"]["A"][r, A_ZERO_SLOT] = 0.0
        elif kind == "a_small":
            case["eph"]["A"][r, A_SMALL_SLOT] = A_SMALL
            case["obs"]["flags"][1, r, A_SMALL_SLOT] &= ~np.uint32(O.F_VALID)      # (the first update's gate is as wide as P0)
        elif kind == "cut_all":
            case["obs"]["flags"][1:, r] &= ~np.uint32(O.F_VALID)
        case["names"].append(kind)
    return _flat(case)


# ---- state pokes ------------------------------------------------------------------------------------------------------------------------------
def set_field(field, idx, val):
    def fn(st, r):
        if idx is None:
            st[field][r] = val
        else:
            st[field][r, idx] = val
    return fn


def _p01(st, r):      # P_01 = 2 sqrt(P_00 P_11): the second pivot of INV(P-) is about -3 P_11
    st["P"][r, K.tri(0, 1)] = 2.0 * math.sqrt(st["P"][r, K.tri(0, 0)] * st["P"][r, K.tri(1, 1)])


def _origin(st, r):      # x- is 36 m from the earth's centre: ecef2pos gives a height just above -Re there
    st["x"][r, :3] = 0.0


def _origin_at_rest(st, r):      # x- is the earth's centre itself: ecef2pos' loop does not run, the height is -Re exactly
    st["x"][r, :3], st["x"][r, 4:7] = 0.0, 0.0


BIG = 1.7e308
# name -> (what is written to the state ahead of launch 2, the slots are cut in launch 2, what launch 2 must end in)
STATE_POKES = {"bad_x_nan": (set_field("x", 7, np.nan), False, K.F_BAD), "bad_x_inf": (set_field("x", 0, -np.inf), False, K.F_BAD),
               "bad_p_inf": (set_field("P", K.tri(3, 5), np.inf), False, K.F_BAD), "bad_flag_bit": (set_field("flags", None, 3), False, K.F_BAD),
               "bad_rcv_week": (set_field("rcv_ms", None, WEEK_MS), False, K.F_BAD), "bad_rcv_minus": (set_field("rcv_ms", None, -1), False, K.F_BAD),
               "bad_p33_zero": (set_field("P", K.tri(3, 3), 0.0), False, K.F_BAD), "bad_p77_minus": (set_field("P", K.tri(7, 7), -1.0), False, K.F_BAD),
               "lost_pivot": (_p01, False, K.F_LOST), "coast_pivot": (_p01, True, K.F_COAST),
               "lost_x4_big": (set_field("x", 4, BIG), False, K.F_LOST), "lost_x4_big_cut": (set_field("x", 4, BIG), True, K.F_LOST),
               "lost_p44_big": (set_field("P", K.tri(4, 4), BIG), False, K.F_LOST), "lost_p44_big_cut": (set_field("P", K.tri(4, 4), BIG), True, K.F_LOST),
               "origin": (_origin, False, K.F_COAST | K.F_REJECTED), "origin_at_rest": (_origin_at_rest, False, K.F_COAST | K.F_REJECTED)}
# name -> what is spoiled in the records offered in launches 0 .. 2 (launch 3 offers a good one): NOT_INIT, nothing written
FIX_POKES = {"tow_nan": ("rx_tow_s", None, np.nan), "tow_inf": ("rx_tow_s", None, np.inf), "tow_1e300": ("rx_tow_s", None, 1e300),
             "rr_nan": ("rr", 1, np.nan), "vel_inf": ("vel", 2, np.inf)}
POKED = tuple(STATE_POKES) + tuple(FIX_POKES)
POKE_LAUNCHES, POKE_AT, POKE_BLOCKS = 4, 2, 1000
POKE_PLACES = (0, 7, 3)      # the place in its wave of eight receivers, in turn: with one poked receiver per wave none is next to another


def poke_index(i):
    return 8 * i + POKE_PLACES[i % 3]


@functools.lru_cache(maxsize=None)
def poke_case():
    """Four launches of 8 x len(POKED) + 1 eight-slot receivers, one poked receiver per wave at its first, last or a middle place, every
    other receiver untouched: INIT, an update, the pokes and a third launch, then the BAD states put back as they were and a fourth.
    The NOT_INIT varieties are records, not states: spoiled in launches 0 .. 2 (the velocity record in every launch)"""
    ch, n_rx = 8, 8 * len(POKED) + 1
    sites = sorted(W.SITES)
    case = _empty(ch, n_rx, POKE_LAUNCHES, POKE_BLOCKS)
    poked = {poke_index(i): name for i, name in enumerate(POKED)}
    case["poke"][POKE_AT], case["repair"][POKE_AT + 1] = [], []
    for r in range(n_rx):
        drift = (1e-6, -1e-6)[r % 2]
        eps, eph = C.track(sites[r % 4], 8, 3 * (r % 3), C.VELOCITY, drift, POKE_LAUNCHES)
        slots = [(r + k) % ch for k in range(8)]
        name = poked.get(r)
        _place(case, r, eps, eph, slots, int(eph["week"][0]), vel=C.vel_record(C.VELOCITY, drift) if r % 2 == 0 or name == "vel_inf" else None)
        if name in STATE_POKES:
            fn, cut, _ = STATE_POKES[name]
            case["poke"][POKE_AT].append((r, fn))
            if cut:
                case["obs"]["flags"][POKE_AT, r] &= ~np.uint32(O.F_VALID)
            if name.startswith("bad"):
                case["repair"][POKE_AT + 1].append(r)
        elif name == "vel_inf":
            case["vel"]["vel"][r, 2] = np.inf
        elif name in FIX_POKES:
            field, idx, val = FIX_POKES[name]
            for k in range(POKE_LAUNCHES - 1):
                if idx is None:
                    case["fix"][field][k, r] = val
                else:
                    case["fix"][field][k, r, idx] = val
        case["names"].append(name or "untouched")
    return _flat(case)


def without_pokes(case):
    """the same launches with no state poked (the spoiled records stay: they are inputs), through the restatement"""
    return finish(dict(case, poke={}, repair={}))


# ---- the device-only invariants' launches ---------------------------------------------------------------------------------------------------
PERMUTED_CH, PERMUTED_RX = (1, 5, 33, 64), 17
LONG_LAUNCHES = 32


def permutations(n_rx):
    """a reversal and one fixed shuffle"""
    return np.arange(n_rx)[::-1].copy(), np.random.default_rng(2026).permutation(n_rx)


@functools.lru_cache(maxsize=None)
def repair_case():
    """Four launches of three eight-slot receivers on one Munich track: the first as it is, the second with slot 3 a millisecond early
    and the third with slot 5 a millisecond late in launch 2, both AMBIGUOUS"""
    ch = 8
    case = _empty(ch, 3, 4, C.N_BLOCKS)
    eps, eph = C.track("munich", 8, 0, C.VELOCITY, 1e-6, 4)
    for r in range(3):
        _place(case, r, eps, eph, list(range(8)), int(eph["week"][0]), vel=C.vel_record(C.VELOCITY, 1e-6))
        case["names"].append(("unshifted", "early", "late")[r])
    for r, slot, ms in ((1, 3, -1), (2, 5, 1)):
        case["obs"]["tx_ms"][2, r, slot] += ms
        case["obs"]["flags"][2, r, slot] |= O.F_AMBIGUOUS
    return _flat(case)


@functools.lru_cache(maxsize=None)
def long_case():
    """32 launches of three eight-slot Munich receivers (three skies, both drifts), noise-free: what 31 updates in a row do to parity"""
    ch = 8
    case = _empty(ch, 3, LONG_LAUNCHES, C.N_BLOCKS)
    for r in range(3):
        drift = (1e-6, -1e-6)[r % 2]
        eps, eph = C.track("munich", 8, 3 * r, C.VELOCITY, drift, LONG_LAUNCHES)
        _place(case, r, eps, eph, [(r + k) % ch for k in range(8)], int(eph["week"][0]), vel=C.vel_record(C.VELOCITY, drift) if r != 1 else None)
        case["names"].append(f"munich sky {3 * r}")
    return _flat(case)


# ---- decisions ------------------------------------------------------------------------------------------------------------------------------
TK_LIMIT, TK_CLEAR, STEER_CLEAR_M, INIT_CLEAR_MS = 7201.0, 1e-3, 1.0, 1e-3


def decisions_clear(case):
    """weighted_kf_cases.decisions_clear's four margins over the case's launches, and three more: every candidate slot's |tk| at least
    1e-3 s from the 7201 s limit, step 11's x+_3 at least 1 m from +- ms / 2, step 2's u at least 1e-3 ms from a half-integer.  A
    receiver that the restatement ends LOST on a pivot is left out of the share margin (its share is not above 1e-7: it failed) and must
    have failed clearly instead: a share below -1e-7 or one that is not finite, or a result that is not finite (step 12) -- and then its
    rows' margins do not count, for it is LOST whatever they decide
    -> the margins found: dict(gate, rint, share, el, tk, steer, init)"""
    details, m = [], dict(tk=np.inf, steer=np.inf, init=np.inf)
    for d, want in zip(case["details"], case["want"]):
        d = dict(d, **{k: d[k].copy() for k in ("shares", "gate_pr", "gate_dop", "rint_arg", "el")})
        for r in np.flatnonzero(d["pivot_failed"] | d["not_finite"]):
            row = d["shares"][r]
            clear = d["not_finite"][r] or (~np.isfinite(row)).any() or float(row[np.isfinite(row)].min()) < -C.SHARE_CLEAR
            assert want["flags"][r] in (K.F_LOST, K.F_NOT_INIT) and (clear or d["starved_out"][r]), (r, row)
            d["shares"][r] = np.nan
            if clear:      # (whatever its rows decide, the receiver ends LOST)
                for k in ("gate_pr", "gate_dop", "rint_arg", "el"):
                    d[k][r] = np.nan
        details.append(d)
        tk = d["tk"][np.isfinite(d["tk"])]
        if tk.size:
            m["tk"] = min(m["tk"], float(np.abs(np.abs(tk) - TK_LIMIT).min()))
        x3 = d["x3_pre"][np.isfinite(d["x3_pre"])]
        if x3.size:
            m["steer"] = min(m["steer"], float(np.abs(np.abs(x3) - K.MS / 2.0).min()))
        u = d["init_u"][np.isfinite(d["init_u"])]
        if u.size:
            m["init"] = min(m["init"], float(np.abs(np.abs(u - np.floor(u)) - 0.5).min()))
    m.update(C.decisions_clear(details))
    assert m["tk"] > TK_CLEAR and m["steer"] > STEER_CLEAR_M and m["init"] > INIT_CLEAR_MS, m
    return m


# ---- comparison -------------------------------------------------------------------------------------------------------------------------------
def measure(got, want):
    """weighted_kf_cases.compare's per-field maxima over the records that hold a solution, nothing asserted"""
    solved = (want["flags"] & (K.F_INIT | K.F_UPDATED | K.F_COAST)) != 0
    g, w = got[solved], want[solved]
    mx = lambda a: float(np.nan_to_num(np.abs(a), nan=np.inf).max()) if a.size else 0.0      # noqa: E731
    return {"rr_m": mx(g["rr"] - w["rr"]), "clk_m": mx(g["clk_m"] - w["clk_m"]), "height_m": mx(g["geo"][:, 2] - w["geo"][:, 2]),
            "lat_m": mx(g["geo"][:, 0] - w["geo"][:, 0]) * 6.4e6, "lon_m": mx((g["geo"][:, 1] - w["geo"][:, 1]) * np.cos(w["geo"][:, 0])) * 6.4e6,
            "latlon_rad": mx(g["geo"][:, :2] - w["geo"][:, :2]), "vel_mps": mx(g["vel"] - w["vel"]), "enu_mps": mx(g["enu"] - w["enu"]),
            "cdrift_mps": mx(g["cdrift_mps"] - w["cdrift_mps"])}, int(solved.sum())


def record_parity(label, worst, n_solved):
    """under $GPSX_WKF_PARITY_JSON (weighted_kf_cases.PARITY_ENV): how profiles/r25_weighted_kf_edges_parity.json is written"""
    path = os.environ.get(C.PARITY_ENV)
    if not path or label is None:
        return
    doc = json.load(open(path)) if os.path.exists(path) else {"launches": {}}
    doc["launches"][label] = dict(worst, solved=n_solved)
    doc["what"] = ("largest |device - restatement| in rr, clk_m, height (m) and vel, enu, cdrift_mps (m/s) per compared launch of "
                   "tests/test_gpu_weighted_kf_edges.py, one MI355X; written by weighted_kf_edge_cases.compare under $" + C.PARITY_ENV)
    doc["largest_m"] = max(max(w[k] for k in ("rr_m", "clk_m", "height_m")) for w in doc["launches"].values())
    doc["largest_mps"] = max(max(w[k] for k in ("vel_mps", "enu_mps", "cdrift_mps")) for w in doc["launches"].values())
    doc["cap_m"], doc["bound_m"] = C.PARITY_CAP_M, min(8.0 * doc["largest_m"], C.PARITY_CAP_M)
    doc["cap_mps"], doc["bound_mps"] = C.PARITY_CAP_MPS, min(8.0 * doc["largest_mps"], C.PARITY_CAP_MPS)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)


def compare(got, want, label):
    """the launch's maxima measured and recorded, then weighted_kf_cases.compare as it is.  rr, clk_m and height are held to this
    module's position bound, vel, enu and cdrift_mps to its velocity bound -- and latitude and longitude to the position bound as ground
    distance (|dlat| 6.4e6, |dlon| cos(lat) 6.4e6 metres), as weighted_edge_cases.compare holds them and for its reason:
    weighted_kf_cases.compare asks for bound / 6e6 radians, and at 89.9 S two filters 5e-9 m apart differ by 5e-14 rad of longitude, a
    figure that says where the receiver stands and nothing about the kernel (at the measured bound that criterion fails there; at the
    project's cap, which weighted_kf_cases.compare is given here for it, it is 573 x looser in metres than at the equator)"""
    worst, n = measure(got, want)
    record_parity(label, worst, n)
    C.compare(got, want, None, C.PARITY_CAP_M, PARITY_BOUND_MPS)      # (flags, counts, masks, bytes, sigma, NIS, the velocity bound)
    assert max(worst[k] for k in ("rr_m", "clk_m", "height_m", "lat_m", "lon_m")) <= PARITY_BOUND_M, (label, worst)
    return worst


def compare_states(got, want, keep=None):
    """weighted_kf_cases.compare_states under this module's bounds, over the receivers of `keep` (None: all)"""
    keep = slice(None) if keep is None else keep
    C.compare_states(got[keep], want[keep], PARITY_BOUND_M, PARITY_BOUND_MPS)


# ---- bounds -----------------------------------------------------------------------------------------------------------------------------------
# MEASURED on the CPU, the restatement against the truth model (tests/test_weighted_kf_edge_reference.py prints them; its bounds are
# 1.5 x these); never against the device.  edge_*: the largest error of rr, vel, cdrift_mps and clk_m over launches 1 .. 3 of every
# receiver of edge_case(12, 25); steer_*: the same over launches 1 .. 6 of steer_case().
# Measured: the edge figures are all straddle_a's (twelve slots, launches 1 and 2); what they are made of is the float32 code phase (0.009 m of
# range) and Doppler (6e-4 m/s) through the geometry, as weighted_edge_cases.MEASURED["truth_m"] is.
MEASURED = {"edge_pos_m": 0.0394795, "edge_vel_mps": 0.0325720, "edge_cdrift_mps": 0.0273682, "edge_clk_m": 0.0488595,
            "steer_pos_m": 0.0150491, "steer_vel_mps": 0.00318341, "steer_cdrift_mps": 0.00326491, "steer_clk_m": 0.0255355}
# the device against the restatement: 8 x the largest difference measured on one MI355X over every labelled launch of
# tests/test_gpu_weighted_kf_edges.py (profiles/r25_weighted_kf_edges_parity.json: that file run with $GPSX_WKF_PARITY_JSON naming it),
# capped at the project's 1e-4 m and 1e-6 m/s.  Until measured, the caps hold.
# Measured: 1.5832e-8 m (rr and height, slot_case at 4096 blocks, its last launch; the edge launches 6.5e-9 m, steering 5.6e-9 m, the pokes
# 1.2e-8 m, the 32-launch run at most 4.7e-9 m with no growth over the launches) -- 1.2 x weighted_kf_cases' 1.3039e-8 m: e = 0.4 and
# |tk| = 7200 s cost nothing.  3.6754e-7 m/s (cdrift_mps, slot_case at 1 block, its last launch) -- 109 x weighted_kf_cases' 3.3722e-9 m/s, and
# not the kernel's arithmetic: it is the code_only receiver's, which has no Doppler row and so observes its drift through the change of
# the clock term over dt = 1 ms alone.  In the restatement 1e-8 m on that receiver's x_3 ahead of a launch moves its cdrift_mps by
# 1.1e-6 m/s at 1 block, 7.3e-7 at 7, 5.5e-9 at 1000 and 2.0e-9 at 4096 (every other kind: below 1e-10), and the device's clk_m there is
# 4e-9 .. 7e-9 m from the restatement's; at 7 blocks the same receiver gives 2.8e-7 m/s, everywhere else the largest is 9.0e-9 m/s (1000 blocks).  8 x
# this figure is above the cap, so the cap is the velocity bound.
PARITY_MEASURED_M = 1.5832e-8
PARITY_MEASURED_MPS = 3.6754e-7
PARITY_BOUND_M = C.PARITY_CAP_M if PARITY_MEASURED_M is None else min(8.0 * PARITY_MEASURED_M, C.PARITY_CAP_M)
PARITY_BOUND_MPS = C.PARITY_CAP_MPS if PARITY_MEASURED_MPS is None else min(8.0 * PARITY_MEASURED_MPS, C.PARITY_CAP_MPS)
