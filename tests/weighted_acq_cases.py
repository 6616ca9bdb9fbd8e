"""The acquisition decisions and the slot hand-over, clause by clause (include/gpsx.h gpsx_wacq): a table of fabricated peak records
and slot states that reach every clause of the definition, shared by tests/test_weighted_acq_reference.py (the restatement alone:
every row's predicate proves its clause on the restatement's own integers) and tests/test_gpu_weighted_acq.py (k_wacq against the
restatement, byte for byte), and the two-receiver scenario with what was measured on it.

A row is ONE receiver at the canonical shape: 5 PRN indices x 8 Doppler bins, 4 slots.  cfg and the Doppler grid are per launch, so
the rows are grouped:
  A   det 5/2, min_peak 1000, lead_blocks 80, code_per_hz GPSX_WAID_L1CA, evict_after_blocks 1000, bins -5000 + 1500 b Hz
  B   the same with lead_blocks 0 and min_peak 0: the phase is not projected; max(min_peak, 1)
  C   the same as A with code_per_hz 0: the phase is not projected
  D   lead_blocks 1, bins -3475 + 500 b Hz (bin 7: 25 Hz): a step below half an ulp of 16368
For a launch of another shape a row is embedded (embed): its PRN indices and bins keep their order but are spread over the launch's,
the PRN rows and bins between them are filled with records that win nothing, the slots behind its four hold channels that stay; a
smaller shape takes the row's first indices, bins and slots.  The predicates are proven at the canonical shape; random receivers
(random_rx: any number of detections, slots in every condition) are tiled between the rows at every shape."""
from types import SimpleNamespace

import numpy as np

import weighted_acq_ref as Q
import weighted_lock_ref as R

F = np.float32
N_PRN, N_DOPP, CH = 5, 8, 4
WAID_L1CA = F(0.010389610)
NONE = Q.PRN_NONE
U32 = (1 << 32) - 1
GROUPS = {"A": (Q.make_cfg(CH, (5, 2), 1000, 80, WAID_L1CA, 1000), (-5000, 1500)),
          "B": (Q.make_cfg(CH, (5, 2), 0, 0, WAID_L1CA, 1000), (-5000, 1500)),
          "C": (Q.make_cfg(CH, (5, 2), 1000, 80, 0.0, 1000), (-5000, 1500)),
          "D": (Q.make_cfg(CH, (5, 2), 1000, 1, WAID_L1CA, 1000), (-3475, 500))}


def prn_list(n_prn):
    """n_prn distinct PRN numbers of 1 .. 210 (11 is coprime to 210)"""
    return np.array([(11 * i) % 210 + 1 for i in range(n_prn)], np.uint8)


def other_prn(k):
    """a PRN number that no list of up to 64 holds"""
    return (11 * (100 + k)) % 210 + 1


# ---- a row's records: {PRN index: {bin: (M, S, tau)}}; what is not named is absent() ----------------------------------------------
def absent(p, b):
    """a record that is no detection under any group's cfg: peak over mean 2 (the threshold is 5/2), M of 1000 .. 1770"""
    m = 1000 + 110 * b + 17 * p
    return m, m * Q.PHASES // 2, (977 * b + 131 * p) % Q.PHASES


def present(m, tau, ratio=8):
    """a record whose peak is `ratio` times its mean"""
    return m, m * Q.PHASES // ratio, tau


def _rec(m, s, tau):
    """(M, S, tau) in a peak record's order (avr is filled in at the end)"""
    return m, tau, s, 0


class Row(SimpleNamespace):
    pass


def _row(group, name, check, recs=None, slots=None):
    """slots: up to four of (PRN or ("row", p) or NONE, lock flags, blocks_seen); missing ones are empty"""
    slots = list(slots or []) + [(NONE, 0, 0)] * (CH - len(slots or []))
    return Row(group=group, name=name, check=check, recs=recs or {}, slots=slots)


def _flags(o, p):
    return int(o.det[p]["flags"])


def _st(o, j):
    return o.sync[j]["loop"]


def _only(o, assigned=None, evicted=(), written=None):
    """the receiver's outcome in one look: {PRN index: slot}, the evicted slots, the slots written"""
    t = o.trace
    want_written = sorted(set((assigned or {}).values()) | set(evicted)) if written is None else written
    return t["assigned"] == (assigned or {}) and t["evicted"] == list(evicted) and t["written"] == want_written


def _untouched(o, slots):
    return all(o.sync[j].tobytes() == o.sync0[j].tobytes() and o.lock[j].tobytes() == o.lock0[j].tobytes() for j in slots)


def _lhs(o, p):
    _, m, s, _ = o.trace["best"][p]
    return m * Q.PHASES * o.cfg["det_den"], o.cfg["det_num"] * s


KEPT = (R.F_CODE, 5000)          # a slot that stays: the code is there
STALE = (0, 1000)                # ... that goes: no code, evict_after_blocks reached


def _rows():
    rows = []
    add = lambda *a, **kw: rows.append(_row(*a, **kw))      # noqa: E731
    big = 450000
    # -- detection
    add("A", "no_detection", lambda o: o.trace["detected"] == [] and _only(o) and int(o.acq["flags"]) == 0 and int(o.acq["free_mask"]) == 15
        and all(_flags(o, p) == 0 and int(o.det[p]["slot"]) == -1 for p in range(N_PRN)))
    add("A", "ratio_met_with_equality_and_missed_by_one",
        lambda o: _lhs(o, 0)[0] == _lhs(o, 0)[1] and 0 in o.trace["detected"] and _lhs(o, 1)[1] - _lhs(o, 1)[0] == o.cfg["det_num"]
        and 1 not in o.trace["detected"] and _only(o, {0: 0}),
        recs={0: {3: (5000, 5000 * Q.PHASES * 2 // 5, 77)}, 1: {3: (5000, 5000 * Q.PHASES * 2 // 5 + 1, 78)}})
    add("A", "min_peak_met_with_equality_and_missed_by_one",
        lambda o: o.trace["best"][0][1] == o.cfg["min_peak"] and 0 in o.trace["detected"] and o.trace["best"][1][1] == o.cfg["min_peak"] - 1
        and _lhs(o, 1)[0] >= _lhs(o, 1)[1] and 1 not in o.trace["detected"],
        recs={0: {b: ((1000, 1000 * 2046, 5) if b == 2 else (900 - b, 900 * Q.PHASES // 2, b)) for b in range(N_DOPP)},
              1: {b: ((999, 999 * 2046, 6) if b == 2 else (900 - b, 900 * Q.PHASES // 2, b)) for b in range(N_DOPP)}})
    add("B", "min_peak_zero_still_asks_for_one",
        lambda o: o.cfg["min_peak"] == 0 and o.trace["best"][0][:3] == (0, 0, 0) and 0 not in o.trace["detected"] and _lhs(o, 0) == (0, 0)
        and o.trace["best"][1][:3] == (4, 1, 0) and 1 in o.trace["detected"],
        recs={0: {b: (0, 0, 40 + b) for b in range(N_DOPP)}, 1: {b: ((1, 0, 50) if b == 4 else (0, 0, b)) for b in range(N_DOPP)}})
    add("A", "all_ones", lambda o: o.trace["best"][2][1:3] == (U32, U32) and _lhs(o, 2)[0] < 1 << 56 and 2 in o.trace["detected"] and _only(o, {2: 0})
        and int(o.det[2]["max_val"]) == U32,
        recs={2: {6: (U32, U32, 16367)}})
    # -- ties
    add("A", "tie_between_bins_lowest_wins",
        lambda o: o.trace["best"][1][0] == 2 and o.trace["best"][1][3] == 2002 and int(o.det[1]["dopp_hz"]) == -5000 + 2 * 1500
        and float(_st(o, 0)["if_freq_offset_hz"]) == -2000.0,
        recs={1: {2: present(big, 2002), 5: present(big, 5005), 7: present(big, 7007)}})
    add("A", "tie_between_prns_lower_index_wins",
        lambda o: o.trace["candidates"] == [1, 3] and o.trace["best"][1][1] == o.trace["best"][3][1] and _only(o, {1: 2})
        and _flags(o, 3) == Q.DET_DETECTED | Q.DET_DROPPED and int(o.acq["flags"]) == Q.F_ASSIGNED | Q.F_FULL and int(o.acq["n_dropped"]) == 1,
        recs={1: {4: present(big, 100)}, 3: {1: present(big, 200)}},
        slots=[(other_prn(0),) + KEPT, (other_prn(1),) + KEPT, (NONE, 0, 0), (other_prn(2),) + KEPT])
    # -- slots
    add("A", "more_candidates_than_free_slots",
        lambda o: o.trace["candidates"] == [3, 0, 4, 2] and _only(o, {3: 1, 0: 3}) and o.trace["dropped"] == [4, 2]
        and [_flags(o, p) for p in (4, 2)] == [Q.DET_DETECTED | Q.DET_DROPPED] * 2 and int(o.acq["flags"]) & Q.F_FULL and int(o.acq["free_mask"]) == 0
        and int(o.acq["assigned_mask"]) == 0b1010 and [int(o.det[p]["slot"]) for p in range(N_PRN)] == [3, -1, -1, 1, -1],
        recs={0: {0: present(big - 1, 10)}, 2: {1: present(big - 3, 20)}, 3: {2: present(big, 30)}, 4: {3: present(big - 2, 40)}},
        slots=[(other_prn(0),) + KEPT, (NONE, 0, 0), (other_prn(1),) + KEPT, (NONE, 0, 0)])
    add("A", "detected_prn_in_a_kept_slot_is_tracked",
        lambda o: o.trace["tracked"] == [0] and _flags(o, 0) == Q.DET_DETECTED | Q.DET_TRACKED and int(o.det[0]["slot"]) == -1 and _only(o)
        and int(o.acq["n_tracked"]) == 1 and int(o.acq["flags"]) == 0 and _untouched(o, range(CH)),
        recs={0: {5: present(big, 300)}}, slots=[(NONE, 0, 0), (("row", 0),) + KEPT])
    add("A", "the_prn_only_in_a_slot_evicted_this_call_is_a_candidate",
        lambda o: o.trace["tracked"] == [] and _only(o, {0: 0}, evicted=[0]) and _flags(o, 0) == Q.DET_DETECTED | Q.DET_ASSIGNED
        and int(o.acq["flags"]) == Q.F_ASSIGNED | Q.F_EVICTED and int(_st(o, 0)["prn"]) == o.prns[0] and int(o.lock[0]["blocks_seen"]) == 0,
        recs={0: {5: present(big, 300)}}, slots=[(("row", 0),) + STALE])
    add("A", "eviction_at_the_block_count_and_one_below_and_with_code",
        lambda o: _only(o, evicted=[0]) and o.trace["kept"] == [1, 2] and int(_st(o, 0)["prn"]) == NONE
        and o.sync[0].tobytes() == Q.handover_state(NONE).tobytes() and not o.lock[0].tobytes().strip(b"\0") and _untouched(o, [1, 2, 3])
        and int(o.acq["evicted_mask"]) == 1 and int(o.acq["kept_mask"]) == 0b110 and int(o.acq["free_mask"]) == 0b1001,
        slots=[(other_prn(0), 0, 1000), (other_prn(1), 0, 999), (other_prn(2), R.F_CODE, 1 << 40)])
    add("A", "an_evicted_slot_is_reused_in_the_same_call",
        lambda o: _only(o, {4: 2}, evicted=[2]) and int(_st(o, 2)["prn"]) == o.prns[4] and int(o.acq["assigned_mask"]) == 4
        and int(o.acq["evicted_mask"]) == 4 and int(o.acq["free_mask"]) == 0 and _untouched(o, [0, 1, 3]),
        recs={4: {6: present(big, 6000)}},
        slots=[(other_prn(0),) + KEPT, (other_prn(1),) + KEPT, (other_prn(2),) + STALE, (other_prn(3),) + KEPT])
    # -- the phase
    add("A", "projection_wraps_below_zero",
        lambda o: o.raw(0) < 0 and float(_st(o, 0)["code_phase_fine"]) == float(F(o.raw(0) + Q.SPAN)) and 16360 < float(_st(o, 0)["code_phase_fine"]) < 16368,
        recs={0: {7: present(big, 3)}})
    add("A", "projection_wraps_above_the_span",
        lambda o: o.raw(0) >= Q.SPAN and float(_st(o, 0)["code_phase_fine"]) == float(F(o.raw(0) - Q.SPAN)) and 0 <= float(_st(o, 0)["code_phase_fine"]) < 8,
        recs={0: {0: present(big, 16367)}})
    add("D", "projection_lands_on_the_span",
        lambda o: -2.0 ** -11 < o.raw(0) < 0 and float(_st(o, 0)["code_phase_fine"]) == 16368.0 and float(_st(o, 0)["if_freq_offset_hz"]) == 25.0,
        recs={0: {7: present(big, 0)}})
    add("B", "no_lead_no_projection",
        lambda o: o.cfg["lead_blocks"] == 0 and o.cfg["code_per_hz"] != 0 and float(_st(o, 0)["code_phase_fine"]) == 12007.0
        and float(_st(o, 1)["code_phase_fine"]) == float(F(U32)),
        recs={0: {7: present(big, 12007)}, 1: {0: present(big - 1, U32)}})
    add("C", "no_factor_no_projection",
        lambda o: o.cfg["lead_blocks"] == 80 and o.cfg["code_per_hz"] == 0 and float(_st(o, 0)["code_phase_fine"]) == 12007.0
        and int(o.sync[0]["loop"]["if_freq_accum"]) == 0,
        recs={0: {7: present(big, 12007)}})
    add("A", "the_order_of_the_two_products_shows_in_the_last_bit",
        lambda o: o.raw(0) == float(_st(o, 0)["code_phase_fine"]) and o.other_order(0) != o.raw(0)
        and abs(Q.F(o.other_order(0)).view(np.uint32).astype(np.int64) - Q.F(o.raw(0)).view(np.uint32).astype(np.int64)) == 1,
        recs={0: {0: present(big, 0)}})
    return rows


ROWS = _rows()


def random_rx(seed, n_prn, n_dopp, ch):
    """a receiver that proves nothing by itself: every PRN row detected with probability 1/2, equal peaks among them now and then,
    slots empty, kept, stale or holding a listed PRN -> (peaks [n_prn][n_dopp], [(prn, lock flags, blocks_seen)] x ch)"""
    rng = np.random.default_rng(1000 + seed)
    pk = np.zeros((n_prn, n_dopp), Q.PEAK_DTYPE)
    pk["max_val"] = rng.integers(1000, 3000, (n_prn, n_dopp))
    pk["sum"] = pk["max_val"].astype(np.int64) * Q.PHASES // 2
    pk["phase"] = rng.integers(0, Q.PHASES, (n_prn, n_dopp))
    for p in np.nonzero(rng.random(n_prn) < 0.5)[0]:
        m = int(rng.choice([400000, 400000, 410000, int(rng.integers(300000, 500000))]))
        for b in rng.integers(0, n_dopp, 2):             # (the same peak in up to two bins)
            pk[p, b] = _rec(m, m * Q.PHASES // 8, int(rng.integers(0, Q.PHASES)))
    pk["avr"] = pk["sum"] // Q.PHASES
    prns, slots = prn_list(n_prn), []
    for j in range(ch):
        kind = rng.integers(0, 5)
        prn = NONE if kind == 0 else int(prns[rng.integers(0, n_prn)]) if kind in (1, 2) else other_prn(int(rng.integers(0, 30)))
        slots.append((prn, int(rng.choice([0, R.F_CODE, R.F_CODE | R.F_CARRIER, R.F_EPOCH_LOCKED])), int(rng.choice([0, 999, 1000, 1001, 1 << 33]))))
    return pk, slots


def _spread(i, n_small, n_big):
    """where index i of n_small goes among n_big >= n_small: order kept, first to first, last to last"""
    return i * (n_big - 1) // (n_small - 1)


def embed(row, n_prn, n_dopp, ch):
    """the row at a launch's shape -> (peaks [n_prn][n_dopp], [(prn, lock flags, blocks_seen)] x ch)"""
    prns = prn_list(n_prn)
    pk = np.zeros((n_prn, n_dopp), Q.PEAK_DTYPE)
    p_at = [_spread(p, N_PRN, n_prn) if n_prn >= N_PRN else p for p in range(N_PRN)]
    b_at = [_spread(b, N_DOPP, n_dopp) if n_dopp >= N_DOPP else b for b in range(N_DOPP)]
    for p in range(n_prn):
        for b in range(n_dopp):
            pk[p, b] = _rec(*absent(p, b))
    for p in range(N_PRN):
        if p_at[p] >= n_prn:
            continue
        named = row.recs.get(p, {})
        canon = [named.get(b, absent(p, b)) for b in range(N_DOPP)]
        low = min(m for m, _, _ in canon)
        for b in range(n_dopp):                          # between the row's bins: nothing that wins (below the row's least peak, or 0)
            m = (low * (b % 5)) // 5
            pk[p_at[p], b] = _rec(m, (m * Q.PHASES // 2) & U32, (31 * b) % Q.PHASES)
        for b in range(N_DOPP):
            if b_at[b] < n_dopp:
                pk[p_at[p], b_at[b]] = _rec(*canon[b])
    pk["avr"] = pk["sum"] // Q.PHASES
    slots = []
    for j in range(ch):
        if j < CH:
            prn, flags, seen = row.slots[j]
            if isinstance(prn, tuple):                   # ("row", p): the PRN of the row's index p, wherever it went (none: an unlisted one)
                prn = int(prns[p_at[prn[1]]]) if p_at[prn[1]] < n_prn else other_prn(40)
            slots.append((prn, flags, seen))
        else:
            slots.append((other_prn(10 + j), R.F_CODE, 7000 + j))
    return pk, slots


def states_of(slots, seed):
    """the five state arrays of one receiver's slots: a holding slot's states are a channel's in mid-flight (every byte of the sync
    state's tail and of the four others set, so that a hand-over's zeroes show), an empty slot's sync state is a hand-over's"""
    rng = np.random.default_rng(5000 + seed)
    out = {name: np.frombuffer(rng.integers(1, 255, len(slots) * dt.itemsize, dtype=np.uint8).tobytes(), dt).copy() for name, dt in Q.STATE_DTYPES.items()}
    for j, (prn, flags, seen) in enumerate(slots):
        if prn == NONE:
            out["sync"][j] = Q.handover_state(NONE)
        else:
            out["sync"]["loop"]["prn"][j] = prn
        out["lock"]["flags"][j], out["lock"]["blocks_seen"][j] = flags, seen
    return out


def _entries(rows):
    """the rows with a random receiver (None) after every fifth and at the end, and as many more as make the period odd: receiver r
    of a launch takes entry r % period, so a row meets every one of a workgroup's four waves"""
    out = []
    for i, row in enumerate(rows):
        out.append(row)
        if i % 5 == 4:
            out.append(None)
    out.append(None)
    return out + [None] * (1 - len(out) % 2)


def launch(group, n_rx, n_prn=N_PRN, n_dopp=N_DOPP, ch=CH, rows=None):
    """a launch of the group's rows (or `rows`) with random receivers between them, tiled with an odd period -> SimpleNamespace(cfg, grid (dopp_min_hz,
    dopp_step_hz), prns, peaks [n_rx][n_prn][n_dopp], states {name: [n_rx * ch]}, rows [per receiver: the Row or None])"""
    cfg, grid = GROUPS[group]
    cfg = dict(cfg, ch_per_rx=ch)
    entries = _entries([r for r in ROWS if r.group == group] if rows is None else list(rows))
    peaks = np.zeros((n_rx, n_prn, n_dopp), Q.PEAK_DTYPE)
    states, used = {name: [] for name in Q.STATE_DTYPES}, []
    for r in range(n_rx):
        e = entries[r % len(entries)]
        pk, slots = random_rx(r, n_prn, n_dopp, ch) if e is None else embed(e, n_prn, n_dopp, ch)
        peaks[r] = pk
        st = states_of(slots, r)
        for name in states:
            states[name].append(st[name])
        used.append(e)
    return SimpleNamespace(group=group, cfg=cfg, grid=grid, prns=prn_list(n_prn), peaks=peaks, states={k: np.concatenate(v) for k, v in states.items()},
                           rows=used, n_rx=n_rx, n_prn=n_prn, n_dopp=n_dopp, ch=ch)


def n_entries(group):
    """receivers a launch of the group needs for every row to appear once: the period"""
    return len(_entries([r for r in ROWS if r.group == group]))


def outcome(la, r, acq, det, states_after, trace):
    """what a row's predicate looks at: receiver r of launch `la` after the restatement"""
    ch = la.ch
    sl = slice(r * ch, (r + 1) * ch)
    o = SimpleNamespace(row=la.rows[r], cfg=la.cfg, prns=[int(v) for v in la.prns], acq=acq[r], det=det[r], trace=trace[r],
                        sync=states_after["sync"][sl], lock=states_after["lock"][sl], sync0=la.states["sync"][sl], lock0=la.states["lock"][sl])

    def steps(p):
        d, _, _, tau = o.trace["best"][p]
        f = F(la.grid[0] + d * la.grid[1])
        return F(tau), f, F(la.cfg["code_per_hz"]), F(F(la.cfg["lead_blocks"]) * F(0.001))
    o.raw = lambda p: (lambda tau, f, k, t: float(F(tau - F(F(k * f) * t))))(*steps(p))              # the projected phase before its wrap
    o.other_order = lambda p: (lambda tau, f, k, t: float(F(tau - F(F(k * t) * f))))(*steps(p))      # ... with (code_per_hz x T) x f
    return o


# ---- the scenario: weighted_multi_cases.chain_blocks' two receivers through the hybrid grid's restatement ---------------------------
SCN_PRNS = (7, 19, 30, 3, 11, 25, 1, 2)
SCN_GRID = (-5000, 100, 101)                 # dopp_min_hz, dopp_step_hz, n_dopp
SCN_COH, SCN_SEG = 10, 8
SCN_DET = (4, 1)
# measured on the CPU restatement (tests/test_weighted_acq_reference.py measures both again and compares): M 16368 / S of the best
# records of the six present (receiver, PRN) rows at least / of the ten absent rows at most; the threshold 4/1 lies between them
MEASURED = dict(present_min=6.88, absent_max=2.126)
SCN_CH = 5
SCN_EVICT = 1000
SCN_STALE = (3, 2222.0, -1705.0)             # the re-acquisition leg's slot 0: PRN 3 as it is on receiver 1's stream, which receiver 0's lacks
SCN_AGAIN_AT = 1000                          # the leg's second grid starts here
SCN_AGAIN_PRNS = (7, 19, 30, 3)
_memo = {}


def scenario_blocks(r):
    import weighted_multi_cases as M
    if ("blocks", r) not in _memo:
        _memo[("blocks", r)] = M.chain_blocks(r)[0]
    return _memo[("blocks", r)]


def scenario_present(r):
    """receiver r's satellites as PRN indices of SCN_PRNS"""
    import weighted_multi_cases as M
    return [SCN_PRNS.index(sat[0]) for sat in M.CHAIN_SATS[r]]


def scenario_peaks(oracle):
    """the hybrid grid's restatement, 10 x 8 blocks from block 0, on both receivers -> PEAK_DTYPE [2][8][101], once per process"""
    import weighted_hyb_ref as H
    if "peaks" not in _memo:
        _memo["peaks"] = np.stack([H.grid(oracle, scenario_blocks(r)[:SCN_COH * SCN_SEG], 1, SCN_PRNS, SCN_COH, SCN_SEG, *SCN_GRID)[0] for r in range(2)])
    return _memo["peaks"]


def scenario_again_peaks(oracle):
    """... and on receiver 0's blocks 1000 .. 1079 with SCN_AGAIN_PRNS -> PEAK_DTYPE [1][4][101]"""
    import weighted_hyb_ref as H
    if "again" not in _memo:
        _memo["again"] = H.grid(oracle, scenario_blocks(0)[SCN_AGAIN_AT:SCN_AGAIN_AT + SCN_COH * SCN_SEG], 1, SCN_AGAIN_PRNS, SCN_COH, SCN_SEG, *SCN_GRID)
    return _memo["again"]


def scenario_measure(peaks):
    """M 16368 / S of the best records: the least of the present rows', the greatest of the absent rows'"""
    present, absent = [], []
    for r in range(2):
        for p in range(len(SCN_PRNS)):
            _, m, s, _ = Q.best_record(peaks[r, p])
            (present if p in scenario_present(r) else absent).append(Q.ratio(m, s))
    assert len(present) == 6 and len(absent) == 10
    return dict(present_min=round(min(present), 3), absent_max=round(max(absent), 3))


def scenario_cfg(lead_blocks=0, evict_after_blocks=0):
    return Q.make_cfg(SCN_CH, SCN_DET, 0, lead_blocks, WAID_L1CA if lead_blocks else 0.0, evict_after_blocks)


def empty_states(n_ch):
    """every slot empty, every stage fresh"""
    st = {name: np.zeros(n_ch, dt) for name, dt in Q.STATE_DTYPES.items()}
    st["sync"]["loop"]["prn"] = NONE
    return st


def again_states():
    """the re-acquisition leg's start: five empty slots, slot 0 holding SCN_STALE"""
    import weighted_sync_ref as Y
    st = empty_states(SCN_CH)
    st["sync"][0] = Y.handover(*SCN_STALE)[0]
    return st


# ---- the smoke fixture (tests/golden/wacq_smoke.npz) -----------------------------------------------------------------------------------
def smoke_case():
    """group A's rows at the canonical shape -- every clause of the definition but the unprojected phase, once --: the launch's
    arrays and what the restatement makes of them -> the arrays of the fixture"""
    la = launch("A", n_entries("A"))
    after = {k: v.copy() for k, v in la.states.items()}
    acq, det = Q.run(la.cfg, la.prns, la.grid[0], la.grid[1], la.peaks, *[after[k] for k in Q.STATE_DTYPES])
    out = dict(cfg=Q.cfg_record(la.cfg), prns=la.prns, grid=np.array(la.grid, np.int32), peaks=la.peaks, acq=acq, det=det)
    for k in Q.STATE_DTYPES:
        out[k + "_before"], out[k + "_after"] = la.states[k], after[k]
    return out


def write_smoke():
    """(`python tests/weighted_acq_cases.py`) writes the fixture"""
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wacq_smoke.npz")
    np.savez_compressed(path, **smoke_case())
    return path


if __name__ == "__main__":
    print(write_smoke())
