"""The window update and the bit synchroniser's decision of the weighted loops, branch by branch (include/gpsx.h
gpsx_track_loop_weighted and gpsx_track_loop_weighted_sync): a table of states that FORCE every case of the definition, shared by
tests/test_weighted_forced_reference.py (the restatement alone: every row's predicate proves that its branch was taken) and
tests/test_gpu_weighted_forced.py (k_track_wsync against the restatement, byte for byte).

How a case is forced: gpsx_wsync_state_t carries the open window.  A state with win_n = (what ends the window) - 1 and
win_iq = target - r, r being the block's six correlator values for the state's floats (taken from the restatement: a probe run
of weighted_sync_ref.run on the same floats with win_iq = 0), ends a window whose sums are exactly `target` at its first block.
Every |target| and |prev| is <= 2^30, so that every int64 expression of the definition is exact.

Launches (cfg is per launch, so the rows are grouped):
  A   n_coh 4 / 20, one block: the update's branches, the window bookkeeping, the decision's boundaries
  B   the same cfg, two blocks: two window ends in one slot, a search round's twentieth block
  C   n_coh 1 / 1, two blocks: what needs a window at the second block too
The search gains carry a frequency loop (fll_c = 0.1), the lock gains none: LOCKED rows take the fll_c == 0 branch.
Rows that end no window, WAIT rows that stay in WAIT and one bad channel per dozen rows are interleaved, so that the window-end
mask is partial in every wave that holds more than one channel.

k_track_wloop has no open window in its state; wloop_table() holds what its state alone can force (the FLL through prev, the
code-phase wrap through phase and dll_err)."""
import math
from types import SimpleNamespace

import numpy as np

import weighted_loop_cases as S
import weighted_loop_ref as L
import weighted_sync_cases as K
import weighted_sync_ref as Y
import weighted_track_ref as T

F = np.float32
BOUND = 1 << 30
SEARCH, WAIT, LOCKED = Y.SEARCH, Y.WAIT, Y.LOCKED
SPAN = F(16368.0)

GAINS_SEARCH = dict(dll=(1.0, 100.0), pll=(56.0, 1600.0), fll=0.1)
GAINS_LOCK = S.STEADY
SYNC_BITS, RATIO = 1, (5, 4)
DECIDE_AT = 20 * (SYNC_BITS + 1)
# group -> ((n_coh_search, n_coh_lock), blocks per launch)
GROUPS = {"A": ((4, 20), 1), "B": ((4, 20), 2), "C": ((1, 1), 2)}
SEED = 3

# the limits of gpsx_libm::atanf_fdlibm's intervals and the interval AT each limit / just below it
LIMITS = [("2^-29", 2.0 ** -29, "poly", "tiny"), ("7/16", 7 / 16, "hi0", "poly"), ("11/16", 11 / 16, "hi1", "hi0"),
          ("19/16", 19 / 16, "hi2", "hi1"), ("39/16", 39 / 16, "hi3", "hi2"), ("2^25", 2.0 ** 25, "huge", "hi3")]
# (numerator, denominator) whose float quotient is the limit, and a pair below it: one float below wherever QP / IP with integers
# <= 2^30 reaches that float.  Below 2^-29 it does not: n / d >= 2^-30 leaves n = 1 (n = 2 needs d > 2^30), and (float)d moves in
# steps of 64 there, so the nearest Costas quotient below is two floats below the limit.  That holds for QP / IP only: cross and dot
# are products of up to 2^61 and do reach the float below 2^-29 (FLL_BELOW_TINY).
PAIRS = {"2^-29": ((1, 1 << 29), (1, (1 << 29) + 64), 2), "7/16": ((7, 16), (7 * (1 << 21) - 1, 1 << 25), 1),
         "11/16": ((11, 16), (11 * (1 << 20) - 1, 1 << 24), 1), "19/16": ((19, 16), (19 * (1 << 19) - 1, 1 << 23), 1),
         "39/16": ((39, 16), (39 * (1 << 18) - 1, 1 << 22), 1), "2^25": ((1 << 25, 1), ((1 << 25) - 2, 1), 1)}


# prev and (IP, QP) with cross = prev_ip QP - prev_qp IP = 44 739 240 and dot = prev_ip IP + prev_qp QP = 178 956 968 x 2^27 + 1, whose
# float quotient is the float just below 2^-29: (float)dot = 2^54 (1 + 2^-2 + ...) and cross are both exact or rounded once, and the
# predicate counts the floats
FLL_BELOW_TINY = ((178956968, 1), (1 << 27, 1))


def cfg_of(group, use_magnitude=True, spacing=8):
    pair = GROUPS[group][0]
    return Y.make_cfg(pair[0], pair[1], GAINS_SEARCH, GAINS_LOCK, SYNC_BITS, RATIO, use_magnitude, spacing)


_blocks = []


def blocks(n=2):
    """the first n of the two blocks every launch of the table runs on"""
    if not _blocks:
        _blocks.append(K.strong_blocks(2, seed=SEED))
    return _blocks[0][:n]


# ---- what the predicates are made of -------------------------------------------------------------------------------------------
def bits(x):
    return int(np.array([x], "<f4").view("<u4")[0])


def interval(q):
    """the branch of gpsx_libm::atanf_fdlibm a float takes, from its bits"""
    ix = bits(q) & 0x7FFFFFFF
    for top, name in ((0x31000000, "tiny"), (0x3EE00000, "poly"), (0x3F300000, "hi0"), (0x3F980000, "hi1"), (0x401C0000, "hi2"),
                      (0x4C000000, "hi3")):
        if ix < top:
            return name
    return "huge"


def tie(v):
    """None, or which way (float)(int64)v rounds when v lies exactly between two floats: "down" / "up" in magnitude, to even"""
    a = abs(int(v))
    n = a.bit_length()
    if n <= 24:
        return None
    sh = n - 24
    if a & ((1 << sh) - 1) != 1 << (sh - 1):
        return None
    return "up" if (a >> sh) & 1 else "down"


def quotient(num, den):
    return F(L.i64_to_f32(num) / L.i64_to_f32(den))


def ulps_below(q, limit):
    """floats between |q| and the limit (0: q is the limit)"""
    return bits(F(limit)) - (bits(q) & 0x7FFFFFFF)


def dll_terms(t):
    e2, l2 = t[0] * t[0] + t[1] * t[1], t[4] * t[4] + t[5] * t[5]
    return e2 - l2, e2 + l2


def fll_terms(o):
    pi, pq = int(o.st0["loop"]["prev_ip"]), int(o.st0["loop"]["prev_qp"])
    ip, qp = o.row.target[2], o.row.target[3]
    return pi * qp - pq * ip, pi * ip + pq * qp


def fll_on(o):
    return int(o.st0["loop"]["n_updates"]) > 0 and o.cfg["search" if int(o.st0["mode"]) == SEARCH else "lock"]["fll_c"] != 0


def first(o):
    """the record of the window that ended at the launch's first block"""
    r = o.rec[0]
    assert int(r["flags"]) & Y.F_WINDOW and int(r["end_block"]) == 0, (o.row.name, r)
    return r


def decision(o):
    d = [e for e in o.events if e[1] == "decision"]
    assert len(d) == 1, (o.row.name, o.events)
    return SimpleNamespace(block=d[0][0], best=d[0][2], accepted=d[0][3], agreed=d[0][4], e_best=d[0][5], opp=d[0][6], prev=d[0][7])


# ---- the rows ------------------------------------------------------------------------------------------------------------------
class Row(SimpleNamespace):
    pass


def _row(group, name, tags, check, target=None, ends=None, mode=SEARCH, win_n=None, ms_count=5, edge=0, bit_ip=0, phase=None, dll_err=0.0,
         pll_err=0.0, prev=(0, 0), n_updates=0, search_n=0, prev_best_p1=0, e=None, words=None, prn=None, quiet=False):
    """win_n None: what ends the mode's window at the first block (n_coh - 1) when a target is given, 0 otherwise.  e: {candidate:
    energy}.  quiet: base[] is set so that this block adds no energy to e[].  words(st, r): last touches, r the block's correlators."""
    return Row(group=group, name=name, tags=set(tags if isinstance(tags, (list, tuple, set)) else [tags]), check=check,
               target=None if target is None else tuple(int(v) for v in target), ends=(target is not None) if ends is None else ends,
               mode=mode, win_n=win_n, ms_count=ms_count, edge=edge, bit_ip=bit_ip, phase=phase, dll_err=dll_err, pll_err=pll_err, prev=prev,
               n_updates=n_updates, search_n=search_n, prev_best_p1=prev_best_p1, e=e or {}, words=words, prn=prn, quiet=quiet)


def _tie_quads():
    """(IE, QE, IL, QL) whose e2 - l2 / e2 + l2 is an exact tie of the int64 -> float conversion, one per (which, direction); the
    other of the two is no tie where the small search finds such a quadruple.  Scaled by 2^12: the ties sit at 2^48."""
    want = {(w, d): None for w in ("num", "den") for d in ("down", "up")}
    # (26- and 27-bit values: e2 - l2 and e2 + l2 differ by 2 l2, so that one can be a tie -- the bits below the 24th are 10 / 100 --
    # without the other; sums of two squares are never 3 mod 4, which leaves the lone tie of e2 - l2 to the 27-bit ones)
    for ie in list(range(5793, 5797)) + list(range(8193, 8197)):
        for qe in range(0, 12):
            e2 = ie * ie + qe * qe
            for il in range(0, 12):
                for ql in range(0, 3):
                    l2 = il * il + ql * ql
                    tn, td = tie(e2 - l2), tie(e2 + l2)
                    for key, mine, other in ((("num", tn), tn, td), (("den", td), td, tn)):
                        if mine is not None and other is None and want[key] is None:
                            want[key] = (ie << 12, qe << 12, il << 12, ql << 12)
        if all(v is not None for v in want.values()):
            break
    assert all(v is not None for v in want.values()), want
    return want


def _fillers(group, n):
    """rows that end no window at the launch's blocks, a WAIT row that stays in WAIT, and a bad channel: cycled between the others"""
    n_lock = GROUPS[group][0][1]
    kinds = []
    if GROUPS[group][0][0] > GROUPS[group][1]:
        kinds.append(lambda i: _row(group, f"filler_search_{i}", "no_end:search", lambda o: int(o.st["win_n"]) == 1 + GROUPS[group][1], win_n=1, ends=False,
                                    dll_err=0.125, prev=(900, -77), n_updates=4))
    kinds.append(lambda i: _row(group, f"filler_wait_{i}", "no_end:wait", lambda o: int(o.st["mode"]) == WAIT and int(o.st["win_n"]) == 0 and not o.events,
                                mode=WAIT, win_n=0, ms_count=3, edge=11, prev_best_p1=12, ends=False))
    if n_lock > 2 + GROUPS[group][1]:
        kinds.append(lambda i: _row(group, f"filler_locked_{i}", "no_end:locked", lambda o: int(o.st["win_n"]) == 2 + GROUPS[group][1], mode=LOCKED, win_n=2,
                                    ms_count=3, edge=11, bit_ip=-4000, ends=False))
    kinds.append(lambda i: _row(group, f"filler_bad_{i}", "bad", lambda o: o.events == [(0, "bad")] and int(o.st["win_n"]) == 2, win_n=2,
                                prn=(0, 211)[i % 2], ends=False))
    return [kinds[i % len(kinds)](i) for i in range(n)]


def _interleave(rows, group):
    """a filler after every second row, the bad one among them once per three fillers or rarer: at least one bad channel per dozen"""
    out, fill = [], _fillers(group, (len(rows) + 1) // 2)
    for i, r in enumerate(rows):
        out.append(r)
        if i % 2 == 1 or i == len(rows) - 1:
            out.append(fill.pop(0))
    return out


def _set_energy(values):
    """words(): e[] preset (rows of the decision are quiet: the block adds nothing to them)"""
    def words(st, r):
        for c, v in values.items():
            st["e"][0][c] = v
    return words


def _decision_rows():
    rows = []
    A = lambda name, tags, check, **kw: rows.append(_row("A", name, tags, check, **{**dict(search_n=DECIDE_AT - 1, win_n=0, ms_count=5, quiet=True,
                                                                                     ends=False), **kw}))
    big = 1 << 40
    A("decide_three_way_tie", "decision:tie", lambda o: decision(o).best == 3 and decision(o).opp == 5 and not decision(o).accepted,
      e={3: big, 7: big, 15: big, 13: 5}, prev_best_p1=8)
    A("decide_best_low", "decision:best<10", lambda o: (decision(o).best, decision(o).opp, decision(o).accepted) == (4, 1000, True) and
      int(o.st["mode"]) == WAIT and int(o.st["edge"]) == 4, e={4: big, 14: 1000, 0: big - 1}, prev_best_p1=5)
    A("decide_best_high", "decision:best>=10", lambda o: (decision(o).best, decision(o).opp, decision(o).accepted) == (14, 1000, True) and
      int(o.st["edge"]) == 14, e={14: big, 4: 1000, 19: big - 1}, prev_best_p1=15)
    k = (1 << 38) + 12345
    A("decide_ratio_exact", "decision:ratio==", lambda o: decision(o).accepted and decision(o).e_best * RATIO[1] == decision(o).opp * RATIO[0],
      e={9: 5 * k, 19: 4 * k}, prev_best_p1=10)
    A("decide_ratio_one_less", "decision:ratio-1", lambda o: not decision(o).accepted and decision(o).agreed and
      decision(o).e_best * RATIO[1] + RATIO[1] == decision(o).opp * RATIO[0] and int(o.st["mode"]) == SEARCH, e={9: 5 * k - 1, 19: 4 * k}, prev_best_p1=10)
    A("decide_no_predecessor", "decision:prev=0", lambda o: not decision(o).accepted and not decision(o).agreed and decision(o).prev == 0 and
      int(o.st["prev_best_p1"]) == 10, e={9: big, 19: 1}, prev_best_p1=0)
    A("decide_disagree", "decision:disagree", lambda o: not decision(o).accepted and decision(o).prev == 11 and int(o.st["prev_best_p1"]) == 10,
      e={9: big, 19: 1}, prev_best_p1=11)
    # both products leave int64: e[best] * 4 = 3 x 2^63 wraps to -2^63, opp * 5 = 2^63 + 2^61 to -2^63 + 2^61, which is above it:
    # refused, where unbounded integers would accept
    A("decide_products_wrap", "decision:wrap", lambda o: not decision(o).accepted and decision(o).agreed and
      decision(o).e_best * RATIO[1] >= 1 << 63 and decision(o).opp * RATIO[0] >= 1 << 63 and
      decision(o).e_best * RATIO[1] >= decision(o).opp * RATIO[0] and Y._i64(decision(o).e_best * RATIO[1]) < Y._i64(decision(o).opp * RATIO[0]),
      e={2: 3 << 61, 12: 1 << 61}, prev_best_p1=3)
    A("decide_at_4020", "search_n:4020", lambda o: int(o.st0["search_n"]) == 4020 and decision(o).accepted and int(o.st["search_n"]) == 0,
      e={6: big, 16: 7}, prev_best_p1=7, search_n=4020)
    # an accept at a block where a window ends as well: the record is written, then the window, bit_ip and n_updates are cleared
    A("decide_accept_with_window_end", "decision:accept+end", lambda o: decision(o).accepted and tuple(first(o)["w"]["iq"]) == o.row.target and
      int(o.st["loop"]["n_updates"]) == 0 and int(o.st["win_n"]) == 0 and int(o.st["mode"]) == WAIT and
      float(o.st["loop"]["pll_err"]) != 0, e={6: big, 16: 7}, prev_best_p1=7, win_n=None, ends=True,
      target=(300, -40, 9000, 4000, 250, 60), prev=(5000, 100), n_updates=17)
    # the prompt sum and base[] at the ends of int32: p_i + IP_b, p_q + QP_b and di, dq all wrap
    top = (1 << 31) - 1

    def near_ends(st, r):
        for name, v, j in (("p_i", r[2], 0), ("p_q", r[3], 1)):
            st[name][0] = top if v > 0 else -top - 1
            new = Y._i32(int(st[name][0]) + v)
            delta = (100000, 70000)[j]     # (larger than any block's prompt: the difference leaves int32 and comes back as -+delta)
            st["base"][0][6][j] = Y._i32(new - delta) if v > 0 else Y._i32(new + delta)
        st["e"][0][6] = 1 << 20

    def wrapped(o):
        r = o.r[0]
        ok = r[2] != 0 and r[3] != 0
        for name, v, j in (("p_i", r[2], 0), ("p_q", r[3], 1)):
            s0 = int(o.st0[name]) + v
            ok = ok and not -(1 << 31) <= s0 < 1 << 31 and not -(1 << 31) <= Y._i32(s0) - int(o.st0["base"][6][j]) < 1 << 31
        return ok and int(o.st["e"][6]) == (1 << 20) + 100000 ** 2 + 70000 ** 2 and int(o.st["search_n"]) == 31
    A("search_prompt_and_base_wrap", "search:wrap32", wrapped, search_n=30, quiet=False, words=near_ends)
    # e[c] just below 2^63: the sum wraps modulo 2^64
    A("search_energy_wraps", "search:wrap64", lambda o: int(o.st["e"][6]) < 0 and int(o.st0["e"][6]) == (1 << 63) - 1 and o.r[0][2] ** 2 + o.r[0][3] ** 2 > 0,
      search_n=30, quiet=False, words=_set_energy({6: (1 << 63) - 1}))
    A("search_n_19", "search_n:19", lambda o: not o.st["e"].any() and int(o.st["search_n"]) == 20 and tuple(o.st["base"][6]) == (o.r[0][2], o.r[0][3]),
      search_n=19, quiet=False)
    A("search_n_20", "search_n:20", lambda o: int(o.st["e"][6]) == o.r[0][2] ** 2 + o.r[0][3] ** 2 > 0 and int(o.st["search_n"]) == 21, search_n=20, quiet=False)
    rows.append(_row("B", "search_n_19_two_blocks", "search_n:19+20", lambda o: int(o.st["e"][6]) == 0 and int(o.st["e"][7]) ==
                     (o.r[0][2] + o.r[1][2]) ** 2 + (o.r[0][3] + o.r[1][3]) ** 2 > 0 and int(o.st["search_n"]) == 21, search_n=19, win_n=0, ends=False))
    return rows


def _update_rows():
    rows = []
    A = lambda name, tags, check, target, **kw: rows.append(_row("A", name, tags, check, target=target, **kw))
    rec_phase = lambda o: first(o)["w"]["code_phase_fine"]
    d_of = lambda o: o.st["loop"]["dll_err"]
    p_of = lambda o: o.st["loop"]["pll_err"]
    # ---- DLL
    A("dll_no_early_late", "dll:e2+l2=0", lambda o: dll_terms(o.row.target)[1] == 0 and o.row.target[2] != 0 and bits(d_of(o)) == 0 and
      rec_phase(o) == F(4321.375), (0, 0, 7, 3, 0, 0), dll_err=0.375, phase=4321.0)
    A("dll_balanced", "dll:e2=l2", lambda o: dll_terms(o.row.target) == (0, 50) and bits(d_of(o)) == 0 and rec_phase(o) == F(4321.125),
      (3, 4, 100, 5, 4, -3), dll_err=0.125, phase=4321.0)
    A("dll_no_early", "dll:d=-1", lambda o: d_of(o) == F(-1.0), (0, 0, 50, 1, 9, 2), mode=LOCKED, edge=0, ms_count=5)
    A("dll_no_late", "dll:d=+1", lambda o: d_of(o) == F(1.0), (9, 2, 50, 1, 0, 0))
    A("all_six_zero", ["dll:all0", "pll:ip=0,qp=0"], lambda o: bits(d_of(o)) == 0 and bits(p_of(o)) == 0 and
      o.st["loop"]["code_phase_fine"] == o.st0["loop"]["code_phase_fine"] and int(o.st["loop"]["n_updates"]) == 6, (0,) * 6, n_updates=5, prev=(3, 4))
    A("all_six_at_the_bound", "bound:+-2^30", lambda o: dll_terms(o.row.target) == (0, 1 << 62) and fll_on(o) and fll_terms(o) == (-(1 << 60), 1 << 60) and
      p_of(o) == F(L.atanf(F(-1.0)) * L.CYCLES), (BOUND, -BOUND, BOUND, -BOUND, -BOUND, BOUND), prev=(BOUND, 0), n_updates=9, dll_err=-0.5)
    for (which, way), quad in sorted(_tie_quads().items()):
        A(f"dll_tie_{which}_{way}", f"dll:tie:{which}:{way}", lambda o, which=which, way=way: tie(dll_terms(o.row.target)[which == "den"]) == way and
          d_of(o) == quotient(*dll_terms(o.row.target)), (quad[0], quad[1], 77, -31, quad[2], quad[3]), mode=(SEARCH, LOCKED)[way == "up"])
    # ---- the code-phase wrap (search gains 1, 100; T = 0.004: d = +-1 moves the phase by 1.4)
    A("wrap_down_across_0", "wrap:down", lambda o: o.st0["loop"]["code_phase_fine"] < 1 and 16366 < rec_phase(o) < SPAN and d_of(o) == 1, (9, 0, 5, 1, 0, 0), phase=0.5)
    A("wrap_up_across_16368", "wrap:up", lambda o: o.st0["loop"]["code_phase_fine"] > 16367 and 0 < rec_phase(o) < 1 and d_of(o) == -1, (0, 0, 5, 1, 9, 0), phase=16367.5)
    # d = 0 makes the correction -dll_c1 * dll_err = -dll_err, exactly
    A("wrap_exactly_16368", "wrap:==16368", lambda o: F(o.st0["loop"]["code_phase_fine"] + F(1.0)) == SPAN and bits(rec_phase(o)) == 0, (3, 4, 5, 1, 4, 3),
      phase=16367.0, dll_err=1.0)
    A("wrap_phase_equals_correction", "wrap:==0", lambda o: bits(rec_phase(o)) == 0 and bits(d_of(o)) == 0, (3, 4, 5, 1, 4, 3), phase=2.5, dll_err=-2.5)
    rows.append(_row("C", "wrap_lands_on_16368", "wrap:lands", lambda o: bits(first(o)["w"]["code_phase_fine"]) == bits(SPAN) and
                     T.tau_of(first(o)["w"]["code_phase_fine"]) == 0 and int(o.rec[1]["flags"]) & Y.F_WINDOW and int(o.rec[1]["end_block"]) == 1 and
                     not any(e[1] == "bad" for e in o.events) and np.array_equal(o.rec[1]["w"]["iq"], o.tau0), target=(9, 0, 5, 1, 0, 0),
                     phase=F(1.3996999), win_n=3))
    # ---- Costas PLL
    A("pll_ip0_qp_positive", "pll:ip=0,qp>0", lambda o: p_of(o) == F(0.25), (5, 5, 0, 7, 5, 4), mode=LOCKED)
    A("pll_ip0_qp_negative", "pll:ip=0,qp<0", lambda o: p_of(o) == F(-0.25), (5, 5, 0, -7, 5, 4))
    A("pll_ip0_qp0", "pll:ip=0,qp=0", lambda o: bits(p_of(o)) == 0, (5, 5, 0, 0, 5, 4), pll_err=0.0625)
    A("pll_qp0_ip_positive", "pll:qp=0,ip>0", lambda o: bits(p_of(o)) == 0, (5, 5, 70, 0, 5, 4), pll_err=0.0625, mode=LOCKED)
    A("pll_qp0_ip_negative", "pll:qp=0,ip<0", lambda o: bits(p_of(o)) == 0x80000000, (5, 5, -70, 0, 5, 4), pll_err=0.0625)
    for name, ip, qp in (("pp", 12345, 12345), ("pn", 12345, -12345), ("np", -BOUND, BOUND), ("nn", -3, -3)):
        A(f"pll_diagonal_{name}", "pll:qp=+-ip", lambda o, s=(1 if (ip > 0) == (qp > 0) else -1): p_of(o) == F(L.atanf(F(s)) * L.CYCLES) and
          quotient(o.row.target[3], o.row.target[2]) == F(s) and interval(F(s)) == "hi1", (5, 5, ip, qp, 5, 4), mode=(SEARCH, LOCKED)[ip > 0])
    i = 0
    for lim, value, at, below in LIMITS:
        for where, (n, d), want, away in (("at", PAIRS[lim][0], at, 0), ("below", PAIRS[lim][1], below, PAIRS[lim][2])):
            # (both signs of the quotient; QP and IP take turns in carrying them from one (limit, side) to the next)
            for sign, sn, sd in ((("+", 1, 1), ("-", -1, 1)), (("-", 1, -1), ("+", -1, -1)))[(i // 2) % 2]:
                i += 1

                def check(o, value=value, want=want, away=away, sign=sign):
                    q = quotient(o.row.target[3], o.row.target[2])
                    return interval(q) == want and ulps_below(q, value) == away and (q < 0) == (sign == "-") and \
                        (away > 0 or abs(float(q)) == value) and p_of(o) == F(L.atanf(q) * L.CYCLES)
                A(f"pll_{lim}_{where}_{sign}{i}", f"pll:{lim}:{where}:{sign}", check, (5, 5, sd * d, sn * n, 5, 4), mode=(SEARCH, LOCKED)[i % 3 == 0])
    A("pll_operand_rounds", "pll:rounds", lambda o: int(F(o.row.target[3])) != o.row.target[3] and int(F(o.row.target[2])) != o.row.target[2] and
      p_of(o) == F(L.atanf(F(F((1 << 24) + 4) / F((1 << 25) + 8))) * L.CYCLES), (5, 5, (1 << 25) + 6, (1 << 24) + 3, 5, 4))
    # ---- FLL (SEARCH: fll_c = 0.1).  prev = (2^k, 0) makes cross = 2^k QP, dot = 2^k IP: the Costas pairs again, as 64-bit products;
    # the float below 2^-29, which those pairs miss, has a prev and a prompt of its own
    A("fll_first_window", "fll:n_updates=0", lambda o: not fll_on(o) and fll_terms(o)[0] != 0 and int(o.st["loop"]["n_updates"]) == 1, (5, 5, 900, 40, 5, 4),
      prev=(100, 900), n_updates=0)
    A("fll_no_previous_prompt", "fll:dot=0:prev=0", lambda o: fll_on(o) and fll_terms(o) == (0, 0), (5, 5, 900, 40, 5, 4), prev=(0, 0), n_updates=3)
    A("fll_quarter_turn", "fll:dot=0:perp", lambda o: fll_on(o) and fll_terms(o)[1] == 0 and fll_terms(o)[0] != 0, (5, 5, 900, 40, 5, 4), prev=(40, -900), n_updates=3)
    A("fll_half_turn", "fll:cross=0,dot<0", lambda o: fll_on(o) and fll_terms(o)[0] == 0 and fll_terms(o)[1] < 0, (5, 5, 900, 40, 5, 4), prev=(-900, -40), n_updates=3)
    A("fll_off_in_locked", "fll:fll_c=0", lambda o: not fll_on(o) and int(o.st0["loop"]["n_updates"]) > 0 and fll_terms(o)[0] != 0, (5, 5, 900, 40, 5, 4),
      prev=(100, 900), n_updates=3, mode=LOCKED)
    for lim, value, at, below in LIMITS:
        for where, (n, d), want, away in (("at", PAIRS[lim][0], at, 0), ("below", PAIRS[lim][1], below, PAIRS[lim][2])):
            for sign, sn in (("+", 1), ("-", -1)):
                i += 1
                shift = 30 if max(n, d) < 1 << 26 else 4
                prev, t = (1 << shift, 0), (5, 5, d, sn * n, 5, 4)
                if (lim, where) == ("2^-29", "below"):
                    (pi, pq), (ip, qp) = FLL_BELOW_TINY
                    prev, t, away = (pi, sn * pq), (5, 5, ip, sn * qp, 5, 4), 1

                def check(o, value=value, want=want, away=away, sign=sign):
                    q = quotient(*fll_terms(o))
                    return fll_on(o) and interval(q) == want and ulps_below(q, value) == away and (q < 0) == (sign == "-") and max(map(abs, fll_terms(o))) >= 1 << 29
                A(f"fll_{lim}_{where}_{sign}", f"fll:{lim}:{where}:{sign}", check, t, prev=prev, n_updates=2 + i)
    for which in ("cross", "dot"):
        for way, odd in (("down", 1), ("up", 3)):
            t = (5, 5, 1000, (1 << 24) + odd, 5, 4) if which == "cross" else (5, 5, (1 << 24) + odd, 1000, 5, 4)
            A(f"fll_tie_{which}_{way}", f"fll:tie:{which}:{way}", lambda o, which=which, way=way: fll_on(o) and
              tie(fll_terms(o)[which == "dot"]) == way and abs(fll_terms(o)[which == "dot"]) > 1 << 44, t, prev=(1 << 20, 0), n_updates=1)
    rows.append(_row("C", "n_updates_wraps", "n_updates:0xFFFFFFFF", lambda o: int(o.st0["loop"]["n_updates"]) == 0xFFFFFFFF and fll_terms(o)[0] != 0 and
                     int(o.st["loop"]["n_updates"]) == 1 and int(o.rec[1]["flags"]) & Y.F_WINDOW, target=(5, 5, 900, 40, 5, 4), prev=(100, 900),
                     n_updates=0xFFFFFFFF, win_n=0))
    return rows


def _window_rows():
    rows = []
    t = (40, -30, 2000, 90, 35, 33)
    flags = lambda o, u=0: int(o.rec[u]["flags"])
    WL, BIT = Y.F_WINDOW | Y.F_LOCKED, Y.F_BIT
    rows.append(_row("A", "locked_ends_by_length", "window:length", lambda o: flags(o) == WL and int(o.st["bit_ip"]) == 777 + 2000, target=t, mode=LOCKED,
                     win_n=19, edge=0, ms_count=5, bit_ip=777))
    rows.append(_row("A", "locked_ends_by_edge", "window:edge", lambda o: flags(o) == WL | BIT and int(o.st0["win_n"]) == 0 and
                     int(first(o)["bit_ip"]) == 777 + 2000 and int(o.st["bit_ip"]) == 0, target=t, mode=LOCKED, win_n=0, edge=0, ms_count=19, bit_ip=777))
    rows.append(_row("A", "locked_ends_by_both", "window:both", lambda o: flags(o) == WL | BIT and int(o.st0["win_n"]) == 19, target=t, mode=LOCKED,
                     win_n=19, edge=8, ms_count=7, bit_ip=-5))
    rows.append(_row("A", "bit_ip_wraps", "window:bit_ip_wraps", lambda o: int(o.st0["bit_ip"]) + o.row.target[2] >= 1 << 31 and
                     int(first(o)["bit_ip"]) == int(o.st0["bit_ip"]) + o.row.target[2] - (1 << 32), target=t, mode=LOCKED, win_n=4, edge=8, ms_count=7,
                     bit_ip=(1 << 31) - 5))
    rows.append(_row("C", "window_of_21", "window:win_n=20", lambda o: int(o.st0["win_n"]) == 20 and flags(o) == Y.F_WINDOW and flags(o, 1) == Y.F_WINDOW,
                     target=t, win_n=20, dll_err=0.25, prev=(700, 20), n_updates=2))
    rows.append(_row("C", "wait_locks_and_ends", "window:wait->end", lambda o: (0, "locked") in o.events and flags(o) == WL and flags(o, 1) == WL and
                     int(o.st["mode"]) == LOCKED, target=t, mode=WAIT, win_n=0, edge=7, ms_count=7, prev_best_p1=8))
    rows.append(_row("B", "two_ends_in_one_slot", "window:two_in_a_slot", lambda o: int(o.rec[0]["end_block"]) == 1 and flags(o) == WL | BIT and
                     int(o.st["loop"]["n_updates"]) == 5 and int(o.st["win_n"]) == 0, mode=LOCKED, win_n=19, edge=9, ms_count=7, n_updates=3, ends=True))
    return rows


_tables = {}


def table(group):
    """the group's rows in launch order"""
    if group not in _tables:
        rows = [r for r in _update_rows() + _window_rows() + _decision_rows() if r.group == group]
        _tables[group] = _interleave(rows, group)
        assert len({r.name for r in _tables[group]}) == len(_tables[group])
    return _tables[group]


# what the table must hold (tests/test_weighted_forced_reference.py asserts that every tag is some row's)
REQUIRED = (["dll:e2+l2=0", "dll:e2=l2", "dll:d=-1", "dll:d=+1", "dll:all0", "bound:+-2^30", "wrap:down", "wrap:up", "wrap:==16368", "wrap:==0",
             "wrap:lands", "pll:ip=0,qp>0", "pll:ip=0,qp<0", "pll:ip=0,qp=0", "pll:qp=0,ip>0", "pll:qp=0,ip<0", "pll:qp=+-ip", "pll:rounds",
             "fll:n_updates=0", "fll:dot=0:prev=0", "fll:dot=0:perp", "fll:cross=0,dot<0", "fll:fll_c=0", "n_updates:0xFFFFFFFF",
             "window:length", "window:edge", "window:both", "window:win_n=20", "window:bit_ip_wraps", "window:wait->end", "window:two_in_a_slot",
             "decision:tie", "decision:best<10", "decision:best>=10", "decision:ratio==", "decision:ratio-1", "decision:prev=0",
             "decision:disagree", "decision:wrap", "decision:accept+end", "search_n:4020", "search_n:19", "search_n:20", "search_n:19+20",
             "search:wrap32", "search:wrap64", "no_end:search", "no_end:wait", "no_end:locked", "bad"]
            + [f"dll:tie:{w}:{d}" for w in ("num", "den") for d in ("down", "up")] + [f"fll:tie:{w}:{d}" for w in ("cross", "dot") for d in ("down", "up")]
            + [f"{loop}:{lim[0]}:{where}:{sign}" for loop in ("pll", "fll") for lim in LIMITS for where in ("at", "below") for sign in "+-"])


# ---- states ----------------------------------------------------------------------------------------------------------------------
_probe = {}


def correlators(oracle, st, cfg, n):
    """r: the six correlator values of blocks 0 .. n - 1 for the state's floats and accumulator, from the restatement (one run on
    a LOCKED state with win_iq = 0 and no window end in reach, block by block)"""
    lp = st["loop"][0]
    key = (int(lp["prn"]), bits(lp["code_phase_fine"]), bits(lp["if_freq_offset_hz"]), int(lp["if_freq_accum"]), cfg["use_magnitude"], cfg["spacing"], n)
    if key not in _probe:
        probe_cfg = Y.make_cfg(20, 20, GAINS_LOCK, GAINS_LOCK, 1, RATIO, cfg["use_magnitude"], cfg["spacing"])
        ps = Y.handover(lp["prn"], lp["code_phase_fine"], lp["if_freq_offset_hz"], lp["if_freq_accum"])
        ps["mode"], ps["edge"], ps["ms_count"] = LOCKED, 10, 10
        out, seen = [], np.zeros(6, np.int64)
        for b in range(n):
            rec = Y.run(oracle, blocks()[b:b + 1], ps, probe_cfg)
            assert not rec["flags"].any()
            now = ps["win_iq"][0].astype(np.int64)
            out.append(tuple(int(v) for v in now - seen))
            seen = now
        _probe[key] = out
    return _probe[key]


def state_of(oracle, row, index, cfg, lead=1):
    """the row's state.  lead: blocks the window still has to see before it ends at `target` (1: it ends at the launch's first
    block; 2, for the table cut differently: win_n and the counters one block earlier, win_iq = target - r_0 - r_1)"""
    prn, fd, delay = K.STRONG[index % 3][:3]
    st = Y.handover(prn if row.prn is None else row.prn, delay if row.phase is None else row.phase, fd,
                    0 if index % 5 == 0 else (index * 0x9E3779B1) & 0xFFFFFFFF)
    lp = st["loop"]
    lp["dll_err"], lp["pll_err"], lp["prev_ip"], lp["prev_qp"], lp["n_updates"] = row.dll_err, row.pll_err, row.prev[0], row.prev[1], row.n_updates
    n_coh = cfg["n_coh_lock" if row.mode != SEARCH else "n_coh_search"]
    win_n = row.win_n if row.win_n is not None else (n_coh - 1 if row.target is not None else 0)
    st["mode"], st["win_n"], st["ms_count"], st["edge"], st["bit_ip"] = row.mode, win_n - (lead - 1), (row.ms_count - (lead - 1)) % 20, row.edge, row.bit_ip
    st["search_n"], st["prev_best_p1"] = row.search_n, row.prev_best_p1
    for c, v in row.e.items():
        st["e"][0][c] = v
    valid = 1 <= int(lp["prn"][0]) <= 210
    r = correlators(oracle, st, cfg, max(lead, GROUPS[row.group][1])) if valid else [(0,) * 6] * 2
    if row.target is not None:
        st["win_iq"] = [Y._i32(t - sum(x[k] for x in r[:lead])) for k, t in enumerate(row.target)]
    elif win_n:
        st["win_iq"] = [(index + 1) * v for v in (11, -7, 900, 301, 10, 3)]
    if row.quiet:          # the block's prompt lands on base[ms_count + 1]: no energy
        st["base"][0][(int(st["ms_count"][0]) + 1) % 20] = (r[0][2], r[0][3])
    if row.words is not None:
        row.words(st, r[0])
    return st, r


def group_states(oracle, group, use_magnitude=True, spacing=8):
    """(rows, states [n_rows], correlators per row, cfg)"""
    cfg = cfg_of(group, use_magnitude, spacing)
    rows = table(group)
    built = [state_of(oracle, row, i, cfg) for i, row in enumerate(rows)]
    return rows, np.concatenate([b[0] for b in built]), [b[1] for b in built], cfg


_restated = {}


def restated(oracle, group):
    """the group on the restatement, once per process: (rows, states before, cfg, records [slots][n_rows], states after, outcomes).
    Nothing of it is modified by the tests."""
    if group not in _restated:
        rows, st0, r, cfg = group_states(oracle, group)
        n = GROUPS[group][1]
        after, events = st0.copy(), []
        rec = Y.run(oracle, blocks(n), after, cfg, events=events)
        tau0 = {}
        outcomes = []
        for i, row in enumerate(rows):
            o = SimpleNamespace(row=row, st0=st0[i], st=after[i], rec=rec[:, i], events=[e[1:] for e in events if e[0] == i], cfg=cfg, r=r[i], tau0=None)
            if row.name == "wrap_lands_on_16368":      # what the second block gives at tau = 0, from the open-loop restatement
                trk = np.zeros(1, L.TRK_DTYPE)
                trk["prn"], trk["code_phase_fine"], trk["if_freq_offset_hz"], trk["if_freq_accum"] = (st0[i]["loop"]["prn"], 0.0, rec[0, i]["w"]["if_freq_offset_hz"],
                                                                                                      rec[0, i]["w"]["if_freq_accum"])
                o.tau0 = T.track(oracle, blocks()[1:2], trk, cfg["use_magnitude"], cfg["spacing"])[0][0, 0]
            outcomes.append(o)
        _restated[group] = (rows, st0, cfg, rec, after, outcomes)
    return _restated[group]


def tiled(n_ch, n_rows, cpw):
    """row index of every channel: the table repeated with the smallest period >= n_rows that is coprime to cpw, so that the
    channels of a wave sit on different rows and the rows move through the lanes"""
    period = n_rows
    while math.gcd(period, cpw) != 1:
        period += 1
    return (np.arange(n_ch) % period) % n_rows


def cut_rows(group="A"):
    """rows of a one-block group that can be cut one block earlier: a window with at least one block in it that the launch's
    first block ends at `target`, and nothing else due at either block"""
    assert GROUPS[group][1] == 1
    out = []
    for i, row in enumerate(table(group)):
        n_coh = GROUPS[group][0][1 if row.mode == LOCKED else 0]
        win_n = row.win_n if row.win_n is not None else n_coh - 1
        if row.target is None or row.mode == WAIT or win_n < 1 or row.search_n or (row.mode == LOCKED and (row.ms_count - row.edge) % 20 == 0):
            continue
        out.append(i)
    return out


# ---- k_track_wloop: what its state alone can force -------------------------------------------------------------------------------
WLOOP_N_COH, WLOOP_BLOCKS = 1, 2
WLOOP_GAINS = dict(dll=(1.0, 300.0), pll=(4.0, 3000.0), fll=0.5)
# (name, c, s): prev = (c IP - s QP, c QP + s IP) gives dot = c N, cross = -s N with N = IP^2 + QP^2, so cross / dot = -s / c
ROTATIONS = ([("dot=0", 0, 1), ("dot=0,cross>0", 0, -1), ("half_turn", -1, 0), ("none", 1, 0)] +
             [(f"{lim}:{side}:{sign}", c, -sg * s) for lim, pairs in (("7/16", ((6, 16), (8, 16))), ("11/16", ((10, 16), (12, 16))),
                                                                      ("19/16", ((18, 16), (20, 16))), ("39/16", ((38, 16), (40, 16))))
              for side, (s, c) in zip(("below", "above"), pairs) for sign, sg in (("+", 1), ("-", -1))])
WLOOP_INTERVAL = {"7/16": ("poly", "hi0"), "11/16": ("hi0", "hi1"), "19/16": ("hi1", "hi2"), "39/16": ("hi2", "hi3")}
# (name, phase, dll_err): with d in [-1, 1], gains (1, 300) and T = 0.001 the correction is 1.3 d - dll_err: a dll_err of +-3
# carries a phase within 1.5 of an end across it whatever d is
WLOOP_WRAPS = [("down", 0.75, -3.0), ("up", 16367.25, 3.0)]


def wloop_cfg():
    return L.make_cfg(WLOOP_N_COH, True, 8, WLOOP_GAINS["dll"], WLOOP_GAINS["pll"], WLOOP_GAINS["fll"])


_wloop = {}


def wloop_table(oracle):
    """once per process: (names, states before [n], records wanted [2][n], states wanted, per row what the first window's FLL and
    wrap saw).  Row j tracks one of the strong stream's satellites; its first window's prompt comes from the restatement, and
    prev is that prompt rotated, so that the FIRST window's FLL sees the chosen cross / dot."""
    if not _wloop:
        cfg = wloop_cfg()
        blk = blocks(WLOOP_BLOCKS)
        kinds = [("fll:" + n, c, s, None) for n, c, s in ROTATIONS] + [("fll:prev=0", None, None, None), ("fll:n_updates=0xFFFFFFFF", 3, 1, None)] + \
                [("wrap:" + n, 1, 0, (ph, de)) for n, ph, de in WLOOP_WRAPS]
        st0 = np.zeros(len(kinds), L.STATE_DTYPE)
        for j in range(len(kinds)):
            prn, fd, delay = K.STRONG[j % 3][:3]
            st0[j:j + 1] = L.handover(prn, delay, fd, 0 if j % 5 == 0 else (j * 0x9E3779B1) & 0xFFFFFFFF)
        for j, (name, c, s, wrap) in enumerate(kinds):
            if wrap:
                st0["code_phase_fine"][j], st0["dll_err"][j] = wrap
        probe = st0.copy()
        first_window = L.run(oracle, blk[:WLOOP_N_COH], probe, cfg)["iq"][0]
        facts = []
        for j, (name, c, s, wrap) in enumerate(kinds):
            ip, qp = int(first_window[j, 2]), int(first_window[j, 3])
            st0["n_updates"][j] = 0xFFFFFFFF if "0xFFFFFFFF" in name else 3 + j
            if c is not None:
                st0["prev_ip"][j], st0["prev_qp"][j] = c * ip - s * qp, c * qp + s * ip
            st0["pll_err"][j] = 0.03125 * (j % 5 - 2)
        want_st = st0.copy()
        want = L.run(oracle, blk, want_st, cfg)
        for j, (name, c, s, wrap) in enumerate(kinds):
            ip, qp = int(want["iq"][0, j, 2]), int(want["iq"][0, j, 3])
            pi, pq = int(st0["prev_ip"][j]), int(st0["prev_qp"][j])
            cross, dot = pi * qp - pq * ip, pi * ip + pq * qp
            facts.append(SimpleNamespace(name=name, c=c, s=s, n=ip * ip + qp * qp, cross=cross, dot=dot, q=None if dot == 0 else quotient(cross, dot),
                                         phase0=st0["code_phase_fine"][j], phase1=want["code_phase_fine"][0, j], d=float(want_st["dll_err"][j])))
        _wloop["t"] = ([k[0] for k in kinds], st0, want, want_st, facts)
    return _wloop["t"]
