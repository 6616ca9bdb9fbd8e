"""The weighted grid in a window around each prediction, clause by clause (include/gpsx.h gpsx_acq_window_weighted): a table of
fabricated prediction records that reach every clause of the definition, shared by tests/test_weighted_win_reference.py (the
restatement alone: every row's predicate proves its clause on the restatement's own integers) and tests/test_gpu_weighted_win.py
(k_acq_win against the restatement, byte for byte), seeded random launches at the shapes the kernel takes its paths at, the
two-receiver scenario with what was measured on it, and the smoke fixture.

A row is ONE (receiver, PRN index) unit.  cfg, the lattice, the weights, the stride and the blocks are per launch, so the rows are
grouped; a group's rows fill its launch's receivers N_PRN at a time, in the table's order:
  E   1 x 1 blocks, W 7, D 1, guard 0, bins -1000 + 500 d Hz (5 of them), both bits, random blocks, stride 1 (the searches overlap
      nothing and leave nothing out): selection, the centre's rounding, the seam, the lattice's ends
  G   2 x 2 blocks, W 8, D 0, guard W - 1 = 7, ONE bin at 250 Hz, sign only, stride 0 (every receiver reads the same blocks)
  D   1 x 1 blocks, W 8, D 32, guard 3, bins -5000 + 100 d Hz (101 of them), stride 3 (blocks are left out between the searches)
  T   20 x 1 blocks matched to PRN 7 at phase T_TAU and 250 Hz, the top of the correlation's range: I = 3 x 16352 x 20; W 128, D 0
  Q   1 x 1 blocks, sign only, W 2047, D 0, guard 0: two equal maxima in one window (seeds found by tie_search on the CPU)"""
from types import SimpleNamespace

import numpy as np

import weighted_coh_ref as R
import weighted_win_ref as V

SAMPLES = V.SAMPLES
N_PRN = 3
SEL = V.PREDICTED | V.VISIBLE | 1            # what gpsx_wpred writes for a satellite to be searched: HAVE_EPH | PREDICTED | VISIBLE
NAN, INF = float("nan"), float("inf")
T_PRN, T_TAU, T_HZ = 7, 5000, 250
# (seed, c): random sign-only blocks whose window of W = 2047 around c holds its maximum twice -- Q_SEAM's pair straddles the seam
# (one tau above 14321, one below 2048, so that the smallest tau is NOT the first j), Q_FLAT's does not.  tie_search finds them.
Q_PRN = 19
Q_SEAM = (320, 0)
Q_FLAT = (0, 8000)

GROUPS = {
    "E": SimpleNamespace(cfg=V.make_cfg(1, 1, 7, 1, 0), grid=(-1000, 500, 5), mag=True, stride=1, blocks="random"),
    "G": SimpleNamespace(cfg=V.make_cfg(2, 2, 8, 0, 7), grid=(250, 500, 1), mag=False, stride=0, blocks="random"),
    "D": SimpleNamespace(cfg=V.make_cfg(1, 1, 8, 32, 3), grid=(-5000, 100, 101), mag=True, stride=3, blocks="random"),
    "T": SimpleNamespace(cfg=V.make_cfg(20, 1, 128, 0, 32), grid=(T_HZ, 25, 1), mag=True, stride=0, blocks="matched"),
    "Q": SimpleNamespace(cfg=V.make_cfg(1, 1, 2047, 0, 0), grid=(0, 500, 1), mag=False, stride=1, blocks="tie"),
}


def prn_list(n_prn):
    """n_prn distinct PRN numbers of 1 .. 210 (11 is coprime to 210)"""
    return np.array([(11 * i) % 210 + 1 for i in range(n_prn)], np.uint8)


def random_blocks(seed, n):
    return np.random.default_rng(7000 + seed).integers(0, 256, (n, R.BYTES_2BIT), dtype=np.uint8)


def matched_blocks(oracle, prn, freq_hz, n, tau):
    """weighted_coh_ref.code_matched_blocks with the replica at phase tau: I(tau) = 3 x 16352 x n"""
    chip = np.roll(np.repeat(oracle.ca_code(prn).astype(np.uint8), 16), tau)
    step32 = (oracle.nco_step(freq_hz) * 32) & 0xFFFFFFFF
    out = []
    for b in range(n):
        ci, _, _ = oracle.wipeoff(np.zeros(2046, np.uint8), freq_hz, (b * 511 * step32) & 0xFFFFFFFF)
        carrier = np.unpackbits(ci.view(np.uint8), bitorder="little")[:SAMPLES]
        out.append(R._pack2((1 - chip) ^ carrier, np.ones(SAMPLES, np.uint8)))
    return np.stack(out)


def tie_search(oracle, c, want_seam, seeds=range(400)):
    """the first seed whose random block has two equal maxima of E in the window of W = 2047 around c (PRN Q_PRN, 4092000 Hz, sign
    only); want_seam: one of them above the seam and one below"""
    taus = V.window(c, 2047)
    for seed in seeds:
        e = V.energy(oracle, random_blocks(seed, 1), 0, 1, 1, Q_PRN, 4092000, False)[taus]
        at = taus[e == e.max()]
        if len(at) >= 2 and (not want_seam or (at.min() < 2048 and at.max() > 14320)) and (want_seam or at.max() - at.min() < 4095):
            return seed
    return None


class Row(SimpleNamespace):
    pass


def _rows():
    rows = []

    def add(group, name, check, code_phase=100.0, f_hz=0.0, flags=SEL, prn=None):
        rows.append(Row(group=group, name=name, check=check, code_phase=code_phase, f_hz=f_hz, flags=flags, prn=prn))

    zero = lambda o: not o.peaks.tobytes().strip(b"\0")                                                  # noqa: E731
    only = lambda o, f: int(o.rep["flags"]) == f and (o.rep["first_bin"], o.rep["n_bins"], o.rep["centre"]) == (0, 0, 0) and zero(o)   # noqa: E731
    centre = lambda o, c: int(o.rep["flags"]) & V.SEARCHED and int(o.rep["centre"]) == c and o.phases_inside()   # noqa: E731
    bins = lambda o, flags, d0, n: (int(o.rep["flags"]), int(o.rep["first_bin"]), int(o.rep["n_bins"])) == (flags, d0, n) and o.outside_zero()  # noqa: E731
    # -- selection
    add("E", "skipped_without_predicted", lambda o: only(o, V.SKIPPED), flags=V.VISIBLE | 1)
    add("E", "skipped_without_visible", lambda o: only(o, V.SKIPPED), flags=V.PREDICTED | 1)
    add("E", "skipped_by_tracked", lambda o: only(o, V.SKIPPED), flags=SEL | V.TRACKED)
    add("E", "skipped_by_assigned", lambda o: only(o, V.SKIPPED), flags=SEL | V.ASSIGNED)
    add("E", "bits_outside_both_masks_do_not_matter", lambda o: int(o.rep["flags"]) == V.SEARCHED, flags=SEL | 8 | 64)
    add("E", "bad_nan_code_phase", lambda o: only(o, V.BAD), code_phase=NAN)
    add("E", "bad_infinite_code_phase", lambda o: only(o, V.BAD), code_phase=INF)
    add("E", "bad_code_phase_below_zero", lambda o: only(o, V.BAD), code_phase=-0.5)
    add("E", "bad_code_phase_above_the_span", lambda o: only(o, V.BAD), code_phase=16368.5)
    add("E", "bad_nan_f_hz", lambda o: only(o, V.BAD), f_hz=NAN)
    add("E", "bad_infinite_f_hz", lambda o: only(o, V.BAD), f_hz=-INF)
    add("E", "skipped_comes_before_bad", lambda o: only(o, V.SKIPPED), code_phase=NAN, flags=SEL | V.TRACKED)
    # -- the centre
    add("E", "code_phase_on_the_span_is_zero", lambda o: centre(o, 0), code_phase=16368.0)
    add("E", "code_phase_16367_5_rounds_to_even_and_wraps", lambda o: centre(o, 0), code_phase=16367.5)
    add("E", "code_phase_0_5_rounds_to_even", lambda o: centre(o, 0), code_phase=0.5)
    add("E", "code_phase_1_5_rounds_to_even", lambda o: centre(o, 2), code_phase=1.5)
    add("E", "code_phase_2_5_rounds_to_even", lambda o: centre(o, 2), code_phase=2.5)
    # -- the seam
    add("E", "window_across_the_seam_c_0", lambda o: centre(o, 0) and o.taus.min() == 0 and o.taus.max() == 16367, code_phase=0.0)
    add("E", "window_touches_the_seam_c_w_minus_1", lambda o: centre(o, 6) and o.taus.max() == 16367 and o.taus[0] == 16367, code_phase=6.0)
    add("E", "window_ends_at_the_seam_c_span_minus_w", lambda o: centre(o, 16361) and o.taus[-1] == 0, code_phase=16361.0)
    add("E", "window_across_the_seam_c_16367", lambda o: centre(o, 16367) and o.taus[-1] == 6, code_phase=16367.0)
    # -- the bins (D = 1, bins 0 .. 4 at -1000 + 500 d)
    add("E", "dc_minus_one_clipped_to_bin_0", lambda o: bins(o, V.SEARCHED | V.CLIPPED, 0, 1), f_hz=-1500.0)
    add("E", "dc_zero_clipped", lambda o: bins(o, V.SEARCHED | V.CLIPPED, 0, 2), f_hz=-1000.0)
    add("E", "dc_inside", lambda o: bins(o, V.SEARCHED, 1, 3), f_hz=0.0)
    add("E", "dc_last_clipped", lambda o: bins(o, V.SEARCHED | V.CLIPPED, 3, 2), f_hz=1000.0)
    add("E", "dc_n_dopp_clipped_to_the_last", lambda o: bins(o, V.SEARCHED | V.CLIPPED, 4, 1), f_hz=1500.0)
    add("E", "off_lattice_below", lambda o: only(o, V.OFF_LATTICE), f_hz=-2000.0)
    add("E", "off_lattice_above", lambda o: only(o, V.OFF_LATTICE), f_hz=2000.0)
    add("E", "x_just_over_2_30", lambda o: only(o, V.OFF_LATTICE) and o.x > 2.0 ** 30, f_hz=-1000.0 + 500.0 * (2.0 ** 30 + 1))
    add("E", "x_just_under_minus_2_30", lambda o: only(o, V.OFF_LATTICE) and -2.0 ** 30 < o.x < -2.0 ** 30 + 2, f_hz=-1000.0 - 500.0 * (2.0 ** 30 - 1))
    # (|x| == 2^30 passes the first clause and is rounded; with n_dopp <= 2^20 and D <= 32 its bins are off the lattice all the same, so no
    #  call can tell `>` from `>=`: weighted_win_ref.select is held to `>` in test_weighted_win_reference.py on a lattice no call accepts)
    add("E", "x_on_2_30_is_off_the_lattice_too", lambda o: only(o, V.OFF_LATTICE) and o.x == 2.0 ** 30, f_hz=-1000.0 + 500.0 * 2.0 ** 30)
    add("E", "x_at_0_5_rounds_to_even", lambda o: o.x == 0.5 and bins(o, V.SEARCHED | V.CLIPPED, 0, 2), f_hz=-750.0)
    add("E", "x_at_1_5_rounds_to_even", lambda o: o.x == 1.5 and bins(o, V.SEARCHED, 1, 3), f_hz=-250.0)
    # -- the guard and the far sum
    add("E", "guard_0_leaves_out_the_peak_alone", lambda o: o.far_count(1) == 14 and o.sum_from_e(1), f_hz=0.0, code_phase=9000.0)
    add("G", "guard_w_minus_1", lambda o: int(o.rep["flags"]) == V.SEARCHED and 2 <= o.far_count(0) <= 9 and o.sum_from_e(0), code_phase=4000.0, f_hz=250.0)
    add("G", "n_dopp_1_and_d_0", lambda o: bins(o, V.SEARCHED, 0, 1) and o.sum_from_e(0), code_phase=12.25, f_hz=499.0)
    add("G", "n_dopp_1_off_by_one_bin", lambda o: only(o, V.OFF_LATTICE), code_phase=12.25, f_hz=750.1)
    add("G", "stride_0_same_blocks_same_record", lambda o: int(o.rep["flags"]) == V.SEARCHED and o.peaks.tobytes() == o.other(0, 0).tobytes(),
        code_phase=4000.0, f_hz=250.0)
    # -- D = 32 on 101 bins
    add("D", "d_32_inside", lambda o: bins(o, V.SEARCHED, 18, 65), f_hz=0.0)
    add("D", "d_32_clipped_below", lambda o: bins(o, V.SEARCHED | V.CLIPPED, 0, 43), f_hz=-4000.0)
    add("D", "d_32_clipped_above", lambda o: bins(o, V.SEARCHED | V.CLIPPED, 78, 23), f_hz=6000.0)
    add("D", "d_32_last_bin_alone", lambda o: bins(o, V.SEARCHED | V.CLIPPED, 100, 1), f_hz=8200.0)
    # -- the top of the range
    add("T", "the_top_of_the_range", lambda o: int(o.peaks[0]["max_val"]) == 3 * 16352 * 20 and int(o.peaks[0]["phase"]) == T_TAU and o.sum_from_e(0),
        code_phase=T_TAU + 40.0, f_hz=float(T_HZ), prn=T_PRN)
    add("T", "the_peak_on_the_windows_edge", lambda o: int(o.peaks[0]["max_val"]) == 3 * 16352 * 20 and int(o.peaks[0]["phase"]) == T_TAU and o.taus[0] == T_TAU,
        code_phase=T_TAU + 128.0, f_hz=float(T_HZ), prn=T_PRN)
    add("T", "the_peak_one_outside_the_window", lambda o: int(o.peaks[0]["max_val"]) < 3 * 16352 * 20 and o.taus[0] == T_TAU + 1,
        code_phase=T_TAU + 129.0, f_hz=float(T_HZ), prn=T_PRN)
    # -- two equal maxima
    add("Q", "equal_maxima_across_the_seam_smallest_tau_is_not_the_first_j",
        lambda o: len(o.maxima(0)) >= 2 and o.maxima(0).min() < 2048 and o.maxima(0).max() > 14320 and int(o.peaks[0]["phase"]) == o.maxima(0).min()
        and o.taus[np.argmax(o.e[0])] > 14320, code_phase=float(Q_SEAM[1]), prn=Q_PRN)
    add("Q", "equal_maxima_smallest_tau_wins",
        lambda o: len(o.maxima(0)) >= 2 and int(o.peaks[0]["phase"]) == o.maxima(0).min() == o.taus[np.argmax(o.e[0])], code_phase=float(Q_FLAT[1]), prn=Q_PRN)
    return rows


ROWS = _rows()
_memo = {}


def launch(oracle, group):
    """the group's rows, N_PRN to a receiver (the last receiver filled up with records that select nothing) -> SimpleNamespace(cfg, grid,
    mag, stride, prns, pred [n_rx][N_PRN], blocks, units [(row, r, p)]); group Q: a receiver per row, its own block each"""
    if ("launch", group) in _memo:
        return _memo[("launch", group)]
    g = GROUPS[group]
    rows = [row for row in ROWS if row.group == group]
    n_prn = 1 if group in ("T", "Q") else N_PRN
    n_rx = (len(rows) + n_prn - 1) // n_prn
    prns = prn_list(n_prn)
    if group == "T":
        prns[0] = T_PRN
    if group == "Q":
        prns[0] = Q_PRN
    pred = V.make_pred(n_rx, n_prn)
    units = []
    for i, row in enumerate(rows):
        r, p = divmod(i, n_prn)
        assert row.prn is None or int(prns[p]) == row.prn
        V.set_pred(pred, r, p, row.code_phase, row.f_hz, row.flags)
        units.append((row, r, p))
    span = g.cfg["n_coh"] * g.cfg["n_seg"]
    if g.blocks == "matched":
        blocks = matched_blocks(oracle, T_PRN, 4092000 + T_HZ, span, T_TAU)
    elif g.blocks == "tie":
        blocks = np.concatenate([random_blocks(Q_SEAM[0], 1), random_blocks(Q_FLAT[0], 1)])
    else:
        blocks = random_blocks(ord(group), (n_rx - 1) * g.stride + span)
    la = SimpleNamespace(group=group, cfg=g.cfg, grid=g.grid, mag=g.mag, stride=g.stride, prns=prns, pred=pred, blocks=blocks, units=units, n_rx=n_rx,
                         n_prn=n_prn)
    _memo[("launch", group)] = la
    return la


def restated(oracle, la):
    """the restatement of a launch, once per process -> (peaks, rep, {(r, p, d): E over the window})"""
    key = ("restated", id(la))
    if key not in _memo:
        energies = {}
        peaks, rep = V.run(oracle, la.cfg, la.pred, la.blocks, la.prns, *la.grid, use_magnitude=la.mag, stride=la.stride, energies=energies)
        _memo[key] = (la, peaks, rep, energies)
    return _memo[key][1:]


def outcome(la, row, r, p, peaks, rep, energies):
    """what a row's predicate looks at"""
    cfg, (dmin, dstep, n_dopp) = la.cfg, la.grid
    d0, n = int(rep[r, p]["first_bin"]), int(rep[r, p]["n_bins"])
    searched = bool(int(rep[r, p]["flags"]) & V.SEARCHED)
    o = SimpleNamespace(row=row, rep=rep[r, p], peaks=peaks[r, p, d0:d0 + n] if searched else peaks[r, p], all_peaks=peaks[r, p],
                        taus=V.window(int(rep[r, p]["centre"]), cfg["half_width"]), e=[energies[(r, p, d)] for d in range(d0, d0 + n)] if searched else [])
    with np.errstate(all="ignore"):
        o.x = float((np.float64(row.f_hz) - np.float64(dmin)) / np.float64(dstep))
    o.phases_inside = lambda: all(int(pk["phase"]) in set(o.taus.tolist()) for pk in o.peaks if int(pk["max_val"]))
    o.outside_zero = lambda: not np.delete(o.all_peaks, np.arange(d0, d0 + n)).tobytes().strip(b"\0")
    o.maxima = lambda i: o.taus[o.e[i] == o.e[i].max()]

    def far(i):
        ph = int(o.peaks[i]["phase"])
        dist = np.minimum(np.abs(o.taus - ph), SAMPLES - np.abs(o.taus - ph))
        return o.e[i][dist > cfg["guard"]]
    o.far_count = lambda i: len(far(i))
    o.sum_from_e = lambda i: int(o.peaks[i]["sum"]) == (sum(int(v) for v in far(i)) * SAMPLES // len(far(i))) % (1 << 32) \
        and int(o.peaks[i]["avr"]) == int(o.peaks[i]["sum"]) // SAMPLES and int(o.peaks[i]["max_val"]) == int(o.e[i].max())
    o.other = lambda rr, pp: peaks[rr, pp, d0:d0 + n]
    return o


# ---- seeded random launches at the shapes the kernel takes its paths at -------------------------------------------------------------
# (n_rx, n_prn, n_coh, n_seg, W, D, both bits, n_dopp, stride): W 1 and 7: one phase per offset at most (64 lanes per phase); 8: two;
# 128: 17 (8 lanes per phase); 2047: 256 (a lane per phase).  n_prn 33 and 64: the PRN list's fifth and eighth word.
SHAPES = [
    (1, 1, 1, 1, 1, 0, True, 1, 1),
    (2, 2, 2, 2, 7, 1, False, 4, 0),
    (5, 33, 1, 1, 8, 0, True, 3, 1),
    (1, 64, 1, 2, 128, 1, False, 5, 2),
    (2, 2, 20, 3, 2047, 1, True, 6, 61),
    (1, 2, 2, 3, 128, 32, True, 70, 6),
    (3, 2, 2, 3, 8, 1, True, 4, 2),              # stride 2 under a span of 6: the receivers' searches overlap in part
]


def random_launch(i, permute=None):
    """shape i's launch: every unit selected with probability 0.6 (its centre anywhere, now and then on the seam; its Doppler anywhere on
    the lattice and a little beyond), else skipped, bad or off the lattice; permute: the receivers (their blocks and records) in this order"""
    n_rx, n_prn, n_coh, n_seg, w, d, mag, n_dopp, stride = SHAPES[i]
    rng = np.random.default_rng(9000 + i)
    grid = (-300 * (n_dopp // 2), 300, n_dopp)
    cfg = V.make_cfg(n_coh, n_seg, w, d, int(rng.integers(0, w)))
    pred = V.make_pred(n_rx, n_prn)
    for r in range(n_rx):
        for p in range(n_prn):
            kind = rng.random()
            cp = float(rng.choice([rng.uniform(0, 16368), rng.integers(0, 16369), rng.choice([0.0, 16367.6, w - 1.0, 16368.0 - w])]))
            f = float(rng.uniform(grid[0] - 450, grid[0] + 300 * n_dopp + 150))
            flags = SEL | (int(rng.integers(0, 2)) * 8)
            if kind > 0.9:
                flags = int(rng.choice([0, 1, V.PREDICTED | 1, SEL | V.TRACKED, SEL | V.ASSIGNED]))
            elif kind > 0.8:
                cp, f = [(NAN, f), (-1.0, f), (cp, INF), (16368.25, f)][int(rng.integers(0, 4))]
            elif kind > 0.6:
                f = float(rng.choice([-1e6, 1e6, 3e12]))
            if r == 0 and p == 0:            # (one unit of every launch is searched, whatever the draws)
                cp, f, flags = float(rng.integers(0, 16368)) + 0.25, float(grid[0] + 300 * (n_dopp // 2) + 20), SEL
            V.set_pred(pred, r, p, cp, f, flags)
    span = n_coh * n_seg
    blocks = random_blocks(100 + i, max((n_rx - 1) * stride + span, n_rx * stride))
    if permute is not None:
        assert stride >= span                # (a receiver's blocks are its own)
        pred = pred[list(permute)]
        blocks = np.concatenate([blocks[r * stride:(r + 1) * stride] for r in permute])
    return SimpleNamespace(cfg=cfg, grid=grid, mag=mag, stride=stride, prns=prn_list(n_prn), pred=pred, blocks=blocks, n_rx=n_rx, n_prn=n_prn)


# ---- more workgroups than one launch holds -------------------------------------------------------------------------------------------------
BIG_RX, BIG_D = 1 << 20, 8                   # 2^20 receivers x 1 PRN x 17 workgroups = 17.8 M: the launcher cuts at 2^24 - 1 workgroups, 986 895 receivers
BIG_CUT = ((1 << 24) - 1) // (2 * BIG_D + 1)
BIG_SELECTED = (0, 1, BIG_CUT - 1, BIG_CUT, BIG_CUT + 1, BIG_RX - 1)


def big_launch():
    """BIG_RX receivers on ONE block (stride 0), one PRN, one bin: every record skipped but BIG_SELECTED's, which sit on both sides of the
    launcher's cut -> the launch; its restatement is the selected receivers' alone (the others' records and reports are a flag and zeros)"""
    pred = V.make_pred(BIG_RX, 1)
    for i, r in enumerate(BIG_SELECTED):
        V.set_pred(pred, r, 0, 1000.0 + 37.0 * i, 3.0 * i)
    return SimpleNamespace(cfg=V.make_cfg(1, 1, 1, BIG_D, 0), grid=(0, 500, 1), mag=True, stride=0, prns=prn_list(1), pred=pred, blocks=random_blocks(55, 1),
                           n_rx=BIG_RX, n_prn=1)


# ---- the scenario: weighted_acq_cases' two receivers, predictions 40 samples and 130 Hz off the truth ---------------------------------
SCN_W, SCN_D, SCN_GUARD = 128, 2, 32
SCN_OFF = (40, 130.0)
# measured on the CPU restatement (tests/test_weighted_win_reference.py measures both again and compares): max_val 16368 / sum of the best
# window records of the six present (receiver, PRN) rows at least / of the ten absent rows at most
MEASURED = dict(present_min=6.734, absent_max=1.926)
# ... and on the warm start (weighted_pvt_cases' stream at block 24 576, the bank's four entries replaced by an almanac cut of the stream's
# ephemerides): the largest error of gpsx_wpred's code phase (samples) and f_hz (Hz) against the synthesiser's truth, and the least peak over
# far mean of the four satellites' best window records at 10 x 8 blocks.  W and D follow from the first two (test_weighted_win_reference.py)
WARM_MEASURED = dict(phase_samples=16.74, freq_hz=0.663, present_min=25.6)
WARM_GRID = (-10000, 50, 401)                # the stream's Dopplers are -2873 .. 2722 Hz


def scenario_pred():
    """prediction records for weighted_acq_cases' scenario: the six present pairs SCN_OFF off weighted_multi_cases.CHAIN_SATS' truth,
    the ten absent ones anywhere (seeded)"""
    import weighted_acq_cases as AC
    import weighted_multi_cases as M
    rng = np.random.default_rng(31)
    pred = V.make_pred(2, len(AC.SCN_PRNS))
    for r in range(2):
        truth = {sat[0]: sat for sat in M.CHAIN_SATS[r]}
        for p, prn in enumerate(AC.SCN_PRNS):
            if prn in truth:
                _, dopp, delay = truth[prn][:3]
                V.set_pred(pred, r, p, (float(delay) + SCN_OFF[0]) % SAMPLES, float(dopp) + SCN_OFF[1])
            else:
                V.set_pred(pred, r, p, float(rng.uniform(0, SAMPLES)), float(rng.uniform(-4000, 4000)))
    return pred


def scenario_cfg():
    import weighted_acq_cases as AC
    return V.make_cfg(AC.SCN_COH, AC.SCN_SEG, SCN_W, SCN_D, SCN_GUARD)


# ---- the smoke fixture (tests/golden/wwin_smoke.npz) -----------------------------------------------------------------------------------
SMOKE_SEED = 4242


def smoke_case(oracle):
    """3 receivers x 3 PRNs x 2 x 2 blocks: searched windows (one across the seam, one clipped), a skipped, a bad and an off-lattice
    record; the blocks are random_blocks(SMOKE_SEED, 12) -> the arrays of the fixture"""
    cfg, grid = V.make_cfg(2, 2, 24, 1, 4), (-600, 300, 5)
    prns = np.array([5, 14, 20], np.uint8)
    pred = V.make_pred(3, 3)
    for (r, p), (cp, f, fl) in {(0, 0): (1234.4, 10.0, SEL), (0, 1): (3.5, -600.0, SEL), (0, 2): (100.0, 0.0, SEL | V.TRACKED),
                                (1, 0): (16360.0, 600.0, SEL | 8), (1, 1): (NAN, 0.0, SEL), (1, 2): (9000.5, 140.0, SEL),
                                (2, 0): (500.0, 5000.0, SEL), (2, 1): (16368.0, -149.9, SEL), (2, 2): (0.0, 0.0, 1)}.items():
        V.set_pred(pred, r, p, cp, f, fl)
    blocks = random_blocks(SMOKE_SEED, 12)
    peaks, rep = V.run(oracle, cfg, pred, blocks, prns, *grid, use_magnitude=True, stride=4)
    return dict(cfg=V.cfg_record(cfg), prns=prns, grid=np.array(grid, np.int32), seed=np.int64(SMOKE_SEED), n_blocks=np.int64(12), stride=np.int64(4), pred=pred,
                peaks=peaks, rep=rep)


def smoke_blocks(seed, n):
    """the fixture's blocks from its stored seed (what __graft_entry__.smoke() does without this module)"""
    return random_blocks(int(seed), int(n))


def write_smoke():
    """(`python tests/weighted_win_cases.py`) writes the fixture"""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    from oracle import pyoracle
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wwin_smoke.npz")
    np.savez_compressed(path, **smoke_case(pyoracle.Oracle()))
    return path


if __name__ == "__main__":
    print(write_smoke())
