"""What the CPU and GPU tests of the weighted loop with bit sync share (include/gpsx.h gpsx_track_loop_weighted_sync): the
three-satellite scenario with bit edges that differ, the strong short stream with mixed initial states the byte-for-byte comparisons
run on, and helpers that read records.  The launch shape is k_track_wloop's (csrc/gpsx_track_loop_weighted_plan.hpp, asserted row by
row in tests/test_track_loop_weighted_plan.py): channel counts come from weighted_loop_cases.SHAPES."""
import numpy as np

import weighted_loop_cases as S
import weighted_sync_ref as Y

# ---- the scenario: three satellites whose data bit edges sit 0, 10 and 5 ms after the stream's start ------------------------------
# (prn, Doppler Hz, code delay in samples, bit edge in ms, carrier phase).  A satellite whose code starts late in a block
# (12007, 13000 of 16368 samples) has its first mostly-new block one later: the synchroniser's edges are 0, 11, 6.
SATS = [(7, 1310.0, 4321.0, 0, 0.4), (19, -2240.0, 12007.0, 10, 2.0), (30, 2018.0, 13000.0, 5, 4.0)]
EDGES_FOUND = (0, 11, 6)
AMPLITUDE = S.AMPLITUDE
SEEDS = S.SEEDS
N_MS = 2000
SYNC_BITS, RATIO = 20, (5, 4)
N_COH_SEARCH, N_COH_LOCK = 4, 20


def scenario(seed, n_ms, amp=AMPLITUDE):
    """n_ms two-bit blocks and per satellite its +-1 data bits: bit u of satellite j starts SATS[j] edge + 20 u ms (plus its code
    delay) after the stream's start; what comes before is the bit array's last entry"""
    from stm32f4_sdr_gps_amd import synth
    sats, bits = [], []
    for j, (prn, fd, delay, edge, phase) in enumerate(SATS):
        rng = np.random.default_rng(1000 * (j + 1) + seed)
        bits.append(rng.integers(0, 2, n_ms // 20 + 2) * 2.0 - 1.0)
        sats.append(synth.Sat(prn, fd, delay + 16368.0 * edge, amp, phase, nav_bits=bits[-1]))
    return synth.make_if(n_ms, sats, noise_amp=1.0, seed=seed, two_bit=True), bits


def handover_states(seed):
    """the three channels' zeroed states with a _coh-style record's errors (weighted_loop_cases.HANDOVER: 3 samples, 12.5 Hz)"""
    d_phase, d_hz = S.HANDOVER[seed]
    return np.concatenate([Y.handover(prn, delay + d_phase, fd + d_hz) for prn, fd, delay, _, _ in SATS])


def sync_cfg():
    return Y.make_cfg(N_COH_SEARCH, N_COH_LOCK, S.PULL_IN, S.STEADY, SYNC_BITS, RATIO)


def bit_errors(bit_records, bits, edge_found):
    """bit_records: [(absolute last block of the bit, bit_ip)] of a channel that started SEARCH with ms_count 0 at block 0 and
    locked on edge_found -> (mismatches up to one polarity, bits compared).  The bit that ends at block e started at e - 19 =
    edge_found + 20 u."""
    got, want = [], []
    for end, ip in bit_records:
        u, r = divmod(end - 19 - edge_found, 20)
        assert r == 0 and u >= 0, (end, edge_found)
        got.append(1.0 if ip > 0 else -1.0)
        want.append(bits[u])
    got, want = np.array(got), np.array(want)
    return min(int((got != want).sum()), int((got != -want).sum())), len(got)


def rekey(rec_list):
    """[(first block of the launch, REC array [slots][n_ch])] -> {(channel, absolute end block): the record's bytes with end_block
    made absolute}, and a check that every slot is a window's record or the empty pattern"""
    out = {}
    for at, rec in rec_list:
        for slot in range(rec.shape[0]):
            for ch in range(rec.shape[1]):
                r = rec[slot, ch].copy()
                if int(r["flags"]) == 0:
                    want = np.zeros((), Y.REC_DTYPE)
                    want["end_block"] = -1
                    assert r.tobytes() == want.tobytes(), (at, slot, ch, r)
                    continue
                assert int(r["flags"]) & Y.F_WINDOW and int(r["end_block"]) >= 0
                r["end_block"] += at
                key = (ch, int(r["end_block"]))
                assert key not in out
                out[key] = r.tobytes()
    return out


# ---- the strong short stream: data bits alternating every 20 ms, edges differing per satellite ------------------------------------
STRONG = [(7, 1310.0, 4321.0, 3, 0.4), (19, -2240.0, 12007.0, 16, 2.0), (30, 2018.0, 13000.0, 9, 4.0)]
STRONG_EDGES = (3, 17, 10)    # as a SEARCH that starts with ms_count 0 at block 0 finds them


def strong_blocks(n, amp=0.3, seed=3):
    from stm32f4_sdr_gps_amd import synth
    alt = np.array([1.0, -1.0])
    sats = [synth.Sat(prn, fd, delay + 16368.0 * edge, amp, phase, nav_bits=alt) for prn, fd, delay, edge, phase in STRONG]
    return synth.make_if(n, sats, noise_amp=1.0, seed=seed, two_bit=True)


# code phases on the seam (tau -+ spacing wraps on either side for every spacing; an update can carry them across either end)
PHASES = [4321.0, 12007.0, 13000.0, 0.0, 7.9, 16367.99, 3.0, 16365.0, 0.5, 14.0, 16353.0, 12007.25, 1.0, 16367.0, 15.0, 16352.5]
PRNS = [7, 19, 30, 1, 33, 64, 150, 210, 32, 209, 5, 100]


def mixed_states(n, seed, kinds=None):
    """n states: the first three are fresh SEARCH handovers on the stream's satellites; the others cycle through fresh SEARCH,
    SEARCH with a half-open window and a running round, WAIT, and LOCKED at assorted edge / ms_count / win_n, with and without loop
    memory; three in four track one of the stream's satellites at its code phase.  `kinds`: restrict the cycle."""
    rng = np.random.default_rng(seed)
    st = np.zeros(n, Y.STATE_DTYPE)
    lp = st["loop"]
    for ch in range(n):
        sat = ch % 3
        on = ch < 3 or ch % 4 != 3
        lp["prn"][ch] = STRONG[sat][0] if on else PRNS[ch % len(PRNS)]
        lp["code_phase_fine"][ch] = (STRONG[sat][2] + (0.0 if ch < 3 else float(rng.integers(-2, 3)))) if on else PHASES[ch % len(PHASES)]
        lp["if_freq_offset_hz"][ch] = STRONG[sat][1] + (0.0 if ch < 3 else float(rng.integers(-8, 9))) if on else float(rng.integers(-5000, 5001))
        lp["if_freq_accum"][ch] = 0 if ch % 5 == 0 else int(rng.integers(0, 1 << 32))
        kind = 0 if ch < 3 else (ch % 4 if kinds is None else kinds[ch % len(kinds)])
        if ch >= 3 and ch % 2 == 1:
            lp["dll_err"][ch], lp["pll_err"][ch] = rng.uniform(-0.5, 0.5), rng.uniform(-0.2, 0.2)
            lp["prev_ip"][ch], lp["prev_qp"][ch] = rng.integers(-30000, 30001, 2)
            lp["n_updates"][ch] = rng.integers(1, 1000)
        if kind == 1:            # SEARCH in the middle of a window and of a round
            st["win_iq"][ch] = rng.integers(-20000, 20001, 6)
            st["win_n"][ch] = 1 + ch % 3
            st["ms_count"][ch] = rng.integers(0, 20)
            st["search_n"][ch] = (5, 20, 27, 38, 39)[(ch // 4) % 5]
            st["p_i"][ch], st["p_q"][ch] = rng.integers(-100000, 100001, 2)
            st["base"][ch] = rng.integers(-100000, 100001, (20, 2))
            st["e"][ch] = rng.integers(0, 1 << 36, 20)
            st["prev_best_p1"][ch] = rng.integers(0, 21)
            st["sync_rounds"][ch] = rng.integers(0, 5)
            if st["search_n"][ch] == 39:      # decides at the launch's first block, in agreement with its predecessor, at a ratio of 2
                j = int(rng.integers(0, 20))
                st["e"][ch][j], st["e"][ch][(j + 10) % 20], st["prev_best_p1"][ch] = 1 << 40, 1 << 39, j + 1
        elif kind == 2:          # WAIT: leaves it inside the launch (after at most 19 blocks)
            st["mode"][ch], st["edge"][ch], st["ms_count"][ch] = Y.WAIT, rng.integers(0, 20), rng.integers(0, 20)
            st["prev_best_p1"][ch], st["sync_rounds"][ch] = st["edge"][ch] + 1, 2
        elif kind == 3:          # LOCKED, mid-bit, a window open
            st["mode"][ch], st["edge"][ch] = Y.LOCKED, rng.integers(0, 20)
            into = int(rng.integers(0, 20))                    # blocks of the bit already seen
            st["ms_count"][ch] = (st["edge"][ch] + into) % 20
            st["win_n"][ch] = into % 5      # (not always what one cfg would have left: a short window may follow another closely)
            st["win_iq"][ch] = rng.integers(-20000, 20001, 6) * (1 if st["win_n"][ch] else 0)
            st["bit_ip"][ch] = rng.integers(-200000, 200001)
    return st


DISTINCT = 32


def tiled_states(n, seed, period=DISTINCT):
    """n states that repeat mixed_states(period): a restatement of `period` channels answers for all of them"""
    distinct = mixed_states(min(n, period), seed)
    return distinct[np.arange(n) % len(distinct)].copy(), len(distinct)


# ---- the case table of the byte-for-byte comparison: 130 blocks, sync_bits = 1 (decisions of a fresh search at blocks 39 and 79) ---
N_BLOCKS = 130
# (channels, (n_coh_search, n_coh_lock), sign and magnitude, spacing, (sync_num, sync_den))
CASES = [(1, (4, 20), True, 8, (5, 4)), (3, (1, 10), False, 1, (5, 4)), (5, (20, 5), True, 15, (5, 4)), (64, (5, 5), True, 8, (5, 4)),
         (257, (4, 20), False, 15, (5, 4)), (64, (1, 10), True, 8, (1024, 1)), (5, (5, 5), False, 15, (2, 1)), (64, (20, 5), False, 1, (5, 4))]
_cases = {}


def case(oracle, i):
    """case i on the restatement, computed once per process: (blocks, states before, cfg, records wanted, states wanted, events)"""
    if i not in _cases:
        n_ch, pair, use_mag, spacing, ratio = CASES[i]
        blocks = strong_blocks(N_BLOCKS)
        st0, distinct = tiled_states(n_ch, 100 * n_ch + i)
        cfg = Y.make_cfg(pair[0], pair[1], S.PULL_IN, S.STEADY, 1, ratio, use_mag, spacing)
        first = st0[:distinct].copy()
        events = []
        rec = Y.run(oracle, blocks, first, cfg, events=events)
        idx = np.arange(n_ch) % distinct
        _cases[i] = (blocks, st0, cfg, np.ascontiguousarray(rec[:, idx]), first[idx].copy(), events)
    return _cases[i]


def case_table_events(oracle):
    """what the table's channels meet, from the restatement's events and records: {"accept", "disagree" (a round before it named
    another candidate), "ratio" (agreed, refused for its energy ratio), "left_wait", "bit"} -> [(case, channel, block)]"""
    seen = {k: [] for k in ("accept", "disagree", "ratio", "left_wait", "bit")}
    for i in range(len(CASES)):
        _, st0, _, rec, _, events = case(oracle, i)
        for e in events:
            if e[2] == "decision":
                _, _, _, best, accepted, agreed, _, _, prev = e
                what = "accept" if accepted else ("ratio" if agreed else ("disagree" if prev != 0 else None))
                if what:
                    seen[what].append((i, e[0], e[1]))
            elif e[2] == "locked" and int(st0["mode"][e[0]]) == Y.WAIT:
                seen["left_wait"].append((i, e[0], e[1]))
        for ch in np.nonzero((rec["flags"] & Y.F_BIT).any(axis=0))[0][:4]:
            seen["bit"].append((i, int(ch), -1))
    return seen


def bad_channel_states():
    """twelve states, five of them bad: a PRN of 0, a NaN code phase, mode = 7, ms_count = 20, and edge = -1 in LOCKED"""
    st = mixed_states(12, 4)
    st["loop"]["prn"][2] = 0
    st["loop"]["code_phase_fine"][5] = np.nan
    st["mode"][7] = 7
    st["ms_count"][8] = 20
    st["mode"][11], st["edge"][11] = Y.LOCKED, -1
    return st, (2, 5, 7, 8, 11)
