"""An exact CPU restatement of the weighted path's observables (include/gpsx.h gpsx_wobs), for the tests: the header's two passes
per channel and launch, in its order, on Python integers and np.float32.  Nothing of the library's code is included or imported."""
import numpy as np

F_PHASE, F_EDGE, F_TOW, F_CONFIRMED, F_AMBIGUOUS, F_VALID = 1, 2, 4, 8, 16, 32
STATE_FLAGS = F_PHASE | F_EDGE | F_TOW | F_CONFIRMED | F_AMBIGUOUS
WSYNC_WINDOW, WSYNC_LOCKED, WSYNC_BIT = 1, 2, 4
WNAV_WORD, WNAV_OK = 1, 2

CFG_DTYPE = np.dtype([("edge_guard", "<f4"), ("reserved", "<i4")])
STATE_DTYPE = np.dtype([("blocks_seen", "<i8"), ("last_bit_end_p1", "<i8"), ("chain_first_p1", "<i8"), ("edge_block", "<i8"),
                        ("tx_ms_at_edge", "<i8"), ("last_win_end_p1", "<i8"), ("last_phase", "<f4"), ("last_freq", "<f4"), ("flags", "<u4"),
                        ("n_wraps", "<u4"), ("n_anchor", "<u4"), ("n_mismatch", "<u4"), ("n_break", "<u4"), ("reserved", "<u4")])
OBS_DTYPE = np.dtype([("tx_ms", "<i8"), ("code_phase_fine", "<f4"), ("if_freq_offset_hz", "<f4"), ("flags", "<u4"), ("age_blocks", "<i4"),
                      ("n_wraps", "<u4"), ("reserved", "<u4")])
assert CFG_DTYPE.itemsize == 8 and STATE_DTYPE.itemsize == 80 and OBS_DTYPE.itemsize == 32

WEEK_MS = 604_800_000
SAMPLES = 16368
MAX_COUNT = 1 << 62
M32 = 0xFFFFFFFF
HALF, FULL = np.float32(8184.0), np.float32(16368.0)


def state_valid(s):
    if s["flags"] & ~STATE_FLAGS or s["reserved"] != 0:
        return False
    if not all(0 <= s[name] <= MAX_COUNT for name in ("blocks_seen", "last_bit_end_p1", "chain_first_p1", "last_win_end_p1")):
        return False
    if abs(s["edge_block"]) > MAX_COUNT or not 0 <= s["tx_ms_at_edge"] < WEEK_MS:
        return False
    p = s["last_phase"]
    return not (s["flags"] & F_PHASE) or bool(p >= np.float32(0.0) and p < FULL)


def _broke(s):
    if s["flags"] & F_EDGE:
        s["n_break"] = (s["n_break"] + 1) & M32
    s["flags"] &= ~(F_EDGE | F_TOW | F_CONFIRMED | F_AMBIGUOUS)


def channel(windows, words, s, n_blocks, edge_guard):
    """windows: [(end_block, flags, code_phase_fine, if_freq_offset_hz)] of one launch in slot order, words: [(end_block, flags,
    index, aux)] likewise, neither filtered; s: the state as a dict (Python ints, np.float32 for the two floats), advanced in place
    -> the observable as a dict"""
    edge_guard = np.float32(edge_guard)
    seen = s["blocks_seen"]
    # pass 1: the window records
    for end_block, flags, p, freq in windows:
        p = np.float32(p)
        if not (flags & WSYNC_WINDOW and 0 <= end_block < n_blocks and p >= np.float32(0.0) and p < FULL):
            continue
        w_p1 = seen + end_block + 1
        if not flags & WSYNC_LOCKED:                                   # 1: a SEARCH window
            _broke(s)
            s["last_bit_end_p1"] = 0
        if s["flags"] & F_EDGE and s["flags"] & F_PHASE:               # 2: a wrap of the code phase
            d = np.float32(p - s["last_phase"])
            if d > HALF:
                s["edge_block"] -= 1
                s["n_wraps"] = (s["n_wraps"] + 1) & M32
            elif d < -HALF:
                s["edge_block"] += 1
                s["n_wraps"] = (s["n_wraps"] + 1) & M32
        s["last_phase"], s["last_freq"], s["last_win_end_p1"] = p, np.float32(freq), w_p1      # 3: the newest record
        s["flags"] |= F_PHASE
        if flags & WSYNC_BIT and flags & WSYNC_LOCKED:                 # 4: a bit
            if s["last_bit_end_p1"] != 0 and w_p1 != s["last_bit_end_p1"] + 20:
                _broke(s)
            if not s["flags"] & F_EDGE:
                s["edge_block"] = w_p1 - (1 if p >= HALF else 0)
                s["chain_first_p1"] = w_p1
                s["flags"] |= F_EDGE
                if np.abs(np.float32(p - HALF)) < edge_guard:
                    s["flags"] |= F_AMBIGUOUS
            s["last_bit_end_p1"] = w_p1
    # pass 2: the HOWs
    for end_block, flags, index, aux in words:
        if not (flags & WNAV_WORD and flags & WNAV_OK and index == 2 and aux < 100800 and 0 <= end_block < n_blocks and s["flags"] & F_EDGE):
            continue
        e_p1 = seen + end_block + 1
        if not (e_p1 >= s["chain_first_p1"] + 1220 and e_p1 <= s["last_bit_end_p1"] and (s["last_bit_end_p1"] - e_p1) % 20 == 0):
            continue
        t = 6000 * ((aux + 100799) % 100800) + 1200
        j = (e_p1 - s["edge_block"] + 10) // 20
        r = e_p1 - s["edge_block"] - 20 * j
        if abs(r) > 5:
            s["n_mismatch"] = (s["n_mismatch"] + 1) & M32
            continue
        tc = (t - 20 * j) % WEEK_MS
        if not s["flags"] & F_TOW:
            s["tx_ms_at_edge"] = tc
            s["flags"] |= F_TOW
            s["n_anchor"] = (s["n_anchor"] + 1) & M32
        elif tc == s["tx_ms_at_edge"]:
            s["flags"] |= F_CONFIRMED
        else:
            s["tx_ms_at_edge"] = tc
            s["flags"] &= ~F_CONFIRMED
            s["n_mismatch"] = (s["n_mismatch"] + 1) & M32
    # the observable at the first sample of block B
    s["blocks_seen"] = b = seen + n_blocks
    need = F_PHASE | F_EDGE | F_TOW
    valid = s["flags"] & need == need
    has_phase = bool(s["flags"] & F_PHASE)
    return dict(tx_ms=(s["tx_ms_at_edge"] + b - s["edge_block"]) % WEEK_MS if valid else 0,
                code_phase_fine=s["last_phase"] if has_phase else np.float32(0.0), if_freq_offset_hz=s["last_freq"] if has_phase else np.float32(0.0),
                flags=s["flags"] | (F_VALID if valid else 0), age_blocks=max(0, min(b - s["last_win_end_p1"], (1 << 31) - 1)) if has_phase else -1,
                n_wraps=s["n_wraps"], reserved=0)


def _state_dict(states, ch):
    return {name: (np.float32(states[name][ch]) if name in ("last_phase", "last_freq") else int(states[name][ch])) for name in STATE_DTYPE.names}


def run(rec, n_blocks, words, states, edge_guard, channels=None):
    """one launch: rec [n_slots][n_ch] (the sync loop's records: fields w.code_phase_fine, w.if_freq_offset_hz, end_block, flags),
    words [n_blocks // 600 + 2][n_ch] (the word layer's: end_block, flags, index, aux), states a STATE_DTYPE array advanced in place
    -> (OBS_DTYPE [n_ch], the BAD channels)"""
    assert states.dtype == STATE_DTYPE and 1 <= n_blocks <= 4096 and 1 <= rec.shape[0] <= n_blocks and words.shape[0] == n_blocks // 600 + 2
    assert np.isfinite(edge_guard) and 0 <= edge_guard <= 8184
    obs = np.zeros(len(states), OBS_DTYPE)
    bad = []
    for ch in (range(len(states)) if channels is None else channels):
        s = _state_dict(states, ch)
        if not state_valid(s):
            bad.append(ch)
            obs["age_blocks"][ch] = -1
            continue
        col, wcol = rec[:, ch], words[:, ch]
        o = channel(list(zip(col["end_block"].tolist(), col["flags"].tolist(), col["w"]["code_phase_fine"], col["w"]["if_freq_offset_hz"])),
                    list(zip(wcol["end_block"].tolist(), wcol["flags"].tolist(), wcol["index"].tolist(), wcol["aux"].tolist())), s, n_blocks, edge_guard)
        for name in STATE_DTYPE.names:
            states[name][ch] = s[name]
        for name in OBS_DTYPE.names:
            obs[name][ch] = o[name]
    return obs, bad


def tx_time_ms(o):
    """the transmit time at sample 0 of block B, in ms of the week, as a float64 (exact to 2^-23 ms): tx_ms - code_phase_fine / 16368"""
    return float(int(o["tx_ms"])) - float(o["code_phase_fine"]) / SAMPLES


def pseudoranges(obs, offset_ms):
    """gpsx_wobs_pseudoranges on float64 -> (pr_m, rx_tow_s, the number of VALID observables)"""
    def fold(d):
        return (d + WEEK_MS // 2) % WEEK_MS - WEEK_MS // 2
    valid = [i for i in range(len(obs)) if int(obs["flags"][i]) & F_VALID]
    pr = np.zeros(len(obs))
    if not valid:
        return pr, 0.0, 0
    ref = valid[0]
    for i in valid[1:]:      # the latest transmit time: the whole milliseconds folded, then the phases (a smaller phase is later)
        d = fold(int(obs["tx_ms"][i]) - int(obs["tx_ms"][ref])) - (float(obs["code_phase_fine"][i]) - float(obs["code_phase_fine"][ref])) / SAMPLES
        if d > 0:
            ref = i
    for i in valid:
        pr[i] = 299792458e-3 * (float(fold(int(obs["tx_ms"][ref]) - int(obs["tx_ms"][i]))) +
                                (float(obs["code_phase_fine"][i]) - float(obs["code_phase_fine"][ref])) / 16368.0 + offset_ms)
    rx = (float(int(obs["tx_ms"][ref])) - float(obs["code_phase_fine"][ref]) / 16368.0 + offset_ms) / 1000.0
    rx = rx - 604800.0 if rx >= 604800.0 else (rx + 604800.0 if rx < 0.0 else rx)
    return pr, rx, len(valid)
