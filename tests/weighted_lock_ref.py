"""An exact CPU restatement of the weighted path's lock monitor (include/gpsx.h gpsx_wlock), for the tests: the header's five steps
per record and its launch end, in its order, on Python integers and np.float32.  Nothing of the library's code is included or
imported."""
import math

import numpy as np

F_CODE, F_CARRIER, F_PENDING, F_OPEN_LOCKED, F_EPOCH_LOCKED = 1, 2, 4, 8, 16
F_LOST_CODE, F_LOST_CARRIER, F_REARMED, F_RANGE = 32, 64, 128, 256
STATE_FLAGS = F_CODE | F_CARRIER | F_PENDING | F_OPEN_LOCKED | F_EPOCH_LOCKED
OUT_FLAGS = F_CODE | F_CARRIER | F_EPOCH_LOCKED
WSYNC_WINDOW, WSYNC_LOCKED, WSYNC_BIT = 1, 2, 4
SYNC_SEARCH, SYNC_WAIT, SYNC_LOCKED = 0, 1, 2

CFG_DTYPE = np.dtype([("epoch_search", "<i4"), ("epoch_lock", "<i4"), ("code_min", "<f4"), ("car_min", "<f4"), ("snr_min", "<f4"),
                      ("n_good", "<i4"), ("n_bad", "<i4"), ("rearm", "<i4"), ("patience", "<i4"), ("reserved", "<i4")])
STATE_DTYPE = np.dtype([("blocks_seen", "<i8"), ("last_epoch_end_p1", "<i8"), ("sum_a", "<i8"), ("sum_p", "<i8"), ("sum_d", "<i8"),
                        ("sum_e", "<i8"), ("sum_l", "<i8"), ("last_p", "<i8"), ("last_code_ratio", "<f4"), ("last_car_ratio", "<f4"),
                        ("last_snr", "<f4"), ("epoch_n", "<u4"), ("flags", "<u4"), ("last_k", "<u4"), ("code_good", "<u4"),
                        ("code_bad", "<u4"), ("car_good", "<u4"), ("car_bad", "<u4"), ("false_run", "<u4"), ("n_lost_code", "<u4"),
                        ("n_lost_carrier", "<u4"), ("n_rearm", "<u4"), ("n_range", "<u4"), ("reserved", "<u4")])
LOCK_DTYPE = np.dtype([("flags", "<u4"), ("n_epochs", "<u4"), ("last_k", "<u4"), ("age_blocks", "<i4"), ("code_ratio", "<f4"),
                       ("car_ratio", "<f4"), ("snr", "<f4"), ("n_range", "<u4"), ("p", "<i8"), ("n_lost_code", "<u4"),
                       ("n_lost_carrier", "<u4"), ("n_rearm", "<u4"), ("reserved", "<u4", (3,))])
assert CFG_DTYPE.itemsize == 40 and STATE_DTYPE.itemsize == 128 and LOCK_DTYPE.itemsize == 64
FLOATS = ("last_code_ratio", "last_car_ratio", "last_snr")

RANGE = 1 << 20
MAX_COUNT = 1 << 62
MAX_SUM, MAX_A = 1 << 51, 1 << 30
M32 = 0xFFFFFFFF
ZERO = np.float32(0.0)


def make_cfg(epoch_search, epoch_lock, code_min, car_min, snr_min, n_good, n_bad, rearm=0, patience=0):
    assert 1 <= epoch_search <= 1024 and 1 <= epoch_lock <= 1024 and 1 <= n_good <= 255 and 1 <= n_bad <= 255 and 0 <= rearm <= 3 and patience >= 0
    assert all(math.isfinite(t) for t in (code_min, car_min, snr_min))
    return dict(epoch_search=int(epoch_search), epoch_lock=int(epoch_lock), code_min=np.float32(code_min), car_min=np.float32(car_min),
                snr_min=np.float32(snr_min), n_good=int(n_good), n_bad=int(n_bad), rearm=int(rearm), patience=int(patience))


def cfg_array(cfg, reserved=0):
    out = np.zeros(1, CFG_DTYPE)
    for name in cfg:
        out[name] = cfg[name]
    out["reserved"] = reserved
    return out


def f32_of_int(v):
    """(float)v of an int64: one rounding, to nearest even (through a double it would be two for |v| >= 2^53)"""
    a = abs(v)
    over = a.bit_length() - 24
    if over > 0:
        q, rest, half = a >> over, a & ((1 << over) - 1), 1 << (over - 1)
        if rest > half or (rest == half and q & 1):
            q += 1
        a = q << over
    return np.float32(-float(a) if v < 0 else float(a))


def ratios(k, a, p, d, e, l):
    """an epoch's (code_ratio, car_ratio, snr) from its K and five sums"""
    el, aa = e + l, a * a
    den = k * p - aa
    assert abs(den) < 1 << 63 and 2 * p < 1 << 63 and el < 1 << 63
    return (ZERO if el == 0 else f32_of_int(2 * p) / f32_of_int(el), ZERO if p == 0 else f32_of_int(d) / f32_of_int(p),
            ZERO if den == 0 else f32_of_int(aa) / f32_of_int(den))


def state_valid(s):
    if s["flags"] & ~STATE_FLAGS or s["reserved"] != 0:
        return False
    if not (0 <= s["blocks_seen"] <= MAX_COUNT and 0 <= s["last_epoch_end_p1"] <= MAX_COUNT and s["epoch_n"] <= 1023 and s["last_k"] <= 1024):
        return False
    if any(s[name] > 255 for name in ("code_good", "code_bad", "car_good", "car_bad")):
        return False
    return 0 <= s["sum_a"] <= MAX_A and all(0 <= s[name] <= MAX_SUM for name in ("sum_p", "sum_e", "sum_l")) and abs(s["sum_d"]) <= MAX_SUM


def _verdict(s, ev, good, run_good, run_bad, bit, lost_count, lost_event, cfg):
    """one verdict on an indicator's two runs and its flag -> the flag was cleared"""
    if good:
        s[run_bad] = 0
        s[run_good] = min(s[run_good] + 1, 255)
        if s[run_good] >= cfg["n_good"]:
            s["flags"] |= bit
        return False
    s[run_good] = 0
    s[run_bad] = min(s[run_bad] + 1, 255)
    if s["flags"] & bit and s[run_bad] >= cfg["n_bad"]:
        s["flags"] &= ~bit
        s[lost_count] = (s[lost_count] + 1) & M32
        ev["flags"] |= lost_event
        return True
    return False


def _clear_epoch(s):
    for name in ("sum_a", "sum_p", "sum_d", "sum_e", "sum_l", "epoch_n"):
        s[name] = 0


def channel(windows, s, n_blocks, cfg, sync=None, trace=None):
    """windows: [(end_block, flags, (IE, QE, IP, QP, IL, QL))] of one launch in slot order, not filtered; s: the state as a dict
    (Python ints, np.float32 for the three floats), advanced in place; sync: the channel's sync state as a one-element view (written
    on a re-arm) or None; trace: a list that gets (end_block, locked, K, code_ratio, car_ratio, snr, flags after) per epoch
    -> the record as a dict"""
    seen = s["blocks_seen"]
    ev = dict(flags=0, n_epochs=0)
    for end_block, flags, iq in windows:
        if not (flags & WSYNC_WINDOW and 0 <= end_block < n_blocks):
            continue
        ie, qe, ip, qp, il, ql = (int(v) for v in iq)
        if max(abs(v) for v in (ie, qe, ip, qp, il, ql)) >= RANGE:          # 1: range
            s["n_range"] = (s["n_range"] + 1) & M32
            ev["flags"] |= F_RANGE
            continue
        locked = bool(flags & WSYNC_LOCKED)
        if not locked:                                                  # 2: a SEARCH window
            if s["flags"] & F_CARRIER:
                s["flags"] &= ~F_CARRIER
                s["n_lost_carrier"] = (s["n_lost_carrier"] + 1) & M32
                ev["flags"] |= F_LOST_CARRIER
            s["car_good"] = s["car_bad"] = s["false_run"] = 0
        if s["epoch_n"] > 0 and bool(s["flags"] & F_OPEN_LOCKED) != locked:    # 3: the open epoch's kind
            _clear_epoch(s)
        s["flags"] = s["flags"] | F_OPEN_LOCKED if locked else s["flags"] & ~F_OPEN_LOCKED
        s["sum_a"] += abs(ip)                                           # 4: the sums
        s["sum_p"] += ip * ip + qp * qp
        s["sum_d"] += ip * ip - qp * qp
        s["sum_e"] += ie * ie + qe * qe
        s["sum_l"] += il * il + ql * ql
        s["epoch_n"] += 1
        if s["epoch_n"] < (cfg["epoch_lock"] if locked else cfg["epoch_search"]):
            continue
        k = s["epoch_n"]                                                # 5: the epoch's end
        code_ratio, car_ratio, snr = ratios(k, s["sum_a"], s["sum_p"], s["sum_d"], s["sum_e"], s["sum_l"])
        s["last_code_ratio"], s["last_car_ratio"], s["last_snr"], s["last_p"], s["last_k"] = code_ratio, car_ratio, snr, s["sum_p"], k
        s["last_epoch_end_p1"] = seen + end_block + 1
        s["flags"] = s["flags"] | F_EPOCH_LOCKED if locked else s["flags"] & ~F_EPOCH_LOCKED
        ev["n_epochs"] += 1
        if _verdict(s, ev, bool(code_ratio >= cfg["code_min"]), "code_good", "code_bad", F_CODE, "n_lost_code", F_LOST_CODE, cfg) and cfg["rearm"] & 1:
            s["flags"] |= F_PENDING
        if locked:
            good = bool(car_ratio >= cfg["car_min"] and snr >= cfg["snr_min"])
            was = bool(s["flags"] & F_CARRIER)
            _verdict(s, ev, good, "car_good", "car_bad", F_CARRIER, "n_lost_carrier", F_LOST_CARRIER, cfg)
            s["false_run"] = 0 if good or was else (s["false_run"] + 1) & M32
            if not good and not was and cfg["rearm"] & 2 and s["false_run"] >= cfg["patience"]:
                s["flags"] |= F_PENDING
                s["false_run"] = 0
        _clear_epoch(s)
        if trace is not None:
            trace.append((end_block, locked, k, float(code_ratio), float(car_ratio), float(snr), s["flags"]))
    # the launch's end
    s["blocks_seen"] = b = seen + n_blocks
    if s["flags"] & F_PENDING:
        if cfg["rearm"] != 0 and int(sync["mode"][0]) == SYNC_LOCKED:
            sync["mode"], sync["search_n"], sync["prev_best_p1"] = SYNC_SEARCH, 0, 0
            sync["win_iq"], sync["win_n"], sync["bit_ip"] = 0, 0, 0
            sync["loop"]["n_updates"] = 0
            ev["flags"] |= F_REARMED
            s["n_rearm"] = (s["n_rearm"] + 1) & M32
            s["flags"] &= ~(F_CODE | F_CARRIER | F_OPEN_LOCKED)
            s["code_good"] = s["code_bad"] = s["car_good"] = s["car_bad"] = s["false_run"] = 0
            _clear_epoch(s)
        s["flags"] &= ~F_PENDING
    have = s["last_k"] != 0
    return dict(flags=(s["flags"] & OUT_FLAGS) | ev["flags"], n_epochs=ev["n_epochs"], last_k=s["last_k"],
                age_blocks=max(0, min(b - s["last_epoch_end_p1"], (1 << 31) - 1)) if have else -1, code_ratio=s["last_code_ratio"],
                car_ratio=s["last_car_ratio"], snr=s["last_snr"], n_range=s["n_range"], p=s["last_p"], n_lost_code=s["n_lost_code"],
                n_lost_carrier=s["n_lost_carrier"], n_rearm=s["n_rearm"], reserved=0)


def _state_dict(states, ch):
    return {name: (np.float32(states[name][ch]) if name in FLOATS else int(states[name][ch])) for name in STATE_DTYPE.names}


def run(rec, n_blocks, states, cfg, sync_states=None, channels=None, traces=None):
    """one launch: rec [n_slots][n_ch] (the sync loop's records: fields w.iq, end_block, flags), states a STATE_DTYPE array advanced
    in place, sync_states the sync loop's state array (weighted_sync_ref.STATE_DTYPE; needed when cfg's rearm is not 0, written on a
    re-arm), traces: {channel: list} that get the epochs -> (LOCK_DTYPE [n_ch], the BAD channels)"""
    assert states.dtype == STATE_DTYPE and 1 <= n_blocks <= 4096 and 1 <= rec.shape[0] <= n_blocks and rec.shape[1] == len(states)
    assert cfg["rearm"] == 0 or (sync_states is not None and len(sync_states) == len(states))
    lock = np.zeros(len(states), LOCK_DTYPE)
    bad = []
    for ch in (range(len(states)) if channels is None else channels):
        s = _state_dict(states, ch)
        if not state_valid(s):
            bad.append(ch)
            lock["age_blocks"][ch] = -1
            continue
        col = rec[:, ch]
        o = channel(list(zip(col["end_block"].tolist(), col["flags"].tolist(), col["w"]["iq"].tolist())), s, n_blocks, cfg,
                    None if sync_states is None else sync_states[ch:ch + 1], None if traces is None else traces.setdefault(ch, []))
        for name in STATE_DTYPE.names:
            states[name][ch] = s[name]
        for name in LOCK_DTYPE.names:
            lock[name][ch] = o[name]
    return lock, bad


def cn0_dbhz(lock, n_coh_lock):
    """gpsx_wlock_cn0_dbhz: the double logarithm, stored as float32"""
    lock = np.atleast_1d(lock)
    out = np.zeros(len(lock), np.float32)
    for i in range(len(lock)):
        snr = float(lock["snr"][i])
        if int(lock["flags"][i]) & F_EPOCH_LOCKED and int(lock["last_k"][i]) > 0 and snr > 0.0:
            out[i] = np.float32(10.0 * math.log10(snr / (n_coh_lock * 0.001)))
    return out
