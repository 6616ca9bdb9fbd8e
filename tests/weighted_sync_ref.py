"""An exact CPU restatement of the weighted loop with a per-channel bit synchroniser and bit-aligned windows (include/gpsx.h
gpsx_track_loop_weighted_sync), for the tests: the header's seven steps per channel and block, in its order.  The correlators of a
block are weighted_track_ref.track on the state's first four fields (tau and the carrier step of the state's floats, the
accumulator as it stands); a window's update is weighted_loop_ref.update with the window's own length passed as n_coh; every
integer is a Python int, wrapped where the header says it wraps.  Nothing of the library's kernel code is included or imported."""
import numpy as np

import weighted_loop_ref as L
import weighted_track_ref as T

SEARCH, WAIT, LOCKED = 0, 1, 2
F_WINDOW, F_LOCKED, F_BIT = 1, 2, 4

STATE_DTYPE = np.dtype([("loop", L.STATE_DTYPE), ("win_iq", "<i4", 6), ("win_n", "<i4"), ("ms_count", "<i4"), ("mode", "<i4"),
                        ("edge", "<i4"), ("bit_ip", "<i4"), ("search_n", "<i4"), ("prev_best_p1", "<i4"), ("sync_rounds", "<i4"),
                        ("p_i", "<i4"), ("p_q", "<i4"), ("last_best_e", "<i8"), ("last_opp_e", "<i8"), ("zero", "<i4", 2),
                        ("base", "<i4", (20, 2)), ("e", "<i8", 20)])
REC_DTYPE = np.dtype([("w", L.REC_DTYPE), ("end_block", "<i4"), ("flags", "<u4"), ("bit_ip", "<i4")])
assert STATE_DTYPE.itemsize == 448 and REC_DTYPE.itemsize == 48 and STATE_DTYPE.fields["base"][1] == 128 and STATE_DTYPE.fields["e"][1] == 288

N_COH = (1, 2, 4, 5, 10, 20)


def make_cfg(n_coh_search, n_coh_lock, search, lock, sync_bits=20, sync_ratio=(5, 4), use_magnitude=True, spacing=8):
    """search / lock: dict(dll=(c1, c2), pll=(c1, c2), fll=c) (an n_coh key, as weighted_loop_cases' gain sets have, is ignored)"""
    assert n_coh_search in N_COH and n_coh_lock in N_COH and 1 <= sync_bits <= 200 and 1 <= sync_ratio[1] <= sync_ratio[0] <= 1024
    loop = {name: L.make_cfg(1, use_magnitude, spacing, g["dll"], g["pll"], g.get("fll", 0.0)) for name, g in (("search", search), ("lock", lock))}
    return dict(n_coh_search=int(n_coh_search), n_coh_lock=int(n_coh_lock), search=loop["search"], lock=loop["lock"], sync_bits=int(sync_bits),
                sync_num=int(sync_ratio[0]), sync_den=int(sync_ratio[1]), use_magnitude=bool(use_magnitude), spacing=int(spacing))


def slots(n_blocks, cfg):
    span = min(cfg["n_coh_search"], cfg["n_coh_lock"])
    return (n_blocks + span - 1) // span


def _i32(v):
    return ((int(v) + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def _i64(v):
    return ((int(v) + (1 << 63)) & 0xFFFFFFFFFFFFFFFF) - (1 << 63)


def _valid_floats(st):
    return T.tau_of(st["loop"]["code_phase_fine"]) is not None and 1 <= int(st["loop"]["prn"]) <= 210


def _valid_words(st):
    return (0 <= int(st["mode"]) <= 2 and 0 <= int(st["ms_count"]) <= 19 and 0 <= int(st["edge"]) <= 19 and 0 <= int(st["win_n"]) <= 20
            and 0 <= int(st["search_n"]) <= 4020)


def empty_records(n_slots, n_ch):
    rec = np.zeros((n_slots, n_ch), REC_DTYPE)
    rec["end_block"] = -1
    return rec


def run(oracle, blocks_2bit, states, cfg, if_hz=4092000, channels=None, events=None):
    """one launch over all of `blocks_2bit` on `states` (a STATE_DTYPE array, modified in place) -> REC_DTYPE [slots][n_ch].
    `channels`: only these are advanced (the others' states are left alone, their records the empty pattern).  `events`: a list
    that gets (channel, block, what, ...) tuples: ("decision", best, accepted, agreed, e_best, opp, prev_best_p1 before), ("locked",), ("bad",)."""
    blks = np.asarray(blocks_2bit, np.uint8).reshape(-1, 4092)
    assert states.dtype == STATE_DTYPE and 1 <= len(blks) <= 4096
    span = min(cfg["n_coh_search"], cfg["n_coh_lock"])
    rec = empty_records(slots(len(blks), cfg), len(states))
    todo = range(len(states)) if channels is None else sorted({int(c) for c in channels})
    with np.errstate(all="ignore"):
        for ch in todo:
            _channel(oracle, blks, states[ch:ch + 1], cfg, if_hz, rec[:, ch], span, ch, events)
    return rec


def _channel(oracle, blks, st1, cfg, if_hz, rec, span, ch, events):
    st = st1[0]                  # (a view: writes go to the array)
    loop = st["loop"]
    note = (lambda *a: events.append((ch,) + a)) if events is not None else (lambda *a: None)
    trk = np.zeros(1, L.TRK_DTYPE)
    # 1: validation at the launch's start
    bad = not (_valid_floats(st) and _valid_words(st))
    if bad:
        note(0, "bad")
    for b in range(len(blks)):
        for f in trk.dtype.names:
            trk[f][0] = loop[f]
        if bad:                  # nothing but the accumulator moves
            _, acc = T.track(oracle, blks[b:b + 1], trk, cfg["use_magnitude"], cfg["spacing"], if_hz, channels=[])
            loop["if_freq_accum"] = acc[0]
            continue
        # 2: leaving WAIT
        if int(st["mode"]) == WAIT and int(st["ms_count"]) == int(st["edge"]):
            st["mode"] = LOCKED
            note(b, "locked")
        mode = int(st["mode"])
        # 3: correlators
        iq, acc = T.track(oracle, blks[b:b + 1], trk, cfg["use_magnitude"], cfg["spacing"], if_hz, channels=[0] if mode != WAIT else [])
        if mode != WAIT:
            for k in range(6):
                st["win_iq"][k] = _i32(int(st["win_iq"][k]) + int(iq[0, 0, k]))
            st["win_n"] = int(st["win_n"]) + 1
        loop["if_freq_accum"] = acc[0]
        # 4: counter
        ms = (int(st["ms_count"]) + 1) % 20
        st["ms_count"] = ms
        # 5: search bookkeeping
        if mode == SEARCH:
            p_i, p_q = _i32(int(st["p_i"]) + int(iq[0, 0, 2])), _i32(int(st["p_q"]) + int(iq[0, 0, 3]))
            st["p_i"], st["p_q"] = p_i, p_q
            if int(st["search_n"]) >= 20:
                di, dq = _i32(p_i - int(st["base"][ms][0])), _i32(p_q - int(st["base"][ms][1]))
                st["e"][ms] = _i64(int(st["e"][ms]) + di * di + dq * dq)
            st["base"][ms] = (p_i, p_q)
            st["search_n"] = int(st["search_n"]) + 1
        # 6: window end
        if mode != WAIT and (int(st["win_n"]) >= cfg["n_coh_lock" if mode == LOCKED else "n_coh_search"] or (mode == LOCKED and ms == int(st["edge"]))):
            sums = [int(v) for v in st["win_iq"]]
            gains = dict(cfg["lock" if mode == LOCKED else "search"], n_coh=int(st["win_n"]))
            L.update(L._Scalar({name: st1["loop"][name] for name in L.STATE_DTYPE.names}), sums, gains)     # (one-element views: writes go through)
            flags, bit_out = F_WINDOW, 0
            if mode == LOCKED:
                flags |= F_LOCKED
                st["bit_ip"] = _i32(int(st["bit_ip"]) + sums[2])
                if ms == int(st["edge"]):
                    flags |= F_BIT
                    bit_out = int(st["bit_ip"])
                    st["bit_ip"] = 0
            rec[b // span] = ((sums, loop["code_phase_fine"], loop["if_freq_offset_hz"], loop["if_freq_accum"]), b, flags, bit_out)
            st["win_iq"] = 0
            st["win_n"] = 0
            if not _valid_floats(st):      # 1: validation after a window's end, for the blocks that follow
                bad = True
                note(b, "bad")
        # 7: decision
        if mode == SEARCH and int(st["search_n"]) >= 20 * (cfg["sync_bits"] + 1):
            e = [int(v) for v in st["e"]]
            best = e.index(max(e))
            opp = e[(best + 10) % 20]
            agreed = best + 1 == int(st["prev_best_p1"])
            accepted = agreed and _i64(e[best] * cfg["sync_den"]) >= _i64(opp * cfg["sync_num"])
            note(b, "decision", best, accepted, agreed, e[best], opp, int(st["prev_best_p1"]))
            st["last_best_e"], st["last_opp_e"], st["prev_best_p1"] = e[best], opp, best + 1
            st["sync_rounds"] = _i32(int(st["sync_rounds"]) + 1)
            st["e"] = 0
            st["p_i"], st["p_q"], st["search_n"] = 0, 0, 0
            if accepted:
                st["edge"], st["mode"] = best, WAIT
                st["win_iq"] = 0
                st["win_n"], st["bit_ip"] = 0, 0
                loop["n_updates"] = 0


def handover(prn, phase, offset_hz, accum=0):
    """a zeroed state with the four fields a grid record fills"""
    st = np.zeros(1, STATE_DTYPE)
    st["loop"]["prn"], st["loop"]["code_phase_fine"], st["loop"]["if_freq_offset_hz"], st["loop"]["if_freq_accum"] = prn, phase, offset_hz, accum
    return st


def bits_after_lock(rec_list):
    """[(absolute block of the bit's last block, bit_ip)] of one channel from [(first block of the launch, REC array [slots])]:
    the BIT records"""
    out = []
    for at, r in rec_list:
        for x in r:
            if int(x["flags"]) & F_BIT:
                out.append((at + int(x["end_block"]), int(x["bit_ip"])))
    return out
