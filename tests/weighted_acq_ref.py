"""An exact CPU restatement of the acquisition decisions and the slot hand-over (include/gpsx.h gpsx_wacq), for the tests: a weighted
grid's peak records and the slots' states in, the hand-overs written into the states, one record per receiver and one per
(receiver, PRN index) out.  Every decision is a Python integer; the hand-over's float steps are explicit np.float32 operations, one
per line, in the header's order.  Nothing of the library's kernel code is included or imported."""
import numpy as np

import weighted_eph_ref as E
import weighted_lock_ref as R
import weighted_nav_ref as N
import weighted_obs_ref as O
import weighted_sync_ref as Y

F = np.float32
SPAN = F(16368.0)
PHASES = 16368
PRN_NONE = -2147483648                                   # GPSX_PRN_NONE
DET_DETECTED, DET_TRACKED, DET_ASSIGNED, DET_DROPPED = 1, 2, 4, 8      # GPSX_WACQ_DET_*
F_ASSIGNED, F_EVICTED, F_FULL = 1, 2, 4                                # GPSX_WACQ_*
PEAK_DTYPE = np.dtype([("max_val", "<u4"), ("phase", "<u4"), ("sum", "<u4"), ("avr", "<u4")])
CFG_DTYPE = np.dtype([("ch_per_rx", "<i4"), ("det_num", "<i4"), ("det_den", "<i4"), ("min_peak", "<u4"), ("lead_blocks", "<i4"),
                      ("code_per_hz", "<f4"), ("evict_after_blocks", "<i4"), ("reserved", "<i4")])
DET_DTYPE = np.dtype([("max_val", "<u4"), ("phase", "<u4"), ("dopp_hz", "<i4"), ("flags", "u1"), ("slot", "i1"), ("zero", "<u2")])
ACQ_DTYPE = np.dtype([("flags", "<u4"), ("n_detected", "<u4"), ("n_tracked", "<u4"), ("n_assigned", "<u4"), ("n_evicted", "<u4"),
                      ("n_dropped", "<u4"), ("assigned_mask", "<u8"), ("evicted_mask", "<u8"), ("kept_mask", "<u8"), ("free_mask", "<u8"),
                      ("reserved", "<u4", (2,))])
assert CFG_DTYPE.itemsize == 32 and DET_DTYPE.itemsize == 16 and ACQ_DTYPE.itemsize == 64
# the states a hand-over touches, in the call's order
STATE_DTYPES = dict(sync=Y.STATE_DTYPE, lock=R.STATE_DTYPE, nav=N.STATE_DTYPE, obs=O.STATE_DTYPE, eph=E.STATE_DTYPE)
assert [d.itemsize for d in STATE_DTYPES.values()] == [448, 128, 64, 80, 192]


def make_cfg(ch_per_rx, det=(4, 1), min_peak=0, lead_blocks=0, code_per_hz=0.0, evict_after_blocks=0):
    return dict(ch_per_rx=int(ch_per_rx), det_num=int(det[0]), det_den=int(det[1]), min_peak=int(min_peak), lead_blocks=int(lead_blocks),
                code_per_hz=F(code_per_hz), evict_after_blocks=int(evict_after_blocks))


def cfg_record(cfg):
    """the dict as a one-element CFG_DTYPE array: the library's gpsx_wacq_cfg_t"""
    out = np.zeros(1, CFG_DTYPE)
    for k, v in cfg.items():
        out[k] = v
    return out


def best_record(row):
    """step 1 on one PRN's row of records -> (d*, M, S, tau): the LOWEST bin whose max_val is the row's greatest"""
    vals = [int(v) for v in row["max_val"]]
    m = max(vals)
    d = vals.index(m)
    return d, m, int(row["sum"][d]), int(row["phase"][d])


def detected(m, s, cfg):
    """step 2, in Python's integers"""
    return m >= max(cfg["min_peak"], 1) and m * PHASES * cfg["det_den"] >= cfg["det_num"] * s


def ratio(m, s):
    """M 16368 / S as a float, for reading (the decision never forms it); inf for S = 0"""
    return float("inf") if s == 0 else m * PHASES / s


def projected_phase(tau, dopp_hz, cfg):
    """step 5's floats -> (code_phase_fine, if_freq_offset_hz), one IEEE single operation per line"""
    f = F(int(dopp_hz))
    p = F(int(tau))
    k = F(cfg["code_per_hz"])
    if k != F(0.0) and cfg["lead_blocks"] != 0:
        per_s = F(k * f)
        span_s = F(F(cfg["lead_blocks"]) * F(0.001))
        step = F(per_s * span_s)
        p = F(p - step)
        if p < F(0.0):
            p = F(p + SPAN)
        elif p >= SPAN:
            p = F(p - SPAN)
    return p, f


def handover_state(prn, phase=F(0.0), freq=F(0.0)):
    """a slot's sync state after a hand-over (or, prn = PRN_NONE, an eviction without a successor): zero but for loop's first four"""
    st = np.zeros(1, Y.STATE_DTYPE)
    st["loop"]["prn"] = prn
    st["loop"]["code_phase_fine"] = phase
    st["loop"]["if_freq_offset_hz"] = freq
    return st[0]


def run(cfg, prns, dopp_min_hz, dopp_step_hz, peaks, sync, lock=None, nav=None, obs=None, eph=None, want_det=True, trace=None):
    """gpsx_wacq on peaks [n_rx][n_prn][n_dopp] and the states [n_rx * ch_per_rx] (lock .. eph: None for a NULL pointer), which are
    changed in place -> (ACQ_DTYPE [n_rx], DET_DTYPE [n_rx][n_prn] or None).  trace (a list): per receiver a dict of the integers the
    decisions were taken on -- best [(d*, M, S, tau)], detected / tracked / candidates [PRN indices; candidates in rank order],
    holds / evicted / kept / free [slots, before the call], assigned {PRN index: slot}, written [slots]"""
    n_rx, n_prn, n_dopp = peaks.shape
    ch = cfg["ch_per_rx"]
    assert len(prns) == n_prn and len(sync) == n_rx * ch and (cfg["evict_after_blocks"] == 0 or lock is not None)
    acq = np.zeros(n_rx, ACQ_DTYPE)
    det = np.zeros((n_rx, n_prn), DET_DTYPE) if want_det else None
    for r in range(n_rx):
        c0 = r * ch
        best = [best_record(peaks[r, p]) for p in range(n_prn)]
        is_det = [detected(m, s, cfg) for _, m, s, _ in best]
        holds = [j for j in range(ch) if int(sync["loop"]["prn"][c0 + j]) != PRN_NONE]
        evicted = [j for j in holds if cfg["evict_after_blocks"] > 0 and (int(lock["flags"][c0 + j]) & R.F_CODE) == 0
                   and int(lock["blocks_seen"][c0 + j]) >= cfg["evict_after_blocks"]]
        kept = [j for j in holds if j not in evicted]
        free = [j for j in range(ch) if j not in kept]
        kept_prns = {int(sync["loop"]["prn"][c0 + j]) for j in kept}
        tracked = [p for p in range(n_prn) if is_det[p] and int(prns[p]) in kept_prns]
        cands = sorted((p for p in range(n_prn) if is_det[p] and p not in tracked), key=lambda p: (-best[p][1], p))
        assigned = dict(zip(cands, free))                     # the k-th candidate to the k-th free slot
        dropped = cands[len(free):]
        for j in sorted(set(assigned.values()) | set(evicted)):
            who = [p for p, slot in assigned.items() if slot == j]
            if who:
                d, _, _, tau = best[who[0]]
                phase, freq = projected_phase(tau, dopp_min_hz + d * dopp_step_hz, cfg)
                sync[c0 + j] = handover_state(int(prns[who[0]]), phase, freq)
            else:
                sync[c0 + j] = handover_state(PRN_NONE)
            for other in (lock, nav, obs, eph):
                if other is not None:
                    other[c0 + j] = np.zeros(1, other.dtype)[0]
        mask = lambda slots: sum(1 << j for j in slots)       # noqa: E731
        a = acq[r]
        a["n_detected"], a["n_tracked"], a["n_assigned"], a["n_evicted"], a["n_dropped"] = sum(is_det), len(tracked), len(assigned), len(evicted), len(dropped)
        a["flags"] = (F_ASSIGNED if assigned else 0) | (F_EVICTED if evicted else 0) | (F_FULL if dropped else 0)
        a["assigned_mask"], a["evicted_mask"], a["kept_mask"] = mask(assigned.values()), mask(evicted), mask(kept)
        a["free_mask"] = mask(j for j in free if j not in assigned.values())
        if want_det:
            for p, (d, m, _, tau) in enumerate(best):
                e = det[r, p]
                e["max_val"], e["phase"], e["dopp_hz"] = m, tau, dopp_min_hz + d * dopp_step_hz
                e["flags"] = ((DET_DETECTED if is_det[p] else 0) | (DET_TRACKED if p in tracked else 0) | (DET_ASSIGNED if p in assigned else 0)
                              | (DET_DROPPED if p in dropped else 0))
                e["slot"] = assigned.get(p, -1)
        if trace is not None:
            trace.append(dict(best=best, detected=[p for p in range(n_prn) if is_det[p]], tracked=tracked, candidates=cands, holds=holds,
                              evicted=evicted, kept=kept, free=free, assigned=assigned, dropped=dropped,
                              written=sorted(set(assigned.values()) | set(evicted))))
    return acq, det
