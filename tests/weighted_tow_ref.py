"""An exact CPU restatement of the time-of-week aiding of the weighted path's observables (include/gpsx.h gpsx_wtow), for the tests:
the header's steps per receiver and slot, in its order.  Integers are Python integers, step 3 is explicit np.float64 operations in the
written order, the one cast to float is np.float32.  Nothing of the library's code is included or imported."""
import numpy as np

import weighted_obs_ref as O
import weighted_pred_ref as P
import weighted_sync_ref as Y

PRN_NONE = P.PRN_NONE
(T_NO_PRED, T_EMPTY, T_UNLISTED, T_BAD, T_WAITING, T_STALE, T_UNCERTAIN, T_INCONSISTENT, T_OFF_GRID, T_REARMED, T_SHIFTED, T_AIDED, T_AGREES,
 T_DISAGREES) = (1 << i for i in range(14))                                                                  # GPSX_WTOW_*
RX_NO_PRED, RX_AIDED, RX_SHIFTED, RX_DISAGREES, RX_OFF_GRID, RX_REARMED = 1, 2, 4, 8, 16, 32              # GPSX_WTOW_RX_*
FLAG_NAMES = {T_NO_PRED: "NO_PRED", T_EMPTY: "EMPTY", T_UNLISTED: "UNLISTED", T_BAD: "BAD", T_WAITING: "WAITING", T_STALE: "STALE",
              T_UNCERTAIN: "UNCERTAIN", T_INCONSISTENT: "INCONSISTENT", T_OFF_GRID: "OFF_GRID", T_REARMED: "REARMED", T_SHIFTED: "SHIFTED",
              T_AIDED: "AIDED", T_AGREES: "AGREES", T_DISAGREES: "DISAGREES"}
CFG_DTYPE = np.dtype([("max_sigma_m", "<f8"), ("max_resid_samples", "<f4"), ("ch_per_rx", "<i4"), ("max_age_blocks", "<i4"), ("resolve", "<i4"),
                      ("rearm", "<i4"), ("reserved", "<i4")])
TOW_DTYPE = np.dtype([("flags", "<u4"), ("prn_index", "<i4"), ("tx_ms", "<i8"), ("resid", "<f4"), ("m", "<i4"), ("shift", "<i4"), ("zero", "<u4")])
TOW_RX_DTYPE = np.dtype([("flags", "<u2"), ("n_aided", "u1"), ("n_agrees", "u1"), ("n_disagrees", "u1"), ("n_off_grid", "u1"), ("n_shifted", "u1"),
                         ("n_inconsistent", "u1"), ("aided_mask", "<u8"), ("agrees_mask", "<u8"), ("disagrees_mask", "<u8"), ("off_grid_mask", "<u8"),
                         ("shifted_mask", "<u8"), ("inconsistent_mask", "<u8"), ("valid_after_mask", "<u8")])
assert CFG_DTYPE.itemsize == 32 and TOW_DTYPE.itemsize == 32 and TOW_RX_DTYPE.itemsize == 64
W = O.WEEK_MS
F64 = np.float64
HALF, FULL = F64(8184.0), 16368
QUIET_NAN = np.frombuffer(np.uint32(0x7FC00000).tobytes(), np.float32)[0]


def make_cfg(ch_per_rx, max_sigma_m=300.0, max_resid_samples=8.0, max_age_blocks=40, resolve=1, rearm=0):
    """the library's gpsx_wtow_cfg_t as a one-element array"""
    cfg = np.zeros(1, CFG_DTYPE)
    for name, v in (("max_sigma_m", max_sigma_m), ("max_resid_samples", max_resid_samples), ("ch_per_rx", ch_per_rx), ("max_age_blocks", max_age_blocks),
                    ("resolve", resolve), ("rearm", rearm)):
        cfg[name] = v
    return cfg


def names(flags):
    return "|".join(n for f, n in FLAG_NAMES.items() if int(flags) & f) or "0"


def slot(c, w, s, mode):
    """steps 1 (from BAD on) .. 5 for one listed slot: c the cfg item, w its PRN's PRED_DTYPE item, s the state as weighted_obs_ref's dict,
    changed in place; mode: the sync state's, or None without cfg.rearm -> dict(flags, tx, resid, m, s, rearm)"""
    out = dict(flags=0, tx=0, resid=np.float32(0.0), m=-1, s=0)
    if not O.state_valid(s):
        return dict(out, flags=T_BAD)
    if not (s["flags"] & O.F_PHASE and s["flags"] & O.F_EDGE):
        return dict(out, flags=T_WAITING)
    if s["blocks_seen"] - s["last_win_end_p1"] > int(c["max_age_blocks"]):
        return dict(out, flags=T_STALE)
    # 2 prediction
    if not int(w["flags"]) & P.P_PREDICTED or F64(w["sigma_m"]) > F64(c["max_sigma_m"]):
        return dict(out, flags=T_UNCERTAIN)
    # 3 millisecond
    with np.errstate(all="ignore"):
        d = F64(s["last_phase"]) - F64(w["code_phase"])
        k = 1 if d > HALF else (-1 if d < -HALF else 0)
        rho = d - F64(FULL * k)
        resid = np.float32(rho)
    out["resid"] = QUIET_NAN if np.isnan(resid) else resid
    if not np.abs(rho) <= F64(c["max_resid_samples"]):
        return dict(out, flags=T_INCONSISTENT)
    tx = (int(w["tx_ms"]) % W + k) % W
    b, z = s["blocks_seen"], s["edge_block"]
    tz1 = (tx - (b % W - z % W)) % W
    m = tz1 % 20
    out.update(tx=tx, m=m)
    # 4 grid
    sh = 0
    if m != 0:
        if m in (1, 19) and s["flags"] & O.F_AMBIGUOUS and int(c["resolve"]):
            sh = -1 if m == 1 else 1
        else:
            return dict(out, flags=T_OFF_GRID | (T_REARMED if int(c["rearm"]) and mode != 0 else 0))
    z_new, tz_new = z + sh, (tz1 + sh) % W
    out["s"] = sh
    flags = T_SHIFTED if sh else 0
    # 5 anchor
    if not s["flags"] & O.F_TOW:
        s["edge_block"], s["tx_ms_at_edge"] = z_new, tz_new
        s["flags"] |= O.F_TOW
        if int(c["resolve"]):
            s["flags"] &= ~O.F_AMBIGUOUS
        return dict(out, flags=flags | T_AIDED)
    if s["tx_ms_at_edge"] == tz_new:
        if int(c["resolve"]):
            s["edge_block"] = z_new
            s["flags"] &= ~O.F_AMBIGUOUS
        return dict(out, flags=flags | T_AGREES)
    return dict(out, flags=flags | T_DISAGREES)


def run(cfg, prns, pred_rx, pred, sync, states, obs=None):
    """gpsx_wtow on pred_rx [n_rx], pred [n_rx][n_prn] (read only), sync [n_rx * ch] (Y.STATE_DTYPE), states [n_rx * ch] (O.STATE_DTYPE) and
    obs [n_rx * ch] (O.OBS_DTYPE) or None; sync, states and obs are changed in place -> (TOW_DTYPE [n_rx * ch], TOW_RX_DTYPE [n_rx])"""
    c = np.asarray(cfg, CFG_DTYPE).reshape(1)[0]
    ch, prns = int(c["ch_per_rx"]), [int(v) for v in prns]
    n_rx, n_prn = len(pred_rx), len(prns)
    assert pred.shape == (n_rx, n_prn) and len(sync) == n_rx * ch and len(states) == n_rx * ch and (obs is None or len(obs) == n_rx * ch)
    assert sync.dtype == Y.STATE_DTYPE and states.dtype == O.STATE_DTYPE and (obs is None or obs.dtype == O.OBS_DTYPE)
    tow, tow_rx = np.zeros(n_rx * ch, TOW_DTYPE), np.zeros(n_rx, TOW_RX_DTYPE)
    need = O.F_PHASE | O.F_EDGE | O.F_TOW
    for r in range(n_rx):
        if not int(pred_rx["flags"][r]) & P.RX_PREDICTED:                      # 0 receiver
            tow["flags"][r * ch:(r + 1) * ch] = T_NO_PRED
            tow_rx["flags"][r] = RX_NO_PRED
            continue
        masks = dict(aided=0, agrees=0, disagrees=0, off_grid=0, shifted=0, inconsistent=0, valid_after=0, rearmed=0)
        for j in range(ch):
            at = r * ch + j
            t = tow[at]
            prn = int(sync["loop"]["prn"][at])
            if prn == PRN_NONE or prn not in prns:                             # 1 slot
                t["flags"], t["prn_index"], t["m"] = T_EMPTY if prn == PRN_NONE else T_UNLISTED, -1, -1
                continue
            p = prns.index(prn)
            s = O._state_dict(states, at)
            before = (s["edge_block"], s["tx_ms_at_edge"], s["flags"])
            o = slot(c, pred[r, p], s, int(sync["mode"][at]) if int(c["rearm"]) else None)
            f = o["flags"]
            if f & T_REARMED:
                sync["mode"][at], sync["search_n"][at], sync["prev_best_p1"][at] = 0, 0, 0
            if (s["edge_block"], s["tx_ms_at_edge"], s["flags"]) != before:                                                  # (steps 5 and 6: only what changed is written)
                for name in ("edge_block", "tx_ms_at_edge", "flags"):
                    states[name][at] = s[name]
                if obs is not None:
                    obs["tx_ms"][at] = (s["tx_ms_at_edge"] + s["blocks_seen"] - s["edge_block"]) % W
                    obs["flags"][at] = s["flags"] | O.F_VALID
            t["flags"], t["prn_index"], t["tx_ms"], t["resid"], t["m"], t["shift"] = f, p, o["tx"], o["resid"], o["m"], o["s"]
            for name, bit in (("aided", T_AIDED), ("agrees", T_AGREES), ("disagrees", T_DISAGREES), ("off_grid", T_OFF_GRID), ("shifted", T_SHIFTED),
                              ("inconsistent", T_INCONSISTENT), ("rearmed", T_REARMED)):
                if f & bit:
                    masks[name] |= 1 << j
            if not f & T_BAD and s["flags"] & need == need:
                masks["valid_after"] |= 1 << j
        x = tow_rx[r]
        x["flags"] = ((RX_AIDED if masks["aided"] else 0) | (RX_SHIFTED if masks["shifted"] else 0) | (RX_DISAGREES if masks["disagrees"] else 0) |
                      (RX_OFF_GRID if masks["off_grid"] else 0) | (RX_REARMED if masks["rearmed"] else 0))
        for name in ("aided", "agrees", "disagrees", "off_grid", "shifted", "inconsistent"):
            x[name + "_mask"], x["n_" + name] = masks[name], bin(masks[name]).count("1")
        x["valid_after_mask"] = masks["valid_after"]
    return tow, tow_rx
