"""An exact CPU restatement of the weighted grid in a window around each prediction (include/gpsx.h gpsx_acq_window_weighted), for the
tests: steps 0 - 2 on the prediction records with np.rint on float64 (ties to even, one subtraction and one division), step 3 as
weighted_hyb_ref.energy -- the hybrid grid's E(tau) over all 16368 phases -- with a slice, step 4 with the grids' key, the far sum in
Python integers and the report."""
import numpy as np

import weighted_coh_ref as R
import weighted_hyb_ref as H
import weighted_ms_ref as W

SAMPLES = W.SAMPLES
SEARCHED, SKIPPED, BAD, OFF_LATTICE, CLIPPED = 1, 2, 4, 8, 16
PREDICTED, VISIBLE, TRACKED, ASSIGNED = 2, 4, 16, 32
REP_DTYPE = np.dtype([("flags", "<u4"), ("first_bin", "<i4"), ("n_bins", "<i4"), ("centre", "<i4")])
PEAK_DTYPE = np.dtype([("max_val", "<u4"), ("phase", "<u4"), ("sum", "<u4"), ("avr", "<u4")])
CFG_DTYPE = np.dtype([("n_coh", "<i4"), ("n_seg", "<i4"), ("half_width", "<i4"), ("half_bins", "<i4"), ("guard", "<i4"),
                      ("need_flags", "<u4"), ("skip_flags", "<u4"), ("reserved", "<i4")])


def make_cfg(n_coh, n_seg, half_width, half_bins, guard, need=PREDICTED | VISIBLE, skip=TRACKED | ASSIGNED):
    return dict(n_coh=n_coh, n_seg=n_seg, half_width=half_width, half_bins=half_bins, guard=guard, need_flags=need, skip_flags=skip, reserved=0)


def cfg_record(cfg):
    rec = np.zeros(1, CFG_DTYPE)
    for k, v in cfg.items():
        rec[k] = v
    return rec


def select(cfg, flags, code_phase, f_hz, dopp_min_hz, dopp_step_hz, n_dopp):
    """steps 0 - 2 of one record -> (report flags, c, d0, d1); d0 > d1 and c = 0 unless SEARCHED"""
    flags = int(flags)
    if (flags & cfg["need_flags"]) != cfg["need_flags"] or (flags & cfg["skip_flags"]) != 0:
        return SKIPPED, 0, 0, -1
    cp, f = np.float64(code_phase), np.float64(f_hz)
    if not (np.isfinite(cp) and 0.0 <= cp <= 16368.0) or not np.isfinite(f):
        return BAD, 0, 0, -1
    c = int(np.rint(cp))
    c = 0 if c == SAMPLES else c
    x = (f - np.float64(dopp_min_hz)) / np.float64(dopp_step_hz)
    if abs(x) > 2.0 ** 30:
        return OFF_LATTICE, 0, 0, -1
    dc, d = int(np.rint(x)), cfg["half_bins"]
    d0, d1 = max(dc - d, 0), min(dc + d, n_dopp - 1)
    if d0 > d1:
        return OFF_LATTICE, 0, 0, -1
    return SEARCHED | (CLIPPED if dc - d < 0 or dc + d > n_dopp - 1 else 0), c, d0, d1


def window(c, half_width):
    """the window's phases (c + j) mod 16368, j = -W .. W, in j's order"""
    return (c + np.arange(-half_width, half_width + 1)) % SAMPLES


def record(e_win, taus, guard):
    """step 4 from the window's E and phases -> (max_val, phase, sum, avr), in Python integers"""
    e = [int(v) for v in e_win]
    taus = [int(t) for t in taus]
    mx = max(e)
    phase = min(t for t, v in zip(taus, e) if v == mx) if mx else 0
    far = [v for t, v in zip(taus, e) if min(abs(t - phase), SAMPLES - abs(t - phase)) > guard]
    s = (sum(far) * SAMPLES // len(far)) % (1 << 32) if far else 0
    return mx, phase, s, s // SAMPLES


def energy(oracle, blocks_2bit, first, n_coh, n_seg, prn, freq_hz, use_magnitude, cache=None):
    """weighted_hyb_ref.energy with the segments' spectra and the replicas kept in `cache` between calls"""
    if cache is None:
        return H.energy(oracle, blocks_2bit, first, n_coh, n_seg, prn, freq_hz, use_magnitude)
    if ("rep", prn) not in cache:
        cache[("rep", prn)] = W.replica_fft(oracle, prn)
    e = np.zeros(SAMPLES, np.int64)
    for j in range(n_seg):
        key = (first + j * n_coh, n_coh, freq_hz, bool(use_magnitude))
        if key not in cache:
            mi, mq = R.presum(oracle, blocks_2bit, key[0], n_coh, freq_hz, use_magnitude)
            cache[key] = np.fft.fft(mi + 1j * mq)
        z = np.fft.ifft(cache[key] * cache[("rep", prn)])
        i, q = np.rint(z.real).astype(np.int64), np.rint(z.imag).astype(np.int64)
        e += W.isqrt(i * i + q * q)
    return e


def run(oracle, cfg, pred, blocks_2bit, prns, dopp_min_hz, dopp_step_hz, n_dopp, use_magnitude=True, stride=None, if_hz=4092000, energies=None,
        cache=None):
    """-> (PEAK_DTYPE [n_rx][n_prn][n_dopp], REP_DTYPE [n_rx][n_prn]); `energies`: a dict that takes {(r, p, d): E over the window}; E is
    weighted_hyb_ref.energy's, sliced -- or, for a caller that brings a `cache` dict, energy()'s below, which keeps the segments'
    spectra between units (tests/test_weighted_win_reference.py holds the two equal over all phases)"""
    stride = cfg["n_coh"] * cfg["n_seg"] if stride is None else stride
    prns = [int(p) for p in prns]
    n_rx = len(pred)
    peaks, rep = np.zeros((n_rx, len(prns), n_dopp), PEAK_DTYPE), np.zeros((n_rx, len(prns)), REP_DTYPE)
    for r in range(n_rx):
        for p, prn in enumerate(prns):
            rec = pred[r][p]
            flags, c, d0, d1 = select(cfg, rec["flags"], rec["code_phase"], rec["f_hz"], dopp_min_hz, dopp_step_hz, n_dopp)
            rep[r, p]["flags"] = flags
            if not flags & SEARCHED:
                continue
            rep[r, p]["first_bin"], rep[r, p]["n_bins"], rep[r, p]["centre"] = d0, d1 - d0 + 1, c
            taus = window(c, cfg["half_width"])
            for d in range(d0, d1 + 1):
                e = energy(oracle, blocks_2bit, r * stride, cfg["n_coh"], cfg["n_seg"], prn, if_hz + dopp_min_hz + d * dopp_step_hz, use_magnitude, cache)
                e_win = e[taus]
                if energies is not None:
                    energies[(r, p, d)] = e_win
                peaks[r, p, d] = record(e_win, taus, cfg["guard"])
    return peaks, rep


def make_pred(n_rx, n_prn):
    """[n_rx][n_prn] prediction records that select nothing (flags 0, slot -1)"""
    from stm32f4_sdr_gps_amd.capi import WPRED_DTYPE
    pred = np.zeros((n_rx, n_prn), WPRED_DTYPE)
    pred["slot"] = -1
    return pred


def set_pred(pred, r, p, code_phase, f_hz, flags=PREDICTED | VISIBLE | 1):
    pred[r, p]["flags"], pred[r, p]["code_phase"], pred[r, p]["f_hz"] = flags, code_phase, f_hz
