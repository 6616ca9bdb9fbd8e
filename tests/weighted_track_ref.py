"""An exact CPU restatement of the weighted two-bit Early / Prompt / Late correlators over K blocks (include/gpsx.h
gpsx_track_epl_weighted), for the tests: per (block, channel) weighted_coh_ref.wiped_values with the NCO accumulator chained from
the channel state's, then integer dot products with the +-1 replica rolled to tau - spacing, tau, tau + spacing.  The carrier
frequency is formed in float32, np.float32(if_hz) + np.float32(offset), as the kernel forms it."""
import numpy as np

import weighted_coh_ref as R

SAMPLES = R.SAMPLES


def tau_of(code_phase_fine):
    """(int)code_phase_fine (C truncation towards zero) reduced to [0, 16368) with a non-negative remainder; None for a phase the
    call treats like a bad PRN (not finite, or magnitude >= 2^24)"""
    x = float(np.float32(code_phase_fine))
    if not np.isfinite(x) or abs(x) >= float(1 << 24):
        return None
    return int(x) % SAMPLES   # int() truncates towards zero; Python's % is non-negative for a positive modulus


def carrier_hz(if_hz, offset_hz):
    return np.float32(np.float32(if_hz) + np.float32(offset_hz))


def track(oracle, blocks_2bit, states, use_magnitude=True, spacing=8, if_hz=4092000, channels=None, blocks=None, count=None):
    """int32 [n_blocks][n_ch][6] = IE, QE, IP, QP, IL, QL and the uint32 accumulator every channel leaves.  `states`: a TRK_DTYPE
    array (not modified).  `channels`: only these are computed (the others' records stay zero; accumulators are always formed).
    `blocks`: only these blocks of the chosen channels are computed, block b wiped from the closed form acc + b x 511 x step32
    (the others' records stay zero; the accumulators returned are the whole call's either way).  `count`: a one-element list
    the number of (channel, block) records computed is added to."""
    blks = np.asarray(blocks_2bit, np.uint8).reshape(-1, R.BYTES_2BIT)
    n_blocks, n_ch = len(blks), len(states)
    out = np.zeros((n_blocks, n_ch, 6), np.int32)
    acc_out = np.zeros(n_ch, np.uint32)
    todo = set(range(n_ch) if channels is None else channels)
    which = list(range(n_blocks)) if blocks is None else sorted({int(b) for b in blocks})
    assert all(0 <= b < n_blocks for b in which)
    reps, wiped = {}, {}
    for ch in range(n_ch):
        prn, acc0 = int(states["prn"][ch]), int(states["if_freq_accum"][ch])
        f = carrier_hz(if_hz, states["if_freq_offset_hz"][ch])
        step32 = (oracle.nco_step(f) * 32) & 0xFFFFFFFF
        acc_out[ch] = (acc0 + n_blocks * 511 * step32) & 0xFFFFFFFF
        tau = tau_of(states["code_phase_fine"][ch])
        if ch not in todo or tau is None or not 1 <= prn <= 210:
            continue
        if prn not in reps:
            reps[prn] = np.repeat(1 - 2 * oracle.ca_code(prn).astype(np.int64), 16)
        rolled = [np.roll(reps[prn], (tau + d) % SAMPLES) for d in (-spacing, 0, spacing)]   # rolled[n] = c[(n - tau_k) mod 16368]
        for b in which:
            acc = (acc0 + b * 511 * step32) & 0xFFFFFFFF
            key = (b, float(f), acc)
            if key not in wiped:
                wiped[key] = R.wiped_values(oracle, blks[b], f, acc, use_magnitude)
            vi, vq, acc = wiped[key]
            assert acc == (acc0 + (b + 1) * 511 * step32) & 0xFFFFFFFF   # the wipe-off's own chaining IS the closed form
            for k in range(3):
                out[b, ch, 2 * k] = int(vi @ rolled[k])
                out[b, ch, 2 * k + 1] = int(vq @ rolled[k])
        if count is not None:
            count[0] += len(which)
    return out, acc_out


def discriminator(iq):
    """(|E| - |L|) / (|E| + |L|) with the magnitudes summed over the blocks of iq [n_blocks][6]; positive: tau is too large"""
    iq = np.asarray(iq, np.float64)
    e = np.hypot(iq[:, 0], iq[:, 1]).sum()
    late = np.hypot(iq[:, 4], iq[:, 5]).sum()
    return (e - late) / (e + late)
