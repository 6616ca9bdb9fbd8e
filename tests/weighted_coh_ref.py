"""An exact CPU restatement of the weighted two-bit grid over n_coh blocks integrated coherently (include/gpsx.h
gpsx_acq_grid_weighted_coh), for the tests: per (search, Doppler) the oracle's carrier wipe-off of each block's sign plane with the
NCO accumulator chained from block to block (oracle.wipeoff(..., accum) returns the accumulator it leaves), v in {0, +-1, +-3}
summed over the blocks sample by sample, ONE circular correlation with the +-1 replica as a float64 FFT (|I| <= 981 120 < 2^20:
rounding is exact), exact integer roots of the int64 I^2 + Q^2, then weighted_ms_ref's fold."""
import numpy as np

import weighted_ms_ref as W

SAMPLES, MIXED, BYTES_2BIT = W.SAMPLES, W.MIXED, W.BYTES_2BIT


def wiped_values(oracle, block_2bit, freq_hz, accum, use_magnitude=True):
    """vI, vQ (int64, 16368 each) of one block wiped from NCO accumulator `accum`, and the accumulator the block leaves"""
    sign, mag = W.planes(block_2bit)
    di, dq, acc_out = oracle.wipeoff(np.packbits(sign, bitorder="little"), freq_hz, accum)
    bi = np.unpackbits(di.view(np.uint8), bitorder="little")[:SAMPLES].astype(np.int64)
    bq = np.unpackbits(dq.view(np.uint8), bitorder="little")[:SAMPLES].astype(np.int64)
    w = 1 + 2 * mag.astype(np.int64) if use_magnitude else np.ones(SAMPLES, np.int64)
    vi, vq = (2 * bi - 1) * w, (2 * bq - 1) * w
    vi[MIXED:] = 0
    vq[MIXED:] = 0
    return vi, vq, acc_out


def presum(oracle, blocks_2bit, first, n_coh, freq_hz, use_magnitude=True):
    """M_I, M_Q: the n_coh blocks from `first` wiped with the accumulator chained (block 0 from 0) and added sample by sample"""
    blocks = np.asarray(blocks_2bit, np.uint8).reshape(-1, BYTES_2BIT)
    mi, mq = np.zeros(SAMPLES, np.int64), np.zeros(SAMPLES, np.int64)
    acc = 0
    for b in range(n_coh):
        vi, vq, acc = wiped_values(oracle, blocks[first + b], freq_hz, acc, use_magnitude)
        mi += vi
        mq += vq
    return mi, mq


def iq(oracle, blocks_2bit, first, n_coh, prn, freq_hz, use_magnitude=True, rep=None):
    """I(tau), Q(tau) for every fine phase: sum_b sum_n v_b[n] c[((n - tau) mod 16368) / 16]"""
    mi, mq = presum(oracle, blocks_2bit, first, n_coh, freq_hz, use_magnitude)
    rep = W.replica_fft(oracle, prn) if rep is None else rep
    z = np.fft.ifft(np.fft.fft(mi + 1j * mq) * rep)
    return np.rint(z.real).astype(np.int64), np.rint(z.imag).astype(np.int64)


def grid(oracle, blocks_2bit, n_search, prns, n_coh, dopp_min_hz, dopp_step_hz, n_dopp, use_magnitude=True, stride=None,
         if_hz=4092000, units=None):
    """PEAK-like records [n_search][n_prn][n_dopp] (max_val, phase, sum, avr); `units`: only these (search, prn index, dopp)
    triples are computed (the others stay zero)"""
    from stm32f4_sdr_gps_amd.capi import PEAK_DTYPE
    stride = n_coh if stride is None else stride
    prns = list(prns)
    out = np.zeros((n_search, len(prns), n_dopp), PEAK_DTYPE)
    todo = units if units is not None else [(s, p, d) for s in range(n_search) for p in range(len(prns)) for d in range(n_dopp)]
    reps, spectra = {}, {}
    for s, p, d in todo:
        if p not in reps:
            reps[p] = W.replica_fft(oracle, prns[p])
        if (s, d) not in spectra:
            mi, mq = presum(oracle, blocks_2bit, s * stride, n_coh, if_hz + dopp_min_hz + d * dopp_step_hz, use_magnitude)
            spectra[(s, d)] = np.fft.fft(mi + 1j * mq)
        z = np.fft.ifft(spectra[(s, d)] * reps[p])
        i, q = np.rint(z.real).astype(np.int64), np.rint(z.imag).astype(np.int64)
        out[s, p, d] = W.fold(W.isqrt(i * i + q * q))
    return out


def _pack2(sign, mag):
    """4092-byte block from sign / magnitude bits: sample n in bits 2 (n % 4), 2 (n % 4) + 1 of byte n // 4"""
    pairs = (np.asarray(sign, np.uint8) | (np.asarray(mag, np.uint8) << 1)).reshape(-1, 4)
    return (pairs[:, 0] | (pairs[:, 1] << 2) | (pairs[:, 2] << 4) | (pairs[:, 3] << 6)).astype(np.uint8)


def code_matched_blocks(oracle, prn, freq_hz, n):
    """n blocks whose wiped I samples (accumulator chained) are 3 x the replica at phase 0: I(0) = 3 x 16352 x n, the top of
    the correlation's range"""
    chip = np.repeat(oracle.ca_code(prn).astype(np.uint8), 16)
    step32 = (oracle.nco_step(freq_hz) * 32) & 0xFFFFFFFF
    out = []
    for b in range(n):
        ci, _, _ = oracle.wipeoff(np.zeros(2046, np.uint8), freq_hz, (b * 511 * step32) & 0xFFFFFFFF)
        carrier = np.unpackbits(ci.view(np.uint8), bitorder="little")[:16368]
        out.append(_pack2((1 - chip) ^ carrier, np.ones(16368, np.uint8)))
    return np.stack(out)


def hits(pk, prns, truth, n, dopp_min_hz, dopp_step_hz):
    """(capture, satellite) pairs acquired: the PRN's best Doppler bin within one bin (of this grid's step) of the true Doppler
    and its phase within 8 samples of the true code phase (test_gpu_weighted.py's rule)"""
    h = 0
    for i, p in enumerate(prns):
        dopp, delay = truth[int(p)]
        bb = pk[:, i, :]["max_val"].argmax(axis=1)
        best = pk[np.arange(n), i, bb]
        ok = (np.abs(dopp_min_hz + dopp_step_hz * bb - dopp) <= dopp_step_hz) & \
             (np.abs((best["phase"].astype(int) - delay + 8184) % 16368 - 8184) <= 8)
        h += int(ok.sum())
    return h
