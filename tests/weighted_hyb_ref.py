"""An exact CPU restatement of the weighted two-bit grid over n_seg coherent windows of n_coh blocks each, the windows' magnitudes
summed (include/gpsx.h gpsx_acq_grid_weighted_hyb), for the tests: per segment weighted_coh_ref's pre-sum from the segment's own
first block (the NCO accumulator from 0 there, chained through the segment's blocks), ONE circular correlation with the +-1
replica as a float64 FFT (|I| <= 981 120 < 2^20: rounding is exact), weighted_ms_ref's exact integer roots, the roots summed over
the segments in int64, then weighted_ms_ref's fold."""
import numpy as np

import weighted_coh_ref as R
import weighted_ms_ref as W

SAMPLES = W.SAMPLES


def energy(oracle, blocks_2bit, first, n_coh, n_seg, prn, freq_hz, use_magnitude=True, rep=None):
    """E(tau) = sum_j floor(sqrt(I_j^2 + Q_j^2)) of the search whose first block is `first`"""
    rep = W.replica_fft(oracle, prn) if rep is None else rep
    e = np.zeros(SAMPLES, np.int64)
    for j in range(n_seg):
        i, q = R.iq(oracle, blocks_2bit, first + j * n_coh, n_coh, prn, freq_hz, use_magnitude, rep)
        e += W.isqrt(i * i + q * q)
    return e


def grid(oracle, blocks_2bit, n_search, prns, n_coh, n_seg, dopp_min_hz, dopp_step_hz, n_dopp, use_magnitude=True, stride=None,
         if_hz=4092000, units=None):
    """PEAK-like records [n_search][n_prn][n_dopp] (max_val, phase, sum, avr); `units`: only these (search, prn index, dopp)
    triples are computed (the others stay zero)"""
    from stm32f4_sdr_gps_amd.capi import PEAK_DTYPE
    stride = n_coh * n_seg if stride is None else stride
    prns = list(prns)
    out = np.zeros((n_search, len(prns), n_dopp), PEAK_DTYPE)
    todo = units if units is not None else [(s, p, d) for s in range(n_search) for p in range(len(prns)) for d in range(n_dopp)]
    reps, spectra = {}, {}
    for s, p, d in todo:
        if p not in reps:
            reps[p] = W.replica_fft(oracle, prns[p])
        e = np.zeros(SAMPLES, np.int64)
        for j in range(n_seg):
            key = (s * stride + j * n_coh, d)            # a segment's spectrum: its first block and the Doppler bin
            if key not in spectra:
                mi, mq = R.presum(oracle, blocks_2bit, key[0], n_coh, if_hz + dopp_min_hz + d * dopp_step_hz, use_magnitude)
                spectra[key] = np.fft.fft(mi + 1j * mq)
            z = np.fft.ifft(spectra[key] * reps[p])
            i, q = np.rint(z.real).astype(np.int64), np.rint(z.imag).astype(np.int64)
            e += W.isqrt(i * i + q * q)
        out[s, p, d] = W.fold(e)
    return out
