"""An exact CPU restatement of the weighted two-bit grid over n_ms blocks (include/gpsx.h gpsx_acq_grid_weighted_ms), for the
tests: per (block, Doppler) the oracle's carrier wipe-off of the sign plane, v in {0, +-1, +-3}, the circular correlation with
the +-1 replica as a float64 FFT (|I| <= 49 056: rounding is exact), exact integer roots, summed over the blocks, then the
record's fold.  The oracle's own weighted grid returns the per-block fold only, which cannot be summed over blocks."""
import numpy as np

SAMPLES, MIXED, CHIPS = 16368, 16352, 1023
BYTES_2BIT = 4092


def planes(block_2bit):
    """(sign, magnitude) bits of one 4092-byte block, sample n in bits 2 (n % 4), 2 (n % 4) + 1 of byte n // 4"""
    b = np.asarray(block_2bit, np.uint8).reshape(-1)[:BYTES_2BIT]
    shifts = np.arange(4, dtype=np.uint8) * 2
    sign = ((b[:, None] >> shifts) & 1).reshape(-1).astype(np.uint8)
    mag = ((b[:, None] >> (shifts + 1)) & 1).reshape(-1).astype(np.uint8)
    return sign, mag


def wiped_values(oracle, block_2bit, freq_hz, use_magnitude=True):
    """vI, vQ (int64, 16368 each): the wiped sign x the magnitude weight, the sixteen unmixed samples 0"""
    sign, mag = planes(block_2bit)
    di, dq, _ = oracle.wipeoff(np.packbits(sign, bitorder="little"), freq_hz)
    bi = np.unpackbits(di.view(np.uint8), bitorder="little")[:SAMPLES].astype(np.int64)
    bq = np.unpackbits(dq.view(np.uint8), bitorder="little")[:SAMPLES].astype(np.int64)
    w = 1 + 2 * mag.astype(np.int64) if use_magnitude else np.ones(SAMPLES, np.int64)
    vi, vq = (2 * bi - 1) * w, (2 * bq - 1) * w
    vi[MIXED:] = 0
    vq[MIXED:] = 0
    return vi, vq


def replica_fft(oracle, prn):
    c = 1 - 2 * oracle.ca_code(int(prn)).astype(np.int64)
    return np.conj(np.fft.fft(np.repeat(c, 16).astype(np.float64)))


def iq(oracle, block_2bit, prn, freq_hz, use_magnitude=True, rep=None):
    """I(tau), Q(tau) for every fine phase: sum_n v[n] c[((n - tau) mod 16368) / 16]"""
    vi, vq = wiped_values(oracle, block_2bit, freq_hz, use_magnitude)
    rep = replica_fft(oracle, prn) if rep is None else rep
    z = np.fft.ifft(np.fft.fft(vi + 1j * vq) * rep)
    return np.rint(z.real).astype(np.int64), np.rint(z.imag).astype(np.int64)


def isqrt(e):
    e = np.asarray(e, np.int64)
    r = np.floor(np.sqrt(e.astype(np.float64))).astype(np.int64)
    r = np.where(r * r > e, r - 1, r)
    return np.where((r + 1) * (r + 1) <= e, r + 1, r)


def fold(energy):
    """one record from E[16368]: max, the smallest phase reaching it, the sum mod 2^32, sum / 16368"""
    energy = np.asarray(energy, np.int64)
    mx = int(energy.max())
    s = int(energy.sum()) % (1 << 32)
    return mx, int(np.argmax(energy)), s, s // SAMPLES


def energy(oracle, blocks_2bit, search, prn, freq_hz, n_ms, stride, use_magnitude=True, rep=None):
    blocks = np.asarray(blocks_2bit, np.uint8).reshape(-1, BYTES_2BIT)
    rep = replica_fft(oracle, prn) if rep is None else rep
    e = np.zeros(SAMPLES, np.int64)
    for b in range(n_ms):
        i, q = iq(oracle, blocks[search * stride + b], prn, freq_hz, use_magnitude, rep)
        e += isqrt(i * i + q * q)
    return e


def grid(oracle, blocks_2bit, n_search, prns, n_ms, dopp_min_hz, dopp_step_hz, n_dopp, use_magnitude=True, stride=None,
         if_hz=4092000, units=None):
    """PEAK-like records [n_search][n_prn][n_dopp] as a structured array (max_val, phase, sum, avr); `units`: only these
    (search, prn index, dopp) triples are computed (the others stay zero)"""
    from stm32f4_sdr_gps_amd.capi import PEAK_DTYPE
    stride = n_ms if stride is None else stride
    blocks = np.asarray(blocks_2bit, np.uint8).reshape(-1, BYTES_2BIT)
    prns = list(prns)
    out = np.zeros((n_search, len(prns), n_dopp), PEAK_DTYPE)
    todo = units if units is not None else [(s, p, d) for s in range(n_search) for p in range(len(prns)) for d in range(n_dopp)]
    reps = {}
    spectra = {}
    for s, p, d in todo:
        if p not in reps:
            reps[p] = replica_fft(oracle, prns[p])
        e = np.zeros(SAMPLES, np.int64)
        for b in range(n_ms):
            key = (s * stride + b, d)
            if key not in spectra:
                vi, vq = wiped_values(oracle, blocks[key[0]], if_hz + dopp_min_hz + d * dopp_step_hz, use_magnitude)
                spectra[key] = np.fft.fft(vi + 1j * vq)
            z = np.fft.ifft(spectra[key] * reps[p])
            i, q = np.rint(z.real).astype(np.int64), np.rint(z.imag).astype(np.int64)
            e += isqrt(i * i + q * q)
        out[s, p, d] = fold(e)
    return out
