"""Orbiting satellites' IF samples to a position fix on the weighted chain's CPU restatements (no GPU): weighted_sync_ref ->
weighted_nav_ref -> weighted_obs_ref + weighted_eph_ref, then the library's host helpers gpsx_wobs_pseudoranges and gpsx_weph_to_eph
and its pntpos.  What no other weighted test has: a code phase that moves -- the signal is tests/pvt_chain.py's, four satellites on
broadcast orbits, two-bit quantised -- and a solver that joins the observables' and the ephemerides' time bases (tx_ms, rx_tow_s,
toe / toc / week, the sign of the code phase in a pseudorange).  The device's partner is tests/test_gpu_weighted_pvt.py.

Cost: the stream is synthesised once (25 s on 8 CPUs) and both gain sets' chains run side by side in worker processes (eight
channel runs of 35 s each: 40 s on 8 CPUs, 160 s on two); everything else takes a second or two.  The file: 110 s on 8 CPUs.

The finding this file pins.  The weighted code loop has no carrier aiding, so its PI DLL follows the code's Doppler ramp with the
integrator alone and rests at a discriminator value of d = fd x 0.01039 / dll_c2.  With the steady gains the suite used on motionless
codes, (0.5, 40), that is 3.3 samples of code error at 2.7 kHz and loss of lock at 3.85 kHz; with (0.5, 200) it is 0.6 samples.
Measured on the restatements (tools/experiments/weighted_pvt_gains.py, EXPERIMENTS.md; hand-over + 3 samples, + 12.5 Hz), transmit-time
error at block 25 000 for fd = -2861 / +2729 / +2711 / +63 Hz, and the fix through pntpos:
  (0.5, 40)   +2.19 / -4.19 / -4.02 / -1.16 samples   124.8 m
  (0.5, 200)  -1.37 / -1.66 / -1.76 / -0.69 samples    35.1 m
With the reference's own (1, 300) the fix is 69.4 m: not kept (weighted_pvt_cases.MEASURED).  All of this is measured on the CPU
restatements; the device gives the same bytes (tests/test_gpu_weighted_pvt.py).
The largest residual against lag_model over both runs' six launch ends is 0.85 samples (bound: 1.5 x that); the receiver clock term
is 1.205 ms at an offset of 68.802 ms and 2.403 ms at 70 ms, within 0.15 us of offset - the reference channel's apparent travel
time, and the two fixes lie 1e-7 m apart."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import pvt_chain as pc
import weighted_pvt_cases as P

# sha256 of the first 40 one-bit blocks of make_if_from_orbits' default form on tests/test_gpu_pvt_chain.py's scenario, taken on the
# commit before the two-bit output was added: that test's signal has not moved
ONE_BIT_40 = "95f6b56cc101c0a2e0af021ff2978996658c8dbd4b2119ddb6aed682d5a5865d"


@pytest.fixture(scope="module")
def lib(lib_path):
    return P.solver(C.CDLL(lib_path))


@pytest.fixture(scope="module")
def chains():
    """both gain sets' chains on the restatements, with the tests' hand-over: {gains: (launches, states)}"""
    names = ("still", "moving")
    return dict(zip(names, P.chains_on_restatements([(g, P.HANDOVER) for g in names])))


def test_the_one_bit_stream_is_unchanged_and_the_two_bit_stream_has_its_signs():
    from stm32f4_sdr_gps_amd import synth
    one, first = pc.make_if_from_orbits(40, P.sats(), P.RX, P.TOW0, cycle=3)
    assert one.shape == (40, 2046) and hashlib.sha256(one.tobytes()).hexdigest() == ONE_BIT_40
    two, first2 = pc.make_if_from_orbits(40, P.sats(), P.RX, P.TOW0, cycle=3, two_bit=True)
    assert two.shape == (40, 4092) and two.dtype == np.uint8 and first2 == first
    pairs = np.unpackbits(two, axis=1, bitorder="little")
    sign, mag = pairs[:, 0::2], pairs[:, 1::2]
    assert np.array_equal(np.packbits(sign, axis=1, bitorder="little"), one)
    for b in (0, 17, 39):
        assert np.array_equal(synth.pack_2bit(sign[b], mag[b]), two[b])
    # amplitude 0.6 x 4 over uniform +-1 noise, threshold 0.6: more than half of the magnitudes are set, and not all
    assert 0.5 < mag.mean() < 0.9
    for threshold, want in ((0.0, 1.0), (10.0, 0.0)):
        other = np.unpackbits(pc.make_if_from_orbits(3, P.sats(), P.RX, P.TOW0, cycle=3, two_bit=True, mag_threshold=threshold)[0], axis=1, bitorder="little")
        assert other[:, 1::2].mean() == want and np.array_equal(other[:, 0::2], sign[:3])
    # the scenario's own stream: the signs of its first 40 blocks are the one-bit stream's at the same amplitude
    one = pc.make_if_from_orbits(40, P.sats(), P.RX, P.TOW0, amp=P.AMPLITUDE, cycle=3)[0]
    sign = np.unpackbits(P.blocks()[:40], axis=1, bitorder="little")[:, 0::2]
    assert P.blocks().shape == (P.N_BLOCKS, 4092) and np.array_equal(np.packbits(sign, axis=1, bitorder="little"), one)


def test_the_truth_and_the_lag_model():
    """truth_tx_ms against the synthesiser's own code delay at block 0; the discriminator's closed form at half a chip; the model's
    figures of the finding; the loss-of-lock frequency"""
    for (raw, row), (fd, delay) in zip(P.sats(), P.first()):
        t = P.truth_tx_ms(row, 0)
        assert abs((-t) % 1.0 * 16368.0 - delay) < 1e-3 and 60.0 < P.TOW0 * 1000.0 - t < 90.0
        assert abs(P.doppler_at(row, 0) - fd) < 1e-6
        # 100 blocks later the satellite's clock has advanced by 100 ms and the code's slide (a float64 near 4e8 ms resolves 0.001 samples)
        assert abs((P.truth_tx_ms(row, 100) - t - 100.0) * 16368.0 - fd * P.SAMPLES_PER_HZ * 0.1) < 5e-3
    for tau in (-7.5, -3.0, 0.0, 0.25, 5.0, 8.0):
        assert abs(P.discriminator(tau, 8) - 16.0 * tau / (64.0 + tau * tau)) < 1e-12
    assert abs(P.lag_model(0.0, 40.0)) < 1e-12 and abs(P.lag_model(2700.0, 40.0) - 3.28) < 0.01 and abs(P.lag_model(2700.0, 200.0) - 0.563) < 0.001
    assert abs(P.lag_model(-2700.0, 40.0) + P.lag_model(2700.0, 40.0)) < 1e-9 and abs(P.lag_model(2700.0, 300.0) - 0.374) < 0.001
    for spacing in (1, 8, 15):
        assert abs(P.discriminator(P.lag_model(1500.0, 100.0, spacing), spacing) - 1500.0 * P.SAMPLES_PER_HZ / 100.0) < 1e-9
    assert P.lag_model(3840.0, 40.0) is not None and P.lag_model(3860.0, 40.0) is None and P.lag_model(-3860.0, 40.0) is None
    assert P.lag_model(19000.0, 200.0) is not None      # (five times the range at c2 = 200)


@pytest.mark.parametrize("gains", ["still", "moving"])
def test_the_chain_holds_together(chains, gains):
    """no channel left out, every observable VALID | CONFIRMED and not AMBIGUOUS, no break, no mismatch, 25 000 blocks seen, every
    ephemeris VALID with NEW exactly once, n_sets 1 and have 7 -- and every field of every VALID ephemeris record, in every launch
    that has one, is pvt_chain.quantize's for that satellite, exactly: four rows, from samples"""
    out, st = chains[gains]
    P.check_conditions(out, st)
    assert [int(f) for f in out[0][4]["flags"]] == [3] * 4      # (the first launch: bits, but no HOW yet)
    valid_from = min(at + n for at, n, _, _, obs, _ in out if (obs["flags"] & 32).all())
    assert valid_from == 8192
    confirmed_from = min(at + n for at, n, _, _, obs, _ in out if (obs["flags"] & 8).all())
    assert confirmed_from == 16384
    assert [int(o[5]["flags"][0]) for o in out] == [0, 0, 0, 0, 0, 3, 1]


@pytest.mark.parametrize("gains", ["still", "moving"])
def test_transmit_times_lag_as_a_type_1_dll_does(chains, gains):
    """at the end of every launch from the first VALID one, code phase extrapolated over age_blocks: each channel's error minus the
    four channels' mean is -lag_model at the satellite's true Doppler, within 1.5 x the largest residual measured on these two runs
    (0.85 samples) -- which tells c2 = 40 from c2 = 200, 2.7 samples apart at 2.7 kHz.  Measured, samples (error | model | residual):
      still   25000  [ 2.19 -4.19 -4.02 -1.16] | [ 3.58 -3.31 -3.29 -0.05] | [-0.36  0.15  0.30 -0.08]
      moving  25000  [-1.37 -1.66 -1.76 -0.69] | [ 0.60 -0.57 -0.57 -0.01] | [-0.73  0.14  0.04  0.55]"""
    out, _ = chains[gains]
    worst = P.check_lag(out, gains)
    print("largest residual", worst, "of", P.MEASURED["lag_residual"], "measured; bound", P.BOUNDS["lag_residual"])
    # the other gain set's model does not fit: the test can tell the two
    other = {"still": "moving", "moving": "still"}[gains]
    rows = P.lag_table(out, other)
    assert min(float(np.abs(res).max()) for _, _, _, res in rows) > P.BOUNDS["lag_residual"]


@pytest.mark.parametrize("gains", ["still", "moving"])
def test_the_position_through_the_library(chains, lib, gains):
    """gpsx_weph_to_eph + gpsx_wobs_pseudoranges + pntpos at offsets of 68.802 and 70 ms: all four channels used, the two fixes less
    than a centimetre apart (the bound; measured: 1e-7 m), the clock term within 10 us of offset - the reference channel's apparent travel
    time (measured 0.15 us off), the epoch less the clock term on the true reception time (measured 0.19 us off; bound 1 us), and the
    error within 1.5 x the worst of the gain set's three measured hand-overs (BOUNDS).  Measured on the CPU restatements, hand-overs
    (3, 12.5) / (-3, -12.5) / (2, 7): 124.82 / 124.58 / 123.29 m with (0.5, 40) -> bound 187.2 m; 35.13 / 18.85 / 12.81 m with (0.5, 200)
    -> bound 52.7 m; clock terms 1.2054 ms at 68.802 and 2.4034 ms at 70.  This test runs the first hand-over"""
    out, _ = chains[gains]
    fixes = P.check_fixes(lib, out[-1][4], out[-1][5], gains)
    for fix, offset in zip(fixes, P.OFFSETS_MS):
        print(gains, "offset", offset, "ms: error", round(P.position_error(fix), 2), "m, clock term", fix["dtr"], "s, rx_tow_s", fix["rx_tow_s"])
    # pseudorange - c x (true apparent travel time) is one constant less each channel's own transmit-time error (as it stands in the
    # observable, not extrapolated): the sign of the code phase in a pseudorange, and the whole milliseconds
    import weighted_obs_ref as O
    obs = out[-1][4]
    raw = np.array([(O.tx_time_ms(obs[c]) - P.truth_tx_ms(row, P.N_BLOCKS)) * 16368.0 for c, (_, row) in enumerate(P.sats())])
    lags = np.array([P.lag_s(row, P.N_BLOCKS) for _, row in P.sats()])
    common = (fixes[1]["pr"] / 299792458.0 - lags) * 16.368e6 + raw
    assert np.ptp(common) < 0.01, common - common.mean()


def test_the_moving_gains_give_the_better_fix(chains, lib):
    errs = {g: P.position_error(P.position(lib, chains[g][0][-1][4], chains[g][0][-1][5], P.PRNS, 70.0)) for g in ("still", "moving")}
    assert errs["moving"] < errs["still"], errs
