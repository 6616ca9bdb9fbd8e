"""Early / Prompt / Late on weighted two-bit samples, K blocks per launch (EXTENSION, not in the reference: include/gpsx.h
gpsx_track_epl_weighted; k_track_epl_weighted on the vector ALU) against its exact CPU restatement (tests/weighted_track_ref.py,
pinned to the weighted grids' restatements in tests/test_weighted_track_reference.py).  Every comparison is for equality, on every
int32 and every written-back accumulator: records over channel counts, block counts, PRNs, weight modes, spacings, code phases on
and around the circle's seam, starting accumulators, fractional offsets and a non-default IF; one call against many; degenerate
captures; the handover from the coherent and the hybrid grid (GPU against GPU); a launch that fills the chip, with canaries; the
argument checks; bad channels; and what the call is for -- the weighted prompt's post-correlation SNR against the sign plane's."""
import ctypes as C
import math

import numpy as np
import pytest

import weighted_coh_ref as R
import weighted_track_ref as T

pytestmark = pytest.mark.gpu

EINVAL = -22


@pytest.fixture(scope="module")
def eng():
    from stm32f4_sdr_gps_amd import capi
    e = capi.Engine(0)
    yield e
    e.close()


def _blocks(n, amp=0.3, seed=3):
    from stm32f4_sdr_gps_amd import synth
    sats = [synth.Sat(7, 1310.0, 4321.0, amp, 0.4), synth.Sat(19, -2240.0, 12007.0, amp, 2.0), synth.Sat(30, 2018.0, 13000.0, amp, 4.0)]
    return synth.make_if_static(n, sats, noise_amp=1.0, seed=seed, two_bit=True)


# code phases on the seam: 0, fractions, the last sample, tau -+ spacing wrapping on either side for every spacing, and values just
# outside the circle (-3.5 -> 16365, 16370.2 -> 2)
PHASES = [4321.0, 0.0, 7.9, 16367.99, 3.0, 16365.0, -3.5, 16370.2, 0.5, 14.0, 16353.0, 12007.25, 1.0, 16367.0, 15.0, 16352.5]
PRNS = [7, 19, 30, 1, 33, 64, 150, 210, 32, 209, 5, 100]


def _states(n, seed):
    from stm32f4_sdr_gps_amd import capi
    rng = np.random.default_rng(seed)
    st = np.zeros(n, capi.TRK_DTYPE)
    st["prn"] = [PRNS[i % len(PRNS)] for i in range(n)]
    st["code_phase_fine"] = [PHASES[i % len(PHASES)] if i < 2 * len(PHASES) else rng.uniform(-20.0, 16400.0) for i in range(n)]
    st["if_freq_offset_hz"] = np.where(np.arange(n) % 3 == 0, rng.integers(-5000, 5001, n), rng.uniform(-5000.0, 5000.0, n))
    st["if_freq_offset_hz"][:3] = [1310.0, -2240.0, 2018.0][:n]
    st["if_freq_accum"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    st["if_freq_accum"][::5] = 0
    return st


def _same(got, st_after, want, acc, what):
    assert got.dtype == np.int32 and got.shape == want.shape, what
    assert np.array_equal(got, want), (what, np.argwhere(got != want)[:4].tolist())
    assert np.array_equal(st_after["if_freq_accum"], acc), (what, np.argwhere(st_after["if_freq_accum"] != acc)[:4].tolist())


# (channels, blocks, use_magnitude, spacing)
CASES = [(1, 1, True, 8), (3, 2, False, 1), (64, 20, True, 15), (257, 2, True, 8), (257, 1, False, 15), (3, 20, False, 8), (64, 1, True, 1)]


@pytest.mark.parametrize("n_ch,n_blocks,use_mag,spacing", CASES)
def test_records_match_the_reference(eng, oracle, n_ch, n_blocks, use_mag, spacing):
    blocks = _blocks(22)[:n_blocks]
    st = _states(n_ch, 100 * n_ch + n_blocks)
    want, acc = T.track(oracle, blocks, st, use_mag, spacing)
    before = st.copy()
    got = eng.track_epl_weighted(blocks, st, use_magnitude=use_mag, spacing=spacing)
    assert eng.lib.gpsx_last_kernel(eng.h) == b"k_track_epl_weighted"
    _same(got, st, want, acc, (n_ch, n_blocks, use_mag, spacing))
    for f in ("prn", "code_phase_fine", "if_freq_offset_hz"):
        assert np.array_equal(st[f], before[f]), f


def test_non_default_if(oracle):
    from stm32f4_sdr_gps_amd import capi
    blocks = _blocks(3, seed=8)
    st = _states(20, 5)
    want, acc = T.track(oracle, blocks, st, True, 8, if_hz=4_100_000)
    e = capi.Engine(0)
    try:
        e.set_config(if_hz=4_100_000)
        got = e.track_epl_weighted(blocks, st)
    finally:
        e.close()
    _same(got, st, want, acc, "if_hz")


def test_one_call_is_many_calls(eng):
    """20 blocks in one call = 20 one-block calls on the same state array = four 5-block calls: records and final accumulators"""
    blocks = _blocks(22)[:20]
    st0 = _states(40, 77)
    for use_mag, spacing in ((True, 8), (False, 3)):
        one = st0.copy()
        whole = eng.track_epl_weighted(blocks, one, use_magnitude=use_mag, spacing=spacing)
        for step in (1, 5):
            st = st0.copy()
            parts = [eng.track_epl_weighted(blocks[b:b + step], st, use_magnitude=use_mag, spacing=spacing) for b in range(0, 20, step)]
            assert np.array_equal(np.concatenate(parts), whole), (use_mag, step)
            assert st.tobytes() == one.tobytes(), (use_mag, step)


def test_degenerate_captures(eng, oracle):
    """all-0xFF, every magnitude bit set, and blocks whose wiped I is 3 x the replica: prompt I = 49 056 (the top of the range) in
    every one of the 20 blocks"""
    from stm32f4_sdr_gps_amd import capi, synth
    strong = synth.make_if_static(20, [synth.Sat(7, 1310.0, 4321.0, 4.0, 0.4)], noise_amp=0.05, seed=5, two_bit=True)
    flat = np.full_like(strong, 0xFF)
    mag_set = strong | np.uint8(0xAA)
    matched = R.code_matched_blocks(oracle, 8, 4092000 + 1310, 20)
    st0 = np.zeros(3, capi.TRK_DTYPE)
    st0[0] = (8, 0.0, 1310.0, 0)
    st0[1] = (7, 4321.0, 1310.0, 0)
    st0[2] = (8, 16364.0, 810.5, 0xDEADBEEF)
    for name, blocks in (("flat", flat), ("mag_set", mag_set), ("matched", matched)):
        for use_mag in (True, False):
            st = st0.copy()
            want, acc = T.track(oracle, blocks, st, use_mag, 8)
            got = eng.track_epl_weighted(blocks, st, use_magnitude=use_mag)
            _same(got, st, want, acc, (name, use_mag))
    got = eng.track_epl_weighted(matched, st0.copy())
    assert (got[:, 0, 2] == 49056).all(), got[:, 0, 2]


def _best(pk, d0, step):
    d = int(pk[0, 0, :]["max_val"].argmax())
    return int(pk[0, 0, d]["max_val"]), int(pk[0, 0, d]["phase"]), d0 + step * d


def _root_of_prompt_sum(iq):
    i, q = int(iq[:, 0, 2].astype(np.int64).sum()), int(iq[:, 0, 3].astype(np.int64).sum())
    return math.isqrt(i * i + q * q)


def test_a_grid_record_hands_over_exactly(eng):
    """GPU against GPU: the best record of the coherent grid (n_coh = 10) becomes a channel state -- phase -> code_phase_fine,
    bin -> if_freq_offset_hz, accumulator 0 -- and floor(sqrt((sum IP)^2 + (sum QP)^2)) over the 10 blocks IS the record's max_val
    (5486 at phase 3999, bin 4050 Hz on the CPU restatements); the hybrid grid's (n_coh = 5, n_seg = 2) is the sum of the roots of
    two 5-block calls with accumulator 0 each"""
    from stm32f4_sdr_gps_amd import capi, synth
    blocks = synth.cold_start_block(10, seed=11, amp_scale=0.03, two_bit=True)
    prns = np.array([14], np.uint8)
    max_val, phase, dopp = _best(eng.acq_grid_weighted_coh(blocks, prns, 1, 10, 3800, 50, 11), 3800, 50)
    st = np.zeros(1, capi.TRK_DTYPE)
    st[0] = (14, float(phase), float(dopp), 0)
    got = _root_of_prompt_sum(eng.track_epl_weighted(blocks, st))
    print("coherent record", max_val, "at phase", phase, "bin", dopp, "Hz; tracker", got)
    assert got == max_val

    max_val, phase, dopp = _best(eng.acq_grid_weighted_hyb(blocks, prns, 1, 5, 2, 3800, 50, 11), 3800, 50)
    roots = []
    for seg in range(2):
        st[0] = (14, float(phase), float(dopp), 0)
        roots.append(_root_of_prompt_sum(eng.track_epl_weighted(blocks[5 * seg:5 * seg + 5], st)))
    print("hybrid record", max_val, "at phase", phase, "bin", dopp, "Hz; tracker", roots)
    assert sum(roots) == max_val


def test_chip_filling_launch_with_canaries(eng, oracle):
    """65 536 channels x 4 blocks of random bytes through the device entry point: 66 sampled channels (the first and the last
    among them) against the reference on all 4 blocks, every accumulator against its closed form, and nothing written around the
    records or the state array"""
    from stm32f4_sdr_gps_amd import capi
    n, k, guard = 65536, 4, 4096
    rng = np.random.default_rng(31)
    blocks = rng.integers(0, 256, (k, 4092), dtype=np.uint8)
    st = np.zeros(n, capi.TRK_DTYPE)
    st["prn"] = (np.arange(n) % 32) + 1
    st["code_phase_fine"] = (61 * np.arange(n) % 16368).astype(np.float32)
    st["if_freq_offset_hz"] = (-5000 + 39 * (np.arange(n) % 256)).astype(np.float32)
    st["if_freq_accum"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    iq_bytes = k * n * 24
    h_iq = np.full(guard + iq_bytes + guard, 0xA5, np.uint8)
    h_st = np.full(guard + st.nbytes + guard, 0xA5, np.uint8)
    h_st[guard:guard + st.nbytes] = st.view(np.uint8)
    d_if, d_iq, d_st = eng.malloc(blocks.nbytes), eng.malloc(h_iq.nbytes), eng.malloc(h_st.nbytes)
    try:
        eng.h2d(d_if, blocks)
        eng.h2d(d_iq, h_iq)
        eng.h2d(d_st, h_st)
        cfg = np.array([1, 8], np.int32)
        eng._chk(eng.lib.gpsx_track_epl_weighted_dev(eng.h, cfg.ctypes.data, C.c_void_p(d_if), k, C.c_void_p(d_st + guard), n,
                                                     C.c_void_p(d_iq + guard)), "gpsx_track_epl_weighted_dev")
        eng.synchronize()
        eng.d2h(h_iq, d_iq)
        eng.d2h(h_st, d_st)
    finally:
        for p in (d_if, d_iq, d_st):
            eng.free(p)
    for h, size in ((h_iq, iq_bytes), (h_st, st.nbytes)):
        assert (h[:guard] == 0xA5).all() and (h[guard + size:] == 0xA5).all()
    got = h_iq[guard:guard + iq_bytes].view(np.int32).reshape(k, n, 6)
    after = h_st[guard:guard + st.nbytes].view(capi.TRK_DTYPE)
    sample = sorted({0, n - 1, 63, 64, 4095, 4096} | {int(c) for c in rng.integers(0, n, 60)})
    assert len(sample) >= 64
    want, acc = T.track(oracle, blocks, st, True, 8, channels=sample)
    assert np.array_equal(got[:, sample, :], want[:, sample, :]), np.argwhere(got[:, sample, :] != want[:, sample, :])[:4].tolist()
    assert np.array_equal(after["if_freq_accum"], acc)
    for f in ("prn", "code_phase_fine", "if_freq_offset_hz"):
        assert np.array_equal(after[f], st[f]), f
    assert np.abs(got).max() <= 49056 and np.count_nonzero(got) > 0.9 * got.size


def test_argument_checks_write_nothing(eng):
    blocks = _blocks(2)
    st0 = _states(4, 9)
    good = dict(cfg=(1, 8), null_cfg=False, null_if=False, null_st=False, null_out=False, n_blocks=2, n_ch=4)
    # every refusal with its exact text; the last row of a group fails a later clause as well: the first failing clause decides
    by_message = {
        b"null argument": [dict(null_cfg=True), dict(null_if=True), dict(null_st=True), dict(null_out=True), dict(null_if=True, n_ch=0)],
        b"unknown weights": [dict(cfg=(2, 8)), dict(cfg=(-1, 8)), dict(cfg=(2, 8), n_blocks=0), dict(cfg=(2, 0))],
        b"spacing must be 1..15 samples": [dict(cfg=(1, 0)), dict(cfg=(1, 16)), dict(cfg=(1, -8)), dict(cfg=(1, 16), n_blocks=4097)],
        b"n_blocks must be 1..4096": [dict(n_blocks=0), dict(n_blocks=-1), dict(n_blocks=4097), dict(n_blocks=0, n_ch=0)],
        b"n_ch must be at least 1": [dict(n_ch=0), dict(n_ch=-3)],
    }
    refusals = [(message, change) for message, changes in by_message.items() for change in changes]
    for fn in (eng.lib.gpsx_track_epl_weighted, eng.lib.gpsx_track_epl_weighted_dev):
        for message, change in refusals:
            a = {**good, **change}
            cfg = np.array(a["cfg"], np.int32)
            st = st0.copy()
            iq = np.full((2, 4, 6), 0xA5A5A5A5, np.uint32)
            rc = fn(eng.h, None if a["null_cfg"] else cfg.ctypes.data, None if a["null_if"] else blocks.ctypes.data, a["n_blocks"],
                    None if a["null_st"] else st.ctypes.data, a["n_ch"], None if a["null_out"] else iq.ctypes.data)
            assert rc == EINVAL and eng.lib.gpsx_last_error(eng.h) == message, (change, eng.lib.gpsx_last_error(eng.h))
            assert (iq == 0xA5A5A5A5).all() and st.tobytes() == st0.tobytes(), change
    eng.synchronize()   # nothing was enqueued, nothing is pending


def test_bad_channels(eng, oracle):
    """PRN 0, PRN 211, a NaN code phase and one of magnitude 2^24 among good channels: the good channels' records are unchanged,
    the bad ones get zeros, every accumulator is advanced, GPSX_EINVAL is reported -- by the device call at the next synchronize"""
    blocks = _blocks(3)
    st0 = _states(12, 4)
    bad = {2: ("prn", 0), 5: ("prn", 211), 7: ("code_phase_fine", np.nan), 11: ("code_phase_fine", -16777216.0), 8: ("prn", -7)}
    for ch, (field, value) in bad.items():
        st0[field][ch] = value
    want, acc = T.track(oracle, blocks, st0, True, 8)
    assert not want[:, sorted(bad), :].any() and want[:, [0, 1, 3, 4, 6, 9, 10], :].any(axis=(0, 2)).all()

    st = st0.copy()
    cfg = np.array([1, 8], np.int32)
    iq = np.full((3, 12, 6), 0x5A5A5A5A, np.int32)
    rc = eng.lib.gpsx_track_epl_weighted(eng.h, cfg.ctypes.data, blocks.ctypes.data, 3, st.ctypes.data, 12, iq.ctypes.data)
    assert rc == EINVAL and b"prn" in eng.lib.gpsx_last_error(eng.h)
    _same(iq, st, want, acc, "host call")
    good = eng.track_epl_weighted(blocks, st0[[0, 1, 3, 4, 6, 9, 10]].copy())     # the same channels without the bad ones: no error
    assert np.array_equal(good, want[:, [0, 1, 3, 4, 6, 9, 10], :])

    d_if, d_iq, d_st = eng.malloc(blocks.nbytes), eng.malloc(iq.nbytes), eng.malloc(st0.nbytes)
    try:
        eng.h2d(d_if, blocks)
        eng.h2d(d_st, st0)
        eng.synchronize()
        rc = eng.lib.gpsx_track_epl_weighted_dev(eng.h, cfg.ctypes.data, C.c_void_p(d_if), 3, C.c_void_p(d_st), 12, C.c_void_p(d_iq))
        assert rc == 0
        assert eng.lib.gpsx_synchronize(eng.h) == EINVAL
        assert eng.lib.gpsx_synchronize(eng.h) == 0
        st, iq = st0.copy(), np.zeros((3, 12, 6), np.int32)
        eng.d2h(iq, d_iq)
        eng.d2h(st, d_st)
    finally:
        for p in (d_if, d_iq, d_st):
            eng.free(p)
    _same(iq, st, want, acc, "device call")


def test_weighted_prompt_carries_more_snr_than_the_sign_plane(eng, oracle):
    """What the call is for.  200 blocks with PRN 7 at amplitude 0.05 (far below the noise), a channel at the true Doppler and
    delay and one 5000 samples off the peak, spacing 8: the ratio of the prompt powers (mean I^2 + Q^2 over the blocks) is r_w on
    weighted samples and r_s under GPSX_WEIGHTS_SIGN_ONLY.  The GPU computes the restatement's integers (asserted), on which
    r_w = 17.75 and r_s = 8.43 were calibrated; asserted: r_w >= 1.5 r_s and r_w >= 12."""
    from stm32f4_sdr_gps_amd import capi, synth
    blocks = synth.make_if_static(200, [synth.Sat(7, 1310.0, 4321.0, 0.05, 0.4), synth.Sat(19, -2240.0, 12007.0, 0.05, 2.0)],
                                  noise_amp=1.0, seed=3, two_bit=True)
    st0 = np.zeros(2, capi.TRK_DTYPE)
    st0[0] = (7, 4321.0, 1310.0, 0)
    st0[1] = (7, 4321.0 + 5000.0, 1310.0, 0)
    ratio = {}
    for use_mag in (True, False):
        st = st0.copy()
        want, acc = T.track(oracle, blocks, st, use_mag, 8)
        got = eng.track_epl_weighted(blocks, st, use_magnitude=use_mag)
        _same(got, st, want, acc, use_mag)
        p = (got[:, :, 2].astype(np.float64) ** 2 + got[:, :, 3].astype(np.float64) ** 2).mean(axis=0)
        ratio[use_mag] = p[0] / p[1]
    r_w, r_s = ratio[True], ratio[False]
    print("prompt power / off-peak power: weighted %.2f, sign plane only %.2f, ratio of (x - 1) %.2f" % (r_w, r_s, (r_w - 1) / (r_s - 1)))
    assert r_w >= 1.5 * r_s and r_w >= 12
