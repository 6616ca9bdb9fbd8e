"""k_track_epl_weighted at every launch shape (include/gpsx.h gpsx_track_epl_weighted).  The launcher picks cpw, the
channels a wave serves one after the other, from (n_ch, n_blocks) (csrc/gpsx_track_weighted_plan.hpp); the per-channel values then
travel by readlane(.., 4 c), the results are latched lane by lane, the last wave may be ragged, the last workgroup may have idle
waves, and at K > 1 a second kernel writes the accumulators.  Here: every cpw from 1 to 16, from 2 on with a ragged last wave, cpw set by the
ceil(n_ch / 4) bound at up to 4096 blocks, every spacing and weight mode on and around the circle's seam and the table's word
boundaries, every PRN row, bad channels at every place of a multi-channel wave, device calls chained on one state array without
a synchronisation, and the sign-plane step on the same states.  Every comparison is for equality, on every int32 record and
every written-back if_freq_accum, and the other state fields must come back as they went in.

The CPU restatement (tests/weighted_track_ref.py) costs ~0.75 ms per (channel, block), so at large shapes it checks a sample --
always with channel 0, the last channel, the ragged last wave, the full wave before it and every in-wave position -- and every
other channel is held by GPU-against-GPU identities that change the geometry: the same states in another order, and one K-block
call against K one-block calls and ceil(K / 4)-block pieces, which run at another cpw.  Every launch made here is a row of
tests/weighted_track_shapes.py, whose shape tests/test_track_weighted_plan.py asserts without a GPU.  The restated (channel,
block) records are counted; the last test prints the count and the file's wall time and holds the count under 200 000."""
import ctypes as C
import time

import numpy as np
import pytest

import weighted_track_ref as T
import weighted_track_shapes as S

pytestmark = pytest.mark.gpu

EINVAL = -22
PAD_PRN = -2147483648          # kTrackPadPrn: a padding channel, the empty code, not an error
BUDGET = 200_000               # restated (channel, block) records in this file
RESTATED = [0]
STARTED = [None]
FIELDS = ("prn", "code_phase_fine", "if_freq_offset_hz")

# code phases on the seam (tests/test_gpu_weighted_track.py's)
PHASES = [4321.0, 0.0, 7.9, 16367.99, 3.0, 16365.0, -3.5, 16370.2, 0.5, 14.0, 16353.0, 12007.25, 1.0, 16367.0, 15.0, 16352.5]


@pytest.fixture(scope="module")
def eng():
    from stm32f4_sdr_gps_amd import capi
    STARTED[0] = time.time()
    e = capi.Engine(0)
    yield e
    e.close()


def _rand_blocks(k, seed):
    return np.random.default_rng(seed).integers(0, 256, (k, 4092), dtype=np.uint8)


def _states(n, seed):
    """random PRNs 1 .. 210, seam and random phases, integer (every third) and fractional offsets, random accumulators, a fifth 0"""
    from stm32f4_sdr_gps_amd import capi
    rng = np.random.default_rng(seed)
    st = np.zeros(n, capi.TRK_DTYPE)
    st["prn"] = rng.integers(1, 211, n)
    st["code_phase_fine"] = rng.uniform(-20.0, 16400.0, n)
    seam = rng.permutation(n)[:min(n, 2 * len(PHASES))]            # the seam phases at random places
    st["code_phase_fine"][seam] = [PHASES[i % len(PHASES)] for i in range(len(seam))]
    st["if_freq_offset_hz"] = np.where(np.arange(n) % 3 == 0, rng.integers(-5000, 5001, n), rng.uniform(-5000.0, 5000.0, n))
    st["if_freq_accum"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    st["if_freq_accum"][rng.permutation(n)[:(n + 4) // 5]] = 0
    return st


def _restate(oracle, blocks, st, use_mag, spacing, channels=None, block_sel=None):
    return T.track(oracle, blocks, st, use_mag, spacing, channels=channels, blocks=block_sel, count=RESTATED)


def _sample(n_ch, cpw, rng, others=12):
    """channels compared with the restatement: 0, the last, every channel of the last active wave, the full wave before it,
    random others -- and, as a condition, every in-wave position 0 .. cpw - 1 (channel ch sits at position ch % cpw)"""
    first, n_last, _ = S.geometry(n_ch, cpw, -(-n_ch // (4 * cpw)))
    s = {0, n_ch - 1} | set(range(first, n_ch)) | set(range(max(first - cpw, 0), first)) | {int(c) for c in rng.integers(0, n_ch, others)}
    assert first + n_last == n_ch and {0, n_ch - 1} <= s and set(range(max(first - cpw, 0), n_ch)) <= s
    assert {c % cpw for c in s} == set(range(cpw))
    return sorted(s)


def _block_sample(k, rng, n=64):
    """all blocks up to 53; beyond: the first two, the last two and random others, n in all"""
    if k <= 53:
        return list(range(k))
    sel = {0, 1, k - 2, k - 1}
    while len(sel) < n:
        sel.add(int(rng.integers(0, k)))
    return sorted(sel)


def _equal(got, want, what):
    assert got.dtype == np.int32 and got.shape == want.shape, what
    assert np.array_equal(got, want), (what, np.argwhere(got != want)[:6].tolist())


def _state_check(after, before, acc, what):
    assert np.array_equal(after["if_freq_accum"], acc), (what, np.argwhere(after["if_freq_accum"] != acc)[:6].ravel().tolist())
    for f in FIELDS:
        assert after[f].tobytes() == before[f].tobytes(), (what, f)      # (bytes: a NaN phase must come back as it went in)


def _host_raw(eng, blocks, st, use_mag, spacing):
    """gpsx_track_epl_weighted with its return code (st is updated in place)"""
    cfg = np.array([1 if use_mag else 0, spacing], np.int32)
    blocks = np.ascontiguousarray(blocks, np.uint8).reshape(-1, 4092)
    iq = np.full((len(blocks), len(st), 6), 0x5A5A5A5A, np.int32)
    rc = eng.lib.gpsx_track_epl_weighted(eng.h, cfg.ctypes.data, blocks.ctypes.data, len(blocks), st.ctypes.data, len(st), iq.ctypes.data)
    return rc, iq


def _dev_calls(eng, blocks, st, calls, use_mag, spacing, expect_sync=0, guard=4096):
    """gpsx_track_epl_weighted_dev once per (first block, blocks) of `calls`, all on one device state array and one record array
    (a call's records start at its first block's row), NO synchronisation in between, canaries around records and states
    -> (records [K][n_ch][6], the states afterwards); expect_sync: what the first gpsx_synchronize afterwards returns"""
    from stm32f4_sdr_gps_amd import capi
    k, n = len(blocks), len(st)
    iq_bytes = k * n * 24
    h_iq = np.full(guard + iq_bytes + guard, 0xA5, np.uint8)
    h_st = np.full(guard + st.nbytes + guard, 0xA5, np.uint8)
    h_st[guard:guard + st.nbytes] = st.view(np.uint8)
    cfg = np.array([1 if use_mag else 0, spacing], np.int32)
    d_if, d_iq, d_st = eng.malloc(blocks.nbytes), eng.malloc(h_iq.nbytes), eng.malloc(h_st.nbytes)
    try:
        eng.h2d(d_if, blocks)
        eng.h2d(d_iq, h_iq)
        eng.h2d(d_st, h_st)
        eng.synchronize()
        for first, nb in calls:
            assert 0 <= first and nb >= 1 and first + nb <= k                # (the calls stay inside the arrays)
            S.tabled(n, nb)
            rc = eng.lib.gpsx_track_epl_weighted_dev(eng.h, cfg.ctypes.data, C.c_void_p(d_if + first * 4092), nb, C.c_void_p(d_st + guard),
                                                     n, C.c_void_p(d_iq + guard + first * n * 24))
            assert rc == 0, (first, nb, rc)
        assert eng.lib.gpsx_synchronize(eng.h) == expect_sync
        assert eng.lib.gpsx_synchronize(eng.h) == 0
        eng.d2h(h_iq, d_iq)
        eng.d2h(h_st, d_st)
    finally:
        for p in (d_if, d_iq, d_st):
            eng.free(p)
    for h, size in ((h_iq, iq_bytes), (h_st, st.nbytes)):
        assert (h[:guard] == 0xA5).all() and (h[guard + size:] == 0xA5).all(), "written outside the array"
    return h_iq[guard:guard + iq_bytes].view(np.int32).reshape(k, n, 6).copy(), h_st[guard:guard + st.nbytes].view(capi.TRK_DTYPE).copy()


@pytest.mark.parametrize("i", range(len(S.SHAPES)), ids=["%dx%d-cpw%d" % r[:3] for r in S.SHAPES])
def test_every_channels_per_wave_with_ragged_and_idle_waves(eng, oracle, i):
    """One shape per cpw 2 .. 16 (3 twice), each with a ragged last wave, eleven with idle waves, and the benchmark's 212 992
    channels: a sample against the restatement on all blocks, then ALL channels twice over -- the same states in a random order
    give the same records and states in that order, and the K-block call equals K one-block calls (cpw 1) and ceil(K / 4)-block
    pieces (another cpw again) on one state array, byte for byte.  Both weight modes and all fifteen spacings over the table."""
    n_ch, k, cpw = S.SHAPES[i][:3]
    assert S.tabled(n_ch, k) == cpw
    use_mag, spacing = i % 2 == 0, 1 + (7 * i) % 15
    rng = np.random.default_rng(4000 + i)
    blocks = _rand_blocks(k, 5000 + i)
    st0 = _states(n_ch, 6000 + i)
    st = st0.copy()
    whole = eng.track_epl_weighted(blocks, st, use_magnitude=use_mag, spacing=spacing)
    assert eng.lib.gpsx_last_kernel(eng.h) == b"k_track_epl_weighted"

    sample = _sample(n_ch, cpw, rng)
    bsel = _block_sample(k, rng)
    want, acc = _restate(oracle, blocks, st0, use_mag, spacing, sample, bsel)
    print("shape", (n_ch, k), "cpw", cpw, "spacing", spacing, "weighted" if use_mag else "sign only", "restated", len(sample), "channels x",
          len(bsel), "blocks")
    _equal(whole[np.ix_(bsel, sample)], want[np.ix_(bsel, sample)], ("restatement", n_ch, k, [(c, c % cpw) for c in sample][:8]))
    _state_check(st, st0, acc, ("restatement", n_ch, k))
    assert np.abs(whole).max() <= 49056 and np.count_nonzero(whole) > 0.9 * whole.size

    perm = rng.permutation(n_ch)                                            # position independence
    st2 = st0[perm].copy()
    got2 = eng.track_epl_weighted(blocks, st2, use_magnitude=use_mag, spacing=spacing)
    _equal(got2, whole[:, perm, :], ("permuted", n_ch, k))
    assert st2.tobytes() == st[perm].tobytes(), ("permuted states", n_ch, k)

    if k > 1:                                                               # K-split, at another cpw
        for step in (1, -(-k // 4)):
            assert S.tabled(n_ch, step) != cpw
            st3 = st0.copy()
            parts = []
            for b in range(0, k, step):
                S.tabled(n_ch, min(step, k - b))
                parts.append(eng.track_epl_weighted(blocks[b:b + step], st3, use_magnitude=use_mag, spacing=spacing))
            _equal(np.concatenate(parts), whole, ("split", n_ch, k, step))
            assert st3.tobytes() == st.tobytes(), ("split states", n_ch, k, step)


@pytest.mark.parametrize("row", S.FEW, ids=["%dx%d-cpw%d" % r[:3] for r in S.FEW])
def test_few_channels_many_blocks(eng, oracle, row):
    """cpw set by ceil(n_ch / 4) (61, 37, 5 and 2 channels x 4096 blocks, the documented limit) and just below it (23 x 900,
    45 x 700), on the device entry point with canaries: EVERY channel against the restatement on 64 blocks -- the first two, the
    last two, random others; block b restated from acc + b x 511 x step32, which wraps 2^32 thousands of times by the last block --
    and the whole call against eight calls of ceil(K / 8) blocks chained on the device (another cpw), byte for byte"""
    n_ch, k, cpw = row[:3]
    assert S.tabled(n_ch, k) == cpw
    use_mag, spacing = {61: (True, 15), 37: (False, 1), 5: (True, 8), 2: (False, 11), 23: (False, 4), 45: (True, 13)}[n_ch]
    rng = np.random.default_rng(7000 + n_ch)
    blocks = _rand_blocks(k, 7100 + n_ch)
    st0 = _states(n_ch, 7200 + n_ch)
    st0["if_freq_offset_hz"][0] = 4999.5
    wraps = [((k - 1) * 511 * ((oracle.nco_step(T.carrier_hz(4092000, f)) * 32) & 0xFFFFFFFF)) >> 32 for f in st0["if_freq_offset_hz"]]
    assert max(wraps) > 1000, wraps

    whole, after = _dev_calls(eng, blocks, st0, [(0, k)], use_mag, spacing)
    bsel = _block_sample(k, rng)
    assert len(bsel) == 64 and {0, 1, k - 2, k - 1} <= set(bsel)
    want, acc = _restate(oracle, blocks, st0, use_mag, spacing, None, bsel)
    print("shape", (n_ch, k), "cpw", cpw, "restated", n_ch, "channels x", len(bsel), "blocks; most wraps of 2^32:", max(wraps))
    _equal(whole[bsel], want[bsel], ("restatement", n_ch, k))
    _state_check(after, st0, acc, ("restatement", n_ch, k))

    piece = -(-k // 8)
    calls = [(b, min(piece, k - b)) for b in range(0, k, piece)]
    assert len(calls) == 8 and (S.tabled(n_ch, piece) != cpw or n_ch == 2)
    pieces, after8 = _dev_calls(eng, blocks, st0, calls, use_mag, spacing)
    assert pieces.tobytes() == whole.tobytes(), ("eight pieces", np.argwhere(pieces != whole)[:6].tolist())
    assert after8.tobytes() == after.tobytes()


TAUS = list(range(48)) + list(range(16320, 16368)) + [4095, 4096, 4097, 8191, 8192, 8193, 12287, 12288]


@pytest.mark.parametrize("use_mag", [True, False], ids=["weighted", "sign"])
@pytest.mark.parametrize("spacing", range(1, 16))
def test_seam_and_word_boundaries_at_every_spacing(eng, oracle, spacing, use_mag):
    """tau over 0 .. 47, 16320 .. 16367 and the 32-bit word boundaries in mid-table, all 15 spacings x both weight modes, one
    block, one carrier and accumulator per case, random PRNs and fractions: EVERY channel against the restatement.  Late's window
    starts at table bit t_l = -(tau + spacing) mod 16368: more than 32 consecutive tau per range, so every funnel shift 0 .. 31
    occurs (0 among them), and Early sits 30 bits on at spacing 15.  Half the cases run 8219 channels (cpw 2, ragged)."""
    n_ch = 8219 if (spacing + use_mag) % 2 == 1 else 107
    cpw = S.tabled(n_ch, 1)
    assert cpw == (2 if n_ch == 8219 else 1)
    assert {((2 * 16368 - t - spacing) % 16368) % 32 for t in TAUS} == set(range(32))
    from stm32f4_sdr_gps_amd import capi
    rng = np.random.default_rng(8000 + 2 * spacing + use_mag)
    st0 = np.zeros(n_ch, capi.TRK_DTYPE)
    taus = rng.permutation(np.resize(np.array(TAUS), n_ch))
    st0["prn"] = rng.integers(1, 211, n_ch)
    st0["code_phase_fine"] = taus + rng.integers(0, 4, n_ch) * 0.25
    st0["if_freq_offset_hz"] = np.float32(rng.uniform(-5000.0, 5000.0)) if spacing % 3 else float(rng.integers(-5000, 5001))
    st0["if_freq_accum"] = 0 if spacing % 5 == 0 else int(rng.integers(0, 1 << 32))
    assert set(taus.tolist()) == set(TAUS) and [T.tau_of(p) for p in st0["code_phase_fine"][:200]] == taus[:200].tolist()
    blocks = _rand_blocks(1, 8100 + spacing)
    want, acc = _restate(oracle, blocks, st0, use_mag, spacing)
    st = st0.copy()
    got = eng.track_epl_weighted(blocks, st, use_magnitude=use_mag, spacing=spacing)
    _equal(got, want, ("seam", spacing, use_mag, n_ch))
    _state_check(st, st0, acc, ("seam", spacing, use_mag))


def test_every_prn_row_of_the_tracking_table(eng, oracle):
    """210 channels, PRN 1 .. 210, at a mid-table phase and on the seam, against the restatement"""
    from stm32f4_sdr_gps_amd import capi
    assert S.tabled(210, 1) == 1
    blocks = _rand_blocks(1, 9000)
    for j, phase in enumerate((9000.5, 16367.0)):
        rng = np.random.default_rng(9001 + j)
        st0 = np.zeros(210, capi.TRK_DTYPE)
        st0["prn"] = np.arange(1, 211)
        st0["code_phase_fine"] = phase
        st0["if_freq_offset_hz"] = rng.uniform(-5000.0, 5000.0, 210)
        st0["if_freq_accum"] = rng.integers(0, 1 << 32, 210, dtype=np.uint64).astype(np.uint32)
        want, acc = _restate(oracle, blocks, st0, j == 0, 8)
        st = st0.copy()
        got = eng.track_epl_weighted(blocks, st, use_magnitude=j == 0, spacing=8)
        _equal(got, want, ("prn rows", phase))
        _state_check(st, st0, acc, ("prn rows", phase))
        assert got.any(axis=(0, 2)).all()


def test_every_prn_row_of_the_sign_plane_step(eng, oracle):
    """the same sweep for gpsx_track_epl_batch (k_track_epl_wave reads the same table) against the oracle's track_epl"""
    from stm32f4_sdr_gps_amd import capi, synth
    block = synth.make_if_static(1, [synth.Sat(7, 1310.0, 4321.0, 0.3, 0.4), synth.Sat(19, -2240.0, 12007.0, 0.3, 2.0)], noise_amp=1.0,
                                 seed=12)[0]
    assert block.size == 2046
    for j, phase in enumerate((9000.5, 16367.0)):
        rng = np.random.default_rng(9101 + j)
        st0 = np.zeros(210, capi.TRK_DTYPE)
        st0["prn"] = np.arange(1, 211)
        st0["code_phase_fine"] = phase
        st0["if_freq_offset_hz"] = rng.uniform(-5000.0, 5000.0, 210)
        st0["if_freq_accum"] = rng.integers(0, 1 << 32, 210, dtype=np.uint64).astype(np.uint32)
        st = st0.copy()
        iq = eng.track_epl(block, st)
        for c in range(210):
            want, acc = oracle.track_epl(block, oracle.ca_code(c + 1), float(st0["code_phase_fine"][c]), float(st0["if_freq_offset_hz"][c]),
                                         int(st0["if_freq_accum"][c]))
            assert np.array_equal(iq[c], want) and int(st["if_freq_accum"][c]) == acc, (phase, c + 1)
        for f in FIELDS:
            assert np.array_equal(st[f], st0[f]), f


BAD = [("prn", 0), ("prn", 211), ("prn", -7), ("code_phase_fine", np.nan), ("code_phase_fine", 16777216.0), ("code_phase_fine", -16777216.0)]


def test_bad_channels_inside_multi_channel_waves(eng, oracle):
    """1367 channels x 12 blocks: cpw 4, waves of channels 4 w .. 4 w + 3, a ragged last wave 1364 .. 1366.  PRN 0, 211, -7 and
    phases NaN, +-2^24, each at in-wave position 0 (the state the lanes beyond a wave's channels copy), in the middle and as the
    last channel of a full wave, a wave with nothing but bad channels, and per launch one of the six as the last channel of the
    ragged wave and another at its position 0.  The good channels' records are those of the same launch with good states in the
    bad places, channel for channel; the bad ones get zeros; every accumulator advances; GPSX_EINVAL comes back from the host
    call and from the next gpsx_synchronize after the device call.  A padding PRN alone is no error."""
    n_ch, k = 1367, 12
    assert S.tabled(n_ch, k) == 4 and S.geometry(n_ch, 4, 86) == (1364, 3, 2)
    blocks = _rand_blocks(k, 9200)
    good = _states(n_ch, 9201)
    st = good.copy()
    rc, base = _host_raw(eng, blocks, st, True, 8)
    assert rc == 0
    base_after = st
    rng = np.random.default_rng(9202)
    sample = _sample(n_ch, 4, rng, others=8)
    want, acc = _restate(oracle, blocks, good, True, 8, sample)
    _equal(base[:, sample], want[:, sample], "good states")
    _state_check(base_after, good, acc, "good states")
    assert base.any(axis=(0, 2)).all()

    for j in range(len(BAD)):
        st0 = good.copy()
        bad = {}
        for i, (field, value) in enumerate(BAD):
            bad[4 * (10 + 7 * i)] = bad[4 * (100 + 7 * i) + 1 + i % 2] = bad[4 * (200 + 7 * i) + 3] = (field, value)
        for c in range(4):
            bad[4 * 320 + c] = BAD[(j + c) % 6]                               # a wave of bad channels
        bad[1366] = BAD[j]                                                  # the last channel of the ragged wave
        if j % 2:
            bad[1364] = BAD[(j + 3) % 6]                                    # ... and its position 0; 1365 stays good
        for ch, (field, value) in bad.items():
            st0[field][ch] = value
        ok = np.array([c not in bad for c in range(n_ch)])
        st = st0.copy()
        rc, got = _host_raw(eng, blocks, st, True, 8)
        assert rc == EINVAL and eng.lib.gpsx_last_error(eng.h), j
        _equal(got[:, ok], base[:, ok], ("good channels", j))
        assert not got[:, ~ok].any(), ("bad channels", j, np.argwhere(got[:, ~ok])[:4].tolist())
        _state_check(st, st0, acc, ("host call", j))
        if j in (0, 3):
            dev, after = _dev_calls(eng, blocks, st0, [(0, k)], True, 8, expect_sync=EINVAL)
            assert dev.tobytes() == got.tobytes() and after.tobytes() == st.tobytes(), j

    for at in (1364, 1366):                                                  # the padding PRN: zeros, success
        st0 = good.copy()
        st0["prn"][at] = PAD_PRN
        st = st0.copy()
        rc, got = _host_raw(eng, blocks, st, True, 8)
        assert rc == 0, at
        ok = np.arange(n_ch) != at
        _equal(got[:, ok], base[:, ok], ("padding", at))
        assert not got[:, at].any()
        _state_check(st, st0, acc, ("padding", at))
    assert S.tabled(7, 1) == 1
    st0 = good[:7].copy()
    st0["prn"][3] = PAD_PRN
    want7, acc7 = _restate(oracle, blocks[:1], st0, True, 8)
    st = st0.copy()
    rc, got = _host_raw(eng, blocks[:1], st, True, 8)
    assert rc == 0 and not got[:, 3].any() and got[:, [0, 1, 2, 4, 5, 6]].any(axis=(0, 2)).all()
    _equal(got, want7, "padding, 7 channels")
    _state_check(st, st0, acc7, "padding, 7 channels")


def test_stream_order_of_the_accumulator(eng, oracle):
    """4099 channels (a ragged last wave at every K here): one 20-block device call (cpw 16, k_track_weighted_advance) against
    five 4-block calls (cpw 4, the advance kernel between them) and against twenty 1-block calls (the kernel's own write), each
    sequence on one state array with no synchronisation in between: records and final states byte for byte"""
    n_ch, k = 4099, 20
    assert (S.tabled(n_ch, 20), S.tabled(n_ch, 4), S.tabled(n_ch, 1)) == (16, 4, 1)
    blocks = _rand_blocks(k, 9300)
    st0 = _states(n_ch, 9301)
    whole, after = _dev_calls(eng, blocks, st0, [(0, k)], True, 8)
    sample = _sample(n_ch, 16, np.random.default_rng(9302), others=4)
    want, acc = _restate(oracle, blocks, st0, True, 8, sample)
    _equal(whole[:, sample], want[:, sample], "20 blocks")
    _state_check(after, st0, acc, "20 blocks")
    for step in (4, 1):
        got, after_s = _dev_calls(eng, blocks, st0, [(b, step) for b in range(0, k, step)], True, 8)
        assert got.tobytes() == whole.tobytes(), (step, np.argwhere(got != whole)[:6].tolist())
        assert after_s.tobytes() == after.tobytes(), step


@pytest.mark.parametrize("n_ch", [300, 8195])
def test_one_state_array_serves_both_steps(oracle, n_ch):
    """A context in the two-bit IF format: one weighted block (K = 1) and one gpsx_track_epl_batch step from the same states leave
    the same states -- if_freq_accum = acc + 511 x step32 from either, as include/gpsx.h says -- and a weighted call that follows
    the sign step is the restatement started from the accumulator the sign step left"""
    from stm32f4_sdr_gps_amd import capi, synth
    cpw = S.tabled(n_ch, 1)
    blocks = synth.make_if_static(2, [synth.Sat(7, 1310.0, 4321.0, 0.3, 0.4), synth.Sat(19, -2240.0, 12007.0, 0.3, 2.0)], noise_amp=1.0,
                                  seed=21, two_bit=True)
    st0 = _states(n_ch, 9400 + n_ch)
    st0["code_phase_fine"] = np.mod(st0["code_phase_fine"], np.float32(16368.0))   # (both steps' domain)
    e = capi.Engine(0)
    try:
        e.set_if_format(capi.IF_2BIT_SM)
        st_w, st_s = st0.copy(), st0.copy()
        e.track_epl_weighted(blocks[:1], st_w)
        e.track_epl(blocks[0], st_s)
        assert st_s.tobytes() == st_w.tobytes(), np.argwhere(st_s["if_freq_accum"] != st_w["if_freq_accum"])[:6].ravel().tolist()
        assert np.array_equal(st_w["if_freq_accum"], T.track(oracle, blocks[:1], st0, channels=[])[1])
        mid = st_s.copy()
        got = e.track_epl_weighted(blocks[1:], st_s)
    finally:
        e.close()
    sample = list(range(n_ch)) if n_ch <= 300 else _sample(n_ch, cpw, np.random.default_rng(9402), others=30)
    want, acc = _restate(oracle, blocks[1:], mid, True, 8, sample)
    _equal(got[:, sample], want[:, sample], ("after the sign step", n_ch))
    _state_check(st_s, mid, acc, ("after the sign step", n_ch))


def test_reference_budget():
    """(last in the file) the restated (channel, block) records of this file and its wall time"""
    wall = time.time() - STARTED[0] if STARTED[0] else float("nan")
    print("restated channel-blocks: %d of at most %d; wall time of the file %.1f s" % (RESTATED[0], BUDGET, wall))
    assert RESTATED[0] <= BUDGET
