"""The single-block fine grid's epilogue on trust (k_acq_mx<0>; csrc/k_acq_mx.hip mxt_epilogue): all 64 hypotheses
of a lane take the small-radius root without a radius test, the lane's winning local key is compared once with the key of magnitude
1024, and a wave in which any lane reaches it throws its chains away and runs the group-tested code over the same accumulators.  A
wave-uniform flag -- did a winner reach magnitude 768 in this wave's previous epilogue -- sends the next epilogue down the careful
path at once.  What can go wrong: a magnitude in 1024..1181 or beyond 1182 that keeps its trusted root; a redo that keeps part of the
trusted chains (a wrong `sum`, which every hypothesis feeds); a wave that redoes next to one that does not; the flag surviving where
it must not or deciding a result.  So every record and key is compared bit for bit with the CPU oracle computed live, and every
premise -- that the input reaches the path it is meant for -- is asserted from the oracle alone, before the GPU is compared.

Every launch is one or two captures x 32 PRNs x 1-3 Doppler bins.
"""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import oracle_threads
from golden_util import IF_HZ

ORC_THREADS = oracle_threads()
FIELDS = ("max_val", "phase", "sum", "avr")
PRNS32 = np.arange(1, 33, dtype=np.uint8)
DOPP2 = dict(dopp_min_hz=-1500, dopp_step_hz=4000, n_dopp=2)
# the satellites of synth.cold_start_block: (PRN, Doppler)
COLD_START_SATS = ((3, -3210.0), (5, 912.5), (11, 4480.0), (14, 4037.0), (20, -1025.0), (30, 2018.0))
# a placed satellite: PRN 14 on the centre of a one-bin grid, carrier phase as in cold_start_block
PLACED = dict(prn=14, dopp=4000.0, phase=1.1)
DOPP_PLACED = dict(dopp_min_hz=4000, dopp_step_hz=500, n_dopp=1)
# chip offsets of the placed peaks: 127 = the last of its 128 (tile 3, wave 1), 300 (tile 9, wave 3)
PLACED_Q = (127, 300)
PLACED_T0 = (0, 1, 7, 8, 9, 15)        # the anchor epilogue, the offsets around the half switch, the last step
TRUST_RADIUS, PROVEN_RADIUS = 1024, 1182

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def monkeypatch_module():
    mp = pytest.MonkeyPatch()
    yield mp
    mp.undo()


@pytest.fixture(scope="module")
def eng(monkeypatch_module):
    """The lab library with $GPSX_ACQ_NO_SPLIT: launches of a handful of clusters stay one workgroup per cluster (k_acq_mx<0>)."""
    from stm32f4_sdr_gps_amd import capi
    monkeypatch_module.setenv("GPSX_ACQ_NO_SPLIT", "1")
    e = capi.Engine(0, lab=True)
    monkeypatch_module.delenv("GPSX_ACQ_NO_SPLIT")
    yield e
    e.close()


@pytest.fixture(scope="module")
def orc():
    from oracle import pyoracle
    return pyoracle.Oracle()


def _keys(want):
    from stm32f4_sdr_gps_amd import sharding
    return sharding.pack_keys(want["max_val"], want["phase"])


def _grid(eng, blocks, prns, two_bit=False, **kw):
    from stm32f4_sdr_gps_amd import capi
    if two_bit:
        eng.set_if_format(capi.IF_2BIT_SM)
    try:
        pk, keys = eng.acq_grid(blocks, prns, n_search=len(blocks), **kw)
    finally:
        eng.set_if_format(capi.IF_1BIT)
    assert eng.lib.gpsx_last_kernel(eng.h) == b"k_acq_mx<0>"
    return pk, keys


def _check(pk, keys, want):
    for i, w in enumerate(want):
        for f in FIELDS:
            assert np.array_equal(pk[i][f], w[f]), (i, f)
        assert np.array_equal(keys[i], _keys(w)), i


def _oracle_grid(orc, blocks, dopp):
    return [orc.acq_grid(blocks[i:i + 1], 1, PRNS32, dopp["dopp_min_hz"], dopp["dopp_step_hz"], dopp["n_dopp"], 8,
                         n_threads=ORC_THREADS, live=True) for i in range(len(blocks))]


def _one_sat(delays, two_bit=False, extra=(), seed=41, amp=0.6, **sat):
    """One capture per delay: noise as in cold_start_block (U(-1, 1)), the placed satellite at amplitude `amp` and whatever `extra`
    (PRN, ...) says at the same delay"""
    from stm32f4_sdr_gps_amd import synth
    s = dict(PLACED, **sat)
    caps = [synth.make_if_static(1, [synth.Sat(p, s["dopp"], float(d), amp, s["phase"]) for p in (s["prn"],) + tuple(extra)],
                                 noise_amp=1.0, seed=seed, two_bit=two_bit) for d in delays]
    return np.concatenate(caps)


def _cell_energy(orc, block, prn, freq_hz, win=(0, 2046)):
    """The oracle's magnitudes of one (PRN, bin): [8 bit shifts][2046 byte offsets], and the triplets"""
    code = orc.ca_code(int(prn))

    def job(b):
        return orc.search_job(block, 1, code, float(IF_HZ + freq_hz), b, win[0], win[1], want_energy=True)[:2]
    with ThreadPoolExecutor(8) as pool:
        res = list(pool.map(job, range(8)))
    return np.stack([e for _, e in res]), [p for p, _ in res]


# ---- 1. the threshold band ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def band(orc):
    """cold_start_block(2, seed 11) at amp_scale 0.5, per satellite its three nearest bins of the 500 Hz grid, all 32 PRNs:
    (sign captures, 2-bit captures, {satellite index: (grid, oracle triplets per capture)}), computed when first asked for"""
    from stm32f4_sdr_gps_amd import synth
    sign = synth.cold_start_block(2, seed=11, amp_scale=0.5)
    two = synth.cold_start_block(2, seed=11, amp_scale=0.5, two_bit=True)
    want = {}

    def get(k):
        if k not in want:
            centre = int(round(COLD_START_SATS[k][1] / 500.0)) * 500
            dopp = dict(dopp_min_hz=centre - 500, dopp_step_hz=500, n_dopp=3)
            want[k] = (dopp, _oracle_grid(orc, sign, dopp))
        return want[k]
    return sign, two, get


def test_threshold_band_premise(band):
    """Among the satellites' own cells there is a maximum just below the limit, one between the limit and the end of the small path's
    proven range, and one beyond it."""
    _, _, get = band
    tops = []
    for k, (prn, _) in enumerate(COLD_START_SATS):
        for w in get(k)[1]:
            tops += w["max_val"][prn - 1].max(axis=1).tolist()          # per bin, over the eight bit shifts
    assert any(960 <= v < TRUST_RADIUS for v in tops), sorted(tops)
    assert any(TRUST_RADIUS <= v < PROVEN_RADIUS for v in tops), sorted(tops)
    assert any(v >= PROVEN_RADIUS for v in tops), sorted(tops)


@pytest.mark.parametrize("two_bit", [False, True], ids=["sign", "two_bit"])
@pytest.mark.parametrize("k", range(len(COLD_START_SATS)), ids=["prn%d" % p for p, _ in COLD_START_SATS])
def test_threshold_band(eng, band, k, two_bit):
    """All 32 PRNs in the launch: the waves that hold the satellite's peak redo, the other waves of the workgroup do not."""
    sign, two, get = band
    dopp, want = get(k)
    pk, keys = _grid(eng, two if two_bit else sign, PRNS32, two_bit=two_bit, **dopp)
    _check(pk, keys, want)


# ---- 2. placed peaks ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t0", PLACED_T0)
def test_placed_peak(eng, orc, t0):
    """One satellite, its peak at sample offset t0 of chip offsets 127 and 300 (two captures): the first epilogue at or above the
    limit is the anchor's (t0 = 0, no flag yet), falls around the even-to-odd switch, or is the last step's."""
    blocks = _one_sat([16 * q + t0 for q in PLACED_Q])
    for i, q in enumerate(PLACED_Q):
        energy, peaks = _cell_energy(orc, blocks[i:i + 1], PLACED["prn"], PLACED["dopp"])
        assert max(p["max_val"] for p in peaks) >= PROVEN_RADIUS
        assert int((energy >= TRUST_RADIUS).sum()) >= 2
        b, o = np.unravel_index(int(np.argmax(energy)), energy.shape)
        assert 8 * int(o) + int(b) == 16 * q + t0                        # the peak is where it was placed
    pk, keys = _grid(eng, blocks, PRNS32, **DOPP_PLACED)
    _check(pk, keys, _oracle_grid(orc, blocks, DOPP_PLACED))


def test_two_peaks_in_one_wave(eng, orc):
    """PRNs 3 and 5 at the same delay: two lanes of one wave at or above the limit in the same epilogues."""
    blocks = _one_sat([16 * 700 + 5], prn=3, extra=(5,), seed=43)
    want = _oracle_grid(orc, blocks, DOPP_PLACED)
    for prn in (3, 5):
        assert int(want[0]["max_val"][prn - 1].max()) >= PROVEN_RADIUS
        assert set((want[0]["phase"][prn - 1, 0] // 2).tolist()) <= {700, 701}
    pk, keys = _grid(eng, blocks, PRNS32, **DOPP_PLACED)
    _check(pk, keys, want)


@pytest.mark.parametrize("stop", [600, 601], ids=["even_stop", "odd_stop"])
def test_peak_one_byte_offset_outside_the_window(eng, orc, stop):
    """The peak in the last bit shift of byte offset `stop`, the first one outside the window (200, stop): its start value clips it,
    and with nothing at or above the limit inside the window the trust path stays on the small path.  An odd stop cuts chip offset
    300 between its two byte offsets (the half switch's edge term).  Amplitude 0.35: the last sample offset inside the window is
    half a chip from the peak and keeps about half of it -- at 0.6 (a peak of 2700) that alone is beyond the limit, and the premise
    -- below 1024 inside the window, beyond 1182 without it -- could not hold."""
    from stm32f4_sdr_gps_amd import capi
    win = (200, stop)
    blocks = _one_sat([8 * stop + 7], amp=0.35)
    _, whole = _cell_energy(orc, blocks, PLACED["prn"], PLACED["dopp"])
    assert max(p["max_val"] for p in whole) >= PROVEN_RADIUS
    codes = [orc.ca_code(int(p)) for p in PRNS32]

    def job(pb):
        p, b = pb
        peak = orc.search_job(blocks, 1, codes[p], float(IF_HZ + PLACED["dopp"]), b, win[0], win[1])[0]
        return tuple(peak[f] for f in FIELDS)
    cells = [(p, b) for p in range(32) for b in range(8)]
    with ThreadPoolExecutor(ORC_THREADS) as pool:
        res = list(pool.map(job, cells))
    want = np.zeros((32, 1, 8), capi.PEAK_DTYPE)
    for (p, b), r in zip(cells, res):
        want[p, 0, b] = r
    assert 0 < int(want["max_val"].max()) < TRUST_RADIUS
    pk, keys = _grid(eng, blocks, PRNS32, win=win, **DOPP_PLACED)
    _check(pk, keys, [want])


# ---- 3. the predictor: off, on, off -------------------------------------------------------------------------------------------------
def test_strong_launch_between_noise_launches(eng, orc):
    """A capture whose only strong PRN has its peak region inside one wave, three times, each time behind a launch of a noise-only
    capture on the same engine: the flag is per launch and per wave, nothing survives a launch."""
    from stm32f4_sdr_gps_amd import synth
    strong = _one_sat([16 * 300 + 4])
    noise = synth.make_if_static(1, [], noise_amp=1.0, seed=47)
    want_s, want_n = _oracle_grid(orc, strong, DOPP_PLACED), _oracle_grid(orc, noise, DOPP_PLACED)
    energy, _ = _cell_energy(orc, strong, PLACED["prn"], PLACED["dopp"])
    hot_q = np.unique(np.nonzero(energy >= 768)[1] // 2)
    assert int(want_s[0]["max_val"].max()) >= PROVEN_RADIUS and len(hot_q) >= 1 and set(hot_q.tolist()) <= {299, 300}   # tile 9
    others = np.delete(want_s[0]["max_val"], PLACED["prn"] - 1, axis=0)
    assert int(others.max()) < 768 and int(want_n[0]["max_val"].max()) < 768
    runs = []
    for _ in range(3):
        pk, keys = _grid(eng, noise, PRNS32, **DOPP_PLACED)
        _check(pk, keys, want_n)
        pk, keys = _grid(eng, strong, PRNS32, **DOPP_PLACED)
        _check(pk, keys, want_s)
        runs.append((pk.tobytes(), keys.tobytes()))
    assert runs[0] == runs[1] == runs[2]


# ---- 4. repeats -----------------------------------------------------------------------------------------------------------------------
def test_repeated_strong_launches_are_byte_identical(eng, orc):
    """cold_start_block(2, seed 73) at amp_scale 1.0, ten times on device-resident captures, every run into fresh, differently
    pre-filled buffers."""
    from stm32f4_sdr_gps_amd import capi, synth
    sign = synth.cold_start_block(2, seed=73, amp_scale=1.0)
    two = synth.cold_start_block(2, seed=73, amp_scale=1.0, two_bit=True)
    want = _oracle_grid(orc, sign, DOPP2)
    assert max(int(w["max_val"].max()) for w in want) >= PROVEN_RADIUS
    g = eng.grid_desc(PRNS32, n_search=2, **DOPP2)
    eng.set_if_format(capi.IF_2BIT_SM)
    d_if = eng.malloc(two.size + 2)
    try:
        eng.h2d(d_if, np.concatenate([two.reshape(-1), np.zeros(2, np.uint8)]))
        first = None
        for run in range(10):
            pk = np.zeros((2, 32, 2, 8), capi.PEAK_DTYPE)
            pk.view(np.uint8)[...] = 0x3C + 11 * run
            keys = np.full((2, 32, 2), -5 - 3 * run, np.int64)
            d_pk, d_keys = eng.malloc(pk.nbytes), eng.malloc(keys.nbytes)
            try:
                eng.h2d(d_pk, pk)
                eng.h2d(d_keys, keys)
                rc = eng.lib.gpsx_acq_grid_dev(eng.h, C.byref(g), C.c_void_p(d_if), 2, C.c_void_p(d_pk), C.c_void_p(d_keys),
                                               None, None, None)
                assert rc == 0, eng.lib.gpsx_last_error(eng.h)
                eng.synchronize()
                eng.d2h(pk, d_pk)
                eng.d2h(keys, d_keys)
            finally:
                eng.free(d_pk)
                eng.free(d_keys)
            assert eng.lib.gpsx_last_kernel(eng.h) == b"k_acq_mx<0>"
            if first is None:
                first = (pk.tobytes(), keys.tobytes())
                _check(pk, keys, want)
            else:
                assert pk.tobytes() == first[0] and keys.tobytes() == first[1], run
    finally:
        eng.free(d_if)
        eng.set_if_format(capi.IF_1BIT)
