"""The single-block fine grid without the quirk terms' extra K step (k_acq_mx<0>): in the fifteen recurrence passes
the term  c1022 * ca(q) + c1021 * cb(q)  rides in chip columns 1021 / 1022 of the main GEMM -- a table of code pairs per (stream,
chip offset), built next to the pass's vector, is patched into the fourth dword of the fragment that holds chips 992..1023.  A
wrong pair, a patch in the wrong lanes or tile, a pass that is patched and should not be (the half switch, the anchor) or a table
read before its barrier is a wrong triplet somewhere, so everything is compared bit for bit with the CPU oracle computed live:
noise captures in both IF formats, constant captures and a capture with its complement (the plane bits the special cases at chip
offsets 0 and 1 read take both values at every sample offset), windows around chip offsets 0, 1 and the last one, a PRN set with
empty slots, and one launch repeated.  The forms that keep the extra K step share the code: one split launch (k_acq_mx<5>) and
one two-block launch still match the oracle.

Every case is at most 2 captures x 2 Doppler bins x 32 PRNs (or one capture with a second, partial PRN set).
"""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import oracle_threads
from golden_util import IF_HZ

ORC_THREADS = oracle_threads()
FIELDS = ("max_val", "phase", "sum", "avr")
DOPP2 = dict(dopp_min_hz=-1500, dopp_step_hz=4000, n_dopp=2)
# bin 0 at 1 Hz, the lowest carrier the API admits: the NCO never leaves its first quadrant within a block, so the carrier replica
# is one constant word all along it and the wiped stream is the capture XOR a constant
ZERO_BIN_HZ = 1
DOPP_ZERO = dict(dopp_min_hz=ZERO_BIN_HZ - IF_HZ, dopp_step_hz=IF_HZ + 250, n_dopp=2)
PRNS32 = np.arange(1, 33, dtype=np.uint8)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def monkeypatch_module():
    mp = pytest.MonkeyPatch()
    yield mp
    mp.undo()


def _lab_engine(mp, **env):
    from stm32f4_sdr_gps_amd import capi
    for k, v in env.items():
        mp.setenv(k, v)
    e = capi.Engine(0, lab=True)
    for k in env:
        mp.delenv(k)
    return e


@pytest.fixture(scope="module")
def eng(monkeypatch_module):
    """The lab library with $GPSX_ACQ_NO_SPLIT: launches of a handful of clusters stay one workgroup per cluster (k_acq_mx<0>)."""
    e = _lab_engine(monkeypatch_module, GPSX_ACQ_NO_SPLIT="1")
    yield e
    e.close()


@pytest.fixture(scope="module")
def orc():
    from oracle import pyoracle
    return pyoracle.Oracle()


def _keys(want):
    from stm32f4_sdr_gps_amd import sharding
    return sharding.pack_keys(want["max_val"], want["phase"])


def _two_bit(sign_blocks, seed):
    """2-bit sign/magnitude captures with the given sign planes and random magnitude bits."""
    from stm32f4_sdr_gps_amd import synth
    rng = np.random.default_rng(seed)
    out = []
    for blk in sign_blocks:
        bits = np.unpackbits(blk, bitorder="little")
        out.append(synth.pack_2bit(bits, rng.integers(0, 2, bits.size).astype(np.uint8)))
    return np.stack(out)


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


# ---- noise captures, both IF formats ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def noise(orc):
    """amp -> (sign-plane captures [2], their 2-bit form, oracle triplets per capture)"""
    from stm32f4_sdr_gps_amd import synth
    out = {}
    for amp, seed in ((0.25, 71), (1.0, 73)):
        sign = synth.cold_start_block(2, seed=seed, amp_scale=amp)
        two = synth.cold_start_block(2, seed=seed, amp_scale=amp, two_bit=True)
        want = [orc.acq_grid(sign[i:i + 1], 1, PRNS32, DOPP2["dopp_min_hz"], DOPP2["dopp_step_hz"], 2, 8, n_threads=ORC_THREADS,
                             live=True) for i in range(2)]
        out[amp] = (sign, two, want)
    return out


@pytest.mark.parametrize("amp", [0.25, 1.0])
@pytest.mark.parametrize("two_bit", [False, True])
def test_noise_captures_vs_live_oracle(eng, noise, amp, two_bit):
    sign, two, want = noise[amp]
    pk, keys = _grid(eng, two if two_bit else sign, PRNS32, two_bit=two_bit, **DOPP2)
    _check(pk, keys, want)


# ---- the plane bits that chip offsets 0 and 1 read --------------------------------------------------------------------------------
def _plane_bits(words, t0, ks):
    """d_t0[k] = D(16 k + t0) of a wiped stream given as 16-bit words (word k = samples 16 k .. 16 k + 15, bit i = sample 16 k + i)"""
    return [(int(words[k]) >> t0) & 1 for k in ks]


@pytest.fixture(scope="module")
def extremes(orc):
    """Four captures: constant 0x00, constant 0xFF, a noise capture and its complement.
    -> (captures [4, 2046], oracle triplets per capture for DOPP_ZERO)
    The premise, by the oracle's own wipe-off: in the zero bin, d[0], d[1], d[1020] and d[1021] (entry 1022, the samples the NCO
    never mixes, is empty whatever the capture holds) take both values at every sample offset, in the I and in the Q stream, over
    each of the two pairs."""
    from stm32f4_sdr_gps_amd import synth
    caps = np.zeros((4, 2046), np.uint8)
    caps[1] = 0xFF
    caps[2] = synth.cold_start_block(1, seed=79, amp_scale=0.25)[0]
    caps[3] = ~caps[2]
    streams = [orc.wipeoff(caps[i], float(ZERO_BIN_HZ))[:2] for i in range(4)]
    for pair in ((0, 1), (2, 3)):
        for iq in range(2):
            for t0 in range(16):
                seen = {tuple(_plane_bits(streams[i][iq], t0, (0, 1, 1020, 1021))) for i in pair}
                assert len(seen) == 2 and all(a != b for a, b in zip(*seen)), (pair, iq, t0)
                assert all(_plane_bits(streams[i][iq], t0, (1022,)) == [0] for i in pair)
    want = [orc.acq_grid(caps[i:i + 1], 1, PRNS32, DOPP_ZERO["dopp_min_hz"], DOPP_ZERO["dopp_step_hz"], 2, 8,
                         n_threads=ORC_THREADS, live=True) for i in range(4)]
    return caps, want


@pytest.mark.parametrize("pair", [(0, 1), (2, 3)], ids=["constant_bytes", "capture_and_complement"])
@pytest.mark.parametrize("two_bit", [False, True])
def test_extreme_captures_vs_live_oracle(eng, extremes, pair, two_bit):
    caps, want = extremes
    blocks = caps[list(pair)]
    pk, keys = _grid(eng, _two_bit(blocks, 83) if two_bit else blocks, PRNS32, two_bit=two_bit, **DOPP_ZERO)
    _check(pk, keys, [want[i] for i in pair])


# ---- launch shapes -------------------------------------------------------------------------------------------------------------------
def _windowed(orc, block, prns, dopp, win):
    codes = [orc.ca_code(int(p)) for p in prns]
    cells = [(p, d, b) for p in range(len(prns)) for d in range(dopp["n_dopp"]) for b in range(8)]

    def job(pdb):
        p, d, b = pdb
        freq = float(IF_HZ + dopp["dopp_min_hz"] + dopp["dopp_step_hz"] * d)
        peak, _, _ = orc.search_job(block, 1, codes[p], freq, b, win[0], win[1])
        return tuple(peak[f] for f in FIELDS)
    with ThreadPoolExecutor(ORC_THREADS) as pool:
        res = list(pool.map(job, cells))
    from stm32f4_sdr_gps_amd import capi
    want = np.zeros((len(prns), dopp["n_dopp"], 8), capi.PEAK_DTYPE)
    for (p, d, b), r in zip(cells, res):
        want[p, d, b] = r
    return want


@pytest.mark.parametrize("win", [(0, 1), (1, 2045), (0, 4), (2045, 2046)])
def test_window_edges(eng, orc, extremes, win):
    """Windows that leave only chip offset 0 (its even byte offset), cut it off, hold chip offsets 0 and 1 alone, and hold the last
    byte offset alone: the folded pairs of q = 0 and q = 1 decide these results.  PRNs with all four (chip 1021, chip 1022) pairs."""
    caps, _ = extremes
    prns = np.array([1, 4, 6, 9, 16, 22, 28, 31], np.uint8)
    chips = np.stack([orc.ca_code(int(p)) for p in prns])
    assert len({(int(c[1021]), int(c[1022])) for c in chips}) == 4
    pk, keys = _grid(eng, caps[2:3], prns, win=win, **DOPP_ZERO)
    want = _windowed(orc, caps[2:3], prns, DOPP_ZERO, win)
    _check(pk, keys, [want])


def test_second_prn_set_with_five_prns(eng, orc, noise):
    """37 PRNs: set 0 whole, set 1 (slots 32..63) with five PRNs -- its other slots have both flags zero: 4 clusters."""
    sign = noise[1.0][0][:1]
    prns = np.concatenate([np.arange(1, 33), [33, 61, 120, 150, 210]]).astype(np.uint8)
    pk, keys = _grid(eng, sign, prns, **DOPP2)
    want = orc.acq_grid(sign, 1, prns, DOPP2["dopp_min_hz"], DOPP2["dopp_step_hz"], 2, 8, n_threads=ORC_THREADS, live=True)
    _check(pk, keys, [want])


def test_repeated_launches_are_byte_identical(eng, noise):
    """The same 2-capture launch 20 times on device-resident captures, every run into fresh, differently pre-filled buffers: a
    table read before the barrier that publishes it shows here."""
    from stm32f4_sdr_gps_amd import capi
    _, two, want = noise[0.25]
    g = eng.grid_desc(PRNS32, n_search=2, **DOPP2)
    eng.set_if_format(capi.IF_2BIT_SM)
    d_if = eng.malloc(two.size + 2)
    try:
        eng.h2d(d_if, np.concatenate([two.reshape(-1), np.zeros(2, np.uint8)]))
        first = None
        for run in range(20):
            pk = np.zeros((2, 32, 2, 8), capi.PEAK_DTYPE)
            pk.view(np.uint8)[...] = 0x3C + run
            keys = np.full((2, 32, 2), -7 - run, np.int64)
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


# ---- the forms that keep the extra K step ----------------------------------------------------------------------------------------------
def test_split_form_still_matches_the_oracle(monkeypatch_module, noise):
    """$GPSX_ACQ_SPLIT=2: k_acq_mx<5>, whose passes keep the extra K step in the shared loop."""
    sign, _, want = noise[1.0]
    e = _lab_engine(monkeypatch_module, GPSX_ACQ_SPLIT="2")
    try:
        pk, keys = e.acq_grid(sign, PRNS32, n_search=2, **DOPP2)
        assert b"k_acq_mx<5>" in e.lib.gpsx_last_kernel(e.h)
    finally:
        e.close()
    _check(pk, keys, want)


def test_two_block_search_still_matches_the_oracle(eng, orc, noise):
    """n_ms = 2: a multi-block form of k_acq_mx sums the two captures of noise[0.25] as one search."""
    sign = noise[0.25][0]
    prns = np.arange(1, 9, dtype=np.uint8)
    pk, keys = eng.acq_grid(sign, prns, n_search=1, n_ms=2, **DOPP2)
    assert eng.lib.gpsx_last_kernel(eng.h).startswith(b"k_acq_mx<") and eng.lib.gpsx_last_kernel(eng.h) != b"k_acq_mx<0>"
    want = orc.acq_grid(sign, 2, prns, DOPP2["dopp_min_hz"], DOPP2["dopp_step_hz"], 2, 8, n_threads=ORC_THREADS, live=True)
    _check(pk, keys, [want])
