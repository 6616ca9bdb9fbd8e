"""The single-block fine grid's one-pass anchor (k_acq_mx<0>): sample offset 0 comes from ONE matrix pass whose
vector holds 8 - S_0[k] as E3M2 codes, cut out of one packed six-bit stream per lane, and the loop starts one half-step pair
earlier.  A wrong code, a wrong window, a wrong start value or a piece that its reader overtakes is a wrong triplet somewhere,
so everything is compared bit for bit with the CPU oracle computed live: noise captures in both IF formats, hand-made blocks
whose block sums take every value 0..16 (0 and 16 adjacent, and at entries 0 and 1021 next to the always-empty entry 1022),
the launch shapes that change what a workgroup owns, and one launch repeated.  The forms that keep the two-pass anchor share
the code: one split launch (k_acq_mx<5>) and one two-block launch still match the oracle.

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
# bin 0 at 1 Hz, the lowest carrier the API admits (0 Hz is refused): the NCO never leaves its first quadrant within a block, so
# the carrier replica is the 0 Hz word all along it and the wiped stream is the capture XOR a constant
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
    for amp, seed in ((0.25, 53), (1.0, 59)):
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


# ---- hand-made block sums -------------------------------------------------------------------------------------------------------
def _sums_to_words(sums):
    """16-bit words with the given popcounts (low bits set)."""
    return ((1 << np.asarray(sums, np.uint32)) - 1).astype(np.uint16)


@pytest.fixture(scope="module")
def handmade(orc):
    """Four captures whose wiped streams in the zero bin are chosen word by word.  The wipe-off is an XOR with the carrier replica c
    (what it makes of an all-zero capture; in the zero bin one constant word), so the capture  d ^ c  has the wiped I stream d.  Entry 1022 (the sixteen samples
    the NCO never mixes) is empty whatever the capture holds.
      0  I sums: 16, 0, 16, 0, every value 0..16 up and down, runs of sixteen 16s / sixteen 0s, ..., entry 1021 = 16
      1  the complement of capture 0's I stream (sums 16 - S: entry 0 = 0, entry 1021 = 0), against the Q carrier word
      2  constant 0x00 bytes    3  constant 0xFF bytes
    -> (captures [4, 2046], oracle triplets per capture for DOPP_ZERO)"""
    zeros = np.zeros(2046, np.uint8)
    ci, cq, _ = orc.wipeoff(zeros, float(ZERO_BIN_HZ))
    assert len(set(ci[:1022].view(np.uint32).tolist())) == 1 and len(set(cq[:1022].view(np.uint32).tolist())) == 1
    ramp = list(range(17)) + list(range(16, -1, -1))
    sums = [16, 0, 16, 0] + ramp + [16] * 16 + [0] * 16 + [16] * 16 + ramp
    rng = np.random.default_rng(61)
    sums = sums + rng.integers(0, 17, 1021 - len(sums)).tolist() + [16]      # entries 0 .. 1021
    d = _sums_to_words(sums)
    caps = np.zeros((4, 2046), np.uint8)
    caps[0, :2044] = (d ^ ci[:1022]).view(np.uint8)
    caps[1, :2044] = (~d ^ cq[:1022]).view(np.uint8)
    caps[0, 2044:] = 0xA5       # the unmixed samples: read as zero by every implementation
    caps[3] = 0xFF
    # the premise, by the oracle's own wipe-off: every block sum 0..16 occurs in capture 0's I and capture 1's Q stream
    di, _, _ = orc.wipeoff(caps[0], float(ZERO_BIN_HZ))
    _, dq, _ = orc.wipeoff(caps[1], float(ZERO_BIN_HZ))
    pop_i = np.array([bin(int(w)).count("1") for w in di[:1023]]), np.array([bin(int(w)).count("1") for w in dq[:1023]])
    assert pop_i[0][:1022].tolist() == sums and pop_i[0][1022] == 0
    assert pop_i[1][:1022].tolist() == [16 - s for s in sums] and pop_i[1][1022] == 0
    assert set(pop_i[0].tolist()) == set(range(17))
    want = [orc.acq_grid(caps[i:i + 1], 1, PRNS32, DOPP_ZERO["dopp_min_hz"], DOPP_ZERO["dopp_step_hz"], 2, 8,
                         n_threads=ORC_THREADS, live=True) for i in range(4)]
    return caps, want


@pytest.mark.parametrize("pair", [(0, 1), (2, 3)], ids=["every_sum", "constant_bytes"])
@pytest.mark.parametrize("two_bit", [False, True])
def test_handmade_block_sums_vs_live_oracle(eng, handmade, pair, two_bit):
    caps, want = handmade
    blocks = caps[list(pair)]
    pk, keys = _grid(eng, _two_bit(blocks, 67) if two_bit else blocks, PRNS32, two_bit=two_bit, **DOPP_ZERO)
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


def test_second_prn_set_ending_inside_a_set(eng, orc, noise):
    """37 PRNs: set 0 whole, set 1 (slots 32..63) with five PRNs -- 4 clusters."""
    sign = noise[1.0][0][:1]
    prns = np.concatenate([np.arange(1, 33), [33, 61, 120, 150, 210]]).astype(np.uint8)
    pk, keys = _grid(eng, sign, prns, **DOPP2)
    want = orc.acq_grid(sign, 1, prns, DOPP2["dopp_min_hz"], DOPP2["dopp_step_hz"], 2, 8, n_threads=ORC_THREADS, live=True)
    _check(pk, keys, [want])


@pytest.mark.parametrize("win", [(1, 2045), (0, 1), (2045, 2046), (301, 1001)])
def test_window_edges(eng, orc, handmade, win):
    """Byte offsets outside the window start at the value that clips to zero -- the one-pass start value less 2^20.  Edges at byte
    offsets 0 / 1 (chip offset 0 split), 2045 (the last one) and inside a wave's tile, on the capture with every block sum."""
    caps, _ = handmade
    prns = np.array([1, 7, 13, 19, 22, 25, 31, 32], np.uint8)
    pk, keys = _grid(eng, caps[:1], prns, win=win, **DOPP_ZERO)
    want = _windowed(orc, caps[:1], prns, DOPP_ZERO, win)
    _check(pk, keys, [want])


def test_shard_owning_one_group_of_a_cluster(eng, noise):
    """32 PRNs x 2 Doppler bins = 8 units; shard 5 of 8 owns one: the second cluster runs with one 8-PRN group of its four."""
    from stm32f4_sdr_gps_amd import sharding
    sign, _, want = noise[0.25]
    pk, keys = _grid(eng, sign[:1], PRNS32, shard=(5, 8), **DOPP2)
    mine = sharding.owned_mask(1, 32, 2, 5, 8)[0]
    assert mine.sum() == 8          # (PRN, Doppler) cells of one 8-PRN unit
    for f in FIELDS:
        assert np.array_equal(pk[0][f][mine], want[0][f][mine]), f
        assert not pk[0][f][~mine].any(), f
    assert np.array_equal(keys[0][mine], _keys(want[0])[mine]) and not keys[0][~mine].any()


def test_repeated_launches_are_byte_identical(eng, noise):
    """The same 2-capture launch 20 times on device-resident captures, every run into fresh, differently pre-filled buffers."""
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
            pk.view(np.uint8)[...] = 0x5A + run
            keys = np.full((2, 32, 2), -1 - run, np.int64)
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


# ---- the forms that keep the two-pass anchor ----------------------------------------------------------------------------------------
def test_split_form_still_matches_the_oracle(monkeypatch_module, noise):
    """$GPSX_ACQ_SPLIT=2: k_acq_mx<5>, whose first run starts with the two FP4 passes in the shared loop."""
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
