"""The single-block fine grid with its accumulator tile transposed (k_acq_mx<0>; csrc/gpsx_mx_transposed.hpp): the
Toeplitz fragment is the MFMA's A operand and the chips are B, so a lane holds ONE PRN and its 64 registers hold 64 chip offsets.
The windowed maximum is a register chain over LOCAL keys that becomes a global key once per lane and sample offset; start values
and window edges are per register; the even-to-odd switch adds entries of a table built once per workgroup; the result slots are
one word per (bit shift, field, lane half, PRN).  A wrong register-to-offset map, a tie decided for the later offset, a window
edge in the wrong register, a PRN group published by the wrong lanes or a table read before its barrier is a wrong triplet
somewhere, so every record and key is compared bit for bit with the CPU oracle computed live.

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
# bin 0 at 1 Hz, the lowest carrier the API admits: the carrier replica is one constant word along the block (the fold test's zero bin)
ZERO_BIN_HZ = 1
DOPP_ZERO = dict(dopp_min_hz=ZERO_BIN_HZ - IF_HZ, dopp_step_hz=IF_HZ + 250, n_dopp=2)
DOPP_ZERO_ONLY = dict(dopp_min_hz=ZERO_BIN_HZ - IF_HZ, dopp_step_hz=IF_HZ + 250, n_dopp=1)
PRNS32 = np.arange(1, 33, dtype=np.uint8)
# register, register-quad, lane-half, tile, wave-pair and role boundaries of the transposed layout
TIE_Q = (0, 3, 4, 7, 8, 28, 31, 32, 63, 64, 96, 127, 128, 255, 256, 511, 512, 768, 1018)
EDGE_Q = (0, 1, 4, 35, 1021, 1022)

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


def _windowed(orc, block, prns, dopp, win, want_energy=False):
    """The oracle's windowed search_job per (PRN, bin, bit shift) -> (triplets [n_prn, n_dopp, 8], number of cells whose non-zero
    maximum is reached at two or more offsets of the window)"""
    from stm32f4_sdr_gps_amd import capi
    codes = [orc.ca_code(int(p)) for p in prns]
    cells = [(p, d, b) for p in range(len(prns)) for d in range(dopp["n_dopp"]) for b in range(8)]

    def job(pdb):
        p, d, b = pdb
        freq = float(IF_HZ + dopp["dopp_min_hz"] + dopp["dopp_step_hz"] * d)
        peak, energy, _ = orc.search_job(block, 1, codes[p], freq, b, win[0], win[1], want_energy=want_energy)
        tied = False
        if want_energy:
            vals = energy[win[0]:win[1]]
            assert int(vals.max()) == peak["max_val"]
            tied = peak["max_val"] > 0 and int((vals == vals.max()).sum()) >= 2
        return tuple(peak[f] for f in FIELDS), tied
    with ThreadPoolExecutor(ORC_THREADS) as pool:
        res = list(pool.map(job, cells))
    want = np.zeros((len(prns), dopp["n_dopp"], 8), capi.PEAK_DTYPE)
    for (p, d, b), (r, _) in zip(cells, res):
        want[p, d, b] = r
    return want, sum(t for _, t in res)


@pytest.fixture(scope="module")
def extremes():
    """The captures of the fold test's `extremes` fixture: constant 0x00, constant 0xFF, a noise capture and its complement."""
    from stm32f4_sdr_gps_amd import synth
    caps = np.zeros((4, 2046), np.uint8)
    caps[1] = 0xFF
    caps[2] = synth.cold_start_block(1, seed=79, amp_scale=0.25)[0]
    caps[3] = ~caps[2]
    return caps


# ---- 1. ties at every position of the new layout ------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", [(0, 1), (2, 3)], ids=["constant_bytes", "capture_and_complement"])
@pytest.mark.parametrize("q", TIE_Q)
def test_ties_at_layout_boundaries(eng, orc, extremes, q, pair):
    """Windows of 8 byte offsets starting at 2 q + s, in the zero bin: the maximum of a cell is reached at several offsets that sit
    in different registers, register quads, lane halves, tiles or waves, and the FIRST one must win.  The premise -- in every window
    some cell of one of the pair's captures has its non-zero maximum at two or more in-window offsets -- is asserted from the oracle
    alone, before the launch."""
    blocks = extremes[list(pair)]
    for s in (0, 1):
        win = (2 * q + s, 2 * q + s + 8)
        want, tied = zip(*[_windowed(orc, blocks[i:i + 1], PRNS32, DOPP_ZERO_ONLY, win, want_energy=True) for i in range(2)])
        assert max(tied) > 0, (q, s, tied)
        pk, keys = _grid(eng, blocks, PRNS32, win=win, **DOPP_ZERO_ONLY)
        _check(pk, keys, want)


# ---- 2. window edges inside a lane's registers ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", EDGE_Q)
def test_window_edges_inside_a_lane(eng, orc, extremes, q):
    """Windows of two byte offsets, (2 q, 2 q + 2) and (2 q + 1, 2 q + 3): one chip offset's pair, and the odd offset of one with
    the even offset of the next -- the per-register start values and the half switch's window-edge term decide these.  PRNs
    with all four (chip 1021, chip 1022) pairs."""
    prns = np.array([1, 4, 6, 9, 16, 22, 28, 31], np.uint8)
    chips = np.stack([orc.ca_code(int(p)) for p in prns])
    assert len({(int(c[1021]), int(c[1022])) for c in chips}) == 4
    for win in ((2 * q, 2 * q + 2), (2 * q + 1, min(2 * q + 3, 2046))):   # (byte offset 2045 is the last one)
        pk, keys = _grid(eng, extremes[2:3], prns, win=win, **DOPP_ZERO)
        want, _ = _windowed(orc, extremes[2:3], prns, DOPP_ZERO, win)
        _check(pk, keys, [want])


# ---- 3. ownership by lane group, 4. strong signal, 5. repeatability ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def strong(orc):
    """Two captures at amp_scale 1.0: (sign planes, 2-bit form, oracle triplets per capture)"""
    from stm32f4_sdr_gps_amd import synth
    sign = synth.cold_start_block(2, seed=73, amp_scale=1.0)
    two = synth.cold_start_block(2, seed=73, amp_scale=1.0, two_bit=True)
    want = [orc.acq_grid(sign[i:i + 1], 1, PRNS32, DOPP2["dopp_min_hz"], DOPP2["dopp_step_hz"], 2, 8, n_threads=ORC_THREADS,
                         live=True) for i in range(2)]
    return sign, two, want


def _check_shard(pk, keys, want, n_prn, shard):
    from stm32f4_sdr_gps_amd import sharding
    mine = sharding.owned_mask(1, n_prn, 2, *shard)[0]                  # [n_prn, n_dopp]
    assert mine.any() and not mine.all()
    for f in FIELDS:
        assert np.array_equal(pk[0][f][mine], want[f][mine]), (shard, f)
        assert not pk[0][f][~mine].any(), (shard, f)
    assert np.array_equal(keys[0][mine], _keys(want)[mine]) and not keys[0][~mine].any(), shard


@pytest.mark.parametrize("shard", [(1, 3), (2, 3)])
def test_ownership_by_lane_group(eng, strong, shard):
    """One capture x 2 bins x 32 PRNs = 8 units: a third of them cuts the cluster between lane groups (lane & 31) >> 3."""
    sign, _, want = strong
    pk, keys = _grid(eng, sign[:1], PRNS32, shard=shard, **DOPP2)
    _check_shard(pk, keys, want[0], 32, shard)


def test_ownership_with_a_second_partial_prn_set(eng, orc, strong):
    """37 PRNs: set 1 holds five -- one lane group, 27 lanes without a PRN; unsharded and as shard 1 of 3."""
    sign = strong[0][:1]
    prns = np.concatenate([np.arange(1, 33), [33, 61, 120, 150, 210]]).astype(np.uint8)
    want = orc.acq_grid(sign, 1, prns, DOPP2["dopp_min_hz"], DOPP2["dopp_step_hz"], 2, 8, n_threads=ORC_THREADS, live=True)
    pk, keys = _grid(eng, sign, prns, **DOPP2)
    _check(pk, keys, [want])
    pk, keys = _grid(eng, sign, prns, shard=(1, 3), **DOPP2)
    _check_shard(pk, keys, want, 37, (1, 3))


@pytest.mark.parametrize("two_bit", [False, True])
def test_strong_signal(eng, strong, two_bit):
    """amp_scale 1.0: groups of eight hypotheses beyond radius 1024 take the exact-root path, the others the small one."""
    sign, two, want = strong
    assert max(int(w["max_val"].max()) for w in want) >= 1024
    pk, keys = _grid(eng, two if two_bit else sign, PRNS32, two_bit=two_bit, **DOPP2)
    _check(pk, keys, want)


def test_repeated_launches_are_byte_identical(eng, strong):
    """The strong-signal launch ten times on device-resident captures, every run into fresh, differently pre-filled buffers: a table
    or result slot read before the barrier that publishes it shows here."""
    from stm32f4_sdr_gps_amd import capi
    _, two, want = strong
    g = eng.grid_desc(PRNS32, n_search=2, **DOPP2)
    eng.set_if_format(capi.IF_2BIT_SM)
    d_if = eng.malloc(two.size + 2)
    try:
        eng.h2d(d_if, np.concatenate([two.reshape(-1), np.zeros(2, np.uint8)]))
        first = None
        for run in range(10):
            pk = np.zeros((2, 32, 2, 8), capi.PEAK_DTYPE)
            pk.view(np.uint8)[...] = 0x5A + 7 * run
            keys = np.full((2, 32, 2), -11 - run, np.int64)
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
