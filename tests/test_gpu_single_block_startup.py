"""The single-block fine grid's start-up schedule (k_acq_mx<0>): the preamble builds only what pass 0 reads; the
planes, the lookup tables, vector 1 and the zeroes of the result slots are made in the first three half steps by the role that
has no pass of its own there, each published by a barrier in front of its first reader.  A piece that its reader overtakes is a
wrong triplet somewhere -- or a different one from run to run: everything here is compared bit for bit, against the CPU oracle
computed live, and one launch is repeated into fresh buffers.  The split form (k_acq_mx<5>, mx_unit) keeps the old
start-up: one case checks that it still gives what it gave.
"""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import oracle_threads
from golden_util import IF_HZ

ORC_THREADS = oracle_threads()
FIELDS = ("max_val", "phase", "sum", "avr")
DOPP = dict(dopp_min_hz=-5000, dopp_step_hz=500, n_dopp=21)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from stm32f4_sdr_gps_amd import capi
    e = capi.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng_no_split(monkeypatch_module):
    """The lab library with $GPSX_ACQ_NO_SPLIT: small launches stay one workgroup per cluster (k_acq_mx<0>)."""
    from stm32f4_sdr_gps_amd import capi
    monkeypatch_module.setenv("GPSX_ACQ_NO_SPLIT", "1")
    e = capi.Engine(0, lab=True)
    monkeypatch_module.delenv("GPSX_ACQ_NO_SPLIT")
    yield e
    e.close()


@pytest.fixture(scope="module")
def monkeypatch_module():
    mp = pytest.MonkeyPatch()
    yield mp
    mp.undo()


@pytest.fixture(scope="module")
def one_group():
    """8 captures x 8 PRNs (one 8-PRN group: the cluster's group mask is partial) x 21 Doppler: 168 clusters, more than half a
    round of the 256 CUs, so the product library launches k_acq_mx<0> with 168 workgroups.  2-bit IF in, its sign plane to the
    oracle.  -> (2-bit blocks, PRNs, {capture: oracle triplets})"""
    from oracle import pyoracle
    from stm32f4_sdr_gps_amd import synth
    blocks2 = synth.cold_start_block(8, seed=31, amp_scale=0.5, two_bit=True)
    blocks1 = synth.cold_start_block(8, seed=31, amp_scale=0.5)
    prns = np.array([3, 5, 11, 14, 20, 30, 1, 32], np.uint8)
    orc = pyoracle.Oracle()
    want = {i: orc.acq_grid(blocks1[i:i + 1], 1, prns, -5000, 500, 21, 8, n_threads=ORC_THREADS, live=True) for i in (0, 3, 7)}
    return blocks2, prns, want


def _want_keys(want):
    from stm32f4_sdr_gps_amd import sharding
    return sharding.pack_keys(want["max_val"], want["phase"])


def test_one_group_more_than_half_a_round_vs_live_oracle(eng, one_group):
    from stm32f4_sdr_gps_amd import capi
    blocks2, prns, want = one_group
    eng.set_if_format(capi.IF_2BIT_SM)
    try:
        pk, keys = eng.acq_grid(blocks2, prns, n_search=8, **DOPP)
    finally:
        eng.set_if_format(capi.IF_1BIT)
    assert eng.lib.gpsx_last_kernel(eng.h) == b"k_acq_mx<0>"
    for i, w in want.items():
        for f in FIELDS:
            assert np.array_equal(pk[i][f], w[f]), (i, f)
        assert np.array_equal(keys[i], _want_keys(w)), i


def test_repeated_launches_are_byte_identical(eng, one_group):
    """The same launch 20 times on device-resident captures, every run into freshly allocated (and differently pre-filled) result
    buffers: peaks and keys of every run equal the first run's byte for byte, and the first run's equal the oracle's."""
    from stm32f4_sdr_gps_amd import capi
    blocks2, prns, want = one_group
    g = eng.grid_desc(prns, n_search=8, **DOPP)
    eng.set_if_format(capi.IF_2BIT_SM)
    d_if = eng.malloc(blocks2.size + 2)
    try:
        eng.h2d(d_if, np.concatenate([blocks2.reshape(-1), np.zeros(2, np.uint8)]))
        first = None
        for run in range(20):
            pk = np.zeros((8, len(prns), 21, 8), capi.PEAK_DTYPE)
            pk.view(np.uint8)[...] = 0x5A + run
            keys = np.full((8, len(prns), 21), -1 - run, np.int64)
            d_pk, d_keys = eng.malloc(pk.nbytes), eng.malloc(keys.nbytes)
            try:
                eng.h2d(d_pk, pk)
                eng.h2d(d_keys, keys)
                rc = eng.lib.gpsx_acq_grid_dev(eng.h, C.byref(g), C.c_void_p(d_if), 8, C.c_void_p(d_pk), C.c_void_p(d_keys),
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
                for i, w in want.items():
                    for f in FIELDS:
                        assert np.array_equal(pk[i][f], w[f]), (i, f)
                    assert np.array_equal(keys[i], _want_keys(w)), i
            else:
                assert pk.tobytes() == first[0] and keys.tobytes() == first[1], run
    finally:
        eng.free(d_if)
        eng.set_if_format(capi.IF_1BIT)


@pytest.fixture(scope="module")
def full_cluster():
    """1 capture x 32 PRNs x 21 Doppler, 1-bit IF -> (blocks, PRNs, oracle triplets, computed live once for both shards)"""
    from oracle import pyoracle
    from stm32f4_sdr_gps_amd import synth
    blocks = synth.cold_start_block(1, seed=37, amp_scale=0.5)
    prns = np.arange(1, 33, dtype=np.uint8)
    want = pyoracle.Oracle().acq_grid(blocks, 1, prns, -5000, 500, 21, 8, n_threads=ORC_THREADS, live=True)
    return blocks, prns, want


@pytest.mark.parametrize("rank", [0, 1])
def test_two_shards_of_one_capture_vs_live_oracle(eng, full_cluster, rank):
    """84 units in two runs of 42: eleven clusters each, the one at the seam with two of its four 8-PRN groups foreign.  Sharded
    launches never split: k_acq_mx<0> with 11 workgroups."""
    from stm32f4_sdr_gps_amd import sharding
    blocks, prns, want = full_cluster
    pk, keys = eng.acq_grid(blocks, prns, n_search=1, shard=(rank, 2), **DOPP)
    assert eng.lib.gpsx_last_kernel(eng.h) == b"k_acq_mx<0>"
    mine = sharding.owned_mask(1, len(prns), 21, rank, 2)[0]
    assert mine.sum() == 42 * 8
    for f in FIELDS:
        assert np.array_equal(pk[0][f][mine], want[f][mine]), f
        assert not pk[0][f][~mine].any(), f
    assert np.array_equal(keys[0][mine], _want_keys(want)[mine]) and not keys[0][~mine].any()


def test_two_prn_sets_and_a_window_inside_the_block_vs_live_oracle(eng_no_split):
    """37 PRNs = two 32-slot sets, the second with five PRNs, x 2 Doppler bins = 4 clusters on the lab library (one workgroup per
    cluster whatever the size), byte offsets [301, 1001): both edges fall between the two byte offsets of a chip offset and
    inside a wave's tile, everything outside starts at the value that clips to zero.  Every triplet and key against
    correlation_search over that window (the oracle's search_job)."""
    from oracle import pyoracle
    from stm32f4_sdr_gps_amd import synth
    orc = pyoracle.Oracle()
    block = synth.cold_start_block(1, seed=41, amp_scale=0.5)
    prns = np.concatenate([np.arange(1, 33), [33, 61, 120, 150, 210]]).astype(np.uint8)
    win = (301, 1001)
    pk, keys = eng_no_split.acq_grid(block, prns, n_search=1, dopp_min_hz=-750, dopp_step_hz=1500, n_dopp=2, win=win)
    assert eng_no_split.lib.gpsx_last_kernel(eng_no_split.h) == b"k_acq_mx<0>"
    codes = [orc.ca_code(int(p)) for p in prns]

    def job(pdb):
        p, d, b = pdb
        peak, _, _ = orc.search_job(block, 1, codes[p], float(IF_HZ - 750 + 1500 * d), b, win[0], win[1])
        return tuple(peak[f] for f in FIELDS)
    cells = [(p, d, b) for p in range(len(prns)) for d in range(2) for b in range(8)]
    with ThreadPoolExecutor(ORC_THREADS) as pool:
        res = list(pool.map(job, cells))
    want = np.zeros((len(prns), 2, 8), pk.dtype)
    for (p, d, b), r in zip(cells, res):
        want[p, d, b] = r
    for f in FIELDS:
        assert np.array_equal(pk[0][f], want[f]), f
    assert np.array_equal(keys[0], _want_keys(want))


def test_split_tail_next_to_the_single_form_is_unchanged(eng, oracle):
    """16 captures = 336 clusters: 256 on k_acq_mx<0>, the 80 of the last round as 160 workgroups of the split form (k_acq_mx<5>,
    mx_unit, which keeps the all-hands start-up) behind k_acq_finalize_from.  Captures 0 (single form), 12 (the seam
    runs through its Doppler bins) and 15 (split form) against the oracle."""
    from stm32f4_sdr_gps_amd import synth
    blocks = synth.cold_start_block(16, seed=23, amp_scale=0.5)
    prns = np.arange(1, 33, dtype=np.uint8)
    pk, keys = eng.acq_grid(blocks, prns, n_search=16, **DOPP)
    assert eng.lib.gpsx_last_kernel(eng.h) == b"k_acq_mx<0>"
    for i in (0, 12, 15):
        want = oracle.acq_grid(blocks[i:i + 1], 1, prns, -5000, 500, 21, 8, n_threads=ORC_THREADS)
        for f in FIELDS:
            assert np.array_equal(pk[i][f], want[f]), (i, f)
        assert np.array_equal(keys[i], _want_keys(want)), i
