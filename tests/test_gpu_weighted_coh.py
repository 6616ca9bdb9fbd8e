"""The weighted two-bit grid over n_coh coherently integrated blocks (EXTENSION, not in the reference: include/gpsx.h
gpsx_acq_grid_weighted_coh; k_acq_coh_mx on the matrix cores, k_acq_coh_vec on the vector ALU) against its exact CPU restatement
(tests/weighted_coh_ref.py, pinned to the oracle in tests/test_weighted_coh_reference.py): records on both paths over PRN lists,
block counts, strides, weight modes and a non-default IF; degenerate captures at 10 and 20 blocks (I^2 + Q^2 towards 2^41);
n_coh = 1 against the one-block call; a launch that fills the chip on both paths; the argument checks; and what the call is for --
ten coherent blocks acquire satellites that ten non-coherently summed blocks miss."""
import ctypes as C

import numpy as np
import pytest

import weighted_coh_ref as R

pytestmark = pytest.mark.gpu

FIELDS = ("max_val", "phase", "sum", "avr")


@pytest.fixture(scope="module")
def eng():
    from stm32f4_sdr_gps_amd import capi
    e = capi.Engine(0)
    yield e
    e.close()


def _path(eng, path):
    from stm32f4_sdr_gps_amd import capi
    eng.set_acq_path(capi.ACQ_PATH_MATRIX if path == "matrix" else capi.ACQ_PATH_VECTOR)
    return b"k_acq_coh_mx" if path == "matrix" else b"k_acq_coh_vec"


def _same(got, want, what):
    for f in FIELDS:
        assert np.array_equal(got[f], want[f]), (what, f, np.argwhere(got[f] != want[f])[:4].tolist())


def _blocks(n, amp=0.3, seed=3):
    from stm32f4_sdr_gps_amd import synth
    sats = [synth.Sat(7, 1310.0, 4321.0, amp, 0.4), synth.Sat(19, -2240.0, 12007.0, amp, 2.0), synth.Sat(30, 2018.0, 13000.0, amp, 4.0)]
    return synth.make_if_static(n, sats, noise_amp=1.0, seed=seed, two_bit=True)


# (PRNs, n_search, n_coh, stride, dopp_min, dopp_step, n_dopp, use_magnitude)
CASES = [
    (np.array([19], np.uint8), 3, 2, 1, -2240, 250, 2, True),                                  # overlapping searches
    (np.array([7, 19, 30, 1, 2, 3, 150, 5, 6, 210, 9], np.uint8), 2, 3, 3, -2500, 500, 3, False),   # PRNs above 32
    (np.arange(1, 17, dtype=np.uint8), 2, 10, 0, 1000, 50, 2, True),                        # stride 0: both read blocks 0..9
    (np.arange(1, 41, dtype=np.uint8), 1, 20, 20, 1310, 25, 1, True),                       # two 32-PRN sets, the second partial
    (np.arange(25, 41, dtype=np.uint8), 2, 10, 10, 2000, 50, 1, False),                     # stride n_coh, sign plane only
]


@pytest.mark.parametrize("path", ["matrix", "vector"])
def test_records_match_the_reference(eng, oracle, path):
    blocks = _blocks(22)
    kernel = _path(eng, path)
    try:
        for prns, n_search, n_coh, stride, d0, ds, nd, um in CASES:
            got = eng.acq_grid_weighted_coh(blocks, prns, n_search, n_coh, d0, ds, nd, use_magnitude=um, stride_blocks=stride)
            assert eng.lib.gpsx_last_kernel(eng.h) == kernel
            want = R.grid(oracle, blocks, n_search, prns, n_coh, d0, ds, nd, um, stride=stride)
            _same(got, want, (len(prns), n_coh, stride))
    finally:
        _path(eng, "matrix")


@pytest.mark.parametrize("path", ["matrix", "vector"])
def test_non_default_if(path, oracle):
    from stm32f4_sdr_gps_amd import capi
    blocks = _blocks(6, seed=8)
    prns = np.array([7, 19, 44], np.uint8)
    e = capi.Engine(0)
    try:
        e.set_config(if_hz=4_100_000)
        kernel = _path(e, path)
        got = e.acq_grid_weighted_coh(blocks, prns, 2, 3, -3000, 250, 3)
        assert e.lib.gpsx_last_kernel(e.h) == kernel
    finally:
        e.close()
    _same(got, R.grid(oracle, blocks, 2, prns, 3, -3000, 250, 3, True, if_hz=4_100_000), "if_hz")


@pytest.mark.parametrize("path", ["matrix", "vector"])
def test_degenerate_captures_at_10_and_20_blocks(eng, oracle, path):
    """a clean strong satellite (I^2 + Q^2 near 2^39 at 20 blocks), all-0xFF, every magnitude bit set, and blocks whose wiped
    I is 3 x the replica (I = 981 120: the top of the range)"""
    from stm32f4_sdr_gps_amd import synth
    strong = synth.make_if_static(20, [synth.Sat(7, 1310.0, 4321.0, 4.0, 0.4)], noise_amp=0.05, seed=5, two_bit=True)
    flat = np.full_like(strong, 0xFF)
    mag_set = strong | np.uint8(0xAA)
    matched = R.code_matched_blocks(oracle, 8, 4092000 + 1310, 20)
    prns = np.array([7, 8], np.uint8)
    kernel = _path(eng, path)
    try:
        for n_coh in (10, 20):
            for blocks in (strong, flat, mag_set, matched):
                got = eng.acq_grid_weighted_coh(blocks, prns, 1, n_coh, 810, 500, 2)
                assert eng.lib.gpsx_last_kernel(eng.h) == kernel
                _same(got, R.grid(oracle, blocks, 1, prns, n_coh, 810, 500, 2, True), n_coh)
        assert got[0, 1, 1]["max_val"] >= 981120 and got[0, 1, 1]["phase"] == 0
    finally:
        _path(eng, "matrix")


@pytest.mark.parametrize("path", ["matrix", "vector"])
def test_one_block_is_the_one_block_call(eng, path):
    blocks = _blocks(4)
    prns = np.array([7, 19, 30, 2, 3], np.uint8)
    _path(eng, path)
    try:
        for um in (True, False):
            old = eng.acq_grid_weighted(blocks, prns, 3, -1000, 500, 3, use_magnitude=um, stride_blocks=1)
            k_old = eng.lib.gpsx_last_kernel(eng.h)
            new = eng.acq_grid_weighted_coh(blocks, prns, 3, 1, -1000, 500, 3, use_magnitude=um, stride_blocks=1)
            assert eng.lib.gpsx_last_kernel(eng.h) == k_old == (b"k_acq_mxw" if path == "matrix" else b"k_acq_weighted")
            assert new.tobytes() == old.tobytes()
    finally:
        _path(eng, "matrix")


def test_chip_filling_launch_both_paths(eng, oracle):
    """256 searches x 32 PRNs x 21 Doppler bins x 10 blocks (5376 clusters: 21 rounds of the chip): the two paths
    byte-identical, and one unit per (Doppler bin, 8-PRN group) against the reference"""
    rng = np.random.default_rng(21)
    blocks = rng.integers(0, 256, (2560, 4092), dtype=np.uint8)
    prns = np.arange(1, 33, dtype=np.uint8)
    mx = eng.acq_grid_weighted_coh(blocks, prns, 256, 10, -5000, 500, 21)
    assert eng.lib.gpsx_last_kernel(eng.h) == b"k_acq_coh_mx"
    _path(eng, "vector")
    try:
        vec = eng.acq_grid_weighted_coh(blocks, prns, 256, 10, -5000, 500, 21)
        assert eng.lib.gpsx_last_kernel(eng.h) == b"k_acq_coh_vec"
    finally:
        _path(eng, "matrix")
    assert mx.tobytes() == vec.tobytes()
    units = [(int(rng.integers(0, 256)), 8 * g + int(rng.integers(0, 8)), d) for d in range(21) for g in range(4)]
    units += [(0, 0, 0), (255, 31, 20)]
    want = R.grid(oracle, blocks, 256, prns, 10, -5000, 500, 21, True, units=units)
    idx = tuple(np.array(units).T)
    _same(mx[idx], want[idx], "sampled units")


@pytest.mark.parametrize("path", ["matrix", "vector"])
def test_argument_checks_write_nothing(eng, path):
    from stm32f4_sdr_gps_amd import capi
    blocks = _blocks(4)
    _path(eng, path)
    try:
        # (PRN, n_search, n_coh, stride, weights, null capture, null records)
        for prn, n_search, n_coh, stride, wt, null_if, null_pk in ((5, 1, 0, 1, 1, 0, 0), (5, 1, 21, 1, 1, 0, 0), (5, 2, 3, 2, 1, 0, 0),
                                                                   (5, 1, 5, 5, 1, 0, 0), (5, 1, 2, 2, 2, 0, 0), (5, 1, 2, 2, -1, 0, 0),
                                                                   (0, 1, 2, 2, 1, 0, 0), (211, 1, 2, 2, 1, 0, 0), (5, 1, 2, 2, 1, 1, 0),
                                                                   (5, 1, 2, 2, 1, 0, 1)):
            prns = np.array([prn, 7], np.uint8)
            g = capi.AcqWeightedT(n_search, stride, 2, prns.ctypes.data_as(C.POINTER(C.c_uint8)), 0, 500, 1, wt)
            peaks = np.zeros((n_search, 2, 1), capi.PEAK_DTYPE)
            peaks.view(np.uint8)[...] = 0xA5
            rc = eng.lib.gpsx_acq_grid_weighted_coh(eng.h, C.byref(g), n_coh, None if null_if else blocks.ctypes.data, 4,
                                                    None if null_pk else peaks.ctypes.data)
            assert rc == -22 and eng.lib.gpsx_last_error(eng.h), (prn, n_search, n_coh, stride, wt)
            assert (peaks.view(np.uint8) == 0xA5).all()
        rc = eng.lib.gpsx_acq_grid_weighted_coh(eng.h, None, 2, blocks.ctypes.data, 4, peaks.ctypes.data)
        assert rc == -22 and (peaks.view(np.uint8) == 0xA5).all()
    finally:
        _path(eng, "matrix")


def test_ten_coherent_blocks_acquire_what_ten_non_coherent_blocks_miss(eng):
    """Eight cold-start captures of ten blocks each, the bench's six satellites at amplitude scale 0.03 (far below the noise;
    make_if_static keeps the carrier phase continuous from block to block and carries no data bits).  Ten coherent blocks on
    50 Hz bins over +-5 kHz against ten non-coherently summed weighted blocks on 500 Hz bins (test_gpu_weighted_ms.py's grid).
    A (capture, satellite) pair acquires when the PRN's best bin is within one bin (of its grid's step) of the true Doppler and
    its phase within 8 samples of the true code phase.  Calibrated on the CPU restatements (the GPU computes the same records):
    coherent 36 of 48, non-coherent 20 (at 0.04: 48 and 42).  Asserted with margin: coherent at least 30 and at least ten more."""
    from stm32f4_sdr_gps_amd import synth
    n = 8
    blocks = synth.cold_start_block(10 * n, seed=11, amp_scale=0.03, two_bit=True)
    truth = {3: (-3210.0, 777.0), 5: (912.5, 1600.0), 11: (4480.0, 12001.0), 14: (4037.0, 4000.0), 20: (-1025.0, 9000.0), 30: (2018.0, 13000.0)}
    prns = np.array(sorted(truth), np.uint8)
    coh = R.hits(eng.acq_grid_weighted_coh(blocks, prns, n, 10, -5000, 50, 201), prns, truth, n, -5000, 50)
    assert eng.lib.gpsx_last_kernel(eng.h) == b"k_acq_coh_mx"
    nc = R.hits(eng.acq_grid_weighted_ms(blocks, prns, n, 10, -5000, 500, 21), prns, truth, n, -5000, 500)
    print("acquired of", 6 * n, ": ten coherent blocks", coh, "ten non-coherent blocks", nc)
    assert coh >= 30 and coh >= nc + 10
