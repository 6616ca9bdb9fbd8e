"""The weighted two-bit grid over n_ms blocks (EXTENSION, not in the reference: include/gpsx.h gpsx_acq_grid_weighted_ms;
k_acq_wmx_ms on the matrix cores, k_acq_weighted_ms on the vector ALU) against its exact CPU restatement (tests/weighted_ms_ref.py,
pinned to the oracle in tests/test_weighted_ms_reference.py): records on both paths over PRN lists, block counts, strides and
weight modes; degenerate captures up to 128 blocks (E at the top of its range); n_ms = 1 against the one-block call; a launch
that fills the chip on both paths and in chunks; the argument checks; and what the call is for -- ten weighted blocks acquire
satellites that one weighted block, or ten blocks of the sign plane, do not."""
import ctypes as C
import os

import numpy as np
import pytest

import weighted_ms_ref as R

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
    return b"k_acq_wmx_ms" if path == "matrix" else b"k_acq_weighted_ms"


def _same(got, want, what):
    for f in FIELDS:
        assert np.array_equal(got[f], want[f]), (what, f, np.argwhere(got[f] != want[f])[:4].tolist())


def _blocks(n, amp=0.3, seed=3):
    from stm32f4_sdr_gps_amd import synth
    sats = [synth.Sat(7, 1310.0, 4321.0, amp, 0.4), synth.Sat(19, -2240.0, 12007.0, amp, 2.0), synth.Sat(30, 2018.0, 13000.0, amp, 4.0)]
    return synth.make_if_static(n, sats, noise_amp=1.0, seed=seed, two_bit=True)


# (PRNs, n_search, n_ms, stride, dopp_min, dopp_step, n_dopp, use_magnitude)
CASES = [
    (np.array([19], np.uint8), 3, 2, 1, -2240, 250, 2, True),                            # overlapping searches
    (np.array([7, 19, 30, 1, 2, 3, 4, 5, 6, 8, 9], np.uint8), 2, 3, 3, -2500, 500, 3, False),
    (np.arange(1, 17, dtype=np.uint8), 2, 10, 0, 1000, 500, 1, True),                  # stride 0: both searches read blocks 0..9
    (np.arange(1, 41, dtype=np.uint8), 1, 3, 3, 1310, 500, 1, True),                   # two 32-PRN sets, the second partial
]


@pytest.mark.parametrize("path", ["matrix", "vector"])
def test_records_match_the_reference(eng, oracle, path):
    blocks = _blocks(12)
    kernel = _path(eng, path)
    try:
        for prns, n_search, n_ms, stride, d0, ds, nd, um in CASES:
            got = eng.acq_grid_weighted_ms(blocks, prns, n_search, n_ms, d0, ds, nd, use_magnitude=um, stride_blocks=stride)
            assert eng.lib.gpsx_last_kernel(eng.h) == kernel
            want = R.grid(oracle, blocks, n_search, prns, n_ms, d0, ds, nd, um, stride=stride)
            _same(got, want, (len(prns), n_ms, stride))
    finally:
        _path(eng, "matrix")


@pytest.mark.parametrize("path", ["matrix", "vector"])
def test_degenerate_captures_up_to_128_blocks(eng, oracle, path):
    """test_gpu_weighted.py's strong / all-one-value / magnitude-always-set captures, at 10 and at 128 blocks: a clean strong
    satellite takes E towards 128 x 69 375 (the exact-root path in every block)"""
    from stm32f4_sdr_gps_amd import synth
    strong = synth.make_if_static(128, [synth.Sat(7, 1310.0, 4321.0, 4.0, 0.4)], noise_amp=0.05, seed=5, two_bit=True)
    flat = np.full_like(strong, 0xFF)
    sign_only = strong | np.uint8(0xAA)
    prns = np.array([7, 8], np.uint8)
    kernel = _path(eng, path)
    try:
        for n_ms in (10, 128):
            for blocks in (strong, flat, sign_only):
                got = eng.acq_grid_weighted_ms(blocks, prns, 1, n_ms, 810, 500, 2)
                assert eng.lib.gpsx_last_kernel(eng.h) == kernel
                _same(got, R.grid(oracle, blocks, 1, prns, n_ms, 810, 500, 2, True), n_ms)
        assert got["max_val"].max() > 2 ** 21          # (past the single-block kernel's 32-bit keys)
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
            new = eng.acq_grid_weighted_ms(blocks, prns, 3, 1, -1000, 500, 3, use_magnitude=um, stride_blocks=1)
            assert eng.lib.gpsx_last_kernel(eng.h) == k_old == (b"k_acq_mxw" if path == "matrix" else b"k_acq_weighted")
            assert new.tobytes() == old.tobytes()
    finally:
        _path(eng, "matrix")


def test_chip_filling_launch_both_paths_and_chunks(eng, oracle):
    """64 searches x 32 PRNs x 21 Doppler bins x 10 blocks (1344 clusters: more than five rounds of the chip): the two paths
    byte-identical, 48 seeded units against the reference, and the lab library with the scratch capped at 1 GB (512 clusters a
    launch: three chunks) byte-identical again"""
    from stm32f4_sdr_gps_amd import capi, synth
    blocks = synth.cold_start_block(640, seed=21, amp_scale=0.3, two_bit=True)
    prns = np.arange(1, 33, dtype=np.uint8)
    mx = eng.acq_grid_weighted_ms(blocks, prns, 64, 10, -5000, 500, 21)
    assert eng.lib.gpsx_last_kernel(eng.h) == b"k_acq_wmx_ms"
    _path(eng, "vector")
    try:
        vec = eng.acq_grid_weighted_ms(blocks, prns, 64, 10, -5000, 500, 21)
        assert eng.lib.gpsx_last_kernel(eng.h) == b"k_acq_weighted_ms"
    finally:
        _path(eng, "matrix")
    assert mx.tobytes() == vec.tobytes()
    rng = np.random.default_rng(48)
    units = sorted({(int(s), int(p), int(d)) for s, p, d in zip(rng.integers(0, 64, 48), rng.integers(0, 32, 48), rng.integers(0, 21, 48))})
    units += [(0, 2, 0), (63, 31, 20), (10, 10, 3)]      # (PRN 3 sits in its true bin at capture 10: a satellite's peak too)
    want = R.grid(oracle, blocks, 64, prns, 10, -5000, 500, 21, True, units=units)
    idx = tuple(np.array(units).T)
    _same(mx[idx], want[idx], "sampled units")
    os.environ["GPSX_ACQ_WMS_SCRATCH_MB"] = "1024"
    try:
        lab = capi.Engine(0, lab=True)
    finally:
        del os.environ["GPSX_ACQ_WMS_SCRATCH_MB"]
    try:
        chunked = lab.acq_grid_weighted_ms(blocks, prns, 64, 10, -5000, 500, 21)
        assert lab.lib.gpsx_last_kernel(lab.h) == b"k_acq_wmx_ms"
    finally:
        lab.close()
    assert chunked.tobytes() == mx.tobytes()


@pytest.mark.parametrize("path", ["matrix", "vector"])
def test_argument_checks_write_nothing(eng, path):
    from stm32f4_sdr_gps_amd import capi
    blocks = _blocks(4)
    _path(eng, path)
    try:
        for prn, n_search, n_ms, stride in ((5, 1, 0, 1), (5, 1, 129, 1), (5, 2, 3, 2), (0, 1, 2, 2), (5, 1, 5, 5)):
            prns = np.array([prn, 7], np.uint8)
            g = capi.AcqWeightedT(n_search, stride, 2, prns.ctypes.data_as(C.POINTER(C.c_uint8)), 0, 500, 1, 1)
            peaks = np.zeros((n_search, 2, 1), capi.PEAK_DTYPE)
            peaks.view(np.uint8)[...] = 0xA5
            rc = eng.lib.gpsx_acq_grid_weighted_ms(eng.h, C.byref(g), n_ms, blocks.ctypes.data, 4, peaks.ctypes.data)
            assert rc == -22 and eng.lib.gpsx_last_error(eng.h), (prn, n_search, n_ms, stride)
            assert (peaks.view(np.uint8) == 0xA5).all()
    finally:
        _path(eng, "matrix")


def test_ten_weighted_blocks_acquire_what_one_block_and_the_sign_plane_miss(eng):
    """Eight cold-start captures of ten blocks each, the bench's six satellites at amplitude scale 0.04 (far below the noise).
    A (capture, satellite) pair acquires when the PRN's best (Doppler bin, phase) is within one bin of the true Doppler and
    8 samples of the true code phase (test_gpu_weighted.py's rule).  Calibrated on the CPU restatement (the GPU computes the
    same records): ten weighted blocks 42 of 48, one weighted block 1, ten blocks of the sign plane alone 10.  Asserted with
    margin: at least 30, more than twice the sign plane's ten blocks, more than three times one block plus ten."""
    from stm32f4_sdr_gps_amd import synth
    n = 8
    blocks = synth.cold_start_block(10 * n, seed=11, amp_scale=0.04, two_bit=True)
    truth = {3: (-3210.0, 777.0), 5: (912.5, 1600.0), 11: (4480.0, 12001.0), 14: (4037.0, 4000.0), 20: (-1025.0, 9000.0), 30: (2018.0, 13000.0)}
    prns = np.array(sorted(truth), np.uint8)

    def hits(pk):
        h = 0
        for i, p in enumerate(prns):
            dopp, delay = truth[int(p)]
            bb = pk[:, i, :]["max_val"].argmax(axis=1)
            best = pk[np.arange(n), i, bb]
            ok = (np.abs(-5000 + 500 * bb - dopp) <= 500) & (np.abs((best["phase"].astype(int) - delay + 8184) % 16368 - 8184) <= 8)
            h += int(ok.sum())
        return h

    ten = hits(eng.acq_grid_weighted_ms(blocks, prns, n, 10, -5000, 500, 21))
    one = hits(eng.acq_grid_weighted_ms(blocks, prns, n, 1, -5000, 500, 21, stride_blocks=10))
    sign = hits(eng.acq_grid_weighted_ms(blocks, prns, n, 10, -5000, 500, 21, use_magnitude=False))
    print("acquired of", 6 * n, ": ten weighted blocks", ten, "one weighted block", one, "ten sign-plane blocks", sign)
    assert ten >= 30 and ten > 2 * sign and ten > 3 * one + 10
