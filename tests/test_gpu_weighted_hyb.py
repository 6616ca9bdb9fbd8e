"""The weighted two-bit grid over n_seg coherent windows of n_coh blocks each, the windows' magnitudes summed (EXTENSION, not in the
reference: include/gpsx.h gpsx_acq_grid_weighted_hyb; k_acq_hyb_mx on the matrix cores, k_acq_hyb_vec on the vector ALU) against
its exact CPU restatement (tests/weighted_hyb_ref.py, pinned in tests/test_weighted_hyb_reference.py): records on both paths over
PRN lists, window shapes from 2 x 2 to 2 x 128, strides, weight modes and a non-default IF; degenerate captures at 20 x 3 and
10 x 8; one window / one-block windows against the two older calls, byte for byte; a launch that fills the chip and is chunked;
the argument checks; and what the call is for -- on a stream with data bits, eight windows of ten blocks acquire what neither the
best single window nor eighty non-coherent blocks do."""
import ctypes as C
import os

import numpy as np
import pytest

import weighted_coh_ref as R
import weighted_hyb_ref as H

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
    return b"k_acq_hyb_mx" if path == "matrix" else b"k_acq_hyb_vec"


def _same(got, want, what):
    for f in FIELDS:
        assert np.array_equal(got[f], want[f]), (what, f, np.argwhere(got[f] != want[f])[:4].tolist())


def _blocks(n, amp=0.3, seed=3):
    from stm32f4_sdr_gps_amd import synth
    sats = [synth.Sat(7, 1310.0, 4321.0, amp, 0.4), synth.Sat(19, -2240.0, 12007.0, amp, 2.0), synth.Sat(30, 2018.0, 13000.0, amp, 4.0)]
    return synth.make_if_static(n, sats, noise_amp=1.0, seed=seed, two_bit=True)


# (PRNs, n_search, n_coh, n_seg, stride, dopp_min, dopp_step, n_dopp, use_magnitude, restated units or None for all)
CASES = [
    (np.array([19], np.uint8), 3, 2, 2, 1, -2240, 250, 2, True, None),                               # overlapping searches
    (np.array([7, 19, 30, 1, 2, 3, 150, 5, 6, 210, 9], np.uint8), 2, 3, 5, 15, -2500, 150, 3, False, None),   # PRNs above 32
    (np.arange(1, 17, dtype=np.uint8), 2, 10, 8, 0, 1000, 50, 2, True,                               # stride 0: the same 80 blocks
     [(0, 0, 0), (1, 6, 1), (0, 8, 1), (1, 15, 0), (0, 11, 0)]),
    (np.arange(1, 41, dtype=np.uint8), 1, 20, 3, 60, 1310, 25, 1, True,                              # two 32-PRN sets, the second
     [(0, p, 0) for p in (0, 6, 18, 31, 32, 35, 39)]),                                               # partial (a list of 40)
    (np.arange(25, 41, dtype=np.uint8), 2, 5, 25, 10, 2000, 100, 1, False,                           # overlapping, sign plane only
     [(0, 0, 0), (1, 5, 0), (1, 8, 0), (0, 15, 0)]),
    (np.array([7, 19, 30], np.uint8), 2, 2, 128, 3, -2240, 250, 1, True, None),                      # the most windows
]


@pytest.mark.parametrize("path", ["matrix", "vector"])
def test_records_match_the_reference(eng, oracle, path):
    blocks = _blocks(259)
    kernel = _path(eng, path)
    try:
        for prns, n_search, n_coh, n_seg, stride, d0, ds, nd, um, units in CASES:
            got = eng.acq_grid_weighted_hyb(blocks, prns, n_search, n_coh, n_seg, d0, ds, nd, use_magnitude=um, stride_blocks=stride)
            assert eng.lib.gpsx_last_kernel(eng.h) == kernel
            want = H.grid(oracle, blocks, n_search, prns, n_coh, n_seg, d0, ds, nd, um, stride=stride, units=units)
            if units is not None:
                idx = tuple(np.array(units).T)
                got, want = got[idx], want[idx]
            _same(got, want, (len(prns), n_coh, n_seg, stride))
    finally:
        _path(eng, "matrix")


@pytest.mark.parametrize("path", ["matrix", "vector"])
def test_non_default_if(path, oracle):
    from stm32f4_sdr_gps_amd import capi
    blocks = _blocks(14, seed=8)
    prns = np.array([7, 19, 44], np.uint8)
    e = capi.Engine(0)
    try:
        e.set_config(if_hz=4_100_000)
        kernel = _path(e, path)
        got = e.acq_grid_weighted_hyb(blocks, prns, 2, 3, 4, -3000, 250, 3, stride_blocks=2)
        assert e.lib.gpsx_last_kernel(e.h) == kernel
    finally:
        e.close()
    _same(got, H.grid(oracle, blocks, 2, prns, 3, 4, -3000, 250, 3, True, stride=2, if_hz=4_100_000), "if_hz")


@pytest.mark.parametrize("path", ["matrix", "vector"])
def test_degenerate_captures_at_20x3_and_10x8(eng, oracle, path):
    """a clean strong satellite, all-0xFF, every magnitude bit set, and per segment the blocks whose wiped I is 3 x the replica
    (I_j = 3 x 16352 x n_coh in every segment -- 981 120 at n_coh = 20, the top of the range -- so E(0) >= n_seg x that)"""
    from stm32f4_sdr_gps_amd import synth
    strong = synth.make_if_static(80, [synth.Sat(7, 1310.0, 4321.0, 4.0, 0.4)], noise_amp=0.05, seed=5, two_bit=True)
    flat = np.full_like(strong, 0xFF)
    mag_set = strong | np.uint8(0xAA)
    prns = np.array([7, 8], np.uint8)
    kernel = _path(eng, path)
    try:
        for n_coh, n_seg in ((20, 3), (10, 8)):
            matched = np.concatenate([R.code_matched_blocks(oracle, 8, 4092000 + 1310, n_coh)] * n_seg)
            for blocks in (strong, flat, mag_set, matched):
                got = eng.acq_grid_weighted_hyb(blocks, prns, 1, n_coh, n_seg, 810, 500, 2)
                assert eng.lib.gpsx_last_kernel(eng.h) == kernel
                _same(got, H.grid(oracle, blocks, 1, prns, n_coh, n_seg, 810, 500, 2, True), (n_coh, n_seg))
            assert got[0, 1, 1]["max_val"] >= n_seg * 3 * 16352 * n_coh and got[0, 1, 1]["phase"] == 0
    finally:
        _path(eng, "matrix")


@pytest.mark.parametrize("path", ["matrix", "vector"])
def test_degenerate_arguments_are_the_older_calls(eng, path):
    """n_seg = 1 is gpsx_acq_grid_weighted_coh, n_coh = 1 is gpsx_acq_grid_weighted_ms with n_ms = n_seg: their kernels, their bytes"""
    blocks = _blocks(12)
    prns = np.array([7, 19, 30, 2, 3], np.uint8)
    _path(eng, path)
    try:
        for um in (True, False):
            old = eng.acq_grid_weighted_coh(blocks, prns, 3, 5, -1000, 100, 3, use_magnitude=um, stride_blocks=2)
            k_old = eng.lib.gpsx_last_kernel(eng.h)
            new = eng.acq_grid_weighted_hyb(blocks, prns, 3, 5, 1, -1000, 100, 3, use_magnitude=um, stride_blocks=2)
            assert eng.lib.gpsx_last_kernel(eng.h) == k_old == (b"k_acq_coh_mx" if path == "matrix" else b"k_acq_coh_vec")
            assert new.tobytes() == old.tobytes()
            old = eng.acq_grid_weighted_ms(blocks, prns, 3, 6, -1000, 500, 3, use_magnitude=um, stride_blocks=2)
            k_old = eng.lib.gpsx_last_kernel(eng.h)
            new = eng.acq_grid_weighted_hyb(blocks, prns, 3, 1, 6, -1000, 500, 3, use_magnitude=um, stride_blocks=2)
            assert eng.lib.gpsx_last_kernel(eng.h) == k_old == (b"k_acq_wmx_ms" if path == "matrix" else b"k_acq_weighted_ms")
            assert new.tobytes() == old.tobytes()
            old = eng.acq_grid_weighted(blocks, prns, 3, -1000, 500, 3, use_magnitude=um, stride_blocks=2)
            k_old = eng.lib.gpsx_last_kernel(eng.h)
            new = eng.acq_grid_weighted_hyb(blocks, prns, 3, 1, 1, -1000, 500, 3, use_magnitude=um, stride_blocks=2)
            assert eng.lib.gpsx_last_kernel(eng.h) == k_old == (b"k_acq_mxw" if path == "matrix" else b"k_acq_weighted")
            assert new.tobytes() == old.tobytes()
    finally:
        _path(eng, "matrix")


def test_chip_filling_launch_both_paths_and_chunks(eng, oracle):
    """256 searches x 32 PRNs x 21 Doppler bins, 10 x 8 (20 480 random blocks; 5376 clusters, 10.5 GB of running sums at one launch:
    six chunks under the default 2 GB cap): the two paths byte-identical, one seeded unit per (Doppler bin, 8-PRN group) plus the
    first and the last unit against the reference (a bin's four units in one seeded search: they share the restated spectra), and
    the lab library with the scratch capped at 1 GB (eleven chunks) byte-identical again"""
    from stm32f4_sdr_gps_amd import capi
    rng = np.random.default_rng(29)
    blocks = rng.integers(0, 256, (20480, 4092), dtype=np.uint8)
    prns = np.arange(1, 33, dtype=np.uint8)
    mx = eng.acq_grid_weighted_hyb(blocks, prns, 256, 10, 8, -5000, 50, 21)
    assert eng.lib.gpsx_last_kernel(eng.h) == b"k_acq_hyb_mx"
    _path(eng, "vector")
    try:
        vec = eng.acq_grid_weighted_hyb(blocks, prns, 256, 10, 8, -5000, 50, 21)
        assert eng.lib.gpsx_last_kernel(eng.h) == b"k_acq_hyb_vec"
    finally:
        _path(eng, "matrix")
    assert mx.tobytes() == vec.tobytes()
    units = []
    for d in range(21):
        s = int(rng.integers(0, 256))
        units += [(s, 8 * g + int(rng.integers(0, 8)), d) for g in range(4)]
    units += [(0, 0, 0), (255, 31, 20)]
    want = H.grid(oracle, blocks, 256, prns, 10, 8, -5000, 50, 21, True, units=units)
    idx = tuple(np.array(units).T)
    _same(mx[idx], want[idx], "sampled units")
    os.environ["GPSX_ACQ_WMS_SCRATCH_MB"] = "1024"
    try:
        lab = capi.Engine(0, lab=True)
    finally:
        del os.environ["GPSX_ACQ_WMS_SCRATCH_MB"]
    try:
        chunked = lab.acq_grid_weighted_hyb(blocks, prns, 256, 10, 8, -5000, 50, 21)
        assert lab.lib.gpsx_last_kernel(lab.h) == b"k_acq_hyb_mx"
    finally:
        lab.close()
    assert chunked.tobytes() == mx.tobytes()


@pytest.mark.parametrize("path", ["matrix", "vector"])
def test_argument_checks_write_nothing(eng, path):
    from stm32f4_sdr_gps_amd import capi
    blocks = _blocks(12)
    _path(eng, path)
    try:
        # (PRN, n_search, n_coh, n_seg, stride, weights, null capture, null records) on 12 blocks
        for prn, n_search, n_coh, n_seg, stride, wt, null_if, null_pk in (
                (5, 1, 0, 2, 1, 1, 0, 0), (5, 1, 21, 2, 1, 1, 0, 0), (5, 1, 2, 0, 1, 1, 0, 0), (5, 1, 2, 129, 1, 1, 0, 0),
                (5, 1, 13, 1, 1, 1, 0, 0), (5, 1, 1, 13, 1, 1, 0, 0),            # one block too few, one search
                (5, 1, 4, 4, 1, 1, 0, 0), (5, 2, 3, 4, 1, 1, 0, 0),              # 16 > 12; 1 + 12 > 12 with a second search
                (5, 1, 2, 3, 2, 2, 0, 0), (5, 1, 2, 3, 2, -1, 0, 0), (0, 1, 2, 3, 2, 1, 0, 0), (211, 1, 2, 3, 2, 1, 0, 0),
                (5, 1, 2, 3, 2, 1, 1, 0), (5, 1, 2, 3, 2, 1, 0, 1)):
            prns = np.array([prn, 7], np.uint8)
            g = capi.AcqWeightedT(n_search, stride, 2, prns.ctypes.data_as(C.POINTER(C.c_uint8)), 0, 500, 1, wt)
            peaks = np.zeros((n_search, 2, 1), capi.PEAK_DTYPE)
            peaks.view(np.uint8)[...] = 0xA5
            rc = eng.lib.gpsx_acq_grid_weighted_hyb(eng.h, C.byref(g), n_coh, n_seg, None if null_if else blocks.ctypes.data, 12,
                                                    None if null_pk else peaks.ctypes.data)
            assert rc == -22 and eng.lib.gpsx_last_error(eng.h), (prn, n_search, n_coh, n_seg, stride, wt)
            assert (peaks.view(np.uint8) == 0xA5).all()
        rc = eng.lib.gpsx_acq_grid_weighted_hyb(eng.h, None, 2, 3, blocks.ctypes.data, 12, peaks.ctypes.data)
        assert rc == -22 and eng.lib.gpsx_last_error(eng.h) and (peaks.view(np.uint8) == 0xA5).all()
    finally:
        _path(eng, "matrix")


def test_windows_summed_acquire_what_one_window_and_eighty_blocks_miss(eng):
    """Eight captures of 90 blocks from one stream WITH random 50 bit/s data on every satellite (synth.make_if, the bench's six
    satellites at amplitude scale 0.015, far below the noise), each searched over 80 blocks starting 5 blocks after a bit edge, so
    every second 10-block window straddles one.  Three integrations of the same 80 blocks: eight coherent windows of ten summed
    non-coherently on 50 Hz bins (this call); the better of the eight windows on their own (the coherent call: per capture and PRN
    the window whose best bin has the largest max_val); eighty non-coherent blocks on 500 Hz bins.  A (capture, satellite) pair
    acquires by weighted_coh_ref.hits' rule.  Calibrated on the CPU restatements, whose records the GPU computes exactly:
    37, 2 and 10 of 48.  Asserted with margin against a changed numpy or synthesis detail: at least 30, and at least 15 more than
    either of the others."""
    from stm32f4_sdr_gps_amd import synth
    base = [(3, -3210.0, 777.0, 0.5, 0.7), (5, 912.5, 1600.0, 0.6, 0.3), (11, 4480.0, 12001.0, 0.5, 5.1),
            (14, 4037.0, 4000.0, 0.6, 1.1), (20, -1025.0, 9000.0, 0.6, 2.5), (30, 2018.0, 13000.0, 0.6, 4.0)]
    truth = {p: (f, d) for p, f, d, a, ph in base}
    prns = np.array(sorted(truth), np.uint8)
    rng = np.random.Generator(np.random.PCG64(511))
    sats = [synth.Sat(p, f, d, a * 0.015, ph, 1.0 - 2.0 * rng.integers(0, 2, 64).astype(np.float64)) for p, f, d, a, ph in base]
    n = 8
    blocks = synth.make_if(n * 90, sats, noise_amp=1.0, seed=11, two_bit=True)[5:]
    hyb = R.hits(eng.acq_grid_weighted_hyb(blocks, prns, n, 10, 8, -5000, 50, 201, stride_blocks=90), prns, truth, n, -5000, 50)
    assert eng.lib.gpsx_last_kernel(eng.h) == b"k_acq_hyb_mx"
    win = eng.acq_grid_weighted_coh(blocks, prns, 71, 10, -5000, 50, 201, stride_blocks=10)   # capture c: searches 9 c .. 9 c + 7
    best = np.zeros_like(win[:n])
    for c in range(n):
        for p in range(len(prns)):
            j = int(np.argmax([win[9 * c + j, p]["max_val"].max() for j in range(8)]))
            best[c, p] = win[9 * c + j, p]
    one = R.hits(best, prns, truth, n, -5000, 50)
    nc = R.hits(eng.acq_grid_weighted_ms(blocks, prns, n, 80, -5000, 500, 21, stride_blocks=90), prns, truth, n, -5000, 500)
    print("acquired of", 6 * n, ": 10 x 8 hybrid", hyb, "best single window", one, "80 non-coherent blocks", nc)
    assert hyb >= 30 and hyb >= nc + 15 and hyb >= one + 15
