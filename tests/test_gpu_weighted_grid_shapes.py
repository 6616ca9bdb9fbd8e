"""The eight weighted acquisition kernels (k_acq_mxw, k_acq_weighted, k_acq_wmx_ms, k_acq_weighted_ms, k_acq_coh_mx, k_acq_coh_vec,
k_acq_hyb_mx, k_acq_hyb_vec) where tests/test_gpu_weighted{,_ms,_coh,_hyb}.py do not take them, on tests/weighted_grid_cases.py's
cases (pinned in tests/test_weighted_grid_cases_reference.py) and against the exact restatements tests/weighted_{ms,coh,hyb}_ref.py:
the four _dev entry points on the caller's own device memory, capture and records between canaries, over PRN lists on the edges
of a group of 8 and a set of 32 up to 255 slots with repeats; the two scratch walks under caps that cut the call below a round,
unevenly, inside a (search, Doppler) pair and across a search, and the GPSX_ENOMEM exit; one context serving sign-only walks and
every weighted form in turn; max_val at the top of a block's range and a sum past 2^32; and a Doppler axis walked with a zero and
a negative step.  Every comparison is equality."""
import ctypes as C
import os

import numpy as np
import pytest

import weighted_coh_ref as R
import weighted_grid_cases as G
import weighted_hyb_ref as H
import weighted_ms_ref as W
from weighted_gpu import Guarded, Pool, STATE_FILL, OUT_FILL, eng      # noqa: F401 -- eng: the module's engine fixture

pytestmark = pytest.mark.gpu

FIELDS = ("max_val", "phase", "sum", "avr")
ENOMEM = -12
PATHS = ("matrix", "vector")
# call -> (its window arguments, the blocks one search reads, its kernel on the matrix cores, on the vector ALU)
CALLS = {"w": ((), 1, b"k_acq_mxw", b"k_acq_weighted"), "ms": ((3,), 3, b"k_acq_wmx_ms", b"k_acq_weighted_ms"),
         "coh": ((3,), 3, b"k_acq_coh_mx", b"k_acq_coh_vec"), "hyb": ((2, 2), 4, b"k_acq_hyb_mx", b"k_acq_hyb_vec")}


def _path(e, path):
    from stm32f4_sdr_gps_amd import capi
    e.set_acq_path(capi.ACQ_PATH_MATRIX if path == "matrix" else capi.ACQ_PATH_VECTOR)


def _same(got, want, what):
    for f in FIELDS:
        assert np.array_equal(got[f], want[f]), (what, f, np.argwhere(got[f] != want[f])[:4].tolist())


def _desc(prns, n_search, stride, d0, ds, nd):
    from stm32f4_sdr_gps_amd import capi
    return capi.AcqWeightedT(n_search, stride, len(prns), prns.ctypes.data_as(C.POINTER(C.c_uint8)), d0, ds, nd, 1)


def _dev_rc(e, call, win, g, d_if, n_blocks, d_peaks):
    """the _dev entry point of `call` on device pointers -> its return code (nothing is waited for)"""
    name = {"w": "gpsx_acq_grid_weighted_dev", "ms": "gpsx_acq_grid_weighted_ms_dev", "coh": "gpsx_acq_grid_weighted_coh_dev",
            "hyb": "gpsx_acq_grid_weighted_hyb_dev"}[call]
    return getattr(e.lib, name)(e.h, C.byref(g), *win, d_if, n_blocks, d_peaks)


def _dev(e, call, win, blocks, prns, n_search, d0, ds, nd, kernel, stride=1, fill=STATE_FILL):
    """one _dev call on the caller's memory: exactly the blocks passed between canaries of `fill`, the records prefilled with 0xA5
    between canaries -> the records, after a look at the canaries and at every record's having been written"""
    prns = np.ascontiguousarray(prns, np.uint8)
    blocks = np.ascontiguousarray(blocks, np.uint8).reshape(-1, 4092)
    shape = (n_search, len(prns), nd)
    with Pool() as pool:
        cap = pool.add(Guarded(e, blocks.nbytes, fill, blocks))
        out = pool.add(Guarded(e, int(np.prod(shape)) * 16))
        rc = _dev_rc(e, call, win, _desc(prns, n_search, stride, d0, ds, nd), cap.ptr, len(blocks), out.ptr)
        assert rc == 0, (rc, e.lib.gpsx_last_error(e.h))
        assert e.lib.gpsx_last_kernel(e.h) == kernel
        e.synchronize()
        assert cap.untouched(), "the capture or its canaries were written"
        from stm32f4_sdr_gps_amd import capi
        got = out.get(capi.PEAK_DTYPE, shape)
    assert (got["max_val"] != 0xA5A5A5A5).all(), ("records left at their prefill", np.argwhere(got["max_val"] == 0xA5A5A5A5)[:4].tolist())
    return got


def _host(e, call, win, blocks, prns, n_search, d0, ds, nd, stride=1):
    if call == "w":
        return e.acq_grid_weighted(blocks, prns, n_search, d0, ds, nd, stride_blocks=stride)
    fn = {"ms": e.acq_grid_weighted_ms, "coh": e.acq_grid_weighted_coh, "hyb": e.acq_grid_weighted_hyb}[call]
    return fn(blocks, prns, n_search, *win, d0, ds, nd, stride_blocks=stride)


def _restated(oracle, call, win, blocks, prns, n_search, d0, ds, nd, stride=1, units=None):
    if call in ("w", "ms"):
        return W.grid(oracle, blocks, n_search, prns, win[0] if win else 1, d0, ds, nd, stride=stride, units=units)
    ref = R if call == "coh" else H
    return ref.grid(oracle, blocks, n_search, prns, *win, d0, ds, nd, stride=stride, units=units)


# ---- 1. the _dev calls on guarded memory, PRN lists on every edge ---------------------------------------------------------------
D0, DS = -2240, 3550      # two bins: a satellite's and an empty one


@pytest.mark.parametrize("n", G.LENGTHS)
@pytest.mark.parametrize("call", list(CALLS))
def test_dev_calls_on_guarded_memory(eng, oracle, call, n):
    """2 searches x n PRNs x 2 Doppler bins at stride 1, the last search ending on the last block passed.  Per path: the _dev call
    with the capture followed by 0x5A and by 0xA5 and the host call, the same bytes from all three; the same bytes from both paths;
    the slots of a repeated PRN alike; and the restatement -- of every record up to 65 PRNs, of weighted_grid_cases.sample_units' at 255"""
    win, span, k_mx, k_vec = CALLS[call]
    prns = G.prn_list(n)
    blocks = G.noisy_blocks(5)[:1 + span]
    args = (blocks, prns, 2, D0, DS, 2)
    by_path = {}
    try:
        for path in PATHS:
            _path(eng, path)
            kernel = k_mx if path == "matrix" else k_vec
            got = _dev(eng, call, win, *args, kernel, fill=STATE_FILL)
            assert _dev(eng, call, win, *args, kernel, fill=OUT_FILL).tobytes() == got.tobytes(), (path, "the bytes behind the capture show")
            assert _host(eng, call, win, *args).tobytes() == got.tobytes(), (path, "host and _dev differ")
            assert eng.lib.gpsx_last_kernel(eng.h) == kernel
            by_path[path] = got
    finally:
        _path(eng, "matrix")
    got = by_path["matrix"]
    assert by_path["vector"].tobytes() == got.tobytes()
    for slots in G.duplicates(prns):
        for s in slots[1:]:
            assert got[:, s].tobytes() == got[:, slots[0]].tobytes(), ("slots of one PRN differ", slots[0], s)
    units = G.sample_units(prns, 2, 2) if n > 65 else None
    want = _restated(oracle, call, win, *args, units=units)
    if units is not None:
        idx = tuple(np.array(units).T)
        got, want = got[idx], want[idx]
    _same(got, want, (call, n))


@pytest.mark.parametrize("path", PATHS)
def test_255_prns_one_block_every_record(eng, oracle, path):
    prns = G.prn_list(255)
    blocks = G.noisy_blocks(5)[4:]
    _path(eng, path)
    try:
        got = _dev(eng, "w", (), blocks, prns, 1, 1310, 500, 1, CALLS["w"][2 if path == "matrix" else 3])
    finally:
        _path(eng, "matrix")
    _same(got, W.grid(oracle, blocks, 1, prns, 1, 1310, 500, 1, stride=1), path)


# ---- 2. the scratch walks in chunks ----------------------------------------------------------------------------------------------
def _lab(cap_mb):
    from stm32f4_sdr_gps_amd import capi
    os.environ["GPSX_ACQ_WMS_SCRATCH_MB"] = str(cap_mb)
    try:
        return capi.Engine(0, lab=True)
    finally:
        del os.environ["GPSX_ACQ_WMS_SCRATCH_MB"]


def _chunk_calls():
    c = G.CHUNK
    blocks = G.noisy_blocks(7, seed=12)
    grid = (c["n_search"], c["dopp_min_hz"], c["dopp_step_hz"], c["n_dopp"])
    return {"ms": ((c["n_ms"],), blocks[:c["n_search"] - 1 + c["n_ms"]], grid),
            "hyb": ((c["n_coh"], c["n_seg"]), blocks[:c["n_search"] - 1 + c["n_coh"] * c["n_seg"]], grid)}


@pytest.fixture(scope="module")
def chunk_want(oracle):
    """all 240 records of the chunk call, as _ms and as _hyb: restated once"""
    return {call: _restated(oracle, call, win, blocks, G.chunk_prns(), *grid) for call, (win, blocks, grid) in _chunk_calls().items()}


@pytest.mark.parametrize("cap_mb", list(G.CHUNK_CAPS_MB))
def test_chunked_walks(eng, chunk_want, cap_mb):
    """1, 3, 5 and 7 clusters a launch on 12 (12, 4, 3 and 2 launches: tests/test_weighted_grid_cases_reference.py) against the
    restatement and against the product library's single launch, byte for byte"""
    prns = G.chunk_prns()
    lab = _lab(cap_mb)
    try:
        for call, (win, blocks, grid) in _chunk_calls().items():
            kernel = CALLS[call][2]
            got = _dev(lab, call, win, blocks, prns, *grid, kernel)
            _same(got, chunk_want[call], (call, cap_mb))
            assert got.shape == (2, 40, 3) and got.size == 240
            assert _dev(eng, call, win, blocks, prns, *grid, kernel).tobytes() == got.tobytes(), (call, cap_mb)
    finally:
        lab.close()


def test_no_scratch_for_one_cluster_is_enomem_and_the_engine_serves_on(eng, oracle):
    """under a cap of 1 MB both walks are refused on the host, before any launch: GPSX_ENOMEM, a text that names the kernel, not a
    byte written; the calls that need no scratch then run on the same engine"""
    from stm32f4_sdr_gps_amd import capi
    prns = G.chunk_prns()
    lab = _lab(G.CHUNK_REFUSED_MB)
    try:
        for call, (win, blocks, grid) in _chunk_calls().items():
            with Pool() as pool:
                cap = pool.add(Guarded(lab, blocks.nbytes, STATE_FILL, blocks))
                out = pool.add(Guarded(lab, 240 * 16))
                rc = _dev_rc(lab, call, win, _desc(prns, grid[0], 1, *grid[1:]), cap.ptr, len(blocks), out.ptr)
                assert rc == ENOMEM and CALLS[call][2] in lab.lib.gpsx_last_error(lab.h), (call, rc, lab.lib.gpsx_last_error(lab.h))
                lab.synchronize()
                assert out.untouched() and cap.untouched()
            peaks = np.zeros((2, 40, 3), capi.PEAK_DTYPE)                                   # the host call alike
            peaks.view(np.uint8)[...] = OUT_FILL
            before = peaks.tobytes()
            g = _desc(prns, grid[0], 1, *grid[1:])
            fn = lab.lib.gpsx_acq_grid_weighted_ms if call == "ms" else lab.lib.gpsx_acq_grid_weighted_hyb
            assert fn(lab.h, C.byref(g), *win, blocks.ctypes.data, len(blocks), peaks.ctypes.data) == ENOMEM
            assert peaks.tobytes() == before
        few = np.array([7, 19, 210], np.uint8)
        blocks = G.noisy_blocks(7, seed=12)[:4]
        for call, path in (("w", "matrix"), ("coh", "matrix"), ("ms", "vector")):
            win = CALLS[call][0]
            _path(lab, path)
            got = _dev(lab, call, win, blocks[:1 + CALLS[call][1]], few, 2, D0, DS, 2, CALLS[call][2 if path == "matrix" else 3])
            _same(got, _restated(oracle, call, win, blocks[:1 + CALLS[call][1]], few, 2, D0, DS, 2), (call, path))
            assert _dev(eng, call, win, blocks[:1 + CALLS[call][1]], few, 2, D0, DS, 2, CALLS[call][2]).tobytes() == got.tobytes()
    finally:
        lab.close()


# ---- 3. one context, interleaved ------------------------------------------------------------------------------------------------
def test_one_context_serves_every_form_in_turn(oracle):
    """One product engine's scratch (three layouts: the sign-only walk's, k_acq_wmx_ms's, k_acq_hyb_mx's), its cached code tables
    (keyed by the PRN list, shared with the sign-only grid) and its staged PRN list, across sign-only ten-block walks, the matrix
    walks, the one-block, the coherent and the vector forms, PRN lists of 65, 3, 33, another 3 and the first 3 again: a first
    answer is its restatement's (the sign-only grid's: its own, on the fresh engine), and every repeat returns the first answer's bytes"""
    from stm32f4_sdr_gps_amd import capi
    p65, p33, p3a, p3b = G.prn_list(65), G.prn_list(33), np.array([7, 19, 210], np.uint8), np.array([30, 1, 19], np.uint8)
    blocks = G.noisy_blocks(5)
    sign = np.random.default_rng(41).integers(0, 256, (22, 2046), dtype=np.uint8)
    e = capi.Engine(0)
    first = {}

    def sign_walk():
        """13 searches x 21 bins of ten blocks: 273 clusters, more than a round of the chip -- the walk form, both widths of sums"""
        pk, keys = e.acq_grid(sign, p3a, n_search=13, n_ms=10, search_stride_blocks=1, dopp_min_hz=-5000, dopp_step_hz=500, n_dopp=21)
        assert e.lib.gpsx_last_kernel(e.h) == b"k_acq_mx<3>"
        return pk.tobytes() + keys.tobytes()

    def sign_one():
        pk, keys = e.acq_grid(sign, p3a, n_search=2, n_ms=1, search_stride_blocks=1, dopp_min_hz=-5000, dopp_step_hz=500, n_dopp=21)
        return pk.tobytes() + keys.tobytes()

    def weighted(call, prns, path="matrix"):
        win, span, k_mx, k_vec = CALLS[call]
        _path(e, path)
        try:
            return _dev(e, call, win, blocks[:1 + span], prns, 2, D0, DS, 2, k_mx if path == "matrix" else k_vec)
        finally:
            _path(e, "matrix")

    def step(what, fn, *args, **kw):
        """a first answer is kept (and restated, for a weighted call); a repeat must return its bytes"""
        got = fn(*args, **kw)
        key = (what,) + tuple(a.tobytes() if isinstance(a, np.ndarray) else a for a in args)
        if key not in first:
            first[key] = got if isinstance(got, bytes) else got.tobytes()
            if fn is weighted:
                win, span = CALLS[args[0]][:2]
                _same(got, _restated(oracle, args[0], win, blocks[:1 + span], args[1], 2, D0, DS, 2), (what, len(first)))
        assert (got if isinstance(got, bytes) else got.tobytes()) == first[key], (what, "differs from its first answer")

    try:
        step("one block", weighted, "w", p65)
        step("sign walk", sign_walk)
        step("ms", weighted, "ms", p33)
        step("sign walk", sign_walk)
        step("hyb", weighted, "hyb", p3a)
        step("ms", weighted, "ms", p33)
        step("sign walk", sign_walk)
        step("one block", weighted, "w", p3a)
        step("sign one block", sign_one)
        step("coh", weighted, "coh", p33)
        step("one block", weighted, "w", p3b)                     # another list of the same length
        step("one block", weighted, "w", p3a)
        step("sign one block", sign_one)
        step("ms", weighted, "ms", p3b)
        step("ms", weighted, "ms", p3a)
        step("coh", weighted, "coh", p3b)                         # the staged list: another of the same length behind hyb's and ms's
        step("hyb", weighted, "hyb", p3b)
        step("coh", weighted, "coh", p3a)
        # matrix -> vector -> matrix
        for call, prns in (("ms", p33), ("w", p65), ("hyb", p3a), ("hyb", p3b), ("coh", p33), ("ms", p3a), ("ms", p3b), ("w", p3a), ("w", p3b)):
            assert weighted(call, prns, path="vector").tobytes() == first[(("one block" if call == "w" else call), call, prns.tobytes())], (call, len(prns))
        step("hyb", weighted, "hyb", p3a)
        step("ms", weighted, "ms", p33)
        step("one block", weighted, "w", p65)
        step("coh", weighted, "coh", p33)
        step("sign walk", sign_walk)
        step("one block", weighted, "w", p3b)
        step("sign one block", sign_one)
    finally:
        e.close()


# ---- 4. the top of the range and a wrapped sum ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_matched_block_reaches_the_top_of_the_range(eng, oracle, path):
    """I(0) = 3 x 16352, Q(0) = 0 (tests/test_weighted_grid_cases_reference.py): max_val = 49 056 x n_ms at phase 0"""
    blk = G.matched_block(oracle)
    prns = np.array([G.TOP_PRN, 7], np.uint8)
    grid = (1, G.TOP_DOPP_HZ, 500, 1)
    _path(eng, path)
    try:
        one = _host(eng, "w", (), blk, prns, *grid)
        assert eng.lib.gpsx_last_kernel(eng.h) == CALLS["w"][2 if path == "matrix" else 3]
        assert _host(eng, "ms", (1,), blk, prns, *grid).tobytes() == one.tobytes()
        four = _host(eng, "ms", (4,), np.tile(blk, (4, 1)), prns, *grid)
        assert eng.lib.gpsx_last_kernel(eng.h) == CALLS["ms"][2 if path == "matrix" else 3]
    finally:
        _path(eng, "matrix")
    for n_ms, got in ((1, one), (4, four)):
        assert (int(got[0, 0, 0]["max_val"]), int(got[0, 0, 0]["phase"])) == (G.TOP_I * n_ms, 0), (n_ms, got[0, 0, 0])
        _same(got, W.grid(oracle, np.tile(blk, (n_ms, 1)), 1, prns, n_ms, G.TOP_DOPP_HZ, 500, 1), (path, n_ms))


@pytest.fixture(scope="module")
def wrap_want(oracle):
    """the wrapping capture's search restated once: {n_seg: [per PRN (the unwrapped sum, the record)]}"""
    by_prn = [G.wrap_energy(oracle, prn) for prn in G.WRAP_PRNS]
    return {n_seg: [(int(e[n_seg].sum()), W.fold(e[n_seg])) for e in by_prn] for n_seg in G.WRAP_SEGS}


@pytest.mark.parametrize("path", PATHS)
def test_hybrid_sum_wraps_past_2_to_the_32(eng, wrap_want, path):
    """20 x 128 on a capture whose sum over the phases is 4 440 768 896 for PRN 7: `sum` is that mod 2^32, by the matrix route (HBM
    records, per-lane totals, a 32-lane fold) and by the vector route (registers and LDS) alike; 20 x 64 on its first half, where
    the sum is 2 220 384 448: every bit of a u32 total is used before it wraps"""
    half, full = (wrap_want[n_seg][0] for n_seg in G.WRAP_SEGS)
    assert full[0] >> 32 >= 1 and full[1][2] == full[0] - (1 << 32)
    assert 1 << 31 <= half[0] < 1 << 32 and half[1][2] == half[0]
    prns = np.array(G.WRAP_PRNS, np.uint8)
    _path(eng, path)
    try:
        for n_seg in G.WRAP_SEGS:
            got = eng.acq_grid_weighted_hyb(G.wrap_capture()[:G.WRAP_N_COH * n_seg], prns, 1, G.WRAP_N_COH, n_seg, G.WRAP_DOPP_HZ, 500, 1)
            assert eng.lib.gpsx_last_kernel(eng.h) == CALLS["hyb"][2 if path == "matrix" else 3]
            for k, (total, record) in enumerate(wrap_want[n_seg]):
                assert tuple(int(got[0, k, 0][f]) for f in FIELDS) == record, (path, n_seg, G.WRAP_PRNS[k], total, got[0, k, 0])
    finally:
        _path(eng, "matrix")


# ---- 5. the Doppler axis ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("call", list(CALLS))
def test_doppler_axis_with_zero_and_negative_steps(eng, call, path):
    """f = (float)(if_hz + dopp_min_hz + d * dopp_step_hz) whatever the step's sign: a zero step gives the same record three times
    (the ascending call's in that bin), a negative step from the top the ascending call's records in reverse"""
    win, span, k_mx, k_vec = CALLS[call]
    prns = np.array([7, 19, 30, 1, 2, 3, 150, 5, 6, 210, 9], np.uint8)
    blocks = G.noisy_blocks(5)[:1 + span]
    kernel = k_mx if path == "matrix" else k_vec
    _path(eng, path)
    try:
        up = _dev(eng, call, win, blocks, prns, 2, -2240, 1775, 3, kernel)
        down = _dev(eng, call, win, blocks, prns, 2, -2240 + 2 * 1775, -1775, 3, kernel)
        still = _dev(eng, call, win, blocks, prns, 2, -465, 0, 3, kernel)
    finally:
        _path(eng, "matrix")
    assert np.ascontiguousarray(down[:, :, ::-1]).tobytes() == up.tobytes()
    for d in range(3):
        assert np.ascontiguousarray(still[:, :, d]).tobytes() == np.ascontiguousarray(up[:, :, 1]).tobytes(), d
