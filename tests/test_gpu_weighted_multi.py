"""The sync loop for many receivers per launch on the device (EXTENSION, not in the reference: include/gpsx.h
gpsx_track_loop_weighted_sync_multi; k_track_wsync_multi, a workgroup per receiver) against the exact CPU restatement applied per
receiver (tests/weighted_sync_ref.py with tests/weighted_aided_ref.py, the cases of tests/weighted_multi_cases.py, whose grounds
tests/test_weighted_multi_reference.py asserts).  Every comparison is for equality, byte for byte, on whole states and records, with
guard regions around both: every wave geometry of the plan, unaided (aid NULL), a factor of 0 and GPSX_WAID_L1CA, both variants;
the two identities with the single-stream calls on the device; a stream cut into launches; empty slots; bad channels; refusals;
and two receivers from IF samples through gpsx_wnav_words_dev and gpsx_wlock_dev on the one record array.  Every receiver's stream has
its own seed and satellites, and poison lies between a receiver's blocks and the next receiver's first."""
import ctypes as C

import numpy as np
import pytest

import weighted_aided_ref as A
import weighted_lock_cases as X
import weighted_lock_ref as R
import weighted_multi_cases as M
import weighted_nav_ref as N
import weighted_sync_cases as K
import weighted_sync_ref as Y

pytestmark = pytest.mark.gpu

EINVAL = -22
GUARD = 4096
L1CA = float(A.WAID_L1CA)


@pytest.fixture(scope="module")
def eng():
    from stm32f4_sdr_gps_amd import capi
    e = capi.Engine(0)
    yield e
    e.close()


def _cfg(c):
    from stm32f4_sdr_gps_amd import capi
    gains = {name: dict(dll=(c[name]["dll_c1"], c[name]["dll_c2"]), pll=(c[name]["pll_c1"], c[name]["pll_c2"]), fll=c[name]["fll_c"]) for name in ("search", "lock")}
    return capi.wsync_cfg(c["n_coh_search"], c["n_coh_lock"], gains["search"], gains["lock"], c["sync_bits"], (c["sync_num"], c["sync_den"]),
                          c["use_magnitude"], c["spacing"])


def _run(eng, call, st, n_ch, cfg, launches, dev, codes=None):
    """`call(d_if_or_host_pointer_offset, n_blocks, state pointer, record pointer)` launch after launch on a copy of `st` in device
    memory, guards around states and records (the records prefilled) -> ([(first block, records)], states after).  launches:
    [(first block, n_blocks, host array or device address of the launch's first byte)]; codes: a list that gets what every call and
    the synchronize behind it returned, instead of an assertion that both are 0"""
    h_st = np.full(GUARD + st.nbytes + GUARD, 0xA5, np.uint8)
    h_st[GUARD:GUARD + st.nbytes] = np.ascontiguousarray(st).view(np.uint8)
    d_st = eng.malloc(h_st.nbytes)
    recs = []
    try:
        eng.h2d(d_st, h_st)
        for at, k, where in launches:
            shape = (Y.slots(k, cfg), n_ch)
            size = shape[0] * n_ch * Y.REC_DTYPE.itemsize
            h_rec = np.full(GUARD + size + GUARD, 0x5A, np.uint8)
            if dev:
                d_rec = eng.malloc(h_rec.nbytes)
                try:
                    eng.h2d(d_rec, h_rec)
                    rc = call(C.c_void_p(where), k, C.c_void_p(d_st + GUARD), C.c_void_p(d_rec + GUARD))
                    sync = eng.lib.gpsx_synchronize(eng.h)
                    eng.d2h(h_rec, d_rec)
                finally:
                    eng.free(d_rec)
            else:
                rc, sync = call(where, k, C.c_void_p(d_st + GUARD), h_rec[GUARD:].ctypes.data), 0
            if codes is None:
                assert (rc, sync) == (0, 0), (rc, sync, eng.lib.gpsx_last_error(eng.h))
            else:
                codes.append((rc, sync))
            assert (h_rec[:GUARD] == 0x5A).all() and (h_rec[GUARD + size:] == 0x5A).all(), "guards around the records"
            recs.append((at, h_rec[GUARD:GUARD + size].view(Y.REC_DTYPE).reshape(shape).copy()))
        eng.d2h(h_st, d_st)
    finally:
        eng.free(d_st)
    assert (h_st[:GUARD] == 0xA5).all() and (h_st[GUARD + st.nbytes:] == 0xA5).all(), "guards around the states"
    return recs, h_st[GUARD:GUARD + st.nbytes].view(Y.STATE_DTYPE).copy()


def _multi(eng, streams, st, ch_per_rx, cfg, aid, dev, pieces=None, n_blocks=M.N_BLOCKS, codes=None):
    """gpsx_track_loop_weighted_sync_multi(_dev) on streams [n_rx][stride][4092] (receiver r's blocks are streams[r, :n_blocks]).
    aid: None (a NULL pointer) or the factor; pieces: launch lengths, each launch starting from the pointer advanced by its
    predecessors' blocks with the stride unchanged"""
    from stm32f4_sdr_gps_amd import capi
    streams = np.ascontiguousarray(streams, np.uint8)
    n_rx, stride = streams.shape[:2]
    rx, c = capi.wmulti(n_rx, ch_per_rx, stride), _cfg(cfg)
    a = None if aid is None else capi.waid(aid)
    fn = eng.lib.gpsx_track_loop_weighted_sync_multi_dev if dev else eng.lib.gpsx_track_loop_weighted_sync_multi
    d_if = eng.malloc(streams.nbytes) if dev else 0
    try:
        if dev:
            eng.h2d(d_if, streams)
        base = d_if if dev else streams.ctypes.data
        launches, at = [], 0
        for k in pieces or [n_blocks]:
            launches.append((at, k, base + at * 4092))
            at += k
        assert at == n_blocks <= stride

        def call(where, k, p_st, p_rec):
            rc = fn(eng.h, c.ctypes.data, None if a is None else a.ctypes.data, rx.ctypes.data, where, k, p_st, p_rec)
            if rc == 0 or codes is not None:
                assert eng.lib.gpsx_last_kernel(eng.h) == b"k_track_wsync_multi"
            return rc
        return _run(eng, call, st, n_rx * ch_per_rx, cfg, launches, dev, codes)
    finally:
        if dev:
            eng.free(d_if)


def _single(eng, blocks, st, cfg, aid):
    """gpsx_track_loop_weighted_sync_dev (aid None) or gpsx_track_loop_weighted_sync_aided_dev on one stream"""
    from stm32f4_sdr_gps_amd import capi
    blocks = np.ascontiguousarray(blocks, np.uint8)
    c = _cfg(cfg)
    a = None if aid is None else capi.waid(aid)
    d_if = eng.malloc(blocks.nbytes)
    try:
        eng.h2d(d_if, blocks)

        def call(where, k, p_st, p_rec):
            if a is None:
                return eng.lib.gpsx_track_loop_weighted_sync_dev(eng.h, c.ctypes.data, where, k, p_st, len(st), p_rec)
            return eng.lib.gpsx_track_loop_weighted_sync_aided_dev(eng.h, c.ctypes.data, a.ctypes.data, where, k, p_st, len(st), p_rec)
        recs, after = _run(eng, call, st, len(st), cfg, [(0, len(blocks), d_if)], True)
        return recs[0][1], after
    finally:
        eng.free(d_if)


def _same(rec, after, want_rec, want_st, what):
    assert rec.dtype == want_rec.dtype and rec.shape == want_rec.shape, what
    if rec.tobytes() != np.ascontiguousarray(want_rec).tobytes():
        bad = [c for c in range(rec.shape[1]) if rec[:, c].tobytes() != want_rec[:, c].tobytes()]
        slot = [u for u in range(rec.shape[0]) if rec[u, bad[0]].tobytes() != want_rec[u, bad[0]].tobytes()][0]
        assert not bad, (what, "records", bad[:4], slot, rec[slot, bad[0]], want_rec[slot, bad[0]])
    if after.tobytes() != want_st.tobytes():
        bad = [c for c in range(len(after)) if after[c:c + 1].tobytes() != want_st[c:c + 1].tobytes()]
        assert not bad, (what, "states", bad[:4], after[bad[0]], want_st[bad[0]])


SHAPE_IDS = [f"{s[0]}x{s[1]}" for s in M.SHAPES]


# ---- 1: records and whole states, every wave geometry, the three forms of aid, both variants ---------------------------------------
@pytest.mark.parametrize("aid", [None, 0.0, L1CA], ids=["null", "zero", "l1ca"])
@pytest.mark.parametrize("i", range(len(M.SHAPES)), ids=SHAPE_IDS)
def test_records_and_states_match_the_restatement(eng, i, aid):
    n_rx, ch, cpw, _ = M.SHAPES[i]
    assert M.plans([(n_rx, ch)]) == [(cpw, n_rx)]       # (the compiled plan header's shape is the table's row)
    blocks, st0, cfg = M.shape_inputs(i)
    want_rec, want_st, _ = M.shapes_on_restatement()[(i, aid or 0.0)]
    streams = M.streams_of(blocks, M.N_BLOCKS + M.EXTRA)
    for dev in (True, False):
        recs, after = _multi(eng, streams, st0, ch, cfg, aid, dev)
        _same(recs[0][1], after, want_rec, want_st, (n_rx, ch, aid, dev))
    assert want_st.tobytes() != st0.tobytes() and (want_rec["flags"] & Y.F_WINDOW).sum() > n_rx * ch


@pytest.mark.parametrize("i", range(len(M.SHAPES)), ids=SHAPE_IDS)
def test_null_and_a_zero_factor_give_identical_bytes(eng, i):
    blocks, st0, cfg = M.shape_inputs(i)
    streams = M.streams_of(blocks, M.N_BLOCKS + M.EXTRA)
    null, zero, l1ca = (_multi(eng, streams, st0, M.SHAPES[i][1], cfg, aid, True) for aid in (None, 0.0, L1CA))
    assert null[0][0][1].tobytes() == zero[0][0][1].tobytes() and null[1].tobytes() == zero[1].tobytes()
    assert l1ca[1].tobytes() != null[1].tobytes()


# ---- 2: the identities with the single-stream calls, on the device -------------------------------------------------------------------
@pytest.mark.parametrize("aid", [None, L1CA], ids=["unaided", "l1ca"])
@pytest.mark.parametrize("i", range(len(M.SHAPES)), ids=SHAPE_IDS)
def test_a_receivers_slice_is_the_single_stream_call_on_its_stream(eng, i, aid):
    n_rx, ch = M.SHAPES[i][:2]
    blocks, st0, cfg = M.shape_inputs(i)
    recs, after = _multi(eng, M.streams_of(blocks, M.N_BLOCKS + M.EXTRA), st0, ch, cfg, aid, True)
    for r in range(n_rx):
        one_rec, one_st = _single(eng, blocks[r], st0[r * ch:(r + 1) * ch], cfg, aid)
        _same(np.ascontiguousarray(recs[0][1][:, r * ch:(r + 1) * ch]), after[r * ch:(r + 1) * ch], one_rec, one_st, (n_rx, ch, aid, r))


@pytest.mark.parametrize("aid", [None, L1CA], ids=["unaided", "l1ca"])
@pytest.mark.parametrize("i", range(len(M.SHAPES)), ids=SHAPE_IDS)
def test_one_stream_for_every_receiver_is_one_single_stream_call(eng, i, aid):
    """every receiver gets a copy of the same stream, rx_stride_blocks = n_blocks: the bytes of one single-stream call with
    n_ch = n_rx * ch_per_rx"""
    n_rx, ch = M.SHAPES[i][:2]
    blocks, st0, cfg = M.shape_inputs(i)
    streams = M.streams_of([blocks[0]] * n_rx, M.N_BLOCKS)
    recs, after = _multi(eng, streams, st0, ch, cfg, aid, True)
    one_rec, one_st = _single(eng, blocks[0], st0, cfg, aid)
    _same(recs[0][1], after, one_rec, one_st, (n_rx, ch, aid))


# ---- 3: a stream cut into launches, both variants ------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [0, 2], ids=[SHAPE_IDS[0], SHAPE_IDS[2]])
def test_split_launches_are_one_launch(eng, i):
    """61 blocks as 61 and as 1 + 19 + 41, aiding on: states identical, records identical once keyed by the absolute end block; each
    later launch starts from the pointer advanced by its predecessors' blocks, the stride unchanged"""
    n_rx, ch = M.SHAPES[i][:2]
    blocks, st0, cfg = M.shape_inputs(i)
    want_rec, want_st, _ = M.shapes_on_restatement()[(i, L1CA)]
    streams = M.streams_of(blocks, M.N_BLOCKS + M.EXTRA)
    one = _multi(eng, streams, st0, ch, cfg, L1CA, True)
    _same(one[0][0][1], one[1], want_rec, want_st, "one launch")
    whole = K.rekey(one[0])
    for dev in (True, False):
        got = _multi(eng, streams, st0, ch, cfg, L1CA, dev, pieces=list(M.PIECES))
        assert got[1].tobytes() == one[1].tobytes() and K.rekey(got[0]) == whole, dev


# ---- 4: empty slots ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aid", [None, L1CA], ids=["unaided", "l1ca"])
def test_empty_slots_are_empty_and_no_error(eng, oracle, aid):
    """GPSX_PRN_NONE at the front, in the middle and at the end of a receiver: empty records, no error from either variant (the _dev
    call's synchronize included), and the neighbours' bytes are those of the case without the hole"""
    n_rx, ch = M.SHAPES[0][:2]
    blocks, _, cfg = M.shape_inputs(0)
    base_rec, base_st, _ = M.shapes_on_restatement()[(0, aid or 0.0)]
    st0, want_rec, want_st = M.patched(oracle, 0, aid or 0.0, M.HOLES)
    streams = M.streams_of(blocks, M.N_BLOCKS + M.EXTRA)
    empty = Y.empty_records(want_rec.shape[0], 1)[:, 0].tobytes()
    for dev in (True, False):
        recs, after = _multi(eng, streams, st0, ch, cfg, aid, dev)       # (asserts that every return code is 0)
        _same(recs[0][1], after, want_rec, want_st, ("holes", aid, dev))
        for c in range(n_rx * ch):
            if c in M.HOLES:
                assert recs[0][1][:, c].tobytes() == empty
            else:
                assert recs[0][1][:, c].tobytes() == base_rec[:, c].tobytes() and after[c:c + 1].tobytes() == base_st[c:c + 1].tobytes(), c


# ---- 5: bad channels --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", sorted(M.BAD))
def test_a_bad_channel_in_one_receiver_changes_nothing_elsewhere(eng, oracle, what):
    """a PRN of 0, a mode of 3, a NaN phase in receiver 1 of 3: GPSX_EINVAL from the host variant itself and from the next
    gpsx_synchronize after _dev; receivers 0 and 2, and receiver 1's other channels, are the restatement's byte for byte"""
    n_rx, ch = M.SHAPES[0][:2]
    blocks, _, cfg = M.shape_inputs(0)
    st0, want_rec, want_st = M.patched(oracle, 0, L1CA, {M.BAD_CHANNEL: M.BAD[what]})
    assert M.BAD_CHANNEL // ch == 1 and n_rx == 3
    streams = M.streams_of(blocks, M.N_BLOCKS + M.EXTRA)
    for dev in (True, False):
        codes = []
        recs, after = _multi(eng, streams, st0, ch, cfg, L1CA, dev, codes=codes)
        assert codes == [(0, EINVAL) if dev else (EINVAL, 0)], (what, dev, codes)
        if not dev:
            assert b"prn" in eng.lib.gpsx_last_error(eng.h)
        assert eng.lib.gpsx_synchronize(eng.h) == 0
        _same(recs[0][1], after, want_rec, want_st, (what, dev))


# ---- 6: refusals ------------------------------------------------------------------------------------------------------------------------
def test_argument_checks_write_nothing(eng):
    from stm32f4_sdr_gps_amd import capi
    n_rx, ch, n = 2, 3, 8
    streams = M.streams_of([M.rx_blocks(r, n) for r in range(n_rx)], n + M.EXTRA)
    st0 = np.concatenate([M.rx_states(r, ch) for r in range(n_rx)])
    nan = float("nan")
    good = dict(null=None, spacing=8, n_blocks=n, rx=(n_rx, ch, n + M.EXTRA, 0), aid=(L1CA, 0), gain=1.0, sync_bits=20)
    by_message = {
        b"null argument": [dict(null="cfg"), dict(null="rx"), dict(null="blocks"), dict(null="state"), dict(null="rec"), dict(null="rx", n_blocks=0)],
        b"spacing must be 1..15 samples": [dict(spacing=0), dict(spacing=16, rx=(0, 0, 0, 1))],                  # (the single-stream call's order)
        b"sync_bits must be 1..200": [dict(sync_bits=201, rx=(n_rx, 65, n, 0))],
        b"n_blocks must be 1..4096": [dict(n_blocks=0), dict(n_blocks=4097, rx=(n_rx, ch, 5000, 0)), dict(n_blocks=0, rx=(0, ch, 0, 0))],
        b"n_rx must be 1..1048576": [dict(rx=(0, ch, n, 0)), dict(rx=(-1, ch, n, 0)), dict(rx=((1 << 20) + 1, ch, n, 0)), dict(rx=(0, 65, n - 1, 1))],
        b"ch_per_rx must be 1..64": [dict(rx=(n_rx, 65, n, 0)), dict(rx=(n_rx, 0, n, 0)), dict(rx=(n_rx, -4, n - 1, 0))],
        b"rx_stride_blocks must not be below n_blocks": [dict(rx=(n_rx, ch, n - 1, 0)), dict(rx=(n_rx, ch, 0, 0)), dict(rx=(n_rx, ch, -7, 3))],
        b"reserved must be 0": [dict(rx=(n_rx, ch, n, 1)), dict(rx=(n_rx, ch, n, -1), gain=nan), dict(aid=(L1CA, 1))],
        b"a loop gain is not finite": [dict(gain=nan), dict(gain=float("inf"), aid=(nan, 0))],
        b"code_per_hz must be finite and -1..1": [dict(aid=(nan, 0)), dict(aid=(1.5, 1))],
    }
    n_slots = Y.slots(n, Y.make_cfg(4, 20, K.S.PULL_IN, K.S.STEADY, 20, (5, 4)))
    n_rec = n_slots * n_rx * ch * 48
    d_st, d_if, d_rec = eng.malloc(st0.nbytes), eng.malloc(streams.nbytes), eng.malloc(n_rec)
    try:
        eng.h2d(d_if, streams)
        for dev in (False, True):
            fn = eng.lib.gpsx_track_loop_weighted_sync_multi_dev if dev else eng.lib.gpsx_track_loop_weighted_sync_multi
            for message, changes in by_message.items():
                for change in changes:
                    a = {**good, **change}
                    cfg = _cfg(Y.make_cfg(4, 20, K.S.PULL_IN, K.S.STEADY, 20, (5, 4)))
                    cfg["spacing"], cfg["sync_bits"] = a["spacing"], a["sync_bits"]
                    cfg["lock"]["pll_c2"] = cfg["lock"]["pll_c2"] * np.float32(a["gain"])
                    aid = capi.waid(a["aid"][0])
                    aid["reserved"] = a["aid"][1]
                    rx = capi.wmulti(*a["rx"][:3])
                    rx["reserved"] = a["rx"][3]
                    rec = np.full(n_rec, 0xA5, np.uint8)
                    eng.h2d(d_st, st0)
                    eng.h2d(d_rec, rec)
                    null = a["null"]
                    rc = fn(eng.h, None if null == "cfg" else cfg.ctypes.data, aid.ctypes.data, None if null == "rx" else rx.ctypes.data,
                            None if null == "blocks" else (C.c_void_p(d_if) if dev else streams.ctypes.data), a["n_blocks"],
                            None if null == "state" else C.c_void_p(d_st), None if null == "rec" else (C.c_void_p(d_rec) if dev else rec.ctypes.data))
                    assert rc == EINVAL and eng.lib.gpsx_last_error(eng.h) == message, (dev, change, eng.lib.gpsx_last_error(eng.h))
                    eng.synchronize()   # nothing was enqueued, nothing is pending
                    st, dr = st0.copy(), np.zeros_like(rec)
                    eng.d2h(st, d_st)
                    eng.d2h(dr, d_rec)
                    assert (rec == 0xA5).all() and (dr == 0xA5).all() and st.tobytes() == st0.tobytes(), (dev, change)
            # the limits themselves are accepted: a stride of exactly n_blocks, aid NULL (64 slots: the shapes above)
            cfg = _cfg(Y.make_cfg(4, 20, K.S.PULL_IN, K.S.STEADY, 20, (5, 4)))
            rx = capi.wmulti(n_rx, ch, n)
            packed = np.ascontiguousarray(streams[:, :n])
            eng.h2d(d_if, packed)
            eng.h2d(d_st, st0)
            rec = np.zeros(n_rec, np.uint8)
            eng._chk(fn(eng.h, cfg.ctypes.data, None, rx.ctypes.data, C.c_void_p(d_if) if dev else packed.ctypes.data, n, C.c_void_p(d_st),
                        C.c_void_p(d_rec) if dev else rec.ctypes.data), "gpsx_track_loop_weighted_sync_multi")
            eng.synchronize()
            eng.h2d(d_if, streams)
    finally:
        for p in (d_st, d_if, d_rec):
            eng.free(p)


def test_the_engine_convenience(eng):
    n_rx, ch = M.SHAPES[0][:2]
    blocks, st0, cfg = M.shape_inputs(0)
    want_rec, want_st, _ = M.shapes_on_restatement()[(0, L1CA)]
    d_st = eng.malloc(st0.nbytes)
    try:
        eng.h2d(d_st, st0)
        rec = eng.track_loop_weighted_sync_multi(np.stack(blocks), d_st, ch, _cfg(cfg), L1CA)
        after = st0.copy()
        eng.d2h(after, d_st)
    finally:
        eng.free(d_st)
    _same(rec, after, want_rec, want_st, "Engine.track_loop_weighted_sync_multi")


# ---- 7: the chain: two receivers' IF samples to words and lock flags through one record array -----------------------------------------
def test_two_receivers_from_if_samples_to_words_and_lock_flags(eng):
    """weighted_multi_cases' chain -- two receivers, three satellites each at amplitude 0.035, five slots of which one holds a PRN
    that is present only on the other receiver's stream and one GPSX_PRN_NONE -- 2000 blocks in launches of 500 through
    gpsx_track_loop_weighted_sync_multi_dev, gpsx_wnav_words_dev and gpsx_wlock_dev with n_ch = 10.  The sync records and states are
    the restatement's; the readers' outputs equal their restatements on the device's records; every present satellite is LOCKED and
    its bits after lock are the synthesised ones; the cross-stream PRN never gets GPSX_WLOCK_CODE"""
    from stm32f4_sdr_gps_amd import capi
    n_ch = 2 * M.CHAIN_CH
    want_recs, want_sync, want_locks, _ = M.chain_on_restatement()
    both = [M.chain_blocks(r) for r in range(2)]
    stride = M.CHAIN_MS + M.EXTRA
    streams = M.streams_of([b for b, _ in both], stride)
    sync_cfg, rx = _cfg(K.sync_cfg()), capi.wmulti(2, M.CHAIN_CH, stride)
    nav_cfg = np.zeros(1, capi.WNAV_CFG_DTYPE)
    nav_cfg["max_bad_words"] = 3
    cfg = X.scenario_cfg(0)
    lock_cfg = R.cfg_array(cfg)
    sync_st = M.chain_states()
    nav, lock_st = np.zeros(n_ch, N.STATE_DTYPE), np.zeros(n_ch, R.STATE_DTYPE)
    want_nav, want_lock_st = nav.copy(), lock_st.copy()
    max_slots = capi.wsync_slots(M.CHAIN_LAUNCH, K.N_COH_SEARCH, K.N_COH_LOCK)
    sizes = (streams.nbytes, sync_st.nbytes, nav.nbytes, lock_st.nbytes, max_slots * n_ch * 48, N.max_words(M.CHAIN_LAUNCH) * n_ch * 16, n_ch * 64)
    ptrs = [eng.malloc(s) for s in sizes]
    d_if, d_sync, d_nav, d_lock_st, d_rec, d_words, d_lock = ptrs
    recs, flags = [], []
    try:
        for d, a in ((d_if, streams), (d_sync, sync_st), (d_nav, nav), (d_lock_st, lock_st)):
            eng.h2d(d, a)
        at = 0
        for i, n in enumerate(M.chain_launches()):
            n_slots = capi.wsync_slots(n, K.N_COH_SEARCH, K.N_COH_LOCK)
            eng._chk(eng.lib.gpsx_track_loop_weighted_sync_multi_dev(eng.h, sync_cfg.ctypes.data, None, rx.ctypes.data, C.c_void_p(d_if + at * 4092), n,
                                                                     C.c_void_p(d_sync), C.c_void_p(d_rec)), "gpsx_track_loop_weighted_sync_multi_dev")
            eng._chk(eng.lib.gpsx_wnav_words_dev(eng.h, nav_cfg.ctypes.data, C.c_void_p(d_rec), n_slots, n, C.c_void_p(d_nav), n_ch, C.c_void_p(d_words)),
                     "gpsx_wnav_words_dev")
            eng._chk(eng.lib.gpsx_wlock_dev(eng.h, lock_cfg.ctypes.data, C.c_void_p(d_rec), n_slots, n, C.c_void_p(d_lock_st), None, n_ch, C.c_void_p(d_lock)),
                     "gpsx_wlock_dev")
            eng.synchronize()       # (0: the empty slots are not bad channels)
            rec, words, lock = np.zeros((n_slots, n_ch), Y.REC_DTYPE), np.zeros((N.max_words(n), n_ch), N.WORD_DTYPE), np.zeros(n_ch, R.LOCK_DTYPE)
            for a, d in ((rec, d_rec), (words, d_words), (lock, d_lock), (nav, d_nav), (lock_st, d_lock_st), (sync_st, d_sync)):
                eng.d2h(a, d)
            assert rec.tobytes() == np.ascontiguousarray(want_recs[i]).tobytes(), ("sync records of the launch at", at)
            w_words, bad = N.run(rec, n, want_nav, 3)
            assert not bad and words.tobytes() == w_words.tobytes() and nav.tobytes() == want_nav.tobytes(), ("words of the launch at", at)
            w_lock, bad = R.run(rec, n, want_lock_st, cfg, None)
            assert not bad and lock.tobytes() == w_lock.tobytes() == want_locks[i].tobytes() and lock_st.tobytes() == want_lock_st.tobytes(), at
            recs.append((at, rec))
            flags.append(lock["flags"].copy())
            at += n
    finally:
        for p in ptrs:
            eng.free(p)
    assert sync_st.tobytes() == want_sync.tobytes()
    flags = np.array(flags)
    code_car = R.F_CODE | R.F_CARRIER
    for ch in M.chain_slots("sat"):
        r, j = divmod(ch, M.CHAIN_CH)
        sat = M.CHAIN_SLOTS[r][j][1]
        assert int(sync_st["mode"][ch]) == Y.LOCKED and (flags[-1, ch] & code_car) == code_car, (ch, flags[:, ch])
        errors, n_bits = K.bit_errors(Y.bits_after_lock([(a, rec[:, ch]) for a, rec in recs]), both[r][1][sat], int(sync_st["edge"][ch]))
        assert errors == 0 and n_bits >= 40, (ch, errors, n_bits)
    for ch in M.chain_slots("cross"):
        assert not (flags[:, ch] & R.F_CODE).any(), (ch, flags[:, ch])
    for ch in M.chain_slots("none"):
        assert not flags[:, ch].any() and all((rec[:, ch]["flags"] == 0).all() for _, rec in recs)
