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
import weighted_gpu as G
import weighted_lock_cases as X
import weighted_lock_ref as R
import weighted_multi_cases as M
import weighted_nav_ref as N
import weighted_sync_cases as K
import weighted_sync_ref as Y
from weighted_gpu import EINVAL, eng  # noqa: F401
from weighted_gpu import sync_cfg as _cfg

pytestmark = pytest.mark.gpu

L1CA = float(A.WAID_L1CA)


def _multi(eng, streams, st, ch_per_rx, cfg, aid, dev, pieces=None, n_blocks=M.N_BLOCKS, codes=None):
    """gpsx_track_loop_weighted_sync_multi(_dev) on streams [n_rx][stride][4092] (receiver r's blocks are streams[r, :n_blocks]), launch
    after launch on a copy of `st` in device memory -> ([(first block, records)], states after).  aid: None (a NULL pointer) or the
    factor; pieces: launch lengths, each launch starting from the pointer advanced by its predecessors' blocks with the stride
    unchanged; codes: a list that gets every launch's return code (the synchronize's behind the _dev call), instead of an assertion
    that all are 0"""
    from stm32f4_sdr_gps_amd import capi
    streams = np.ascontiguousarray(streams, np.uint8)
    n_rx, stride = streams.shape[:2]
    n_ch, rx, c = n_rx * ch_per_rx, capi.wmulti(n_rx, ch_per_rx, stride), _cfg(cfg)
    a = None if aid is None else capi.waid(aid)
    fn = eng.lib.gpsx_track_loop_weighted_sync_multi_dev if dev else eng.lib.gpsx_track_loop_weighted_sync_multi
    cuts = pieces or [n_blocks]
    firsts = [sum(cuts[:i]) for i in range(len(cuts))]
    assert sum(cuts) == n_blocks <= stride
    with G.Guarded(eng if dev else None, streams.nbytes, G.STATE_FILL, streams) as d_if:

        def call(ins, sts, out, i):
            return fn(eng.h, c.ctypes.data, None if a is None else a.ctypes.data, rx.ctypes.data, C.c_void_p(ins[0]), cuts[i], sts[0], out)
        recs, after, got = G.run_stage(eng, call, b"k_track_wsync_multi", st,
                                       [([d_if.ptr.value + at * 4092], Y.REC_DTYPE, (Y.slots(k, cfg), n_ch)) for at, k in zip(firsts, cuts)], dev)
    if codes is None:
        assert not any(got), (got, eng.lib.gpsx_last_error(eng.h))
    else:
        codes.extend(got)
    return list(zip(firsts, recs)), after


def _single(eng, blocks, st, cfg, aid):
    """gpsx_track_loop_weighted_sync_dev (aid None) or gpsx_track_loop_weighted_sync_aided_dev on one stream"""
    from stm32f4_sdr_gps_amd import capi
    blocks = np.ascontiguousarray(blocks, np.uint8)
    c, a = _cfg(cfg), None if aid is None else capi.waid(aid)

    def call(ins, sts, out, k):
        if a is None:
            return eng.lib.gpsx_track_loop_weighted_sync_dev(eng.h, c.ctypes.data, ins[0], len(blocks), sts[0], len(st), out)
        return eng.lib.gpsx_track_loop_weighted_sync_aided_dev(eng.h, c.ctypes.data, a.ctypes.data, ins[0], len(blocks), sts[0], len(st), out)
    recs, after, codes = G.run_stage(eng, call, b"k_track_waid_sync" if a is not None else b"k_track_wsync", st,
                                     [([blocks], Y.REC_DTYPE, (Y.slots(len(blocks), cfg), len(st)))])
    assert codes == [0]
    return recs[0], after


def _same(rec, after, want_rec, want_st, what):
    G.same_columns(rec, want_rec, (what, "records"))
    G.same_rows(after, want_st, (what, "states"))


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
        assert codes == [EINVAL], (what, dev, codes)      # (the _dev call itself returned 0: the driver asserts it)
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
    n_rec = Y.slots(n, Y.make_cfg(4, 20, K.S.PULL_IN, K.S.STEADY, 20, (5, 4))) * n_rx * ch * Y.REC_DTYPE.itemsize
    with G.Pool() as pool:
        d_st, d_if = pool.add(G.Guarded(eng, st0.nbytes, G.STATE_FILL, st0)), pool.add(G.Guarded(eng, streams.nbytes, G.STATE_FILL, streams))
        outs = {True: pool.add(G.Guarded(eng, n_rec)), False: pool.add(G.Guarded(None, n_rec))}
        fns = {True: eng.lib.gpsx_track_loop_weighted_sync_multi_dev, False: eng.lib.gpsx_track_loop_weighted_sync_multi}

        def call(a, dev):
            cfg = _cfg(Y.make_cfg(4, 20, K.S.PULL_IN, K.S.STEADY, 20, (5, 4)))
            cfg["spacing"], cfg["sync_bits"] = a["spacing"], a["sync_bits"]
            cfg["lock"]["pll_c2"] = cfg["lock"]["pll_c2"] * np.float32(a["gain"])
            aid = capi.waid(a["aid"][0])
            aid["reserved"] = a["aid"][1]
            rx = capi.wmulti(*a["rx"][:3])
            rx["reserved"] = a["rx"][3]
            null = a["null"]
            return fns[dev](eng.h, None if null == "cfg" else cfg.ctypes.data, aid.ctypes.data, None if null == "rx" else rx.ctypes.data,
                            None if null == "blocks" else (d_if.ptr if dev else streams.ctypes.data), a["n_blocks"],
                            None if null == "state" else d_st.ptr, None if null == "rec" else outs[dev].ptr)
        G.refusals(eng, by_message, good, call, [d_st, *outs.values()])
        # the limits themselves are accepted: a stride of exactly n_blocks, aid NULL (64 slots: the shapes above)
        cfg, rx = _cfg(Y.make_cfg(4, 20, K.S.PULL_IN, K.S.STEADY, 20, (5, 4))), capi.wmulti(n_rx, ch, n)
        packed = np.ascontiguousarray(streams[:, :n])
        d_if.put(packed)
        for dev in (False, True):
            d_st.refill()
            eng._chk(fns[dev](eng.h, cfg.ctypes.data, None, rx.ctypes.data, d_if.ptr if dev else packed.ctypes.data, n, d_st.ptr, outs[dev].ptr),
                     "gpsx_track_loop_weighted_sync_multi")
            eng.synchronize()


def test_the_engine_convenience(eng):
    n_rx, ch = M.SHAPES[0][:2]
    blocks, st0, cfg = M.shape_inputs(0)
    want_rec, want_st, _ = M.shapes_on_restatement()[(0, L1CA)]
    with G.Guarded(eng, st0.nbytes, G.STATE_FILL, st0) as d_st:
        rec = eng.track_loop_weighted_sync_multi(np.stack(blocks), d_st.ptr.value, ch, _cfg(cfg), L1CA)
        after = d_st.get(st0.dtype, st0.shape)
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
    cfg = X.scenario_cfg(0)
    states = dict(sync=M.chain_states(), nav=np.zeros(n_ch, N.STATE_DTYPE), lock=np.zeros(n_ch, R.STATE_DTYPE))
    want_nav, want_lock_st = states["nav"].copy(), states["lock"].copy()
    recs, flags = [], []
    with G.Guarded(eng, streams.nbytes, G.STATE_FILL, streams) as d_if, \
            G.Chain(eng, _cfg(K.sync_cfg()), states, M.CHAIN_LAUNCH, lock_cfg=R.cfg_array(cfg), rx=capi.wmulti(2, M.CHAIN_CH, stride)) as chain:
        at = 0
        for i, n in enumerate(M.chain_launches()):
            chain.sync(d_if.ptr.value + at * 4092, n)
            chain.words()
            chain.lock()
            eng.synchronize()       # (0: the empty slots are not bad channels)
            rec, words, lock, nav, lock_st, sync_st = (chain.read(name) for name in ("rec", "words", "l", "nav", "lock", "sync"))
            assert rec.tobytes() == np.ascontiguousarray(want_recs[i]).tobytes(), ("sync records of the launch at", at)
            w_words, bad = N.run(rec, n, want_nav, 3)
            assert not bad and words.tobytes() == w_words.tobytes() and nav.tobytes() == want_nav.tobytes(), ("words of the launch at", at)
            w_lock, bad = R.run(rec, n, want_lock_st, cfg, None)
            assert not bad and lock.tobytes() == w_lock.tobytes() == want_locks[i].tobytes() and lock_st.tobytes() == want_lock_st.tobytes(), at
            recs.append((at, rec))
            flags.append(lock["flags"].copy())
            at += n
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
