"""The weighted path's observables on the device (EXTENSION, not in the reference: include/gpsx.h gpsx_wobs; k_wobs on the vector ALU,
one channel per lane) against its exact CPU restatement (tests/weighted_obs_ref.py, pinned in tests/test_weighted_obs_reference.py).
Every comparison is for equality, byte for byte, on the 32-byte observables and on the 80-byte states.  The sync loop's records and
the word layer's words are fabricated (tests/weighted_obs_cases.py: 32 distinct streams tiled over the channels -- code phases that
drift and dither through the seam, sit on either side of mid-block or are no phases at all, SEARCH windows, a gap, another edge, a
week that ends, a HOW that contradicts; initial states from the restatements' run over the stream's earlier blocks); only the last
test starts from IF samples."""
import ctypes as C

import numpy as np
import pytest

import weighted_loop_cases as S
import weighted_nav_ref as N
import weighted_obs_cases as X
import weighted_obs_ref as O
import weighted_sync_cases as K
import weighted_sync_ref as Y

pytestmark = pytest.mark.gpu

EINVAL = -22
GUARD = 4096


@pytest.fixture(scope="module")
def eng():
    from stm32f4_sdr_gps_amd import capi
    e = capi.Engine(0)
    yield e
    e.close()


def _cfg(edge_guard, reserved=0):
    cfg = np.zeros(1, O.CFG_DTYPE)
    cfg["edge_guard"], cfg["reserved"] = edge_guard, reserved
    return cfg


def _gpu(eng, launches, st, edge_guard=X.EDGE_GUARD, dev=True):
    """the library on a copy of `st` in device memory, launch after launch.  launches: [(records [n_slots][n_ch], words
    [n_blocks // 600 + 2][n_ch], n_blocks)].  States and observables sit between canaries, the observables are prefilled with 0xA5.
    -> ([observables per launch], states after, [return codes])"""
    n_ch = len(st)
    cfg = _cfg(edge_guard)
    h_st = np.full(GUARD + st.nbytes + GUARD, 0x5A, np.uint8)
    h_st[GUARD:GUARD + st.nbytes] = np.ascontiguousarray(st).view(np.uint8)
    d_st = eng.malloc(h_st.nbytes)
    obs_out, codes = [], []
    try:
        eng.h2d(d_st, h_st)
        for rec, words, n_blocks in launches:
            rec, words = np.ascontiguousarray(rec), np.ascontiguousarray(words)
            assert rec.dtype == Y.REC_DTYPE and words.dtype == N.WORD_DTYPE and rec.shape[1] == n_ch and words.shape == (N.max_words(n_blocks), n_ch)
            size = n_ch * 32
            h_obs = np.full(GUARD + size + GUARD, 0xA5, np.uint8)
            d_rec, d_words, d_obs = eng.malloc(rec.nbytes), eng.malloc(words.nbytes), eng.malloc(h_obs.nbytes)
            try:
                eng.h2d(d_rec, rec)
                eng.h2d(d_words, words)
                if dev:
                    eng.h2d(d_obs, h_obs)
                    rc = eng.lib.gpsx_wobs_dev(eng.h, cfg.ctypes.data, C.c_void_p(d_rec), rec.shape[0], n_blocks, C.c_void_p(d_words),
                                               C.c_void_p(d_st + GUARD), n_ch, C.c_void_p(d_obs + GUARD))
                    assert rc == 0 and eng.lib.gpsx_last_kernel(eng.h) == b"k_wobs"
                    codes.append(eng.lib.gpsx_synchronize(eng.h))
                    eng.d2h(h_obs, d_obs)
                else:
                    codes.append(eng.lib.gpsx_wobs(eng.h, cfg.ctypes.data, C.c_void_p(d_rec), rec.shape[0], n_blocks, C.c_void_p(d_words),
                                                   C.c_void_p(d_st + GUARD), n_ch, h_obs[GUARD:].ctypes.data))
            finally:
                for p in (d_rec, d_words, d_obs):
                    eng.free(p)
            assert (h_obs[:GUARD] == 0xA5).all() and (h_obs[GUARD + size:] == 0xA5).all(), "canary around the observables"
            obs_out.append(h_obs[GUARD:GUARD + size].view(O.OBS_DTYPE).copy())
        eng.d2h(h_st, d_st)
    finally:
        eng.free(d_st)
    assert (h_st[:GUARD] == 0x5A).all() and (h_st[GUARD + st.nbytes:] == 0x5A).all(), "canary around the states"
    return obs_out, h_st[GUARD:GUARD + st.nbytes].view(O.STATE_DTYPE).copy(), codes


def _same(obs, after, want_obs, want_st, what):
    assert obs.shape == want_obs.shape and after.shape == want_st.shape, what
    bad = [c for c in range(len(obs)) if obs[c:c + 1].tobytes() != want_obs[c:c + 1].tobytes()]
    assert not bad, (what, "observables", bad[:4], obs[bad[0]], want_obs[bad[0]])
    bad = [c for c in range(len(after)) if after[c:c + 1].tobytes() != want_st[c:c + 1].tobytes()]
    assert not bad, (what, "states", bad[:4], after[bad[0]], want_st[bad[0]])


@pytest.mark.parametrize("i", range(len(X.CASES)))
def test_observables_and_states_match_the_restatement(eng, i):
    """the table: 1, 3, 64, 65, 257 and 1000 channels (one lane, part of a wave, the wave's edge, part of the last workgroup), spans
    20 / 1 / 4 / 5 (slot counts on either side of the two register sets' sixteen), launches of 4096, 1237, 600, 2047, 1 and 19
    blocks, fresh states and states in the middle of anything.  The observables were prefilled: equality says every byte was written"""
    rec, words, n_blocks, st0, want, want_st = X.case(i)
    for dev in (True, False):
        obs, after, codes = _gpu(eng, [(rec, words, n_blocks)], st0, dev=dev)
        assert codes == [0]
        _same(obs[0], after, want, want_st, (X.CASES[i], dev))


SPLIT = dict(n_ch=64, span=20, n_blocks=4096, warm=500)
_split = {}


def _split_states():
    if not _split:
        _split["st"] = X.warm_states(SPLIT["warm"])
    nav, st = _split["st"]
    return nav.copy(), st.copy()


def _split_launches(parts):
    """the launches (warm + a, n) on the restatements -> ([(records, words, n)] tiled over the channels, last observables, states)"""
    nav, st = _split_states()
    idx = X.tiled(SPLIT["n_ch"])
    out = []
    for at, n in parts:
        rec, words, obs = X.launch(nav, st, at, n, SPLIT["span"], filler=False)
        out.append((np.ascontiguousarray(rec[:, idx]), np.ascontiguousarray(words[:, idx]), n))
    return out, obs[idx].copy(), st[idx].copy()


@pytest.mark.parametrize("cut", [1, 599, 600, 2050, 4095])
def test_split_launches_equal_one_launch(eng, cut):
    """one 4096-block launch cut in two, both ways on the device: each equals the restatement of the same launches byte for byte, and
    the two agree with each other as the restatements do (tests/test_weighted_obs_reference.py: all but n_anchor, and tx_ms_at_edge
    without TOW, on channels whose chain broke)"""
    warm, n_blocks = SPLIT["warm"], SPLIT["n_blocks"]
    st0 = _split_states()[1][X.tiled(SPLIT["n_ch"])].copy()
    whole, want_obs, want_st = _split_launches([(warm, n_blocks)])
    obs1, after1, codes = _gpu(eng, whole, st0)
    assert codes == [0]
    _same(obs1[0], after1, want_obs, want_st, "one launch")
    parts, part_obs, part_st = _split_launches([(warm, cut), (warm + cut, n_blocks - cut)])
    obs2, after2, codes = _gpu(eng, parts, st0)
    assert codes == [0, 0]
    _same(obs2[1], after2, part_obs, part_st, ("two launches", cut))
    assert obs2[1].tobytes() == obs1[0].tobytes() and (obs1[0]["flags"] & O.F_VALID).sum() >= 20
    broke = after1["n_break"] != st0["n_break"]
    assert broke.any() and not broke.all()
    for st in (after1, after2):
        st["n_anchor"][broke] = 0
        st["tx_ms_at_edge"][broke & (st["flags"] & O.F_TOW == 0)] = 0
    assert after1.tobytes() == after2.tobytes()


def test_every_byte_of_the_observables_is_written(eng):
    """257 channels, a fresh state among them and a bad one: no byte of the 0xA5 prefill is left in either variant"""
    rec, words, n_blocks, st0, _, _ = X.case(4)
    st0 = st0.copy()
    st0[5] = np.zeros(1, O.STATE_DTYPE)[0]
    st0["reserved"][70] = 9
    want_st = st0.copy()
    want, bad = O.run(rec, n_blocks, words, want_st, X.EDGE_GUARD)
    assert bad == [70] and not want["reserved"].any()
    for dev in (True, False):
        obs, after, codes = _gpu(eng, [(rec, words, n_blocks)], st0, dev=dev)
        assert codes == [EINVAL]
        _same(obs[0], after, want, want_st, ("every byte", dev))
    assert eng.lib.gpsx_synchronize(eng.h) == 0


BAD_FIELDS = [("flags", 32), ("flags", 1 << 31), ("reserved", 1), ("blocks_seen", -1), ("blocks_seen", (1 << 62) + 1), ("last_bit_end_p1", -1),
              ("last_bit_end_p1", (1 << 62) + 1), ("chain_first_p1", -3), ("chain_first_p1", (1 << 62) + 1), ("last_win_end_p1", -1),
              ("last_win_end_p1", (1 << 62) + 1), ("edge_block", (1 << 62) + 1), ("edge_block", -(1 << 62) - 1), ("tx_ms_at_edge", -1),
              ("tx_ms_at_edge", 604800000), ("last_phase", np.nan), ("last_phase", -1.0), ("last_phase", 16368.0)]
GOOD_EDGES = [("blocks_seen", 1 << 62), ("edge_block", 1 << 62), ("edge_block", -(1 << 62)), ("tx_ms_at_edge", 604799999), ("last_phase", 16367.998),
              ("last_bit_end_p1", 1 << 62), ("chain_first_p1", 1 << 62), ("last_win_end_p1", 1 << 62), ("last_win_end_p1", 1 << 40)]


def test_bad_channels(eng):
    """one bad state per field among good neighbours of the same wave: untouched, their observables zero with age -1, GPSX_EINVAL
    from the host variant and from the next synchronize after the device variant; the neighbours are the restatement's -- among
    them states at the very ends of the ranges, where no sum may overflow"""
    rec, words, n_blocks, st0, _, _ = X.case(2)
    st0 = st0.copy()
    bad = [1 + 3 * k for k in range(len(BAD_FIELDS))]
    for ch, (field, value) in zip(bad, BAD_FIELDS):
        assert int(st0["flags"][ch]) & O.F_PHASE
        st0[field][ch] = value
    edges = [2 + 3 * k for k in range(len(GOOD_EDGES))]
    for ch, (field, value) in zip(edges, GOOD_EDGES):
        st0[field][ch] = value
    st0["flags"][63], st0["last_phase"][63] = 0, np.nan      # (without PHASE a NaN there is nobody's business)
    want_st = st0.copy()
    want, found = O.run(rec, n_blocks, words, want_st, X.EDGE_GUARD)
    assert found == bad and want_st[bad].tobytes() == st0[bad].tobytes() and (want["age_blocks"][bad] == -1).all() and not want["flags"][bad].any()
    for dev in (True, False):
        obs, after, codes = _gpu(eng, [(rec, words, n_blocks)], st0, dev=dev)
        assert codes == [EINVAL] and eng.lib.gpsx_last_error(eng.h), dev
        assert eng.lib.gpsx_synchronize(eng.h) == 0
        _same(obs[0], after, want, want_st, ("bad channels", dev))
    good = [c for c in range(len(st0)) if c not in bad]
    obs, after, codes = _gpu(eng, [(np.ascontiguousarray(rec[:, good]), np.ascontiguousarray(words[:, good]), n_blocks)], st0[good].copy())
    assert codes == [0]
    _same(obs[0], after, want[good], want_st[good], "the same channels without the bad ones")


def test_argument_checks_write_nothing(eng):
    n_ch, n_blocks, n_slots = 5, 40, 2
    nav, st0 = X.warm_states(0)
    rec, words, _ = X.launch(nav, st0.copy(), 0, n_blocks, 20)
    rec, words, st0 = np.ascontiguousarray(rec[:, :n_ch]), np.ascontiguousarray(words[:, :n_ch]), st0[:n_ch].copy()
    good = dict(null_cfg=False, null_rec=False, null_words=False, null_st=False, null_out=False, guard=512.0, reserved=0, n_slots=n_slots,
                n_blocks=n_blocks, n_ch=n_ch)
    # every refusal with its exact text; the last row of a group fails a later clause as well: the first failing clause decides
    by_message = {
        b"null argument": [dict(null_cfg=True), dict(null_rec=True), dict(null_words=True), dict(null_st=True), dict(null_out=True),
                           dict(null_words=True, n_ch=0)],
        b"edge_guard must be finite and 0..8184": [dict(guard=-0.001), dict(guard=8184.001), dict(guard=np.nan), dict(guard=np.inf), dict(guard=-np.inf),
                                                   dict(guard=np.nan, reserved=1), dict(guard=-1.0, n_blocks=0)],
        b"reserved must be 0": [dict(reserved=1), dict(reserved=-1), dict(reserved=1, n_blocks=4097)],
        b"n_blocks must be 1..4096": [dict(n_blocks=0), dict(n_blocks=-40), dict(n_blocks=4097), dict(n_blocks=0, n_slots=0)],
        b"n_slots must be 1..n_blocks": [dict(n_slots=0), dict(n_slots=-1), dict(n_slots=41), dict(n_blocks=1, n_slots=2), dict(n_slots=0, n_ch=0)],
        b"n_ch must be at least 1": [dict(n_ch=0), dict(n_ch=-3)],
    }
    refusals = [(message, change) for message, changes in by_message.items() for change in changes]
    d_rec, d_words, d_st, d_obs = eng.malloc(rec.nbytes), eng.malloc(words.nbytes), eng.malloc(st0.nbytes), eng.malloc(n_ch * 32)
    try:
        eng.h2d(d_rec, rec)
        eng.h2d(d_words, words)
        for dev, fn in ((False, eng.lib.gpsx_wobs), (True, eng.lib.gpsx_wobs_dev)):
            for message, change in refusals:
                a = {**good, **change}
                cfg = _cfg(a["guard"], a["reserved"])
                host = np.full(n_ch * 32, 0xA5, np.uint8)
                eng.h2d(d_st, st0)
                eng.h2d(d_obs, host)
                rc = fn(eng.h, None if a["null_cfg"] else cfg.ctypes.data, None if a["null_rec"] else C.c_void_p(d_rec), a["n_slots"], a["n_blocks"],
                        None if a["null_words"] else C.c_void_p(d_words), None if a["null_st"] else C.c_void_p(d_st), a["n_ch"],
                        None if a["null_out"] else (C.c_void_p(d_obs) if dev else host.ctypes.data))
                assert rc == EINVAL and eng.lib.gpsx_last_error(eng.h) == message, (dev, change, eng.lib.gpsx_last_error(eng.h))
                eng.synchronize()      # nothing was enqueued, nothing is pending
                st, dw = st0.copy(), np.zeros_like(host)
                eng.d2h(st, d_st)
                eng.d2h(dw, d_obs)
                assert (host == 0xA5).all() and (dw == 0xA5).all() and st.tobytes() == st0.tobytes(), (dev, change)
        # the ends of the guard's range are in range
        for guard in (0.0, 8184.0):
            assert eng.lib.gpsx_wobs_dev(eng.h, _cfg(guard).ctypes.data, C.c_void_p(d_rec), n_slots, n_blocks, C.c_void_p(d_words), C.c_void_p(d_st), n_ch,
                                         C.c_void_p(d_obs)) == 0
        eng.synchronize()
    finally:
        for p in (d_rec, d_words, d_st, d_obs):
            eng.free(p)


def test_records_and_words_that_do_not_count_are_ignored(eng):
    """in the slots between the records: windows without WINDOW, with an end_block outside the launch, with a phase that is none; in the
    empty word slots: HOWs that are no word, failed, not word 2, outside the launch or with a count of 100 800 -- nothing changes"""
    rec, words, n_blocks, st0, want, want_st = X.case(4)      # span 4, fillers in every other slot: free slots in between
    rec, words = rec.copy(), words.copy()
    free = rec["flags"] == 0
    slots, chans = np.nonzero(free)
    kind = (slots + chans) % 8
    rec["end_block"][free] = np.array([n_blocks, -1, 3, 3, 3, 3, -2**31, 2**31 - 1], np.int32)[kind]
    rec["flags"][free] = np.where(kind == 2, Y.F_BIT | Y.F_LOCKED, Y.F_WINDOW | Y.F_LOCKED | Y.F_BIT)      # (kind 2: in range, no WINDOW)
    rec["w"]["code_phase_fine"][free] = np.array([5.0, 5.0, 5.0, np.nan, -1.0, 16368.0, 5.0, 5.0], np.float32)[kind]
    rec["w"]["if_freq_offset_hz"][free] = -12345.0
    empty = words["flags"] == 0
    slots, chans = np.nonzero(empty)
    kind = (slots + chans) % 6
    ends = want_st["last_bit_end_p1"][chans] - 1 - st0["blocks_seen"][chans]      # (where a HOW would count: on the chain's newest bit)
    words["end_block"][empty] = np.where(kind == 4, n_blocks, np.where(kind == 5, -1, ends)).astype(np.int32)
    words["flags"][empty] = np.array([N.F_OK, N.F_WORD, 3, 3, 3, 3], np.uint8)[kind]
    words["index"][empty] = np.where(kind == 2, 3, 2)
    words["aux"][empty] = np.where(kind == 3, 100800, 101)
    assert free.sum() > 1000 and empty.sum() > 200
    check_st = st0.copy()
    check, _ = O.run(rec, n_blocks, words, check_st, X.EDGE_GUARD)
    assert check.tobytes() == want.tobytes() and check_st.tobytes() == want_st.tobytes()
    obs, after, codes = _gpu(eng, [(rec, words, n_blocks)], st0)
    assert codes == [0]
    _same(obs[0], after, want, want_st, "ignored records")


def test_an_edge_that_moved_under_the_words(eng):
    """states whose Z was moved by -7 .. 7 blocks before a launch with HOWs: |r| > 5 is counted and not used, the rest anchors with
    the nearest bit; and edge guards of 0 and 8184"""
    rec, words, n_blocks, st0, _, _ = X.case(2)
    idx = X.tiled(480)
    rec, words, st0 = np.ascontiguousarray(rec[:, idx]), np.ascontiguousarray(words[:, idx]), st0[idx].copy()
    st0["edge_block"] += (np.arange(480) // 32 - 7).astype(np.int64)
    seen = 0
    for guard in (0.0, 8184.0):
        want_st = st0.copy()
        want, bad = O.run(rec, n_blocks, words, want_st, guard)
        assert not bad
        seen = max(seen, int((want_st["n_mismatch"] != st0["n_mismatch"]).sum()))
        obs, after, codes = _gpu(eng, [(rec, words, n_blocks)], st0, edge_guard=guard)
        assert codes == [0]
        _same(obs[0], after, want, want_st, ("moved edges", guard))
    assert seen >= 20


def test_if_samples_to_observables_on_the_device(eng):
    """seed 1 of the seam scenario (delays 0.4, 16367.6 and 8184.2 samples): IF samples -> gpsx_track_loop_weighted_sync_dev ->
    gpsx_wnav_words_dev -> gpsx_wobs_dev on one stream, 3500 blocks in launches of 1000 / 1000 / 1500.  Each launch's observables
    equal the restatement on the device's own records and words; the last ones meet the truth within the CPU test's bounds
    (measured on one MI355X: channel 1 wraps 60 times, as on the restatements; errors -0.57 and -0.67 samples)"""
    from stm32f4_sdr_gps_amd import capi
    blocks = X.seam_scenario(1)
    sync = capi.wsync_cfg(K.N_COH_SEARCH, K.N_COH_LOCK, S.PULL_IN, S.STEADY, K.SYNC_BITS, K.RATIO)
    nav_cfg = np.zeros(1, capi.WNAV_CFG_DTYPE)
    nav_cfg["max_bad_words"] = 3
    cfg = _cfg(X.EDGE_GUARD)
    st = X.seam_handover(1)
    nav, obs_st = np.zeros(3, N.STATE_DTYPE), np.zeros(3, O.STATE_DTYPE)
    max_slots = capi.wsync_slots(1500, K.N_COH_SEARCH, K.N_COH_LOCK)
    d_if, d_st, d_nav, d_obs_st = eng.malloc(blocks.nbytes), eng.malloc(st.nbytes), eng.malloc(nav.nbytes), eng.malloc(obs_st.nbytes)
    d_rec, d_words, d_obs = eng.malloc(max_slots * 3 * 48), eng.malloc(N.max_words(1500) * 3 * 16), eng.malloc(3 * 32)
    want_st = obs_st.copy()
    at = 0
    try:
        eng.h2d(d_if, blocks)
        eng.h2d(d_st, st)
        eng.h2d(d_nav, nav)
        eng.h2d(d_obs_st, obs_st)
        for n in X.LAUNCHES:
            n_slots = capi.wsync_slots(n, K.N_COH_SEARCH, K.N_COH_LOCK)
            eng._chk(eng.lib.gpsx_track_loop_weighted_sync_dev(eng.h, sync.ctypes.data, C.c_void_p(d_if + at * 4092), n, C.c_void_p(d_st), 3,
                                                               C.c_void_p(d_rec)), "gpsx_track_loop_weighted_sync_dev")
            eng._chk(eng.lib.gpsx_wnav_words_dev(eng.h, nav_cfg.ctypes.data, C.c_void_p(d_rec), n_slots, n, C.c_void_p(d_nav), 3, C.c_void_p(d_words)),
                     "gpsx_wnav_words_dev")
            eng._chk(eng.lib.gpsx_wobs_dev(eng.h, cfg.ctypes.data, C.c_void_p(d_rec), n_slots, n, C.c_void_p(d_words), C.c_void_p(d_obs_st), 3,
                                           C.c_void_p(d_obs)), "gpsx_wobs_dev")
            eng.synchronize()
            rec, words, obs = np.zeros((n_slots, 3), Y.REC_DTYPE), np.zeros((N.max_words(n), 3), N.WORD_DTYPE), np.zeros(3, O.OBS_DTYPE)
            eng.d2h(rec, d_rec)
            eng.d2h(words, d_words)
            eng.d2h(obs, d_obs)
            eng.d2h(obs_st, d_obs_st)
            want, bad = O.run(rec, n, words, want_st, X.EDGE_GUARD)
            assert not bad
            _same(obs, obs_st, want, want_st, ("launch at", at))
            at += n
    finally:
        for p in (d_if, d_st, d_nav, d_obs_st, d_rec, d_words, d_obs):
            eng.free(p)
    assert int(obs_st["n_wraps"][1]) > 10 and not obs_st["n_break"][:2].any() and (obs_st["blocks_seen"] == 3500).all()
    for ch in (0, 1):
        assert int(obs["flags"][ch]) == O.F_VALID | O.F_PHASE | O.F_EDGE | O.F_TOW, ch
        err = X.error_samples(obs[ch], X.SEAM_DELAYS[ch], K.SATS[ch][3])
        print("channel", ch, "wraps", int(obs_st["n_wraps"][ch]), "error in samples", err)
        assert abs(err) < 2.0, (ch, err)
    # channel 2 sits at mid-block: whatever edge the device's synchroniser accepted, a VALID time is the truth or 1 ms off it, and flagged
    assert int(obs["flags"][2]) & O.F_EDGE and int(obs["flags"][2]) & O.F_AMBIGUOUS
    if int(obs["flags"][2]) & O.F_VALID:
        err = X.error_samples(obs[2], X.SEAM_DELAYS[2], K.SATS[2][3])
        assert min(abs(err - 16368.0 * k) for k in (-1, 0, 1)) < 4.0, err
