"""The weighted path's observables on the device (EXTENSION, not in the reference: include/gpsx.h gpsx_wobs; k_wobs on the vector ALU,
one channel per lane) against its exact CPU restatement (tests/weighted_obs_ref.py, pinned in tests/test_weighted_obs_reference.py).
Every comparison is for equality, byte for byte, on the 32-byte observables and on the 80-byte states.  The sync loop's records and
the word layer's words are fabricated (tests/weighted_obs_cases.py: 32 distinct streams tiled over the channels -- code phases that
drift and dither through the seam, sit on either side of mid-block or are no phases at all, SEARCH windows, a gap, another edge, a
week that ends, a HOW that contradicts; initial states from the restatements' run over the stream's earlier blocks); only the last
test starts from IF samples."""
import numpy as np
import pytest

import weighted_gpu as G
import weighted_loop_cases as S
import weighted_nav_ref as N
import weighted_obs_cases as X
import weighted_obs_ref as O
import weighted_sync_cases as K
import weighted_sync_ref as Y
from weighted_gpu import EINVAL, eng  # noqa: F401

pytestmark = pytest.mark.gpu

def _cfg(edge_guard, reserved=0):
    cfg = np.zeros(1, O.CFG_DTYPE)
    cfg["edge_guard"], cfg["reserved"] = edge_guard, reserved
    return cfg


def _gpu(eng, launches, st, edge_guard=X.EDGE_GUARD, dev=True):
    """the library on a copy of `st` in device memory, launch after launch.  launches: [(records [n_slots][n_ch], words
    [n_blocks // 600 + 2][n_ch], n_blocks)].  -> ([observables per launch], states after, [return codes])"""
    n_ch, cfg = len(st), _cfg(edge_guard)
    fn = eng.lib.gpsx_wobs_dev if dev else eng.lib.gpsx_wobs

    def call(ins, sts, out, k):
        return fn(eng.h, cfg.ctypes.data, ins[0], launches[k][0].shape[0], launches[k][2], ins[1], sts[0], n_ch, out)
    for rec, words, n_blocks in launches:
        assert rec.dtype == Y.REC_DTYPE and words.dtype == N.WORD_DTYPE and rec.shape[1] == n_ch and words.shape == (N.max_words(n_blocks), n_ch)
    return G.run_stage(eng, call, b"k_wobs", st,
                       [([np.ascontiguousarray(rec), np.ascontiguousarray(words)], O.OBS_DTYPE, (n_ch,)) for rec, words, _ in launches], dev)


def _same(obs, after, want_obs, want_st, what):
    G.same_rows(obs, want_obs, (what, "observables"))
    G.same_rows(after, want_st, (what, "states"))


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
    with G.Pool() as pool:
        d_rec, d_words, d_st = (pool.add(G.Guarded(eng, a.nbytes, G.STATE_FILL, a)) for a in (rec, words, st0))
        outs = {True: pool.add(G.Guarded(eng, n_ch * O.OBS_DTYPE.itemsize)), False: pool.add(G.Guarded(None, n_ch * O.OBS_DTYPE.itemsize))}

        def call(a, dev):
            cfg = _cfg(a["guard"], a["reserved"])
            fn = eng.lib.gpsx_wobs_dev if dev else eng.lib.gpsx_wobs
            return fn(eng.h, None if a["null_cfg"] else cfg.ctypes.data, None if a["null_rec"] else d_rec.ptr, a["n_slots"], a["n_blocks"],
                      None if a["null_words"] else d_words.ptr, None if a["null_st"] else d_st.ptr, a["n_ch"], None if a["null_out"] else outs[dev].ptr)
        G.refusals(eng, by_message, good, call, [d_st, *outs.values()])
        # the ends of the guard's range are in range
        for guard in (0.0, 8184.0):
            assert eng.lib.gpsx_wobs_dev(eng.h, _cfg(guard).ctypes.data, d_rec.ptr, n_slots, n_blocks, d_words.ptr, d_st.ptr, n_ch, outs[True].ptr) == 0
        eng.synchronize()


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
    states = dict(sync=X.seam_handover(1), nav=np.zeros(3, N.STATE_DTYPE), obs=np.zeros(3, O.STATE_DTYPE))
    want_st = states["obs"].copy()
    at = 0
    with G.Guarded(eng, blocks.nbytes, G.STATE_FILL, blocks) as d_if, G.Chain(eng, sync, states, 1500, edge_guard=X.EDGE_GUARD) as chain:
        for n in X.LAUNCHES:
            chain.sync(d_if.ptr.value + at * 4092, n)
            chain.words()
            chain.obs()
            eng.synchronize()
            rec, words, obs, obs_st = (chain.read(name) for name in ("rec", "words", "o", "obs"))
            want, bad = O.run(rec, n, words, want_st, X.EDGE_GUARD)
            assert not bad
            _same(obs, obs_st, want, want_st, ("launch at", at))
            at += n
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
