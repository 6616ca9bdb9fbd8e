"""LNAV frame sync and parity-checked words on the device (EXTENSION, not in the reference: include/gpsx.h gpsx_wnav_words;
k_wnav_words on the vector ALU, one channel per lane) against its exact CPU restatement (tests/weighted_nav_ref.py, pinned in
tests/test_weighted_nav_reference.py).  Every comparison is for equality, byte for byte, on the word records and on the 64-byte
states.  The sync loop's records are fabricated (tests/weighted_nav_cases.py: 32 distinct bit streams tiled over the channels, with
bit errors, a slip, a gap, another edge and noise; initial states from the restatement's run over the stream's earlier blocks);
only the last test starts from IF samples."""

import numpy as np
import pytest

import weighted_gpu as G
import weighted_loop_cases as S
import weighted_nav_cases as W
import weighted_nav_ref as N
import weighted_sync_cases as K
import weighted_sync_ref as Y
from weighted_gpu import EINVAL, eng  # noqa: F401

pytestmark = pytest.mark.gpu


def _cfg(max_bad_words, reserved=0):
    from stm32f4_sdr_gps_amd import capi
    cfg = np.zeros(1, capi.WNAV_CFG_DTYPE)
    cfg["max_bad_words"], cfg["reserved"] = max_bad_words, reserved
    return cfg


def _gpu(eng, launches, st, max_bad_words, dev=True):
    """the library on a copy of `st` in device memory, launch after launch.  launches: [(records [n_slots][n_ch], n_blocks)].
    -> ([word records per launch], states after, [return codes])"""
    n_ch, cfg = len(st), _cfg(max_bad_words)
    fn = eng.lib.gpsx_wnav_words_dev if dev else eng.lib.gpsx_wnav_words

    def call(ins, sts, out, k):
        return fn(eng.h, cfg.ctypes.data, ins[0], launches[k][0].shape[0], launches[k][1], sts[0], n_ch, out)
    for rec, _ in launches:
        assert rec.dtype == Y.REC_DTYPE and rec.shape[1] == n_ch
    return G.run_stage(eng, call, b"k_wnav_words", st,
                       [([np.ascontiguousarray(rec)], N.WORD_DTYPE, (N.max_words(n), n_ch)) for rec, n in launches], dev)


def _same(words, after, want_words, want_st, what):
    G.same_columns(words, want_words, (what, "words"))
    G.same_rows(after, want_st, (what, "states"))


@pytest.mark.parametrize("i", range(len(W.CASES)))
def test_words_and_states_match_the_restatement(eng, i):
    """the table: 1, 3, 64, 65, 257 and 1000 channels (one lane, part of a wave, the wave's edge, part of the last workgroup), spans
    20 / 1 / 4 / 5, launches of 4096, 1237, 600, 2047, 1 and 19 blocks, fresh states and states in the middle of anything.  The word
    records were prefilled: equality says that every byte was written"""
    rec, n_blocks, st0, max_bad, want, want_st = W.case(i)
    for dev in (True, False):
        words, after, codes = _gpu(eng, [(rec, n_blocks)], st0, max_bad, dev)
        assert codes == [0]
        _same(words[0], after, want, want_st, (W.CASES[i], dev))
    W.absolute_words([(0, words[0])])      # (filled slots first, then the empty pattern)


SPLIT = dict(n_ch=64, span=20, n_blocks=4096, warm=500, max_bad=3)      # stream 0 synchronises at block 1240: 140 blocks after a cut at 600
_split = {}


def _split_whole():
    """the one launch on the restatement, once per process -> (states before, words wanted, states wanted)"""
    if not _split:
        st0 = W.warm_states(SPLIT["warm"], SPLIT["max_bad"])[W.tiled(SPLIT["n_ch"])].copy()
        after = st0.copy()
        rec = W.launch_records(W.specs(), W.tiled(SPLIT["n_ch"]), SPLIT["warm"], SPLIT["n_blocks"], SPLIT["span"])
        words, bad = N.run(rec, SPLIT["n_blocks"], after, SPLIT["max_bad"])
        assert not bad
        _split["whole"] = (st0, words, after)
    return _split["whole"]


@pytest.mark.parametrize("cut", [1, 599, 600, 2050, 4095])
def test_split_launches_equal_one_launch(eng, cut):
    """one 4096-block record array cut in two: states byte-identical, word records the same once end_block is absolute"""
    st0, want, want_st = _split_whole()
    warm, n_blocks = SPLIT["warm"], SPLIT["n_blocks"]
    parts = [(warm, cut), (warm + cut, n_blocks - cut)]
    launches = [(W.launch_records(W.specs(), W.tiled(SPLIT["n_ch"]), at, n, SPLIT["span"]), n) for at, n in parts]
    words, after, codes = _gpu(eng, launches, st0, SPLIT["max_bad"])
    assert codes == [0, 0] and after.tobytes() == want_st.tobytes()
    got = W.absolute_words([(at, w) for (at, _), w in zip(parts, words)])
    assert got == W.absolute_words([(warm, want)]) and sum(len(g) for g in got) > SPLIT["n_ch"]
    if cut == 600:      # a sync early in the second launch: its word 1 ended in the first
        early = (words[1]["flags"][0] & N.F_SYNC != 0) & (words[1]["end_block"][0] < 0)
        assert early.any() and (words[1]["end_block"][1][early] == words[1]["end_block"][0][early] + 600).all()


def test_every_byte_of_the_word_records_is_written(eng):
    """257 channels, a launch in which most slots stay empty: no byte of the 0xA5 prefill is left, and an empty slot is the pattern"""
    rec, n_blocks, st0, max_bad, want, _ = W.case(4)
    words, _, _ = _gpu(eng, [(rec, n_blocks)], st0, max_bad)
    empty = words[0]["flags"] == 0
    assert empty.any() and (~empty).any()
    assert (words[0]["end_block"][empty] == -1).all() and not words[0]["word"][empty].any() and not words[0]["aux"][empty].any()
    assert not words[0]["zero"].any() and words[0].tobytes() == want.tobytes()


BAD_FIELDS = [("mode", 2), ("mode", -1), ("inv", 2), ("inv", -1), ("word_idx", 10), ("bit_idx", 30), ("bit_idx", -1), ("fresh", 63), ("fresh", -1),
              ("bad_run", 11), ("blocks_seen", -1), ("blocks_seen", (1 << 62) + 1), ("last_bit_end_p1", -5), ("last_bit_end_p1", (1 << 62) + 1)]


def test_bad_channels(eng):
    """one bad state per field among good neighbours of the same wave: untouched, their slots empty, GPSX_EINVAL from the host
    variant and from the next synchronize after the device variant; the neighbours are the restatement's"""
    rec, n_blocks, st0, max_bad, _, _ = W.case(2)
    st0 = st0.copy()
    bad = [3 + 4 * k for k in range(len(BAD_FIELDS))]
    for ch, (field, value) in zip(bad, BAD_FIELDS):
        st0[field][ch] = value
    want_st = st0.copy()
    want, found = N.run(rec, n_blocks, want_st, max_bad)
    assert found == bad and (want["flags"][:, bad] == 0).all() and want_st[bad].tobytes() == st0[bad].tobytes()
    for dev in (True, False):
        words, after, codes = _gpu(eng, [(rec, n_blocks)], st0, max_bad, dev)
        assert codes == [EINVAL] and eng.lib.gpsx_last_error(eng.h), dev
        assert eng.lib.gpsx_synchronize(eng.h) == 0
        _same(words[0], after, want, want_st, ("bad channels", dev))
    good = [c for c in range(len(st0)) if c not in bad]
    words, after, codes = _gpu(eng, [(np.ascontiguousarray(rec[:, good]), n_blocks)], st0[good].copy(), max_bad)
    assert codes == [0]
    _same(words[0], after, np.ascontiguousarray(want[:, good]), want_st[good], "the same channels without the bad ones")


def test_argument_checks_write_nothing(eng):
    n_ch, n_blocks, n_slots = 5, 40, 2
    rec = W.launch_records(W.specs(), np.arange(n_ch), 0, n_blocks, 20)
    st0 = W.warm_states(0)[:n_ch].copy()
    good = dict(null_cfg=False, null_rec=False, null_st=False, null_out=False, max_bad=3, reserved=0, n_slots=n_slots, n_blocks=n_blocks, n_ch=n_ch)
    # every refusal with its exact text; the last row of a group fails a later clause as well: the first failing clause decides
    by_message = {
        b"null argument": [dict(null_cfg=True), dict(null_rec=True), dict(null_st=True), dict(null_out=True), dict(null_rec=True, n_ch=0)],
        b"max_bad_words must be 1..10": [dict(max_bad=0), dict(max_bad=11), dict(max_bad=-1), dict(max_bad=0, reserved=1), dict(max_bad=11, n_blocks=0)],
        b"reserved must be 0": [dict(reserved=1), dict(reserved=-1), dict(reserved=1, n_blocks=4097)],
        b"n_blocks must be 1..4096": [dict(n_blocks=0), dict(n_blocks=-40), dict(n_blocks=4097), dict(n_blocks=0, n_slots=0)],
        b"n_slots must be 1..n_blocks": [dict(n_slots=0), dict(n_slots=-1), dict(n_slots=41), dict(n_blocks=1, n_slots=2), dict(n_slots=0, n_ch=0)],
        b"n_ch must be at least 1": [dict(n_ch=0), dict(n_ch=-3)],
    }
    with G.Pool() as pool:
        d_rec, d_st = pool.add(G.Guarded(eng, rec.nbytes, G.STATE_FILL, rec)), pool.add(G.Guarded(eng, st0.nbytes, G.STATE_FILL, st0))
        n_words = N.max_words(n_blocks) * n_ch * N.WORD_DTYPE.itemsize
        outs = {True: pool.add(G.Guarded(eng, n_words)), False: pool.add(G.Guarded(None, n_words))}

        def call(a, dev):
            cfg = _cfg(a["max_bad"], a["reserved"])
            fn = eng.lib.gpsx_wnav_words_dev if dev else eng.lib.gpsx_wnav_words
            return fn(eng.h, None if a["null_cfg"] else cfg.ctypes.data, None if a["null_rec"] else d_rec.ptr, a["n_slots"], a["n_blocks"],
                      None if a["null_st"] else d_st.ptr, a["n_ch"], None if a["null_out"] else outs[dev].ptr)
        G.refusals(eng, by_message, good, call, [d_st, *outs.values()])


def test_records_that_are_no_bits_are_ignored(eng):
    """BIT records whose end_block lies outside the launch, and BIT without WINDOW, in the slots between the bits: nothing changes"""
    rec, n_blocks, st0, max_bad, want, want_st = W.case(4)      # span 4: four slots in five hold no bit
    rec = rec.copy()
    free = (rec["flags"] & Y.F_BIT) == 0
    slots, chans = np.nonzero(free)
    values = np.array([n_blocks, n_blocks + 5, -1, -7, -2**31, 2**31 - 1, 4096, 3], np.int32)
    rec["end_block"][free] = values[(slots + chans) % 8]
    rec["flags"][free] = np.where((slots + chans) % 8 == 7, Y.F_BIT | Y.F_LOCKED, W.F_BITREC)      # (the in-range one lacks WINDOW)
    rec["bit_ip"][free] = -12345
    check_st = st0.copy()
    check, _ = N.run(rec, n_blocks, check_st, max_bad)
    assert check.tobytes() == want.tobytes() and check_st.tobytes() == want_st.tobytes()
    words, after, codes = _gpu(eng, [(rec, n_blocks)], st0, max_bad)
    assert codes == [0]
    _same(words[0], after, want, want_st, "ignored records")


def test_if_samples_to_words_on_the_device(eng):
    """seed 1: IF samples -> gpsx_track_loop_weighted_sync_dev -> gpsx_wnav_words_dev on one stream, 3500 blocks in launches of
    1000 / 1000 / 1500.  What comes back per launch is 16 B x (n_blocks / 600 + 2) per channel: the sync at the restatement's end
    blocks, words 3 and 4 passed, the source bits those that were synthesised"""
    from stm32f4_sdr_gps_amd import capi
    blocks, truth = W.e2e_scenario(1)
    sync = capi.wsync_cfg(K.N_COH_SEARCH, K.N_COH_LOCK, S.PULL_IN, S.STEADY, K.SYNC_BITS, K.RATIO)
    word_list, copied, at = [], 0, 0
    with G.Guarded(eng, blocks.nbytes, G.STATE_FILL, blocks) as d_if, \
            G.Chain(eng, sync, dict(sync=K.handover_states(1), nav=np.zeros(3, N.STATE_DTYPE)), 1500) as chain:
        for n in (1000, 1000, 1500):
            chain.sync(d_if.ptr.value + at * 4092, n)
            chain.words()
            eng.synchronize()
            words = chain.read("words")
            copied += words.nbytes
            word_list.append((at, words))
            at += n
        nav = chain.read("nav")
    assert copied == 16 * 3 * (3 + 3 + 4)
    words_abs = W.absolute_words(word_list)
    for ch in range(3):
        assert int(nav["mode"][ch]) == N.SYNCED and int(nav["n_sync"][ch]) == 1 and int(nav["n_drop"][ch]) == 0 and int(nav["blocks_seen"][ch]) == 3500
        W.e2e_check_words(ch, words_abs[ch], W.e2e_bit_seed(1, ch), int(nav["inv"][ch]))
        # inv against the truth: the newest received bits (hist, polarity as received) are the satellite's, inverted iff inv
        last = (int(nav["last_bit_end_p1"][ch]) - 1 - 19 - K.EDGES_FOUND[ch]) // 20
        got = [(int(nav["hist"][ch]) >> k) & 1 for k in range(40)]
        assert got == [int(truth[ch][last - k]) ^ int(nav["inv"][ch]) for k in range(40)], ch
