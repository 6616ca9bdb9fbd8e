"""The weighted path's ephemeris stage on the device (EXTENSION, not in the reference: include/gpsx.h gpsx_weph; k_weph on the vector
ALU, one channel per lane) against its exact CPU restatement (tests/weighted_eph_ref.py, pinned in tests/test_weighted_eph_reference.py
to the library's host decoder and to the reference's recorded outputs).  Every comparison is for equality, byte for byte, on the
256-byte records and on the 192-byte states, with canaries around both and the records prefilled with 0xA5.  The word records are
fabricated (tests/weighted_eph_cases.py: 32 distinct streams tiled over the channels -- frames from subframe 1, 2 and 3, failed words,
a missing record, a word out of order, re-syncs, a cutover, HOWs that do not pass, all-ones and all-zeros sets, a week that ends;
initial states from the restatement's run over the stream's earlier blocks); the last test puts the word layer's kernel in front."""
import numpy as np
import pytest

import weighted_eph_cases as X
import weighted_eph_ref as E
import weighted_gpu as G
from weighted_gpu import EINVAL, eng  # noqa: F401

pytestmark = pytest.mark.gpu

VALID, NEW = E.F_VALID, E.F_NEW


def _cfg(reserved0=0, reserved1=0):
    cfg = np.zeros(1, E.CFG_DTYPE)
    cfg["reserved0"], cfg["reserved1"] = reserved0, reserved1
    return cfg


def _gpu(eng, launches, st, dev=True):
    """the library on a copy of `st` in device memory, launch after launch.  launches: [(words [n_blocks // 600 + 2][n_ch], n_blocks)].
    -> ([records per launch], states after, [codes])"""
    n_ch, cfg = len(st), _cfg()
    fn = eng.lib.gpsx_weph_dev if dev else eng.lib.gpsx_weph

    def call(ins, sts, out, k):
        return fn(eng.h, cfg.ctypes.data, ins[0], launches[k][1], sts[0], n_ch, out)
    for words, n_blocks in launches:
        assert words.dtype == E.WORD_DTYPE and words.shape == (E.max_words(n_blocks), n_ch)
    return G.run_stage(eng, call, b"k_weph", st, [([np.ascontiguousarray(words)], E.EPH_DTYPE, (n_ch,)) for words, _ in launches], dev)


def _same(eph, after, want, want_st, what):
    G.same_rows(eph, want, (what, "records"))
    G.same_rows(after, want_st, (what, "states"))


@pytest.mark.parametrize("i", range(len(X.CASES)))
def test_records_and_states_match_the_restatement(eng, i):
    """the table: 1, 3, 64, 65, 257 and 1000 channels (one lane, part of a wave, the wave's edge, part of the last workgroup), launches
    of 4096, 1237, 600, 19 and 1 blocks, fresh states and states in the middle of a subframe, both variants.  The records were
    prefilled: equality says every byte was written"""
    words, n_blocks, st0, want, want_st = X.case(i)
    for dev in (True, False):
        eph, after, codes = _gpu(eng, [(words, n_blocks)], st0, dev=dev)
        assert codes == [0]
        _same(eph[0], after, want, want_st, (X.CASES[i], dev))


def test_the_table_covers_what_it_claims():
    """(no GPU work: the cases' own census) commits, sets that become VALID | NEW, VALID records without NEW, cleared VALID, states in
    the middle of a subframe and fresh ones, every launch length and channel count of the issue"""
    assert {c[0] for c in X.CASES} == {1, 3, 64, 65, 257, 1000} and {c[1] for c in X.CASES} == {4096, 1237, 600, 19, 1}
    new = old = commits = cleared = mid = fresh = 0
    for i in range(len(X.CASES)):
        _, _, st0, want, after = X.case(i)
        new += int((want["flags"] == VALID | NEW).sum())
        old += int((want["flags"] == VALID).sum())
        commits += int((after["n_subframes"] != st0["n_subframes"]).sum())
        cleared += int(((st0["flags"] & VALID != 0) & (after["flags"] & VALID == 0)).sum())
        mid += int((st0["cur_next"] != 0).sum())
        fresh += int((st0["blocks_seen"] == 0).sum())
    assert new >= 50 and old >= 500 and commits >= 500 and cleared >= 2 and mid >= 1000 and fresh >= 1, (new, old, commits, cleared, mid, fresh)


SPLIT = dict(n_ch=64, n_blocks=4096, warm=15000)


def _split_launches(parts):
    idx = X.tiled(SPLIT["n_ch"])
    st = X.warm_states(SPLIT["warm"])
    out, new = [], np.zeros(X.DISTINCT, np.uint32)
    for at, n in parts:
        words = X.launch_words(X.specs(), at, n)
        eph, bad = E.run(words, n, st)
        assert not bad
        new |= eph["flags"] & NEW
        out.append((np.ascontiguousarray(words[:, idx]), n))
    return out, eph[idx].copy(), st[idx].copy(), new[idx].copy()


@pytest.mark.parametrize("cut", [1, 599, 600, 2050, 4095])
def test_split_launches_equal_one_launch(eng, cut):
    """one 4096-block launch cut in two, both ways on the device: each equals the restatement of the same launches byte for byte; the
    states agree, and so do the last records but for NEW, which either part may have given"""
    warm, n_blocks = SPLIT["warm"], SPLIT["n_blocks"]
    st0 = X.warm_states(warm)[X.tiled(SPLIT["n_ch"])].copy()
    whole, want, want_st, new1 = _split_launches([(warm, n_blocks)])
    eph1, after1, codes = _gpu(eng, whole, st0)
    assert codes == [0]
    _same(eph1[0], after1, want, want_st, "one launch")
    parts, part_want, part_st, new2 = _split_launches([(warm, cut), (warm + cut, n_blocks - cut)])
    eph2, after2, codes = _gpu(eng, parts, st0)
    assert codes == [0, 0]
    _same(eph2[1], after2, part_want, part_st, ("two launches", cut))
    assert after1.tobytes() == after2.tobytes() and (new1 == new2).all() and new1.any() and not new1.all()
    both = eph2[1].copy()
    both["flags"] |= eph2[0]["flags"] & NEW
    assert both.tobytes() == eph1[0].tobytes()
    assert ((eph2[0]["flags"] | eph2[1]["flags"]) & NEW == eph1[0]["flags"] & NEW).all()


def test_every_byte_of_the_records_is_written(eng):
    """257 channels, a fresh state among them and a bad one: no byte of the 0xA5 prefill is left in either variant"""
    words, n_blocks, st0, _, _ = X.case(8)
    st0 = st0.copy()
    st0[5] = np.zeros(1, E.STATE_DTYPE)[0]
    st0["reserved"][70] = 9
    want_st = st0.copy()
    want, bad = E.run(words, n_blocks, want_st)
    assert bad == [70] and want[70].tobytes() == bytes(256) and (want["flags"] & VALID).sum() > 100
    for dev in (True, False):
        eph, after, codes = _gpu(eng, [(words, n_blocks)], st0, dev=dev)
        assert codes == [EINVAL]
        _same(eph[0], after, want, want_st, ("every byte", dev))
    assert eng.lib.gpsx_synchronize(eng.h) == 0


def test_records_that_do_not_count_change_nothing(eng):
    """in the empty word slots: records without GPSX_WNAV_WORD, with index 0 or 11, with end_block = n_blocks or -601, and -- on
    fresh channels -- with E1 < 1.  And HOWs that are OK but carry a count of 100 800 or an ID of 0, 6 or 7 do what a failed HOW does"""
    for i, ends in ((2, None), (0, -1), (4, None)):
        words, n_blocks, st0, want, want_st = X.case(i)
        words = words.copy()
        empty = words["flags"] == 0
        slots, chans = np.nonzero(empty)
        kind = (slots + chans) % 5
        assert empty.sum() >= 2
        words["end_block"][empty] = np.array([5, 5, 5, n_blocks, -601], np.int32)[kind] if ends is None else ends
        words["flags"][empty] = np.where((kind == 0) & (ends is None), E.WNAV_OK, E.WNAV_WORD | E.WNAV_OK)
        words["index"][empty] = np.array([2, 0, 11, 2, 1], np.uint8)[kind] if ends is None else 1
        words["subframe_id"][empty], words["aux"][empty], words["word"][empty] = 2, 77, 0x3FFFFFFF
        check_st = st0.copy()
        check, _ = E.run(words, n_blocks, check_st)
        assert check.tobytes() == want.tobytes() and check_st.tobytes() == want_st.tobytes()
        eph, after, codes = _gpu(eng, [(words, n_blocks)], st0)
        assert codes == [0]
        _same(eph[0], after, want, want_st, ("ignored records", i))
    # the HOWs: one stream, its second subframe's HOW in five forms
    forms = [dict(fail=(2,)), dict(how_tow=100800), dict(how_id=0), dict(how_id=6), dict(how_id=7), {}]
    rng = np.random.default_rng(3)
    sets = X.random_set(rng)
    events = [X.stream_events(300, [(1, 10, sets[1], {}), (2, 11, sets[2], kw), (3, 12, sets[3], {})]) for kw in forms]
    st0, launches, wants, want_st = np.zeros(len(forms), E.STATE_DTYPE), [], [], None
    want_st = st0.copy()
    for at in range(0, 20480, 4096):
        words = X.launch_words(events, at, 4096)
        wants.append(E.run(words, 4096, want_st)[0])
        launches.append((words, 4096))
    assert want_st["have"].tolist() == [5] * 5 + [7] and want_st["n_subframes"].tolist() == [2] * 5 + [3]
    assert all(want_st[k:k + 1].tobytes() == want_st[0:1].tobytes() for k in range(5)) and wants[-1]["flags"].tolist() == [0] * 5 + [VALID | NEW]
    eph, after, codes = _gpu(eng, launches, st0)
    assert codes == [0] * 5
    for k in range(5):
        _same(eph[k], after, wants[k], want_st, ("HOWs", k))


def test_bad_channels(eng):
    """one bad state per clause among good neighbours of the same wave: untouched, their records zero, GPSX_EINVAL from the host
    variant and from the next synchronize after the device variant; the neighbours are the restatement's -- among them states at the
    very ends of the ranges; and the same good channels without the bad ones give the same bytes"""
    words, n_blocks, st0, _, _ = X.case(2)      # 64 channels: one wave
    st0 = st0.copy()
    bad = [1 + 2 * k for k in range(len(X.BAD_FIELDS))]
    assert bad[-1] < 64
    for ch, (field, value) in zip(bad, X.BAD_FIELDS):
        X.set_field_of(st0, ch, field, value)
        if field == "flags" and value == VALID:
            st0["have"][ch] = 3
    edges = [2 + 2 * k for k in range(len(X.GOOD_EDGES))]
    for ch, (field, value) in zip(edges, X.GOOD_EDGES):
        X.set_field_of(st0, ch, field, value)
    want_st = st0.copy()
    want, found = E.run(words, n_blocks, want_st)
    assert found == bad and want_st[bad].tobytes() == st0[bad].tobytes() and want[bad].tobytes() == bytes(256 * len(bad))
    for dev in (True, False):
        eph, after, codes = _gpu(eng, [(words, n_blocks)], st0, dev=dev)
        assert codes == [EINVAL], dev
        assert dev or eng.lib.gpsx_last_error(eng.h) == b"a channel's ephemeris state is out of range (its state is untouched, its record is zero)"
        assert eng.lib.gpsx_synchronize(eng.h) == 0
        _same(eph[0], after, want, want_st, ("bad channels", dev))
    good = [c for c in range(len(st0)) if c not in bad]
    eph, after, codes = _gpu(eng, [(np.ascontiguousarray(words[:, good]), n_blocks)], st0[good].copy())
    assert codes == [0]
    _same(eph[0], after, want[good], want_st[good], "the same channels without the bad ones")


def test_argument_checks_write_nothing(eng):
    n_ch, n_blocks = 5, 1237
    words, _, st0, _, _ = X.case(3)
    words, st0 = np.ascontiguousarray(words[:, :n_ch]), st0[:n_ch].copy()
    good = dict(null_cfg=False, null_words=False, null_st=False, null_out=False, r0=0, r1=0, n_blocks=n_blocks, n_ch=n_ch)
    # every refusal with its exact text; the last row of a group fails a later clause as well: the first failing clause decides
    by_message = {
        b"null argument": [dict(null_cfg=True), dict(null_words=True), dict(null_st=True), dict(null_out=True), dict(null_words=True, n_ch=0)],
        b"reserved must be 0": [dict(r0=1), dict(r1=1), dict(r0=-1), dict(r1=-(1 << 31)), dict(r1=1, n_blocks=4097)],
        b"n_blocks must be 1..4096": [dict(n_blocks=0), dict(n_blocks=-40), dict(n_blocks=4097), dict(n_blocks=0, n_ch=0)],
        b"n_ch must be at least 1": [dict(n_ch=0), dict(n_ch=-3)],
    }
    with G.Pool() as pool:
        d_words, d_st = pool.add(G.Guarded(eng, words.nbytes, G.STATE_FILL, words)), pool.add(G.Guarded(eng, st0.nbytes, G.STATE_FILL, st0))
        outs = {True: pool.add(G.Guarded(eng, n_ch * E.EPH_DTYPE.itemsize)), False: pool.add(G.Guarded(None, n_ch * E.EPH_DTYPE.itemsize))}

        def call(a, dev):
            cfg = _cfg(a["r0"], a["r1"])
            fn = eng.lib.gpsx_weph_dev if dev else eng.lib.gpsx_weph
            return fn(eng.h, None if a["null_cfg"] else cfg.ctypes.data, None if a["null_words"] else d_words.ptr, a["n_blocks"],
                      None if a["null_st"] else d_st.ptr, a["n_ch"], None if a["null_out"] else outs[dev].ptr)
        G.refusals(eng, by_message, good, call, [d_st, *outs.values()])


def test_bits_to_ephemerides_on_the_device(eng):
    """fabricated bit records of three channels (spans of 20, three bit edges, channel 1 inverted; 61 bits of a subframe 5's end, then
    subframes 1, 2 and 3 of a set per channel: 1220 + 18 000 blocks) -> gpsx_wnav_words_dev -> gpsx_weph_dev on one stream, in
    launches of 4096 blocks.  Each launch's records equal the restatement run on the device's own words, and every channel ends
    VALID with the payload that was encoded"""
    import weighted_nav_cases as W
    import weighted_nav_ref as N
    from stm32f4_sdr_gps_amd import synth
    rng = np.random.default_rng(11)
    gen = np.random.Generator(np.random.PCG64(12))
    sets, specs = [], []
    for ch, edge in enumerate((0, 7, 19)):
        s = X.random_set(rng)
        sets.append(s)
        bits = synth.lnav_subframe(5, 200 + ch, gen)[-61:]
        for sub_id in (1, 2, 3):
            payload = [[(w >> (23 - i)) & 1 for i in range(24)] for w in s[sub_id]]
            bits += synth.lnav_subframe(sub_id, 200 + ch + sub_id, gen, payload)
        bits = np.array(bits, np.uint8) ^ (1 if ch == 1 else 0)
        specs.append((edge + 19 + 20 * np.arange(len(bits), dtype=np.int64), bits))
    n, n_launch, n_slots = 4096, 5, 205
    assert max(int(ends[-1]) for ends, _ in specs) < n * n_launch
    want_st = np.zeros(3, E.STATE_DTYPE)
    seen_new = np.zeros(3, np.uint32)
    with G.Chain(eng, None, dict(nav=np.zeros(3, N.STATE_DTYPE), eph=want_st.copy()), n, max_slots=n_slots) as chain:
        for k in range(n_launch):
            rec = W.launch_records(specs, np.arange(3), k * n, n, 20, filler=False)
            assert rec.shape == (n_slots, 3)
            chain.records(rec, n)
            chain.words()
            chain.eph()
            eng.synchronize()
            words, eph, st = chain.read("words"), chain.read("e"), chain.read("eph")
            want, bad = E.run(words, n, want_st)
            assert not bad
            _same(eph, st, want, want_st, ("launch", k))
            seen_new |= eph["flags"] & NEW
    assert (eph["flags"] & VALID).all() and (seen_new == NEW).all() and st["n_sets"].tolist() == [1, 1, 1] and st["n_subframes"].tolist() == [3, 3, 3]
    for ch in range(3):
        for k in range(3):      # (d23, d24 of word 10 are solved for parity: not the payload's)
            assert st["sf"][ch][k].tolist()[:7] == sets[ch][k + 1][:7] and int(st["sf"][ch][k][7]) >> 2 == sets[ch][k + 1][7] >> 2, (ch, k)
        assert int(st["sf_tow"][ch][0]) == 200 + ch + 1
