"""The weighted chain's almanac stage on the device (EXTENSION, not in the reference: include/gpsx.h gpsx_walm; k_walm on the vector
ALU, a wave per receiver) against its exact CPU restatement (tests/weighted_alm_ref.py, held to the header in
tests/test_weighted_alm_reference.py).  Every comparison is for equality, byte for byte, on the slot states, the banks and both record
arrays, with canaries around all four and the records prefilled with 0xA5: every double is an integer times a power of two through at
most two further IEEE operations that Python repeats.  The word records are fabricated (tests/weighted_alm_cases.py); the last test
puts the word layer's kernel in front and the ephemeris stage beside."""
import numpy as np
import pytest

import weighted_alm_cases as A
import weighted_alm_ref as R
import weighted_gpu as G
from weighted_gpu import EINVAL, eng  # noqa: F401

pytestmark = pytest.mark.gpu

BAD_TEXT = b"a slot's almanac state or a receiver's almanac bank is out of range (it is untouched, a bad bank's records are zero)"
OUT_DTYPE = np.dtype("u1")


def _cfg(ch, reserved=(0, 0, 0)):
    cfg = np.zeros(1, R.CFG_DTYPE)
    cfg["ch_per_rx"], cfg["reserved"] = ch, reserved
    return cfg


def _gpu(eng, launches, ch, slots, banks, dev=True, want_alm=True):
    """the library on copies of the states in device memory, launch after launch.  launches: [(words, n_blocks)].  The two record arrays
    are one guarded output buffer: rx [n_rx], then alm [n_rx][32] (160 n_rx is a multiple of 16).
    -> ([(rx, alm) per launch], slots after, banks after, [codes])"""
    n_rx, cfg = len(banks), _cfg(ch)
    fn = eng.lib.gpsx_walm_dev if dev else eng.lib.gpsx_walm
    rx_bytes, alm_bytes = n_rx * R.RX_DTYPE.itemsize, n_rx * 32 * R.SV_DTYPE.itemsize

    def call(ins, sts, out, k):
        return fn(eng.h, cfg.ctypes.data, ins[0], launches[k][1], n_rx, sts[0], sts[1], out, (out.value + rx_bytes) if want_alm else None)
    outs, (s, b), codes = G.run_stage(eng, call, b"k_walm", [slots, banks],
                                      [([np.ascontiguousarray(w)], OUT_DTYPE, (rx_bytes + alm_bytes,)) for w, _ in launches], dev)
    recs = []
    for o in outs:
        if not want_alm:
            assert (o[rx_bytes:] == G.OUT_FILL).all(), "d_alm NULL: nothing behind the receiver records may be written"
        recs.append((o[:rx_bytes].view(R.RX_DTYPE).copy(), o[rx_bytes:].view(R.SV_DTYPE).reshape(n_rx, 32).copy()))
    return recs, s, b, codes


def _same(got, s, b, want, what):
    """got: _gpu's records of the launches; want: run_launches' dict"""
    for k, (rx, alm) in enumerate(got):
        G.same_rows(rx, want["rx"][k], (what, "rx", k))
        G.same_rows(alm, want["alm"][k], (what, "alm", k))
    G.same_rows(s, want["slots"], (what, "slots"))
    G.same_rows(b, want["banks"], (what, "banks"))


@pytest.mark.parametrize("shape", A.SHAPES)
def test_records_states_and_banks_match_the_restatement(eng, shape):
    """(n_rx, ch_per_rx) = (1, 1), (4, 4), (5, 33): a second workgroup, (5, 64): every lane a slot, (67, 1), (67, 33); states and banks
    three launches deep, two launches of 4096, both variants.  The records were prefilled: equality says every byte was written"""
    c = A.shape_case(*shape, n_launch=2)
    for dev in (True, False):
        got, s, b, codes = _gpu(eng, c["launches"], shape[1], c["slots_before"], c["banks_before"], dev)
        assert codes == [0, 0]
        _same(got, s, b, c, (shape, dev))


@pytest.mark.parametrize("n_blocks", A.N_BLOCKS)
def test_launch_lengths(eng, n_blocks):
    """1, 599, 600, 4000 and 4096 blocks (two to eight word slots) on (5, 33), three launches of each from warm states"""
    c = A.shape_case(5, 33, n_blocks, 3, 3)
    got, s, b, codes = _gpu(eng, c["launches"], 33, c["slots_before"], c["banks_before"])
    assert codes == [0, 0, 0]
    _same(got, s, b, c, n_blocks)


def test_the_table_on_the_device(eng):
    """the table's own shape (a receiver per row, three slots) from fresh states over its four launches: byte for byte, and every row's
    predicate holds on the device's bytes"""
    t = A.table()
    got, s, b, codes = _gpu(eng, t["launches"], A.CH, t["slots_before"], t["banks_before"])
    assert codes == [0] * A.N_LAUNCH
    _same(got, s, b, t, "table")
    outcomes = A.outcomes(b, [rx for rx, _ in got], [alm for _, alm in got])
    for (name, _, check), o in zip(A.rows(), outcomes):
        assert check(o), name


def test_without_alm_and_the_three_entry_points_agree(eng):
    """d_alm NULL: the receiver records, states and banks are the same and nothing else is written; the host variant, the _dev variant
    and the binding give the same bytes"""
    from stm32f4_sdr_gps_amd import capi
    c = A.shape_case(5, 33)
    full, s1, b1, _ = _gpu(eng, c["launches"], 33, c["slots_before"], c["banks_before"])
    for dev in (True, False):
        got, s, b, codes = _gpu(eng, c["launches"], 33, c["slots_before"], c["banks_before"], dev, want_alm=False)
        assert codes == [0]
        G.same_rows(got[0][0], c["rx"][0], ("no alm", dev))
        assert s.tobytes() == s1.tobytes() and b.tobytes() == b1.tobytes()
    words, n_blocks = c["launches"][0]
    with G.Pool() as pool:
        d_w = pool.add(G.Guarded(eng, words.nbytes, G.STATE_FILL, words))
        d_s = pool.add(G.Guarded(eng, c["slots_before"].nbytes, G.STATE_FILL, c["slots_before"]))
        d_b = pool.add(G.Guarded(eng, c["banks_before"].nbytes, G.STATE_FILL, c["banks_before"]))
        rx, alm = eng.walm(capi.walm_cfg(33), d_w.ptr.value, n_blocks, 5, d_s.ptr.value, d_b.ptr.value)
        assert rx.tobytes() == full[0][0].tobytes() and alm.tobytes() == full[0][1].tobytes()
        assert d_s.get(R.SLOT_DTYPE, (5 * 33,)).tobytes() == s1.tobytes() and d_b.get(R.BANK_DTYPE, (5,)).tobytes() == b1.tobytes()
        d_s.refill()
        d_b.refill()
        assert eng.walm(capi.walm_cfg(33), d_w.ptr.value, n_blocks, 5, d_s.ptr.value, d_b.ptr.value, want_alm=False).tobytes() == rx.tobytes()


def test_receivers_permuted(eng):
    """the receivers of (67, 33) in another order: each one's records, states and bank are what they were"""
    c = A.shape_case(67, 33)
    perm = np.random.default_rng(67).permutation(67)
    ch = 33
    idx = (perm[:, None] * ch + np.arange(ch)[None, :]).reshape(-1)
    words, n_blocks = c["launches"][0]
    got, s, b, codes = _gpu(eng, [(np.ascontiguousarray(words[:, idx]), n_blocks)], ch, c["slots_before"][idx].copy(), c["banks_before"][perm].copy())
    assert codes == [0]
    G.same_rows(got[0][0], c["rx"][0][perm], "rx")
    G.same_rows(got[0][1], c["alm"][0][perm], "alm")
    G.same_rows(s, c["slots"][idx], "slots")
    G.same_rows(b, c["banks"][perm], "banks")


def test_a_second_call_on_the_same_words(eng):
    """the same launch's words given again to the states the first call left: the restatement says what that is (the words lie in the
    past of blocks_seen, they are out of step) -- and no bank gains a page it did not have"""
    c = A.shape_case(5, 33)
    words, n_blocks = c["launches"][0]
    slots, banks = c["slots"].copy(), c["banks"].copy()
    rx, alm, bad_s, bad_b = R.run(words, n_blocks, 33, slots, banks)
    assert not bad_s and not bad_b
    want = dict(rx=[c["rx"][0], rx], alm=[c["alm"][0], alm], slots=slots, banks=banks)
    got, s, b, codes = _gpu(eng, [(words, n_blocks)] * 2, 33, c["slots_before"], c["banks_before"])
    assert codes == [0, 0]
    _same(got, s, b, want, "second call")


def test_bad_slots_and_banks_are_left_untouched_and_their_neighbours_served(eng):
    """one bad slot per clause, one bad bank per clause, states at the very ends of every range among them: the bad ones untouched, a
    bad bank's records zero, GPSX_EINVAL from the host variant and from the next synchronize after _dev, everything else the restatement's"""
    per_channel, slots, banks = A.bad_case()
    want = A.run_launches(per_channel, 4, 1, slots=slots, banks=banks, at=3 * 4096)
    assert len(want["bad_slots"]) == len(A.BAD_SLOT_FIELDS) and len(want["bad_banks"]) == len(A.BAD_BANK_FIELDS)
    for dev in (True, False):
        got, s, b, codes = _gpu(eng, want["launches"], 4, slots, banks, dev)
        assert codes == [EINVAL], dev
        assert dev or eng.lib.gpsx_last_error(eng.h) == BAD_TEXT
        assert eng.lib.gpsx_synchronize(eng.h) == 0
        _same(got, s, b, want, ("bad", dev))
        assert s[want["bad_slots"]].tobytes() == slots[want["bad_slots"]].tobytes() and b[want["bad_banks"]].tobytes() == banks[want["bad_banks"]].tobytes()
        for r in want["bad_banks"]:
            assert got[0][0][r].tobytes() == bytes(160) and got[0][1][r].tobytes() == bytes(96 * 32)


def test_argument_checks_write_nothing(eng):
    n_rx, ch, n_blocks = 5, 33, 4096
    c = A.shape_case(n_rx, ch)
    words = c["launches"][0][0]
    good = dict(null=None, ch=ch, reserved=(0, 0, 0), n_blocks=n_blocks, n_rx=n_rx, off=None, overlap=None, null_alm=False)
    by_message = {
        b"null argument": [dict(null="cfg"), dict(null="words"), dict(null="slots"), dict(null="banks"), dict(null="rx"), dict(null="rx", ch=0)],
        b"ch_per_rx must be 1..64": [dict(ch=0), dict(ch=65), dict(ch=-1), dict(ch=0, reserved=(1, 0, 0))],
        b"reserved must be 0": [dict(reserved=(1, 0, 0)), dict(reserved=(0, -1, 0)), dict(reserved=(0, 0, 1 << 30)), dict(reserved=(0, 0, 1), n_blocks=0)],
        b"n_blocks must be 1..4096": [dict(n_blocks=0), dict(n_blocks=-5), dict(n_blocks=4097), dict(n_blocks=0, n_rx=0)],
        b"n_rx must be 1..1048576": [dict(n_rx=0), dict(n_rx=-1), dict(n_rx=(1 << 20) + 1), dict(n_rx=0, off="slots")],
        b"d_words, d_slot_state and d_bank must be 16-byte aligned": [dict(off="words"), dict(off="slots"), dict(off="banks")],
        b"two arrays overlap": [dict(overlap="slots_banks"), dict(overlap="rx_alm"), dict(overlap="words_slots")],
    }
    dev_only = {b"d_rx and d_alm must be 16-byte aligned": [dict(off="rx"), dict(off="alm")]}
    rx_bytes, alm_bytes = n_rx * 160, n_rx * 32 * 96
    with G.Pool() as pool:
        d_w = pool.add(G.Guarded(eng, words.nbytes, G.STATE_FILL, words))
        d_s = pool.add(G.Guarded(eng, c["slots_before"].nbytes, G.STATE_FILL, c["slots_before"]))
        d_b = pool.add(G.Guarded(eng, c["banks_before"].nbytes, G.STATE_FILL, c["banks_before"]))
        outs = {True: pool.add(G.Guarded(eng, rx_bytes + alm_bytes)), False: pool.add(G.Guarded(None, rx_bytes + alm_bytes))}

        def call(a, dev):
            cfg = _cfg(a["ch"], a["reserved"])
            fn = eng.lib.gpsx_walm_dev if dev else eng.lib.gpsx_walm
            p = dict(cfg=cfg.ctypes.data, words=d_w.ptr.value, slots=d_s.ptr.value, banks=d_b.ptr.value, rx=outs[dev].ptr.value,
                     alm=outs[dev].ptr.value + rx_bytes)
            if a["off"]:
                p[a["off"]] += 8
            if a["overlap"] == "slots_banks":
                p["banks"] = p["slots"] + 64 * (n_rx * ch - 1)
            elif a["overlap"] == "rx_alm":
                p["alm"] = p["rx"] + 16 * (rx_bytes // 16 - 1)
            elif a["overlap"] == "words_slots":
                p["slots"] = p["words"] + 16
            if a["null"]:
                p[a["null"]] = None
            return fn(eng.h, p["cfg"], p["words"], a["n_blocks"], a["n_rx"], p["slots"], p["banks"], p["rx"], None if a["null_alm"] else p["alm"])
        G.refusals(eng, by_message, good, call, [d_s, d_b, *outs.values()])
        for message, changes in dev_only.items():
            for change in changes:
                assert call({**good, **change}, True) == EINVAL and eng.lib.gpsx_last_error(eng.h) == message
                assert all(x.untouched() for x in (d_s, d_b, outs[True]))
        # (a size product cannot overflow 64 bits inside the ranges above: 2^20 receivers x 64 slots x 8 word slots x 16 bytes is 2^33)


def test_bits_to_almanac_on_the_device_beside_the_ephemeris_stage(eng):
    """fabricated bit records of two receivers x 3 slots (spans of 20, a bit edge and a polarity per channel): subframes 4 and 5 with
    pages 18 and 25 and four almanac pages, subframes 1 .. 3 in between -- 61 bits of a subframe's end, then six subframes: 37 220
    blocks in launches of 4096 -> gpsx_wnav_words_dev -> gpsx_weph_dev and gpsx_walm_dev on the same d_words.  Each launch's records
    equal the restatement run on the device's own words; at the end both banks hold exactly the pages sent, ion[] is the encoded set,
    the slot that failed a word contributed nothing, and gpsx_weph's outputs are byte for byte what they are without the new call"""
    import weighted_eph_cases as X
    import weighted_eph_ref as E
    import weighted_nav_cases as W
    import weighted_nav_ref as N
    from stm32f4_sdr_gps_amd import synth
    rng = np.random.default_rng(30)
    sets = X.random_set(rng)
    raw18 = A.random_raw(A.P18_FIELDS, rng, dn=4)
    p18, p25 = A.page18(raw18), A.page25(40, 252, {7: 5})
    alm = {sv: A.random_almanac(rng, sv, toa=40) for sv in (3, 9, 26, 31)}
    # what each channel sends as its subframes 4 and 5 (twice each): receiver 0 = channels 0 .. 2, receiver 1 = channels 3 .. 5
    plan = [((4, p18), (5, alm[3]), (4, alm[26]), (5, p25)), ((4, alm[31]), (5, alm[9]), (4, p18), (5, alm[3])), ((4, alm[26]), (5, p25), (4, alm[31]), (5, alm[9])),
            ((4, alm[26]), (5, alm[9]), (4, p18), (5, p25)), ((4, p18), (5, p25), (4, alm[31]), (5, alm[3])), ((4, alm[31]), (5, alm[3]), (4, alm[26]), (5, alm[9]))]
    order = (4, 5, 1, 4, 5, 2)      # six subframes a channel: its two 4s and two 5s with a 1 and a 2 in between
    specs = []
    for ch, pages in enumerate(plan):
        gen = np.random.Generator(np.random.PCG64(100 + ch))
        bits = synth.lnav_subframe(3, 300 + ch, gen)[-61:]
        mine = {4: [w for s_, w in pages if s_ == 4], 5: [w for s_, w in pages if s_ == 5]}
        for k, sub_id in enumerate(order):
            w8 = mine[sub_id].pop(0) if sub_id >= 4 else sets[sub_id]
            payload = [[(w >> (23 - i)) & 1 for i in range(24)] for w in w8]
            sub = synth.lnav_subframe(sub_id, 300 + ch + k + 1, gen, payload)
            if ch == 5 and k == 3:      # receiver 1's slot 2 fails a word of its second subframe 4 (the only place it sends SV 26 again)
                sub[30 * 5 + 7] ^= 1
            bits += sub
        bits = np.array(bits, np.uint8) ^ (ch & 1)
        specs.append(((0, 7, 19, 3, 11, 16)[ch] + 19 + 20 * np.arange(len(bits), dtype=np.int64), bits))
    n, n_slots = 4096, 205
    n_launch = -(-max(int(ends[-1]) + 1 for ends, _ in specs) // n)
    assert n_launch == 10
    cfg = _cfg(3)
    want_slots, want_banks, want_eph = np.zeros(6, R.SLOT_DTYPE), np.zeros(2, R.BANK_DTYPE), np.zeros(6, E.STATE_DTYPE)
    eph_alone = []
    for with_alm in (False, True):
        with G.Chain(eng, None, dict(nav=np.zeros(6, N.STATE_DTYPE), eph=np.zeros(6, E.STATE_DTYPE)), n, max_slots=n_slots) as chain, G.Pool() as pool:
            d_s = pool.add(G.Guarded(eng, want_slots.nbytes, G.STATE_FILL, np.zeros(6, R.SLOT_DTYPE)))
            d_b = pool.add(G.Guarded(eng, want_banks.nbytes, G.STATE_FILL, np.zeros(2, R.BANK_DTYPE)))
            d_rx, d_alm = pool.add(G.Guarded(eng, 2 * 160)), pool.add(G.Guarded(eng, 2 * 32 * 96))
            for k in range(n_launch):
                rec = W.launch_records(specs, np.arange(6), k * n, n, 20, filler=False)
                chain.records(rec, n)
                chain.words()
                chain.eph()
                if with_alm:
                    assert eng.lib.gpsx_walm_dev(eng.h, cfg.ctypes.data, chain.buf["words"].ptr, n, 2, d_s.ptr, d_b.ptr, d_rx.ptr, d_alm.ptr) == 0
                eng.synchronize()
                words, e, st = chain.read("words"), chain.read("e"), chain.read("eph")
                if not with_alm:
                    eph_alone.append((e, st))
                    continue
                assert e.tobytes() == eph_alone[k][0].tobytes() and st.tobytes() == eph_alone[k][1].tobytes(), k
                rx, alm_recs, bad_s, bad_b = R.run(words.astype(R.WORD_DTYPE), n, 3, want_slots, want_banks)
                assert not bad_s and not bad_b
                G.same_rows(d_rx.get(R.RX_DTYPE, (2,)), rx, ("rx", k))
                G.same_rows(d_alm.get(R.SV_DTYPE, (2, 32)), alm_recs, ("alm", k))
                G.same_rows(d_s.get(R.SLOT_DTYPE, (6,)), want_slots, ("slots", k))
                G.same_rows(d_b.get(R.BANK_DTYPE, (2,)), want_banks, ("banks", k))
            if with_alm:
                banks, rx = d_b.get(R.BANK_DTYPE, (2,)), d_rx.get(R.RX_DTYPE, (2,))
    sent = 1 << 2 | 1 << 8 | 1 << 25 | 1 << 30 | 1 << 32 | 1 << 33
    assert banks["have_mask"].tolist() == [sent, sent] and banks["n_stored"].tolist() == [12, 11] and banks["n_other"].tolist() == [0, 0]
    for r in range(2):
        for e, w8 in ((2, alm[3]), (8, alm[9]), (25, alm[26]), (30, alm[31]), (32, p18), (33, p25)):      # (d23, d24 of word 10 are solved for parity)
            got = [int(w) for w in banks["page"][r][e]]
            assert got[:7] == w8[:7] and got[7] >> 2 == w8[7] >> 2, (r, e)
        assert A.p18_matches(rx[r], raw18) and int(rx[r]["flags"]) == R.IONUTC | R.PAGE25 and int(rx[r]["week_mask"]) == sent & 0xFFFFFFFF
        assert int(rx[r]["p25_unhealthy_mask"]) == 1 << 6 and int(rx[r]["wna"]) == 2300
