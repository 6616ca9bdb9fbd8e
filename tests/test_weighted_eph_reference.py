"""The weighted path's ephemeris stage (include/gpsx.h gpsx_weph), without a GPU: the layout of its structs as a C compiler sees them,
the exported entry points and the binding, the host-side gpsx_weph_to_eph, and the exact CPU restatement its GPU tests compare against
(tests/weighted_eph_ref.py): its decoding against the library's own host decoder (gps_nav_data_decode_subframe, which
tests/test_ephemeris.py pins to the reference) and against the reference's recorded outputs, its assembly rules on hand-made streams,
and one broadcast row from its quantized elements through LNAV bits and the word layer's restatement back to the same doubles."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import steps_driver as sd
import weighted_eph_cases as X
import weighted_eph_ref as E
from golden_util import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"gpsx_weph", "gpsx_weph_dev", "gpsx_weph_to_eph"}
EINVAL = -22
VALID, NEW = E.F_VALID, E.F_NEW
EPH_AT, EPH_SIZE = 344, 272      # eph_data.eph inside gps_ch_t (tests/pvt_chain.py pins the offsets), sizeof(eph_t)

LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "gpsx_compat.h"
typedef int (*dev_fn)(gpsx_ctx *, const gpsx_weph_cfg_t *, const gpsx_wnav_word_t *, int, gpsx_weph_state_t *, int, gpsx_weph_t *);
typedef int (*eph_fn)(const gpsx_weph_t *, int, eph_t *);
_Static_assert(__builtin_types_compatible_p(__typeof__(&gpsx_weph_dev), dev_fn), "the _dev entry point");
_Static_assert(__builtin_types_compatible_p(__typeof__(&gpsx_weph), dev_fn), "the host entry point");
_Static_assert(__builtin_types_compatible_p(__typeof__(&gpsx_weph_to_eph), eph_fn), "the eph_t helper");
#define S(f) printf("state.%s %zu\n", #f, offsetof(gpsx_weph_state_t, f))
#define R(f) printf("eph.%s %zu\n", #f, offsetof(gpsx_weph_t, f))
#define T(f) printf("epht.%s %zu\n", #f, offsetof(eph_t, f))
int main(void)
{
  printf("sizeof.state %zu\nsizeof.eph %zu\nsizeof.cfg %zu\nsizeof.epht %zu\n", sizeof(gpsx_weph_state_t), sizeof(gpsx_weph_t), sizeof(gpsx_weph_cfg_t),
         sizeof(eph_t));
  S(blocks_seen); S(last_word_end_p1); S(cur); S(cur_mask); S(cur_next); S(cur_id); S(cur_tow); S(sf); S(sf_tow); S(have); S(flags); S(n_sets);
  S(n_subframes); S(reserved);
  R(flags); R(iode); R(iodc); R(sva); R(svh); R(week); R(code); R(flag); R(toe_time); R(toc_time); R(ttr_time); R(toe_sec); R(toc_sec); R(ttr_sec);
  R(A); R(e); R(i0); R(OMG0); R(omg); R(M0); R(deln); R(OMGd); R(idot); R(crc); R(crs); R(cuc); R(cus); R(cic); R(cis); R(toes); R(fit); R(f0); R(f1);
  R(f2); R(tgd); R(n_sets); R(have);
  T(sat); T(iode); T(flag); T(toe); T(toc); T(ttr); T(A); T(tgd);
  printf("cfg.reserved0 %zu\ncfg.reserved1 %zu\n", offsetof(gpsx_weph_cfg_t, reserved0), offsetof(gpsx_weph_cfg_t, reserved1));
  printf("flag.valid %u\nflag.new %u\nversion %d\n", GPSX_WEPH_VALID, GPSX_WEPH_NEW, GPSX_VERSION);
  return 0;
}
"""


def test_struct_layout_as_a_c_compiler_sees_it():
    with tempfile.TemporaryDirectory(prefix="weph_layout_") as tmp:
        src, exe = os.path.join(tmp, "layout.c"), os.path.join(tmp, "layout")
        with open(src, "w") as f:
            f.write(LAYOUT_C)
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
        got = {k: int(v) for k, v in (line.split() for line in subprocess.check_output([exe], text=True).splitlines())}
    assert got["sizeof.cfg"] == 8 and got["sizeof.state"] == 192 and got["sizeof.eph"] == 256 and got["sizeof.epht"] == EPH_SIZE
    assert got["flag.valid"] == 1 and got["flag.new"] == 2 and got["version"] == 110
    assert (got["cfg.reserved0"], got["cfg.reserved1"]) == (0, 4)
    state = {k[6:]: v for k, v in got.items() if k.startswith("state.")}
    assert state == {"blocks_seen": 0, "last_word_end_p1": 8, "cur": 16, "cur_mask": 48, "cur_next": 52, "cur_id": 56, "cur_tow": 60, "sf": 64,
                     "sf_tow": 160, "have": 172, "flags": 176, "n_sets": 180, "n_subframes": 184, "reserved": 188}
    eph = {k[4:]: v for k, v in got.items() if k.startswith("eph.")}
    names = ["flags"] + list(E.INTS) + ["toe_time", "toc_time", "ttr_time", "toe_sec", "toc_sec", "ttr_sec"] + list(E.DOUBLES) + ["n_sets", "have"]
    want, at = {}, 0
    for name in names:
        want[name] = at
        at += 4 if name in ("flags", "n_sets", "have") + E.INTS else 8
    assert eph == want and at == 256 and eph["toe_time"] == 32 and eph["toe_sec"] == 56 and eph["A"] == 80 and eph["n_sets"] == 248
    assert {k[5:]: v for k, v in got.items() if k.startswith("epht.")} == {"sat": 0, "iode": 4, "flag": 28, "toe": 32, "toc": 48, "ttr": 64, "A": 80,
                                                                            "tgd": 240}
    for name, off in state.items():      # the restatement's and the binding's dtypes are that layout
        assert E.STATE_DTYPE.fields[name][1] == off, name
    for name, off in eph.items():
        assert E.EPH_DTYPE.fields[name][1] == off, name
    from stm32f4_sdr_gps_amd import capi
    assert capi.WEPH_STATE_DTYPE == E.STATE_DTYPE and capi.WEPH_DTYPE == E.EPH_DTYPE and capi.WEPH_CFG_DTYPE == E.CFG_DTYPE
    assert (capi.WEPH_FLAG_VALID, capi.WEPH_FLAG_NEW) == (VALID, NEW)
    assert capi.EPH_DTYPE.itemsize == EPH_SIZE and capi.EPH_DTYPE.fields["toe_time"][1] == 32 and capi.EPH_DTYPE.fields["ttr_sec"][1] == 72
    assert capi.EPH_DTYPE.fields["A"][1] == 80 and capi.EPH_DTYPE.fields["tgd"][1] == 240


def test_library_exports_the_stage(lib_path):
    syms = subprocess.check_output(["nm", "-D", "--defined-only", lib_path], text=True)
    assert SYMBOLS <= {line.split()[-1] for line in syms.splitlines() if line.strip()}
    from stm32f4_sdr_gps_amd import capi
    import __graft_entry__ as entry
    assert SYMBOLS <= set(entry.ABI_SYMBOLS)
    assert callable(getattr(capi.Engine, "weph", None)) and callable(capi.weph_to_eph)
    lib = capi.load_library()
    assert lib.gpsx_weph.argtypes and lib.gpsx_weph_dev.argtypes and lib.gpsx_weph_to_eph.argtypes


def _valid_record(sets, tow1):
    o = np.zeros(1, E.EPH_DTYPE)
    o["flags"], o["n_sets"], o["have"] = VALID, 1, 7
    for k, v in E.decode([sets[1], sets[2], sets[3]], tow1).items():
        o[k] = v
    return o


def test_to_eph_refuses_null_and_records_that_are_not_valid(lib_path):
    from stm32f4_sdr_gps_amd import capi
    lib = capi.load_library()
    rec = _valid_record(X.constant_set(X.M24, 255), 5)
    out = np.full(EPH_SIZE, 0xA5, np.uint8)
    assert lib.gpsx_weph_to_eph(None, 3, out.ctypes.data) == EINVAL and lib.gpsx_weph_to_eph(rec.ctypes.data, 3, None) == EINVAL
    for flags in (0, NEW, 4):
        rec["flags"] = flags
        assert lib.gpsx_weph_to_eph(rec.ctypes.data, 3, out.ctypes.data) == EINVAL and (out == 0xA5).all()
        try:
            capi.weph_to_eph(rec, 3)
            raise AssertionError("no refusal")
        except capi.GpsxError:
            pass
    rec["flags"] = VALID | NEW
    assert lib.gpsx_weph_to_eph(rec.ctypes.data, 3, out.ctypes.data) == 0
    eph = capi.weph_to_eph(rec, 3)
    assert eph.tobytes() == out.tobytes() and int(eph["sat"][0]) == 3 and not eph["tgd"][0, 1:].any()      # (every byte was written: no 0xA5 is left)
    for name in E.INTS + E.DOUBLES[:-1] + ("toe_time", "toc_time", "ttr_time", "toe_sec", "toc_sec", "ttr_sec"):
        assert eph[name][0].tobytes() == rec[name][0].tobytes(), name
    assert eph["tgd"][0, 0].tobytes() == rec["tgd"][0].tobytes()


def _decoder(lib):
    lib.gps_nav_data_decode_subframe.argtypes = [C.c_void_p]
    lib.gps_nav_data_decode_subframe.restype = C.c_uint8
    return lib.gps_nav_data_decode_subframe


def _ten_records(sub_id, tow, words8):
    ten = np.zeros(10, E.WORD_DTYPE)
    for k, (_, end, word, index, flags, rec_id, aux) in enumerate(X.subframe_events(0, sub_id, tow, words8)):
        ten[k] = (end, word, index, flags, rec_id, 0, aux)
    return ten


def test_decoding_equals_the_host_decoder_byte_for_byte(lib_path):
    """about 200 consistent sets: the restatement's record through gpsx_weph_to_eph equals, as bytes, eph_data.eph of a zeroed gps_ch_t
    that was given the three images in the order 1, 2, 3, each built by gpsx_wnav_subframe_image from the same ten records"""
    from stm32f4_sdr_gps_amd import capi
    lib = C.CDLL(lib_path)
    decode = _decoder(lib)
    cases = X.decode_sets()
    assert len(cases) >= 200
    weeks = set()
    for n, (sets, tow1) in enumerate(cases):
        prn = 1 + n % 32
        ch = np.zeros(sd.CH_SIZE, np.uint8)
        ch[664] = prn
        for sub_id in (1, 2, 3):
            ten = _ten_records(sub_id, tow1 if sub_id == 1 else (tow1 + sub_id) % 100800, sets[sub_id])
            ch[212 + 71:212 + 71 + 38] = capi.subframe_image(ten)
            assert decode(ch.ctypes.data) == sub_id
        rec = _valid_record(sets, tow1)
        got = capi.weph_to_eph(rec, prn)
        assert got.tobytes() == ch[EPH_AT:EPH_AT + EPH_SIZE].tobytes(), (n, got, ch[EPH_AT:EPH_AT + EPH_SIZE].view(capi.EPH_DTYPE))
        weeks.add(int(rec["week"][0]))
    assert {2048, 2047, 2300, 2802, 1779, 2049} <= weeks      # week fields 0, 1023, 252, and either side of the roll-over's turn


def _image_words(img):
    bits = np.unpackbits(np.asarray(img, np.uint8), bitorder="little")
    words = [int("".join(str(b) for b in bits[30 * w:30 * w + 24]), 2) for w in range(10)]
    return words[2:], words[1] >> 7, (words[1] >> 2) & 7


ALONE = {1: ("code", "sva", "svh", "flag", "tgd", "f2", "f1", "f0", "iodc", "week", "ttr_time", "ttr_sec", "toc_time", "toc_sec"),
         2: ("crs", "deln", "M0", "cuc", "e", "cus", "toes", "fit", "A"),
         3: ("cic", "OMG0", "cis", "i0", "crc", "omg", "OMGd", "iode", "idot")}


def test_decoding_equals_the_references_recorded_outputs():
    """every image of tests/golden/f8_ephemeris.npz with ID 1, 2 or 3: the fields this subframe alone determines equal the reference's
    snapshot after that call (subframe 2's IODE, which a later subframe 3 overwrites, is compared through the restatement's take)"""
    from stm32f4_sdr_gps_amd import capi
    g = load("f8_ephemeris.npz")
    seen = {1: 0, 2: 0, 3: 0}
    zero = [0] * 8
    for img, sub_id, snap in zip(g["imgs"], g["ids"], g["snaps"]):
        sub_id = int(sub_id)
        words8, tow, how_id = _image_words(img)
        assert how_id == sub_id
        if sub_id not in seen:
            continue
        seen[sub_id] += 1
        ref = np.ascontiguousarray(snap[:EPH_SIZE]).view(capi.EPH_DTYPE)[0]
        got = E.decode([words8 if k == sub_id else zero for k in (1, 2, 3)], tow)
        for name in ALONE[sub_id]:
            want = ref["tgd"][0] if name == "tgd" else ref[name]
            assert np.asarray(got[name], want.dtype).tobytes() == want.tobytes(), (sub_id, name, got[name], want)
        if sub_id == 2:
            assert E.take(words8, 60, 8) == int(ref["iode"])
    assert min(seen.values()) >= 5, seen


# ---- the assembly rules on the restatement ------------------------------------------------------------------------------------------
RNG = np.random.default_rng(77)
A, B = X.random_set(RNG, 0x31), X.random_set(RNG, 0x32)


def _frames(ids, sets=A, tow0=500, kw=None):
    return [(sub_id, tow0 + i, (sets(i) if callable(sets) else sets)[sub_id], dict((kw or {}).get(i, {}))) for i, sub_id in enumerate(ids)]


def _flags_per_subframe(events, start, n):
    """the record's flags after the launch in which subframe i ends (with the NEW of either of the two launches that cover the
    subframe) -> ([flags], state)"""
    st = np.zeros(1, E.STATE_DTYPE)
    if start:
        E.run(X.launch_words([events], 0, start), start, st)
    out = []
    for i in range(n):
        flags = 0
        for at, m in ((0, 4096), (4096, 1904)):
            rec, bad = E.run(X.launch_words([events], start + 6000 * i + at, m), m, st)
            assert not bad
            flags = int(rec["flags"][0]) | (flags & NEW)
        out.append(flags)
    return out, st


def test_valid_and_new_come_with_the_third_needed_subframe():
    for ids, want in (((1, 2, 3, 4), [0, 0, VALID | NEW, VALID]), ((2, 3, 1, 2), [0, 0, VALID | NEW, VALID]),
                      ((3, 4, 5, 1, 2, 3), [0, 0, 0, 0, VALID | NEW, VALID])):
        events = X.stream_events(100, _frames(ids))
        flags, st = _flags_per_subframe(events, 100, len(ids))
        assert flags == want, (ids, flags)
        assert int(st["n_sets"][0]) == 1 and int(st["n_subframes"][0]) == len(ids) and int(st["have"][0]) == 7
        rec = E.record(E.get_state(st, 0), 0)
        tow1 = 500 + ids.index(1)
        assert rec.tobytes() == _valid_record(A, tow1).tobytes() and int(rec["ttr_time"][0]) == 315964800 + 604800 * int(rec["week"][0]) + 6 * tow1


def _launch_ends(until, cuts=()):
    ends = sorted(set(range(4096, until, 4096)) | {until} | {c for c in cuts if 0 < c < until})
    return ends


def _run_cut(events, until, cuts=()):
    """-> (state, {baseline launch end: (record without NEW, NEW of every launch since the baseline end before)})"""
    st = np.zeros(1, E.STATE_DTYPE)
    base = set(_launch_ends(until))
    at, new, out = 0, 0, {}
    for end in _launch_ends(until, cuts):
        while at < end:      # (a cut pattern may leave more than 4096 blocks between two cuts: never, the baseline's ends are in it)
            n = min(4096, end - at)
            rec, bad = E.run(X.launch_words([events], at, n), n, st)
            assert not bad
            at += n
            new |= int(rec["flags"][0]) & NEW
        if end in base:
            rec = rec.copy()
            rec["flags"] &= ~np.uint32(NEW)
            out[end] = (rec.tobytes(), new)
            new = 0
    return st, out


def test_where_a_stream_is_cut_into_launches_does_not_matter():
    """streams with every disturbance, cut at every word boundary and at 1, 599 and 600 blocks past one: the same states, and at every
    end of a 4096-block launch the same record, NEW having come in one of the launches since the end before"""
    until = 50000
    for j in (0, 3, 6, 7, 22, 12):
        events = X.specs()[j]
        ends = sorted({ev[1] + 1 for ev in events})
        want_st, want = _run_cut(events, until)
        assert any(new for _, new in want.values())
        for past in (0, 1, 599, 600):
            st, got = _run_cut(events, until, [e + past for e in ends])
            assert st.tobytes() == want_st.tobytes() and got == want, (j, past)


def _after(frames, start=0):
    events = X.stream_events(start, frames)
    st, recs = X.feed(events)
    return st, recs


def test_a_failed_word_means_no_commit():
    for w in range(1, 11):
        st, recs = _after(_frames((1, 2, 3), kw={1: dict(fail=(w,))}))
        assert int(st["have"][0]) == 5 and int(st["n_subframes"][0]) == 2 and int(st["flags"][0]) == 0 and int(st["n_sets"][0]) == 0, w
        assert not any(int(r["flags"]) for _, r in recs)
    st, _ = _after(_frames((1, 2, 3)))
    assert int(st["have"][0]) == 7 and int(st["flags"][0]) == VALID


def test_breaks_restart_at_the_next_word_1_and_keep_valid():
    """set A is held; then a 600-block gap, a word out of order, a re-sync whose word 1 ended before its launch began: the subframe is
    lost, the next one is taken from its word 1 on, and VALID stays all the time"""
    for kw in (dict(drop=(5,)), dict(relabel={4: 5}), dict(drop=(1, 2, 3)), dict(fail=(6,))):
        frames = _frames((1, 2, 3, 4, 5, 1), kw={3: kw})
        st, recs = _after(frames)
        assert all(int(r["flags"]) & VALID for at, r in recs if at >= 3 * 6000), kw
        assert int(st["n_subframes"][0]) == 5 and int(st["n_sets"][0]) == 1 and int(st["flags"][0]) == VALID, kw
        assert int(st["sf_tow"][0][0]) == 505      # the last subframe 1 was taken whole
    # the break itself: after the word that follows the gap the channel waits for a word 1
    events = X.stream_events(0, _frames((1, 2), kw={1: dict(drop=(5,))}))
    st = np.zeros(1, E.STATE_DTYPE)
    E.run(X.launch_words([events], 0, 4096), 4096, st)
    E.run(X.launch_words([events], 4096, 4096), 4096, st)          # up to block 8191: words 1 .. 3 of the second subframe
    assert int(st["cur_next"][0]) == 4 and int(st["cur_mask"][0]) == 7
    E.run(X.launch_words([events], 8192, 1500), 1500, st)          # word 4 (ends 8399), no word 5, word 6 (ends 9599)
    assert int(st["cur_next"][0]) == 0 and int(st["cur_mask"][0]) == 0 and int(st["last_word_end_p1"][0]) == 9600
    # a re-sync in the launch's first blocks: the pair's word 1 has end_block - 600 < 0 and counts
    frames = _frames((1, 2, 3), kw={1: dict(sync=True)})
    events = X.stream_events(0, frames)
    st, _ = X.feed(events, until=6000)
    words = X.launch_words([events], 6000 + 700, 4096)
    assert int(words["end_block"][0, 0]) == -101 and int(words["flags"][0, 0]) & E.WNAV_SYNC and int(words["index"][0, 0]) == 1
    st["blocks_seen"] = 6700                                       # (nothing was sent in between)
    E.run(words, 4096, st)
    assert int(st["cur_next"][0]) == 8 and int(st["cur_mask"][0]) == 0x7F and int(st["cur_id"][0]) == 2      # words 1 .. 7 end before block 10 796
    st2, _ = X.feed(events)
    assert int(st2["have"][0]) == 7 and int(st2["flags"][0]) == VALID
    # at the stream's very start the word 1 of a pair lies before block 0 (E1 < 1): it does not count, the subframe is not taken
    events = X.stream_events(-700, _frames((1, 2, 3, 4, 5, 1), kw={0: dict(sync=True)}))
    st3, _ = X.feed(events)
    assert int(st3["n_subframes"][0]) == 5 and int(st3["sf_tow"][0][0]) == 505


def test_a_cutover_clears_valid_until_the_new_set_is_whole():
    ids = (1, 2, 3, 4, 5, 1, 2, 3, 4, 5, 1, 2)
    frames = _frames(ids, sets=lambda i: A if i < 6 else B)
    flags, st = _flags_per_subframe(X.stream_events(40, frames), 40, len(ids))
    assert flags == [0, 0, VALID | NEW, VALID, VALID, VALID, 0, 0, 0, 0, VALID | NEW, VALID]
    assert int(st["n_sets"][0]) == 2
    want = _valid_record(B, 510)
    want["n_sets"] = 2
    assert E.record(E.get_state(st, 0), 0).tobytes() == want.tobytes()


def test_one_set_over_and_over_is_new_once_and_ttr_follows():
    ids = (1, 2, 3, 4, 5) * 5
    flags, st = _flags_per_subframe(X.stream_events(0, _frames(ids)), 0, len(ids))
    assert flags == [0, 0, VALID | NEW] + [VALID] * 22 and int(st["n_sets"][0]) == 1 and int(st["n_subframes"][0]) == 25
    rec = E.record(E.get_state(st, 0), 0)
    assert int(st["sf_tow"][0][0]) == 520 and int(rec["ttr_time"][0]) == 315964800 + 604800 * int(rec["week"][0]) + 6 * 520
    # a satellite that comes back with the same set: a break, then the three subframes again -- VALID, no NEW
    frames = _frames((1, 2, 3, 4, 1, 2, 3), kw={3: dict(drop=(7, 8, 9, 10))})
    flags, st = _flags_per_subframe(X.stream_events(0, frames), 0, 7)
    assert flags == [0, 0, VALID | NEW, VALID, VALID, VALID, VALID] and int(st["n_sets"][0]) == 1


def test_subframes_4_and_5_are_counted_and_not_stored():
    st, recs = _after(_frames((4, 5, 4, 5)))
    assert int(st["n_subframes"][0]) == 4 and int(st["have"][0]) == 0 and not st["sf"].any() and not st["sf_tow"].any()
    assert all(r.tobytes() == bytes(256) for _, r in recs)
    st, _ = _after(_frames((1, 4, 5, 2)))
    assert int(st["n_subframes"][0]) == 4 and int(st["have"][0]) == 3 and st["sf"][0][2].tolist() == [0] * 8


def test_bad_states_and_the_ends_of_the_ranges():
    good = np.zeros(1, E.STATE_DTYPE)
    assert E.state_valid(E.get_state(good, 0))
    for field, value in X.BAD_FIELDS:
        st = good.copy()
        X.set_field_of(st, 0, field, value)
        if field == "flags" and value == VALID:
            st["have"] = 3
        assert not E.state_valid(E.get_state(st, 0)), (field, value)
    for field, value in X.GOOD_EDGES:
        st = good.copy()
        X.set_field_of(st, 0, field, value)
        assert E.state_valid(E.get_state(st, 0)), (field, value)


def test_a_broadcast_row_comes_back_exactly():
    """pvt_chain.quantize / subframe_payloads of one broadcast row -> synth.lnav_subframe -> the word layer's restatement -> this one:
    the record's doubles equal quantize's returned row exactly"""
    import pvt_chain as P
    import weighted_nav_cases as W
    import weighted_nav_ref as N
    from stm32f4_sdr_gps_amd import synth
    row = dict(sat=9, iode=77, iodc=77, sva=1, svh=0, week=P.WEEK, A=26559710.0 + 1234.5, e=0.00731, i0=0.9612, OMG0=-2.1, omg=1.3, M0=0.77,
               deln=4.4e-9, OMGd=-8.1e-9, idot=1.5e-10, crc=231.0, crs=-41.3, cuc=-2.1e-6, cus=7.3e-6, cic=1.1e-7, cis=-0.8e-7,
               toes=352800.0, f0=-1.7e-4, f1=3.1e-12, f2=0.0, tgd0=-1.1e-8)
    raw, q = P.quantize(row)
    pay = P.subframe_payloads(raw)
    rng = np.random.Generator(np.random.PCG64(5))
    bits = []
    for sub_id, tow in ((5, 58700), (1, 58701), (2, 58702), (3, 58703)):
        bits += synth.lnav_subframe(sub_id, tow, rng, pay.get(sub_id))
    recs, _ = W.feed(np.array(bits, np.uint8) ^ 1)      # (inverted: the word layer removes the polarity)
    assert [r[2] for r in recs] == list(range(1, 11)) * 3 and all(r[3] & N.F_OK for r in recs) and recs[0][3] & N.F_SYNC
    events = [(recs[1][0] if k == 0 else r[0],) + tuple(r) for k, r in enumerate(recs)]
    st, out = X.feed(events, launch=4096)
    rec = out[-1][1]
    assert int(rec["flags"]) & VALID and int(st["n_sets"][0]) == 1 and int(st["sf_tow"][0][0]) == 58701
    for name in E.DOUBLES:
        if name != "fit":      # (the row has none: the payload's bit is 0)
            assert float(rec[name]) == float(q["tgd0" if name == "tgd" else name]), (name, float(rec[name]), q)
    assert (int(rec["iode"]), int(rec["iodc"]), int(rec["sva"]), int(rec["svh"]), int(rec["week"]), int(rec["code"])) == (77, 77, 1, 0, P.WEEK, 1)
    assert float(rec["fit"]) == 0.0 and int(rec["toe_time"]) == 315964800 + 604800 * P.WEEK + 352800 == int(rec["toc_time"])
