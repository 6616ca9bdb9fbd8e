"""What the CPU and GPU tests of the weighted path's ephemeris stage share (include/gpsx.h gpsx_weph): consistent data sets, fabricated
word records of the word layer for any launch of a stream (a GPSX_WNAV_SYNC pair's word 1 travels with its word 2, as the word layer
writes it), 32 distinct streams that cover every rule of the definition, and the case table of the byte-for-byte comparison with
initial states taken from the restatement's own run over the stream's earlier blocks."""
import numpy as np

import weighted_eph_ref as E

OK, BAD_WORD, SYNC = E.WNAV_WORD | E.WNAV_OK, E.WNAV_WORD, E.WNAV_WORD | E.WNAV_OK | E.WNAV_SYNC
M24 = 0xFFFFFF


# ---- data sets: {1, 2, 3, 4, 5: eight 24-bit words (words 3 .. 10, d1 in bit 23)} -----------------------------------------------------
def with_issue(sets, iode):
    """subframes 1, 2, 3 made one issue of data: IODC's low byte (subframe 1 word 8), IODE (subframe 2 word 3, subframe 3 word 10)"""
    sets = {k: list(v) for k, v in sets.items()}
    sets[1][5] = (sets[1][5] & 0x00FFFF) | iode << 16
    sets[2][0] = (sets[2][0] & 0x00FFFF) | iode << 16
    sets[3][7] = (sets[3][7] & 0x00FFFF) | iode << 16
    return sets


def random_set(rng, iode=None):
    sets = {k: [int(x) for x in rng.integers(0, 1 << 24, 8)] for k in range(1, 6)}
    return with_issue(sets, int(rng.integers(0, 256)) if iode is None else iode)


def constant_set(word, iode):
    return with_issue({k: [word] * 8 for k in range(1, 6)}, iode)


def put(words8, pos, length, value):
    """`length` bits at subframe bit pos (first bit most significant) into words 3 .. 10"""
    for i in range(length):
        word, bit = divmod(pos + i, 30)
        assert 2 <= word <= 9 and bit < 24
        mask = 1 << (23 - bit)
        words8[word - 2] = (words8[word - 2] & ~mask) | (mask if (value >> (length - 1 - i)) & 1 else 0)


# every field of subframes 1 .. 3 as (subframe, runs, signed)
FIELDS = {"week": (1, [(60, 10)], False), "code": (1, [(70, 2)], False), "sva": (1, [(72, 4)], False), "svh": (1, [(76, 6)], False),
          "iodc_hi": (1, [(82, 2)], False), "flag": (1, [(90, 1)], False), "tgd": (1, [(196, 8)], True), "toc": (1, [(218, 16)], False),
          "f2": (1, [(240, 8)], True), "f1": (1, [(248, 16)], True), "f0": (1, [(270, 22)], True),
          "crs": (2, [(68, 16)], True), "deln": (2, [(90, 16)], True), "M0": (2, [(106, 8), (120, 24)], True), "cuc": (2, [(150, 16)], True),
          "e": (2, [(166, 8), (180, 24)], False), "cus": (2, [(210, 16)], True), "sqrtA": (2, [(226, 8), (240, 24)], False),
          "toes": (2, [(270, 16)], False), "fit": (2, [(286, 1)], False),
          "cic": (3, [(60, 16)], True), "OMG0": (3, [(76, 8), (90, 24)], True), "cis": (3, [(120, 16)], True),
          "i0": (3, [(136, 8), (150, 24)], True), "crc": (3, [(180, 16)], True), "omg": (3, [(196, 8), (210, 24)], True),
          "OMGd": (3, [(240, 24)], True), "idot": (3, [(278, 14)], True)}


def set_field(sets, name, raw):
    sub, runs, _ = FIELDS[name]
    length = sum(n for _, n in runs)
    for pos, n in runs:
        length -= n
        put(sets[sub], pos, n, (raw >> length) & ((1 << n) - 1))


def decode_sets():
    """about 200 consistent sets for the decoding tests: random payloads, all-ones, all-zeros, every signed field at both extremes
    (and the unsigned ones at theirs), week fields 0 / 1023 / 252, toc and toes at 0 and 0xFFFF -> [(sets, HOW count of subframe 1)]"""
    rng = np.random.default_rng(2290)
    out = [(constant_set(M24, 255), 100799), (constant_set(0, 0), 0)]
    for name, (_, runs, is_signed) in FIELDS.items():
        length = sum(n for _, n in runs)
        ends = ((1 << (length - 1)) - 1, 1 << (length - 1)) if is_signed else (0, (1 << length) - 1)      # (largest, most negative)
        for raw in ends + ((0, (1 << length) - 1) if is_signed else ()):
            sets = random_set(rng)
            set_field(sets, name, raw)
            out.append((sets, int(rng.integers(0, 100800))))      # (no field shares a bit with IODE or IODC's low byte)
    for week in (0, 1023, 252, 754, 755, 1):      # (754 | 755: where the roll-over resolution around build week 2290 turns)
        sets = random_set(rng)
        set_field(sets, "week", week)
        out.append((sets, int(rng.integers(0, 100800))))
    while len(out) < 200:
        out.append((random_set(rng), int(rng.integers(0, 100800))))
    return out


# ---- word records -----------------------------------------------------------------------------------------------------------------
def how_word(tow, sub_id):
    return ((tow & 0x1FFFF) << 7 | (sub_id & 7) << 2) << 6


def subframe_events(start, sub_id, tow, words8, fail=(), drop=(), sync=False, relabel=None, how_id=None, how_tow=None, junk=0):
    """the ten word records of the subframe whose first block is `start` (word w ends at start + 600 w - 1), as events
    (emit block, absolute end block, word, index, flags, subframe_id, aux).  fail: indices that miss GPSX_WNAV_OK; drop: indices
    without a record; sync: words 1 and 2 are a GPSX_WNAV_SYNC pair, both written when word 2 ends; relabel {index: other index};
    how_id / how_tow: what the HOW's record says instead of sub_id / tow; junk: the words' six parity bits"""
    out = []
    hid = sub_id if how_id is None else how_id
    htow = tow if how_tow is None else how_tow
    how_ok = 2 not in fail
    for w in range(1, 11):
        if w in drop:
            continue
        end = start + 600 * w - 1
        data = (0x8B << 16 | 0x1234) if w == 1 else (how_word(htow, hid) >> 6 if w == 2 else words8[w - 3])
        flags = (BAD_WORD if w in fail else OK) | (E.WNAV_SYNC if sync and w <= 2 else 0)
        index = (relabel or {}).get(w, w)
        rec_id = hid if how_ok and (w >= 2 or sync) else 0
        out.append((end + 600 if sync and w == 1 else end, end, data << 6 | (junk + w) & 63, index, flags, rec_id, htow if w == 2 and how_ok else 0))
    return out


def stream_events(start, frames):
    """frames: [(sub_id, tow, words8, {keyword arguments of subframe_events})] sent one after the other from block `start`"""
    out = []
    for i, (sub_id, tow, words8, kw) in enumerate(frames):
        out += subframe_events(start + 6000 * i, sub_id, tow, words8, **kw)
    return sorted(out, key=lambda ev: (ev[0], ev[1]))


def launch_words(events_per_channel, at, n_blocks):
    """WORD_DTYPE [n_blocks // 600 + 2][channels]: the records the word layer writes for blocks at .. at + n_blocks - 1"""
    words = np.zeros((E.max_words(n_blocks), len(events_per_channel)), E.WORD_DTYPE)
    words["end_block"] = -1
    for ch, events in enumerate(events_per_channel):
        here = [ev for ev in events if at <= ev[0] < at + n_blocks]
        assert len(here) <= words.shape[0], (ch, at, len(here))
        for k, (_, end, word, index, flags, sub_id, aux) in enumerate(here):
            words[k, ch] = (end - at, word, index, flags, sub_id, 0, aux)
    return words


def feed(events, st=None, launch=4096, until=None):
    """one channel's events through the restatement in launches of `launch` blocks -> (state array [1], [(first block, record)])"""
    st = np.zeros(1, E.STATE_DTYPE) if st is None else st
    at = int(st["blocks_seen"][0])
    until = max(ev[0] for ev in events) + 1 if until is None else until
    recs = []
    while at < until:
        n = min(launch, until - at)
        out, bad = E.run(launch_words([events], at, n), n, st)
        assert not bad
        recs.append((at, out[0].copy()))
        at += n
    return st, recs


# ---- the 32 streams -----------------------------------------------------------------------------------------------------------------
DISTINCT = 32
N_FRAMES = 15                     # subframes per stream: three frames, 90 000 blocks


def _frames(sets_of, first_id, tow0, kw_of=None):
    """N_FRAMES subframes from ID first_id on; sets_of(i) -> the data set subframe i is taken from; kw_of {i: keywords}"""
    out = []
    for i in range(N_FRAMES):
        sub_id = (first_id - 1 + i) % 5 + 1
        out.append((sub_id, (tow0 + i) % 100800, sets_of(i)[sub_id], dict((kw_of or {}).get(i, {}), junk=i)))
    return out


def streams():
    """32 streams of word events, each at a subframe offset of its own (so that commits fall into different launches from channel to
    channel): plain frames from subframe 1, 2 and 3; a failed word; a missing record (a 600-block gap); a word out of order; a
    re-sync (GPSX_WNAV_SYNC pairs, one of them at the stream's very start with its word 1 before block 0); a cutover from set A to
    set B; one set over and over; a HOW that failed, that has a count of 100 800, an ID of 0, 6 or 7; all-ones and all-zeros sets;
    a week that ends (the HOW count wraps)"""
    rng = np.random.default_rng(515)
    out = []
    for j in range(DISTINCT):
        a, b = random_set(rng), random_set(rng)
        if b[2][0] >> 16 == a[2][0] >> 16:
            b = with_issue(b, (a[2][0] >> 16) ^ 0x55)
        start = -700 if j == 6 else (187 * j + 5) % 6000
        same, first_id, tow0, kw = (lambda i: a), 1, 1000 + 17 * j, {}
        kind = j % 16
        if kind == 1:
            first_id = 2
        elif kind == 2:
            first_id = 3
        elif kind == 3:                     # a failed word in the first subframe 2: committed one frame later
            kw = {1: dict(fail=(7,))}
        elif kind == 4:                     # a missing record in the first subframe 3; the rest of it is out of step
            kw = {2: dict(drop=(5,))}
        elif kind == 5:                     # word 6 of the first subframe 1 calls itself word 8
            kw = {0: dict(relabel={6: 8})}
        elif kind == 6:                     # SYNC pairs: at the start (stream 6: word 1 ends before block 0), and after a break
            kw = {0: dict(sync=True), 6: dict(drop=(9, 10)), 7: dict(sync=True)}
        elif kind == 7:                     # cutover: subframes 2 and 3 of the second frame and all that follows are set B
            same = lambda i, a=a, b=b: a if i < 6 else b
        elif kind == 8:                     # HOWs that do not pass: failed, count 100 800, ID 0 / 6 / 7
            kw = {0: dict(fail=(2,)), 1: dict(how_tow=100800), 2: dict(how_id=0), 5: dict(how_id=6), 6: dict(how_id=7)}
        elif kind == 9:
            a = constant_set(M24, 255)
            same = lambda i, a=a: a
        elif kind == 10:
            a = constant_set(0, 0)
            same = lambda i, a=a: a
        elif kind == 11:                    # the week ends in the second frame
            tow0 = 100800 - 7
        elif kind == 12:                    # a new subframe 1 alone with another IODC: VALID goes, and comes back with set A's
            same = lambda i, a=a, b=b: b if i == 5 else a
        elif kind == 13:                    # a word 1 that failed, a word 10 that failed
            kw = {1: dict(fail=(1,)), 2: dict(fail=(10,))}
        elif kind == 14:                    # subframes 4 and 5 only at first (first_id 4), then a frame with its word 3s failed
            first_id = 4
            kw = {2: dict(fail=(3,)), 3: dict(fail=(3,))}
        out.append(stream_events(start, _frames(same, first_id, tow0, kw)))
    return out


_memo = {}


def specs():
    if "streams" not in _memo:
        _memo["streams"] = streams()
    return _memo["streams"]


def tiled(n_ch):
    return np.arange(n_ch) % DISTINCT


def warm_states(warm):
    """the 32 distinct channels' states after the restatement has run over blocks 0 .. warm - 1 in launches of at most 4096"""
    if ("warm", warm) not in _memo:
        st = np.zeros(DISTINCT, E.STATE_DTYPE)
        at = 0
        while at < warm:
            n = min(4096, warm - at)
            _, bad = E.run(launch_words(specs(), at, n), n, st)
            assert not bad
            at += n
        _memo[("warm", warm)] = st
    return _memo[("warm", warm)].copy()


# (channels, blocks of the launch, blocks before it that the initial states have seen)
CASES = [(1, 4096, 0), (3, 4096, 14000), (64, 4096, 3000), (65, 1237, 17000), (257, 600, 11500), (1000, 4096, 15000), (64, 19, 5990),
         (65, 1, 18191), (257, 4096, 33000), (1000, 1237, 47200), (64, 4096, 45000), (65, 4096, 62000)]


def case(i):
    """case i on the restatement, once per process -> (words, n_blocks, states before, records wanted, states wanted)"""
    if ("case", i) not in _memo:
        n_ch, n_blocks, warm = CASES[i]
        st0 = warm_states(warm)
        words = launch_words(specs(), warm, n_blocks)
        after = st0.copy()
        want, bad = E.run(words, n_blocks, after)
        assert not bad
        idx = tiled(n_ch)
        _memo[("case", i)] = (np.ascontiguousarray(words[:, idx]), n_blocks, st0[idx].copy(), want[idx].copy(), after[idx].copy())
    return _memo[("case", i)]


# one bad state per clause of the header's list (("flags", E.F_VALID): with have == 3), and states at the very ends of every range
BAD_FIELDS = [("blocks_seen", -1), ("blocks_seen", (1 << 62) + 1), ("last_word_end_p1", -1), ("last_word_end_p1", (1 << 62) + 1), ("cur_next", 1),
              ("cur_next", 11), ("cur_mask", 0x400), ("cur_id", 6), ("cur_tow", 100800), (("sf_tow", 0), 100800), (("sf_tow", 2), 100800),
              (("cur", 0), 1 << 24), (("cur", 7), 1 << 31), (("sf", 0, 0), 1 << 24), (("sf", 1, 3), 1 << 24), (("sf", 2, 7), 1 << 24), ("have", 8),
              ("flags", E.F_NEW), ("flags", 1 << 31), ("flags", E.F_VALID), ("reserved", 1)]
GOOD_EDGES = [("blocks_seen", 1 << 62), ("last_word_end_p1", 1 << 62), ("cur_next", 10), ("cur_next", 2), ("cur_mask", 0x3FF), ("cur_id", 5),
              ("cur_tow", 100799), (("sf_tow", 1), 100799), (("cur", 3), (1 << 24) - 1), (("sf", 2, 7), (1 << 24) - 1), ("have", 7)]


def set_field_of(st, ch, field, value):
    if isinstance(field, tuple):
        st[field[0]][(ch,) + field[1:]] = value
    else:
        st[field][ch] = value
