"""What the CPU and GPU tests of the weighted chain's almanac stage share (include/gpsx.h gpsx_walm): an encoder of almanac pages, of
subframe 4 page 18 and of subframe 5 page 25 written from the field list (not from the decoder), fabricated word records built on
weighted_eph_cases' put / subframe_events / launch_words, the table with one row per clause of the definition (a receiver of three
slots and a predicate on what comes out), 32 distinct slot streams tiled over any launch shape with warm states from the
restatement's own run, the bad states, the physics of an almanac orbit against its ephemeris, and the smoke fixture."""
import functools
import math
import os

import numpy as np

import weighted_alm_ref as R
import weighted_eph_cases as X

SC = 3.1415926535898
M24 = 0xFFFFFF

# ---- the encoder: IS-GPS-200 20.3.3.5's field list as (subframe bit, length, signed) runs, most significant run first ----------------
ALM_FIELDS = {"e": ([(68, 16)], False), "toa": ([(90, 8)], False), "di": ([(98, 16)], True), "OMGd": ([(120, 16)], True), "svh": ([(136, 8)], False),
              "rootA": ([(150, 24)], False), "OMG0": ([(180, 24)], True), "omg": ([(210, 24)], True), "M0": ([(240, 24)], True),
              "f0": ([(270, 8), (289, 3)], True), "f1": ([(278, 11)], True)}
P18_FIELDS = {"a0": ([(68, 8)], True), "a1": ([(76, 8)], True), "a2": ([(90, 8)], True), "a3": ([(98, 8)], True), "b0": ([(106, 8)], True),
              "b1": ([(120, 8)], True), "b2": ([(128, 8)], True), "b3": ([(136, 8)], True), "A1": ([(150, 24)], True),
              "A0": ([(180, 24), (210, 8)], True), "tot": ([(218, 8)], False), "wnt": ([(226, 8)], False), "dt_ls": ([(240, 8)], True),
              "wn_lsf": ([(248, 8)], False), "dn": ([(256, 8)], False), "dt_lsf": ([(270, 8)], True)}
ION_EXP = (-30, -27, -24, -24, 11, 14, 16, 16)
ALM_SIGNED = [k for k, (_, sg) in ALM_FIELDS.items() if sg]
P18_SIGNED = [k for k, (_, sg) in P18_FIELDS.items() if sg]


def bits_of(fields, name):
    return sum(n for _, n in fields[name][0])


def _encode(fields, raw, data_id, svid):
    """eight 24-bit words (words 3 .. 10) with the data ID, the page's SV ID and every field of `raw` (two's complement where signed)"""
    w8 = [0] * 8
    X.put(w8, 60, 2, data_id)
    X.put(w8, 62, 6, svid)
    for name, value in raw.items():
        runs, _ = fields[name]
        left = bits_of(fields, name)
        value &= (1 << left) - 1
        for pos, n in runs:
            left -= n
            X.put(w8, pos, n, (value >> left) & ((1 << n) - 1))
    return w8


def almanac_page(sv, raw, data_id=1):
    return _encode(ALM_FIELDS, raw, data_id, sv)


def page18(raw, data_id=1, svid=56):
    return _encode(P18_FIELDS, raw, data_id, svid)


def page25(toa, wna, health=(), data_id=1, svid=51):
    """health: {SV 1 .. 24: six-bit word}"""
    w8 = [0] * 8
    X.put(w8, 60, 2, data_id)
    X.put(w8, 62, 6, svid)
    X.put(w8, 68, 8, toa)
    X.put(w8, 76, 8, wna)
    for n, h in dict(health).items():
        X.put(w8, 90 + 30 * ((n - 1) // 4) + 6 * ((n - 1) % 4), 6, h)
    return w8


def random_raw(fields, rng, **fixed):
    raw = {k: int(rng.integers(0, 1 << bits_of(fields, k))) for k in fields}
    raw.update(fixed)
    return raw


def random_almanac(rng, sv, toa=None, **fixed):
    return almanac_page(sv, random_raw(ALM_FIELDS, rng, toa=int(rng.integers(0, 148)) if toa is None else toa, **fixed))


def as_signed(raw, bits):
    return raw - (1 << bits) if raw >> (bits - 1) else raw


def extreme(fields, signed_names, kind, rng, **fixed):
    """random raw fields with every signed one at its minimum, -1, 0 or its maximum"""
    raw = random_raw(fields, rng, **fixed)
    for k in signed_names:
        b = bits_of(fields, k)
        raw[k] = {"min": 1 << (b - 1), "-1": (1 << b) - 1, "0": 0, "max": (1 << (b - 1)) - 1}[kind]
    return raw


# ---- word events ------------------------------------------------------------------------------------------------------------------
def frame(start, sub_id, w8, tow=1000, **kw):
    return X.subframe_events(start, sub_id, tow, w8, **kw)


def events(*frames):
    return sorted((ev for f in frames for ev in f), key=lambda ev: (ev[0], ev[1]))


def respace(evs, from_word, by):
    """the words from `from_word` on end `by` blocks later: a wrong spacing"""
    return [(emit + by, end + by, *rest) if rest[1] >= from_word else (emit, end, *rest) for emit, end, *rest in evs]


def run_launches(per_channel, ch_per_rx, n_launch, n_blocks=4096, slots=None, banks=None, at=0, lengths=None):
    """the restatement over n_launch launches of n_blocks blocks (or launches of `lengths`) from block `at` -> {"launches": [(words,
    n_blocks)], "rx": [...], "alm": [...], "slots_before", "banks_before", "slots", "banks", "bad_slots", "bad_banks"}"""
    n_ch = len(per_channel)
    n_rx = n_ch // ch_per_rx
    assert n_rx * ch_per_rx == n_ch
    slots = np.zeros(n_ch, R.SLOT_DTYPE) if slots is None else slots.copy()
    banks = np.zeros(n_rx, R.BANK_DTYPE) if banks is None else banks.copy()
    out = dict(launches=[], rx=[], alm=[], slots_before=slots.copy(), banks_before=banks.copy(), ch_per_rx=ch_per_rx)
    for n_blocks in lengths or [n_blocks] * n_launch:
        words = X.launch_words(per_channel, at, n_blocks).astype(R.WORD_DTYPE)
        at += n_blocks
        rx, alm, bad_slots, bad_banks = R.run(words, n_blocks, ch_per_rx, slots, banks)
        out["launches"].append((words, n_blocks))
        out["rx"].append(rx)
        out["alm"].append(alm)
        out["bad_slots"], out["bad_banks"] = bad_slots, bad_banks
    out["slots"], out["banks"] = slots, banks
    return out


# ---- the table: one row per clause; a row is one receiver of CH slots over N_LAUNCH launches and a predicate on its outcome ------------
CH, N_LAUNCH = 3, 4      # 16 384 blocks: two subframes one after the other from block 300 end at 12 299
START = 300


class Outcome:
    """what a predicate sees of its receiver: the bank at the end, the records of every launch, the last launch's almanac records"""

    def __init__(self, bank, rxs, alms):
        self.bank, self.rxs, self.alms = bank, rxs, alms
        self.rx, self.alm = rxs[-1], alms[-1]
        self.have = int(bank["have_mask"])
        self.stored, self.changed, self.other = int(bank["n_stored"]), int(bank["n_changed"]), int(bank["n_other"])
        self.seen = [int(x["seen_mask"]) for x in rxs]
        self.new = [int(x["new_mask"]) for x in rxs]

    def page(self, e):
        return [int(w) for w in self.bank["page"][e]]

    def nothing(self):
        return self.have == 0 and self.stored == 0 and self.changed == 0 and all(int(x["flags"]) == 0 for x in self.rxs)


def _rows():
    rng = np.random.default_rng(30)
    rows = []

    def row(name, slots, check):
        slots = list(slots) + [[]] * (CH - len(slots))
        rows.append((name, [events(*s) if s and isinstance(s[0], list) else s for s in slots], check))

    def stored_at(e, w8, n_other=0):
        return lambda o: o.have == 1 << e and o.stored == 1 and o.changed == 1 and o.other == n_other and o.page(e) == w8 and sum(o.new) == 1 << e

    def other_only(o):
        return o.nothing() and o.other == 1

    for sv, sub in ((1, 5), (24, 5), (25, 4), (32, 4)):
        w8 = random_almanac(rng, sv)
        row(f"almanac SV {sv} from subframe {sub}", [[frame(START, sub, w8)]], stored_at(sv - 1, w8))
    row("dummy SV 0", [[frame(START, 5, random_almanac(rng, 0))]], other_only)
    for data_id in (0, 2, 3):
        row(f"data ID {data_id}", [[frame(START, 5, almanac_page(7, random_raw(ALM_FIELDS, rng, toa=9), data_id))]], other_only)
    row("SV 24 in subframe 4", [[frame(START, 4, random_almanac(rng, 24))]], other_only)
    row("SV 25 in subframe 5", [[frame(START, 5, random_almanac(rng, 25))]], other_only)
    row("SV ID 57 in subframe 4", [[frame(START, 4, random_almanac(rng, 57))]], other_only)
    row("SV ID 63 in subframe 4", [[frame(START, 4, random_almanac(rng, 63))]], other_only)
    row("page 25's SV ID in subframe 4, page 18's in subframe 5", [[frame(START, 4, page25(9, 9)), frame(START + 6000, 5, page18({}))]],
        lambda o: o.nothing() and o.other == 2)
    row("toa raw 148", [[frame(START, 5, random_almanac(rng, 3, toa=148))]], other_only)
    w147 = random_almanac(rng, 3, toa=147)
    row("toa raw 147", [[frame(START, 5, w147)]], lambda o: stored_at(2, w147)(o) and float(o.alm[2]["toas"]) == 602112.0)
    p18 = page18(random_raw(P18_FIELDS, rng, dn=3))
    row("page 18", [[frame(START, 4, p18)]],
        lambda o: stored_at(32, p18)(o) and int(o.rx["flags"]) == R.IONUTC and int(o.rx["dn"]) == 3 and not o.alm["flags"].any())
    p25 = page25(77, 200, {1: 63, 5: 1, 24: 32})
    row("page 25", [[frame(START, 5, p25)]],
        lambda o: stored_at(33, p25)(o) and int(o.rx["flags"]) == R.PAGE25 and int(o.rx["toa_s"]) == 77 * 4096 and int(o.rx["wna"]) == 200 + 2048
        and int(o.rx["p25_unhealthy_mask"]) == 1 | 1 << 4 | 1 << 23)
    sets = X.random_set(rng)
    row("subframes 1, 2 and 3 are ignored", [[frame(START, 1, sets[1]), frame(START + 6000, 2, sets[2])], [frame(START + 77, 3, sets[3])]],
        lambda o: o.nothing() and o.other == 0)
    good = random_almanac(rng, 9)
    for name, kw in (("a failed word", dict(fail=(6,))), ("a failed HOW", dict(fail=(2,))), ("a failed word 1", dict(fail=(1,))),
                     ("a dropped word", dict(drop=(4,))), ("a relabelled word", dict(relabel={7: 8})), ("a HOW with ID 6", dict(how_id=6))):
        row(name, [[frame(START, 5, good, **kw)]], lambda o: o.nothing() and o.other == 0)
    row("a wrong spacing", [respace(frame(START, 5, good), 6, 1)], lambda o: o.nothing() and o.other == 0)
    row("a sync pair as words 1 and 2", [[frame(START, 5, good, sync=True)]], stored_at(8, good))
    row("a sync pair whose word 1 ends before a fresh slot's block 0 (E1 < 1) does not count", [[frame(-700, 5, good, sync=True)]],
        lambda o: o.nothing() and o.other == 0)
    row("... and counts when it ends inside the stream", [[frame(4096 - 700, 5, good, sync=True)]], stored_at(8, good))
    a, b = random_almanac(rng, 11, toa=5), random_almanac(rng, 11, toa=6)
    row("two slots complete one entry in one launch", [[frame(START, 5, a)], [], [frame(START + 40, 5, b)]],
        lambda o: o.have == 1 << 10 and o.stored == 2 and o.changed == 1 and o.page(10) == b and max(int(x["n_stored"]) for x in o.rxs) == 2)
    row("two slots complete one entry in one launch, the other way round", [[frame(START + 40, 5, b)], [frame(START, 5, a)]],
        lambda o: o.have == 1 << 10 and o.stored == 2 and o.page(10) == a)
    row("the same words again", [[frame(START, 5, a), frame(START + 6000, 5, a)]],
        lambda o: o.stored == 2 and o.changed == 1 and [s for s in o.seen if s] == [1 << 10] * 2 and [n for n in o.new if n] == [1 << 10]
        and [int(x[10]["flags"]) & R.NEW for x in o.alms if int(x[10]["flags"])][:1] == [R.NEW] and int(o.alm[10]["flags"]) & R.NEW == 0)
    flipped = list(a)
    flipped[6] ^= 1
    row("one changed bit", [[frame(START, 5, a), frame(START + 6000, 5, flipped)]],
        lambda o: o.stored == 2 and o.changed == 2 and [n for n in o.new if n] == [1 << 10] * 2 and o.page(10) == flipped)
    row("a toa that is not page 25's", [[frame(START, 5, page25(6, 100))], [frame(START + 9, 5, a)]],
        lambda o: o.have == 1 << 10 | 1 << 33 and int(o.alm[10]["flags"]) & (R.HELD | R.WEEK) == R.HELD and int(o.alm[10]["week"]) == 0
        and int(o.rx["week_mask"]) == 0)
    row("a toa that is page 25's", [[frame(START, 5, page25(6, 100))], [frame(START + 9, 5, b)]],
        lambda o: int(o.alm[10]["flags"]) & (R.HELD | R.WEEK) == R.HELD | R.WEEK and int(o.alm[10]["week"]) == 2404 and int(o.rx["week_mask"]) == 1 << 10)
    for wna, week in ((34, 2338), (33, 2337), (114, 2418), (115, 2163), (0, 2304), (255, 2303)):      # (114 | 115: where the resolution turns)
        row(f"wna {wna}", [[frame(START, 5, page25(1, wna))]], lambda o, week=week: int(o.rx["wna"]) == week)
    healthy = random_almanac(rng, 2, svh=0)
    sick = random_almanac(rng, 3, svh=0x3F)
    row("health", [[frame(START, 5, healthy)], [frame(START, 5, sick)]],
        lambda o: int(o.rx["healthy_mask"]) == 2 and int(o.alm[1]["flags"]) & R.HEALTHY and not int(o.alm[2]["flags"]) & R.HEALTHY
        and int(o.alm[2]["svh"]) == 0x3F)
    for kind in ("min", "-1", "0", "max"):
        raw = extreme(ALM_FIELDS, ALM_SIGNED, kind, rng, toa=20)
        row(f"almanac: signed fields at {kind}", [[frame(START, 5, almanac_page(17, raw))]],
            lambda o, raw=raw: sv_matches(o.alm[16], 17, raw))
        raw18 = extreme(P18_FIELDS, P18_SIGNED, kind, rng, dn=7)
        row(f"page 18: signed fields at {kind}", [[frame(START, 4, page18(raw18))]], lambda o, raw18=raw18: p18_matches(o.rx, raw18))
    zero_ion = random_raw(P18_FIELDS, rng, a0=0, a1=0, a2=0, a3=0, b0=0, b1=0, b2=0, b3=0, dn=1)
    row("all-zero alpha and beta", [[frame(START, 4, page18(zero_ion))]],
        lambda o: int(o.rx["flags"]) == R.IONUTC and not o.rx["ion"].any() and p18_matches(o.rx, zero_ion))
    return rows


def scaled(raw, bits, exp, is_signed=True, semi=False):
    """a field's value from its raw integer: the conversion, the power of two, pi -- written from the field list's scale column"""
    v = float(as_signed(raw, bits) if is_signed else raw) * 2.0 ** exp
    return v * SC if semi else v


def sv_matches(rec, sv, raw):
    root_a = scaled(raw["rootA"], 24, -11, False)
    want = dict(e=scaled(raw["e"], 16, -21, False), toas=float(raw["toa"] * 4096), i0=(0.3 + scaled(raw["di"], 16, -19)) * SC,
                OMGd=scaled(raw["OMGd"], 16, -38, semi=True), A=root_a * root_a, OMG0=scaled(raw["OMG0"], 24, -23, semi=True),
                omg=scaled(raw["omg"], 24, -23, semi=True), M0=scaled(raw["M0"], 24, -23, semi=True), f0=scaled(raw["f0"], 11, -20),
                f1=scaled(raw["f1"], 11, -38))
    return int(rec["flags"]) & R.HELD and int(rec["svid"]) == sv and int(rec["svh"]) == raw["svh"] and all(float(rec[k]) == v for k, v in want.items())


def p18_matches(rx, raw):
    ion = [scaled(raw[k], 8, e) for k, e in zip(("a0", "a1", "a2", "a3", "b0", "b1", "b2", "b3"), ION_EXP)]
    week = lambda w: w + (2290 - w + 128) // 256 * 256      # noqa: E731
    ints = dict(tot_s=raw["tot"] * 4096, wnt=week(raw["wnt"]), dt_ls=as_signed(raw["dt_ls"], 8), wn_lsf=week(raw["wn_lsf"]), dn=raw["dn"],
                dt_lsf=as_signed(raw["dt_lsf"], 8))
    return (int(rx["flags"]) & R.IONUTC and rx["ion"].tolist() == ion and float(rx["A1"]) == scaled(raw["A1"], 24, -50)
            and float(rx["A0"]) == scaled(raw["A0"], 32, -30) and all(int(rx[k]) == v for k, v in ints.items()))


@functools.lru_cache(maxsize=None)
def rows():
    return _rows()


@functools.lru_cache(maxsize=None)
def table():
    """the table as one launch sequence: receiver r is row r -> run_launches' dict"""
    return run_launches([s for _, slots, _ in rows() for s in slots], CH, N_LAUNCH)


def outcomes(banks, rxs, alms):
    """[Outcome per row] from the final banks [n_rx] and every launch's records"""
    return [Outcome(banks[r], [x[r] for x in rxs], [a[r] for a in alms]) for r in range(len(banks))]


# ---- 32 distinct slot streams for any shape -------------------------------------------------------------------------------------------
DISTINCT = 32
N_FRAMES = 5


@functools.lru_cache(maxsize=None)
def streams():
    """32 streams of five subframes each, from a subframe ID and at a block offset of their own (commits fall into different launches
    from slot to slot): almanac pages of SVs that collide from stream to stream, pages 18 and 25, pages that go nowhere, failed and
    dropped words, sync pairs, subframes 1 .. 3 in between"""
    rng = np.random.default_rng(3030)
    sets = X.random_set(rng)
    # what the constellation sends: two issues of a dozen SVs' pages and of pages 18 and 25 -- every satellite sends the same ones
    pool = {sv: [random_almanac(rng, sv, toa=31 + v) for v in range(2)] for sv in list(range(1, 7)) + list(range(25, 31))}
    pool18 = [page18(random_raw(P18_FIELDS, rng)) for _ in range(2)]
    pool25 = [page25(31 + v, 252, {3 + v: 1}) for v in range(2)]
    out = []
    for j in range(DISTINCT):
        start = -700 if j == 6 else (187 * j + 5) % 6000
        frames = []
        for i in range(N_FRAMES):
            sub_id = (j + i) % 5 + 1
            kw = {}
            if sub_id <= 3:
                w8 = sets[sub_id]
            else:
                pick, issue = (3 * j + 7 * i + j // 5) % 10, int(rng.integers(0, 4) == 0)
                sv = int(rng.integers(1, 7)) + (0 if sub_id == 5 else 24)
                if pick < 5:
                    w8 = pool[sv][issue]
                elif pick < 7:
                    w8 = pool18[issue] if sub_id == 4 else pool25[issue]
                elif pick == 7:
                    w8 = random_almanac(rng, 0)
                elif pick == 8:
                    w8 = random_almanac(rng, sv, toa=200)
                else:
                    w8 = [int(x) for x in rng.integers(0, 1 << 24, 8)]
                if j % 8 == 3 and i < 2:
                    kw = dict(fail=(int(rng.integers(1, 11)),))
                elif j % 8 == 5 and i < 2:
                    kw = dict(drop=(int(rng.integers(3, 11)),))
            if j % 8 == 6 and i in (0, 3):
                kw = dict(kw, sync=True)
            frames.append(frame(start + 6000 * i, sub_id, w8, tow=(500 + 31 * j + i) % 100800, junk=i, **kw))
        out.append(events(*frames))
    return tuple(out)


def channel_streams(n_rx, ch_per_rx):
    s = streams()
    return [s[(r * 5 + j * 3 + r // 7) % DISTINCT] for r in range(n_rx) for j in range(ch_per_rx)]


@functools.lru_cache(maxsize=None)
def shape_case(n_rx, ch_per_rx, n_blocks=4096, warm_launches=3, n_launch=1):
    """a launch shape on the streams: the states warm_launches launches of 4096 blocks deep (0: fresh), then n_launch launches of n_blocks"""
    per_channel = channel_streams(n_rx, ch_per_rx)
    warm = run_launches(per_channel, ch_per_rx, warm_launches)
    return run_launches(per_channel, ch_per_rx, n_launch, n_blocks, warm["slots"], warm["banks"], at=4096 * warm_launches)


SHAPES = [(1, 1), (4, 4), (5, 33), (5, 64), (67, 1), (67, 33)]
N_BLOCKS = [1, 599, 600, 4000, 4096]


# ---- bad states ---------------------------------------------------------------------------------------------------------------------
BAD_SLOT_FIELDS = [("blocks_seen", -1), ("blocks_seen", (1 << 62) + 1), ("last_word_end_p1", -1), ("last_word_end_p1", (1 << 62) + 1), ("cur_next", 1),
                   ("cur_next", 11), ("cur_mask", 0x400), ("cur_id", 6), (("cur", 0), 1 << 24), (("cur", 7), 1 << 31), ("reserved", 1)]
GOOD_SLOT_EDGES = [("blocks_seen", 1 << 62), ("last_word_end_p1", 1 << 62), ("cur_next", 10), ("cur_next", 2), ("cur_mask", 0x3FF), ("cur_id", 5),
                   (("cur", 3), M24)]
BAD_BANK_FIELDS = [(("page", 0, 0), 1 << 24), (("page", 33, 7), 1 << 31), (("page", 17, 3), 1 << 24), ("have_mask", 1 << 34), ("have_mask", 1 << 63),
                   (("reserved", 0), 1), (("reserved", 2), 1 << 31)]
GOOD_BANK_EDGES = [(("page", 33, 7), M24), ("have_mask", (1 << 34) - 1), ("n_stored", 0xFFFFFFFF), ("n_changed", 0xFFFFFFFF), ("n_other", 0xFFFFFFFF)]
set_field_of = X.set_field_of


def bad_case():
    """(4, 4)-like shape grown to 24 receivers of 4 slots: one bad slot per clause in receivers 0 .. 10 (slot r % 4), good edges in their
    neighbours' slots, one bad bank per clause in receivers 12 .. 18, good bank edges in 19 .. 23 -> (per_channel, slots, banks)"""
    n_rx, ch = 24, 4
    base = shape_case(n_rx, ch)
    slots, banks = base["slots_before"].copy(), base["banks_before"].copy()
    for r, (field, value) in enumerate(BAD_SLOT_FIELDS):
        set_field_of(slots, r * ch + r % ch, field, value)
    for r, (field, value) in enumerate(GOOD_SLOT_EDGES):
        set_field_of(slots, r * ch + (r + 1) % ch, field, value)
    for k, (field, value) in enumerate(BAD_BANK_FIELDS):
        set_field_of(banks, 12 + k, field, value)
    for k, (field, value) in enumerate(GOOD_BANK_EDGES):
        set_field_of(banks, 19 + k, field, value)
    return channel_streams(n_rx, ch), slots, banks


# ---- physics: an almanac orbit against the ephemeris it was cut from -------------------------------------------------------------------
# MEASURED on the CPU (tests/test_weighted_alm_reference.py prints it): the largest distance between the position from the ephemeris
# and from its almanac (truncated to the almanac's fields and resolution, through the restatement's gpsx_walm_to_eph), over +-2 h
# around toa, 12 satellites above Munich (weighted_fix_cases.sky seed 0).  Other orbit seeds are held to 2 x this.
MEASURED_ORBIT_M = 1319.5
ALM_WEEK = 2300


def almanac_raw_of(row):
    """an ephemeris row (pvt_chain.quantize's) -> the almanac's raw fields: its Kepler terms moved to toa and rounded to the almanac's
    resolution; the harmonic terms, deln and idot have no place in it"""
    toa = int(round(row["toes"] / 4096.0))
    dt = toa * 4096.0 - row["toes"]
    n = math.sqrt(3.9860050E14 / row["A"] ** 3) + row["deln"]
    wrap = lambda x: (x + math.pi) % (2.0 * math.pi) - math.pi      # noqa: E731
    q = lambda v, exp, bits, semi=False: int(round(v / (SC if semi else 1.0) / 2.0 ** exp)) & ((1 << bits) - 1)      # noqa: E731
    return dict(e=q(row["e"], -21, 16), toa=toa, di=q((row["i0"] + row["idot"] * dt) / SC - 0.3, -19, 16), OMGd=q(row["OMGd"], -38, 16, True),
                svh=int(row["svh"]), rootA=q(math.sqrt(row["A"]), -11, 24), OMG0=q(wrap(row["OMG0"] + row["OMGd"] * dt), -23, 24, True),
                omg=q(row["omg"], -23, 24, True), M0=q(wrap(row["M0"] + n * dt), -23, 24, True), f0=q(row["f0"] + row["f1"] * dt, -20, 11),
                f1=q(row["f1"], -38, 11))


def almanac_records(rows_, wna=ALM_WEEK % 256):
    """ephemeris rows (SV = position + 1, at most 24) -> the restatement's records after one launch that carries every page and page 25"""
    assert len(rows_) <= 24
    per_channel = [events(frame(START, 5, almanac_page(k + 1, almanac_raw_of(row)))) for k, row in enumerate(rows_)]
    per_channel.append(events(frame(START, 5, page25(almanac_raw_of(rows_[0])["toa"], wna))))
    out = run_launches(per_channel, len(per_channel), 2)
    return out["alm"][-1][0][:len(rows_)], out["rx"][-1][0]


def row_of_eph(rec):
    """a gpsx_weph_t record -> the row pvt_chain.sat_state takes"""
    row = {k: float(rec[k]) for k in ("A", "e", "i0", "OMG0", "omg", "M0", "deln", "OMGd", "idot", "crc", "crs", "cuc", "cus", "cic", "cis", "toes",
                                      "f0", "f1", "f2")}
    return row


def orbit_distance(row, eph_rec, n=97):
    """the largest distance, over +-2 h around the almanac's toa, between the ephemeris row's position and the record's"""
    import pvt_chain as pc
    t = float(eph_rec["toes"]) + np.linspace(-7200.0, 7200.0, n)
    a, _ = pc.sat_state(row, t)
    b, _ = pc.sat_state(row_of_eph(eph_rec), t)
    return float(np.linalg.norm(a - b, axis=-1).max())


# ---- the smoke fixture (tests/golden/walm_smoke.npz) -----------------------------------------------------------------------------------
def smoke_case():
    """the table's receivers, every launch: the words, the states and banks before and after, the last launch's records"""
    t = table()
    return dict(ch=np.int32(CH), n_blocks=np.int32(4096), words=np.stack([w for w, _ in t["launches"]]), slots_before=t["slots_before"],
                banks_before=t["banks_before"], slots_after=t["slots"], banks_after=t["banks"], rx=np.stack(t["rx"]), alm=np.stack(t["alm"]))


def write_smoke(path=None):
    """(`python tests/weighted_alm_cases.py`) writes the fixture"""
    path = path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "walm_smoke.npz")
    np.savez_compressed(path, **smoke_case())
    return path


if __name__ == "__main__":
    print(write_smoke())
