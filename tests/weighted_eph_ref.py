"""An exact CPU restatement of the weighted path's ephemeris stage (include/gpsx.h gpsx_weph), for the tests: the header's three steps
per word record and its commit, in its order, on Python integers; the decoding on Python integers and np.float64, one IEEE operation
at a time in the order include/gpsx.h names (the decoder's own: stm32f4_sdr_gps_amd/csrc/gpsx_ephemeris.cpp, which
tests/test_ephemeris.py pins to the reference byte for byte).  Nothing of the library's code is included or imported."""
import numpy as np

F_VALID, F_NEW = 1, 2
WNAV_WORD, WNAV_OK, WNAV_SYNC = 1, 2, 8
MAX_COUNT = 1 << 62
TOW_COUNTS = 100800
M32 = 0xFFFFFFFF

CFG_DTYPE = np.dtype([("reserved0", "<i4"), ("reserved1", "<i4")])
STATE_DTYPE = np.dtype([("blocks_seen", "<i8"), ("last_word_end_p1", "<i8"), ("cur", "<u4", (8,)), ("cur_mask", "<u4"), ("cur_next", "<u4"),
                        ("cur_id", "<u4"), ("cur_tow", "<u4"), ("sf", "<u4", (3, 8)), ("sf_tow", "<u4", (3,)), ("have", "<u4"), ("flags", "<u4"),
                        ("n_sets", "<u4"), ("n_subframes", "<u4"), ("reserved", "<u4")])
INTS = ("iode", "iodc", "sva", "svh", "week", "code", "flag")
DOUBLES = ("A", "e", "i0", "OMG0", "omg", "M0", "deln", "OMGd", "idot", "crc", "crs", "cuc", "cus", "cic", "cis", "toes", "fit", "f0", "f1", "f2", "tgd")
EPH_DTYPE = np.dtype([("flags", "<u4")] + [(k, "<i4") for k in INTS] + [(k, "<i8") for k in ("toe_time", "toc_time", "ttr_time")] +
                     [(k, "<f8") for k in ("toe_sec", "toc_sec", "ttr_sec")] + [(k, "<f8") for k in DOUBLES] + [("n_sets", "<u4"), ("have", "<u4")])
WORD_DTYPE = np.dtype([("end_block", "<i4"), ("word", "<u4"), ("index", "u1"), ("flags", "u1"), ("subframe_id", "u1"), ("zero", "u1"),
                       ("aux", "<u4")])
assert CFG_DTYPE.itemsize == 8 and STATE_DTYPE.itemsize == 192 and EPH_DTYPE.itemsize == 256 and WORD_DTYPE.itemsize == 16

# the decoder's constants: IS-GPS-200's pi, the build week that resolves the 10-bit week, the epochs' distance, and RTKLIB's 16-digit
# decimal scale literals (2^-33, 2^-43 and 2^-55 parse to one or two ulps below the power of two)
F64 = np.float64
SC = F64(3.1415926535898)
BUILD_WEEK = 2290
UNIX_TO_GPS = 315964800
SCALE = {4: F64(16.0), -5: F64(0.03125), -19: F64(1.907348632812500E-06), -29: F64(1.862645149230957E-09), -31: F64(4.656612873077393E-10),
         -33: F64(1.164153218269348E-10), -43: F64(1.136868377216160E-13), -55: F64(2.775557561562891E-17)}


def max_words(n_blocks):
    return n_blocks // 600 + 2


# ---- decoding ---------------------------------------------------------------------------------------------------------------------
def take(w8, pos, length):
    """`length` bits from subframe bit pos, first bit most significant, out of words 3 .. 10 (d1 in bit 23): bit n lies in word n // 30"""
    v = 0
    for n in range(pos, pos + length):
        word, bit = divmod(n, 30)
        assert 2 <= word <= 9 and bit < 24
        v = v << 1 | (int(w8[word - 2]) >> (23 - bit)) & 1
    return v


def signed(raw, length):
    return raw - (1 << length) if raw >> (length - 1) else raw


def value(w8, runs, exp, is_signed=True, semicircles=False):
    """a field of one or two runs: the integer, converted; times the scale literal; times pi for semicircles -- one multiply each"""
    raw, length = 0, 0
    for pos, n in runs:
        raw, length = raw << n | take(w8, pos, n), length + n
    v = F64(signed(raw, length) if is_signed else raw)
    if exp:
        v = v * SCALE[exp]
    if semicircles:
        v = v * SC
    return v


def c_int(sec):
    """(int)sec of a double within an int's range"""
    return int(np.trunc(sec))


def gps_time(week, sec):
    sec = F64(sec)
    if sec < F64(-1e9) or F64(1e9) < sec:
        sec = F64(0.0)
    whole = 86400 * 7 * week + c_int(sec)
    assert -(1 << 31) <= whole < 1 << 31
    return UNIX_TO_GPS + whole, sec - F64(c_int(sec))


def decode(sf, tow1):
    """sf: three subframes' eight words (1, 2, 3); tow1: subframe 1's HOW count -> {field: value} of a VALID record"""
    s1, s2, s3 = sf
    o = {}
    week10 = take(s1, 60, 10) + 1024
    o["code"], o["sva"], o["svh"], o["flag"] = take(s1, 70, 2), take(s1, 72, 4), take(s1, 76, 6), take(s1, 90, 1)
    o["tgd"] = value(s1, [(196, 8)], -31)
    o["f2"] = value(s1, [(240, 8)], -55)
    o["f1"] = value(s1, [(248, 16)], -43)
    o["f0"] = value(s1, [(270, 22)], -31)
    o["iodc"] = (take(s1, 82, 2) << 8) + take(s1, 210, 8)
    toc = F64(take(s1, 218, 16)) * F64(16.0)
    q = BUILD_WEEK - week10 + 512
    o["week"] = week10 + (q // 1024 if q >= 0 else -(-q // 1024)) * 1024      # C's division truncates
    o["ttr_time"], o["ttr_sec"] = gps_time(o["week"], F64(tow1) * F64(6.0))
    o["toc_time"], o["toc_sec"] = gps_time(o["week"], toc)
    o["crs"] = value(s2, [(68, 16)], -5)
    o["deln"] = value(s2, [(90, 16)], -43, semicircles=True)
    o["M0"] = value(s2, [(106, 8), (120, 24)], -31, semicircles=True)
    o["cuc"] = value(s2, [(150, 16)], -29)
    o["e"] = value(s2, [(166, 8), (180, 24)], -33, is_signed=False)
    o["cus"] = value(s2, [(210, 16)], -29)
    o["toes"] = value(s2, [(270, 16)], 4, is_signed=False)
    o["fit"] = value(s2, [(286, 1)], 0, is_signed=False)
    sqrt_a = value(s2, [(226, 8), (240, 24)], -19, is_signed=False)
    o["A"] = sqrt_a * sqrt_a
    o["toe_time"], o["toe_sec"] = gps_time(o["week"], o["toes"])
    o["cic"] = value(s3, [(60, 16)], -29)
    o["OMG0"] = value(s3, [(76, 8), (90, 24)], -31, semicircles=True)
    o["cis"] = value(s3, [(120, 16)], -29)
    o["i0"] = value(s3, [(136, 8), (150, 24)], -31, semicircles=True)
    o["crc"] = value(s3, [(180, 16)], -5)
    o["omg"] = value(s3, [(196, 8), (210, 24)], -31, semicircles=True)
    o["OMGd"] = value(s3, [(240, 24)], -43, semicircles=True)
    o["iode"] = take(s3, 270, 8)      # (subframe 3's is the one that stays; a VALID set's subframe 2 has the same)
    o["idot"] = value(s3, [(278, 14)], -43, semicircles=True)
    return o


# ---- assembly ---------------------------------------------------------------------------------------------------------------------
def state_valid(s):
    return (0 <= s["blocks_seen"] <= MAX_COUNT and 0 <= s["last_word_end_p1"] <= MAX_COUNT and s["cur_next"] in (0, 2, 3, 4, 5, 6, 7, 8, 9, 10)
            and s["cur_mask"] <= 0x3FF and s["cur_id"] <= 5 and s["cur_tow"] < TOW_COUNTS and all(t < TOW_COUNTS for t in s["sf_tow"])
            and all(w < 1 << 24 for w in s["cur"]) and all(w < 1 << 24 for k in s["sf"] for w in k) and s["have"] <= 7
            and s["flags"] & ~F_VALID == 0 and (not s["flags"] & F_VALID or s["have"] == 7) and s["reserved"] == 0)


def commit(s):
    """the subframe in cur -> sf[cur_id - 1]; -> NEW or 0"""
    k = s["cur_id"] - 1
    changed = not (s["have"] >> k) & 1 or s["sf"][k] != s["cur"]
    s["sf"][k] = list(s["cur"])
    s["sf_tow"][k] = s["cur_tow"]
    s["have"] |= 1 << k
    sf = s["sf"]
    consistent = s["have"] == 7 and sf[1][0] >> 16 == sf[2][7] >> 16 and sf[1][0] >> 16 == sf[0][5] >> 16
    if not consistent:
        s["flags"] &= ~F_VALID
        return 0
    new = not s["flags"] & F_VALID or changed
    s["flags"] |= F_VALID
    if new:
        s["n_sets"] = (s["n_sets"] + 1) & M32
    return F_NEW if new else 0


def channel(records, s, n_blocks):
    """records: one channel's [(end_block, word, index, flags, subframe_id, aux)] in slot order; s: the state as a dict of Python
    ints and lists, advanced in place -> the launch's NEW"""
    new = 0
    for end_block, word, index, flags, sub_id, aux in records:
        e1 = s["blocks_seen"] + end_block + 1
        if not (flags & WNAV_WORD and 1 <= index <= 10 and -600 <= end_block < n_blocks and e1 >= 1):
            continue
        passed = bool(flags & WNAV_OK) and (index != 2 or (1 <= sub_id <= 5 and aux < TOW_COUNTS))
        if index == 1:
            s["cur_mask"], s["cur_next"], s["cur_id"], s["cur_tow"] = int(passed), 2, 0, 0
        elif index == s["cur_next"] and e1 == s["last_word_end_p1"] + 600:
            if passed:
                s["cur_mask"] |= 1 << (index - 1)
                if index == 2:
                    s["cur_id"], s["cur_tow"] = sub_id, aux
                else:
                    s["cur"][index - 3] = (word >> 6) & 0xFFFFFF
            s["cur_next"] = 0 if index == 10 else index + 1
            if index == 10 and s["cur_mask"] == 0x3FF:
                s["n_subframes"] = (s["n_subframes"] + 1) & M32
                if 1 <= s["cur_id"] <= 3:
                    new |= commit(s)
        else:
            s["cur_next"], s["cur_mask"] = 0, 0
        s["last_word_end_p1"] = e1
    s["blocks_seen"] += n_blocks
    return new


def get_state(states, ch):
    s = {}
    for name in STATE_DTYPE.names:
        v = states[name][ch]
        s[name] = [[int(x) for x in row] for row in v] if v.ndim == 2 else ([int(x) for x in v] if v.ndim == 1 else int(v))
    return s


def record(s, new):
    """the launch's record of a good channel, as an EPH_DTYPE scalar array"""
    o = np.zeros(1, EPH_DTYPE)
    o["flags"], o["n_sets"], o["have"] = s["flags"] | new, s["n_sets"], s["have"]
    if s["flags"] & F_VALID:
        for k, v in decode(s["sf"], s["sf_tow"][0]).items():
            o[k] = v
    return o


def run(words, n_blocks, states):
    """one launch: words WORD_DTYPE [n_blocks // 600 + 2][n_ch]; states a STATE_DTYPE array advanced in place -> (EPH_DTYPE [n_ch],
    the BAD channels, whose states stay and whose records are zero)"""
    assert states.dtype == STATE_DTYPE and 1 <= n_blocks <= 4096 and words.shape == (max_words(n_blocks), len(states))
    out = np.zeros(len(states), EPH_DTYPE)
    bad = []
    for ch in range(len(states)):
        s = get_state(states, ch)
        if not state_valid(s):
            bad.append(ch)
            continue
        col = words[:, ch]
        recs = [(int(r["end_block"]), int(r["word"]), int(r["index"]), int(r["flags"]), int(r["subframe_id"]), int(r["aux"])) for r in col]
        new = channel(recs, s, n_blocks)
        for name in STATE_DTYPE.names:
            states[name][ch] = s[name]
        out[ch] = record(s, new)[0]
    return out, bad
