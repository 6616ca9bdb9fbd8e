"""An exact CPU restatement of the weighted chain's almanac stage (include/gpsx.h gpsx_walm), for the tests: the header's three steps
per word record, its commit table and its bank rules in its order, on Python integers; the decoding on Python integers and floats
(IEEE doubles), one operation at a time in the order the header names; and the two host helpers.  Nothing of the library's code is
included or imported."""
import math

import numpy as np

IONUTC, PAGE25 = 1, 2
HELD, WEEK, HEALTHY, NEW = 1, 2, 4, 8
WNAV_WORD, WNAV_OK, WNAV_SYNC = 1, 2, 8
WEPH_VALID = 1
ENTRIES, PAGE18_ENTRY, PAGE25_ENTRY = 34, 32, 33
MAX_COUNT = 1 << 62
TOW_COUNTS = 100800
TOA_MAX = 147
M32 = 0xFFFFFFFF
SC = 3.1415926535898
BUILD_WEEK = 2290
UNIX_TO_GPS = 315964800

CFG_DTYPE = np.dtype([("ch_per_rx", "<i4"), ("reserved", "<i4", (3,))])
SLOT_DTYPE = np.dtype([("blocks_seen", "<i8"), ("last_word_end_p1", "<i8"), ("cur", "<u4", (8,)), ("cur_mask", "<u4"), ("cur_next", "<u4"),
                       ("cur_id", "<u4"), ("reserved", "<u4")])
BANK_DTYPE = np.dtype([("page", "<u4", (ENTRIES, 8)), ("have_mask", "<u8"), ("n_stored", "<u4"), ("n_changed", "<u4"), ("n_other", "<u4"),
                       ("reserved", "<u4", (3,))])
RX_INTS = ("toa_s", "wna", "tot_s", "wnt", "dt_ls", "wn_lsf", "dn", "dt_lsf")
RX_DTYPE = np.dtype([("flags", "<u4"), ("n_stored", "<u4"), ("have_mask", "<u8"), ("new_mask", "<u8"), ("seen_mask", "<u8"), ("healthy_mask", "<u4"),
                     ("week_mask", "<u4"), ("p25_unhealthy_mask", "<u4")] + [(k, "<i4") for k in RX_INTS] +
                    [("reserved", "<u4"), ("A0", "<f8"), ("A1", "<f8"), ("ion", "<f8", (8,))])
SV_DOUBLES = ("toas", "e", "A", "i0", "OMG0", "omg", "M0", "OMGd", "f0", "f1")
SV_DTYPE = np.dtype([("flags", "<u4"), ("svid", "<i4"), ("svh", "<i4"), ("week", "<i4")] + [(k, "<f8") for k in SV_DOUBLES])
WORD_DTYPE = np.dtype([("end_block", "<i4"), ("word", "<u4"), ("index", "u1"), ("flags", "u1"), ("subframe_id", "u1"), ("zero", "u1"),
                       ("aux", "<u4")])
assert (CFG_DTYPE.itemsize, SLOT_DTYPE.itemsize, BANK_DTYPE.itemsize, RX_DTYPE.itemsize, SV_DTYPE.itemsize, WORD_DTYPE.itemsize) == (16, 64, 1120, 160, 96, 16)


def max_words(n_blocks):
    return n_blocks // 600 + 2


# ---- bits -------------------------------------------------------------------------------------------------------------------------
def u(w8, pos, length):
    """`length` bits from subframe bit pos, first bit most significant, out of words 3 .. 10 (d1 in bit 23): bit n lies in word n // 30"""
    v = 0
    for n in range(pos, pos + length):
        word, bit = divmod(n, 30)
        assert 2 <= word <= 9 and bit < 24
        v = v << 1 | (int(w8[word - 2]) >> (23 - bit)) & 1
    return v


def signed(raw, length):
    return raw - (1 << length) if raw >> (length - 1) else raw


def s(w8, pos, length):
    return signed(u(w8, pos, length), length)


def week8(w):
    return w + (BUILD_WEEK - w + 128) // 256 * 256      # (2290 - w + 128 > 0: floor and C's division agree)


# ---- decoding: the integer converted, one multiply by the power of two, one by pi -------------------------------------------------
def decode_sv(w8):
    o = {"svid": u(w8, 62, 6), "svh": u(w8, 136, 8)}
    o["e"] = float(u(w8, 68, 16)) * 2.0 ** -21
    o["toas"] = float(u(w8, 90, 8) * 4096)
    di = float(s(w8, 98, 16)) * 2.0 ** -19
    semi = 0.3 + di
    o["i0"] = semi * SC
    o["OMGd"] = float(s(w8, 120, 16)) * 2.0 ** -38 * SC
    root_a = float(u(w8, 150, 24)) * 2.0 ** -11
    o["A"] = root_a * root_a
    o["OMG0"] = float(s(w8, 180, 24)) * 2.0 ** -23 * SC
    o["omg"] = float(s(w8, 210, 24)) * 2.0 ** -23 * SC
    o["M0"] = float(s(w8, 240, 24)) * 2.0 ** -23 * SC
    o["f0"] = float(signed(u(w8, 270, 8) << 3 | u(w8, 289, 3), 11)) * 2.0 ** -20
    o["f1"] = float(s(w8, 278, 11)) * 2.0 ** -38
    return o


def decode_page18(w8):
    o = {"ion": [float(s(w8, p, 8)) * 2.0 ** e for p, e in ((68, -30), (76, -27), (90, -24), (98, -24), (106, 11), (120, 14), (128, 16), (136, 16))]}
    o["A1"] = float(s(w8, 150, 24)) * 2.0 ** -50
    o["A0"] = float(signed(u(w8, 180, 24) << 8 | u(w8, 210, 8), 32)) * 2.0 ** -30
    o["tot_s"] = u(w8, 218, 8) * 4096
    o["wnt"] = week8(u(w8, 226, 8))
    o["dt_ls"] = s(w8, 240, 8)
    o["wn_lsf"] = week8(u(w8, 248, 8))
    o["dn"] = u(w8, 256, 8)
    o["dt_lsf"] = s(w8, 270, 8)
    return o


def decode_page25(w8):
    unhealthy = 0
    for n in range(1, 25):
        if u(w8, 90 + 30 * ((n - 1) // 4) + 6 * ((n - 1) % 4), 6) != 0:
            unhealthy |= 1 << (n - 1)
    return {"toa_s": u(w8, 68, 8) * 4096, "wna": week8(u(w8, 76, 8)), "p25_unhealthy_mask": unhealthy}


# ---- assembly and commit ------------------------------------------------------------------------------------------------------------
def slot_valid(t):
    return (0 <= t["blocks_seen"] <= MAX_COUNT and 0 <= t["last_word_end_p1"] <= MAX_COUNT and t["cur_next"] in (0, 2, 3, 4, 5, 6, 7, 8, 9, 10)
            and t["cur_mask"] <= 0x3FF and t["cur_id"] <= 5 and all(w < 1 << 24 for w in t["cur"]) and t["reserved"] == 0)


def bank_valid(b):
    return all(w < 1 << 24 for p in b["page"] for w in p) and b["have_mask"] >> ENTRIES == 0 and all(w == 0 for w in b["reserved"])


def entry_of(cur_id, w8):
    """the bank entry a complete subframe 4 or 5 goes to, or -1"""
    data_id, sv, toa = u(w8, 60, 2), u(w8, 62, 6), u(w8, 90, 8)
    if data_id != 1:
        return -1
    if cur_id == 5 and 1 <= sv <= 24 and toa <= TOA_MAX:
        return sv - 1
    if cur_id == 4 and 25 <= sv <= 32 and toa <= TOA_MAX:
        return sv - 1
    if cur_id == 4 and sv == 56:
        return PAGE18_ENTRY
    if cur_id == 5 and sv == 51:
        return PAGE25_ENTRY
    return -1


def slot(records, t, n_blocks):
    """records: one slot's [(end_block, word, index, flags, subframe_id, aux)] in order; t: its state as Python ints and a list,
    advanced in place -> (cur_id, eight words) of the subframe 4 or 5 that completed, or None"""
    done = None
    for end_block, word, index, flags, sub_id, aux in records:
        e1 = t["blocks_seen"] + end_block + 1
        if not (flags & WNAV_WORD and 1 <= index <= 10 and -600 <= end_block < n_blocks and e1 >= 1):
            continue
        passed = bool(flags & WNAV_OK) and (index != 2 or (1 <= sub_id <= 5 and aux < TOW_COUNTS))
        if index == 1:
            t["cur_mask"], t["cur_next"], t["cur_id"] = int(passed), 2, 0
        elif index == t["cur_next"] and e1 == t["last_word_end_p1"] + 600:
            if passed:
                t["cur_mask"] |= 1 << (index - 1)
                if index == 2:
                    t["cur_id"] = sub_id
                else:
                    t["cur"][index - 3] = (word >> 6) & 0xFFFFFF
            t["cur_next"] = 0 if index == 10 else index + 1
            if index == 10 and t["cur_mask"] == 0x3FF and t["cur_id"] in (4, 5):
                done = (t["cur_id"], list(t["cur"]))
        else:
            t["cur_next"], t["cur_mask"] = 0, 0
        t["last_word_end_p1"] = e1
    t["blocks_seen"] += n_blocks
    return done


def get(arr, i):
    """record i of a structured array as Python ints and nested lists"""
    return {name: arr[name][i].tolist() for name in arr.dtype.names}


def put(arr, i, d):
    for name in arr.dtype.names:
        arr[name][i] = d[name]


def run(words, n_blocks, ch_per_rx, slots, banks):
    """one launch: words WORD_DTYPE [n_blocks // 600 + 2][n_rx * ch_per_rx]; slots SLOT_DTYPE [n_rx * ch_per_rx] and banks BANK_DTYPE
    [n_rx], advanced in place -> (RX_DTYPE [n_rx], SV_DTYPE [n_rx][32], the BAD channels, the receivers with a BAD bank)"""
    n_rx = len(banks)
    assert slots.dtype == SLOT_DTYPE and banks.dtype == BANK_DTYPE and 1 <= n_blocks <= 4096 and 1 <= ch_per_rx <= 64
    assert len(slots) == n_rx * ch_per_rx and words.shape == (max_words(n_blocks), n_rx * ch_per_rx)
    rx, alm = np.zeros(n_rx, RX_DTYPE), np.zeros((n_rx, 32), SV_DTYPE)
    bad_slots, bad_banks = [], []
    for r in range(n_rx):
        b = get(banks, r)
        if not bank_valid(b):
            bad_banks.append(r)
            continue
        before_have, before_page = b["have_mask"], [list(p) for p in b["page"]]
        seen, n_stored = 0, 0
        for j in range(ch_per_rx):
            ch = r * ch_per_rx + j
            t = get(slots, ch)
            if not slot_valid(t):
                bad_slots.append(ch)
                continue
            col = words[:, ch]
            done = slot([(int(q["end_block"]), int(q["word"]), int(q["index"]), int(q["flags"]), int(q["subframe_id"]), int(q["aux"])) for q in col],
                        t, n_blocks)
            put(slots, ch, t)
            if done is None:
                continue
            e = entry_of(*done)
            if e < 0:
                b["n_other"] = (b["n_other"] + 1) & M32
                continue
            b["page"][e] = done[1]
            b["have_mask"] |= 1 << e
            b["n_stored"] = (b["n_stored"] + 1) & M32
            seen |= 1 << e
            n_stored += 1
        new = 0
        for e in range(ENTRIES):
            if seen >> e & 1 and (not before_have >> e & 1 or b["page"][e] != before_page[e]):
                new |= 1 << e
        b["n_changed"] = (b["n_changed"] + bin(new).count("1")) & M32
        put(banks, r, b)
        o = rx[r:r + 1]
        have = b["have_mask"]
        o["n_stored"], o["have_mask"], o["new_mask"], o["seen_mask"] = n_stored, have, new, seen
        has18, has25 = have >> PAGE18_ENTRY & 1, have >> PAGE25_ENTRY & 1
        o["flags"] = (IONUTC if has18 else 0) | (PAGE25 if has25 else 0)
        p25 = decode_page25(b["page"][PAGE25_ENTRY]) if has25 else None
        if has25:
            for k, v in p25.items():
                o[k] = v
        if has18:
            for k, v in decode_page18(b["page"][PAGE18_ENTRY]).items():
                o[k] = v
        healthy_mask = week_mask = 0
        for sv in range(32):
            if not have >> sv & 1:
                continue
            d = decode_sv(b["page"][sv])
            flags = HELD | (NEW if new >> sv & 1 else 0)
            if d["svh"] == 0:
                flags |= HEALTHY
                healthy_mask |= 1 << sv
            week = 0
            if has25 and p25["toa_s"] == int(d["toas"]):
                flags |= WEEK
                week_mask |= 1 << sv
                week = p25["wna"]
            a = alm[r, sv:sv + 1]
            a["flags"], a["week"] = flags, week
            for k, v in d.items():
                a[k] = v
        o["healthy_mask"], o["week_mask"] = healthy_mask, week_mask
    return rx, alm, bad_slots, bad_banks


# ---- the host helpers ---------------------------------------------------------------------------------------------------------------
def gps_time(week, sec):
    if sec < -1e9 or 1e9 < sec:
        sec = 0.0
    return UNIX_TO_GPS + 86400 * 7 * week + int(math.trunc(sec)), sec - float(int(math.trunc(sec)))


def to_eph(sv, eph_dtype):
    """gpsx_walm_to_eph: one SV_DTYPE record -> a VALID record of eph_dtype (the ephemeris stage's), or None where it refuses"""
    if int(sv["flags"]) & (HELD | WEEK) != HELD | WEEK:
        return None
    o = np.zeros(1, eph_dtype)
    o["flags"] = WEPH_VALID
    for k in ("svh", "week", "A", "e", "i0", "OMG0", "omg", "M0", "OMGd", "f0", "f1"):
        o[k] = sv[k]
    o["toes"] = sv["toas"]
    t, sec = gps_time(int(sv["week"]), float(sv["toas"]))
    o["toe_time"], o["toe_sec"], o["toc_time"], o["toc_sec"] = t, sec, t, sec
    return o


def gps_minus_utc(rx, week, tow_s):
    """gpsx_walm_gps_minus_utc on one RX_DTYPE record, or None where it refuses"""
    if not int(rx["flags"]) & IONUTC or not 1 <= int(rx["dn"]) <= 7 or not math.isfinite(tow_s):
        return None
    now = float(week) * 604800.0 + tow_s
    then = float(int(rx["wn_lsf"])) * 604800.0 + float(int(rx["dn"])) * 86400.0
    ls = int(rx["dt_lsf"]) if now >= then else int(rx["dt_ls"])
    since = (tow_s - float(int(rx["tot_s"]))) + 604800.0 * (float(week) - float(int(rx["wnt"])))
    return (float(ls) + float(rx["A0"])) + float(rx["A1"]) * since
