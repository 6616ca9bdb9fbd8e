"""An exact CPU restatement of the weighted path's LNAV word layer (include/gpsx.h gpsx_wnav_words), for the tests: the header's
four steps per bit record, in its order, on Python integers.  The parity equations are written out from IS-GPS-200 table 20-XIV.
Nothing of the library's code is included or imported."""
import numpy as np

HUNT, SYNCED = 0, 1
F_WORD, F_OK, F_INVERTED, F_SYNC, F_FLIPPED, F_SUBFRAME, F_DROPPED = 1, 2, 4, 8, 16, 32, 64
WSYNC_WINDOW, WSYNC_BIT = 1, 4

STATE_DTYPE = np.dtype([("hist", "<u8"), ("blocks_seen", "<i8"), ("last_bit_end_p1", "<i8"), ("fresh", "<i4"), ("mode", "<i4"), ("inv", "<i4"),
                        ("word_idx", "<i4"), ("bit_idx", "<i4"), ("bad_run", "<i4"), ("ok_mask", "<u4"), ("n_sync", "<u4"), ("n_drop", "<u4"),
                        ("n_subframes", "<u4")])
WORD_DTYPE = np.dtype([("end_block", "<i4"), ("word", "<u4"), ("index", "u1"), ("flags", "u1"), ("subframe_id", "u1"), ("zero", "u1"),
                       ("aux", "<u4")])
assert STATE_DTYPE.itemsize == 64 and WORD_DTYPE.itemsize == 16

# table 20-XIV: D25 .. D30 = the previous word's D29* or D30*, XORed with these source bits d1 .. d24
_TAPS = ((29, (1, 2, 3, 5, 6, 10, 11, 12, 13, 14, 17, 18, 20, 23)), (30, (2, 3, 4, 6, 7, 11, 12, 13, 14, 15, 18, 19, 21, 24)),
         (29, (1, 3, 4, 5, 7, 8, 12, 13, 14, 15, 16, 19, 20, 22)), (30, (2, 4, 5, 6, 8, 9, 13, 14, 15, 16, 17, 20, 21, 23)),
         (30, (1, 3, 5, 6, 7, 9, 10, 14, 15, 16, 17, 18, 21, 22, 24)), (29, (3, 5, 6, 8, 9, 10, 11, 13, 15, 19, 22, 23, 24)))
_MASKS = tuple((start, sum(1 << (24 - t) for t in taps)) for start, taps in _TAPS)      # d1 in bit 23
M30, M62, M64 = (1 << 30) - 1, (1 << 62) - 1, (1 << 64) - 1
MAX_COUNT = 1 << 62


def max_words(n_blocks):
    return n_blocks // 600 + 2


def source_bits(w, p30):
    return ((w >> 6) ^ (0xFFFFFF if p30 else 0)) & 0xFFFFFF


def parity_ok(w, p29, p30):
    d = source_bits(w, p30)
    for k, (start, mask) in enumerate(_MASKS):
        if (bin(d & mask).count("1") & 1) ^ (p29 if start == 29 else p30) != (w >> (5 - k)) & 1:
            return False
    return True


def how_ok(x, p30):
    """x: word 2 with the polarity removed; p30: the bit before it, likewise -> its ID if the HOW conditions hold, else 0"""
    sub_id = (source_bits(x, p30) >> 2) & 7
    return sub_id if (x & 3) == 0 and 1 <= sub_id <= 5 else 0


def out_word(w, p30, inv):
    x = (w ^ (M30 if inv else 0)) & M30
    return source_bits(w, p30) << 6 | (x & 63)


def hunt_test(hist):
    """the header's step 3 on the newest 62 bits -> (inv', ID) or None"""
    for inv in (0, 1):
        x = (hist ^ (M64 if inv else 0)) & M62
        w1, w2 = (x >> 30) & M30, x & M30
        if w1 >> 22 != 0x8B or not parity_ok(w1, (x >> 61) & 1, (x >> 60) & 1) or not parity_ok(w2, (w1 >> 1) & 1, w1 & 1):
            continue
        sub_id = how_ok(w2, w1 & 1)
        if sub_id:
            return inv, sub_id
    return None


def state_valid(s):
    return (0 <= s["mode"] <= 1 and 0 <= s["inv"] <= 1 and 0 <= s["word_idx"] <= 9 and 0 <= s["bit_idx"] <= 29 and 0 <= s["fresh"] <= 62
            and 0 <= s["bad_run"] <= 10 and 0 <= s["blocks_seen"] <= MAX_COUNT and 0 <= s["last_bit_end_p1"] <= MAX_COUNT)


def channel(bits, s, n_blocks, max_bad_words, events=None):
    """bits: [(end_block, bit_ip)] of one launch in slot order, already filtered; s: the state as a dict of Python ints, advanced in
    place -> the word records [(end_block, word, index, flags, subframe_id, aux)]"""
    out = []
    for end_block, bit_ip in bits:
        e_p1 = s["blocks_seen"] + end_block + 1
        # 1: continuity
        if s["last_bit_end_p1"] != 0 and e_p1 != s["last_bit_end_p1"] + 20:
            if s["mode"] == SYNCED:
                s["n_drop"] = (s["n_drop"] + 1) & 0xFFFFFFFF
            s["mode"] = HUNT
            s["fresh"] = s["word_idx"] = s["bit_idx"] = s["bad_run"] = s["ok_mask"] = 0
        s["last_bit_end_p1"] = e_p1
        # 2: shift
        s["hist"] = (s["hist"] << 1 | (1 if bit_ip < 0 else 0)) & M64
        s["fresh"] = min(s["fresh"] + 1, 62)
        hist = s["hist"]
        if s["mode"] == HUNT:
            # 3: TLM + HOW as a whole
            got = hunt_test(hist) if s["fresh"] == 62 else None
            if got:
                inv, sub_id = got
                s.update(inv=inv, mode=SYNCED, word_idx=2, bit_idx=0, bad_run=0, ok_mask=3 | sub_id << 16, n_sync=(s["n_sync"] + 1) & 0xFFFFFFFF)
                flags = F_WORD | F_OK | F_SYNC | (F_INVERTED if inv else 0)
                w1, w2 = (hist >> 30) & M30, hist & M30
                out.append((end_block - 600, out_word(w1, (hist >> 60) & 1, inv), 1, flags, sub_id, 0))
                out.append((end_block, out_word(w2, w1 & 1, inv), 2, flags, sub_id, (source_bits(w2, w1 & 1) >> 7) & 0x1FFFF))
                if events is not None:
                    events.append(("sync", end_block, inv, sub_id))
            continue
        # 4: SYNCED
        s["bit_idx"] += 1
        if s["bit_idx"] < 30:
            continue
        w, p29, p30 = hist & M30, (hist >> 31) & 1, (hist >> 30) & 1
        index = s["word_idx"] + 1
        passed = parity_ok(w, p29, p30)
        flags = F_WORD
        if index == 1:
            t = ((w ^ (M30 if s["inv"] else 0)) & M30) >> 22
            if t == 0x74 and passed:
                s["inv"] ^= 1
                flags |= F_FLIPPED
            elif t != 0x8B:
                passed = False
        inv = s["inv"]
        aux = 0
        if index == 2:
            sub_id = how_ok((w ^ (M30 if inv else 0)) & M30, p30 ^ inv) if passed else 0
            passed = sub_id != 0
            s["ok_mask"] = (s["ok_mask"] & 0x3FF) | sub_id << 16
            if passed:
                aux = (source_bits(w, p30) >> 7) & 0x1FFFF
        if passed:
            flags |= F_OK
            s["ok_mask"] |= 1 << (index - 1)
        if inv:
            flags |= F_INVERTED
        sub_id = (s["ok_mask"] >> 16) & 7
        s["bad_run"] = 0 if passed else min(s["bad_run"] + 1, 10)
        s["bit_idx"] = 0
        s["word_idx"] = (s["word_idx"] + 1) % 10
        if index == 10:
            if s["ok_mask"] & 0x3FF == 0x3FF:
                flags |= F_SUBFRAME
                s["n_subframes"] = (s["n_subframes"] + 1) & 0xFFFFFFFF
            s["ok_mask"] = 0
        if s["bad_run"] >= max_bad_words:
            flags |= F_DROPPED
            s["n_drop"] = (s["n_drop"] + 1) & 0xFFFFFFFF
            s["mode"], s["fresh"], s["word_idx"] = HUNT, 0, 0
        out.append((end_block, out_word(w, p30, inv), index, flags, sub_id, aux))
    s["blocks_seen"] += n_blocks
    return out


def empty_words(n_slots, n_ch):
    words = np.zeros((n_slots, n_ch), WORD_DTYPE)
    words["end_block"] = -1
    return words


def bit_records(rec_col, n_blocks):
    """one channel's column of a WSYNC record array (fields end_block, flags, bit_ip) -> [(end_block, bit_ip)] of its BIT records"""
    is_bit = ((rec_col["flags"] & (WSYNC_WINDOW | WSYNC_BIT)) == (WSYNC_WINDOW | WSYNC_BIT)) & (rec_col["end_block"] >= 0) & (rec_col["end_block"] < n_blocks)
    at = np.nonzero(is_bit)[0]
    return list(zip(rec_col["end_block"][at].tolist(), rec_col["bit_ip"][at].tolist()))


def run(rec, n_blocks, states, max_bad_words, channels=None, events=None):
    """one launch: rec [n_slots][n_ch] (any structured array with end_block, flags, bit_ip), states a STATE_DTYPE array advanced
    in place -> (WORD_DTYPE [n_blocks // 600 + 2][n_ch], the BAD channels).  events: {channel: [...]}"""
    assert states.dtype == STATE_DTYPE and 1 <= n_blocks <= 4096 and 1 <= rec.shape[0] <= n_blocks and 1 <= max_bad_words <= 10
    words = empty_words(max_words(n_blocks), len(states))
    bad = []
    for ch in (range(len(states)) if channels is None else channels):
        s = {name: int(states[name][ch]) for name in STATE_DTYPE.names}
        if not state_valid(s):
            bad.append(ch)
            continue
        ev = None if events is None else events.setdefault(ch, [])
        out = channel(bit_records(rec[:, ch], n_blocks), s, n_blocks, max_bad_words, ev)
        assert len(out) <= words.shape[0], (ch, len(out))
        for k, (end_block, word, index, flags, sub_id, aux) in enumerate(out):
            words[k, ch] = (end_block, word, index, flags, sub_id, 0, aux)
        for name in STATE_DTYPE.names:
            states[name][ch] = s[name]
    return words, bad


def subframe_image(ten):
    """ten records (index 1 .. 10, all OK) -> the 38-byte image: subframe bit 30 w + i = bit 29 - i of word w"""
    assert [int(r["index"]) for r in ten] == list(range(1, 11)) and all(int(r["flags"]) & F_OK for r in ten)
    bits = np.zeros(304, np.uint8)
    for w, r in enumerate(ten):
        for i in range(30):
            bits[30 * w + i] = (int(r["word"]) >> (29 - i)) & 1
    return np.packbits(bits, bitorder="little")
