"""The weighted path's LNAV word layer (include/gpsx.h gpsx_wnav_words), without a GPU: the layout of its structs as a C compiler
sees them, the exported entry points and the binding, and the exact CPU restatement its GPU tests compare against
(tests/weighted_nav_ref.py) on synthesised LNAV: where it synchronises, what a half-cycle slip, bit errors, a gap and plain noise
do to it, the subframe image and the existing decoder, and the whole weighted chain on the restatements -- IF samples, the loop with
bit sync, words.

Measured on the restatements (PRN 7 / 19 / 30 at amplitude 0.035 carrying LNAV 250 bits into subframe 1, the middle satellite
inverted, 3500 ms, seeds 1, 2, 3): every channel reads 132 or 133 bits after lock without an error, synchronises at the satellite's
bit 109 (word 2 ends at block 2199 / 2210 / 2205) with subframe ID 2 and passes words 3 and 4.  On 3 000 000 random bits the TLM + HOW
test accepts once (expected 3e6 * 2^-21 * 5/8 = 0.89)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import steps_driver as sd
import weighted_nav_cases as W
import weighted_nav_ref as N
import weighted_sync_cases as K
import weighted_sync_ref as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"gpsx_wnav_words", "gpsx_wnav_words_dev", "gpsx_wnav_subframe_image"}

LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "gpsx.h"
typedef int (*dev_fn)(gpsx_ctx *, const gpsx_wnav_cfg_t *, const gpsx_wsync_rec_t *, int, int, gpsx_wnav_state_t *, int, gpsx_wnav_word_t *);
typedef int (*img_fn)(const gpsx_wnav_word_t *, uint8_t *);
_Static_assert(__builtin_types_compatible_p(__typeof__(&gpsx_wnav_words_dev), dev_fn), "the _dev entry point");
_Static_assert(__builtin_types_compatible_p(__typeof__(&gpsx_wnav_words), dev_fn), "the host entry point");
_Static_assert(__builtin_types_compatible_p(__typeof__(&gpsx_wnav_subframe_image), img_fn), "the image helper");
#define S(f) printf("state.%s %zu\n", #f, offsetof(gpsx_wnav_state_t, f))
#define R(f) printf("word.%s %zu\n", #f, offsetof(gpsx_wnav_word_t, f))
#define G(f) printf("cfg.%s %zu\n", #f, offsetof(gpsx_wnav_cfg_t, f))
int main(void)
{
  printf("sizeof.state %zu\nsizeof.word %zu\nsizeof.cfg %zu\n", sizeof(gpsx_wnav_state_t), sizeof(gpsx_wnav_word_t), sizeof(gpsx_wnav_cfg_t));
  S(hist); S(blocks_seen); S(last_bit_end_p1); S(fresh); S(mode); S(inv); S(word_idx); S(bit_idx); S(bad_run); S(ok_mask); S(n_sync); S(n_drop);
  S(n_subframes);
  R(end_block); R(word); R(index); R(flags); R(subframe_id); R(zero); R(aux);
  G(max_bad_words); G(reserved);
  printf("flag.all %u\nmode.synced %d\nversion %d\n", GPSX_WNAV_WORD | GPSX_WNAV_OK | GPSX_WNAV_INVERTED | GPSX_WNAV_SYNC | GPSX_WNAV_FLIPPED |
         GPSX_WNAV_SUBFRAME | GPSX_WNAV_DROPPED, GPSX_WNAV_SYNCED - GPSX_WNAV_HUNT, GPSX_VERSION);
  return 0;
}
"""


def test_struct_layout_as_a_c_compiler_sees_it():
    with tempfile.TemporaryDirectory(prefix="wnav_layout_") as tmp:
        src, exe = os.path.join(tmp, "layout.c"), os.path.join(tmp, "layout")
        with open(src, "w") as f:
            f.write(LAYOUT_C)
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
        got = {k: int(v) for k, v in (line.split() for line in subprocess.check_output([exe], text=True).splitlines())}
    assert got["sizeof.state"] == 64 and got["sizeof.word"] == 16 and got["sizeof.cfg"] == 8
    assert got["flag.all"] == 127 and got["mode.synced"] == 1 and got["version"] == 110
    state = {k[6:]: v for k, v in got.items() if k.startswith("state.")}
    word = {k[5:]: v for k, v in got.items() if k.startswith("word.")}
    assert state == {"hist": 0, "blocks_seen": 8, "last_bit_end_p1": 16, "fresh": 24, "mode": 28, "inv": 32, "word_idx": 36, "bit_idx": 40,
                     "bad_run": 44, "ok_mask": 48, "n_sync": 52, "n_drop": 56, "n_subframes": 60}
    assert word == {"end_block": 0, "word": 4, "index": 8, "flags": 9, "subframe_id": 10, "zero": 11, "aux": 12}
    assert {k[4:]: v for k, v in got.items() if k.startswith("cfg.")} == {"max_bad_words": 0, "reserved": 4}
    for name, off in state.items():      # the restatement's and the binding's dtypes are that layout
        assert N.STATE_DTYPE.fields[name][1] == off, name
    for name, off in word.items():
        assert N.WORD_DTYPE.fields[name][1] == off, name
    from stm32f4_sdr_gps_amd import capi
    assert capi.WNAV_STATE_DTYPE == N.STATE_DTYPE and capi.WNAV_WORD_DTYPE == N.WORD_DTYPE and capi.WNAV_CFG_DTYPE.itemsize == 8
    assert (capi.WNAV_FLAG_WORD, capi.WNAV_FLAG_OK, capi.WNAV_FLAG_INVERTED, capi.WNAV_FLAG_SYNC, capi.WNAV_FLAG_FLIPPED, capi.WNAV_FLAG_SUBFRAME,
            capi.WNAV_FLAG_DROPPED) == (N.F_WORD, N.F_OK, N.F_INVERTED, N.F_SYNC, N.F_FLIPPED, N.F_SUBFRAME, N.F_DROPPED)


def test_library_exports_the_word_layer(lib_path):
    syms = subprocess.check_output(["nm", "-D", "--defined-only", lib_path], text=True)
    assert SYMBOLS <= {line.split()[-1] for line in syms.splitlines() if line.strip()}
    from stm32f4_sdr_gps_amd import capi
    import __graft_entry__ as entry
    assert SYMBOLS <= set(entry.ABI_SYMBOLS)
    assert callable(getattr(capi.Engine, "wnav_words", None)) and callable(capi.subframe_image)
    lib = capi.load_library()
    assert lib.gpsx_wnav_words_dev.argtypes is not None and lib.gpsx_version() == 110
    assert capi.wnav_word_slots(1) == 2 and capi.wnav_word_slots(599) == 2 and capi.wnav_word_slots(600) == 3 and capi.wnav_word_slots(4096) == 8


def test_word_kernel_has_no_scratch_and_no_lds(lib_path):
    from stm32f4_sdr_gps_amd import build
    hits = [v for k, v in build.check_no_scratch().items() if "k_wnav_words" in k]
    assert len(hits) == 1 and hits[0]["scratch_bytes"] == 0 and hits[0]["lds_bytes"] == 0, hits
    assert hits[0]["vgprs"] <= 128      # two sets of eight slots' three words, the frame state: four waves per SIMD


# ---- the rule on synthesised LNAV ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first,flip,seed,sync_bit,sub_id,later", [(37, 0, 1, 322, 2, 22), (161, 1, 2, 198, 2, 26), (299, 0, 3, 360, 3, 21),
                                                                    (0, 1, 4, 359, 2, 21), (239, 0, 5, 120, 2, 29)])
def test_sync_on_lnav(first, flip, seed, sync_bit, sub_id, later):
    """one sync, where TLM + HOW of the first subframe that has two bits before it end; first = 0 waits a whole subframe"""
    from stm32f4_sdr_gps_amd import synth
    events = []
    out, s = W.feed(synth.lnav_bits(1000, first, seed) ^ flip, events=events)
    assert events == [("sync", 20 * sync_bit + 19, flip, sub_id)] and s["inv"] == flip and s["n_sync"] == 1 and s["n_drop"] == 0
    assert len(out) == 2 + later and all(r[3] & N.F_OK for r in out) and not any(r[3] & (N.F_DROPPED | N.F_FLIPPED) for r in out)
    assert [r[2] for r in out] == [(k % 10) + 1 for k in range(len(out))]
    assert [r[0] for r in out] == [20 * (sync_bit - 30 + 30 * k) + 19 for k in range(len(out))]
    # the words' source bits are what lnav_subframe was given
    subs = W.source_words(8, seed)
    k0 = (sync_bit - 59 + first) // 300      # the subframe the sync fell into, counted from the stream's subframe 1
    for k, r in enumerate(out):
        sub, tow, words = subs[k0 + k // 10]
        assert W.word_matches(r[1], words[r[2] - 1]), (k, r)
        assert r[4] == (0 if r[2] == 1 and k else sub) and r[5] == (tow if r[2] == 2 else 0), (k, r)      # (a TLM's HOW is yet to come)
    assert out[0][4] == sub_id and (out[0][3] & N.F_INVERTED != 0) == bool(flip)
    tens = [r for r in out if r[2] == 10]
    assert tens and all(r[3] & N.F_SUBFRAME for r in tens) and s["n_subframes"] == len(tens)


def test_a_half_cycle_slip():
    from stm32f4_sdr_gps_amd import synth
    bits = synth.lnav_bits(1500, 100, 9)
    bits[700:] ^= 1
    events = []
    out, s = W.feed(bits, 3, events=events)
    assert events == [("sync", 20 * 259 + 19, 0, 2)] and s["n_drop"] == 0 and s["n_sync"] == 1 and s["inv"] == 1
    failed = [r for r in out if not r[3] & N.F_OK]
    assert [(r[2], r[0]) for r in failed] == [(7, 20 * 709 + 19)]
    flipped = [r for r in out if r[3] & N.F_FLIPPED]
    assert [(r[2], r[0]) for r in flipped] == [(1, 20 * 829 + 19)]          # the next TLM
    tens = {r[0] // 20: bool(r[3] & N.F_SUBFRAME) for r in out if r[2] == 10}
    assert tens == {499: True, 799: False, 1099: True, 1399: True}          # the slipped subframe is not one, the next is
    # the source bits d = D ^ D30* do not see the polarity: every word that passes carries them, also between the slip and the next
    # TLM; what is the old polarity's there is the record's six parity bits (and its _INVERTED flag)
    subs = W.source_words(6, 9)
    sent = synth.lnav_bits(1500, 100, 9)
    for r in out:
        last = r[0] // 20
        sub_no, word_no = divmod((last + 100 - 29) // 30, 10)
        assert W.word_matches(r[1], subs[sub_no][2][word_no]) == (r[3] & N.F_OK != 0), r
        parity = int("".join(str(b) for b in sent[last - 5:last + 1]), 2)
        if r[3] & N.F_OK:
            assert r[1] & 63 == (parity ^ 63 if 709 < last < 829 else parity), r
            assert bool(r[3] & N.F_INVERTED) == (last >= 829), r


def test_noise_rarely_synchronises():
    """3 000 000 random bits as one channel's: the HUNT rule alone, on every window that begins with either preamble"""
    bits = np.random.default_rng(1).integers(0, 2, 3_000_000).astype(np.uint8)
    windows = np.lib.stride_tricks.sliding_window_view(bits, 8)
    pre = np.array([1, 0, 0, 0, 1, 0, 1, 1], np.uint8)
    starts = np.nonzero((windows == pre).all(axis=1) | (windows == 1 - pre).all(axis=1))[0]      # word 1's first bit
    weights = 1 << np.arange(61, -1, -1, dtype=np.uint64)
    accepted = 0
    for p in starts:
        if p >= 2 and p + 60 <= len(bits):
            hist = int((bits[p - 2:p + 60].astype(np.uint64) * weights).sum())
            accepted += N.hunt_test(hist) is not None
    print("candidates", len(starts), "accepted", accepted)
    assert len(starts) > 20000 and accepted <= 6


def test_bit_errors():
    from stm32f4_sdr_gps_amd import synth
    clean = synth.lnav_bits(1500, 239, 5)          # sync at bit 120: word 3 begins at bit 121
    one = clean.copy()
    one[121 + 2 * 30 + 7] ^= 1                     # word 5
    out, s = W.feed(one)
    assert [(r[2], r[0] // 20) for r in out if not r[3] & N.F_OK] == [(5, 121 + 3 * 30 - 1)] and s["n_drop"] == 0 and s["bad_run"] == 0
    three = clean.copy()
    three[[121 + 30 + 3, 121 + 60 + 3, 121 + 90 + 3]] ^= 1      # words 4, 5, 6
    events = []
    out, s = W.feed(three, 3, events=events)
    bad = [r for r in out if not r[3] & N.F_OK]
    assert [r[2] for r in bad] == [4, 5, 6] and [bool(r[3] & N.F_DROPPED) for r in bad] == [False, False, True]
    assert s["n_drop"] == 1 and s["n_sync"] == 2 and [e[1] // 20 for e in events] == [120, 420]      # again at the next TLM + HOW
    after = [r for r in out if r[0] // 20 >= 390]
    assert after[0][2] == 1 and after[0][3] & N.F_SYNC and all(r[3] & N.F_OK for r in after)
    # with max_bad_words = 4 the same stream is never dropped
    out, s = W.feed(three, 4)
    assert s["n_drop"] == 0 and s["n_sync"] == 1 and len([r for r in out if not r[3] & N.F_OK]) == 3


def test_discontinuity():
    from stm32f4_sdr_gps_amd import synth
    bits = synth.lnav_bits(600, 239, 5)
    ends = 19 + 20 * np.arange(600, dtype=np.int64)
    ends[300:] += 40                               # a gap of 40 blocks in SYNCED
    s = {name: 0 for name in N.STATE_DTYPE.names}
    events = []
    out = N.channel([(int(e), -1 if b else 1) for e, b in zip(ends[:305], bits[:305])], s, int(ends[304]) + 1, 3, events)
    assert s["mode"] == N.HUNT and s["n_drop"] == 1 and s["fresh"] == 5 and s["bit_idx"] == 0 and s["word_idx"] == 0 and s["ok_mask"] == 0
    assert len(events) == 1 and all(r[0] < ends[300] for r in out)
    # bits 1 block apart (BIT in every slot at span 1): never 62 fresh bits, never a word
    rec = Y.empty_records(1237, 1)
    rec["end_block"][:, 0] = np.arange(1237)
    rec["flags"] = W.F_BITREC
    rec["bit_ip"][:, 0] = 1 - 2 * synth.lnav_bits(1237, 239, 5).astype(np.int32)
    st = np.zeros(1, N.STATE_DTYPE)
    words, bad = N.run(rec, 1237, st, 3)
    assert not bad and words.tobytes() == N.empty_words(4, 1).tobytes() and int(st["fresh"][0]) == 1 and int(st["n_sync"][0]) == 0
    assert int(st["blocks_seen"][0]) == 1237 and int(st["last_bit_end_p1"][0]) == 1237


def test_the_case_table_stands_on_every_ground():
    """what the table the GPU runs meets, from the restatement: every flag, failed words, channels that start mid-word in SYNCED,
    a channel in HUNT with fresh = 61 that synchronises on its first bit (word 1 ends before the launch), a launch without a bit"""
    seen, starts = 0, set()
    for i in range(len(W.CASES)):
        rec, n_blocks, st0, _, words, after = W.case(i)
        filled = words["flags"] != 0
        seen |= int(np.bitwise_or.reduce(words["flags"][filled])) if filled.any() else 0
        if ((words["flags"] & N.F_WORD != 0) & (words["flags"] & N.F_OK == 0)).any():
            starts.add("failed word")
        if ((st0["mode"] == N.SYNCED) & (st0["bit_idx"] > 0)).any():
            starts.add("mid-word")
        hunt61 = (st0["mode"] == N.HUNT) & (st0["fresh"] == 61)
        if (hunt61 & (words["flags"][0] & N.F_SYNC != 0) & (words["end_block"][0] < 0)).any():
            starts.add("fresh 61")
        if not filled.any() and after["hist"].tobytes() == st0["hist"].tobytes():
            starts.add("no bit")
        if (after["n_drop"] > st0["n_drop"]).any():
            starts.add("drop")
    assert seen == 127 and starts == {"failed word", "mid-word", "fresh 61", "no bit", "drop"}, (seen, starts)


# ---- the subframe image and the existing decoder ------------------------------------------------------------------------------------------
def _records(out):
    rec = np.zeros(len(out), N.WORD_DTYPE)
    for k, (end_block, word, index, flags, sub_id, aux) in enumerate(out):
        rec[k] = (end_block, word, index, flags, sub_id, 0, aux)
    return rec


def test_subframe_image_and_the_decoder(lib_path):
    from stm32f4_sdr_gps_amd import capi, synth
    bits = np.concatenate([np.zeros(2, np.uint8), synth.lnav_bits(998, 0, 6)]) ^ 1      # subframes 1, 2, 3 begin at bits 2, 302, 602; received inverted
    out, s = W.feed(bits)
    rec = _records(out)
    assert s["inv"] == 1 and len(rec) >= 30 and (rec["flags"][:30] & N.F_OK).all()
    images = []
    for k in range(3):
        ten = rec[10 * k:10 * k + 10]
        assert ten["flags"][9] & N.F_SUBFRAME and (ten["subframe_id"][1:] == k + 1).all() and ten["subframe_id"][0] == (1 if k == 0 else 0)
        image = capi.subframe_image(ten)
        assert image.tobytes() == N.subframe_image(ten).tobytes() and image.shape == (38,)
        images.append(image)
        # the image's bits: source bits + transmitted parity, word by word
        sub, _, words = W.source_words(3, 6)[k]
        sent = (bits[2 + 300 * k:302 + 300 * k] ^ 1).astype(np.uint8)
        got = np.unpackbits(image, bitorder="little")[:300]
        for w in range(10):
            assert np.array_equal(got[30 * w + 24:30 * w + 30], sent[30 * w + 24:30 * w + 30]), (k, w)
            assert all(b is None or b == g for b, g in zip(words[w], got[30 * w:30 * w + 24])), (k, w)
        assert not np.unpackbits(image, bitorder="little")[300:].any()
    ids, snaps = sd.run_ephemeris(C.CDLL(lib_path), np.stack(images))
    assert ids.tolist() == [1, 2, 3] and snaps[2].any()
    # refusals: a record without _OK, indices out of order, nine records
    ten = rec[:10].copy()
    ten["flags"][4] &= ~np.uint8(N.F_OK)
    with pytest.raises(capi.GpsxError):
        capi.subframe_image(ten)
    with pytest.raises(capi.GpsxError):
        capi.subframe_image(rec[1:11])
    with pytest.raises(capi.GpsxError):
        capi.subframe_image(rec[:9])
    lib = capi.load_library()
    assert lib.gpsx_wnav_subframe_image(None, np.zeros(38, np.uint8).ctypes.data) == -22 and lib.gpsx_wnav_subframe_image(rec[:10].ctypes.data, None) == -22


# ---- the whole weighted chain on the restatements -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", K.SEEDS)
def test_if_samples_to_words_on_the_restatements(oracle, seed):
    blocks, truth = W.e2e_scenario(seed)
    st = K.handover_states(seed)
    nav = np.zeros(3, N.STATE_DTYPE)
    rec_list, word_list, at = [], [], 0
    for n in (1000, 1000, 1500):
        rec = Y.run(oracle, blocks[at:at + n], st, K.sync_cfg())
        words, bad = N.run(rec, n, nav, 3)
        assert not bad and words.shape == (n // 600 + 2, 3)
        rec_list.append((at, rec))
        word_list.append((at, words))
        at += n
    words_abs = W.absolute_words(word_list)
    for ch in range(3):
        edge = K.EDGES_FOUND[ch]
        assert int(st["mode"][ch]) == Y.LOCKED and int(st["edge"][ch]) == edge
        got = Y.bits_after_lock([(a, r[:, ch]) for a, r in rec_list])
        assert len(got) in (132, 133), len(got)
        # bit u of the satellite ends at block edge + 20 u + 19; received = truth ^ flip ^ (what the Costas loop fell into)
        polarity = {int(ip < 0) ^ int(truth[ch][(end - 19 - edge) // 20]) for end, ip in got}
        assert len(polarity) == 1, (ch, "bit errors")
        inv = polarity.pop()
        print("seed", seed, "channel", ch, "bits", len(got), "inv", inv, "flip", W.E2E_FLIP[ch])
        assert int(nav["inv"][ch]) == inv and int(nav["mode"][ch]) == N.SYNCED and int(nav["n_sync"][ch]) == 1 and int(nav["n_drop"][ch]) == 0
        assert W.E2E_WORD2_END[ch] == edge + 20 * W.E2E_SYNC_BIT + 19
        W.e2e_check_words(ch, words_abs[ch], W.e2e_bit_seed(seed, ch), inv)
        assert int(nav["blocks_seen"][ch]) == W.E2E_MS and int(nav["word_idx"][ch]) == 4
