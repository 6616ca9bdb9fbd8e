"""The weighted path's observables (include/gpsx.h gpsx_wobs), without a GPU: the layout of its structs as a C compiler sees them,
the exported entry points and the binding, the host-side pseudorange step, and the exact CPU restatement its GPU tests compare
against (tests/weighted_obs_ref.py): hand-made chains for every rule of the definition, continuity across the seam, split launches,
and the whole weighted chain on the restatements -- IF samples, the loop with bit sync, words, observables.

Measured on the restatements (amplitude 0.035, 3500 ms in launches of 1000 / 1000 / 1500, edge_guard 512; error = the observable's
transmit time at block 3500 minus the synthesised one, in samples):
  (a) PRN 7 / 19 / 30 at delays 4321 / 12007 / 13000: Z = 860 / 870 / 865, Tz = 599 860, no wraps, VALID without AMBIGUOUS;
      seed 1: -0.14 / -0.78 / -0.72, the largest over seeds 1, 2, 3: 0.91 (the loop's own code-phase error reaches 1.48 in locked
      windows); the whole millisecond exact everywhere
  (b) the same at delays 0.4 / 16367.6 / 8184.2: channel 1 wraps 60 times on seed 1 and 42 times on seed 2 and ends -0.67 / -0.74
      off; seed 2, channel 2 is VALID | AMBIGUOUS and exactly 1 ms late, +1.79 samples beside that (the loop sits half a block off
      its bits there: the synchroniser accepted edge 5); seed 1, channel 2 accepts edge 6 at block 1705 and has EDGE without TOW."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import weighted_obs_cases as X
import weighted_obs_ref as O
import weighted_sync_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"gpsx_wobs", "gpsx_wobs_dev", "gpsx_wobs_pseudoranges"}
F32 = np.float32
WIN, LOCKED, BIT = O.WSYNC_WINDOW, O.WSYNC_WINDOW | O.WSYNC_LOCKED, O.WSYNC_WINDOW | O.WSYNC_LOCKED | O.WSYNC_BIT
HOW_OK = O.WNAV_WORD | O.WNAV_OK

LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "gpsx.h"
typedef int (*dev_fn)(gpsx_ctx *, const gpsx_wobs_cfg_t *, const gpsx_wsync_rec_t *, int, int, const gpsx_wnav_word_t *, gpsx_wobs_state_t *, int,
                      gpsx_wobs_t *);
typedef int (*pr_fn)(const gpsx_wobs_t *, int, double, double *, double *);
_Static_assert(__builtin_types_compatible_p(__typeof__(&gpsx_wobs_dev), dev_fn), "the _dev entry point");
_Static_assert(__builtin_types_compatible_p(__typeof__(&gpsx_wobs), dev_fn), "the host entry point");
_Static_assert(__builtin_types_compatible_p(__typeof__(&gpsx_wobs_pseudoranges), pr_fn), "the pseudorange step");
#define S(f) printf("state.%s %zu\n", #f, offsetof(gpsx_wobs_state_t, f))
#define R(f) printf("obs.%s %zu\n", #f, offsetof(gpsx_wobs_t, f))
#define G(f) printf("cfg.%s %zu\n", #f, offsetof(gpsx_wobs_cfg_t, f))
int main(void)
{
  printf("sizeof.state %zu\nsizeof.obs %zu\nsizeof.cfg %zu\n", sizeof(gpsx_wobs_state_t), sizeof(gpsx_wobs_t), sizeof(gpsx_wobs_cfg_t));
  S(blocks_seen); S(last_bit_end_p1); S(chain_first_p1); S(edge_block); S(tx_ms_at_edge); S(last_win_end_p1); S(last_phase); S(last_freq);
  S(flags); S(n_wraps); S(n_anchor); S(n_mismatch); S(n_break); S(reserved);
  R(tx_ms); R(code_phase_fine); R(if_freq_offset_hz); R(flags); R(age_blocks); R(n_wraps); R(reserved);
  G(edge_guard); G(reserved);
  printf("flag.all %u\nflag.valid %u\nversion %d\n", GPSX_WOBS_PHASE | GPSX_WOBS_EDGE | GPSX_WOBS_TOW | GPSX_WOBS_CONFIRMED | GPSX_WOBS_AMBIGUOUS |
         GPSX_WOBS_VALID, GPSX_WOBS_VALID, GPSX_VERSION);
  return 0;
}
"""


def test_struct_layout_as_a_c_compiler_sees_it():
    with tempfile.TemporaryDirectory(prefix="wobs_layout_") as tmp:
        src, exe = os.path.join(tmp, "layout.c"), os.path.join(tmp, "layout")
        with open(src, "w") as f:
            f.write(LAYOUT_C)
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
        got = {k: int(v) for k, v in (line.split() for line in subprocess.check_output([exe], text=True).splitlines())}
    assert got["sizeof.cfg"] == 8 and got["sizeof.state"] == 80 and got["sizeof.obs"] == 32
    assert got["flag.all"] == 63 and got["flag.valid"] == 32 and got["version"] == 110
    state = {k[6:]: v for k, v in got.items() if k.startswith("state.")}
    obs = {k[4:]: v for k, v in got.items() if k.startswith("obs.")}
    assert state == {"blocks_seen": 0, "last_bit_end_p1": 8, "chain_first_p1": 16, "edge_block": 24, "tx_ms_at_edge": 32, "last_win_end_p1": 40,
                     "last_phase": 48, "last_freq": 52, "flags": 56, "n_wraps": 60, "n_anchor": 64, "n_mismatch": 68, "n_break": 72, "reserved": 76}
    assert obs == {"tx_ms": 0, "code_phase_fine": 8, "if_freq_offset_hz": 12, "flags": 16, "age_blocks": 20, "n_wraps": 24, "reserved": 28}
    assert {k[4:]: v for k, v in got.items() if k.startswith("cfg.")} == {"edge_guard": 0, "reserved": 4}
    for name, off in state.items():      # the restatement's and the binding's dtypes are that layout
        assert O.STATE_DTYPE.fields[name][1] == off, name
    for name, off in obs.items():
        assert O.OBS_DTYPE.fields[name][1] == off, name
    from stm32f4_sdr_gps_amd import capi
    assert capi.WOBS_STATE_DTYPE == O.STATE_DTYPE and capi.WOBS_DTYPE == O.OBS_DTYPE and capi.WOBS_CFG_DTYPE == O.CFG_DTYPE
    assert (capi.WOBS_FLAG_PHASE, capi.WOBS_FLAG_EDGE, capi.WOBS_FLAG_TOW, capi.WOBS_FLAG_CONFIRMED, capi.WOBS_FLAG_AMBIGUOUS,
            capi.WOBS_FLAG_VALID) == (O.F_PHASE, O.F_EDGE, O.F_TOW, O.F_CONFIRMED, O.F_AMBIGUOUS, O.F_VALID)


def test_library_exports_the_observables(lib_path):
    syms = subprocess.check_output(["nm", "-D", "--defined-only", lib_path], text=True)
    assert SYMBOLS <= {line.split()[-1] for line in syms.splitlines() if line.strip()}
    from stm32f4_sdr_gps_amd import capi
    import __graft_entry__ as entry
    assert SYMBOLS <= set(entry.ABI_SYMBOLS)
    assert callable(getattr(capi.Engine, "wobs", None)) and callable(capi.wobs_pseudoranges)
    lib = capi.load_library()
    assert lib.gpsx_wobs_dev.argtypes is not None and len(lib.gpsx_wobs.argtypes) == 9 and lib.gpsx_version() == 110


def test_observable_kernel_has_no_scratch_and_no_lds(lib_path):
    from stm32f4_sdr_gps_amd import build
    hits = [v for k, v in build.check_no_scratch().items() if "k_wobs" in k]
    assert len(hits) == 1 and hits[0]["scratch_bytes"] == 0 and hits[0]["lds_bytes"] == 0, hits
    assert hits[0]["vgprs"] <= 128      # two sets of eight slots' four words, the state: four waves per SIMD


# ---- hand-made chains: every rule of the definition ---------------------------------------------------------------------------------
def fresh():
    s = {name: 0 for name in O.STATE_DTYPE.names}
    s["last_phase"] = s["last_freq"] = F32(0.0)
    return s


def chain_windows(first_end, n_bits, phase, span=20, at=0):
    """LOCKED windows of `span` blocks that end with the bits' last blocks first_end, first_end + 20, ..; phase: a float or f(block)"""
    out = []
    for u in range(n_bits):
        for b in range(first_end + 20 * u - 20 + span, first_end + 20 * u + 1, span):
            p = phase(b) if callable(phase) else phase
            out.append((b - at, BIT if b == first_end + 20 * u else LOCKED, F32(p), F32(b)))
    return out


def test_which_side_of_mid_block_and_the_guard():
    """a bit that ends with block 99: the edge lies in block 100 for a code phase below half a block, in block 99 from 8184.0 on;
    AMBIGUOUS iff |p - 8184| < edge_guard, in float32 (8183.99 is 8183.990234375)"""
    for p, z, guards in ((8183.99, 100, {0.0: 0, 0.009: 0, 0.01: 1, 512.0: 1}), (8184.0, 99, {0.0: 0, 1e-30: 1, 8184.0: 1}),
                         (7672.0, 100, {512.0: 0, 512.001: 1}), (8696.0, 99, {512.0: 0, 512.001: 1}), (0.0, 100, {8184.0: 0}), (16367.99, 99, {8184.0: 1})):
        for guard, ambiguous in guards.items():
            s = fresh()
            o = O.channel(chain_windows(99, 3, p), [], s, 200, guard)
            assert s["edge_block"] == z and s["chain_first_p1"] == 100 and s["last_bit_end_p1"] == 140, (p, guard)
            assert s["flags"] == O.F_PHASE | O.F_EDGE | (O.F_AMBIGUOUS if ambiguous else 0), (p, guard, s["flags"])
            assert o["flags"] == s["flags"] and o["tx_ms"] == 0 and o["age_blocks"] == 60 and o["code_phase_fine"] == F32(p), (p, guard)
            assert o["if_freq_offset_hz"] == F32(139.0) and s["blocks_seen"] == 200 and s["last_win_end_p1"] == 140


def test_records_that_do_not_count():
    """no WINDOW, an end_block outside the launch, a phase that is none (NaN, negative, 16368.0, infinite): skipped, also as bits"""
    good = chain_windows(99, 5, 100.0)
    s = fresh()
    want = O.channel(good, [], s, 200, 0.0)
    junk = [(50, BIT & ~WIN, F32(5.0), F32(1.0)), (200, BIT, F32(5.0), F32(1.0)), (-1, BIT, F32(5.0), F32(1.0)), (4096, BIT, F32(5.0), F32(1.0)),
            (105, BIT, F32(np.nan), F32(1.0)), (106, WIN, F32(-0.001), F32(1.0)), (107, BIT, F32(16368.0), F32(1.0)), (108, WIN, F32(np.inf), F32(1.0)),
            (109, BIT, F32(-np.inf), F32(1.0)), (110, WIN, -F32(0.0) - F32(1e-38), F32(1.0))]
    mixed = []
    for k, w in enumerate(good):
        mixed += [junk[k % len(junk)], w, junk[(k + 3) % len(junk)]]
    s2 = fresh()
    assert O.channel(mixed, [], s2, 200, 0.0) == want and s2 == s and s["n_break"] == 0 and s["flags"] == O.F_PHASE | O.F_EDGE
    # a bit whose phase is none is a bit that is missing: the chain breaks at the next one
    holed = [w if k != 2 else (w[0], w[1], F32(np.nan), w[3]) for k, w in enumerate(good)]
    s3 = fresh()
    O.channel(holed, [], s3, 200, 0.0)
    assert s3["n_break"] == 1 and s3["chain_first_p1"] == 160 and s3["edge_block"] == 160
    # -0.0 is a phase (it is >= 0.0f)
    s4 = fresh()
    O.channel(chain_windows(99, 1, -0.0), [], s4, 200, 0.0)
    assert s4["flags"] == O.F_PHASE | O.F_EDGE and s4["edge_block"] == 100


def test_a_launch_without_a_record():
    s = fresh()
    o = O.channel([(-1, 0, F32(0.0), F32(0.0))] * 3, [(-1, 0, 0, 0)] * 2, s, 77, 512.0)
    assert o == dict(tx_ms=0, code_phase_fine=F32(0.0), if_freq_offset_hz=F32(0.0), flags=0, age_blocks=-1, n_wraps=0, reserved=0)
    assert s == dict(fresh(), blocks_seen=77)


def how(end_block, aux, flags=HOW_OK, index=2):
    return (end_block, flags, index, aux)


def anchored(z_phase=100.0, first_end=99, n_bits=70, aux=101, how_bit=61):
    """a chain of n_bits bits whose bit how_bit (0-based, >= 61) ends a HOW -> (windows, words, the HOW's end block)"""
    e = first_end + 20 * how_bit
    return chain_windows(first_end, n_bits, z_phase), [how(e, aux)], e


def test_the_anchor_and_the_week():
    """Tz from a HOW: T = 6000 (count - 1) + 1200 at the word's end, carried back to the edge of block Z; count 0 is the week's
    end (the next subframe is the week's first), 100 799 the last that can be sent"""
    for aux, t in ((101, 601200), (1, 1200), (0, 6000 * 100799 + 1200), (100799, 6000 * 100798 + 1200)):
        for phase, z in ((100.0, 100), (12000.0, 99)):
            wins, words, e = anchored(phase, aux=aux)
            s = fresh()
            o = O.channel(wins, words, s, 1500, 512.0)
            j = (e + 1 - z + 10) // 20
            assert j == 61 and s["tx_ms_at_edge"] == (t - 20 * j) % O.WEEK_MS and s["flags"] == O.F_PHASE | O.F_EDGE | O.F_TOW, (aux, phase)
            assert s["n_anchor"] == 1 and s["n_mismatch"] == 0 and o["flags"] == s["flags"] | O.F_VALID
            # at block B the transmit time is the word's end time plus the blocks since, the edge's offset in the block aside
            assert o["tx_ms"] == (t + 1500 - (e + 1) + (e + 1 - z - 20 * j)) % O.WEEK_MS, (aux, phase)
    # aux >= 100800 is no count; word 3, a failed word, a word outside the launch: not used
    for bad in (how(1319, 100800), how(1319, 2**32 - 1), how(1319, 101, index=3), how(1319, 101, flags=O.WNAV_WORD), how(1319, 101, flags=O.WNAV_OK),
                how(1500, 101), how(-1, 101)):
        wins, _, _ = anchored()
        s = fresh()
        O.channel(wins, [bad], s, 1500, 512.0)
        assert s["flags"] == O.F_PHASE | O.F_EDGE and s["n_anchor"] == 0 and s["n_mismatch"] == 0, bad
    # a tx_ms that crosses the week's end between Tz and B
    wins, words, e = anchored(aux=0)
    s = fresh()
    o = O.channel(wins, words, s, 4096, 0.0)
    assert s["tx_ms_at_edge"] == O.WEEK_MS - 6000 + 1200 - 1220 and o["tx_ms"] == s["tx_ms_at_edge"] + 4096 - 100
    o = O.channel([], [], s, 4096, 0.0)      # (a launch without a record: the time goes on, the phase ages)
    assert o["tx_ms"] == 1200 - 1220 + 8192 - 100 - 6000 + 0 * O.WEEK_MS == 2072 and o["age_blocks"] == 8192 - 1480 and o["flags"] & O.F_VALID


def test_which_hows_may_anchor():
    """a HOW needs 62 bits of this chain before its end, must end on one of the chain's bits, and must stand on the chain's edge"""
    wins, _, _ = anchored(n_bits=70)
    for end, used in ((99 + 20 * 60, False), (99 + 20 * 61, True), (99 + 20 * 69, True), (99 + 20 * 70, False), (99 + 20 * 61 + 1, False),
                      (99 + 20 * 61 - 7, False)):
        s = fresh()
        O.channel(wins, [how(end, 101)], s, 1500, 0.0)
        assert bool(s["flags"] & O.F_TOW) == used and s["n_mismatch"] == 0, end
    # the edge moved under the words (six wraps one way): |r| > 5, counted and not used; five are tolerated
    for wraps, used in ((5, True), (-5, True), (6, False), (-6, False)):
        s = fresh()
        O.channel(wins, [], s, 1480, 0.0)
        s["edge_block"] += wraps
        late = chain_windows(99 + 20 * 70, 10, 100.0, at=1480)
        O.channel(late, [how(99 + 20 * 75 - 1480, 101)], s, 500, 0.0)
        assert bool(s["flags"] & O.F_TOW) == used and s["n_mismatch"] == (0 if used else 1), wraps
        if used:      # the whole bits between the edge and the word's end: the nearest
            assert s["tx_ms_at_edge"] == 601200 - 20 * 75 and s["n_break"] == 0


def test_a_second_how():
    """one that agrees confirms; one that does not replaces the anchor, clears CONFIRMED and is counted"""
    wins = chain_windows(99, 400, 100.0, at=0)
    words = [how(99 + 20 * 61, 101), how(99 + 20 * 361, 102)]
    s = fresh()
    O.channel([w for w in wins if w[0] < 4096], [words[0]], s, 4096, 0.0)
    assert s["flags"] == O.F_PHASE | O.F_EDGE | O.F_TOW and s["tx_ms_at_edge"] == 601200 - 1220
    tz = s["tx_ms_at_edge"]
    rest = [(w[0] - 4096, w[1], w[2], w[3]) for w in wins if w[0] >= 4096]
    agree, differ = dict(s), dict(s)
    O.channel(rest, [how(99 + 20 * 361 - 4096, 102)], agree, 4000, 0.0)
    assert agree["flags"] & O.F_CONFIRMED and agree["tx_ms_at_edge"] == tz and agree["n_anchor"] == 1 and agree["n_mismatch"] == 0
    O.channel(rest, [how(99 + 20 * 361 - 4096, 103)], differ, 4000, 0.0)
    assert not differ["flags"] & O.F_CONFIRMED and differ["tx_ms_at_edge"] == tz + 6000 and differ["n_anchor"] == 1 and differ["n_mismatch"] == 1
    # ... and after a contradiction the next one that agrees confirms the NEW anchor
    O.channel(chain_windows(99 + 20 * 400, 205, 100.0, at=8096), [], differ, 4096, 0.0)
    o = O.channel(chain_windows(99 + 20 * 605, 100, 100.0, at=12192), [how(99 + 20 * 661 - 12192, 104)], differ, 2000, 0.0)
    assert differ["flags"] & O.F_CONFIRMED and differ["tx_ms_at_edge"] == tz + 6000 and differ["n_mismatch"] == 1 and differ["n_break"] == 0
    assert o["flags"] & O.F_VALID and o["tx_ms"] == tz + 6000 + 14192 - 100


def test_breaks():
    """a SEARCH window inside a chain, a gap of 40 blocks, a bit one block late: EDGE and TOW go, the next bit starts a chain, and a
    HOW that ended before the break in the same launch cannot anchor it"""
    wins, words, e = anchored(n_bits=70)
    for what in ("search", "gap", "late"):
        s = fresh()
        O.channel(wins, words, s, 1480, 512.0)
        assert s["flags"] & O.F_TOW
        at = 1480
        more = chain_windows(99 + 20 * 70, 70, 8184.0, at=at)
        if what == "search":
            more.insert(5, (more[5][0] - 7, WIN, F32(8184.0), F32(0.0)))
            first = more[6][0]
        elif what == "gap":
            more = more[:5] + [(b + 40, f, p, q) for b, f, p, q in more[5:]]
            first = more[5][0]
        else:
            more = more[:5] + [(b + 1, f, p, q) for b, f, p, q in more[5:]]
            first = more[5][0]
        stale = how(more[3][0], 101)                 # ends on a bit of the old chain
        own = how(first + 20 * 61, 107)              # ends on bit 61 of the new one
        for given, tow in (([stale], False), ([stale, own], True)):
            s2 = dict(s)
            o = O.channel(more, given, s2, 1500, 512.0)
            assert s2["n_break"] == 1 and s2["chain_first_p1"] == at + first + 1 and s2["edge_block"] == at + first, (what, given)
            assert bool(s2["flags"] & O.F_TOW) == tow and s2["flags"] & O.F_AMBIGUOUS and not s2["flags"] & O.F_CONFIRMED, (what, given)
            assert s2["n_anchor"] == (2 if tow else 1) and bool(o["flags"] & O.F_VALID) == tow
    # a SEARCH window forgets the newest bit: the bit after it starts a chain whatever its distance, and breaks nothing twice
    s = fresh()
    O.channel([(19, BIT, F32(1.0), F32(0.0)), (25, WIN, F32(1.0), F32(0.0)), (31, BIT, F32(1.0), F32(0.0)), (51, BIT, F32(1.0), F32(0.0))], [], s, 100, 0.0)
    assert s["n_break"] == 1 and s["chain_first_p1"] == 32 and s["last_bit_end_p1"] == 52 and s["flags"] == O.F_PHASE | O.F_EDGE


# ---- the seam -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("span", [1, 4, 5, 20])
@pytest.mark.parametrize("rate", [37.0, -29.0, 0.37])
def test_continuity_across_the_seam(span, rate):
    """a code phase drifting through the seam, in windows of `span` blocks (wraps fall between bits and on bit records), launches of
    300 blocks: from one observable to the next  d tx_ms - d phase / 16368 = n_blocks - d unwrapped / 16368, i.e. the whole
    milliseconds change by n_blocks minus the seam crossings, in integers"""
    start = {37.0: 16300.0, -29.0: 60.0, 0.37: 16368.0 - 0.37 * 3000}[rate]      # (the slow one crosses once, at block 3000)
    unwrapped = lambda b: start + rate * b      # noqa: E731
    first_end, n = 19, 300
    s = fresh()
    before, crossings = None, 0
    for at in range(0, 6000, n):
        bits = [u for u in range(400) if at <= first_end + 20 * u < at + n]
        wins = chain_windows(first_end + 20 * bits[0], len(bits), lambda b: unwrapped(b) % 16368.0, span, at)
        wins = [w for w in wins if w[0] >= 0]
        words = [how(first_end + 20 * 61 - at, 101)] if at <= first_end + 20 * 61 < at + n else []
        o = O.channel(wins, words, s, n, 0.0)
        if before is not None and before["flags"] & O.F_VALID:
            b0, b1 = at - 1, at + n - 1                     # the newest records' last blocks
            turns = int(unwrapped(b1) // 16368.0) - int(unwrapped(b0) // 16368.0)
            crossings += abs(turns)
            assert o["flags"] & O.F_VALID and o["tx_ms"] - before["tx_ms"] == n - turns, (at, turns)
            assert o["age_blocks"] == 0 and o["code_phase_fine"] == F32(unwrapped(b1) % 16368.0)
        before = o
    assert s["n_break"] == 0 and s["n_anchor"] == 1 and s["n_wraps"] >= crossings and crossings >= (1 if abs(rate) < 1 else 8)


def test_dithering_on_the_seam():
    """a phase that hops across the seam and back window after window: Z follows, and the transmit time stays within a sample"""
    phases = (16367.9, 0.05, 16367.95, 0.1, 0.02, 16367.99)
    wins = chain_windows(19, 200, lambda b: phases[(b // 5) % 6], 5)
    s = fresh()
    O.channel(wins, [how(19 + 20 * 61, 101)], s, 4000, 0.0)
    assert s["n_wraps"] > 200 and s["flags"] == O.F_PHASE | O.F_EDGE | O.F_TOW
    times = []
    for k in range(6):                                   # six further windows, one launch each
        b = 4000 + 5 * k
        o = O.channel([(4, LOCKED, F32(phases[(b + 4) // 5 % 6]), F32(0.0))], [], s, 5, 0.0)
        times.append(O.tx_time_ms(o) - (b + 5))
    assert max(times) - min(times) < 0.2 / 16368.0 + 1e-9 and {o["age_blocks"]} == {0}


# ---- split launches -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cuts", [(1,), (599,), (600,), (2050,), (4095,), (1000, 2000, 3000), (1237, 1238, 3333)])
def test_split_launches_equal_one_launch(cuts):
    """the 32 fabricated streams over blocks 500 .. 4595 in one launch and cut into several: the same last observable and the same
    states -- but for the one thing the two passes cannot give: a HOW that a break follows in its own launch anchors nothing, and
    with a cut between the two it anchors the chain that then ends.  On channels whose chain broke n_anchor may differ, and
    tx_ms_at_edge where no TOW holds (test_a_how_before_a_break_and_a_cut pins that)"""
    warm, n_blocks = 500, 4096
    nav0, st0 = X.warm_states(warm)
    nav1, whole = nav0.copy(), st0.copy()
    _, _, want = X.launch(nav1, whole, warm, n_blocks, 20, filler=False)
    nav2, parts = nav0.copy(), st0.copy()
    edges = (0,) + tuple(cuts) + (n_blocks,)
    for a, b in zip(edges, edges[1:]):
        _, _, got = X.launch(nav2, parts, warm + a, b - a, 20, filler=False)
    assert got.tobytes() == want.tobytes()
    broke = whole["n_break"] != st0["n_break"]
    assert (parts["n_break"] == whole["n_break"]).all() and broke.any() and not broke.all()
    for st in (parts, whole):
        st["n_anchor"][broke] = 0
        st["tx_ms_at_edge"][broke & (st["flags"] & O.F_TOW == 0)] = 0
    assert parts.tobytes() == whole.tobytes()
    assert (want["flags"] & O.F_VALID).sum() >= 10


def test_a_how_before_a_break_and_a_cut():
    """the exception to "split launches equal one": a HOW, then a gap, in one launch and with a cut between them"""
    wins, words, e = anchored(n_bits=70)
    tail = [(b + 40, f, p, q) for b, f, p, q in chain_windows(99 + 20 * 70, 20, 100.0)]
    whole = fresh()
    o1 = O.channel(wins + tail, words, whole, 2000, 0.0)
    parts = fresh()
    O.channel(wins, words, parts, 1480, 0.0)
    o2 = O.channel([(b - 1480, f, p, q) for b, f, p, q in tail], [], parts, 520, 0.0)
    assert o1 == o2 and o1["flags"] == O.F_PHASE | O.F_EDGE and whole["n_break"] == parts["n_break"] == 1
    assert (whole["n_anchor"], whole["tx_ms_at_edge"]) == (0, 0) and (parts["n_anchor"], parts["tx_ms_at_edge"]) == (1, 601200 - 1220)
    assert {k: v for k, v in whole.items() if k not in ("n_anchor", "tx_ms_at_edge")} == {k: v for k, v in parts.items() if k not in ("n_anchor", "tx_ms_at_edge")}


def test_the_case_table_stands_on_every_ground():
    """what the table the GPU runs meets, from the restatement"""
    seen = set()
    for i in range(len(X.CASES)):
        rec, words, n_blocks, st0, obs, after = X.case(i)
        d = {name: after[name].astype(np.int64) - st0[name].astype(np.int64) for name in ("n_wraps", "n_anchor", "n_mismatch", "n_break", "edge_block")}
        kept = (st0["flags"] & after["flags"] & O.F_EDGE != 0) & (d["n_break"] == 0)
        if (kept & (d["edge_block"] > 0)).any():
            seen.add("Z up")
        if (kept & (d["edge_block"] < 0)).any():
            seen.add("Z down")
        if (kept & (d["n_wraps"] >= 2) & (d["edge_block"] == 0)).any():
            seen.add("there and back")
        for name, what in (("n_anchor", "anchor"), ("n_mismatch", "mismatch"), ("n_break", "break")):
            if (d[name] > 0).any():
                seen.add(what)
        for flag, what in ((O.F_CONFIRMED, "confirmed"), (O.F_AMBIGUOUS, "ambiguous"), (O.F_VALID, "valid")):
            if (obs["flags"] & flag != 0).any():
                seen.add(what)
        if ((st0["flags"] & after["flags"] & O.F_TOW != 0) & (d["n_break"] == 0) & (st0["tx_ms_at_edge"] != after["tx_ms_at_edge"])).any():
            seen.add("contradicted")
        if ((st0["flags"] & O.F_TOW != 0) & (after["flags"] & O.F_TOW == 0)).any():
            seen.add("TOW lost")
        if (obs["age_blocks"] > 0).any():
            seen.add("aged")
        if ((obs["flags"] & O.F_VALID != 0) & (obs["tx_ms"] < 100000)).any() and (st0["tx_ms_at_edge"] > 604000000).any():
            seen.add("week's end")
        phases = rec["w"]["code_phase_fine"][rec["flags"] & 1 != 0]
        if np.isnan(phases).any() and (phases < 0).any() and (phases >= 16368.0).any():
            seen.add("no phase")
        if ((rec["flags"] & 3) == 1).any():
            seen.add("search")
    want = {"Z up", "Z down", "there and back", "anchor", "mismatch", "break", "confirmed", "ambiguous", "valid", "contradicted", "TOW lost", "aged", "week's end", "no phase", "search"}
    assert seen == want, (want - seen, seen - want)


# ---- bad states -------------------------------------------------------------------------------------------------------------------------
BAD_FIELDS = [("flags", 32), ("flags", 1 << 31), ("reserved", 1), ("blocks_seen", -1), ("blocks_seen", (1 << 62) + 1), ("last_bit_end_p1", -1),
              ("last_bit_end_p1", (1 << 62) + 1), ("chain_first_p1", -3), ("chain_first_p1", (1 << 62) + 1), ("last_win_end_p1", -1),
              ("last_win_end_p1", (1 << 62) + 1), ("edge_block", (1 << 62) + 1), ("edge_block", -(1 << 62) - 1), ("tx_ms_at_edge", -1),
              ("tx_ms_at_edge", 604800000), ("last_phase", np.nan), ("last_phase", -1.0), ("last_phase", 16368.0)]
GOOD_EDGES = [("blocks_seen", 1 << 62), ("edge_block", 1 << 62), ("edge_block", -(1 << 62)), ("tx_ms_at_edge", 604799999), ("last_phase", 16367.998),
              ("last_bit_end_p1", 1 << 62), ("chain_first_p1", 1 << 62), ("last_win_end_p1", 1 << 62)]


def test_bad_states():
    rec, words, n_blocks, st0, _, _ = X.case(2)
    st0 = st0[:32].copy()
    assert (st0["flags"] & O.F_PHASE).all()
    for field, value in BAD_FIELDS:
        st = st0.copy()
        st[field][7] = value
        keep = st.copy()
        obs, bad = O.run(rec[:, :32], n_blocks, words[:, :32], st, 512.0)
        assert bad == [7] and st[7:8].tobytes() == keep[7:8].tobytes(), (field, value)
        want = np.zeros(1, O.OBS_DTYPE)
        want["age_blocks"] = -1
        assert obs[7:8].tobytes() == want.tobytes() and (st["blocks_seen"][:7] == keep["blocks_seen"][:7] + n_blocks).all()
    # a NaN in last_phase without PHASE is nobody's business; the ends of the ranges are in range, and nothing overflows there
    st = st0.copy()
    st["flags"][7], st["last_phase"][7] = 0, np.nan
    assert O.run(rec[:, :32], n_blocks, words[:, :32], st, 512.0)[1] == []
    for field, value in GOOD_EDGES:
        st = st0.copy()
        st[field][7] = value
        obs, bad = O.run(rec[:, :32], n_blocks, words[:, :32], st, 512.0)
        assert bad == [] and 0 <= int(obs["tx_ms"][7]) < O.WEEK_MS and int(obs["age_blocks"][7]) >= 0, (field, value)


# ---- the whole weighted chain on the restatements ---------------------------------------------------------------------------------------
BOUND = 2.0          # samples; measured 0.91 at most (this file's docstring)


@pytest.mark.parametrize("seed", K.SEEDS)
def test_if_samples_to_observables_on_the_restatements(oracle, lib_path, seed):
    """scenario (a): the three standard satellites"""
    out, st, loop = X.chain_on_restatements(oracle, "a", seed)
    assert [int(z) for z in st["edge_block"]] == [860, 870, 865] and (st["tx_ms_at_edge"] == 599860).all() and not st["n_wraps"].any()
    assert (st["n_anchor"] == 1).all() and not st["n_mismatch"].any() and not st["n_break"].any() and (st["blocks_seen"] == 3500).all()
    last = out[-1][3]
    errors = []
    for ch, (_, _, delay, edge, _) in enumerate(K.SATS):
        assert int(last["flags"][ch]) == O.F_VALID | O.F_PHASE | O.F_EDGE | O.F_TOW, ch
        assert 0 <= int(last["age_blocks"][ch]) < 20 and int(loop["edge"][ch]) == K.EDGES_FOUND[ch]
        errors.append(X.error_samples(last[ch], delay, edge))
        print("seed", seed, "channel", ch, "tx_ms", int(last["tx_ms"][ch]), "phase", float(last["code_phase_fine"][ch]), "error in samples", errors[-1])
        assert abs(errors[-1]) < BOUND, (ch, errors[-1])
    # earlier launches: nothing VALID before a HOW (the first ends at block 2199), everything from then on
    assert not (out[0][3]["flags"] & O.F_VALID).any() and not (out[1][3]["flags"] & O.F_VALID).any()
    assert (out[1][3]["flags"] & O.F_EDGE).all() and (out[0][3]["flags"] & O.F_PHASE).all()
    # pseudorange differences are the synthesised delay differences
    from stm32f4_sdr_gps_amd import capi
    pr, rx_tow, n = capi.wobs_pseudoranges(last, 68.802)
    want_pr, want_rx, _ = O.pseudoranges(last, 68.802)
    assert n == 3 and np.array_equal(pr, want_pr) and rx_tow == want_rx
    truth = [X.truth_tx_ms(delay, edge, 3500) for _, _, delay, edge, _ in K.SATS]
    ref = int(np.argmax(truth))
    assert pr[ref] == 299792458e-3 * 68.802 and abs(rx_tow - (truth[ref] + 68.802) / 1000.0) < BOUND / 16368.0 / 1000.0
    for ch in range(3):
        got = (pr[ch] - pr[ref]) / 299792458e-3 * 16368.0
        assert abs(got - (truth[ref] - truth[ch]) * 16368.0) < 2 * BOUND, (ch, got)      # (two channels' errors)


@pytest.mark.parametrize("seed", [1, 2])
def test_the_seam_and_mid_block_on_the_restatements(oracle, seed):
    """scenario (b): delays 0.4, 16367.6 and 8184.2 samples"""
    out, st, loop = X.chain_on_restatements(oracle, "b", seed)
    last = out[-1][3]
    assert int(st["n_wraps"][1]) == {1: 60, 2: 42}[seed] and int(st["n_break"][1]) == 0
    for ch in (0, 1):
        assert int(last["flags"][ch]) == O.F_VALID | O.F_PHASE | O.F_EDGE | O.F_TOW, ch
        err = X.error_samples(last[ch], X.SEAM_DELAYS[ch], K.SATS[ch][3])
        print("seed", seed, "channel", ch, "wraps", int(st["n_wraps"][ch]), "error in samples", err)
        assert abs(err) < BOUND, (ch, err)
    err = X.error_samples(last[2], X.SEAM_DELAYS[2], K.SATS[2][3])
    if seed == 2:
        assert int(last["flags"][2]) == O.F_VALID | O.F_AMBIGUOUS | O.F_PHASE | O.F_EDGE | O.F_TOW
        print("seed 2 channel 2: error in samples", err, "=", round(err / 16368.0), "ms and", err - 16368.0 * round(err / 16368.0))
        assert min(abs(err - 16368.0 * k) for k in (-1, 0, 1)) < 4.0, err
    else:
        assert int(last["flags"][2]) & (O.F_EDGE | O.F_TOW | O.F_VALID) == O.F_EDGE and int(last["tx_ms"][2]) == 0
        assert int(last["flags"][2]) & O.F_AMBIGUOUS and int(loop["edge"][2]) == 6


# ---- gpsx_wobs_pseudoranges ---------------------------------------------------------------------------------------------------------------
def _obs(rows):
    obs = np.zeros(len(rows), O.OBS_DTYPE)
    for k, (tx_ms, phase, flags) in enumerate(rows):
        obs[k] = (tx_ms, phase, 0.0, flags, 0, 0, 0)
    return obs


def test_pseudoranges(lib_path):
    from stm32f4_sdr_gps_amd import capi
    v = O.F_VALID | 7
    c_ms = 299792458e-3
    # the latest transmit time is the reference, whole milliseconds first, then the smaller phase; invalid entries get 0
    obs = _obs([(1000, 5000.0, v), (1003, 16000.0, v), (1003, 200.5, v), (2000, 0.0, 7), (990, 8184.0, v | O.F_AMBIGUOUS)])
    pr, rx, n = capi.wobs_pseudoranges(obs, 70.0)
    assert n == 4 and pr[3] == 0.0 and pr[2] == c_ms * 70.0 and rx == (1003 - 200.5 / 16368.0 + 70.0) / 1000.0
    assert pr[0] == c_ms * (3.0 + (5000.0 - 200.5) / 16368.0 + 70.0) and pr[4] == c_ms * (13.0 + (8184.0 - 200.5) / 16368.0 + 70.0)
    want, want_rx, want_n = O.pseudoranges(obs, 70.0)
    assert np.array_equal(pr, want) and rx == want_rx and n == want_n
    # across the week's end: 604 799 990 is 25 ms BEFORE 15
    obs = _obs([(604799990, 100.0, v), (15, 300.0, v), (5, 100.0, v)])
    pr, rx, n = capi.wobs_pseudoranges(obs, 68.802)
    assert n == 3 and pr[1] == c_ms * 68.802 and pr[0] == c_ms * (25.0 - 200.0 / 16368.0 + 68.802) and pr[2] == c_ms * (10.0 - 200.0 / 16368.0 + 68.802)
    assert np.array_equal(pr, O.pseudoranges(obs, 68.802)[0])
    # the receiver time is folded into the week on either side
    obs = _obs([(604799990, 100.0, v)])
    assert capi.wobs_pseudoranges(obs, 68.802)[1] == O.pseudoranges(obs, 68.802)[1] < 1.0
    obs = _obs([(0, 8000.0, v)])
    assert capi.wobs_pseudoranges(obs, 0.0)[1] == O.pseudoranges(obs, 0.0)[1] > 604799.0
    # equal times: the first is the reference; nothing valid: zeros
    obs = _obs([(7, 1.0, v), (7, 1.0, v)])
    assert capi.wobs_pseudoranges(obs, 1.0)[0].tolist() == [c_ms, c_ms]
    pr, rx, n = capi.wobs_pseudoranges(_obs([(7, 1.0, 7), (9, 1.0, 0)]), 68.802)
    assert n == 0 and rx == 0.0 and not pr.any()
    # refusals
    lib = capi.load_library()
    one, pr1, rx1 = _obs([(7, 1.0, v)]), np.full(1, 5.0), C.c_double(5.0)
    for args in ((None, 1, 1.0, pr1.ctypes.data, C.byref(rx1)), (one.ctypes.data, 1, 1.0, None, C.byref(rx1)), (one.ctypes.data, 1, 1.0, pr1.ctypes.data, None),
                 (one.ctypes.data, 0, 1.0, pr1.ctypes.data, C.byref(rx1)), (one.ctypes.data, -1, 1.0, pr1.ctypes.data, C.byref(rx1)),
                 (one.ctypes.data, 1, float("nan"), pr1.ctypes.data, C.byref(rx1)), (one.ctypes.data, 1, float("inf"), pr1.ctypes.data, C.byref(rx1)),
                 (one.ctypes.data, 1, float("-inf"), pr1.ctypes.data, C.byref(rx1))):
        assert lib.gpsx_wobs_pseudoranges(*args) == -22 and pr1[0] == 5.0 and rx1.value == 5.0, args
    with pytest.raises(capi.GpsxError):
        capi.wobs_pseudoranges(one, float("nan"))
