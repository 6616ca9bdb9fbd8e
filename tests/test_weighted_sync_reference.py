"""The weighted loop with a per-channel bit synchroniser (include/gpsx.h gpsx_track_loop_weighted_sync), without a GPU: the layout
of its structs as a C compiler sees them, the exact CPU restatement its GPU tests compare against (tests/weighted_sync_ref.py) on
the three-satellite scenario -- per-channel synchronisation finds every edge and reads every bit where the launch-uniform recipe
does not --, the restatement's equivalences with the existing loop's, split launches, bad channels, and the exported entry points,
the binding and the kernel's resources.

Measured on the restatement (PRN 7 / 19 / 30 at amplitude 0.035, bit edges 0 / 10 / 5 ms after the stream's start, 2000 ms, uniform
noise of amplitude 1, seeds 1, 2, 3; search: n_coh 4 with weighted_loop_cases.PULL_IN's gains, lock: n_coh 20 with STEADY's,
sync_bits 20, ratio 5/4): on every seed every channel rejects its first decision (block 419: no round before it), accepts its
second (block 839) with edges 0 / 11 / 6, locks at blocks 840 / 851 / 846 and reads the 58 / 57 / 57 bits that follow with 0
errors.  The old recipe (200 ms of PULL_IN, then n_coh = 20 uniform over the launch) on the edge-10 channel: 32 / 41 / 42 errors of
90 against the bit in the window's first half, 43 / 44 / 43 against the one in its second."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import weighted_loop_cases as S
import weighted_loop_ref as L
import weighted_sync_cases as K
import weighted_sync_ref as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "gpsx.h"
typedef int (*dev_fn)(gpsx_ctx *, const gpsx_wsync_cfg_t *, const void *, int, gpsx_wsync_state_t *, int, gpsx_wsync_rec_t *);
typedef int (*host_fn)(gpsx_ctx *, const gpsx_wsync_cfg_t *, const uint8_t *, int, gpsx_wsync_state_t *, int, gpsx_wsync_rec_t *);
_Static_assert(__builtin_types_compatible_p(__typeof__(&gpsx_track_loop_weighted_sync_dev), dev_fn), "the _dev entry point");
_Static_assert(__builtin_types_compatible_p(__typeof__(&gpsx_track_loop_weighted_sync), host_fn), "the host entry point");
#define S(f) printf("state.%s %zu\n", #f, offsetof(gpsx_wsync_state_t, f))
#define R(f) printf("rec.%s %zu\n", #f, offsetof(gpsx_wsync_rec_t, f))
#define G(f) printf("cfg.%s %zu\n", #f, offsetof(gpsx_wsync_cfg_t, f))
int main(void)
{
  printf("sizeof.state %zu\nsizeof.rec %zu\nsizeof.cfg %zu\nsizeof.loop %zu\nsizeof.wrec %zu\n", sizeof(gpsx_wsync_state_t), sizeof(gpsx_wsync_rec_t),
         sizeof(gpsx_wsync_cfg_t), sizeof(gpsx_wloop_state_t), sizeof(gpsx_wloop_rec_t));
  S(loop); S(win_iq); S(win_n); S(ms_count); S(mode); S(edge); S(bit_ip); S(search_n); S(prev_best_p1); S(sync_rounds); S(p_i); S(p_q);
  S(last_best_e); S(last_opp_e); S(zero); S(base); S(e);
  R(w); R(end_block); R(flags); R(bit_ip);
  G(weights); G(spacing); G(n_coh_search); G(n_coh_lock); G(search); G(lock); G(sync_bits); G(sync_num); G(sync_den);
  printf("version %d\n", GPSX_VERSION);
  return 0;
}
"""


def test_struct_layout_as_a_c_compiler_sees_it():
    with tempfile.TemporaryDirectory(prefix="wsync_layout_") as tmp:
        src, exe = os.path.join(tmp, "layout.c"), os.path.join(tmp, "layout")
        with open(src, "w") as f:
            f.write(LAYOUT_C)
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
        got = dict(line.split() for line in subprocess.check_output([exe], text=True).splitlines())
    got = {k: int(v) for k, v in got.items()}
    assert got["sizeof.state"] == 448 and got["sizeof.rec"] == 48 and got["sizeof.cfg"] == 68 and got["sizeof.loop"] == 40 and got["sizeof.wrec"] == 36
    want = {"loop": 0, "win_iq": 40, "win_n": 64, "ms_count": 68, "mode": 72, "edge": 76, "bit_ip": 80, "search_n": 84, "prev_best_p1": 88,
            "sync_rounds": 92, "p_i": 96, "p_q": 100, "last_best_e": 104, "last_opp_e": 112, "zero": 120, "base": 128, "e": 288}
    assert {k[6:]: v for k, v in got.items() if k.startswith("state.")} == want
    assert {k[4:]: v for k, v in got.items() if k.startswith("rec.")} == {"w": 0, "end_block": 36, "flags": 40, "bit_ip": 44}
    assert {k[4:]: v for k, v in got.items() if k.startswith("cfg.")} == {"weights": 0, "spacing": 4, "n_coh_search": 8, "n_coh_lock": 12, "search": 16,
                                                                       "lock": 36, "sync_bits": 56, "sync_num": 60, "sync_den": 64}
    assert got["version"] == 110
    for name, off in want.items():      # the restatement's and the binding's dtypes are that layout
        assert Y.STATE_DTYPE.fields[name][1] == off, name
    from stm32f4_sdr_gps_amd import capi
    assert capi.WSYNC_STATE_DTYPE == Y.STATE_DTYPE and capi.WSYNC_REC_DTYPE == Y.REC_DTYPE


@pytest.mark.parametrize("seed", K.SEEDS)
def test_per_channel_sync_reads_every_satellite_where_the_uniform_recipe_does_not(oracle, seed):
    blocks, bits = K.scenario(seed, K.N_MS)
    # ---- per-channel synchronisation
    st = K.handover_states(seed)
    events = []
    rec = Y.run(oracle, blocks[:1000], st, K.sync_cfg(), events=events)          # (two launches: the open window crosses the cut)
    rec2 = Y.run(oracle, blocks[1000:], st, K.sync_cfg(), events=[])
    for ch in range(3):
        decisions = [e for e in events if e[0] == ch and e[2] == "decision"]
        locked = [e[1] for e in events if e[0] == ch and e[2] == "locked"]
        assert [(d[1], d[4]) for d in decisions] == [(419, False), (839, True)], decisions      # (block, accepted)
        assert not decisions[0][5] and decisions[1][5]                                           # rejected for want of a round before it
        ratio = decisions[1][6] / decisions[1][7]
        assert int(st[ch]["edge"]) == K.EDGES_FOUND[ch] == decisions[1][3] and int(st[ch]["mode"]) == Y.LOCKED
        assert len(locked) == 1 and 840 <= locked[0] < 860
        recs = Y.bits_after_lock([(0, rec[:, ch]), (1000, rec2[:, ch])])
        errors, n_bits = K.bit_errors(recs, bits[ch], K.EDGES_FOUND[ch])
        print("seed", seed, "channel", ch, "edge", int(st[ch]["edge"]), "locked at", locked[0], "energy ratio %.2f" % ratio, "bit errors", errors, "of", n_bits)
        assert errors == 0 and n_bits == (K.N_MS - locked[0]) // 20 >= 57
    # ---- the old recipe on the edge-10 channel: 200 ms of pull-in, then windows of 20 blocks uniform over the launch
    old = K.handover_states(seed)["loop"].copy()
    L.run(oracle, blocks[:S.PULL_IN_MS], old, L.make_cfg(**S.PULL_IN), channels=[1])
    r = L.run(oracle, blocks[S.PULL_IN_MS:], old, L.make_cfg(**S.STEADY), channels=[1])
    got = np.where(r["iq"][:, 1, 2] > 0, 1.0, -1.0)
    # window u holds the second half of the satellite's bit 9 + u and the first half of bit 10 + u: against either, either polarity
    worst = []
    for first in (9, 10):
        want = bits[1][first:first + 90]
        worst.append(min(int((got != want).sum()), int((got != -want).sum())))
    print("seed", seed, "the uniform recipe on the edge-10 channel:", worst, "errors of 90")
    assert len(got) == 90 and min(worst) >= 20


def _case_states(n=12, seed=5):
    return K.mixed_states(n, seed)


def test_locked_at_the_launchs_grid_is_the_existing_loop(oracle):
    """every channel preset LOCKED with edge = ms_count = 0 and n_coh_search = n_coh_lock = n: records and loop states are
    weighted_loop_ref.run's with n_coh = n; a BIT record every 20 / n windows with the sum of their prompts"""
    blocks = K.strong_blocks(40)
    for n, gains in ((1, S.REFERENCE_1MS), (4, S.PULL_IN), (20, S.STEADY)):
        st = K.mixed_states(5, 7, kinds=[0])
        st["mode"] = Y.LOCKED
        want_st = st["loop"].copy()
        want = L.run(oracle, blocks, want_st, L.make_cfg(n, True, 8, gains["dll"], gains["pll"], gains["fll"]))
        rec = Y.run(oracle, blocks, st, Y.make_cfg(n, n, gains, gains, 1, (5, 4)))
        assert rec.shape == want.shape and rec["w"].tobytes() == want.tobytes() and st["loop"].tobytes() == want_st.tobytes()
        per_bit = 20 // n
        for u in range(rec.shape[0]):
            is_bit = u % per_bit == per_bit - 1
            assert (rec["flags"][u] == (Y.F_WINDOW | Y.F_LOCKED | (Y.F_BIT if is_bit else 0))).all() and (rec["end_block"][u] == (u + 1) * n - 1).all()
            if is_bit:
                assert np.array_equal(rec["bit_ip"][u], want["iq"][u + 1 - per_bit:u + 1, :, 2].sum(axis=0))
            else:
                assert not rec["bit_ip"][u].any()
        assert (st["win_n"] == 0).all() and (st["ms_count"] == 0).all() and (st["mode"] == Y.LOCKED).all()


def test_a_search_before_its_first_decision_is_the_existing_loop(oracle):
    blocks = K.strong_blocks(36)
    st = K.mixed_states(5, 8, kinds=[0])
    want_st = st["loop"].copy()
    want = L.run(oracle, blocks, want_st, L.make_cfg(**S.PULL_IN))
    rec = Y.run(oracle, blocks, st, Y.make_cfg(4, 20, S.PULL_IN, S.STEADY, 1, (5, 4)))
    assert rec["w"].tobytes() == want.tobytes() and st["loop"].tobytes() == want_st.tobytes()
    assert (rec["flags"] == Y.F_WINDOW).all() and (st["search_n"] == 36).all() and (st["sync_rounds"] == 0).all()


def test_split_launches_are_one_launch(oracle):
    """130 blocks in launches of 37 / 1 / 92: states identical, records identical once keyed by the absolute end block"""
    blocks = K.strong_blocks(130)
    for pair in ((4, 20), (20, 5)):
        cfg = Y.make_cfg(pair[0], pair[1], S.PULL_IN, S.STEADY, 1, (5, 4))
        one = _case_states()
        whole = K.rekey([(0, Y.run(oracle, blocks, one, cfg))])
        st, parts, at = _case_states(), [], 0
        for k in (37, 1, 92):
            parts.append((at, Y.run(oracle, blocks[at:at + k], st, cfg)))
            at += k
        assert st.tobytes() == one.tobytes() and K.rekey(parts) == whole and len(whole) > 12 * 130 // 20


def test_the_case_table_stands_on_every_ground(oracle):
    """accept, rejection for disagreement, rejection for the ratio and a channel that leaves WAIT: all in the table the GPU runs"""
    seen = K.case_table_events(oracle)
    print({k: len(v) for k, v in seen.items()})
    assert all(seen[k] for k in ("accept", "disagree", "ratio", "left_wait", "bit"))


def test_bad_channels_move_nothing_but_their_accumulator(oracle):
    blocks = K.strong_blocks(45)
    st0, bad = K.bad_channel_states()
    st = st0.copy()
    cfg = Y.make_cfg(4, 20, S.PULL_IN, S.STEADY, 1, (5, 4))
    rec = Y.run(oracle, blocks, st, cfg)
    empty = Y.empty_records(rec.shape[0], 1)[:, 0]
    for ch in range(len(st)):
        if ch in bad:
            assert rec[:, ch].tobytes() == empty.tobytes(), ch
            a, b = st[ch:ch + 1].copy(), st0[ch:ch + 1].copy()
            assert a["loop"]["if_freq_accum"][0] != b["loop"]["if_freq_accum"][0]
            a["loop"]["if_freq_accum"] = b["loop"]["if_freq_accum"]
            assert a.tobytes() == b.tobytes(), ch
        else:
            assert (rec["flags"][:, ch] & Y.F_WINDOW).any() and st[ch:ch + 1].tobytes() != st0[ch:ch + 1].tobytes()


def test_library_exports_the_sync_entry_points(lib_path):
    syms = subprocess.check_output(["nm", "-D", "--defined-only", lib_path], text=True)
    names = {line.split()[-1] for line in syms.splitlines() if line.strip()}
    assert {"gpsx_track_loop_weighted_sync", "gpsx_track_loop_weighted_sync_dev"} <= names
    from stm32f4_sdr_gps_amd import capi
    import __graft_entry__ as entry
    assert {"gpsx_track_loop_weighted_sync", "gpsx_track_loop_weighted_sync_dev"} <= set(entry.ABI_SYMBOLS)
    assert callable(getattr(capi.Engine, "track_loop_weighted_sync", None))
    lib = capi.load_library()
    assert lib.gpsx_track_loop_weighted_sync_dev.argtypes is not None and lib.gpsx_version() == 110
    cfg = capi.wsync_cfg(4, 20, S.PULL_IN, S.STEADY, 20, (5, 4), False, 3)
    assert cfg.tobytes() == (np.array([0, 3, 4, 20], "<i4").tobytes() + np.array([1, 100, 56, 1600, 0.1, 0.5, 40, 21, 225, 0], "<f4").tobytes()
                             + np.array([20, 5, 4], "<i4").tobytes())
    assert capi.wsync_slots(130, 4, 20) == 33 and capi.wsync_slots(48, 20, 5) == 10


def test_sync_kernel_has_no_scratch(lib_path):
    from stm32f4_sdr_gps_amd import build
    res = build.check_no_scratch()
    hits = [v for k, v in res.items() if "k_track_wsync" in k]
    assert len(hits) == 1 and hits[0]["scratch_bytes"] == 0, hits
    assert 8192 <= hits[0]["lds_bytes"] <= 8192 + 64 and hits[0]["vgprs"] <= 128    # two plane buffers; four waves per SIMD
