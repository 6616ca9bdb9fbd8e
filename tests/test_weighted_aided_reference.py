"""Carrier aiding of the weighted code loop (include/gpsx.h gpsx_track_loop_weighted_aided, gpsx_track_loop_weighted_sync_aided),
without a GPU: the restatement the GPU tests compare against (tests/weighted_aided_ref.py) reduces to the unaided restatements at a
factor of 0; the clause pinned by hand, operation by operation; one satellite at +-4500 Hz, where the unaided steady loop loses the
code and the aided one holds it; the orbit chain of tests/weighted_pvt_cases.py with the quiet lock gains (0.5, 40), which aiding
turns from a 125 m fix into a 16 m one; the interface and the kernels' resources.

Measured on the restatement (tests/weighted_aided_cases.py MEASURED; EXPERIMENTS.md "Carrier aiding of the weighted code loop"):
  +4500 Hz, 2200 blocks: aided largest |code error| 0.77 samples from steady window 25 on, unaided +19.3 and growing, prompt ratio 0.053
  -4500 Hz, 2200 blocks: aided 1.90 samples, unaided -17.3 and growing, prompt ratio 0.052
  orbit chain, STILL + GPSX_WAID_L1CA: fixes 15.97 m (hand-over 3, 12.5) and 14.42 m (2, 7), unaided 124.8 / 123.3 m; transmit-time
  errors minus their mean within 0.72 samples, every observable VALID | CONFIRMED (0x2f)
Cost: the chain test synthesises the stream (25 s, shared with test_weighted_pvt_reference.py in one process) and runs two chains
side by side on eight CPUs (about 45 s)."""
import os
import subprocess
import tempfile

import numpy as np

import weighted_aided_cases as W
import weighted_aided_ref as A
import weighted_loop_cases as S
import weighted_loop_ref as L
import weighted_pvt_cases as P
import weighted_obs_ref as O
import weighted_sync_cases as K
import weighted_sync_ref as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SYMBOLS = {"gpsx_track_loop_weighted_aided", "gpsx_track_loop_weighted_aided_dev", "gpsx_track_loop_weighted_sync_aided",
           "gpsx_track_loop_weighted_sync_aided_dev"}


# ---- 1: a factor of 0 ----------------------------------------------------------------------------------------------------------------
def test_a_zero_factor_is_the_unaided_restatement(oracle):
    """both loops on an existing scenario of each: bytes of records and states; and the unaided restatements are still themselves
    after aided runs (weighted_loop_ref.update is put back)"""
    blocks, _ = S.scenario(S.AMPLITUDE, 1, 240)
    want_st = S.handover_state(1)
    want = [L.run(oracle, blocks[:200], want_st, L.make_cfg(**S.PULL_IN)), L.run(oracle, blocks[200:], want_st, L.make_cfg(**S.STEADY))]
    st = S.handover_state(1)
    got = [A.run(oracle, blocks[:200], st, L.make_cfg(**S.PULL_IN), 0.0), A.run(oracle, blocks[200:], st, L.make_cfg(**S.STEADY), 0.0)]
    assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want)) and st.tobytes() == want_st.tobytes()
    aided = S.handover_state(1)
    rec = A.run(oracle, blocks[:200], aided, L.make_cfg(**S.PULL_IN), A.WAID_L1CA)
    assert rec.tobytes() != want[0].tobytes() and L.update is A._unaided_update
    # the sync loop on the strong stream with mixed states (130 blocks: decisions, a channel leaving WAIT, bits)
    blocks = K.strong_blocks(130)
    cfg = Y.make_cfg(4, 20, S.PULL_IN, S.STEADY, 1, (5, 4))
    want_st = K.mixed_states(12, 5)
    want = Y.run(oracle, blocks, want_st, cfg)
    st = K.mixed_states(12, 5)
    got = A.run_sync(oracle, blocks, st, cfg, 0.0)
    assert got.tobytes() == want.tobytes() and st.tobytes() == want_st.tobytes()
    st = K.mixed_states(12, 5)
    assert A.run_sync(oracle, blocks, st, cfg, A.WAID_L1CA).tobytes() != want.tobytes()
    again = K.mixed_states(12, 5)
    assert Y.run(oracle, blocks, again, cfg).tobytes() == want.tobytes() and again.tobytes() == want_st.tobytes()


# ---- 2: the clause by hand -------------------------------------------------------------------------------------------------------------
# (code_phase_fine, dll_err, if_freq_offset_hz, (IE, QE, IL, QL), (dll_c1, dll_c2), n_coh, code_per_hz, what the row is for)
K1 = float(A.WAID_L1CA)
HAND = [
    (0.25, 0.0, 4800.0, (3000, 100, 3000, -100), (0.5, 40.0), 20, K1, "below 0: the aiding step carries it, the wrap comes after"),
    (16367.5, 0.0, -4800.0, (3000, 100, 3000, -100), (0.5, 40.0), 20, K1, "to >= 16368: the aiding step carries it, the wrap comes after"),
    (9000.0, 0.1, 4503.25, (52000, -300, 48000, 900), (0.5, 40.0), 20, K1, "a positive offset, T of 20 blocks"),
    (9000.0, -0.2, -4503.25, (41000, 7000, 46000, -2000), (1.0, 100.0), 4, K1, "a negative offset, T of 4 blocks"),
    (123.5, 0.0, 2718.5, (900, 20, 1100, -35), (1.0, 300.0), 1, K1, "T of 1 block"),
    (0.05, 0.3, -1234.5, (3000, 0, 2000, 0), (1.0, 100.0), 4, K1, "the DLL's own step wraps it, the aiding step moves it on from there"),
    (5000.0, 0.0, 1000.0, (0, 0, 0, 0), (0.5, 40.0), 20, 1.0, "no energy: d = 0; the factor's upper limit"),
    (5000.0, 0.0, 1000.0, (0, 0, 0, 0), (0.5, 40.0), 20, 0.0, "a factor of 0: no term"),
    (0.75, 0.0, 0.0, (0, 0, 0, 0), (0.5, 40.0), 20, K1, "(code_per_hz * T) * f would differ in the last bit (the offset is searched for)"),
]


def _last_bit_row():
    """an offset at which (k * f) * T and (k * T) * f differ, T = 20 blocks, and the phase 0.75 shows it: searched, so that the row
    does not rest on a constant"""
    k, t = F(K1), F(F(20) * F(0.001))
    for i in range(1, 4000):
        f = F(2700.0 + 0.25 * i)
        if F(F(0.75) - F(F(k * f) * t)) != F(F(0.75) - F(F(k * t) * f)):
            return f
    raise AssertionError("no such offset")


def test_the_clause_by_hand():
    seen = set()
    for phase0, dll_err, hz, (IE, QE, IL, QL), (c1, c2), n_coh, k, what in HAND:
        if "last bit" in what:
            hz = _last_bit_row()
        # ---- expected, with explicit float32 steps in the header's order
        t = F(F(n_coh) * F(0.001))
        e2, l2 = IE * IE + QE * QE, IL * IL + QL * QL
        d = F(0.0) if e2 + l2 == 0 else F(F(e2 - l2) / F(e2 + l2))        # (these sums are below 2^53: float32 of the exact integer)
        x = F(F(c1) * F(d - F(dll_err)))
        y = F(F(F(c2) * t) * d)
        phase = F(F(phase0) - F(x + y))
        before = phase
        if F(k) != F(0.0):
            step = F(F(k) * F(hz))
            step = F(step * t)
            phase = F(phase - step)
            if "last bit" in what:
                assert F(before - F(F(F(k) * t) * F(hz))) != phase      # (the other grouping gives another phase)
                seen.add("last bit")
        unwrapped = phase
        if phase < F(0.0):
            phase = F(phase + F(16368.0))
        elif phase >= F(16368.0):
            phase = F(phase - F(16368.0))
        # ---- the restatement's update on a state
        st = L.handover(7, phase0, hz)
        st["dll_err"] = dll_err
        cfg = A.loop_cfg(L.make_cfg(n_coh, True, 8, (c1, c2), S.STEADY["pll"], 0.0), k)
        iq = (IE, QE, 5000, 100, IL, QL)
        A.update(L._Scalar({name: st[name] for name in L.STATE_DTYPE.names}), iq, cfg)
        assert st["code_phase_fine"][0].tobytes() == phase.tobytes(), (what, st["code_phase_fine"][0], phase)
        assert st["dll_err"][0].tobytes() == d.tobytes() and int(st["n_updates"][0]) == 1
        # the carrier step and the loop memory are the unaided update's
        plain = L.handover(7, phase0, hz)
        plain["dll_err"] = dll_err
        L.update(L._Scalar({name: plain[name] for name in L.STATE_DTYPE.names}), iq, cfg)
        for f in L.STATE_DTYPE.names:
            same = st[f].tobytes() == plain[f].tobytes()
            assert same or f == "code_phase_fine", (what, f)
        if F(k) == F(0.0):
            assert st.tobytes() == plain.tobytes()
        # what the row is for
        if what.startswith("below 0"):
            assert before >= F(0.0) and unwrapped < F(0.0) and phase > F(16367.0)
            seen.add("down")
        if what.startswith("to >= 16368"):
            assert before < F(16368.0) and unwrapped >= F(16368.0) and phase < F(1.0)
            seen.add("up")
        if what.startswith("the DLL's own step wraps"):
            assert before < F(0.0) and float(phase) == float(F(F(before - F(F(F(k) * F(hz)) * t)) + F(16368.0)))
        seen.add(("T", n_coh))
        seen.add(("sign", hz > 0))
    assert {"down", "up", "last bit", ("T", 1), ("T", 4), ("T", 20), ("sign", True), ("sign", False)} <= seen


# ---- 3: one satellite at +-4500 Hz ---------------------------------------------------------------------------------------------------
def test_the_aided_steady_loop_holds_a_code_that_the_unaided_one_loses(oracle):
    import pytest
    from stm32f4_sdr_gps_amd import capi
    assert capi.WAID_L1CA == A.WAID_L1CA      # (the factor of these runs is the binding's GPSX_WAID_L1CA)
    for fd in W.DOPPLERS:
        _, aided, _, _ = W.scenario_run(oracle, fd, A.WAID_L1CA)
        _, plain, _, _ = W.scenario_run(oracle, fd, 0.0)
        assert len(aided) == len(plain) == (W.N_BLOCKS - W.PULL_IN_MS) // 20 == 100
        err, lost = W.steady_errors(fd, aided)[W.FIRST_WINDOW:], W.steady_errors(fd, plain)
        later = W.steady_errors(fd, aided, at_middle_of_next=True)[W.FIRST_WINDOW:]
        ratio = W.prompt_20ms(plain)[-10:].mean() / W.prompt_20ms(aided)[-10:].mean()
        print(f"fd {fd:+.0f} Hz: aided largest |code error| {np.abs(err).max():.4f} (mean {err.mean():+.4f}; against the delay half a window later "
              f"{later.mean():+.4f}), unaided error at the end {lost[-1]:+.2f}, 20 ms prompt aided {W.prompt_20ms(aided)[-10:].mean():.0f} "
              f"unaided / aided {ratio:.4f}")
        assert ratio < W.PROMPT_RATIO_MAX and abs(lost[-1]) > 8.0                  # the unaided loop has lost the code
        assert np.abs(err).max() < W.bounds()["scenario_error"][fd]              # the aided loop holds it
        assert np.abs(err).max() == pytest.approx(W.MEASURED["scenario_error"][fd], abs=5e-4)      # (the number written down is this run's)
        assert ratio == pytest.approx(W.MEASURED["prompt_ratio"][fd], abs=5e-4)


# ---- 4: the orbit chain ----------------------------------------------------------------------------------------------------------------
def test_the_orbit_chain_with_the_quiet_gains_and_aiding(lib_path):
    import pytest
    from stm32f4_sdr_gps_amd import capi
    lib = capi.load_library()
    assert capi.WAID_L1CA == A.WAID_L1CA and hasattr(lib, "gpsx_track_loop_weighted_sync_aided_dev")      # (the call this chain restates)
    assert W.HANDOVERS[0] == P.HANDOVER and [S.HANDOVER[k] for k in (1, 3)] == list(W.HANDOVERS)
    still = [P.MEASURED["still"][k] for k in (0, 2)]        # the unaided fixes of the same two hand-overs
    bounds = W.bounds()
    worst = 0.0
    for i, (out, st) in enumerate(W.chains_on_restatements()):
        P.check_conditions(out, st)
        _, _, _, _, obs, eph = out[-1]
        fixes = [P.position(lib, obs, eph, P.PRNS, offset) for offset in P.OFFSETS_MS]
        for fix, offset in zip(fixes, P.OFFSETS_MS):      # weighted_pvt_cases.check_fixes' conditions, with this run's bound
            assert fix["used"] == [0, 1, 2, 3], fix["used"]
            want = offset * 1e-3 - P.lag_s(P.sats()[fix["ref"]][1], P.N_BLOCKS)
            assert abs(fix["dtr"] - want) < P.CLOCK_TOL_S, (offset, fix["dtr"], want)
            assert abs(fix["rx_tow_s"] - fix["dtr"] - (P.TOW0 + P.N_BLOCKS * 1e-3)) < 1e-6 and fix["ref"] == 3
            err_m = P.position_error(fix)
            assert err_m < still[i] and err_m < max(P.MEASURED["moving"]), (i, err_m)      # better than unaided (0.5, 40) and (0.5, 200)
            assert err_m < bounds["position_m"][i], (i, err_m)
            assert err_m == pytest.approx(W.MEASURED["position_m"][i], abs=5e-3)
        assert float(np.linalg.norm(fixes[0]["rr"] - fixes[1]["rr"])) < P.OFFSETS_AGREE_M
        rows = [(at + n,) + W.tx_residuals(obs, at + n) for at, n, _, _, obs, _ in out if (obs["flags"] & O.F_VALID).all()]
        assert len(rows) >= 5 and rows[0][0] <= 8192
        for block, err, res in rows:
            print(f"hand-over {W.HANDOVERS[i]} block {block:5d}  error {np.round(err, 2)}  minus the mean {np.round(res, 2)}")
            worst = max(worst, float(np.abs(res).max()))
        print(f"hand-over {W.HANDOVERS[i]}: fix {P.position_error(fixes[0]):.3f} m (unaided (0.5, 40): {still[i]} m)")
        assert worst < bounds["tx_residual"], worst
    assert worst == pytest.approx(W.MEASURED["tx_residual"], abs=5e-4)


# ---- 5: the interface --------------------------------------------------------------------------------------------------------------------
LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "gpsx.h"
typedef int (*loop_dev)(gpsx_ctx *, const gpsx_wloop_cfg_t *, const gpsx_waid_t *, const void *, int, gpsx_wloop_state_t *, int, gpsx_wloop_rec_t *);
typedef int (*loop_host)(gpsx_ctx *, const gpsx_wloop_cfg_t *, const gpsx_waid_t *, const uint8_t *, int, gpsx_wloop_state_t *, int, gpsx_wloop_rec_t *);
typedef int (*sync_dev)(gpsx_ctx *, const gpsx_wsync_cfg_t *, const gpsx_waid_t *, const void *, int, gpsx_wsync_state_t *, int, gpsx_wsync_rec_t *);
typedef int (*sync_host)(gpsx_ctx *, const gpsx_wsync_cfg_t *, const gpsx_waid_t *, const uint8_t *, int, gpsx_wsync_state_t *, int, gpsx_wsync_rec_t *);
_Static_assert(__builtin_types_compatible_p(__typeof__(&gpsx_track_loop_weighted_aided_dev), loop_dev), "the loop's _dev entry point");
_Static_assert(__builtin_types_compatible_p(__typeof__(&gpsx_track_loop_weighted_aided), loop_host), "the loop's host entry point");
_Static_assert(__builtin_types_compatible_p(__typeof__(&gpsx_track_loop_weighted_sync_aided_dev), sync_dev), "the sync loop's _dev entry point");
_Static_assert(__builtin_types_compatible_p(__typeof__(&gpsx_track_loop_weighted_sync_aided), sync_host), "the sync loop's host entry point");
int main(void)
{
  printf("sizeof %zu\ncode_per_hz %zu\nreserved %zu\nversion %d\nl1ca %.9g\n", sizeof(gpsx_waid_t), offsetof(gpsx_waid_t, code_per_hz),
         offsetof(gpsx_waid_t, reserved), GPSX_VERSION, (double)GPSX_WAID_L1CA);
  return 0;
}
"""


def test_the_struct_and_the_entry_points_as_a_c_compiler_sees_them():
    with tempfile.TemporaryDirectory(prefix="waid_layout_") as tmp:
        src, exe = os.path.join(tmp, "layout.c"), os.path.join(tmp, "layout")
        with open(src, "w") as f:
            f.write(LAYOUT_C)
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
        got = dict(line.split() for line in subprocess.check_output([exe], text=True).splitlines())
    assert (int(got["sizeof"]), int(got["code_per_hz"]), int(got["reserved"]), int(got["version"])) == (8, 0, 4, 110)
    from stm32f4_sdr_gps_amd import capi
    assert F(float(got["l1ca"])) == capi.WAID_L1CA == A.WAID_L1CA == F(16.0 / 1540.0)
    assert capi.WAID_DTYPE.itemsize == 8 and capi.WAID_DTYPE.fields["reserved"][1] == 4
    assert capi.waid().tobytes() == np.array([0.010389610], "<f4").tobytes() + bytes(4)


def test_library_exports_the_aided_entry_points(lib_path):
    syms = subprocess.check_output(["nm", "-D", "--defined-only", lib_path], text=True)
    names = {line.split()[-1] for line in syms.splitlines() if line.strip()}
    assert SYMBOLS <= names
    from stm32f4_sdr_gps_amd import capi
    import __graft_entry__ as entry
    assert SYMBOLS <= set(entry.ABI_SYMBOLS)
    assert callable(getattr(capi.Engine, "track_loop_weighted_aided", None)) and callable(getattr(capi.Engine, "track_loop_weighted_sync_aided", None))
    lib = capi.load_library()
    assert all(len(getattr(lib, s).argtypes) == 8 for s in SYMBOLS) and lib.gpsx_version() == 110


def test_aided_kernels_resources(lib_path):
    from stm32f4_sdr_gps_amd import build
    res = build.check_no_scratch()
    for name in ("k_track_waid_loop", "k_track_waid_sync"):
        hits = [v for k, v in res.items() if name in k]
        assert len(hits) == 1 and hits[0]["scratch_bytes"] == 0 and hits[0]["vgprs"] <= 128, (name, hits)
        assert 8192 <= hits[0]["lds_bytes"] <= 8192 + 64      # two plane buffers, as the unaided kernels
    for name in ("k_track_wloop", "k_track_wsync"):          # the unaided kernels: still one of each
        assert len([k for k in res if name in k]) == 1, name


def test_the_shape_table_is_the_plan_headers():
    for row in W.SHAPES:
        assert W.tabled(row[0]) == row[1]
    assert [r[1] for r in W.SHAPES] == [1, 2, 16]


def test_the_split_case_has_a_channel_that_leaves_wait_in_the_one_block_piece(oracle):
    """the states of the GPU test's 37 + 1 + 92 comparison, on the restatement: split launches are one launch, and the made channel
    is accepted at block 25 and leaves WAIT at block 37"""
    blocks = K.strong_blocks(W.SPLIT_BLOCKS)
    one, events = W.split_states(), []
    whole = K.rekey([(0, A.run_sync(oracle, blocks, one, W.split_cfg(), A.WAID_L1CA, events=events))])
    ch, block = W.SPLIT_LEAVES_WAIT
    mine = [e for e in events if e[0] == ch]
    assert [e[1:3] for e in mine] == [(25, "decision"), (block, "locked")] and mine[0][4] and sum(W.SPLIT_PIECES[:1]) == block, mine
    st, parts, at = W.split_states(), [], 0
    for k in W.SPLIT_PIECES:
        parts.append((at, A.run_sync(oracle, blocks[at:at + k], st, W.split_cfg(), A.WAID_L1CA)))
        at += k
    assert st.tobytes() == one.tobytes() and K.rekey(parts) == whole


def test_the_parity_states_stand_on_every_ground(oracle):
    """what the GPU's byte-for-byte comparison runs on: wraps that the aiding term causes, in both directions (recomputed window by
    window from the restatement's own records); modes mixed, windows open; offsets of both signs up to 5 kHz"""
    seen = W.seam_wraps(oracle)
    assert seen["down"] and seen["up"], seen
    st, _ = W.parity_states(W.DISTINCT, 41)
    hz = st["loop"]["if_freq_offset_hz"]
    assert {int(m) for m in st["mode"]} == {Y.SEARCH, Y.WAIT, Y.LOCKED} and (st["win_n"] > 0).any()
    assert hz.min() <= -4800.0 and hz.max() >= 4800.0 and np.abs(hz).max() <= 5000.0
