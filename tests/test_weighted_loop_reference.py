"""The closed DLL / Costas PLL / FLL on weighted two-bit samples (include/gpsx.h gpsx_track_loop_weighted), without a GPU: the exact
CPU restatement its GPU tests compare against (tests/weighted_loop_ref.py) pinned to the open-loop correlators' restatement and to
its own chaining, the physics of the loop on that restatement alone -- it pulls in from a coherent grid's handover, stays in and
reads the data bits at an amplitude where the sign plane's 1 ms loop does not --, the edge cases of the definition, and the
exported entry points, the binding and the kernel's resources.

Measured on the restatement (PRN 7 at 1310 Hz and 4321 samples with 20 ms data bits, uniform noise of amplitude 1, 2000 ms,
200 ms of pull-in at n_coh = 4 with the frequency loop, then n_coh = 20; weighted_loop_cases.py holds the gains):
  amplitude 0.035 is the lowest of {0.1, 0.07, 0.05, 0.035} -- the lowest there is -- at which every one of the 90 bits after
  pull-in is decoded on the seeds 1, 2, 3 (0 / 0 / 0 errors; 0.05 likewise).  Over the run's last quarter the largest code-phase
  error is 0.681 / 0.580 / 0.403 samples and the largest distance of the carrier from fd (1 + 1/1022) is 0.784 / 0.691 / 0.784 Hz:
  the bounds asserted are twice the largest, 1.37 samples and 1.57 Hz.
  GPSX_WEIGHTS_SIGN_ONLY with n_coh = 1 and the reference's gains at that amplitude: from a carrier 250 / n_coh = 250 Hz off (the
  same rule at n_coh = 1) it never pulls in -- 41 / 38 / 39 bit errors of 90, the carrier 160 .. 260 Hz away; from the very handover
  the weighted loop starts from (12.5 Hz off) it slips half cycles -- 4 / 28 / 0 bit errors of 90."""
import subprocess

import numpy as np
import pytest

import weighted_loop_cases as S
import weighted_loop_ref as L
import weighted_track_ref as T

N_MS = 2000
CODE_BOUND, CARRIER_BOUND = 2 * 0.681, 2 * 0.784   # twice what the restatement shows on the three seeds (the docstring)


def _blocks(n, amp=0.3, seed=3):
    from stm32f4_sdr_gps_amd import synth
    sats = [synth.Sat(7, 1310.0, 4321.0, amp, 0.4), synth.Sat(19, -2240.0, 12007.0, amp, 2.0)]
    return synth.make_if_static(n, sats, noise_amp=1.0, seed=seed, two_bit=True)


def _states(rows):
    st = np.zeros(len(rows), L.STATE_DTYPE)
    for i, (prn, phase, off, acc) in enumerate(rows):
        st[i]["prn"], st[i]["code_phase_fine"], st[i]["if_freq_offset_hz"], st[i]["if_freq_accum"] = prn, phase, off, acc
    return st


ROWS = [(7, 4321.0, 1310.0, 0), (19, 12007.6, -2240.5, 0xFEDCBA98), (150, 3.0, 4999.75, 77), (30, 16360.2, 250.0, 0xFFFFFFF0)]


@pytest.mark.parametrize("n_coh,use_mag,spacing", [(1, True, 8), (4, False, 1), (10, True, 15), (20, True, 8)])
def test_with_gains_zero_the_windows_are_the_open_loop_sums(oracle, n_coh, use_mag, spacing):
    blocks = _blocks(2 * n_coh if n_coh > 4 else 8)
    st = _states(ROWS)
    before = st.copy()
    trk = np.zeros(len(st), L.TRK_DTYPE)
    for f in trk.dtype.names:
        trk[f] = st[f]
    per_block, acc = T.track(oracle, blocks, trk, use_mag, spacing)
    rec = L.run(oracle, blocks, st, L.make_cfg(n_coh, use_mag, spacing, dll=(0, 0), pll=(0, 0), fll=0))
    n_win = len(blocks) // n_coh
    want = per_block.astype(np.int64).reshape(n_win, n_coh, len(st), 6).sum(axis=1)
    assert rec.shape == (n_win, len(st)) and np.array_equal(rec["iq"], want) and np.abs(want).max() > 1000
    for f in ("prn", "code_phase_fine", "if_freq_offset_hz", "reserved"):
        assert st[f].tobytes() == before[f].tobytes(), f
    assert np.array_equal(st["if_freq_accum"], acc) and (st["n_updates"] == n_win).all()
    for ch, (_, _, off, a0) in enumerate(ROWS):                      # the accumulator's closed form, window by window
        step32 = (oracle.nco_step(np.float32(4092000) + np.float32(off)) * 32) & 0xFFFFFFFF
        for u in range(n_win):
            assert int(rec["if_freq_accum"][u, ch]) == (a0 + (u + 1) * n_coh * 511 * step32) % (1 << 32)
    assert (rec["code_phase_fine"] == before["code_phase_fine"]).all() and (rec["if_freq_offset_hz"] == before["if_freq_offset_hz"]).all()


def test_one_run_is_several_runs(oracle):
    """40 blocks in one run = the same blocks in runs of 8 / 12 / 20 (n_coh = 4) and of 20 / 20 (n_coh = 20, gains that move the
    state): states and records byte for byte"""
    blocks = _blocks(40, seed=5)
    for cfg, pieces in ((L.make_cfg(4, True, 8, dll=(1, 100), pll=(56, 1600), fll=0.1), (8, 12, 20)),
                        (L.make_cfg(20, False, 3, dll=(0.5, 40), pll=(21, 225), fll=0.0), (20, 20))):
        one = _states(ROWS)
        whole = L.run(oracle, blocks, one, cfg)
        st, parts, at = _states(ROWS), [], 0
        for k in pieces:
            parts.append(L.run(oracle, blocks[at:at + k], st, cfg))
            at += k
        assert np.concatenate(parts).tobytes() == whole.tobytes() and st.tobytes() == one.tobytes()
        assert not np.array_equal(whole["code_phase_fine"][0], whole["code_phase_fine"][-1])   # (the loop did move)


def _track(oracle, blocks, st, launches):
    records, at = [], 0
    for k, cfg in launches:
        k = len(blocks) - at if k is None else k
        records.append((at, cfg["n_coh"], L.run(oracle, blocks[at:at + k], st, cfg)))
        at += k
    return records


@pytest.mark.parametrize("seed", S.SEEDS)
def test_the_loop_pulls_in_stays_in_and_reads_the_data_bits(oracle, seed):
    blocks, bits = S.scenario(S.AMPLITUDE, seed, N_MS)
    st = S.handover_state(seed)
    recs = _track(oracle, blocks, st, [(S.PULL_IN_MS, L.make_cfg(**S.PULL_IN)), (None, L.make_cfg(**S.STEADY))])
    errors, n_bits = S.bit_errors(recs, bits, S.PULL_IN_MS // 20, N_MS)
    code, carrier = S.tail_errors(recs, N_MS)
    print("seed", seed, "amplitude", S.AMPLITUDE, "bit errors", errors, "of", n_bits, "code phase error %.3f samples" % code,
          "carrier %.3f Hz from fd (1 + 1/1022)" % carrier, "(%.3f from fd)" % abs(float(st["if_freq_offset_hz"][0]) - S.FD))
    assert errors == 0 and n_bits == 90
    assert code <= CODE_BOUND and carrier <= CARRIER_BOUND
    assert int(st["n_updates"][0]) == S.PULL_IN_MS // 4 + (N_MS - S.PULL_IN_MS) // 20


def test_the_sign_planes_one_millisecond_loop_does_not(oracle):
    """What the call is for: at the same amplitude GPSX_WEIGHTS_SIGN_ONLY with n_coh = 1 and the reference's gains loses lock or
    makes bit errors -- on every seed from a carrier 250 / n_coh Hz off, and in sum from the weighted loop's own handover"""
    cfg = L.make_cfg(use_magnitude=False, **S.REFERENCE_1MS)
    far, near = [], []
    for seed in S.SEEDS:
        blocks, bits = S.scenario(S.AMPLITUDE, seed, N_MS)
        for scale, out in ((20.0, far), (1.0, near)):
            st = S.handover_state(seed, carrier_scale=scale)
            recs = _track(oracle, blocks, st, [(None, cfg)])
            errors, n_bits = S.bit_errors(recs, bits, S.PULL_IN_MS // 20, N_MS)
            out.append((errors, S.tail_errors(recs, N_MS)[1]))
    print("sign only, n_coh = 1: (bit errors of 90, carrier distance) from 250 Hz off", far, "from the same handover", near)
    assert all(e > 0 or hz > CARRIER_BOUND for e, hz in far)
    assert sum(e for e, _ in near) > 0


def _one(phase=100.0, off=10.0, dll_err=0.0, pll_err=0.0, prev=(0, 0), n_updates=0):
    st = L.handover(5, phase, off)
    st[0]["dll_err"], st[0]["pll_err"], st[0]["prev_ip"], st[0]["prev_qp"], st[0]["n_updates"] = dll_err, pll_err, prev[0], prev[1], n_updates
    return st


def _update(st, iq, cfg):
    L.update(L._Scalar({name: st[name] for name in L.STATE_DTYPE.names}), iq, cfg)


def test_edge_cases_of_the_definition():
    cfg = L.make_cfg(1, dll=(1, 300), pll=(4, 3000), fll=0.5)
    f32 = np.float32
    # IP == 0: a quarter cycle with QP's sign, nothing for QP == 0
    for qp, p in ((7, 0.25), (-7, -0.25), (0, 0.0)):
        st = _one(n_updates=0)
        _update(st, (5, 5, 0, qp, 5, 5), cfg)
        assert st["pll_err"][0] == f32(p)
        assert st["if_freq_offset_hz"][0] == f32(10.0) - ((f32(4) * f32(p) + (f32(3000) * f32(0.001)) * f32(p)) + f32(0.5) * f32(0))
    # e2 + l2 == 0 (what a window without weight on Early and Late gives): d = 0, the code phase stays; dot == 0: no FLL term
    st = _one(prev=(3, 4), n_updates=1)
    _update(st, (0, 0, 4, -3, 0, 0), cfg)
    assert st["dll_err"][0] == 0 and st["code_phase_fine"][0] == f32(100.0)
    p = f32(L.atanf(f32(-3) / f32(4)) * L.CYCLES)
    assert st["if_freq_offset_hz"][0] == f32(f32(10.0) - f32(f32(f32(4) * p) + f32(f32(f32(3000) * f32(0.001)) * p)))
    assert (st["prev_ip"][0], st["prev_qp"][0], st["n_updates"][0]) == (4, -3, 2)
    # all six zero: nothing moves but the window count
    st = _one(phase=7.5, off=-3.25)
    _update(st, (0,) * 6, cfg)
    assert (st["code_phase_fine"][0], st["if_freq_offset_hz"][0], st["n_updates"][0]) == (f32(7.5), f32(-3.25), 1)
    # the FLL waits for a previous prompt, and is insensitive to a data bit flip between the windows
    a, b = _one(prev=(100, 0), n_updates=0), _one(prev=(100, 0), n_updates=1)
    for st in (a, b):
        _update(st, (1, 0, 90, 30, 1, 0), cfg)
    fe = f32(f32(L.atanf(f32(3000) / f32(9000)) * L.CYCLES) / f32(0.001))
    assert a["if_freq_offset_hz"][0] - b["if_freq_offset_hz"][0] == pytest.approx(0.5 * float(fe), rel=1e-5) and fe > 50
    c = _one(prev=(-100, 0), n_updates=1)
    _update(c, (1, 0, 90, 30, 1, 0), cfg)
    assert c["if_freq_offset_hz"][0] == b["if_freq_offset_hz"][0]
    # one wrap at either end of [0, 16368): d = +1 moves the phase down by c1 + c2 T = 1.3, d = -1 up
    for phase, iq, want in ((0.5, (9, 0, 5, 0, 0, 0), f32(f32(0.5) - f32(1.3)) + f32(16368.0)),
                            (16367.5, (0, 0, 5, 0, 9, 0), f32(f32(16367.5) + f32(1.3)) - f32(16368.0)),
                            (16367.0, (0, 0, 5, 0, 9, 0), f32(16367.0) + f32(1.3) - f32(16368.0))):
        st = _one(phase=phase)
        _update(st, iq, L.make_cfg(1, dll=(1, 300), pll=(0, 0)))
        assert st["code_phase_fine"][0] == f32(want) and 0 <= st["code_phase_fine"][0] < 16368
    assert T.tau_of(f32(f32(0.5) - f32(1.3)) + f32(16368.0)) == 16367
    # int64 -> float rounds to nearest even, as the conversion instruction does
    for v in (0, 1, -1, (1 << 24) + 1, (1 << 24) + 3, -(1 << 25) - 2, 981120 ** 2 * 2, 981120 ** 2 * 2 - 1, (1 << 40) + (1 << 16)):
        assert L.i64_to_f32(v) == np.array([v], np.int64).astype(np.float32)[0] and float(L.i64_to_f32(v)) == float(np.float32(v))


def test_no_nan_from_finite_inputs():
    """random window sums over the whole range, random finite states, the scenario's gains and the reference's: every float stays
    finite and the code phase stays on the circle"""
    rng = np.random.default_rng(9)
    cfgs = [L.make_cfg(**S.PULL_IN), L.make_cfg(**S.STEADY), L.make_cfg(**S.REFERENCE_1MS), L.make_cfg(20, dll=(1, 300), pll=(8, 5000), fll=1.0)]
    for trial in range(400):
        cfg = cfgs[trial % len(cfgs)]
        top = 49056 * cfg["n_coh"]
        st = _one(phase=float(rng.uniform(0, 16368)), off=float(rng.uniform(-5000, 5000)), dll_err=float(rng.uniform(-1, 1)),
                  pll_err=float(rng.uniform(-0.25, 0.25)), prev=tuple(int(v) for v in rng.integers(-top, top + 1, 2)),
                  n_updates=int(rng.integers(0, 3)))
        iq = rng.integers(-top, top + 1, 6) * rng.integers(0, 2, 6) if trial % 3 == 0 else rng.integers(-top, top + 1, 6)
        _update(st, iq, cfg)
        for f in ("code_phase_fine", "if_freq_offset_hz", "dll_err", "pll_err"):
            assert np.isfinite(st[f][0]), (trial, f)
        assert 0 <= st["code_phase_fine"][0] < 16368 and abs(st["dll_err"][0]) <= 1 and abs(st["pll_err"][0]) <= 0.25


def test_bad_channels_keep_their_floats_and_advance_their_accumulator(oracle):
    blocks = _blocks(8)
    rows = [(7, 4321.0, 1310.0, 5), (0, 100.0, 77.0, 5), (211, 200.0, -3.0, 9), (9, float("nan"), 12.0, 1), (9, -16777216.0, 12.0, 1)]
    st = _states(rows)
    st["dll_err"], st["pll_err"], st["prev_ip"], st["prev_qp"], st["n_updates"] = 0.125, -0.0625, 11, -12, 3
    before = st.copy()
    rec = L.run(oracle, blocks, st, L.make_cfg(4, dll=(1, 100), pll=(56, 1600), fll=0.1))
    assert rec["iq"][:, 0].any() and not rec["iq"][:, 1:].any()
    for ch in range(1, len(rows)):
        for f in ("prn", "code_phase_fine", "if_freq_offset_hz", "dll_err", "pll_err", "prev_ip", "prev_qp", "n_updates", "reserved"):
            assert st[f][ch:ch + 1].tobytes() == before[f][ch:ch + 1].tobytes(), (ch, f)
        step32 = (oracle.nco_step(np.float32(4092000) + np.float32(rows[ch][2])) * 32) & 0xFFFFFFFF
        assert int(st["if_freq_accum"][ch]) == (rows[ch][3] + 8 * 511 * step32) % (1 << 32)
        assert int(rec["if_freq_accum"][0, ch]) == (rows[ch][3] + 4 * 511 * step32) % (1 << 32)
    assert st["n_updates"][0] == 5 and st["code_phase_fine"][0] != before["code_phase_fine"][0]
    with pytest.raises(AssertionError):
        L.run(oracle, blocks[:7], st, L.make_cfg(4))     # n_blocks must be a multiple of n_coh


def test_library_exports_the_weighted_loop_entry_points(lib_path):
    syms = subprocess.check_output(["nm", "-D", "--defined-only", lib_path], text=True)
    names = {line.split()[-1] for line in syms.splitlines() if line.strip()}
    assert {"gpsx_track_loop_weighted", "gpsx_track_loop_weighted_dev"} <= names
    from stm32f4_sdr_gps_amd import capi
    import __graft_entry__ as entry
    assert {"gpsx_track_loop_weighted", "gpsx_track_loop_weighted_dev"} <= set(entry.ABI_SYMBOLS)
    assert callable(getattr(capi.Engine, "track_loop_weighted", None))
    assert capi.WLOOP_STATE_DTYPE == L.STATE_DTYPE and capi.WLOOP_REC_DTYPE == L.REC_DTYPE
    lib = capi.load_library()
    assert lib.gpsx_track_loop_weighted_dev.argtypes is not None and lib.gpsx_version() == 110
    cfg = capi.wloop_cfg(20, False, 3, (0.5, 40.0), (21.0, 225.0), 0.25)
    assert cfg.nbytes == 32 and cfg.tobytes() == np.array([0, 3, 20], "<i4").tobytes() + np.array([0.5, 40, 21, 225, 0.25], "<f4").tobytes()


def test_weighted_loop_kernel_has_no_scratch(lib_path):
    from stm32f4_sdr_gps_amd import build
    res = build.check_no_scratch()
    hits = [v for k, v in res.items() if "k_track_wloop" in k]
    assert len(hits) == 1 and hits[0]["scratch_bytes"] == 0, hits
    assert 8192 <= hits[0]["lds_bytes"] <= 8192 + 64 and hits[0]["vgprs"] <= 128    # two plane buffers; four waves per SIMD
