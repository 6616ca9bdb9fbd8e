"""The weighted two-bit E/P/L correlators over K blocks (include/gpsx.h gpsx_track_epl_weighted), without a GPU: the exact CPU
restatement its GPU tests compare against (tests/weighted_track_ref.py) pinned to the weighted grids' restatements -- the prompt of
one block is weighted_ms_ref.iq at tau, the prompts of chained blocks sum to weighted_coh_ref.iq at tau and Early / Late to the
same arrays at tau -+ spacing --, to the closed form of the accumulator a call leaves, to the popcount identity the kernel
evaluates, and to the sign convention of the Early-minus-Late discriminator; plus the exported entry points, the binding and the
kernel's resources."""
import subprocess

import numpy as np
import pytest

import weighted_coh_ref as R
import weighted_ms_ref as W
import weighted_track_ref as T


def _blocks(n, amp=0.3, seed=3):
    from stm32f4_sdr_gps_amd import synth
    sats = [synth.Sat(7, 1310.0, 4321.0, amp, 0.4), synth.Sat(19, -2240.0, 12007.0, amp, 2.0)]
    return synth.make_if_static(n, sats, noise_amp=1.0, seed=seed, two_bit=True)


def _states(rows):
    from stm32f4_sdr_gps_amd import capi
    st = np.zeros(len(rows), capi.TRK_DTYPE)
    for i, (prn, phase, off, acc) in enumerate(rows):
        st[i] = (prn, phase, off, acc)
    return st


@pytest.mark.parametrize("use_mag", [True, False])
def test_prompt_of_one_block_is_the_one_block_grid_at_tau(oracle, use_mag):
    blocks = _blocks(1)
    st = _states([(7, 4321.0, 1310.0, 0), (19, 12007.6, -2240.0, 0), (3, 0.0, 500.0, 0)])
    got, _ = T.track(oracle, blocks, st, use_mag)
    for ch in range(len(st)):
        i, q = W.iq(oracle, blocks[0], int(st["prn"][ch]), 4092000 + int(st["if_freq_offset_hz"][ch]), use_mag)
        tau = int(st["code_phase_fine"][ch])
        assert (got[0, ch, 2], got[0, ch, 3]) == (i[tau], q[tau])


@pytest.mark.parametrize("spacing", [1, 8, 15])
def test_three_chained_blocks_sum_to_the_coherent_grid(oracle, spacing):
    blocks = _blocks(3)
    st = _states([(7, 4321.0, 1310.0, 0), (19, 5.0, -2240.0, 0), (30, 16360.2, 250.0, 0)])   # tau -+ spacing wraps on both sides
    got, _ = T.track(oracle, blocks, st, True, spacing)
    for ch in range(len(st)):
        i, q = R.iq(oracle, blocks, 0, 3, int(st["prn"][ch]), 4092000 + int(st["if_freq_offset_hz"][ch]))
        tau = int(st["code_phase_fine"][ch])
        s = got[:, ch, :].astype(np.int64).sum(axis=0)
        for k, t in enumerate(((tau - spacing) % 16368, tau, (tau + spacing) % 16368)):
            assert (s[2 * k], s[2 * k + 1]) == (i[t], q[t]), (ch, k)


def test_accumulator_left_after_k_blocks(oracle):
    blocks = _blocks(5)
    rows = [(7, 100.0, 1310.0, 0), (8, 200.0, -4999.5, 0x12345678), (9, 300.0, 0.25, 0xFFFFFFF0), (0, 1.0, 77.0, 5),
            (10, float("nan"), -3.0, 9)]
    st = _states(rows)
    for k in (1, 2, 5):
        _, acc = T.track(oracle, blocks[:k], st, channels=[0])
        for ch, (_, _, off, a0) in enumerate(rows):
            step32 = (oracle.nco_step(np.float32(4092000) + np.float32(off)) * 32) & 0xFFFFFFFF
            assert int(acc[ch]) == (a0 + k * 511 * step32) % (1 << 32)


@pytest.mark.parametrize("use_mag", [True, False])
def test_selected_blocks_equal_the_full_computation(oracle, use_mag):
    """track(blocks=...) starts block b from acc + b x 511 x step32: the selected records are the full computation's bit for
    bit, the others stay zero, the accumulators are the whole call's; with a channel selection on top, and counted"""
    blocks = _blocks(7, seed=9)
    st = _states([(7, 4321.0, 1310.0, 0), (19, 16367.2, -2240.5, 0xFEDCBA98), (150, 3.0, 4999.75, 77), (0, 5.0, 10.0, 1),
                  (33, float("nan"), -8.0, 2)])
    full, acc_full = T.track(oracle, blocks, st, use_mag, 5)
    assert full[:, :3, :].any(axis=2).all() and not full[:, 3:, :].any()
    for pick in ([0], [6], [2, 5], [6, 0, 3, 3], range(7)):
        n = [0]
        got, acc = T.track(oracle, blocks, st, use_mag, 5, blocks=pick, count=n)
        assert got.dtype == np.int32 and acc.dtype == np.uint32 and np.array_equal(acc, acc_full)
        sel = sorted(set(pick))
        rest = [b for b in range(7) if b not in sel]
        assert np.array_equal(got[sel], full[sel]) and not got[rest].any()
        assert n[0] == 3 * len(sel)                                        # the bad channels are not restated
    n = [0]
    got, acc = T.track(oracle, blocks, st, use_mag, 5, channels=[1, 3], blocks=[4, 1], count=n)
    assert np.array_equal(acc, acc_full) and np.array_equal(got[[1, 4], 1], full[[1, 4], 1]) and n[0] == 2
    got[[1, 4], 1] = 0
    assert not got.any()
    with pytest.raises(AssertionError):
        T.track(oracle, blocks, st, use_mag, 5, blocks=[7])


def test_tau_truncates_towards_zero_and_wraps():
    for phase, tau in ((0.0, 0), (7.9, 7), (16367.99, 16367), (-3.5, 16365), (16370.2, 2), (-0.9, 0), (16368.0, 0),
                       (-16368.0, 0), (16777215.0, 16777215 % 16368)):
        assert T.tau_of(phase) == tau, phase
    for phase in (float("nan"), float("inf"), -float("inf"), 16777216.0, -16777216.0, 1e30):
        assert T.tau_of(phase) is None


@pytest.mark.parametrize("use_mag", [True, False])
def test_popcount_identity_of_the_kernel(oracle, use_mag):
    """What k_track_epl_weighted evaluates: with y = wiped bit ^ chip bit and m the magnitude bit over the N = 16352 mixed samples,
    I = (2 pop(y) - N) + 2 (2 pop(y & m) - pop(m))"""
    blocks = _blocks(2, seed=5)
    st = _states([(7, 4321.0, 1310.5, 0x9ABCDEF0), (44, 16367.0, -800.0, 77)])
    got, _ = T.track(oracle, blocks, st, use_mag, 8)
    n = W.MIXED
    for ch in range(2):
        prn, acc = int(st["prn"][ch]), int(st["if_freq_accum"][ch])
        f = T.carrier_hz(4092000, st["if_freq_offset_hz"][ch])
        chip = np.repeat(oracle.ca_code(prn).astype(np.uint8), 16)
        tau = T.tau_of(st["code_phase_fine"][ch])
        for b in range(2):
            sign, mag = W.planes(blocks[b])
            di, dq, acc = oracle.wipeoff(np.packbits(sign, bitorder="little"), f, acc)
            m = (mag if use_mag else np.zeros_like(mag))[:n].astype(np.int64)
            for k, d in enumerate((-8, 0, 8)):
                r = np.roll(chip, (tau + d) % 16368)[:n]
                for c, data in enumerate((di, dq)):
                    y = (np.unpackbits(data.view(np.uint8), bitorder="little")[:n] ^ r).astype(np.int64)
                    assert got[b, ch, 2 * k + c] == (2 * y.sum() - n) + 2 * (2 * (y & m).sum() - m.sum())


def test_sign_convention_of_the_discriminator(oracle):
    """(|E| - |L|) / (|E| + |L|) > 0 means tau is too large: magnitudes summed over 40 blocks, a code phase 3 samples off the
    truth either way, at spacing 8, 2 and 15 (include/gpsx.h quotes +0.36 / +0.14 / +0.40 and -0.32 / -0.12 / -0.45)"""
    from stm32f4_sdr_gps_amd import synth
    blocks = synth.make_if_static(40, [synth.Sat(7, 1310.0, 4321.0, 0.1, 0.4)], noise_amp=1.0, seed=3, two_bit=True)
    want = {(3, 8): 0.36, (3, 2): 0.14, (3, 15): 0.40, (-3, 8): -0.32, (-3, 2): -0.12, (-3, 15): -0.45}
    for (err, spacing), value in want.items():
        got, _ = T.track(oracle, blocks, _states([(7, 4321.0 + err, 1310.0, 0)]), True, spacing)
        d = T.discriminator(got[:, 0, :])
        print("tau error", err, "spacing", spacing, "discriminator", round(float(d), 3))
        # (the header's figures carry two decimals: half a unit of the last one, and a little for the float sums)
        assert d * err > 0 and abs(d - value) < 0.006, (err, spacing, d)


def test_library_exports_the_weighted_tracking_entry_points(lib_path):
    syms = subprocess.check_output(["nm", "-D", "--defined-only", lib_path], text=True)
    names = {line.split()[-1] for line in syms.splitlines() if line.strip()}
    assert {"gpsx_track_epl_weighted", "gpsx_track_epl_weighted_dev"} <= names
    from stm32f4_sdr_gps_amd import capi
    assert callable(getattr(capi.Engine, "track_epl_weighted", None))


def test_weighted_tracking_kernel_has_no_scratch(lib_path):
    from stm32f4_sdr_gps_amd import build
    res = build.check_no_scratch()
    hits = [v for k, v in res.items() if "k_track_epl_weighted" in k]
    assert len(hits) == 1 and hits[0]["scratch_bytes"] == 0, hits
    assert 4096 <= hits[0]["lds_bytes"] <= 8192 and hits[0]["vgprs"] <= 128
