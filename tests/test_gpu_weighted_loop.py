"""The closed DLL / Costas PLL / FLL on weighted two-bit samples (EXTENSION, not in the reference: include/gpsx.h
gpsx_track_loop_weighted; k_track_wloop on the vector ALU) against its exact CPU restatement (tests/weighted_loop_ref.py, pinned in
tests/test_weighted_loop_reference.py).  Every comparison is for equality, byte for byte, on records and final states: channel
counts that fill waves partly and fully and leave waves of a workgroup idle, every channels-per-wave value the plan can choose
(tests/weighted_loop_cases.py, asserted without a GPU in tests/test_track_loop_weighted_plan.py), n_coh 1 / 4 / 10 / 20, both
weights, spacings 1 / 8 / 15, a non-default IF, a few hundred blocks; with gains 0 the window sums against
gpsx_track_epl_weighted_dev on every channel (GPU against GPU); split launches against one; the device against the host variant;
the exact handover from a coherent grid's record; bad channels and refusals, with canaries; the pull-in scenario, truncated; and
the branches of the update that the state alone can force (tests/weighted_forced_cases.py wloop_table)."""
import math

import numpy as np
import pytest

import weighted_forced_cases as W
import weighted_gpu as G
import weighted_loop_cases as S
import weighted_loop_ref as L
from weighted_gpu import EINVAL, eng  # noqa: F401

pytestmark = pytest.mark.gpu


def _blocks(n, amp=0.3, seed=3):
    from stm32f4_sdr_gps_amd import synth
    sats = [synth.Sat(7, 1310.0, 4321.0, amp, 0.4), synth.Sat(19, -2240.0, 12007.0, amp, 2.0), synth.Sat(30, 2018.0, 13000.0, amp, 4.0)]
    return synth.make_if_static(n, sats, noise_amp=1.0, seed=seed, two_bit=True)


# code phases on the seam (tau -+ spacing wraps on either side for every spacing; an update can carry them across either end)
PHASES = [4321.0, 0.0, 7.9, 16367.99, 3.0, 16365.0, 0.5, 14.0, 16353.0, 12007.25, 1.0, 16367.0, 15.0, 16352.5, 0.25, 16366.5]
PRNS = [7, 19, 30, 1, 33, 64, 150, 210, 32, 209, 5, 100]


def _states(n, seed):
    rng = np.random.default_rng(seed)
    st = np.zeros(n, L.STATE_DTYPE)
    idx = np.arange(n)
    st["prn"] = np.where(idx < 3 * len(PRNS), np.array(PRNS)[idx % len(PRNS)], rng.integers(1, 211, n))
    st["code_phase_fine"] = np.where(idx < 2 * len(PHASES), np.array(PHASES, np.float32)[idx % len(PHASES)], rng.uniform(0.0, 16367.0, n).astype(np.float32))
    st["if_freq_offset_hz"] = np.where(idx % 3 == 0, rng.integers(-5000, 5001, n), rng.uniform(-5000.0, 5000.0, n))
    st["if_freq_offset_hz"][:3] = [1310.0, -2240.0, 2018.0][:n]
    st["if_freq_accum"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    st["if_freq_accum"][::5] = 0
    half = idx % 2 == 1                                   # every other channel arrives with a loop memory
    st["dll_err"] = np.where(half, rng.uniform(-0.5, 0.5, n), 0.0)
    st["pll_err"] = np.where(half, rng.uniform(-0.2, 0.2, n), 0.0)
    st["prev_ip"] = np.where(half, rng.integers(-30000, 30001, n), 0)
    st["prev_qp"] = np.where(half, rng.integers(-30000, 30001, n), 0)
    st["n_updates"] = np.where(half, rng.integers(1, 1000, n), 0)
    return st


def _cfg(c):
    from stm32f4_sdr_gps_amd import capi
    return capi.wloop_cfg(c["n_coh"], c["use_magnitude"], c["spacing"], (c["dll_c1"], c["dll_c2"]), (c["pll_c1"], c["pll_c2"]), c["fll_c"])


def _stage(eng, blocks, st, cfg, dev=False, pieces=None):
    """the library on a copy of `st` in device memory -> (records, states after, [return codes]); dev: blocks and records in device memory too"""
    n_ch, c = len(st), _cfg(cfg)
    fn = eng.lib.gpsx_track_loop_weighted_dev if dev else eng.lib.gpsx_track_loop_weighted
    launches, _ = G.block_launches(blocks, pieces, L.REC_DTYPE, lambda k: (k // cfg["n_coh"], n_ch))

    def call(ins, sts, out, k):
        return fn(eng.h, c.ctypes.data, ins[0], len(launches[k][0][0]), sts[0], n_ch, out)
    recs, after, codes = G.run_stage(eng, call, b"k_track_wloop", st, launches, dev, host_inputs=True)
    return np.concatenate(recs), after, codes


def _gpu(eng, blocks, st, cfg, dev=False, pieces=None):
    """_stage where no channel is bad -> (records, states after)"""
    rec, after, codes = _stage(eng, blocks, st, cfg, dev, pieces)
    assert not any(codes), (codes, eng.lib.gpsx_last_error(eng.h))
    return rec, after


def _same(rec, after, want_rec, want_st, channels, what):
    assert rec.dtype == L.REC_DTYPE, what
    G.same_columns(rec, want_rec, (what, "records"), list(channels))
    G.same_rows(after, want_st, (what, "states"), list(channels))


MOVING = dict(dll=(1.0, 100.0), pll=(56.0, 1600.0), fll=0.1)

# (channels, blocks, n_coh, use_magnitude, spacing, gains): every channel is restated
SMALL = [(1, 1, 1, True, 8, MOVING), (3, 8, 4, False, 1, MOVING), (5, 20, 10, True, 15, S.STEADY), (64, 40, 20, True, 8, S.STEADY),
         (257, 12, 4, False, 15, MOVING), (64, 6, 1, True, 1, S.REFERENCE_1MS), (3, 40, 20, False, 8, S.STEADY), (5, 30, 10, False, 1, MOVING)]


@pytest.mark.parametrize("n_ch,n_blocks,n_coh,use_mag,spacing,gains", SMALL)
def test_records_and_states_match_the_restatement(eng, oracle, n_ch, n_blocks, n_coh, use_mag, spacing, gains):
    assert S.tabled(n_ch) == 1
    blocks = _blocks(40)[:n_blocks]
    st = _states(n_ch, 100 * n_ch + n_blocks)
    cfg = L.make_cfg(n_coh, use_mag, spacing, gains["dll"], gains["pll"], gains["fll"])
    want_st = st.copy()
    want = L.run(oracle, blocks, want_st, cfg)
    rec, after = _gpu(eng, blocks, st, cfg)
    _same(rec, after, want, want_st, range(n_ch), (n_ch, n_blocks, n_coh, use_mag, spacing))
    assert not np.array_equal(after["code_phase_fine"], st["code_phase_fine"])


@pytest.mark.parametrize("n_ch", [r[0] for r in S.SHAPES if r[0] > 257])
def test_every_channels_per_wave_value(eng, oracle, n_ch):
    """cpw 2 .. 16 through the device entry point, canaries around records and states: 24 sampled channels (the first, the last,
    the ragged last wave's and the wave boundaries among them) against the restatement over 8 blocks in windows of 4, all of them
    against gpsx_track_epl_weighted_dev's sums with gains 0"""
    from stm32f4_sdr_gps_amd import capi
    cpw = S.tabled(n_ch)
    k, n_coh = 8, 4
    use_mag, spacing = cpw % 2 == 0, (1, 8, 15)[cpw % 3]
    blocks = _blocks(8, seed=cpw)
    st = _states(n_ch, n_ch)
    rng = np.random.default_rng(n_ch)
    last = S.ROWS[n_ch][2]
    sample = sorted({0, 1, cpw - 1, cpw, 4 * cpw - 1, 4 * cpw, n_ch - 1, n_ch - last, max(0, n_ch - last - 1)} | {int(c) for c in rng.integers(0, n_ch, 15)})
    for gains in (MOVING, dict(dll=(0.0, 0.0), pll=(0.0, 0.0), fll=0.0)):
        cfg = L.make_cfg(n_coh, use_mag, spacing, gains["dll"], gains["pll"], gains["fll"])
        rec, after = _gpu(eng, blocks, st, cfg, dev=True)
        trk = np.zeros(n_ch, capi.TRK_DTYPE)
        for f in trk.dtype.names:
            trk[f] = st[f]
        ocfg = np.array([1 if use_mag else 0, spacing], np.int32)
        with G.Guarded(eng, blocks.nbytes, G.STATE_FILL, blocks) as d_if, G.Guarded(eng, trk.nbytes, G.STATE_FILL, trk) as d_trk, \
                G.Guarded(eng, k * n_ch * 6 * 4) as d_iq:
            eng._chk(eng.lib.gpsx_track_epl_weighted_dev(eng.h, ocfg.ctypes.data, d_if.ptr, k, d_trk.ptr, n_ch, d_iq.ptr), "gpsx_track_epl_weighted_dev")
            eng.synchronize()
            iq, trk = d_iq.get(np.int32, (k, n_ch, 6)), d_trk.get(trk.dtype, trk.shape)
        want_st = st.copy()
        want = L.run(oracle, blocks, want_st, cfg, channels=sample)
        _same(rec, after, want, want_st, sample, (n_ch, cpw, gains is MOVING))
        if gains is not MOVING:      # GPU against GPU, every channel: the open-loop correlators' sums, floats untouched, accumulators
            sums = iq.astype(np.int64).reshape(k // n_coh, n_coh, n_ch, 6).sum(axis=1)
            assert np.array_equal(rec["iq"], sums) and np.count_nonzero(sums) > 0.9 * sums.size
            assert np.array_equal(after["if_freq_accum"], trk["if_freq_accum"])
            for f in ("prn", "code_phase_fine", "if_freq_offset_hz", "reserved"):
                assert after[f].tobytes() == st[f].tobytes(), f
            assert np.array_equal(after["n_updates"], st["n_updates"] + k // n_coh)


def test_non_default_if(oracle):
    from stm32f4_sdr_gps_amd import capi
    blocks = _blocks(8, seed=8)
    st = _states(5, 5)
    cfg = L.make_cfg(4, True, 8, **MOVING)
    want_st = st.copy()
    want = L.run(oracle, blocks, want_st, cfg, if_hz=4_100_000)
    e = capi.Engine(0)
    try:
        e.set_config(if_hz=4_100_000)
        rec, after = _gpu(e, blocks, st, cfg)
    finally:
        e.close()
    _same(rec, after, want, want_st, range(5), "if_hz")


def test_a_few_hundred_blocks_split_launches_and_both_variants(eng, oracle):
    """240 blocks, 3 channels: one launch = launches of 40 / 120 / 80 = the device variant, all equal to the restatement"""
    blocks = _blocks(240, seed=6)
    st = _states(3, 42)
    for n_coh, gains in ((20, S.STEADY), (4, MOVING), (1, S.REFERENCE_1MS)):
        cfg = L.make_cfg(n_coh, True, 8, gains["dll"], gains["pll"], gains["fll"])
        want_st = st.copy()
        want = L.run(oracle, blocks, want_st, cfg)
        one = _gpu(eng, blocks, st, cfg)
        _same(*one, want, want_st, range(3), ("one launch", n_coh))
        for what, got in (("split", _gpu(eng, blocks, st, cfg, pieces=[40, 120, 80])), ("device", _gpu(eng, blocks, st, cfg, dev=True)),
                          ("device, split", _gpu(eng, blocks, st, cfg, dev=True, pieces=[100, 140]))):
            assert got[0].tobytes() == one[0].tobytes() and got[1].tobytes() == one[1].tobytes(), (what, n_coh)


def test_a_coherent_grid_record_hands_over_exactly(eng):
    """GPU against GPU: the best record of the coherent grid (n_coh = 10) fills the first four fields of a zeroed state -- phase ->
    code_phase_fine, bin -> if_freq_offset_hz, accumulator 0 -- and the first window's floor(sqrt(IP^2 + QP^2)) IS the record's
    max_val, whatever the gains (the record is written after the update, its sums were formed before)"""
    from stm32f4_sdr_gps_amd import synth
    blocks = synth.cold_start_block(20, seed=11, amp_scale=0.03, two_bit=True)
    pk = eng.acq_grid_weighted_coh(blocks[:10], np.array([14], np.uint8), 1, 10, 3800, 50, 11)
    d = int(pk[0, 0, :]["max_val"].argmax())
    max_val, phase, dopp = int(pk[0, 0, d]["max_val"]), int(pk[0, 0, d]["phase"]), 3800 + 50 * d
    st = L.handover(14, float(phase), float(dopp))
    rec, after = _gpu(eng, blocks, st, L.make_cfg(10, True, 8, **MOVING))
    ip, qp = int(rec["iq"][0, 0, 2]), int(rec["iq"][0, 0, 3])
    print("coherent record", max_val, "at phase", phase, "bin", dopp, "Hz; first window's prompt", ip, qp)
    assert math.isqrt(ip * ip + qp * qp) == max_val and max_val > 3000
    assert after["n_updates"][0] == 2 and (after["prev_ip"][0], after["prev_qp"][0]) == (rec["iq"][1, 0, 2], rec["iq"][1, 0, 3])


def test_argument_checks_write_nothing(eng):
    from stm32f4_sdr_gps_amd import capi
    blocks = _blocks(8)
    st0 = _states(4, 9)
    good = dict(cfg=dict(n_coh=4), null_cfg=False, null_if=False, null_st=False, null_out=False, n_blocks=8, n_ch=4)
    nan, inf = float("nan"), float("inf")
    # every refusal with its exact text; the last row of a group fails a later clause as well: the first failing clause decides
    by_message = {
        b"null argument": [dict(null_cfg=True), dict(null_if=True), dict(null_st=True), dict(null_out=True), dict(null_out=True, n_ch=0)],
        b"unknown weights": [dict(cfg=dict(n_coh=4, weights=2)), dict(cfg=dict(n_coh=4, weights=-1)), dict(cfg=dict(n_coh=4, weights=2), n_blocks=0),
                             dict(cfg=dict(n_coh=4, weights=2, spacing=0))],
        b"spacing must be 1..15 samples": [dict(cfg=dict(n_coh=4, spacing=0)), dict(cfg=dict(n_coh=4, spacing=16)), dict(cfg=dict(n_coh=0, spacing=16))],
        b"n_coh must be 1..20 blocks": [dict(cfg=dict(n_coh=0)), dict(cfg=dict(n_coh=-4)), dict(cfg=dict(n_coh=21)), dict(cfg=dict(n_coh=21), n_blocks=0)],
        b"n_blocks must be 1..4096": [dict(n_blocks=0), dict(n_blocks=-4), dict(n_blocks=4100), dict(n_blocks=4098, n_ch=0)],
        b"n_blocks must be a multiple of n_coh": [dict(cfg=dict(n_coh=3)), dict(cfg=dict(n_coh=16)), dict(n_blocks=6), dict(n_blocks=6, n_ch=0)],
        b"n_ch must be at least 1": [dict(n_ch=0), dict(n_ch=-3), dict(n_ch=0, cfg=dict(n_coh=4, fll=inf))],
        b"a loop gain is not finite": [dict(cfg=dict(n_coh=4, dll=(nan, 1.0))), dict(cfg=dict(n_coh=4, dll=(1.0, inf))), dict(cfg=dict(n_coh=4, pll=(-inf, 1.0))),
                                       dict(cfg=dict(n_coh=4, pll=(1.0, nan))), dict(cfg=dict(n_coh=4, fll=inf))],
    }
    with G.Pool() as pool:
        d_st, d_if = pool.add(G.Guarded(eng, st0.nbytes, G.STATE_FILL, st0)), pool.add(G.Guarded(eng, blocks.nbytes, G.STATE_FILL, blocks))
        outs = {True: pool.add(G.Guarded(eng, 2 * 4 * L.REC_DTYPE.itemsize)), False: pool.add(G.Guarded(None, 2 * 4 * L.REC_DTYPE.itemsize))}

        def call(a, dev):
            c = a["cfg"]
            cfg = capi.wloop_cfg(c["n_coh"], True, c.get("spacing", 8), c.get("dll", (1.0, 100.0)), c.get("pll", (56.0, 1600.0)), c.get("fll", 0.1))
            if "weights" in c:
                cfg["weights"] = c["weights"]
            fn = eng.lib.gpsx_track_loop_weighted_dev if dev else eng.lib.gpsx_track_loop_weighted
            return fn(eng.h, None if a["null_cfg"] else cfg.ctypes.data, None if a["null_if"] else (d_if.ptr if dev else blocks.ctypes.data),
                      a["n_blocks"], None if a["null_st"] else d_st.ptr, a["n_ch"], None if a["null_out"] else outs[dev].ptr)
        G.refusals(eng, by_message, good, call, [d_st, *outs.values()])


def test_bad_channels(eng, oracle):
    """PRN 0, 211 and -7, a NaN code phase and one of magnitude 2^24 among good channels, canaries around states and records: the
    good channels are the restatement's, the bad ones get zero sums, keep floats and loop memory and have their accumulator
    advanced; GPSX_EINVAL comes from the host variant itself and from the next synchronize after the device variant"""
    blocks = _blocks(12)
    st0 = _states(12, 4)
    bad = {2: ("prn", 0), 5: ("prn", 211), 7: ("code_phase_fine", np.nan), 11: ("code_phase_fine", -16777216.0), 8: ("prn", -7)}
    for ch, (field, value) in bad.items():
        st0[field][ch] = value
    good = [c for c in range(12) if c not in bad]
    cfg = L.make_cfg(4, True, 8, **MOVING)
    want_st = st0.copy()
    want = L.run(oracle, blocks, want_st, cfg)
    assert not want["iq"][:, sorted(bad)].any() and want["iq"][:, good].any(axis=(0, 2)).all()
    for ch in bad:
        for f in ("code_phase_fine", "if_freq_offset_hz", "dll_err", "pll_err", "prev_ip", "prev_qp", "n_updates"):
            assert want_st[f][ch:ch + 1].tobytes() == st0[f][ch:ch + 1].tobytes()
        assert want_st["if_freq_accum"][ch] != st0["if_freq_accum"][ch]
    for dev in (False, True):
        rec, after, codes = _stage(eng, blocks, st0, cfg, dev)
        assert codes == [EINVAL], dev
        if dev:
            assert eng.lib.gpsx_synchronize(eng.h) == 0
        else:
            assert b"prn" in eng.lib.gpsx_last_error(eng.h)
        _same(rec, after, want, want_st, range(12), ("device" if dev else "host"))
    rec, after = _gpu(eng, blocks, st0[good].copy(), cfg)      # the same channels without the bad ones: no error
    assert rec.tobytes() == np.ascontiguousarray(want[:, good]).tobytes() and after.tobytes() == want_st[good].tobytes()


def test_the_pull_in_scenario_truncated(eng, oracle):
    """tests/test_weighted_loop_reference.py's scenario at its amplitude, the three seeds' handovers as three channels on seed 1's
    blocks: 200 ms of pull-in (n_coh = 4, frequency loop) and 400 ms of steady state (n_coh = 20) on the same state array, equal to
    the restatement, and the 20 bits after pull-in are read on every channel"""
    n_ms = 600
    blocks, bits = S.scenario(S.AMPLITUDE, 1, n_ms)
    st = np.concatenate([S.handover_state(seed) for seed in S.SEEDS])
    want_st = st.copy()
    want = [L.run(oracle, blocks[:S.PULL_IN_MS], want_st, L.make_cfg(**S.PULL_IN)), L.run(oracle, blocks[S.PULL_IN_MS:], want_st, L.make_cfg(**S.STEADY))]
    with G.Guarded(eng, st.nbytes, G.STATE_FILL, st) as d_st:
        got = [eng.track_loop_weighted(blocks[:S.PULL_IN_MS], d_st.ptr.value, 3, **S.PULL_IN),
               eng.track_loop_weighted(blocks[S.PULL_IN_MS:], d_st.ptr.value, 3, **S.STEADY)]
        after = d_st.get(st.dtype, st.shape)
    for g, w in zip(got, want):
        assert g.tobytes() == w.tobytes()
    assert after.tobytes() == want_st.tobytes()
    for ch in range(3):
        recs = [(0, 4, got[0][:, ch:ch + 1]), (S.PULL_IN_MS, 20, got[1][:, ch:ch + 1])]
        errors, n_bits = S.bit_errors(recs, bits, S.PULL_IN_MS // 20, n_ms)
        print("channel", ch, "bit errors", errors, "of", n_bits, "code phase", after["code_phase_fine"][ch], "carrier", after["if_freq_offset_hz"][ch])
        assert errors == 0 and n_bits == 20


@pytest.mark.parametrize("n_ch", [257, 8195])
def test_the_branches_the_state_alone_can_force(eng, oracle, n_ch):
    """k_track_wloop's own copy of the update, two windows of one block (tests/weighted_forced_cases.py wloop_table; what the rows
    meet is asserted in tests/test_weighted_forced_reference.py): prev is the restatement's first-window prompt rotated, so that
    the FLL sees dot == 0 (a quarter turn either way, and prev = (0, 0) with n_updates > 0), cross == 0 with dot < 0, and cross / dot
    well on either side of 7/16, 11/16, 19/16 and 39/16 in both signs; n_updates = 0xFFFFFFFF, whose second window skips the FLL;
    and phases with a dll_err that carry the code phase across either end.  The rows are tiled over cpw 1 and cpw 2 with a period
    coprime to the cpw; every channel's records and state are the restatement's.
    IP == 0, e2 + l2 == 0 and the outer arctangent intervals (below 2^-29, from 2^25 on) cannot be forced here: this kernel's
    state holds no open window, so its sums are whatever the samples give.  They are forced in k_track_wsync only, which carries
    the same update (tests/test_gpu_weighted_forced.py)."""
    cpw = S.tabled(n_ch)
    names, st0, want, want_st, _ = W.wloop_table(oracle)
    idx = W.tiled(n_ch, len(names), cpw)
    rec, after = _gpu(eng, W.blocks(W.WLOOP_BLOCKS), st0[idx].copy(), W.wloop_cfg(), dev=True)
    _same(rec, after, np.ascontiguousarray(want[:, idx]), want_st[idx].copy(), range(n_ch), (n_ch, [names[i] for i in idx[:len(names)]]))
