"""The weighted loop with a per-channel bit synchroniser and bit-aligned windows (EXTENSION, not in the reference: include/gpsx.h
gpsx_track_loop_weighted_sync; k_track_wsync on the vector ALU) against its exact CPU restatement (tests/weighted_sync_ref.py, pinned
in tests/test_weighted_sync_reference.py).  Every comparison is for equality, byte for byte, on records and on the full 448-byte
states: the case table of tests/weighted_sync_cases.py (channel counts that fill waves partly and leave waves idle, mixed initial
modes, both weights, spacings 1 / 8 / 15, four (n_coh_search, n_coh_lock) pairs; the table's ground -- accept, both rejections, a
channel leaving WAIT -- asserted on the restatement); the ragged sixteen-channels-per-wave shape with canaries; GPU against GPU where
the call must reduce to gpsx_track_loop_weighted_dev; split launches and the device variant; bad channels; refusals; and the
three-satellite scenario, truncated."""
import numpy as np
import pytest

import weighted_gpu as G
import weighted_loop_cases as S
import weighted_loop_ref as L
import weighted_sync_cases as K
import weighted_sync_ref as Y
from weighted_gpu import EINVAL, eng  # noqa: F401
from weighted_gpu import sync_cfg as _cfg

pytestmark = pytest.mark.gpu


def _stage(eng, blocks, st, cfg, dev=False, pieces=None):
    """the library on a copy of `st` in device memory -> ([(first block, records)], states after, [return codes]); dev: blocks and
    records in device memory too"""
    n_ch, c = len(st), _cfg(cfg)
    fn = eng.lib.gpsx_track_loop_weighted_sync_dev if dev else eng.lib.gpsx_track_loop_weighted_sync
    launches, firsts = G.block_launches(blocks, pieces, Y.REC_DTYPE, lambda k: (Y.slots(k, cfg), n_ch))

    def call(ins, sts, out, k):
        return fn(eng.h, c.ctypes.data, ins[0], len(launches[k][0][0]), sts[0], n_ch, out)
    recs, after, codes = G.run_stage(eng, call, b"k_track_wsync", st, launches, dev, host_inputs=True)
    return list(zip(firsts, recs)), after, codes


def _gpu(eng, blocks, st, cfg, dev=False, pieces=None):
    """_stage where no channel is bad -> ([(first block, records)], states after)"""
    recs, after, codes = _stage(eng, blocks, st, cfg, dev, pieces)
    assert not any(codes), (codes, eng.lib.gpsx_last_error(eng.h))
    return recs, after


def _same(rec, after, want_rec, want_st, channels, what):
    assert rec.dtype == Y.REC_DTYPE, what
    G.same_columns(rec, want_rec, (what, "records"), list(channels))
    G.same_rows(after, want_st, (what, "states"), list(channels))


@pytest.mark.parametrize("i", range(len(K.CASES)))
def test_records_and_states_match_the_restatement(eng, oracle, i):
    n_ch = K.CASES[i][0]
    assert S.tabled(n_ch) == 1
    blocks, st0, cfg, want, want_st, _ = K.case(oracle, i)
    recs, after = _gpu(eng, blocks, st0, cfg)
    _same(recs[0][1], after, want, want_st, range(n_ch), K.CASES[i])
    K.rekey(recs)      # (every slot: a window's record or the empty pattern)
    assert (want["flags"] & Y.F_WINDOW).sum() > n_ch * K.N_BLOCKS // 40


def test_the_case_table_stands_on_every_ground(oracle):
    seen = K.case_table_events(oracle)
    assert all(seen[k] for k in ("accept", "disagree", "ratio", "left_wait", "bit")), {k: len(v) for k, v in seen.items()}


def test_the_ragged_sixteen_channels_per_wave_shape(eng, oracle):
    """70003 channels (cpw 16, the last wave holds 3) over 48 blocks through the device entry point, modes and edges varying lane by
    lane (a state period of 61), canaries around states and records: 24 sampled channels against the restatement, every slot of
    every channel a window's record or the empty pattern, and equal states give equal results wherever they sit"""
    n_ch, k, period = 70003, 48, 61
    assert S.tabled(n_ch) == 16
    blocks = K.strong_blocks(k, seed=9)
    st, _ = K.tiled_states(n_ch, 61, period)
    st["search_n"] = np.where((st["mode"] == Y.SEARCH) & (st["search_n"] == 0), 30, st["search_n"])     # (fresh searches decide at block 9)
    cfg = Y.make_cfg(4, 20, S.PULL_IN, S.STEADY, 1, (5, 4))
    n_slots = Y.slots(k, cfg)
    recs, after = _gpu(eng, blocks, st, cfg, dev=True)
    rec = recs[0][1]
    last = S.ROWS[n_ch][2]
    rng = np.random.default_rng(n_ch)
    sample = sorted({0, 1, 15, 16, 63, 64, n_ch - 1, n_ch - last, n_ch - last - 1} | {int(x) for x in rng.integers(0, n_ch, 15)})
    want_st = st.copy()
    want = Y.run(oracle, blocks, want_st, cfg, channels=sample)
    _same(rec, after, want, want_st, sample, "ragged")
    # every slot of every channel: a window's record (flags, an end block inside the slot) or the empty pattern
    window = (rec["flags"] & Y.F_WINDOW) != 0
    span = 4
    lo = (np.arange(n_slots) * span)[:, None]
    assert (((rec["end_block"] >= lo) & (rec["end_block"] < lo + span)) | ~window).all() and ((rec["flags"] & ~np.uint32(7)) == 0).all()
    empty = Y.empty_records(1, 1)[0, 0].tobytes()
    flat, w = rec.reshape(-1), window.reshape(-1)
    assert all(flat[j].tobytes() == empty for j in np.nonzero(~w)[0][:20000:7]) and (rec["end_block"][~window] == -1).all()
    assert not rec["w"]["iq"][~window].any() and not rec["bit_ip"][~window].any() and 0.2 < window.mean() < 0.9
    # the state period: channel c's results are channel c % 61's, wherever its lane, wave and workgroup
    idx = np.arange(n_ch) % period
    assert rec.tobytes() == np.ascontiguousarray(rec[:, idx]).tobytes() and after.tobytes() == after[idx].tobytes()
    modes = after["mode"][:period]
    assert {int(m) for m in modes} == {Y.SEARCH, Y.WAIT, Y.LOCKED} or {int(m) for m in modes} == {Y.SEARCH, Y.LOCKED}


def _wloop(eng, blocks, loop_st, n_coh, gains):
    """gpsx_track_loop_weighted_dev on a copy of the 40-byte states -> (records, states after)"""
    from stm32f4_sdr_gps_amd import capi
    c = capi.wloop_cfg(n_coh, True, 8, gains["dll"], gains["pll"], gains["fll"])

    def call(ins, sts, out, k):
        return eng.lib.gpsx_track_loop_weighted_dev(eng.h, c.ctypes.data, ins[0], len(blocks), sts[0], len(loop_st), out)
    recs, after, codes = G.run_stage(eng, call, b"k_track_wloop", loop_st, [([blocks], L.REC_DTYPE, (len(blocks) // n_coh, len(loop_st)))])
    assert codes == [0]
    return recs[0], after


@pytest.mark.parametrize("n,gains", [(1, S.REFERENCE_1MS), (4, S.PULL_IN), (20, S.STEADY)])
def test_locked_at_the_launchs_grid_is_the_existing_loop(eng, n, gains):
    """GPU against GPU, 257 channels: every channel preset LOCKED with edge = ms_count = 0 and n_coh_search = n_coh_lock = n"""
    blocks = K.strong_blocks(40)
    st = K.mixed_states(257, 7, kinds=[0])
    st["mode"] = Y.LOCKED
    want, want_st = _wloop(eng, blocks, np.ascontiguousarray(st["loop"]), n, gains)
    recs, after = _gpu(eng, blocks, st, Y.make_cfg(n, n, gains, gains, 1, (5, 4)))
    rec = recs[0][1]
    assert np.ascontiguousarray(rec["w"]).tobytes() == want.tobytes() and np.ascontiguousarray(after["loop"]).tobytes() == want_st.tobytes()
    per_bit = 20 // n
    for u in range(rec.shape[0]):
        is_bit = u % per_bit == per_bit - 1
        assert (rec["flags"][u] == (Y.F_WINDOW | Y.F_LOCKED | (Y.F_BIT if is_bit else 0))).all() and (rec["end_block"][u] == (u + 1) * n - 1).all()
        assert np.array_equal(rec["bit_ip"][u], want["iq"][u + 1 - per_bit:u + 1, :, 2].sum(axis=0) if is_bit else np.zeros(257, np.int32))
    assert want["iq"].any() and not np.array_equal(after["loop"]["code_phase_fine"], st["loop"]["code_phase_fine"])


def test_a_search_before_its_first_decision_is_the_existing_loop(eng):
    blocks = K.strong_blocks(36)
    st = K.mixed_states(257, 8, kinds=[0])
    want, want_st = _wloop(eng, blocks, np.ascontiguousarray(st["loop"]), 4, S.PULL_IN)
    recs, after = _gpu(eng, blocks, st, Y.make_cfg(4, 20, S.PULL_IN, S.STEADY, 1, (5, 4)))
    rec = recs[0][1]
    assert np.ascontiguousarray(rec["w"]).tobytes() == want.tobytes() and np.ascontiguousarray(after["loop"]).tobytes() == want_st.tobytes()
    assert (rec["flags"] == Y.F_WINDOW).all() and (after["search_n"] == 36).all() and (after["sync_rounds"] == 0).all()


def test_split_launches_and_both_variants(eng, oracle):
    """130 blocks in launches of 37 / 1 / 92 = one launch of 130 = the device variant: states identical, records identical once
    keyed by the absolute end block; and all of it the restatement's"""
    blocks, st0, cfg, want, want_st, _ = K.case(oracle, 2)       # (20, 5): windows of either mode cross the cuts
    one = _gpu(eng, blocks, st0, cfg)
    _same(one[0][0][1], one[1], want, want_st, range(len(st0)), "one launch")
    whole = K.rekey(one[0])
    for what, got in (("split", _gpu(eng, blocks, st0, cfg, pieces=[37, 1, 92])), ("device", _gpu(eng, blocks, st0, cfg, dev=True)),
                      ("device, split", _gpu(eng, blocks, st0, cfg, dev=True, pieces=[37, 1, 92]))):
        assert got[1].tobytes() == one[1].tobytes(), what
        assert K.rekey(got[0]) == whole, what


def test_bad_channels(eng, oracle):
    """a PRN of 0, a NaN code phase, mode = 7, ms_count = 20 and edge = -1 in LOCKED among good channels, canaries around states and
    records: the good channels are the restatement's, the bad ones get empty slots, keep every word but the accumulator;
    GPSX_EINVAL comes from the host variant itself and from the next synchronize after the device variant"""
    blocks = K.strong_blocks(45)
    st0, bad = K.bad_channel_states()
    n_ch = len(st0)
    good = [c for c in range(n_ch) if c not in bad]
    cfg = Y.make_cfg(4, 20, S.PULL_IN, S.STEADY, 1, (5, 4))
    want_st = st0.copy()
    want = Y.run(oracle, blocks, want_st, cfg)
    assert (want["flags"][:, sorted(bad)] == 0).all() and (want["flags"][:, good] != 0).any(axis=0).all()
    for dev in (False, True):
        recs, after, codes = _stage(eng, blocks, st0, cfg, dev)
        assert codes == [EINVAL], dev
        if dev:
            assert eng.lib.gpsx_synchronize(eng.h) == 0
        else:
            assert b"prn" in eng.lib.gpsx_last_error(eng.h)
        _same(recs[0][1], after, want, want_st, range(n_ch), ("device" if dev else "host"))
    recs, after = _gpu(eng, blocks, st0[good].copy(), cfg)      # the same channels without the bad ones: no error
    assert recs[0][1].tobytes() == np.ascontiguousarray(want[:, good]).tobytes() and after.tobytes() == want_st[good].tobytes()


def test_argument_checks_write_nothing(eng):
    blocks = K.strong_blocks(8)
    st0 = K.mixed_states(4, 9)
    good = dict(cfg={}, null_cfg=False, null_if=False, null_st=False, null_out=False, n_blocks=8, n_ch=4)
    nan, inf = float("nan"), float("inf")
    # every refusal with its exact text; the last row of a group fails a later clause as well: the first failing clause decides
    by_message = {
        b"null argument": [dict(null_cfg=True), dict(null_if=True), dict(null_st=True), dict(null_out=True), dict(null_st=True, n_blocks=0)],
        b"unknown weights": [dict(cfg=dict(weights=2)), dict(cfg=dict(weights=-1)), dict(cfg=dict(weights=2), n_blocks=0), dict(cfg=dict(weights=2, spacing=0))],
        b"spacing must be 1..15 samples": [dict(cfg=dict(spacing=0)), dict(cfg=dict(spacing=16)), dict(cfg=dict(spacing=16, n_coh_lock=8))],
        b"n_coh_search and n_coh_lock must be 1, 2, 4, 5, 10 or 20 blocks": [
            dict(cfg=dict(n_coh_search=0)), dict(cfg=dict(n_coh_search=3)), dict(cfg=dict(n_coh_search=40)), dict(cfg=dict(n_coh_lock=-20)),
            dict(cfg=dict(n_coh_lock=8)), dict(cfg=dict(n_coh_lock=21)), dict(cfg=dict(n_coh_lock=8, sync_bits=0))],
        b"sync_bits must be 1..200": [dict(cfg=dict(sync_bits=0)), dict(cfg=dict(sync_bits=201)), dict(cfg=dict(sync_bits=0, sync_den=0))],
        b"sync_num and sync_den must be 1..1024": [dict(cfg=dict(sync_num=0, sync_den=0)), dict(cfg=dict(sync_num=1025)), dict(cfg=dict(sync_den=0)),
                                                   dict(cfg=dict(sync_num=2000, sync_den=1025)), dict(cfg=dict(sync_num=4, sync_den=1025))],
        b"sync_num must not be below sync_den": [dict(cfg=dict(sync_num=4, sync_den=5)), dict(cfg=dict(sync_num=4, sync_den=5), n_blocks=0)],
        b"n_blocks must be 1..4096": [dict(n_blocks=0), dict(n_blocks=-4), dict(n_blocks=4097), dict(n_blocks=0, n_ch=0)],
        b"n_ch must be at least 1": [dict(n_ch=0), dict(n_ch=-3), dict(n_ch=0, cfg={("lock", "fll_c"): inf})],
        b"a loop gain is not finite": [dict(cfg={(which, field): value}) for which in ("search", "lock")
                                       for field, value in (("dll_c1", nan), ("dll_c2", inf), ("pll_c1", -inf), ("pll_c2", nan), ("fll_c", inf))],
    }
    n_rec = 2 * 4 * Y.REC_DTYPE.itemsize
    with G.Pool() as pool:
        d_st, d_if = pool.add(G.Guarded(eng, st0.nbytes, G.STATE_FILL, st0)), pool.add(G.Guarded(eng, blocks.nbytes, G.STATE_FILL, blocks))
        outs = {True: pool.add(G.Guarded(eng, n_rec)), False: pool.add(G.Guarded(None, n_rec))}

        def call(a, dev):
            cfg = _cfg(Y.make_cfg(4, 20, S.PULL_IN, S.STEADY, 20, (5, 4)))
            for key, value in a["cfg"].items():
                if isinstance(key, tuple):
                    cfg[key[0]][key[1]] = value
                else:
                    cfg[key] = value
            fn = eng.lib.gpsx_track_loop_weighted_sync_dev if dev else eng.lib.gpsx_track_loop_weighted_sync
            return fn(eng.h, None if a["null_cfg"] else cfg.ctypes.data, None if a["null_if"] else (d_if.ptr if dev else blocks.ctypes.data),
                      a["n_blocks"], None if a["null_st"] else d_st.ptr, a["n_ch"], None if a["null_out"] else outs[dev].ptr)
        G.refusals(eng, by_message, good, call, [d_st, *outs.values()])


def test_the_scenario_truncated(eng, oracle):
    """seed 1's three channels over the first 1100 ms in launches of 200 (the last of 100): equal to the restatement launch by
    launch, every channel locked on its own edge, and 0 errors on the BIT records after lock"""
    n_ms = 1100
    blocks, bits = K.scenario(1, n_ms)
    cfg = K.sync_cfg()
    pieces = [200] * 5 + [100]
    want_st = K.handover_states(1)
    want, at = [], 0
    for k in pieces:
        want.append((at, Y.run(oracle, blocks[at:at + k], want_st, cfg)))
        at += k
    st, recs, at = K.handover_states(1), [], 0
    with G.Guarded(eng, st.nbytes, G.STATE_FILL, st) as d_st:      # (the host variant as Engine.track_loop_weighted_sync makes it)
        for k in pieces:
            recs.append((at, eng.track_loop_weighted_sync(blocks[at:at + k], d_st.ptr.value, 3, _cfg(cfg))))
            assert eng.lib.gpsx_last_kernel(eng.h) == b"k_track_wsync"
            at += k
        after = d_st.get(st.dtype, st.shape)
    for (at, g), (_, w) in zip(recs, want):
        assert g.tobytes() == w.tobytes(), at
    assert after.tobytes() == want_st.tobytes()
    for ch in range(3):
        assert int(after["mode"][ch]) == Y.LOCKED and int(after["edge"][ch]) == K.EDGES_FOUND[ch] and int(after["sync_rounds"][ch]) == 2
        errors, n_bits = K.bit_errors(Y.bits_after_lock([(at, r[:, ch]) for at, r in recs]), bits[ch], K.EDGES_FOUND[ch])
        print("channel", ch, "edge", int(after["edge"][ch]), "bit errors", errors, "of", n_bits)
        assert errors == 0 and n_bits >= 12
