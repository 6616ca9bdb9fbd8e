"""The carrier-aided weighted loops (EXTENSION, not in the reference: include/gpsx.h gpsx_track_loop_weighted_aided and
gpsx_track_loop_weighted_sync_aided; k_track_waid_loop and k_track_waid_sync on the vector ALU) against their exact CPU restatement
(tests/weighted_aided_ref.py, pinned in tests/test_weighted_aided_reference.py).  Every comparison is for equality, byte for byte, on
records and on whole states: the three launch shapes of tests/weighted_aided_cases.py (every lane geometry of the launch plan) for
both loops and both variants, with code phases that the aiding step carries across either end of [0, 16368); a factor of 0 against
the unaided calls on the device; a stream cut into launches; bad channels; refusals; and the two scenarios the CPU test measures --
one satellite at +-4500 Hz over 2200 blocks and the first 8192 blocks of the orbit stream (the restatement of 4 x 8192 channel blocks
runs in four processes) -- which carry its numbers over to the device."""
import numpy as np
import pytest

import weighted_aided_cases as W
import weighted_aided_ref as A
import weighted_gpu as G
import weighted_loop_cases as S
import weighted_loop_ref as L
import weighted_pvt_cases as P
import weighted_sync_cases as K
import weighted_sync_ref as Y
from weighted_gpu import EINVAL, eng  # noqa: F401
from weighted_gpu import sync_cfg as _sync_cfg

pytestmark = pytest.mark.gpu


def _loop_cfg(c):
    from stm32f4_sdr_gps_amd import capi
    return capi.wloop_cfg(c["n_coh"], c["use_magnitude"], c["spacing"], (c["dll_c1"], c["dll_c2"]), (c["pll_c1"], c["pll_c2"]), c["fll_c"])


def _call(eng, sync, aided, dev):
    name = "gpsx_track_loop_weighted" + ("_sync" if sync else "") + ("_aided" if aided else "") + ("_dev" if dev else "")
    return name, getattr(eng.lib, name)


def _stage(eng, blocks, st, cfg, code_per_hz, dev, pieces=None):
    """the library on a copy of `st` in device memory -> ([(first block, records)], states after, [return codes]).  cfg: a
    restatement's dict, of either loop (told by the states' dtype); code_per_hz None: the unaided call; dev: blocks and records in
    device memory too"""
    from stm32f4_sdr_gps_amd import capi
    sync = st.dtype == Y.STATE_DTYPE
    assert sync or st.dtype == L.STATE_DTYPE
    n_ch = len(st)
    c = _sync_cfg(cfg) if sync else _loop_cfg(cfg)
    aid = None if code_per_hz is None else capi.waid(code_per_hz)
    _, fn = _call(eng, sync, aid is not None, dev)
    kernel = ("k_track_waid_sync" if sync else "k_track_waid_loop") if aid is not None else ("k_track_wsync" if sync else "k_track_wloop")
    launches, firsts = G.block_launches(blocks, pieces, Y.REC_DTYPE if sync else L.REC_DTYPE,
                                        lambda k: (Y.slots(k, cfg) if sync else k // cfg["n_coh"], n_ch))

    def call(ins, sts, out, k):
        args = [eng.h, c.ctypes.data] + ([aid.ctypes.data] if aid is not None else [])
        return fn(*args, ins[0], len(launches[k][0][0]), sts[0], n_ch, out)
    recs, after, codes = G.run_stage(eng, call, kernel.encode(), st, launches, dev, host_inputs=True)
    return list(zip(firsts, recs)), after, codes


def _gpu(eng, blocks, st, cfg, code_per_hz, dev, pieces=None):
    """_stage where no channel is bad -> ([(first block, records)], states after)"""
    recs, after, codes = _stage(eng, blocks, st, cfg, code_per_hz, dev, pieces)
    assert not any(codes), (codes, eng.lib.gpsx_last_error(eng.h))
    return recs, after


def _same(rec, after, want_rec, want_st, what):
    G.same_columns(rec, want_rec, (what, "records"))
    G.same_rows(after, want_st, (what, "states"))


# ---- 6: records and whole states, every lane geometry, both loops, both variants ---------------------------------------------------
@pytest.mark.parametrize("dev", [True, False], ids=["dev", "host"])
@pytest.mark.parametrize("what", ["sync", 0, 1], ids=["sync48", "loop40x20", "loop3x1"])
@pytest.mark.parametrize("n_ch", [r[0] for r in W.SHAPES])
def test_records_and_states_match_the_restatement(eng, oracle, n_ch, what, dev):
    assert W.tabled(n_ch) == W.ROWS[n_ch][0]      # (the compiled plan header's cpw and geometry are the table's row)
    blocks, st0, cfg, want, want_st = W.parity_case(oracle, what, n_ch)
    recs, after = _gpu(eng, blocks, st0, cfg, A.WAID_L1CA, dev)
    _same(recs[0][1], after, want, want_st, (n_ch, what, dev))
    flags = want["flags"] if what == "sync" else None
    assert want_st.tobytes() != st0.tobytes() and (flags is None or (flags & Y.F_WINDOW).sum() > n_ch)


def test_the_parity_states_stand_on_every_ground(oracle):
    """wraps that the aiding term causes, in both directions; modes mixed; offsets of both signs up to 5 kHz"""
    seen = W.seam_wraps(oracle)
    assert seen["down"] and seen["up"], seen
    st, _ = W.parity_states(W.DISTINCT, 41)
    hz = st["loop"]["if_freq_offset_hz"]
    assert {int(m) for m in st["mode"]} == {Y.SEARCH, Y.WAIT, Y.LOCKED} and hz.min() <= -4800.0 and hz.max() >= 4800.0 and np.abs(hz).max() <= 5000.0
    assert (st["win_n"] > 0).any()


# ---- 7: a factor of 0 is the unaided call, on the device ---------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["sync", 0], ids=["sync", "loop"])
def test_a_zero_factor_returns_the_unaided_calls_bytes(eng, oracle, what):
    n_ch = 7
    blocks, st0, cfg, _, _ = W.parity_case(oracle, what, n_ch)
    plain = _gpu(eng, blocks, st0, cfg, None, True)
    for dev in (True, False):
        zero = _gpu(eng, blocks, st0, cfg, 0.0, dev)
        assert zero[0][0][1].tobytes() == plain[0][0][1].tobytes() and zero[1].tobytes() == plain[1].tobytes(), (what, dev)
    aided = _gpu(eng, blocks, st0, cfg, A.WAID_L1CA, True)
    assert aided[1].tobytes() != plain[1].tobytes()


# ---- 8: a stream cut into launches ---------------------------------------------------------------------------------------------------
def test_split_launches_are_one_launch(eng, oracle):
    """130 blocks as 130 and as 37 + 1 + 92, aiding on: states identical, records identical once keyed by the absolute end block, all
    of it the restatement's; a channel leaves WAIT inside the second piece (its one block), others inside the first"""
    blocks = K.strong_blocks(W.SPLIT_BLOCKS)
    st0, cfg = W.split_states(), W.split_cfg()
    want_st = st0.copy()
    events = []
    want = A.run_sync(oracle, blocks, want_st, cfg, A.WAID_L1CA, events=events)
    assert (W.SPLIT_LEAVES_WAIT[0], W.SPLIT_LEAVES_WAIT[1], "locked") in events
    one = _gpu(eng, blocks, st0, cfg, A.WAID_L1CA, False)
    _same(one[0][0][1], one[1], want, want_st, "one launch")
    whole = K.rekey(one[0])
    for dev in (False, True):
        got = _gpu(eng, blocks, st0, cfg, A.WAID_L1CA, dev, pieces=list(W.SPLIT_PIECES))
        assert got[1].tobytes() == one[1].tobytes() and K.rekey(got[0]) == whole, dev


# ---- 9: bad channels -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sync", [True, False], ids=["sync", "loop"])
def test_bad_channels_take_no_step(eng, oracle, sync):
    """a PRN out of range, a NaN code phase and (sync) out-of-range sync words among good channels: the good channels are the
    restatement's, the bad ones keep every float -- no aiding step -- and advance their accumulator; GPSX_EINVAL comes from the host
    variant itself and from the next synchronize after the device variant"""
    blocks = K.strong_blocks(40)
    if sync:
        st0, bad = K.bad_channel_states()
        cfg = Y.make_cfg(4, 20, S.PULL_IN, S.STEADY, 1, (5, 4))
        want_st = st0.copy()
        want = A.run_sync(oracle, blocks, want_st, cfg, A.WAID_L1CA)
        loop0, loop1 = st0["loop"], want_st["loop"]
    else:
        st0, bad = W.bad_loop_states()
        cfg = W.loop_cfg(S.PULL_IN)
        want_st = st0.copy()
        want = A.run(oracle, blocks, want_st, cfg, A.WAID_L1CA)
        loop0, loop1 = st0, want_st
    for ch in bad:      # (on the restatement: nothing but the accumulator moved)
        for f in L.STATE_DTYPE.names:
            same = loop0[f][ch:ch + 1].tobytes() == loop1[f][ch:ch + 1].tobytes()
            assert same == (f != "if_freq_accum"), (ch, f)
    for dev in (False, True):
        recs, after, codes = _stage(eng, blocks, st0, cfg, A.WAID_L1CA, dev)
        assert codes == [EINVAL], dev
        if dev:
            assert eng.lib.gpsx_synchronize(eng.h) == 0
        else:
            assert b"prn" in eng.lib.gpsx_last_error(eng.h)
        _same(recs[0][1], after, want, want_st, (sync, dev, "bad channels"))


# ---- 10: refusals --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sync", [True, False], ids=["sync", "loop"])
def test_argument_checks_write_nothing(eng, sync):
    from stm32f4_sdr_gps_amd import capi
    blocks = K.strong_blocks(8)
    st0 = K.mixed_states(4, 9)
    if not sync:
        st0 = np.ascontiguousarray(st0["loop"])
    nan, inf = float("nan"), float("inf")
    good = dict(aid=(float(A.WAID_L1CA), 0), null_aid=False, null_cfg=False, spacing=8, n_blocks=8)
    # every refusal with its exact text: the three new clauses, one shared with the unaided calls, and the order of the clauses
    by_message = {
        b"null argument": [dict(null_aid=True), dict(null_cfg=True), dict(null_aid=True, n_blocks=0), dict(null_aid=True, aid=(nan, 1))],
        b"code_per_hz must be finite and -1..1": [dict(aid=(nan, 0)), dict(aid=(inf, 0)), dict(aid=(-inf, 0)), dict(aid=(1.0000001, 0)), dict(aid=(-1.5, 0)),
                                                  dict(aid=(2.0, 7))],
        b"reserved must be 0": [dict(aid=(float(A.WAID_L1CA), 1)), dict(aid=(0.0, -1)), dict(aid=(1.0, 1 << 30))],
        b"spacing must be 1..15 samples": [dict(spacing=0), dict(spacing=16, aid=(nan, 0))],        # (the unaided calls' clauses come first)
        b"n_blocks must be 1..4096": [dict(n_blocks=0, aid=(nan, 3)), dict(n_blocks=4097)],
    }
    n_rec = 2 * 4 * (Y.REC_DTYPE if sync else L.REC_DTYPE).itemsize

    def cfg_of(spacing=8):
        cfg = _sync_cfg(Y.make_cfg(4, 20, S.PULL_IN, S.STEADY, 20, (5, 4))) if sync else _loop_cfg(W.loop_cfg(S.PULL_IN))
        cfg["spacing"] = spacing
        return cfg
    with G.Pool() as pool:
        d_st, d_if = pool.add(G.Guarded(eng, st0.nbytes, G.STATE_FILL, st0)), pool.add(G.Guarded(eng, blocks.nbytes, G.STATE_FILL, blocks))
        outs = {True: pool.add(G.Guarded(eng, n_rec)), False: pool.add(G.Guarded(None, n_rec))}

        def call(a, dev):
            cfg, aid = cfg_of(a["spacing"]), capi.waid(a["aid"][0])
            aid["reserved"] = a["aid"][1]
            return _call(eng, sync, True, dev)[1](eng.h, None if a["null_cfg"] else cfg.ctypes.data, None if a["null_aid"] else aid.ctypes.data,
                                                  d_if.ptr if dev else blocks.ctypes.data, a["n_blocks"], d_st.ptr, 4, outs[dev].ptr)
        G.refusals(eng, by_message, good, call, [d_st, *outs.values()])
        # the limits themselves are accepted
        for dev in (False, True):
            name, fn = _call(eng, sync, True, dev)
            for k in (1.0, -1.0):
                d_st.refill()
                eng._chk(fn(eng.h, cfg_of().ctypes.data, capi.waid(k).ctypes.data, d_if.ptr if dev else blocks.ctypes.data, 8, d_st.ptr, 4, outs[dev].ptr), name)
                eng.synchronize()


# ---- 11: the scenarios the CPU test measures, on the device ------------------------------------------------------------------------
@pytest.mark.parametrize("fd", W.DOPPLERS)
def test_the_sliding_code_scenario_is_the_restatements(eng, oracle, fd):
    """one satellite at +-4500 Hz, 200 blocks of PULL_IN and 2000 of STEADY through gpsx_track_loop_weighted_aided_dev: records and
    states are the restatement's, whose code error tests/test_weighted_aided_reference.py bounds"""
    blocks = W.sliding_blocks(fd)
    pull, steady, mid, end = W.scenario_run(oracle, fd, A.WAID_L1CA)
    got_pull, st = _gpu(eng, blocks[:W.PULL_IN_MS], W.handover_state(fd), W.loop_cfg(S.PULL_IN), A.WAID_L1CA, True)
    _same(got_pull[0][1], st, pull, mid, ("pull-in", fd))
    got, st = _gpu(eng, blocks[W.PULL_IN_MS:], st, W.loop_cfg(S.STEADY), A.WAID_L1CA, True)
    _same(got[0][1], st, steady, end, ("steady", fd))
    err = np.abs(W.steady_errors(fd, got[0][1])[W.FIRST_WINDOW:]).max()
    print("fd", fd, "largest |code error| on the device's records", round(float(err), 3))
    assert err < W.bounds()["scenario_error"][fd]


def test_the_orbit_streams_first_two_launches_are_the_restatements(eng):
    """the first two launches (8192 blocks, 4 channels) of weighted_pvt_cases' stream with the lock gains STILL and GPSX_WAID_L1CA
    through gpsx_track_loop_weighted_sync_aided_dev: records and states are the aided restatement's"""
    launches = (4096, 4096)
    (out, st), = W.chains_on_restatements((P.HANDOVER,), launches)
    blocks = W.orbit_blocks(sum(launches))
    recs, after = _gpu(eng, blocks, P.handover(P.HANDOVER), P.sync_cfg(P.STILL), A.WAID_L1CA, True, pieces=list(launches))
    for (at, got), o in zip(recs, out):
        assert o[0] == at and got.tobytes() == o[2].tobytes(), at
    assert after.tobytes() == st["sync"].tobytes() and (after["mode"] == Y.LOCKED).all()
