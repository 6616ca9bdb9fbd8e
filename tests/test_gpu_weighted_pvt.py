"""Orbiting satellites' IF samples to a position fix on the device: the weighted chain's five stages joined (include/gpsx.h
gpsx_track_loop_weighted_sync_dev -> gpsx_wnav_words_dev -> gpsx_wobs_dev + gpsx_weph_dev on one stream with one synchronize per
launch, then the host helpers gpsx_wobs_pseudoranges and gpsx_weph_to_eph and the library's pntpos) on tests/weighted_pvt_cases.py's
scenario: test_gpu_pvt_chain.py's four satellites, two-bit quantised, 25 000 blocks, so that the code slides under a DLL that has no
carrier aiding.  The CPU partner is tests/test_weighted_pvt_reference.py; its conditions, lag residual and position bounds (measured on
the restatements, tests/weighted_pvt_cases.py BOUNDS) are the ones used here.

Cost.  The stream (102 MB) is synthesised once (about 25 s of CPU) and goes to the device once; the device work is a few seconds in
all.  The byte-for-byte partner, the chain on the CPU restatements, is 35 s of Python per channel in worker processes of their own
(about 35 s with a CPU per channel for the MOVING gains; the still-code gains run only the first and the last launch: 7 s)."""
import numpy as np
import pytest

import weighted_eph_ref as E
import weighted_gpu as G
import weighted_pvt_cases as P
import weighted_sync_ref as Y
from weighted_gpu import eng  # noqa: F401

pytestmark = pytest.mark.gpu

SYNC_FIELDS = [("w", f) for f in Y.REC_DTYPE.fields["w"][0].names] + ["end_block", "flags", "bit_ip"]


@pytest.fixture(scope="module")
def d_if(eng):
    """the whole stream on the device, uploaded once"""
    blocks = P.blocks()
    d = eng.malloc(blocks.nbytes)
    eng.h2d(d, blocks)
    yield d
    eng.free(d)


def _chain(eng, d_if, sync0, lock, cuts, host_last=0, first_block=0, states=None):
    """the five stages over consecutive launches of `cuts` blocks from `first_block`, states in device memory between canaries, every
    output prefilled with 0xA5 between canaries.  The last `host_last` launches run the four stages' host variants (blocks and
    outputs in host memory, one wait per stage).  -> ([(first block, n, records, words, observables, ephemeris records)], states)"""
    lib, n_ch = eng.lib, len(sync0)
    st0 = dict(P.fresh_states(), sync=sync0) if states is None else states
    out, at = [], first_block
    with G.Chain(eng, P.sync_cfg_dev(lock), {k: st0[k] for k in ("sync", "nav", "obs", "eph")}, max(cuts), P.MAX_BAD_WORDS, P.EDGE_GUARD) as chain:
        bufs = chain.buf
        for k, n in enumerate(cuts):
            chain.refill()
            if k < len(cuts) - host_last:
                chain.sync(d_if + at * 4092, n)
                chain.words()
                chain.obs()
                chain.eph()
                eng.synchronize()
                rec, words, obs, eph = (chain.read(name) for name in ("rec", "words", "o", "e"))
            else:
                chain.begin(n)
                rec, words, obs, eph = (np.full(int(np.prod(chain.shape(name))) * chain.OUT[name].itemsize, 0xA5, np.uint8).view(chain.OUT[name])
                                        .reshape(chain.shape(name)) for name in ("rec", "words", "o", "e"))
                blocks = np.ascontiguousarray(P.blocks()[at:at + n])
                eng._chk(lib.gpsx_track_loop_weighted_sync(eng.h, chain.sync_cfg.ctypes.data, blocks.ctypes.data, n, bufs["sync"].ptr, n_ch, rec.ctypes.data),
                         "gpsx_track_loop_weighted_sync")
                bufs["rec"].put(rec)
                eng._chk(lib.gpsx_wnav_words(eng.h, chain.nav_cfg.ctypes.data, bufs["rec"].ptr, chain.n_slots, n, bufs["nav"].ptr, n_ch, words.ctypes.data),
                         "gpsx_wnav_words")
                bufs["words"].put(words)
                eng._chk(lib.gpsx_wobs(eng.h, chain.obs_cfg.ctypes.data, bufs["rec"].ptr, chain.n_slots, n, bufs["words"].ptr, bufs["obs"].ptr, n_ch,
                                       obs.ctypes.data), "gpsx_wobs")
                eng._chk(lib.gpsx_weph(eng.h, chain.eph_cfg.ctypes.data, bufs["words"].ptr, n, bufs["eph"].ptr, n_ch, eph.ctypes.data), "gpsx_weph")
                bufs["rec"].get(np.uint8, (1,)), bufs["words"].get(np.uint8, (1,))      # (the canaries around what was uploaded)
            out.append((at, n, rec, words, obs, eph))
            at += n
        states = {k: chain.read(k) for k in ("sync", "nav", "obs", "eph")}
    return out, states


def _first_difference(got, want, launch):
    """the first (launch, slot, channel, field) at which two sync-record arrays differ, or None"""
    for slot in range(got.shape[0]):
        for ch in range(got.shape[1]):
            if got[slot, ch].tobytes() != want[slot, ch].tobytes():
                for f in SYNC_FIELDS:
                    a, b = (got[f[0]][f[1]], want[f[0]][f[1]]) if isinstance(f, tuple) else (got[f], want[f])
                    if a[slot, ch].tobytes() != b[slot, ch].tobytes():
                        return (launch, slot, ch, f, a[slot, ch], b[slot, ch])
                return (launch, slot, ch, "padding", None, None)
    return None


def _same_launch(got, want, k, what):
    at, n, rec, words, obs, eph = got
    w_at, w_n, w_rec, w_words, w_obs, w_eph = want
    assert (at, n) == (w_at, w_n) and rec.shape == w_rec.shape and words.shape == w_words.shape
    assert rec.tobytes() == w_rec.tobytes(), (what, "sync records: first difference (launch, slot, channel, field, got, want)",
                                              _first_difference(rec, w_rec, k))
    assert words.tobytes() == w_words.tobytes(), (what, "words", k)
    assert obs.tobytes() == w_obs.tobytes(), (what, "observables", k, obs, w_obs)
    assert eph.tobytes() == w_eph.tobytes(), (what, "ephemeris records", k)


def _same_states(got, want, what):
    for name in ("sync", "nav", "obs", "eph"):
        bad = [c for c in range(4) if got[name][c:c + 1].tobytes() != want[name][c:c + 1].tobytes()]
        assert not bad, (what, name, "states of channels", bad)


def _fixes(lib, obs, eph):
    return [P.position(lib, obs, eph, P.PRNS, offset) for offset in P.OFFSETS_MS]


@pytest.fixture(scope="module")
def whole(eng, d_if):
    """the device's chain with the MOVING gains and the CPU test's hand-over in LAUNCHES, run once for the tests that need it"""
    return _chain(eng, d_if, P.handover(), P.MOVING, P.LAUNCHES)


def test_the_chain_equals_the_restatements_launch_by_launch(whole):
    """MOVING gains, the CPU test's hand-over, six launches of 4096 blocks and one of 424: every launch's sync records, words,
    observables and ephemeris records and the four state arrays at the end are the restatements', byte for byte (the first differing
    sync record is named); hence the same position to the last bit through position(), which the CPU test holds against its bounds"""
    from stm32f4_sdr_gps_amd import capi
    want, want_st = P.chain_on_restatements("moving")
    got, st = whole
    for k in range(len(P.LAUNCHES)):
        _same_launch(got[k], want[k], k, "moving")
    _same_states(st, want_st, "moving")
    lib = capi.load_library()
    for a, b in zip(_fixes(lib, got[-1][4], got[-1][5]), _fixes(lib, want[-1][4], want[-1][5])):
        assert a["rr"].tobytes() == b["rr"].tobytes() and a["dtr"] == b["dtr"] and a["rx_tow_s"] == b["rx_tow_s"]
        print("device fix", P.position_error(a), "m from the truth, clock term", a["dtr"])
        assert P.position_error(a) < P.BOUNDS["moving"]["position_m"]


def test_both_variants_and_another_cut(eng, d_if, whole):
    """the same stream in 25 launches of 1000 blocks, the last three through the host variants of the four stages: every launch's
    words, observables and ephemeris records equal the three cheap restatements run on the device's own sync records of that cut
    (hence age_blocks and NEW's launch as this cut has them), and the final observables and ephemerides equal the first test's but for
    those two"""
    cuts = (1000,) * 25
    got, st = _chain(eng, d_if, P.handover(), P.MOVING, cuts, host_last=3)
    ref = P.fresh_states()
    new = np.zeros(4, np.uint32)
    for k, (at, n, rec, words, obs, eph) in enumerate(got):
        w_words, w_obs, w_eph = P.after_sync(rec, n, ref)
        assert words.tobytes() == w_words.tobytes(), ("words", k)
        assert obs.tobytes() == w_obs.tobytes(), ("observables", k, obs, w_obs)
        assert eph.tobytes() == w_eph.tobytes(), ("ephemeris records", k)
        new += (eph["flags"] & E.F_NEW) // E.F_NEW
    for name in ("nav", "obs", "eph"):
        assert st[name].tobytes() == ref[name].tobytes(), name
    assert new.tolist() == [1, 1, 1, 1]
    launches, whole_st = whole
    _same_states(st, whole_st, "the cut does not matter to the states")
    obs, eph, w_obs, w_eph = got[-1][4].copy(), got[-1][5].copy(), launches[-1][4].copy(), launches[-1][5].copy()
    assert (obs["age_blocks"] == (P.N_BLOCKS - st["obs"]["last_win_end_p1"])).all()
    eph["flags"] &= ~np.uint32(E.F_NEW)      # (which launch's record gets NEW is the cut's business: each channel got it once, above)
    w_eph["flags"] &= ~np.uint32(E.F_NEW)
    assert obs.tobytes() == w_obs.tobytes() and eph.tobytes() == w_eph.tobytes()


def test_acquisition_hands_over_and_the_fix_holds(eng, d_if):
    """gpsx_acq_grid_weighted_hyb, 10 x 8 blocks, PRNs 1, 3, 4, 5 and four that are not in the sky, -5000 .. 5000 Hz in 50 Hz steps,
    on the stream's first 80 blocks: each present PRN's best record lies within one bin and 8 samples of the first block's truth and
    above every absent PRN's best; the records fill zeroed states (phase -> code_phase_fine, bin -> if_freq_offset_hz, accumulator
    0) and the chain runs with the MOVING gains from block 0.  No byte-exact partner: the CPU test's conditions, lag residual and
    position bound are asserted on what the device gives.  Measured on one MI355X: records 2 / 1 / 0 / 0 samples and 11 / 21 / 11 / 13 Hz
    off the truth, 436 258 .. 506 056 high; VALID from block 8192; largest lag residual 0.81 samples (bound 1.275); transmit-time errors at
    block 25 000 -1.36 / -2.04 / -1.24 / -0.73 samples; fix 30.02 m from the truth at either offset (bound 52.7 m)"""
    from stm32f4_sdr_gps_amd import capi
    absent = (2, 6, 7, 8)
    prns = np.array(P.PRNS + absent, np.uint8)
    pk = eng.acq_grid_weighted_hyb(P.blocks()[:80], prns, 1, 10, 8, -5000, 50, 201)[0]
    best = pk["max_val"].argmax(axis=1)
    top = pk["max_val"].max(axis=1)
    states = []
    for c, (fd, delay) in enumerate(P.first()):
        dopp, phase = -5000 + 50 * int(best[c]), int(pk["phase"][c, best[c]])
        print("PRN", P.PRNS[c], "record", int(top[c]), "at", phase, "samples,", dopp, "Hz; truth", round(delay, 1), round(fd, 1))
        assert abs(dopp - fd) <= 50.0 and abs((phase - delay + 8184.0) % 16368.0 - 8184.0) <= 8.0, (c, dopp, fd, phase, delay)
        assert int(top[c]) > int(top[4:].max()), (c, top.tolist())
        states.append(Y.handover(P.PRNS[c], float(phase), float(dopp)))
    got, st = _chain(eng, d_if, np.concatenate(states), P.MOVING, P.LAUNCHES)
    P.check_conditions(got, st)
    P.check_lag(got, "moving")
    lib = capi.load_library()
    fixes = P.check_fixes(lib, got[-1][4], got[-1][5], "moving")
    print("position errors (device, acquisition's hand-over)", [P.position_error(f) for f in fixes])


def test_the_still_code_gains_on_a_moving_code(eng, d_if):
    """weighted_sync_cases.sync_cfg()'s gains (steady DLL (0.5, 40)) on the device: the first launch equals the restatement chain's
    byte for byte; so does the last, with the sync restatement restarted from the states the device had before it; and the
    per-channel lag of a type-1 DLL under a Doppler ramp follows lag_model at c2 = 40 -- the finding, pinned on the device (measured
    on one MI355X: both launches equal; errors at block 25 000 +2.19 / -4.19 / -4.02 / -1.16 samples against a model of +3.58 / -3.31 /
    -3.29 / -0.05, largest residual 0.66 samples: the restatements' figures)"""
    before, st6 = _chain(eng, d_if, P.handover(), P.STILL, P.LAUNCHES[:-1])
    last, st7 = _chain(eng, d_if, st6["sync"], P.STILL, P.LAUNCHES[-1:], first_block=sum(P.LAUNCHES[:-1]), states=st6)
    got = before + last
    first_block = sum(P.LAUNCHES[:-1])
    cfg = P.sync_cfg(P.STILL)
    (first_recs, first_after), (last_recs, last_after) = P.sync_on_restatement([(0, P.LAUNCHES[:1], P.handover(), cfg),
                                                                                (first_block, P.LAUNCHES[-1:], st6["sync"], cfg)])
    ref = P.fresh_states()
    want = (0, P.LAUNCHES[0], first_recs[0]) + P.after_sync(first_recs[0], P.LAUNCHES[0], ref)
    _same_launch(got[0], want, 0, "still, first launch")
    ref = {k: st6[k].copy() for k in ("nav", "obs", "eph")}
    want = (first_block, P.LAUNCHES[-1], last_recs[0]) + P.after_sync(last_recs[0], P.LAUNCHES[-1], ref)
    _same_launch(got[-1], want, len(P.LAUNCHES) - 1, "still, last launch")
    _same_states(st7, dict(ref, sync=last_after), "still, last launch")
    P.check_conditions(got, st7)
    P.check_lag(got, "still")
