"""The weighted path's lock monitor on the device (EXTENSION, not in the reference: include/gpsx.h gpsx_wlock; k_wlock on the vector
ALU, one channel per lane) against its exact CPU restatement (tests/weighted_lock_ref.py, pinned in
tests/test_weighted_lock_reference.py).  Every comparison is for equality, byte for byte, on the 64-byte records, the 128-byte lock
states and the 448-byte sync states.  The sync loop's records are fabricated (tests/weighted_lock_cases.py: 32 distinct streams
tiled over the channels, sync states in all three modes behind them); only the last test starts from IF samples."""
import numpy as np
import pytest

import weighted_gpu as G
import weighted_lock_cases as X
import weighted_lock_ref as R
import weighted_nav_ref as N
import weighted_obs_ref as O
import weighted_sync_cases as K
import weighted_sync_ref as Y
from weighted_gpu import EINVAL, eng  # noqa: F401

pytestmark = pytest.mark.gpu


def _gpu(eng, launches, st, cfg, sync=None, dev=True):
    """the library on copies of `st` (and of `sync`, the sync loop's states; None: a NULL pointer) in device memory, launch after
    launch.  launches: [(records [n_slots][n_ch], n_blocks)].
    -> ([lock records per launch], lock states after, sync states after or None, [return codes])"""
    n_ch, c = len(st), R.cfg_array(cfg)
    fn = eng.lib.gpsx_wlock_dev if dev else eng.lib.gpsx_wlock

    def call(ins, sts, out, k):
        return fn(eng.h, c.ctypes.data, ins[0], launches[k][0].shape[0], launches[k][1], sts[0], sts[1], n_ch, out)
    for rec, _ in launches:
        assert rec.dtype == Y.REC_DTYPE and rec.shape[1] == n_ch
    out, (after, sync_after), codes = G.run_stage(eng, call, b"k_wlock", [st, sync],
                                                  [([np.ascontiguousarray(rec)], R.LOCK_DTYPE, (n_ch,)) for rec, _ in launches], dev)
    return out, after, sync_after, codes


_same = G.same_rows


@pytest.mark.parametrize("n_slots", [1, X.AHEAD - 1, X.AHEAD, 2 * X.AHEAD + 1])
@pytest.mark.parametrize("n_ch", [1, 63, 64, 65, 130])
def test_records_and_states_match_the_restatement(eng, n_ch, n_slots):
    """a partial last wave with its idle lanes' loads, slot counts at the load pipeline's edges; states in the middle of anything
    (the restatement's after 11 windows), both variants.  The records were prefilled: equality says every byte was written"""
    st0, sync0, launches, want_st, want_sync = X.fab_run([n_slots], n_ch, warm=11)
    rec, n_blocks, want = launches[0]
    for dev in (True, False):
        lock, after, sync, codes = _gpu(eng, [(rec, n_blocks)], st0, X.FAB, sync0, dev=dev)
        assert codes == [0]
        _same(lock[0], want, ("records", dev))
        _same(after, want_st, ("states", dev))
        _same(sync, want_sync, ("sync states", dev))


_long = {}


@pytest.mark.parametrize("n_ch", [65, 130])
def test_a_launch_of_1024_slots(eng, n_ch):
    """4096 blocks at span 4 from fresh states: every stream through dozens of its cycles, losses and re-arms among them (the
    restatement answers for 96 channels: channel ch repeats channel ch % 96, stream and sync mode)"""
    if not _long:
        _long["run"] = X.fab_run([1024], 96)
    st0, sync0, launches, want_st, want_sync = _long["run"]
    rec, n_blocks, want = launches[0]
    lock, after, sync, codes = _gpu(eng, [(X.tile96(rec, n_ch), n_blocks)], X.tile96(st0, n_ch), X.FAB, X.tile96(sync0, n_ch))
    assert codes == [0]
    _same(lock[0], X.tile96(want, n_ch), "records")
    _same(after, X.tile96(want_st, n_ch), "states")
    _same(sync, X.tile96(want_sync, n_ch), "sync states")
    assert (want["n_rearm"] > 0).sum() >= 4 and (want["n_lost_code"] > 0).sum() >= 4 and (want["n_range"] > 0).sum() >= 2


def test_cut_invariance_without_rearm(eng):
    """the same 1300 blocks of records in launches of 500 / 500 / 300 and in thirteen launches of 100: the same final states, and the
    same final record apart from its per-launch fields, the epoch count and the event flags"""
    cfg = dict(X.FAB, rearm=0)
    n_ch = 65
    results = []
    for parts in ([125, 125, 75], [25] * 13):
        st0, _, launches, want_st, _ = X.fab_run(parts, n_ch, cfg)
        lock, after, sync, codes = _gpu(eng, [(rec, n) for rec, n, _ in launches], st0, cfg, None)
        assert codes == [0] * len(parts) and sync is None
        for got, (_, _, want) in zip(lock, launches):
            _same(got, want, ("records", len(parts)))
        _same(after, want_st, ("states", len(parts)))
        results.append((lock[-1], after))
    (a, st_a), (b, st_b) = results
    assert st_a.tobytes() == st_b.tobytes()
    events = np.uint32(R.F_LOST_CODE | R.F_LOST_CARRIER | R.F_REARMED | R.F_RANGE)
    for r in (a, b):
        r["n_epochs"] = 0
        r["flags"] &= ~events
    assert a.tobytes() == b.tobytes() and (a["last_k"] > 0).all()


def test_rearm_writes_only_what_it_says(eng):
    """130 channels: every stream in front of sync states in SEARCH, WAIT and LOCKED.  All 448 bytes of every sync state equal the
    restatement's; channels without a re-arm are byte-unchanged; those with one differ in the prescribed fields alone"""
    n_ch = 130
    st0, sync0, launches, want_st, want_sync = X.fab_run([40], n_ch)
    rec, n_blocks, want = launches[0]
    lock, after, sync, codes = _gpu(eng, [(rec, n_blocks)], st0, X.FAB, sync0)
    assert codes == [0]
    _same(lock[0], want, "records")
    _same(after, want_st, "states")
    _same(sync, want_sync, "sync states")
    rearmed = (lock[0]["flags"] & R.F_REARMED) != 0
    assert rearmed.sum() >= 5 and set(sync0["mode"][rearmed].tolist()) == {R.SYNC_LOCKED} and (sync["mode"][rearmed] == R.SYNC_SEARCH).all()
    assert sync[~rearmed].tobytes() == sync0[~rearmed].tobytes()
    pending_elsewhere = [c for c in range(n_ch) if c % X.DISTINCT in (4, 8, 10, 15) and not rearmed[c]]
    assert {int(sync0["mode"][c]) for c in pending_elsewhere} == {R.SYNC_SEARCH, R.SYNC_WAIT}      # pending met both, and wrote nothing
    changed = sync[rearmed].copy()
    for name in ("mode", "search_n", "prev_best_p1", "win_iq", "win_n", "bit_ip"):
        changed[name] = sync0[name][rearmed]
    changed["loop"]["n_updates"] = sync0["loop"]["n_updates"][rearmed]
    assert changed.tobytes() == sync0[rearmed].tobytes()
    # rearm == 0: a NULL d_sync_state works, and a pointer is never touched
    none = dict(X.FAB, rearm=0)
    st0, sync0, launches, want_st, _ = X.fab_run([40], n_ch, none)
    for given in (None, sync0):
        lock, after, sync, codes = _gpu(eng, [(launches[0][0], launches[0][1])], st0, none, given)
        assert codes == [0]
        _same(lock[0], launches[0][2], ("records, rearm 0", given is None))
        _same(after, want_st, ("states, rearm 0", given is None))
        assert given is None or sync.tobytes() == sync0.tobytes()


def test_bad_channels(eng):
    """one bad state per field among good neighbours of the same wave: untouched (their sync states too), their records zero with age
    -1, GPSX_EINVAL from the host variant and from the next synchronize after the device variant; the neighbours are the
    restatement's -- among them states at the very ends of the ranges, where no sum may overflow"""
    st0, sync0, launches, _, _ = X.fab_run([9], 64, warm=7)
    rec, n_blocks, _ = launches[0]
    st0 = st0.copy()
    bad = [1 + 2 * i for i in range(len(X.BAD_FIELDS))]
    for ch, (field, value) in zip(bad, X.BAD_FIELDS):
        st0[field][ch] = value
    for ch, (field, value) in zip([2 + 2 * i for i in range(len(X.GOOD_EDGES))], X.GOOD_EDGES):
        st0[field][ch] = value
    st0["flags"][bad[3]] |= R.F_PENDING
    sync0["mode"][bad[3]] = R.SYNC_LOCKED       # a bad channel with a re-arm pending: its sync state stays too
    want_st, want_sync = st0.copy(), sync0.copy()
    want, found = R.run(rec, n_blocks, want_st, X.FAB, want_sync)
    assert found == bad and want_st[bad].tobytes() == st0[bad].tobytes() and (want["age_blocks"][bad] == -1).all()
    for dev in (True, False):
        lock, after, sync, codes = _gpu(eng, [(rec, n_blocks)], st0, X.FAB, sync0, dev=dev)
        assert codes == [EINVAL] and eng.lib.gpsx_last_error(eng.h), dev
        assert eng.lib.gpsx_synchronize(eng.h) == 0
        _same(lock[0], want, ("records", dev))
        _same(after, want_st, ("states", dev))
        _same(sync, want_sync, ("sync states", dev))
        assert sync[bad].tobytes() == sync0[bad].tobytes()
    good = [c for c in range(len(st0)) if c not in bad]
    lock, after, sync, codes = _gpu(eng, [(np.ascontiguousarray(rec[:, good]), n_blocks)], st0[good].copy(), X.FAB, sync0[good].copy())
    assert codes == [0]
    _same(lock[0], want[good], "the same channels without the bad ones")
    _same(after, want_st[good], "their states")


def test_argument_checks_write_nothing(eng):
    n_ch, n_slots = 5, 10
    n_blocks = X.SPAN * n_slots
    st0, sync0, launches, _, _ = X.fab_run([n_slots], n_ch, warm=3)
    rec = launches[0][0]
    good = dict(null_cfg=False, null_rec=False, null_st=False, null_sync=False, null_out=False, n_slots=n_slots, n_blocks=n_blocks, n_ch=n_ch, reserved=0)
    # every refusal with its exact text; the last row of a group fails a later clause as well: the first failing clause decides
    by_message = {
        b"null argument": [dict(null_cfg=True), dict(null_rec=True), dict(null_st=True), dict(null_out=True), dict(null_st=True, n_ch=0)],
        b"epoch_search and epoch_lock must be 1..1024 windows": [dict(epoch_search=0), dict(epoch_search=1025), dict(epoch_lock=0), dict(epoch_lock=-1),
                                                                  dict(epoch_lock=1025, n_good=0)],
        b"n_good and n_bad must be 1..255": [dict(n_good=0), dict(n_good=256), dict(n_bad=0), dict(n_bad=256), dict(n_bad=-1, code_min=np.nan)],
        b"a threshold is not finite": [dict(code_min=np.nan), dict(code_min=np.inf), dict(car_min=-np.inf), dict(car_min=np.nan), dict(snr_min=np.inf),
                                       dict(snr_min=np.nan, rearm=4)],
        b"rearm must be 0..3": [dict(rearm=4), dict(rearm=-1), dict(rearm=4, patience=-1)],
        b"patience must not be negative": [dict(patience=-1), dict(patience=-2**31), dict(patience=-1, reserved=1)],
        b"reserved must be 0": [dict(reserved=1), dict(reserved=-1), dict(reserved=1, null_sync=True)],
        b"rearm needs d_sync_state": [dict(null_sync=True), dict(null_sync=True, rearm=1), dict(null_sync=True, n_blocks=0)],
        b"n_blocks must be 1..4096": [dict(n_blocks=0), dict(n_blocks=-40), dict(n_blocks=4097), dict(n_blocks=0, n_slots=0)],
        b"n_slots must be 1..n_blocks": [dict(n_slots=0), dict(n_slots=-1), dict(n_slots=n_blocks + 1), dict(n_slots=0, n_ch=0)],
        b"n_ch must be at least 1": [dict(n_ch=0), dict(n_ch=-3)],
    }
    with G.Pool() as pool:
        d_rec, d_st, d_sync = (pool.add(G.Guarded(eng, a.nbytes, G.STATE_FILL, a)) for a in (rec, st0, sync0))
        outs = {True: pool.add(G.Guarded(eng, n_ch * R.LOCK_DTYPE.itemsize)), False: pool.add(G.Guarded(None, n_ch * R.LOCK_DTYPE.itemsize))}

        def call(a, dev):
            cfg = R.cfg_array({**X.FAB, **{k: v for k, v in a.items() if k in X.FAB}}, a["reserved"])
            fn = eng.lib.gpsx_wlock_dev if dev else eng.lib.gpsx_wlock
            return fn(eng.h, None if a["null_cfg"] else cfg.ctypes.data, None if a["null_rec"] else d_rec.ptr, a["n_slots"], a["n_blocks"],
                      None if a["null_st"] else d_st.ptr, None if a["null_sync"] else d_sync.ptr, a["n_ch"], None if a["null_out"] else outs[dev].ptr)
        G.refusals(eng, by_message, good, call, [d_st, d_sync, *outs.values()])
        # the ends of the ranges are in range
        for change in (dict(epoch_search=1024, epoch_lock=1024, n_good=255, n_bad=255, patience=2**31 - 1), dict(epoch_search=1, epoch_lock=1, n_good=1, n_bad=1),
                       dict(code_min=-3.0e38, snr_min=3.0e38)):
            assert eng.lib.gpsx_wlock_dev(eng.h, R.cfg_array({**X.FAB, **change}).ctypes.data, d_rec.ptr, n_slots, n_blocks, d_st.ptr, d_sync.ptr, n_ch,
                                          outs[True].ptr) == 0
        eng.synchronize()


def test_the_engine_convenience(eng):
    st0, sync0, launches, want_st, want_sync = X.fab_run([12], 40)
    rec, n_blocks, want = launches[0]
    from stm32f4_sdr_gps_amd import capi
    with G.Pool() as pool:
        d_rec, d_st, d_sync = (pool.add(G.Guarded(eng, a.nbytes, G.STATE_FILL, a)).ptr.value for a in (rec, st0, sync0))
        f = X.FAB
        cfg = capi.wlock_cfg(f["epoch_search"], f["epoch_lock"], f["code_min"], f["car_min"], f["snr_min"], f["n_good"], f["n_bad"], f["rearm"], f["patience"])
        lock = eng.wlock(cfg, d_rec, rec.shape[0], n_blocks, d_st, 40, d_sync)
    _same(lock, want, "Engine.wlock")
    assert capi.wlock_cn0_dbhz(lock, 20).tobytes() == R.cn0_dbhz(want, 20).tobytes()


def test_if_samples_to_lock_flags_on_the_device(eng):
    """seed 1 of the scenario, rearm = 1: IF samples -> gpsx_track_loop_weighted_sync_dev -> gpsx_wnav_words_dev / gpsx_wobs_dev ->
    gpsx_wlock_dev on one stream, 3000 blocks in launches of 500.  Each launch's lock records and states equal the restatement on
    the device's own sync records and states; the scenario's conditions hold on the device's output"""
    from stm32f4_sdr_gps_amd import capi
    seed, n_ch = 1, X.N_CH
    blocks = X.scenario_blocks(seed)
    sync_cfg = capi.wsync_cfg(K.N_COH_SEARCH, K.N_COH_LOCK, K.S.PULL_IN, K.S.STEADY, K.SYNC_BITS, K.RATIO)
    cfg = X.scenario_cfg(1)
    states = dict(sync=X.scenario_states(seed), nav=np.zeros(n_ch, N.STATE_DTYPE), obs=np.zeros(n_ch, O.STATE_DTYPE), lock=np.zeros(n_ch, R.STATE_DTYPE))
    want_st = states["lock"].copy()
    flags, modes, snr, obs_flags, search_after = [], [], [], [], None
    with G.Guarded(eng, blocks.nbytes, G.STATE_FILL, blocks) as d_if, G.Chain(eng, sync_cfg, states, X.LAUNCH, lock_cfg=R.cfg_array(cfg)) as chain:
        for at, n in X.launches():
            chain.sync(d_if.ptr.value + at * 4092, n)
            eng.synchronize()
            before = chain.read("sync")        # what the sync launch left: the restatement's re-arm starts from it
            chain.words()
            chain.obs()
            chain.lock(rearm_on_sync=True)
            eng.synchronize()
            rec, lock, obs, lock_st, sync_st = (chain.read(name) for name in ("rec", "l", "o", "lock", "sync"))
            want, bad = R.run(rec, n, want_st, cfg, before)
            assert not bad
            _same(lock, want, ("records of the launch at", at))
            _same(lock_st, want_st, ("states after the launch at", at))
            _same(sync_st, before, ("sync states after the launch at", at))
            flags.append(lock["flags"].copy())
            modes.append(sync_st["mode"].copy())
            snr.append(lock["snr"].copy())
            obs_flags.append(obs["flags"].copy())
            if search_after is None and int(lock["flags"][X.VANISHING]) & R.F_REARMED:
                search_after = len(flags)
            elif search_after == len(flags) - 1:
                col = rec[:, X.VANISHING]
                assert (col["flags"] & Y.F_WINDOW).any() and not (col["flags"] & Y.F_LOCKED).any()      # the launch after the loss ran in SEARCH
    flags = np.array(flags)
    both = R.F_CODE | R.F_CARRIER
    for ch in X.HEALTHY:
        assert (flags[:, ch] & R.F_CODE).all() and (flags[2:, ch] & both == both).all(), (ch, flags[:, ch])
        assert not (flags[:, ch] & (R.F_LOST_CODE | R.F_LOST_CARRIER | R.F_REARMED)).any() and lock["n_rearm"][ch] == 0
    assert (flags[:4, X.VANISHING] & R.F_CODE).all() and (flags[2:4, X.VANISHING] & both == both).all()
    lost = np.nonzero(flags[:, X.VANISHING] & R.F_LOST_CODE)[0].tolist()
    assert lost == [4] and not (flags[4:, X.VANISHING] & R.F_CODE).any() and flags[4, X.VANISHING] & R.F_REARMED, flags[:, X.VANISHING]
    assert search_after == 5 and [int(m[X.VANISHING]) for m in modes] == [0, 2, 2, 2, 0, 0]
    assert not (flags[:, len(K.SATS):] & both).any()      # the PRNs that are not in the stream
    assert not obs_flags[-1][X.VANISHING] & (O.F_EDGE | O.F_VALID) and obs_flags[3][X.VANISHING] & O.F_EDGE
    assert all(obs_flags[-1][ch] & O.F_EDGE for ch in X.HEALTHY)
    # C/N0 from the launches' records while all three are locked: what the restatements measured, within three standard deviations
    cn0 = np.array([capi.wlock_cn0_dbhz(np.array([(16, 0, 10, 0, 0, 0, s, 0, 0, 0, 0, 0, (0, 0, 0)) for s in row[:3]], R.LOCK_DTYPE), K.N_COH_LOCK)
                    for row in snr[2:4]])
    full = X.MEASURED["cn0_full"]
    print("C/N0 of the launches' newest epochs, dB-Hz:", cn0.tolist())
    assert abs(float(cn0.mean()) - full["mean"]) <= 3 * full["sd"]
