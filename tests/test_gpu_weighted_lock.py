"""The weighted path's lock monitor on the device (EXTENSION, not in the reference: include/gpsx.h gpsx_wlock; k_wlock on the vector
ALU, one channel per lane) against its exact CPU restatement (tests/weighted_lock_ref.py, pinned in
tests/test_weighted_lock_reference.py).  Every comparison is for equality, byte for byte, on the 64-byte records, the 128-byte lock
states and the 448-byte sync states.  The sync loop's records are fabricated (tests/weighted_lock_cases.py: 32 distinct streams
tiled over the channels, sync states in all three modes behind them); only the last test starts from IF samples."""
import ctypes as C

import numpy as np
import pytest

import weighted_lock_cases as X
import weighted_lock_ref as R
import weighted_nav_ref as N
import weighted_obs_ref as O
import weighted_sync_cases as K
import weighted_sync_ref as Y

pytestmark = pytest.mark.gpu

EINVAL = -22
GUARD = 4096


@pytest.fixture(scope="module")
def eng():
    from stm32f4_sdr_gps_amd import capi
    e = capi.Engine(0)
    yield e
    e.close()


def _between_canaries(eng, a, fill):
    h = np.full(GUARD + a.nbytes + GUARD, fill, np.uint8)
    h[GUARD:GUARD + a.nbytes] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    d = eng.malloc(h.nbytes)
    eng.h2d(d, h)
    return h, d


def _back(eng, h, d, nbytes, fill, what):
    eng.d2h(h, d)
    assert (h[:GUARD] == fill).all() and (h[GUARD + nbytes:] == fill).all(), "canary around " + what
    return h[GUARD:GUARD + nbytes]


def _gpu(eng, launches, st, cfg, sync=None, dev=True):
    """the library on copies of `st` (and of `sync`, the sync loop's states; None: a NULL pointer) in device memory, launch after
    launch.  launches: [(records [n_slots][n_ch], n_blocks)].  States and records sit between canaries, the records are prefilled
    with 0xA5.  -> ([lock records per launch], lock states after, sync states after or None, [return codes])"""
    n_ch = len(st)
    c = R.cfg_array(cfg)
    h_st, d_st = _between_canaries(eng, st, 0x5A)
    h_sync, d_sync = _between_canaries(eng, sync, 0x3C) if sync is not None else (None, 0)
    p_sync = C.c_void_p(d_sync + GUARD) if sync is not None else None
    out, codes = [], []
    try:
        for rec, n_blocks in launches:
            rec = np.ascontiguousarray(rec)
            assert rec.dtype == Y.REC_DTYPE and rec.shape[1] == n_ch
            size = n_ch * 64
            h_lock = np.full(GUARD + size + GUARD, 0xA5, np.uint8)
            d_rec, d_lock = eng.malloc(rec.nbytes), eng.malloc(h_lock.nbytes)
            try:
                eng.h2d(d_rec, rec)
                if dev:
                    eng.h2d(d_lock, h_lock)
                    rc = eng.lib.gpsx_wlock_dev(eng.h, c.ctypes.data, C.c_void_p(d_rec), rec.shape[0], n_blocks, C.c_void_p(d_st + GUARD), p_sync, n_ch,
                                                C.c_void_p(d_lock + GUARD))
                    assert rc == 0 and eng.lib.gpsx_last_kernel(eng.h) == b"k_wlock"
                    codes.append(eng.lib.gpsx_synchronize(eng.h))
                    eng.d2h(h_lock, d_lock)
                else:
                    codes.append(eng.lib.gpsx_wlock(eng.h, c.ctypes.data, C.c_void_p(d_rec), rec.shape[0], n_blocks, C.c_void_p(d_st + GUARD), p_sync, n_ch,
                                                    h_lock[GUARD:].ctypes.data))
            finally:
                eng.free(d_rec)
                eng.free(d_lock)
            assert (h_lock[:GUARD] == 0xA5).all() and (h_lock[GUARD + size:] == 0xA5).all(), "canary around the records"
            out.append(h_lock[GUARD:GUARD + size].view(R.LOCK_DTYPE).copy())
        after = _back(eng, h_st, d_st, st.nbytes, 0x5A, "the lock states").view(R.STATE_DTYPE).copy()
        sync_after = _back(eng, h_sync, d_sync, sync.nbytes, 0x3C, "the sync states").view(Y.STATE_DTYPE).copy() if sync is not None else None
    finally:
        eng.free(d_st)
        if sync is not None:
            eng.free(d_sync)
    return out, after, sync_after, codes


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = [c for c in range(len(got)) if got[c:c + 1].tobytes() != want[c:c + 1].tobytes()]
    assert not bad, (what, bad[:4], got[bad[0]], want[bad[0]])


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
    refusals = [(message, change) for message, changes in by_message.items() for change in changes]
    d_rec, d_st, d_sync, d_lock = eng.malloc(rec.nbytes), eng.malloc(st0.nbytes), eng.malloc(sync0.nbytes), eng.malloc(n_ch * 64)
    try:
        eng.h2d(d_rec, rec)
        for dev, fn in ((False, eng.lib.gpsx_wlock), (True, eng.lib.gpsx_wlock_dev)):
            for message, change in refusals:
                a = {**good, **change}
                cfg = R.cfg_array({**X.FAB, **{k: v for k, v in change.items() if k in X.FAB}}, a["reserved"])
                host = np.full(n_ch * 64, 0xA5, np.uint8)
                eng.h2d(d_st, st0)
                eng.h2d(d_sync, sync0)
                eng.h2d(d_lock, host)
                rc = fn(eng.h, None if a["null_cfg"] else cfg.ctypes.data, None if a["null_rec"] else C.c_void_p(d_rec), a["n_slots"], a["n_blocks"],
                        None if a["null_st"] else C.c_void_p(d_st), None if a["null_sync"] else C.c_void_p(d_sync), a["n_ch"],
                        None if a["null_out"] else (C.c_void_p(d_lock) if dev else host.ctypes.data))
                assert rc == EINVAL and eng.lib.gpsx_last_error(eng.h) == message, (dev, change, eng.lib.gpsx_last_error(eng.h))
                eng.synchronize()      # nothing was enqueued, nothing is pending
                st, sync, dw = st0.copy(), sync0.copy(), np.zeros_like(host)
                eng.d2h(st, d_st)
                eng.d2h(sync, d_sync)
                eng.d2h(dw, d_lock)
                assert (host == 0xA5).all() and (dw == 0xA5).all() and st.tobytes() == st0.tobytes() and sync.tobytes() == sync0.tobytes(), (dev, change)
        # the ends of the ranges are in range
        for change in (dict(epoch_search=1024, epoch_lock=1024, n_good=255, n_bad=255, patience=2**31 - 1), dict(epoch_search=1, epoch_lock=1, n_good=1, n_bad=1),
                       dict(code_min=-3.0e38, snr_min=3.0e38)):
            assert eng.lib.gpsx_wlock_dev(eng.h, R.cfg_array({**X.FAB, **change}).ctypes.data, C.c_void_p(d_rec), n_slots, n_blocks, C.c_void_p(d_st),
                                          C.c_void_p(d_sync), n_ch, C.c_void_p(d_lock)) == 0
        eng.synchronize()
    finally:
        for p in (d_rec, d_st, d_sync, d_lock):
            eng.free(p)


def test_the_engine_convenience(eng):
    st0, sync0, launches, want_st, want_sync = X.fab_run([12], 40)
    rec, n_blocks, want = launches[0]
    from stm32f4_sdr_gps_amd import capi
    d_rec, d_st, d_sync = eng.malloc(rec.nbytes), eng.malloc(st0.nbytes), eng.malloc(sync0.nbytes)
    try:
        eng.h2d(d_rec, np.ascontiguousarray(rec))
        eng.h2d(d_st, st0)
        eng.h2d(d_sync, sync0)
        f = X.FAB
        cfg = capi.wlock_cfg(f["epoch_search"], f["epoch_lock"], f["code_min"], f["car_min"], f["snr_min"], f["n_good"], f["n_bad"], f["rearm"], f["patience"])
        lock = eng.wlock(cfg, d_rec, rec.shape[0], n_blocks, d_st, 40, d_sync)
    finally:
        for p in (d_rec, d_st, d_sync):
            eng.free(p)
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
    nav_cfg = np.zeros(1, capi.WNAV_CFG_DTYPE)
    nav_cfg["max_bad_words"] = 3
    obs_cfg = np.zeros(1, capi.WOBS_CFG_DTYPE)
    obs_cfg["edge_guard"] = 512.0
    cfg = X.scenario_cfg(1)
    lock_cfg = R.cfg_array(cfg)
    sync_st = X.scenario_states(seed)
    nav, obs_st, lock_st = np.zeros(n_ch, N.STATE_DTYPE), np.zeros(n_ch, O.STATE_DTYPE), np.zeros(n_ch, R.STATE_DTYPE)
    max_slots = capi.wsync_slots(X.LAUNCH, K.N_COH_SEARCH, K.N_COH_LOCK)
    sizes = (blocks.nbytes, sync_st.nbytes, nav.nbytes, obs_st.nbytes, lock_st.nbytes, max_slots * n_ch * 48, N.max_words(X.LAUNCH) * n_ch * 16, n_ch * 32, n_ch * 64)
    ptrs = [eng.malloc(s) for s in sizes]
    d_if, d_sync, d_nav, d_obs_st, d_lock_st, d_rec, d_words, d_obs, d_lock = ptrs
    want_st = lock_st.copy()
    flags, modes, snr, obs_flags, search_after = [], [], [], [], None
    try:
        for d, a in ((d_if, blocks), (d_sync, sync_st), (d_nav, nav), (d_obs_st, obs_st), (d_lock_st, lock_st)):
            eng.h2d(d, a)
        for at, n in X.launches():
            n_slots = capi.wsync_slots(n, K.N_COH_SEARCH, K.N_COH_LOCK)
            eng._chk(eng.lib.gpsx_track_loop_weighted_sync_dev(eng.h, sync_cfg.ctypes.data, C.c_void_p(d_if + at * 4092), n, C.c_void_p(d_sync), n_ch,
                                                               C.c_void_p(d_rec)), "gpsx_track_loop_weighted_sync_dev")
            eng.synchronize()
            before = sync_st.copy()
            eng.d2h(before, d_sync)        # what the sync launch left: the restatement's re-arm starts from it
            eng._chk(eng.lib.gpsx_wnav_words_dev(eng.h, nav_cfg.ctypes.data, C.c_void_p(d_rec), n_slots, n, C.c_void_p(d_nav), n_ch, C.c_void_p(d_words)),
                     "gpsx_wnav_words_dev")
            eng._chk(eng.lib.gpsx_wobs_dev(eng.h, obs_cfg.ctypes.data, C.c_void_p(d_rec), n_slots, n, C.c_void_p(d_words), C.c_void_p(d_obs_st), n_ch,
                                           C.c_void_p(d_obs)), "gpsx_wobs_dev")
            eng._chk(eng.lib.gpsx_wlock_dev(eng.h, lock_cfg.ctypes.data, C.c_void_p(d_rec), n_slots, n, C.c_void_p(d_lock_st), C.c_void_p(d_sync), n_ch,
                                            C.c_void_p(d_lock)), "gpsx_wlock_dev")
            eng.synchronize()
            rec, lock, obs = np.zeros((n_slots, n_ch), Y.REC_DTYPE), np.zeros(n_ch, R.LOCK_DTYPE), np.zeros(n_ch, O.OBS_DTYPE)
            for a, d in ((rec, d_rec), (lock, d_lock), (obs, d_obs), (lock_st, d_lock_st), (sync_st, d_sync)):
                eng.d2h(a, d)
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
    finally:
        for p in ptrs:
            eng.free(p)
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
