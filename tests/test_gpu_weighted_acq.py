"""The acquisition decisions and the slot hand-over on the device (EXTENSION, not in the reference: include/gpsx.h gpsx_wacq; k_wacq, a
wave per receiver) against the exact CPU restatement (tests/weighted_acq_ref.py, the rows of tests/weighted_acq_cases.py, whose
predicates tests/test_weighted_acq_reference.py asserts).  Every comparison is for equality, byte for byte, on all five state arrays
and both outputs, the states between canaries, the outputs prefilled: the table at every edge of the wave's bin stride, of the PRN
and slot lanes and of four receivers per workgroup; host variant = device variant = binding; a second call that writes nothing;
receivers permuted; every refusal with its text; and two receivers from IF samples through the hybrid grid, this stage, the sync
loop, the words and the lock monitor, with a slot lost and re-acquired, no peak record and no state crossing to the host in between."""
import ctypes as C

import numpy as np
import pytest

import weighted_acq_cases as AC
import weighted_acq_ref as Q
import weighted_gpu as G
from weighted_gpu import EINVAL, eng  # noqa: F401

pytestmark = pytest.mark.gpu

NAMES = ("sync", "lock", "nav", "obs", "eph")


def _desc(prns, n_rx, grid, n_dopp):
    """the gpsx_acq_weighted_t the grid call got (and what keeps its PRN list alive)"""
    from stm32f4_sdr_gps_amd import capi
    prns = np.ascontiguousarray(prns, np.uint8)
    return capi.AcqWeightedT(n_rx, 0, len(prns), prns.ctypes.data_as(C.POINTER(C.c_uint8)), grid[0], grid[1], n_dopp, 1), prns


def _call(eng, la, dev, nulls=(), cfg=None, states=None, want_det=True):
    """gpsx_wacq_dev (dev) or gpsx_wacq on launch `la`: the states (those named in `nulls`: a NULL pointer) between canaries in device
    memory, the records between canaries too, the outputs prefilled -> (acq, det or None, {name: states after})"""
    cfg = Q.cfg_record(la.cfg if cfg is None else cfg)
    states = la.states if states is None else states
    g, keep = _desc(la.prns, la.n_rx, la.grid, la.n_dopp)
    fn = eng.lib.gpsx_wacq_dev if dev else eng.lib.gpsx_wacq
    with G.Pool() as pool:
        st = {k: None if k in nulls else pool.add(G.Guarded(eng, states[k].nbytes, G.STATE_FILL, states[k])) for k in NAMES}
        pk = pool.add(G.Guarded(eng if dev else None, la.peaks.nbytes, G.STATE_FILL, la.peaks))
        acq = pool.add(G.Guarded(eng if dev else None, la.n_rx * Q.ACQ_DTYPE.itemsize))
        det = pool.add(G.Guarded(eng if dev else None, la.n_rx * la.n_prn * Q.DET_DTYPE.itemsize))
        rc = fn(eng.h, cfg.ctypes.data, C.addressof(g), pk.ptr, *[None if st[k] is None else st[k].ptr for k in NAMES], acq.ptr,
                det.ptr if want_det else None)
        assert rc == 0, (rc, eng.lib.gpsx_last_error(eng.h))
        assert eng.lib.gpsx_last_kernel(eng.h) == b"k_wacq"
        assert eng.lib.gpsx_synchronize(eng.h) == 0
        assert pk.untouched()
        if not want_det:
            assert det.untouched()
        return (acq.get(Q.ACQ_DTYPE, (la.n_rx,)), det.get(Q.DET_DTYPE, (la.n_rx, la.n_prn)) if want_det else None,
                {k: None if st[k] is None else st[k].get(states[k].dtype, states[k].shape) for k in NAMES})


def _want(la, nulls=(), cfg=None, states=None, want_det=True):
    """the restatement on the same launch -> (acq, det, {name: states after}, trace)"""
    st = {k: None if k in nulls else (la.states if states is None else states)[k].copy() for k in NAMES}
    trace = []
    acq, det = Q.run(la.cfg if cfg is None else cfg, la.prns, la.grid[0], la.grid[1], la.peaks, st["sync"], st["lock"], st["nav"], st["obs"], st["eph"],
                     want_det=want_det, trace=trace)
    return acq, det, st, trace


def _same(got, want, what):
    acq, det, st = got
    w_acq, w_det, w_st = want[:3]
    G.same_rows(acq, w_acq, (what, "acq"))
    if w_det is not None:
        for r in range(len(acq)):
            G.same_rows(det[r], w_det[r], (what, "det of receiver", r))
    for k in NAMES:
        if w_st[k] is not None:
            G.same_rows(st[k], w_st[k], (what, k))


# ---- 1: the table, byte for byte, at every edge of the launch's shape ------------------------------------------------------------------
# (group, n_rx, n_prn, n_dopp, ch_per_rx, NULL state arrays, evict_after_blocks or None: the group's)
SHAPES = [("A", AC.n_entries("A"), AC.N_PRN, AC.N_DOPP, AC.CH, (), None),      # the canonical shape: what the predicates were proven at
          ("B", AC.n_entries("B"), AC.N_PRN, AC.N_DOPP, AC.CH, (), None),
          ("C", AC.n_entries("C"), AC.N_PRN, AC.N_DOPP, AC.CH, (), None),
          ("D", AC.n_entries("D"), AC.N_PRN, AC.N_DOPP, AC.CH, (), None),
          ("A", 1, 1, 1, 1, (), None),
          ("A", 3, 33, 63, 33, ("nav",), None),
          ("A", 4, 64, 64, 64, ("obs",), None),
          ("A", 5, 5, 65, 4, ("eph",), None),
          ("A", 67, 32, 201, 5, (), None),
          ("B", 5, 32, 201, 64, ("nav", "obs", "eph"), None),
          # ... and of the kernel's own bin stride, four bins per lane and turn: 256.  The rows' bins are spread over the launch's, so row
          # winners lie in the second and later turns, and the last turn is cut off after one, after none and after all four of its loads
          ("A", AC.n_entries("A"), 5, 255, 4, (), None),
          ("A", 5, 33, 256, 5, (), None),
          ("A", AC.n_entries("A"), 5, 257, 4, (), None),
          ("A", 5, 32, 513, 5, (), None),
          ("B", 3, 6, 1025, 4, (), None),
          ("A", 3, 5, 833, 4, (), None),
          ("A", 67, 5, 8, 4, ("lock",), 0),                                     # no lock states: nothing can be evicted
          ("D", 4, 64, 201, 1, ("lock", "nav", "obs", "eph"), 0)]
SHAPE_IDS = [f"{s[0]}-{s[1]}rx-{s[2]}prn-{s[3]}bins-{s[4]}ch" + ("-no_" + "_".join(s[5]) if s[5] else "") for s in SHAPES]


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_the_table_matches_the_restatement(eng, shape):
    group, n_rx, n_prn, n_dopp, ch, nulls, evict = shape
    la = AC.launch(group, n_rx, n_prn, n_dopp, ch)
    cfg = la.cfg if evict is None else dict(la.cfg, evict_after_blocks=evict)
    want = _want(la, nulls, cfg)
    got = _call(eng, la, True, nulls, cfg)
    _same(got, want, shape)
    # what the definition leaves alone, said once more without the restatement: a slot that is neither handed over nor evicted keeps
    # every byte in all five arrays -- kept slots, empty slots that stay empty, and with them whole neighbouring receivers
    for r, t in enumerate(want[3]):
        for j in range(ch):
            if j not in t["written"]:
                for k in NAMES:
                    if k not in nulls:
                        assert got[2][k][r * ch + j].tobytes() == la.states[k][r * ch + j].tobytes(), (shape, r, j, k)
    if group == "A" and (n_prn, n_dopp, ch) == (AC.N_PRN, AC.N_DOPP, AC.CH) and not nulls:
        seen = set()
        for r, row in enumerate(la.rows):          # the predicates, on the DEVICE's bytes
            if row is not None and row.name not in seen:
                assert row.check(AC.outcome(la, r, got[0], got[1], got[2], want[3])), row.name
                seen.add(row.name)
        assert len(seen) == len([r for r in AC.ROWS if r.group == "A"])


# ---- 2: call equivalences ----------------------------------------------------------------------------------------------------------------
def test_host_variant_device_variant_and_binding_agree(eng):
    la = AC.launch("A", 9, 33, 65, 5)
    want = _want(la)
    _same(_call(eng, la, True), want, "dev")
    _same(_call(eng, la, False), want, "host")
    for want_det in (True, False):
        _same(_call(eng, la, False, want_det=want_det), _want(la, want_det=want_det), ("host, det", want_det))
        _same(_call(eng, la, True, want_det=want_det), _want(la, want_det=want_det), ("dev, det", want_det))
    with G.Pool() as pool:
        st = {k: pool.add(G.Guarded(eng, la.states[k].nbytes, G.STATE_FILL, la.states[k])) for k in NAMES}
        acq, det = eng.wacq(Q.cfg_record(la.cfg), la.peaks, la.prns, la.grid[0], la.grid[1], *[st[k].ptr.value for k in NAMES])
        after = {k: st[k].get(la.states[k].dtype, la.states[k].shape) for k in NAMES}
    _same((acq, det, after), want, "Engine.wacq")


def test_a_second_call_tracks_what_the_first_handed_over_and_writes_nothing(eng):
    la = AC.launch("A", AC.n_entries("A"), 32, 65, 5)
    first = _call(eng, la, True)
    second = _call(eng, la, True, states=first[2])
    _same(second, _want(la, states=first[2]), "second call")
    for k in NAMES:
        assert second[2][k].tobytes() == first[2][k].tobytes(), k
    assert not second[0]["n_assigned"].any() and not second[0]["n_evicted"].any() and not second[0]["assigned_mask"].any()
    f1, f2 = first[1]["flags"], second[1]["flags"]
    held = (f1 & (Q.DET_ASSIGNED | Q.DET_TRACKED)) != 0
    assert held.any() and (f2[held] == Q.DET_DETECTED | Q.DET_TRACKED).all()
    dropped = (f1 & Q.DET_DROPPED) != 0
    assert dropped.any() and (f2[dropped] == Q.DET_DETECTED | Q.DET_DROPPED).all()
    assert (f2[(f1 & Q.DET_DETECTED) == 0] == 0).all()
    # ... and where nothing was dropped, every detected PRN is TRACKED
    whole = first[0]["n_dropped"] == 0
    assert whole.any() and (second[0]["n_tracked"][whole] == second[0]["n_detected"][whole]).all()


def test_receivers_permuted_give_the_same_bytes_permuted(eng):
    la = AC.launch("A", 13, 33, 63, 5)
    perm = np.random.default_rng(5).permutation(la.n_rx)
    slots = (perm[:, None] * la.ch + np.arange(la.ch)[None, :]).reshape(-1)
    lb = AC.launch("A", 13, 33, 63, 5)
    lb.peaks, lb.states = np.ascontiguousarray(la.peaks[perm]), {k: np.ascontiguousarray(v[slots]) for k, v in la.states.items()}
    a, b = _call(eng, la, True), _call(eng, lb, True)
    assert a[0][perm].tobytes() == b[0].tobytes() and a[1][perm].tobytes() == b[1].tobytes()
    for k in NAMES:
        assert a[2][k][slots].tobytes() == b[2][k].tobytes(), k


# ---- 3: refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_with_their_text_and_write_nothing(eng):
    """(the last clause of the header's list, a size product that overflows, cannot be reached where a size has 64 bits: n_search
    x n_prn x n_dopp x 16 stays below 2^20 x 2^6 x 2^20 x 2^4)"""
    from stm32f4_sdr_gps_amd import capi
    la = AC.launch("A", 3)
    nan, inf = float("nan"), float("inf")
    good = dict(null=None, ch=la.ch, det=(5, 2), lead=80, k=float(AC.WAID_L1CA), evict=1000, reserved=0, n_rx=la.n_rx, n_prn=la.n_prn, n_dopp=la.n_dopp,
                grid=la.grid, prns=[int(v) for v in la.prns])
    by_message = {
        b"null argument": [dict(null=w) for w in ("cfg", "g", "prns", "peaks", "sync", "acq")] + [dict(null="acq", ch=0)],
        b"ch_per_rx must be 1..64": [dict(ch=0), dict(ch=65), dict(ch=-1, det=(0, 0))],
        b"det_num and det_den must be 1..1024, det_num >= det_den": [dict(det=(0, 1)), dict(det=(1, 0)), dict(det=(1025, 1)), dict(det=(1024, 1025)),
                                                                     dict(det=(3, 4)), dict(det=(-4, -5), lead=-1)],
        b"lead_blocks must be 0..4096": [dict(lead=-1), dict(lead=4097), dict(lead=4097, k=nan)],
        b"code_per_hz must be finite and -1..1": [dict(k=nan), dict(k=inf), dict(k=-1.5), dict(k=1.0000001, evict=-1)],
        b"evict_after_blocks must be 0..1073741824": [dict(evict=-1), dict(evict=(1 << 30) + 1), dict(evict=-5, reserved=1)],
        b"reserved must be 0": [dict(reserved=1), dict(reserved=-1, null="lock")],
        b"evict_after_blocks needs d_lock_state": [dict(null="lock"), dict(null="lock", evict=1, n_rx=0)],
        b"n_search must be 1..1048576": [dict(n_rx=0), dict(n_rx=-1), dict(n_rx=(1 << 20) + 1), dict(n_rx=0, n_prn=0)],
        b"n_prn must be 1..64": [dict(n_prn=0), dict(n_prn=65, prns=list(range(1, 66))), dict(n_prn=-3, n_dopp=0)],
        b"n_dopp must be 1..1048576": [dict(n_dopp=0), dict(n_dopp=-1, prns=[0] * la.n_prn), dict(n_dopp=(1 << 20) + 1, grid=(0, 0)),
                                       dict(n_dopp=(1 << 31) - 1, grid=(-5000, 0)), dict(n_dopp=(1 << 31) - 200, grid=(0, 1))],
        b"PRN outside 1..210": [dict(prns=[0] + good["prns"][1:]), dict(prns=good["prns"][:-1] + [211]), dict(prns=[255] * la.n_prn)],
        b"a PRN is listed twice": [dict(prns=good["prns"][:-1] + good["prns"][:1]), dict(prns=[7] * la.n_prn, grid=((1 << 31) - 1, 1))],
        b"a Doppler bin lies outside int32": [dict(grid=((1 << 31) - 1, 1)), dict(grid=(-(1 << 31), -1)), dict(grid=(0, (1 << 31) - 1), k=1.0, lead=4096)],
        b"the projection must stay below one code period (|code_per_hz| x max |Doppler| x lead_blocks x 0.001 < 16368)":
            [dict(k=1.0, lead=4096), dict(k=-1.0, lead=4096, grid=(5000, -1500)), dict(k=1.0, lead=1, grid=(-16368000, 1))],
    }
    with G.Pool() as pool:
        st = {k: pool.add(G.Guarded(eng, la.states[k].nbytes, G.STATE_FILL, la.states[k])) for k in NAMES}
        d_pk = pool.add(G.Guarded(eng, la.peaks.nbytes, G.STATE_FILL, la.peaks))
        outs = {dev: (pool.add(G.Guarded(eng if dev else None, la.n_rx * Q.ACQ_DTYPE.itemsize)),
                      pool.add(G.Guarded(eng if dev else None, la.n_rx * la.n_prn * Q.DET_DTYPE.itemsize))) for dev in (True, False)}
        fns = {True: eng.lib.gpsx_wacq_dev, False: eng.lib.gpsx_wacq}

        def call(a, dev):
            cfg = Q.cfg_record(Q.make_cfg(a["ch"], a["det"], 1000, a["lead"], a["k"], a["evict"]))
            cfg["reserved"] = a["reserved"]
            prns = np.array(a["prns"], np.uint8)
            g = capi.AcqWeightedT(a["n_rx"], 0, a["n_prn"], None if a["null"] == "prns" else prns.ctypes.data_as(C.POINTER(C.c_uint8)),
                                  a["grid"][0], a["grid"][1], a["n_dopp"], 1)
            null = a["null"]
            return fns[dev](eng.h, None if null == "cfg" else cfg.ctypes.data, None if null == "g" else C.addressof(g),
                            None if null == "peaks" else (d_pk.ptr if dev else la.peaks.ctypes.data), None if null == "sync" else st["sync"].ptr,
                            None if null == "lock" else st["lock"].ptr, st["nav"].ptr, st["obs"].ptr, st["eph"].ptr,
                            None if null == "acq" else outs[dev][0].ptr, outs[dev][1].ptr)
        G.refusals(eng, by_message, good, call, [*st.values(), d_pk, *outs[True], *outs[False]])
        # the limits themselves are accepted
        for change in (dict(det=(1024, 1024)), dict(det=(1, 1)), dict(lead=4096, k=0.5), dict(evict=1 << 30), dict(k=-1.0, lead=1)):
            for dev in (False, True):
                assert call({**good, **change}, dev) == 0, (change, eng.lib.gpsx_last_error(eng.h))
                assert eng.lib.gpsx_synchronize(eng.h) == 0


# ---- 4: the chain on the device: IF samples -> grid -> decisions -> loop -> words -> lock, and a lost slot re-acquired --------------------
def _grid_dev(eng, prns, n_search, stride, d_if_at, n_blocks, d_peaks):
    g, keep = _desc(prns, n_search, AC.SCN_GRID[:2], AC.SCN_GRID[2])
    g.search_stride_blocks = stride
    eng._chk(eng.lib.gpsx_acq_grid_weighted_hyb_dev(eng.h, C.addressof(g), AC.SCN_COH, AC.SCN_SEG, C.c_void_p(d_if_at), n_blocks, d_peaks), "grid")
    return g, keep


def _wacq_dev(eng, cfg, g, d_peaks, chain, d_acq, d_det):
    eng._chk(eng.lib.gpsx_wacq_dev(eng.h, cfg.ctypes.data, C.addressof(g), d_peaks, *[chain.buf[k].ptr for k in NAMES], d_acq, d_det), "gpsx_wacq_dev")
    assert eng.lib.gpsx_last_kernel(eng.h) == b"k_wacq"


def _launches(eng, chain, d_if, first, n_launches, n=500):
    """sync loop, words and lock monitor over n_launches x n blocks from block `first` -> the last launch's lock records"""
    for i in range(n_launches):
        chain.sync(d_if.ptr.value + (first + i * n) * 4092, n)
        chain.words()
        chain.lock()
    assert eng.lib.gpsx_synchronize(eng.h) == 0
    return chain.read("l")


def test_two_receivers_from_if_samples_to_code_lock_and_a_lost_slot_re_acquired(eng):
    """weighted_acq_cases' scenario on the device.  gpsx_acq_grid_weighted_hyb_dev (10 x 8 blocks, n_search = 2, stride = the multi
    loop's rx_stride_blocks) on the two receivers' streams, gpsx_wacq_dev behind it with lead_blocks = 80 and GPSX_WAID_L1CA: its
    outputs and the five state arrays equal the restatement applied to the device's own peak records, each receiver's three satellites
    sit in slots 0 .. 2; gpsx_track_loop_weighted_sync_multi_dev from block 80, gpsx_wnav_words_dev and gpsx_wlock_dev for 1000 blocks:
    every handed-over slot has GPSX_WLOCK_CODE and a code ratio of at least weighted_multi_cases.MEASURED's smallest of a present
    satellite, the empty slots have no record.  Then receiver 0 alone, slot 0 holding PRN 3, which its stream lacks: a grid and a
    call on PRNs 7 and 19, 1000 blocks, and -- enqueued without a look at a peak or a state in between -- a grid over blocks 1000 .. 1079
    on PRNs 7, 19, 30, 3 and a call with evict_after_blocks = 1000: 7 and 19 TRACKED, slot 0 evicted and handed to PRN 30, which reaches
    GPSX_WLOCK_CODE within the next 1000 blocks.  (On the CPU restatements the code ratios are 2.94 .. 3.80 on the first leg and 3.64 ..
    4.10 at the end of the second.)"""
    import weighted_lock_cases as X
    import weighted_lock_ref as R
    import weighted_multi_cases as M
    import weighted_sync_cases as K
    from stm32f4_sdr_gps_amd import capi
    stride = M.CHAIN_MS + M.EXTRA
    streams = M.streams_of([AC.scenario_blocks(r) for r in range(2)], stride)
    n_peaks = len(AC.SCN_PRNS) * AC.SCN_GRID[2]
    lock_cfg, sync_cfg = R.cfg_array(X.scenario_cfg(0)), G.sync_cfg(K.sync_cfg())
    with G.Pool() as pool:
        d_if = pool.add(G.Guarded(eng, streams.nbytes, G.STATE_FILL, streams))
        d_pk = pool.add(G.Guarded(eng, 2 * n_peaks * Q.PEAK_DTYPE.itemsize))
        d_acq, d_det = pool.add(G.Guarded(eng, 2 * Q.ACQ_DTYPE.itemsize)), pool.add(G.Guarded(eng, 2 * len(AC.SCN_PRNS) * Q.DET_DTYPE.itemsize))
        # -- both receivers
        st0 = AC.empty_states(2 * AC.SCN_CH)
        cfg = AC.scenario_cfg(AC.SCN_COH * AC.SCN_SEG)
        with G.Chain(eng, sync_cfg, st0, 500, lock_cfg=lock_cfg, rx=capi.wmulti(2, AC.SCN_CH, stride)) as chain:
            g, keep = _grid_dev(eng, AC.SCN_PRNS, 2, stride, d_if.ptr.value, 2 * stride, d_pk.ptr)
            _wacq_dev(eng, Q.cfg_record(cfg), g, d_pk.ptr, chain, d_acq.ptr, d_det.ptr)
            assert eng.lib.gpsx_synchronize(eng.h) == 0
            peaks = d_pk.get(Q.PEAK_DTYPE, (2, len(AC.SCN_PRNS), AC.SCN_GRID[2]))
            want, trace = {k: v.copy() for k, v in st0.items()}, []
            w_acq, w_det = Q.run(cfg, AC.SCN_PRNS, AC.SCN_GRID[0], AC.SCN_GRID[1], peaks, *[want[k] for k in NAMES], trace=trace)
            _same((d_acq.get(Q.ACQ_DTYPE, (2,)), d_det.get(Q.DET_DTYPE, (2, len(AC.SCN_PRNS))), {k: chain.read(k) for k in NAMES}), (w_acq, w_det, want),
                  "the device's own records")
            handed = []
            for r in range(2):
                assert sorted(trace[r]["assigned"]) == AC.scenario_present(r) and sorted(trace[r]["assigned"].values()) == [0, 1, 2], (r, trace[r])
                handed += [r * AC.SCN_CH + j for j in range(3)]
            lock = _launches(eng, chain, d_if, AC.SCN_COH * AC.SCN_SEG, 2)
            print("code ratios of the handed-over slots", lock["code_ratio"][handed], "flags", lock["flags"][handed])
            assert ((lock["flags"][handed] & R.F_CODE) != 0).all() and (lock["code_ratio"][handed] >= M.MEASURED["code_present_min"]).all()
            empty = [c for c in range(2 * AC.SCN_CH) if c not in handed]
            assert not lock["flags"][empty].any() and (chain.read("rec")["flags"][:, empty] == 0).all()
        # -- receiver 0 alone: a slot that holds a PRN its stream lacks
        st0 = AC.again_states()
        cfg = AC.scenario_cfg(0, AC.SCN_EVICT)
        with G.Chain(eng, sync_cfg, st0, 500, lock_cfg=lock_cfg, rx=capi.wmulti(1, AC.SCN_CH, stride)) as chain:
            g, keep = _grid_dev(eng, AC.SCN_PRNS[:2], 1, stride, d_if.ptr.value, stride, d_pk.ptr)
            _wacq_dev(eng, Q.cfg_record(cfg), g, d_pk.ptr, chain, d_acq.ptr, d_det.ptr)
            lock = _launches(eng, chain, d_if, 0, AC.SCN_AGAIN_AT // 500)
            assert [int(f) & R.F_CODE for f in lock["flags"][:3]] == [0, R.F_CODE, R.F_CODE], lock[:3]
            before = {k: chain.read(k) for k in NAMES}
            assert [int(v) for v in before["sync"]["loop"]["prn"]] == [3, 7, 19, Q.PRN_NONE, Q.PRN_NONE]
            d_pk.refill()
            d_acq.refill()
            d_det.refill()
            g, keep = _grid_dev(eng, AC.SCN_AGAIN_PRNS, 1, stride, d_if.ptr.value + AC.SCN_AGAIN_AT * 4092, stride - AC.SCN_AGAIN_AT, d_pk.ptr)
            _wacq_dev(eng, Q.cfg_record(cfg), g, d_pk.ptr, chain, d_acq.ptr, d_det.ptr)       # (nothing read since the grid was enqueued)
            assert eng.lib.gpsx_synchronize(eng.h) == 0
            peaks = d_pk.get(Q.PEAK_DTYPE, (1, len(AC.SCN_AGAIN_PRNS), AC.SCN_GRID[2]))
            trace = []
            w_acq, w_det = Q.run(cfg, AC.SCN_AGAIN_PRNS, AC.SCN_GRID[0], AC.SCN_GRID[1], peaks, *[before[k] for k in NAMES], trace=trace)
            _same((d_acq.get(Q.ACQ_DTYPE, (1,)), d_det.get(Q.DET_DTYPE, (1, len(AC.SCN_AGAIN_PRNS))), {k: chain.read(k) for k in NAMES}),
                  (w_acq, w_det, before), "the second call")
            t = trace[0]
            assert t["tracked"] == [0, 1] and t["evicted"] == [0] and t["assigned"] == {2: 0} and t["written"] == [0], t
            assert int(before["sync"]["loop"]["prn"][0]) == 30
            lock = _launches(eng, chain, d_if, AC.SCN_AGAIN_AT, 2)
            print("code ratios after the re-acquisition", lock["code_ratio"][:3], "flags", lock["flags"][:3])
            assert ((lock["flags"][:3] & R.F_CODE) != 0).all() and (lock["code_ratio"][:3] >= M.MEASURED["code_present_min"]).all()
