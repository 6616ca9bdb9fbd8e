"""k_acq_win on the GPU (include/gpsx.h gpsx_acq_window_weighted): the table of tests/weighted_win_cases.py and seeded random launches at
every path of the kernel through gpsx_acq_window_weighted_dev, records and reports byte for byte between canaries against the
restatement (nothing here is a float tolerance: steps 1 and 2 are single IEEE operations, the rest is integers); the host variant, the
_dev variant and the binding; a second call; permuted receivers; every refusal with its text; the device's own full grid as a second
witness; the scenario from the predictions to code lock behind the chain driver; the almanac warm start from gpsx_wpred_dev's own records
to code lock; a launch that has to be cut in two; and the committed smoke fixture."""
import ctypes as C
import os

import numpy as np
import pytest

import weighted_acq_cases as AC
import weighted_acq_ref as Q
import weighted_gpu as G
import weighted_win_cases as WC
import weighted_win_ref as V
from weighted_gpu import EINVAL, eng  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sync", "lock", "nav", "obs", "eph")


@pytest.fixture(scope="module")
def oracle():
    from oracle import pyoracle
    return pyoracle.Oracle()


def _desc(la):
    """the gpsx_acq_weighted_t of launch `la` (and what keeps its PRN list alive)"""
    from stm32f4_sdr_gps_amd import capi
    prns = np.ascontiguousarray(la.prns, np.uint8)
    return capi.AcqWeightedT(la.n_rx, la.stride, len(prns), prns.ctypes.data_as(C.POINTER(C.c_uint8)), la.grid[0], la.grid[1], la.grid[2], 1 if la.mag else 0), prns


def _call(eng, la, dev=True, want_rep=True):
    """gpsx_acq_window_weighted_dev (dev) or the host variant on launch `la`: predictions and blocks between canaries, the records and the
    reports between canaries and prefilled -> (peaks, rep or None)"""
    g, keep = _desc(la)
    cfg = V.cfg_record(la.cfg)
    blocks = np.ascontiguousarray(la.blocks, np.uint8)
    shape = (la.n_rx, la.n_prn, la.grid[2])
    fn = eng.lib.gpsx_acq_window_weighted_dev if dev else eng.lib.gpsx_acq_window_weighted
    where = eng if dev else None
    with G.Pool() as pool:
        pred = pool.add(G.Guarded(where, la.pred.nbytes, G.STATE_FILL, la.pred))
        blk = pool.add(G.Guarded(where, blocks.nbytes, G.STATE_FILL, blocks))
        pk = pool.add(G.Guarded(where, int(np.prod(shape)) * V.PEAK_DTYPE.itemsize))
        rep = pool.add(G.Guarded(where, la.n_rx * la.n_prn * V.REP_DTYPE.itemsize))
        rc = fn(eng.h, C.addressof(g), cfg.ctypes.data, pred.ptr, blk.ptr, len(blocks), pk.ptr, rep.ptr if want_rep else None)
        assert rc == 0, (rc, eng.lib.gpsx_last_error(eng.h))
        assert eng.lib.gpsx_last_kernel(eng.h) == b"k_acq_win"
        assert eng.lib.gpsx_synchronize(eng.h) == 0
        assert pred.untouched() and blk.untouched()
        if not want_rep:
            assert rep.untouched()
        return pk.get(V.PEAK_DTYPE, shape), rep.get(V.REP_DTYPE, shape[:2]) if want_rep else None


def _same(got, want, what):
    peaks, rep = got
    w_peaks, w_rep = want
    if rep is not None:
        G.same_rows(rep.reshape(-1), w_rep.reshape(-1), (what, "rep"))
    flat, w_flat = peaks.reshape(-1, peaks.shape[2]), w_peaks.reshape(-1, peaks.shape[2])
    bad = [u for u in range(len(flat)) if flat[u].tobytes() != w_flat[u].tobytes()]
    if bad:
        d = [i for i in range(flat.shape[1]) if flat[bad[0], i] != w_flat[bad[0], i]][0]
        assert not bad, (what, "peaks of units", bad[:6], "bin", d, flat[bad[0], d], w_flat[bad[0], d], None if rep is None else rep.reshape(-1)[bad[0]])


# ---- 1: the table and the random launches, byte for byte -----------------------------------------------------------------------------------
@pytest.mark.parametrize("group", sorted(WC.GROUPS))
def test_the_table_matches_the_restatement(eng, oracle, group):
    la = WC.launch(oracle, group)
    peaks, rep, energies = WC.restated(oracle, la)
    got = _call(eng, la)
    _same(got, (peaks, rep), group)
    for row, r, p in la.units:                     # the predicates, on the DEVICE's bytes
        assert row.check(WC.outcome(la, row, r, p, got[0], got[1], energies)), row.name


@pytest.mark.parametrize("i", range(len(WC.SHAPES)), ids=["-".join(str(v) for v in s) for s in WC.SHAPES])
def test_random_launches_match_the_restatement(eng, oracle, i):
    la = WC.random_launch(i)
    want = V.run(oracle, la.cfg, la.pred, la.blocks, la.prns, *la.grid, use_magnitude=la.mag, stride=la.stride)
    _same(_call(eng, la), want, WC.SHAPES[i])
    _same(_call(eng, la, want_rep=False), want, (WC.SHAPES[i], "no report"))


# ---- 2: call equivalences ----------------------------------------------------------------------------------------------------------------
def test_host_variant_device_variant_and_binding_agree(eng, oracle):
    la = WC.random_launch(1)
    want = V.run(oracle, la.cfg, la.pred, la.blocks, la.prns, *la.grid, use_magnitude=la.mag, stride=la.stride)
    for dev in (True, False):
        for want_rep in (True, False):
            _same(_call(eng, la, dev, want_rep), want, ("dev" if dev else "host", want_rep))
    from stm32f4_sdr_gps_amd import capi
    cfg = capi.acq_window_cfg(la.cfg["n_coh"], la.cfg["n_seg"], la.cfg["half_width"], la.cfg["half_bins"], la.cfg["guard"])
    _same(eng.acq_window(cfg, la.pred, la.blocks, la.prns, *la.grid, use_magnitude=la.mag, stride_blocks=la.stride), want, "Engine.acq_window")
    assert eng.lib.gpsx_last_kernel(eng.h) == b"k_acq_win"
    peaks = eng.acq_window(cfg, la.pred, la.blocks, la.prns, *la.grid, use_magnitude=la.mag, stride_blocks=la.stride, want_rep=False)
    _same((peaks, None), want, "Engine.acq_window without the report")
    with G.Pool() as pool:
        blocks = np.ascontiguousarray(la.blocks)
        d_pred, d_blk = pool.add(G.Guarded(eng, la.pred.nbytes, G.STATE_FILL, la.pred)), pool.add(G.Guarded(eng, blocks.nbytes, G.STATE_FILL, blocks))
        d_pk, d_rep = pool.add(G.Guarded(eng, want[0].nbytes)), pool.add(G.Guarded(eng, want[1].nbytes))
        eng.acq_window_dev(cfg, d_pred.ptr.value, d_blk.ptr.value, len(blocks), la.n_rx, la.prns, *la.grid, d_pk.ptr.value, d_rep.ptr.value, use_magnitude=la.mag,
                           stride_blocks=la.stride)
        eng.synchronize()
        _same((d_pk.get(V.PEAK_DTYPE, want[0].shape), d_rep.get(V.REP_DTYPE, want[1].shape)), want, "Engine.acq_window_dev")


def test_a_second_call_gives_the_same_bytes(eng, oracle):
    la = WC.launch(oracle, "G")
    first, second = _call(eng, la), _call(eng, la)
    assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()
    lb = WC.random_launch(3)                        # ... and with another shape in between
    _call(eng, lb)
    third = _call(eng, la)
    assert first[0].tobytes() == third[0].tobytes() and first[1].tobytes() == third[1].tobytes()


def test_receivers_permuted_give_the_same_bytes_permuted(eng):
    order = [3, 0, 4, 2, 1]
    la, lb = WC.random_launch(2), WC.random_launch(2, permute=order)
    a, b = _call(eng, la), _call(eng, lb)
    assert a[0][order].tobytes() == b[0].tobytes() and a[1][order].tobytes() == b[1].tobytes()
    assert (a[1]["flags"] & V.SEARCHED).sum() >= 10


# ---- 3: refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_with_their_text_and_write_nothing(eng):
    """(the last clause of the header's list, a size product that overflows, cannot be reached where a size has 64 bits)"""
    from stm32f4_sdr_gps_amd import capi
    la = WC.random_launch(1)
    blocks = np.ascontiguousarray(la.blocks)
    n_rx, n_prn, n_dopp = la.n_rx, la.n_prn, la.grid[2]
    good = dict(null=None, n_coh=2, n_seg=2, w=7, d=1, guard=3, need=6, skip=48, reserved=0, weights=1, grid=(la.grid[0], la.grid[1]), n_rx=n_rx, n_prn=n_prn,
                n_dopp=n_dopp, stride=0, prns=[int(v) for v in la.prns], n_blocks=len(blocks), misalign=None)
    by_message = {
        b"null argument": [dict(null=w) for w in ("g", "cfg", "prns", "pred", "blocks", "peaks")] + [dict(null="peaks", n_coh=0)],
        b"n_coh outside 1..20": [dict(n_coh=0), dict(n_coh=21), dict(n_coh=-1, n_seg=0)],
        b"n_seg outside 1..128": [dict(n_seg=0), dict(n_seg=129), dict(n_seg=-1, w=0)],
        b"half_width must be 1..2047": [dict(w=0, guard=0), dict(w=2048), dict(w=-1, d=-1)],
        b"half_bins must be 0..32": [dict(d=-1), dict(d=33), dict(d=33, guard=7)],
        b"guard must be 0..half_width - 1": [dict(guard=-1), dict(guard=7), dict(guard=8, need=0)],
        b"need_flags and skip_flags must be GPSX_WPRED_* bits": [dict(need=2 | 128), dict(skip=1 << 31), dict(need=0x80, skip=0x100)],
        b"need_flags must contain GPSX_WPRED_PREDICTED": [dict(need=0), dict(need=4), dict(need=0x7D, reserved=1)],
        b"reserved must be 0": [dict(reserved=1), dict(reserved=-1, weights=2)],
        b"unknown weights": [dict(weights=2), dict(weights=-1, grid=(0, 0))],
        b"dopp_step_hz must be at least 1": [dict(grid=(0, 0)), dict(grid=(0, -300)), dict(grid=(0, 0), n_rx=0)],
        b"n_search must be 1..1048576": [dict(n_rx=0), dict(n_rx=-1), dict(n_rx=(1 << 20) + 1), dict(n_rx=0, n_prn=0)],
        b"n_prn must be 1..64": [dict(n_prn=0), dict(n_prn=65, prns=list(range(1, 66))), dict(n_prn=-3, n_dopp=0)],
        b"n_dopp must be 1..1048576": [dict(n_dopp=0), dict(n_dopp=-1), dict(n_dopp=(1 << 20) + 1), dict(n_dopp=0, stride=-1)],
        b"search_stride_blocks must be at least 0": [dict(stride=-1), dict(stride=-(1 << 31), prns=[0] * n_prn)],
        b"PRN outside 1..210": [dict(prns=[0] + good["prns"][1:]), dict(prns=good["prns"][:-1] + [211]), dict(prns=[255] * n_prn)],
        b"a PRN is listed twice": [dict(prns=[good["prns"][0]] * n_prn), dict(prns=[7] * n_prn, grid=((1 << 31) - 1, 1))],
        b"a Doppler bin lies outside int32": [dict(grid=((1 << 31) - 1, 1)), dict(grid=(0, (1 << 31) - 1)), dict(grid=((1 << 31) - 3, 1), n_blocks=1)],
        b"not enough blocks for the searches": [dict(n_blocks=3), dict(n_blocks=0), dict(n_blocks=-1), dict(stride=1, n_blocks=4), dict(n_coh=20, n_seg=128),
                                                dict(stride=(1 << 31) - 1)],
    }
    dev_only = {b"d_pred and d_rep must be 16-byte aligned": [dict(misalign="pred"), dict(misalign="rep")]}
    with G.Pool() as pool:
        bufs = {}
        for dev in (True, False):
            where = eng if dev else None
            padded = np.concatenate([np.ascontiguousarray(la.pred).view(np.uint8).reshape(-1), np.zeros(16, np.uint8)])      # (room for the misaligned call)
            bufs[dev] = dict(pred=pool.add(G.Guarded(where, padded.nbytes, G.STATE_FILL, padded)),
                             blocks=pool.add(G.Guarded(where, blocks.nbytes, G.STATE_FILL, blocks)),
                             peaks=pool.add(G.Guarded(where, n_rx * n_prn * n_dopp * 16)), rep=pool.add(G.Guarded(where, n_rx * n_prn * 16 + 16)))
        fns = {True: eng.lib.gpsx_acq_window_weighted_dev, False: eng.lib.gpsx_acq_window_weighted}

        def call(a, dev):
            cfg = V.cfg_record(V.make_cfg(a["n_coh"], a["n_seg"], a["w"], a["d"], a["guard"], a["need"], a["skip"]))
            cfg["reserved"] = a["reserved"]
            prns = np.array(a["prns"], np.uint8)
            g = capi.AcqWeightedT(a["n_rx"], a["stride"], a["n_prn"], None if a["null"] == "prns" else prns.ctypes.data_as(C.POINTER(C.c_uint8)),
                                  a["grid"][0], a["grid"][1], a["n_dopp"], a["weights"])
            null, b = a["null"], bufs[dev]
            ptr = lambda k: None if null == k else C.c_void_p(b[k].ptr.value + (8 if a["misalign"] == k else 0))      # noqa: E731
            return fns[dev](eng.h, None if null == "g" else C.addressof(g), None if null == "cfg" else cfg.ctypes.data, ptr("pred"), ptr("blocks"),
                            a["n_blocks"], ptr("peaks"), ptr("rep"))
        every = [b for dev in bufs for b in bufs[dev].values()]
        G.refusals(eng, by_message, good, call, every)
        for message, changes in dev_only.items():
            for change in changes:
                assert call({**good, **change}, True) == EINVAL and eng.lib.gpsx_last_error(eng.h) == message, change
                eng.synchronize()
                assert all(b.untouched() for b in every)
        # the limits themselves are accepted
        for change in (dict(guard=6), dict(guard=0), dict(need=2, skip=0x7D), dict(need=0x7F, skip=0), dict(d=0), dict(d=32), dict(w=1, guard=0),
                       dict(n_blocks=4), dict(grid=((1 << 31) - n_dopp, 1))):
            for dev in (False, True):
                assert call({**good, **change}, dev) == 0, (change, eng.lib.gpsx_last_error(eng.h))
                assert eng.lib.gpsx_synchronize(eng.h) == 0


# ---- 4: device against device ------------------------------------------------------------------------------------------------------------
def test_the_devices_own_grid_is_a_second_witness(eng, oracle):
    """gpsx_acq_grid_weighted_hyb_dev on the same blocks, PRNs and lattice: every searched unit whose grid record has its phase in the
    window has that record's max_val and phase -- the top of the range (group T), the two ties (group Q) and windows laid around the
    grid's own phases, at and one beyond their edges"""
    from stm32f4_sdr_gps_amd import capi
    inside = 0
    for group in ("T", "Q", "E"):
        la = WC.launch(oracle, group)
        blocks = np.ascontiguousarray(la.blocks)
        g, keep = _desc(la)
        shape = (la.n_rx, la.n_prn, la.grid[2])
        with G.Pool() as pool:
            d_blk = pool.add(G.Guarded(eng, blocks.nbytes, G.STATE_FILL, blocks))
            d_full = pool.add(G.Guarded(eng, int(np.prod(shape)) * 16))
            eng._chk(eng.lib.gpsx_acq_grid_weighted_hyb_dev(eng.h, C.addressof(g), la.cfg["n_coh"], la.cfg["n_seg"], d_blk.ptr, len(blocks), d_full.ptr), "grid")
            assert eng.lib.gpsx_synchronize(eng.h) == 0
            full = d_full.get(capi.PEAK_DTYPE, shape)
        if group == "E":                           # predictions around the grid's own phases of PRN index 0, bin 2
            offs = (-7, -3, 0, 3, 7, 8, -8, 5, 1, -1, 2, -2)[:la.n_rx]
            pred = V.make_pred(la.n_rx, la.n_prn)
            for r, off in enumerate(offs):
                V.set_pred(pred, r, 0, float((int(full[r, 0, 2]["phase"]) + off) % V.SAMPLES), 0.0)
            lb = _with(la, pred=pred)
        else:
            lb = la
        peaks, rep = _call(eng, lb)
        for r in range(lb.n_rx):
            for p in range(lb.n_prn):
                if not int(rep[r, p]["flags"]) & V.SEARCHED:
                    continue
                taus = set(V.window(int(rep[r, p]["centre"]), lb.cfg["half_width"]).tolist())
                for d in range(int(rep[r, p]["first_bin"]), int(rep[r, p]["first_bin"]) + int(rep[r, p]["n_bins"])):
                    gr, w = full[r, p, d], peaks[r, p, d]
                    if int(gr["phase"]) in taus:
                        inside += 1
                        assert (int(w["max_val"]), int(w["phase"])) == (int(gr["max_val"]), int(gr["phase"])), (group, r, p, d)
                    else:
                        assert int(w["max_val"]) <= int(gr["max_val"]), (group, r, p, d)
    print("units whose grid phase lies in the window:", inside)
    assert inside >= 12


def _with(la, **changes):
    from types import SimpleNamespace
    return SimpleNamespace(**{**vars(la), **changes})


# ---- 5: the scenario on the device: predictions -> window -> decisions -> loop -> lock ----------------------------------------------------
def test_two_receivers_from_predictions_to_code_lock(eng):
    """weighted_acq_cases' two receivers on the device, from fabricated prediction records (weighted_win_cases.scenario_pred: 40 samples
    and 130 Hz off the truth; the scenario has no orbits for gpsx_wpred_dev to predict from, so the records are uploaded where that call
    would have left them): gpsx_acq_window_weighted_dev (10 x 8 blocks, W 128, D 2, guard 32, stride = the multi loop's
    rx_stride_blocks), gpsx_wacq_dev behind it with the same descriptor and lead_blocks = 80 -- its outputs and the five state arrays
    equal the restatement applied to the device's own window records, each receiver's three satellites sit in slots 0 .. 2 --, then
    gpsx_track_loop_weighted_sync_multi_dev from block 80, gpsx_wnav_words_dev and gpsx_wlock_dev for 1000 blocks: all six reach
    GPSX_WLOCK_CODE with a code ratio of at least weighted_multi_cases.MEASURED's smallest of a present satellite, as from the full grid."""
    import weighted_lock_cases as X
    import weighted_lock_ref as R
    import weighted_multi_cases as M
    import weighted_sync_cases as K
    from stm32f4_sdr_gps_amd import capi
    stride = M.CHAIN_MS + M.EXTRA
    streams = M.streams_of([AC.scenario_blocks(r) for r in range(2)], stride)
    n_prn, n_dopp = len(AC.SCN_PRNS), AC.SCN_GRID[2]
    lock_cfg, sync_cfg = R.cfg_array(X.scenario_cfg(0)), G.sync_cfg(K.sync_cfg())
    pred, wcfg = WC.scenario_pred(), V.cfg_record(WC.scenario_cfg())
    prns = np.array(AC.SCN_PRNS, np.uint8)
    g = capi.AcqWeightedT(2, stride, n_prn, prns.ctypes.data_as(C.POINTER(C.c_uint8)), AC.SCN_GRID[0], AC.SCN_GRID[1], n_dopp, 1)
    with G.Pool() as pool:
        d_if = pool.add(G.Guarded(eng, streams.nbytes, G.STATE_FILL, streams))
        d_pred = pool.add(G.Guarded(eng, pred.nbytes, G.STATE_FILL, pred))
        d_pk, d_rep = pool.add(G.Guarded(eng, 2 * n_prn * n_dopp * 16)), pool.add(G.Guarded(eng, 2 * n_prn * 16))
        d_acq, d_det = pool.add(G.Guarded(eng, 2 * Q.ACQ_DTYPE.itemsize)), pool.add(G.Guarded(eng, 2 * n_prn * Q.DET_DTYPE.itemsize))
        st0 = AC.empty_states(2 * AC.SCN_CH)
        cfg = AC.scenario_cfg(AC.SCN_COH * AC.SCN_SEG)
        with G.Chain(eng, sync_cfg, st0, 500, lock_cfg=lock_cfg, rx=capi.wmulti(2, AC.SCN_CH, stride)) as chain:
            eng._chk(eng.lib.gpsx_acq_window_weighted_dev(eng.h, C.addressof(g), wcfg.ctypes.data, d_pred.ptr, d_if.ptr, 2 * stride, d_pk.ptr, d_rep.ptr),
                     "gpsx_acq_window_weighted_dev")
            assert eng.lib.gpsx_last_kernel(eng.h) == b"k_acq_win"
            eng._chk(eng.lib.gpsx_wacq_dev(eng.h, Q.cfg_record(cfg).ctypes.data, C.addressof(g), d_pk.ptr, *[chain.buf[k].ptr for k in NAMES], d_acq.ptr,
                                           d_det.ptr), "gpsx_wacq_dev")
            assert eng.lib.gpsx_synchronize(eng.h) == 0
            peaks, rep = d_pk.get(Q.PEAK_DTYPE, (2, n_prn, n_dopp)), d_rep.get(V.REP_DTYPE, (2, n_prn))
            assert (rep["flags"] == V.SEARCHED).all() and (rep["n_bins"] == 5).all()
            want, trace = {k: v.copy() for k, v in st0.items()}, []
            w_acq, w_det = Q.run(cfg, AC.SCN_PRNS, AC.SCN_GRID[0], AC.SCN_GRID[1], peaks, *[want[k] for k in NAMES], trace=trace)
            G.same_rows(d_acq.get(Q.ACQ_DTYPE, (2,)), w_acq, "acq")
            G.same_rows(d_det.get(Q.DET_DTYPE, (2, n_prn)).reshape(-1), w_det.reshape(-1), "det")
            for k in NAMES:
                G.same_rows(chain.read(k), want[k], k)
            handed = []
            for r in range(2):
                assert sorted(trace[r]["assigned"]) == AC.scenario_present(r) and sorted(trace[r]["assigned"].values()) == [0, 1, 2], (r, trace[r])
                handed += [r * AC.SCN_CH + j for j in range(3)]
            for i in range(2):
                chain.sync(d_if.ptr.value + (AC.SCN_COH * AC.SCN_SEG + i * 500) * 4092, 500)
                chain.words()
                chain.lock()
            assert eng.lib.gpsx_synchronize(eng.h) == 0
            lock = chain.read("l")
            print("code ratios of the handed-over slots", lock["code_ratio"][handed], "flags", lock["flags"][handed])
            assert ((lock["flags"][handed] & R.F_CODE) != 0).all() and (lock["code_ratio"][handed] >= M.MEASURED["code_present_min"]).all()
            empty = [c for c in range(2 * AC.SCN_CH) if c not in handed]
            assert not lock["flags"][empty].any()


# ---- 5b: from gpsx_wpred_dev's own records: the almanac warm start on the device -------------------------------------------------------------
def test_an_almanac_warm_start_behind_gpsx_wpred_dev(eng, oracle):
    """weighted_pvt_cases' stream through weighted_gpu.Chain with gpsx_wbank_dev, gpsx_wfix_dev, gpsx_wvel_dev and gpsx_wkf_dev after every
    launch, to the filter's INIT at block 24 576 (test_gpu_weighted_pred.py's way there).  The host then does what a warm start leaves to
    it: the bank's four entries become an almanac cut of the stream's ephemerides (gpsx_walm_to_eph's restatement).  From there nothing
    is read until the end: gpsx_wpred_dev (handover 0) on five-state arrays whose slots are all empty writes d_pred;
    gpsx_acq_window_weighted_dev reads d_pred where it lies (W 64, D 1, guard 16, 10 x 8 blocks from block 24 576, weighted_win_cases.
    WARM_GRID); gpsx_wacq_dev with the same descriptor and lead_blocks = 80; the sync loop, the word layer and gpsx_wlock_dev over the 344
    blocks that remain.  Then: the window records and reports are the restatement's on the device's own d_pred, byte for byte; the
    decisions and the states behind gpsx_wacq_dev are its restatement's on the device's own records; the four PRNs are acquired within 8
    samples and one bin of the synthesiser's truth, the three entries without a prediction are SKIPPED; all four slots reach
    GPSX_WLOCK_CODE.  Cost: the stream's synthesis (about 25 s of CPU, cached per process) and its upload, plus a few seconds of GPU."""
    import weighted_alm_cases as A
    import weighted_alm_ref as AR
    import weighted_coh_ref as CR
    import weighted_fix_ref as F
    import weighted_kf_ref as KR
    import weighted_lock_cases as X
    import weighted_lock_ref as R
    import weighted_pred_cases as PC
    import weighted_pred_ref as P
    import weighted_pvt_cases as S
    import weighted_vel_ref as VR
    from stm32f4_sdr_gps_amd import capi
    lib, n_ch, prns = eng.lib, 4, np.array(PC.STREAM_PRNS, np.uint8)
    four = [PC.STREAM_PRNS.index(prn) for prn in S.PRNS]
    blocks = S.blocks()
    fcfg, vcfg, kcfg = PC.stream_filter_cfgs()
    bcfg = P.bank_cfg_record(n_ch)
    bank0 = P.empty_bank(1, len(prns))
    n_dopp = WC.WARM_GRID[2]
    wcfg_d = V.make_cfg(10, 8, 64, 1, 16)
    wcfg, lead = V.cfg_record(wcfg_d), 80
    acfg = Q.make_cfg(n_ch, AC.SCN_DET, 0, lead, AC.WAID_L1CA, 0)
    g = capi.AcqWeightedT(1, 0, len(prns), prns.ctypes.data_as(C.POINTER(C.c_uint8)), WC.WARM_GRID[0], WC.WARM_GRID[1], n_dopp, 1)
    with G.Pool() as pool:
        d_if = pool.add(G.Guarded(eng, blocks.nbytes, G.STATE_FILL, blocks))
        buf = {k: pool.add(G.Guarded(eng, n)) for k, n in dict(out=n_ch * 256, rep=32, fix=F.FIX_DTYPE.itemsize, vel=VR.VEL_DTYPE.itemsize, kf=KR.KF_DTYPE.itemsize,
                                                              rx=64, pred=len(prns) * 64, peaks=len(prns) * n_dopp * 16, wrep=len(prns) * 16,
                                                              acq=Q.ACQ_DTYPE.itemsize, det=len(prns) * Q.DET_DTYPE.itemsize).items()}
        buf["bank"] = pool.add(G.Guarded(eng, bank0.nbytes, G.STATE_FILL, bank0))
        buf["state"] = pool.add(G.Guarded(eng, 384, G.STATE_FILL, np.zeros(1, KR.STATE_DTYPE)))
        with G.Chain(eng, S.sync_cfg_dev(S.MOVING), dict(S.fresh_states(), sync=S.handover()), max(S.LAUNCHES), S.MAX_BAD_WORDS, S.EDGE_GUARD) as a:
            at = 0
            for n in S.LAUNCHES[:-1]:
                a.sync(d_if.ptr.value + at * 4092, n)
                a.words()
                a.obs()
                a.eph()
                eng._chk(lib.gpsx_wbank_dev(eng.h, bcfg.ctypes.data, 1, len(prns), prns.ctypes.data, a.buf["sync"].ptr, a.buf["e"].ptr, buf["bank"].ptr,
                                            buf["out"].ptr, buf["rep"].ptr), "gpsx_wbank_dev")
                eng._chk(lib.gpsx_wfix_dev(eng.h, fcfg.ctypes.data, a.buf["o"].ptr, buf["out"].ptr, None, buf["fix"].ptr if at else None, 1, buf["fix"].ptr, None), "wfix")
                eng._chk(lib.gpsx_wvel_dev(eng.h, vcfg.ctypes.data, a.buf["o"].ptr, buf["out"].ptr, None, buf["fix"].ptr, 1, buf["vel"].ptr), "wvel")
                eng._chk(lib.gpsx_wkf_dev(eng.h, kcfg.ctypes.data, a.buf["o"].ptr, buf["out"].ptr, None, buf["fix"].ptr, buf["vel"].ptr, 1, n, buf["state"].ptr,
                                          buf["kf"].ptr), "wkf")
                at += n
            eng.synchronize()
            assert at == 24576 and int(buf["kf"].get(KR.KF_DTYPE, 1)["flags"][0]) == KR.F_INIT
        # -- the host's part of a warm start: almanac orbits into the bank
        bank = buf["bank"].get(P.EPH_DTYPE, (1, len(prns)))
        alm, _ = A.almanac_records([row for _, row in S.sats()])
        for k, p in enumerate(four):
            bank[0, p] = AR.to_eph(alm[k], bank.dtype)[0]
        buf["bank"].put(bank)
        # -- prediction -> window -> decisions -> loop -> lock, enqueued without a look at a record or a state in between
        st0 = AC.empty_states(n_ch)
        with G.Chain(eng, S.sync_cfg_dev(S.MOVING), st0, 424, S.MAX_BAD_WORDS, S.EDGE_GUARD, lock_cfg=R.cfg_array(X.scenario_cfg(0))) as b:
            five = [b.buf[k].ptr for k in NAMES]
            pcfg = PC.stream_cfg(0)
            eng._chk(lib.gpsx_wpred_dev(eng.h, pcfg.ctypes.data, 1, len(prns), prns.ctypes.data, buf["state"].ptr, buf["bank"].ptr, *five, buf["rx"].ptr,
                                        buf["pred"].ptr), "gpsx_wpred_dev")
            assert lib.gpsx_last_kernel(eng.h) == b"k_wpred"
            eng._chk(lib.gpsx_acq_window_weighted_dev(eng.h, C.addressof(g), wcfg.ctypes.data, buf["pred"].ptr, C.c_void_p(d_if.ptr.value + at * 4092), 424,
                                                      buf["peaks"].ptr, buf["wrep"].ptr), "gpsx_acq_window_weighted_dev")
            assert lib.gpsx_last_kernel(eng.h) == b"k_acq_win"
            eng._chk(lib.gpsx_wacq_dev(eng.h, Q.cfg_record(acfg).ctypes.data, C.addressof(g), buf["peaks"].ptr, *five, buf["acq"].ptr, buf["det"].ptr), "gpsx_wacq_dev")
            b.sync(d_if.ptr.value + (at + lead) * 4092, 424 - lead)
            b.words()
            b.lock()
            assert eng.lib.gpsx_synchronize(eng.h) == 0
            rx, pred = buf["rx"].get(P.PRED_RX_DTYPE, (1,)), buf["pred"].get(capi.WPRED_DTYPE, (1, len(prns)))
            peaks, rep = buf["peaks"].get(V.PEAK_DTYPE, (1, len(prns), n_dopp)), buf["wrep"].get(V.REP_DTYPE, (1, len(prns)))
            # the window stage against its restatement on the device's own prediction records
            _same((peaks, rep), V.run(oracle, wcfg_d, pred, blocks[at:at + 424], prns, *WC.WARM_GRID, cache={}), "behind gpsx_wpred_dev")
            assert [int(f) for f in rep["flags"][0]] == [V.SEARCHED if p in four else V.SKIPPED for p in range(len(prns))]
            assert int(rx["n_tracked"][0]) == 0 and int(rx["n_visible"][0]) == 4 and not (pred["flags"] & (V.TRACKED | V.ASSIGNED)).any()
            d_phase, d_freq, block = PC.prediction_errors(pred[0], rx["t_ms"][0])
            print("prediction errors at block", block, d_phase, "samples", d_freq, "Hz")
            assert block == at and np.abs(d_phase).max() <= wcfg_d["half_width"] and np.abs(d_freq).max() <= WC.WARM_GRID[1]      # inside W = 64 and D = 1
            truth = {prn: (float(pred[0, p]["f_hz"]) - d_freq[k], (float(pred[0, p]["code_phase"]) + d_phase[k]) % V.SAMPLES) for k, (p, prn) in enumerate(zip(four, S.PRNS))}
            assert CR.hits(peaks[:, four], S.PRNS, truth, 1, WC.WARM_GRID[0], WC.WARM_GRID[1]) == 4
            # the decisions against their restatement on the device's own window records
            want, trace = {k: v.copy() for k, v in st0.items()}, []
            w_acq, w_det = Q.run(acfg, PC.STREAM_PRNS, WC.WARM_GRID[0], WC.WARM_GRID[1], peaks, *[want[k] for k in NAMES], trace=trace)
            G.same_rows(buf["acq"].get(Q.ACQ_DTYPE, (1,)), w_acq, "acq")
            G.same_rows(buf["det"].get(Q.DET_DTYPE, (len(prns),)), w_det[0], "det")
            assert trace[0]["detected"] == sorted(four) and sorted(trace[0]["assigned"]) == sorted(four) and sorted(trace[0]["assigned"].values()) == [0, 1, 2, 3]
            sync = b.read("sync")
            assert sorted(int(v) for v in sync["loop"]["prn"]) == sorted(S.PRNS)
            lock = b.read("l")
            print("after", 424 - lead, "blocks: code ratios", lock["code_ratio"], "flags", lock["flags"])
            assert ((lock["flags"] & R.F_CODE) != 0).all() and (lock["code_ratio"] >= X.CODE_MIN).all()


# ---- 5c: more workgroups than one launch holds -----------------------------------------------------------------------------------------------
def test_a_launch_is_cut_where_the_runtime_would_refuse_it(eng, oracle):
    """2^20 receivers x 17 workgroups is more threads than one launch may have (2^32 - 1): the launcher cuts the receivers into two
    launches.  Every record is skipped but six, on both sides of the cut; records and reports of all 2^20 receivers are what the
    restatement says: the six receivers' own, a flag and zeros everywhere else."""
    la = WC.big_launch()
    sel = list(WC.BIG_SELECTED)
    assert la.n_rx * (2 * WC.BIG_D + 1) * 256 > (1 << 32) - 1 and WC.BIG_CUT - 1 in sel and WC.BIG_CUT in sel
    w_peaks, w_rep = V.run(oracle, la.cfg, la.pred[sel], la.blocks, la.prns, *la.grid, use_magnitude=la.mag, stride=0)
    peaks, rep = _call(eng, la)
    assert peaks[sel].tobytes() == w_peaks.tobytes() and rep[sel].tobytes() == w_rep.tobytes()
    assert (w_rep["flags"] == (V.SEARCHED | V.CLIPPED)).all() and (w_peaks["max_val"] > 0).all()
    others = np.ones(la.n_rx, bool)
    others[sel] = False
    assert not peaks[others].tobytes().strip(b"\0") and (rep["flags"][others] == V.SKIPPED).all()
    assert not any(rep[k][others].any() for k in ("first_bin", "n_bins", "centre"))


# ---- 6: the committed fixture ------------------------------------------------------------------------------------------------------------
def test_the_smoke_fixture(eng):
    gold = np.load(os.path.join(ROOT, "tests", "golden", "wwin_smoke.npz"))
    blocks = WC.smoke_blocks(gold["seed"], gold["n_blocks"])
    peaks, rep = eng.acq_window(gold["cfg"], gold["pred"], blocks, gold["prns"], *[int(v) for v in gold["grid"]], stride_blocks=int(gold["stride"]))
    assert eng.lib.gpsx_last_kernel(eng.h) == b"k_acq_win"
    assert peaks.tobytes() == gold["peaks"].tobytes() and rep.tobytes() == gold["rep"].tobytes()
