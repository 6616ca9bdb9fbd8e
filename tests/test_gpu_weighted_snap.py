"""The snapshot fixes on the device (EXTENSION, not in the reference: include/gpsx.h gpsx_wsnap; k_wsnap, a wave per receiver) against
their CPU restatement (tests/weighted_snap_ref.py, the rows of tests/weighted_snap_cases.py, whose predicates
tests/test_weighted_snap_reference.py asserts).  d_snap and d_sv between canaries and prefilled, the inputs between canaries and
untouched; every integer field, flag, mask and N_p equal, rr, b_m and 1000 m/s x dt_s within weighted_fix_cases' cap of 1e-4 m
(weighted_snap_cases.decisions_clear makes the integers' comparison fair and leaves at most 5 % of a launch out); host variant = device
variant = binding; a second call; receivers permuted; every refusal with its text; the fixture; and the scenario on the device: the
hybrid grid, the snapshot on its records where they lie, gpsx_wsnap_to_fix and the filter's INIT."""
import ctypes as C

import numpy as np
import pytest

import weighted_gpu as G
import weighted_snap_cases as K
import weighted_snap_ref as S
from weighted_gpu import EINVAL, eng  # noqa: F401

pytestmark = pytest.mark.gpu


def _grid(la, prns=None, **over):
    from stm32f4_sdr_gps_amd import capi
    prns = np.ascontiguousarray(la.prns if prns is None else prns, np.uint8)
    a = dict(n_search=la.n_rx, n_prn=la.n_prn, d0=K.DOPP_MIN_HZ, ds=K.DOPP_STEP_HZ, nd=la.n_dopp)
    a.update(over)
    return capi.AcqWeightedT(a["n_search"], 0, a["n_prn"], prns.ctypes.data_as(C.POINTER(C.c_uint8)), a["d0"], a["ds"], a["nd"], 1), prns


def _call(eng, la, cfg, dev, want_sv=True):
    """gpsx_wsnap_dev (dev) or gpsx_wsnap on launch `la`: the bank between canaries in device memory; the records, the priors and the
    outputs between canaries in device (dev) or host memory, the outputs prefilled -> (snap, sv or None)"""
    g, prns = _grid(la)
    where = eng if dev else None
    fn = eng.lib.gpsx_wsnap_dev if dev else eng.lib.gpsx_wsnap
    with G.Pool() as pool:
        d_bank = pool.add(G.Guarded(eng, la.bank.nbytes, G.STATE_FILL, la.bank))
        d_peaks = pool.add(G.Guarded(where, la.peaks.nbytes, G.STATE_FILL, la.peaks))
        d_prior = pool.add(G.Guarded(where, la.prior.nbytes, G.STATE_FILL, la.prior))
        d_snap = pool.add(G.Guarded(where, la.n_rx * S.SNAP_DTYPE.itemsize))
        d_sv = pool.add(G.Guarded(where, la.n_rx * la.n_prn * S.SV_DTYPE.itemsize))
        rc = fn(eng.h, cfg.ctypes.data, C.addressof(g), d_peaks.ptr, d_bank.ptr, la.bank_stride, d_prior.ptr, d_snap.ptr, d_sv.ptr if want_sv else None)
        assert rc == 0, (rc, eng.lib.gpsx_last_error(eng.h))
        assert eng.lib.gpsx_last_kernel(eng.h) == b"k_wsnap"
        assert eng.lib.gpsx_synchronize(eng.h) == 0
        assert d_bank.untouched() and d_peaks.untouched() and d_prior.untouched() and (want_sv or d_sv.untouched())
        return d_snap.get(S.SNAP_DTYPE, (la.n_rx,)), d_sv.get(S.SV_DTYPE, (la.n_rx, la.n_prn)) if want_sv else None


def _skip(la, cfg, snap, trace):
    unclear = K.decisions_clear(la, cfg, snap, trace)
    skip = [r for r in range(la.n_rx) if (la.rows[r].name if la.rows[r] is not None else r) in unclear]
    assert len(skip) <= K.MAX_LEFT_OUT * la.n_rx, unclear
    return skip


# ---- 1: the table and the random launches, at every edge of the launch's shape (weighted_snap_cases.GPU_SHAPES) --------------------------------
SHAPE_IDS = [f"{s[0] or 'table'}rx-{s[1]}prn-{s[2]}bins-{'shared' if s[3] else 'own'}-{'sv' if s[4] else 'nosv'}" for s in K.GPU_SHAPES]


@pytest.mark.parametrize("shape", K.GPU_SHAPES, ids=SHAPE_IDS)
def test_launches_match_the_restatement(eng, shape):
    want_sv = shape[4]
    la, cfg, table = K.gpu_launch(shape)
    snap, sv, trace = K.run(la, cfg)
    skip = _skip(la, cfg, snap, trace)
    got, got_sv = _call(eng, la, cfg, True, want_sv)
    print("parity", K.compare(got, got_sv, snap, sv if want_sv else None, skip, label="-".join(str(v) for v in shape)))
    if shape[:3] == (1, 5, 1):
        assert int(got[0]["flags"]) == S.F_FIX and int(got[0]["n_used"]) == 5      # (a solved record is compared at n_prn = 5)
    if table and want_sv:
        seen = set()
        for r, row in enumerate(la.rows):          # the predicates, on the DEVICE's bytes
            if row is not None:
                assert row.check(K.outcome(la, r, got, got_sv, trace)), row.name
                seen.add(row.name)
        assert len(seen) == len(K.ROWS)


def test_a_candidate_below_the_horizon_has_no_row(eng):
    la, cfg = K.below_horizon_case()
    snap, sv, trace = K.run(la, cfg)
    got, got_sv = _call(eng, la, cfg, True)
    K.compare(got, got_sv, snap, sv, _skip(la, cfg, snap, trace))
    assert K.below_horizon_check(got, got_sv)


def test_a_pass_that_fails_on_rho(eng):
    """an orbit and a prior of 1e13 m: rho <= 0 leaves the satellite DETECTED | HAVE_EPH without CANDIDATE, on the device as in the restatement"""
    la, cfg = K.rho_case()
    snap, sv, trace = K.run(la, cfg)
    got, got_sv = _call(eng, la, cfg, True)
    K.compare(got, got_sv, snap, sv, _skip(la, cfg, snap, trace))
    assert K.rho_check(got_sv, trace)


# ---- 2: call equivalences ----------------------------------------------------------------------------------------------------------------
def test_host_variant_device_variant_and_binding_agree(eng):
    la, cfg, _ = K.gpu_launch(K.GPU_OTHER[1])
    dev, dev_sv = _call(eng, la, cfg, True)
    host, host_sv = _call(eng, la, cfg, False)
    assert dev.tobytes() == host.tobytes() and dev_sv.tobytes() == host_sv.tobytes()
    assert _call(eng, la, cfg, False, want_sv=False)[0].tobytes() == dev.tobytes()
    with G.Guarded(eng, la.bank.nbytes, G.STATE_FILL, la.bank) as d_bank:
        snap, sv = eng.wsnap(cfg, la.peaks, la.prns, K.DOPP_MIN_HZ, K.DOPP_STEP_HZ, d_bank.ptr.value, la.bank_stride, la.prior)
        assert snap.tobytes() == dev.tobytes() and sv.tobytes() == dev_sv.tobytes()
        alone = eng.wsnap(cfg, la.peaks, la.prns, K.DOPP_MIN_HZ, K.DOPP_STEP_HZ, d_bank.ptr.value, la.bank_stride, la.prior, want_sv=False)
        assert alone.tobytes() == dev.tobytes() and d_bank.untouched()
    fix = eng.wsnap_to_fix(dev)
    for r in range(la.n_rx):
        want = S.to_fix(dev[r])
        assert fix[r].tobytes() == (want.tobytes() if want is not None else bytes(128)), r


def test_a_second_call_gives_the_same_bytes(eng):
    la, cfg, _ = K.gpu_launch(K.GPU_OTHER[0])
    a, b = _call(eng, la, cfg, True), _call(eng, la, cfg, True)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_receivers_permuted_give_the_same_bytes_permuted(eng):
    la, lb = K.gpu_launch(K.GPU_OTHER[1])[0], K.gpu_launch(K.GPU_OTHER[1])[0]
    perm = np.random.default_rng(5).permutation(la.n_rx)
    lb.peaks, lb.bank, lb.prior = np.ascontiguousarray(la.peaks[perm]), np.ascontiguousarray(la.bank[perm]), np.ascontiguousarray(la.prior[perm])
    cfg = K.table_cfg()
    a, b = _call(eng, la, cfg, True), _call(eng, lb, cfg, True)
    assert a[0][perm].tobytes() == b[0].tobytes() and a[1][perm].tobytes() == b[1].tobytes()


# ---- 3: refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_with_their_text_and_write_nothing(eng):
    """(a size product that overflows cannot be reached where a size has 64 bits: 2^20 x 64 x 2^20 x 16 stays below 2^64)"""
    la = K.launch(6, 5, 4, rows=False)
    good = dict(null=None, cfg={}, n_search=la.n_rx, n_prn=la.n_prn, prns=[int(v) for v in la.prns], d0=K.DOPP_MIN_HZ, ds=K.DOPP_STEP_HZ, nd=la.n_dopp,
                stride=la.n_prn, off={}, alias=None)
    by_message = {
        b"null argument": [dict(null=w) for w in ("cfg", "g", "prns", "peaks", "bank", "prior", "snap")] + [dict(null="snap", n_prn=0)],
        b"an ionosphere coefficient is not finite": [dict(cfg=dict(ion=(0, 0, np.nan, 0, 0, 0, 0, 0))), dict(cfg=dict(ion=(0, 0, 0, 0, 0, 0, 0, np.inf)))],
        b"el_min_rad must be finite and within -pi/2..pi/2": [dict(cfg=dict(el_min_rad=1.58)), dict(cfg=dict(el_min_rad=-1.58)), dict(cfg=dict(el_min_rad=np.nan))],
        b"epoch_offset_s must be finite and 0..4.096": [dict(cfg=dict(epoch_offset_s=-1e-9)), dict(cfg=dict(epoch_offset_s=4.097)), dict(cfg=dict(epoch_offset_s=np.nan))],
        b"max_resid_m must be finite and above 0": [dict(cfg=dict(max_resid_m=0.0)), dict(cfg=dict(max_resid_m=-1.0)), dict(cfg=dict(max_resid_m=np.inf)),
                                                    dict(cfg=dict(max_resid_m=np.nan))],
        b"det_num and det_den must be 1..1024, det_num >= det_den": [dict(cfg=dict(det_num=0)), dict(cfg=dict(det_num=1025, det_den=1)), dict(cfg=dict(det_den=0)),
                                                                     dict(cfg=dict(det_num=3, det_den=4))],
        b"min_sats must be 5..64": [dict(cfg=dict(min_sats=4)), dict(cfg=dict(min_sats=65)), dict(cfg=dict(min_sats=-1))],
        b"reserved must be 0": [dict(cfg=dict(reserved=(1, 0, 0, 0, 0, 0))), dict(cfg=dict(reserved=(0, 0, 0, 0, 0, -1)))],
        b"n_search must be 1..1048576": [dict(n_search=0), dict(n_search=-1), dict(n_search=(1 << 20) + 1)],
        b"n_prn must be 1..64": [dict(n_prn=0), dict(n_prn=65, prns=list(range(1, 66))), dict(n_prn=-3)],
        b"n_dopp must be 1..1048576": [dict(nd=0), dict(nd=-1), dict(nd=(1 << 20) + 1)],
        b"PRN outside 1..210": [dict(prns=[0] + good["prns"][1:]), dict(prns=good["prns"][:-1] + [211])],
        b"a PRN is listed twice": [dict(prns=good["prns"][:-1] + good["prns"][:1])],
        b"a Doppler bin lies outside int32": [dict(d0=2147483647, ds=1), dict(d0=-2147483648, ds=-1), dict(d0=0, ds=1 << 30, nd=4)],
        b"bank_stride must be 0 or n_prn": [dict(stride=1), dict(stride=-la.n_prn), dict(stride=la.n_prn + 1)],
        b"d_bank must be 16-byte aligned": [dict(off=dict(bank=8))],
    }
    dev_only = {
        b"d_peaks must be 4-byte and d_prior 8-byte aligned": [dict(off=dict(peaks=2)), dict(off=dict(prior=4))],
        b"d_snap and d_sv must be 16-byte aligned": [dict(off=dict(snap=8)), dict(off=dict(sv=8))],
        b"d_snap or d_sv overlaps another array": [dict(alias=("sv", "snap")), dict(alias=("snap", "prior")), dict(alias=("sv", "peaks")), dict(alias=("snap", "bank"))],
    }
    with G.Pool() as pool:
        bufs = {}
        for dev in (False, True):
            where = eng if dev else None
            room = lambda x: np.concatenate([np.ascontiguousarray(x).view(np.uint8).reshape(-1), np.zeros(64, np.uint8)])      # noqa: E731  (for the offsets)
            bufs[dev] = dict(bank=pool.add(G.Guarded(eng, la.bank.nbytes + 64, G.STATE_FILL, room(la.bank))),
                             peaks=pool.add(G.Guarded(where, la.peaks.nbytes + 64, G.STATE_FILL, room(la.peaks))),
                             prior=pool.add(G.Guarded(where, la.prior.nbytes + 64, G.STATE_FILL, room(la.prior))),
                             snap=pool.add(G.Guarded(where, la.n_rx * 128 + 64)), sv=pool.add(G.Guarded(where, la.n_rx * la.n_prn * 48 + 64)))

        def call(a, dev):
            cfg = K.table_cfg()
            for k, v in a["cfg"].items():
                cfg[k] = v
            prns = np.array((a["prns"] + [1] * 64)[:max(a["n_prn"], len(a["prns"]), 1)], np.uint8)
            g, prns = _grid(la, prns, n_search=a["n_search"], n_prn=a["n_prn"], d0=a["d0"], ds=a["ds"], nd=a["nd"])
            if a["null"] == "prns":
                g.prns = None
            p = {k: (None if a["null"] == k else C.c_void_p(b.ptr.value + a["off"].get(k, 0))) for k, b in bufs[dev].items()}
            if a["alias"]:
                p[a["alias"][0]] = p[a["alias"][1]]
            fn = eng.lib.gpsx_wsnap_dev if dev else eng.lib.gpsx_wsnap
            return fn(eng.h, None if a["null"] == "cfg" else cfg.ctypes.data, None if a["null"] == "g" else C.addressof(g), p["peaks"], p["bank"], a["stride"],
                      p["prior"], p["snap"], p["sv"])

        every = [b for d in bufs.values() for b in d.values()]
        G.refusals(eng, by_message, good, call, every)
        for message, changes in dev_only.items():
            for change in changes:
                for b in every:
                    b.refill()
                rc = call({**good, **change}, True)
                assert rc == EINVAL and eng.lib.gpsx_last_error(eng.h) == message, (change, rc, eng.lib.gpsx_last_error(eng.h))
                eng.synchronize()
                assert all(b.untouched() for b in every), change
        assert call(good, True) == 0 and eng.lib.gpsx_synchronize(eng.h) == 0      # (the good arguments are good)


# ---- 4: the fixture, the scenario ----------------------------------------------------------------------------------------------------------
def test_the_smoke_fixture_on_the_device(eng):
    import os
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wsnap_smoke.npz"))
    with G.Guarded(eng, gold["bank"].nbytes, G.STATE_FILL, gold["bank"]) as d_bank:
        snap, sv = eng.wsnap(gold["cfg"], gold["peaks"], gold["prns"], int(gold["dopp"][0]), int(gold["dopp"][1]), d_bank.ptr.value, len(gold["prns"]), gold["prior"])
    K.compare(snap, sv, gold["snap"], gold["sv"], [int(v) for v in gold["skip"]])


def test_the_scenario_on_the_device(eng):
    """six satellites' IF samples on the device: gpsx_acq_grid_weighted_hyb_dev at 1 x 8, then gpsx_wsnap_dev on d_peaks where it lies --
    nothing is read in between --, then gpsx_wsnap_to_fix on the record, then gpsx_wkf_dev, which reaches INIT from it"""
    from stm32f4_sdr_gps_amd import capi
    import weighted_kf_ref as R
    sc = K.scenario()
    prns = np.ascontiguousarray(sc["prns"], np.uint8)
    d0, ds, nd = K.SCEN_GRID
    g = capi.AcqWeightedT(1, 0, 6, prns.ctypes.data_as(C.POINTER(C.c_uint8)), d0, ds, nd, 1)
    with G.Pool() as pool:
        d_blk = pool.add(G.Guarded(eng, sc["blocks"].nbytes, G.STATE_FILL, sc["blocks"]))
        d_bank = pool.add(G.Guarded(eng, sc["bank"].nbytes, G.STATE_FILL, sc["bank"]))
        d_prior = pool.add(G.Guarded(eng, sc["prior"].nbytes, G.STATE_FILL, sc["prior"]))
        d_peaks = pool.add(G.Guarded(eng, 6 * nd * 16))
        d_snap, d_sv = pool.add(G.Guarded(eng, 128)), pool.add(G.Guarded(eng, 6 * 48))
        eng._chk(eng.lib.gpsx_acq_grid_weighted_hyb_dev(eng.h, C.addressof(g), 1, K.SCEN_BLOCKS, d_blk.ptr, K.SCEN_BLOCKS, d_peaks.ptr), "grid")
        eng._chk(eng.lib.gpsx_wsnap_dev(eng.h, sc["cfg"].ctypes.data, C.addressof(g), d_peaks.ptr, d_bank.ptr, 6, d_prior.ptr, d_snap.ptr, d_sv.ptr), "gpsx_wsnap_dev")
        assert eng.lib.gpsx_last_kernel(eng.h) == b"k_wsnap"
        eng.synchronize()
        snap, sv = d_snap.get(S.SNAP_DTYPE, (1,)), d_sv.get(S.SV_DTYPE, (1, 6))
        em, es = K.scenario_check(sc, snap[0], sv[0])
        print("IF scenario on the device: position error %.2f m, time error %.5f s" % (em, es))
        assert em <= K.BOUNDS["scenario_m"] and es <= K.BOUNDS["scenario_s"], (em, es)
        want, want_sv = S.snap(sc["cfg"], prns, d0, ds, d_peaks.get(S.PEAK_DTYPE, (1, 6, nd)), sc["bank"][None], 6, sc["prior"])
        print("parity", K.compare(snap, sv, want, want_sv, label="scenario"))
        fix = eng.wsnap_to_fix(snap)
        assert int(fix["flags"][0]) == 1
        kcfg = R.make_cfg(6)
        d_fix = pool.add(G.Guarded(eng, 128, G.STATE_FILL, fix))
        d_obs, d_eph = pool.add(G.Guarded(eng, 6 * 32, G.STATE_FILL, np.zeros(6 * 32, np.uint8))), pool.add(G.Guarded(eng, 6 * 256, G.STATE_FILL, np.zeros(6 * 256, np.uint8)))
        d_state, d_kf = pool.add(G.Guarded(eng, 384, G.STATE_FILL, np.zeros(1, R.STATE_DTYPE))), pool.add(G.Guarded(eng, R.KF_DTYPE.itemsize))
        eng._chk(eng.lib.gpsx_wkf_dev(eng.h, kcfg.ctypes.data, d_obs.ptr, d_eph.ptr, None, d_fix.ptr, None, 1, K.SCEN_BLOCKS, d_state.ptr, d_kf.ptr), "gpsx_wkf_dev")
        eng.synchronize()
        kf, state = d_kf.get(R.KF_DTYPE, (1,)), d_state.get(R.STATE_DTYPE, (1,))
        assert int(kf["flags"][0]) == R.F_INIT and int(state["flags"][0]) & R.S_INIT
        assert np.array_equal(state["x"][0, :3], snap["rr"][0]) and abs(int(state["rcv_ms"][0]) - round(float(snap["tow_s"][0]) * 1000.0)) <= 1
