"""Every receiver's position fix on the device (include/gpsx.h gpsx_wfix_dev / gpsx_wfix, csrc/k_wfix.hip) against its CPU restatement
(tests/weighted_fix_ref.py) on records built on the CPU in milliseconds (tests/weighted_fix_cases.py): every lane-group width and
receiver count, every kind of slot that gives no row at the first, the last and a middle slot of a group, receivers that cannot be
fixed, both entry points, the warm start in place, every refusal, and one run behind the five device stages of the chain.  Outputs sit
between 4096-byte canaries and start as 0xA5, so a byte that is not written shows.  The CPU partner is
tests/test_weighted_fix_reference.py."""
import ctypes as C

import numpy as np
import pytest

import weighted_fix_cases as W
import weighted_fix_ref as F
import weighted_gpu as G
from weighted_gpu import EINVAL, GUARD, eng  # noqa: F401

pytestmark = pytest.mark.gpu


class _Launch:
    """a launch's inputs on the device, its outputs guarded; run() -> (fix records, pseudoranges)"""

    def __init__(self, eng, cfg, obs, eph, n_rx, lock=None):
        self.eng, self.cfg, self.n_rx, self.n_ch = eng, cfg, n_rx, len(obs)
        self.obs, self.eph = G.Guarded(eng, obs.nbytes, 0x5A, obs), G.Guarded(eng, eph.nbytes, 0x5A, eph)
        self.lock = None if lock is None else G.Guarded(eng, lock.nbytes, 0x5A, lock)
        self.fix, self.pr = G.Guarded(eng, n_rx * 128), G.Guarded(eng, self.n_ch * 8)
        self.bufs = [b for b in (self.obs, self.eph, self.lock, self.fix, self.pr) if b is not None]

    def call(self, prev=None, fix=None, want_pr=True, cfg=None, n_rx=None):
        fix = self.fix.ptr if fix is None else fix
        return self.eng.lib.gpsx_wfix_dev(self.eng.h, (self.cfg if cfg is None else cfg).ctypes.data, self.obs.ptr, self.eph.ptr,
                                          None if self.lock is None else self.lock.ptr, prev, self.n_rx if n_rx is None else n_rx, fix,
                                          self.pr.ptr if want_pr else None)

    def run(self, prev=None):
        self.eng._chk(self.call(prev), "gpsx_wfix_dev")
        self.eng.synchronize()
        return self.fix.get(F.FIX_DTYPE, self.n_rx), self.pr.get(np.float64, self.n_ch)

    def free(self):
        for b in self.bufs:
            b.free()


def _no_nonfinite_bytes(fix):
    for f in ("rr", "dtr_s", "rx_tow_s", "geo", "qr", "resid_rms_m"):
        assert np.isfinite(fix[f]).all(), f


@pytest.mark.parametrize("n_rx", W.SHAPES_RX)
@pytest.mark.parametrize("ch", W.SHAPES_CH)
def test_every_shape_and_slot_mix_equals_the_restatement(eng, ch, n_rx):
    """ch_per_rx x n_rx over every group width (1, 4, 8, 16, 64), a second workgroup (67 x 4), waves with dead upper lanes (17 x 33):
    weighted_fix_cases.launch_case's slot mixes and unfixable receivers, compared as weighted_fix_cases.compare orders it; the same
    call twice gives the same bytes; nothing non-finite is written, NONFINITE receivers included"""
    from stm32f4_sdr_gps_amd import capi
    case = W.launch_case(ch, n_rx)
    cfg = capi.wfix_cfg(W.OFFSET_MS, ch)
    want, want_pr = F.run(cfg, case["obs"], case["eph"], n_rx, lock=case["lock"])
    run = _Launch(eng, cfg, case["obs"], case["eph"], n_rx, case["lock"])
    try:
        got, got_pr = run.run()
        again, again_pr = run.run()
    finally:
        run.free()
    _no_nonfinite_bytes(got)
    print(ch, n_rx, W.compare(got, got_pr, want, want_pr))
    assert got.tobytes() == again.tobytes() and got_pr.tobytes() == again_pr.tobytes()
    if ch == 4 and n_rx >= 17:
        assert {F.F_FIX, F.F_TOO_FEW, F.F_SINGULAR, F.F_NONFINITE} <= set(got["flags"].tolist())


def test_host_arrays_equal_device_arrays_and_the_lock_and_pr_arguments(eng):
    """gpsx_wfix (host arrays) equals gpsx_wfix_dev byte for byte, with and without lock records; without d_pr_m the records are the
    same and the pseudorange buffer stays as it was"""
    from stm32f4_sdr_gps_amd import capi
    for ch, n_rx in ((12, 17), (5, 67)):
        case = W.launch_case(ch, n_rx)
        cfg = capi.wfix_cfg(W.OFFSET_MS, ch)
        for lock in (case["lock"], None):
            run = _Launch(eng, cfg, case["obs"], case["eph"], n_rx, lock)
            try:
                got, got_pr = run.run()
                host, host_pr = eng.wfix(cfg, case["obs"], case["eph"], n_rx, lock=lock, want_pr=True)
                assert got.tobytes() == host.tobytes() and got_pr.tobytes() == host_pr.tobytes()
                assert eng.wfix(cfg, case["obs"], case["eph"], n_rx, lock=lock).tobytes() == got.tobytes()
                quiet = G.Guarded(eng, n_rx * 128)
                eng._chk(run.call(fix=quiet.ptr, want_pr=False), "gpsx_wfix_dev")
                eng.synchronize()
                assert quiet.get(F.FIX_DTYPE, n_rx).tobytes() == got.tobytes()
                quiet.free()
            finally:
                run.free()


def test_warm_start_in_place(eng):
    """d_prev == d_fix (in place) equals d_prev as a separate copy; both reach the cold start's fix within the bound in fewer or equal
    iterations; a record without FIX starts at the origin, so it repeats the cold start's bytes"""
    from stm32f4_sdr_gps_amd import capi
    ch, n_rx = 8, 67
    case = W.launch_case(ch, n_rx)
    cfg = capi.wfix_cfg(W.OFFSET_MS, ch)
    run = _Launch(eng, cfg, case["obs"], case["eph"], n_rx, case["lock"])
    try:
        cold, _ = run.run()
        copy = G.Guarded(eng, cold.nbytes, 0x5A, cold)
        apart, _ = run.run(prev=copy.ptr)
        copy.free()
        run.fix.put(cold)
        in_place, _ = run.run(prev=run.fix.ptr)
    finally:
        run.free()
    assert in_place.tobytes() == apart.tobytes()
    want, _ = F.run(cfg, case["obs"], case["eph"], n_rx, lock=case["lock"], prev=cold)
    W.compare(apart, None, want, None)
    fixed = (cold["flags"] & F.F_FIX) != 0
    assert fixed.sum() > 40 and (apart["flags"] == cold["flags"]).all()
    assert (apart["n_iter"][fixed] <= cold["n_iter"][fixed]).all() and apart["n_iter"][fixed].max() <= 3
    assert float(np.linalg.norm(apart["rr"] - cold["rr"], axis=1).max()) <= W.POSITION_BOUND_M
    assert apart[~fixed].tobytes() == cold[~fixed].tobytes()


def test_every_refusal_returns_einval_and_writes_nothing(eng):
    """every error clause of the header but the size overflow (which no n_rx <= 2^20 x ch_per_rx <= 64 can reach on a 64-bit size_t)"""
    from stm32f4_sdr_gps_amd import capi
    ch, n_rx = 4, 2
    case = W.launch_case(ch, n_rx)
    good = capi.wfix_cfg(W.OFFSET_MS, ch)
    run = _Launch(eng, good, case["obs"], case["eph"], n_rx)
    lib, h = eng.lib, eng.h

    def cfg_with(**kw):
        c = good.copy()
        for k, v in kw.items():
            if k.startswith("ion"):
                c["ion"][0, int(k[3:])] = v
            else:
                c[k] = v
        return c

    bad_cfgs = [cfg_with(offset_ms=np.nan), cfg_with(offset_ms=np.inf), cfg_with(ion0=np.nan), cfg_with(ion7=-np.inf), cfg_with(ch_per_rx=0),
                cfg_with(ch_per_rx=65), cfg_with(min_sats=3), cfg_with(min_sats=65), cfg_with(reserved0=1), cfg_with(reserved1=1),
                cfg_with(reserved2=1), cfg_with(reserved3=-1)]
    try:
        for c in bad_cfgs:
            assert run.call(cfg=c) == EINVAL, c
            assert lib.gpsx_last_error(h)
        for n in (0, -1, (1 << 20) + 1):
            assert run.call(n_rx=n) == EINVAL, n
        assert run.call(fix=C.c_void_p(run.fix.base + GUARD + 8)) == EINVAL
        args = [h, good.ctypes.data, run.obs.ptr, run.eph.ptr, None, None, n_rx, run.fix.ptr, run.pr.ptr]
        for k in (0, 1, 2, 3, 7):
            a = list(args)
            a[k] = None
            assert lib.gpsx_wfix_dev(*a) == EINVAL, k
        host_fix = np.full(n_rx, 0xA5, np.uint8).repeat(128).view(F.FIX_DTYPE)
        assert lib.gpsx_wfix(h, bad_cfgs[4].ctypes.data, case["obs"].ctypes.data, case["eph"].ctypes.data, None, None, n_rx, host_fix.ctypes.data,
                             None) == EINVAL
        assert (host_fix.view(np.uint8) == 0xA5).all()
        eng.synchronize()
        assert run.fix.untouched() and run.pr.untouched()
        got, _ = run.run()      # and the context still works
        assert (got["flags"] != 0).all()
    finally:
        run.free()


def test_behind_the_five_device_stages(eng):
    """weighted_pvt_cases' stream (four orbiting satellites, 25 000 blocks, MOVING gains) through gpsx_track_loop_weighted_sync_dev,
    gpsx_wnav_words_dev, gpsx_wobs_dev, gpsx_weph_dev and gpsx_wlock_dev in weighted_pvt_cases.LAUNCHES, then gpsx_wfix_dev on the last
    launch's d_obs / d_eph where they lie on the device (ch_per_rx = 4, n_rx = 1) at both OFFSETS_MS: the fix equals the host path's
    (weighted_pvt_cases.position: gpsx_wobs_pseudoranges + gpsx_weph_to_eph + pntpos) within the position bound and lies within
    BOUNDS["moving"]["position_m"] of the truth.  Cost: the stream's synthesis (about 25 s of CPU, cached per process in
    weighted_pvt_cases._memo) and its upload, plus a few seconds of GPU."""
    import weighted_pvt_cases as P
    from stm32f4_sdr_gps_amd import capi
    lib, n_ch = eng.lib, 4
    blocks = P.blocks()
    d_if = eng.malloc(blocks.nbytes)
    eng.h2d(d_if, blocks)
    st0 = dict(P.fresh_states(), sync=P.handover(), lock=np.zeros(n_ch, capi.WLOCK_STATE_DTYPE))
    chain = G.Chain(eng, P.sync_cfg_dev(P.MOVING), st0, max(P.LAUNCHES), P.MAX_BAD_WORDS, P.EDGE_GUARD, capi.wlock_cfg(25, 10, 1.5, 0.3, 1.0, 2, 2))
    bufs = dict(chain.buf, fix=G.Guarded(eng, F.FIX_DTYPE.itemsize), pr=G.Guarded(eng, n_ch * 8))
    try:
        at = 0
        for n in P.LAUNCHES:
            chain.sync(d_if + at * 4092, n)
            chain.words()
            chain.obs()
            chain.eph()
            chain.lock()
            eng.synchronize()
            at += n
        obs, eph, lock = chain.read("o"), chain.read("e"), chain.read("l")
        assert P.flags_ok(obs) and (lock["flags"] & capi.WLOCK_FLAG_CODE).all(), (obs["flags"], lock["flags"])
        for offset in P.OFFSETS_MS:
            cfg = capi.wfix_cfg(offset, 4)
            eng._chk(lib.gpsx_wfix_dev(eng.h, cfg.ctypes.data, bufs["o"].ptr, bufs["e"].ptr, bufs["l"].ptr, None, 1, bufs["fix"].ptr, bufs["pr"].ptr), "gpsx_wfix_dev")
            eng.synchronize()
            fix, pr = bufs["fix"].get(F.FIX_DTYPE, 1)[0], bufs["pr"].get(np.float64, n_ch)
            want = P.position(capi.load_library(), obs, eph, P.PRNS, offset)
            assert int(fix["flags"]) == F.F_FIX and int(fix["n_used"]) == 4 and int(fix["used_mask"]) == 15 and int(fix["ref_slot"]) == want["ref"]
            assert pr.tobytes() == want["pr"].tobytes() and float(fix["rx_tow_s"]) == want["rx_tow_s"]
            d = float(np.linalg.norm(fix["rr"] - want["rr"]))
            print("offset", offset, "device fix", P.position_error(dict(rr=fix["rr"])), "m from the truth,", d, "m from the host path's")
            assert d <= W.POSITION_BOUND_M and abs(float(fix["dtr_s"]) - want["dtr"]) * 299792458.0 <= W.POSITION_BOUND_M
            assert P.position_error(dict(rr=fix["rr"])) < P.BOUNDS["moving"]["position_m"]
    finally:
        for b in bufs.values():
            b.free()
        eng.free(d_if)
