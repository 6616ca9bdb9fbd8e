"""Every receiver's fix with millisecond repair and fault exclusion on the device (include/gpsx.h gpsx_wfde_dev / gpsx_wfde,
csrc/k_wfde.hip) against its CPU restatement (tests/weighted_fde_ref.py) on records built on the CPU (tests/weighted_fde_cases.py):
every lane-group width and receiver count with receivers of different kinds -- hence in different rounds -- as neighbours in a wave,
the plain fix it must reduce to, the seeded tables of faults and wrong milliseconds, both entry points, the warm start in place and
every refusal.  Outputs sit between 4096-byte canaries and start as 0xA5, so a byte that is not written shows.  Decisions are
compared for equality: tests/test_weighted_fde_reference.py asserts every compared receiver's margins.

Position parity, measured on one MI355X (profiles/r21_weighted_fde_parity.json): see weighted_fde_cases.PARITY_MEASURED_M."""
import ctypes as C

import numpy as np
import pytest

import weighted_fde_cases as X
import weighted_fde_ref as D
import weighted_fix_cases as W
import weighted_fix_ref as F
import weighted_gpu as G
from weighted_gpu import EINVAL, GUARD, eng  # noqa: F401

pytestmark = pytest.mark.gpu


class _Launch:
    """a launch's inputs on the device, its outputs guarded; run() -> (fix records, fde records, pseudoranges)"""

    def __init__(self, eng, cfg, obs, eph, n_rx, lock=None):
        self.eng, self.cfg, self.n_rx, self.n_ch = eng, cfg, n_rx, len(obs)
        self.obs, self.eph = G.Guarded(eng, obs.nbytes, 0x5A, obs), G.Guarded(eng, eph.nbytes, 0x5A, eph)
        self.lock = None if lock is None else G.Guarded(eng, lock.nbytes, 0x5A, lock)
        self.fix, self.fde, self.pr = G.Guarded(eng, n_rx * 128), G.Guarded(eng, n_rx * 64), G.Guarded(eng, self.n_ch * 8)
        self.bufs = [b for b in (self.obs, self.eph, self.lock, self.fix, self.fde, self.pr) if b is not None]

    def call(self, prev=None, fix=None, fde=None, want_pr=True, cfg=None, n_rx=None):
        return self.eng.lib.gpsx_wfde_dev(self.eng.h, (self.cfg if cfg is None else cfg).ctypes.data, self.obs.ptr, self.eph.ptr,
                                          None if self.lock is None else self.lock.ptr, prev, self.n_rx if n_rx is None else n_rx,
                                          self.fix.ptr if fix is None else fix, self.fde.ptr if fde is None else fde, self.pr.ptr if want_pr else None)

    def run(self, prev=None):
        self.eng._chk(self.call(prev), "gpsx_wfde_dev")
        assert self.eng.lib.gpsx_last_kernel(self.eng.h) == b"k_wfde"
        self.eng.synchronize()
        return self.fix.get(F.FIX_DTYPE, self.n_rx), self.fde.get(D.FDE_DTYPE, self.n_rx), self.pr.get(np.float64, self.n_ch)

    def plain(self):
        """gpsx_wfix_dev on the same device arrays -> (fix records, pseudoranges)"""
        with G.Guarded(self.eng, self.n_rx * 128) as fix, G.Guarded(self.eng, self.n_ch * 8) as pr:
            self.eng._chk(self.eng.lib.gpsx_wfix_dev(self.eng.h, self.cfg["fix"].ctypes.data, self.obs.ptr, self.eph.ptr,
                                                     None if self.lock is None else self.lock.ptr, None, self.n_rx, fix.ptr, pr.ptr), "gpsx_wfix_dev")
            self.eng.synchronize()
            return fix.get(F.FIX_DTYPE, self.n_rx), pr.get(np.float64, self.n_ch)

    def free(self):
        for b in self.bufs:
            b.free()


def _finite(fix, fde, pr):
    for f in ("rr", "dtr_s", "rx_tow_s", "geo", "qr", "resid_rms_m"):
        assert np.isfinite(fix[f]).all(), f
    assert np.isfinite(fde["t_stat"]).all() and np.isfinite(fde["t_limit"]).all() and np.isfinite(pr).all()


def _d_rr(got, want):
    return float(np.linalg.norm(got["rr"] - want["rr"], axis=1).max())


@pytest.mark.parametrize("ch,n_rx", X.SHAPES)
def test_every_shape_and_mix_of_rounds_equals_the_restatement(eng, ch, n_rx):
    """(a) ch_per_rx x n_rx over every group width (4, 8, 16, 64), a second workgroup (67 x 4 and wider), waves with dead upper lanes
    (17 x 33): weighted_fde_cases.launch_case's neighbours in different rounds, compared as weighted_fde_cases.compare orders it;
    the same call twice gives the same bytes; nothing non-finite is written"""
    case = X.launch_case(ch, n_rx)
    run = _Launch(eng, case["cfg"], case["obs"], case["eph"], n_rx, case["lock"])
    try:
        got = run.run()
        again = run.run()
    finally:
        run.free()
    _finite(*got)
    worst = X.compare(got[0], got[1], got[2], *case["want"])
    print("parity", ch, n_rx, worst)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
    if ch == 4:
        assert ((got[1]["flags"] & D.VERDICTS) == D.UNCHECKED).all()


@pytest.mark.parametrize("ch,n_rx", ((5, 67), (12, 67), (33, 17), (64, 17), (4, 67)))
def test_without_repair_and_exclusion_it_is_gpsx_wfix_dev_byte_for_byte(eng, ch, n_rx):
    """(b) repair = 0, max_excl = 0: d_fix and d_pr_m equal gpsx_wfix_dev's on the same device arrays -- the same uncontracted
    operations on the same libm -- on this module's launches (AMBIGUOUS and faulty slots go in as they stand) and on
    weighted_fix_cases' slot mixes with their unfixable receivers"""
    ours, theirs = X.launch_case(ch, n_rx), W.launch_case(ch, n_rx)
    for obs, eph, lock in ((ours["obs"], ours["eph"], ours["lock"]), (theirs["obs"], theirs["eph"], theirs["lock"])):
        run = _Launch(eng, X.cfg(ch, X.launch_min_sats(ch), max_excl=0, repair=0), obs, eph, n_rx, lock)
        try:
            fix, fde, pr = run.run()
            want, want_pr = run.plain()
        finally:
            run.free()
        assert fix.tobytes() == want.tobytes() and pr.tobytes() == want_pr.tobytes()
        assert (fde["n_rounds"] == 1).all() and not fde["excl_mask"].any() and not (fde["plus_mask"] | fde["minus_mask"]).any()
        assert (((fde["flags"] & D.NOFIX) != 0) == ((want["flags"] & F.F_FIX) == 0)).all()


def _packed(draws, ch=12):
    obs, eph = W.pack([(d["obs"], d["eph"]) for d in draws], ch)
    return obs, eph, D.run(X.cfg(ch), obs, eph, len(draws))


def test_the_kept_isolation_draws_in_one_launch(eng):
    """(c) the kept draws of the isolation table (6, 8 and 12 satellites in twelve slots): the device excludes the injected slot and
    nothing else, and its fix is within the position bound of the restatement's"""
    kept = [d for d, _, _ in X.isolation_kept()]
    obs, eph, (want, want_fde, _, _) = _packed(kept)
    run = _Launch(eng, X.cfg(12), obs, eph, len(kept))
    try:
        fix, fde, pr = run.run()
    finally:
        run.free()
    _finite(fix, fde, pr)
    assert (fde["excl_mask"] == [1 << d["slot"] for d in kept]).all() and (fde["n_excluded"] == 1).all() and (fde["n_rounds"] == 2).all()
    assert (fde["flags"] == want_fde["flags"]).all() and ((fix["flags"] & F.F_FIX) != 0).all()
    print("parity isolation", _d_rr(fix, want))
    assert _d_rr(fix, want) <= X.POSITION_BOUND_M


def test_the_wrong_milliseconds_in_one_launch(eng):
    """(d) the +-1 ms draws: the plus and minus masks are as injected, and the fix is within the position bound"""
    draws = X.ms_draws()
    obs, eph, (want, want_fde, _, _) = _packed(draws)
    run = _Launch(eng, X.cfg(12), obs, eph, len(draws))
    try:
        fix, fde, pr = run.run()
    finally:
        run.free()
    _finite(fix, fde, pr)
    assert [(int(p), int(m)) for p, m in zip(fde["plus_mask"], fde["minus_mask"])] == [X.ms_masks(d) for d in draws]
    assert (fde["flags"] == D.PASSED | D.REPAIRED).all() and (fde["flags"] == want_fde["flags"]).all() and (fde["n_rounds"] == 2).all()
    print("parity milliseconds", _d_rr(fix, want))
    assert _d_rr(fix, want) <= X.POSITION_BOUND_M


def test_host_entry_warm_start_in_place_and_no_pr(eng):
    """(e) gpsx_wfde (host arrays) equals gpsx_wfde_dev byte for byte; d_prev == d_fix (in place) equals d_prev as a separate copy and
    both equal the restatement from that start; without d_pr_m the records are the same and the buffer is untouched"""
    for ch, n_rx in ((12, 67), (8, 17)):
        case = X.launch_case(ch, n_rx)
        run = _Launch(eng, case["cfg"], case["obs"], case["eph"], n_rx, case["lock"])
        try:
            cold = run.run()
            host = eng.wfde(case["cfg"], case["obs"], case["eph"], n_rx, lock=case["lock"], want_pr=True)
            assert eng.lib.gpsx_last_kernel(eng.h) == b"k_wfde"
            assert all(a.tobytes() == b.tobytes() for a, b in zip(cold, host))
            with G.Guarded(eng, cold[0].nbytes, 0x5A, cold[0]) as copy:
                apart = run.run(prev=copy.ptr)
            run.fix.put(cold[0])
            in_place = run.run(prev=run.fix.ptr)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(apart, in_place))
            want = D.run(case["cfg"], case["obs"], case["eph"], n_rx, lock=case["lock"], prev=cold[0])
            print("parity warm", ch, n_rx, X.compare(apart[0], apart[1], apart[2], *want[:3]))
            assert (apart[1]["flags"] == cold[1]["flags"]).all() and (apart[1]["excl_mask"] == cold[1]["excl_mask"]).all()
            run.pr.refill()
            with G.Guarded(eng, n_rx * 128) as fix, G.Guarded(eng, n_rx * 64) as fde:
                eng._chk(run.call(fix=fix.ptr, fde=fde.ptr, want_pr=False), "gpsx_wfde_dev")
                eng.synchronize()
                assert fix.get(F.FIX_DTYPE, n_rx).tobytes() == cold[0].tobytes() and fde.get(D.FDE_DTYPE, n_rx).tobytes() == cold[1].tobytes()
            assert run.pr.untouched()
        finally:
            run.free()


def test_host_entry_without_lock_prev_and_pr(eng):
    """(e') gpsx_wfde (host arrays) with lock, prev and pr_m NULL: the records equal gpsx_wfde_dev's without lock records byte for byte,
    and the restatement's without them as weighted_fde_cases.compare orders it"""
    ch, n_rx = 8, 2
    case = X.launch_case(ch, n_rx)
    run = _Launch(eng, case["cfg"], case["obs"], case["eph"], n_rx)
    try:
        fix, fde, pr = run.run()
        host = eng.wfde(case["cfg"], case["obs"], case["eph"], n_rx)
        assert eng.lib.gpsx_last_kernel(eng.h) == b"k_wfde"
    finally:
        run.free()
    assert len(host) == 2 and host[0].tobytes() == fix.tobytes() and host[1].tobytes() == fde.tobytes()
    print("parity no lock", X.compare(fix, fde, pr, *D.run(case["cfg"], case["obs"], case["eph"], n_rx)[:3]))


def test_every_refusal_returns_einval_and_writes_nothing(eng):
    """(f) every error clause of the header but the size overflow: GPSX_EINVAL with a text, canaries and prefill intact, and the
    context works afterwards"""
    ch, n_rx = 8, 2
    case = X.launch_case(ch, n_rx)
    good = case["cfg"]
    run = _Launch(eng, good, case["obs"], case["eph"], n_rx)
    lib, h = eng.lib, eng.h

    def cfg_with(**kw):
        c = good.copy()
        for k, v in kw.items():
            if k.startswith("ion"):
                c["fix"]["ion"][0, int(k[3:])] = v
            elif k.startswith("outer"):
                c["reserved"][0, int(k[5:])] = v
            elif k in c.dtype.names:
                c[k] = v
            else:
                c["fix"][k] = v
        return c

    bad_cfgs = [cfg_with(offset_ms=np.nan), cfg_with(offset_ms=np.inf), cfg_with(ion0=np.nan), cfg_with(ion7=-np.inf), cfg_with(ch_per_rx=0),
                cfg_with(ch_per_rx=65), cfg_with(min_sats=3), cfg_with(min_sats=65), cfg_with(reserved0=1), cfg_with(reserved1=1),
                cfg_with(reserved2=1), cfg_with(reserved3=-1), cfg_with(z_global=np.nan), cfg_with(z_global=np.inf), cfg_with(z_global=-0.5),
                cfg_with(z_global=10.5), cfg_with(max_excl=-1), cfg_with(max_excl=9), cfg_with(repair=2), cfg_with(repair=-1), cfg_with(outer0=1),
                cfg_with(outer1=1), cfg_with(outer2=1), cfg_with(outer3=-1)]
    try:
        for c in bad_cfgs:
            assert run.call(cfg=c) == EINVAL, c
            assert lib.gpsx_last_error(h)
        for n in (0, -1, (1 << 20) + 1):
            assert run.call(n_rx=n) == EINVAL, n
        assert run.call(fix=C.c_void_p(run.fix.base + GUARD + 8)) == EINVAL
        assert run.call(fde=C.c_void_p(run.fde.base + GUARD + 8)) == EINVAL
        args = [h, good.ctypes.data, run.obs.ptr, run.eph.ptr, None, None, n_rx, run.fix.ptr, run.fde.ptr, run.pr.ptr]
        for k in (0, 1, 2, 3, 7, 8):
            a = list(args)
            a[k] = None
            assert lib.gpsx_wfde_dev(*a) == EINVAL, k
        host_fix, host_fde = np.full(n_rx * 128, 0xA5, np.uint8), np.full(n_rx * 64, 0xA5, np.uint8)
        assert lib.gpsx_wfde(h, bad_cfgs[17].ctypes.data, case["obs"].ctypes.data, case["eph"].ctypes.data, None, None, n_rx, host_fix.ctypes.data,
                             host_fde.ctypes.data, None) == EINVAL
        assert (host_fix == 0xA5).all() and (host_fde == 0xA5).all()
        eng.synchronize()
        assert run.fix.untouched() and run.fde.untouched() and run.pr.untouched()
        fix, fde, _ = run.run()      # and the context still works
        assert (fix["flags"] != 0).all() and (fde["flags"] != 0).all()
    finally:
        run.free()
