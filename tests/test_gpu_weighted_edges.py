"""The three solver kernels (csrc/k_wfix.hip, k_wfde.hip, k_wvel.hip -- each with its own copy of the satellite text) at the edges of their
input space, against their CPU restatements (tests/weighted_fix_ref.py, weighted_fde_ref.py, weighted_vel_ref.py) on the receivers of
tests/weighted_edge_cases.py: tk from -7200.6 s to +7200.4 s and one second past the 7201 s limit on either side, e from 0 to 0.4, f2,
tgd and sva drawn, toc apart from toe, both polar sites, a site above and one below the troposphere's cut-offs, receive times at the
week's start, middle and end, records whole weeks away, transmit times that straddle the week's end, and the previous week's broadcast.
Receivers of different kinds are neighbours in a wave.  Outputs sit between 4096-byte canaries and start as 0xA5.  Decisions are compared
for equality: tests/test_weighted_edge_reference.py asserts that every compared receiver's stand clear of round-off, and holds the
restatements to physics and to pntpos at these points.

Parity, measured on one MI355X (profiles/r23_weighted_edges_parity.json): see weighted_edge_cases.PARITY_MEASURED."""
import numpy as np
import pytest

import weighted_edge_cases as X
import weighted_fde_cases as XF
import weighted_fde_ref as D
import weighted_fix_ref as F
import weighted_gpu as G
import weighted_vel_ref as V
from weighted_gpu import eng  # noqa: F401

pytestmark = pytest.mark.gpu
MUNICH_WEEK = 2300      # pvt_chain.WEEK: what the decoder makes of the ten broadcast bits


class _Inputs(G.Pool):
    """a launch's observables and records on the device between canaries, and guarded, prefilled outputs"""

    def __init__(self, eng, obs, eph, n_rx):
        super().__init__()
        self.eng, self.n_rx, self.n_ch = eng, n_rx, len(obs)
        self.obs, self.eph = self.add(G.Guarded(eng, obs.nbytes, G.STATE_FILL, obs)), self.add(G.Guarded(eng, eph.nbytes, G.STATE_FILL, eph))
        self.fix, self.pr = self.add(G.Guarded(eng, n_rx * 128)), self.add(G.Guarded(eng, self.n_ch * 8))
        self.fde, self.vel = self.add(G.Guarded(eng, n_rx * 64)), self.add(G.Guarded(eng, n_rx * 112))

    def wfix(self, cfg, prev=None):
        self.fix.refill(), self.pr.refill()
        self.eng._chk(self.eng.lib.gpsx_wfix_dev(self.eng.h, cfg.ctypes.data, self.obs.ptr, self.eph.ptr, None, prev, self.n_rx, self.fix.ptr, self.pr.ptr),
                      "gpsx_wfix_dev")
        assert self.eng.lib.gpsx_last_kernel(self.eng.h) == b"k_wfix"
        self.eng.synchronize()
        return self.fix.get(F.FIX_DTYPE, self.n_rx), self.pr.get(np.float64, self.n_ch)

    def wfde(self, cfg):
        self.fix.refill(), self.pr.refill(), self.fde.refill()
        self.eng._chk(self.eng.lib.gpsx_wfde_dev(self.eng.h, cfg.ctypes.data, self.obs.ptr, self.eph.ptr, None, None, self.n_rx, self.fix.ptr, self.fde.ptr,
                                                 self.pr.ptr), "gpsx_wfde_dev")
        assert self.eng.lib.gpsx_last_kernel(self.eng.h) == b"k_wfde"
        self.eng.synchronize()
        return self.fix.get(F.FIX_DTYPE, self.n_rx), self.fde.get(D.FDE_DTYPE, self.n_rx), self.pr.get(np.float64, self.n_ch)

    def wvel(self, cfg, d_fix):
        self.vel.refill()
        self.eng._chk(self.eng.lib.gpsx_wvel_dev(self.eng.h, cfg.ctypes.data, self.obs.ptr, self.eph.ptr, None, d_fix, self.n_rx, self.vel.ptr), "gpsx_wvel_dev")
        assert self.eng.lib.gpsx_last_kernel(self.eng.h) == b"k_wvel"
        self.eng.synchronize()
        return self.vel.get(V.VEL_DTYPE, self.n_rx)


def _cfgs(ch):
    """the binding's configurations, which must be the restatements' byte for byte -> (gpsx_wfix's, gpsx_wvel's)"""
    from stm32f4_sdr_gps_amd import capi
    fcfg, vcfg = capi.wfix_cfg(X.OFFSET_MS, ch), capi.wvel_cfg(ch)
    assert fcfg.tobytes() == F.make_cfg(X.OFFSET_MS, ch).tobytes() and vcfg.tobytes() == V.make_cfg(ch).tobytes()
    return fcfg, vcfg


def _shifted_equal_but_for_week(names, fix):
    """the copies whole weeks away: munich_plus' bytes but for `week`, which moved with the records"""
    at = {n: r for r, n in enumerate(names)}
    base = fix[at["munich_plus"]].copy()
    assert int(base["flags"]) == F.F_FIX and int(base["week"]) == MUNICH_WEEK
    seen = 0
    for name, weeks in X.SHIFTS.items():
        if name in at:
            got = fix[at[name]].copy()
            assert int(got["week"]) == MUNICH_WEEK + weeks, (name, int(got["week"]))
            got["week"] = base["week"]
            assert got.tobytes() == base.tobytes(), name
            seen += 1
    return seen


@pytest.mark.parametrize("ch,n_rx", X.SHAPES)
def test_gpsx_wfix_dev_cold_and_warm_equals_the_restatement(eng, ch, n_rx):
    """every launch from the origin and from 30 km off (d_prev): weighted_edge_cases.compare against weighted_fix_ref -- flags, n_used,
    used_mask (the far side of the 7201 s limit costs exactly its slot), ref_slot, week, rx_tow_s and pr_m exact, the receivers whose
    transmit times straddle the week's end and the previous week's broadcast included; the same call twice gives the same bytes; the
    copies whole weeks away are byte-identical but for week"""
    case = X.launch_case(ch, n_rx)
    fcfg, _ = _cfgs(ch)
    want, want_pr = X.want_fix(ch, n_rx)
    warm_want, _ = X.want_fix(ch, n_rx, True)
    with _Inputs(eng, case["obs"], case["eph"], n_rx) as run:
        got, got_pr = run.wfix(fcfg)
        again, again_pr = run.wfix(fcfg)
        with G.Guarded(eng, want.nbytes, G.STATE_FILL, X.warm_start(want)) as prev:
            warm, warm_pr = run.wfix(fcfg, prev.ptr)
    print("parity cold", ch, n_rx, X.compare(got, got_pr, want, want_pr, label=f"wfix cold {ch} x {n_rx}", names=case["names"]))
    print("parity warm", ch, n_rx, X.compare(warm, warm_pr, warm_want, want_pr, label=f"wfix warm {ch} x {n_rx}", names=case["names"]))
    assert got.tobytes() == again.tobytes() and got_pr.tobytes() == again_pr.tobytes()
    assert _shifted_equal_but_for_week(case["names"], got) >= (2 if n_rx == 17 else 4) and _shifted_equal_but_for_week(case["names"], warm)
    solved = [r for r, n in enumerate(case["names"]) if n in X.SOLVED]
    assert (got["flags"][solved] == F.F_FIX).all() and (warm["flags"][solved] == F.F_FIX).all()
    for name in X.NOT_SOLVED_BY_WFIX:      # what they are there for: pr_m, ref_slot, rx_tow_s, and the restatement's flag
        if name in case["names"]:
            r = case["names"].index(name)
            assert int(got["flags"][r]) == int(want["flags"][r]) == F.F_TOO_FEW and int(got["ref_slot"][r]) == int(want["ref_slot"][r]) >= 0
            assert got_pr[r * ch:(r + 1) * ch].tobytes() == want_pr[r * ch:(r + 1) * ch].tobytes() and got_pr[r * ch:(r + 1) * ch].any()


@pytest.mark.parametrize("ch,n_rx", X.SHAPES)
def test_gpsx_wfde_dev_without_repair_and_exclusion_is_gpsx_wfix_dev(eng, ch, n_rx):
    """repair = 0, max_excl = 0: d_fix and d_pr_m are gpsx_wfix_dev's byte for byte on the same device arrays -- k_wfde's own copy of the
    clock, the orbit, the group delay and the weights gives k_wfix's doubles at every one of these arguments"""
    case = X.launch_case(ch, n_rx)
    fcfg, _ = _cfgs(ch)
    with _Inputs(eng, case["obs"], case["eph"], n_rx) as run:
        want, want_pr = run.wfix(fcfg)
        fix, fde, pr = run.wfde(XF.cfg(ch, max_excl=0, repair=0))
    assert fix.tobytes() == want.tobytes() and pr.tobytes() == want_pr.tobytes()
    assert (fde["n_rounds"] == 1).all() and not fde["excl_mask"].any() and not (fde["plus_mask"] | fde["minus_mask"]).any()
    assert (((fde["flags"] & D.NOFIX) != 0) == ((want["flags"] & F.F_FIX) == 0)).all()


def test_gpsx_wfde_dev_finds_the_faults_and_milliseconds_at_the_edges(eng):
    """the kept draws of weighted_edge_cases.fde_draws (a 300 m fault, a slot a millisecond off, at either tk extreme and both polar
    sites) in one twelve-slot launch: the injected masks and nothing else, weighted_fde_cases.compare's exact fields and t_stat, the
    positions within this file's bound"""
    kept, (want, want_fde, want_pr, _) = X.fde_kept()
    obs, eph = XF.W.pack([(d["obs"], d["eph"]) for d in kept], 12)
    with _Inputs(eng, obs, eph, len(kept)) as run:
        fix, fde, pr = run.wfde(XF.cfg(12))
    assert all(X.fde_found(d, fde[r]) for r, d in enumerate(kept)), [(d["name"], d["kind"]) for r, d in enumerate(kept) if not X.fde_found(d, fde[r])]
    names = [d["name"] + " " + d["kind"] for d in kept]
    print("parity fde", X.compare(fix, pr, want, want_pr, bound=X.FDE_BOUND_M, label="wfde kept draws", stage="fde", names=names))
    for f in ("flags", "n_rounds", "n_excluded", "dof", "excl_mask", "plus_mask", "minus_mask", "reserved"):
        assert (fde[f] == want_fde[f]).all(), f
    assert fde["t_limit"].tobytes() == want_fde["t_limit"].tobytes()
    bound = 4.0 * np.sqrt((want_fde["dof"] + 4) * want_fde["t_stat"]) * X.FDE_BOUND_M / XF.MIN_SIGMA_M + 1e-12      # (weighted_fde_cases.t_stat_bound at this bound)
    assert (np.abs(fde["t_stat"] - want_fde["t_stat"]) <= bound).all()
    assert ((fix["flags"] & F.F_FIX) != 0).all()


@pytest.mark.parametrize("ch,n_rx", X.SHAPES)
def test_gpsx_wvel_dev_on_given_fix_records_equals_the_restatement(eng, ch, n_rx):
    """every launch on the true sites' records: weighted_vel_cases.compare against weighted_vel_ref under this file's bound -- the
    receivers whose t_sv lie within 50 ms of either side of the week's end and the one at 1800 s on the previous week's broadcast
    (tk = +5400 s through the fold) solved with every slot; the same call twice gives the same bytes; the copies whole weeks away are
    byte-identical"""
    case = X.launch_case(ch, n_rx)
    _, vcfg = _cfgs(ch)
    want = X.want_vel(ch, n_rx)
    with _Inputs(eng, case["obs"], case["eph"], n_rx) as run, G.Guarded(eng, case["fix"].nbytes, G.STATE_FILL, case["fix"]) as d_fix:
        got = run.wvel(vcfg, d_fix.ptr)
        again = run.wvel(vcfg, d_fix.ptr)
    print("parity vel", ch, n_rx, X.compare_vel(got, want, label=f"wvel given {ch} x {n_rx}", names=case["names"]))
    assert got.tobytes() == again.tobytes()
    at = {n: r for r, n in enumerate(case["names"])}
    for name in X.SHIFTS:
        assert name not in at or got[at[name]].tobytes() == got[at["munich_plus"]].tobytes(), name
    for name in ("straddle_a", "straddle_b", "prev_week"):
        if name in at:
            assert int(got["flags"][at[name]]) == V.F_VEL and int(got["n_used"][at[name]]) == min(ch, 12), name
    for name in ("far_plus", "far_minus"):      # its first satellite's slot is in used_mask and past the limit: no row
        r = at[name]
        assert int(got["flags"][r]) == V.F_VEL and int(got["used_mask"][r]) == int(case["fix"]["used_mask"][r]) & ~(1 << case["slots"][r][0])


def test_gpsx_wvel_dev_behind_gpsx_wfix_dev_on_the_device(eng):
    """12 x 27: gpsx_wfix_dev, then gpsx_wvel_dev on the fix records where they lie on the device -- the restatement's records on the
    device's own fixes; a receiver without FIX gives NO_FIX"""
    ch, n_rx = X.SHAPES[1]
    case = X.launch_case(ch, n_rx)
    fcfg, vcfg = _cfgs(ch)
    with _Inputs(eng, case["obs"], case["eph"], n_rx) as run:
        fix, _ = run.wfix(fcfg)
        vel = run.wvel(vcfg, run.fix.ptr)
    print("parity vel behind wfix", X.compare_vel(vel, V.run(vcfg, case["obs"], case["eph"], fix, n_rx), label=f"wvel behind wfix {ch} x {n_rx}", names=case["names"]))
    assert ((vel["flags"] == V.F_NO_FIX) == ((fix["flags"] & F.F_FIX) == 0)).all() and (vel["flags"] == V.F_VEL).sum() == len(X.SOLVED)
    assert not (vel["used_mask"] & ~fix["used_mask"]).any()
    _shifted = {n: r for r, n in enumerate(case["names"])}
    for name in X.SHIFTS:
        assert vel[_shifted[name]].tobytes() == vel[_shifted["munich_plus"]].tobytes(), name


def test_host_entry_points_equal_the_dev_ones(eng):
    """gpsx_wfix and gpsx_wvel on host arrays are gpsx_wfix_dev and gpsx_wvel_dev byte for byte on the 12 x 27 launch"""
    ch, n_rx = X.SHAPES[1]
    case = X.launch_case(ch, n_rx)
    fcfg, vcfg = _cfgs(ch)
    with _Inputs(eng, case["obs"], case["eph"], n_rx) as run, G.Guarded(eng, case["fix"].nbytes, G.STATE_FILL, case["fix"]) as d_fix:
        fix, pr = run.wfix(fcfg)
        vel = run.wvel(vcfg, d_fix.ptr)
    host, host_pr = eng.wfix(fcfg, case["obs"], case["eph"], n_rx, want_pr=True)
    assert eng.lib.gpsx_last_kernel(eng.h) == b"k_wfix"
    assert host.tobytes() == fix.tobytes() and host_pr.tobytes() == pr.tobytes()
    assert eng.wvel(vcfg, case["obs"], case["eph"], case["fix"], n_rx).tobytes() == vel.tobytes()
    assert eng.lib.gpsx_last_kernel(eng.h) == b"k_wvel"
