"""Every receiver's navigation filter on the device (include/gpsx.h gpsx_wkf_dev / gpsx_wkf, csrc/k_wkf.hip) against its CPU
restatement (tests/weighted_kf_ref.py) on sequences of launches built on the CPU (tests/weighted_kf_cases.py): every lane-group width
and receiver count, receivers of every kind as neighbours in a wave with the spoiled slot at the first, the last and a middle slot of
a group, both entry points and the binding, d_lock / d_vel / d_fix given and NULL, every refusal, one sequence behind gpsx_wfde_dev and
gpsx_wvel_dev on the device and one behind the device stages of the chain from IF samples.  States and records sit between 4096-byte
canaries, the records start as 0xA5, so a byte that is not written or is written beside them shows.  Decisions are compared for
equality: tests/test_weighted_kf_reference.py asserts that every compared receiver's stand clear of round-off.

Parity, measured on one MI355X (profiles/r24_weighted_kf_parity.json): see weighted_kf_cases.PARITY_MEASURED_M / _MPS."""
import ctypes as C

import numpy as np
import pytest

import weighted_fix_cases as W
import weighted_fix_ref as F
import weighted_gpu as G
import weighted_kf_cases as K
import weighted_kf_ref as R
import weighted_vel_ref as V
from weighted_gpu import GUARD, eng  # noqa: F401

pytestmark = pytest.mark.gpu
REC = R.KF_DTYPE.itemsize


def _sequence(eng, case, n_rx, dev=True, lock=True, vel=True, fix_until=None, binding=False):
    """the case's launches on zeroed states in guarded device memory; gpsx_wkf_dev on uploaded arrays (dev), gpsx_wkf on host arrays, or
    Engine.wkf (binding); before the last launch the case's `poke` is applied to the states.  lock / vel False: NULL; fix_until k: from
    launch k on d_fix is NULL -> ([records per launch], [states after each launch], [codes])"""
    cfg = K.cfg(int(case["cfg"]["ch_per_rx"][0]), max_coast=int(case["cfg"]["max_coast"][0]))
    n = len(case["obs"])
    recs, states, codes = [], [], []
    with G.Pool() as pool:
        d_state = pool.add(G.Guarded(eng, n_rx * 384, G.STATE_FILL, np.zeros(n_rx, R.STATE_DTYPE)))
        const = {}
        for name, on in (("eph", True), ("lock", lock), ("vel", vel)):
            a = case[name] if on else None
            const[name] = None if a is None else (pool.add(G.Guarded(eng, a.nbytes, G.STATE_FILL, a)).ptr if dev and not binding else a)
        for k in range(n):
            if k == n - 1 and case["poke"]:
                st = d_state.get(R.STATE_DTYPE, n_rx)
                for r, fields in case["poke"].items():
                    for name, val in fields.items():
                        st[name][r] = val
                d_state.put(st)
            fix = case["fix"][k] if fix_until is None or k < fix_until else None
            if binding:
                try:
                    rec, rc = eng.wkf(cfg, case["obs"][k], case["eph"], n_rx, case["n_blocks"], d_state.base + GUARD, fix=fix, vel=const["vel"],
                                      lock=const["lock"]), 0
                except Exception:      # (a BAD state: the binding raises after the records were copied back; the raw call shows them)
                    rec, rc = None, G.EINVAL
                recs.append(rec)
                codes.append(rc)
                states.append(d_state.get(R.STATE_DTYPE, n_rx))
                continue
            with G.Pool() as launch:
                def arg(a):
                    if a is None:
                        return None
                    return launch.add(G.Guarded(eng, a.nbytes, G.STATE_FILL, a)).ptr if dev else a.ctypes.data
                p_obs, p_fix = arg(case["obs"][k]), arg(fix)
                host = (lambda a: None if a is None else a.ctypes.data)
                out = launch.add(G.Guarded(eng if dev else None, n_rx * REC))
                fn = eng.lib.gpsx_wkf_dev if dev else eng.lib.gpsx_wkf
                rc = fn(eng.h, cfg.ctypes.data, p_obs, const["eph"] if dev else host(const["eph"]), const["lock"] if dev else host(const["lock"]), p_fix,
                        const["vel"] if dev else host(const["vel"]), n_rx, case["n_blocks"], d_state.ptr, out.ptr)
                if dev:
                    assert rc == 0, (rc, eng.lib.gpsx_last_error(eng.h))
                    rc = eng.lib.gpsx_synchronize(eng.h)
                assert eng.lib.gpsx_last_kernel(eng.h) == b"k_wkf"
                codes.append(rc)
                recs.append(out.get(R.KF_DTYPE, n_rx))
                states.append(d_state.get(R.STATE_DTYPE, n_rx))
    return recs, states, codes


@pytest.mark.parametrize("n_rx", K.SHAPES_RX)
@pytest.mark.parametrize("ch", K.SHAPES_CH)
def test_every_shape_and_receiver_mix_equals_the_restatement(eng, ch, n_rx):
    """ch_per_rx x n_rx over every group width (1, 4, 8, 16, 64), a second workgroup (67 x 4 and wider), waves with dead upper lanes
    (17 x 33): weighted_kf_cases.launch_case's four launches, compared as weighted_kf_cases.compare orders it, the states after every
    launch too (a BAD state stays as it was, byte for byte); every byte of d_kf is written and nothing beside it or beside the
    states; the same sequence twice gives the same bytes"""
    case = K.launch_case(ch, n_rx)
    recs, states, codes = _sequence(eng, case, n_rx)
    again, states2, _ = _sequence(eng, case, n_rx)
    for k in range(K.N_LAUNCH):
        print("parity", ch, n_rx, k, K.compare(recs[k], case["want"][k], label=f"shapes {ch} x {n_rx} launch {k}"))
        K.compare_states(states[k], case["states"][k])
        assert recs[k].tobytes() == again[k].tobytes() and states[k].tobytes() == states2[k].tobytes()
    assert codes == case["codes"]
    for r, fields in case["poke"].items():      # (the device's own state of the launch before, with what was poked)
        was = states[-2][r:r + 1].copy()
        for name, val in fields.items():
            was[name] = val
        assert states[-1][r:r + 1].tobytes() == was.tobytes()
    if ch >= 5 and n_rx >= 17:
        seen = set(np.concatenate([rec["flags"] & 63 for rec in recs]).tolist())
        assert seen == {R.F_INIT, R.F_NOT_INIT, R.F_UPDATED, R.F_COAST, R.F_LOST, R.F_BAD}, seen
        assert (recs[-1]["flags"] & R.F_REPAIRED).any() and (recs[-1]["flags"] & R.F_REJECTED).any()


def test_host_arrays_and_the_binding_equal_device_arrays(eng):
    """gpsx_wkf (host arrays) equals gpsx_wkf_dev byte for byte in records and states, and so does the binding's Engine.wkf; the same
    with d_lock and d_vel NULL, against the restatement without them; with d_fix NULL from the second launch on the receivers that
    were initialised give the same bytes and the fresh ones stay NOT_INIT"""
    for ch, n_rx in ((12, 17), (5, 67), (64, 17)):
        case = K.launch_case(ch, n_rx)
        for lock, vel in ((True, True), (False, False)):
            dev = _sequence(eng, case, n_rx, lock=lock, vel=vel)
            host = _sequence(eng, case, n_rx, dev=False, lock=lock, vel=vel)
            bind = _sequence(eng, case, n_rx, binding=True, lock=lock, vel=vel)
            assert dev[2] == host[2] == bind[2] == case["codes"]
            state = np.zeros(n_rx, R.STATE_DTYPE)
            for k in range(K.N_LAUNCH):
                assert dev[0][k].tobytes() == host[0][k].tobytes() and dev[1][k].tobytes() == host[1][k].tobytes() == bind[1][k].tobytes()
                assert bind[0][k] is None or bind[0][k].tobytes() == dev[0][k].tobytes()
                if not lock:      # (with both: the shapes test's comparison)
                    if k == K.N_LAUNCH - 1:
                        for r, fields in case["poke"].items():
                            for name, val in fields.items():
                                state[name][r] = val
                    want, state, _ = R.run(case["cfg"], case["obs"][k], case["eph"], state, n_rx, case["n_blocks"], None, case["fix"][k], None)
                    K.compare(dev[0][k], want)
        nofix = _sequence(eng, case, n_rx, fix_until=1)
        full = _sequence(eng, case, n_rx)
        kept = np.array([k not in ("fresh", "starved") for k in case["kinds"]])
        for k in range(K.N_LAUNCH):
            assert nofix[0][k][kept].tobytes() == full[0][k][kept].tobytes()
        fresh = np.array([k == "fresh" for k in case["kinds"]])
        assert (nofix[0][-1]["flags"][fresh] == R.F_NOT_INIT).all() and (full[0][-1]["flags"][fresh] == R.F_INIT).all()


def test_host_arrays_without_fix_equal_device_arrays(eng):
    """gpsx_wkf (host arrays) with fix NULL from the second launch on, lock and vel given: records and states equal gpsx_wkf_dev's with
    d_fix NULL byte for byte, and the restatement's without the records"""
    ch, n_rx = 8, 2
    case = K.launch_case(ch, n_rx)
    dev = _sequence(eng, case, n_rx, fix_until=1)
    host = _sequence(eng, case, n_rx, dev=False, fix_until=1)
    assert dev[2] == host[2]
    state = np.zeros(n_rx, R.STATE_DTYPE)
    for k in range(K.N_LAUNCH):
        assert dev[0][k].tobytes() == host[0][k].tobytes() and dev[1][k].tobytes() == host[1][k].tobytes()
        if k == K.N_LAUNCH - 1:
            for r, fields in case["poke"].items():
                for name, val in fields.items():
                    state[name][r] = val
        want, state, _ = R.run(case["cfg"], case["obs"][k], case["eph"], state, n_rx, case["n_blocks"], case["lock"], case["fix"][k] if k < 1 else None,
                               case["vel"])
        K.compare(dev[0][k], want)


def test_every_refusal_returns_einval_and_writes_nothing(eng):
    """every error clause of the header but the size overflow (which no n_rx <= 2^20 x ch_per_rx <= 64 can reach on a 64-bit size_t),
    each with its text, in both variants; then the context still works"""
    ch, n_rx = 5, 2
    case = K.launch_case(ch, n_rx)
    good_cfg = K.cfg(ch, max_coast=K.MAX_COAST)

    def cfg_with(**kw):
        c = good_cfg.copy()
        for k, v in kw.items():
            if k.startswith("reserved"):
                c["reserved"][0, int(k[8:])] = v
            elif k.startswith("ion"):
                c["ion"][0, int(k[3:])] = v
            else:
                c[k] = v
        return c

    inputs = (case["obs"][0], case["eph"], case["lock"], case["fix"][0], case["vel"])
    with G.Pool() as pool:
        dev_in = [pool.add(G.Guarded(eng, a.nbytes, G.STATE_FILL, a)) for a in inputs]
        d_state = pool.add(G.Guarded(eng, n_rx * 384, G.STATE_FILL, np.zeros(n_rx, R.STATE_DTYPE)))
        d_out, h_out = pool.add(G.Guarded(eng, n_rx * REC)), pool.add(G.Guarded(None, n_rx * REC))
        good = dict(ctx=eng.h, cfg=good_cfg, obs=0, eph=1, lock=2, fix=3, vel=4, n_rx=n_rx, n_blocks=1000, state=0, out=0)

        def call(a, dev):
            def ptr(k):      # an index: that input; None: NULL
                return None if a[k] is None else (dev_in[a[k]].ptr if dev else inputs[a[k]].ctypes.data)
            out = None if a["out"] is None else C.c_void_p((d_out if dev else h_out).base + GUARD + a["out"])
            state = None if a["state"] is None else C.c_void_p(d_state.base + GUARD + a["state"])
            fn = eng.lib.gpsx_wkf_dev if dev else eng.lib.gpsx_wkf
            return fn(a["ctx"], None if a["cfg"] is None else a["cfg"].ctypes.data, ptr("obs"), ptr("eph"), ptr("lock"), ptr("fix"), ptr("vel"), a["n_rx"],
                      a["n_blocks"], state, out)

        bad_values = (np.nan, np.inf, -np.inf)
        G.refusals(eng, {
            b"null argument": [dict(cfg=None), dict(obs=None), dict(eph=None), dict(state=None), dict(out=None)],
            b"ch_per_rx must be 1..64": [dict(cfg=cfg_with(ch_per_rx=v)) for v in (0, -1, 65)],
            b"n_rx must be 1..1048576": [dict(n_rx=v) for v in (0, -1, (1 << 20) + 1)],
            b"n_blocks must be 1..4096": [dict(n_blocks=v) for v in (0, -1, 4097)],
            b"max_coast must be 0..1000000": [dict(cfg=cfg_with(max_coast=v)) for v in (-1, 1000001)],
            b"gate must be finite, above 0 and at most 100": [dict(cfg=cfg_with(gate=v)) for v in bad_values + (0.0, -1.0, 100.5)],
            b"sig_dop_mps must be finite and above 0": [dict(cfg=cfg_with(sig_dop_mps=v)) for v in bad_values + (0.0, -0.1)],
            b"sig_pr_m, q_* and p0_* must be finite and not negative": [dict(cfg=cfg_with(**{f: v})) for f in (
                "sig_pr_m", "q_acc", "q_clk_f", "q_clk_g", "p0_pos", "p0_clk", "p0_vel", "p0_drift") for v in (np.nan, np.inf, -1.0)],
            b"p0_* must not be 0": [dict(cfg=cfg_with(**{f: 0.0})) for f in ("p0_pos", "p0_clk", "p0_vel", "p0_drift")],
            b"mps_per_hz must be finite and not 0": [dict(cfg=cfg_with(mps_per_hz=v)) for v in bad_values + (0.0,)],
            b"an ionosphere coefficient is not finite": [dict(cfg=cfg_with(**{f"ion{k}": v})) for k, v in ((0, np.nan), (7, np.inf))],
            b"reserved must be 0": [dict(cfg=cfg_with(**{f"reserved{k}": v})) for k, v in ((0, 1), (1, -1), (2, 7), (3, 1 << 30))],
            b"d_state must be 16-byte aligned": [dict(state=8)],
        }, good, call, [d_out, h_out, d_state] + dev_in)
        # the record's alignment rule is the _dev variant's alone; a NULL context has no error text to read: its code alone
        d_out.refill()
        assert call({**good, "out": 8}, True) == G.EINVAL and eng.lib.gpsx_last_error(eng.h) == b"d_kf must be 16-byte aligned"
        assert call({**good, "ctx": None}, True) == G.EINVAL and call({**good, "ctx": None}, False) == G.EINVAL
        eng.synchronize()
        assert d_out.untouched() and h_out.untouched() and d_state.untouched()
        eng._chk(call(good, True), "gpsx_wkf_dev")
        eng.synchronize()
        K.compare(d_out.get(R.KF_DTYPE, n_rx), case["want"][0])


def test_behind_gpsx_wfde_dev_and_gpsx_wvel_dev_on_the_device(eng):
    """two launches of weighted_kf_cases.launch_case(12, 17): gpsx_wfde_dev and gpsx_wvel_dev write d_fix / d_vel on the device and
    gpsx_wkf_dev initialises from them where they lie, then updates; every record is the restatement's on the device's own fix and
    velocity records"""
    from stm32f4_sdr_gps_amd import capi
    ch, n_rx = 12, 17
    case = K.launch_case(ch, n_rx)
    fcfg, vcfg, kcfg = capi.wfde_cfg(W.OFFSET_MS, ch), capi.wvel_cfg(ch), K.cfg(ch, max_coast=K.MAX_COAST)
    state = np.zeros(n_rx, R.STATE_DTYPE)
    with G.Pool() as pool:
        d_eph = pool.add(G.Guarded(eng, case["eph"].nbytes, G.STATE_FILL, case["eph"]))
        d_state = pool.add(G.Guarded(eng, n_rx * 384, G.STATE_FILL, state))
        d_fix, d_fde, d_vel = pool.add(G.Guarded(eng, n_rx * 128)), pool.add(G.Guarded(eng, n_rx * 64)), pool.add(G.Guarded(eng, n_rx * 112))
        for k in range(2):
            with G.Guarded(eng, case["obs"][k].nbytes, G.STATE_FILL, case["obs"][k]) as d_obs, G.Guarded(eng, n_rx * REC) as d_kf:
                eng._chk(eng.lib.gpsx_wfde_dev(eng.h, fcfg.ctypes.data, d_obs.ptr, d_eph.ptr, None, None, n_rx, d_fix.ptr, d_fde.ptr, None), "gpsx_wfde_dev")
                eng._chk(eng.lib.gpsx_wvel_dev(eng.h, vcfg.ctypes.data, d_obs.ptr, d_eph.ptr, None, d_fix.ptr, n_rx, d_vel.ptr), "gpsx_wvel_dev")
                eng._chk(eng.lib.gpsx_wkf_dev(eng.h, kcfg.ctypes.data, d_obs.ptr, d_eph.ptr, None, d_fix.ptr, d_vel.ptr, n_rx, case["n_blocks"], d_state.ptr,
                                              d_kf.ptr), "gpsx_wkf_dev")
                assert eng.lib.gpsx_last_kernel(eng.h) == b"k_wkf"
                eng.synchronize()
                fix, vel, got = d_fix.get(F.FIX_DTYPE, n_rx), d_vel.get(V.VEL_DTYPE, n_rx), d_kf.get(R.KF_DTYPE, n_rx)
            want, state, rc = R.run(kcfg, case["obs"][k], case["eph"], state, n_rx, case["n_blocks"], None, fix, vel)
            print("parity", K.compare(got, want, label=f"behind gpsx_wfde_dev {ch} x {n_rx} launch {k}"))
            K.compare_states(d_state.get(R.STATE_DTYPE, n_rx), state)
            fixed = (fix["flags"] & F.F_FIX) != 0
            if k == 0:
                assert fixed.sum() >= 10 and (got["flags"][fixed] == R.F_INIT).all() and (got["flags"][~fixed] == R.F_NOT_INIT).all()
                has_vel = fixed & (vel["flags"] == V.F_VEL)
                assert has_vel.any() and np.array_equal(got["vel"][has_vel], vel["vel"][has_vel])
            else:
                assert ((got["flags"] & R.F_UPDATED) != 0).sum() >= 10


def test_behind_the_device_stages_from_if_samples(eng):
    """weighted_pvt_cases' stream (four orbiting satellites, 25 000 blocks, MOVING gains; the receiver stands still, its clock is GPS
    time) through the device stages in weighted_pvt_cases.LAUNCHES, with gpsx_wfix_dev, gpsx_wvel_dev and gpsx_wkf_dev after every
    launch on the arrays where they lie: the last record equals the restatement's on the device's own arrays (the restatement carried
    through every launch), and the speed of the receiver at rest is within 1.5 x what the CPU chain gives (weighted_kf_cases.MEASURED).
    Cost: the stream's synthesis (about 25 s of CPU, cached per process in weighted_pvt_cases._memo) and its upload, plus a few seconds
    of GPU."""
    import weighted_pvt_cases as P
    from stm32f4_sdr_gps_amd import capi
    lib, n_ch = eng.lib, 4
    blocks = P.blocks()
    d_if = eng.malloc(blocks.nbytes)
    eng.h2d(d_if, blocks)
    st0 = dict(P.fresh_states(), sync=P.handover(), lock=np.zeros(n_ch, capi.WLOCK_STATE_DTYPE))
    chain = G.Chain(eng, P.sync_cfg_dev(P.MOVING), st0, max(P.LAUNCHES), P.MAX_BAD_WORDS, P.EDGE_GUARD, capi.wlock_cfg(25, 10, 1.5, 0.3, 1.0, 2, 2))
    fcfg, vcfg, kcfg = K.if_cfgs()
    bufs = dict(chain.buf, fix=G.Guarded(eng, F.FIX_DTYPE.itemsize), vel=G.Guarded(eng, V.VEL_DTYPE.itemsize), kf=G.Guarded(eng, REC),
                state=G.Guarded(eng, 384, G.STATE_FILL, np.zeros(1, R.STATE_DTYPE)))
    try:
        at, state, flags = 0, np.zeros(1, R.STATE_DTYPE), []
        for n in P.LAUNCHES:
            chain.sync(d_if + at * 4092, n)
            chain.words()
            chain.obs()
            chain.eph()
            chain.lock()
            bufs["kf"].refill()
            eng._chk(lib.gpsx_wfix_dev(eng.h, fcfg.ctypes.data, bufs["o"].ptr, bufs["e"].ptr, None, bufs["fix"].ptr if at else None, 1, bufs["fix"].ptr, None),
                     "gpsx_wfix_dev")
            eng._chk(lib.gpsx_wvel_dev(eng.h, vcfg.ctypes.data, bufs["o"].ptr, bufs["e"].ptr, None, bufs["fix"].ptr, 1, bufs["vel"].ptr), "gpsx_wvel_dev")
            eng._chk(lib.gpsx_wkf_dev(eng.h, kcfg.ctypes.data, bufs["o"].ptr, bufs["e"].ptr, None, bufs["fix"].ptr, bufs["vel"].ptr, 1, n, bufs["state"].ptr,
                                      bufs["kf"].ptr), "gpsx_wkf_dev")
            assert lib.gpsx_last_kernel(eng.h) == b"k_wkf"
            eng.synchronize()
            at += n
            obs, eph = chain.read("o"), chain.read("e")
            fix, vel, got = bufs["fix"].get(F.FIX_DTYPE, 1), bufs["vel"].get(V.VEL_DTYPE, 1), bufs["kf"].get(R.KF_DTYPE, 1)
            want, state, rc = R.run(kcfg, obs, eph, state, 1, n, None, fix, vel)
            flags.append(int(got["flags"][0]))
            assert rc == 0 and int(want["flags"][0]) == flags[-1], (at, flags, want["flags"])
        speed = float(np.linalg.norm(got["vel"][0]))
        print("flags", flags, "vel", got["vel"][0], "|vel|", speed, "cdrift", float(got["cdrift_mps"][0]), "position error",
              float(np.linalg.norm(got["rr"][0] - P.RX)), "n_pr", int(got["n_pr"][0]), "n_dop", int(got["n_dop"][0]))
        print("parity", K.compare(got, want, label="from IF samples"))
        K.compare_states(bufs["state"].get(R.STATE_DTYPE, 1), state)
        assert flags[-1] & (R.F_INIT | R.F_UPDATED)
        assert speed <= 1.5 * K.MEASURED["if_speed_mps"]
    finally:
        for name in ("fix", "vel", "kf", "state"):
            bufs[name].free()
        chain.free()
        eng.free(d_if)
