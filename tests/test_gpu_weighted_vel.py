"""Every receiver's velocity and clock drift on the device (include/gpsx.h gpsx_wvel_dev / gpsx_wvel, csrc/k_wvel.hip) against its CPU
restatement (tests/weighted_vel_ref.py) on records built on the CPU (tests/weighted_vel_cases.py): every lane-group width and receiver
count, every kind of slot that gives no row at the first, the last and a middle slot of a group, receivers of every outcome as
neighbours in a wave, both entry points, d_lock given and NULL, every refusal, one run behind gpsx_wfde_dev on the device and one
behind the device stages of the chain from IF samples.  Outputs sit between 4096-byte canaries and start as 0xA5, so a byte that is
not written shows.  Decisions are compared for equality: tests/test_weighted_vel_reference.py asserts that every compared receiver's
stand clear of round-off.

Parity, measured on one MI355X (profiles/r22_weighted_vel_parity.json): see weighted_vel_cases.PARITY_MEASURED_MPS."""
import ctypes as C

import numpy as np
import pytest

import weighted_fde_ref as D
import weighted_fix_ref as F
import weighted_gpu as G
import weighted_vel_cases as K
import weighted_vel_ref as V
from weighted_gpu import GUARD, eng  # noqa: F401

pytestmark = pytest.mark.gpu


def _stage(eng, cfg, obs, eph, lock, fix, n_rx, dev=True, times=1):
    """weighted_gpu.run_stage on gpsx_wvel_dev (dev) or gpsx_wvel: the four input arrays uploaded (dev) or passed as they are, the output
    guarded and prefilled; `times` launches on the same inputs -> [VEL_DTYPE [n_rx] per launch]"""
    fn = eng.lib.gpsx_wvel_dev if dev else eng.lib.gpsx_wvel

    def call(p, states, out, k):
        return fn(eng.h, cfg.ctypes.data, p[0], p[1], p[2], p[3], n_rx, out)

    outs, _, codes = G.run_stage(eng, call, b"k_wvel", [], [([obs, eph, lock, fix], V.VEL_DTYPE, (n_rx,))] * times, dev=dev, host_inputs=True)
    assert codes == [0] * times, codes
    return outs


@pytest.mark.parametrize("n_rx", K.SHAPES_RX)
@pytest.mark.parametrize("ch", K.SHAPES_CH)
def test_every_shape_and_slot_mix_equals_the_restatement(eng, ch, n_rx):
    """ch_per_rx x n_rx over every group width (1, 4, 8, 16, 64), a second workgroup (67 x 4 and wider), waves with dead upper lanes
    (17 x 33): weighted_vel_cases.launch_case's slot kinds and receiver kinds, compared as weighted_vel_cases.compare orders it (flags,
    n_used, masks equal; without VEL the bytes equal; with VEL within the parity bound); every byte of d_vel is written and nothing
    beside it; the same call twice gives the same bytes"""
    case = K.launch_case(ch, n_rx)
    got, again = _stage(eng, K.cfg(ch), case["obs"], case["eph"], case["lock"], case["fix"], n_rx, times=2)
    print("parity", ch, n_rx, K.compare(got, case["want"], label=f"shapes {ch} x {n_rx}"))
    assert got.tobytes() == again.tobytes()
    if ch >= 5 and n_rx >= 17:
        assert set(got["flags"].tolist()) == {V.F_VEL, V.F_NO_FIX, V.F_TOO_FEW, V.F_SINGULAR, V.F_NONFINITE}


def test_host_arrays_equal_device_arrays_and_the_lock_argument(eng):
    """gpsx_wvel (host arrays) equals gpsx_wvel_dev byte for byte, and so does the binding's Engine.wvel; with d_lock NULL the slot
    that a no_carrier receiver lost comes back (the restatement's record without lock records), every other receiver's bytes stay"""
    for ch, n_rx in ((12, 17), (5, 67), (64, 17)):
        case = K.launch_case(ch, n_rx)
        cfg, args = K.cfg(ch), (case["obs"], case["eph"])
        dev = _stage(eng, cfg, *args, case["lock"], case["fix"], n_rx)[0]
        host = _stage(eng, cfg, *args, case["lock"], case["fix"], n_rx, dev=False)[0]
        assert dev.tobytes() == host.tobytes() == eng.wvel(cfg, *args, case["fix"], n_rx, lock=case["lock"]).tobytes()
        free = _stage(eng, cfg, *args, None, case["fix"], n_rx)[0]
        assert free.tobytes() == _stage(eng, cfg, *args, None, case["fix"], n_rx, dev=False)[0].tobytes() == eng.wvel(cfg, *args, case["fix"], n_rx).tobytes()
        K.compare(free, V.run(cfg, *args, case["fix"], n_rx))
        lost = np.array([k == "no_carrier" for k in case["kinds"]])
        assert lost.any() and free[~lost].tobytes() == dev[~lost].tobytes()
        for r in np.flatnonzero(lost):
            assert int(free["used_mask"][r]) == int(dev["used_mask"][r]) | (1 << case["spoiled"][r]) and int(free["n_used"][r]) == int(dev["n_used"][r]) + 1


def test_the_other_sign_convention_gives_the_same_bytes(eng):
    """mps_per_hz = -GPSX_WVEL_L1CA on negated Dopplers: the same doubles, the same records"""
    ch, n_rx = 8, 17
    case = K.launch_case(ch, n_rx)
    other = case["obs"].copy()
    other["if_freq_offset_hz"] = -other["if_freq_offset_hz"]
    a = _stage(eng, K.cfg(ch), case["obs"], case["eph"], case["lock"], case["fix"], n_rx)[0]
    b = _stage(eng, K.cfg(ch, mps_per_hz=-V.L1CA), other, case["eph"], case["lock"], case["fix"], n_rx)[0]
    assert a.tobytes() == b.tobytes() and (a["flags"] == V.F_VEL).sum() >= 10


def test_every_refusal_returns_einval_and_writes_nothing(eng):
    """every error clause of the header but the size overflow (which no n_rx <= 2^20 x ch_per_rx <= 64 can reach on a 64-bit size_t),
    each with its text, in both variants; then the context still works"""
    ch, n_rx = 5, 2
    case = K.launch_case(ch, n_rx)
    good_cfg = K.cfg(ch)

    def cfg_with(**kw):
        c = good_cfg.copy()
        for k, v in kw.items():
            if k.startswith("reserved"):
                c["reserved"][0, int(k[8:])] = v
            else:
                c[k] = v
        return c

    with G.Pool() as pool:
        dev_in = [pool.add(G.Guarded(eng, a.nbytes, G.STATE_FILL, a)) for a in (case["obs"], case["eph"], case["lock"], case["fix"])]
        d_out, h_out = pool.add(G.Guarded(eng, n_rx * 112)), pool.add(G.Guarded(None, n_rx * 112))
        host_in = [case["obs"], case["eph"], case["lock"], case["fix"]]
        good = dict(ctx=eng.h, cfg=good_cfg, obs=0, eph=1, lock=2, fix=3, n_rx=n_rx, out=0)

        def call(a, dev):
            def ptr(k):      # an index: that input; None: NULL
                return None if a[k] is None else (dev_in[a[k]].ptr if dev else host_in[a[k]].ctypes.data)
            out = None if a["out"] is None else C.c_void_p((d_out if dev else h_out).base + GUARD + a["out"])
            fn = eng.lib.gpsx_wvel_dev if dev else eng.lib.gpsx_wvel
            return fn(a["ctx"], None if a["cfg"] is None else a["cfg"].ctypes.data, ptr("obs"), ptr("eph"), ptr("lock"), ptr("fix"), a["n_rx"], out)

        G.refusals(eng, {
            b"null argument": [dict(cfg=None), dict(obs=None), dict(eph=None), dict(fix=None), dict(out=None)],
            b"mps_per_hz must be finite and not 0": [dict(cfg=cfg_with(mps_per_hz=v)) for v in (np.nan, np.inf, -np.inf, 0.0, -0.0)],
            b"ch_per_rx must be 1..64": [dict(cfg=cfg_with(ch_per_rx=v)) for v in (0, -1, 65)],
            b"min_sats must be 4..64": [dict(cfg=cfg_with(min_sats=v)) for v in (3, 0, 65)],
            b"reserved must be 0": [dict(cfg=cfg_with(**{f"reserved{k}": v})) for k, v in ((0, 1), (1, -1), (2, 7), (3, 1 << 30))],
            b"n_rx must be 1..1048576": [dict(n_rx=v) for v in (0, -1, (1 << 20) + 1)],
        }, good, call, [d_out, h_out] + dev_in)
        # the alignment rule is the _dev variant's alone; a NULL context has no error text to read: its code alone
        d_out.refill()
        assert call({**good, "out": 8}, True) == G.EINVAL and eng.lib.gpsx_last_error(eng.h) == b"d_vel must be 16-byte aligned"
        assert call({**good, "ctx": None}, True) == G.EINVAL and call({**good, "ctx": None}, False) == G.EINVAL
        eng.synchronize()
        assert d_out.untouched() and h_out.untouched()
        eng._chk(call(good, True), "gpsx_wvel_dev")
        eng.synchronize()
        K.compare(d_out.get(V.VEL_DTYPE, n_rx), case["want"])


def test_behind_gpsx_wfde_dev_on_the_device(eng):
    """weighted_fde_cases' launch (12 x 67: clean, faulty, millisecond-shifted and unfixable receivers as neighbours) with Dopplers of a
    moving receiver: gpsx_wfde_dev, then gpsx_wvel_dev on the fix records where they lie on the device.  A slot that the exclusion or
    the repair took out gives no Doppler row; every record is the restatement's on the device's own fix records; a one_fault receiver
    whose excluded slot also carries a 50 Hz Doppler fault gets the velocity of the clean Dopplers, byte for byte, where an unexcluded
    fault of that size would move it by metres per second"""
    ch, n_rx = 12, 67
    case = K.fde_launch(ch, n_rx)
    vcfg = K.cfg(ch)
    with G.Pool() as pool:
        d_eph, d_lock = (pool.add(G.Guarded(eng, a.nbytes, G.STATE_FILL, a)) for a in (case["eph"], case["lock"]))
        d_obs = {name: pool.add(G.Guarded(eng, case[name].nbytes, G.STATE_FILL, case[name])) for name in ("obs", "obs_faulty")}
        d_fix, d_fde, d_vel = pool.add(G.Guarded(eng, n_rx * 128)), pool.add(G.Guarded(eng, n_rx * 64)), pool.add(G.Guarded(eng, n_rx * 112))
        got = {}
        for name in ("obs", "obs_faulty"):
            d_vel.refill()
            eng._chk(eng.lib.gpsx_wfde_dev(eng.h, case["cfg"].ctypes.data, d_obs[name].ptr, d_eph.ptr, d_lock.ptr, None, n_rx, d_fix.ptr, d_fde.ptr, None),
                     "gpsx_wfde_dev")
            eng._chk(eng.lib.gpsx_wvel_dev(eng.h, vcfg.ctypes.data, d_obs[name].ptr, d_eph.ptr, None, d_fix.ptr, n_rx, d_vel.ptr), "gpsx_wvel_dev")
            assert eng.lib.gpsx_last_kernel(eng.h) == b"k_wvel"
            eng.synchronize()
            got[name] = (d_fix.get(F.FIX_DTYPE, n_rx), d_fde.get(D.FDE_DTYPE, n_rx), d_vel.get(V.VEL_DTYPE, n_rx))
    fix, fde, vel = got["obs"]
    assert fix.tobytes() == got["obs_faulty"][0].tobytes() and fde.tobytes() == got["obs_faulty"][1].tobytes()      # (the fixes read no Doppler)
    print("parity", K.compare(vel, V.run(vcfg, case["obs"], case["eph"], fix, n_rx), label=f"behind gpsx_wfde_dev {ch} x {n_rx}"))
    K.compare(got["obs_faulty"][2], V.run(vcfg, case["obs_faulty"], case["eph"], fix, n_rx))
    assert not (vel["used_mask"] & ~fix["used_mask"]).any() and not (vel["used_mask"] & fde["excl_mask"]).any()
    assert ((vel["flags"] == V.F_NO_FIX) == ((fix["flags"] & F.F_FIX) == 0)).all()
    clear = [r for r in case["fault_slot"] if D.min_margin(case["margins"][r]) >= D.MARGIN]
    assert len(clear) >= 3
    full = fix.copy()
    for r in clear:
        slot = case["fault_slot"][r]
        assert int(fde["excl_mask"][r]) == 1 << slot and int(vel["flags"][r]) == V.F_VEL and int(vel["n_used"][r]) == 11
        assert vel[r].tobytes() == got["obs_faulty"][2][r].tobytes()
        assert np.linalg.norm(vel["vel"][r] - np.array(K.VELOCITIES[1])) <= 0.05      # (the fix is metres off under 2 m of noise: millimetres per second)
        full["used_mask"][r] |= np.uint64(1 << slot)
    moved = V.run(vcfg, case["obs_faulty"], case["eph"], full, n_rx)
    assert all(np.linalg.norm(moved["vel"][r] - vel["vel"][r]) > 1.0 for r in clear)


def test_behind_the_device_stages_from_if_samples(eng):
    """weighted_pvt_cases' stream (four orbiting satellites, 25 000 blocks, MOVING gains; the receiver stands still, its clock is GPS
    time) through gpsx_track_loop_weighted_sync_dev, gpsx_wnav_words_dev, gpsx_wobs_dev, gpsx_weph_dev and gpsx_wlock_dev in
    weighted_pvt_cases.LAUNCHES, then gpsx_wfix_dev and gpsx_wvel_dev on the last launch's arrays where they lie on the device: VEL
    with all four slots, the restatement's record on the same arrays within the parity bound, and |vel| and |c drift| within 1.5 x
    what the CPU restatements of the whole chain give on this stream -- with GPSX_WVEL_L1CA 1.05 m/s, which is the bias of a scale that
    takes the loops' rest point fd (1 + 1/1022) for the Doppler, and with GPSX_WVEL_L1CA_WLOOP 0.07 m/s, the loops' frequency error
    (weighted_vel_cases.MEASURED says which is which).  With the lock records a slot needs CARRIER; the slots that have it give the same rows.  Cost: the stream's synthesis (about 25 s of CPU,
    cached per process in weighted_pvt_cases._memo) and its upload, plus a few seconds of GPU."""
    import weighted_pvt_cases as P
    from stm32f4_sdr_gps_amd import capi
    lib, n_ch = eng.lib, 4
    blocks = P.blocks()
    d_if = eng.malloc(blocks.nbytes)
    eng.h2d(d_if, blocks)
    st0 = dict(P.fresh_states(), sync=P.handover(), lock=np.zeros(n_ch, capi.WLOCK_STATE_DTYPE))
    chain = G.Chain(eng, P.sync_cfg_dev(P.MOVING), st0, max(P.LAUNCHES), P.MAX_BAD_WORDS, P.EDGE_GUARD, capi.wlock_cfg(25, 10, 1.5, 0.3, 1.0, 2, 2))
    bufs = dict(chain.buf, fix=G.Guarded(eng, F.FIX_DTYPE.itemsize), vel=G.Guarded(eng, V.VEL_DTYPE.itemsize))
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
        assert P.flags_ok(obs), obs["flags"]
        fcfg, vcfg = capi.wfix_cfg(P.OFFSETS_MS[0], 4), K.cfg(4)
        eng._chk(lib.gpsx_wfix_dev(eng.h, fcfg.ctypes.data, bufs["o"].ptr, bufs["e"].ptr, None, None, 1, bufs["fix"].ptr, None), "gpsx_wfix_dev")
        eng._chk(lib.gpsx_wvel_dev(eng.h, vcfg.ctypes.data, bufs["o"].ptr, bufs["e"].ptr, None, bufs["fix"].ptr, 1, bufs["vel"].ptr), "gpsx_wvel_dev")
        assert lib.gpsx_last_kernel(eng.h) == b"k_wvel"
        eng.synchronize()
        fix, vel = bufs["fix"].get(F.FIX_DTYPE, 1), bufs["vel"].get(V.VEL_DTYPE, 1)
        speed, cdrift = float(np.linalg.norm(vel["vel"][0])), float(vel["drift_s_s"][0]) * V.C_LIGHT
        print("Dopplers", obs["if_freq_offset_hz"], "age", obs["age_blocks"], "lock flags", lock["flags"], "vel", vel["vel"][0], "|vel|", speed, "c drift", cdrift,
              "enu", vel["enu"][0])
        assert int(fix["flags"][0]) == F.F_FIX and int(vel["flags"][0]) == V.F_VEL and int(vel["n_used"][0]) == 4 and int(vel["used_mask"][0]) == 15
        print("parity", K.compare(vel, V.run(vcfg, obs, eph, fix, 1), label="from IF samples, GPSX_WVEL_L1CA"))
        assert speed <= 1.5 * K.MEASURED["if_vel_mps"] and abs(cdrift) <= 1.5 * K.MEASURED["if_cdrift_mps"]
        # ... and with the scale that these loops' frequencies take (they rest at fd (1 + 1/1022)): what remains is their frequency error
        wcfg = K.cfg(4, mps_per_hz=V.L1CA_WLOOP)
        bufs["vel"].refill()
        eng._chk(lib.gpsx_wvel_dev(eng.h, wcfg.ctypes.data, bufs["o"].ptr, bufs["e"].ptr, None, bufs["fix"].ptr, 1, bufs["vel"].ptr), "gpsx_wvel_dev")
        eng.synchronize()
        rest = bufs["vel"].get(V.VEL_DTYPE, 1)
        speed_w, cdrift_w = float(np.linalg.norm(rest["vel"][0])), float(rest["drift_s_s"][0]) * V.C_LIGHT
        print("GPSX_WVEL_L1CA_WLOOP: vel", rest["vel"][0], "|vel|", speed_w, "c drift", cdrift_w, "enu", rest["enu"][0])
        K.compare(rest, V.run(wcfg, obs, eph, fix, 1), label="from IF samples, GPSX_WVEL_L1CA_WLOOP")
        assert int(rest["flags"][0]) == V.F_VEL and int(rest["used_mask"][0]) == 15
        assert speed_w <= 1.5 * K.MEASURED["if_wloop_vel_mps"] and abs(cdrift_w) <= 1.5 * K.MEASURED["if_wloop_cdrift_mps"]
        bufs["vel"].refill()
        eng._chk(lib.gpsx_wvel_dev(eng.h, vcfg.ctypes.data, bufs["o"].ptr, bufs["e"].ptr, bufs["l"].ptr, bufs["fix"].ptr, 1, bufs["vel"].ptr), "gpsx_wvel_dev")
        eng.synchronize()
        locked = bufs["vel"].get(V.VEL_DTYPE, 1)
        carrier = sum(1 << c for c in range(n_ch) if int(lock["flags"][c]) & capi.WLOCK_FLAG_CARRIER)
        assert int(locked["used_mask"][0]) == carrier and (carrier != 15 or locked.tobytes() == vel.tobytes())
    finally:
        for b in bufs.values():
            b.free()
        eng.free(d_if)
