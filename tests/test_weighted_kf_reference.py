"""The physics of the navigation filter's restatement (tests/weighted_kf_ref.py; include/gpsx.h gpsx_wkf), on the CPU: sequences of
launches built by tests/weighted_kf_cases.py.  Each test states a condition; the figures it measures are printed before anything is
asserted, and those that bound something are held to 1.5 x weighted_kf_cases.MEASURED."""
import numpy as np
import pytest

import weighted_fix_ref as F
import weighted_kf_cases as C
import weighted_kf_ref as K
import weighted_obs_ref as O

SEEDS = (0, 1, 2, 3, 4, 5)
N = 14      # INIT and 13 updates
CH = 8


def _held(name, value):
    print(f"MEASURED {name}: {value:.6g} (bound 1.5 x {C.MEASURED[name]:.6g})")
    assert value <= 1.5 * C.MEASURED[name], (name, value)


def _err(recs, eps):
    return np.array([np.linalg.norm(r["rr"] - e["rx"]) for r, e in zip(recs, eps)])


def _noisy(seed=0, drift=0.0, **kw):
    eps, eph = C.track("munich", CH, 0, C.VELOCITY, drift, N, noise_m=C.NOISE_M, noise_seed=seed, **kw)
    return eps, eph, C.first_fix(eps[0], eph, CH)


def _cut(obs, keep):
    """the launch's observables with only the slots of `keep` VALID"""
    obs = obs.copy()
    for s in range(len(obs)):
        if s not in keep:
            obs["flags"][s] &= ~np.uint32(O.F_VALID)
    return obs


def test_abi_of_the_restatement():
    assert K.tri(0, 0) == 0 and K.tri(0, 7) == 7 and K.tri(1, 1) == 8 and K.tri(7, 7) == 35 and K.tri(5, 2) == K.tri(2, 5)
    rng = np.random.default_rng(1)
    a = rng.normal(size=(3, 8, 8))
    spd = a @ a.transpose(0, 2, 1) + 8.0 * np.eye(8)
    packed = np.stack([spd[:, i, j] for i in range(8) for j in range(i, 8)], -1)
    ok, inv, shares = K.inverse(packed)
    assert ok.all() and (shares > 1e-3).all()
    assert np.abs(K.full(inv) @ spd - np.eye(8)).max() < 1e-12
    ok, _, _ = K.inverse(np.zeros((1, 36)))
    assert not ok[0]


def test_moving_receiver_beats_the_single_epoch_fix():
    """(30, -20, 5) m/s, eight satellites, 3 m of pseudorange noise, 1000-block launches, 13 after INIT: the filter's median 3-D error
    over the last half is below gpsx_wfix's on the same records, for every seed"""
    worst = 0.0
    for seed in SEEDS:
        eps, eph, fix0 = _noisy(seed)
        launches = [e["obs"] for e in eps]
        recs, _ = C.run_sequence(K.make_cfg(CH), launches, eph, [fix0] * N)
        assert [int(r["flags"]) for r in recs] == [K.F_INIT] + [K.F_UPDATED] * (N - 1)
        assert all(int(r["n_pr"]) == CH and int(r["n_dop"]) == CH for r in recs[1:])
        kf, fx = np.median(_err(recs, eps)[N // 2:]), np.median(_err(C.wfix_sequence(launches, eph, CH), eps)[N // 2:])
        print(f"seed {seed}: filter {kf:.3f} m, gpsx_wfix {fx:.3f} m")
        assert kf < fx, (seed, kf, fx)
        worst = max(worst, float(kf))
    _held("moving_median_m", worst)


def test_coasting_on_three_and_on_one_satellite():
    """the same track with the usable slots cut to three for four launches, then to one for two: UPDATED with n_pr 3 and 1 where
    gpsx_wfix says TOO_FEW; the error when the satellites return is bounded"""
    eps, eph, fix0 = _noisy(0)
    keep = {k: (0, 3, 6) for k in (5, 6, 7, 8)}
    keep.update({9: (3,), 10: (3,)})
    launches = [_cut(e["obs"], keep[k]) if k in keep else e["obs"] for k, e in enumerate(eps)]
    recs, _ = C.run_sequence(K.make_cfg(CH), launches, eph, [fix0] * N)
    fx = C.wfix_sequence(launches, eph, CH)
    for k, slots in keep.items():
        assert int(recs[k]["flags"]) == K.F_UPDATED and int(recs[k]["n_pr"]) == len(slots) and int(recs[k]["n_dop"]) == len(slots), (k, recs[k])
        assert int(recs[k]["pr_mask"]) == sum(1 << s for s in slots) and int(recs[k]["n_starved"]) == 0
        assert int(fx[k]["flags"]) == F.F_TOO_FEW
    err = _err(recs, eps)
    print("error through the outage:", np.round(err[4:13], 3))
    assert int(recs[11]["n_pr"]) == CH
    _held("coast_outage_m", float(err[5:11].max()))
    _held("coast_return_m", float(err[11]))


def test_starvation_ends_in_lost_and_a_new_init():
    """no usable slot for max_coast + 1 launches: COAST ... then LOST, NOT_INIT until a FIX record is offered, INIT again"""
    eps, eph, fix0 = _noisy(1)
    cfg = K.make_cfg(CH, max_coast=2)
    none = np.zeros(1, F.FIX_DTYPE)
    none["flags"] = F.F_TOO_FEW
    launches = [e["obs"] if k < 3 or k > 8 else _cut(e["obs"], ()) for k, e in enumerate(eps)]
    fix9 = C.first_fix(eps[9], eph, CH)
    fixes = [fix0, fix0, fix0, fix0, fix0, fix0, None, none, none, fix9, fix9, fix9, fix9, fix9]
    recs, st = C.run_sequence(cfg, launches, eph, fixes)
    flags = [int(r["flags"]) for r in recs]
    assert flags == [K.F_INIT, K.F_UPDATED, K.F_UPDATED, K.F_COAST, K.F_COAST, K.F_LOST, K.F_NOT_INIT, K.F_NOT_INIT, K.F_NOT_INIT, K.F_INIT] + \
        [K.F_UPDATED] * 4, flags
    assert [int(r["n_starved"]) for r in recs[3:5]] == [1, 2]
    lost = recs[5].copy()
    lost["flags"] = 0
    assert lost.tobytes() == bytes(K.KF_DTYPE.itemsize)
    assert int(st["n_init"][0]) == 2 and int(st["n_lost"][0]) == 1 and int(st["flags"][0]) == K.S_INIT
    assert _err(recs[10:], eps[10:]).max() < 30.0


def _shifted(eps, k, slot, ms, ambiguous=True):
    launches = [e["obs"].copy() for e in eps]
    launches[k]["tx_ms"][slot] -= ms      # (a transmit time 1 ms early: the pseudorange 1 ms long, k_j = +1)
    if ambiguous:
        launches[k]["flags"][slot] |= O.F_AMBIGUOUS
    return launches


def test_millisecond_repair():
    """an AMBIGUOUS slot 1 ms early or late lands in plus_mask / minus_mask and the state equals that of the run on the unshifted
    records (bit for bit: the slot is evaluated again at the corrected time); 3 ms off is rejected; a slot 1 ms off without the flag
    is gated out, not repaired"""
    eps, eph, fix0 = _noisy(2)
    cfg = K.make_cfg(CH)
    base, st0 = C.run_sequence(cfg, [e["obs"] for e in eps[:8]], eph, [fix0] * 8)
    for ms, field in ((1, "plus_mask"), (-1, "minus_mask")):
        recs, st = C.run_sequence(cfg, _shifted(eps[:8], 6, 4, ms), eph, [fix0] * 8)
        assert int(recs[6][field]) == 1 << 4 and int(recs[6]["flags"]) == K.F_UPDATED | K.F_REPAIRED and int(recs[6]["n_pr"]) == CH
        assert st["x"].tobytes() == st0["x"].tobytes() and st["P"].tobytes() == st0["P"].tobytes()
    recs, _ = C.run_sequence(cfg, _shifted(eps[:8], 6, 4, 3), eph, [fix0] * 8)
    assert int(recs[6]["rej_pr_mask"]) == 1 << 4 and int(recs[6]["plus_mask"]) == 0 and int(recs[6]["n_pr"]) == CH - 1
    assert int(recs[6]["flags"]) == K.F_UPDATED | K.F_REJECTED and int(recs[6]["n_dop"]) == CH
    recs, _ = C.run_sequence(cfg, _shifted(eps[:8], 6, 4, 1, ambiguous=False), eph, [fix0] * 8)
    assert int(recs[6]["rej_pr_mask"]) == 1 << 4 and int(recs[6]["plus_mask"]) == 0 and int(recs[6]["n_pr"]) == CH - 1
    assert np.linalg.norm(recs[6]["rr"] - base[6]["rr"]) < 5.0


def test_faulty_slot_is_gated_out():
    """a 150 m step on one slot after convergence appears in rej_pr_mask, and the position moves less than with the gate wide open"""
    import weighted_fix_cases as W
    eps, eph, fix0 = _noisy(3)
    launches = [e["obs"].copy() for e in eps[:10]]
    row = W.sky("munich", CH, 0)[2][1]
    dop = launches[8]["if_freq_offset_hz"][2]
    launches[8][2] = W.observable(row, eps[8]["rx"], eps[8]["t"], C.FAULT_M)[0]
    launches[8]["if_freq_offset_hz"][2] = dop
    clean, _ = C.run_sequence(K.make_cfg(CH), [e["obs"] for e in eps[:10]], eph, [fix0] * 10)
    gated, _ = C.run_sequence(K.make_cfg(CH), launches, eph, [fix0] * 10)
    open_, _ = C.run_sequence(K.make_cfg(CH, gate=100.0), launches, eph, [fix0] * 10)
    assert int(gated[8]["rej_pr_mask"]) == 1 << 2 and int(gated[8]["flags"]) == K.F_UPDATED | K.F_REJECTED and int(gated[8]["n_dop"]) == CH
    assert int(open_[8]["rej_pr_mask"]) == 0 and int(open_[8]["n_pr"]) == CH
    moved_gated, moved_open = np.linalg.norm(gated[8]["rr"] - clean[8]["rr"]), np.linalg.norm(open_[8]["rr"] - clean[8]["rr"])
    print(f"a 150 m fault moves the position by {moved_gated:.3f} m behind the gate, {moved_open:.3f} m with the gate open")
    assert moved_gated < moved_open
    _held("fault_gated_move_m", float(moved_gated))


def test_faulty_doppler_is_gated_out_alone():
    """a 50 Hz Doppler fault appears in rej_dop_mask; the slot's pseudorange row is still used"""
    eps, eph, fix0 = _noisy(4)
    launches = [e["obs"].copy() for e in eps[:10]]
    launches[8]["if_freq_offset_hz"][5] += np.float32(C.FAULT_HZ)
    recs, _ = C.run_sequence(K.make_cfg(CH), launches, eph, [fix0] * 10)
    assert int(recs[8]["rej_dop_mask"]) == 1 << 5 and int(recs[8]["rej_pr_mask"]) == 0
    assert int(recs[8]["n_pr"]) == CH and int(recs[8]["n_dop"]) == CH - 1 and (int(recs[8]["pr_mask"]) >> 5) & 1
    assert np.linalg.norm(recs[8]["vel"] - np.array(C.VELOCITY)) < 0.1


@pytest.mark.parametrize("drift", (1e-6, -1e-6))
def test_clock_drift_converges(drift):
    """drift +- 1e-6: cdrift_mps converges to +- 299.79 m/s, and clk_m follows the truth"""
    eps, eph, fix0 = _noisy(5, drift)
    recs, _ = C.run_sequence(K.make_cfg(CH), [e["obs"] for e in eps], eph, [fix0] * N)
    d_err = max(abs(float(r["cdrift_mps"]) - K.C_LIGHT * drift) for r in recs[N // 2:])
    b_err = max(abs(float(r["clk_m"]) - C.truth_clk_m(r, e["t"])) for r, e in zip(recs[N // 2:], eps[N // 2:]))
    print(f"drift {drift}: cdrift within {d_err:.5f} m/s, clk_m within {b_err:.3f} m over the last half")
    _held("cdrift_mps", d_err)
    _held("clk_m", b_err)


def test_clock_is_steered_once():
    """b starts at -0.4975 ms and falls by 299.79 m/s: it crosses -0.5 ms once; the launch is STEERED, rcv_ms moves by one, and the
    pseudoranges stay continuous (the next launches gate nothing out and the position holds)"""
    eps, eph, fix0 = _noisy(0, -1e-6, t0=C.W.TOW + 4.975e-4)
    recs, _ = C.run_sequence(K.make_cfg(CH), [e["obs"] for e in eps], eph, [fix0] * N)
    steered = [k for k, r in enumerate(recs) if int(r["flags"]) & K.F_STEERED]
    print("STEERED at", steered, "clk_m", [round(float(r["clk_m"]), 1) for r in recs])
    assert len(steered) == 1
    k = steered[0]
    assert int(recs[k]["rcv_ms"]) == int(recs[k - 1]["rcv_ms"]) + C.N_BLOCKS + 1 and float(recs[k]["clk_m"]) > 0.49 * K.MS
    assert int(recs[k + 1]["rcv_ms"]) == int(recs[k]["rcv_ms"]) + C.N_BLOCKS
    assert all(int(r["n_pr"]) == CH and int(r["rej_pr_mask"]) == 0 for r in recs[1:])
    assert all(abs(float(r["clk_m"]) - C.truth_clk_m(r, e["t"])) < 10.0 for r, e in zip(recs[3:], eps[3:]))
    assert _err(recs, eps)[N // 2:].max() < 15.0


def test_week_end():
    """a receiver crossing the week's end: rcv_ms wraps, week increments, no row is lost"""
    eps, eph = C.week_end_track()
    fix0 = C.first_fix(eps[0], eph, 12)
    week0 = int(fix0["week"][0])
    dets = []
    recs, _ = C.run_sequence(K.make_cfg(12), [e["obs"] for e in eps], eph, [fix0] * len(eps), n_blocks=500, details=dets)
    print("rcv_ms", [int(r["rcv_ms"]) for r in recs], "week", [int(r["week"]) for r in recs], "n_pr", [int(r["n_pr"]) for r in recs])
    assert [int(r["rcv_ms"]) for r in recs] == [604798800, 604799300, 604799800, 300, 800]
    assert [int(r["week"]) for r in recs] == [week0, week0, week0, week0 + 1, week0 + 1]
    assert all(int(r["n_pr"]) == 12 and int(r["n_dop"]) == 12 and int(r["flags"]) == K.F_UPDATED for r in recs[1:])
    err = _err(recs, eps)
    print("error", np.round(err, 3))
    _held("week_end_m", float(err[1:].max()))
    C.decisions_clear(dets)


def test_if_stream_on_the_restatements():
    """weighted_pvt_cases' IF stream (a receiver at rest) through the restatements of the whole chain, the filter called after every
    launch: NOT_INIT until gpsx_wfix has a FIX, INIT, then updates; the speed of the last record is what the GPU test's repeat is held
    to.  (The chain is weighted_pvt_cases' cached one: half a minute of CPU where no earlier test of the run made it.)"""
    got = C.if_stream_on_restatements()
    print(got)
    first = got["flags"].index(K.F_INIT)
    assert got["flags"][:first] == [K.F_NOT_INIT] * first and all(f & K.F_UPDATED for f in got["flags"][first + 1:]) and first < len(got["flags"]) - 1
    _held("if_speed_mps", got["speed_mps"])
    assert got["position_m"] < 100.0


@pytest.mark.parametrize("ch,n_rx", ((1, 17), (5, 67), (8, 67), (33, 17), (64, 67)))
def test_launch_cases_decisions_are_clear(ch, n_rx):
    """every compared decision of the GPU tests' launches stands clear of round-off, and every kind ends as its description says"""
    case = C.launch_case(ch, n_rx)
    print(C.decisions_clear(case["details"]))
    want, last = case["want"], case["want"][-1]
    for r, kind in enumerate(case["kinds"]):
        seq = [int(w["flags"][r]) & 63 for w in want]
        if kind == "fresh":
            assert seq == [K.F_NOT_INIT] * 3 + [K.F_INIT], (r, seq)
        elif kind == "starved":
            assert seq == [K.F_INIT, K.F_COAST, K.F_LOST, K.F_INIT], (r, seq)
        elif kind == "bad_state":
            assert seq == [K.F_INIT, K.F_UPDATED, K.F_UPDATED, K.F_BAD], (r, seq)
        elif kind == "coasting" and (r // len(C.KINDS)) % 3 == 2:
            assert seq == [K.F_INIT, K.F_UPDATED, K.F_UPDATED, K.F_COAST], (r, seq)
        else:
            assert seq == [K.F_INIT] + [K.F_UPDATED] * 3, (r, kind, seq)
        if kind == "ambiguous" and ch >= 4:
            sub = (r // len(C.KINDS)) % 3
            assert bool(last["plus_mask"][r]) == (sub == 0) and bool(last["minus_mask"][r]) == (sub == 1) and bool(last["rej_pr_mask"][r]) == (sub == 2)
        if kind == "faulty_doppler":
            assert last["rej_dop_mask"][r] != 0 and last["rej_pr_mask"][r] == 0
        if kind == "faulty_slot" and ch >= 4:
            assert last["rej_pr_mask"][r] != 0
    assert case["codes"] == [0, 0, 0, -22 if "bad_state" in case["kinds"] else 0]
