"""The CPU restatements of the three solver stages (tests/weighted_fix_ref.py, weighted_fde_ref.py, weighted_vel_ref.py) at the edges of
their input space (tests/weighted_edge_cases.py), held to what they can be held to without a GPU -- the library's pntpos on four
satellites, the true site, central differences of the truth, the injected velocity, the injected faults -- so that the device's
comparison with them (tests/test_gpu_weighted_edges.py) means something; a census, from the inputs and the true geometry alone, of
the branches that those launches reach; and every compared decision's distance from round-off."""
import ctypes as C
import time

import numpy as np
import pytest

import weighted_edge_cases as X
import weighted_fde_ref as D
import weighted_fix_cases as W
import weighted_fix_ref as F
import weighted_obs_ref as O
import weighted_vel_cases as K
import weighted_vel_ref as V

PHYSICAL = tuple(X.RECEIVERS)


@pytest.fixture(scope="module")
def lib():
    from stm32f4_sdr_gps_amd import capi
    return capi.load_library()


def test_every_pick_returns_within_a_second_and_the_module_builds_within_a_minute():
    """every (site, instant, toes, seed) that the module lists, timed on its own; then every launch, the FDE draws and the restatements'
    records of them, timed together (cached per process from here on)"""
    slowest = 0.0
    for name, (site, t, picks) in X.RECEIVERS.items():
        for toes, seed, _ in picks:
            t0 = time.perf_counter()
            got = X.pick(X.site_ecef(site), t, toes, 4, seed)
            slowest = max(slowest, time.perf_counter() - t0)
            assert got[0][1]["e"] == 0.0 and all(0.0 < row["e"] <= 0.4 for _, row in got[1:])
            assert all(row["toc"] <= row["toes"] and (row["toes"] - row["toc"]) % 16 == 0 and row["toes"] - row["toc"] <= 7200 for _, row in got)
    t0 = time.perf_counter()
    for ch, n_rx in X.SHAPES:
        X.want_fix(ch, n_rx), X.want_fix(ch, n_rx, True), X.want_vel(ch, n_rx)
    X.fde_kept()
    whole = time.perf_counter() - t0
    print("slowest pick", slowest, "s; launches, draws and restatements", whole, "s;", {k: round(v, 3) for k, v in X.BUILD_SECONDS.items() if k.startswith("launch")})
    assert slowest < 1.0 and whole < 60.0


def _gdop(rec, idx):
    rx = X.site_ecef(rec["site"])
    los = np.stack([X.sat_state(rec["rows"][k], np.array([rec["t"] - 0.07]))[0][0] - rx for k in idx])
    H = np.concatenate([-los / np.linalg.norm(los, axis=1, keepdims=True), np.ones((len(idx), 1))], 1)
    return float(np.sqrt(np.trace(np.linalg.inv(H.T @ H))))


def test_four_satellite_subsets_equal_pntpos(lib):
    """(a) the quartets (slots 0-3, 4-7, 8-11) of every solved physical receiver whose true GDOP is at most weighted_fix_cases.GDOP_MAX,
    from the origin and from 30 km off: rr within 1e-6 m, the clock term within 1e-14 s, qr within 1e-5 relative of the library's pntpos;
    pr_m and rx_tow_s bit for bit.  The kept quartets cover every site, tk within a second of either end, and tgd, f2 and toc - toe
    away from zero.  A quartet that the restatement refuses (from the origin, the
    first step can put a satellite below the horizon of where it landed) must be one that pntpos refuses too"""
    kept = []
    for name in PHYSICAL:
        if name in X.SOLVED:
            rec = X.receiver(name)
            for lo in (0, 4, 8):
                idx = list(range(lo, lo + 4))
                if name.startswith("far") and lo == 0:
                    continue      # (its first satellite gives no row: three left)
                if _gdop(rec, idx) <= W.GDOP_MAX:
                    kept.append((name, lo, rec["obs"][idx], rec["eph"][idx], X.geometry(name)["tk"][idx]))
    n = len(kept)
    obs, eph = W.pack([(o, e) for _, _, o, e, _ in kept], 4)
    cfg = F.make_cfg(X.OFFSET_MS, 4)
    cold, pr = F.run(cfg, obs, eph, n)
    warm, _ = F.run(cfg, obs, eph, n, prev=X.warm_start(cold))
    worst = {"rr_m": 0.0, "dtr_s": 0.0}
    for fix, start in ((cold, None), (warm, X.warm_start(cold)["rr"])):
        refused = np.flatnonzero(fix["flags"] != F.F_FIX)
        assert len(refused) <= 1 and (fix["flags"][refused] == F.F_TOO_FEW).all() and (fix["n_used"][fix["flags"] == F.F_FIX] == 4).all()
        for r, (name, lo, o, e, _) in enumerate(kept):
            want = W.pntpos_fix(lib, o, e, X.OFFSET_MS, None if start is None else start[r])
            if r in refused:      # (from the origin the first step can put a satellite below the horizon of where it landed: three rows)
                print(name, lo, "from", "the origin" if start is None else "30 km off", ": TOO_FEW after", int(fix["n_iter"][r]), "iterations, and pntpos finds no fix")
                assert want is None, (name, lo)
                continue
            assert want is not None, (name, lo)
            assert pr[4 * r:4 * r + 4].tobytes() == want["pr"].tobytes() and float(fix["rx_tow_s"][r]) == want["rx_tow_s"], (name, lo)
            worst["rr_m"] = max(worst["rr_m"], float(np.abs(fix["rr"][r] - want["rr"]).max()))
            worst["dtr_s"] = max(worst["dtr_s"], abs(float(fix["dtr_s"][r]) - want["dtr"]))
            assert float(np.abs(fix["rr"][r] - want["rr"]).max()) < 1e-6, (name, lo, fix["rr"][r] - want["rr"])
            assert abs(float(fix["dtr_s"][r]) - want["dtr"]) < 1e-14, (name, lo)
            assert np.allclose(fix["qr"][r], want["qr"], rtol=1e-5, atol=0.0), (name, lo)
    tks = np.concatenate([tk for *_, tk in kept])
    e = np.concatenate([e for _, _, _, e, _ in kept])
    print(n, "quartets kept;", worst, "; tk", tks.min(), "...", tks.max())
    assert {X.RECEIVERS[name][0] for name, *_ in kept} == set(X.SITES)
    assert tks.min() < -7199.0 and tks.max() > 7199.0
    assert (e["tgd"] != 0.0).mean() > 0.9 and (e["f2"] != 0.0).mean() > 0.9 and (e["toc_time"] != e["toe_time"]).mean() > 0.9


def _one(name, eph=None, obs=None, n=12):
    rec = X.receiver(name, n)
    fix, _ = F.run(F.make_cfg(X.OFFSET_MS, n), rec["obs"] if obs is None else obs, rec["eph"] if eph is None else eph, 1)
    return fix[0], rec


def test_every_solved_receiver_lies_at_its_true_site_and_the_check_has_teeth():
    """(b) noise-free, 8 and 12 satellites: every solved receiver within weighted_fix_cases.BOUNDS["noise_free_m"] of the truth, with
    the rows its inputs call for (one second past the 7201 s limit costs exactly the first slot).  Teeth: for one receiver each,
    negating tgd, zeroing f2, and reading toc as toe moves the restatement's fix by more than 10 x that receiver's own truth error"""
    largest = 0.0
    for ch, n_rx in X.SHAPES[:2]:
        case, (fix, _) = X.launch_case(ch, n_rx), X.want_fix(ch, n_rx)
        for r, name in enumerate(case["names"]):
            held = sum(1 << s for s in case["slots"][r])
            if name in X.SOLVED:
                err = float(np.linalg.norm(fix["rr"][r] - X.site_ecef(X._receiver(name)["site"])))
                largest = max(largest, err)
                assert int(fix["flags"][r]) == F.F_FIX and err <= W.BOUNDS["noise_free_m"], (name, err)
                want_mask = held & ~(1 << case["slots"][r][0]) if name.startswith("far") else held
                assert int(fix["used_mask"][r]) == want_mask and int(fix["n_used"][r]) == bin(want_mask).count("1"), name
            else:
                assert int(fix["flags"][r]) == F.F_TOO_FEW and int(fix["n_used"][r]) < 4, name
    print("largest distance from the true site", largest, "m (MEASURED", X.MEASURED["truth_m"], ")")
    assert largest <= 2.0 * X.MEASURED["truth_m"]
    for what, name in (("tgd negated", "munich_minus"), ("f2 zeroed", "arctic_plus"), ("toc read as toe", "pole_minus")):
        base, rec = _one(name)
        eph = rec["eph"].copy()
        if what == "tgd negated":
            eph["tgd"] = -eph["tgd"]
        elif what == "f2 zeroed":
            eph["f2"] = 0.0
        else:
            eph["toc_time"], eph["toc_sec"] = eph["toe_time"], eph["toe_sec"]
        moved, _ = _one(name, eph)
        err = float(np.linalg.norm(base["rr"] - X.site_ecef(rec["site"])))
        d = float(np.linalg.norm(moved["rr"] - base["rr"]))
        print(what, "at", name, ": truth error", err, "m, the fix moves by", d, "m")
        assert int(moved["flags"]) == F.F_FIX and d > 10.0 * err


def test_satellite_velocity_and_clock_rate_at_large_e_and_tk():
    """(c) weighted_vel_ref.satellites' velocity and clock rate against central differences (+- 0.5 s) of this module's truth at the
    restatement's own transmit time, over every satellite of every physical receiver (e to 0.4, |tk| to 7200.6 s, the week's end in
    between for three of them); the position against the truth's.  Bounds: 2 x weighted_edge_cases.MEASURED"""
    worst, h = {"pos_m": 0.0, "sat_vel_mps": 0.0, "sat_clock_rate": 0.0}, 0.5
    for name in PHYSICAL:
        rec = X.receiver(name)
        sat, ps, vs, rate, t = V.satellites(rec["eph"], rec["obs"], np.ones(12, bool))
        far = name.startswith("far")
        assert sat[1:].all() and bool(sat[0]) != far, name
        for j, row in enumerate(rec["rows"]):
            if far and j == 0:
                continue
            pos, dts = X.sat_state(row, np.array([t[j] - h, t[j], t[j] + h]))
            worst["pos_m"] = max(worst["pos_m"], float(np.abs(ps[j] - pos[1]).max()))
            worst["sat_vel_mps"] = max(worst["sat_vel_mps"], float(np.abs(vs[j] - (pos[2] - pos[0]) / (2 * h)).max()))
            worst["sat_clock_rate"] = max(worst["sat_clock_rate"], abs(float(rate[j]) - float(dts[2] - dts[0]) / (2 * h)))
    print(worst, "MEASURED", X.MEASURED)
    assert worst["pos_m"] <= 1e-6
    assert worst["sat_vel_mps"] <= 2.0 * X.MEASURED["sat_vel_mps"] and worst["sat_clock_rate"] <= 2.0 * X.MEASURED["sat_clock_rate"]


def test_injected_velocity_and_drift_are_recovered():
    """(c) every receiver moves at 36 m/s and drifts by 1e-6 s/s; on its true site's record the restatement recovers both within
    weighted_vel_cases' truth bounds (2 x MEASURED truth_vel_mps / truth_cdrift_mps: the terms of second order in 1 / c grow with the
    range rate, which an orbit of e = 0.4 carries to the size that 7.5 km/s receivers gave it there), the receivers at the week's end and on
    the previous week's broadcast with every slot"""
    ev, ed = 0.0, 0.0
    for ch, n_rx in X.SHAPES[:2]:
        case, vel = X.launch_case(ch, n_rx), X.want_vel(ch, n_rx)
        for r, name in enumerate(case["names"]):
            if name in X.SYNTHETIC:
                assert int(vel["flags"][r]) == V.F_NO_FIX
                continue
            assert int(vel["flags"][r]) == V.F_VEL and int(vel["n_used"][r]) == ch - name.startswith("far"), name
            ev = max(ev, float(np.linalg.norm(vel["vel"][r] - np.array(X.VELOCITY))))
            ed = max(ed, abs(float(vel["drift_s_s"][r]) - X.DRIFT) * V.C_LIGHT)
    print("largest velocity error", ev, "m/s, c drift error", ed, "m/s")
    assert ev <= 2.0 * K.MEASURED["truth_vel_mps"] and ed <= 2.0 * K.MEASURED["truth_cdrift_mps"]


def test_the_weights_follow_sva():
    """(d) twelve satellites with 30 m errors on exactly those whose sva is at least 10: the fix is nearer the truth than the same
    observables give with every sva set to 0"""
    name = next(n for n in PHYSICAL if n in X.SOLVED and not n.startswith("far") and 3 <= int((X.geometry(n)["sva"] >= 10).sum()) <= 6)
    bad = X.geometry(name)["sva"] >= 10
    rec = X.noisy(name, np.where(bad, 30.0, 0.0))
    site = X.site_ecef(rec["site"])
    weighted, _ = _one(name, obs=rec["obs"])
    flat_eph = rec["eph"].copy()
    flat_eph["sva"] = 0
    flat, _ = _one(name, eph=flat_eph, obs=rec["obs"])
    a, b = float(np.linalg.norm(weighted["rr"] - site)), float(np.linalg.norm(flat["rr"] - site))
    print(name, "sva", X.geometry(name)["sva"], ": error with the broadcast sva", a, "m, with every sva 0", b, "m")
    assert int(weighted["flags"]) == int(flat["flags"]) == F.F_FIX and a < b


def test_branch_census():
    """(e) from the inputs and the true geometry alone, never from a solver: every branch below is reached by at least one receiver-slot
    that the GPU file compares, with its margin"""
    g = {name: X.geometry(name) for name in PHYSICAL}
    solved = [n for n in PHYSICAL if n in X.SOLVED]
    met = {}
    tk = np.concatenate([g[n]["tk"] for n in solved if not n.startswith("far")] + [g[n]["tk"][1:] for n in solved if n.startswith("far")])
    met["tk within 1 s of +7200 / -7200"] = (float(tk.max()), float(tk.min()), tk.max() > 7199.0 and tk.min() < -7199.0 and np.abs(tk).max() < 7200.9)
    d = {n: X.RECEIVERS[n][2][0][0] - X.RECEIVERS[n][1] for n in ("near_plus", "far_plus", "near_minus", "far_minus")}      # toe - t of the first slot
    met["7201 s limit, both sides of both signs (0.5 s against 0.09 s)"] = (d, d == {"near_plus": -7200.5, "far_plus": -7201.5, "near_minus": 7200.5, "far_minus": 7201.5})
    e = np.concatenate([g[n]["e"] for n in solved])
    met["e = 0 and e > 0.3"] = (int((e == 0.0).sum()), float(e.max()), (e == 0.0).any() and e.max() > 0.3)
    spreads = {shape: X.wave_trip_spreads(*shape) for shape in X.SHAPES}
    met["Kepler trip counts >= 3 apart inside one wave of each launch"] = (spreads, all(max(s.values()) >= 3 for s in spreads.values()))
    sva = np.concatenate([g[n]["sva"][:8] for n in solved])      # (the eight-slot launch's)
    met["sva 0, 14 and 15"] = (np.bincount(sva.astype(int), minlength=16).tolist(), all((sva == v).any() for v in (0, 14, 15)))
    phi = np.concatenate([g[n]["phi_raw"] for n in solved])
    met["both Klobuchar clamps (semicircles beyond +- 0.416)"] = (float(phi.max()), float(phi.min()), phi.max() > 0.43 and phi.min() < -0.43)
    x = np.abs(np.concatenate([g[n]["x"] for n in solved]))
    met["Klobuchar's day and night arms (|x| against 1.57)"] = (float(x.min()), float(x.max()), x.min() < 1.5 and x.max() > 1.65)
    h = {n: X.SITES[n][2] for n in ("high", "deadsea")}
    met["both troposphere cut-offs (10 km, -100 m)"] = (h, h["high"] > 1e4 + 1e3 and h["deadsea"] < -100.0 - 100.0 and all(f"{n}_plus" in solved for n in h))
    ms = np.concatenate([X.receiver(n)["obs"]["tx_ms"].astype(np.int64) for n in ("straddle_a", "straddle_b") + X.SYNTHETIC])
    diffs = (ms[:, None] - ms[None, :]).ravel()
    met["int64 fold operands beyond +- half a week, negative ones included"] = (int(diffs.max()), int(diffs.min()), diffs.max() > 302_400_000 + 10**8 and diffs.min() < -302_400_000 - 10**8)
    dd = []
    for n in ("straddle_a", "straddle_b", "prev_week"):
        rec = X.receiver(n)
        t_sv = (rec["obs"]["tx_ms"] - rec["obs"]["code_phase_fine"].astype(np.float64) / 16368.0) / 1000.0
        dd += list(t_sv - rec["eph"]["toes"]) + list(t_sv - np.array([row["toc"] for row in rec["rows"]]))
    dd = np.array(dd)
    met["double fold operands beyond +- half a week"] = (float(dd.max()), float(dd.min()), dd.max() > 302400.0 + 1e5 and dd.min() < -302400.0 - 1e5)
    near_end = np.concatenate([X.receiver(n)["obs"]["tx_ms"] for n in ("straddle_a", "straddle_b")]).astype(np.int64)
    met["t_sv within 50 ms of either side of the week's end"] = (int((near_end > X.WEEK_MS - 50).sum()), int((near_end < 50).sum()),
                                                                 (near_end > X.WEEK_MS - 50).any() and (near_end < 50).any() and ((near_end > X.WEEK_MS - 50) | (near_end < 50)).all())
    met["tk = +5400 s through the fold (previous week's broadcast at 1800 s)"] = (float(g["prev_week"]["tk"].min()), bool(np.abs(g["prev_week"]["tk"] - 5400.0).max() < 1.0))
    tc = np.concatenate([g[n]["toc_minus_toe"] for n in solved])
    met["toc apart from toe"] = (float(tc.min()), float((tc != 0).mean()), (tc != 0).mean() > 0.9 and tc.min() <= -7000.0)
    for what, v in met.items():
        print("met" if v[-1] else "MISSED", "|", what, "|", *v[:-1])
    assert all(v[-1] for v in met.values()), [k for k, v in met.items() if not v[-1]]


def test_week_shifted_copies_give_the_same_bytes_but_for_week():
    """(f) records whose week, toe_time, toc_time and ttr_time are -522, -1, +1 and +500 whole weeks away: weighted_fix_ref's record
    differs in `week` alone, weighted_vel_ref's not at all"""
    ch, n_rx = X.SHAPES[1]
    case, (fix, _), vel = X.launch_case(ch, n_rx), X.want_fix(ch, n_rx), X.want_vel(ch, n_rx)
    at = {n: r for r, n in enumerate(case["names"])}
    base = fix[at["munich_plus"]].copy()
    for name, weeks in X.SHIFTS.items():
        got = fix[at[name]].copy()
        assert int(got["week"]) == int(base["week"]) + weeks
        got["week"] = base["week"]
        assert got.tobytes() == base.tobytes() and vel[at[name]].tobytes() == vel[at["munich_plus"]].tobytes(), name


def test_straddling_pseudoranges_are_the_librarys_bit_for_bit(lib):
    """(g) transmit milliseconds on both sides of 604 800 000, the first slot and the latest transmitter on either side in turn: the
    restatement's pr_m and rx_tow_s equal gpsx_wobs_pseudoranges bit for bit, and the latest transmitter is the reference"""
    lib.gpsx_wobs_pseudoranges.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.POINTER(C.c_double)]
    firsts = set()
    for name in ("straddle_a", "straddle_b") + X.SYNTHETIC:
        rec = X.receiver(name)
        obs = np.ascontiguousarray(rec["obs"], O.OBS_DTYPE)
        fix, pr = F.run(F.make_cfg(X.OFFSET_MS, 12), obs, rec["eph"], 1)
        want, rx = np.zeros(12), C.c_double(0.0)
        assert lib.gpsx_wobs_pseudoranges(obs.ctypes.data, 12, float(X.OFFSET_MS), want.ctypes.data, C.byref(rx)) == 12
        assert pr.tobytes() == want.tobytes() and float(fix["rx_tow_s"][0]) == rx.value, name
        tx = obs["tx_ms"].astype(np.int64)
        assert (tx < 50).any() and (tx > X.WEEK_MS - 101).any() and 0.0 < float(pr.min()) and float(pr.max()) < 0.2 * 299792458.0, name
        assert int(tx[int(fix["ref_slot"][0])]) < 50 and 0.0 <= rx.value < 0.2 and int(fix["flags"][0]) == F.F_TOO_FEW, name
        firsts.add(bool(tx[0] < 50))
    assert firsts == {True, False}


def test_fde_draws_at_the_edges_are_kept_with_their_margins():
    """(h) sixteen draws (a 300 m fault; a slot a millisecond off) at either tk extreme, both polar sites and the limit's near side: a
    draw is kept where every margin of weighted_fde_ref is at least its MARGIN and the restatement names the injected slot alone; at
    most one draw in eight is dropped"""
    draws = X.fde_draws()
    kept, (fix, fde, _, margins) = X.fde_kept()
    lo = min(D.min_margin(m) for m in margins)
    print(len(kept), "of", len(draws), "draws kept; smallest margin", lo, "; dropped", [(d["name"], d["kind"]) for d in draws if not any(d is k for k in kept)])
    assert len(draws) == 16 and 8 * (len(draws) - len(kept)) <= len(draws) and lo >= D.MARGIN
    assert {d["kind"] for d in kept} == {"fault", "ms"} and {d["site"] for d in kept} == {"munich", "arctic", "pole"}
    for r, d in enumerate(kept):
        assert X.fde_found(d, fde[r]) and int(fix["flags"][r]) == F.F_FIX, (d["name"], d["kind"])
        # 2 m of noise is below every row's modelled sigma (2.4 m at the least), so the fix's own covariance overstates its error
        assert float(np.linalg.norm(fix["rr"][r] - X.site_ecef(d["site"]))) < 3.0 * float(np.sqrt(fix["qr"][r, :3].sum())), (d["name"], d["kind"])


@pytest.mark.parametrize("ch,n_rx", X.SHAPES)
def test_every_compared_decision_stands_clear_of_round_off(ch, n_rx):
    """the launches of tests/test_gpu_weighted_edges.py: every solved receiver's pivot shares, cold and warm and in the velocity system,
    at least 1e-7 (1e3 x the rule's 1e-10); row counts depend on flags, masks and the 7201 s limit, which the cases miss by half a
    second; the warm start ends in the cold start's flags and masks"""
    lo_fix = min(X.fix_decisions_clear(ch, n_rx), X.fix_decisions_clear(ch, n_rx, True))
    case = X.launch_case(ch, n_rx)
    lo_vel, _ = K.decisions_clear(dict(cfg=case["vcfg"], obs=case["obs"], eph=case["eph"], fix=case["fix"], lock=None, want=X.want_vel(ch, n_rx),
                                       kinds=case["names"]), n_rx)
    (cold, _), (warm, _) = X.want_fix(ch, n_rx), X.want_fix(ch, n_rx, True)
    print(ch, n_rx, "smallest pivot share: fix", lo_fix, "vel", lo_vel, "; iterations cold", cold["n_iter"].max(), "warm", warm["n_iter"].max())
    assert (cold["flags"] == warm["flags"]).all() and (cold["used_mask"] == warm["used_mask"]).all()
    assert set(cold["flags"].tolist()) == {F.F_FIX, F.F_TOO_FEW}
