"""The navigation filter's restatement (tests/weighted_kf_ref.py; include/gpsx.h gpsx_wkf) at the edges of its input space, on the CPU:
the sequences of tests/weighted_kf_edge_cases.py held to the truth model, so that the device's parity with the restatement
(tests/test_gpu_weighted_kf_edges.py) means something; the flag, row-count and time-base sequences each case is there for; a census, from
the inputs and the true geometry alone, of the branches the cases reach; every poke's end as the header's steps 0, 2, 9 and 12 say; and
every compared decision clear of round-off.  Figures are printed before anything is asserted; those that bound something are held to
1.5 x weighted_kf_edge_cases.MEASURED (the restatement against the truth, never against the device)."""
import numpy as np
import pytest

import pvt_chain as pc
import weighted_edge_cases as X
import weighted_kf_cases as C
import weighted_kf_edge_cases as XK
import weighted_kf_ref as K

W = K.WEEK_MS
UPD = K.F_UPDATED


def _held(name, value):
    print(f"MEASURED {name}: {value:.6g} (bound 1.5 x {XK.MEASURED[name]:.6g})")
    assert value <= 1.5 * XK.MEASURED[name], (name, value)


def _seq(case, r, field="flags"):
    return [int(w[field][r]) for w in case["want"]]


def _truth_errors(case, launches, v, drift_of):
    """the largest error of rr, vel, cdrift_mps and clk_m over the UPDATED records of `launches`, and the receiver it is at"""
    worst = dict(pos_m=(0.0, None), vel_mps=(0.0, None), cdrift_mps=(0.0, None), clk_m=(0.0, None))
    for k in launches:
        for r, name in enumerate(case["names"]):
            rec = case["want"][k][r]
            if not int(rec["flags"]) & UPD:
                continue
            t, rx = case["truth"][k][r]
            got = dict(pos_m=np.linalg.norm(rec["rr"] - rx), vel_mps=np.linalg.norm(rec["vel"] - np.asarray(v)),
                       cdrift_mps=abs(float(rec["cdrift_mps"]) - K.C_LIGHT * drift_of(name)), clk_m=abs(float(rec["clk_m"]) - C.truth_clk_m(rec, t)))
            for f, e in got.items():
                if e > worst[f][0]:
                    worst[f] = (float(e), f"{name} launch {k}")
    return worst


@pytest.mark.parametrize("which", ("edge", "steer"))
def test_the_restatement_holds_the_truth_along_every_track(which):
    """noise-free tracks: the filter's position, velocity, drift and clock term against the truth model's, over every update of the
    twelve-slot edge launches (21 receivers and four copies) and of the steering launches"""
    if which == "edge":
        case, drift_of = XK.edge_case(12, len(XK.NAMES)), (lambda name: X.DRIFT)
    else:
        case, drift_of = XK.steer_case(), (lambda name: XK.STEER[name][1])
    worst = _truth_errors(case, range(1, len(case["want"])), X.VELOCITY, drift_of)
    print(worst)
    for f, (e, _) in worst.items():
        _held(f"{which}_{f}", e)


def test_edge_sequences():
    """INIT and three updates for every receiver and shape; the satellites whose tk crosses +7201 s between launches 1 and 2 leave (the
    *_plus receivers and the copies 12 -> 8, near_plus 12 -> 11), far_plus never has its first, far_minus gains its first at launch 2;
    t_week_end ends in week + 1; the straddling receivers and the previous week's broadcast keep twelve rows"""
    for ch, n_rx in XK.SHAPES:
        case = XK.edge_case(ch, n_rx)
        n = min(ch, 12)
        lost4 = n - 4 if ch >= 12 else 4      # (the satellites of the first pick are the first four slots' in both)
        for r, name in enumerate(case["names"]):
            assert _seq(case, r) == [K.F_INIT, UPD, UPD, UPD], (ch, name, _seq(case, r))
            n_pr = _seq(case, r, "n_pr")
            assert n_pr == _seq(case, r, "n_dop")
            base = "munich_plus" if name in X.SHIFTS else name
            if base.endswith("_plus") and base not in ("near_plus", "far_plus"):
                assert n_pr == [0, n, lost4, lost4], (ch, name, n_pr)
            elif base == "near_plus":
                assert n_pr == [0, n, n - 1, n - 1], (ch, name, n_pr)
            elif base == "far_plus":
                assert n_pr == [0, n - 1, n - 1, n - 1], (ch, name, n_pr)
            elif base == "far_minus":
                assert n_pr == [0, n - 1, n, n], (ch, name, n_pr)
            else:
                assert n_pr == [0, n, n, n], (ch, name, n_pr)
            assert all(int(w["rej_pr_mask"][r]) == 0 and int(w["rej_dop_mask"][r]) == 0 for w in case["want"])
            week = _seq(case, r, "week")
            if name == "t_week_end":
                assert _seq(case, r, "rcv_ms") == [604798800, 604799300, 604799800, 300] and week == [pc.WEEK] * 3 + [pc.WEEK + 1]
            elif name.startswith("straddle"):      # (604 800.075 s: step 2's wrap)
                assert week == [pc.WEEK + 1] * 4 and _seq(case, r, "rcv_ms")[0] in (75, 78)
            else:
                assert week == [XK.week_of(name)] * 4, (name, week)
        assert case["codes"] == [0] * 4


def test_week_shifted_copies_equal_munich_plus_but_for_week():
    case = XK.edge_case(12, len(XK.NAMES))
    base = case["names"].index("munich_plus")
    for name, weeks in X.SHIFTS.items():
        r = case["names"].index(name)
        for w, s in zip(case["want"], case["states"]):
            rec, st = w[r:r + 1].copy(), s[r:r + 1].copy()
            assert int(rec["week"][0]) == int(w["week"][base]) + weeks and int(st["week"][0]) == int(s["week"][base]) + weeks
            rec["week"], st["week"] = w["week"][base], s["week"][base]
            assert rec.tobytes() == w[base:base + 1].tobytes() and st.tobytes() == s[base:base + 1].tobytes(), name


def test_steering_and_the_weeks_wraps():
    """STEERED once, in launch 3, in both directions across the week's end; COAST | STEERED for the receiver without a usable slot
    there; both wraps of the initialisation; every row accepted until tk crosses 7201 s (launch 5)"""
    case = XK.steer_case()
    wk = pc.WEEK
    r = {name: i for i, name in enumerate(case["names"])}
    S = K.F_STEERED
    for name in case["names"]:
        print(name, _seq(case, r[name]), _seq(case, r[name], "rcv_ms"), _seq(case, r[name], "week"), _seq(case, r[name], "n_pr"),
              [round(float(w["clk_m"][r[name]]) / K.MS, 4) for w in case["want"]])
    assert _seq(case, r["up"]) == [K.F_INIT, UPD, UPD, UPD | S, UPD, UPD, UPD]
    assert _seq(case, r["up"], "rcv_ms") == [604797000, 604798000, 604799000, 604799999, 999, 1999, 2999]
    assert _seq(case, r["up"], "week") == [wk, wk, wk, wk, wk + 1, wk + 1, wk + 1]
    assert _seq(case, r["down"]) == [K.F_INIT, UPD, UPD, UPD | S, UPD, UPD, UPD]
    assert _seq(case, r["down"], "rcv_ms") == [604796999, 604797999, 604798999, 0, 1000, 2000, 3000]
    assert _seq(case, r["down"], "week") == [wk, wk, wk, wk + 1, wk + 1, wk + 1, wk + 1]
    assert _seq(case, r["coast"]) == [K.F_INIT, UPD, UPD, K.F_COAST | S, UPD, UPD, UPD]
    assert _seq(case, r["coast"], "rcv_ms") == _seq(case, r["up"], "rcv_ms") and _seq(case, r["coast"], "week") == _seq(case, r["up"], "week")
    assert _seq(case, r["coast"], "n_starved") == [0, 0, 0, 1, 0, 0, 0]
    assert _seq(case, r["init_over"], "rcv_ms") == [0, 1000, 2000, 3000, 4000, 5000, 6000] and _seq(case, r["init_over"], "week") == [wk + 1] * 7
    assert _seq(case, r["init_under"], "rcv_ms") == [604799999, 999, 1999, 2999, 3999, 4999, 5999]
    assert _seq(case, r["init_under"], "week") == [wk] + [wk + 1] * 6
    for name in ("up", "down"):
        clk = [float(w["clk_m"][r[name]]) / K.MS for w in case["want"]]
        sign = 1.0 if name == "up" else -1.0
        assert 0.499 < sign * clk[2] < 0.5 and -0.5 < sign * clk[3] < -0.499, clk
        assert _seq(case, r[name], "n_pr") == [0, 12, 12, 12, 12, 8, 8]
    for i in range(len(case["names"])):
        assert all(int(w["rej_pr_mask"][i]) == 0 and int(w["rej_dop_mask"][i]) == 0 for w in case["want"])


def test_slot_edges():
    """every slot kind ends as weighted_kf_edge_cases.slot_case says, at every n_blocks and max_coast"""
    for n_blocks, max_coast, ion in XK.SLOT_CASES:
        case = XK.slot_case(n_blocks, max_coast, ion)
        for r, kind in enumerate(case["names"]):
            flags, n_pr, n_dop = _seq(case, r), _seq(case, r, "n_pr"), _seq(case, r, "n_dop")
            pr, dop = _seq(case, r, "pr_mask"), _seq(case, r, "dop_mask")
            what = (n_blocks, max_coast, r, kind, flags, n_pr, n_dop)
            if kind == "plain":
                assert flags == [K.F_INIT] + [UPD] * 4 and n_pr[1:] == [8] * 4 and n_dop[1:] == [8] * 4, what
            elif kind == "code_only":
                assert flags == [K.F_INIT] + [UPD] * 4 and n_pr[1:] == [8] * 4 and n_dop == [0] * 5 and dop == [0] * 5, what
            elif kind == "carrier_only" and max_coast == 2:
                assert flags == [K.F_INIT, UPD, UPD, K.F_LOST, K.F_INIT] and n_dop[1:3] == [8, 8] and n_pr == [0] * 5, what
                assert _seq(case, r, "n_starved") == [0, 1, 2, 0, 0] and [int(s["n_lost"][r]) for s in case["states"]] == [0, 0, 0, 1, 1]
                assert [int(s["n_init"][r]) for s in case["states"]] == [1, 1, 1, 1, 2]
            elif kind == "cut_all" and max_coast == 2:
                assert flags == [K.F_INIT, K.F_COAST, K.F_COAST, K.F_LOST, K.F_INIT] and _seq(case, r, "n_starved") == [0, 1, 2, 0, 0], what
            elif kind in ("carrier_only", "cut_all"):      # max_coast = 0
                assert flags == [K.F_INIT, K.F_LOST, K.F_INIT, K.F_LOST, K.F_INIT], what
            elif kind == "mixed":
                assert flags == [K.F_INIT] + [UPD] * 4 and pr[1:] == [0xd5] * 4 and dop[1:] == [0xe6] * 4, what
            elif kind == "freq_not_finite":
                assert flags == [K.F_INIT] + [UPD] * 4 and pr[1:] == [0xff] * 4 and dop[1:] == [0xff & ~(1 << XK.FREQ_INF | 1 << XK.FREQ_NAN)] * 4, what
                assert _seq(case, r, "rej_dop_mask") == [0] * 5
            elif kind in ("unhealthy", "a_zero"):
                gone = 0xff & ~(1 << (XK.SVH_SLOT if kind == "unhealthy" else XK.A_ZERO_SLOT))
                assert flags == [K.F_INIT] + [UPD] * 4 and pr[1:] == [gone] * 4 and dop[1:] == [gone] * 4, what
                assert _seq(case, r, "rej_pr_mask") == [0] * 5 and _seq(case, r, "rej_dop_mask") == [0] * 5
            elif kind == "a_small":      # a Doppler row without a pseudorange row: it is there (and gated out), the pseudorange row is not
                bit = 1 << XK.A_SMALL_SLOT
                assert flags == [K.F_INIT, UPD] + [UPD | K.F_REJECTED] * 3 and pr[1:] == [0xff & ~bit] * 4 and dop[1:] == [0xff & ~bit] * 4, what
                assert _seq(case, r, "rej_dop_mask") == [0, 0, bit, bit, bit] and _seq(case, r, "rej_pr_mask") == [0] * 5
                for d in case["details"][2:]:
                    assert d["drow"][r, XK.A_SMALL_SLOT] and not d["prow"][r, XK.A_SMALL_SLOT] and d["may_pr"][r, XK.A_SMALL_SLOT]
        assert case["codes"] == [0] * XK.SLOT_LAUNCHES


def test_the_ionosphere_coefficients_are_read():
    """the set of weighted_kf_edge_cases.ION against the default set (cfg.ion all zero): the same records, a solution 1.5 m away"""
    a, b = XK.slot_case(1000, 2, XK.ION), XK.slot_case(1000, 2, None)
    moved = np.linalg.norm(a["want"][-1]["rr"] - b["want"][-1]["rr"], axis=1)
    plain = [r for r, kind in enumerate(a["names"]) if kind == "plain"]
    print("moved by", moved[plain])
    assert (moved[plain] > 0.1).all() and (moved[plain] < 5.0).all()


def test_every_poke_ends_as_the_header_says():
    """step 0: every BAD variety is BAD, the call's code is EINVAL and the state stays as it is (after the repair the code is 0); steps 9
    and 12: a failed pivot with rows is LOST and without rows COAST, a non-finite result is LOST with or without rows, and LOST leaves
    n_init and n_lost + 1; step 2: a record that is not finite leaves NOT_INIT and writes nothing; the origin gates every row out"""
    case, clean = XK.poke_case(), XK.without_pokes(XK.poke_case())
    at = XK.POKE_AT
    assert case["codes"] == [0, 0, -22, 0] and clean["codes"] == [0] * 4
    poked = {XK.poke_index(i): name for i, name in enumerate(XK.POKED)}
    assert all(abs(a - b) > 1 for a in poked for b in poked if a != b) and min(poked) == 0 and max(poked) < case["n_rx"] - 1
    assert {r % 8 for r in poked} == {0, 3, 7}
    for r, name in poked.items():
        flags = _seq(case, r)
        print(name, r, flags)
        if name in XK.STATE_POKES:
            assert flags[:at] == [K.F_INIT, UPD] and flags[at] == XK.STATE_POKES[name][2], (name, flags)
        before, after = case["states"][at - 1][r:r + 1].copy(), case["states"][at][r:r + 1]
        if name.startswith("bad"):
            XK.STATE_POKES[name][0](before, 0)
            assert after.tobytes() == before.tobytes()
            rec = case["want"][at][r:r + 1].copy()
            rec["flags"] = 0
            assert rec.tobytes() == bytes(K.KF_DTYPE.itemsize)
            assert flags[at + 1] & UPD
        elif flags[at] == K.F_LOST:
            want = np.zeros(1, K.STATE_DTYPE)
            want["n_init"], want["n_lost"] = before["n_init"], before["n_lost"] + 1
            assert after.tobytes() == want.tobytes() and flags[at + 1] == K.F_INIT
        elif name == "coast_pivot":
            assert flags[at + 1] == K.F_LOST      # (the rows are back: the pivot fails)
        elif name.startswith("origin"):
            want_mask = 0xff if name == "origin_at_rest" else None
            rej = int(case["want"][at]["rej_pr_mask"][r])
            assert int(case["want"][at]["n_pr"][r]) == 0 and rej != 0 and (want_mask is None or rej == want_mask), (name, hex(rej))
        elif name == "vel_inf":
            assert flags == [K.F_NOT_INIT] * 4 and all(s[r:r + 1].tobytes() == bytes(384) for s in case["states"])
        else:
            assert flags == [K.F_NOT_INIT] * 3 + [K.F_INIT] and all(s[r:r + 1].tobytes() == bytes(384) for s in case["states"][:3])
    others = np.array([r not in poked for r in range(case["n_rx"])])
    for k in range(XK.POKE_LAUNCHES):
        assert case["want"][k][others].tobytes() == clean["want"][k][others].tobytes()
        assert case["states"][k][others].tobytes() == clean["states"][k][others].tobytes()
        assert (case["want"][k]["flags"][others] == (K.F_INIT if k == 0 else UPD)).all()


def test_a_repaired_slot_leaves_the_unshifted_state():
    case = XK.repair_case()
    assert _seq(case, 1, "plus_mask") == [0, 0, 1 << 3, 0] and _seq(case, 2, "minus_mask") == [0, 0, 1 << 5, 0]
    assert _seq(case, 1) == _seq(case, 2) == [K.F_INIT, UPD, UPD | K.F_REPAIRED, UPD] and _seq(case, 0) == [K.F_INIT, UPD, UPD, UPD]
    for st in case["states"]:
        assert st[0:1].tobytes() == st[1:2].tobytes() == st[2:3].tobytes()


def test_branch_census():
    """from the inputs and the true geometry alone (weighted_edge_cases.geometry), never from the filter: every branch below is
    reached by at least one receiver-slot of a launch that the GPU file compares"""
    g = {name: X.geometry(name) for name in XK.PHYSICAL}
    met = {}
    dt = XK.EDGE_BLOCKS * 1e-3
    tk = np.concatenate([g[n]["tk"][None, :] + dt * np.arange(XK.EDGE_LAUNCHES)[:, None] for n in XK.PHYSICAL])      # [launch, slot]
    inside, outside = tk[np.abs(tk) <= 7201.0], tk[np.abs(tk) > 7201.0]
    met["tk on both sides of +7201 s and of -7201 s over the launches"] = (float(inside.max()), float(inside.min()), float(outside.max()), float(outside.min()),
                                                                         inside.max() > 7200.5 and inside.min() < -7200.0 and outside.max() > 7201.0 and outside.min() < -7201.0)
    crossing = [n for n in XK.PHYSICAL if ((np.abs(g[n]["tk"]) <= 7201.0) & (np.abs(g[n]["tk"] + dt * (XK.EDGE_LAUNCHES - 1)) > 7201.0)).any()]
    entering = [n for n in XK.PHYSICAL if ((np.abs(g[n]["tk"]) > 7201.0) & (np.abs(g[n]["tk"] + dt * (XK.EDGE_LAUNCHES - 1)) <= 7201.0)).any()]
    met["a satellite leaves the span between two launches, and one enters it"] = (crossing, entering, len(crossing) >= 5 and entering == ["far_minus"])
    e = np.concatenate([g[n]["e"] for n in XK.PHYSICAL])
    met["e = 0 and e >= 0.3"] = (int((e == 0.0).sum()), float(e.max()), (e == 0.0).any() and e.max() >= 0.3)
    sva = np.concatenate([g[n]["sva"][:8] for n in XK.PHYSICAL])
    met["sva 0, 14 and 15 (the eight-slot launch's)"] = (np.bincount(sva.astype(int), minlength=16).tolist(), all((sva == v).any() for v in (0, 14, 15)))
    phi = np.concatenate([g[n]["phi_raw"] for n in XK.PHYSICAL])
    met["both Klobuchar clamps (semicircles beyond +- 0.416)"] = (float(phi.max()), float(phi.min()), phi.max() > 0.43 and phi.min() < -0.43)
    x = np.abs(np.concatenate([g[n]["x"] for n in XK.PHYSICAL]))
    met["Klobuchar's day and night arms (|x| against 1.57)"] = (float(x.min()), float(x.max()), x.min() < 1.5 and x.max() > 1.65)
    h = {n: X.SITES[n][2] for n in ("high", "deadsea")}
    met["both troposphere cut-offs (10 km, -100 m)"] = (h, h["high"] > 1e4 + 1e3 and h["deadsea"] < -100.0 - 100.0 and all(f"{n}_plus" in XK.PHYSICAL for n in h))
    lat = {n: X.SITES[n][0] for n in ("arctic", "pole")}
    met["the pole (89.9 S) and 84 N"] = (lat, lat["pole"] < -89.0 and lat["arctic"] > 80.0)
    f2, tgd = np.concatenate([X.receiver(n)["eph"]["f2"] for n in XK.PHYSICAL]), np.concatenate([X.receiver(n)["eph"]["tgd"] for n in XK.PHYSICAL])
    tc = np.concatenate([g[n]["toc_minus_toe"] for n in XK.PHYSICAL])
    met["f2, tgd and toc apart from toe"] = (float(np.abs(f2).max()), float(np.abs(tgd).max()), float(tc.min()),
                                             (f2 != 0).mean() > 0.5 and (tgd != 0).mean() > 0.5 and (tc != 0).mean() > 0.9)
    ms = np.concatenate([c["obs"][k]["tx_ms"].astype(np.int64) for c in (XK.edge_case(12, len(XK.NAMES)), XK.steer_case()) for k in range(len(c["obs"]))])
    ms = ms[ms != 0]
    met["transmit times on either side of the week's end"] = (int((ms > W - 100).sum()), int((ms < 100).sum()), (ms > W - 100).any() and (ms < 100).any())
    # the time base, from the records offered and the launches' lengths: step 2's m against 0 and W, step 1's sum against W
    arms = {"step 2 m >= W": [], "step 2 m < 0": [], "step 2 neither": [], "step 1 wraps": [], "step 1 does not": []}
    for case in (XK.edge_case(12, len(XK.NAMES)), XK.steer_case()):
        fix = case["fix"][0]
        m = np.rint(1000.0 * (fix["rx_tow_s"] - fix["dtr_s"])).astype(np.int64)
        for r, name in enumerate(case["names"]):
            arms["step 2 m >= W" if m[r] >= W else ("step 2 m < 0" if m[r] < 0 else "step 2 neither")].append(name)
            last = m[r] % W + case["n_blocks"] * (len(case["obs"]) - 1)
            arms["step 1 wraps" if last >= W - 1 else "step 1 does not"].append(name)
    met["every arm of step 1 and step 2"] = ({k: v[:4] for k, v in arms.items()}, all(arms.values()))
    st = XK.steer_case()
    steered = {name: [(int(w["flags"][r]) & K.F_STEERED) != 0 for w in st["want"]] for r, name in enumerate(st["names"])}
    wrap = {name: (int(st["want"][XK.STEER_AT - 1]["rcv_ms"][r]), int(st["want"][XK.STEER_AT]["rcv_ms"][r])) for r, name in enumerate(st["names"])}
    met["step 11: up with rcv_ms < 0, down with rcv_ms >= W (the restatement's records)"] = (
        wrap["up"], wrap["down"], steered["up"][XK.STEER_AT] and steered["down"][XK.STEER_AT] and wrap["up"] == (604799000, 604799999) and wrap["down"] == (604798999, 0))
    met["step 11: neither arm (init_over's b stays at +0.4 ms)"] = (steered["init_over"], not any(steered["init_over"]))
    for what, v in met.items():
        print("met" if v[-1] else "MISSED", "|", what, "|", *v[:-1])
    assert all(v[-1] for v in met.values()), [k for k, v in met.items() if not v[-1]]


CASES = {"edge 8": lambda: XK.edge_case(*XK.SHAPES[0]), "edge 12": lambda: XK.edge_case(*XK.SHAPES[1]), "edge 33": lambda: XK.edge_case(*XK.SHAPES[2]),
         "steer": XK.steer_case, "poke": XK.poke_case, "without pokes": lambda: XK.without_pokes(XK.poke_case()), "repair": XK.repair_case,
         "long": XK.long_case, **{f"slots {a[0]} {a[1]}": (lambda a=a: XK.slot_case(*a)) for a in XK.SLOT_CASES}}


@pytest.mark.parametrize("which", sorted(CASES))
def test_every_compared_decision_stands_clear_of_round_off(which):
    """every launch that tests/test_gpu_weighted_kf_edges.py compares with the restatement: the four margins of
    weighted_kf_cases.decisions_clear and the three of weighted_kf_edge_cases.decisions_clear"""
    print(which, XK.decisions_clear(CASES[which]()))


def test_the_long_run_only_updates():
    case = XK.long_case()
    assert all(_seq(case, r) == [K.F_INIT] + [UPD] * (XK.LONG_LAUNCHES - 1) and _seq(case, r, "n_pr")[1:] == [8] * (XK.LONG_LAUNCHES - 1) for r in range(3))
