"""The navigation filter on the device (include/gpsx.h gpsx_wkf_dev, csrc/k_wkf.hip) at the edges of its input space, against its CPU
restatement (tests/weighted_kf_ref.py) on the launches of tests/weighted_kf_edge_cases.py: weighted_edge_cases' receivers carried forward
across the 7201 s limit, the week's end and the globe in three launch shapes; clocks steered in both directions across the week's end
and both wraps of the initialisation; lock records per slot, slots that give one row of the two, a set of ionosphere coefficients,
max_coast = 0 and launches of 1, 7 and 4096 blocks; every BAD, LOST and NOT_INIT variety with untouched neighbours on either side; and
three things only the device can show -- a launch with its receivers permuted gives the same bytes permuted, a repaired slot leaves the
unshifted state's bytes, and 31 updates in a row on a state that only the device carries.  tests/test_weighted_kf_edge_reference.py holds
the restatement to the truth on the same launches and asserts that every compared decision stands clear of round-off.  States and
records sit between 4096-byte canaries, the records start as 0xA5.

Parity, measured on one MI355X (profiles/r25_weighted_kf_edges_parity.json): see weighted_kf_edge_cases.PARITY_MEASURED_M / _MPS."""
import numpy as np
import pytest

import weighted_edge_cases as X
import weighted_gpu as G
import weighted_kf_cases as C
import weighted_kf_edge_cases as XK
import weighted_kf_ref as R
from weighted_gpu import eng  # noqa: F401

pytestmark = pytest.mark.gpu
REC = R.KF_DTYPE.itemsize
UPD = R.F_UPDATED


def _run(eng, case):
    """the case's launches through gpsx_wkf_dev on zeroed states in guarded device memory, its pokes and repairs applied to the device's
    own states -> ([records per launch], [states after each launch], [codes of gpsx_synchronize])"""
    cfg = C.cfg(case["ch"], **case["cfg_kw"])
    assert cfg.tobytes() == case["cfg"].tobytes()
    n_rx = case["n_rx"]
    recs, states, codes, before = [], [], [], None
    with G.Pool() as pool:
        def up(p, a):
            return None if a is None else p.add(G.Guarded(eng, a.nbytes, G.STATE_FILL, a)).ptr
        d_state = pool.add(G.Guarded(eng, n_rx * 384, G.STATE_FILL, np.zeros(n_rx, R.STATE_DTYPE)))
        d_eph, d_lock, d_vel = up(pool, case["eph"]), up(pool, case["lock"]), up(pool, case["vel"])
        for k in range(len(case["obs"])):
            if k in case["poke"] or k in case["repair"]:
                st = d_state.get(R.STATE_DTYPE, n_rx)
                before = XK.apply_pokes(case, k, st, before)
                d_state.put(st)
            with G.Pool() as launch:
                d_obs, d_fix = up(launch, np.ascontiguousarray(case["obs"][k])), up(launch, np.ascontiguousarray(case["fix"][k]))
                out = launch.add(G.Guarded(eng, n_rx * REC))
                rc = eng.lib.gpsx_wkf_dev(eng.h, cfg.ctypes.data, d_obs, d_eph, d_lock, d_fix, d_vel, n_rx, case["n_blocks"], d_state.ptr, out.ptr)
                assert rc == 0, (rc, eng.lib.gpsx_last_error(eng.h))
                codes.append(eng.lib.gpsx_synchronize(eng.h))
                assert eng.lib.gpsx_last_kernel(eng.h) == b"k_wkf"
                recs.append(out.get(R.KF_DTYPE, n_rx))
                states.append(d_state.get(R.STATE_DTYPE, n_rx))
    return recs, states, codes


def _against_the_restatement(eng, case, label, keep=None):
    """every launch's records and states against the restatement's, the measured maxima printed and recorded first"""
    recs, states, codes = _run(eng, case)
    for k in range(len(recs)):
        print("parity", label, k, XK.compare(recs[k], case["want"][k], f"{label} launch {k}"))
        XK.compare_states(states[k], case["states"][k], None if keep is None else keep[k])
    assert codes == case["codes"], codes
    return recs, states


def _seq(recs, r, field="flags"):
    return [int(w[field][r]) for w in recs]


@pytest.mark.parametrize("ch,n_rx", XK.SHAPES)
def test_edge_launches_equal_the_restatement(eng, ch, n_rx):
    """weighted_edge_cases' 21 receivers and four copies whole weeks away in four launches of 500 blocks, at 8 and 12 slots (eight and
    four receivers a wave) and at 33 (a wave each, dead upper lanes): satellites leave and enter the 7201 s span between launches, the
    week ends, e reaches 0.4, the sites both clamps and both cut-offs.  Records and states after every launch; the same case twice
    gives the same bytes; a copy whole weeks away is munich_plus byte for byte but for `week`"""
    case = XK.edge_case(ch, n_rx)
    recs, states = _against_the_restatement(eng, case, f"edges {ch} x {n_rx}")
    again, states2, _ = _run(eng, case)
    base = case["names"].index("munich_plus")
    for k in range(XK.EDGE_LAUNCHES):
        assert recs[k].tobytes() == again[k].tobytes() and states[k].tobytes() == states2[k].tobytes()
        for r, name in enumerate(case["names"]):
            if name in X.SHIFTS:
                rec, st = recs[k][r:r + 1].copy(), states[k][r:r + 1].copy()
                assert int(rec["week"][0]) == int(recs[k]["week"][base]) + X.SHIFTS[name] and int(st["week"][0]) == int(states[k]["week"][base]) + X.SHIFTS[name]
                rec["week"], st["week"] = recs[k]["week"][base], states[k]["week"][base]
                assert rec.tobytes() == recs[k][base:base + 1].tobytes() and st.tobytes() == states[k][base:base + 1].tobytes(), (k, name)
    if "t_week_end" in case["names"]:
        r = case["names"].index("t_week_end")
        assert _seq(recs, r, "rcv_ms") == [604798800, 604799300, 604799800, 300] and _seq(recs, r, "week")[3] == _seq(recs, r, "week")[0] + 1
    assert (np.concatenate([w["flags"] for w in recs[1:]]) == UPD).all()


def test_steering_and_the_weeks_wraps_equal_the_restatement(eng):
    """weighted_kf_edge_cases.steer_case: STEERED in both directions in the launch whose step 1 or step 11 crosses the week's end,
    COAST | STEERED without a usable slot, both wraps of the initialisation; integers exactly, the rest within the bound"""
    case = XK.steer_case()
    recs, _ = _against_the_restatement(eng, case, "steering")
    r = {name: i for i, name in enumerate(case["names"])}
    wk, at, S = int(recs[0]["week"][r["up"]]), XK.STEER_AT, R.F_STEERED
    assert _seq(recs, r["up"]) == [R.F_INIT, UPD, UPD, UPD | S, UPD, UPD, UPD] and _seq(recs, r["down"]) == _seq(recs, r["up"])
    assert _seq(recs, r["coast"])[at] == R.F_COAST | S
    assert (_seq(recs, r["up"], "rcv_ms")[at - 1:at + 2], _seq(recs, r["up"], "week")[at - 1:at + 2]) == ([604799000, 604799999, 999], [wk, wk, wk + 1])
    assert (_seq(recs, r["down"], "rcv_ms")[at - 1:at + 2], _seq(recs, r["down"], "week")[at - 1:at + 2]) == ([604798999, 0, 1000], [wk, wk + 1, wk + 1])
    assert float(recs[at]["clk_m"][r["up"]]) < -0.499 * R.MS and float(recs[at]["clk_m"][r["down"]]) > 0.499 * R.MS
    assert (int(recs[0]["rcv_ms"][r["init_over"]]), int(recs[0]["week"][r["init_over"]])) == (0, wk + 1)
    assert (int(recs[0]["rcv_ms"][r["init_under"]]), int(recs[0]["week"][r["init_under"]])) == (604799999, wk)


@pytest.mark.parametrize("n_blocks,max_coast,ion", XK.SLOT_CASES, ids=[f"{a[0]}-{a[1]}-{'ion' if a[2] else 'default'}" for a in XK.SLOT_CASES])
def test_slot_edges_equal_the_restatement(eng, n_blocks, max_coast, ion):
    """weighted_kf_edge_cases.slot_case at 1000 blocks with a set of ionosphere coefficients, at max_coast = 0, and at 1, 7 and 4096
    blocks (dt enters the prediction cubed): the masks exactly"""
    case = XK.slot_case(n_blocks, max_coast, ion)
    recs, states = _against_the_restatement(eng, case, f"slots {n_blocks} blocks max_coast {max_coast}" + (" ion" if ion else ""))
    for r, kind in enumerate(case["names"]):
        pr, dop = _seq(recs, r, "pr_mask")[1:], _seq(recs, r, "dop_mask")[1:]
        if kind == "code_only":
            assert pr == [0xff] * 4 and dop == [0] * 4
        elif kind == "mixed":
            assert pr == [0xd5] * 4 and dop == [0xe6] * 4
        elif kind == "freq_not_finite":
            assert pr == [0xff] * 4 and dop == [0xdb] * 4
        elif kind == "a_small":
            assert pr == [0xbf] * 4 and dop == [0xbf] * 4 and _seq(recs, r, "rej_dop_mask") == [0, 0, 0x40, 0x40, 0x40] and _seq(recs, r, "rej_pr_mask") == [0] * 5
        elif kind == "carrier_only" and max_coast == 2:
            assert _seq(recs, r) == [R.F_INIT, UPD, UPD, R.F_LOST, R.F_INIT] and _seq(recs, r, "n_starved") == [0, 1, 2, 0, 0] and dop[:2] == [0xff] * 2
            assert [int(s["n_lost"][r]) for s in states] == [0, 0, 0, 1, 1] and [int(s["n_init"][r]) for s in states] == [1, 1, 1, 1, 2]
        elif kind in ("carrier_only", "cut_all") and max_coast == 0:
            assert _seq(recs, r) == [R.F_INIT, R.F_LOST, R.F_INIT, R.F_LOST, R.F_INIT]


def test_state_pokes_equal_the_restatement_and_spare_the_neighbours(eng):
    """weighted_kf_edge_cases.poke_case: every BAD receiver keeps its state byte for byte and the call reports EINVAL; the next call, on
    repaired states, reports 0; LOST clears the state but for n_init and n_lost + 1; NOT_INIT writes nothing; and every other receiver
    -- one on either side of each poked one, at the first, the last and a middle place of a wave -- equals its run without pokes byte
    for byte"""
    case = XK.poke_case()
    at, n_rx = XK.POKE_AT, case["n_rx"]
    poked = {XK.poke_index(i): name for i, name in enumerate(XK.POKED)}
    bad = np.array([poked.get(r, "").startswith("bad") for r in range(n_rx)])
    keep = [None, None, ~bad, None]
    recs, states = _against_the_restatement(eng, case, "pokes", keep)
    clean = dict(case, poke={}, repair={})
    recs0, states0, codes0 = _run(eng, clean)
    assert codes0 == [0] * XK.POKE_LAUNCHES
    for r, name in poked.items():
        before, after = states[at - 1][r:r + 1].copy(), states[at][r:r + 1]
        if name.startswith("bad"):
            XK.STATE_POKES[name][0](before, 0)
            assert after.tobytes() == before.tobytes(), name
            assert int(recs[at]["flags"][r]) == R.F_BAD and int(recs[at + 1]["flags"][r]) & UPD
        elif name in XK.STATE_POKES and XK.STATE_POKES[name][2] == R.F_LOST:
            want = np.zeros(1, R.STATE_DTYPE)
            want["n_init"], want["n_lost"] = before["n_init"], before["n_lost"] + 1
            assert int(recs[at]["flags"][r]) == R.F_LOST and after.tobytes() == want.tobytes(), name
        elif name in XK.FIX_POKES:
            n = XK.POKE_LAUNCHES if name == "vel_inf" else XK.POKE_LAUNCHES - 1
            assert _seq(recs, r)[:n] == [R.F_NOT_INIT] * n and all(s[r:r + 1].tobytes() == bytes(384) for s in states[:n]), name
    assert int(recs[at]["rej_pr_mask"][[r for r, n in poked.items() if n == "origin_at_rest"][0]]) == 0xff
    others = ~np.array([r in poked for r in range(n_rx)])
    for k in range(XK.POKE_LAUNCHES):
        assert recs[k][others].tobytes() == recs0[k][others].tobytes() and states[k][others].tobytes() == states0[k][others].tobytes(), k


def _from_kf_case(ch, n_rx):
    """weighted_kf_cases.launch_case in weighted_kf_edge_cases' layout"""
    case = C.launch_case(ch, n_rx)
    n = len(case["obs"])
    return dict(cfg=case["cfg"], cfg_kw=dict(max_coast=C.MAX_COAST), ch=ch, n_rx=n_rx, n_blocks=case["n_blocks"], obs=list(case["obs"]), eph=case["eph"],
                lock=case["lock"], fix=list(case["fix"]), vel=case["vel"], repair={},
                poke={n - 1: [(r, XK.set_field(name, None, val)) for r, fields in case["poke"].items() for name, val in fields.items()]})


def _permuted(case, p):
    """receiver i of the new launches is receiver p[i] of the case's"""
    ch, n_rx, inv = case["ch"], case["n_rx"], np.argsort(p)
    rows = (lambda a: None if a is None else np.ascontiguousarray(a.reshape(n_rx, ch)[p]).reshape(-1))
    return dict(case, obs=[rows(o) for o in case["obs"]], eph=rows(case["eph"]), lock=rows(case["lock"]), fix=[np.ascontiguousarray(f[p]) for f in case["fix"]],
                vel=np.ascontiguousarray(case["vel"][p]), poke={k: [(int(inv[r]), fn) for r, fn in v] for k, v in case["poke"].items()})


@pytest.mark.parametrize("ch", XK.PERMUTED_CH)
def test_a_receiver_does_not_depend_on_its_place_in_the_launch(eng, ch):
    """weighted_kf_cases.launch_case(ch, 17) -- receivers of nine kinds, a BAD state among them -- reversed and shuffled: records and
    states are the unpermuted run's, permuted, byte for byte (group widths 1, 8 and 64: the lane offset of a group in its wave, the
    ballots' shift, the butterflies' width)"""
    case = _from_kf_case(ch, XK.PERMUTED_RX)
    recs, states, codes = _run(eng, case)
    for p in XK.permutations(XK.PERMUTED_RX):
        recs_p, states_p, codes_p = _run(eng, _permuted(case, p))
        assert codes_p == codes
        for k in range(len(recs)):
            assert recs_p[k].tobytes() == recs[k][p].tobytes() and states_p[k].tobytes() == states[k][p].tobytes(), (ch, k)


def test_a_repaired_slot_leaves_the_unshifted_states_bytes(eng):
    """weighted_kf_edge_cases.repair_case: one track three times in a launch, a slot a millisecond early in the second and one a
    millisecond late in the third, AMBIGUOUS: plus_mask / minus_mask name them and the three states are the same bytes after every
    launch, as the header's step 7 promises"""
    case = XK.repair_case()
    recs, states = _against_the_restatement(eng, case, "repair")
    assert _seq(recs, 1, "plus_mask") == [0, 0, 1 << 3, 0] and _seq(recs, 2, "minus_mask") == [0, 0, 1 << 5, 0]
    assert _seq(recs, 1) == _seq(recs, 2) == [R.F_INIT, UPD, UPD | R.F_REPAIRED, UPD]
    for k, st in enumerate(states):
        assert st[0:1].tobytes() == st[1:2].tobytes() == st[2:3].tobytes(), k
        a, b = recs[k][0:1].copy(), recs[k][1:2].copy()
        for rec in (a, b):
            rec["flags"], rec["plus_mask"] = 0, 0
        assert a.tobytes() == b.tobytes(), k


def test_thirty_one_updates_in_a_row(eng):
    """weighted_kf_edge_cases.long_case: 32 launches of three Munich receivers; the device carries its own state, the restatement its
    own, and every launch is held to the bound.  The per-launch maxima are printed and recorded, so a difference that grows with the
    launch index shows"""
    case = XK.long_case()
    recs, _, codes = _run(eng, case)
    series = []
    for k in range(XK.LONG_LAUNCHES):
        worst, n = XK.measure(recs[k], case["want"][k])
        XK.record_parity(f"long run launch {k:02d}", worst, n)
        series.append((max(worst[f] for f in ("rr_m", "clk_m", "height_m")), max(worst[f] for f in ("vel_mps", "enu_mps", "cdrift_mps"))))
    print("long run |device - restatement| per launch (m, m/s):", [(float(f"{a:.3g}"), float(f"{b:.3g}")) for a, b in series])
    for k in range(XK.LONG_LAUNCHES):
        XK.compare(recs[k], case["want"][k], None)
    assert codes == [0] * XK.LONG_LAUNCHES
