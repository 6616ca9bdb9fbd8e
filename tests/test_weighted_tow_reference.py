"""The restatement of the time-of-week aiding (tests/weighted_tow_ref.py) held to the definition in include/gpsx.h (gpsx_wtow): the
layouts, one row per clause with its predicate (tests/weighted_tow_cases.py) under every pair of resolve and rearm, properties that hold
for any launch, the second call, the library's exports and binding, the smoke fixture, and the physics on weighted_pvt_cases' IF
stream.  No GPU."""
import itertools
import os
import re

import numpy as np
import pytest

import weighted_obs_ref as O
import weighted_pred_ref as P
import weighted_tow_cases as TC
import weighted_tow_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = list(itertools.product((0, 1), (0, 1)))      # (resolve, rearm)


def _header():
    with open(os.path.join(ROOT, "include", "gpsx.h")) as f:
        return f.read()


def test_layouts_are_the_headers_and_the_library_exports_both_entry_points():
    import __graft_entry__ as ge
    from stm32f4_sdr_gps_amd import capi
    assert capi.WTOW_CFG_DTYPE == T.CFG_DTYPE and capi.WTOW_DTYPE == T.TOW_DTYPE and capi.WTOW_RX_DTYPE == T.TOW_RX_DTYPE
    assert [T.CFG_DTYPE.fields[k][1] for k in T.CFG_DTYPE.names] == [0, 8, 12, 16, 20, 24, 28]
    assert [T.TOW_DTYPE.fields[k][1] for k in T.TOW_DTYPE.names] == [0, 4, 8, 16, 20, 24, 28]
    assert [T.TOW_RX_DTYPE.fields[k][1] for k in T.TOW_RX_DTYPE.names] == [0, 2, 3, 4, 5, 6, 7, 8, 16, 24, 32, 40, 48, 56]
    h = _header()
    for name, value in T.FLAG_NAMES.items():
        assert re.search(rf"#define GPSX_WTOW_{value}\s+{name}u\b", h), value
        assert getattr(capi, "WTOW_" + value) == name
    for name, value in (("NO_PRED", T.RX_NO_PRED), ("AIDED", T.RX_AIDED), ("SHIFTED", T.RX_SHIFTED), ("DISAGREES", T.RX_DISAGREES), ("OFF_GRID", T.RX_OFF_GRID),
                        ("REARMED", T.RX_REARMED)):
        assert re.search(rf"#define GPSX_WTOW_RX_{name}\s+{value}u\b", h), name
        assert getattr(capi, "WTOW_RX_" + name) == value
    for decl in ("int gpsx_wtow_dev(gpsx_ctx *ctx, const gpsx_wtow_cfg_t *cfg, int n_rx, int n_prn, const uint8_t *prns, const gpsx_wpred_rx_t *d_pred_rx,",
                 "int gpsx_wtow(gpsx_ctx *ctx, const gpsx_wtow_cfg_t *cfg, int n_rx, int n_prn, const uint8_t *prns, const gpsx_wpred_rx_t *d_pred_rx,",
                 "} gpsx_wtow_cfg_t;", "} gpsx_wtow_t;", "} gpsx_wtow_rx_t;", "THE EPOCHS ARE THE CALLER'S DUTY"):
        assert decl in h, decl
    assert re.search(r"#define GPSX_VERSION\s+110\b", h)        # no existing struct changed
    assert "gpsx_wtow" in ge.ABI_SYMBOLS and "gpsx_wtow_dev" in ge.ABI_SYMBOLS
    lib = capi.load_library()
    assert len(lib.gpsx_wtow.argtypes) == 12 and lib.gpsx_wtow_dev.argtypes == lib.gpsx_wtow.argtypes
    cfg = capi.wtow_cfg(12, 30.0, 8.0, 40, resolve=0, rearm=1)
    assert cfg.tobytes() == T.make_cfg(12, 30.0, 8.0, 40, 0, 1).tobytes() and callable(capi.Engine.wtow) and callable(capi.Engine.wtow_dev)


@pytest.fixture(scope="module")
def canonical():
    la = TC.launch(len(TC.ROWS))
    return la, {(pair, with_obs): TC.run(la, TC.cfg(resolve=pair[0], rearm=pair[1]), with_obs) for pair in PAIRS for with_obs in (True, False)}


@pytest.mark.parametrize("k", range(len(TC.ROWS)), ids=[r.name for r in TC.ROWS])
def test_one_row_per_clause(canonical, k):
    la, runs = canonical
    assert la.rows[k] is TC.ROWS[k]
    for (pair, with_obs), out in runs.items():
        o = TC.outcome(la, k, TC.cfg(resolve=pair[0], rearm=pair[1]), *out)
        assert TC.ROWS[k].check(o), (TC.ROWS[k].name, pair, with_obs, [T.names(f) for f in o.t["flags"]], o.t, o.rx)


def test_the_table_reaches_every_flag():
    la = TC.launch(len(TC.ROWS))
    seen = 0
    for pair in PAIRS:
        tow, tow_rx, *_ = TC.run(la, TC.cfg(resolve=pair[0], rearm=pair[1]))
        seen |= int(np.bitwise_or.reduce(tow["flags"]))
    assert seen == (1 << 14) - 1, T.names(~seen & ((1 << 14) - 1))


@pytest.mark.parametrize("shape", [(1, 1, 1), (9, 5, 4), (40, 33, 12), (5, 64, 64), (67, 31, 63)])
@pytest.mark.parametrize("pair", PAIRS)
def test_what_holds_for_any_launch(shape, pair):
    """said without the restatement's own steps: a state changes only under AIDED, or under AGREES with resolve from a state with
    AMBIGUOUS (SHIFTED comes with one of them or with DISAGREES), and then only in edge_block, tx_ms_at_edge, TOW and AMBIGUOUS; the
    counters and every other field stay; a sync state changes only under REARMED, in its three words; an observable changes only with
    its state, in tx_ms and flags, to the output clause of the new state; masks, counts and valid_after agree with records and states"""
    la = TC.launch(*shape, seed=3)
    c = TC.cfg(la.ch, *pair)
    tow, tow_rx, sync, states, obs = TC.run(la, c)
    need = O.F_PHASE | O.F_EDGE | O.F_TOW
    n_changed = 0
    for at in range(la.n_rx * la.ch):
        f = int(tow["flags"][at])
        b, a = la.states[at], states[at]
        if a.tobytes() != b.tobytes():
            n_changed += 1
            assert f & T.T_AIDED or (f & T.T_AGREES and pair[0] and int(b["flags"]) & O.F_AMBIGUOUS), T.names(f)
            w = b.copy()
            w["edge_block"], w["tx_ms_at_edge"], w["flags"] = a["edge_block"], a["tx_ms_at_edge"], a["flags"]
            assert w.tobytes() == a.tobytes() and (int(a["flags"]) ^ int(b["flags"])) & ~(O.F_TOW | O.F_AMBIGUOUS) == 0
            assert int(a["flags"]) & need == need and abs(int(a["edge_block"]) - int(b["edge_block"])) == abs(int(tow["shift"][at]))
            wo = la.obs[at].copy()
            wo["tx_ms"], wo["flags"] = (int(a["tx_ms_at_edge"]) + int(a["blocks_seen"]) - int(a["edge_block"])) % O.WEEK_MS, int(a["flags"]) | O.F_VALID
            assert obs[at].tobytes() == wo.tobytes()
        else:
            assert obs[at].tobytes() == la.obs[at].tobytes() and not f & T.T_AIDED
        if f & T.T_SHIFTED:
            assert f & (T.T_AIDED | T.T_AGREES | T.T_DISAGREES) and pair[0] and int(b["flags"]) & O.F_AMBIGUOUS and int(tow["shift"][at]) in (-1, 1)
        if sync[at].tobytes() != la.sync[at].tobytes():
            ws = la.sync[at].copy()
            ws["mode"], ws["search_n"], ws["prev_best_p1"] = 0, 0, 0
            assert f & T.T_REARMED and f & T.T_OFF_GRID and pair[1] and ws.tobytes() == sync[at].tobytes()
        assert bin(f & (T.T_NO_PRED | T.T_EMPTY | T.T_UNLISTED | T.T_BAD | T.T_WAITING | T.T_STALE | T.T_UNCERTAIN | T.T_INCONSISTENT | T.T_OFF_GRID | T.T_AIDED |
                        T.T_AGREES | T.T_DISAGREES)).count("1") == 1, T.names(f)
    for r in range(la.n_rx):
        x, fl = tow_rx[r], [int(v) for v in tow["flags"][r * la.ch:(r + 1) * la.ch]]
        if int(x["flags"]) & T.RX_NO_PRED:
            continue
        for name, bit in (("aided", T.T_AIDED), ("agrees", T.T_AGREES), ("disagrees", T.T_DISAGREES), ("off_grid", T.T_OFF_GRID), ("shifted", T.T_SHIFTED),
                          ("inconsistent", T.T_INCONSISTENT)):
            mask = sum(1 << j for j in range(la.ch) if fl[j] & bit)
            assert int(x[name + "_mask"]) == mask and int(x["n_" + name]) == bin(mask).count("1")
        va = sum(1 << j for j in range(la.ch) if not fl[j] & (T.T_EMPTY | T.T_UNLISTED | T.T_BAD) and int(states["flags"][r * la.ch + j]) & need == need)
        assert int(x["valid_after_mask"]) == va
    if la.rows.count(None) * la.ch >= 36:
        assert n_changed > 0 and tow_rx["n_agrees"].any() and tow_rx["n_off_grid"].any() and tow_rx["n_inconsistent"].any()       # the random receivers are of every kind
    # without the observables the records and the states are the same
    tow2, tow_rx2, sync2, states2, none = TC.run(la, c, with_obs=False)
    assert none is None and tow2.tobytes() == tow.tobytes() and tow_rx2.tobytes() == tow_rx.tobytes() and states2.tobytes() == states.tobytes()


@pytest.mark.parametrize("pair", PAIRS)
def test_a_second_call_on_the_result_agrees_everywhere_and_changes_nothing(pair):
    la = TC.launch(40, 33, 12, seed=4)
    c = TC.cfg(la.ch, *pair)
    tow, tow_rx, sync, states, obs = TC.run(la, c)
    la.sync, la.states, la.obs = sync, states, obs
    tow2, tow_rx2, sync2, states2, obs2 = TC.run(la, c)
    assert sync2.tobytes() == sync.tobytes() and states2.tobytes() == states.tobytes() and obs2.tobytes() == obs.tobytes()
    first, again = tow["flags"].astype(np.int64), tow2["flags"].astype(np.int64)
    was_aided = (first & T.T_AIDED) != 0
    assert was_aided.any() and ((again[was_aided] & ~T.T_SHIFTED) == T.T_AGREES).all()
    # (a shift that was written is not found again: the edge block has moved; a slot that was re-armed is OFF_GRID again, without REARMED: its mode is 0)
    same = ~was_aided & ((first & T.T_REARMED) == 0)
    moved = same & ((first & (T.T_SHIFTED | T.T_AGREES)) == (T.T_SHIFTED | T.T_AGREES))
    assert (again[same & ~moved] == first[same & ~moved]).all() and (again[moved] == T.T_AGREES).all() and (again[(first & T.T_REARMED) != 0] == T.T_OFF_GRID).all()
    assert (tow_rx2["valid_after_mask"] == tow_rx["valid_after_mask"]).all() and not tow_rx2["n_aided"].any()


def test_the_smoke_fixture_is_what_the_cases_write(tmp_path):
    path = os.path.join(ROOT, "tests", "golden", "wtow_smoke.npz")
    TC.write_smoke(str(tmp_path / "again.npz"))
    a, b = np.load(path), np.load(str(tmp_path / "again.npz"))
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k
    assert os.path.getsize(path) < 400 * 1024
    assert a["tow_rx"]["n_aided"].any() and a["tow_rx"]["n_shifted"].any() and (a["tow_rx"]["flags"] & T.RX_REARMED).any()


def test_physics_on_the_if_stream_the_prediction_names_the_millisecond():
    """weighted_pvt_cases' stream through the cached restatement chain (weighted_pred_cases.stream_on_restatements).  The last launch's
    records and words (blocks 24 576 .. 24 999) go into FRESH observable states: PHASE | EDGE on all four slots, no TOW, none VALID.
    gpsx_wpred's records at block 25 000 then give every slot the tx_ms of the undisturbed, HOW-anchored chain, the edge on the 20 ms
    grid, and the same pseudoranges.  Then three faults on the undisturbed end states: a lost anchor comes back as the HOW's own; an
    edge block moved by +-1 under AMBIGUOUS moves back; without AMBIGUOUS it is OFF_GRID and nothing is written.
    MEASURED (this test prints them, weighted_tow_cases.MEASURED keeps them): |rho| <= 0.0502 samples, sigma_m <= 5.03 m."""
    import weighted_acq_cases as AC
    import weighted_pred_cases as PC
    import weighted_pvt_cases as S
    s = PC.stream_on_restatements()
    first, n, rec, words, obs_und, _ = s["chain"][-1]
    assert (first, n) == (24576, 424)
    fresh = np.zeros(4, O.STATE_DTYPE)
    obs, bad = O.run(rec, n, words, fresh, TC.EDGE_GUARD)
    assert not bad and ((obs["flags"] & (O.F_PHASE | O.F_EDGE)) == (O.F_PHASE | O.F_EDGE)).all()
    assert not (obs["flags"] & (O.F_TOW | O.F_VALID)).any()                                     # before the call no slot is VALID
    print("fresh states: flags", [int(f) for f in fresh["flags"]], "age_blocks", [int(a) for a in obs["age_blocks"]])
    st, bank = s["at"][25000]
    sync = AC.empty_states(4)["sync"]
    sync["loop"]["prn"] = S.PRNS
    rx, pred = P.predict(PC.stream_cfg(0), PC.STREAM_PRNS, st, bank, sync)
    c = T.make_cfg(4, **TC.STREAM)
    tow, tow_rx = T.run(c, PC.STREAM_PRNS, rx, pred, sync, fresh, obs)
    sig = max(float(pred[0, PC.STREAM_PRNS.index(q)]["sigma_m"]) for q in S.PRNS)
    print("records", tow, "tx_ms", [int(v) for v in obs["tx_ms"]])
    print("MEASURED resid_samples", float(np.abs(tow["resid"]).max()), "sigma_m", sig)
    assert [T.names(f) for f in tow["flags"]] == ["AIDED"] * 4                                  # all four AIDED, none SHIFTED
    assert not (fresh["flags"] & O.F_AMBIGUOUS).any() and (tow["m"] == 0).all() and int(tow_rx["valid_after_mask"][0]) == 15
    assert (obs["flags"] & O.F_VALID).all() and obs["tx_ms"].tolist() == obs_und["tx_ms"].tolist()
    assert (obs_und["flags"] & O.F_VALID).all() and (obs_und["flags"] & O.F_CONFIRMED).any()    # (the undisturbed chain is HOW-anchored)
    for off in S.OFFSETS_MS:
        pa, ta, na = O.pseudoranges(obs, off)
        pu, tu, nu = O.pseudoranges(obs_und, off)
        assert na == nu == 4 and pa.tobytes() == pu.tobytes() and ta == tu
    assert float(np.abs(tow["resid"]).max()) <= TC.MEASURED["resid_samples"] * 1.0001 and sig <= TC.MEASURED["sigma_m"] * 1.0001
    # the faults, on the undisturbed end states
    end = s["end"]["obs"]
    assert ((end["flags"] & (O.F_TOW | O.F_PHASE | O.F_EDGE)) == (O.F_TOW | O.F_PHASE | O.F_EDGE)).all() and (end["blocks_seen"] == 25000).all()
    lost = end.copy()
    lost["flags"] &= ~np.uint32(O.F_TOW | O.F_CONFIRMED)
    lost["tx_ms_at_edge"] = 0
    tow, _ = T.run(c, PC.STREAM_PRNS, rx, pred, sync, lost, None)
    assert (tow["flags"] == T.T_AIDED).all() and lost["tx_ms_at_edge"].tolist() == end["tx_ms_at_edge"].tolist() and lost["edge_block"].tolist() == end["edge_block"].tolist()
    for move in (1, -1):
        for amb in (True, False):
            moved = end.copy()
            moved["edge_block"] += move
            moved["flags"] = (moved["flags"] & ~np.uint32(O.F_AMBIGUOUS)) | np.uint32(O.F_AMBIGUOUS if amb else 0)
            before = moved.copy()
            tow, _ = T.run(c, PC.STREAM_PRNS, rx, pred, sync, moved, None)
            if amb:
                assert (tow["flags"] == T.T_AGREES | T.T_SHIFTED).all() and (tow["shift"] == -move).all()
                assert moved["edge_block"].tolist() == end["edge_block"].tolist() and moved["tx_ms_at_edge"].tolist() == end["tx_ms_at_edge"].tolist()
                assert not (moved["flags"] & O.F_AMBIGUOUS).any()
            else:
                assert (tow["flags"] == T.T_OFF_GRID).all() and (tow["m"] == (1 if move > 0 else 19)).all() and moved.tobytes() == before.tobytes()
