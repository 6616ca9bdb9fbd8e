"""The restatements of the ephemeris bank and of the prediction and hot hand-over (tests/weighted_pred_ref.py) held to the definitions in
include/gpsx.h (gpsx_wbank, gpsx_wpred): the layouts, one row per clause with its predicate (tests/weighted_pred_cases.py), properties
that hold for any launch, the prediction's closure with the filter's own rows, the clearance that makes the device comparison fair, the
physics on weighted_pvt_cases' IF stream, the library's exports and binding, and the smoke fixture.  No GPU."""
import os
import re

import numpy as np
import pytest

import weighted_kf_ref as R
import weighted_pred_cases as PC
import weighted_pred_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "gpsx.h")) as f:
        return f.read()


def test_layouts_are_the_headers():
    from stm32f4_sdr_gps_amd import capi
    assert capi.WBANK_CFG_DTYPE == P.BANK_CFG_DTYPE and capi.WBANK_DTYPE == P.BANK_DTYPE and capi.WEPH_DTYPE == P.EPH_DTYPE
    assert (capi.WEPH_FLAG_VALID, capi.WEPH_FLAG_NEW, capi.PRN_NONE) == (P.F_VALID, P.F_NEW, P.PRN_NONE)
    assert [P.BANK_DTYPE.fields[k][1] for k in ("stored_mask", "have_mask", "from_bank_mask", "n_stored", "n_have", "n_from_bank", "zero")] == [0, 8, 16, 24, 26, 28, 30]
    assert P.EPH_DTYPE.fields["flags"][1] == 0 and P.EPH_DTYPE.fields["toe_time"][1] == 32 and P.EPH_DTYPE.fields["ttr_time"][1] == 48
    h = _header()
    for decl in ("int gpsx_wbank_dev(gpsx_ctx *ctx, const gpsx_wbank_cfg_t *cfg, int n_rx, int n_prn, const uint8_t *prns,",
                 "int gpsx_wbank(gpsx_ctx *ctx, const gpsx_wbank_cfg_t *cfg, int n_rx, int n_prn, const uint8_t *prns,", "} gpsx_wbank_cfg_t;", "} gpsx_wbank_t;"):
        assert decl in h, decl
    assert re.search(r"#define GPSX_VERSION\s+110\b", h)        # no existing struct changed


def test_the_library_exports_both_entry_points_and_the_binding_has_them():
    import __graft_entry__ as ge
    from stm32f4_sdr_gps_amd import capi
    assert "gpsx_wbank" in ge.ABI_SYMBOLS and "gpsx_wbank_dev" in ge.ABI_SYMBOLS
    lib = capi.load_library()
    assert len(lib.gpsx_wbank.argtypes) == 10 and lib.gpsx_wbank_dev.argtypes == lib.gpsx_wbank.argtypes
    cfg = capi.wbank_cfg(12)
    assert cfg.dtype == capi.WBANK_CFG_DTYPE and int(cfg["ch_per_rx"][0]) == 12 and not cfg["reserved"].any()
    assert callable(capi.Engine.wbank)


@pytest.fixture(scope="module")
def canonical():
    la = PC.launch(len(PC.ROWS))
    return la, PC.run(la)


@pytest.mark.parametrize("k", range(len(PC.ROWS)), ids=[r.name for r in PC.ROWS])
def test_one_row_per_clause(canonical, k):
    la, (rep, out, bank, trace) = canonical
    assert la.rows[k] is PC.ROWS[k]
    assert PC.ROWS[k].check(PC.outcome(la, k, rep, out, bank, trace)), (PC.ROWS[k].name, trace[k], rep[k])


@pytest.mark.parametrize("shape", [(1, 1, 1), (9, 5, 4), (40, 33, 12), (5, 64, 64), (67, 31, 63)])
def test_what_holds_for_any_launch(shape):
    """said without the restatement's own steps: an entry changes only if reported stored, and then to a slot's VALID record on that PRN
    whose toe_time is not below the old entry's nor below any other offer's; a merged record differs from the launch's only where
    reported, and is then the bank's; masks, counts and bank agree; the launch's records and every unreported byte stay"""
    la = PC.launch(*shape, seed=3)
    rep, out, bank, trace = PC.run(la)
    prns = [int(q) for q in la.prns]
    n_from = 0
    for r in range(la.n_rx):
        o = PC.outcome(la, r, rep, out, bank, trace)
        stored, have, fb = int(o.rep["stored_mask"]), int(o.rep["have_mask"]), int(o.rep["from_bank_mask"])
        assert (bin(stored).count("1"), bin(have).count("1"), bin(fb).count("1"), 0) == tuple(int(o.rep[k]) for k in ("n_stored", "n_have", "n_from_bank", "zero"))
        assert have >> la.n_prn == 0 and fb >> la.ch == 0 and stored & ~have == 0
        for p in range(la.n_prn):
            offers = [j for j in range(la.ch) if int(la.slot_prns[r * la.ch + j]) == prns[p] and int(o.eph[j]["flags"]) & P.F_VALID]
            assert ((have >> p) & 1) == (int(o.bank_after[p]["flags"]) & P.F_VALID)
            if (stored >> p) & 1:
                src = [j for j in offers if o.bank_after[p].tobytes() == P.stored_form(o.eph[j]).tobytes()]
                assert src and int(o.bank_after[p]["flags"]) == P.F_VALID
                top = max(int(o.eph[j]["toe_time"]) for j in offers)
                assert int(o.bank_after[p]["toe_time"]) == top and src[0] == min(j for j in offers if int(o.eph[j]["toe_time"]) == top)
                assert not int(o.bank_before[p]["flags"]) & P.F_VALID or top >= int(o.bank_before[p]["toe_time"])
            else:
                assert o.bank_after[p].tobytes() == o.bank_before[p].tobytes()
                assert not offers or (int(o.bank_before[p]["flags"]) & P.F_VALID and max(int(o.eph[j]["toe_time"]) for j in offers) < int(o.bank_before[p]["toe_time"]))
        for j in range(la.ch):
            if (fb >> j) & 1:
                p = prns.index(int(la.slot_prns[r * la.ch + j]))
                assert not int(o.eph[j]["flags"]) & P.F_VALID and o.out[j].tobytes() == o.bank_after[p].tobytes() and int(o.out[j]["flags"]) & P.F_VALID
            else:
                assert o.out[j].tobytes() == o.eph[j].tobytes()
        n_from += bin(fb).count("1")
    if la.rows.count(None) * la.ch >= 36:
        assert n_from > 0 and rep["n_stored"].any() and (rep["n_stored"] < rep["n_have"]).any()       # the random receivers are of every kind
    # d_eph_out == d_eph: in place only the reported records change, so reading the launch's records before writing suffices
    changed = [c for c in range(la.n_rx * la.ch) if out[c].tobytes() != la.eph[c].tobytes()]
    assert all((int(rep["from_bank_mask"][c // la.ch]) >> (c % la.ch)) & 1 for c in changed)
    # without the merged copy the bank and the report are the same
    rep2, none, bank2, _ = PC.run(la, want_out=False)
    assert none is None and rep2.tobytes() == rep.tobytes() and bank2.tobytes() == bank.tobytes()


def test_a_second_call_on_the_same_records_refreshes_and_changes_nothing():
    la = PC.launch(40, 33, 12, seed=4)
    rep, out, bank, _ = PC.run(la)
    la2 = PC.launch(40, 33, 12, seed=4)
    la2.bank = bank
    rep2, out2, bank2, _ = PC.run(la2)
    assert bank2.tobytes() == bank.tobytes() and out2.tobytes() == out.tobytes()
    assert rep2["have_mask"].tobytes() == rep["have_mask"].tobytes() and rep2["from_bank_mask"].tobytes() == rep["from_bank_mask"].tobytes()
    assert ((rep2["stored_mask"] & ~rep["stored_mask"]) == 0).all()       # (equal toe: stored again; what was refused stays refused)


def test_a_lost_satellite_comes_back_with_its_ephemeris():
    """the reason the stage exists, in three calls: slot 1 decodes PRN 7; the slot is handed to PRN 19 and later PRN 7 returns in slot 3
    with a fresh, empty record: its merged record is the one decoded before"""
    rng = np.random.default_rng(7)
    prns, ch = [3, 7, 19], 4
    bank = P.empty_bank(1, 3)
    eph = np.zeros(ch, P.EPH_DTYPE)
    eph[1] = PC.record(rng, PC.VN, 7200, 100)
    slots = np.array([P.PRN_NONE, 7, P.PRN_NONE, P.PRN_NONE], np.int32)
    rep, out = P.bank(ch, prns, slots, eph, bank)
    assert int(rep["stored_mask"][0]) == 2 and out.tobytes() == eph.tobytes()
    decoded = bank[0, 1].copy()
    slots[1], eph[1] = 19, np.zeros(1, P.EPH_DTYPE)[0]
    rep, out = P.bank(ch, prns, slots, eph, bank)
    assert int(rep["stored_mask"][0]) == 0 and int(rep["have_mask"][0]) == 2 and int(rep["from_bank_mask"][0]) == 0
    slots[3] = 7
    rep, out = P.bank(ch, prns, slots, eph, bank)
    assert int(rep["from_bank_mask"][0]) == 8 and out[3].tobytes() == decoded.tobytes() and int(out[3]["flags"]) == P.F_VALID
    assert not int(eph[3]["flags"]) and bank[0, 1].tobytes() == decoded.tobytes()


def test_the_smoke_fixture_is_what_the_cases_write(tmp_path):
    path = os.path.join(ROOT, "tests", "golden", "wpred_smoke.npz")
    PC.write_smoke(str(tmp_path / "again.npz"))
    a, b = np.load(path), np.load(str(tmp_path / "again.npz"))
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        if k == "p_pred":      # (behind a sine: another machine's libm may differ in the last bits; the decisions and the handed floats may not)
            for f in a[k].dtype.names:
                if a[k][f].dtype.kind == "f":
                    assert np.allclose(a[k][f], b[k][f], rtol=1e-9, atol=1e-7), f
                else:
                    assert a[k][f].tobytes() == b[k][f].tobytes(), f
        else:
            assert a[k].tobytes() == b[k].tobytes(), k
    assert os.path.getsize(path) < (1 << 20)
    assert a["rep"]["n_stored"].any() and a["rep"]["n_from_bank"].any() and a["p_rx"]["n_assigned"].any() and a["p_rx"]["n_evicted"].any()


# ==== gpsx_wpred ===============================================================================================================================
def test_prediction_layouts_are_the_headers():
    from stm32f4_sdr_gps_amd import capi
    assert capi.WPRED_CFG_DTYPE == P.PRED_CFG_DTYPE and capi.WPRED_DTYPE == P.PRED_DTYPE and capi.WPRED_RX_DTYPE == P.PRED_RX_DTYPE
    assert (capi.WPRED_HAVE_EPH, capi.WPRED_PREDICTED, capi.WPRED_VISIBLE, capi.WPRED_CERTAIN, capi.WPRED_TRACKED, capi.WPRED_ASSIGNED, capi.WPRED_DROPPED) == \
        (P.P_HAVE_EPH, P.P_PREDICTED, P.P_VISIBLE, P.P_CERTAIN, P.P_TRACKED, P.P_ASSIGNED, P.P_DROPPED)
    assert (capi.WPRED_RX_PREDICTED, capi.WPRED_RX_NOT_INIT, capi.WPRED_RX_BAD, capi.WPRED_RX_ASSIGNED, capi.WPRED_RX_EVICTED, capi.WPRED_RX_FULL) == \
        (P.RX_PREDICTED, P.RX_NOT_INIT, P.RX_BAD, P.RX_ASSIGNED, P.RX_EVICTED, P.RX_FULL)
    h = _header()
    for name, value in (("HAVE_EPH", 1), ("PREDICTED", 2), ("VISIBLE", 4), ("CERTAIN", 8), ("TRACKED", 16), ("ASSIGNED", 32), ("DROPPED", 64), ("RX_PREDICTED", 1),
                        ("RX_NOT_INIT", 2), ("RX_BAD", 4), ("RX_ASSIGNED", 8), ("RX_EVICTED", 16), ("RX_FULL", 32)):
        assert re.search(rf"#define GPSX_WPRED_{name}\s+{value}u\b", h), name
    for decl in ("int gpsx_wpred_dev(gpsx_ctx *ctx, const gpsx_wpred_cfg_t *cfg, int n_rx, int n_prn, const uint8_t *prns, const gpsx_wkf_state_t *d_kf_state,",
                 "int gpsx_wpred(gpsx_ctx *ctx, const gpsx_wpred_cfg_t *cfg, int n_rx, int n_prn, const uint8_t *prns, const gpsx_wkf_state_t *d_kf_state,",
                 "} gpsx_wpred_cfg_t;", "} gpsx_wpred_t;", "} gpsx_wpred_rx_t;"):
        assert decl in h, decl
    import __graft_entry__ as ge
    assert "gpsx_wpred" in ge.ABI_SYMBOLS and "gpsx_wpred_dev" in ge.ABI_SYMBOLS
    lib = capi.load_library()
    assert len(lib.gpsx_wpred.argtypes) == 14 and lib.gpsx_wpred_dev.argtypes == lib.gpsx_wpred.argtypes
    cfg = capi.wpred_cfg(12, capi.WVEL_L1CA_WLOOP, lead_blocks=80)
    assert cfg.tobytes() == P.pred_cfg(12, capi.WVEL_L1CA_WLOOP, lead_blocks=80).tobytes() and callable(capi.Engine.wpred)


@pytest.fixture(scope="module")
def pred_canonical():
    la = PC.pred_launch(len(PC.PRED_ROWS))
    cfg = PC.pred_cfg()
    return la, cfg, PC.pred_run(la, cfg)


@pytest.mark.parametrize("k", range(len(PC.PRED_ROWS)), ids=[r.name for r in PC.PRED_ROWS])
def test_one_prediction_row_per_clause(pred_canonical, k):
    la, cfg, (rx, pred, after, trace) = pred_canonical
    assert la.rows[k] is PC.PRED_ROWS[k]
    assert PC.PRED_ROWS[k].check(PC.pred_outcome(la, k, rx, pred, after, trace)), (PC.PRED_ROWS[k].name, rx[k], pred[k])


def test_closure_the_prediction_is_the_observable_the_filter_expects(pred_canonical):
    """|v| < 1e-6 m and |y - a . x^_v| < 1e-9 m/s for every PREDICTED (receiver, PRN) of the table: the three-pass bound leaves 1e-9 m, the
    round-off of a 2e7 m range in doubles 4e-9 m (and of pr = ms (q + phase / 16368), where the phase is formed from a difference of
    7e4-sized milliseconds: 1e-7 m)"""
    la, cfg, (rx, pred, after, trace) = pred_canonical
    v, y, n = PC.closure(la, cfg, rx, pred, trace)
    print("closure over", n, "predictions: |v| <=", v, "m, |y| <=", y, "m/s")
    assert n >= 100 and v < 1e-6 and y < 1e-9
    # ... and the three passes do what the header's derivation says: the second moves the range by metres, the third by less than 1e-4 m
    for t in trace:
        if t["kind"] == "run" and t["predicted"].any():
            on = t["predicted"]
            p1, p2, p3 = (t["passes"][k]["pr"][on] for k in range(3))
            assert np.abs(p2 - p1).max() < 40.0 and np.abs(p3 - p2).max() < 1e-4


@pytest.mark.parametrize("handover", (0, 1))
def test_with_handover_0_nothing_is_written_and_the_predictions_are_the_same(pred_canonical, handover):
    la, cfg1, want1 = pred_canonical
    cfg = PC.pred_cfg(handover=handover)
    rx, pred, after, trace = PC.pred_run(la, cfg)
    for f in ("tx_ms", "pr_m", "code_phase", "f_hz", "el", "az", "sigma_m", "sigma_hz"):
        assert pred[f].tobytes() == want1[1][f].tobytes(), f
    if handover == 0:
        assert all(after[k].tobytes() == la.states[k].tobytes() for k in after)
        assert not (pred["flags"] & (P.P_ASSIGNED | P.P_DROPPED)).any() and not rx["assigned_mask"].any() and not rx["n_dropped"].any()
        assert (rx["evicted_mask"] == want1[0]["evicted_mask"]).all() and rx["evicted_mask"].any()
    rx2, pred2, after2, _ = PC.pred_run(la, cfg, nulls=("nav", "obs", "eph"), want_pred=False)
    assert pred2 is None and rx2.tobytes() == rx.tobytes() and after2["sync"].tobytes() == after["sync"].tobytes() and after2["nav"] is None


def test_every_compared_decision_stands_clear_of_the_parity_bound():
    """weighted_pred_cases.decisions_clear on every launch that tests/test_gpu_weighted_pred.py compares byte for byte: 1e3 x the parity
    bound from every threshold and float rounding boundary; a receiver that does not is re-seeded (pred_launch), not tolerated"""
    assert PC.PARITY_MEASURED_M is not None and PC.PARITY_MEASURED_MPS is not None, "the parity bound has not been measured: under the cap no handed float can stand clear"
    worst = 0
    for n_rx, n_prn, ch, handover, evict in [(len(PC.PRED_ROWS), PC.P_N_PRN, PC.P_CH, 1, None), (3, 31, 4, 1, None), (5, 63, 64, 1, None), (67, 64, 12, 1, None),
                                             (21, 12, 64, 1, 0), (len(PC.PRED_ROWS) + 5, 12, 7, 1, None)]:
        la = PC.pred_launch(n_rx, n_prn, ch)
        cfg = PC.pred_cfg(ch, handover, **({} if evict is None else dict(evict_after_blocks=evict)))
        rx, pred, after, trace = PC.pred_run(la, cfg)
        assert PC.decisions_clear(la, cfg, pred, trace) == [], (n_rx, n_prn, ch)
        worst = max(worst, max(la.reseeded))
    print("re-seeding steps, at most", worst, "of", PC.RESEED_TRIES)
    assert worst < PC.RESEED_TRIES


def test_physics_on_the_if_stream_prediction_and_hot_re_acquisition():
    """weighted_pvt_cases' stream (four orbiting satellites, 25 000 blocks) through the cached restatement chain with MOVING gains, the bank
    and the filter behind every launch.  The filter is INIT at block 24 576 and UPDATED at 25 000.  At both blocks the predicted transmit
    time at sample 0 and f_hz of the four PRNs are within weighted_loop_cases.HANDOVER -- 3 samples and 12.5 Hz, the hand-over error from
    which the loops are shown to pull in -- of the synthesiser's own truth.  At 24 576 slot 2 is emptied and gpsx_wpred hands PRN 4 back to
    it; weighted_sync_ref runs the last 424 blocks on that state: its final phase and frequency against the undisturbed channel's are
    MEASURED's repull figures, and its merged ephemeris record at 25 000 is the bank's, byte for byte, while its own is not VALID."""
    import weighted_acq_cases as AC
    import weighted_eph_ref as E
    import weighted_loop_cases as LC
    import weighted_pvt_cases as S
    s = PC.stream_on_restatements()
    assert s["flags"][-2] == R.F_INIT and s["flags"][-1] & R.F_UPDATED, s["flags"]
    worst_phase = worst_freq = 0.0
    for block in (24576, 25000):
        st, bank = s["at"][block]
        rx, pred = P.predict(PC.stream_cfg(0), PC.STREAM_PRNS, st, bank, AC.empty_states(4)["sync"])
        d_phase, d_freq, at = PC.prediction_errors(pred[0], rx["t_ms"][0])
        print("block", block, "phase errors (samples)", d_phase, "frequency errors (Hz)", d_freq, "elevations", pred[0]["el"], "sigmas", pred[0]["sigma_m"], pred[0]["sigma_hz"])
        assert at == block and int(rx["n_have"][0]) == 4 and int(rx["n_visible"][0]) == 4
        worst_phase, worst_freq = max(worst_phase, float(np.abs(d_phase).max())), max(worst_freq, float(np.abs(d_freq).max()))
    print("MEASURED pred_phase_samples", worst_phase, "pred_freq_hz", worst_freq)
    assert worst_phase <= LC.HANDOVER[1][0] and worst_freq <= LC.HANDOVER[1][1], "the prediction is not within the hand-over error the loops pull in from"
    assert worst_phase <= PC.MEASURED["pred_phase_samples"] * 1.0001 and worst_freq <= PC.MEASURED["pred_freq_hz"] * 1.0001
    # the hot hand-over at 24 576
    st, bank = s["at"][24576]
    states = AC.empty_states(4)
    states["sync"]["loop"]["prn"] = [S.PRNS[0], S.PRNS[1], P.PRN_NONE, S.PRNS[3]]
    rx, pred = P.predict(PC.stream_cfg(1), PC.STREAM_PRNS, st, bank, states["sync"], states["lock"], states["nav"], states["obs"], states["eph"])
    p4 = PC.STREAM_PRNS.index(S.PRNS[2])
    assert int(rx["assigned_mask"][0]) == 4 and int(pred[0, p4]["slot"]) == 2 and int(rx["n_tracked"][0]) == 3 and int(states["sync"]["loop"]["prn"][2]) == S.PRNS[2]
    (recs, after), = S.sync_on_restatement([(24576, (424,), states["sync"][2:3].copy(), S.sync_cfg(S.MOVING))])
    und = s["end"]["sync"][2]
    d_phase = float(after["loop"]["code_phase_fine"][0]) - float(und["loop"]["code_phase_fine"])
    d_phase = (d_phase + 8184.0) % 16368.0 - 8184.0
    d_freq = float(after["loop"]["if_freq_offset_hz"][0]) - float(und["loop"]["if_freq_offset_hz"])
    print("MEASURED repull_phase_samples", abs(d_phase), "repull_freq_hz", abs(d_freq))
    assert abs(d_phase) <= PC.MEASURED["repull_phase_samples"] * 1.0001 and abs(d_freq) <= PC.MEASURED["repull_freq_hz"] * 1.0001
    # its ephemeris: a fresh state over the last launch's words gives no set; the merged record is the bank's
    words = s["chain"][-1][3]
    own, bad = E.run(words[:, 2:3], 424, np.zeros(1, E.STATE_DTYPE))
    assert not bad and not int(own["flags"][0]) & P.F_VALID
    eph = s["chain"][-1][5].copy()
    eph[2] = own[0]
    bank = s["at"][24576][1].copy()
    rep, merged = P.bank(4, PC.STREAM_PRNS, np.array(S.PRNS, np.int32), eph, bank)
    assert int(rep["from_bank_mask"][0]) == 4 and merged[2].tobytes() == bank[0, p4].tobytes() and int(merged[2]["flags"]) == P.F_VALID
