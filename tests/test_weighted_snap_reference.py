"""The restatement of the snapshot fixes (tests/weighted_snap_ref.py) held to the definition in include/gpsx.h (gpsx_wsnap): the layouts
and symbols, one row per clause with its predicate (tests/weighted_snap_cases.py), the parts (the butterfly's order, the 5 x 5
factorisation), the method's error on noise-free skies against the synthesiser's truth -- with the truth's own fractional phases and
with whole samples -- over the prior errors step 3 resolves, the IF scenario, the clearance that makes the device comparison fair, the
library's exports and binding, and the smoke fixture.  No GPU."""
import os
import re

import numpy as np
import pytest

import weighted_fix_cases as W
import weighted_snap_cases as K
import weighted_snap_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("gpsx_wsnap", "gpsx_wsnap_dev", "gpsx_wsnap_to_fix")


def _header():
    with open(os.path.join(ROOT, "include", "gpsx.h")) as f:
        return f.read()


def test_layouts_are_the_headers():
    from stm32f4_sdr_gps_amd import capi
    assert (capi.WSNAP_CFG_DTYPE, capi.WSNAP_PRIOR_DTYPE, capi.WSNAP_DTYPE, capi.WSNAP_SV_DTYPE) == (S.CFG_DTYPE, S.PRIOR_DTYPE, S.SNAP_DTYPE, S.SV_DTYPE)
    assert (capi.WSNAP_FIX, capi.WSNAP_RESID, capi.WSNAP_TOO_FEW, capi.WSNAP_SINGULAR, capi.WSNAP_NO_CONV, capi.WSNAP_NONFINITE, capi.WSNAP_NO_PRIOR) == \
        (S.F_FIX, S.F_RESID, S.F_TOO_FEW, S.F_SINGULAR, S.F_NO_CONV, S.F_NONFINITE, S.F_NO_PRIOR)
    assert [S.CFG_DTYPE.fields[k][1] for k in ("ion", "el_min_rad", "epoch_offset_s", "max_resid_m", "det_num", "det_den", "min_peak", "min_sats", "reserved")] == \
        [0, 64, 72, 80, 88, 92, 96, 100, 104]
    assert [S.PRIOR_DTYPE.fields[k][1] for k in ("flags", "week", "rr", "tow_s", "reserved")] == [0, 4, 8, 32, 40]
    assert [S.SNAP_DTYPE.fields[k][1] for k in ("flags", "week", "n_detected", "n_candidates", "n_used", "n_iter", "ref", "used_mask", "rr", "b_m", "dt_s", "tow_s",
                                                "geo", "resid_rms_m", "qr")] == [0, 4, 8, 9, 10, 11, 12, 16, 24, 48, 56, 64, 72, 96, 104]
    assert [S.SV_DTYPE.fields[k][1] for k in ("flags", "n_ms", "phase", "dopp_hz", "el", "az", "resid_m", "reserved")] == [0, 4, 8, 12, 16, 24, 32, 40]
    h = _header()
    for decl in ("int gpsx_wsnap_dev(gpsx_ctx *ctx, const gpsx_wsnap_cfg_t *cfg, const gpsx_acq_weighted_t *g, const gpsx_peak_t *d_peaks,",
                 "int gpsx_wsnap(gpsx_ctx *ctx, const gpsx_wsnap_cfg_t *cfg, const gpsx_acq_weighted_t *g, const gpsx_peak_t *peaks,",
                 "int gpsx_wsnap_to_fix(const gpsx_wsnap_t *in, gpsx_wfix_t *out);", "} gpsx_wsnap_cfg_t;", "} gpsx_wsnap_prior_t;", "} gpsx_wsnap_t;", "} gpsx_wsnap_sv_t;"):
        assert decl in h, decl
    for name, value in (("FIX", 1), ("RESID", 2), ("TOO_FEW", 4), ("SINGULAR", 8), ("NO_CONV", 16), ("NONFINITE", 32), ("NO_PRIOR", 64), ("PRIOR_HAVE", 1),
                        ("SV_DETECTED", 1), ("SV_HAVE_EPH", 2), ("SV_CANDIDATE", 4), ("SV_USED", 8), ("SV_REFERENCE", 16)):
        assert re.search(rf"#define GPSX_WSNAP_{name}\s+{value}u\b", h), name
    assert re.search(r"#define GPSX_VERSION\s+110\b", h)        # no existing struct changed


def test_the_library_exports_the_entry_points_and_the_binding_has_them():
    import __graft_entry__ as ge
    from stm32f4_sdr_gps_amd import capi
    assert all(s in ge.ABI_SYMBOLS for s in SYMBOLS)
    lib = capi.load_library()
    assert len(lib.gpsx_wsnap.argtypes) == 9 and lib.gpsx_wsnap_dev.argtypes == lib.gpsx_wsnap.argtypes and len(lib.gpsx_wsnap_to_fix.argtypes) == 2
    cfg = capi.wsnap_cfg(0.004, min_sats=6)
    assert cfg.dtype == capi.WSNAP_CFG_DTYPE and float(cfg["epoch_offset_s"][0]) == 0.004 and int(cfg["min_sats"][0]) == 6 and not cfg["reserved"].any()
    assert cfg.tobytes() == S.make_cfg(0.004, min_sats=6).tobytes()
    assert capi.wsnap_prior([[1.0, 2.0, 3.0]], 2300, 5.0).tobytes() == S.make_prior([[1.0, 2.0, 3.0]], 2300, 5.0).tobytes()
    assert callable(capi.Engine.wsnap) and callable(capi.Engine.wsnap_dev) and callable(capi.Engine.wsnap_to_fix)


def test_to_fix_is_host_code_and_the_restatements():
    """gpsx_wsnap_to_fix needs no GPU: the fields gpsx_wkf's INIT reads, and a refusal without FIX"""
    from stm32f4_sdr_gps_amd import capi
    lib = capi.load_library()
    la = K.launch(len(K.ROWS))
    snap, _, _ = K.run(la)
    fix = np.zeros(len(snap), W.F.FIX_DTYPE)
    for r in range(len(snap)):
        rc = lib.gpsx_wsnap_to_fix(snap[r:r + 1].ctypes.data, fix[r:r + 1].ctypes.data)
        want = S.to_fix(snap[r])
        assert (rc == 0) == (want is not None) and (rc == 0 or rc == -22), (r, rc)
        assert fix[r].tobytes() == (want.tobytes() if want is not None else bytes(128)), r
    assert lib.gpsx_wsnap_to_fix(None, fix.ctypes.data) == -22 and lib.gpsx_wsnap_to_fix(snap.ctypes.data, None) == -22
    f = fix[0]
    assert int(f["flags"]) == W.F.F_FIX and abs(float(f["rx_tow_s"]) - float(f["dtr_s"]) - float(snap[0]["tow_s"])) < 1e-9 and int(f["week"]) == K.WEEK


def test_the_butterfly_adds_neighbours_first():
    v = np.zeros(64)
    v[0], v[1], v[2] = 1.0, 2.0 ** -53, 2.0 ** -53
    assert float(S.butterfly(v)) == 1.0                       # (1 + 2^-53) + (2^-53 + 0): the first pair rounds to 1 before the second arrives
    v[1], v[3] = 0.0, 2.0 ** -53
    assert float(S.butterfly(v)) == 1.0 + 2.0 ** -52          # (1 + 0) + (2^-53 + 2^-53)


def test_the_factorisation_solves_a_system_and_names_a_singular_one():
    rng = np.random.default_rng(3)
    a = rng.normal(0.0, 1.0, (9, 5))
    N, g = a.T @ a, a.T @ rng.normal(0.0, 1.0, 9)
    n = [np.float64(N[i, j]) for i in range(5) for j in range(i + 1)]
    ok, dx, q, shares = S.cholesky5(n, [np.float64(v) for v in g])
    inv = np.linalg.inv(N)
    assert ok and np.abs(dx - np.linalg.solve(N, g)).max() < 1e-12 and all(s > 1e-3 for s in shares)
    assert np.abs(q - np.array([inv[0, 0], inv[1, 1], inv[2, 2], inv[0, 1], inv[1, 2], inv[0, 2]])).max() < 1e-12
    a[:, 4] = a[:, 3]
    N = a.T @ a
    with np.errstate(all="ignore"):
        ok, _, _, _ = S.cholesky5([np.float64(N[i, j]) for i in range(5) for j in range(i + 1)], [np.float64(v) for v in g])
    assert not ok


@pytest.fixture(scope="module")
def canonical():
    la = K.launch(len(K.ROWS))
    return la, K.run(la)


@pytest.mark.parametrize("k", range(len(K.ROWS)), ids=[r.name for r in K.ROWS])
def test_one_row_per_clause(canonical, k):
    la, (snap, sv, trace) = canonical
    assert la.rows[k] is K.ROWS[k]
    assert K.ROWS[k].check(K.outcome(la, k, snap, sv, trace)), (K.ROWS[k].name, snap[k], sv[k])


def test_every_flag_has_a_row_and_exactly_one_is_set(canonical):
    la, (snap, sv, _) = canonical
    seen = {int(f) for f in snap["flags"]}
    assert seen == {S.F_FIX, S.F_RESID, S.F_TOO_FEW, S.F_SINGULAR, S.F_NO_CONV, S.F_NO_PRIOR}      # (NONFINITE: weighted_snap_cases says why not)
    assert np.isfinite(snap["rr"]).all() and np.isfinite(snap["tow_s"]).all() and np.isfinite(sv["el"]).all() and np.isfinite(sv["resid_m"]).all()
    unsolved = (snap["flags"] & (S.F_FIX | S.F_RESID)) == 0
    for f in ("rr", "b_m", "dt_s", "geo", "resid_rms_m", "qr"):
        assert not snap[f][unsolved].any(), f


def test_a_candidate_below_the_horizon_has_no_row():
    la, cfg = K.below_horizon_case()
    snap, sv, _ = K.run(la, cfg)
    assert K.below_horizon_check(snap, sv), (snap, sv)


def test_the_table_stands_clear_of_every_threshold(canonical):
    la, (snap, _, trace) = canonical
    assert K.decisions_clear(la, K.table_cfg(), snap, trace) == []


def test_a_pass_fails_on_rho_and_on_nothing_else():
    la, cfg = K.rho_case()
    snap, sv, trace = K.run(la, cfg)
    assert K.rho_check(sv, trace), (sv[0], trace[0]["pass0"]["rho"])
    lb, _ = K.rho_case(mirrored=True)
    _, svb, traceb = K.run(lb, cfg)
    assert K.rho_check(svb, traceb, mirrored=True), traceb[0]["pass0"]["rho"]      # the same satellite, the Sagnac term's sign turned: the pass holds


def test_rint_ties_in_n_p_go_to_the_even_millisecond():
    """fractional phases (what no record holds) put (pr + b0) / ms - s on k + 0.5 exactly for five satellites: N_p is the even neighbour,
    below it where k is even and above it where k is odd"""
    la, cfg, tau, want = K.tie_case()
    trace = []
    snap, sv = S.snap(cfg, la.prns, K.DOPP_MIN_HZ, K.DOPP_STEP_HZ, la.peaks, la.bank, la.bank_stride, la.prior, trace=trace, tau=tau)
    assert len(want) == 5
    u = trace[0]["u"]
    ks = [int(np.floor(u[p])) for p in want]
    assert any(k % 2 == 0 for k in ks) and any(k % 2 == 1 for k in ks)      # both directions
    for p, n in want.items():
        assert float(u[p]) - np.floor(u[p]) == 0.5 and int(sv[0, p]["n_ms"]) == n and n % 2 == 0, (p, u[p], sv[0, p])
        assert int(sv[0, p]["n_ms"]) == (int(np.floor(u[p])) if int(np.floor(u[p])) % 2 == 0 else int(np.floor(u[p])) + 1)


@pytest.mark.parametrize("shape", K.GPU_SHAPES + K.GPU_OTHER, ids=["-".join(str(v) for v in s) for s in K.GPU_SHAPES + K.GPU_OTHER])
def test_the_gpu_tests_launches_leave_few_out_on_the_cpu(shape):
    """every launch tests/test_gpu_weighted_snap.py compares, built from the same entry by the same function: at most 5 % of its receivers
    come within round-off of a threshold in the restatement alone; without d_sv the receiver records are the same; the random launches
    hold receivers of every kind and their fixes lie where whole-sample phases put them"""
    la, cfg, table = K.gpu_launch(shape)
    snap, sv, trace = K.run(la, cfg)
    left_out = K.decisions_clear(la, cfg, snap, trace)
    assert len(left_out) <= K.MAX_LEFT_OUT * la.n_rx, left_out
    snap2, none, _ = K.run(la, cfg, want_sv=False)
    assert none is None and snap2.tobytes() == snap.tobytes()
    if shape[:3] == (1, 5, 1):
        assert int(snap[0]["flags"]) == S.F_FIX and int(snap[0]["n_used"]) == 5
    if not table and la.n_rx >= 21 and la.n_prn >= 10:
        assert {S.F_FIX, S.F_NO_PRIOR} <= {int(f) for f in snap["flags"]} and (snap["flags"] == S.F_FIX).sum() >= la.n_rx // 3
    if not table:
        fixed = snap["flags"] == S.F_FIX
        err = np.array([np.linalg.norm(snap["rr"][r] - la.recs[r]["rr"]) for r in np.flatnonzero(fixed)])
        assert err.size == 0 or np.median(err) < 200.0, err


def test_noise_free_skies_recover_site_and_time():
    """four sites x 5 / 8 / 12 satellites x priors 10 / 50 / 100 km and +-20 / 60 s off: each prior's combined error in a range
    difference is inside step 3's limit by the synthesiser's own geometry, the restatement resolves every one, and with the truth's own
    fractional phases it finds the site and the time to round-off and the two models' difference; with whole samples to what a sample
    is worth.  Prints the figures MEASURED holds."""
    worst = {True: [0.0, 0.0], False: [0.0, 0.0]}
    worst_difference = 0.0
    for site in sorted(W.SITES):
        for n in K.SKY_SATS:
            rows = K.truth_phases(site, n, 0, W.TOW + K.EPOCH_S)[3]
            for off_m, off_s in K.prior_errors():
                worst_difference = max(worst_difference, K.difference_error_m(site, rows, W.TOW + K.EPOCH_S, off_m, off_s))
                for exact in (True, False):
                    snap, sv, n_ms = K.sky_run(site, n, 0, off_m, off_s, exact)
                    assert int(snap["flags"]) == S.F_FIX and int(snap["n_used"]) == n, (site, n, off_m, off_s, exact, snap)
                    ref = int(snap["ref"])
                    assert [int(v) - int(sv["n_ms"][ref]) for v in sv["n_ms"]] == [int(v) - int(n_ms[ref]) for v in n_ms]
                    em, es = K.sky_errors(snap, site)
                    worst[exact] = [max(worst[exact][0], em), max(worst[exact][1], es)]
    print("noise-free skies: exact phases %.4e m %.4e s, whole samples %.3f m %.6f s; the priors' largest range-difference error %.0f m"
          % (worst[True][0], worst[True][1], worst[False][0], worst[False][1], worst_difference))
    assert worst_difference < K.LIMIT_M
    assert worst[True][0] <= K.BOUNDS["noise_free_m"] and worst[True][1] <= K.BOUNDS["noise_free_s"], worst
    assert worst[False][0] <= K.BOUNDS["whole_m"] and worst[False][1] <= K.BOUNDS["whole_s"], worst


def test_the_bounds_are_the_measured_figures_with_the_projects_factors():
    assert K.BOUNDS["noise_free_m"] == 2.0 * K.MEASURED["exact_m"] and K.BOUNDS["whole_m"] == 1.5 * K.MEASURED["whole_m"]
    assert K.BOUNDS["scenario_m"] == 1.5 * K.MEASURED["scenario_m"] and K.BOUNDS["scenario_s"] == 1.5 * K.MEASURED["scenario_s"]
    assert K.PARITY_CAP_M == W.PARITY_CAP_M == 1e-4


def test_the_if_scenario_on_the_restatements(oracle):
    """six satellites' IF samples, eight blocks, the hybrid grid's restatement at 1 x 8 on a 500 Hz lattice, the prior 50 km and 20 s off:
    FIX, all six used, the milliseconds the truth's"""
    import weighted_hyb_ref as H
    sc = K.scenario()
    assert abs(float(np.linalg.norm(K.SCEN_OFF_M)) - 50000.0) < 1.0 and float(sc["cfg"]["epoch_offset_s"][0]) == 0.004
    peaks = H.grid(oracle, sc["blocks"], 1, [int(p) for p in sc["prns"]], 1, K.SCEN_BLOCKS, *K.SCEN_GRID, True)
    for p, (fd, delay) in enumerate(sc["first"]):
        d, m, s, tau = S.Q.best_record(peaks[0, p])
        assert abs(K.SCEN_GRID[0] + d * K.SCEN_GRID[1] - fd) <= 300.0 and min((tau - delay) % 16368.0, (delay - tau) % 16368.0) <= 2.0, (p, d, tau, fd, delay)
    snap, sv = S.snap(sc["cfg"], sc["prns"], K.SCEN_GRID[0], K.SCEN_GRID[1], peaks, sc["bank"][None], 6, sc["prior"])
    em, es = K.scenario_check(sc, snap[0], sv[0])
    print("IF scenario: position error %.2f m, time error %.5f s, resid_rms_m %.2f" % (em, es, float(snap[0]["resid_rms_m"])))
    assert em <= K.BOUNDS["scenario_m"] and es <= K.BOUNDS["scenario_s"], (em, es)
    fix = S.to_fix(snap[0])
    assert fix is not None and int(fix["flags"]) == W.F.F_FIX


def test_smoke_fixture_is_the_restatements_answer():
    gold = np.load(os.path.join(ROOT, "tests", "golden", "wsnap_smoke.npz"))
    la = K.smoke_case()
    snap, sv, _ = K.run(la)
    assert gold["peaks"].tobytes() == la.peaks.tobytes() and gold["bank"].tobytes() == la.bank.tobytes() and gold["prior"].tobytes() == la.prior.tobytes()
    assert gold["cfg"].tobytes() == K.table_cfg().tobytes() and list(gold["prns"]) == list(la.prns)
    for f in K.SNAP_INT_FIELDS:
        assert gold["snap"][f].tobytes() == snap[f].tobytes(), f
    assert np.abs(gold["snap"]["rr"] - snap["rr"]).max() < 1e-6 and len(gold["skip"]) <= K.MAX_LEFT_OUT * la.n_rx
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "wsnap_smoke.npz")) < 1 << 20
