"""The weighted grid in a window around each prediction without a GPU (include/gpsx.h gpsx_acq_window_weighted): the two structs and the
flags as a C compiler sees them against the restatement's and the binding's dtypes; both entry points exported, listed and bound,
k_acq_win's resources in the build; every row of tests/weighted_win_cases.py proven on the restatement's own integers; one small window
against a plain sum that uses no FFT; the identity with the hybrid grid's restatement; what holds for any launch; the fixture; and the
scenario on the restatements -- weighted_acq_cases' two receivers with predictions 40 samples and 130 Hz off the truth, decided and
handed over by weighted_acq_ref exactly as from the full grid; and an almanac warm start on weighted_pvt_cases' IF stream."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import weighted_acq_cases as AC
import weighted_acq_ref as Q
import weighted_coh_ref as R
import weighted_hyb_ref as H
import weighted_ms_ref as W
import weighted_win_cases as WC
import weighted_win_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "gpsx.h"
typedef int (*dev_fn)(gpsx_ctx *, const gpsx_acq_weighted_t *, const gpsx_acq_window_t *, const gpsx_wpred_t *, const void *, int, gpsx_peak_t *,
                      gpsx_acq_window_rep_t *);
typedef int (*host_fn)(gpsx_ctx *, const gpsx_acq_weighted_t *, const gpsx_acq_window_t *, const gpsx_wpred_t *, const uint8_t *, int, gpsx_peak_t *,
                       gpsx_acq_window_rep_t *);
_Static_assert(__builtin_types_compatible_p(__typeof__(&gpsx_acq_window_weighted_dev), dev_fn), "the _dev entry point");
_Static_assert(__builtin_types_compatible_p(__typeof__(&gpsx_acq_window_weighted), host_fn), "the host entry point");
#define C(f) printf("cfg.%s %zu\n", #f, offsetof(gpsx_acq_window_t, f))
#define P(f) printf("rep.%s %zu\n", #f, offsetof(gpsx_acq_window_rep_t, f))
int main(void)
{
  printf("sizeof.cfg %zu\nsizeof.rep %zu\nsizeof.peak %zu\nsizeof.pred %zu\n", sizeof(gpsx_acq_window_t), sizeof(gpsx_acq_window_rep_t), sizeof(gpsx_peak_t),
         sizeof(gpsx_wpred_t));
  C(n_coh); C(n_seg); C(half_width); C(half_bins); C(guard); C(need_flags); C(skip_flags); C(reserved);
  P(flags); P(first_bin); P(n_bins); P(centre);
  printf("flag.SEARCHED %u\nflag.SKIPPED %u\nflag.BAD %u\nflag.OFF_LATTICE %u\nflag.CLIPPED %u\n", GPSX_ACQ_WINDOW_SEARCHED, GPSX_ACQ_WINDOW_SKIPPED,
         GPSX_ACQ_WINDOW_BAD, GPSX_ACQ_WINDOW_OFF_LATTICE, GPSX_ACQ_WINDOW_CLIPPED);
  printf("pred.PREDICTED %u\npred.VISIBLE %u\npred.TRACKED %u\npred.ASSIGNED %u\nversion %d\n", GPSX_WPRED_PREDICTED, GPSX_WPRED_VISIBLE, GPSX_WPRED_TRACKED,
         GPSX_WPRED_ASSIGNED, GPSX_VERSION);
  return 0;
}
"""
FLAGS = ("SEARCHED", "SKIPPED", "BAD", "OFF_LATTICE", "CLIPPED")


@pytest.fixture(scope="module")
def oracle():
    from oracle import pyoracle
    return pyoracle.Oracle()


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_struct_layout_and_flags_against_the_dtypes():
    with tempfile.TemporaryDirectory(prefix="wwin_layout_") as tmp:
        src, exe = os.path.join(tmp, "layout.c"), os.path.join(tmp, "layout")
        with open(src, "w") as f:
            f.write(LAYOUT_C)
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
        got = {k: int(v) for k, v in (line.split() for line in subprocess.check_output([exe], text=True).splitlines())}
    assert (got["sizeof.cfg"], got["sizeof.rep"], got["sizeof.peak"], got["sizeof.pred"], got["version"]) == (32, 16, 16, 64, 110)
    for prefix, dtype in (("cfg.", V.CFG_DTYPE), ("rep.", V.REP_DTYPE)):
        offsets = {k[len(prefix):]: v for k, v in got.items() if k.startswith(prefix)}
        assert offsets == {name: dtype.fields[name][1] for name in dtype.names}, prefix
    assert [got["flag." + k] for k in FLAGS] == [getattr(V, k) for k in FLAGS] == [1, 2, 4, 8, 16]
    assert [got["pred." + k] for k in ("PREDICTED", "VISIBLE", "TRACKED", "ASSIGNED")] == [V.PREDICTED, V.VISIBLE, V.TRACKED, V.ASSIGNED]
    from stm32f4_sdr_gps_amd import capi
    assert capi.ACQ_WINDOW_CFG_DTYPE == V.CFG_DTYPE and capi.ACQ_WINDOW_REP_DTYPE == V.REP_DTYPE and capi.PEAK_DTYPE == V.PEAK_DTYPE
    assert (capi.ACQ_WINDOW_SEARCHED, capi.ACQ_WINDOW_SKIPPED, capi.ACQ_WINDOW_BAD, capi.ACQ_WINDOW_OFF_LATTICE, capi.ACQ_WINDOW_CLIPPED) == (1, 2, 4, 8, 16)
    assert capi.acq_window_cfg(20, 128, 2047, 32, 2046, need_flags=2, skip_flags=0x7D).tobytes() == V.cfg_record(V.make_cfg(20, 128, 2047, 32, 2046, 2, 0x7D)).tobytes()
    assert capi.acq_window_cfg(10, 8, 128, 2, 32).tobytes() == V.cfg_record(V.make_cfg(10, 8, 128, 2, 32)).tobytes()
    assert int(capi.acq_window_cfg(1, 1, 1, 0, 0)["need_flags"][0]) == capi.WPRED_PREDICTED | capi.WPRED_VISIBLE
    assert int(capi.acq_window_cfg(1, 1, 1, 0, 0)["skip_flags"][0]) == capi.WPRED_TRACKED | capi.WPRED_ASSIGNED


def test_symbols_binding_and_kernel_resources():
    """both entry points exported, listed in ABI_SYMBOLS and bound; exactly one k_acq_win in the build, without scratch and with the LDS
    it was planned with, and check_no_scratch asks for it; the grids' kernels still there; GPSX_VERSION still 110"""
    import inspect

    import __graft_entry__ as entry
    from stm32f4_sdr_gps_amd import build, capi
    names = {"gpsx_acq_window_weighted", "gpsx_acq_window_weighted_dev"}
    syms = subprocess.check_output(["nm", "-D", "--defined-only", build.LIB], text=True)
    assert names <= {line.split()[-1] for line in syms.splitlines() if line.strip()}
    assert names <= set(entry.ABI_SYMBOLS) and callable(getattr(capi.Engine, "acq_window", None)) and callable(getattr(capi.Engine, "acq_window_dev", None))
    lib = capi.load_library()
    assert len(lib.gpsx_acq_window_weighted.argtypes) == 8 and len(lib.gpsx_acq_window_weighted_dev.argtypes) == 8 and lib.gpsx_version() == 110
    res = build.check_wwin()
    print(res)
    assert len(res) == 1 and all("k_acq_win" in k and v["scratch_bytes"] == 0 and v["lds_bytes"] == build.WWIN_LDS_BYTES for k, v in res.items())
    assert build.WWIN_LDS_BYTES <= 80 * 1024          # two workgroups to a compute unit's 160 KiB
    assert "check_wwin()" in inspect.getsource(build.check_no_scratch)
    assert len(build.check_wacq()) == 1 and len(build.check_wpred()) == 1


# ---- the table ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", sorted(WC.GROUPS))
def test_every_row_reaches_its_clause(oracle, group):
    la = WC.launch(oracle, group)
    peaks, rep, energies = WC.restated(oracle, la)
    assert sorted(row.name for row, _, _ in la.units) == sorted(row.name for row in WC.ROWS if row.group == group)
    for row, r, p in la.units:
        assert row.check(WC.outcome(la, row, r, p, peaks, rep, energies)), (row.name, rep[r, p], peaks[r, p])


def test_the_table_covers_the_definition():
    names = [row.name for row in WC.ROWS]
    assert len(set(names)) == len(names)
    for word in ("skipped_without_predicted", "skipped_by_tracked", "skipped_by_assigned", "bad_nan_code_phase", "bad_infinite_code_phase",
                 "bad_code_phase_below_zero", "bad_code_phase_above_the_span", "bad_nan_f_hz", "code_phase_on_the_span", "code_phase_16367_5", "code_phase_0_5",
                 "code_phase_1_5", "code_phase_2_5", "seam_c_0", "seam_c_w_minus_1", "seam_c_span_minus_w", "seam_c_16367", "equal_maxima_across_the_seam",
                 "equal_maxima_smallest", "guard_0", "guard_w_minus_1", "d_32", "dc_minus_one", "dc_zero", "dc_last", "dc_n_dopp", "off_lattice_below",
                 "off_lattice_above", "x_just_over", "x_just_under", "x_on_2_30", "x_at_0_5", "x_at_1_5", "n_dopp_1", "stride_0", "top_of_the_range"):
        assert any(word in n for n in names), word
    groups = WC.GROUPS
    assert {g.mag for g in groups.values()} == {True, False}
    assert {g.cfg["half_bins"] for g in groups.values()} >= {0, 1, 32}
    assert any(s[0] >= 2 and 0 < s[8] < s[2] * s[3] for s in WC.SHAPES)      # searches that overlap in part
    assert groups["G"].stride == 0 and groups["D"].stride > groups["D"].cfg["n_coh"] * groups["D"].cfg["n_seg"]
    assert groups["G"].cfg["guard"] == groups["G"].cfg["half_width"] - 1 and groups["E"].cfg["guard"] == 0 and groups["G"].grid[2] == 1


def test_the_tie_seeds_are_what_the_search_finds(oracle):
    assert WC.tie_search(oracle, WC.Q_SEAM[1], True, range(WC.Q_SEAM[0], WC.Q_SEAM[0] + 1)) == WC.Q_SEAM[0]
    assert WC.tie_search(oracle, WC.Q_FLAT[1], False, range(WC.Q_FLAT[0], WC.Q_FLAT[0] + 1)) == WC.Q_FLAT[0]


def test_the_first_clause_of_the_bins_is_greater_than(oracle):
    """|x| > 2^30, not >=: on a lattice longer than any call accepts x = 2^30 is a bin and is searched, x = 2^30 + 1 is not looked at"""
    cfg = V.make_cfg(1, 1, 1, 0, 0)
    assert V.select(cfg, WC.SEL, 5.0, 2.0 ** 30, 0, 1, (1 << 30) + 2) == (V.SEARCHED, 5, 1 << 30, 1 << 30)
    assert V.select(cfg, WC.SEL, 5.0, 2.0 ** 30 + 1.0, 0, 1, (1 << 30) + 2) == (V.OFF_LATTICE, 0, 0, -1)
    assert V.select(cfg, WC.SEL, 5.0, -(2.0 ** 30), 0, 1, 5) == (V.OFF_LATTICE, 0, 0, -1)


def test_the_cached_energy_is_weighted_hyb_refs(oracle):
    """run() slices weighted_hyb_ref.energy unless its caller brings a cache; the cached form (the scenario's) equals it over all phases"""
    blocks = WC.random_blocks(5, 7)
    for first, n_coh, n_seg, prn, freq, mag in ((0, 1, 1, 3, 4092000, True), (1, 2, 3, 17, 4091250, False), (0, 3, 2, 17, 4091250, True)):
        cache = {}
        for _ in range(2):                      # (the second time from the cache)
            assert np.array_equal(V.energy(oracle, blocks, first, n_coh, n_seg, prn, freq, mag, cache), H.energy(oracle, blocks, first, n_coh, n_seg, prn, freq, mag))
    assert V.energy(oracle, blocks, 0, 1, 1, 3, 4092000, True).tolist() == H.energy(oracle, blocks, 0, 1, 1, 3, 4092000, True).tolist()


# ---- the energy against a sum that uses no FFT ------------------------------------------------------------------------------------------------
def test_a_small_window_against_a_direct_sum(oracle):
    """W = 3 around c = 1 (the seam inside), 2 x 2 blocks, both bits: I and Q of every window phase as a plain sum over segments' blocks
    and samples of the wiped values times the replica's chip"""
    cfg, grid, prn = V.make_cfg(2, 2, 3, 0, 1), (700, 500, 1), 9
    blocks = WC.random_blocks(77, 4)
    pred = V.make_pred(1, 1)
    V.set_pred(pred, 0, 0, 1.0, 700.0)
    energies = {}
    peaks, rep = V.run(oracle, cfg, pred, blocks, [prn], *grid, energies=energies)
    chip = 1 - 2 * np.repeat(oracle.ca_code(prn).astype(np.int64), 16)
    taus = V.window(1, 3)
    assert taus.tolist() == [16366, 16367, 0, 1, 2, 3, 4] and int(rep[0, 0]["flags"]) == V.SEARCHED
    want = []
    for tau in taus:
        e = 0
        for seg in range(2):
            acc, si, sq = 0, 0, 0
            for b in range(2):
                vi, vq, acc = R.wiped_values(oracle, blocks[2 * seg + b], 4092000 + 700, acc)
                shifted = chip[(np.arange(V.SAMPLES) - tau) % V.SAMPLES]
                si += int((vi * shifted).sum())
                sq += int((vq * shifted).sum())
            e += int(W.isqrt(si * si + sq * sq))
        want.append(e)
    assert energies[(0, 0, 0)].tolist() == want
    assert tuple(int(v) for v in peaks[0, 0, 0]) == V.record(want, taus, 1)


# ---- the identity with the grid ------------------------------------------------------------------------------------------------------------
def test_the_grids_record_when_its_phase_is_in_the_window(oracle):
    """every searched unit of the table: where the hybrid grid's restatement has its phase inside the window, max_val and phase are its;
    elsewhere max_val is below the grid's or reaches it at a later phase"""
    inside = 0
    for group in sorted(WC.GROUPS):
        la = WC.launch(oracle, group)
        peaks, rep, _ = WC.restated(oracle, la)
        units = [(r, p, d) for _, r, p in la.units if int(rep[r, p]["flags"]) & V.SEARCHED
                 for d in range(int(rep[r, p]["first_bin"]), int(rep[r, p]["first_bin"]) + int(rep[r, p]["n_bins"]))]
        units = sorted(set(units))[::7] if group == "D" else sorted(set(units))      # (D's 130 units: every seventh)
        full = H.grid(oracle, la.blocks, la.n_rx, la.prns, la.cfg["n_coh"], la.cfg["n_seg"], *la.grid, use_magnitude=la.mag, stride=la.stride, units=units)
        for r, p, d in units:
            taus = set(V.window(int(rep[r, p]["centre"]), la.cfg["half_width"]).tolist())
            g, w = full[r, p, d], peaks[r, p, d]
            if int(g["phase"]) in taus:
                inside += 1
                assert (int(w["max_val"]), int(w["phase"])) == (int(g["max_val"]), int(g["phase"])), (group, r, p, d)
            else:
                assert int(w["max_val"]) <= int(g["max_val"]), (group, r, p, d)
    print("units whose grid phase lies in the window:", inside)
    assert inside >= 2
    # ... and windows laid around the grid's own phases: group E's blocks and lattice, the prediction `off` samples from the grid's phase
    la = WC.launch(oracle, "E")
    offs = (-7, -3, 0, 3, 7, 8, -8)
    full = H.grid(oracle, la.blocks, len(offs), la.prns[:1], 1, 1, *la.grid, use_magnitude=la.mag, stride=1, units=[(r, 0, 2) for r in range(len(offs))])
    pred = V.make_pred(len(offs), 1)
    for r, off in enumerate(offs):
        V.set_pred(pred, r, 0, float((int(full[r, 0, 2]["phase"]) + off) % V.SAMPLES), 0.0)
    peaks, rep = V.run(oracle, la.cfg, pred, la.blocks, la.prns[:1], *la.grid, use_magnitude=la.mag, stride=1)
    for r, off in enumerate(offs):
        same = (int(peaks[r, 0, 2]["max_val"]), int(peaks[r, 0, 2]["phase"])) == (int(full[r, 0, 2]["max_val"]), int(full[r, 0, 2]["phase"]))
        assert same == (abs(off) <= la.cfg["half_width"]), (r, off)


# ---- what holds for any launch ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(WC.SHAPES)))
def test_any_launch(oracle, i):
    """unsearched records zero, the phase inside the window, max_val and sum reproducible from E, the reports' fields in range"""
    la = WC.random_launch(i)
    energies = {}
    peaks, rep = V.run(oracle, la.cfg, la.pred, la.blocks, la.prns, *la.grid, use_magnitude=la.mag, stride=la.stride, energies=energies)
    n_dopp = la.grid[2]
    assert (rep["flags"] & V.SEARCHED).any()
    for r in range(la.n_rx):
        for p in range(la.n_prn):
            f, d0, n, c = (int(rep[r, p][k]) for k in ("flags", "first_bin", "n_bins", "centre"))
            assert f in (V.SEARCHED, V.SEARCHED | V.CLIPPED, V.SKIPPED, V.BAD, V.OFF_LATTICE)
            if not f & V.SEARCHED:
                assert (d0, n, c) == (0, 0, 0) and not peaks[r, p].tobytes().strip(b"\0")
                continue
            assert 0 <= d0 and 1 <= n <= 2 * la.cfg["half_bins"] + 1 and d0 + n <= n_dopp and 0 <= c < V.SAMPLES
            assert bool(f & V.CLIPPED) == (n < 2 * la.cfg["half_bins"] + 1)
            assert not np.delete(peaks[r, p], np.arange(d0, d0 + n)).tobytes().strip(b"\0")
            taus = V.window(c, la.cfg["half_width"])
            for d in range(d0, d0 + n):
                e, pk = energies[(r, p, d)], peaks[r, p, d]
                assert int(pk["max_val"]) == int(e.max()) and (int(pk["phase"]) in taus.tolist() or int(pk["max_val"]) == 0)
                assert tuple(int(v) for v in pk) == V.record(e, taus, la.cfg["guard"])
    if _permutable(i):
        order = list(range(la.n_rx))[::-1]
        lb = WC.random_launch(i, permute=order)
        peaks_b, rep_b = V.run(oracle, lb.cfg, lb.pred, lb.blocks, lb.prns, *lb.grid, use_magnitude=lb.mag, stride=lb.stride)
        assert peaks_b.tobytes() == peaks[order].tobytes() and rep_b.tobytes() == rep[order].tobytes()


def _permutable(i):
    n_rx, _, n_coh, n_seg, _, _, _, _, stride = WC.SHAPES[i]
    return n_rx > 1 and stride >= n_coh * n_seg


# ---- the fixture -------------------------------------------------------------------------------------------------------------------------------
def test_smoke_fixture_is_the_cases_modules(oracle):
    """tests/golden/wwin_smoke.npz holds weighted_win_cases.smoke_case() bit for bit, in the binding's dtypes, and something happens in it"""
    from stm32f4_sdr_gps_amd import capi
    gold = np.load(os.path.join(ROOT, "tests", "golden", "wwin_smoke.npz"))
    want = WC.smoke_case(oracle)
    assert sorted(gold.files) == sorted(want)
    for k, v in want.items():
        assert np.asarray(gold[k]).tobytes() == np.asarray(v).tobytes() and np.asarray(gold[k]).dtype == np.asarray(v).dtype, k
    assert gold["cfg"].dtype == capi.ACQ_WINDOW_CFG_DTYPE and gold["rep"].dtype == capi.ACQ_WINDOW_REP_DTYPE and gold["pred"].dtype == capi.WPRED_DTYPE
    assert gold["pred"].shape == (3, 3) and int(gold["cfg"]["n_coh"][0]) == 2 and int(gold["cfg"]["n_seg"][0]) == 2
    flags = gold["rep"]["flags"].ravel().tolist()
    assert flags.count(V.SEARCHED) >= 3 and V.SEARCHED | V.CLIPPED in flags and V.SKIPPED in flags and V.BAD in flags and V.OFF_LATTICE in flags
    assert (gold["peaks"]["max_val"] > 0).sum() >= 12


# ---- the scenario ------------------------------------------------------------------------------------------------------------------------------
def test_two_receivers_are_acquired_from_predictions(oracle):
    """weighted_acq_cases' two receivers (10 x 8 blocks, PRNs 7, 19, 30, 3, 11, 25, 1, 2, -5000 .. 5000 Hz in 100 Hz steps) with
    fabricated predictions 40 samples and 130 Hz off weighted_multi_cases.CHAIN_SATS' truth for the six present pairs and anywhere for the
    ten absent ones; W = 128, D = 2, guard = 32.  The six present pairs give the full grid's max_val, phase and bin.  Peak over the mean
    of the far phases is measured again and compared with weighted_win_cases.MEASURED; weighted_acq_cases.SCN_DET's 4/1 lies between the
    two sides, so it is the threshold.  weighted_acq_ref on the window records detects exactly the six and writes the hand-over states it
    writes from the full grid's records, byte for byte."""
    full = AC.scenario_peaks(oracle)
    pred, cfg = WC.scenario_pred(), WC.scenario_cfg()
    span = AC.SCN_COH * AC.SCN_SEG
    blocks = np.concatenate([AC.scenario_blocks(r)[:span] for r in range(2)])
    peaks, rep = V.run(oracle, cfg, pred, blocks, AC.SCN_PRNS, *AC.SCN_GRID, cache={})
    assert (rep["flags"] == V.SEARCHED).all() and (rep["n_bins"] == 5).all()
    present, absent = [], []
    for r in range(2):
        for p in range(len(AC.SCN_PRNS)):
            d, m, s, tau = Q.best_record(peaks[r, p])
            if p in AC.scenario_present(r):
                assert (d, m, tau) == tuple(Q.best_record(full[r, p])[i] for i in (0, 1, 3)), (r, p)
                present.append(Q.ratio(m, s))
            else:
                absent.append(Q.ratio(m, s))
    got = dict(present_min=round(min(present), 3), absent_max=round(max(absent), 3))
    print("scenario: window peak over far mean", got)
    assert len(present) == 6 and len(absent) == 10 and got == WC.MEASURED
    num, den = AC.SCN_DET
    assert WC.MEASURED["absent_max"] < num / den < WC.MEASURED["present_min"]
    after = []
    for records in (peaks, full):
        st = AC.empty_states(2 * AC.SCN_CH)
        trace = []
        acq, det = Q.run(AC.scenario_cfg(), AC.SCN_PRNS, AC.SCN_GRID[0], AC.SCN_GRID[1], records, st["sync"], st["lock"], st["nav"], st["obs"], st["eph"],
                         trace=trace)
        after.append((st, acq, [t["detected"] for t in trace]))
    assert after[0][2] == [sorted(AC.scenario_present(r)) for r in range(2)] == after[1][2]
    for k in after[0][0]:
        assert after[0][0][k].tobytes() == after[1][0][k].tobytes(), k
    assert after[0][1].tobytes() == after[1][1].tobytes()


# ---- the warm start ----------------------------------------------------------------------------------------------------------------------------
def test_an_almanac_warm_start_on_the_if_stream(oracle):
    """weighted_pvt_cases' stream (four orbiting satellites) through the cached restatement chain to the filter state at block 24 576.  The
    bank's four entries are replaced by an almanac cut of the stream's ephemerides (weighted_alm_cases.almanac_records, then the
    restatement of gpsx_walm_to_eph); weighted_pred_ref predicts with handover = 0.  How far code_phase and f_hz land from the
    synthesiser's truth is measured again and compared with weighted_win_cases.WARM_MEASURED (16.74 samples, 0.663 Hz: the almanac's
    kilometre is 72 samples only along the line of sight).  W is the next power of two above twice the phase error (64), D covers twice
    the frequency error at a 50 Hz step (1).  The window search over blocks 24 576 .. 24 655 at 10 x 8 acquires the four PRNs by
    weighted_coh_ref.hits' rule (within 8 samples and one bin of the truth) with a peak over far mean of 25.6 at least -- n_seg did not
    have to be lengthened --, the three other entries of weighted_pred_cases.STREAM_PRNS have no prediction, are SKIPPED and detected by
    no threshold, and weighted_acq_ref hands exactly the four to slots."""
    import weighted_alm_cases as A
    import weighted_alm_ref as AR
    import weighted_pred_cases as PC
    import weighted_pred_ref as P
    import weighted_pvt_cases as S
    s = PC.stream_on_restatements()
    state, bank = s["at"][24576]
    alm, _ = A.almanac_records([row for _, row in S.sats()])
    bank = bank.copy()
    four = [PC.STREAM_PRNS.index(prn) for prn in S.PRNS]
    for k, p in enumerate(four):
        bank[0, p] = AR.to_eph(alm[k], bank.dtype)[0]
    rx, pred = P.predict(PC.stream_cfg(0), PC.STREAM_PRNS, state, bank, AC.empty_states(4)["sync"])
    d_phase, d_freq, at = PC.prediction_errors(pred[0], rx["t_ms"][0])
    got = dict(phase_samples=round(float(np.abs(d_phase).max()), 2), freq_hz=round(float(np.abs(d_freq).max()), 3))
    print("warm start: prediction errors", d_phase, d_freq, got)
    assert at == 24576 and got == {k: WC.WARM_MEASURED[k] for k in got}
    half_width = 1 << int(np.ceil(np.log2(2.0 * got["phase_samples"])))
    half_bins = int(np.ceil(2.0 * got["freq_hz"] / WC.WARM_GRID[1]))
    assert (half_width, half_bins) == (64, 1)
    cfg = V.make_cfg(10, 8, half_width, half_bins, half_width // 4)
    peaks, rep = V.run(oracle, cfg, pred, S.blocks()[24576:24576 + 80], PC.STREAM_PRNS, *WC.WARM_GRID, cache={})
    assert [int(f) for f in rep["flags"][0]] == [V.SEARCHED if p in four else V.SKIPPED for p in range(len(PC.STREAM_PRNS))]
    truth = {prn: (float(pred[0, p]["f_hz"]) - d_freq[k], (float(pred[0, p]["code_phase"]) + d_phase[k]) % V.SAMPLES) for k, (p, prn) in enumerate(zip(four, S.PRNS))}
    assert R.hits(peaks[:, four], S.PRNS, truth, 1, WC.WARM_GRID[0], WC.WARM_GRID[1]) == 4
    ratios = [Q.ratio(*Q.best_record(peaks[0, p])[1:3]) for p in four]
    print("warm start: peak over far mean", ratios)
    assert round(min(ratios), 1) == WC.WARM_MEASURED["present_min"] and WC.WARM_MEASURED["present_min"] > AC.SCN_DET[0] / AC.SCN_DET[1]
    assert not peaks[0, [p for p in range(len(PC.STREAM_PRNS)) if p not in four]].tobytes().strip(b"\0")
    st = AC.empty_states(4)
    trace = []
    acfg = Q.make_cfg(4, AC.SCN_DET, 0, 0, 0.0, 0)
    Q.run(acfg, PC.STREAM_PRNS, WC.WARM_GRID[0], WC.WARM_GRID[1], peaks, st["sync"], st["lock"], st["nav"], st["obs"], st["eph"], trace=trace)
    assert trace[0]["detected"] == sorted(four) and sorted(trace[0]["assigned"]) == sorted(four)
    assert sorted(int(v) for v in st["sync"]["loop"]["prn"]) == sorted(S.PRNS)
