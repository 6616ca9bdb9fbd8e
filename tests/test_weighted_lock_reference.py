"""The weighted path's lock monitor (include/gpsx.h gpsx_wlock), without a GPU: the layout of its structs as a C compiler sees them,
the exported entry points and the binding, the host-side C/N0 helper, and the exact CPU restatement its GPU tests compare against
(tests/weighted_lock_ref.py): hand-computed epochs, every branch of the definition on the fabricated streams, launches cut anywhere,
and the scenario on the restatements -- IF samples, the loop with bit sync, the lock monitor -- on three seeds.

Measured on the restatements (tests/weighted_lock_cases.py MEASURED; amplitude 0.035, 3000 ms in launches of 500, PRN 19 absent from
block 2000 on, two channels handed PRNs 3 and 25 that are not in the stream, seeds 1, 2, 3; SEARCH epochs of 25 windows, LOCKED
epochs of 10):
  code_ratio   satellites >= 2.66 (the weakest a SEARCH epoch during pull-in), noise only <= 1.94; code_min = 2.3
  car_ratio    satellites >= 0.973, noise only <= 0.572; car_min = 0.75
  snr          satellites >= 42.4, noise only <= 1.06; snr_min = 6
  loss         LOST_CODE 451 blocks after the satellite has gone, on every seed (two LOCKED epochs of 200 blocks that began after it)
  false sync   the bit synchroniser locks on noise in two of the six absent-PRN runs (seed 1 PRN 3 at block 1782, seed 3 PRN 25 at
               2621): neither raises CODE or CARRIER
  C/N0         37.2 dB-Hz at a = 0.035 (analytic 41.8: 4.6 below) and 31.5 at a / 2 (analytic 35.8: 4.3 below), per-epoch standard
               deviations 1.65 and 1.67 dB over 27 epochs each; halving the amplitude lowers it by 5.7 dB."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import weighted_lock_cases as X
import weighted_lock_ref as R
import weighted_nav_ref as N
import weighted_obs_ref as O
import weighted_sync_cases as K
import weighted_sync_ref as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"gpsx_wlock", "gpsx_wlock_dev", "gpsx_wlock_cn0_dbhz"}
F32 = np.float32
WIN, LOCKED = R.WSYNC_WINDOW, R.WSYNC_WINDOW | R.WSYNC_LOCKED

LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "gpsx.h"
typedef int (*dev_fn)(gpsx_ctx *, const gpsx_wlock_cfg_t *, const gpsx_wsync_rec_t *, int, int, gpsx_wlock_state_t *, gpsx_wsync_state_t *, int,
                      gpsx_wlock_t *);
typedef int (*cn0_fn)(const gpsx_wlock_t *, int, int, float *);
_Static_assert(__builtin_types_compatible_p(__typeof__(&gpsx_wlock_dev), dev_fn), "the _dev entry point");
_Static_assert(__builtin_types_compatible_p(__typeof__(&gpsx_wlock), dev_fn), "the host entry point");
_Static_assert(__builtin_types_compatible_p(__typeof__(&gpsx_wlock_cn0_dbhz), cn0_fn), "the C/N0 helper");
#define S(f) printf("state.%s %zu\n", #f, offsetof(gpsx_wlock_state_t, f))
#define R(f) printf("lock.%s %zu\n", #f, offsetof(gpsx_wlock_t, f))
#define G(f) printf("cfg.%s %zu\n", #f, offsetof(gpsx_wlock_cfg_t, f))
int main(void)
{
  printf("sizeof.state %zu\nsizeof.lock %zu\nsizeof.cfg %zu\n", sizeof(gpsx_wlock_state_t), sizeof(gpsx_wlock_t), sizeof(gpsx_wlock_cfg_t));
  S(blocks_seen); S(last_epoch_end_p1); S(sum_a); S(sum_p); S(sum_d); S(sum_e); S(sum_l); S(last_p); S(last_code_ratio); S(last_car_ratio);
  S(last_snr); S(epoch_n); S(flags); S(last_k); S(code_good); S(code_bad); S(car_good); S(car_bad); S(false_run); S(n_lost_code);
  S(n_lost_carrier); S(n_rearm); S(n_range); S(reserved);
  R(flags); R(n_epochs); R(last_k); R(age_blocks); R(code_ratio); R(car_ratio); R(snr); R(n_range); R(p); R(n_lost_code); R(n_lost_carrier);
  R(n_rearm); R(reserved);
  G(epoch_search); G(epoch_lock); G(code_min); G(car_min); G(snr_min); G(n_good); G(n_bad); G(rearm); G(patience); G(reserved);
  printf("flag.state %u\nflag.events %u\nversion %d\n", GPSX_WLOCK_CODE | GPSX_WLOCK_CARRIER | GPSX_WLOCK_PENDING | GPSX_WLOCK_OPEN_LOCKED |
         GPSX_WLOCK_EPOCH_LOCKED, GPSX_WLOCK_LOST_CODE | GPSX_WLOCK_LOST_CARRIER | GPSX_WLOCK_REARMED | GPSX_WLOCK_RANGE, GPSX_VERSION);
  return 0;
}
"""


def test_struct_layout_as_a_c_compiler_sees_it():
    with tempfile.TemporaryDirectory(prefix="wlock_layout_") as tmp:
        src, exe = os.path.join(tmp, "layout.c"), os.path.join(tmp, "layout")
        with open(src, "w") as f:
            f.write(LAYOUT_C)
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
        got = {k: int(v) for k, v in (line.split() for line in subprocess.check_output([exe], text=True).splitlines())}
    assert got["sizeof.cfg"] == 40 and got["sizeof.state"] == 128 and got["sizeof.lock"] == 64
    assert got["flag.state"] == R.STATE_FLAGS == 31 and got["flag.events"] == R.F_LOST_CODE | R.F_LOST_CARRIER | R.F_REARMED | R.F_RANGE == 480
    assert got["version"] == 110
    for prefix, dtype in (("state.", R.STATE_DTYPE), ("lock.", R.LOCK_DTYPE), ("cfg.", R.CFG_DTYPE)):
        offsets = {k[len(prefix):]: v for k, v in got.items() if k.startswith(prefix)}
        assert offsets == {name: dtype.fields[name][1] for name in dtype.names}, prefix
    from stm32f4_sdr_gps_amd import capi
    assert capi.WLOCK_STATE_DTYPE == R.STATE_DTYPE and capi.WLOCK_DTYPE == R.LOCK_DTYPE and capi.WLOCK_CFG_DTYPE == R.CFG_DTYPE
    assert (capi.WLOCK_FLAG_CODE, capi.WLOCK_FLAG_CARRIER, capi.WLOCK_FLAG_PENDING, capi.WLOCK_FLAG_OPEN_LOCKED, capi.WLOCK_FLAG_EPOCH_LOCKED,
            capi.WLOCK_FLAG_LOST_CODE, capi.WLOCK_FLAG_LOST_CARRIER, capi.WLOCK_FLAG_REARMED, capi.WLOCK_FLAG_RANGE) == (
                R.F_CODE, R.F_CARRIER, R.F_PENDING, R.F_OPEN_LOCKED, R.F_EPOCH_LOCKED, R.F_LOST_CODE, R.F_LOST_CARRIER, R.F_REARMED, R.F_RANGE)
    assert capi.wlock_cfg(25, 10, 2.3, 0.75, 6.0, 2, 2, 1, 5).tobytes() == R.cfg_array(X.scenario_cfg(1)).tobytes()


def test_library_exports_the_lock_monitor(lib_path):
    syms = subprocess.check_output(["nm", "-D", "--defined-only", lib_path], text=True)
    assert SYMBOLS <= {line.split()[-1] for line in syms.splitlines() if line.strip()}
    from stm32f4_sdr_gps_amd import capi
    import __graft_entry__ as entry
    assert SYMBOLS <= set(entry.ABI_SYMBOLS)
    assert callable(getattr(capi.Engine, "wlock", None)) and callable(capi.wlock_cn0_dbhz)
    lib = capi.load_library()
    assert lib.gpsx_wlock_dev.argtypes is not None and len(lib.gpsx_wlock.argtypes) == 9 and lib.gpsx_version() == 110


def test_lock_kernel_has_no_scratch_no_lds_and_the_look_ahead_the_tests_assume(lib_path):
    from stm32f4_sdr_gps_amd import build
    hits = [v for k, v in build.check_no_scratch().items() if "k_wlock" in k]
    assert len(hits) == 1 and hits[0]["scratch_bytes"] == 0 and hits[0]["lds_bytes"] == 0, hits
    assert hits[0]["vgprs"] <= 128      # two sets of four slots' eight words, five int64 sums, the state: four waves per SIMD
    text = open(os.path.join(ROOT, "stm32f4_sdr_gps_amd", "csrc", "k_wlock.hip")).read()
    assert int(re.search(r"constexpr int kAhead = (\d+);", text).group(1)) == X.AHEAD


# ---- the arithmetic -----------------------------------------------------------------------------------------------------------------
def test_int64_to_float_rounds_once_to_nearest_even():
    for v, want in ((0, 0.0), (1 << 24, 2.0 ** 24), ((1 << 24) + 1, 2.0 ** 24), ((1 << 24) + 3, 2.0 ** 24 + 4), ((1 << 24) + 2, 2.0 ** 24 + 2),
                    (-((1 << 25) + 2), -(2.0 ** 25)), (-((1 << 25) + 6), -(2.0 ** 25 + 8)), ((1 << 62) - 1, 2.0 ** 62)):
        assert R.f32_of_int(v) == F32(want) and R.f32_of_int(v).dtype == np.float32, v
    # one rounding, not two: above the tie in bit 36 by one unit -- a double drops the unit and the tie then goes to even, down
    v = (1 << 60) + (1 << 36) + 1
    assert float(v) == float((1 << 60) + (1 << 36)) and np.float32(float(v)) == F32(2.0 ** 60)
    assert R.f32_of_int(v) == F32(2.0 ** 60 + 2.0 ** 37)


def test_an_epoch_by_hand():
    """two LOCKED windows: A = 3 + 5, P = 25 + 25, D = -7 + 25, E = L = 10: code 100 / 20, carrier 18 / 50, snr 64 / (2 x 50 - 64)"""
    cfg = R.make_cfg(7, 2, 5.0, 0.36, 1.75, 1, 1)
    s = {name: 0 for name in R.STATE_DTYPE.names}
    s.update(last_code_ratio=F32(0), last_car_ratio=F32(0), last_snr=F32(0), blocks_seen=1000)
    o = R.channel([(19, LOCKED, (1, 2, 3, 4, 2, 1)), (-1, 0, (0,) * 6), (39, LOCKED, (-1, -2, -5, 0, 1, -2))], s, 50, cfg)
    assert o["code_ratio"] == F32(5.0) and o["car_ratio"] == F32(18) / F32(50) and o["snr"] == F32(64) / F32(36) and o["p"] == 50 and o["last_k"] == 2
    assert o["flags"] == R.F_CODE | R.F_CARRIER | R.F_EPOCH_LOCKED and o["n_epochs"] == 1 and o["age_blocks"] == 10
    assert s["last_epoch_end_p1"] == 1040 and s["blocks_seen"] == 1050 and s["epoch_n"] == 0 and s["sum_p"] == 0 and s["flags"] & R.F_OPEN_LOCKED
    # the thresholds are inclusive; one ulp above any of them and the verdict fails
    for name in ("code_min", "car_min", "snr_min"):
        up = dict(cfg)
        up[name] = np.nextafter({"code_min": o["code_ratio"], "car_min": o["car_ratio"], "snr_min": o["snr"]}[name], F32(np.inf))
        s2 = {k: 0 for k in R.STATE_DTYPE.names}
        s2.update(last_code_ratio=F32(0), last_car_ratio=F32(0), last_snr=F32(0))
        exact = dict(cfg, **{name: {"code_min": o["code_ratio"], "car_min": o["car_ratio"], "snr_min": o["snr"]}[name]})
        wins = [(19, LOCKED, (1, 2, 3, 4, 2, 1)), (39, LOCKED, (-1, -2, -5, 0, 1, -2))]
        assert R.channel(wins, dict(s2), 50, exact)["flags"] & 3 == 3
        assert R.channel(wins, dict(s2), 50, up)["flags"] & 3 == (2 if name == "code_min" else 1), name
    # zero denominators give 0, not a NaN
    assert R.ratios(3, 0, 0, 0, 5, 5) == (F32(0), F32(0), F32(0)) and R.ratios(2, 10, 50, 50, 0, 0)[0] == F32(0)
    assert R.ratios(2, 10, 50, 50, 1, 1)[2] == F32(0)      # K P == A A
    # the largest sums of the definition are exact in int64: 1024 windows of 2^20 - 1
    top = (1 << 20) - 1
    code, car, snr = R.ratios(1024, 1024 * top, 2048 * top * top, 0, 2048 * top * top, 2048 * top * top)
    assert code == F32(1.0) and car == F32(0.0) and snr == F32(1.0)


def _fab(k, n_windows, cfg=X.FAB, mode=R.SYNC_LOCKED, launches=None):
    """stream k of the fabricated table alone over n_windows windows -> (lock records per launch, state, sync state, epochs)"""
    st, sync = np.zeros(1, R.STATE_DTYPE), Y.handover(7, 100.0, 0.0)
    sync["mode"], sync["win_n"], sync["bit_ip"], sync["search_n"], sync["prev_best_p1"] = mode, 3, 999, 17, 4
    sync["win_iq"], sync["loop"]["n_updates"] = 55, 9
    out, trace, at = [], {}, 0
    for n in launches or [n_windows]:
        rec = X.fab_records(at, n, k + 1)[:, k:k + 1]
        lock, bad = R.run(rec, X.SPAN * n, st, cfg, sync, traces=trace)
        assert not bad
        out.append(lock[0].copy())
        at += n
    return out, st[0], sync[0], trace.get(0, [])


def test_the_fabricated_streams_reach_every_branch():
    """32 streams x 60 windows with FAB (LOCKED epochs of 2 windows, SEARCH epochs of 3, n_good 3, n_bad 2, patience 3, rearm 3)"""
    none = dict(X.FAB, rearm=0)
    lock, st, _, ep = _fab(0, 60, none)
    assert lock[0]["flags"] == R.F_CODE | R.F_CARRIER | R.F_EPOCH_LOCKED and lock[0]["n_epochs"] == 30 and ep[2][6] & 3 == 3 and ep[1][6] & 3 == 0
    lock, st, _, _ = _fab(1, 60, none)
    assert lock[0]["flags"] == R.F_CODE and lock[0]["n_epochs"] == 20 and lock[0]["last_k"] == 3 and st["car_good"] == 0
    lock, st, _, ep = _fab(2, 60, none)      # n_good - 1 good epochs, then a bad one
    assert not any(e[6] & 3 for e in ep) and max(st["code_good"], st["car_good"]) <= 2 and lock[0]["n_lost_code"] == 0
    lock, st, _, ep = _fab(3, 60, none)      # n_bad - 1 bad epochs, then a good one
    assert all(e[6] & 3 == 3 for e in ep[2:]) and lock[0]["n_lost_code"] == 0 and lock[0]["n_lost_carrier"] == 0
    lock, st, _, ep = _fab(4, 60, none)      # lost: both, again and again
    assert lock[0]["n_lost_code"] == 5 and lock[0]["n_lost_carrier"] == 5 and lock[0]["flags"] & (R.F_LOST_CODE | R.F_LOST_CARRIER) and not st["flags"] & R.F_PENDING
    lock, st, _, ep = _fab(5, 60, none)      # the kind changes in mid-epoch: of ten windows only the last four make an epoch (the next cycle's first three too)
    assert [e[1] for e in ep[:3]] == [True, False, True] and [e[0] for e in ep[:3]] == [X.SPAN * 2 - 1, X.SPAN * 9 - 1, X.SPAN * 12 - 1]
    assert lock[0]["n_lost_carrier"] == 0 and not lock[0]["flags"] & R.F_CARRIER
    for k, zero in ((6, "code_ratio"), (7, "car_ratio"), (8, "snr")):      # a zero denominator in each ratio
        lock, st, _, _ = _fab(k, 60, none)
        assert lock[0][zero] == 0 and lock[0]["n_epochs"] == 30, k
    assert _fab(7, 60, none)[0][0]["snr"] == 0 and _fab(6, 60, none)[0][0]["snr"] > 100
    lock, st, _, _ = _fab(11, 60, none)      # 2^20 - 1 everywhere
    assert lock[0]["n_range"] == 0 and lock[0]["p"] > 1 << 41 and lock[0]["flags"] & R.F_EPOCH_LOCKED
    lock, st, _, ep = _fab(12, 60, none)     # 2^20 somewhere: counted, not accumulated
    assert lock[0]["n_range"] == 12 and lock[0]["flags"] & R.F_RANGE and lock[0]["n_epochs"] == 24 and lock[0]["flags"] & 3 == 3
    assert _fab(13, 60, none)[0][0]["n_epochs"] == 20 and _fab(14, 60, none)[0][0]["n_epochs"] < 30      # empty slots; end_block out of range
    # patience: one short, and complete
    lock, st, sync, ep = _fab(9, 60)
    assert lock[0]["n_rearm"] == 0 and sync["mode"] == R.SYNC_LOCKED and not lock[0]["flags"] & (R.F_CARRIER | R.F_REARMED) and lock[0]["flags"] & R.F_CODE
    lock, st, sync, ep = _fab(10, 60)
    assert lock[0]["n_rearm"] == 1 and lock[0]["flags"] == R.F_REARMED | R.F_EPOCH_LOCKED and any(e[6] & R.F_PENDING for e in ep) and st["flags"] == R.F_EPOCH_LOCKED
    assert (sync["mode"], sync["win_n"], sync["bit_ip"], sync["search_n"], sync["prev_best_p1"], sync["loop"]["n_updates"]) == (0, 0, 0, 0, 0, 0)
    assert not sync["win_iq"].any() and sync["loop"]["prn"] == 7 and sync["loop"]["code_phase_fine"] == 100.0
    first = [i for i, e in enumerate(ep) if e[6] & R.F_PENDING][0]
    assert first == 2 and st["false_run"] == 0      # the third bad verdict
    # pending with the sync state in SEARCH and WAIT: cleared, nothing written; with rearm == 0 nothing is ever pending
    for mode in (R.SYNC_SEARCH, R.SYNC_WAIT):
        lock, st, sync, _ = _fab(10, 60, mode=mode)
        assert lock[0]["n_rearm"] == 0 and not lock[0]["flags"] & R.F_REARMED and not st["flags"] & R.F_PENDING and st["false_run"] < 3
        assert (sync["mode"], sync["win_n"], sync["bit_ip"], sync["search_n"], sync["prev_best_p1"]) == (mode, 3, 999, 17, 4)
    lock, st, sync, ep = _fab(10, 60, none)
    assert not any(e[6] & R.F_PENDING for e in ep) and st["false_run"] == 30 and sync["mode"] == R.SYNC_LOCKED
    # a code loss re-arms with bit 0 alone, a missing carrier with bit 1 alone
    assert _fab(4, 60, dict(X.FAB, rearm=1))[0][0]["n_rearm"] == 1 and _fab(10, 60, dict(X.FAB, rearm=1))[0][0]["n_rearm"] == 0
    assert _fab(4, 60, dict(X.FAB, rearm=2))[0][0]["n_rearm"] == 0 and _fab(10, 60, dict(X.FAB, rearm=2))[0][0]["n_rearm"] == 1
    # a SEARCH window clears CARRIER and counts the loss
    s = {name: 0 for name in R.STATE_DTYPE.names}
    s.update(last_code_ratio=F32(0), last_car_ratio=F32(0), last_snr=F32(0), flags=R.F_CARRIER | R.F_CODE, car_good=7, car_bad=1, false_run=2)
    o = R.channel([(3, WIN, (400, 20, 1000, 50, 400, -20))], s, 4, X.FAB)
    assert o["flags"] == R.F_CODE | R.F_LOST_CARRIER and o["n_lost_carrier"] == 1 and (s["car_good"], s["car_bad"], s["false_run"]) == (0, 0, 0)


@pytest.mark.parametrize("parts", [[4, 1, 9, 3], [1] * 17, [16, 1], [2, 15]])
def test_launches_cut_anywhere(parts):
    """17 windows of every stream in one launch and in parts (an epoch that ends with a launch's last slot, one that ends with the
    next launch's first): the same states, and the same last record but for its per-launch fields"""
    idx = range(X.DISTINCT)
    cfg = dict(X.FAB, rearm=0)
    _, _, whole, want_st, _ = X.fab_run([17], X.DISTINCT, cfg)
    _, _, cut, st, _ = X.fab_run(parts, X.DISTINCT, cfg)
    assert st.tobytes() == want_st.tobytes()
    a, b = whole[-1][2].copy(), cut[-1][2].copy()
    assert sum(int(c[2]["n_epochs"][0]) for c in cut) == int(a["n_epochs"][0]) and (a["n_epochs"] > 0).all()
    events = R.F_LOST_CODE | R.F_LOST_CARRIER | R.F_REARMED | R.F_RANGE
    for k in idx:
        assert int(a["flags"][k]) & events == np.bitwise_or.reduce([int(c[2]["flags"][k]) & events for c in cut]), k
    for r in (a, b):
        r["n_epochs"] = 0
        r["flags"] &= ~np.uint32(events)
    assert a.tobytes() == b.tobytes()


def test_bad_states_are_left_alone():
    st0, sync0, launches, _, _ = X.fab_run([9], 64, warm=7)
    st = st0.copy()
    bad = [1 + 2 * i for i in range(len(X.BAD_FIELDS))]
    for ch, (field, value) in zip(bad, X.BAD_FIELDS):
        st[field][ch] = value
    edges = [2 + 2 * i for i in range(len(X.GOOD_EDGES))]
    for ch, (field, value) in zip(edges, X.GOOD_EDGES):
        st[field][ch] = value
    before, sync = st.copy(), sync0.copy()
    lock, found = R.run(launches[0][0], launches[0][1], st, X.FAB, sync)
    assert found == bad and st[bad].tobytes() == before[bad].tobytes() and sync[bad].tobytes() == sync0[bad].tobytes()
    assert (lock["age_blocks"][bad] == -1).all() and not lock["flags"][bad].any() and not lock["snr"][bad].any()
    good = [c for c in range(64) if c not in bad]
    assert (st["blocks_seen"][good] != before["blocks_seen"][good]).all()


def test_cn0_helper_against_numpys_double_logarithm(lib_path):
    """10 log10(snr / (n_coh_lock ms)) in double, stored as float: within 1e-4 dB of numpy's (a float's spacing is 5e-7 dB there)"""
    from stm32f4_sdr_gps_amd import capi
    lock = np.zeros(9, R.LOCK_DTYPE)
    lock["snr"] = [300.0, 0.5, 1e-30, 3e38, 0.0, -4.0, 75.0, 75.0, np.float32(1.0) / np.float32(3.0)]
    lock["flags"] = [16, 16 | 3, 16, 16, 16, 16, 3, 16, 16]
    lock["last_k"] = [10, 5, 1, 1024, 10, 10, 10, 0, 10]
    for n_coh in (1, 4, 20):
        got = capi.wlock_cn0_dbhz(lock, n_coh)
        want = np.where((lock["snr"] > 0) & (lock["flags"] & 16 != 0) & (lock["last_k"] > 0),
                        10.0 * np.log10(np.maximum(lock["snr"].astype(np.float64), 1e-300) / (n_coh * 0.001)), 0.0)
        assert got.dtype == np.float32 and np.abs(got - want).max() <= 1e-4, (got, want)
        assert (got[[4, 5, 6, 7]] == 0).all() and got.tobytes() == R.cn0_dbhz(lock, n_coh).tobytes()
    lib = capi.load_library()
    out = np.zeros(9, np.float32)
    for args in ((None, 9, 20, out.ctypes.data), (lock.ctypes.data, 9, 20, None), (lock.ctypes.data, 0, 20, out.ctypes.data),
                 (lock.ctypes.data, 9, 0, out.ctypes.data), (lock.ctypes.data, 9, 21, out.ctypes.data)):
        assert lib.gpsx_wlock_cn0_dbhz(*args) == -22
    assert not out.any()


# ---- the scenario on the restatements ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scenario():
    jobs = X.all_jobs()
    out = X.runs(jobs)
    n = len(X.SEEDS)
    return dict(plain=out[:n], rearm=out[n:2 * n], half=out[2 * n:])


def _flags(run):
    return [int(lock["flags"][0]) for lock in run[1]]


def test_scenario_conditions_on_three_seeds(scenario):
    for seed, plain, rearm in zip(X.SEEDS, scenario["plain"], scenario["rearm"]):
        for ch in X.PRESENT:
            run = plain[ch]
            epochs = X._epochs(run)
            there = [e for e in epochs if ch != X.VANISHING or e[0] < X.GONE_AT]
            first_code = [e[0] for e in there if e[6] & R.F_CODE][0]
            first_lock = [e[0] for e in there if e[1]][0]
            first_car = [e[0] for e in there if e[6] & R.F_CARRIER][0]
            print("seed", seed, "channel", ch, "CODE from block", first_code, "LOCKED from", first_lock, "CARRIER from", first_car)
            assert first_code < 300 and first_lock < first_car < X.LOCKED_FROM + 200
            # ... and keep both while the satellite is there
            assert all(e[6] & R.F_CODE for e in there if e[0] >= first_code) and all(e[6] & R.F_CARRIER for e in there if e[0] >= first_car)
        for ch in X.HEALTHY:
            assert not any(f & (R.F_LOST_CODE | R.F_LOST_CARRIER) for f in _flags(plain[ch])), (seed, ch)
            assert int(plain[ch][4]["n_lost_code"][0]) == 0 and int(plain[ch][4]["n_lost_carrier"][0]) == 0
        for ch in range(len(K.SATS), X.N_CH):      # the PRNs that are not there: never CODE, in any epoch
            assert not any(e[6] & (R.F_CODE | R.F_CARRIER) for e in X._epochs(plain[ch])), (seed, ch)
            assert not any(f & R.F_CODE for f in _flags(plain[ch]))
        # the satellite that sets: LOST_CODE in some launch after block 2000, CODE down afterwards
        flags = _flags(plain[X.VANISHING])
        lost = [i for i, f in enumerate(flags) if f & R.F_LOST_CODE]
        assert len(lost) == 1 and X.launches()[lost[0]][0] >= X.GONE_AT and not any(f & R.F_CODE for f in flags[lost[0]:]), (seed, flags)
        assert plain[X.VANISHING][2] == [0, 2, 2, 2, 2, 2]      # without a re-arm the sync loop stays LOCKED on nothing
        # with rearm = 1: back in SEARCH when the launch of the loss ends, the healthy channels byte for byte as without
        got = rearm[X.VANISHING]
        assert _flags(got)[lost[0]] & R.F_REARMED and got[2][lost[0] - 1] == R.SYNC_LOCKED and all(m == R.SYNC_SEARCH for m in got[2][lost[0]:])
        assert int(got[4]["n_rearm"][0]) == 1 and lost[0] + 1 < len(flags)
        after = got[0][lost[0] + 1][:, 0]
        assert (after["flags"] & Y.F_WINDOW).any() and not (after["flags"] & Y.F_LOCKED).any()
        for ch in X.HEALTHY:
            for a, b in zip(plain[ch][0], rearm[ch][0]):
                assert a.tobytes() == b.tobytes()
            assert plain[ch][5].tobytes() == rearm[ch][5].tobytes() and plain[ch][4].tobytes() == rearm[ch][4].tobytes()
        # the observables on the same records: without the re-arm the channel keeps its chain of bits on noise; with it the
        # chain ends in the launch after the loss.  (No channel is VALID within 3000 blocks: a HOW needs 62 bits after bit sync)
        ends = {}
        for name, run in (("plain", plain[X.VANISHING]), ("rearm", got)):
            nav, obs_st = np.zeros(1, N.STATE_DTYPE), np.zeros(1, O.STATE_DTYPE)
            for (at, n), rec in zip(X.launches(), run[0]):
                words, bad = N.run(rec, n, nav, 3)
                obs, bad2 = O.run(rec, n, words, obs_st, 512.0)
                assert not bad and not bad2
            ends[name] = (int(obs["flags"][0]), int(obs_st["n_break"][0]))
        assert ends["plain"][0] & O.F_EDGE and ends["plain"][1] == 0
        assert not ends["rearm"][0] & (O.F_EDGE | O.F_VALID) and ends["rearm"][1] == 1


def test_scenario_measurements(scenario):
    got = X.measure(scenario["plain"], scenario["half"])
    print(got)

    def same(a, b):      # (figures rounded to the table's digits: one unit of the last for a mean that sits on a rounding edge)
        if isinstance(a, dict):
            return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
        return a == b if isinstance(a, (tuple, int)) else abs(a - b) <= 0.0101
    assert same(got, X.MEASURED), (got, X.MEASURED)
    # every threshold sits between what noise and what the satellites give
    assert got["code_noise_max"] < X.CODE_MIN < got["code_present_min"] and got["car_noise_max"] < X.CAR_MIN < got["car_present_min"]
    assert got["snr_noise_max"] < X.SNR_MIN < got["snr_present_min"]
    assert max(got["loss_latency_blocks"]) <= X.LAUNCH


def test_cn0_estimate(scenario):
    """what the estimator reads, per seed, against MEASURED with a margin of three standard deviations of the per-epoch estimates;
    halving the amplitude lowers it by 6 dB within the same margin"""
    full, half = X.MEASURED["cn0_full"], X.MEASURED["cn0_half"]
    for seed, a, b in zip(X.SEEDS, scenario["plain"], scenario["half"]):
        one = X.measure([a], [b])
        print("seed", seed, one["cn0_full"], one["cn0_half"])
        assert abs(one["cn0_full"]["mean"] - full["mean"]) <= 3 * full["sd"] and abs(one["cn0_half"]["mean"] - half["mean"]) <= 3 * half["sd"]
        drop = one["cn0_full"]["mean"] - one["cn0_half"]["mean"]
        assert abs(drop - 20.0 * np.log10(2.0)) <= 3 * max(full["sd"], half["sd"]), (seed, drop)
    # the helper on the launches' records says what the epochs say
    run = scenario["plain"][0][0]
    lock = run[1][3]
    assert R.cn0_dbhz(lock, K.N_COH_LOCK)[0] == np.float32(10.0 * np.log10(float(lock["snr"][0]) / 0.02))
