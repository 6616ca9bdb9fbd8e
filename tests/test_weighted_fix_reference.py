"""The CPU restatement of the weighted path's position fixes (tests/weighted_fix_ref.py, include/gpsx.h gpsx_wfix) against what it can
be held to without a GPU: the library's own pntpos at exactly four satellites, the true receiver under larger skies, the gain from
more satellites under noise, and weighted_obs_ref.pseudoranges bit for bit.  The GPU partner is tests/test_gpu_weighted_fix.py."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import weighted_fix_cases as W
import weighted_fix_ref as F
import weighted_obs_ref as O


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "gpsx.h"
typedef int (*fix_fn)(gpsx_ctx *, const gpsx_wfix_cfg_t *, const gpsx_wobs_t *, const gpsx_weph_t *, const gpsx_wlock_t *, const gpsx_wfix_t *, int,
                      gpsx_wfix_t *, double *);
_Static_assert(__builtin_types_compatible_p(__typeof__(&gpsx_wfix_dev), fix_fn), "the _dev entry point");
_Static_assert(__builtin_types_compatible_p(__typeof__(&gpsx_wfix), fix_fn), "the host entry point");
#define R(f) printf("fix.%s %zu\n", #f, offsetof(gpsx_wfix_t, f))
#define G(f) printf("cfg.%s %zu\n", #f, offsetof(gpsx_wfix_cfg_t, f))
int main(void)
{
  printf("sizeof.fix %zu\nsizeof.cfg %zu\n", sizeof(gpsx_wfix_t), sizeof(gpsx_wfix_cfg_t));
  R(flags); R(n_used); R(n_iter); R(ref_slot); R(used_mask); R(rr); R(dtr_s); R(rx_tow_s); R(geo); R(qr); R(resid_rms_m); R(week); R(reserved);
  G(offset_ms); G(ion); G(ch_per_rx); G(min_sats); G(reserved0); G(reserved1); G(reserved2); G(reserved3);
  printf("flags %u\nversion %d\n", GPSX_WFIX_FIX | GPSX_WFIX_TOO_FEW | GPSX_WFIX_SINGULAR | GPSX_WFIX_NO_CONV | GPSX_WFIX_NONFINITE, GPSX_VERSION);
  return 0;
}
"""


def test_struct_layout_exports_binding_and_kernel_resources():
    """the two structs as a C compiler sees them against the restatement's dtypes and the binding's; both entry points exported, listed
    in ABI_SYMBOLS and bound; exactly one k_wfix in the build, without scratch"""
    with tempfile.TemporaryDirectory(prefix="wfix_layout_") as tmp:
        src, exe = os.path.join(tmp, "layout.c"), os.path.join(tmp, "layout")
        with open(src, "w") as f:
            f.write(LAYOUT_C)
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
        got = {k: int(v) for k, v in (line.split() for line in subprocess.check_output([exe], text=True).splitlines())}
    assert got["sizeof.cfg"] == 96 and got["sizeof.fix"] == 128 and got["flags"] == 31 and got["version"] == 110
    for prefix, dtype in (("fix.", F.FIX_DTYPE), ("cfg.", F.CFG_DTYPE)):
        offsets = {k[len(prefix):]: v for k, v in got.items() if k.startswith(prefix)}
        assert offsets == {name: dtype.fields[name][1] for name in dtype.names}, prefix
    import __graft_entry__ as entry
    from stm32f4_sdr_gps_amd import build, capi
    assert capi.WFIX_DTYPE == F.FIX_DTYPE and capi.WFIX_CFG_DTYPE == F.CFG_DTYPE
    assert (capi.WFIX_FLAG_FIX, capi.WFIX_FLAG_TOO_FEW, capi.WFIX_FLAG_SINGULAR, capi.WFIX_FLAG_NO_CONV, capi.WFIX_FLAG_NONFINITE) == (
        F.F_FIX, F.F_TOO_FEW, F.F_SINGULAR, F.F_NO_CONV, F.F_NONFINITE)
    assert capi.wfix_cfg(68.802, 12, 5, ion=[1, 2, 3, 4, 5, 6, 7, 8]).tobytes() == F.make_cfg(68.802, 12, 5, ion=[1, 2, 3, 4, 5, 6, 7, 8]).tobytes()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", build.LIB], text=True)
    assert {"gpsx_wfix", "gpsx_wfix_dev"} <= {line.split()[-1] for line in syms.splitlines() if line.strip()}
    assert {"gpsx_wfix", "gpsx_wfix_dev"} <= set(entry.ABI_SYMBOLS) and callable(getattr(capi.Engine, "wfix", None))
    lib = capi.load_library()
    assert len(lib.gpsx_wfix.argtypes) == 9 and lib.gpsx_wfix_dev.argtypes is not None
    res = build.check_wfix()
    assert len(res) == 1 and all("k_acq_mx" not in k and "k_track_loop" not in k and v["scratch_bytes"] == 0 for k, v in res.items())


@pytest.fixture(scope="module")
def lib():
    from stm32f4_sdr_gps_amd import capi
    return capi.load_library()


def test_four_satellites_equal_pntpos(lib):
    """(a) 32 four-satellite receivers at the four sites, from the origin and from a warm start 30 km off: rr within 1e-6 m, the
    clock term within 1e-14 s, qr within 1e-5 relative of pntpos through the host glue (tests/test_pvt.py's tolerances for a
    different elimination order); the pseudoranges and rx_tow_s are the helper's bit for bit"""
    recs = [W.receiver(site, 4, seed) for site, seed in W.quartets(32)]
    obs, eph = W.pack(recs, 4)
    cfg = F.make_cfg(W.OFFSET_MS, 4)
    cold, pr = F.run(cfg, obs, eph, 32)
    prev = np.zeros(32, F.FIX_DTYPE)
    prev["flags"] = F.F_FIX
    prev["rr"] = cold["rr"] + np.array([30e3, -20e3, 10e3])
    warm, _ = F.run(cfg, obs, eph, 32, prev=prev)
    for fix, start in ((cold, None), (warm, prev["rr"])):
        assert (fix["flags"] == F.F_FIX).all() and (fix["n_used"] == 4).all() and (fix["used_mask"] == 15).all()
        for r, (o, e) in enumerate(recs):
            want = W.pntpos_fix(lib, o, e, W.OFFSET_MS, None if start is None else start[r])
            assert want is not None
            assert pr[4 * r:4 * r + 4].tobytes() == want["pr"].tobytes() and float(fix["rx_tow_s"][r]) == want["rx_tow_s"]
            assert float(np.abs(fix["rr"][r] - want["rr"]).max()) < 1e-6, (r, fix["rr"][r] - want["rr"])
            assert abs(float(fix["dtr_s"][r]) - want["dtr"]) < 1e-14
            assert np.allclose(fix["qr"][r], want["qr"], rtol=1e-5, atol=0.0)
    assert (warm["n_iter"] < cold["n_iter"]).all()


def _pntpos_subset_errors(lib, n_sats):
    out = []
    for site, seed in W.big_skies(n_sats):
        o, e = W.receiver(site, n_sats, seed)
        for sub in (slice(0, 4), slice(n_sats - 4, n_sats)):
            fix = W.pntpos_fix(lib, o[sub], e[sub], W.OFFSET_MS)
            assert fix is not None
            out.append(W.fix_error(fix, site))
    return out


@pytest.mark.parametrize("n_sats", (5, 8, 12))
def test_larger_skies_are_as_close_as_pntpos_on_four(lib, n_sats):
    """(b) noise-free skies of 5, 8 and 12 satellites over ten receivers each: every satellite used, and the fix no farther from the
    true receiver than twice the largest distance pntpos shows on four-satellite subsets of the same receivers (MEASURED["pntpos_m"])"""
    sub = max(_pntpos_subset_errors(lib, n_sats))
    print("pntpos on four-satellite subsets: largest error", sub, "m")
    assert sub <= W.MEASURED["pntpos_m"] * 1.0000001
    skies = W.big_skies(n_sats)
    obs, eph = W.pack([W.receiver(site, n_sats, seed) for site, seed in skies], n_sats)
    fix, _ = F.run(F.make_cfg(W.OFFSET_MS, n_sats), obs, eph, len(skies))
    assert (fix["flags"] == F.F_FIX).all() and (fix["n_used"] == n_sats).all()
    errors = [W.fix_error(fix[r], site) for r, (site, _) in enumerate(skies)]
    print(n_sats, "satellites: errors", np.round(errors, 4), "rms residuals", np.round(fix["resid_rms_m"], 4))
    assert max(errors) <= W.BOUNDS["noise_free_m"], errors


def test_twelve_noisy_satellites_beat_four():
    """(c) 3 m of seeded Gaussian pseudorange noise over 64 receivers: the median error with all twelve satellites is below the
    median with each receiver's first four (more rows can only shrink the covariance); the two medians are MEASURED's"""
    rx = W.noisy()
    obs12, eph12 = W.pack([(o, e) for _, o, e in rx], 12)
    obs4, eph4 = W.pack([(o[:4], e[:4]) for _, o, e in rx], 4)
    fix12, _ = F.run(F.make_cfg(W.OFFSET_MS, 12), obs12, eph12, len(rx))
    fix4, _ = F.run(F.make_cfg(W.OFFSET_MS, 4), obs4, eph4, len(rx))
    assert (fix12["flags"] == F.F_FIX).all() and (fix4["flags"] == F.F_FIX).all() and (fix12["n_used"] == 12).all()
    m12 = float(np.median([W.fix_error(fix12[r], rx[r][0]) for r in range(len(rx))]))
    m4 = float(np.median([W.fix_error(fix4[r], rx[r][0]) for r in range(len(rx))]))
    print("median error: twelve satellites", m12, "m, the first four", m4, "m")
    assert m12 < m4
    assert abs(m12 - W.MEASURED["noise_median_m"][0]) < 0.01 and abs(m4 - W.MEASURED["noise_median_m"][1]) < 0.01


def test_pseudoranges_over_a_masked_subset_are_the_obs_restatement_bit_for_bit():
    """(d) pr_m, ref_slot and rx_tow_s over the usable slots of weighted_fix_cases.launch_case's mixes equal
    weighted_obs_ref.pseudoranges on that subset (the others marked not VALID), bit for bit"""
    for ch, n_rx in ((5, 17), (12, 17), (33, 17)):
        case = W.launch_case(ch, n_rx)
        fix, pr = F.run(F.make_cfg(W.OFFSET_MS, ch), case["obs"], case["eph"], n_rx, lock=case["lock"])
        obs, eph = case["obs"].reshape(n_rx, ch), case["eph"].reshape(n_rx, ch)
        usable = ((obs["flags"] & O.F_VALID) != 0) & ((eph["flags"] & 1) != 0)
        if case["lock"] is not None:
            usable &= (case["lock"].reshape(n_rx, ch)["flags"] & 1) != 0
        assert not usable.all() and usable.any()
        for r in range(n_rx):
            masked = obs[r].copy()
            masked["flags"][~usable[r]] &= ~np.uint32(O.F_VALID)
            want_pr, want_rx, count = O.pseudoranges(masked, W.OFFSET_MS)
            assert count == int(usable[r].sum())
            assert pr[r * ch:(r + 1) * ch].tobytes() == np.asarray(want_pr, np.float64).tobytes() and float(fix["rx_tow_s"][r]) == float(want_rx)
            valid = np.flatnonzero(usable[r])
            if len(valid):      # the reference slot: the smallest pseudorange, the first of equals
                assert int(fix["ref_slot"][r]) == int(valid[np.argmin(want_pr[valid])])
            else:
                assert int(fix["ref_slot"][r]) == -1
