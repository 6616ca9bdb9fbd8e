"""The CPU restatement of the weighted path's fault detection and exclusion (tests/weighted_fde_ref.py, include/gpsx.h gpsx_wfde) against
what it can be held to without a GPU: the structs as a C compiler sees them, the plain fix it must reduce to, the seeded tables of
faulty, clean and millisecond-shifted receivers (tests/weighted_fde_cases.py), and the margins that let the GPU partner,
tests/test_gpu_weighted_fde.py, demand equal decisions."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import weighted_fde_cases as X
import weighted_fde_ref as D
import weighted_fix_cases as W
import weighted_fix_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "gpsx.h"
typedef int (*fde_fn)(gpsx_ctx *, const gpsx_wfde_cfg_t *, const gpsx_wobs_t *, const gpsx_weph_t *, const gpsx_wlock_t *, const gpsx_wfix_t *, int,
                      gpsx_wfix_t *, gpsx_wfde_t *, double *);
_Static_assert(__builtin_types_compatible_p(__typeof__(&gpsx_wfde_dev), fde_fn), "the _dev entry point");
_Static_assert(__builtin_types_compatible_p(__typeof__(&gpsx_wfde), fde_fn), "the host entry point");
#define R(f) printf("fde.%s %zu\n", #f, offsetof(gpsx_wfde_t, f))
#define G(f) printf("cfg.%s %zu\n", #f, offsetof(gpsx_wfde_cfg_t, f))
int main(void)
{
  printf("sizeof.fde %zu\nsizeof.cfg %zu\nsizeof.fixcfg %zu\n", sizeof(gpsx_wfde_t), sizeof(gpsx_wfde_cfg_t), sizeof(gpsx_wfix_cfg_t));
  R(flags); R(n_rounds); R(n_excluded); R(dof); R(excl_mask); R(plus_mask); R(minus_mask); R(t_stat); R(t_limit); R(reserved);
  G(fix); G(z_global); G(max_excl); G(repair); G(reserved);
  printf("flag.PASSED %u\nflag.UNCHECKED %u\nflag.FAULT %u\nflag.NOFIX %u\nflag.EXCLUDED %u\nflag.REPAIRED %u\nflag.UNRESOLVED %u\n", GPSX_WFDE_PASSED,
         GPSX_WFDE_UNCHECKED, GPSX_WFDE_FAULT, GPSX_WFDE_NOFIX, GPSX_WFDE_EXCLUDED, GPSX_WFDE_REPAIRED, GPSX_WFDE_UNRESOLVED);
  printf("version %d\n", GPSX_VERSION);
  return 0;
}
"""


def test_struct_layout_exports_binding_and_kernel_resources():
    """the two structs and the seven flags as a C compiler sees them against the restatement's and the binding's; both entry points
    exported, listed in ABI_SYMBOLS and bound; exactly one k_wfde in the build, without scratch; GPSX_VERSION still 110"""
    with tempfile.TemporaryDirectory(prefix="wfde_layout_") as tmp:
        src, exe = os.path.join(tmp, "layout.c"), os.path.join(tmp, "layout")
        with open(src, "w") as f:
            f.write(LAYOUT_C)
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
        got = {k: int(v) for k, v in (line.split() for line in subprocess.check_output([exe], text=True).splitlines())}
    assert got["sizeof.cfg"] == 128 and got["sizeof.fde"] == 64 and got["sizeof.fixcfg"] == 96 and got["version"] == 110
    for prefix, dtype in (("fde.", D.FDE_DTYPE), ("cfg.", D.CFG_DTYPE)):
        offsets = {k[len(prefix):]: v for k, v in got.items() if k.startswith(prefix)}
        assert offsets == {name: dtype.fields[name][1] for name in dtype.names}, prefix
    flags = {k[5:]: v for k, v in got.items() if k.startswith("flag.")}
    assert flags == {name: getattr(D, name) for name in ("PASSED", "UNCHECKED", "FAULT", "NOFIX", "EXCLUDED", "REPAIRED", "UNRESOLVED")}
    assert sorted(flags.values()) == [1, 2, 4, 8, 16, 32, 64]
    import __graft_entry__ as entry
    from stm32f4_sdr_gps_amd import build, capi
    assert capi.WFDE_DTYPE == D.FDE_DTYPE and capi.WFDE_CFG_DTYPE == D.CFG_DTYPE
    assert (capi.WFDE_FLAG_PASSED, capi.WFDE_FLAG_UNCHECKED, capi.WFDE_FLAG_FAULT, capi.WFDE_FLAG_NOFIX, capi.WFDE_FLAG_EXCLUDED, capi.WFDE_FLAG_REPAIRED,
            capi.WFDE_FLAG_UNRESOLVED) == (D.PASSED, D.UNCHECKED, D.FAULT, D.NOFIX, D.EXCLUDED, D.REPAIRED, D.UNRESOLVED)
    assert capi.wfde_cfg(68.802, 12, 5, [1, 2, 3, 4, 5, 6, 7, 8], 2.5, 3, False).tobytes() == D.make_cfg(68.802, 12, 5, [1, 2, 3, 4, 5, 6, 7, 8], 2.5, 3, 0).tobytes()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", build.LIB], text=True)
    assert {"gpsx_wfde", "gpsx_wfde_dev"} <= {line.split()[-1] for line in syms.splitlines() if line.strip()}
    assert {"gpsx_wfde", "gpsx_wfde_dev"} <= set(entry.ABI_SYMBOLS) and callable(getattr(capi.Engine, "wfde", None))
    lib = capi.load_library()
    assert len(lib.gpsx_wfde.argtypes) == 10 and len(lib.gpsx_wfde_dev.argtypes) == 10
    assert lib.gpsx_version() == 110
    res = build.check_wfde()
    assert len(res) == 1 and all("k_wfde" in k and v["scratch_bytes"] == 0 for k, v in res.items())
    assert len(build.check_wfix()) == 1


@pytest.mark.parametrize("ch,n_rx", ((5, 17), (12, 17), (33, 17), (4, 8)))
def test_without_repair_and_exclusion_the_records_are_the_plain_fix(ch, n_rx):
    """repair = 0, max_excl = 0: the restatement's fix records and pseudoranges equal weighted_fix_ref.run's byte for byte, on
    weighted_fix_cases' slot mixes (unfixable receivers included) and on this module's launches (AMBIGUOUS slots included, which
    then are UNRESOLVED); four usable slots: UNCHECKED"""
    plain = W.launch_case(ch, n_rx)
    ours = X.launch_case(ch, 17 if ch != 4 else 67)
    for obs, eph, lock, n in ((plain["obs"], plain["eph"], plain["lock"], n_rx), (ours["obs"], ours["eph"], ours["lock"], len(ours["kinds"]))):
        want, want_pr = F.run(F.make_cfg(W.OFFSET_MS, ch), obs, eph, n, lock=lock)
        fix, fde, pr, _ = D.run(X.cfg(ch, max_excl=0, repair=0), obs, eph, n, lock=lock)
        assert fix.tobytes() == want.tobytes() and pr.tobytes() == want_pr.tobytes()
        fixed = (want["flags"] & F.F_FIX) != 0
        assert (((fde["flags"] & D.NOFIX) != 0) == ~fixed).all() and (fde["n_rounds"] == 1).all() and not fde["excl_mask"].any()
        assert ((fde["flags"][fixed & (want["n_used"] == 4)] & D.VERDICTS) == D.UNCHECKED).all()
        assert (np.bincount(fde["flags"] & D.VERDICTS, minlength=9)[[1, 2, 4, 8]].sum()) == n      # exactly one verdict each
    if ch == 4:
        assert ((ours["want"][1]["flags"] & D.VERDICTS) == D.UNCHECKED).all()


def test_the_isolation_table():
    """216 seeded draws (4 sites x 6 / 8 / 12 satellites x six skies x faults of 150 / 1000 / -400 m over 3 m of noise): the draws in
    which the restatement excludes exactly the injected slot with every margin >= 1e-6 number at least 150 (the prototype of the
    rule kept 208), every n_sats and every site is among them, and in each the error after exclusion is below that of the plain fix"""
    draws, kept = X.isolation_draws(), X.isolation_kept()
    print("kept", len(kept), "of", len(draws))
    assert len(draws) == 216 and len(kept) >= 150
    assert {d["n"] for d, _, _ in kept} == set(X.N_SATS) and {d["site"] for d, _, _ in kept} == set(W.SITES)
    after = []
    for d, fix, fde in kept:
        plain, _ = F.run(F.make_cfg(W.OFFSET_MS, d["n"]), d["obs"], d["eph"], 1)
        assert int(fde["flags"]) & D.EXCLUDED and int(fde["n_excluded"]) == 1 and int(fde["n_rounds"]) == 2
        after.append(W.fix_error(fix, d["site"]))
        assert after[-1] < W.fix_error(plain[0], d["site"]), (d["site"], d["n"], d["seed0"], d["fault"])
    print("median error after exclusion", float(np.median(after)), "m")


def test_clean_receivers_raise_no_alarm():
    """48 clean receivers under 3 m of noise at z = 3.09: PASSED, nothing excluded, one round"""
    res = X.run_each(X.clean_draws())
    print("largest T / limit", max(float(fde["t_stat"] / fde["t_limit"]) for _, fde, _ in res))
    for _, fde, m in res:
        assert int(fde["flags"]) == D.PASSED and int(fde["excl_mask"]) == 0 and int(fde["n_rounds"]) == 1
        assert D.min_margin(m) >= D.MARGIN


def test_every_wrong_millisecond_is_repaired_to_the_injected_sign():
    """32 receivers with one or two slots moved by +-1 ms and flagged AMBIGUOUS: the plus and minus masks undo what was injected,
    nothing is excluded, and the fix is as good as a clean receiver's"""
    draws = X.ms_draws()
    for d, (fix, fde, m) in zip(draws, X.run_each(draws)):
        assert (int(fde["plus_mask"]), int(fde["minus_mask"])) == X.ms_masks(d), d["ms"]
        assert int(fde["flags"]) == D.PASSED | D.REPAIRED and int(fde["n_rounds"]) == 2
        assert W.fix_error(fix, d["site"]) < 30.0 and D.min_margin(m) >= D.MARGIN
        assert all(f < 1e-3 for f in m["repair"])      # a wrong millisecond is a whole one: 300 m would be 1e-3 of it


@pytest.mark.parametrize("ch,n_rx", X.SHAPES)
def test_every_launch_of_the_gpu_tests_has_its_margins(ch, n_rx):
    """every receiver of every launch that tests/test_gpu_weighted_fde.py compares decision for decision: all margins >= 1e-6; the
    kinds do what their names say; exactly one verdict per receiver"""
    case = X.launch_case(ch, n_rx)
    fix, fde, _ = case["want"]
    for r, m in enumerate(case["margins"]):
        assert D.min_margin(m) >= D.MARGIN, (r, case["kinds"][r], m)
    verdict = fde["flags"] & D.VERDICTS
    assert np.isin(verdict, (D.PASSED, D.UNCHECKED, D.FAULT, D.NOFIX)).all()
    assert ((verdict == D.NOFIX) == ((fix["flags"] & F.F_FIX) == 0)).all()
    assert (fde["n_excluded"] == [bin(int(v)).count("1") for v in fde["excl_mask"]]).all()
    for r, kind in enumerate(case["kinds"]):
        f, rounds = int(fde["flags"][r]), int(fde["n_rounds"][r])
        if ch == 4:
            assert f & D.UNCHECKED and rounds == 1
        elif kind == "clean":
            assert f == D.PASSED and rounds == 1
        elif kind == "one_fault" and ch != 5:
            assert f == D.PASSED | D.EXCLUDED and rounds == 2
        elif kind == "one_fault":
            assert f == D.FAULT and rounds == 1
        elif kind in ("ambig_minus", "ambig_two", "ambig_latest"):
            assert f == D.PASSED | D.REPAIRED and rounds == 2
        elif kind == "fault_and_ambig":
            assert f == D.PASSED | D.REPAIRED | D.EXCLUDED and rounds == 3
        elif kind == "ambig_3ms":
            assert f == D.PASSED | D.EXCLUDED and rounds == 2 and int(fde["plus_mask"][r] | fde["minus_mask"][r]) == 0
        elif kind == "few_unambiguous":
            assert f == D.PASSED | D.UNRESOLVED and rounds == 1
        elif kind == "four_usable":
            assert f == (D.UNCHECKED if ch != 5 else D.NOFIX) and rounds == 1
        elif kind == "too_few":
            assert f == D.NOFIX and int(fix["flags"][r]) == F.F_TOO_FEW
        elif kind == "duplicate":
            assert f == D.NOFIX and int(fix["flags"][r]) == (F.F_SINGULAR if ch != 5 else F.F_TOO_FEW)
        elif kind == "three_faults":
            assert f == D.FAULT | D.EXCLUDED and rounds == 3 and int(fde["n_excluded"][r]) == 2
        elif kind == "lock_masked":      # (ch_per_rx 5: four slots are left under min_sats 5)
            assert f == (D.PASSED if ch != 5 else D.NOFIX) and rounds == 1
    if n_rx == 67 and ch >= 8:
        assert set(case["kinds"]) == set(X.KINDS) and {1, 2, 3} <= set(fde["n_rounds"].tolist())


def test_the_smoke_fixture_is_what_the_cases_module_builds():
    gold = np.load(os.path.join(ROOT, "tests", "golden", "wfde_smoke.npz"))
    want = X.smoke_case()
    assert set(gold.files) == set(want)
    for k, v in want.items():      # (what lies behind a sine -- the code phases, the fix -- to its accuracy, everything else to the bit)
        if k == "obs":
            assert (gold[k]["tx_ms"] == v["tx_ms"]).all() and (gold[k]["flags"] == v["flags"]).all()
            assert np.abs(gold[k]["code_phase_fine"] - v["code_phase_fine"]).max() < 1e-2
        elif k == "rr":
            assert np.abs(gold[k] - v).max() < 1e-4
        else:
            assert np.asarray(v).tobytes() == gold[k].tobytes(), k
    assert int(gold["excl_mask"]) == 1 << 5 and int(gold["minus_mask"]) == 1 << 2 and int(gold["plus_mask"]) == 0
    assert int(gold["flags"]) == D.PASSED | D.EXCLUDED | D.REPAIRED and int(gold["n_rounds"]) == 3
    assert np.linalg.norm(gold["rr"] - gold["truth"]) < 30.0
