"""The navigation filter's C ABI without a GPU (include/gpsx.h gpsx_wkf): the three structs and the flags as a C compiler sees them
against the restatement's and the binding's dtypes, both entry points exported, listed and bound, the kernel's resources in the build,
and the smoke fixture.  Every test here needs the library, the binding and the build: they fail where gpsx_wkf does not exist."""
import os
import subprocess
import tempfile

import numpy as np

import weighted_kf_cases as K
import weighted_kf_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "gpsx.h"
typedef int (*kf_fn)(gpsx_ctx *, const gpsx_wkf_cfg_t *, const gpsx_wobs_t *, const gpsx_weph_t *, const gpsx_wlock_t *, const gpsx_wfix_t *,
                     const gpsx_wvel_t *, int, int, gpsx_wkf_state_t *, gpsx_wkf_t *);
_Static_assert(__builtin_types_compatible_p(__typeof__(&gpsx_wkf_dev), kf_fn), "the _dev entry point");
_Static_assert(__builtin_types_compatible_p(__typeof__(&gpsx_wkf), kf_fn), "the host entry point");
#define R(f) printf("kf.%s %zu\n", #f, offsetof(gpsx_wkf_t, f))
#define S(f) printf("state.%s %zu\n", #f, offsetof(gpsx_wkf_state_t, f))
#define G(f) printf("cfg.%s %zu\n", #f, offsetof(gpsx_wkf_cfg_t, f))
int main(void)
{
  printf("sizeof.kf %zu\nsizeof.state %zu\nsizeof.cfg %zu\n", sizeof(gpsx_wkf_t), sizeof(gpsx_wkf_state_t), sizeof(gpsx_wkf_cfg_t));
  R(flags); R(n_pr); R(n_dop); R(n_starved); R(pr_mask); R(dop_mask); R(rej_pr_mask); R(rej_dop_mask); R(plus_mask); R(minus_mask); R(rr); R(clk_m);
  R(vel); R(cdrift_mps); R(geo); R(enu); R(sigma); R(nis_pr); R(nis_dop); R(rcv_ms); R(week); R(reserved);
  S(x); S(P); S(rcv_ms); S(week); S(flags); S(n_starved); S(n_init); S(n_lost); S(reserved);
  G(ion); G(mps_per_hz); G(sig_pr_m); G(sig_dop_mps); G(gate); G(q_acc); G(q_clk_f); G(q_clk_g); G(p0_pos); G(p0_clk); G(p0_vel); G(p0_drift);
  G(ch_per_rx); G(max_coast); G(reserved);
  printf("flag.F_INIT %u\nflag.F_NOT_INIT %u\nflag.F_UPDATED %u\nflag.F_COAST %u\nflag.F_LOST %u\nflag.F_BAD %u\nflag.F_REPAIRED %u\n"
         "flag.F_REJECTED %u\nflag.F_STEERED %u\nflag.S_INIT %u\n", GPSX_WKF_INIT, GPSX_WKF_NOT_INIT, GPSX_WKF_UPDATED, GPSX_WKF_COAST, GPSX_WKF_LOST,
         GPSX_WKF_BAD, GPSX_WKF_REPAIRED, GPSX_WKF_REJECTED, GPSX_WKF_STEERED, GPSX_WKF_STATE_INIT);
  printf("version %d\n", GPSX_VERSION);
  return 0;
}
"""
FLAGS = ("F_INIT", "F_NOT_INIT", "F_UPDATED", "F_COAST", "F_LOST", "F_BAD", "F_REPAIRED", "F_REJECTED", "F_STEERED", "S_INIT")


def test_struct_layout_against_the_dtypes():
    with tempfile.TemporaryDirectory(prefix="wkf_layout_") as tmp:
        src, exe = os.path.join(tmp, "layout.c"), os.path.join(tmp, "layout")
        with open(src, "w") as f:
            f.write(LAYOUT_C)
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
        got = {k: int(v) for k, v in (line.split() for line in subprocess.check_output([exe], text=True).splitlines())}
    assert got["sizeof.cfg"] == 176 and got["sizeof.state"] == 384 and got["sizeof.kf"] == 240 and got["version"] == 110
    assert all(got[k] % 16 == 0 for k in ("sizeof.cfg", "sizeof.state", "sizeof.kf"))
    for prefix, dtype in (("kf.", R.KF_DTYPE), ("state.", R.STATE_DTYPE), ("cfg.", R.CFG_DTYPE)):
        offsets = {k[len(prefix):]: v for k, v in got.items() if k.startswith(prefix)}
        assert offsets == {name: dtype.fields[name][1] for name in dtype.names}, prefix
    flags = {k[5:]: v for k, v in got.items() if k.startswith("flag.")}
    assert flags == {name: getattr(R, name) for name in FLAGS}
    assert sorted(v for k, v in flags.items() if k != "S_INIT") == [1, 2, 4, 8, 16, 32, 64, 128, 256]
    from stm32f4_sdr_gps_amd import capi
    assert capi.WKF_DTYPE == R.KF_DTYPE and capi.WKF_STATE_DTYPE == R.STATE_DTYPE and capi.WKF_CFG_DTYPE == R.CFG_DTYPE
    assert (capi.WKF_FLAG_INIT, capi.WKF_FLAG_NOT_INIT, capi.WKF_FLAG_UPDATED, capi.WKF_FLAG_COAST, capi.WKF_FLAG_LOST, capi.WKF_FLAG_BAD,
            capi.WKF_FLAG_REPAIRED, capi.WKF_FLAG_REJECTED, capi.WKF_FLAG_STEERED, capi.WKF_STATE_INIT) == tuple(getattr(R, name) for name in FLAGS)
    kw = dict(mps_per_hz=0.25, sig_pr_m=2.0, sig_dop_mps=0.3, gate=4.0, q_acc=0.5, q_clk_f=0.1, q_clk_g=0.2, p0=(1.0, 2.0, 3.0, 4.0), max_coast=7,
              ion=np.arange(1.0, 9.0))
    assert capi.wkf_cfg(12, **kw).tobytes() == R.make_cfg(12, **kw).tobytes() and K.cfg(8).tobytes() == R.make_cfg(8).tobytes()


def test_symbols_binding_and_kernel_resources():
    """both entry points exported, listed in ABI_SYMBOLS and bound; exactly one k_wkf in the build, without scratch and without LDS;
    k_wfix, k_wfde and k_wvel still there; GPSX_VERSION still 110"""
    import __graft_entry__ as entry
    from stm32f4_sdr_gps_amd import build, capi
    syms = subprocess.check_output(["nm", "-D", "--defined-only", build.LIB], text=True)
    assert {"gpsx_wkf", "gpsx_wkf_dev"} <= {line.split()[-1] for line in syms.splitlines() if line.strip()}
    assert {"gpsx_wkf", "gpsx_wkf_dev"} <= set(entry.ABI_SYMBOLS) and callable(getattr(capi.Engine, "wkf", None))
    lib = capi.load_library()
    assert len(lib.gpsx_wkf.argtypes) == 11 and len(lib.gpsx_wkf_dev.argtypes) == 11 and lib.gpsx_version() == 110
    res = build.check_wkf()
    print(res)
    assert len(res) == 1 and all("k_wkf" in k and v["scratch_bytes"] == 0 and v["lds_bytes"] == 0 for k, v in res.items())
    assert len(build.check_wfix()) == 1 and len(build.check_wfde()) == 1 and len(build.check_wvel()) == 1


def test_smoke_fixture_is_the_cases_modules():
    """tests/golden/wkf_smoke.npz holds weighted_kf_cases.smoke_case() bit for bit, and that receiver's last record is near what was
    injected"""
    gold = np.load(os.path.join(ROOT, "tests", "golden", "wkf_smoke.npz"))
    want = K.smoke_case()
    assert sorted(gold.files) == sorted(want)
    for k, v in want.items():
        assert np.asarray(gold[k]).tobytes() == np.asarray(v).tobytes() and np.asarray(gold[k]).dtype == np.asarray(v).dtype, k
    assert np.linalg.norm(gold["rr"] - gold["truth_rr"]) < 0.5 and np.linalg.norm(gold["vel_out"] - gold["truth_vel"]) < 0.01
    assert abs(float(gold["cdrift_mps"]) - float(gold["truth_cdrift"])) < 0.01
