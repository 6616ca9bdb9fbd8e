"""The CPU restatement of the weighted path's velocity fixes (tests/weighted_vel_ref.py, include/gpsx.h gpsx_wvel) against what it can
be held to without a GPU: the structs as a C compiler sees them, the analytic satellite velocity against difference quotients of the
orbit, velocities and clock drifts injected through Dopplers that were fabricated from physics (tests/weighted_vel_cases.py), and the
margins that let the GPU partner, tests/test_gpu_weighted_vel.py, demand equal decisions.

The first and the last test need the library, the binding and the build (they fail where gpsx_wvel does not exist); the others hold
the restatement alone and need neither."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import pvt_chain as pc
import weighted_fix_cases as W
import weighted_vel_cases as K
import weighted_vel_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "gpsx.h"
typedef int (*vel_fn)(gpsx_ctx *, const gpsx_wvel_cfg_t *, const gpsx_wobs_t *, const gpsx_weph_t *, const gpsx_wlock_t *, const gpsx_wfix_t *, int,
                      gpsx_wvel_t *);
_Static_assert(__builtin_types_compatible_p(__typeof__(&gpsx_wvel_dev), vel_fn), "the _dev entry point");
_Static_assert(__builtin_types_compatible_p(__typeof__(&gpsx_wvel), vel_fn), "the host entry point");
#define R(f) printf("vel.%s %zu\n", #f, offsetof(gpsx_wvel_t, f))
#define G(f) printf("cfg.%s %zu\n", #f, offsetof(gpsx_wvel_cfg_t, f))
int main(void)
{
  printf("sizeof.vel %zu\nsizeof.cfg %zu\n", sizeof(gpsx_wvel_t), sizeof(gpsx_wvel_cfg_t));
  R(flags); R(n_used); R(used_mask); R(vel); R(drift_s_s); R(enu); R(qv); R(resid_rms_mps); R(reserved);
  G(mps_per_hz); G(ch_per_rx); G(min_sats); G(reserved);
  printf("flag.F_VEL %u\nflag.F_NO_FIX %u\nflag.F_TOO_FEW %u\nflag.F_SINGULAR %u\nflag.F_NONFINITE %u\n", GPSX_WVEL_VEL, GPSX_WVEL_NO_FIX,
         GPSX_WVEL_TOO_FEW, GPSX_WVEL_SINGULAR, GPSX_WVEL_NONFINITE);
  printf("version %d\nl1ca_ok %d\ncarrier %u\n", GPSX_VERSION, GPSX_WVEL_L1CA == -299792458.0 / 1575.42e6, GPSX_WLOCK_CARRIER);
  printf("wloop_ok %d\n", GPSX_WVEL_L1CA_WLOOP == -299792458.0 / 1575.42e6 * 1022.0 / 1023.0 && GPSX_WVEL_L1CA_WLOOP == %.17g);
  return 0;
}
"""


def test_struct_layout_exports_binding_and_kernel_resources():
    """(needs the library) the two structs, the five flags and GPSX_WVEL_L1CA as a C compiler sees them against the restatement's and the
    binding's; both entry points exported, listed in ABI_SYMBOLS and bound; exactly one k_wvel in the build, without scratch and
    without LDS; k_wfix and k_wfde still there; GPSX_VERSION still 110"""
    with tempfile.TemporaryDirectory(prefix="wvel_layout_") as tmp:
        src, exe = os.path.join(tmp, "layout.c"), os.path.join(tmp, "layout")
        with open(src, "w") as f:
            f.write(LAYOUT_C.replace("%.17g", repr(V.L1CA_WLOOP)))      # (the restatement's double, to the bit)
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
        got = {k: int(v) for k, v in (line.split() for line in subprocess.check_output([exe], text=True).splitlines())}
    assert got["sizeof.cfg"] == 32 and got["sizeof.vel"] == 112 and got["version"] == 110 and got["l1ca_ok"] == 1 and got["wloop_ok"] == 1 and got["carrier"] == V.LOCK_CARRIER
    for prefix, dtype in (("vel.", V.VEL_DTYPE), ("cfg.", V.CFG_DTYPE)):
        offsets = {k[len(prefix):]: v for k, v in got.items() if k.startswith(prefix)}
        assert offsets == {name: dtype.fields[name][1] for name in dtype.names}, prefix
    flags = {k[5:]: v for k, v in got.items() if k.startswith("flag.")}
    assert flags == {name: getattr(V, name) for name in ("F_VEL", "F_NO_FIX", "F_TOO_FEW", "F_SINGULAR", "F_NONFINITE")}
    assert sorted(flags.values()) == [1, 2, 4, 8, 16]
    import __graft_entry__ as entry
    from stm32f4_sdr_gps_amd import build, capi
    assert capi.WVEL_DTYPE == V.VEL_DTYPE and capi.WVEL_CFG_DTYPE == V.CFG_DTYPE and capi.WVEL_L1CA == V.L1CA and capi.WVEL_L1CA_WLOOP == V.L1CA_WLOOP
    assert (capi.WVEL_FLAG_VEL, capi.WVEL_FLAG_NO_FIX, capi.WVEL_FLAG_TOO_FEW, capi.WVEL_FLAG_SINGULAR, capi.WVEL_FLAG_NONFINITE) == (
        V.F_VEL, V.F_NO_FIX, V.F_TOO_FEW, V.F_SINGULAR, V.F_NONFINITE)
    assert capi.wvel_cfg(12, 5, 0.25).tobytes() == V.make_cfg(12, 5, 0.25).tobytes() and K.cfg(8).tobytes() == V.make_cfg(8).tobytes()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", build.LIB], text=True)
    assert {"gpsx_wvel", "gpsx_wvel_dev"} <= {line.split()[-1] for line in syms.splitlines() if line.strip()}
    assert {"gpsx_wvel", "gpsx_wvel_dev"} <= set(entry.ABI_SYMBOLS) and callable(getattr(capi.Engine, "wvel", None))
    lib = capi.load_library()
    assert len(lib.gpsx_wvel.argtypes) == 8 and len(lib.gpsx_wvel_dev.argtypes) == 8
    assert lib.gpsx_version() == 110
    res = build.check_wvel()
    print(res)
    assert len(res) == 1 and all("k_wvel" in k and v["scratch_bytes"] == 0 and v["lds_bytes"] == 0 for k, v in res.items())
    assert len(build.check_wfix()) == 1 and len(build.check_wfde()) == 1


def test_satellite_velocity_and_clock_rate_against_central_differences():
    """step 2's analytic velocity and clock rate against (f(t + h) - f(t - h)) / 2 h, h = 0.5 s, of pvt_chain.sat_state's position and
    clock at the restatement's own transmit time, over every satellite of every sky that truth_draws() uses; the position itself
    against sat_state's.  Bounds: 2 x MEASURED"""
    worst = {"pos_m": 0.0, "sat_vel_mps": 0.0, "sat_clock_rate": 0.0}
    h = 0.5
    for site in sorted(W.SITES):
        k = sorted(W.SITES).index(site)
        for n in K.N_SATS:
            obs, eph = K.receiver(site, n, 3 * k)
            sat, ps, vs, rate, t = V.satellites(eph, obs, np.ones(n, bool))
            assert sat.all()
            for j, (_, row) in enumerate(W.sky(site, n, 3 * k)):
                pos, dts = pc.sat_state(row, np.array([t[j] - h, t[j], t[j] + h]))
                worst["pos_m"] = max(worst["pos_m"], float(np.abs(ps[j] - pos[1]).max()))
                worst["sat_vel_mps"] = max(worst["sat_vel_mps"], float(np.abs(vs[j] - (pos[2] - pos[0]) / (2 * h)).max()))
                worst["sat_clock_rate"] = max(worst["sat_clock_rate"], abs(float(rate[j]) - float(dts[2] - dts[0]) / (2 * h)))
    print(worst)
    assert worst["pos_m"] <= 1e-6      # (the same formulas on the same numbers: nanometres of libm order)
    assert worst["sat_vel_mps"] <= 2.0 * K.MEASURED["sat_vel_mps"] and worst["sat_clock_rate"] <= 2.0 * K.MEASURED["sat_clock_rate"]


def test_injected_truth_is_recovered():
    """144 receivers (four sites x 5 / 8 / 12 satellites x 0, 36 m/s, 300 m/s, 7.5 km/s x drifts of 0 and +- 1e-6) whose Dopplers were
    fabricated from the travel time's own derivative: every one gets VEL with all its satellites, and the largest errors in velocity
    and c x drift stay within 2 x MEASURED (which says what they are made of); enu is vel rotated: the same length, and up = the
    radial component at a site"""
    draws = K.truth_draws()
    got = K.run_each(draws)
    assert len(draws) == 144 and all(int(g["flags"]) == V.F_VEL and int(g["n_used"]) == d["n"] and int(g["used_mask"]) == (1 << d["n"]) - 1
                                     for g, d in zip(got, draws))
    speed = np.array([np.linalg.norm(d["v"]) for d in draws])
    ev = np.array([np.linalg.norm(g["vel"] - d["v"]) for g, d in zip(got, draws)])
    ed = np.array([abs(float(g["drift_s_s"]) - d["drift"]) * V.C_LIGHT for g, d in zip(got, draws)])
    for s in sorted(set(speed.round())):
        print("speed", s, "m/s: velocity error", ev[speed.round() == s].max(), "m/s, c drift error", ed[speed.round() == s].max(), "m/s, largest rms",
              max(float(g["resid_rms_mps"]) for g, sp in zip(got, speed) if round(sp) == s))
    print("largest", ev.max(), ed.max(), "up to 300 m/s", ev[speed < 1000.0].max())
    assert ev.max() <= 2.0 * K.MEASURED["truth_vel_mps"] and ed.max() <= 2.0 * K.MEASURED["truth_cdrift_mps"]
    assert ev[speed < 1000.0].max() <= 2.0 * K.MEASURED["truth_slow_vel_mps"]
    for g, d in zip(got, draws):
        assert abs(np.linalg.norm(g["enu"]) - np.linalg.norm(g["vel"])) <= 1e-9 * max(1.0, float(np.linalg.norm(g["vel"])))
        lat, lon = d["fix"]["geo"][0, 0], d["fix"]["geo"][0, 1]
        normal = np.array([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)])
        assert abs(float(g["enu"][2]) - float(normal @ g["vel"])) <= 1e-9 * max(1.0, float(np.linalg.norm(g["vel"])))


def test_negated_scale_on_negated_dopplers_gives_the_same_bytes():
    """mps_per_hz = -GPSX_WVEL_L1CA on Dopplers of the other sign convention: the product is the same double, so are the records"""
    draws = K.truth_draws()[::7]
    plain, other = K.run_each(draws), K.run_each(draws, mps_per_hz=-V.L1CA, negate=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(plain, other))


def test_the_weeks_end_is_folded():
    """observables a whole week earlier or later on the same records (t_sv - toes beyond +- 302 400 s) give the satellites back within
    the round-off of the larger argument, and the same rows"""
    d = K.truth_draws()[17]
    base = K.run_each([d])[0]
    for weeks in (-1, 1):
        obs = d["obs"].copy()
        obs["tx_ms"] += weeks * 604_800_000
        got = K.run_each([dict(d, obs=obs)])[0]
        assert int(got["flags"]) == V.F_VEL and int(got["used_mask"]) == int(base["used_mask"])
        assert np.abs(got["vel"] - base["vel"]).max() <= 1e-6 and abs(float(got["drift_s_s"] - base["drift_s_s"])) * V.C_LIGHT <= 1e-6


@pytest.mark.parametrize("ch", K.SHAPES_CH)
def test_every_gpu_launch_decides_clear_of_round_off(ch):
    """the launches of tests/test_gpu_weighted_vel.py, every n_rx of this ch_per_rx: a spoiled slot gives no row and every other
    satellite's slot gives one (so n_used is what the kinds say, never an accident of a threshold); exactly one flag per receiver, the
    one its kind calls for; pivots a factor >= 1e3 away from the rule's 1e-10 N_kk on either side (the duplicated satellite's sits at
    about 1e-16); a record without VEL is zero but for flags, n_used and used_mask"""
    for n_rx in K.SHAPES_RX:
        case = K.launch_case(ch, n_rx)
        want, fix = case["want"], case["fix"]
        lo, hi = K.decisions_clear(case, n_rx)
        print(ch, n_rx, "smallest passing pivot share", lo, "largest failing", hi, "flags", np.bincount(want["flags"], minlength=17)[[1, 2, 4, 8, 16]])
        for r, (kind, at) in enumerate(zip(case["kinds"], case["spoiled"])):
            held = int(fix["used_mask"][r]) | ((1 << at) if kind == "not_in_mask" else 0)      # the slots that hold a satellite
            n_sats = bin(held).count("1")
            flag, mask = int(want["flags"][r]), int(want["used_mask"][r])
            if kind == "no_fix":
                assert flag == V.F_NO_FIX and mask == 0 and int(want["n_used"][r]) == 0
                continue
            assert mask == (held & ~(1 << at) if kind in K.SLOT_KINDS else held), (r, kind, at, bin(mask), bin(held))
            assert int(want["n_used"][r]) == bin(mask).count("1") == n_sats - (kind in K.SLOT_KINDS)
            if int(want["n_used"][r]) < 4:
                assert flag == V.F_TOO_FEW
            else:
                assert flag == {"singular": V.F_SINGULAR, "nonfinite": V.F_NONFINITE}.get(kind, V.F_VEL), (r, kind, flag)
        blank = want[want["flags"] != V.F_VEL].copy()
        blank["flags"], blank["n_used"], blank["used_mask"] = 0, 0, 0
        assert not blank.view(np.uint8).any()
        if ch >= 5 and n_rx >= 17:
            assert set(want["flags"].tolist()) == {V.F_VEL, V.F_NO_FIX, V.F_TOO_FEW, V.F_SINGULAR, V.F_NONFINITE}
        moving = [r for r, k in enumerate(case["kinds"]) if k == "moving" and want["flags"][r] == V.F_VEL]
        still = [r for r, k in enumerate(case["kinds"]) if k == "still" and want["flags"][r] == V.F_VEL]
        assert all(np.linalg.norm(want["vel"][r]) > 30.0 for r in moving) and all(np.linalg.norm(want["vel"][r]) < 0.1 for r in still)


def test_smoke_fixture_is_the_cases_modules():
    """(needs the fixture, which comes with gpsx_wvel) tests/golden/wvel_smoke.npz holds weighted_vel_cases.smoke_case() bit for bit, and
    that receiver's restatement is within the truth bounds of what was injected"""
    gold = np.load(os.path.join(ROOT, "tests", "golden", "wvel_smoke.npz"))
    want = K.smoke_case()
    assert sorted(gold.files) == sorted(want)
    for k, v in want.items():
        assert np.asarray(gold[k]).tobytes() == np.asarray(v).tobytes() and np.asarray(gold[k]).dtype == np.asarray(v).dtype, k
    assert np.linalg.norm(gold["vel"] - gold["truth_vel"]) <= 2.0 * K.MEASURED["truth_slow_vel_mps"]
    assert abs(float(gold["drift_s_s"]) - float(gold["truth_drift"])) * V.C_LIGHT <= 2.0 * K.MEASURED["truth_cdrift_mps"]
