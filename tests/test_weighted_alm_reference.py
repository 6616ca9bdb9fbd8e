"""The restatement of the almanac stage (tests/weighted_alm_ref.py) held to the definition in include/gpsx.h (gpsx_walm): the layouts,
one row per clause with its predicate (tests/weighted_alm_cases.py), subframes cut across launches at every word boundary, the bad
states, an encoder written from the field list with two hand-computed pages pinned as literals, the two host helpers of the library
against the restatement's, the physics of an almanac orbit against its ephemeris, the exports, the build check and the smoke fixture.
No GPU."""
import inspect
import math
import os
import re

import numpy as np
import pytest

import weighted_alm_cases as A
import weighted_alm_ref as R
import weighted_eph_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SC = 3.1415926535898


def _header():
    with open(os.path.join(ROOT, "include", "gpsx.h")) as f:
        return f.read()


def test_layouts_are_the_headers_and_the_library_exports_the_entry_points():
    import __graft_entry__ as ge
    from stm32f4_sdr_gps_amd import build, capi
    for mine, theirs in ((R.CFG_DTYPE, capi.WALM_CFG_DTYPE), (R.SLOT_DTYPE, capi.WALM_SLOT_DTYPE), (R.BANK_DTYPE, capi.WALM_BANK_DTYPE),
                         (R.RX_DTYPE, capi.WALM_RX_DTYPE), (R.SV_DTYPE, capi.WALM_SV_DTYPE)):
        assert mine == theirs
    offsets = lambda d: [d.fields[k][1] for k in d.names]      # noqa: E731
    assert offsets(R.CFG_DTYPE) == [0, 4] and offsets(R.SLOT_DTYPE) == [0, 8, 16, 48, 52, 56, 60]
    assert offsets(R.BANK_DTYPE) == [0, 1088, 1096, 1100, 1104, 1108] and R.BANK_DTYPE.itemsize % 16 == 0
    assert offsets(R.RX_DTYPE) == [0, 4, 8, 16, 24, 32, 36, 40, 44, 48, 52, 56, 60, 64, 68, 72, 76, 80, 88, 96] and R.RX_DTYPE.itemsize % 16 == 0
    assert offsets(R.SV_DTYPE) == [0, 4, 8, 12] + list(range(16, 96, 8))
    h = _header()
    for name, value in (("IONUTC", R.IONUTC), ("PAGE25", R.PAGE25), ("HELD", R.HELD), ("WEEK", R.WEEK), ("HEALTHY", R.HEALTHY), ("NEW", R.NEW)):
        assert re.search(rf"#define GPSX_WALM_{name}\s+{value}u\b", h), name
        assert getattr(capi, "WALM_" + name) == value
    for decl in ("int gpsx_walm_dev(gpsx_ctx *ctx, const gpsx_walm_cfg_t *cfg, const gpsx_wnav_word_t *d_words, int n_blocks, int n_rx,",
                 "int gpsx_walm(gpsx_ctx *ctx, const gpsx_walm_cfg_t *cfg, const gpsx_wnav_word_t *d_words, int n_blocks, int n_rx,",
                 "int gpsx_walm_to_eph(const gpsx_walm_sv_t *in, gpsx_weph_t *out);",
                 "int gpsx_walm_gps_minus_utc(const gpsx_walm_rx_t *rx, int week, double tow_s, double *dt_s);",
                 "} gpsx_walm_cfg_t;", "} gpsx_walm_slot_t;", "} gpsx_walm_bank_t;", "} gpsx_walm_rx_t;", "} gpsx_walm_sv_t;"):
        assert decl in h, decl
    assert re.search(r"#define GPSX_VERSION\s+110\b", h)        # no existing struct changed
    for sym in ("gpsx_walm", "gpsx_walm_dev", "gpsx_walm_to_eph", "gpsx_walm_gps_minus_utc"):
        assert sym in ge.ABI_SYMBOLS
    lib = capi.load_library()
    assert len(lib.gpsx_walm.argtypes) == 9 and lib.gpsx_walm_dev.argtypes == lib.gpsx_walm.argtypes
    assert capi.walm_cfg(12).tobytes() == np.array([(12, (0, 0, 0))], R.CFG_DTYPE).tobytes() and callable(capi.Engine.walm) and callable(capi.Engine.walm_dev)
    # the build check is there and the build calls it
    assert "check_walm()" in inspect.getsource(build.check_no_scratch) and '"k_walm.o", "k_walm", True' in inspect.getsource(build.check_walm)
    if os.path.exists(os.path.join(build.PKG, "build", "k_walm.o")):
        (res,) = build.check_walm().values()
        assert res["scratch_bytes"] == 0 and res["lds_bytes"] == 0


# ---- the table ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def outcomes():
    t = A.table()
    assert not t["bad_slots"] and not t["bad_banks"]
    return A.outcomes(t["banks"], t["rx"], t["alm"])


@pytest.mark.parametrize("k", range(len(A.rows())), ids=[re.sub(r"\W+", "_", name) for name, _, _ in A.rows()])
def test_one_row_per_clause(outcomes, k):
    name, _, check = A.rows()[k]
    o = outcomes[k]
    assert check(o), (name, o.have, o.stored, o.changed, o.other, o.seen, o.new)


def test_the_table_and_the_streams_reach_what_they_claim():
    names = " ".join(name for name, _, _ in A.rows())
    for clause in ("SV 1 ", "SV 24 from subframe 5", "SV 25 from subframe 4", "SV 32", "dummy SV 0", "data ID 0", "data ID 2", "data ID 3", "SV 24 in subframe 4",
                   "SV 25 in subframe 5", "57", "63", "toa raw 148", "toa raw 147", "page 18", "page 25", "subframes 1, 2 and 3", "failed word", "dropped word",
                   "relabelled", "wrong spacing", "sync pair", "two slots", "same words again", "one changed bit", "not page 25's", "wna 34", "wna 33",
                   "wna 114", "wna 115", "at min", "at -1", "at 0", "at max", "all-zero alpha"):
        assert clause in names, clause
    c = A.shape_case(67, 33)
    have = int(np.bitwise_or.reduce(c["banks"]["have_mask"]))
    assert have >> 32 == 3 and have & 0xFFFFFF and have >> 24 & 0xFF and int(c["banks"]["n_other"].sum()) > 50
    assert int(c["rx"][0]["n_stored"].sum()) > 100 and (c["rx"][0]["n_stored"] >= 2).any()        # commits in the measured launch, several per receiver
    assert (c["slots_before"]["cur_next"] != 0).sum() > 500 and int((c["rx"][0]["new_mask"] != c["rx"][0]["seen_mask"]).sum()) > 0


def _cut_lengths(cuts, total):
    """launch lengths that cover blocks 0 .. total - 1 with a launch boundary at every block of `cuts`, none longer than 4096"""
    lengths, at = [], 0
    for c in sorted(cuts) + [total]:
        while c - at > 4096:
            lengths.append(4096)
            at += 4096
        if c > at:
            lengths.append(c - at)
            at = c
    return lengths


def test_a_subframe_cut_across_two_and_three_launches_at_every_word_boundary():
    """a page from block 4500 on, beside a page 18 in the next slot 17 blocks later: wherever the launches end -- at every word boundary
    of the first, at every pair of them, a block before and after -- the bank and the states come out as from launches of 4096"""
    rng = np.random.default_rng(7)
    w8, p18 = A.random_almanac(rng, 6), A.page18(A.random_raw(A.P18_FIELDS, rng))
    per_channel = [A.events(A.frame(4500, 5, w8)), A.events(A.frame(4517, 4, p18))]
    total = 12288
    whole = A.run_launches(per_channel, 2, 3)
    assert int(whole["banks"]["have_mask"][0]) == 1 << 5 | 1 << 32 and int(whole["banks"]["n_stored"][0]) == 2
    bounds = [4500 + 600 * w for w in range(1, 10)]
    cuts = [[b + d] for b in bounds for d in (-1, 0, 1)] + [[a, b] for a in bounds for b in bounds if a < b]
    for cut in cuts:
        lengths = _cut_lengths(cut, total)
        assert max(lengths) <= 4096 and sum(lengths) == total
        got = A.run_launches(per_channel, 2, 0, lengths=lengths)
        assert got["banks"].tobytes() == whole["banks"].tobytes() and got["slots"].tobytes() == whole["slots"].tobytes(), cut
        assert sum(int(x["n_stored"][0]) for x in got["rx"]) == 2
        last, ref = got["rx"][-1].copy(), whole["rx"][-1].copy()      # (which launch a commit falls into is the cut's: the rest is not)
        for x in (last, ref):
            x["n_stored"], x["new_mask"], x["seen_mask"] = 0, 0, 0
        assert last.tobytes() == ref.tobytes()


# ---- bad states ---------------------------------------------------------------------------------------------------------------------
def test_every_bad_clause_of_slot_and_bank():
    per_channel, slots, banks = A.bad_case()
    before_slots, before_banks = slots.copy(), banks.copy()
    out = A.run_launches(per_channel, 4, 1, slots=slots, banks=banks, at=3 * 4096)
    bad_slots = [r * 4 + r % 4 for r in range(len(A.BAD_SLOT_FIELDS))]
    bad_banks = list(range(12, 12 + len(A.BAD_BANK_FIELDS)))
    assert out["bad_slots"] == bad_slots and out["bad_banks"] == bad_banks
    after_slots, after_banks = out["slots"], out["banks"]
    assert after_slots[bad_slots].tobytes() == before_slots[bad_slots].tobytes() and after_banks[bad_banks].tobytes() == before_banks[bad_banks].tobytes()
    for r in bad_banks:      # a BAD bank: the receiver's slots stay too, its records are zero
        assert after_slots[4 * r:4 * r + 4].tobytes() == before_slots[4 * r:4 * r + 4].tobytes()
        assert out["rx"][0][r].tobytes() == bytes(160) and out["alm"][0][r].tobytes() == bytes(96 * 32)
    served = [c for c in range(len(slots)) if c not in bad_slots and c // 4 not in bad_banks]
    assert (after_slots["blocks_seen"][served] == before_slots["blocks_seen"][served] + 4096).all()
    # the same receivers without the bad states' neighbours: a BAD slot takes nothing from the others
    clean = A.shape_case(24, 4)
    for r in range(len(A.BAD_SLOT_FIELDS), 12):
        assert out["rx"][0][r].tobytes() == clean["rx"][0][r].tobytes()


# ---- the encoder and two pages computed by hand ---------------------------------------------------------------------------------------
def test_the_encoder_round_trips_random_raw_fields():
    rng = np.random.default_rng(5)
    for _ in range(200):
        sv, raw = int(rng.integers(0, 64)), A.random_raw(A.ALM_FIELDS, rng)
        w8 = A.almanac_page(sv, raw, int(rng.integers(0, 4)))
        assert all(0 <= w < 1 << 24 for w in w8) and R.u(w8, 62, 6) == sv
        for name, (runs, _) in A.ALM_FIELDS.items():
            got = 0
            for pos, n in runs:
                got = got << n | R.u(w8, pos, n)
            assert got == raw[name], name
        raw18 = A.random_raw(A.P18_FIELDS, rng)
        w8 = A.page18(raw18)
        assert R.u(w8, 60, 2) == 1 and R.u(w8, 62, 6) == 56
        for name, (runs, _) in A.P18_FIELDS.items():
            got = 0
            for pos, n in runs:
                got = got << n | R.u(w8, pos, n)
            assert got == raw18[name], name
        toa, wna, health = int(rng.integers(0, 256)), int(rng.integers(0, 256)), {int(n): int(rng.integers(0, 64)) for n in rng.integers(1, 25, 5)}
        w8 = A.page25(toa, wna, health)
        assert (R.u(w8, 62, 6), R.u(w8, 68, 8), R.u(w8, 76, 8)) == (51, toa, wna)
        assert R.decode_page25(w8)["p25_unhealthy_mask"] == sum(1 << (n - 1) for n, v in health.items() if v)


def test_two_pages_computed_by_hand():
    """an almanac page of SV 5 and a page 18, bit by bit on paper: the words the encoder must give and the values the decoder must"""
    raw = dict(e=0x1234, toa=42, di=-2, OMGd=-700, svh=0, rootA=0xA10D00, OMG0=0x400000, omg=-0x400000, M0=1, f0=-1023, f1=-1)
    words = [0x451234, 0x2AFFFE, 0xFD4400, 0xA10D00, 0x400000, 0xC00000, 0x000001, 0x80FFE4]
    assert A.almanac_page(5, raw) == words
    d = R.decode_sv(words)
    assert d == dict(svid=5, svh=0, e=4660.0 / 2097152.0, toas=172032.0, i0=(0.3 - 2.0 / 524288.0) * SC, OMGd=-700.0 / 274877906944.0 * SC,
                     A=5153.625 * 5153.625, OMG0=0.5 * SC, omg=-0.5 * SC, M0=SC / 8388608.0, f0=-1023.0 / 1048576.0, f1=-1.0 / 274877906944.0)
    assert R.entry_of(5, words) == 4 and R.entry_of(4, words) == -1
    raw18 = dict(a0=16, a1=-1, a2=-128, a3=127, b0=42, b1=-2, b2=1, b3=0, A1=-3, A0=5, tot=36, wnt=137, dt_ls=18, wn_lsf=137, dn=7, dt_lsf=18)
    words18 = [0x7810FF, 0x807F2A, 0xFE0100, 0xFFFFFD, 0x000000, 0x052489, 0x128907, 0x120000]
    assert A.page18(raw18) == words18
    d = R.decode_page18(words18)
    assert d == dict(ion=[16.0 / 2 ** 30, -1.0 / 2 ** 27, -128.0 / 2 ** 24, 127.0 / 2 ** 24, 42.0 * 2048, -2.0 * 16384, 65536.0, 0.0], A1=-3.0 / 2 ** 50,
                     A0=5.0 / 2 ** 30, tot_s=147456, wnt=2185, dt_ls=18, wn_lsf=2185, dn=7, dt_lsf=18)
    assert R.entry_of(4, words18) == 32 and R.entry_of(5, words18) == -1


def test_eight_bit_weeks_resolve_around_the_build_week():
    assert [R.week8(w) for w in (34, 33, 114, 115, 0, 255)] == [2338, 2337, 2418, 2163, 2304, 2303]
    assert all(2290 - 127 <= R.week8(w) <= 2290 + 128 and R.week8(w) % 256 == w for w in range(256))


# ---- the helpers ------------------------------------------------------------------------------------------------------------------------
def _records():
    t = A.table()
    alm = np.concatenate([a.reshape(-1) for a in t["alm"]])
    rx = np.concatenate(t["rx"])
    return alm, rx


def test_walm_to_eph_field_for_field_and_its_refusals():
    from stm32f4_sdr_gps_amd import capi
    alm, _ = _records()
    held_week = [a for a in alm if int(a["flags"]) & (R.HELD | R.WEEK) == R.HELD | R.WEEK]
    others = [a for a in alm if int(a["flags"]) & (R.HELD | R.WEEK) != R.HELD | R.WEEK]
    assert held_week and any(int(a["flags"]) & R.HELD for a in others) and any(int(a["flags"]) == 0 for a in others)
    for a in held_week:
        got, want = capi.walm_to_eph(a), R.to_eph(a, E.EPH_DTYPE)
        assert got.tobytes() == want.tobytes()
        g = got[0]
        assert int(g["flags"]) == E.F_VALID and float(g["toes"]) == float(a["toas"]) and int(g["week"]) == int(a["week"]) and int(g["svh"]) == int(a["svh"])
        assert all(float(g[k]) == float(a[k]) for k in ("A", "e", "i0", "OMG0", "omg", "M0", "OMGd", "f0", "f1"))
        assert int(g["toe_time"]) == 315964800 + 604800 * int(a["week"]) + int(a["toas"]) == int(g["toc_time"]) and float(g["toe_sec"]) == 0.0
        zero = [k for k in E.EPH_DTYPE.names if k not in ("flags", "week", "svh", "toe_time", "toc_time", "A", "e", "i0", "OMG0", "omg", "M0", "OMGd",
                                                         "toes", "f0", "f1")]
        assert all(g[k] == 0 for k in zero)
        eph = capi.weph_to_eph(got, 9)      # ... and the existing helper takes it as it is
        assert float(eph["A"][0]) == float(a["A"]) and int(eph["sat"][0]) == 9
    lib = capi.load_library()
    out = np.full(1, 0x5A, np.uint8).repeat(256)
    for a in others[:40]:
        assert R.to_eph(a, E.EPH_DTYPE) is None
        assert lib.gpsx_walm_to_eph(np.ascontiguousarray(a).ctypes.data, out.ctypes.data) == -22 and (out == 0x5A).all()
        with pytest.raises(capi.GpsxError):
            capi.walm_to_eph(a)
    a = np.ascontiguousarray(held_week[0])
    assert lib.gpsx_walm_to_eph(None, out.ctypes.data) == -22 and lib.gpsx_walm_to_eph(a.ctypes.data, None) == -22 and (out == 0x5A).all()


def test_gps_minus_utc_on_both_sides_of_the_leap_second_and_its_refusals():
    import ctypes as C
    from stm32f4_sdr_gps_amd import capi
    raw = dict(a0=1, a1=2, a2=3, a3=4, b0=5, b1=6, b2=7, b3=8, A1=-11, A0=-900, tot=90, wnt=2300 % 256, dt_ls=17, wn_lsf=2301 % 256, dn=3, dt_lsf=18)
    out = A.run_launches([A.events(A.frame(300, 4, A.page18(raw)))], 1, 2)
    rx = out["rx"][-1][0]
    assert int(rx["flags"]) == R.IONUTC and (int(rx["wnt"]), int(rx["wn_lsf"]), int(rx["dt_ls"]), int(rx["dt_lsf"])) == (2300, 2301, 17, 18)
    a0, a1 = -900.0 / 2 ** 30, -11.0 / 2 ** 50
    instant = 3 * 86400.0      # the end of day 3 of week 2301
    for week, tow, ls in ((2301, instant - 0.5, 17), (2301, instant, 18), (2301, instant + 0.5, 18), (2300, 604799.0, 17), (2302, 0.0, 18), (2301, 0.0, 17),
                          (2290, 1234.5, 17)):
        got = capi.walm_gps_minus_utc(rx, week, tow)
        assert got == R.gps_minus_utc(rx, week, tow)
        assert got == (float(ls) + a0) + a1 * ((tow - 90 * 4096.0) + 604800.0 * (week - 2300.0)), (week, tow)
        assert abs(got - ls) < 1e-6
    lib = capi.load_library()
    dt = C.c_double(-7.0)
    bad = []
    for field, value in (("flags", 0), ("flags", R.PAGE25), ("dn", 0), ("dn", 8), ("dn", -1)):
        x = np.array([rx], R.RX_DTYPE)
        x[field] = value
        bad.append((x, 2301, 5.0))
    bad += [(np.array([rx], R.RX_DTYPE), 2301, float("nan")), (np.array([rx], R.RX_DTYPE), 2301, float("inf"))]
    for x, week, tow in bad:
        assert R.gps_minus_utc(x[0], week, tow) is None
        assert lib.gpsx_walm_gps_minus_utc(x.ctypes.data, week, tow, C.byref(dt)) == -22 and dt.value == -7.0
        with pytest.raises(capi.GpsxError):
            capi.walm_gps_minus_utc(x, week, tow)
    x = np.array([rx], R.RX_DTYPE)
    assert lib.gpsx_walm_gps_minus_utc(None, 2301, 5.0, C.byref(dt)) == -22 and lib.gpsx_walm_gps_minus_utc(x.ctypes.data, 2301, 5.0, None) == -22


# ---- physics ----------------------------------------------------------------------------------------------------------------------------
def _sky(site, seed0):
    import weighted_fix_cases as W
    return [row for _, row in W.sky(site, 12, seed0)]


def _orbit_distances(site, seed0, to_eph):
    rows = _sky(site, seed0)
    alm, rx = A.almanac_records(rows)
    assert int(rx["wna"]) == A.ALM_WEEK and all(int(a["flags"]) & (R.HELD | R.WEEK | R.HEALTHY) == R.HELD | R.WEEK | R.HEALTHY for a in alm)
    ephs = [to_eph(a) for a in alm]
    return rows, ephs, [A.orbit_distance(row, e[0]) for row, e in zip(rows, ephs)]


def test_physics_an_almanac_orbit_stays_near_its_ephemeris():
    """MEASURED on the CPU with the restatement's gpsx_walm_to_eph (never with the library's): the largest distance over +-2 h around toa
    between twelve Munich satellites' ephemeris positions (pvt_chain.sat_state on weighted_fix_cases.sky's rows) and the positions from
    their almanac pages is 1319.5 m (weighted_alm_cases.MEASURED_ORBIT_M), under the 2 km the dropped terms suggested: at two hours
    the missing deln alone moves a satellite by 4.5e-9 rad/s x 7200 s x 26 560 km = 860 m, crc adds 220 m and cus 160 m.  Other orbit seeds and sites are held to 2 x that; the library's helper gives the restatement's records byte for byte,
    so the same distances"""
    from stm32f4_sdr_gps_amd import capi
    _, _, d0 = _orbit_distances("munich", 0, lambda a: R.to_eph(a, E.EPH_DTYPE))
    print("largest almanac-to-ephemeris distance over +-2 h, seed 0 at Munich:", max(d0), "m")
    assert abs(max(d0) - A.MEASURED_ORBIT_M) <= 0.05 * A.MEASURED_ORBIT_M       # the constant is the measurement
    for site, seed0 in (("munich", 3), ("sydney", 0), ("taveuni", 6), ("quito", 9)):
        rows, ephs, d = _orbit_distances(site, seed0, capi.walm_to_eph)
        print(site, seed0, max(d))
        assert max(d) <= 2.0 * A.MEASURED_ORBIT_M, (site, seed0, d)


def test_physics_the_elevation_mask_names_the_same_satellites():
    """at a 5 degree mask the almanac and the ephemerides name the same visible set from four sites -- satellites picked for another
    site's sky among them, most of them below the horizon --, except those within the bound's angle (2 x the measured distance seen
    from 20 000 km) of the mask"""
    import pvt_chain as pc
    import weighted_fix_cases as W
    from stm32f4_sdr_gps_amd import capi
    mask, slack = math.radians(5.0), 2.0 * A.MEASURED_ORBIT_M / 20.0e6
    n_vis = n_hidden = 0
    for seed0 in (0, 5):
        rows, ephs, _ = _orbit_distances("munich", seed0, capi.walm_to_eph)
        for site in W.SITES:
            rx = W.site_ecef(site)
            geo = pc._geodetic(rx)
            for row, e in zip(rows, ephs):
                for t in (W.TOW - 3000.0, W.TOW, W.TOW + 3000.0):
                    el_e = float(pc._azel(rx, geo, pc.sat_state(row, np.array([t]))[0])[1][0])
                    el_a = float(pc._azel(rx, geo, pc.sat_state(A.row_of_eph(e[0]), np.array([t]))[0])[1][0])
                    assert abs(el_e - el_a) <= slack
                    if abs(el_e - mask) > slack:
                        assert (el_e > mask) == (el_a > mask), (site, t)
                        n_vis += el_e > mask
                        n_hidden += el_e <= mask
    assert n_vis > 50 and n_hidden > 50, (n_vis, n_hidden)


def test_the_smoke_fixture_is_what_the_cases_write(tmp_path):
    path = os.path.join(ROOT, "tests", "golden", "walm_smoke.npz")
    A.write_smoke(str(tmp_path / "again.npz"))
    a, b = np.load(path), np.load(str(tmp_path / "again.npz"))
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
    assert os.path.getsize(path) < 1 << 20
