"""What the CPU and GPU tests of the weighted chain's fault detection and exclusion share (include/gpsx.h gpsx_wfde): receivers of
weighted_fix_cases.receiver with faults injected through its `noise` and through tx_ms +- 1 with GPSX_WOBS_AMBIGUOUS, the seeded
tables of draws (one fault, clean, one or two wrong milliseconds), the launches of the GPU tests with receivers of different kinds as
neighbours, the smoke fixture and the bounds.  Test infrastructure; nothing here is product code.

A draw or receiver is used for a decision comparison only where every margin of the restatement (tests/weighted_fde_ref.py: each
test's |T - limit| / limit, each exclusion's gap between the best and second-best w^2, each repair's distance from a half) is at least
1e-6: the device's libm differs from glibc by about 1e-6 m, so there the two must decide alike.  The selection looks at the
restatement alone, never at the device."""
import functools

import numpy as np

import weighted_eph_ref as E
import weighted_fde_ref as D
import weighted_fix_cases as W
import weighted_fix_ref as F
import weighted_obs_ref as O

Z, MAX_EXCL = 3.09, 2
SEED = 2025
NOISE_M = 3.0


@functools.lru_cache(maxsize=None)
def _noisy(site, n_sats, seed0, noise):
    return W.receiver(site, n_sats, seed0, noise=noise)


def receiver(site, n_sats, seed0, noise=None, ms=None):
    """weighted_fix_cases.receiver with `noise` metres per pseudorange (faults are large entries of it) and ms: {slot: d}, which moves
    that slot's tx_ms by d and flags it AMBIGUOUS -> (obs, eph)"""
    obs, eph = (a.copy() for a in _noisy(site, n_sats, seed0, None if noise is None else tuple(float(v) for v in noise)))
    for slot, d in (ms or {}).items():
        obs["tx_ms"][slot] += d
        obs["flags"][slot] |= O.F_AMBIGUOUS
    return obs, eph


def cfg(ch, min_sats=4, max_excl=MAX_EXCL, repair=1, z=Z):
    """the binding's gpsx_wfde_cfg_t, which must be the restatement's byte for byte"""
    from stm32f4_sdr_gps_amd import capi
    c = capi.wfde_cfg(W.OFFSET_MS, ch, min_sats, z_global=z, max_excl=max_excl, repair=bool(repair))
    assert c.tobytes() == D.make_cfg(W.OFFSET_MS, ch, min_sats, z_global=z, max_excl=max_excl, repair=repair).tobytes()
    return c


# ---- the isolation table: one receiver, one fault ------------------------------------------------------------------------------------
FAULTS_M, N_SATS, N_SKIES = (150.0, 1000.0, -400.0), (6, 8, 12), 6


@functools.lru_cache(maxsize=None)
def isolation_draws():
    """4 sites x 6 / 8 / 12 satellites x six skies x faults of 150 / 1000 / -400 m at a drawn slot over NOISE_M metres of Gaussian
    noise: 216 draws, seeded -> [dict(site, n, seed0, slot, fault, obs, eph)]"""
    rng = np.random.default_rng(SEED)
    out = []
    for site in sorted(W.SITES):
        for n in N_SATS:
            for k in range(N_SKIES):
                for fault in FAULTS_M:
                    noise, slot = rng.normal(0.0, NOISE_M, n), int(rng.integers(n))
                    noise[slot] += fault
                    obs, eph = receiver(site, n, 3 * k, noise)
                    out.append(dict(site=site, n=n, seed0=3 * k, slot=slot, fault=fault, obs=obs, eph=eph))
    return out


def run_each(draws, **kw):
    """every draw as a launch of its own width, grouped by width -> per draw (fix record, fde record, margins)"""
    out = [None] * len(draws)
    for n in sorted({len(d["obs"]) for d in draws}):
        idx = [i for i, d in enumerate(draws) if len(d["obs"]) == n]
        obs, eph = W.pack([(draws[i]["obs"], draws[i]["eph"]) for i in idx], n)
        fix, fde, _, margins = D.run(cfg(n, **kw), obs, eph, len(idx))
        for at, i in enumerate(idx):
            out[i] = (fix[at], fde[at], margins[at])
    return out


@functools.lru_cache(maxsize=None)
def isolation_kept():
    """the draws in which the restatement excludes exactly the injected slot and every margin is >= 1e-6 -> [(draw, fix, fde)]"""
    draws = isolation_draws()
    return [(d, fix, fde) for d, (fix, fde, m) in zip(draws, run_each(draws))
            if int(fde["excl_mask"]) == 1 << d["slot"] and (int(fde["flags"]) & D.VERDICTS) in (D.PASSED, D.UNCHECKED) and D.min_margin(m) >= D.MARGIN]


# ---- clean draws, wrong milliseconds ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def clean_draws(n=48):
    """n receivers without a fault under NOISE_M metres of noise: sites, 6 / 8 / 12 satellites and skies in turn"""
    rng = np.random.default_rng(SEED + 1)
    names = sorted(W.SITES)
    out = []
    for i in range(n):
        site, ns, seed0 = names[i % 4], N_SATS[(i // 4) % 3], 3 * ((i // 12) % N_SKIES)
        obs, eph = receiver(site, ns, seed0, rng.normal(0.0, NOISE_M, ns))
        out.append(dict(site=site, n=ns, seed0=seed0, obs=obs, eph=eph))
    return out


@functools.lru_cache(maxsize=None)
def ms_draws(n=32):
    """n receivers of 8 or 12 satellites with one (even draws) or two slots moved by +-1 ms and flagged AMBIGUOUS, over NOISE_M metres
    of noise; `ms` {slot: d} is what was injected: the repair's k is -d"""
    rng = np.random.default_rng(SEED + 2)
    names = sorted(W.SITES)
    out = []
    for i in range(n):
        site, ns, seed0 = names[i % 4], (8, 12)[(i // 4) % 2], 3 * ((i // 8) % N_SKIES)
        slots = rng.choice(ns, 1 + i % 2, replace=False)
        ms = {int(s): int(rng.choice((-1, 1))) for s in slots}
        obs, eph = receiver(site, ns, seed0, rng.normal(0.0, NOISE_M, ns), ms)
        out.append(dict(site=site, n=ns, seed0=seed0, ms=ms, obs=obs, eph=eph))
    return out


def ms_masks(draw):
    """(plus_mask, minus_mask) that repairs draw's injected milliseconds: tx_ms moved by d is corrected by -d"""
    return sum(1 << s for s, d in draw["ms"].items() if d < 0), sum(1 << s for s, d in draw["ms"].items() if d > 0)


# ---- the GPU tests' launches -----------------------------------------------------------------------------------------------------------
SHAPES = tuple((ch, n_rx) for ch in (5, 8, 12, 33, 64) for n_rx in (1, 17, 67)) + ((4, 67),)
KINDS = ("clean", "one_fault", "ambig_minus", "two_faults", "ambig_two", "four_usable", "fault_and_ambig", "ambig_latest", "too_few", "ambig_3ms",
         "few_unambiguous", "duplicate", "three_faults", "lock_masked")
KINDS_4 = ("clean", "one_fault", "ambig_flag_only")      # four slots: UNCHECKED whatever they hold
KINDS_5 = ("clean", "one_fault", "few_unambiguous", "four_usable", "too_few", "duplicate", "lock_masked")


def launch_min_sats(ch):
    """ch_per_rx 5 runs with min_sats 5: with one degree of freedom every w^2 is the same number, so a five-row exclusion has no
    margin; there a failed test ends in FAULT (n_counted - 1 < min_sats) and four usable slots in NOFIX"""
    return 5 if ch == 5 else 4


@functools.lru_cache(maxsize=None)
def launch_case(ch, n_rx):
    """One launch: receiver r is of kind KINDS[(r + ch) % 14] (ch_per_rx 4 and 5: of their shorter lists), so the groups of a wave sit
    in different rounds; its satellites (twelve at most) start at slot r % ch and wrap, the rest of its slots are all-zero pairs; every
    pseudorange carries 2 m of seeded noise.  A fault or wrong millisecond sits at the first, a middle or the last satellite's slot, in turn.
    -> dict(cfg, obs, eph, lock (always given: all CODE but a lock_masked receiver's faulty slot), kinds, want (fix, fde, pr), margins)"""
    names = sorted(W.SITES)
    kinds_of = KINDS_4 if ch == 4 else KINDS_5 if ch == 5 else KINDS
    obs, eph = np.zeros((n_rx, ch), O.OBS_DTYPE), np.zeros((n_rx, ch), E.EPH_DTYPE)
    lock = np.zeros((n_rx, ch), F.LOCK_DTYPE)
    lock["flags"] = F.LOCK_CODE
    kinds = []
    for r in range(n_rx):
        rng = np.random.default_rng([SEED, ch, r])
        site, kind = names[(r + ch) % len(names)], kinds_of[(r + ch) % len(kinds_of)]
        n = min(ch, 12)
        if kind == "four_usable":
            n = 4
        elif kind == "too_few":
            n = 3
        at = (0, n - 1, n // 2)[r % 3]                   # the satellite that is spoiled first
        others = [k for k in range(n) if k != at]
        noise, ms = rng.normal(0.0, 2.0, n), {}
        if kind in ("one_fault", "fault_and_ambig", "lock_masked"):
            noise[at] += 300.0 if kind != "lock_masked" else 1000.0
        if kind == "two_faults":
            noise[at] += 400.0
            noise[others[1]] -= 700.0
        if kind == "three_faults":
            noise[at] += 400.0
            noise[others[1]] -= 700.0
            noise[others[3]] += 900.0
        if kind == "ambig_minus":
            ms = {at: 1}
        if kind == "ambig_two":
            ms = {at: 1, others[2]: -1}
        if kind == "fault_and_ambig":
            ms = {others[0]: -1}
        if kind == "ambig_3ms":
            ms = {at: 3}
        if kind == "ambig_flag_only":                    # flagged, not wrong
            ms = {others[0]: 0}
        if kind == "few_unambiguous":                    # flagged, not wrong; three unambiguous slots are left: |C| < min_sats
            ms = {k: 0 for k in others[:n - 3]}
        o, e = receiver(site, n, 3 * (r % 20), noise, ms if kind != "ambig_latest" else None)
        if kind == "ambig_latest":                      # the latest transmitter (the reference slot), one millisecond later still
            pr, ref, _ = F.pseudoranges(o.reshape(1, n), np.ones((1, n), bool), W.OFFSET_MS)
            o["tx_ms"][int(ref[0])] += 1
            o["flags"][int(ref[0])] |= O.F_AMBIGUOUS
        if kind == "duplicate":                          # four slots, two of them the same satellite
            n, o, e = 4, o[[0, 1, 2, 2]], e[[0, 1, 2, 2]]
        slots = [(r + k) % ch for k in range(n)]
        obs[r, slots], eph[r, slots] = o, e
        if kind == "lock_masked":
            lock["flags"][r, slots[at]] = 0
        kinds.append(kind)
    obs, eph, lock = obs.reshape(-1), eph.reshape(-1), lock.reshape(-1)
    c = cfg(ch, launch_min_sats(ch))
    fix, fde, pr, margins = D.run(c, obs, eph, n_rx, lock=lock)
    return dict(cfg=c, obs=obs, eph=eph, lock=lock, kinds=kinds, want=(fix, fde, pr), margins=margins)


# ---- the smoke fixture (tests/golden/wfde_smoke.npz) -----------------------------------------------------------------------------------
def smoke_case():
    """one eight-slot Munich receiver with a 300 m fault at slot 5 and slot 2 one millisecond late and AMBIGUOUS, 2 m of noise; the
    restatement's records -> the arrays of the fixture"""
    noise = np.random.default_rng(SEED + 3).normal(0.0, 2.0, 8)
    noise[5] += 300.0
    obs, eph = receiver("munich", 8, 0, noise, {2: 1})
    fix, fde, _, margins = D.run(cfg(8), obs, eph, 1)
    assert D.min_margin(margins[0]) >= D.MARGIN
    return dict(obs=obs, eph=eph, offset_ms=np.float64(W.OFFSET_MS), z_global=np.float64(Z), max_excl=np.int32(MAX_EXCL), rr=fix["rr"][0],
                truth=W.site_ecef("munich"), flags=fde["flags"][0], excl_mask=fde["excl_mask"][0], plus_mask=fde["plus_mask"][0],
                minus_mask=fde["minus_mask"][0], n_rounds=fde["n_rounds"][0])


# ---- comparison and bounds -------------------------------------------------------------------------------------------------------------
# the device against the restatement: 8 x the largest |d rr| measured on one MI355X over every receiver of tests/test_gpu_weighted_fde.py
# (profiles/r21_weighted_fde_parity.json), capped at 1e-4 m -- gpsx_wfix's practice; the factor covers libm round-off that
# accumulates differently in the later rounds.  Measured under the cap: 1.0324e-6 m (ch_per_rx 4, n_rx 67); the isolation draws 5.2e-7 m.
PARITY_MEASURED_M = 1.0325e-6
PARITY_CAP_M = 1e-4
POSITION_BOUND_M = PARITY_CAP_M if PARITY_MEASURED_M is None else min(8.0 * PARITY_MEASURED_M, PARITY_CAP_M)
MIN_SIGMA_M = 2.4      # the smallest row sigma: the URA table's first entry


def t_stat_bound(n_counted, T):
    """a position within the bound moves a residual by at most twice the bound, a y by that over the smallest sigma; over n rows
    |dT| <= 2 sqrt(n T) |dy| to first order"""
    return 4.0 * np.sqrt(n_counted * T) * POSITION_BOUND_M / MIN_SIGMA_M + 1e-12


def compare(got_fix, got_fde, got_pr, want_fix, want_fde, want_pr):
    """a launch against the restatement: flags, masks, n_rounds, n_excluded and dof equal; the fix records as
    weighted_fix_cases.compare orders it (under this module's bound); t_limit bit-equal; t_stat within t_stat_bound; nothing
    non-finite -> the fix comparison's maxima and the largest |d t_stat| over its bound"""
    for f in ("flags", "n_rounds", "n_excluded", "dof", "excl_mask", "plus_mask", "minus_mask", "reserved"):
        bad = np.flatnonzero(got_fde[f] != want_fde[f])
        assert bad.size == 0, (f, bad[:8], got_fde[f][bad][:8], want_fde[f][bad][:8])
    assert np.isfinite(got_fde["t_stat"]).all() and np.isfinite(got_fde["t_limit"]).all()
    assert got_fde["t_limit"].tobytes() == want_fde["t_limit"].tobytes(), "t_limit"
    worst = W.compare(got_fix, got_pr, want_fix, want_pr, bound=POSITION_BOUND_M)
    bound = t_stat_bound(want_fde["dof"] + 4, want_fde["t_stat"])
    dt = np.abs(got_fde["t_stat"] - want_fde["t_stat"])
    worst["t_stat_over_bound"] = float((dt / bound).max())
    assert (dt <= bound).all(), (np.flatnonzero(dt > bound)[:8], dt.max())
    return worst
