"""What the CPU and GPU tests of the weighted chain's navigation filter share (include/gpsx.h gpsx_wkf): sequences of launches -- a
receiver's position advanced by its velocity, true time advanced by n_blocks ms / (1 + drift), per-epoch observables and Dopplers built
on the CPU by weighted_fix_cases / weighted_vel_cases / weighted_edge_cases (no IF stream) --, the launches of the GPU tests, the smoke
fixture and the bounds.  Test infrastructure; nothing here is product code.

The receiver's clock reads rint(1000 t0) ms at the end of launch 0 and n_blocks ms more after every further launch; GPS time at the end
of launch k is t_k = t0 + k n_blocks 1e-3 / (1 + drift), so the clock gains `drift` seconds per second and b = c (clock - GPS time)."""
import functools
import json
import os

import numpy as np

import weighted_edge_cases as X
import weighted_eph_ref as E
import weighted_fix_cases as W
import weighted_fix_ref as F
import weighted_kf_ref as K
import weighted_obs_ref as O
import weighted_vel_cases as VC
import weighted_vel_ref as V

VELOCITY = VC.VELOCITIES[1]      # (30, -20, 5) m/s
N_BLOCKS = 1000
T0 = W.TOW + 2e-4      # the clock starts 0.2 ms behind GPS time: b = -59 958 m
NOISE_M = 3.0
LOCK_BOTH = 3


def fix_record(rr, slots, t, week, dtr_s=0.0):
    """a gpsx_wfix_t with FIX at rr whose receive time is t + dtr_s on a clock that is dtr_s fast"""
    fix = VC.fix_record(rr, slots)
    fix["rx_tow_s"], fix["dtr_s"], fix["week"] = t + dtr_s, dtr_s, week
    return fix


def vel_record(v, drift):
    vel = np.zeros(1, V.VEL_DTYPE)
    vel["flags"], vel["vel"][0], vel["drift_s_s"] = V.F_VEL, v, drift
    return vel


# ---- tracks ---------------------------------------------------------------------------------------------------------------------------
def epoch_times(t0, drift, n_launch, n_blocks=N_BLOCKS):
    return [t0 + k * n_blocks * 1e-3 / (1.0 + drift) for k in range(n_launch)]


@functools.lru_cache(maxsize=None)
def _track(site, n_sats, seed0, v, drift, n_launch, n_blocks, noise_m, noise_seed, t0):
    rx0 = W.site_ecef(site)
    sats = W.sky(site, n_sats, seed0)
    eph = np.concatenate([W.eph_record(raw) for raw, _ in sats])
    rng = np.random.default_rng(noise_seed)
    v = np.asarray(v, np.float64)
    out = []
    for t in epoch_times(t0, drift, n_launch, n_blocks):
        rx = rx0 + v * (t - t0)
        noise = rng.normal(0.0, noise_m, n_sats) if noise_m else np.zeros(n_sats)
        obs = np.concatenate([W.observable(row, rx, t, float(m)) for (_, row), m in zip(sats, noise)])
        # (weighted_vel_cases.doppler puts the receiver at its rx0 + v (t - W.TOW))
        obs["if_freq_offset_hz"] = [VC.doppler(row, rx - v * (t - W.TOW), v, drift, t) for _, row in sats]
        out.append(dict(t=t, rx=rx, obs=obs))
    return tuple(out), eph


def track(site="munich", n_sats=8, seed0=0, v=VELOCITY, drift=0.0, n_launch=14, n_blocks=N_BLOCKS, noise_m=0.0, noise_seed=0, t0=T0):
    """-> ([dict(t, rx, obs [n_sats])] per launch, eph [n_sats]); copies"""
    eps, eph = _track(site, n_sats, seed0, tuple(float(a) for a in v), float(drift), n_launch, n_blocks, float(noise_m), noise_seed, float(t0))
    return [dict(e, obs=e["obs"].copy()) for e in eps], eph.copy()


@functools.lru_cache(maxsize=None)
def _week_end_track(n_launch, n_blocks):
    r = X.receiver("t_week_end")
    rx0, t0 = X.site_ecef(r["site"]), r["t"]
    v = np.asarray(X.VELOCITY, np.float64)
    out = []
    for t in epoch_times(t0, X.DRIFT, n_launch, n_blocks):
        rx = rx0 + v * (t - t0)
        obs = np.concatenate([X.observable(row, rx, t) for row in r["rows"]])
        obs["if_freq_offset_hz"] = [X.doppler(row, rx, t) for row in r["rows"]]
        out.append(dict(t=t, rx=rx, obs=obs))
    return tuple(out), r["eph"]


def week_end_track(n_launch=5, n_blocks=500):
    """weighted_edge_cases' t_week_end receiver (twelve satellites, 604 798.8 s, 36 m/s, drift 1e-6) carried across the week's end in
    launches of half a second: the transmit times wrap, every satellite's |tk| stays below 7201 s"""
    eps, eph = _week_end_track(n_launch, n_blocks)
    return [dict(e, obs=e["obs"].copy()) for e in eps], eph.copy()


def run_sequence(cfg, launches, eph, fixes, vels=None, n_blocks=N_BLOCKS, state=None, locks=None, details=None):
    """the restatement, launch after launch, on one receiver: launches [obs [ch]], fixes / vels [record or None] per launch
    -> ([record], the state after)"""
    state = np.zeros(1, K.STATE_DTYPE) if state is None else state
    recs = []
    for k, obs in enumerate(launches):
        d = {} if details is not None else None
        rec, state, _ = K.run(cfg, obs, eph, state, 1, n_blocks, None if locks is None else locks[k], fixes[k], None if vels is None else vels[k],
                              detail=d)
        recs.append(rec[0])
        if details is not None:
            details.append(d)
    return recs, state


def wfix_sequence(launches, eph, ch):
    """gpsx_wfix's restatement on the same records, each launch started from the one before -> [FIX_DTYPE record]"""
    cfg, prev, out = F.make_cfg(W.OFFSET_MS, ch), None, []
    for obs in launches:
        prev = F.run(cfg, obs, eph, 1, prev=prev)[0]
        out.append(prev[0])
    return out


def first_fix(ep, eph, ch):
    """the INIT record of a track: gpsx_wfix's restatement on the first launch"""
    fix = F.run(F.make_cfg(W.OFFSET_MS, ch), ep["obs"], eph, 1)[0]
    assert int(fix["flags"][0]) == F.F_FIX
    return fix


def truth_clk_m(rec, t):
    """b = c (the record's clock reading - GPS time t), the difference folded into half a week"""
    d = (int(rec["rcv_ms"]) - 1000.0 * t + 302_400_000.0) % 604_800_000.0 - 302_400_000.0
    return K.MS * d


def cfg(ch, **kw):
    """the binding's gpsx_wkf_cfg_t, which must be the restatement's byte for byte"""
    from stm32f4_sdr_gps_amd import capi
    c = capi.wkf_cfg(ch, **kw)
    assert c.tobytes() == K.make_cfg(ch, **kw).tobytes()
    return c


# ---- the GPU tests' launches -----------------------------------------------------------------------------------------------------------
SHAPES_CH, SHAPES_RX = (1, 4, 5, 8, 12, 33, 64), (1, 17, 67)
KINDS = ("clean", "coasting", "starved", "fresh", "ambiguous", "faulty_slot", "faulty_doppler", "bad_state", "singular")
N_LAUNCH = 4
MAX_COAST = 1
FAULT_M, FAULT_HZ = 150.0, 50.0


@functools.lru_cache(maxsize=None)
def launch_case(ch, n_rx):
    """Four launches of n_rx receivers with ch slots: INIT, two updates and one launch that mixes kinds; receiver r is of
    KINDS[(r + ch) % 9], so receivers of every kind are neighbours in a wave.  Its satellites (eight at most) start at slot r % ch and
    wrap; the rest of its slots are all-zero pairs.  The slot that a kind spoils is the first, the last or a middle slot of the group in
    turn.  In the last launch: coasting has three, one or no usable slot (r // 9 % 3); starved has lock records without CODE or CARRIER in
    every launch, which with max_coast = 1 is COAST, LOST, then INIT again from the record still offered; fresh is offered no FIX record until the last launch (NOT_INIT x 3, INIT); ambiguous has a
    slot +1, -1 or +3 ms off with GPSX_WOBS_AMBIGUOUS; faulty_slot 150 m on a pseudorange, faulty_doppler 50 Hz on a frequency;
    bad_state's rcv_ms is set to -1 before the last launch (`poke`); singular holds one satellite twice, in every launch.  Half the
    receivers are offered a velocity record.
    -> dict(cfg, n_blocks, obs [4][n_rx * ch], eph, lock, fix [4] (None or [n_rx]), vel [n_rx], poke {receiver: field values}, kinds,
       want [4] records, states [4] after each launch, codes [4], details [4])"""
    names = sorted(W.SITES)
    obs = np.zeros((N_LAUNCH, n_rx, ch), O.OBS_DTYPE)
    eph = np.zeros((n_rx, ch), E.EPH_DTYPE)
    lock = np.zeros((n_rx, ch), F.LOCK_DTYPE)
    lock["flags"] = LOCK_BOTH
    fix = np.zeros((N_LAUNCH, n_rx), F.FIX_DTYPE)
    vel = np.zeros(n_rx, V.VEL_DTYPE)
    kinds, poke = [], {}
    for r in range(n_rx):
        site, kind = names[(r + ch) % len(names)], KINDS[(r + ch) % len(KINDS)]
        drift = (1e-6, -1e-6)[r % 2]
        n = min(ch, 8)
        eps, e = track(site, n, 3 * (r % 3), VELOCITY, drift, N_LAUNCH)
        sats = list(range(n))
        if kind == "singular" and ch >= 4:
            sats = [0, 1, 2, 2]
        slots = [(r + k) % ch for k in range(len(sats))]
        eph[r, slots] = e[sats]
        for k in range(N_LAUNCH):
            obs[k, r, slots] = eps[k]["obs"][sats]
        at = slots[(0, len(slots) - 1, len(slots) // 2)[(r // len(KINDS) + r) % 3]]
        sub = (r // len(KINDS)) % 3
        last = N_LAUNCH - 1
        if kind == "coasting":
            keep = slots[:(3, 1, 0)[sub]]
            for s in slots:
                if s not in keep:
                    obs["flags"][last, r, s] &= ~np.uint32(O.F_VALID)
        elif kind == "starved":
            lock["flags"][r, :] = 0      # (the lock records serve every launch: starved from the first update on, LOST in the third)
        elif kind == "ambiguous":
            obs["tx_ms"][last, r, at] -= (1, -1, 3)[sub]
            obs["flags"][last, r, at] |= O.F_AMBIGUOUS
        elif kind == "faulty_slot":
            row = W.sky(site, n, 3 * (r % 3))[sats[slots.index(at)]][1]
            dop = obs["if_freq_offset_hz"][last, r, at]
            obs[last, r, at] = W.observable(row, eps[last]["rx"], eps[last]["t"], FAULT_M)[0]
            obs["if_freq_offset_hz"][last, r, at] = dop
        elif kind == "faulty_doppler":
            obs["if_freq_offset_hz"][last, r, at] += np.float32(FAULT_HZ)
        elif kind == "bad_state":
            poke[r] = dict(rcv_ms=-1)
        rec = fix_record(eps[0]["rx"], slots, eps[0]["t"], int(e["week"][0]), dtr_s=(0.0, 3e-4)[r % 2])
        for k in range(N_LAUNCH):
            if kind != "fresh":
                fix[k, r] = rec[0]
            elif k == last:
                fix[k, r] = fix_record(eps[k]["rx"], slots, eps[k]["t"], int(e["week"][0]), dtr_s=(0.0, 3e-4)[r % 2])[0]
            else:
                fix["flags"][k, r] = F.F_TOO_FEW
        if r % 2 == 0:
            vel[r] = vel_record(VELOCITY, drift)[0]
        else:
            vel["flags"][r] = V.F_TOO_FEW
        kinds.append(kind)
    c = K.make_cfg(ch, max_coast=MAX_COAST)
    obs, eph, lock = obs.reshape(N_LAUNCH, -1), eph.reshape(-1), lock.reshape(-1)
    state = np.zeros(n_rx, K.STATE_DTYPE)
    want, states, codes, details = [], [], [], []
    for k in range(N_LAUNCH):
        if k == N_LAUNCH - 1:
            for r, fields in poke.items():
                for name, val in fields.items():
                    state[name][r] = val
        d = {}
        rec, state, rc = K.run(c, obs[k], eph, state, n_rx, N_BLOCKS, lock, fix[k], vel, detail=d)
        want.append(rec)
        states.append(state.copy())
        codes.append(rc)
        details.append(d)
    return dict(cfg=c, n_blocks=N_BLOCKS, obs=obs, eph=eph, lock=lock, fix=fix, vel=vel, poke=poke, kinds=kinds, want=want, states=states, codes=codes,
                details=details)


GATE_CLEAR, RINT_CLEAR, SHARE_CLEAR, EL_CLEAR = 1e-3, 1e-3, 1e-7, 1e-3


def decisions_clear(details):
    """every compared decision of a run's launches stands clear of round-off in the restatement: a gate ratio v^2 / (gate^2 s) is not
    within 1e-3 of 1 (relative), a repair's rint argument not within 1e-3 of a half-integer, every pivot share of an update above 1e-7
    (1e3 x the rule's 1e-10), a row's elevation not within 1e-3 rad of 0
    -> the margins found: dict(gate, rint, share, el)"""
    m = dict(gate=np.inf, rint=np.inf, share=np.inf, el=np.inf)
    for d in details:
        for g in (d["gate_pr"], d["gate_dop"]):
            g = g[np.isfinite(g)]
            if g.size:
                m["gate"] = min(m["gate"], float(np.abs(g - 1.0).min()))
        q = d["rint_arg"][np.isfinite(d["rint_arg"])]
        if q.size:
            m["rint"] = min(m["rint"], float(np.abs(np.abs(q - np.floor(q)) - 0.5).min()))
        s = d["shares"][np.isfinite(d["shares"])]
        if s.size:
            m["share"] = min(m["share"], float(s.min()))
        el = d["el"][np.isfinite(d["el"])]
        if el.size:
            m["el"] = min(m["el"], float(np.abs(el).min()))
    assert m["gate"] > GATE_CLEAR and m["rint"] > RINT_CLEAR and m["share"] > SHARE_CLEAR and m["el"] > EL_CLEAR, m
    return m


PARITY_ENV = "GPSX_WKF_PARITY_JSON"      # a path: every labelled compare() records its maxima there (how the profile is written)
INT_FIELDS = ("flags", "n_pr", "n_dop", "n_starved", "pr_mask", "dop_mask", "rej_pr_mask", "rej_dop_mask", "plus_mask", "minus_mask", "rcv_ms", "week",
              "reserved")


def _record_parity(label, worst, n_solved):
    path = os.environ.get(PARITY_ENV)
    if not path or label is None:
        return
    doc = json.load(open(path)) if os.path.exists(path) else {"launches": {}}
    doc["launches"][label] = dict(worst, solved=n_solved)
    doc["what"] = ("largest |device - restatement| in rr, clk_m, height (m) and vel, enu, cdrift_mps (m/s) per compared launch of "
                   "tests/test_gpu_weighted_kf.py, one MI355X; written by weighted_kf_cases.compare under $" + PARITY_ENV)
    doc["largest_m"] = max(max(w[k] for k in ("rr_m", "clk_m", "height_m")) for w in doc["launches"].values())
    doc["largest_mps"] = max(max(w[k] for k in ("vel_mps", "enu_mps", "cdrift_mps")) for w in doc["launches"].values())
    doc["cap_m"], doc["bound_m"] = PARITY_CAP_M, min(8.0 * doc["largest_m"], PARITY_CAP_M)
    doc["cap_mps"], doc["bound_mps"] = PARITY_CAP_MPS, min(8.0 * doc["largest_mps"], PARITY_CAP_MPS)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)


def compare(got, want, label=None, bound_m=None, bound_mps=None):
    """a launch's records against the restatement's: flags, counts, masks, rcv_ms, week equal; records without a solution byte-equal; rr,
    clk_m and height within the position bound, vel, enu and cdrift_mps within the velocity bound, latitude and longitude within the
    position bound over the earth's radius, sigma 1e-5 relative, the two NIS 1e-6 relative (+ 1e-9); nothing non-finite
    -> the per-field maxima (measured, and with a label recorded under $GPSX_WKF_PARITY_JSON, before anything is asserted)"""
    bound_m = PARITY_BOUND_M if bound_m is None else bound_m
    bound_mps = PARITY_BOUND_MPS if bound_mps is None else bound_mps
    for f in ("rr", "clk_m", "vel", "cdrift_mps", "geo", "enu", "sigma", "nis_pr", "nis_dop"):
        assert np.isfinite(got[f]).all(), f
    solved = (want["flags"] & (K.F_INIT | K.F_UPDATED | K.F_COAST)) != 0
    g, w = got[solved], want[solved]
    mx = lambda a: float(np.abs(a).max()) if a.size else 0.0      # noqa: E731
    worst = {"rr_m": mx(g["rr"] - w["rr"]), "clk_m": mx(g["clk_m"] - w["clk_m"]), "height_m": mx(g["geo"][:, 2] - w["geo"][:, 2]),
             "latlon_rad": mx(g["geo"][:, :2] - w["geo"][:, :2]), "vel_mps": mx(g["vel"] - w["vel"]), "enu_mps": mx(g["enu"] - w["enu"]),
             "cdrift_mps": mx(g["cdrift_mps"] - w["cdrift_mps"]),
             "sigma_rel": mx((g["sigma"].astype(np.float64) - w["sigma"]) / np.maximum(np.abs(w["sigma"]), 1e-30)),
             "nis_rel": max(mx((g[f] - w[f]) / (np.abs(w[f]) + 1e-3)) for f in ("nis_pr", "nis_dop"))}
    _record_parity(label, worst, int(solved.sum()))
    for f in INT_FIELDS:
        bad = np.flatnonzero(got[f] != want[f])
        assert bad.size == 0, (label, f, bad[:8], got[f][bad][:8], want[f][bad][:8])
    assert got[~solved].tobytes() == want[~solved].tobytes(), "records without a solution"
    assert max(worst["rr_m"], worst["clk_m"], worst["height_m"]) <= bound_m and worst["latlon_rad"] <= bound_m / 6.0e6, (label, worst)
    assert max(worst["vel_mps"], worst["enu_mps"], worst["cdrift_mps"]) <= bound_mps, (label, worst)
    assert worst["sigma_rel"] <= 1e-5 and worst["nis_rel"] <= 1e-6, (label, worst)
    return worst


def compare_states(got, want, bound_m=None, bound_mps=None):
    """the resident states: the integers equal, x within the bounds, P 1e-6 relative to sqrt(P_ii P_jj)"""
    bound_m = PARITY_BOUND_M if bound_m is None else bound_m
    bound_mps = PARITY_BOUND_MPS if bound_mps is None else bound_mps
    for f in ("rcv_ms", "week", "flags", "n_starved", "n_init", "n_lost", "reserved"):
        assert (got[f] == want[f]).all(), (f, np.flatnonzero(got[f] != want[f])[:8])
    assert np.isfinite(got["x"]).all() and np.isfinite(got["P"]).all()
    assert np.abs(got["x"][:, :4] - want["x"][:, :4]).max() <= bound_m and np.abs(got["x"][:, 4:] - want["x"][:, 4:]).max() <= bound_mps
    d = np.sqrt(np.maximum(np.stack([want["P"][:, K.tri(i, i)] for i in range(8)], -1), 1e-300))
    for i in range(8):
        for j in range(i, 8):
            assert (np.abs(got["P"][:, K.tri(i, j)] - want["P"][:, K.tri(i, j)]) <= 1e-6 * d[:, i] * d[:, j]).all(), (i, j)


# ---- the smoke fixture (tests/golden/wkf_smoke.npz) ------------------------------------------------------------------------------------
SMOKE_LAUNCHES = 3


def smoke_case():
    """one eight-slot Munich receiver at (30, -20, 5) m/s whose clock drifts by 1e-6 s/s, three launches: INIT from its true position
    record and velocity record, two updates; the restatement's last record -> the arrays of the fixture"""
    eps, eph = track("munich", 8, 0, VELOCITY, 1e-6, SMOKE_LAUNCHES)
    fix = fix_record(eps[0]["rx"], range(8), eps[0]["t"], int(eph["week"][0]))
    vel = vel_record(VELOCITY, 1e-6)
    obs = np.stack([e["obs"] for e in eps])
    recs, _ = run_sequence(K.make_cfg(8), list(obs), eph, [fix] * SMOKE_LAUNCHES, [vel] * SMOKE_LAUNCHES)
    last = recs[-1]
    assert [int(r["flags"]) for r in recs] == [K.F_INIT, K.F_UPDATED, K.F_UPDATED] and int(last["n_pr"]) == 8 and int(last["n_dop"]) == 8
    return dict(obs=obs, eph=eph, fix=fix, vel=vel, n_blocks=np.int64(N_BLOCKS), rr=last["rr"], clk_m=last["clk_m"], vel_out=last["vel"],
                cdrift_mps=last["cdrift_mps"], rcv_ms=last["rcv_ms"], week=last["week"], truth_rr=eps[-1]["rx"], truth_vel=np.array(VELOCITY),
                truth_cdrift=np.float64(K.C_LIGHT * 1e-6))


def write_smoke():
    """(`python tests/weighted_kf_cases.py`) writes the fixture"""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wkf_smoke.npz")
    np.savez_compressed(path, **smoke_case())
    return path


# ---- behind the chain from IF samples ---------------------------------------------------------------------------------------------------
def if_cfgs():
    """(gpsx_wfix's, gpsx_wvel's, gpsx_wkf's configuration) for weighted_pvt_cases' four-channel stream: the weighted loops' scale"""
    import weighted_pvt_cases as P
    return F.make_cfg(P.OFFSETS_MS[0], 4), V.make_cfg(4, 4, V.L1CA_WLOOP), K.make_cfg(4, mps_per_hz=V.L1CA_WLOOP)


def if_filter(launches):
    """the three restatements behind one another on [(n_blocks, obs [4], eph [4])] per launch, the filter called after every launch
    -> ([(fix, vel, kf record)] per launch, the state after)"""
    fcfg, vcfg, kcfg = if_cfgs()
    state, prev, out = np.zeros(1, K.STATE_DTYPE), None, []
    for n, obs, eph in launches:
        fix = F.run(fcfg, obs, eph, 1, prev=prev)[0]
        prev = fix
        vel = V.run(vcfg, obs, eph, fix, 1)
        rec, state, rc = K.run(kcfg, obs, eph, state, 1, n, None, fix, vel)
        assert rc == 0
        out.append((fix, vel, rec))
    return out, state


def if_stream_on_restatements():
    """weighted_pvt_cases' stream (a receiver at rest, its clock on GPS time) through the restatements of the whole chain, the filter
    behind them -> dict(flags per launch, speed_mps and cdrift_mps of the last record, position_m: its distance from the truth)"""
    import weighted_pvt_cases as P
    chain, _ = P.chain_on_restatements("moving")
    out, _ = if_filter([(n, obs, eph) for _, n, _, _, obs, eph in chain])
    last = out[-1][2][0]
    return dict(flags=[int(o[2]["flags"][0]) for o in out], speed_mps=float(np.linalg.norm(last["vel"])), cdrift_mps=float(last["cdrift_mps"]),
                position_m=float(np.linalg.norm(last["rr"] - P.RX)))


# ---- bounds -----------------------------------------------------------------------------------------------------------------------
# MEASURED, each on the CPU (tests/test_weighted_kf_reference.py prints them; a GPU-side repeat is bounded at 1.5 x these): see that
# file's tests for what each figure is.
#   moving_median_m: the largest, over the reference test's seeds, of the filter's median 3-D error over the last seven of fourteen launches
#     (3 m of pseudorange noise, eight satellites); gpsx_wfix's restatement on the same records: 3.8 to 7.4 m.
#   coast_outage_m, coast_return_m: the largest error while three, then one satellite are left, and the error of the first launch with
#     all eight back.
#   fault_gated_move_m: what a 150 m range fault moves the position by behind the gate (12.45 m with the gate open).
#   cdrift_mps, clk_m: the largest error of cdrift_mps and clk_m over the last seven launches at drifts of +- 1e-6.
#   week_end_m: the largest error of the noise-free receiver that crosses the week's end.
#   if_speed_mps: |vel| of the last record on weighted_pvt_cases' IF stream (a receiver at rest), the restatements all the way.
MEASURED = {"moving_median_m": 6.0383, "coast_outage_m": 3.54168, "coast_return_m": 1.6543, "fault_gated_move_m": 0.246081, "cdrift_mps": 0.00348504,
            "clk_m": 1.24108, "week_end_m": 0.00430492, "if_speed_mps": 0.069628}
# the device against the restatement: 8 x the largest difference measured on one MI355X over every compared launch of
# tests/test_gpu_weighted_kf.py (profiles/r24_weighted_kf_parity.json: that file run with $GPSX_WKF_PARITY_JSON naming it), capped at the
# project's 1e-4 m for position and clock and 1e-6 m/s for velocity and drift.  Until measured, the caps hold.
# Measured: 1.3039e-8 m (height, ch_per_rx 33, the first update) and 3.3722e-9 m/s (enu, 4 x 67, the last launch); the run behind gpsx_wfde_dev 1.2e-8 m, the IF
# stream's quartet 2.1e-14 m and 2.8e-17 m/s (all in the profile).
PARITY_MEASURED_M = 1.3039e-8
PARITY_MEASURED_MPS = 3.3722e-9
PARITY_CAP_M, PARITY_CAP_MPS = 1e-4, 1e-6
PARITY_BOUND_M = PARITY_CAP_M if PARITY_MEASURED_M is None else min(8.0 * PARITY_MEASURED_M, PARITY_CAP_M)
PARITY_BOUND_MPS = PARITY_CAP_MPS if PARITY_MEASURED_MPS is None else min(8.0 * PARITY_MEASURED_MPS, PARITY_CAP_MPS)


if __name__ == "__main__":
    print(write_smoke())
