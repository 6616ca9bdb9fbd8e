"""What the CPU and GPU tests of the weighted path's lock monitor share (include/gpsx.h gpsx_wlock): fabricated records of the sync
loop with scripted correlator sums (32 distinct streams tiled over the channels, sync states in all three modes behind them), the
thresholds and epochs of the scenario, the scenario itself -- three satellites, one of which sets, and two channels handed PRNs that
are not in the sky -- run on the restatements, and what was measured on it."""
import os
import sys
import tempfile

import numpy as np

import weighted_lock_ref as R
import weighted_sync_cases as K
import weighted_sync_ref as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AHEAD = 4                      # k_wlock's look-ahead in slots (csrc/k_wlock.hip kAhead; tests/test_weighted_lock_reference.py reads it there)
DISTINCT = 32

# ---- fabricated records ----------------------------------------------------------------------------------------------------------
# small epochs and runs, so that a few dozen windows reach every branch
FAB = R.make_cfg(epoch_search=3, epoch_lock=2, code_min=1.5, car_min=0.5, snr_min=2.0, n_good=3, n_bad=2, rearm=3, patience=3)
SPAN = 4                       # blocks per slot; window j of a stream ends with absolute block SPAN j + SPAN - 1
TOP = (1 << 20) - 1


def _level(name, k, j):
    """a window's (IE, QE, IP, QP, IL, QL) at a level of the FAB thresholds; k and j vary the figures, never the verdicts"""
    v = (7 * k + 3 * j) % 41
    sign = -1 if (j * (k + 1)) % 3 == 0 else 1          # data bits: |IP| and the squares do not see them
    if name == "good":         # code 6, carrier 0.99, snr in the hundreds (0 / 0 -> 0 where |IP| is constant and QP is 0: level "flat")
        return (400 + v, 20, sign * (1000 + v), 50 - v, 400 - v, -20)
    if name == "nocode":       # the prompt no stronger than the taps: code 1.1, carrier 0
        return (400, 20 + v, sign * 300, 300, 400, -20)
    if name == "nocar":        # a code that is there, the carrier in quadrature: code 11, carrier below 0
        return (300, 20, sign * (700 + v), 720 + v, 300, -20 + v)
    if name == "flat":         # QP = 0 and |IP| constant: K P == A A
        return (200, 0, sign * 500, 0, 200, 0)
    if name == "notaps":       # E + L == 0
        return (0, 0, sign * (1000 + v), 50, 0, 0)
    if name == "noprompt":     # P == 0 (and A == 0)
        return (400, 20, 0, 0, 400 + v, -20)
    if name == "top":          # the largest sums that are accumulated
        return (TOP, -TOP, sign * TOP, TOP - v, -TOP, TOP)
    if name == "over":         # one sum too large: not accumulated
        return ((400, 20, 1 << 20, 50, 400, -20), (400, 20, 1000, 50, 400, -(1 << 20)), (-(1 << 31), 20, 1000, 50, 400, -20))[j % 3]
    raise KeyError(name)


# a stream's script: segments (locked, level, windows) repeated for ever.  With FAB: LOCKED epochs are 2 windows, SEARCH epochs 3,
# three good epochs set an indicator, two bad ones clear it, three bad carrier verdicts without CARRIER ask for a re-arm
SCRIPTS = {
    0: [(1, "good", 1)],                                          # CODE and CARRIER
    1: [(0, "good", 1)],                                          # CODE in SEARCH, never CARRIER
    2: [(1, "good", 4), (1, "nocode", 2)],                        # n_good - 1 good epochs, then a bad one: never set
    3: [(1, "good", 8), (1, "nocode", 2)],                        # set, then n_bad - 1 bad epochs, then a good one: never lost
    4: [(1, "good", 8), (1, "nocode", 4)],                        # set, lost (code and carrier), a re-arm pending; again and again
    5: [(1, "good", 3), (0, "good", 2), (1, "good", 1), (0, "good", 4)],   # the kind changes in mid-epoch
    6: [(1, "notaps", 1)],                                        # E + L == 0
    7: [(1, "noprompt", 1)],                                      # P == 0
    8: [(1, "flat", 1)],                                          # K P - A A == 0: snr 0, a patience run that completes
    9: [(1, "nocar", 4), (1, "good", 2)],                         # a patience run that ends one short
    10: [(1, "nocar", 1)],                                        # a patience run that completes every three epochs
    11: [(1, "top", 1)],                                          # 2^20 - 1 everywhere: the largest exact sums
    12: [(1, "good", 4), (1, "over", 1)],                         # a record at 2^20: counted, not accumulated, the epoch goes on
    13: [(1, "good", 2), (1, "empty", 1)],                        # empty slots
    14: [(1, "good", 3), (1, "outside", 1), (0, "good", 1), (1, "before", 1)],   # end_block out of range in a WINDOW record
    15: [(0, "nocode", 4), (1, "nocar", 7)],                      # a SEARCH window zeroes the patience run one short, then it completes
}


def _script(k):
    if k in SCRIPTS:
        return SCRIPTS[k]
    rng = np.random.default_rng(500 + k)     # streams 16 .. 31: mixtures
    names = ("good", "good", "good", "nocode", "nocar", "flat", "top", "over", "empty", "notaps", "noprompt")
    return [(int(rng.integers(0, 4) != 0), names[int(rng.integers(0, len(names)))], int(rng.integers(1, 9))) for _ in range(12)]


def _window(k, j):
    """stream k's window j -> (locked, level)"""
    script = _script(k)
    j %= sum(n for _, _, n in script)
    for locked, name, n in script:
        if j < n:
            return locked, name
        j -= n


def fab_records(first_window, n_slots, n_ch):
    """the records of one launch of n_slots slots (SPAN n_slots blocks) whose first slot holds every stream's window first_window"""
    rec = Y.empty_records(n_slots, min(n_ch, DISTINCT))      # (a stream's records are the same on every tile)
    n_blocks = SPAN * n_slots
    for k in range(rec.shape[1]):
        for slot in range(n_slots):
            j = first_window + slot
            locked, name = _window(k, j)
            if name == "empty":
                continue
            end = SPAN * slot + SPAN - 1
            if name == "outside":
                end, name = n_blocks + (j % 2) * 100000, "nocode"
            elif name == "before":
                end, name = -1 - (j % 2) * 7, "nocode"
            r = rec[slot, k]
            r["w"]["iq"] = _level(name, k, j)
            r["w"]["code_phase_fine"], r["w"]["if_freq_offset_hz"], r["w"]["if_freq_accum"] = 100.0 + k, -3.0 * j, 77 * j + k
            r["end_block"] = end
            r["flags"] = Y.F_WINDOW | (Y.F_LOCKED if locked else 0) | (Y.F_BIT if locked and j % 5 == 4 else 0)
            r["bit_ip"] = 12345 if locked and j % 5 == 4 else 0
    return np.ascontiguousarray(rec[:, np.arange(n_ch) % DISTINCT])


def fab_sync_states(n_ch):
    """sync states with something in every field a re-arm writes; channel ch (stream ch % 32, tile ch // 32) is in mode
    (stream + tile) % 3: from 96 channels on every stream meets SEARCH, WAIT and LOCKED; streams 4, 8, 10 and 15, which ask for
    re-arms, start in WAIT, LOCKED, WAIT and SEARCH"""
    st = K.mixed_states(n_ch, 11, kinds=(1,))
    rng = np.random.default_rng(12)
    st["mode"] = (np.arange(n_ch) % DISTINCT + np.arange(n_ch) // DISTINCT) % 3
    st["edge"] = np.arange(n_ch) % 20
    st["bit_ip"] = rng.integers(-200000, 200001, n_ch)
    st["win_n"] = 1 + np.arange(n_ch) % 3
    st["loop"]["n_updates"] = rng.integers(1, 1000, n_ch)
    return st


def fab_run(launches, n_ch, cfg=FAB, warm=0, st=None, sync=None):
    """launches: slot counts of consecutive launches, the first one starting with window `warm` on states that the restatement
    left after windows 0 .. warm - 1 (one launch, this cfg, the same sync states)
    -> (states before, sync states before, [(records, n_blocks, lock records wanted)], states wanted, sync states wanted)"""
    st = np.zeros(n_ch, R.STATE_DTYPE) if st is None else st.copy()
    sync = fab_sync_states(n_ch) if sync is None else sync.copy()
    if warm:
        _, bad = R.run(fab_records(0, warm, n_ch), SPAN * warm, st, cfg, sync)
        assert not bad
    st0, sync0 = st.copy(), sync.copy()
    out, at = [], warm
    for n_slots in launches:
        rec = fab_records(at, n_slots, n_ch)
        lock, bad = R.run(rec, SPAN * n_slots, st, cfg, sync)
        assert not bad
        out.append((rec, SPAN * n_slots, lock))
        at += n_slots
    return st0, sync0, out, st, sync


def tile96(a, n_ch):
    """channel ch of the fabricated tables equals channel ch % 96 (the same stream, the same sync mode)"""
    return a[..., np.arange(n_ch) % 96].copy() if a.ndim > 1 else a[np.arange(n_ch) % 96].copy()


# ---- the scenario's thresholds and epochs -------------------------------------------------------------------------------------------
# SEARCH epochs of 25 windows of 4 blocks (100 ms), LOCKED epochs of 10 windows of 20 (200 ms: with 5 the noise-only code ratio
# reaches 2.57 on these seeds, where the weakest SEARCH epoch of a satellite gives 2.66).  Each threshold sits between the largest
# noise-only and the smallest present-satellite figure of MEASURED below, the geometric way for snr; two epochs set, two clear
EPOCH_SEARCH, EPOCH_LOCK = 25, 10
CODE_MIN, CAR_MIN, SNR_MIN = 2.3, 0.75, 6.0
N_GOOD, N_BAD = 2, 2
PATIENCE = 5


def scenario_cfg(rearm=0):
    return R.make_cfg(EPOCH_SEARCH, EPOCH_LOCK, CODE_MIN, CAR_MIN, SNR_MIN, N_GOOD, N_BAD, rearm, PATIENCE)


# ---- the scenario --------------------------------------------------------------------------------------------------------------------
N_MS, GONE_AT, LAUNCH = 3000, 2000, 500
VANISHING = 1                                        # K.SATS[1], PRN 19, is absent from block 2000 on
ABSENT = [(3, 5000.0, 900.0), (25, 9000.5, -1500.0)]   # (prn, code phase, carrier offset) of the channels whose PRN is not in the stream
N_CH = len(K.SATS) + len(ABSENT)
HALF_MS = GONE_AT                                    # the C/N0 runs at half the amplitude end where the satellite would set
SEEDS = K.SEEDS


def scenario_blocks(seed, amp=K.AMPLITUDE, n_ms=N_MS):
    """K.scenario's satellites and data bits; from block GONE_AT on a second synth.make_if piece without satellite VANISHING, carrier
    and code continuous through start_ms, its noise from a seed of its own (a piece's noise is positioned by the piece's own index)"""
    from stm32f4_sdr_gps_amd import synth
    sats = []
    for j, (prn, fd, delay, edge, phase) in enumerate(K.SATS):
        bits = np.random.default_rng(1000 * (j + 1) + seed).integers(0, 2, N_MS // 20 + 2) * 2.0 - 1.0
        sats.append(synth.Sat(prn, fd, delay + 16368.0 * edge, amp, phase, nav_bits=bits))
    first = synth.make_if(min(n_ms, GONE_AT), sats, noise_amp=1.0, seed=seed, two_bit=True)
    if n_ms <= GONE_AT:
        return first
    rest = synth.make_if(n_ms - GONE_AT, [s for j, s in enumerate(sats) if j != VANISHING], noise_amp=1.0, seed=7000 + seed, start_ms=GONE_AT, two_bit=True)
    return np.concatenate([first, rest])


def scenario_states(seed):
    """K.handover_states for the three satellites, and the two absent PRNs' hand-overs"""
    return np.concatenate([K.handover_states(seed)] + [Y.handover(prn, phase, hz) for prn, phase, hz in ABSENT])


def launches(n_ms=N_MS):
    return [(at, min(LAUNCH, n_ms - at)) for at in range(0, n_ms, LAUNCH)]


_memo = {}


def _worker(args):
    """(in a process of its own) one channel through the sync loop's and the lock monitor's restatements, launch after launch"""
    path, n_ms, st_bytes, cfg = args
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from oracle import pyoracle
    orc = pyoracle.Oracle()
    blks = np.load(path, mmap_mode="r")
    sync = np.frombuffer(bytearray(st_bytes), Y.STATE_DTYPE)
    st = np.zeros(1, R.STATE_DTYPE)
    recs, locks, modes, traces = [], [], [], []
    for at, n in launches(n_ms):
        rec = Y.run(orc, blks[at:at + n], sync, K.sync_cfg())
        trace = {}
        lock, bad = R.run(rec, n, st, cfg, sync, traces=trace)
        assert not bad
        recs.append(rec)
        locks.append(lock)
        modes.append(int(sync["mode"][0]))
        traces.append([(at + t[0],) + t[1:] for t in trace.get(0, [])])
    return recs, locks, modes, traces, st.tobytes(), sync.tobytes()


def runs(jobs):
    """jobs: [(seed, amplitude, n_ms, rearm, channels)] -> per job {channel: (records per launch [slots][1], lock records per launch
    [1], the sync mode after each launch, the epochs per launch [(absolute end block, locked, K, code_ratio, car_ratio, snr, flags)],
    lock state, sync state)}.  Channels share nothing: one spawned CPU-only process per job and channel, those not yet cached side
    by side on the CPUs this process may use, eight at the most (a channel's 3000 blocks are 5 s of Python)"""
    import multiprocessing
    from concurrent.futures import ProcessPoolExecutor
    todo = [(seed, amp, n_ms, rearm, ch) for seed, amp, n_ms, rearm, chans in jobs for ch in chans if (seed, amp, n_ms, rearm, ch) not in _memo]
    if todo:
        tmp = _memo.setdefault("tmp", tempfile.TemporaryDirectory(prefix="weighted_lock_"))
        tasks = []
        for seed, amp, n_ms, rearm, ch in todo:
            path = os.path.join(tmp.name, f"blocks_{seed}_{amp}_{n_ms}.npy")
            if not os.path.exists(path):
                np.save(path, scenario_blocks(seed, amp, n_ms))
            tasks.append((path, n_ms, scenario_states(seed)[ch:ch + 1].tobytes(), scenario_cfg(rearm)))
        workers = max(1, min(len(tasks), len(os.sched_getaffinity(0)), 8))
        with ProcessPoolExecutor(workers, mp_context=multiprocessing.get_context("spawn")) as ex:
            for key, (recs, locks, modes, traces, st, sync) in zip(todo, ex.map(_worker, tasks)):
                _memo[key] = (recs, locks, modes, traces, np.frombuffer(st, R.STATE_DTYPE).copy(), np.frombuffer(sync, Y.STATE_DTYPE).copy())
    return [{ch: _memo[(seed, amp, n_ms, rearm, ch)] for ch in chans} for seed, amp, n_ms, rearm, chans in jobs]


PRESENT = tuple(range(len(K.SATS)))
HEALTHY = tuple(c for c in PRESENT if c != VANISHING)
EVERY = tuple(range(N_CH))


def all_jobs():
    """what the CPU test needs, asked for at once so that it runs side by side: every seed without re-arm on the five channels and
    with it on the three satellites', and the three satellites' channels at half the amplitude"""
    return ([(seed, K.AMPLITUDE, N_MS, 0, EVERY) for seed in SEEDS] + [(seed, K.AMPLITUDE, N_MS, 1, PRESENT) for seed in SEEDS] +
            [(seed, K.AMPLITUDE / 2, HALF_MS, 0, PRESENT) for seed in SEEDS])


def analytic_cn0(amp):
    """the synthesiser's C/N0 in dB-Hz before quantisation: signal power a^2 / 2 over uniform noise of variance 1 / 3 in fs / 2"""
    return 10.0 * np.log10(0.75 * amp * amp * 16.368e6)


# ---- what was measured on the restatements (tests/test_weighted_lock_reference.py measures it again and compares) ---------------------
LOCKED_FROM = 1200             # every satellite's channel has been LOCKED for a whole epoch by here, on every seed


def _epochs(run):
    return [e for tr in run[3] for e in tr]


def _began(e):
    """the first block of an epoch: its windows are K.N_COH_LOCK or K.N_COH_SEARCH blocks long"""
    return e[0] + 1 - e[2] * (K.N_COH_LOCK if e[1] else K.N_COH_SEARCH)


def measure(full, half):
    """full: runs() of the rearm = 0 jobs on EVERY channel per seed, half: of the half-amplitude jobs -> the figures of MEASURED.
    Present: the satellites' channels, of the vanishing one the epochs that end before GONE_AT; carrier and snr on LOCKED epochs that
    began at or after LOCKED_FROM.  Noise only: the absent PRNs' channels, and the vanishing one's epochs that began at or after GONE_AT"""
    pres, noise = dict(code=[], car=[], snr=[]), dict(code=[], car=[], snr=[])
    latency = []
    for res in full:
        for ch in EVERY:
            for e in _epochs(res[ch]):
                there = ch in HEALTHY or (ch == VANISHING and e[0] < GONE_AT)
                gone = ch not in PRESENT or (ch == VANISHING and _began(e) >= GONE_AT)
                for to, use in ((pres, there), (noise, gone)):
                    if use:
                        to["code"].append(e[3])
                        if e[1] and (to is noise or _began(e) >= LOCKED_FROM):
                            to["car"].append(e[4])
                            to["snr"].append(e[5])
        lost = [e[0] for e in _epochs(res[VANISHING]) if e[0] >= GONE_AT and not e[6] & R.F_CODE]
        latency.append(lost[0] + 1 - GONE_AT)
    out = {}
    for name in ("code", "car", "snr"):
        out[name + "_present_min"], out[name + "_noise_max"] = round(min(pres[name]), 3), round(max(noise[name]), 3)
    out["loss_latency_blocks"] = tuple(latency)
    for name, runs_, amp, upto in (("full", full, K.AMPLITUDE, GONE_AT), ("half", half, K.AMPLITUDE / 2, HALF_MS)):
        est = [v for res in runs_ for ch in PRESENT for e in _epochs(res[ch]) if e[1] and _began(e) >= LOCKED_FROM and e[0] < upto and e[5] > 0
               for v in [10.0 * np.log10(e[5] / (K.N_COH_LOCK * 0.001))]]
        out["cn0_" + name] = dict(mean=round(float(np.mean(est)), 2), sd=round(float(np.std(est)), 2), epochs=len(est), analytic=round(float(analytic_cn0(amp)), 2),
                                  off=round(float(np.mean(est) - analytic_cn0(amp)), 2))
    return out


MEASURED = dict(
    code_present_min=2.66, code_noise_max=1.94, car_present_min=0.973, car_noise_max=0.572, snr_present_min=42.437, snr_noise_max=1.059,
    loss_latency_blocks=(451, 451, 451),
    cn0_full=dict(mean=37.19, sd=1.65, epochs=27, analytic=41.77, off=-4.58),
    cn0_half=dict(mean=31.47, sd=1.67, epochs=27, analytic=35.75, off=-4.29),
)

# ---- states out of range, one field each, and states at the very ends of the ranges -------------------------------------------------
BAD_FIELDS = [("flags", 32), ("flags", 1 << 31), ("reserved", 1), ("blocks_seen", -1), ("blocks_seen", (1 << 62) + 1), ("last_epoch_end_p1", -1),
              ("last_epoch_end_p1", (1 << 62) + 1), ("epoch_n", 1024), ("last_k", 1025), ("code_good", 256), ("code_bad", 256), ("car_good", 256),
              ("car_bad", 1 << 31), ("sum_a", -1), ("sum_a", (1 << 30) + 1), ("sum_p", -1), ("sum_p", (1 << 51) + 1), ("sum_e", -1),
              ("sum_e", (1 << 51) + 1), ("sum_l", -(1 << 63)), ("sum_l", (1 << 51) + 1), ("sum_d", (1 << 51) + 1), ("sum_d", -(1 << 51) - 1)]
GOOD_EDGES = [("blocks_seen", 1 << 62), ("last_epoch_end_p1", 1 << 62), ("epoch_n", 1023), ("last_k", 1024), ("code_good", 255), ("car_bad", 255),
              ("sum_a", 1 << 30), ("sum_p", 1 << 51), ("sum_e", 1 << 51), ("sum_l", 1 << 51), ("sum_d", -(1 << 51)), ("false_run", 0xFFFFFFFF),
              ("last_snr", np.nan), ("last_code_ratio", np.inf), ("flags", 31), ("n_range", 0xFFFFFFFF)]
