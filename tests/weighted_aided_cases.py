"""What the CPU and GPU tests of the carrier-aided weighted loops share (include/gpsx.h gpsx_track_loop_weighted_aided,
gpsx_track_loop_weighted_sync_aided): one satellite at +-4500 Hz whose code slides with its Doppler, the orbit chain of
tests/weighted_pvt_cases.py through the aided restatement, the shapes and states of the byte-for-byte comparisons, and the numbers
measured on the restatement with the bounds made of them.  Test infrastructure; nothing here is product code."""
import os
import sys

import numpy as np

import weighted_aided_ref as A
import weighted_loop_cases as S
import weighted_loop_ref as L
import weighted_pvt_cases as P
import weighted_sync_cases as K
import weighted_sync_ref as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- one satellite with a sliding code -------------------------------------------------------------------------------------------
PRN, D0, CARRIER_PHASE, AMPLITUDE, NOISE_SEED = 7, 9000.0, 0.4, 0.3, 1
DOPPLERS = (4500.0, -4500.0)
SLIDE = 16.0 / 1540.0                  # samples of code per second and Hz, towards smaller delays
HANDOVER = (2.0, 7.0)                  # the truth + (samples, Hz)
N_BLOCKS = 2200
PULL_IN_MS = S.PULL_IN_MS              # 200 blocks of weighted_loop_cases.PULL_IN, then STEADY
FIRST_WINDOW = 25                      # the steady phase's windows from this one on are measured

_memo = {}


def delay_at(fd, n):
    """the code delay in samples at sample n of the stream"""
    return D0 - fd * SLIDE * np.asarray(n, np.float64) / 16368000.0


def sliding_blocks(fd, n_ms=N_BLOCKS):
    """[n_ms][4092] two-bit blocks of PRN 7 at IF + fd with the code delay of delay_at, amplitude 0.3 in uniform +-1 noise"""
    key = ("blocks", fd, n_ms)
    if key not in _memo:
        from stm32f4_sdr_gps_amd import synth
        code = 1.0 - 2.0 * synth.ca_code(PRN).astype(np.float64)
        out = np.zeros((n_ms, 4092), np.uint8)
        for m0 in range(0, n_ms, 8):
            m1 = min(n_ms, m0 + 8)
            rng = synth.noise_generator(NOISE_SEED, m0 * synth.SAMPLES_PER_MS)
            n = np.arange(m0 * synth.SAMPLES_PER_MS, m1 * synth.SAMPLES_PER_MS, dtype=np.float64)
            x = rng.uniform(-1.0, 1.0, n.shape)
            chip = np.floor((n - delay_at(fd, n)) / 16.0).astype(np.int64) % synth.CHIPS
            x = x + AMPLITUDE * code[chip] * np.cos(2.0 * np.pi * ((synth.IF_HZ + fd) / synth.FS_HZ) * n + CARRIER_PHASE)
            sign, mag = (x >= 0).astype(np.uint8).reshape(m1 - m0, -1), (np.abs(x) > 0.6).astype(np.uint8).reshape(m1 - m0, -1)
            for i in range(m1 - m0):
                out[m0 + i] = synth.pack_2bit(sign[i], mag[i])
        _memo[key] = out
    return _memo[key]


def handover_state(fd):
    return L.handover(PRN, D0 + HANDOVER[0], fd + HANDOVER[1])


def scenario_run(oracle, fd, code_per_hz, n_ms=N_BLOCKS):
    """the scenario on the restatement, once per process: PULL_IN over the first 200 blocks, STEADY over the rest
    -> (pull-in records, steady records, state after the pull-in, state at the end)"""
    key = ("run", fd, float(code_per_hz), n_ms)
    if key not in _memo:
        blocks = sliding_blocks(fd, n_ms)
        st = handover_state(fd)
        pull = A.run(oracle, blocks[:PULL_IN_MS], st, L.make_cfg(**S.PULL_IN), code_per_hz)
        mid = st.copy()
        steady = A.run(oracle, blocks[PULL_IN_MS:], st, L.make_cfg(**S.STEADY), code_per_hz)
        _memo[key] = (pull, steady, mid, st.copy())
    return _memo[key]


def steady_errors(fd, steady, at_middle_of_next=False):
    """per steady window: the recorded code phase minus the true delay at the record's instant (the window's end) -- or, with
    at_middle_of_next, half a window later --, samples"""
    n_coh = S.STEADY["n_coh"]
    ends = PULL_IN_MS + (np.arange(len(steady)) + 1.0) * n_coh + (0.5 * n_coh if at_middle_of_next else 0.0)
    err = steady["code_phase_fine"][:, 0].astype(np.float64) - delay_at(fd, ends * 16368.0) % 16368.0
    return (err + 8184.0) % 16368.0 - 8184.0


def prompt_20ms(steady):
    """|IP + j QP| of every steady window"""
    return np.hypot(steady["iq"][:, 0, 2].astype(np.float64), steady["iq"][:, 0, 3].astype(np.float64))


# ---- the orbit chain of weighted_pvt_cases through the aided sync restatement -----------------------------------------------------
HANDOVERS = (P.HANDOVER, S.HANDOVER[3])      # weighted_pvt_cases.HANDOVER = (3, 12.5) and (2, 7)


def orbit_blocks(n):
    """the first n blocks of weighted_pvt_cases' stream: a slice of the whole stream where this process has it, synthesised on their
    own otherwise (the synthesiser's samples do not depend on the length)"""
    if n == P.N_BLOCKS or "stream" in P._memo:
        return P.blocks()[:n]
    if ("orbit", n) not in _memo:
        _memo[("orbit", n)] = P.pc.make_if_from_orbits(n, P.sats(), P.RX, P.TOW0, amp=P.AMPLITUDE, noise_amp=P.NOISE_AMP, seed=P.NOISE_SEED,
                                                       cycle=P.CYCLE, two_bit=True, mag_threshold=P.MAG_THRESHOLD)[0]
    return _memo[("orbit", n)]


def _blocks_file(n):
    """those blocks as a .npy file in a temporary directory, for the worker processes to map"""
    if n == P.N_BLOCKS:
        return P._blocks_file()
    if ("file", n) not in _memo:
        import tempfile
        _memo[("tmp", n)] = tempfile.TemporaryDirectory(prefix="weighted_aided_")
        _memo[("file", n)] = os.path.join(_memo[("tmp", n)].name, "blocks.npy")
        np.save(_memo[("file", n)], orbit_blocks(n))
    return _memo[("file", n)]


def _sync_worker(args):
    """(in a process of its own) the aided sync restatement on one channel's state over consecutive launches"""
    path, at, launches, st_bytes, cfg, code_per_hz = args
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from oracle import pyoracle
    orc = pyoracle.Oracle()
    blks = np.load(path, mmap_mode="r")
    st = np.frombuffer(bytearray(st_bytes), Y.STATE_DTYPE)
    out = []
    for n in launches:
        out.append(A.run_sync(orc, blks[at:at + n], st, cfg, code_per_hz))
        at += n
    return out, st.tobytes()


def sync_on_restatement(jobs, code_per_hz=A.WAID_L1CA):
    """weighted_pvt_cases.sync_on_restatement with the aided restatement: jobs [(first block, launch lengths, states, cfg)]
    -> [([records per launch], states after)]"""
    import multiprocessing
    from concurrent.futures import ProcessPoolExecutor
    tasks = [(_blocks_file(max(at + sum(launches) for at, launches, _, _ in jobs)), at, tuple(launches), st[c:c + 1].tobytes(), cfg, float(code_per_hz)) for at, launches, st, cfg in jobs for c in range(len(st))]
    workers = max(1, min(len(tasks), len(os.sched_getaffinity(0)), 8))
    with ProcessPoolExecutor(workers, mp_context=multiprocessing.get_context("spawn")) as ex:
        done = list(ex.map(_sync_worker, tasks))
    out, k = [], 0
    for at, launches, st, cfg in jobs:
        mine, k = done[k:k + len(st)], k + len(st)
        out.append(([np.concatenate([m[0][i] for m in mine], axis=1) for i in range(len(launches))],
                    np.concatenate([np.frombuffer(m[1], Y.STATE_DTYPE) for m in mine])))
    return out


def chains_on_restatements(handovers=HANDOVERS, launches=P.LAUNCHES):
    """the orbit stream with the lock gains STILL (0.5, 40) and GPSX_WAID_L1CA through the aided sync restatement and then the word,
    observable and ephemeris restatements, per hand-over, side by side, once per process
    -> [([(first block, n, records, words, observables, ephemeris records)], states at the end)]"""
    todo = [tuple(e) for e in handovers if ("chain", tuple(e), tuple(launches)) not in _memo]
    if todo:
        runs = sync_on_restatement([(0, launches, P.handover(e), P.sync_cfg(P.STILL)) for e in todo])
        for e, (recs, after) in zip(todo, runs):
            st = dict(P.fresh_states(), sync=after)
            out, at = [], 0
            for n, rec in zip(launches, recs):
                out.append((at, n, rec) + P.after_sync(rec, n, st))
                at += n
            _memo[("chain", e, tuple(launches))] = (out, st)
    return [_memo[("chain", tuple(e), tuple(launches))] for e in handovers]


def tx_residuals(obs, block):
    """the four transmit-time errors at `block` and the same minus their mean (a lag model of zero), samples"""
    err = P.tx_errors(obs, block)
    return err, err - err.mean()


# ---- the byte-for-byte comparisons: launch shapes, states, configurations ----------------------------------------------------------
# (n_ch, cpw, workgroups, channels of the last active wave, idle waves of the last workgroup), as weighted_loop_cases.SHAPES: the
# smallest shapes that reach every lane geometry of plan_track_loop_weighted -- cpw 1 with a second workgroup of three channels and an
# idle wave; cpw 2, the last wave holding one; cpw 16, the last wave holding three
SHAPES = [(7, 1, 2, 1, 1), (8195, 2, 1025, 1, 2), (70003, 16, 1094, 3, 0)]
ROWS = {r[0]: r[1:] for r in SHAPES}
DISTINCT = 32
SYNC_BLOCKS, SYNC_PAIR = 48, (4, 20)
LOOP_RUNS = ((40, S.STEADY), (3, S.REFERENCE_1MS))       # (blocks, gains with their n_coh)
# channels whose code phase sits within one aiding step of an end of [0, 16368): (channel, phase, carrier offset), LOCKED at a bit's
# first block, so that their first window is 20 blocks and the step (code_per_hz x 5000 Hz x 20 ms) 1.04 samples; on noise (a PRN the
# stream does not hold), where the DLL's own step is a few tenths of a sample.  A positive offset steps the phase down.
SEAM = [(7, 0.5, 5000.0), (11, 0.45, 4800.0), (15, 16367.5, -5000.0), (19, 16367.55, -4800.0), (23, 0.55, 4900.0), (27, 16367.45, -4900.0),
        (3, 0.5, -5000.0), (31, 16367.5, 5000.0)]


def tabled(n_ch):
    """cpw of a launch the GPU tests make, from the compiled plan header -- which must be the row above, geometry included"""
    assert n_ch in ROWS, f"{n_ch} channels are launched but not in tests/weighted_aided_cases.py"
    cpw, groups = S.plans([n_ch])[0]
    assert (cpw, groups) == ROWS[n_ch][:2] and S.geometry(n_ch, cpw, groups) == ROWS[n_ch][2:]
    return cpw


def parity_states(n, seed):
    """n sync states that repeat DISTINCT: weighted_sync_cases.mixed_states (modes, edges and open windows mixed; offsets of both
    signs up to 5 kHz) with the SEAM channels set on noise, LOCKED with nothing open -> (states, distinct)"""
    distinct = K.mixed_states(DISTINCT, seed)
    for ch, phase, hz in SEAM:
        one = Y.handover(K.PRNS[ch % len(K.PRNS)], phase, hz, accum=ch * 0x01234567)
        one["mode"] = Y.LOCKED
        distinct[ch] = one[0]
    m = min(n, DISTINCT)
    return distinct[np.arange(n) % m].copy(), m


def sync_cfg():
    return Y.make_cfg(SYNC_PAIR[0], SYNC_PAIR[1], S.PULL_IN, S.STEADY, 1, (5, 4))


def loop_cfg(gains):
    return L.make_cfg(gains["n_coh"], True, 8, gains["dll"], gains["pll"], gains["fll"])


def parity_case(oracle, what, n_ch, code_per_hz=A.WAID_L1CA):
    """what: "sync" or an index into LOOP_RUNS -> (blocks, states before [n_ch], cfg, records wanted, states wanted), the
    restatement run on the distinct channels only and tiled, once per process"""
    distinct = min(n_ch, DISTINCT)
    key = ("parity", what, distinct, float(code_per_hz))
    if key not in _memo:
        st0, _ = parity_states(distinct, 41)
        if what == "sync":
            blocks, cfg = K.strong_blocks(SYNC_BLOCKS, seed=9), sync_cfg()
            first = st0.copy()
            rec = A.run_sync(oracle, blocks, first, cfg, code_per_hz)
        else:
            n, gains = LOOP_RUNS[what]
            blocks, cfg = K.strong_blocks(n, seed=9), loop_cfg(gains)
            st0 = np.ascontiguousarray(st0["loop"])
            first = st0.copy()
            rec = A.run(oracle, blocks, first, cfg, code_per_hz)
        _memo[key] = (blocks, st0, cfg, rec, first)
    blocks, st0, cfg, rec, first = _memo[key]
    idx = np.arange(n_ch) % distinct
    return blocks, st0[idx].copy(), cfg, np.ascontiguousarray(rec[:, idx]), first[idx].copy()


def seam_wraps(oracle):
    """the wraps the aiding term causes on the SEAM channels in the sync case: {"down", "up"} -> [(channel, end block)].  Every
    window of those channels is recomputed from the restatement's own records (the state before it, its sums) with the factor and
    with 0: counted where the phase crosses that end of [0, 16368) with the factor and does not without it."""
    _, st0, cfg, rec, _ = parity_case(oracle, "sync", DISTINCT)
    seen = {"down": [], "up": []}
    for ch, _, _ in SEAM:
        phase, hz, dll_err = (st0["loop"][f][ch] for f in ("code_phase_fine", "if_freq_offset_hz", "dll_err"))
        for u in np.nonzero(rec["flags"][:, ch] & Y.F_WINDOW)[0]:
            r = rec[u, ch]
            assert int(r["flags"]) & Y.F_LOCKED
            gains = dict(cfg["lock"], n_coh=SYNC_PAIR[1])
            with np.errstate(all="ignore"):
                got, d = A.aided_phase(phase, dll_err, r["w"]["iq"], gains, hz, A.WAID_L1CA)
                plain, _ = A.aided_phase(phase, dll_err, r["w"]["iq"], gains, hz, 0.0)
            assert got.tobytes() == r["w"]["code_phase_fine"].tobytes(), (ch, u)
            if float(phase) < 100.0 and float(plain) < 100.0 and float(got) > 16268.0:
                seen["down"].append((ch, int(r["end_block"])))
            if float(phase) > 16268.0 and float(plain) > 16268.0 and float(got) < 100.0:
                seen["up"].append((ch, int(r["end_block"])))
            phase, hz, dll_err = r["w"]["code_phase_fine"], r["w"]["if_freq_offset_hz"], d
    return seen


SPLIT_BLOCKS, SPLIT_PIECES, SPLIT_LEAVES_WAIT = 130, (37, 1, 92), (11, 37)      # (channel, block): inside the one-block piece


def split_states():
    """twelve mixed sync states for the split-launch comparison (sync_bits = 1), the last of them made to leave WAIT at block 37, the
    one block of the second piece: a SEARCH on PRN 7 whose round ends at block 25 with a candidate that outweighs anything 130 blocks
    can add (2^50 against 2^49 opposite, in agreement with the round before), so that it is accepted with edge 0 and, ms_count being
    3 at the start, waits from block 26 to the first block at which the counter is 0"""
    st = K.mixed_states(12, 5)
    ch, block = SPLIT_LEAVES_WAIT
    one = Y.handover(K.STRONG[0][0], K.STRONG[0][2], K.STRONG[0][1])
    one["ms_count"], one["search_n"] = 3, 40 - 26
    edge = (3 + block) % 20
    one["e"][0][edge], one["e"][0][(edge + 10) % 20], one["prev_best_p1"] = 1 << 50, 1 << 49, edge + 1
    st[ch] = one[0]
    return st


def split_cfg():
    return Y.make_cfg(4, 20, S.PULL_IN, S.STEADY, 1, (5, 4))


def bad_loop_states():
    """twelve 40-byte loop states, three of them bad: a PRN of 0, of 211, and a NaN code phase"""
    st = np.ascontiguousarray(K.mixed_states(12, 4)["loop"])
    st["prn"][2], st["prn"][6] = 0, 211
    st["code_phase_fine"][5] = np.nan
    return st, (2, 5, 6)


# ---- measured on the restatement; every bound is 1.5 x the value measured (EXPERIMENTS.md, "Carrier aiding of the weighted code loop") --
# scenario_error: per Doppler the largest |code error| -- the recorded phase minus the true delay at the record's instant -- over the
#   steady windows from FIRST_WINDOW on of the aided run (2200 blocks).  Its mean is +0.40 samples at +4500 Hz and +1.50 at -4500 Hz:
#   against the delay half a window later (the middle of the window the phase is used for) +0.87 and +1.03, the header's half-window
#   term (0.47 samples at 4500 Hz) on either side of an offset of about 0.95 samples that all Dopplers share.
# prompt_ratio: the unaided STEADY run's mean 20 ms prompt over the last ten windows / the aided run's (the code is lost unaided:
#   its error is +19.3 / -17.3 samples at the end and growing; the aided prompt is 179 340 / 178 533)
# position_m: per hand-over of HANDOVERS the fix's error in metres at block 25 000, the same at both offsets to a millimetre
# tx_residual: the largest |transmit-time error minus the four channels' mean| over both chains' launch ends with four VALID
#   observables, samples (0.59 with the first hand-over, 0.72 with the second)
MEASURED = {
    "scenario_error": {4500.0: 0.7659, -4500.0: 1.8978},
    "prompt_ratio": {4500.0: 0.0531, -4500.0: 0.0519},
    "position_m": (15.971, 14.420),
    "tx_residual": 0.7239,
}
PROMPT_RATIO_MAX = 0.25


def bounds():
    return {"scenario_error": {fd: 1.5 * v for fd, v in MEASURED["scenario_error"].items()},
            "position_m": tuple(1.5 * v for v in MEASURED["position_m"]), "tx_residual": 1.5 * MEASURED["tx_residual"]}
