"""What the CPU and GPU tests of the sync loop for many receivers per launch share (include/gpsx.h
gpsx_track_loop_weighted_sync_multi): the case table of the byte-for-byte comparisons -- short strong streams, one per receiver, each
with its own seed and satellites, and hand-overs in all three modes from weighted_sync_cases' state table --, the cases with empty
slots (GPSX_PRN_NONE) and with bad channels, the two-receiver chain scenario, and what was measured on it.  The arithmetic is
weighted_sync_ref's with weighted_aided_ref's clause, applied per receiver: nothing is restated here."""
import os
import sys

import numpy as np

import weighted_aided_ref as A
import weighted_lock_cases as X
import weighted_lock_ref as R
import weighted_loop_cases as S
import weighted_sync_cases as K
import weighted_sync_ref as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRN_NONE = -2147483648         # GPSX_PRN_NONE
POISON = 0xEE                  # the bytes between a receiver's n_blocks and the next receiver's first block
N_BLOCKS = 61                  # no multiple of 20, 5 or 4
EXTRA = 3                      # rx_stride_blocks = n_blocks + EXTRA unless a test says otherwise
PIECES = (1, 19, 41)
TABLE = 32                     # rows of the state table; receiver r's slot j takes row (j + 5 r) % TABLE
ACCEPT_ROW = 17                # weighted_sync_cases.mixed_states: search_n = 39, decides -- and accepts -- at the launch's first block

# ---- launch shapes: (n_rx, ch_per_rx, cpw, channels of waves 0 .. 3) ---------------------------------------------------------------
SHAPES = [(3, 5, 2, (2, 2, 1, 0)),        # an idle wave
          (9, 1, 1, (1, 0, 0, 0)),        # three idle waves
          (2, 17, 5, (5, 5, 5, 2)),       # a ragged last wave
          (2, 64, 16, (16, 16, 16, 16)),  # full waves
          (5, 4, 1, (1, 1, 1, 1))]        # the four-channel receiver
# per shape: (n_coh_search, n_coh_lock), sign and magnitude, spacing
CFGS = [((4, 20), True, 8), ((1, 10), False, 1), ((20, 5), True, 15), ((5, 5), True, 8), ((4, 20), False, 15)]
AIDS = (0.0, float(A.WAID_L1CA))          # the unaided bytes (aid NULL and a factor of 0), and GPSX_WAID_L1CA

DRIVER = r"""
#include "gpsx_track_loop_weighted_plan.hpp"
#include <stdio.h>
int main()
{
  int n_rx, ch_per_rx;
  while (scanf("%d %d", &n_rx, &ch_per_rx) == 2) {
    const gpsx::TrackLoopWeightedPlan p = gpsx::plan_track_loop_weighted_multi(n_rx, ch_per_rx);
    printf("%d %u\n", p.cpw, p.groups);
  }
  return 0;
}
"""
_memo = {}


def plans(shapes):
    """[(cpw, workgroups)] of [(n_rx, ch_per_rx)] from the header itself, compiled with g++ once per process"""
    import subprocess
    import tempfile
    if "exe" not in _memo:
        tmp = _memo["plan_tmp"] = tempfile.TemporaryDirectory(prefix="track_loop_weighted_multi_plan_")
        src, exe = os.path.join(tmp.name, "plan.cpp"), os.path.join(tmp.name, "plan")
        with open(src, "w") as f:
            f.write(DRIVER)
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "stm32f4_sdr_gps_amd", "csrc"), "-o", exe, src])
        _memo["exe"] = exe
    out = subprocess.run([_memo["exe"]], input="".join(f"{a} {b}\n" for a, b in shapes), capture_output=True, text=True, check=True).stdout
    got = [tuple(int(v) for v in line.split()) for line in out.splitlines()]
    assert len(got) == len(shapes)
    return got


def waves(ch_per_rx, cpw):
    """what the kernel's indexing makes of cpw: the slots of waves 0 .. 3"""
    return tuple(max(0, min(cpw, ch_per_rx - w * cpw)) for w in range(4))


# ---- streams and states ------------------------------------------------------------------------------------------------------------
def rx_sats(r):
    """receiver r's three satellites, weighted_sync_cases.STRONG's moved: other PRNs, Dopplers, delays and bit edges per receiver"""
    return [((prn - 1 + 5 * r) % 32 + 1, fd + 137.0 * r * (-1) ** r, (delay + 1111.0 * r) % 16368.0, (edge + 3 * r) % 20, phase + 0.3 * r)
            for prn, fd, delay, edge, phase in K.STRONG]


def rx_blocks(r, n=N_BLOCKS, amp=0.3):
    from stm32f4_sdr_gps_amd import synth
    alt = np.array([1.0, -1.0])
    sats = [synth.Sat(prn, fd, delay + 16368.0 * edge, amp, phase, nav_bits=alt) for prn, fd, delay, edge, phase in rx_sats(r)]
    return synth.make_if(n, sats, noise_amp=1.0, seed=3 + 10 * r, two_bit=True)


def rx_rows(r, ch_per_rx):
    return (np.arange(ch_per_rx) + 5 * r) % TABLE


def rx_states(r, ch_per_rx):
    """receiver r's hand-overs: rows of weighted_sync_cases.mixed_states(TABLE) -- fresh SEARCH, SEARCH in the middle of a window and
    of a round, WAIT, LOCKED in mid-bit -- with the rows that track a satellite of STRONG moved to this receiver's satellite"""
    if "table" not in _memo:
        _memo["table"] = K.mixed_states(TABLE, 77)
    st = _memo["table"][rx_rows(r, ch_per_rx)].copy()
    mine = rx_sats(r)
    for j, row in enumerate(rx_rows(r, ch_per_rx)):
        if row < 3 or row % 4 != 3:
            sat = row % 3
            lp = st["loop"]
            lp["prn"][j] = mine[sat][0]
            lp["code_phase_fine"][j] = (float(lp["code_phase_fine"][j]) - K.STRONG[sat][2] + mine[sat][2]) % 16368.0
            lp["if_freq_offset_hz"][j] = float(lp["if_freq_offset_hz"][j]) - K.STRONG[sat][1] + mine[sat][1]
    return st


def streams_of(blocks_per_rx, stride):
    """[n_rx] arrays [n_blocks][4092] -> uint8 [n_rx][stride][4092], POISON behind every receiver's blocks"""
    n = len(blocks_per_rx[0])
    out = np.full((len(blocks_per_rx), stride, 4092), POISON, np.uint8)
    for r, b in enumerate(blocks_per_rx):
        out[r, :n] = b
    return out


def shape_cfg(i):
    pair, use_mag, spacing = CFGS[i]
    return Y.make_cfg(pair[0], pair[1], S.PULL_IN, S.STEADY, 1, (5, 4), use_mag, spacing)


def shape_inputs(i, n_blocks=N_BLOCKS):
    """shape i -> ([n_rx] blocks, states [n_rx ch_per_rx], cfg)"""
    n_rx, ch_per_rx = SHAPES[i][:2]
    key = ("inputs", i, n_blocks)
    if key not in _memo:
        _memo[key] = ([rx_blocks(r, n_blocks) for r in range(n_rx)], np.concatenate([rx_states(r, ch_per_rx) for r in range(n_rx)]), shape_cfg(i))
    return _memo[key]


# ---- the restatement, per receiver, side by side -----------------------------------------------------------------------------------
def _worker(args):
    """(in a process of its own) some channels of one receiver through the aided sync restatement, launch after launch, and -- lock
    given -- the lock monitor's behind it -> ([records per launch], states, events, [lock records per launch], [epochs per launch])"""
    blocks, st_bytes, cfg, code_per_hz, pieces, lock_cfg = args
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from oracle import pyoracle
    orc = pyoracle.Oracle()
    st = np.frombuffer(bytearray(st_bytes), Y.STATE_DTYPE)
    lock_st = np.zeros(len(st), R.STATE_DTYPE)
    recs, events, locks, epochs, at = [], [], [], [], 0
    for n in pieces:
        ev = []
        recs.append(A.run_sync(orc, blocks[at:at + n], st, cfg, code_per_hz, events=ev))
        events += [(e[0], at + e[1]) + tuple(e[2:]) for e in ev]
        if lock_cfg is not None:
            trace = {}
            lock, bad = R.run(recs[-1], n, lock_st, lock_cfg, None, traces=trace)
            assert not bad
            locks.append(lock)
            epochs.append({c: [(at + t[0],) + tuple(t[1:]) for t in tr] for c, tr in trace.items()})
        at += n
    return recs, st.tobytes(), events, locks, epochs


def on_restatement(jobs, chunk=6):
    """jobs: [(blocks [n][4092], states, cfg, code_per_hz, launch lengths, lock cfg or None)], one per receiver -> per job
    ([records per launch], states after, events [(channel, absolute block, what, ...)], [lock records], [{channel: epochs}]).
    Channels share nothing: a job is cut into tasks of `chunk` channels, run in spawned CPU-only processes, eight at the most."""
    import multiprocessing
    from concurrent.futures import ProcessPoolExecutor
    tasks, owner = [], []
    for j, (blocks, st, cfg, k, pieces, lock_cfg) in enumerate(jobs):
        for c in range(0, len(st), chunk):
            tasks.append((np.ascontiguousarray(blocks), st[c:c + chunk].tobytes(), cfg, float(k), tuple(pieces), lock_cfg))
            owner.append((j, c))
    workers = max(1, min(len(tasks), len(os.sched_getaffinity(0)), 8))
    with ProcessPoolExecutor(workers, mp_context=multiprocessing.get_context("spawn")) as ex:
        done = list(ex.map(_worker, tasks))
    out = []
    for j, job in enumerate(jobs):
        mine = [(c, d) for (jj, c), d in zip(owner, done) if jj == j]
        n_launch = len(job[4])
        recs = [np.concatenate([d[0][i] for _, d in mine], axis=1) for i in range(n_launch)]
        st = np.concatenate([np.frombuffer(d[1], Y.STATE_DTYPE) for _, d in mine])
        events = [(c + e[0],) + tuple(e[1:]) for c, d in mine for e in d[2]]
        locks = [np.concatenate([d[3][i] for _, d in mine]) for i in range(n_launch)] if job[5] is not None else []
        epochs = [{c + ch: tr for c, d in mine for ch, tr in d[4][i].items()} for i in range(n_launch)] if job[5] is not None else []
        out.append((recs, st, events, locks, epochs))
    return out


def shapes_on_restatement():
    """every shape with every factor of AIDS, one launch of N_BLOCKS, computed once per process (all of it side by side)
    -> {(shape, factor): (records [slots][n_ch], states after, events [(channel of the launch, block, what, ...)])}"""
    if "shapes" not in _memo:
        jobs, keys = [], []
        for i, (n_rx, ch_per_rx, _, _) in enumerate(SHAPES):
            blocks, st, cfg = shape_inputs(i)
            distinct = min(ch_per_rx, TABLE)          # (slot j of a receiver repeats slot j - TABLE)
            for k in AIDS:
                for r in range(n_rx):
                    jobs.append((blocks[r], st[r * ch_per_rx:r * ch_per_rx + distinct], cfg, k, (N_BLOCKS,), None))
                    keys.append((i, k, r))
        done = dict(zip(keys, on_restatement(jobs)))
        out = {}
        for i, (n_rx, ch_per_rx, _, _) in enumerate(SHAPES):
            idx = np.arange(ch_per_rx) % min(ch_per_rx, TABLE)
            for k in AIDS:
                per = [done[(i, k, r)] for r in range(n_rx)]
                rec = np.concatenate([p[0][0][:, idx] for p in per], axis=1)
                st = np.concatenate([p[1][idx] for p in per])
                events = [(r * ch_per_rx + e[0],) + tuple(e[1:]) for r, p in enumerate(per) for e in p[2]]     # (of the distinct slots)
                out[(i, k)] = (np.ascontiguousarray(rec), st.copy(), events)
        _memo["shapes"] = out
    return _memo["shapes"]


def patched(oracle, i, k, changes):
    """shape i with factor k and some states changed: {channel: function(state row)} -> (states before, records wanted, states
    wanted).  Only the changed channels go through the restatement again: channels share nothing."""
    n_rx, ch_per_rx = SHAPES[i][:2]
    blocks, st0, cfg = shape_inputs(i)
    st0 = st0.copy()
    rec, st, _ = shapes_on_restatement()[(i, k)]
    rec, st = rec.copy(), st.copy()
    for ch, change in changes.items():
        change(st0[ch:ch + 1])
        one = st0[ch:ch + 1].copy()
        rec[:, ch] = A.run_sync(oracle, blocks[ch // ch_per_rx], one, cfg, k)[:, 0]
        st[ch] = one[0]
    return st0, rec, st


def _set_prn(v):
    def change(s):
        s["loop"]["prn"] = v
    return change


def _set_mode(v):
    def change(s):
        s["mode"] = v
    return change


def _set_phase(v):
    def change(s):
        s["loop"]["code_phase_fine"] = v
    return change


# shape 0, (3, 5): empty slots at the front, in the middle and at the end of a receiver (receivers 0, 1, 2)
HOLES = {0: _set_prn(PRN_NONE), 7: _set_prn(PRN_NONE), 14: _set_prn(PRN_NONE)}
# ... and a bad channel in receiver 1 of 3 (slot 1: channel 6)
BAD_CHANNEL = 6
BAD = {"prn0": _set_prn(0), "mode3": _set_mode(3), "nan": _set_phase(np.nan)}


def grounds(oracle):
    """what the restatement meets over the table's cases: {ground: [(case, channel, ...)]} -- windows in SEARCH and LOCKED, channels
    that sit in WAIT and channels that leave it, an accept, a BIT record, an empty slot, a GPSX_PRN_NONE slot, a bad channel"""
    seen = {k: [] for k in ("search_window", "locked_window", "wait", "left_wait", "accept", "bit", "empty_slot", "none_slot", "bad")}
    for (i, k), (rec, _, events) in shapes_on_restatement().items():
        st0 = shape_inputs(i)[1]
        fl = rec["flags"]
        win = (fl & Y.F_WINDOW) != 0
        for name, hit in (("search_window", win & ((fl & Y.F_LOCKED) == 0)), ("locked_window", win & ((fl & Y.F_LOCKED) != 0)),
                          ("bit", (fl & Y.F_BIT) != 0)):
            seen[name] += [((i, k), int(c)) for c in np.nonzero(hit.any(axis=0))[0][:2]]
        good = np.nonzero(win.any(axis=0))[0]
        seen["empty_slot"] += [((i, k), int(c)) for c in good if (fl[:, c] == 0).any()][:2]
        seen["wait"] += [((i, k), int(c)) for c in np.nonzero(st0["mode"] == Y.WAIT)[0][:2]]
        for e in events:
            if e[2] == "decision" and e[4]:
                seen["accept"].append(((i, k), e[0], e[1]))
            elif e[2] == "locked":
                seen["left_wait"].append(((i, k), e[0], e[1]))
    for k in AIDS:
        st0, rec, st = patched(oracle, 0, k, HOLES)
        for ch in HOLES:
            assert (rec[:, ch]["flags"] == 0).all() and st0["loop"]["prn"][ch] == PRN_NONE
            seen["none_slot"].append(((0, k), ch))
        for name, change in BAD.items():
            st0, rec, st = patched(oracle, 0, k, {BAD_CHANNEL: change})
            assert (rec[:, BAD_CHANNEL]["flags"] == 0).all()
            seen["bad"].append(((0, k), BAD_CHANNEL, name))
    return seen


# ---- the chain: two receivers, three satellites each, five slots ---------------------------------------------------------------------
# weighted_sync_cases' 2 s scenario (amplitude 0.035) on receiver 0; on receiver 1 other PRNs, Dopplers, delays and bit edges.  Of the
# five slots of a receiver three hold its satellites, one a PRN that is present only on the OTHER receiver's stream -- handed over at
# the code phase and Doppler it has there, the most a mixed-up layout could flatter it --, one GPSX_PRN_NONE
CHAIN_MS, CHAIN_LAUNCH, CHAIN_CH = 2000, 500, 5
CHAIN_SEEDS = (1, 2)           # receiver r's noise and data bits
CHAIN_SATS = [K.SATS, [(3, -1705.0, 2222.0, 4, 1.0), (11, 2890.0, 9001.0, 15, 3.0), (25, 640.0, 15003.0, 8, 5.0)]]
# slot -> ("sat", j) | ("cross", j of the other receiver) | ("none",)
CHAIN_SLOTS = [[("sat", 0), ("cross", 1), ("sat", 1), ("none",), ("sat", 2)], [("none",), ("sat", 0), ("sat", 1), ("sat", 2), ("cross", 0)]]


def chain_blocks(r, n_ms=CHAIN_MS):
    """-> (blocks, the +-1 data bits per satellite)"""
    from stm32f4_sdr_gps_amd import synth
    sats, bits = [], []
    for j, (prn, fd, delay, edge, phase) in enumerate(CHAIN_SATS[r]):
        rng = np.random.default_rng(1000 * (j + 1) + CHAIN_SEEDS[r] + 50 * r)
        bits.append(rng.integers(0, 2, n_ms // 20 + 2) * 2.0 - 1.0)
        sats.append(synth.Sat(prn, fd, delay + 16368.0 * edge, K.AMPLITUDE, phase, nav_bits=bits[-1]))
    return synth.make_if(n_ms, sats, noise_amp=1.0, seed=CHAIN_SEEDS[r] + 50 * r, two_bit=True), bits


def chain_states():
    """the ten hand-overs, with weighted_loop_cases.HANDOVER's errors (3 samples, 12.5 Hz)"""
    out = []
    for r in range(2):
        d_phase, d_hz = S.HANDOVER[CHAIN_SEEDS[r]]
        for slot in CHAIN_SLOTS[r]:
            if slot[0] == "none":
                out.append(Y.handover(PRN_NONE, 0.0, 0.0))
            else:
                prn, fd, delay, _, _ = CHAIN_SATS[r if slot[0] == "sat" else 1 - r][slot[1]]
                out.append(Y.handover(prn, delay + d_phase, fd + d_hz))
    return np.concatenate(out)


def chain_launches():
    return [CHAIN_LAUNCH] * (CHAIN_MS // CHAIN_LAUNCH)


def chain_slots(kind):
    return [r * CHAIN_CH + j for r in range(2) for j, s in enumerate(CHAIN_SLOTS[r]) if s[0] == kind]


def chain_on_restatement():
    """the chain on the sync loop's and the lock monitor's restatements, once per process -> ([records per launch][slots][10], sync
    states after, [lock records per launch][10], [{channel: epochs}] per launch)"""
    if "chain" not in _memo:
        st = chain_states()
        jobs = [(chain_blocks(r)[0], st[r * CHAIN_CH:(r + 1) * CHAIN_CH], K.sync_cfg(), 0.0, chain_launches(), X.scenario_cfg(0)) for r in range(2)]
        a, b = on_restatement(jobs, chunk=1)
        n = len(chain_launches())
        _memo["chain"] = ([np.concatenate([a[0][i], b[0][i]], axis=1) for i in range(n)], np.concatenate([a[1], b[1]]),
                          [np.concatenate([a[3][i], b[3][i]]) for i in range(n)],
                          [{**a[4][i], **{CHAIN_CH + c: tr for c, tr in b[4][i].items()}} for i in range(n)])
    return _memo["chain"]


def chain_measure():
    """the code ratios of the epochs (weighted_lock_ref's traces: (end block, locked, K, code_ratio, car_ratio, snr, flags)): the
    smallest of a present satellite's, the largest of a cross-stream PRN's"""
    _, _, _, epochs = chain_on_restatement()
    ratio = lambda chans: [float(e[3]) for per in epochs for c in chans for e in per.get(c, [])]   # noqa: E731
    return dict(code_present_min=round(min(ratio(chain_slots("sat"))), 3), code_cross_max=round(max(ratio(chain_slots("cross"))), 3))


# measured on the restatements (tests/test_weighted_multi_reference.py measures it again and compares): weighted_lock_cases.CODE_MIN
# = 2.3 lies between the two
MEASURED = dict(code_present_min=2.553, code_cross_max=1.442)
