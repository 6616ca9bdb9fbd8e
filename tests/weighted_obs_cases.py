"""What the CPU and GPU tests of the weighted path's observables share (include/gpsx.h gpsx_wobs): fabricated records of the sync
loop with code phases, with the word records the word layer's restatement makes of them, the case table of the byte-for-byte
comparison with initial states taken from the restatements' own run over the stream's earlier blocks, and the two end-to-end
scenarios with their truth."""
import numpy as np

import weighted_nav_cases as W
import weighted_nav_ref as N
import weighted_obs_ref as O
import weighted_sync_cases as K
import weighted_sync_ref as Y

DISTINCT = W.DISTINCT
EDGE_GUARD = 512.0
F32 = np.float32


# ---- fabricated records: weighted_nav_cases' bit streams, with a code phase and a carrier offset in every window record -------------
def phase_at(k, block):
    """stream k's code phase at the window that ends with absolute block `block` (float32, some of them not a phase at all)"""
    kind = k % 8
    if kind == 0:        # drifting up through the seam, 2.5 samples per block: four wraps in the stream's 20 000 blocks
        return F32((16000.0 + 2.5 * block + 11.0 * k) % 16368.0)
    if kind == 1:        # drifting down through it
        return F32((400.0 - 2.9 * block + 7.0 * k) % 16368.0)
    if kind == 2:        # dithering across the seam
        return F32((16367.9, 0.05, 16367.95, 0.1, 0.02)[(block // 3 + k) % 5])
    if kind == 3:        # on either side of mid-block, exactly
        return F32(8183.99) if k % 16 == 3 else F32(8184.0)
    if kind == 4:        # inside the edge guard, drifting through mid-block
        return F32(8000.0 + 0.11 * block + k)
    if kind == 5:        # what is no phase, now and then: skipped records
        bad = (np.nan, -0.5, 16368.0, np.inf, -np.inf, 16368.002)
        return F32(bad[(block // 7) % 6]) if (block + k) % 97 == 0 else F32(1234.5 + (block % 100) * 0.01)
    if kind == 6:        # a drift through the seam on a stream whose edge moves
        return F32((16360.0 + 1.3 * block) % 16368.0)
    return F32(4321.0 + k)


def launch_records(idx, at, n_blocks, span, search_every=0, filler=True):
    """weighted_nav_cases.launch_records (bits and, with `filler`, LOCKED windows that are no bits; their places depend on where the
    launch begins, so launches that are to be compared with their parts go without) with phases and carrier offsets; `search_every`: the filler
    windows of every search_every-th bit lose LOCKED (SEARCH windows inside a chain), on streams 9 and 20"""
    one = W.launch_records(W.specs(), np.arange(DISTINCT), at, n_blocks, span, filler)
    for k in range(DISTINCT):
        for slot in np.nonzero(one["flags"][:, k])[0]:
            block = at + int(one["end_block"][slot, k])
            one["w"]["code_phase_fine"][slot, k] = phase_at(k, block)
            one["w"]["if_freq_offset_hz"][slot, k] = F32(100.0 * k + 0.001 * block)
            if search_every and k in (9, 20) and (block // 20) % search_every == 7 and not int(one["flags"][slot, k]) & Y.F_BIT:
                one["flags"][slot, k] &= ~np.uint32(Y.F_LOCKED)
    return np.ascontiguousarray(one[:, idx])


def tweak_words(words, at):
    """the streams' HOWs all count 101, 102, ..: streams 4 and 20 get them moved to 0, 1, 2, .. (the week ends with the subframe of
    the first), stream 12 gets every second one off by one (a HOW that contradicts the anchor)"""
    for k in (4, 12, 20):
        for slot in range(words.shape[0]):
            r = words[slot, k]
            if int(r["flags"]) & N.F_OK and int(r["index"]) == 2:
                if k == 12:
                    words["aux"][slot, k] = int(r["aux"]) ^ int((at + int(r["end_block"])) // 6000 % 2 == 1)
                else:
                    words["aux"][slot, k] = (int(r["aux"]) + 100800 - 101) % 100800


def launch(st_nav, st_obs, at, n_blocks, span, edge_guard=EDGE_GUARD, search_every=50, filler=True):
    """one launch of the 32 distinct streams on both restatements (states advanced in place) -> (records, words, observables)"""
    rec = launch_records(np.arange(DISTINCT), at, n_blocks, span, search_every, filler)
    words, bad = N.run(rec, n_blocks, st_nav, 3)
    assert not bad
    tweak_words(words, at)
    obs, bad = O.run(rec, n_blocks, words, st_obs, edge_guard)
    assert not bad
    return rec, words, obs


def warm_states(warm, span=20):
    """the 32 distinct channels' word-layer and observable states after blocks 0 .. warm - 1 in launches of at most 4096"""
    nav, obs = np.zeros(DISTINCT, N.STATE_DTYPE), np.zeros(DISTINCT, O.STATE_DTYPE)
    at = 0
    while at < warm:
        n = min(4096, warm - at)
        launch(nav, obs, at, n, span)
        at += n
    return nav, obs


def tiled(n_ch):
    return np.arange(n_ch) % DISTINCT


# (channels, span, blocks of the launch, blocks before it that the initial states have seen)
CASES = [(1, 20, 4096, 0), (3, 20, 4096, 4096), (64, 20, 4096, 1240), (65, 1, 1237, 1240), (257, 4, 600, 5336), (1000, 20, 4096, 6000),
         (64, 20, 1, 1240), (65, 20, 19, 3000), (65, 5, 2047, 10001)]
_cases = {}


def case(i):
    """case i on the restatements, once per process -> (records, words, n_blocks, states before, observables wanted, states wanted)"""
    if i not in _cases:
        n_ch, span, n_blocks, warm = CASES[i]
        nav, st0 = warm_states(warm)
        after = st0.copy()
        rec, words, obs = launch(nav, after, warm, n_blocks, span)
        idx = tiled(n_ch)
        _cases[i] = (np.ascontiguousarray(rec[:, idx]), np.ascontiguousarray(words[:, idx]), n_blocks, st0[idx].copy(), obs[idx].copy(),
                     after[idx].copy())
    return _cases[i]


# ---- end to end: IF samples -> the sync loop -> words -> observables ---------------------------------------------------------------
LAUNCHES = (1000, 1000, 1500)
TOW_MS = 599000                        # the transmit time, ms of the week, of the satellites' bit 0 (subframe 1 with TOW count 100, 250 bits in)
SEAM_DELAYS = (0.4, 16367.6, 8184.2)   # scenario (b): on the seam from either side, and at mid-block


def seam_scenario(seed):
    """weighted_nav_cases.e2e_scenario with the code delays on the seam and at mid-block -> blocks"""
    from stm32f4_sdr_gps_amd import synth
    sats = []
    for j, (prn, fd, _, edge, phase) in enumerate(K.SATS):
        t = synth.lnav_bits(177, W.E2E_FIRST, W.e2e_bit_seed(seed, j))
        sats.append(synth.Sat(prn, fd, SEAM_DELAYS[j] + 16368.0 * edge, K.AMPLITUDE, phase, nav_bits=1.0 - 2.0 * (t ^ W.E2E_FLIP[j])))
    return synth.make_if(W.E2E_MS, sats, noise_amp=1.0, seed=seed, two_bit=True)


def seam_handover(seed):
    """the hand-over errors of weighted_sync_cases.handover_states on the seam scenario's delays, on the circle"""
    import weighted_loop_cases as S
    d_phase, d_hz = S.HANDOVER[seed]
    return np.concatenate([Y.handover(prn, (delay + d_phase) % 16368.0, fd + d_hz) for (prn, fd, _, _, _), delay in zip(K.SATS, SEAM_DELAYS)])


def truth_tx_ms(delay, edge, block):
    """the transmit time of what arrives at sample 0 of `block`: the satellite's bit 0 starts delay + 16368 edge samples into the
    stream"""
    return TOW_MS + block - edge - delay / 16368.0


def chain(run_sync, run_words, run_obs):
    """the three stages over 3500 blocks in LAUNCHES.  run_sync(at, n) -> records, run_words(rec, n) -> words, run_obs(rec, n, words)
    -> observables -> [(first block, records, words, observables)]"""
    out, at = [], 0
    for n in LAUNCHES:
        rec = run_sync(at, n)
        words = run_words(rec, n)
        out.append((at, rec, words, run_obs(rec, n, words)))
        at += n
    return out


_chains = {}


def chain_on_restatements(oracle, which, seed, edge_guard=EDGE_GUARD):
    """scenario "a" (weighted_nav_cases.e2e_scenario) or "b" (the seam) on the three restatements, once per process
    -> ([(first block, records, words, observables)], the observable states, the loop's states)"""
    key = (which, seed, edge_guard)
    if key not in _chains:
        blocks = W.e2e_scenario(seed)[0] if which == "a" else seam_scenario(seed)
        st = K.handover_states(seed) if which == "a" else seam_handover(seed)
        nav, obs_st = np.zeros(3, N.STATE_DTYPE), np.zeros(3, O.STATE_DTYPE)

        def words_of(rec, n):
            words, bad = N.run(rec, n, nav, 3)
            assert not bad
            return words

        def obs_of(rec, n, words):
            obs, bad = O.run(rec, n, words, obs_st, edge_guard)
            assert not bad
            return obs

        out = chain(lambda at, n: Y.run(oracle, blocks[at:at + n], st, K.sync_cfg()), words_of, obs_of)
        _chains[key] = (out, obs_st, st)
    return _chains[key]


def error_samples(o, delay, edge, block=W.E2E_MS):
    """an observable's transmit time minus the truth, in samples (a whole millisecond is 16 368)"""
    return (O.tx_time_ms(o) - truth_tx_ms(delay, edge, block)) * 16368.0
