#!/usr/bin/env python3
"""k_track_epl alone (device-resident block, states and accumulators; HIP events on the engine's stream): what part of
the per-millisecond tracking step is the kernel and what part the PCIe round trip.

  bench_track_kernel.py [channels ...]                the sign-plane step, 50 launches per count (one JSON line)
  bench_track_kernel.py --weighted [K] [channels ...] gpsx_track_epl_weighted_dev (EXTENSION: both bits, K blocks per launch, K = 1
                                                      and the K given) beside gpsx_track_epl_batch_dev: the calls take turns in one
                                                      process, WINDOWS timed windows each, every window some tenths of a second
                                                      long (--window-s S: another length); median, minimum and maximum per launch (one JSON line per row)
  bench_track_kernel.py --weighted-loop [n_coh] [channels ...]
                                                      gpsx_track_loop_weighted_dev (EXTENSION: the closed loop on both bits, K = 200
                                                      blocks per launch, n_coh = 1, 20 and the n_coh given) beside what it is made of
                                                      and measured against: gpsx_track_epl_weighted_dev at K = 20 (the same correlators,
                                                      open loop), and the sign plane's pair gpsx_track_loop_dev (K = 200) /
                                                      gpsx_track_epl_batch_dev -- time per channel-millisecond and the two
                                                      closed-over-open ratios, and gpsx_track_loop_weighted_aided_dev (carrier
                                                      aiding, GPSX_WAID_L1CA) beside every unaided row with that row timed a
                                                      second time for the spread; then the host-driven alternative: one K = 200,
                                                      n_coh = 10 launch against twenty gpsx_track_epl_weighted calls of K = 10 with the
                                                      records copied back and the states rewritten by the host (wall clock)
  bench_track_kernel.py --weighted-sync [channels ...]
                                                      gpsx_track_loop_weighted_sync_dev (EXTENSION: the loop with a bit synchroniser per
                                                      channel, K = 200) in three states -- (a) every channel LOCKED at n_coh_lock = 20
                                                      with edges spread over 0 .. 19, (b) the same with all edges equal, (c) every channel
                                                      in SEARCH at n_coh_search = 4 (ratio 1024 / 1: noise never leaves it) -- beside
                                                      gpsx_track_loop_weighted_dev at n_coh = 1, 4, 20 in the same process, the calls
                                                      taking turns, and gpsx_track_loop_weighted_sync_aided_dev (carrier aiding) beside
                                                      every leg with the leg timed a second time; then the wall clock of 2000 ms in host launches of 200 with the
                                                      records copied back
  bench_track_kernel.py --weighted-nav [channels ...]
                                                      gpsx_wnav_words_dev (EXTENSION: LNAV frame sync and parity-checked words from the
                                                      sync loop's records) on the records of a 4000-block launch at span 20 (200 slots,
                                                      one bit per slot, every channel SYNCED on a parity-correct stream) beside (1) a
                                                      device-to-device hipMemcpyAsync of the same record array -- the bar: the kernel
                                                      takes no longer -- and (2) the gpsx_track_loop_weighted_sync_dev launch that
                                                      writes such records (n_coh_lock = 20, every channel LOCKED), the calls taking
                                                      turns in one process
  bench_track_kernel.py --weighted-obs [channels ...]
                                                      gpsx_wobs_dev (EXTENSION: every channel's transmit time at the launch's end, from
                                                      the records and the words) on the same fabricated record arrays, with code
                                                      phases in them (one channel in four drifts through the seam) and with the word
                                                      records gpsx_wnav_words_dev made of each, beside (1) a device-to-device
                                                      hipMemcpyAsync of the record array -- the bar: the kernel takes no longer -- and
                                                      (2) gpsx_wnav_words_dev, which reads the same lines, the calls taking turns in one
                                                      process
  bench_track_kernel.py --weighted-eph [channels ...]
                                                      gpsx_weph_dev (EXTENSION: every channel's broadcast ephemeris from the words) on
                                                      the word records of 4000-block launches -- every channel mid-stream on a repeating
                                                      parity-correct 1-2-3-4-5 frame, 32 distinct offsets, fifteen word arrays (two
                                                      frames) used in turn -- beside (a) a device-to-device hipMemcpyAsync of half the
                                                      768 bytes per channel it touches (a copy reads and writes what it is given) and
                                                      (b) gpsx_wnav_words_dev on the records of a 4000-block launch -- the bar: the stage
                                                      at the chain's end takes no longer than the one before it -- the calls taking
                                                      turns in one process; then what a host does without the stage: d_words copied
                                                      back, gpsx_wnav_subframe_image and gps_nav_data_decode_subframe per channel
  bench_track_kernel.py --weighted-lock [channels ...]
                                                      gpsx_wlock_dev (EXTENSION: every channel's code-lock, carrier-lock and C/N0
                                                      indicators from the records) on the records of 4000-block launches at span 20 (200
                                                      slots, every channel LOCKED; three channels in four carry a satellite's sums, the
                                                      fourth noise), three record arrays used in turn, LOCKED epochs of 10 windows,
                                                      beside (1) a device-to-device hipMemcpyAsync of the record array -- the bar: the
                                                      kernel takes no longer -- and (2) gpsx_wobs_dev on the same lines (no bar: it
                                                      reads 16 bytes of a record where this reads 32), the calls taking turns in one
                                                      process
  bench_track_kernel.py --weighted-multi [--single-only] [--parent-rows FILE] [N_RXxCH_PER_RX ...]
                                                      gpsx_track_loop_weighted_sync_multi_dev (EXTENSION: many receivers per launch, one
                                                      IF stream each; k_track_wsync_multi) at (n_rx, ch_per_rx) = (16384, 4), (8192, 8),
                                                      (5461, 12), (1024, 64), 64 blocks, every channel LOCKED at n_coh_lock = 20, beside
                                                      gpsx_track_loop_weighted_sync_aided_dev on ONE stream with the same n_ch, the
                                                      calls taking turns: time, ns per channel-ms, the ratio, and the IF bytes the
                                                      launch must read from HBM.  --single-only: the single-stream rows alone, for a
                                                      library without the new call (the parent commit's, in a neighbouring process);
                                                      --parent-rows: such rows, against which the ratio is formed too
  bench_track_kernel.py --weighted-fix [N_RXxCH_PER_RX ...]
                                                      gpsx_wfix_dev (EXTENSION: every receiver's position fix; k_wfix) at (n_rx,
                                                      ch_per_rx) = (16384, 4), (8192, 8), (4096, 12), (1024, 64), every slot usable (16
                                                      distinct skies of tests/weighted_fix_cases.py, tiled), cold start, beside a
                                                      device-to-device hipMemcpyAsync of the bytes the kernel reads (288 per slot); then,
                                                      for the 4-slot shape, the wall time of the host path on records already in host
                                                      memory: gpsx_wobs_pseudoranges_rx, gpsx_weph_to_eph per slot and pntpos per
                                                      receiver, called through ctypes (the interpreter's share is in it)
  bench_track_kernel.py --weighted-fde [N_RXxCH_PER_RX ...]
                                                      gpsx_wfde_dev (EXTENSION: the fixes with millisecond repair and fault exclusion;
                                                      k_wfde) at --weighted-fix's four shapes, 2 m of noise: on clean records beside
                                                      gpsx_wfix_dev on the same arrays (the ratio of one round to k_wfix), and on records
                                                      with one 300 m fault per receiver (the cost of a second round), the calls taking
                                                      turns in one process; the lines also go to profiles/r21_weighted_fde_bench.jsonl
  bench_track_kernel.py --weighted-vel [N_RXxCH_PER_RX ...]
                                                      gpsx_wvel_dev (EXTENSION: every receiver's velocity and clock drift; k_wvel) at
                                                      --weighted-fix's four shapes, receivers at 36 m/s, on the fix records that
                                                      gpsx_wfix_dev left on the device, beside gpsx_wfix_dev on the same arrays, the
                                                      calls taking turns in one process; the lines also go to
                                                      profiles/r22_weighted_vel_bench.jsonl
  bench_track_kernel.py --weighted-kf [N_RXxCH_PER_RX ...]
                                                      gpsx_wkf_dev (EXTENSION: every receiver's navigation filter; k_wkf) at
                                                      --weighted-fix's four shapes: one update per receiver from states initialised one
                                                      launch earlier (a device-to-device copy puts them back before every timed launch;
                                                      it is timed alone and subtracted), beside gpsx_wfix_dev (warm start) and
                                                      gpsx_wvel_dev on the same records, the calls taking turns in one process; the
                                                      lines also go to profiles/r24_weighted_kf_bench.jsonl
  bench_track_kernel.py --weighted-acq [N_RXxN_PRNxN_DOPPxCH_PER_RX ...]
                                                      gpsx_wacq_dev (EXTENSION: acquisition decisions and slot hand-over; k_wacq) at
                                                      (receivers, PRNs, bins, slots) = (256, 32, 201, 12), (4096, 32, 41, 8), (16384,
                                                      32, 21, 4): eight of the PRNs detected per receiver, half the slots free, beside
                                                      (1) a device-to-device hipMemcpyAsync of the peak records it reads and (2)
                                                      gpsx_memcpy_d2h of those records, the first step of the host path it replaces,
                                                      the calls taking turns in one process (a hand-over changes the states, so a
                                                      device-to-device copy puts them back before every timed launch; it is timed alone
                                                      and subtracted); the lines also go to profiles/r27_weighted_acq_bench.jsonl
  bench_track_kernel.py --weighted-bank [N_RXxN_PRNxCH_PER_RX ...]
                                                      gpsx_wbank_dev (EXTENSION: the ephemeris bank; k_wbank) at 256, 4096 and 16384
                                                      receivers x 32 PRNs with 8 and 12 slots: a full bank, three slots of four refresh
                                                      their entry and the fourth takes the bank's record, beside (1) a device-to-device
                                                      hipMemcpyAsync of the ephemeris records it reads and (2) gpsx_wkf_dev's update at
                                                      the same receivers, the calls taking turns in one process; then gpsx_wpred_dev
                                                      (EXTENSION: prediction and hot hand-over; k_wpred) on the same filter states and
                                                      bank with half the slots emptied, predicting only and handing over, beside a
                                                      copy of what it reads and gpsx_wkf_dev; the lines also go to
                                                      profiles/r28_weighted_pred_bench.jsonl
  bench_track_kernel.py --weighted-tow [N_RXxN_PRNxCH_PER_RX ...]
                                                      gpsx_wtow_dev (EXTENSION: time-of-week aiding; k_wtow) at the same shapes behind
                                                      gpsx_wpred_dev's records: every slot anchored (a device-to-device copy puts the
                                                      observable states back before every timed launch; it is timed alone and
                                                      subtracted), with and without d_obs, and the steady state in which every slot
                                                      agrees, beside (1) a device-to-device copy of the bytes it reads and (2)
                                                      gpsx_wpred_dev predicting only; the lines also go to
                                                      profiles/r29_weighted_tow_bench.jsonl
  bench_track_kernel.py --weighted-alm [N_RXxCH_PER_RX ...]
                                                      gpsx_walm_dev (EXTENSION: almanac, ionosphere and UTC; k_walm) on gpsx_weph's and
                                                      gpsx_wbank's shapes (53248 x 4; 256, 4096 and 16384 receivers x 8 and 12 slots),
                                                      4000-block launches in which every slot receives words 5 .. 10 of a subframe: of a
                                                      subframe 2 (no page), of an almanac page in slot 0 (a page per receiver) and in
                                                      every slot (a page per slot), with and without d_alm, beside (1) gpsx_weph_dev on
                                                      the same words and (2) a device-to-device copy of the bytes touched (a copy puts
                                                      the states back before every timed launch; it is timed alone and subtracted); the
                                                      lines also go to profiles/r30_weighted_alm_bench.jsonl
  bench_track_kernel.py --weighted-snap [N_RXxN_PRN ...]   k_wsnap (snapshot fixes from grid records, a bank and a prior) at 21 bins, beside a
                                                      device-to-device copy of what it reads, k_wfix on as many rows, and the host path
                                                      (records copied back, the CPU restatement): profiles/r32_weighted_snap_bench.jsonl
  bench_track_kernel.py --weighted-win [N_RXxN_COHxN_SEGxW ...]
                                                      gpsx_acq_window_weighted_dev (EXTENSION: the weighted grid in a window around
                                                      each prediction; k_acq_win) on 12 PRNs per receiver, D = 2, every record
                                                      searched on all five bins (256 and 4096 receivers; 10 x 8 and 20 x 4 blocks; W =
                                                      128 and 1024), beside gpsx_acq_grid_weighted_hyb_dev on the same receivers, PRNs,
                                                      blocks and five bins -- the cheapest way the grids answer the same question; the
                                                      calls take turns; the lines also go to profiles/r31_weighted_win_bench.jsonl"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


WINDOWS = 7          # timed windows per call and row (the calls alternate)
WINDOW_S = 0.3       # each window's length


def _bench_states(n):
    from stm32f4_sdr_gps_amd import capi
    st = np.zeros(n, capi.TRK_DTYPE)
    st["prn"] = (np.arange(n) % 32) + 1
    st["code_phase_fine"] = (61 * np.arange(n) % 16368).astype(np.float32)
    st["if_freq_offset_hz"] = (-5000 + 39 * (np.arange(n) % 256)).astype(np.float32)
    return st


def weighted(k_blocks, counts):
    from stm32f4_sdr_gps_amd import capi, synth
    eng = capi.Engine(0)
    e0, e1 = eng.event(), eng.event()
    blk = synth.default_four_sv(1, seed=7)[0]
    d_if = eng.malloc(2048)
    eng.h2d(d_if, np.concatenate([blk, np.zeros(2, np.uint8)]))
    blocks2 = np.random.default_rng(7).integers(0, 256, (k_blocks, 4092), dtype=np.uint8)
    d_if2 = eng.malloc(blocks2.nbytes)
    eng.h2d(d_if2, blocks2)
    cfg = np.array([1, 8], np.int32)
    for n in counts:
        st = _bench_states(n)
        d_st, d_iq, d_iqw = eng.malloc(st.nbytes), eng.malloc(n * 12), eng.malloc(k_blocks * n * 24)
        eng.h2d(d_st, st)
        calls = {"baseline": (1, lambda: eng.lib.gpsx_track_epl_batch_dev(eng.h, C.c_void_p(d_if), C.c_void_p(d_st), n, C.c_void_p(d_iq)))}
        for k in sorted({1, k_blocks}):
            calls[f"weighted_k{k}"] = (k, lambda k=k: eng.lib.gpsx_track_epl_weighted_dev(eng.h, cfg.ctypes.data, C.c_void_p(d_if2), k,
                                                                                        C.c_void_p(d_st), n, C.c_void_p(d_iqw)))

        def window(fn, reps):
            eng.record(e0)
            for _ in range(reps):
                fn()
            eng.record(e1)
            eng.synchronize()
            return eng.elapsed_ms(e0, e1) / reps * 1e3

        reps = {}
        for name, (_, fn) in calls.items():   # warm-up, then as many launches as fill a window
            eng._chk(fn(), name)
            window(fn, 5)
            reps[name] = max(10, int(WINDOW_S * 1e6 / window(fn, 20)))
        us = {name: [] for name in calls}
        for _ in range(WINDOWS):
            for name, (_, fn) in calls.items():
                us[name].append(window(fn, reps[name]))
        base = float(np.median(us["baseline"]))
        for name, (k, _) in calls.items():
            med = float(np.median(us[name]))
            print(json.dumps({"call": name, "channels": n, "blocks": k, "windows": WINDOWS, "launches_per_window": reps[name],
                              "us_median": round(med, 3), "us_min": round(min(us[name]), 3), "us_max": round(max(us[name]), 3),
                              "us_per_block": round(med / k, 3), "ns_per_channel_ms": round(med / k / n * 1e3, 4),
                              "per_block_over_baseline": round(med / k / base, 3)}), flush=True)
        for p in (d_st, d_iq, d_iqw):
            eng.free(p)


def _timed_rows(eng, calls, extra, per_channel_ms=True):
    """calls: {name: (blocks per launch, fn)} taking turns, WINDOWS windows each -> {name: median us per launch}, one JSON line each
    (per_channel_ms False: a leg whose calls are not per block and channel -- no `blocks`, no `ns_per_channel_ms` in its lines)"""
    e0, e1 = eng.event(), eng.event()

    def window(fn, reps):
        eng.record(e0)
        for _ in range(reps):
            fn()
        eng.record(e1)
        eng.synchronize()
        return eng.elapsed_ms(e0, e1) / reps * 1e3

    reps = {}
    for name, (_, fn) in calls.items():   # warm-up, then as many launches as fill a window
        eng._chk(fn(), name)
        window(fn, 3)
        reps[name] = max(3, int(WINDOW_S * 1e6 / window(fn, 5)))
    us = {name: [] for name in calls}
    for _ in range(WINDOWS):
        for name, (_, fn) in calls.items():
            us[name].append(window(fn, reps[name]))
    med = {}
    for name, (k, _) in calls.items():
        med[name] = float(np.median(us[name]))
        row = {"call": name, **extra, "blocks": k, "windows": WINDOWS, "launches_per_window": reps[name],
               "us_median": round(med[name], 3), "us_min": round(min(us[name]), 3), "us_max": round(max(us[name]), 3),
               "ns_per_channel_ms": round(med[name] / k / extra["channels"] * 1e3, 4)}
        if not per_channel_ms:
            del row["blocks"], row["ns_per_channel_ms"]
        print(json.dumps(row), flush=True)
    return med


def weighted_loop(n_coh_arg, counts, k_loop=200, k_open=20):
    import time
    from stm32f4_sdr_gps_amd import capi, synth
    eng = capi.Engine(0)
    blk = synth.default_four_sv(k_loop, seed=7)
    d_if = eng.malloc(blk.nbytes + 2)
    eng.h2d(d_if, np.concatenate([blk.reshape(-1), np.zeros(2, np.uint8)]))
    blocks2 = np.random.default_rng(7).integers(0, 256, (k_loop, 4092), dtype=np.uint8)
    d_if2 = eng.malloc(blocks2.nbytes)
    eng.h2d(d_if2, blocks2)
    ocfg = np.array([1, 8], np.int32)
    for n in counts:
        trk = _bench_states(n)
        loop = np.zeros(n, capi.LOOP_DTYPE)
        wst = np.zeros(n, capi.WLOOP_STATE_DTYPE)
        for f in ("prn", "code_phase_fine", "if_freq_offset_hz"):
            loop[f] = trk[f]
            wst[f] = trk[f]
        loop["found_freq_offset_hz"] = loop["if_freq_offset_hz"].astype(np.int16)
        loop["rng"] = np.arange(n) + 1
        d_trk, d_iq, d_iqw = eng.malloc(trk.nbytes), eng.malloc(n * 12), eng.malloc(k_open * n * 24)
        d_loop, d_fl, d_wst, d_rec = eng.malloc(loop.nbytes), eng.malloc(n * k_loop), eng.malloc(wst.nbytes), eng.malloc(k_loop * n * 36)
        eng.h2d(d_trk, trk)
        eng.h2d(d_loop, loop)
        eng.h2d(d_wst, wst)
        tick = [0]

        def sign_loop():
            tick[0] += k_loop
            return eng.lib.gpsx_track_loop_dev(eng.h, C.c_void_p(d_if), k_loop, C.c_void_p(d_loop), n, tick[0], C.c_void_p(d_fl), None)

        calls = {"sign_epl_k1": (1, lambda: eng.lib.gpsx_track_epl_batch_dev(eng.h, C.c_void_p(d_if), C.c_void_p(d_trk), n, C.c_void_p(d_iq))),
                 f"sign_loop_k{k_loop}": (k_loop, sign_loop),
                 f"weighted_epl_k{k_open}": (k_open, lambda: eng.lib.gpsx_track_epl_weighted_dev(eng.h, ocfg.ctypes.data, C.c_void_p(d_if2), k_open,
                                                                                                C.c_void_p(d_trk), n, C.c_void_p(d_iqw)))}
        cfgs = {}
        for n_coh in sorted({1, 20, n_coh_arg}):
            cfgs[n_coh] = capi.wloop_cfg(n_coh, True, 8, (1.0, 300.0), (4.0, 3000.0), 0.1)
            calls[f"weighted_loop_k{k_loop}_ncoh{n_coh}"] = (k_loop, lambda c=cfgs[n_coh]: eng.lib.gpsx_track_loop_weighted_dev(
                eng.h, c.ctypes.data, C.c_void_p(d_if2), k_loop, C.c_void_p(d_wst), n, C.c_void_p(d_rec)))
        # the carrier-aided call beside each unaided row (k_track_waid_loop, GPSX_WAID_L1CA, states of its own), and the unaided row
        # a second time: what two rows of ONE kernel differ by is the spread the aided row is read against
        d_wst_aid = eng.malloc(wst.nbytes)
        eng.h2d(d_wst_aid, wst)
        aid = capi.waid()
        for n_coh in cfgs:
            calls[f"weighted_loop_aided_k{k_loop}_ncoh{n_coh}"] = (k_loop, lambda c=cfgs[n_coh]: eng.lib.gpsx_track_loop_weighted_aided_dev(
                eng.h, c.ctypes.data, aid.ctypes.data, C.c_void_p(d_if2), k_loop, C.c_void_p(d_wst_aid), n, C.c_void_p(d_rec)))
            calls[f"weighted_loop_k{k_loop}_ncoh{n_coh}_again"] = calls[f"weighted_loop_k{k_loop}_ncoh{n_coh}"]
        med = _timed_rows(eng, calls, {"channels": n})
        for n_coh in cfgs:
            base = med[f"weighted_loop_k{k_loop}_ncoh{n_coh}"]
            print(json.dumps({"ratio": "k_track_waid_loop over k_track_wloop", "channels": n, "n_coh": n_coh,
                              "aided": round(med[f"weighted_loop_aided_k{k_loop}_ncoh{n_coh}"] / base, 4),
                              "unaided_again": round(med[f"weighted_loop_k{k_loop}_ncoh{n_coh}_again"] / base, 4)}), flush=True)
        eng.free(d_wst_aid)
        per = {name: med[name] / calls[name][0] for name in calls}
        sign_ratio = per[f"sign_loop_k{k_loop}"] / per["sign_epl_k1"]
        for n_coh in cfgs:
            ratio = per[f"weighted_loop_k{k_loop}_ncoh{n_coh}"] / per[f"weighted_epl_k{k_open}"]
            print(json.dumps({"ratio": "closed over open, per channel-ms", "channels": n, "n_coh": n_coh, "weighted": round(ratio, 4),
                              "sign_plane": round(sign_ratio, 4), "bound_sign_plane_x_1.10": round(1.1 * sign_ratio, 4),
                              "within_bound": bool(ratio <= 1.1 * sign_ratio)}), flush=True)
        for p in (d_trk, d_iq, d_iqw, d_loop, d_fl, d_rec):
            eng.free(p)

        # the host-driven alternative (wall clock, blocks in host memory either way)
        if n <= 65536:
            cfg10 = dict(n_coh=10, dll=(1.0, 300.0), pll=(4.0, 3000.0), fll=0.1)
            walls = {"device_loop_1x200": [], "host_loop_20x10": []}
            for _ in range(WINDOWS):
                t0 = time.perf_counter()
                eng.track_loop_weighted(blocks2, d_wst, n, **cfg10)
                walls["device_loop_1x200"].append(time.perf_counter() - t0)
                st = trk.copy()
                t0 = time.perf_counter()
                for w in range(k_loop // 10):
                    iq = eng.track_epl_weighted(blocks2[10 * w:10 * w + 10], st)
                    iq.sum(axis=0, dtype=np.int64)       # (the window sums a host loop would start from; its arithmetic is not counted)
                walls["host_loop_20x10"].append(time.perf_counter() - t0)
            print(json.dumps({"host_driven_alternative": True, "channels": n, "blocks": k_loop, "n_coh": 10,
                              **{k: round(float(np.median(v)) * 1e3, 3) for k, v in walls.items()}, "unit": "ms wall clock, median of %d" % WINDOWS}), flush=True)
        eng.free(d_wst)


def weighted_sync(counts, k_loop=200):
    import time
    from stm32f4_sdr_gps_amd import capi
    eng = capi.Engine(0)
    blocks2 = np.random.default_rng(7).integers(0, 256, (k_loop, 4092), dtype=np.uint8)
    d_if2 = eng.malloc(blocks2.nbytes)
    eng.h2d(d_if2, blocks2)
    gains = dict(dll=(1.0, 300.0), pll=(4.0, 3000.0), fll=0.1)
    for n in counts:
        trk = _bench_states(n)
        wst = np.zeros(n, capi.WLOOP_STATE_DTYPE)
        for f in ("prn", "code_phase_fine", "if_freq_offset_hz"):
            wst[f] = trk[f]
        legs = {}
        for leg in ("a_locked_spread", "b_locked_equal", "c_search"):
            st = np.zeros(n, capi.WSYNC_STATE_DTYPE)
            st["loop"] = wst
            if leg != "c_search":
                st["mode"] = capi.WSYNC_LOCKED
                st["edge"] = np.arange(n) % 20 if leg == "a_locked_spread" else 0
            legs[leg] = st
        d_wst, d_rec = eng.malloc(wst.nbytes), eng.malloc(k_loop * n * 36)
        eng.h2d(d_wst, wst)
        d_sync = {leg: eng.malloc(st.nbytes) for leg, st in legs.items()}
        for leg, st in legs.items():
            eng.h2d(d_sync[leg], st)
        d_srec = eng.malloc(capi.wsync_slots(k_loop, 4, 4) * n * 48)
        calls, keep = {}, []
        for n_coh in (1, 4, 20):
            c = capi.wloop_cfg(n_coh, True, 8, gains["dll"], gains["pll"], gains["fll"])
            keep.append(c)
            calls[f"weighted_loop_k{k_loop}_ncoh{n_coh}"] = (k_loop, lambda c=c: eng.lib.gpsx_track_loop_weighted_dev(
                eng.h, c.ctypes.data, C.c_void_p(d_if2), k_loop, C.c_void_p(d_wst), n, C.c_void_p(d_rec)))
        for leg in legs:
            pair = (4, 4) if leg == "c_search" else (20, 20)
            c = capi.wsync_cfg(pair[0], pair[1], gains, gains, 20, (1024, 1))
            keep.append(c)
            calls[f"weighted_sync_k{k_loop}_{leg}"] = (k_loop, lambda c=c, d=d_sync[leg]: eng.lib.gpsx_track_loop_weighted_sync_dev(
                eng.h, c.ctypes.data, C.c_void_p(d_if2), k_loop, C.c_void_p(d), n, C.c_void_p(d_srec)))
        # the carrier-aided call beside each leg (k_track_waid_sync, GPSX_WAID_L1CA, states of its own), and the unaided leg a second
        # time: the spread the aided row is read against
        d_aid = {leg: eng.malloc(st.nbytes) for leg, st in legs.items()}
        aid = capi.waid()
        for i, leg in enumerate(legs):
            eng.h2d(d_aid[leg], legs[leg])
            calls[f"weighted_sync_aided_k{k_loop}_{leg}"] = (k_loop, lambda c=keep[3 + i], d=d_aid[leg]: eng.lib.gpsx_track_loop_weighted_sync_aided_dev(
                eng.h, c.ctypes.data, aid.ctypes.data, C.c_void_p(d_if2), k_loop, C.c_void_p(d), n, C.c_void_p(d_srec)))
            calls[f"weighted_sync_k{k_loop}_{leg}_again"] = calls[f"weighted_sync_k{k_loop}_{leg}"]
        med = _timed_rows(eng, calls, {"channels": n})
        for leg in legs:
            base = med[f"weighted_sync_k{k_loop}_{leg}"]
            print(json.dumps({"ratio": "k_track_waid_sync over k_track_wsync", "channels": n, "leg": leg,
                              "aided": round(med[f"weighted_sync_aided_k{k_loop}_{leg}"] / base, 4),
                              "unaided_again": round(med[f"weighted_sync_k{k_loop}_{leg}_again"] / base, 4)}), flush=True)
        for p in d_aid.values():
            eng.free(p)
        for leg, against in (("a_locked_spread", 1), ("b_locked_equal", 20), ("c_search", 4)):
            ratio = med[f"weighted_sync_k{k_loop}_{leg}"] / med[f"weighted_loop_k{k_loop}_ncoh{against}"]
            print(json.dumps({"ratio": "k_track_wsync over k_track_wloop", "channels": n, "leg": leg, "against_n_coh": against,
                              "value": round(ratio, 4), **({"bound": 1.10, "within_bound": bool(ratio <= 1.10)} if leg != "c_search" else {})}), flush=True)
        after = legs["c_search"].copy()
        eng.d2h(after, d_sync["c_search"])
        print(json.dumps({"leg_c_check": "channels still in SEARCH", "channels": n, "in_search": int((after["mode"] == 0).sum()),
                          "sync_rounds_max": int(after["sync_rounds"].max())}), flush=True)
        for p in [d_wst, d_rec, d_srec] + [d_sync[leg] for leg in ("a_locked_spread", "b_locked_equal")]:
            eng.free(p)
        if n <= 65536:      # the scenario's shape: 2000 ms in ten host launches of 200, records copied back (wall clock)
            eng.h2d(d_sync["c_search"], legs["c_search"])
            c = capi.wsync_cfg(4, 20, gains, gains, 20, (5, 4))
            eng.track_loop_weighted_sync(blocks2, d_sync["c_search"], n, c)      # (warm-up: the arena grows once)
            eng.h2d(d_sync["c_search"], legs["c_search"])
            t0 = time.perf_counter()
            for _ in range(10):
                eng.track_loop_weighted_sync(blocks2, d_sync["c_search"], n, c)
            wall = time.perf_counter() - t0
            print(json.dumps({"scenario_wall_clock": True, "channels": n, "blocks": 10 * k_loop, "launches": 10, "n_coh_search": 4, "n_coh_lock": 20,
                              "seconds": round(wall, 4), "record_bytes_per_launch": capi.wsync_slots(k_loop, 4, 20) * n * 48}), flush=True)
        eng.free(d_sync["c_search"])


MULTI_SHAPES = [(16384, 4), (8192, 8), (5461, 12), (1024, 64)]


def weighted_multi(shapes, n_blocks=64, single_only=False, parent_rows=None):
    """gpsx_track_loop_weighted_sync_multi_dev (k_track_wsync_multi: a workgroup per receiver, one IF stream each) per shape
    (n_rx, ch_per_rx), every channel LOCKED at n_coh_lock = 20 with edges spread, GPSX_WAID_L1CA, beside
    gpsx_track_loop_weighted_sync_aided_dev (k_track_waid_sync) on ONE stream with the same n_ch and n_blocks, the calls taking
    turns.  single_only: the single-stream rows alone (a library without the new call: the parent commit's, in a neighbouring
    process); parent_rows: a file of such rows, against which the ratios are formed as well"""
    from stm32f4_sdr_gps_amd import capi
    eng = capi.Engine(0)
    gains = dict(dll=(1.0, 300.0), pll=(4.0, 3000.0), fll=0.1)
    cfg, aid = capi.wsync_cfg(20, 20, gains, gains, 20, (1024, 1)), capi.waid()
    parent = {}
    if parent_rows:
        for line in open(parent_rows):
            row = json.loads(line)
            if row.get("call", "").startswith("weighted_sync_aided_single"):
                parent[row["channels"]] = row["us_median"]
    chunk_rx = 256
    chunk = np.random.default_rng(7).integers(0, 256, (chunk_rx, n_blocks, 4092), dtype=np.uint8)      # (receivers beyond 256 repeat these bytes)
    for n_rx, ch in shapes:
        n = n_rx * ch
        trk = _bench_states(n)
        st = np.zeros(n, capi.WSYNC_STATE_DTYPE)
        for f in ("prn", "code_phase_fine", "if_freq_offset_hz"):
            st["loop"][f] = trk[f]
        st["mode"], st["edge"] = capi.WSYNC_LOCKED, np.arange(n) % 20
        d_single, d_rec = eng.malloc(st.nbytes), eng.malloc(capi.wsync_slots(n_blocks, 20, 20) * n * 48)
        eng.h2d(d_single, st)
        d_one = eng.malloc(chunk[0].nbytes)
        eng.h2d(d_one, chunk[0])
        calls = {f"weighted_sync_aided_single_k{n_blocks}": (n_blocks, lambda: eng.lib.gpsx_track_loop_weighted_sync_aided_dev(
            eng.h, cfg.ctypes.data, aid.ctypes.data, C.c_void_p(d_one), n_blocks, C.c_void_p(d_single), n, C.c_void_p(d_rec)))}
        ptrs = [d_single, d_rec, d_one]
        if not single_only:
            rx = capi.wmulti(n_rx, ch, n_blocks)
            d_multi, d_if = eng.malloc(st.nbytes), eng.malloc(n_rx * chunk[0].nbytes)
            ptrs += [d_multi, d_if]
            eng.h2d(d_multi, st)
            for r in range(0, n_rx, chunk_rx):
                eng.h2d(d_if + r * chunk[0].nbytes, chunk[:min(chunk_rx, n_rx - r)])
            calls[f"weighted_sync_multi_k{n_blocks}"] = (n_blocks, lambda: eng.lib.gpsx_track_loop_weighted_sync_multi_dev(
                eng.h, cfg.ctypes.data, aid.ctypes.data, rx.ctypes.data, C.c_void_p(d_if), n_blocks, C.c_void_p(d_multi), C.c_void_p(d_rec)))
            calls[f"weighted_sync_aided_single_k{n_blocks}_again"] = calls[f"weighted_sync_aided_single_k{n_blocks}"]
        med = _timed_rows(eng, calls, {"channels": n, "n_rx": n_rx, "ch_per_rx": ch})
        if not single_only:
            single, multi = med[f"weighted_sync_aided_single_k{n_blocks}"], med[f"weighted_sync_multi_k{n_blocks}"]
            print(json.dumps({"ratio": "k_track_wsync_multi over k_track_waid_sync on one stream", "n_rx": n_rx, "ch_per_rx": ch, "channels": n,
                              "blocks": n_blocks, "multi_us": round(multi, 3), "ns_per_channel_ms": round(multi / n_blocks / n * 1e3, 4),
                              "over_single": round(multi / single, 4),
                              "single_again": round(med[f"weighted_sync_aided_single_k{n_blocks}_again"] / single, 4),
                              **({"over_parent_single": round(multi / parent[n], 4), "parent_single_us": parent[n]} if n in parent else {}),
                              "if_bytes_from_hbm": n_rx * n_blocks * 4092, "gb_per_s_of_if": round(n_rx * n_blocks * 4092 / multi / 1e3, 2)}), flush=True)
        for p in ptrs:
            eng.free(p)


def weighted_nav(counts, n_blocks=4000, span=20):
    from stm32f4_sdr_gps_amd import capi, synth
    hip = C.CDLL("libamdhip64.so")
    hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    capi.load_library()
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    eng = capi.Engine(0, stream=stream.value)      # (the copy below goes onto the stream the engine's events are recorded on)
    n_slots = n_blocks // span
    blocks2 = np.random.default_rng(7).integers(0, 256, (n_blocks, 4092), dtype=np.uint8)
    d_if2 = eng.malloc(blocks2.nbytes)
    eng.h2d(d_if2, blocks2)
    gains = dict(dll=(1.0, 300.0), pll=(4.0, 3000.0), fll=0.1)
    # 32 distinct channels on ONE parity-correct subframe repeated for ever (it ends in D29 = D30 = 0, as every subframe does), each
    # at its own offset into it and half of them inverted: three consecutive launches of 200 bits are two subframes, so the record
    # arrays A, B, C used in turn keep every channel SYNCED, with words completing in different slots from lane to lane
    sub = np.array(synth.lnav_subframe(3, 4711, np.random.Generator(np.random.PCG64(5))), np.int64)
    distinct = 32
    bits = np.stack([np.tile(sub, 4)[(37 * j) % 300:(37 * j) % 300 + 600] ^ (j & 1) for j in range(distinct)], axis=1)      # [600][32]
    cfg = np.zeros(1, capi.WNAV_CFG_DTYPE)
    cfg["max_bad_words"] = 3
    for n in counts:
        idx = np.arange(n) % distinct
        rec_bytes = n_slots * n * 48
        d_recs = []
        for leg in range(3):
            small = np.zeros((n_slots, distinct), capi.WSYNC_REC_DTYPE)
            small["end_block"] = (np.arange(n_slots) * span + span - 1)[:, None]
            small["flags"] = capi.WSYNC_FLAG_WINDOW | capi.WSYNC_FLAG_LOCKED | capi.WSYNC_FLAG_BIT
            small["bit_ip"] = (1 - 2 * bits[leg * n_slots:(leg + 1) * n_slots]) * 20000
            d = eng.malloc(rec_bytes)
            eng.h2d(d, np.ascontiguousarray(small[:, idx]))
            d_recs.append(d)
        d_copy, d_srec = eng.malloc(rec_bytes), eng.malloc(rec_bytes)
        nav = np.zeros(n, capi.WNAV_STATE_DTYPE)
        d_nav, d_words = eng.malloc(nav.nbytes), eng.malloc(capi.wnav_word_slots(n_blocks) * n * 16)
        eng.h2d(d_nav, nav)
        trk = _bench_states(n)
        st = np.zeros(n, capi.WSYNC_STATE_DTYPE)
        for f in ("prn", "code_phase_fine", "if_freq_offset_hz"):
            st["loop"][f] = trk[f]
        st["mode"] = capi.WSYNC_LOCKED
        d_sync = eng.malloc(st.nbytes)
        eng.h2d(d_sync, st)
        c_sync = capi.wsync_cfg(20, 20, gains, gains, 20, (1024, 1))
        turn = [0]

        def words():
            d = d_recs[turn[0] % 3]
            turn[0] += 1
            return eng.lib.gpsx_wnav_words_dev(eng.h, cfg.ctypes.data, C.c_void_p(d), n_slots, n_blocks, C.c_void_p(d_nav), n, C.c_void_p(d_words))

        for _ in range(6):      # 1200 bits: every channel has met TLM + HOW with 62 fresh bits by now
            eng._chk(words(), "gpsx_wnav_words_dev")
        eng.synchronize()
        eng.d2h(nav, d_nav)
        synced_before = int((nav["mode"] == capi.WNAV_SYNCED).sum())
        calls = {"d2d_copy_of_d_rec": (n_blocks, lambda: hip.hipMemcpyAsync(d_copy, d_recs[0], rec_bytes, 3, stream)),
                 "wnav_words": (n_blocks, words),
                 "weighted_sync_locked_ncoh20": (n_blocks, lambda: eng.lib.gpsx_track_loop_weighted_sync_dev(
                     eng.h, c_sync.ctypes.data, C.c_void_p(d_if2), n_blocks, C.c_void_p(d_sync), n, C.c_void_p(d_srec)))}
        med = _timed_rows(eng, calls, {"channels": n, "slots": n_slots, "rec_bytes": rec_bytes})
        eng.d2h(nav, d_nav)
        print(json.dumps({"wnav_check": "channels SYNCED before / after the timed launches", "channels": n, "before": synced_before,
                          "after": int((nav["mode"] == capi.WNAV_SYNCED).sum()), "drops": int(nav["n_drop"].sum()),
                          "launches": turn[0], "subframes_min": int(nav["n_subframes"].min())}), flush=True)
        r = med["wnav_words"] / med["d2d_copy_of_d_rec"]
        print(json.dumps({"ratio": "k_wnav_words over a device-to-device copy of d_rec", "channels": n, "value": round(r, 4), "bound": 1.0,
                          "within_bound": bool(r <= 1.0), "read_GBps": round(rec_bytes / med["wnav_words"] / 1e3, 1),
                          "copy_GBps_read_plus_write": round(2 * rec_bytes / med["d2d_copy_of_d_rec"] / 1e3, 1)}), flush=True)
        print(json.dumps({"ratio": "k_wnav_words over the k_track_wsync launch that writes its records", "channels": n,
                          "value": round(med["wnav_words"] / med["weighted_sync_locked_ncoh20"], 5)}), flush=True)
        for p in d_recs + [d_copy, d_srec, d_nav, d_words, d_sync]:
            eng.free(p)


def weighted_obs(counts, n_blocks=4000, span=20):
    from stm32f4_sdr_gps_amd import capi, synth
    hip = C.CDLL("libamdhip64.so")
    hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    capi.load_library()
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    eng = capi.Engine(0, stream=stream.value)      # (the copy below goes onto the stream the engine's events are recorded on)
    n_slots = n_blocks // span
    # weighted_nav's streams: 32 distinct channels on one parity-correct subframe repeated for ever, three record arrays used in turn
    sub = np.array(synth.lnav_subframe(3, 4711, np.random.Generator(np.random.PCG64(5))), np.int64)
    distinct = 32
    bits = np.stack([np.tile(sub, 4)[(37 * j) % 300:(37 * j) % 300 + 600] ^ (j & 1) for j in range(distinct)], axis=1)      # [600][32]
    # code phases: three channels in four stand still somewhere on the circle, the fourth drifts through the seam (0.004 samples per
    # block: 5 kHz of Doppler) -- up, and back down where the three arrays start over, so that its edge block moves both ways
    j = np.arange(distinct)
    still = (511.0 * j + 100.0) % 16368.0
    nav_cfg = np.zeros(1, capi.WNAV_CFG_DTYPE)
    nav_cfg["max_bad_words"] = 3
    cfg = np.zeros(1, capi.WOBS_CFG_DTYPE)
    cfg["edge_guard"] = 512.0
    for n in counts:
        idx = np.arange(n) % distinct
        rec_bytes = n_slots * n * 48
        word_slots = capi.wnav_word_slots(n_blocks)
        d_recs, d_words = [], []
        for leg in range(3):
            small = np.zeros((n_slots, distinct), capi.WSYNC_REC_DTYPE)
            ends = np.arange(n_slots) * span + span - 1
            small["end_block"] = ends[:, None]
            small["flags"] = capi.WSYNC_FLAG_WINDOW | capi.WSYNC_FLAG_LOCKED | capi.WSYNC_FLAG_BIT
            small["bit_ip"] = (1 - 2 * bits[leg * n_slots:(leg + 1) * n_slots]) * 20000
            drift = (16368.0 - 24.0 + 0.004 * (leg * n_blocks + ends)) % 16368.0
            small["w"]["code_phase_fine"] = np.where(j[None, :] % 4 == 3, drift[:, None], still[None, :]).astype(np.float32)
            small["w"]["if_freq_offset_hz"] = (-5000.0 + 300.0 * j)[None, :].astype(np.float32)
            d = eng.malloc(rec_bytes)
            eng.h2d(d, np.ascontiguousarray(small[:, idx]))
            d_recs.append(d)
            d_words.append(eng.malloc(word_slots * n * 16))
        d_copy, d_words_timed = eng.malloc(rec_bytes), eng.malloc(word_slots * n * 16)
        nav, obs_st = np.zeros(n, capi.WNAV_STATE_DTYPE), np.zeros(n, capi.WOBS_STATE_DTYPE)
        d_nav, d_obs_st, d_obs = eng.malloc(nav.nbytes), eng.malloc(obs_st.nbytes), eng.malloc(n * 32)
        eng.h2d(d_nav, nav)
        eng.h2d(d_obs_st, obs_st)
        turn = {"words": 0, "obs": 0}

        def words(out=None):
            leg = turn["words"] % 3
            turn["words"] += 1
            return eng.lib.gpsx_wnav_words_dev(eng.h, nav_cfg.ctypes.data, C.c_void_p(d_recs[leg]), n_slots, n_blocks, C.c_void_p(d_nav), n,
                                               C.c_void_p(d_words_timed if out is None else out[leg]))

        def observables():
            leg = turn["obs"] % 3
            turn["obs"] += 1
            return eng.lib.gpsx_wobs_dev(eng.h, cfg.ctypes.data, C.c_void_p(d_recs[leg]), n_slots, n_blocks, C.c_void_p(d_words[leg]),
                                         C.c_void_p(d_obs_st), n, C.c_void_p(d_obs))

        for _ in range(6):      # 1200 bits: every channel has met TLM + HOW with 62 fresh bits by now ...
            eng._chk(words(), "gpsx_wnav_words_dev")
        for _ in range(3):      # ... and these are the words of each array from then on (the stream repeats after the three)
            eng._chk(words(d_words), "gpsx_wnav_words_dev")
        eng.synchronize()
        calls = {"d2d_copy_of_d_rec": (n_blocks, lambda: hip.hipMemcpyAsync(d_copy, d_recs[0], rec_bytes, 3, stream)),
                 "wobs": (n_blocks, observables),
                 "wnav_words": (n_blocks, words)}
        med = _timed_rows(eng, calls, {"channels": n, "slots": n_slots, "rec_bytes": rec_bytes})
        obs = np.zeros(n, capi.WOBS_DTYPE)
        eng.d2h(obs, d_obs)
        eng.d2h(obs_st, d_obs_st)
        print(json.dumps({"wobs_check": "observables after the timed launches", "channels": n, "launches": turn["obs"],
                          "valid": int((obs["flags"] & capi.WOBS_FLAG_VALID != 0).sum()), "breaks": int(obs_st["n_break"].sum()),
                          "wraps_min_of_the_drifting": int(obs_st["n_wraps"][idx % 4 == 3].min()), "wraps_of_the_others": int(obs_st["n_wraps"][idx % 4 != 3].sum()),
                          "blocks_seen": int(obs_st["blocks_seen"].min())}), flush=True)
        r = med["wobs"] / med["d2d_copy_of_d_rec"]
        print(json.dumps({"ratio": "k_wobs over a device-to-device copy of d_rec", "channels": n, "value": round(r, 4), "bound": 1.0,
                          "within_bound": bool(r <= 1.0), "read_GBps": round(rec_bytes / med["wobs"] / 1e3, 1),
                          "copy_GBps_read_plus_write": round(2 * rec_bytes / med["d2d_copy_of_d_rec"] / 1e3, 1)}), flush=True)
        print(json.dumps({"ratio": "k_wobs over k_wnav_words on the same records (no bar)", "channels": n,
                          "value": round(med["wobs"] / med["wnav_words"], 4)}), flush=True)
        for p in d_recs + d_words + [d_copy, d_words_timed, d_nav, d_obs_st, d_obs]:
            eng.free(p)


def weighted_eph(counts, n_blocks=4000, span=20):
    import time
    from stm32f4_sdr_gps_amd import capi, synth
    hip = C.CDLL("libamdhip64.so")
    hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    lib = capi.load_library()
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    eng = capi.Engine(0, stream=stream.value)      # (the copy below goes onto the stream the engine's events are recorded on)
    distinct, legs, frame = 32, 15, 30000
    n_slots, word_slots = n_blocks // span, capi.wnav_word_slots(n_blocks)
    # one frame of five parity-correct subframes; subframes 1, 2, 3 of one issue of data (IODC's low byte, IODE twice)
    rng = np.random.Generator(np.random.PCG64(5))
    frame_words = []      # 50 x (word as the word layer writes it, index, subframe ID, TOW count)
    for sub_id in range(1, 6):
        payload = [[int(b) for b in rng.integers(0, 2, 24)] for _ in range(8)]
        for word, first in ((5, sub_id == 1), (0, sub_id == 2), (7, sub_id == 3)):
            if first:
                payload[word][:8] = [0, 1, 0, 0, 1, 1, 0, 1]
        bits = synth.lnav_subframe(sub_id, 1000 + sub_id, rng, payload)
        d30 = 0
        for w in range(10):
            t = bits[30 * w:30 * w + 30]
            data = int("".join(str(b ^ d30) for b in t[:24]), 2)
            frame_words.append((data << 6 | int("".join(str(b) for b in t[24:]), 2), w + 1, sub_id, 1000 + sub_id if w == 1 else 0))
            d30 = t[29]
    offsets = [(937 * j + 11) % frame for j in range(distinct)]      # word 1 of subframe 1 of channel j ends at block offsets[j] + 599 (mod the frame)
    small = np.zeros((legs, word_slots, distinct), capi.WNAV_WORD_DTYPE)
    small["end_block"] = -1
    for j, off in enumerate(offsets):
        fill = [0] * legs
        for k in range(-50, 2 * 50 + 50):      # words of the frame before, of the two frames of the fifteen launches, of the one after
            end = off + 600 * (k + 1) - 1
            leg = end // n_blocks
            if 0 <= end and leg < legs:
                word, index, sub_id, aux = frame_words[k % 50]
                small[leg, fill[leg], j] = (end - leg * n_blocks, word, index, capi.WNAV_FLAG_WORD | capi.WNAV_FLAG_OK, sub_id if index >= 2 else 0, 0, aux)
                fill[leg] += 1
    # gpsx_wnav_words_dev's input as in --weighted-nav: one parity-correct subframe repeated for ever, three record arrays used in turn
    sub = np.array(synth.lnav_subframe(3, 4711, np.random.Generator(np.random.PCG64(5))), np.int64)
    nav_bits = np.stack([np.tile(sub, 4)[(37 * j) % 300:(37 * j) % 300 + 600] ^ (j & 1) for j in range(distinct)], axis=1)
    nav_cfg = np.zeros(1, capi.WNAV_CFG_DTYPE)
    nav_cfg["max_bad_words"] = 3
    cfg = np.zeros(1, capi.WEPH_CFG_DTYPE)
    for n in counts:
        idx = np.arange(n) % distinct
        words_bytes, rec_bytes, touched = word_slots * n * 16, n_slots * n * 48, n * (word_slots * 16 + 2 * 192 + 256)
        d_words = []
        for leg in range(legs):
            d = eng.malloc(words_bytes)
            eng.h2d(d, np.ascontiguousarray(small[leg][:, idx]))
            d_words.append(d)
        d_recs = []
        for leg in range(3):
            rec = np.zeros((n_slots, distinct), capi.WSYNC_REC_DTYPE)
            rec["end_block"] = (np.arange(n_slots) * span + span - 1)[:, None]
            rec["flags"] = capi.WSYNC_FLAG_WINDOW | capi.WSYNC_FLAG_LOCKED | capi.WSYNC_FLAG_BIT
            rec["bit_ip"] = (1 - 2 * nav_bits[leg * n_slots:(leg + 1) * n_slots]) * 20000
            d = eng.malloc(rec_bytes)
            eng.h2d(d, np.ascontiguousarray(rec[:, idx]))
            d_recs.append(d)
        nav, st = np.zeros(n, capi.WNAV_STATE_DTYPE), np.zeros(n, capi.WEPH_STATE_DTYPE)
        d_nav, d_st, d_eph, d_nav_words = eng.malloc(nav.nbytes), eng.malloc(st.nbytes), eng.malloc(n * 256), eng.malloc(words_bytes)
        d_src, d_dst = eng.malloc(touched // 2), eng.malloc(touched // 2)
        eng.h2d(d_nav, nav)
        eng.h2d(d_st, st)
        turn = {"words": 0, "eph": 0}

        def words():
            leg = turn["words"] % 3
            turn["words"] += 1
            return eng.lib.gpsx_wnav_words_dev(eng.h, nav_cfg.ctypes.data, C.c_void_p(d_recs[leg]), n_slots, n_blocks, C.c_void_p(d_nav), n,
                                               C.c_void_p(d_nav_words))

        def ephemerides():
            leg = turn["eph"] % legs
            turn["eph"] += 1
            return eng.lib.gpsx_weph_dev(eng.h, cfg.ctypes.data, C.c_void_p(d_words[leg]), n_blocks, C.c_void_p(d_st), n, C.c_void_p(d_eph))

        for _ in range(6):          # every channel of the word layer SYNCED ...
            eng._chk(words(), "gpsx_wnav_words_dev")
        for _ in range(legs):       # ... and every channel here holding its set, mid-stream
            eng._chk(ephemerides(), "gpsx_weph_dev")
        eng.synchronize()
        calls = {"d2d_copy_of_half_the_bytes_touched": (n_blocks, lambda: hip.hipMemcpyAsync(d_dst, d_src, touched // 2, 3, stream)),
                 "weph": (n_blocks, ephemerides),
                 "wnav_words": (n_blocks, words)}
        med = _timed_rows(eng, calls, {"channels": n, "word_slots": word_slots, "bytes_touched": touched})
        eph = np.zeros(n, capi.WEPH_DTYPE)
        eng.d2h(eph, d_eph)
        eng.d2h(st, d_st)
        print(json.dumps({"weph_check": "records after the timed launches", "channels": n, "launches": turn["eph"],
                          "valid": int((eph["flags"] & capi.WEPH_FLAG_VALID != 0).sum()), "n_sets_max": int(st["n_sets"].max()),
                          "subframes_min": int(st["n_subframes"].min()), "subframes_max": int(st["n_subframes"].max()),
                          "blocks_seen": int(st["blocks_seen"].min())}), flush=True)
        print(json.dumps({"ratio": "k_weph over k_wnav_words on the 4000-block launch that feeds it", "channels": n,
                          "value": round(med["weph"] / med["wnav_words"], 4), "bound": 1.0, "within_bound": bool(med["weph"] <= med["wnav_words"])}), flush=True)
        print(json.dumps({"ratio": "k_weph over a device-to-device copy of the bytes it touches (no bar)", "channels": n,
                          "value": round(med["weph"] / med["d2d_copy_of_half_the_bytes_touched"], 4),
                          "touched_GBps": round(touched / med["weph"] / 1e3, 1),
                          "copy_GBps_read_plus_write": round(touched / med["d2d_copy_of_half_the_bytes_touched"] / 1e3, 1)}), flush=True)
        # the alternative without the stage: d_words back to the host (wall clock, three copies), then per channel and complete subframe
        # gpsx_wnav_subframe_image + gps_nav_data_decode_subframe -- timed through ctypes on up to 4096 subframes (the figure includes
        # the two foreign calls' overhead) and scaled to the n_blocks / 6000 subframes a channel completes per launch
        host_words = np.zeros((word_slots, n), capi.WNAV_WORD_DTYPE)
        copies = []
        for _ in range(3):
            t0 = time.perf_counter()
            eng.d2h(host_words, d_words[0])
            copies.append(time.perf_counter() - t0)
        lib.gps_nav_data_decode_subframe.argtypes = [C.c_void_p]
        ten = np.zeros(10, capi.WNAV_WORD_DTYPE)
        for w in range(10):
            ten[w] = (600 * w + 599, frame_words[w][0], w + 1, capi.WNAV_FLAG_WORD | capi.WNAV_FLAG_OK, 1, 0, frame_words[w][3])
        ch = np.zeros(1688, np.uint8)      # a gps_ch_t
        image = ch[212 + 71:212 + 71 + 38]
        m = min(n, 4096)
        t0 = time.perf_counter()
        for _ in range(m):
            lib.gpsx_wnav_subframe_image(ten.ctypes.data, image.ctypes.data)
            lib.gps_nav_data_decode_subframe(ch.ctypes.data)
        per_subframe = (time.perf_counter() - t0) / m
        decode_s = per_subframe * n * n_blocks / 6000
        print(json.dumps({"alternative": "d_words copied back + host decode per channel and subframe", "channels": n,
                          "d_words_MB": round(words_bytes / 1e6, 1), "copy_back_ms_median": round(float(np.median(copies)) * 1e3, 3),
                          "host_decode_us_per_subframe_through_ctypes": round(per_subframe * 1e6, 3), "host_decode_ms_per_launch": round(decode_s * 1e3, 3),
                          "total_ms_per_launch": round((float(np.median(copies)) + decode_s) * 1e3, 3), "weph_ms_per_launch": round(med["weph"] / 1e3, 4)}),
              flush=True)
        for p in d_words + d_recs + [d_nav, d_st, d_eph, d_nav_words, d_src, d_dst]:
            eng.free(p)


def weighted_lock(counts, n_blocks=4000, span=20):
    from stm32f4_sdr_gps_amd import capi
    hip = C.CDLL("libamdhip64.so")
    hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    capi.load_library()
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    eng = capi.Engine(0, stream=stream.value)      # (the copy below goes onto the stream the engine's events are recorded on)
    n_slots, distinct = n_blocks // span, 32
    rng = np.random.default_rng(17)
    j = np.arange(distinct)
    there = (j % 4 != 3)[None, :]      # three channels in four: a prompt of 17 000 with data bits on noise of 1000, half of it on the taps
    cfg = capi.wlock_cfg(25, 10, 2.3, 0.75, 6.0, 2, 2)
    obs_cfg = np.zeros(1, capi.WOBS_CFG_DTYPE)
    obs_cfg["edge_guard"] = 512.0
    for n in counts:
        idx = np.arange(n) % distinct
        rec_bytes = n_slots * n * 48
        word_slots = capi.wnav_word_slots(n_blocks)
        d_recs = []
        for leg in range(3):
            small = np.zeros((n_slots, distinct), capi.WSYNC_REC_DTYPE)
            small["end_block"] = (np.arange(n_slots) * span + span - 1)[:, None]
            small["flags"] = capi.WSYNC_FLAG_WINDOW | capi.WSYNC_FLAG_LOCKED | capi.WSYNC_FLAG_BIT
            noise = rng.normal(0.0, 1000.0, (n_slots, distinct, 6))
            bit = rng.integers(0, 2, (n_slots, distinct)) * 2 - 1
            noise[:, :, 2] += np.where(there, 17000.0 * bit, 0.0)
            noise[:, :, 0] += np.where(there, 8500.0 * bit, 0.0)
            noise[:, :, 4] += np.where(there, 8500.0 * bit, 0.0)
            small["w"]["iq"] = np.rint(noise).astype(np.int32)
            small["w"]["code_phase_fine"] = ((511.0 * j + 100.0) % 16368.0)[None, :].astype(np.float32)
            small["bit_ip"] = small["w"]["iq"][:, :, 2]
            d = eng.malloc(rec_bytes)
            eng.h2d(d, np.ascontiguousarray(small[:, idx]))
            d_recs.append(d)
        words = np.zeros((word_slots, n), capi.WNAV_WORD_DTYPE)      # no words: k_wobs' time is its pass over d_rec
        words["end_block"] = -1
        st, obs_st = np.zeros(n, capi.WLOCK_STATE_DTYPE), np.zeros(n, capi.WOBS_STATE_DTYPE)
        d_copy, d_words, d_st, d_obs_st = eng.malloc(rec_bytes), eng.malloc(words.nbytes), eng.malloc(st.nbytes), eng.malloc(obs_st.nbytes)
        d_lock, d_obs = eng.malloc(n * 64), eng.malloc(n * 32)
        eng.h2d(d_words, words)
        eng.h2d(d_st, st)
        eng.h2d(d_obs_st, obs_st)
        turn = {"lock": 0, "obs": 0}

        def lock():
            leg = turn["lock"] % 3
            turn["lock"] += 1
            return eng.lib.gpsx_wlock_dev(eng.h, cfg.ctypes.data, C.c_void_p(d_recs[leg]), n_slots, n_blocks, C.c_void_p(d_st), None, n, C.c_void_p(d_lock))

        def observables():
            leg = turn["obs"] % 3
            turn["obs"] += 1
            return eng.lib.gpsx_wobs_dev(eng.h, obs_cfg.ctypes.data, C.c_void_p(d_recs[leg]), n_slots, n_blocks, C.c_void_p(d_words), C.c_void_p(d_obs_st), n,
                                         C.c_void_p(d_obs))

        for _ in range(3):
            eng._chk(lock(), "gpsx_wlock_dev")
            eng._chk(observables(), "gpsx_wobs_dev")
        eng.synchronize()
        calls = {"d2d_copy_of_d_rec": (n_blocks, lambda: hip.hipMemcpyAsync(d_copy, d_recs[0], rec_bytes, 3, stream)),
                 "wlock": (n_blocks, lock),
                 "wobs": (n_blocks, observables)}
        med = _timed_rows(eng, calls, {"channels": n, "slots": n_slots, "rec_bytes": rec_bytes})
        rec = np.zeros(n, capi.WLOCK_DTYPE)
        eng.d2h(rec, d_lock)
        eng.d2h(st, d_st)
        both = capi.WLOCK_FLAG_CODE | capi.WLOCK_FLAG_CARRIER
        print(json.dumps({"wlock_check": "records after the timed launches", "channels": n, "launches": turn["lock"],
                          "code_and_carrier": int((rec["flags"] & both == both).sum()), "neither": int((rec["flags"] & both == 0).sum()),
                          "epochs_per_launch": int(rec["n_epochs"].min()), "losses": int(st["n_lost_code"].sum() + st["n_lost_carrier"].sum()),
                          "cn0_dbhz_median_of_the_locked": round(float(np.median(capi.wlock_cn0_dbhz(rec, 20)[rec["flags"] & both == both])), 2),
                          "blocks_seen": int(st["blocks_seen"].min())}), flush=True)
        r = med["wlock"] / med["d2d_copy_of_d_rec"]
        print(json.dumps({"ratio": "k_wlock over a device-to-device copy of d_rec", "channels": n, "value": round(r, 4), "bound": 1.0,
                          "within_bound": bool(r <= 1.0), "read_GBps_of_the_32_bytes_per_record": round(rec_bytes * 2 / 3 / med["wlock"] / 1e3, 1),
                          "read_GBps_of_whole_lines": round(rec_bytes / med["wlock"] / 1e3, 1),
                          "copy_GBps_read_plus_write": round(2 * rec_bytes / med["d2d_copy_of_d_rec"] / 1e3, 1)}), flush=True)
        print(json.dumps({"ratio": "k_wlock over k_wobs on the same records (no bar)", "channels": n,
                          "value": round(med["wlock"] / med["wobs"], 4)}), flush=True)
        for p in d_recs + [d_copy, d_words, d_st, d_obs_st, d_lock, d_obs]:
            eng.free(p)


FIX_SHAPES = [(16384, 4), (8192, 8), (4096, 12), (1024, 64)]


def weighted_fix(shapes):
    import time
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import weighted_fix_cases as W
    from pvt_types import UNIX2GPS, Eph, GTime, Nav, Obsd, Sol
    from stm32f4_sdr_gps_amd import capi
    hip = C.CDLL("libamdhip64.so")
    hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    lib = capi.load_library()
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    eng = capi.Engine(0, stream=stream.value)
    names = sorted(W.SITES)
    for n_rx, ch in shapes:
        pool = [W.receiver(names[k % len(names)], ch, 3 * k) for k in range(16)]
        obs, eph = W.pack([pool[r % 16] for r in range(n_rx)], ch)
        cfg = capi.wfix_cfg(W.OFFSET_MS, ch)
        read_bytes = obs.nbytes + eph.nbytes
        d_obs, d_eph, d_fix, d_src, d_dst = eng.malloc(obs.nbytes), eng.malloc(eph.nbytes), eng.malloc(n_rx * 128), eng.malloc(read_bytes), eng.malloc(read_bytes)
        eng.h2d(d_obs, obs)
        eng.h2d(d_eph, eph)
        calls = {"d2d_copy_of_the_bytes_read": (1, lambda: hip.hipMemcpyAsync(d_dst, d_src, read_bytes, 3, stream)),
                 "wfix": (1, lambda: eng.lib.gpsx_wfix_dev(eng.h, cfg.ctypes.data, C.c_void_p(d_obs), C.c_void_p(d_eph), None, None, n_rx, C.c_void_p(d_fix), None))}
        med = _timed_rows(eng, calls, {"channels": n_rx * ch, "n_rx": n_rx, "ch_per_rx": ch, "read_bytes": read_bytes})
        fix = np.zeros(n_rx, capi.WFIX_DTYPE)
        eng.d2h(fix, d_fix)
        print(json.dumps({"wfix_check": "records after the timed launches", "n_rx": n_rx, "ch_per_rx": ch, "fixed": int((fix["flags"] == 1).sum()),
                          "n_iter_max": int(fix["n_iter"].max()), "n_used_min": int(fix["n_used"].min())}), flush=True)
        print(json.dumps({"ratio": "k_wfix over a device-to-device copy of the bytes it reads", "n_rx": n_rx, "ch_per_rx": ch,
                          "value": round(med["wfix"] / med["d2d_copy_of_the_bytes_read"], 2), "ns_per_receiver": round(med["wfix"] / n_rx * 1e3, 2),
                          "read_GBps": round(read_bytes / med["wfix"] / 1e3, 2)}), flush=True)
        if ch == 4:      # the host path on the same records
            lib.pntpos.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
            lib.gpsx_weph_to_eph.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
            t0 = time.perf_counter()
            pr, rx_tow = capi.wobs_pseudoranges_rx(obs, n_rx, ch, W.OFFSET_MS)[:2]
            ephs = np.zeros(n_rx * ch, capi.EPH_DTYPE)
            n_fix = 0
            for r in range(n_rx):
                nav, od, sol = Nav(), (Obsd * ch)(), Sol()
                nav.n = ch
                whole = int(rx_tow[r])
                for k in range(ch):
                    at = r * ch + k
                    lib.gpsx_weph_to_eph(eph[at:at + 1].ctypes.data, k + 1, ephs[at:at + 1].ctypes.data)
                    nav.eph[k] = C.cast(ephs[at:at + 1].ctypes.data, C.POINTER(Eph))
                    od[k].time = GTime(UNIX2GPS + 604800 * int(ephs["week"][at]) + whole, float(rx_tow[r]) - whole)
                    od[k].sat, od[k].rcv, od[k].code[0], od[k].P[0] = k + 1, 1, 1, float(pr[at])
                n_fix += lib.pntpos(od, ch, C.byref(nav), C.byref(sol)) == 1
            host_us = (time.perf_counter() - t0) * 1e6
            print(json.dumps({"call": "host_path_pseudoranges_rx_weph_to_eph_pntpos", "n_rx": n_rx, "ch_per_rx": ch, "fixed": int(n_fix),
                              "wall_us": round(host_us, 1), "us_per_receiver": round(host_us / n_rx, 2),
                              "ratio_to_wfix": round(host_us / med["wfix"], 1), "note": "through ctypes from Python, one process, one thread"}), flush=True)
        for p in (d_obs, d_eph, d_fix, d_src, d_dst):
            eng.free(p)


FDE_OUT = os.path.join(ROOT, "profiles", "r21_weighted_fde_bench.jsonl")


class _Tee:
    """stdout, and every line of it into a file as well"""

    def __init__(self, path):
        self.out, self.file = sys.stdout, open(path, "w")

    def write(self, text):
        self.out.write(text)
        self.file.write(text)

    def flush(self):
        self.out.flush()
        self.file.flush()


def weighted_fde(shapes, out=FDE_OUT):
    """k_wfde at k_wfix's shapes: on clean records (one round; beside k_wfix on the same arrays, the calls taking turns) and on records
    with one 300 m fault per receiver (two rounds); the lines go to stdout and to `out`"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import weighted_fde_cases as X
    import weighted_fix_cases as W
    from stm32f4_sdr_gps_amd import capi
    tee = sys.stdout = _Tee(out)
    eng = capi.Engine(0)
    names = sorted(W.SITES)
    try:
        for n_rx, ch in shapes:
            rng = np.random.default_rng(ch)
            clean, faulty = [], []
            for k in range(16):      # --weighted-fix's sixteen skies, every slot usable, 2 m of noise; the fault at slot k
                site, noise = names[k % len(names)], rng.normal(0.0, 2.0, ch)
                clean.append(X.receiver(site, ch, 3 * k, noise))
                noise[k % ch] += 300.0
                faulty.append(X.receiver(site, ch, 3 * k, noise))
            cfg, fix_cfg = capi.wfde_cfg(W.OFFSET_MS, ch), capi.wfix_cfg(W.OFFSET_MS, ch)
            d_fix, d_fde = eng.malloc(n_rx * 128), eng.malloc(n_rx * 64)
            dev = {}
            for name, pool in (("clean", clean), ("one_fault", faulty)):
                obs, eph = W.pack([pool[r % 16] for r in range(n_rx)], ch)
                dev[name] = (eng.malloc(obs.nbytes), eng.malloc(eph.nbytes))
                eng.h2d(dev[name][0], obs)
                eng.h2d(dev[name][1], eph)

            def fde(which):
                return eng.lib.gpsx_wfde_dev(eng.h, cfg.ctypes.data, C.c_void_p(dev[which][0]), C.c_void_p(dev[which][1]), None, None, n_rx,
                                             C.c_void_p(d_fix), C.c_void_p(d_fde), None)

            calls = {"wfix_clean": (1, lambda: eng.lib.gpsx_wfix_dev(eng.h, fix_cfg.ctypes.data, C.c_void_p(dev["clean"][0]), C.c_void_p(dev["clean"][1]), None,
                                                                     None, n_rx, C.c_void_p(d_fix), None)),
                     "wfde_clean": (1, lambda: fde("clean")),
                     "wfde_one_fault": (1, lambda: fde("one_fault"))}
            med = _timed_rows(eng, calls, {"channels": n_rx * ch, "n_rx": n_rx, "ch_per_rx": ch})
            rec = np.zeros(n_rx, capi.WFDE_DTYPE)
            for which in ("clean", "one_fault"):
                eng._chk(fde(which), "gpsx_wfde_dev")
                eng.synchronize()
                eng.d2h(rec, d_fde)
                print(json.dumps({"wfde_check": which, "n_rx": n_rx, "ch_per_rx": ch, "passed": int((rec["flags"] & 1 != 0).sum()),
                                  "excluded_one": int((rec["n_excluded"] == 1).sum()), "rounds_min": int(rec["n_rounds"].min()),
                                  "rounds_max": int(rec["n_rounds"].max())}), flush=True)
            print(json.dumps({"ratio": "k_wfde over k_wfix on clean records (one round each)", "n_rx": n_rx, "ch_per_rx": ch,
                              "value": round(med["wfde_clean"] / med["wfix_clean"], 3), "ns_per_receiver": round(med["wfde_clean"] / n_rx * 1e3, 2)}), flush=True)
            print(json.dumps({"ratio": "k_wfde with one fault per receiver (two rounds) over k_wfde on clean records", "n_rx": n_rx, "ch_per_rx": ch,
                              "value": round(med["wfde_one_fault"] / med["wfde_clean"], 3),
                              "second_round_us": round(med["wfde_one_fault"] - med["wfde_clean"], 3)}), flush=True)
            for p in (d_fix, d_fde) + dev["clean"] + dev["one_fault"]:
                eng.free(p)
    finally:
        sys.stdout = tee.out
        tee.file.close()
        eng.close()


VEL_OUT = os.path.join(ROOT, "profiles", "r22_weighted_vel_bench.jsonl")


def weighted_vel(shapes, out=VEL_OUT):
    """k_wvel at k_wfix's shapes, every slot usable, receivers at 36 m/s: gpsx_wvel_dev on the fix records that gpsx_wfix_dev left on the
    device, beside gpsx_wfix_dev (cold start) on the same arrays, the calls taking turns; the lines go to stdout and to `out`"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import weighted_fix_cases as W
    import weighted_vel_cases as K
    from stm32f4_sdr_gps_amd import capi
    tee = sys.stdout = _Tee(out)
    eng = capi.Engine(0)
    names = sorted(W.SITES)
    try:
        for n_rx, ch in shapes:
            pool = [K.receiver(names[k % len(names)], ch, 3 * k, K.VELOCITIES[1], K.DRIFTS[1]) for k in range(16)]      # --weighted-fix's sixteen skies
            obs, eph = W.pack([pool[r % 16] for r in range(n_rx)], ch)
            fix_cfg, vel_cfg = capi.wfix_cfg(W.OFFSET_MS, ch), capi.wvel_cfg(ch)
            d_obs, d_eph, d_fix, d_fix2, d_vel = eng.malloc(obs.nbytes), eng.malloc(eph.nbytes), eng.malloc(n_rx * 128), eng.malloc(n_rx * 128), eng.malloc(n_rx * 112)
            eng.h2d(d_obs, obs)
            eng.h2d(d_eph, eph)

            def wfix(d_out):
                return eng.lib.gpsx_wfix_dev(eng.h, fix_cfg.ctypes.data, C.c_void_p(d_obs), C.c_void_p(d_eph), None, None, n_rx, C.c_void_p(d_out), None)

            eng._chk(wfix(d_fix), "gpsx_wfix_dev")
            eng.synchronize()
            calls = {"wfix": (1, lambda: wfix(d_fix2)),
                     "wvel": (1, lambda: eng.lib.gpsx_wvel_dev(eng.h, vel_cfg.ctypes.data, C.c_void_p(d_obs), C.c_void_p(d_eph), None, C.c_void_p(d_fix), n_rx,
                                                               C.c_void_p(d_vel)))}
            med = _timed_rows(eng, calls, {"channels": n_rx * ch, "n_rx": n_rx, "ch_per_rx": ch, "read_bytes": obs.nbytes + eph.nbytes + n_rx * 128})
            vel = np.zeros(n_rx, capi.WVEL_DTYPE)
            eng.d2h(vel, d_vel)
            err = np.linalg.norm(vel["vel"] - np.array(K.VELOCITIES[1]), axis=1)
            print(json.dumps({"wvel_check": "records after the timed launches", "n_rx": n_rx, "ch_per_rx": ch, "solved": int((vel["flags"] == capi.WVEL_FLAG_VEL).sum()),
                              "n_used_min": int(vel["n_used"].min()), "largest_velocity_error_mps": round(float(err.max()), 5)}), flush=True)
            print(json.dumps({"ratio": "k_wvel over k_wfix on the same arrays", "n_rx": n_rx, "ch_per_rx": ch, "value": round(med["wvel"] / med["wfix"], 3),
                              "cheaper": bool(med["wvel"] < med["wfix"]), "ns_per_receiver": round(med["wvel"] / n_rx * 1e3, 2),
                              "read_GBps": round((obs.nbytes + eph.nbytes + n_rx * 128) / med["wvel"] / 1e3, 2)}), flush=True)
            for p in (d_obs, d_eph, d_fix, d_fix2, d_vel):
                eng.free(p)
    finally:
        sys.stdout = tee.out
        tee.file.close()
        eng.close()


KF_OUT = os.path.join(ROOT, "profiles", "r24_weighted_kf_bench.jsonl")


def weighted_kf(shapes, out=KF_OUT):
    """k_wkf at k_wfix's shapes, every slot usable, receivers at 36 m/s whose clocks drift by 1e-6: the states are initialised from
    gpsx_wfix_dev's and gpsx_wvel_dev's records of one launch; the timed call is the update of the NEXT launch (1000 blocks later),
    and because a filter call advances its state, each timed launch is preceded by a device-to-device copy that puts the initialised
    states back -- that copy is timed alone beside it and subtracted.  The yardstick is k_wfix (warm start) + k_wvel on the same
    records, the calls taking turns; the lines go to stdout and to `out`"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import weighted_fix_cases as W
    import weighted_kf_cases as K
    from stm32f4_sdr_gps_amd import capi
    hip = C.CDLL("libamdhip64.so")
    hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    tee = sys.stdout = _Tee(out)
    eng = capi.Engine(0, stream=stream.value)
    names = sorted(W.SITES)
    try:
        for n_rx, ch in shapes:
            pool = [K.track(names[k % len(names)], ch, 3 * k, K.VELOCITY, 1e-6, 2) for k in range(16)]      # --weighted-fix's sixteen skies
            obs0, eph = W.pack([(pool[r % 16][0][0]["obs"], pool[r % 16][1]) for r in range(n_rx)], ch)
            obs1, _ = W.pack([(pool[r % 16][0][1]["obs"], pool[r % 16][1]) for r in range(n_rx)], ch)
            fix_cfg, vel_cfg, kf_cfg = capi.wfix_cfg(W.OFFSET_MS, ch), capi.wvel_cfg(ch), capi.wkf_cfg(ch)
            state_bytes = n_rx * capi.WKF_STATE_DTYPE.itemsize
            d_obs0, d_obs1, d_eph = eng.malloc(obs0.nbytes), eng.malloc(obs1.nbytes), eng.malloc(eph.nbytes)
            d_fix, d_fix2, d_vel, d_vel2 = eng.malloc(n_rx * 128), eng.malloc(n_rx * 128), eng.malloc(n_rx * 112), eng.malloc(n_rx * 112)
            d_state, d_state0, d_kf = eng.malloc(state_bytes), eng.malloc(state_bytes), eng.malloc(n_rx * capi.WKF_DTYPE.itemsize)
            for d, a in ((d_obs0, obs0), (d_obs1, obs1), (d_eph, eph), (d_state0, np.zeros(n_rx, capi.WKF_STATE_DTYPE))):
                eng.h2d(d, a)

            def wfix(d_o, d_prev, d_out):
                return eng.lib.gpsx_wfix_dev(eng.h, fix_cfg.ctypes.data, C.c_void_p(d_o), C.c_void_p(d_eph), None, None if d_prev is None else C.c_void_p(d_prev),
                                             n_rx, C.c_void_p(d_out), None)

            def wvel(d_o, d_f, d_out):
                return eng.lib.gpsx_wvel_dev(eng.h, vel_cfg.ctypes.data, C.c_void_p(d_o), C.c_void_p(d_eph), None, C.c_void_p(d_f), n_rx, C.c_void_p(d_out))

            def wkf(d_o, d_st):
                return eng.lib.gpsx_wkf_dev(eng.h, kf_cfg.ctypes.data, C.c_void_p(d_o), C.c_void_p(d_eph), None, C.c_void_p(d_fix), C.c_void_p(d_vel), n_rx, 1000,
                                            C.c_void_p(d_st), C.c_void_p(d_kf))

            def restore():
                return hip.hipMemcpyAsync(d_state, d_state0, state_bytes, 3, stream)

            def restore_and_update():
                restore()
                return wkf(d_obs1, d_state)

            eng._chk(wfix(d_obs0, None, d_fix), "gpsx_wfix_dev")
            eng._chk(wvel(d_obs0, d_fix, d_vel), "gpsx_wvel_dev")
            eng._chk(wkf(d_obs0, d_state0), "gpsx_wkf_dev")      # INIT: what every timed launch starts from
            eng.synchronize()
            calls = {"d2d_copy_of_the_states": (1, restore),
                     "wfix_warm": (1, lambda: wfix(d_obs1, d_fix, d_fix2)),
                     "wvel": (1, lambda: wvel(d_obs1, d_fix, d_vel2)),
                     "state_copy_then_wkf": (1, restore_and_update)}
            med = _timed_rows(eng, calls, {"channels": n_rx * ch, "n_rx": n_rx, "ch_per_rx": ch, "state_bytes": state_bytes,
                                           "read_bytes": obs1.nbytes + eph.nbytes + state_bytes})
            kf = np.zeros(n_rx, capi.WKF_DTYPE)
            eng.d2h(kf, d_kf)
            truth = np.stack([pool[r % 16][0][1]["rx"] for r in range(n_rx)])
            print(json.dumps({"wkf_check": "records after the timed launches", "n_rx": n_rx, "ch_per_rx": ch,
                              "updated": int((kf["flags"] == capi.WKF_FLAG_UPDATED).sum()), "n_pr_min": int(kf["n_pr"].min()), "n_dop_min": int(kf["n_dop"].min()),
                              "largest_position_error_m": round(float(np.linalg.norm(kf["rr"] - truth, axis=1).max()), 4)}), flush=True)
            own = med["state_copy_then_wkf"] - med["d2d_copy_of_the_states"]
            both = med["wfix_warm"] + med["wvel"]
            print(json.dumps({"ratio": "k_wkf (the timed pair less the state copy) over k_wfix + k_wvel on the same records", "n_rx": n_rx, "ch_per_rx": ch,
                              "wkf_us": round(own, 3), "wfix_plus_wvel_us": round(both, 3), "value": round(own / both, 3), "cheaper": bool(own < both),
                              "over_the_state_copy": round(own / med["d2d_copy_of_the_states"], 2), "ns_per_receiver": round(own / n_rx * 1e3, 2)}), flush=True)
            for p in (d_obs0, d_obs1, d_eph, d_fix, d_fix2, d_vel, d_vel2, d_state, d_state0, d_kf):
                eng.free(p)
    finally:
        sys.stdout = tee.out
        tee.file.close()
        eng.close()


ACQ_OUT = os.path.join(ROOT, "profiles", "r27_weighted_acq_bench.jsonl")
ACQ_SHAPES = [(256, 32, 201, 12), (4096, 32, 41, 8), (16384, 32, 21, 4)]


def weighted_acq(shapes, out=ACQ_OUT):
    """k_wacq at (receivers, PRNs, bins, slots per receiver): noise records with eight PRNs per receiver standing out, half of a
    receiver's slots empty and half holding a channel with code lock, so that every receiver hands over ch / 2 PRNs and drops the rest.
    A call changes the sync states it hands over to, so each timed launch is preceded by a device-to-device copy that puts the sync
    states back -- timed alone beside it and subtracted.  The yardsticks: a device-to-device copy of the peak records the kernel reads,
    and gpsx_memcpy_d2h of them into page-locked host memory, the first step of the host path; the calls take turns; the lines go to
    stdout and to `out`"""
    from stm32f4_sdr_gps_amd import capi
    hip = C.CDLL("libamdhip64.so")
    hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    tee = sys.stdout = _Tee(out)
    eng = capi.Engine(0, stream=stream.value)
    try:
        for n_rx, n_prn, n_dopp, ch in shapes:
            rng = np.random.default_rng(27)
            peaks = np.zeros((n_rx, n_prn, n_dopp), capi.PEAK_DTYPE)
            peaks["max_val"] = rng.integers(15000, 18000, peaks.shape)
            peaks["sum"] = 138000000
            peaks["phase"] = rng.integers(0, 16368, peaks.shape)
            for k in range(8):                   # PRN indices 4 k + (r % 4) stand out in a bin of their own
                r = np.arange(n_rx)
                peaks["max_val"][r, (4 * k + r % 4) % n_prn, (37 * k + r) % n_dopp] = 60000 + 1000 * k
            peaks["avr"] = peaks["sum"] // 16368
            prns = np.arange(1, n_prn + 1, dtype=np.uint8)
            n_ch = n_rx * ch
            sync = np.zeros(n_ch, capi.WSYNC_STATE_DTYPE)
            sync["loop"]["prn"] = np.where(np.arange(n_ch) % 2 == 0, capi.PRN_NONE, 100 + np.arange(n_ch) % ch)
            lock = np.zeros(n_ch, capi.WLOCK_STATE_DTYPE)
            lock["flags"], lock["blocks_seen"] = capi.WLOCK_FLAG_CODE, 5000
            cfg = capi.wacq_cfg(ch, (4, 1), 0, 80, capi.WAID_L1CA, 1000)
            g = capi.AcqWeightedT(n_rx, 80, n_prn, prns.ctypes.data_as(C.POINTER(C.c_uint8)), -5000, 10000 // max(n_dopp - 1, 1), n_dopp, 1)
            sizes = [n_ch * capi.WNAV_STATE_DTYPE.itemsize, n_ch * capi.WOBS_STATE_DTYPE.itemsize, n_ch * capi.WEPH_STATE_DTYPE.itemsize]
            d_pk, d_copy, d_sync, d_sync0, d_lock = (eng.malloc(b) for b in (peaks.nbytes, peaks.nbytes, sync.nbytes, sync.nbytes, lock.nbytes))
            d_nav, d_obs, d_eph = (eng.malloc(b) for b in sizes)
            d_acq, d_det = eng.malloc(n_rx * capi.WACQ_DTYPE.itemsize), eng.malloc(n_rx * n_prn * capi.WACQ_DET_DTYPE.itemsize)
            host = eng.host_array(peaks.shape, capi.PEAK_DTYPE)
            for d, a in ((d_pk, peaks), (d_sync0, sync), (d_sync, sync), (d_lock, lock), (d_nav, np.zeros(sizes[0], np.uint8)),
                         (d_obs, np.zeros(sizes[1], np.uint8)), (d_eph, np.zeros(sizes[2], np.uint8))):
                eng.h2d(d, a)

            def restore():
                return hip.hipMemcpyAsync(d_sync, d_sync0, sync.nbytes, 3, stream)

            def wacq():
                return eng.lib.gpsx_wacq_dev(eng.h, cfg.ctypes.data, C.addressof(g), C.c_void_p(d_pk), C.c_void_p(d_sync), C.c_void_p(d_lock), C.c_void_p(d_nav),
                                             C.c_void_p(d_obs), C.c_void_p(d_eph), C.c_void_p(d_acq), C.c_void_p(d_det))

            def restore_and_decide():
                restore()
                return wacq()

            calls = {"d2d_copy_of_the_sync_states": (1, restore),
                     "d2d_copy_of_the_peaks": (1, lambda: hip.hipMemcpyAsync(d_copy, d_pk, peaks.nbytes, 3, stream)),
                     "memcpy_d2h_of_the_peaks": (1, lambda: eng.lib.gpsx_memcpy_d2h(eng.h, host.ctypes.data, C.c_void_p(d_pk), peaks.nbytes)),
                     "state_copy_then_wacq": (1, restore_and_decide)}
            med = _timed_rows(eng, calls, {"channels": n_ch, "n_rx": n_rx, "n_prn": n_prn, "n_dopp": n_dopp, "ch_per_rx": ch, "peak_bytes": peaks.nbytes},
                              per_channel_ms=False)
            acq = np.zeros(n_rx, capi.WACQ_DTYPE)
            eng.d2h(acq, d_acq)
            print(json.dumps({"wacq_check": "records after the timed launches", "n_rx": n_rx, "detected_per_rx": [int(acq["n_detected"].min()), int(acq["n_detected"].max())],
                              "assigned_per_rx": [int(acq["n_assigned"].min()), int(acq["n_assigned"].max())],
                              "dropped_per_rx": [int(acq["n_dropped"].min()), int(acq["n_dropped"].max())]}), flush=True)
            own = med["state_copy_then_wacq"] - med["d2d_copy_of_the_sync_states"]
            print(json.dumps({"ratio": "k_wacq (the timed pair less the state copy) over the two yardsticks", "n_rx": n_rx, "n_prn": n_prn, "n_dopp": n_dopp,
                              "ch_per_rx": ch, "wacq_us": round(own, 3), "over_d2d_copy_of_the_peaks": round(own / med["d2d_copy_of_the_peaks"], 3),
                              "over_memcpy_d2h_of_the_peaks": round(own / med["memcpy_d2h_of_the_peaks"], 4),
                              "cheaper_than_the_host_copy": bool(own < med["memcpy_d2h_of_the_peaks"]), "ns_per_receiver": round(own / n_rx * 1e3, 2),
                              "read_GBps": round(peaks.nbytes / own / 1e3, 1)}), flush=True)
            for p in (d_pk, d_copy, d_sync, d_sync0, d_lock, d_nav, d_obs, d_eph, d_acq, d_det):
                eng.free(p)
    finally:
        sys.stdout = tee.out
        tee.file.close()
        eng.close()


BANK_OUT = os.path.join(ROOT, "profiles", "r28_weighted_pred_bench.jsonl")
BANK_SHAPES = [(256, 32, 8), (256, 32, 12), (4096, 32, 8), (4096, 32, 12), (16384, 32, 8), (16384, 32, 12)]


def weighted_bank(shapes, out=BANK_OUT):
    """k_wbank at (receivers, PRNs, slots per receiver) on --weighted-kf's records (real ephemerides, every slot on a listed PRN of its
    own): the steady state of a tracking receiver whose bank is full -- three slots of four offer a set of the bank's own toe (stored
    again: a refresh), the fourth has no set and takes the bank's.  Such a call leaves the bank as it was, so the timed launches need no
    copy that puts anything back.  It is timed with the merged copy apart from d_eph and without one (in place a call changes its own
    input: not timed).  The yardsticks: a device-to-device copy of
    the ephemeris records the kernel reads, and k_wkf's update at the same receivers on the same records (as --weighted-kf times it:
    the pair of state copy and update less the state copy); the calls take turns; the lines go to stdout and to `out`.  Behind it, on
    the same receivers, k_wpred (see the comment there)"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import weighted_fix_cases as W
    import weighted_kf_cases as K
    from stm32f4_sdr_gps_amd import capi
    hip = C.CDLL("libamdhip64.so")
    hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    tee = sys.stdout = _Tee(out)
    eng = capi.Engine(0, stream=stream.value)
    names = sorted(W.SITES)
    try:
        for n_rx, n_prn, ch in shapes:
            pool = [K.track(names[k % len(names)], ch, 3 * k, K.VELOCITY, 1e-6, 2) for k in range(16)]
            obs0, eph = W.pack([(pool[r % 16][0][0]["obs"], pool[r % 16][1]) for r in range(n_rx)], ch)
            obs1, _ = W.pack([(pool[r % 16][0][1]["obs"], pool[r % 16][1]) for r in range(n_rx)], ch)
            n_ch = n_rx * ch
            prns = np.arange(1, n_prn + 1, dtype=np.uint8)
            index = (np.arange(n_ch) // ch + np.arange(n_ch) % ch) % n_prn          # receiver r's slot j: PRN index (r + j) mod n_prn
            sync = np.zeros(n_ch, capi.WSYNC_STATE_DTYPE)
            sync["loop"]["prn"] = prns[index]
            bank = np.zeros((n_rx, n_prn), capi.WEPH_DTYPE)
            bank[np.arange(n_ch) // ch, index] = eph
            bank["flags"] &= capi.WEPH_FLAG_VALID
            launch_eph = eph.copy()
            launch_eph["flags"][3::4] = 0
            fix_cfg, vel_cfg, kf_cfg, bank_cfg = capi.wfix_cfg(W.OFFSET_MS, ch), capi.wvel_cfg(ch), capi.wkf_cfg(ch), capi.wbank_cfg(ch)
            state_bytes = n_rx * capi.WKF_STATE_DTYPE.itemsize
            d_obs0, d_obs1, d_eph, d_leph, d_out, d_copy = (eng.malloc(b) for b in (obs0.nbytes, obs1.nbytes, eph.nbytes, eph.nbytes, eph.nbytes, eph.nbytes))
            d_fix, d_vel, d_state, d_state0, d_kf = (eng.malloc(b) for b in (n_rx * 128, n_rx * 112, state_bytes, state_bytes, n_rx * capi.WKF_DTYPE.itemsize))
            d_sync, d_bank, d_rep = eng.malloc(sync.nbytes), eng.malloc(bank.nbytes), eng.malloc(n_rx * capi.WBANK_DTYPE.itemsize)
            for d, a in ((d_obs0, obs0), (d_obs1, obs1), (d_eph, eph), (d_leph, launch_eph), (d_state0, np.zeros(n_rx, capi.WKF_STATE_DTYPE)), (d_sync, sync),
                         (d_bank, bank)):
                eng.h2d(d, a)

            def wkf(d_o, d_st):
                return eng.lib.gpsx_wkf_dev(eng.h, kf_cfg.ctypes.data, C.c_void_p(d_o), C.c_void_p(d_eph), None, C.c_void_p(d_fix), C.c_void_p(d_vel), n_rx, 1000,
                                            C.c_void_p(d_st), C.c_void_p(d_kf))

            def restore():
                return hip.hipMemcpyAsync(d_state, d_state0, state_bytes, 3, stream)

            def restore_and_update():
                restore()
                return wkf(d_obs1, d_state)

            def wbank(d_o):
                return eng.lib.gpsx_wbank_dev(eng.h, bank_cfg.ctypes.data, n_rx, n_prn, prns.ctypes.data, C.c_void_p(d_sync), C.c_void_p(d_leph), C.c_void_p(d_bank),
                                              None if d_o is None else C.c_void_p(d_o), C.c_void_p(d_rep))

            eng._chk(eng.lib.gpsx_wfix_dev(eng.h, fix_cfg.ctypes.data, C.c_void_p(d_obs0), C.c_void_p(d_eph), None, None, n_rx, C.c_void_p(d_fix), None), "gpsx_wfix_dev")
            eng._chk(eng.lib.gpsx_wvel_dev(eng.h, vel_cfg.ctypes.data, C.c_void_p(d_obs0), C.c_void_p(d_eph), None, C.c_void_p(d_fix), n_rx, C.c_void_p(d_vel)),
                     "gpsx_wvel_dev")
            eng._chk(wkf(d_obs0, d_state0), "gpsx_wkf_dev")      # INIT: what every timed update starts from
            eng.synchronize()
            calls = {"d2d_copy_of_the_states": (1, restore),
                     "d2d_copy_of_the_eph_records": (1, lambda: hip.hipMemcpyAsync(d_copy, d_leph, eph.nbytes, 3, stream)),
                     "state_copy_then_wkf": (1, restore_and_update),
                     "wbank_no_merged_copy": (1, lambda: wbank(None)),
                     "wbank_merged_apart": (1, lambda: wbank(d_out))}
            med = _timed_rows(eng, calls, {"channels": n_ch, "n_rx": n_rx, "n_prn": n_prn, "ch_per_rx": ch, "eph_bytes": eph.nbytes, "bank_bytes": bank.nbytes},
                              per_channel_ms=False)
            rep, kf = np.zeros(n_rx, capi.WBANK_DTYPE), np.zeros(n_rx, capi.WKF_DTYPE)
            eng.d2h(rep, d_rep)
            eng.d2h(kf, d_kf)
            after = np.zeros_like(bank)
            eng.d2h(after, d_bank)
            print(json.dumps({"wbank_check": "records after the timed launches", "n_rx": n_rx, "stored_per_rx": [int(rep["n_stored"].min()), int(rep["n_stored"].max())],
                              "from_bank_per_rx": [int(rep["n_from_bank"].min()), int(rep["n_from_bank"].max())],
                              "bank_unchanged": bool(after.tobytes() == bank.tobytes()), "wkf_updated": int((kf["flags"] == capi.WKF_FLAG_UPDATED).sum())}), flush=True)
            own_kf = med["state_copy_then_wkf"] - med["d2d_copy_of_the_states"]
            own = med["wbank_merged_apart"]
            print(json.dumps({"ratio": "k_wbank (merged copy apart) over the two yardsticks", "n_rx": n_rx, "n_prn": n_prn, "ch_per_rx": ch, "wbank_us": round(own, 3),
                              "wbank_no_copy_us": round(med["wbank_no_merged_copy"], 3),
                              "wkf_us": round(own_kf, 3), "over_d2d_copy_of_the_eph_records": round(own / med["d2d_copy_of_the_eph_records"], 3),
                              "over_wkf": round(own / own_kf, 3), "ns_per_receiver": round(own / n_rx * 1e3, 2),
                              "moved_GBps": round((eph.nbytes * 2 + eph.nbytes * 3 // 4 * 2) / own / 1e3, 1)}), flush=True)
            # -- k_wpred on the same receivers: their initialised filter states and the full bank; half of every receiver's slots emptied,
            #    so that handover = 1 hands satellites over (a device-to-device copy puts the sync states back before every timed launch;
            #    it is timed alone and subtracted); max_sigma_hz is wide open, because a freshly initialised filter's drift prior is 500 m/s
            sync_h = sync.copy()
            sync_h["loop"]["prn"][1::2] = capi.PRN_NONE
            d_sync_h, d_sync_h0, d_states_copy = eng.malloc(sync.nbytes), eng.malloc(sync.nbytes), eng.malloc(state_bytes + bank.nbytes)
            eng.h2d(d_sync_h, sync_h)
            eng.h2d(d_sync_h0, sync_h)
            d_prx, d_ppred = eng.malloc(n_rx * capi.WPRED_RX_DTYPE.itemsize), eng.malloc(n_rx * n_prn * capi.WPRED_DTYPE.itemsize)
            pcfg = {h: capi.wpred_cfg(ch, capi.WVEL_L1CA, max_sigma_m=1e4, max_sigma_hz=1e4, lead_blocks=20, handover=h) for h in (0, 1)}

            def wpred(h, d_s):
                return eng.lib.gpsx_wpred_dev(eng.h, pcfg[h].ctypes.data, n_rx, n_prn, prns.ctypes.data, C.c_void_p(d_state0), C.c_void_p(d_bank), C.c_void_p(d_s),
                                              None, None, None, None, C.c_void_p(d_prx), C.c_void_p(d_ppred))

            def restore_slots():
                return hip.hipMemcpyAsync(d_sync_h, d_sync_h0, sync.nbytes, 3, stream)

            def restore_and_hand_over():
                restore_slots()
                return wpred(1, d_sync_h)

            pcalls = {"d2d_copy_of_the_sync_states": (1, restore_slots),
                      "d2d_copy_of_the_filter_states_and_the_bank": (1, lambda: hip.hipMemcpyAsync(d_states_copy, d_bank, bank.nbytes, 3, stream) or
                                                                     hip.hipMemcpyAsync(d_states_copy + bank.nbytes, d_state0, state_bytes, 3, stream)),
                      "state_copy_then_wkf": (1, restore_and_update),
                      "d2d_copy_of_the_states": (1, restore),
                      "wpred_predict_only": (1, lambda: wpred(0, d_sync_h0)),
                      "slot_copy_then_wpred_handover": (1, restore_and_hand_over)}
            pmed = _timed_rows(eng, pcalls, {"channels": n_ch, "n_rx": n_rx, "n_prn": n_prn, "ch_per_rx": ch, "read_bytes": state_bytes + bank.nbytes},
                               per_channel_ms=False)
            prx = np.zeros(n_rx, capi.WPRED_RX_DTYPE)
            eng.d2h(prx, d_prx)
            print(json.dumps({"wpred_check": "records after the timed launches", "n_rx": n_rx, "have_per_rx": [int(prx["n_have"].min()), int(prx["n_have"].max())],
                              "visible_per_rx": [int(prx["n_visible"].min()), int(prx["n_visible"].max())],
                              "assigned_per_rx": [int(prx["n_assigned"].min()), int(prx["n_assigned"].max())],
                              "tracked_per_rx": [int(prx["n_tracked"].min()), int(prx["n_tracked"].max())]}), flush=True)
            own_p = pmed["slot_copy_then_wpred_handover"] - pmed["d2d_copy_of_the_sync_states"]
            own_k = pmed["state_copy_then_wkf"] - pmed["d2d_copy_of_the_states"]
            print(json.dumps({"ratio": "k_wpred with handover = 1 (the timed pair less the slot copy) over the two yardsticks", "n_rx": n_rx, "n_prn": n_prn,
                              "ch_per_rx": ch, "wpred_us": round(own_p, 3), "wpred_predict_only_us": round(pmed["wpred_predict_only"], 3), "wkf_us": round(own_k, 3),
                              "over_d2d_copy_of_what_it_reads": round(own_p / pmed["d2d_copy_of_the_filter_states_and_the_bank"], 3),
                              "over_wkf": round(own_p / own_k, 3), "ns_per_receiver": round(own_p / n_rx * 1e3, 2),
                              "ns_per_satellite_evaluation": round(own_p / max(int(prx["n_have"].sum()) * 3, 1) * 1e3, 3)}), flush=True)
            for p in (d_sync_h, d_sync_h0, d_states_copy, d_prx, d_ppred):
                eng.free(p)
            for p in (d_obs0, d_obs1, d_eph, d_leph, d_out, d_copy, d_fix, d_vel, d_state, d_state0, d_kf, d_sync, d_bank, d_rep):
                eng.free(p)
    finally:
        sys.stdout = tee.out
        tee.file.close()
        eng.close()


TOW_OUT = os.path.join(ROOT, "profiles", "r29_weighted_tow_bench.jsonl")


def weighted_tow(shapes, out=TOW_OUT):
    """k_wtow at (receivers, PRNs, slots per receiver) behind k_wpred on --weighted-bank's receivers (real ephemerides, initialised filter
    states, a full bank, every slot on a listed PRN of its own): gpsx_wpred_dev predicts once, and the observable states are made from its
    records -- a running chain without an anchor in every slot, the loop's phase the predicted one, the edge on the 20 ms grid.  Timed:
    the call that anchors every slot (a device-to-device copy puts the states back before every timed launch; it is timed alone and
    subtracted), with and without d_obs, and the steady state behind it (every slot AGREES, nothing is written).  The yardsticks: a
    device-to-device copy of the bytes the kernel reads (the prediction's records and the observable states), and k_wpred predicting only
    at the same receivers; the calls take turns; the lines go to stdout and to `out`"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import weighted_fix_cases as W
    import weighted_kf_cases as K
    from stm32f4_sdr_gps_amd import capi
    hip = C.CDLL("libamdhip64.so")
    hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    tee = sys.stdout = _Tee(out)
    eng = capi.Engine(0, stream=stream.value)
    names = sorted(W.SITES)
    try:
        for n_rx, n_prn, ch in shapes:
            pool = [K.track(names[k % len(names)], ch, 3 * k, K.VELOCITY, 1e-6, 2) for k in range(16)]
            obs0, eph = W.pack([(pool[r % 16][0][0]["obs"], pool[r % 16][1]) for r in range(n_rx)], ch)
            n_ch = n_rx * ch
            prns = np.arange(1, n_prn + 1, dtype=np.uint8)
            index = (np.arange(n_ch) // ch + np.arange(n_ch) % ch) % n_prn          # receiver r's slot j: PRN index (r + j) mod n_prn
            sync = np.zeros(n_ch, capi.WSYNC_STATE_DTYPE)
            sync["loop"]["prn"], sync["mode"] = prns[index], 2
            bank = np.zeros((n_rx, n_prn), capi.WEPH_DTYPE)
            bank[np.arange(n_ch) // ch, index] = eph
            bank["flags"] &= capi.WEPH_FLAG_VALID
            fix_cfg, vel_cfg, kf_cfg = capi.wfix_cfg(W.OFFSET_MS, ch), capi.wvel_cfg(ch), capi.wkf_cfg(ch)
            pcfg = capi.wpred_cfg(ch, capi.WVEL_L1CA, max_sigma_m=1e4, max_sigma_hz=1e4, lead_blocks=20, handover=0)
            tcfg = capi.wtow_cfg(ch, max_sigma_m=1e4, max_resid_samples=8.0, max_age_blocks=40, resolve=1, rearm=0)
            state_bytes = n_rx * capi.WKF_STATE_DTYPE.itemsize
            prx_bytes, ppred_bytes = n_rx * capi.WPRED_RX_DTYPE.itemsize, n_rx * n_prn * capi.WPRED_DTYPE.itemsize
            st_bytes, o_bytes = n_ch * capi.WOBS_STATE_DTYPE.itemsize, n_ch * capi.WOBS_DTYPE.itemsize
            d_obs0, d_eph, d_fix, d_vel, d_state0, d_kf = (eng.malloc(b) for b in (obs0.nbytes, eph.nbytes, n_rx * 128, n_rx * 112, state_bytes,
                                                                                   n_rx * capi.WKF_DTYPE.itemsize))
            d_sync, d_bank, d_prx, d_ppred = (eng.malloc(b) for b in (sync.nbytes, bank.nbytes, prx_bytes, ppred_bytes))
            d_st, d_st0, d_o, d_tow, d_tow_rx, d_copy = (eng.malloc(b) for b in (st_bytes, st_bytes, o_bytes, n_ch * capi.WTOW_DTYPE.itemsize,
                                                                               n_rx * capi.WTOW_RX_DTYPE.itemsize, prx_bytes + ppred_bytes + st_bytes))
            for d, a in ((d_obs0, obs0), (d_eph, eph), (d_state0, np.zeros(n_rx, capi.WKF_STATE_DTYPE)), (d_sync, sync), (d_bank, bank)):
                eng.h2d(d, a)
            eng._chk(eng.lib.gpsx_wfix_dev(eng.h, fix_cfg.ctypes.data, C.c_void_p(d_obs0), C.c_void_p(d_eph), None, None, n_rx, C.c_void_p(d_fix), None), "gpsx_wfix_dev")
            eng._chk(eng.lib.gpsx_wvel_dev(eng.h, vel_cfg.ctypes.data, C.c_void_p(d_obs0), C.c_void_p(d_eph), None, C.c_void_p(d_fix), n_rx, C.c_void_p(d_vel)),
                     "gpsx_wvel_dev")
            eng._chk(eng.lib.gpsx_wkf_dev(eng.h, kf_cfg.ctypes.data, C.c_void_p(d_obs0), C.c_void_p(d_eph), None, C.c_void_p(d_fix), C.c_void_p(d_vel), n_rx, 1000,
                                          C.c_void_p(d_state0), C.c_void_p(d_kf)), "gpsx_wkf_dev")      # INIT

            def wpred():
                return eng.lib.gpsx_wpred_dev(eng.h, pcfg.ctypes.data, n_rx, n_prn, prns.ctypes.data, C.c_void_p(d_state0), C.c_void_p(d_bank), C.c_void_p(d_sync),
                                              None, None, None, None, C.c_void_p(d_prx), C.c_void_p(d_ppred))
            eng._chk(wpred(), "gpsx_wpred_dev")
            eng.synchronize()
            pred = np.zeros((n_rx, n_prn), capi.WPRED_DTYPE)
            eng.d2h(pred, d_ppred)
            w = pred[np.arange(n_ch) // ch, index]                                 # every slot's record
            st = np.zeros(n_ch, capi.WOBS_STATE_DTYPE)                              # a running chain without an anchor, the edge on the 20 ms grid
            st["blocks_seen"], st["last_bit_end_p1"], st["chain_first_p1"], st["last_win_end_p1"] = 25000, 24997, 24597, 24990
            st["edge_block"] = 25000 - w["tx_ms"] % 20
            st["last_phase"] = np.minimum(w["code_phase"].astype(np.float32), np.float32(16367.0))
            st["flags"] = 3                                                          # PHASE | EDGE
            eng.h2d(d_st0, st)
            eng.h2d(d_st, st)
            eng.h2d(d_o, np.zeros(n_ch, capi.WOBS_DTYPE))

            def wtow(d_states, d_obs):
                return eng.lib.gpsx_wtow_dev(eng.h, tcfg.ctypes.data, n_rx, n_prn, prns.ctypes.data, C.c_void_p(d_prx), C.c_void_p(d_ppred), C.c_void_p(d_sync),
                                             C.c_void_p(d_states), None if d_obs is None else C.c_void_p(d_obs), C.c_void_p(d_tow), C.c_void_p(d_tow_rx))

            def restore():
                return hip.hipMemcpyAsync(d_st, d_st0, st_bytes, 3, stream)

            def copy_of_what_it_reads():
                return (hip.hipMemcpyAsync(d_copy, d_prx, prx_bytes, 3, stream) or hip.hipMemcpyAsync(d_copy + prx_bytes, d_ppred, ppred_bytes, 3, stream) or
                        hip.hipMemcpyAsync(d_copy + prx_bytes + ppred_bytes, d_st0, st_bytes, 3, stream))
            eng._chk(wtow(d_st, d_o), "gpsx_wtow_dev")
            eng.synchronize()
            first = np.zeros(n_rx, capi.WTOW_RX_DTYPE)
            eng.d2h(first, d_tow_rx)
            calls = {"d2d_copy_of_the_obs_states": (1, restore),
                     "d2d_copy_of_what_it_reads": (1, copy_of_what_it_reads),
                     "state_copy_then_wtow_aids": (1, lambda: restore() or wtow(d_st, d_o)),
                     "state_copy_then_wtow_aids_no_obs": (1, lambda: restore() or wtow(d_st, None)),
                     "wpred_predict_only": (1, wpred)}
            med = _timed_rows(eng, calls, {"channels": n_ch, "n_rx": n_rx, "n_prn": n_prn, "ch_per_rx": ch, "read_bytes": prx_bytes + ppred_bytes + st_bytes},
                              per_channel_ms=False)
            eng._chk(wtow(d_st, d_o), "gpsx_wtow_dev")                              # (the last timed launch aided without d_obs: d_st is anchored)
            med.update(_timed_rows(eng, {"wtow_agrees": (1, lambda: wtow(d_st, d_o))},
                                   {"channels": n_ch, "n_rx": n_rx, "n_prn": n_prn, "ch_per_rx": ch, "read_bytes": prx_bytes + ppred_bytes + st_bytes}, per_channel_ms=False))
            steady = np.zeros(n_rx, capi.WTOW_RX_DTYPE)
            eng.d2h(steady, d_tow_rx)
            print(json.dumps({"wtow_check": "records of the first launch and after the timed ones", "n_rx": n_rx,
                              "aided_per_rx_first": [int(first["n_aided"].min()), int(first["n_aided"].max())],
                              "agrees_per_rx_steady": [int(steady["n_agrees"].min()), int(steady["n_agrees"].max())],
                              "aided_steady": int(steady["n_aided"].sum()), "inconsistent_first": int(first["n_inconsistent"].sum())}), flush=True)
            own = med["state_copy_then_wtow_aids"] - med["d2d_copy_of_the_obs_states"]
            print(json.dumps({"ratio": "k_wtow anchoring every slot (the timed pair less the state copy) over the two yardsticks", "n_rx": n_rx, "n_prn": n_prn,
                              "ch_per_rx": ch, "wtow_us": round(own, 3),
                              "wtow_no_obs_us": round(med["state_copy_then_wtow_aids_no_obs"] - med["d2d_copy_of_the_obs_states"], 3),
                              "wtow_agrees_us": round(med["wtow_agrees"], 3), "wpred_predict_only_us": round(med["wpred_predict_only"], 3),
                              "over_d2d_copy_of_what_it_reads": round(own / med["d2d_copy_of_what_it_reads"], 3),
                              "agrees_over_d2d_copy_of_what_it_reads": round(med["wtow_agrees"] / med["d2d_copy_of_what_it_reads"], 3),
                              "over_wpred_predict_only": round(own / med["wpred_predict_only"], 3), "ns_per_receiver": round(own / n_rx * 1e3, 2)}), flush=True)
            for p in (d_obs0, d_eph, d_fix, d_vel, d_state0, d_kf, d_sync, d_bank, d_prx, d_ppred, d_st, d_st0, d_o, d_tow, d_tow_rx, d_copy):
                eng.free(p)
    finally:
        sys.stdout = tee.out
        tee.file.close()
        eng.close()


ALM_OUT = os.path.join(ROOT, "profiles", "r30_weighted_alm_bench.jsonl")
ALM_SHAPES = [(53248, 4), (256, 8), (256, 12), (4096, 8), (4096, 12), (16384, 8), (16384, 12)]


def weighted_alm(shapes, out=ALM_OUT, n_blocks=4000):
    """k_walm at (receivers, slots per receiver): every slot stands behind word 4 of a subframe and the launch's word records bring its
    words 5 .. 10 -- six records that count, the subframe completes.  Three loads: `none` (every slot assembles a subframe 2: nothing is
    offered to the bank), `per_rx` (slot 0 of every receiver completes an almanac page), `per_slot` (every slot completes the page of an
    SV of its own).  After the first launch the bank holds these very words, so a timed launch commits (SEEN) without writing an entry
    back: the steady state of a receiver that hears the same almanac from every satellite.  A device-to-device copy puts the slot states
    back before every timed launch; it is timed alone and subtracted, for k_weph on the same words and 192-byte states likewise.  The
    other yardstick: a device-to-device copy of half the bytes k_walm touches (read plus written); the calls take turns; the lines go to
    stdout and to `out`"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import weighted_alm_cases as A
    from stm32f4_sdr_gps_amd import capi
    hip = C.CDLL("libamdhip64.so")
    hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    tee = sys.stdout = _Tee(out)
    eng = capi.Engine(0, stream=stream.value)
    rng = np.random.default_rng(30)
    pages = np.array([A.random_almanac(rng, sv, toa=31) for sv in range(1, 25)], np.uint32)      # [24][8]
    other = np.array(rng.integers(0, 1 << 24, 8), np.uint32)
    word_slots, seen0 = capi.wnav_word_slots(n_blocks), 60000
    ecfg = np.zeros(1, capi.WEPH_CFG_DTYPE)
    try:
        for n_rx, ch in shapes:
            n_ch = n_rx * ch
            rx_of, slot_of = np.arange(n_ch) // ch, np.arange(n_ch) % ch
            first_end = 37 + (53 * np.arange(n_ch)) % 900                           # word 5 ends at this block of the launch
            cfg = capi.walm_cfg(ch)
            slot_bytes, est_bytes, bank_bytes = n_ch * 64, n_ch * 192, n_rx * 1120
            rx_bytes, alm_bytes, words_bytes = n_rx * 160, n_rx * 32 * 96, word_slots * n_ch * 16
            d_words, d_slots, d_slots0, d_est, d_est0, d_bank = (eng.malloc(b) for b in (words_bytes, slot_bytes, slot_bytes, est_bytes, est_bytes, bank_bytes))
            d_rx, d_alm, d_eph = eng.malloc(rx_bytes), eng.malloc(alm_bytes), eng.malloc(n_ch * 256)
            for mode in ("none", "per_rx", "per_slot"):
                paged = {"none": np.zeros(n_ch, bool), "per_rx": slot_of == 0, "per_slot": np.ones(n_ch, bool)}[mode]
                sv = (rx_of + slot_of) % 24
                w8 = np.where(paged[:, None], pages[sv], other[None, :])             # [n_ch][8]: words 3 .. 10 of every slot's subframe
                slots = np.zeros(n_ch, capi.WALM_SLOT_DTYPE)
                slots["blocks_seen"], slots["last_word_end_p1"] = seen0, seen0 + first_end + 1 - 600
                slots["cur"][:, :2], slots["cur_mask"], slots["cur_next"], slots["cur_id"] = w8[:, :2], 0xF, 5, np.where(paged, 5, 2)
                est = np.zeros(n_ch, capi.WEPH_STATE_DTYPE)
                for k in ("blocks_seen", "last_word_end_p1", "cur", "cur_mask", "cur_next", "cur_id"):
                    est[k] = slots[k]
                est["cur_tow"] = 1000
                words = np.zeros((word_slots, n_ch), capi.WNAV_WORD_DTYPE)
                words["end_block"] = -1
                for k in range(6):
                    words["end_block"][k], words["word"][k], words["index"][k] = first_end + 600 * k, w8[:, 2 + k] << 6, 5 + k
                    words["flags"][k], words["subframe_id"][k] = capi.WNAV_FLAG_WORD | capi.WNAV_FLAG_OK, np.where(paged, 5, 2)
                for d, a in ((d_words, words), (d_slots0, slots), (d_slots, slots), (d_est0, est), (d_est, est), (d_bank, np.zeros(n_rx, capi.WALM_BANK_DTYPE))):
                    eng.h2d(d, a)
                touched = words_bytes + 2 * slot_bytes + bank_bytes + rx_bytes + alm_bytes
                d_src, d_dst = eng.malloc(touched // 2), eng.malloc(touched // 2)

                def restore():
                    return hip.hipMemcpyAsync(d_slots, d_slots0, slot_bytes, 3, stream)

                def restore_eph():
                    return hip.hipMemcpyAsync(d_est, d_est0, est_bytes, 3, stream)

                def walm(with_alm):
                    return eng.lib.gpsx_walm_dev(eng.h, cfg.ctypes.data, C.c_void_p(d_words), n_blocks, n_rx, C.c_void_p(d_slots), C.c_void_p(d_bank),
                                                 C.c_void_p(d_rx), C.c_void_p(d_alm) if with_alm else None)

                def weph():
                    return eng.lib.gpsx_weph_dev(eng.h, ecfg.ctypes.data, C.c_void_p(d_words), n_blocks, C.c_void_p(d_est), n_ch, C.c_void_p(d_eph))
                eng._chk(walm(True), "gpsx_walm_dev")                                # the first launch fills the bank
                eng.synchronize()
                first = np.zeros(n_rx, capi.WALM_RX_DTYPE)
                eng.d2h(first, d_rx)
                calls = {"d2d_copy_of_the_slot_states": (1, restore),
                         "d2d_copy_of_the_eph_states": (1, restore_eph),
                         "d2d_copy_of_half_the_bytes_touched": (1, lambda: hip.hipMemcpyAsync(d_dst, d_src, touched // 2, 3, stream)),
                         "slot_copy_then_walm": (1, lambda: restore() or walm(True)),
                         "slot_copy_then_walm_no_alm": (1, lambda: restore() or walm(False)),
                         "state_copy_then_weph": (1, lambda: restore_eph() or weph())}
                extra = {"channels": n_ch, "n_rx": n_rx, "ch_per_rx": ch, "pages": mode, "n_blocks": n_blocks, "bytes_touched": touched}
                med = _timed_rows(eng, calls, extra, per_channel_ms=False)
                steady, bank = np.zeros(n_rx, capi.WALM_RX_DTYPE), np.zeros(n_rx, capi.WALM_BANK_DTYPE)
                eng.d2h(steady, d_rx)
                eng.d2h(bank, d_bank)
                print(json.dumps({"walm_check": "records of the first launch and after the timed ones", "n_rx": n_rx, "ch_per_rx": ch, "pages": mode,
                                  "stored_per_rx_first": [int(first["n_stored"].min()), int(first["n_stored"].max())], "new_first": int((first["new_mask"] != 0).sum()),
                                  "stored_per_rx_steady": [int(steady["n_stored"].min()), int(steady["n_stored"].max())], "new_steady": int((steady["new_mask"] != 0).sum()),
                                  "held_per_rx": [int(min(bin(int(m)).count("1") for m in bank["have_mask"])), int(max(bin(int(m)).count("1") for m in bank["have_mask"]))],
                                  "sync_code": int(eng.lib.gpsx_synchronize(eng.h))}), flush=True)
                own = med["slot_copy_then_walm"] - med["d2d_copy_of_the_slot_states"]
                own_no = med["slot_copy_then_walm_no_alm"] - med["d2d_copy_of_the_slot_states"]
                own_e = med["state_copy_then_weph"] - med["d2d_copy_of_the_eph_states"]
                print(json.dumps({"ratio": "k_walm (the timed pair less the slot copy) over the two yardsticks", "n_rx": n_rx, "ch_per_rx": ch, "pages": mode,
                                  "walm_us": round(own, 3), "walm_no_alm_us": round(own_no, 3), "weph_us": round(own_e, 3),
                                  "over_weph": round(own / own_e, 3), "no_alm_over_weph": round(own_no / own_e, 3),
                                  "over_d2d_copy_of_the_bytes_touched": round(own / med["d2d_copy_of_half_the_bytes_touched"], 3),
                                  "touched_GBps": round(touched / own / 1e3, 1), "ns_per_receiver": round(own / n_rx * 1e3, 2)}), flush=True)
                eng.free(d_src)
                eng.free(d_dst)
            for p in (d_words, d_slots, d_slots0, d_est, d_est0, d_bank, d_rx, d_alm, d_eph):
                eng.free(p)
    finally:
        sys.stdout = tee.out
        tee.file.close()
        eng.close()


WIN_OUT = os.path.join(ROOT, "profiles", "r31_weighted_win_bench.jsonl")
WIN_SHAPES = [(n_rx, n_coh, n_seg, w) for n_rx in (256, 4096) for n_coh, n_seg in ((10, 8), (20, 4)) for w in (128, 1024)]
WIN_PRNS, WIN_D = 12, 2


def weighted_win(shapes, out=WIN_OUT):
    """k_acq_win at (receivers, n_coh, n_seg, W) on WIN_PRNS PRNs per receiver, D = WIN_D: every prediction selected, its centre anywhere,
    its Doppler on the middle of a five-bin lattice (step 500 / n_coh Hz), so that the window call and the hybrid grid call search the
    same 2 D + 1 bins of the same receivers and PRNs on the same blocks.  Receiver r reads blocks r .. r + n_coh n_seg - 1 of one random
    stream (stride 1: every receiver's samples differ, the stream stays a few megabytes).  The two calls take turns; the lines go to
    stdout and to `out`.  From the counts: products per (receiver, PRN, bin, segment) -- the pre-sum's 16352 x n_coh weighted samples in
    two streams, the window's (2 W + 1) x 1023 x 2 chip products -- beside the kernel time"""
    from stm32f4_sdr_gps_amd import capi
    tee = sys.stdout = _Tee(out)
    eng = capi.Engine(0)
    prns = np.arange(1, WIN_PRNS + 1, dtype=np.uint8)
    n_dopp = 2 * WIN_D + 1
    try:
        for n_rx, n_coh, n_seg, w in shapes:
            span, step = n_coh * n_seg, max(1, 500 // n_coh)
            rng = np.random.default_rng(31)
            blocks = rng.integers(0, 256, (n_rx - 1 + span, 4092), dtype=np.uint8)
            pred = np.zeros((n_rx, WIN_PRNS), capi.WPRED_DTYPE)
            pred["flags"], pred["slot"] = capi.WPRED_HAVE_EPH | capi.WPRED_PREDICTED | capi.WPRED_VISIBLE, -1
            pred["code_phase"], pred["f_hz"] = rng.uniform(0.0, 16368.0, pred.shape), rng.uniform(-0.4 * step, 0.4 * step, pred.shape)
            cfg = capi.acq_window_cfg(n_coh, n_seg, w, WIN_D, min(32, w - 1))
            g = capi.AcqWeightedT(n_rx, 1, WIN_PRNS, prns.ctypes.data_as(C.POINTER(C.c_uint8)), -WIN_D * step, step, n_dopp, 1)
            n_peaks = n_rx * WIN_PRNS * n_dopp
            d_if, d_pred, d_pk, d_pk2, d_rep = (eng.malloc(b) for b in (blocks.nbytes + 2, pred.nbytes, n_peaks * 16, n_peaks * 16, n_rx * WIN_PRNS * 16))
            eng.h2d(d_if, blocks)
            eng.h2d(d_pred, pred)

            def win():
                return eng.lib.gpsx_acq_window_weighted_dev(eng.h, C.addressof(g), cfg.ctypes.data, C.c_void_p(d_pred), C.c_void_p(d_if), len(blocks),
                                                            C.c_void_p(d_pk), C.c_void_p(d_rep))

            def grid():
                return eng.lib.gpsx_acq_grid_weighted_hyb_dev(eng.h, C.addressof(g), n_coh, n_seg, C.c_void_p(d_if), len(blocks), C.c_void_p(d_pk2))
            eng._chk(grid(), "gpsx_acq_grid_weighted_hyb_dev")
            grid_kernel = eng.lib.gpsx_last_kernel(eng.h).decode()
            eng._chk(win(), "gpsx_acq_window_weighted_dev")
            eng.synchronize()
            rep, pk, pk2 = np.zeros((n_rx, WIN_PRNS), capi.ACQ_WINDOW_REP_DTYPE), np.zeros(n_peaks, capi.PEAK_DTYPE), np.zeros(n_peaks, capi.PEAK_DTYPE)
            eng.d2h(rep, d_rep)
            eng.d2h(pk, d_pk)
            eng.d2h(pk2, d_pk2)
            extra = {"channels": n_rx * WIN_PRNS, "n_rx": n_rx, "n_prn": WIN_PRNS, "n_coh": n_coh, "n_seg": n_seg, "half_width": w, "half_bins": WIN_D,
                     "n_dopp": n_dopp, "dopp_step_hz": step, "grid_kernel": grid_kernel}
            med = _timed_rows(eng, {"window": (1, win), "grid_restricted_to_the_bins": (1, grid)}, extra, per_channel_ms=False)
            units = n_rx * WIN_PRNS * n_dopp * n_seg
            print(json.dumps({"ratio": "k_acq_win over the hybrid grid restricted to the same bins", **extra, "window_us": round(med["window"], 1),
                              "grid_us": round(med["grid_restricted_to_the_bins"], 1), "window_over_grid": round(med["window"] / med["grid_restricted_to_the_bins"], 4),
                              "searched": int((rep["flags"] == capi.ACQ_WINDOW_SEARCHED).sum()), "bins_searched": int(rep["n_bins"].sum()),
                              "same_record_where_the_grids_phase_is_in_the_window": int(((pk["max_val"] == pk2["max_val"]) & (pk["phase"] == pk2["phase"])).sum()),
                              "presum_samples_per_us": round(units * 2 * 16352 * n_coh / med["window"], 1),
                              "chip_products_per_us": round(units * (2 * w + 1) * 1023 * 2 / med["window"], 1),
                              "ns_per_unit_segment": round(med["window"] / units * 1e3, 2), "sync_code": int(eng.lib.gpsx_synchronize(eng.h))}), flush=True)
            for p_ in (d_if, d_pred, d_pk, d_pk2, d_rep):
                eng.free(p_)
    finally:
        sys.stdout = tee.out
        tee.file.close()
        eng.close()


SNAP_OUT = os.path.join(ROOT, "profiles", "r32_weighted_snap_bench.jsonl")
SNAP_SHAPES = [(256, 12), (256, 32), (4096, 12), (4096, 32), (16384, 12), (16384, 32)]
SNAP_BINS = 21


def weighted_snap(shapes, out=SNAP_OUT):
    """k_wsnap at (receivers, PRNs) x 21 bins: sixteen receivers (the four sites under skies of twelve satellites, the prior up to 30 km
    and 20 s off, whole-sample phases from the restatement's model; tests/weighted_snap_cases.py) tiled over the launch, every one a
    FIX in four or five passes.  The yardsticks, taking turns with it: a device-to-device copy of the records it reads (peaks, bank,
    priors), and k_wfix on as many rows (the same skies' twelve satellites per receiver as observables).  Behind them, timed on the
    host clock: the parent's only way to the same answer -- the records copied back and the CPU restatement run on them (the
    restatement on at most 256 receivers, scaled).  The lines go to stdout and to `out`"""
    import time
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import weighted_fix_cases as W
    import weighted_snap_cases as K
    import weighted_snap_ref as S
    from stm32f4_sdr_gps_amd import capi
    hip = C.CDLL("libamdhip64.so")
    hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    tee = sys.stdout = _Tee(out)
    eng = capi.Engine(0, stream=stream.value)
    names = sorted(W.SITES)
    try:
        for n_rx, n_prn in shapes:
            rng = np.random.default_rng(n_prn)
            pool = []
            for k in range(16):
                site = names[k % len(names)]
                bank = np.zeros(n_prn, S.EPH_DTYPE)
                for (raw, _), p in zip(W.sky(site, 12, 3 * k), rng.permutation(n_prn)[:12]):
                    bank[p] = W.eph_record(raw)[0]
                rr = np.asarray(W.site_ecef(site), np.float64)
                d = rng.normal(0.0, 1.0, 3)
                pool.append((K.receiver(bank, rr, W.TOW, rr + d / np.linalg.norm(d) * float(rng.uniform(0.0, 30000.0)), W.TOW + float(rng.uniform(-20.0, 20.0)),
                                        seed=k, n_dopp=SNAP_BINS), W.receiver(site, 12, 3 * k)))
            peaks = np.stack([pool[r % 16][0]["peaks"] for r in range(n_rx)])
            bank = np.stack([pool[r % 16][0]["bank"] for r in range(n_rx)])
            prior = np.array([pool[r % 16][0]["prior"] for r in range(n_rx)], S.PRIOR_DTYPE)
            obs, eph = W.pack([pool[r % 16][1] for r in range(n_rx)], 12)
            prns = np.arange(1, n_prn + 1, dtype=np.uint8)
            cfg, fix_cfg = capi.wsnap_cfg(K.EPOCH_S), capi.wfix_cfg(W.OFFSET_MS, 12)
            read_bytes = peaks.nbytes + bank.nbytes + prior.nbytes
            d_peaks, d_bank, d_prior, d_copy = (eng.malloc(b) for b in (peaks.nbytes, bank.nbytes, prior.nbytes, read_bytes))
            d_snap, d_sv, d_obs, d_eph, d_fix = (eng.malloc(b) for b in (n_rx * 128, n_rx * n_prn * 48, obs.nbytes, eph.nbytes, n_rx * 128))
            for d, a in ((d_peaks, peaks), (d_bank, bank), (d_prior, prior), (d_obs, obs), (d_eph, eph)):
                eng.h2d(d, a)
            g = capi.AcqWeightedT(n_rx, 0, n_prn, prns.ctypes.data_as(C.POINTER(C.c_uint8)), K.DOPP_MIN_HZ, K.DOPP_STEP_HZ, SNAP_BINS, 1)

            def wsnap(want_sv):
                return eng.lib.gpsx_wsnap_dev(eng.h, cfg.ctypes.data, C.addressof(g), C.c_void_p(d_peaks), C.c_void_p(d_bank), n_prn, C.c_void_p(d_prior),
                                              C.c_void_p(d_snap), C.c_void_p(d_sv) if want_sv else None)

            def copy():
                return (hip.hipMemcpyAsync(d_copy, d_peaks, peaks.nbytes, 3, stream) or hip.hipMemcpyAsync(d_copy + peaks.nbytes, d_bank, bank.nbytes, 3, stream) or
                        hip.hipMemcpyAsync(d_copy + peaks.nbytes + bank.nbytes, d_prior, prior.nbytes, 3, stream))

            calls = {"d2d_copy_of_the_records_read": (1, copy),
                     "wfix_on_as_many_rows": (1, lambda: eng.lib.gpsx_wfix_dev(eng.h, fix_cfg.ctypes.data, C.c_void_p(d_obs), C.c_void_p(d_eph), None, None, n_rx,
                                                                               C.c_void_p(d_fix), None)),
                     "wsnap": (1, lambda: wsnap(True)),
                     "wsnap_without_d_sv": (1, lambda: wsnap(False))}
            med = _timed_rows(eng, calls, {"channels": n_rx * 12, "n_rx": n_rx, "n_prn": n_prn, "n_dopp": SNAP_BINS, "read_bytes": read_bytes}, per_channel_ms=False)
            snap = np.zeros(n_rx, capi.WSNAP_DTYPE)
            eng.d2h(snap, d_snap)
            back = np.empty_like(peaks)
            d2h = []
            for _ in range(5):
                t0 = time.perf_counter()
                eng.d2h(back, d_peaks)
                d2h.append((time.perf_counter() - t0) * 1e6)
            n_host = min(n_rx, 256)
            t0 = time.perf_counter()
            want, _ = S.snap(cfg, prns, K.DOPP_MIN_HZ, K.DOPP_STEP_HZ, back[:n_host], bank[:n_host], n_prn, prior[:n_host], want_sv=False)
            host_us = (time.perf_counter() - t0) * 1e6 * n_rx / n_host
            err = np.array([np.linalg.norm(snap["rr"][r] - pool[r % 16][0]["rr"]) for r in range(min(n_rx, 16))])
            print(json.dumps({"wsnap_check": "records after the timed launches", "n_rx": n_rx, "fix": int((snap["flags"] == capi.WSNAP_FIX).sum()),
                              "n_iter": [int(snap["n_iter"].min()), int(snap["n_iter"].max())], "n_used": [int(snap["n_used"].min()), int(snap["n_used"].max())],
                              "largest_error_m": round(float(err.max()), 2), "flags_equal_the_restatement": bool((want["flags"] == snap["flags"][:n_host]).all())}), flush=True)
            own = med["wsnap"]
            print(json.dumps({"ratio": "k_wsnap over the yardsticks", "n_rx": n_rx, "n_prn": n_prn, "n_dopp": SNAP_BINS, "wsnap_us": round(own, 3),
                              "wsnap_without_d_sv_us": round(med["wsnap_without_d_sv"], 3), "wfix_us": round(med["wfix_on_as_many_rows"], 3),
                              "over_d2d_copy_of_the_records_read": round(own / med["d2d_copy_of_the_records_read"], 3),
                              "over_wfix": round(own / med["wfix_on_as_many_rows"], 3), "ns_per_receiver": round(own / n_rx * 1e3, 2),
                              "host_path_d2h_us_median": round(float(np.median(d2h)), 1), "host_path_restatement_us": round(host_us, 1),
                              "host_path_restatement_receivers_timed": n_host, "host_path_over_wsnap": round((float(np.median(d2h)) + host_us) / own, 1)}), flush=True)
            for d in (d_peaks, d_bank, d_prior, d_copy, d_snap, d_sv, d_obs, d_eph, d_fix):
                eng.free(d)
    finally:
        sys.stdout = tee.out
        tee.file.close()
        eng.close()


def main():
    global WINDOW_S
    if "--weighted-snap" in sys.argv[1:]:
        args = [a for a in sys.argv[1:] if a != "--weighted-snap"]
        if "--window-s" in args:
            at = args.index("--window-s")
            WINDOW_S = float(args.pop(at + 1))
            args.pop(at)
        return weighted_snap([tuple(int(v) for v in a.split("x")) for a in args] or SNAP_SHAPES)
    if "--weighted-win" in sys.argv[1:]:
        args = [a for a in sys.argv[1:] if a != "--weighted-win"]
        if "--window-s" in args:
            at = args.index("--window-s")
            WINDOW_S = float(args.pop(at + 1))
            args.pop(at)
        return weighted_win([tuple(int(v) for v in a.split("x")) for a in args] or WIN_SHAPES)
    if "--weighted-alm" in sys.argv[1:]:
        args = [a for a in sys.argv[1:] if a != "--weighted-alm"]
        if "--window-s" in args:
            at = args.index("--window-s")
            WINDOW_S = float(args.pop(at + 1))
            args.pop(at)
        return weighted_alm([tuple(int(v) for v in a.split("x")) for a in args] or ALM_SHAPES)
    if "--weighted-tow" in sys.argv[1:]:
        args = [a for a in sys.argv[1:] if a != "--weighted-tow"]
        if "--window-s" in args:
            at = args.index("--window-s")
            WINDOW_S = float(args.pop(at + 1))
            args.pop(at)
        return weighted_tow([tuple(int(v) for v in a.split("x")) for a in args] or BANK_SHAPES)
    if "--weighted-bank" in sys.argv[1:]:
        args = [a for a in sys.argv[1:] if a != "--weighted-bank"]
        if "--window-s" in args:
            at = args.index("--window-s")
            WINDOW_S = float(args.pop(at + 1))
            args.pop(at)
        return weighted_bank([tuple(int(v) for v in a.split("x")) for a in args] or BANK_SHAPES)
    if "--weighted-acq" in sys.argv[1:]:
        args = [a for a in sys.argv[1:] if a != "--weighted-acq"]
        if "--window-s" in args:
            at = args.index("--window-s")
            WINDOW_S = float(args.pop(at + 1))
            args.pop(at)
        return weighted_acq([tuple(int(v) for v in a.split("x")) for a in args] or ACQ_SHAPES)
    if "--weighted-kf" in sys.argv[1:]:
        args = [a for a in sys.argv[1:] if a != "--weighted-kf"]
        if "--window-s" in args:
            at = args.index("--window-s")
            WINDOW_S = float(args.pop(at + 1))
            args.pop(at)
        return weighted_kf([tuple(int(v) for v in a.split("x")) for a in args] or FIX_SHAPES)
    if "--weighted-vel" in sys.argv[1:]:
        args = [a for a in sys.argv[1:] if a != "--weighted-vel"]
        if "--window-s" in args:
            at = args.index("--window-s")
            WINDOW_S = float(args.pop(at + 1))
            args.pop(at)
        return weighted_vel([tuple(int(v) for v in a.split("x")) for a in args] or FIX_SHAPES)
    if "--weighted-fde" in sys.argv[1:]:
        args = [a for a in sys.argv[1:] if a != "--weighted-fde"]
        if "--window-s" in args:
            at = args.index("--window-s")
            WINDOW_S = float(args.pop(at + 1))
            args.pop(at)
        return weighted_fde([tuple(int(v) for v in a.split("x")) for a in args] or FIX_SHAPES)
    if "--weighted-fix" in sys.argv[1:]:
        args = [a for a in sys.argv[1:] if a != "--weighted-fix"]
        if "--window-s" in args:
            at = args.index("--window-s")
            WINDOW_S = float(args.pop(at + 1))
            args.pop(at)
        return weighted_fix([tuple(int(v) for v in a.split("x")) for a in args] or FIX_SHAPES)
    if "--weighted-lock" in sys.argv[1:]:
        args = [a for a in sys.argv[1:] if a != "--weighted-lock"]
        if "--window-s" in args:
            at = args.index("--window-s")
            WINDOW_S = float(args.pop(at + 1))
            args.pop(at)
        return weighted_lock([int(a) for a in args] or [65536, 212992])
    if "--weighted-multi" in sys.argv[1:]:
        args = [a for a in sys.argv[1:] if a != "--weighted-multi"]
        if "--window-s" in args:
            at = args.index("--window-s")
            WINDOW_S = float(args.pop(at + 1))
            args.pop(at)
        parent_rows = None
        if "--parent-rows" in args:
            at = args.index("--parent-rows")
            parent_rows = args.pop(at + 1)
            args.pop(at)
        single_only = "--single-only" in args
        shapes = [tuple(int(v) for v in a.split("x")) for a in args if a != "--single-only"]
        return weighted_multi(shapes or MULTI_SHAPES, single_only=single_only, parent_rows=parent_rows)
    if "--weighted-eph" in sys.argv[1:]:
        args = [a for a in sys.argv[1:] if a != "--weighted-eph"]
        if "--window-s" in args:
            at = args.index("--window-s")
            WINDOW_S = float(args.pop(at + 1))
            args.pop(at)
        return weighted_eph([int(a) for a in args] or [65536, 212992])
    if "--weighted-obs" in sys.argv[1:]:
        args = [a for a in sys.argv[1:] if a != "--weighted-obs"]
        if "--window-s" in args:
            at = args.index("--window-s")
            WINDOW_S = float(args.pop(at + 1))
            args.pop(at)
        return weighted_obs([int(a) for a in args] or [65536, 212992])
    from stm32f4_sdr_gps_amd import capi, synth
    if "--weighted-nav" in sys.argv[1:]:
        args = [a for a in sys.argv[1:] if a != "--weighted-nav"]
        if "--window-s" in args:
            at = args.index("--window-s")
            WINDOW_S = float(args.pop(at + 1))
            args.pop(at)
        return weighted_nav([int(a) for a in args] or [65536, 212992])
    if "--weighted-sync" in sys.argv[1:]:
        args = [a for a in sys.argv[1:] if a != "--weighted-sync"]
        if "--window-s" in args:
            at = args.index("--window-s")
            WINDOW_S = float(args.pop(at + 1))
            args.pop(at)
        return weighted_sync([int(a) for a in args] or [65536, 212992])
    if "--weighted-loop" in sys.argv[1:]:
        args = sys.argv[1:]
        at = args.index("--weighted-loop")
        n_coh = int(args.pop(at + 1)) if at + 1 < len(args) and args[at + 1].isdigit() and int(args[at + 1]) <= 20 else 20
        args.pop(at)
        if "--window-s" in args:
            at = args.index("--window-s")
            WINDOW_S = float(args.pop(at + 1))
            args.pop(at)
        return weighted_loop(n_coh, [int(a) for a in args] or [65536, 212992])
    if "--weighted" in sys.argv[1:]:
        args = sys.argv[1:]
        at = args.index("--weighted")
        k = int(args.pop(at + 1)) if at + 1 < len(args) and args[at + 1].isdigit() else 1
        args.pop(at)
        if "--window-s" in args:   # (a profiler run wants short windows)
            at = args.index("--window-s")
            WINDOW_S = float(args.pop(at + 1))
            args.pop(at)
        return weighted(k, [int(a) for a in args] or [65536, 212992])
    eng = capi.Engine(0)
    blk = synth.default_four_sv(1, seed=7)[0]
    d_if = eng.malloc(2048)
    eng.h2d(d_if, np.concatenate([blk, np.zeros(2, np.uint8)]))
    rows = []
    for n in [int(a) for a in sys.argv[1:]] or [256, 4096, 65536, 212992]:
        st = np.zeros(n, capi.TRK_DTYPE)
        st["prn"] = (np.arange(n) % 32) + 1
        st["code_phase_fine"] = (61 * np.arange(n) % 16368).astype(np.float32)
        st["if_freq_offset_hz"] = (-5000 + 39 * (np.arange(n) % 256)).astype(np.float32)
        d_st, d_iq = eng.malloc(st.nbytes), eng.malloc(n * 12)
        eng.h2d(d_st, st)
        for _ in range(5):
            eng._chk(eng.lib.gpsx_track_epl_batch_dev(eng.h, C.c_void_p(d_if), C.c_void_p(d_st), n, C.c_void_p(d_iq)), "trk")
        e0, e1 = eng.event(), eng.event()
        reps = 50
        eng.record(e0)
        for _ in range(reps):
            eng.lib.gpsx_track_epl_batch_dev(eng.h, C.c_void_p(d_if), C.c_void_p(d_st), n, C.c_void_p(d_iq))
        eng.record(e1)
        eng.synchronize()
        rows.append({"channels": n, "kernel_us": eng.elapsed_ms(e0, e1) / reps * 1e3})
        eng.free(d_st)
        eng.free(d_iq)
    print(json.dumps({"kernel": "gpsx::k_track_epl", "rows": rows}))


if __name__ == "__main__":
    main()
