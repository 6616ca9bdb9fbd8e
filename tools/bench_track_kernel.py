#!/usr/bin/env python3
"""k_track_epl alone (device-resident block, states and accumulators; HIP events on the engine's stream): what part of
the per-millisecond tracking step is the kernel and what part the PCIe round trip.

  bench_track_kernel.py [channels ...]                the sign-plane step, 50 launches per count (one JSON line)
  bench_track_kernel.py --weighted [K] [channels ...] gpsx_track_epl_weighted_dev (EXTENSION: both bits, K blocks per launch, K = 1
                                                      and the K given) beside gpsx_track_epl_batch_dev: the calls take turns in one
                                                      process, WINDOWS timed windows each, every window some tenths of a second
                                                      long (--window-s S: another length); median, minimum and maximum per launch (one JSON line per row)"""
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


def main():
    from stm32f4_sdr_gps_amd import capi, synth
    if "--weighted" in sys.argv[1:]:
        args = sys.argv[1:]
        at = args.index("--weighted")
        k = int(args.pop(at + 1)) if at + 1 < len(args) and args[at + 1].isdigit() else 1
        args.pop(at)
        if "--window-s" in args:   # (a profiler run wants short windows)
            global WINDOW_S
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
