#!/usr/bin/env python3
"""The weighted two-bit acquisition extension's kernels alone (device-resident captures, HIP events on the engine's stream):
searches x 32 PRN x 21 Doppler x 16368 phases per launch, first on the matrix cores (k_acq_mxw), then on the vector ALU
(k_acq_weighted), and the sign-only fine grid (k_acq_mx<0>) on the same captures' sign plane beside them.
--n-ms N: the multi-block call instead (gpsx_acq_grid_weighted_ms_dev: k_acq_wmx_ms / k_acq_weighted_ms), N blocks per search, on
both paths, beside N single-block calls on the same captures (block b of every search: the same hypothesis-blocks), in one process.
--coh N: the coherent call (gpsx_acq_grid_weighted_coh_dev: k_acq_coh_mx / k_acq_coh_vec), N blocks per search, on both paths,
alternating with the non-coherent call over the same N blocks (n_ms = N) on the same captures, in one process.
--hyb N S: the hybrid call (gpsx_acq_grid_weighted_hyb_dev: k_acq_hyb_mx / k_acq_hyb_vec), S coherent windows of N blocks per search,
on both paths (--matrix-only: that path alone), alternating with (a) the coherent call over the same windows as searches x S searches
of stride N -- what a caller without the hybrid call has to run, and still cannot add up -- and (b) the non-coherent call over the
same N x S blocks (at most its 128), in one process.
usage: bench_weighted_kernel.py [--n-ms N | --coh N | --hyb N S [--matrix-only]] [searches [reps]]"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from stm32f4_sdr_gps_amd import capi, synth
    argv = list(sys.argv[1:])
    n_ms = n_coh = 0
    if "--n-ms" in argv:
        at = argv.index("--n-ms")
        n_ms = int(argv[at + 1])
        del argv[at:at + 2]
    if "--coh" in argv:
        at = argv.index("--coh")
        n_coh = int(argv[at + 1])
        del argv[at:at + 2]
    hyb = None
    if "--hyb" in argv:
        at = argv.index("--hyb")
        hyb = (int(argv[at + 1]), int(argv[at + 2]))
        del argv[at:at + 3]
    matrix_only = "--matrix-only" in argv
    if matrix_only:
        argv.remove("--matrix-only")
    searches = int(argv[0]) if len(argv) > 0 else 16
    reps = int(argv[1]) if len(argv) > 1 else 5
    if os.environ.get("GPSX_LIB"):   # A/B runs against another build of the library (tools/build_variant.sh)
        capi.LIB_PATH = capi.LAB_LIB_PATH = os.environ["GPSX_LIB"]
    eng = capi.Engine(0, lab=bool(os.environ.get("GPSX_LIB")))
    blocks = synth.cold_start_block(searches, seed=11, amp_scale=0.25, two_bit=True)
    prns = np.arange(1, 33, dtype=np.uint8)
    g = capi.AcqWeightedT(searches, 1, 32, prns.ctypes.data_as(C.POINTER(C.c_uint8)), -5000, 500, 21, 1)
    d_if = eng.malloc(blocks.size + 2)
    eng.h2d(d_if, np.concatenate([blocks.reshape(-1), np.zeros(2, np.uint8)]))
    d_pk = eng.malloc(searches * 32 * 21 * 16)

    def run():
        rc = eng.lib.gpsx_acq_grid_weighted_dev(eng.h, C.byref(g), C.c_void_p(d_if), searches, C.c_void_p(d_pk))
        assert rc == 0, eng.lib.gpsx_last_error(eng.h)

    def timed(fn):
        for _ in range(2):
            fn()
        e0, e1 = eng.event(), eng.event()
        eng.record(e0)
        for _ in range(reps):
            fn()
        eng.record(e1)
        eng.synchronize()
        return eng.elapsed_ms(e0, e1) / reps
    hyp = searches * 32 * 21 * 16368
    if hyb:
        return hybrid(eng, capi, synth, searches, hyb[0], hyb[1], timed, matrix_only)
    if n_coh:
        return coherent(eng, capi, synth, searches, n_coh, reps, timed)
    if n_ms:
        return multi_block(eng, capi, synth, searches, n_ms, reps, timed)
    for path in (capi.ACQ_PATH_MATRIX, capi.ACQ_PATH_VECTOR):
        eng.set_acq_path(path)
        ms = timed(run)
        line = {"kernel": "gpsx::" + eng.lib.gpsx_last_kernel(eng.h).decode(), "searches": searches, "ms": round(ms, 3), "hyp_per_s": hyp / (ms * 1e-3)}
        if path == capi.ACQ_PATH_MATRIX:
            # per hypothesis 2 streams x 18 passes x 1024 chips x 2 (multiply, add) on MX-FP4 operands
            flops = hyp / 16 * 2 * 18 * 1024 * 2
            line.update({"mfma_tflops": flops / (ms * 1e-3) / 1e12, "frac_of_fp4_dense_peak": flops / (ms * 1e-3) / 10.0e15,
                         "note": "MFMA flops as issued (18 passes per 16 sample offsets) against the 10 PFLOP/s dense MX-FP4 peak"})
        else:
            dot4 = hyp * 2 * 256            # per hypothesis two streams x 256 four-chip steps
            line.update({"dot4_lane_ops_per_s": dot4 / (ms * 1e-3), "frac_of_valu_issue_peak": dot4 / (ms * 1e-3) / (256 * 64 * 2.4e9),
                         "note": "algorithmic v_dot4_i32_i8 lane-ops (512 per hypothesis) against one wave64 op per 4 cycles per SIMD at 2.4 GHz"})
        print(json.dumps(line))
    eng.set_acq_path(capi.ACQ_PATH_MATRIX)
    # the sign-only fine grid on the same captures (their sign plane): the reference-parity kernel this one is built from
    eng.set_if_format(capi.IF_2BIT_SM)
    gd = eng.grid_desc(prns, n_search=searches, dopp_min_hz=-5000, dopp_step_hz=500, n_dopp=21)
    d_keys = eng.malloc(searches * 32 * 21 * 8)
    d_pk8 = eng.malloc(searches * 32 * 21 * 8 * 16)

    def run_sign():
        rc = eng.lib.gpsx_acq_grid_dev(eng.h, C.byref(gd), C.c_void_p(d_if), searches, C.c_void_p(d_pk8), C.c_void_p(d_keys), None, None, None)
        assert rc == 0, eng.lib.gpsx_last_error(eng.h)
    ms = timed(run_sign)
    print(json.dumps({"kernel": "gpsx::" + eng.lib.gpsx_last_kernel(eng.h).decode(), "searches": searches, "ms": round(ms, 3), "hyp_per_s": hyp / (ms * 1e-3),
                      "note": "the sign-only fine grid, same shape"}))


def multi_block(eng, capi, synth, searches, n_ms, reps, timed):
    blocks = synth.cold_start_block(searches * n_ms, seed=11, amp_scale=0.25, two_bit=True)
    prns = np.arange(1, 33, dtype=np.uint8)
    g = capi.AcqWeightedT(searches, n_ms, 32, prns.ctypes.data_as(C.POINTER(C.c_uint8)), -5000, 500, 21, 1)
    d_if = eng.malloc(blocks.size + 2)
    eng.h2d(d_if, np.concatenate([blocks.reshape(-1), np.zeros(2, np.uint8)]))
    d_pk = eng.malloc(searches * 32 * 21 * 16)
    n_blocks = searches * n_ms

    def run_ms():
        rc = eng.lib.gpsx_acq_grid_weighted_ms_dev(eng.h, C.byref(g), n_ms, C.c_void_p(d_if), n_blocks, C.c_void_p(d_pk))
        assert rc == 0, eng.lib.gpsx_last_error(eng.h)

    def run_sweeps():   # block b of every search: the single-block call from byte offset b x 4092, stride n_ms
        for b in range(n_ms):
            rc = eng.lib.gpsx_acq_grid_weighted_dev(eng.h, C.byref(g), C.c_void_p(d_if + b * capi.BYTES_PER_MS_2BIT), n_blocks - b,
                                                    C.c_void_p(d_pk))
            assert rc == 0, eng.lib.gpsx_last_error(eng.h)
    hyp_blocks = searches * 32 * 21 * 16368 * n_ms
    for path in (capi.ACQ_PATH_MATRIX, capi.ACQ_PATH_VECTOR):
        eng.set_acq_path(path)
        ms_sweeps = timed(run_sweeps)
        k_one = eng.lib.gpsx_last_kernel(eng.h).decode()
        ms_multi = timed(run_ms)
        k_ms = eng.lib.gpsx_last_kernel(eng.h).decode()
        line = {"kernel": "gpsx::" + k_ms, "searches": searches, "n_ms": n_ms, "ms": round(ms_multi, 3),
                "hyp_blocks_per_s": hyp_blocks / (ms_multi * 1e-3), "sweeps_kernel": "gpsx::" + k_one, "sweeps_ms": round(ms_sweeps, 3),
                "sweeps_hyp_blocks_per_s": hyp_blocks / (ms_sweeps * 1e-3), "ratio": round(ms_multi / ms_sweeps, 3)}
        if path == capi.ACQ_PATH_MATRIX:
            # running sums: u32 read and written per hypothesis-block but for the first (no read) and last (no write) block
            scratch = searches * 32 * 21 * 16384 * 4 * 2 * (n_ms - 1)
            line.update({"scratch_bytes": scratch, "scratch_bytes_per_hyp_block": scratch / hyp_blocks,
                         "scratch_tb_per_s": scratch / (ms_multi * 1e-3) / 1e12})
        print(json.dumps(line))
    eng.set_acq_path(capi.ACQ_PATH_MATRIX)


def coherent(eng, capi, synth, searches, n_coh, reps, timed, rounds=3):
    blocks = synth.cold_start_block(searches * n_coh, seed=11, amp_scale=0.25, two_bit=True)
    prns = np.arange(1, 33, dtype=np.uint8)
    g = capi.AcqWeightedT(searches, n_coh, 32, prns.ctypes.data_as(C.POINTER(C.c_uint8)), -5000, 500, 21, 1)
    d_if = eng.malloc(blocks.size + 2)
    eng.h2d(d_if, np.concatenate([blocks.reshape(-1), np.zeros(2, np.uint8)]))
    d_pk = eng.malloc(searches * 32 * 21 * 16)
    n_blocks = searches * n_coh

    def run_coh():
        rc = eng.lib.gpsx_acq_grid_weighted_coh_dev(eng.h, C.byref(g), n_coh, C.c_void_p(d_if), n_blocks, C.c_void_p(d_pk))
        assert rc == 0, eng.lib.gpsx_last_error(eng.h)

    def run_ms():
        rc = eng.lib.gpsx_acq_grid_weighted_ms_dev(eng.h, C.byref(g), n_coh, C.c_void_p(d_if), n_blocks, C.c_void_p(d_pk))
        assert rc == 0, eng.lib.gpsx_last_error(eng.h)
    hyp = searches * 32 * 21 * 16368
    for path in (capi.ACQ_PATH_MATRIX, capi.ACQ_PATH_VECTOR):
        eng.set_acq_path(path)
        t_coh, t_ms = [], []
        for _ in range(rounds):        # alternating: the two calls see the same clocks
            t_coh.append(timed(run_coh))
            k_coh = eng.lib.gpsx_last_kernel(eng.h).decode()
            t_ms.append(timed(run_ms))
            k_ms = eng.lib.gpsx_last_kernel(eng.h).decode()
        ms_coh, ms_nc = float(np.median(t_coh)), float(np.median(t_ms))
        line = {"kernel": "gpsx::" + k_coh, "searches": searches, "n_coh": n_coh, "ms": round(ms_coh, 3), "hyp_per_s": hyp / (ms_coh * 1e-3),
                "noncoherent_kernel": "gpsx::" + k_ms, "noncoherent_ms": round(ms_nc, 3), "ratio": round(ms_coh / ms_nc, 3),
                "ms_runs": [round(t, 3) for t in t_coh], "noncoherent_ms_runs": [round(t, 3) for t in t_ms]}
        if k_coh == "k_acq_coh_mx":
            # per hypothesis 2 streams x 17 passes x 1024 chips x 2 (multiply, add) on int8 operands, against ~5 x 10^15 dense I8
            ops = hyp / 16 * 2 * 17 * 1024 * 2
            line.update({"mfma_tops": ops / (ms_coh * 1e-3) / 1e12, "frac_of_i8_dense_peak": ops / (ms_coh * 1e-3) / 5.0e15,
                         "note": "MFMA int8 ops as issued (17 passes per 16 sample offsets) against the ~5 POP/s dense I8 peak (2x BF16)"})
        elif k_coh == "k_acq_coh_vec":
            dot2 = hyp * 2 * 512            # per hypothesis two streams x 512 two-chip steps
            line.update({"dot2_lane_ops_per_s": dot2 / (ms_coh * 1e-3), "frac_of_valu_issue_peak": dot2 / (ms_coh * 1e-3) / (256 * 64 * 2.4e9),
                         "note": "algorithmic v_dot2_i32_i16 lane-ops (1024 per hypothesis) against one wave64 op per 4 cycles per SIMD at 2.4 GHz"})
        print(json.dumps(line), flush=True)
    eng.set_acq_path(capi.ACQ_PATH_MATRIX)


def hybrid(eng, capi, synth, searches, n_coh, n_seg, timed, matrix_only, rounds=3):
    span = n_coh * n_seg
    n_blocks = searches * span
    blocks = synth.cold_start_block(n_blocks, seed=11, amp_scale=0.25, two_bit=True)
    prns = np.arange(1, 33, dtype=np.uint8)
    p_prns = prns.ctypes.data_as(C.POINTER(C.c_uint8))
    g = capi.AcqWeightedT(searches, span, 32, p_prns, -5000, 500, 21, 1)
    g_win = capi.AcqWeightedT(searches * n_seg, n_coh, 32, p_prns, -5000, 500, 21, 1)    # every window a search of its own
    n_ms = min(span, 128)
    d_if = eng.malloc(blocks.size + 2)
    eng.h2d(d_if, np.concatenate([blocks.reshape(-1), np.zeros(2, np.uint8)]))
    d_pk = eng.malloc(searches * n_seg * 32 * 21 * 16)

    def run_hyb():
        rc = eng.lib.gpsx_acq_grid_weighted_hyb_dev(eng.h, C.byref(g), n_coh, n_seg, C.c_void_p(d_if), n_blocks, C.c_void_p(d_pk))
        assert rc == 0, eng.lib.gpsx_last_error(eng.h)

    def run_windows():
        rc = eng.lib.gpsx_acq_grid_weighted_coh_dev(eng.h, C.byref(g_win), n_coh, C.c_void_p(d_if), n_blocks, C.c_void_p(d_pk))
        assert rc == 0, eng.lib.gpsx_last_error(eng.h)

    def run_ms():
        rc = eng.lib.gpsx_acq_grid_weighted_ms_dev(eng.h, C.byref(g), n_ms, C.c_void_p(d_if), n_blocks, C.c_void_p(d_pk))
        assert rc == 0, eng.lib.gpsx_last_error(eng.h)
    hyp_win = searches * n_seg * 32 * 21 * 16368          # hypotheses x windows
    for path in (capi.ACQ_PATH_MATRIX,) if matrix_only else (capi.ACQ_PATH_MATRIX, capi.ACQ_PATH_VECTOR):
        eng.set_acq_path(path)
        t_hyb, t_win, t_ms = [], [], []
        for _ in range(rounds):        # alternating: the three calls see the same clocks
            t_hyb.append(timed(run_hyb))
            k_hyb = eng.lib.gpsx_last_kernel(eng.h).decode()
            t_win.append(timed(run_windows))
            k_win = eng.lib.gpsx_last_kernel(eng.h).decode()
            t_ms.append(timed(run_ms))
            k_ms = eng.lib.gpsx_last_kernel(eng.h).decode()
        ms_hyb, ms_win, ms_nc = float(np.median(t_hyb)), float(np.median(t_win)), float(np.median(t_ms))
        line = {"kernel": "gpsx::" + k_hyb, "searches": searches, "n_coh": n_coh, "n_seg": n_seg, "ms": round(ms_hyb, 3),
                "hyp_windows_per_s": hyp_win / (ms_hyb * 1e-3),
                "windows_kernel": "gpsx::" + k_win, "windows_searches": searches * n_seg, "windows_ms": round(ms_win, 3),
                "ratio_to_windows": round(ms_hyb / ms_win, 3),
                "noncoherent_kernel": "gpsx::" + k_ms, "noncoherent_n_ms": n_ms, "noncoherent_ms": round(ms_nc, 3),
                "ratio_to_noncoherent": round(ms_hyb / ms_nc, 3), "ms_runs": [round(t, 3) for t in t_hyb],
                "windows_ms_runs": [round(t, 3) for t in t_win], "noncoherent_ms_runs": [round(t, 3) for t in t_ms]}
        if k_hyb == "k_acq_hyb_mx":
            # per hypothesis and window 2 streams x 17 passes x 1024 chips x 2 (multiply, add) on int8 operands; running sums: 2 MB
            # per cluster, read by every window but the first and written by every window but the last
            ops = hyp_win / 16 * 2 * 17 * 1024 * 2
            scratch = searches * 21 * (2 << 20) * 2 * (n_seg - 1)
            line.update({"mfma_tops": ops / (ms_hyb * 1e-3) / 1e12, "frac_of_i8_dense_peak": ops / (ms_hyb * 1e-3) / 5.0e15,
                         "scratch_bytes": scratch, "scratch_gb_per_s": scratch / (ms_hyb * 1e-3) / 1e9,
                         "note": "MFMA int8 ops as issued (17 passes per 16 sample offsets and window) against the ~5 POP/s dense I8 "
                                 "peak (2x BF16); scratch: the u32 running sums' reads and writes over the call's time"})
        elif k_hyb == "k_acq_hyb_vec":
            dot2 = hyp_win * 2 * 512            # per hypothesis and window two streams x 512 two-chip steps
            line.update({"dot2_lane_ops_per_s": dot2 / (ms_hyb * 1e-3), "frac_of_valu_issue_peak": dot2 / (ms_hyb * 1e-3) / (256 * 64 * 2.4e9),
                         "note": "algorithmic v_dot2_i32_i16 lane-ops (1024 per hypothesis and window) against one wave64 op per 4 cycles "
                                 "per SIMD at 2.4 GHz"})
        print(json.dumps(line), flush=True)
    eng.set_acq_path(capi.ACQ_PATH_MATRIX)


if __name__ == "__main__":
    main()
