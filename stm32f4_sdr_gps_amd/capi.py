"""ctypes binding of the C ABI in include/gpsx.h / include/gpsx_compat.h (libgpsx.so).

Used by tests/ and bench.py.  It adds nothing to the computation: arrays in, arrays out, every call forwarded to the
shared library, which runs on the GPU or fails.  If the library has not been built, or there is no gfx950 device,
construction raises -- there is no Python/CPU fallback.

Import torch BEFORE this module in processes that use both (one HIP runtime per process: torch's bundled
libamdhip64 and /opt/rocm's share a SONAME, whichever loads first serves both).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG, "lib", "libgpsx.so")
LAB_LIB_PATH = os.path.join(PKG, "lib", "libgpsx_lab.so")

BYTES_PER_MS = 2046
BYTES_PER_MS_2BIT = 4092
IF_1BIT, IF_2BIT_SM = 0, 1
PHASES_BYTE = 2046
PHASES_FINE = 16368
IF_HZ = 4092000
SCHED_EVERY_MS, SCHED_MUX17 = 0, 1
WORDSYNC_DEVICE, WORDSYNC_HOST = 0, 1
DRAWS_XORSHIFT, DRAWS_LIBC = 0, 1
ACQ_PATH_MATRIX, ACQ_PATH_VECTOR = 0, 1

LOOP_DTYPE = np.dtype([("prn", "<i4"), ("code_phase_fine", "<f4"), ("if_freq_offset_hz", "<f4"), ("if_freq_accum", "<u4"),
                       ("dll_code_err", "<f4"), ("pll_code_err", "<f4"), ("fll_err", "<f4"), ("fll_old_i", "<i2"),
                       ("fll_old_q", "<i2"), ("pll_check_buf", "<i2", 4), ("pll_bad_state_master_cnt", "<u2"),
                       ("pll_bad_state_cnt", "u1"), ("period_sync_ok_flag", "u1"), ("found_freq_offset_hz", "<i2"),
                       ("reseed_count", "<u2"), ("rng", "<u4"), ("i_part_summ", "<u4"), ("q_part_summ", "<u4"),
                       ("snr_value", "<f4"), ("snr_summ_cnt", "<u2"), ("code_filt_cnt", "<u2"), ("code_phase_fine_filt", "<f4"),
                       ("old_swap_time", "<u4"), ("slot_start_ticks", "<u4"), ("slot_ip", "<i2", 4), ("slot_bits", "u1"),
                       ("right_period_cnt", "u1"), ("old_reminder", "u1"), ("accurate_swap_time", "u1"),
                       ("accurate_swap_ok", "u1"), ("last_bit_pos_cnt", "u1"), ("last_bit_neg_cnt", "u1"),
                       ("inv_polarity_flag", "u1"), ("prev_track_timestamp", "<u4"), ("snr_i_latch", "<u4"),
                       ("snr_q_latch", "<u4"), ("word_buf", "<u4"), ("word_detection_timestamp", "<u4"), ("word_cnt", "u1"),
                       ("word_bit_cnt", "u1"), ("inv_preabmle_cnt", "u1"), ("word_flags", "u1")])   # gpsx_loop_state_t, 120 bytes
LOOP_TRACE_DTYPE = np.dtype([("iq", "<i2", 6), ("code_phase_fine", "<f4"), ("if_freq_offset_hz", "<f4"), ("if_freq_accum", "<u4")])
assert LOOP_DTYPE.itemsize == 120 and LOOP_TRACE_DTYPE.itemsize == 24
PEAK_DTYPE = np.dtype([("max_val", "<u4"), ("phase", "<u4"), ("sum", "<u4"), ("avr", "<u4")])
TRACK_CHUNK_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_int)   # gpsx_track_chunk_fn
# gpsx_wloop_state_t / gpsx_wloop_cfg_t / gpsx_wloop_rec_t (the closed loop on weighted two-bit samples)
WLOOP_STATE_DTYPE = np.dtype([("prn", "<i4"), ("code_phase_fine", "<f4"), ("if_freq_offset_hz", "<f4"), ("if_freq_accum", "<u4"),
                              ("dll_err", "<f4"), ("pll_err", "<f4"), ("prev_ip", "<i4"), ("prev_qp", "<i4"), ("n_updates", "<u4"),
                              ("reserved", "<u4")])
WLOOP_CFG_DTYPE = np.dtype([("weights", "<i4"), ("spacing", "<i4"), ("n_coh", "<i4"), ("dll_c1", "<f4"), ("dll_c2", "<f4"),
                            ("pll_c1", "<f4"), ("pll_c2", "<f4"), ("fll_c", "<f4")])
WLOOP_REC_DTYPE = np.dtype([("iq", "<i4", 6), ("code_phase_fine", "<f4"), ("if_freq_offset_hz", "<f4"), ("if_freq_accum", "<u4")])
assert WLOOP_STATE_DTYPE.itemsize == 40 and WLOOP_CFG_DTYPE.itemsize == 32 and WLOOP_REC_DTYPE.itemsize == 36


def wloop_cfg(n_coh, use_magnitude=True, spacing=8, dll=(1.0, 300.0), pll=(4.0, 3000.0), fll=0.0) -> np.ndarray:
    """a gpsx_wloop_cfg_t as a one-element WLOOP_CFG_DTYPE array"""
    cfg = np.zeros(1, WLOOP_CFG_DTYPE)
    cfg[0] = (1 if use_magnitude else 0, spacing, n_coh, dll[0], dll[1], pll[0], pll[1], fll)
    return cfg


# gpsx_wsync_state_t / gpsx_wsync_cfg_t / gpsx_wsync_rec_t (the weighted loop with a per-channel bit synchroniser)
WSYNC_SEARCH, WSYNC_WAIT, WSYNC_LOCKED = 0, 1, 2
WSYNC_FLAG_WINDOW, WSYNC_FLAG_LOCKED, WSYNC_FLAG_BIT = 1, 2, 4
WSYNC_GAINS_DTYPE = np.dtype([("dll_c1", "<f4"), ("dll_c2", "<f4"), ("pll_c1", "<f4"), ("pll_c2", "<f4"), ("fll_c", "<f4")])
WSYNC_CFG_DTYPE = np.dtype([("weights", "<i4"), ("spacing", "<i4"), ("n_coh_search", "<i4"), ("n_coh_lock", "<i4"),
                            ("search", WSYNC_GAINS_DTYPE), ("lock", WSYNC_GAINS_DTYPE), ("sync_bits", "<i4"), ("sync_num", "<i4"),
                            ("sync_den", "<i4")])
WSYNC_STATE_DTYPE = np.dtype([("loop", WLOOP_STATE_DTYPE), ("win_iq", "<i4", 6), ("win_n", "<i4"), ("ms_count", "<i4"), ("mode", "<i4"),
                              ("edge", "<i4"), ("bit_ip", "<i4"), ("search_n", "<i4"), ("prev_best_p1", "<i4"), ("sync_rounds", "<i4"),
                              ("p_i", "<i4"), ("p_q", "<i4"), ("last_best_e", "<i8"), ("last_opp_e", "<i8"), ("zero", "<i4", 2),
                              ("base", "<i4", (20, 2)), ("e", "<i8", 20)])
WSYNC_REC_DTYPE = np.dtype([("w", WLOOP_REC_DTYPE), ("end_block", "<i4"), ("flags", "<u4"), ("bit_ip", "<i4")])
assert WSYNC_CFG_DTYPE.itemsize == 68 and WSYNC_STATE_DTYPE.itemsize == 448 and WSYNC_REC_DTYPE.itemsize == 48


def wsync_cfg(n_coh_search, n_coh_lock, search, lock, sync_bits=20, sync_ratio=(5, 4), use_magnitude=True, spacing=8) -> np.ndarray:
    """a gpsx_wsync_cfg_t as a one-element WSYNC_CFG_DTYPE array.  search / lock: dict(dll=(c1, c2), pll=(c1, c2), fll=c), the gains
    of the windows before and after bit sync; sync_ratio: (sync_num, sync_den)"""
    cfg = np.zeros(1, WSYNC_CFG_DTYPE)
    cfg["weights"], cfg["spacing"], cfg["n_coh_search"], cfg["n_coh_lock"] = (1 if use_magnitude else 0), spacing, n_coh_search, n_coh_lock
    for name, g in (("search", search), ("lock", lock)):
        cfg[name][0] = (g["dll"][0], g["dll"][1], g["pll"][0], g["pll"][1], g.get("fll", 0.0))
    cfg["sync_bits"], cfg["sync_num"], cfg["sync_den"] = sync_bits, sync_ratio[0], sync_ratio[1]
    return cfg


def wsync_slots(n_blocks, n_coh_search, n_coh_lock) -> int:
    """record slots of a launch: ceil(n_blocks / min(n_coh_search, n_coh_lock))"""
    span = max(1, min(n_coh_search, n_coh_lock))
    return (n_blocks + span - 1) // span


# gpsx_waid_t (carrier aiding of the weighted code loop: gpsx_track_loop_weighted_aided, gpsx_track_loop_weighted_sync_aided)
WAID_L1CA = np.float32(0.010389610)      # GPSX_WAID_L1CA: 16 samples per chip / 1540 carrier cycles per chip
WAID_DTYPE = np.dtype([("code_per_hz", "<f4"), ("reserved", "<i4")])
assert WAID_DTYPE.itemsize == 8


def waid(code_per_hz=WAID_L1CA) -> np.ndarray:
    """a gpsx_waid_t as a one-element WAID_DTYPE array"""
    aid = np.zeros(1, WAID_DTYPE)
    aid["code_per_hz"] = code_per_hz
    return aid


# gpsx_wmulti_t (gpsx_track_loop_weighted_sync_multi: many receivers per launch, one IF stream each)
PRN_NONE = -2147483648                   # GPSX_PRN_NONE: a channel slot that holds no channel
WMULTI_DTYPE = np.dtype([("n_rx", "<i4"), ("ch_per_rx", "<i4"), ("rx_stride_blocks", "<i4"), ("reserved", "<i4")])
assert WMULTI_DTYPE.itemsize == 16


def wmulti(n_rx, ch_per_rx, rx_stride_blocks) -> np.ndarray:
    """a gpsx_wmulti_t as a one-element WMULTI_DTYPE array"""
    rx = np.zeros(1, WMULTI_DTYPE)
    rx["n_rx"], rx["ch_per_rx"], rx["rx_stride_blocks"] = n_rx, ch_per_rx, rx_stride_blocks
    return rx


# gpsx_wnav_cfg_t / gpsx_wnav_state_t / gpsx_wnav_word_t (LNAV frame sync and parity-checked words from the sync loop's records)
WNAV_HUNT, WNAV_SYNCED = 0, 1
WNAV_FLAG_WORD, WNAV_FLAG_OK, WNAV_FLAG_INVERTED, WNAV_FLAG_SYNC, WNAV_FLAG_FLIPPED, WNAV_FLAG_SUBFRAME, WNAV_FLAG_DROPPED = 1, 2, 4, 8, 16, 32, 64
WNAV_CFG_DTYPE = np.dtype([("max_bad_words", "<i4"), ("reserved", "<i4")])
WNAV_STATE_DTYPE = np.dtype([("hist", "<u8"), ("blocks_seen", "<i8"), ("last_bit_end_p1", "<i8"), ("fresh", "<i4"), ("mode", "<i4"),
                             ("inv", "<i4"), ("word_idx", "<i4"), ("bit_idx", "<i4"), ("bad_run", "<i4"), ("ok_mask", "<u4"),
                             ("n_sync", "<u4"), ("n_drop", "<u4"), ("n_subframes", "<u4")])
WNAV_WORD_DTYPE = np.dtype([("end_block", "<i4"), ("word", "<u4"), ("index", "u1"), ("flags", "u1"), ("subframe_id", "u1"), ("zero", "u1"),
                            ("aux", "<u4")])
assert WNAV_CFG_DTYPE.itemsize == 8 and WNAV_STATE_DTYPE.itemsize == 64 and WNAV_WORD_DTYPE.itemsize == 16


def wnav_word_slots(n_blocks) -> int:
    """word slots per channel of a launch: n_blocks / 600 + 2"""
    return n_blocks // 600 + 2


def subframe_image(ten: np.ndarray) -> np.ndarray:
    """ten WNAV_WORD_DTYPE records of one subframe (index 1 .. 10 in order, all OK) -> the 38-byte image
    gps_nav_data_decode_subframe reads; GpsxError otherwise.  Host only."""
    ten = np.ascontiguousarray(ten, WNAV_WORD_DTYPE)
    if ten.shape != (10,):
        raise GpsxError("subframe_image takes ten word records")
    image = np.zeros(38, np.uint8)
    rc = load_library().gpsx_wnav_subframe_image(ten.ctypes.data, image.ctypes.data)
    if rc != 0:
        raise GpsxError(f"gpsx_wnav_subframe_image -> {rc}: the records are not words 1 .. 10 of one subframe, all of them OK")
    return image


# gpsx_wobs_cfg_t / gpsx_wobs_state_t / gpsx_wobs_t (every channel's transmit time at the launch's end, from the records and the words)
WOBS_FLAG_PHASE, WOBS_FLAG_EDGE, WOBS_FLAG_TOW, WOBS_FLAG_CONFIRMED, WOBS_FLAG_AMBIGUOUS, WOBS_FLAG_VALID = 1, 2, 4, 8, 16, 32
WOBS_CFG_DTYPE = np.dtype([("edge_guard", "<f4"), ("reserved", "<i4")])
WOBS_STATE_DTYPE = np.dtype([("blocks_seen", "<i8"), ("last_bit_end_p1", "<i8"), ("chain_first_p1", "<i8"), ("edge_block", "<i8"),
                             ("tx_ms_at_edge", "<i8"), ("last_win_end_p1", "<i8"), ("last_phase", "<f4"), ("last_freq", "<f4"), ("flags", "<u4"),
                             ("n_wraps", "<u4"), ("n_anchor", "<u4"), ("n_mismatch", "<u4"), ("n_break", "<u4"), ("reserved", "<u4")])
WOBS_DTYPE = np.dtype([("tx_ms", "<i8"), ("code_phase_fine", "<f4"), ("if_freq_offset_hz", "<f4"), ("flags", "<u4"), ("age_blocks", "<i4"),
                       ("n_wraps", "<u4"), ("reserved", "<u4")])
assert WOBS_CFG_DTYPE.itemsize == 8 and WOBS_STATE_DTYPE.itemsize == 80 and WOBS_DTYPE.itemsize == 32


def wobs_pseudoranges(obs: np.ndarray, offset_ms: float = 68.802):
    """WOBS_DTYPE observables of one launch -> (pr_m float64 [n], 0 where an observable is not VALID; rx_tow_s; the number of VALID
    ones), against the channel with the latest transmit time at offset_ms of travel time.  Host only."""
    obs = np.ascontiguousarray(obs, WOBS_DTYPE).reshape(-1)
    pr = np.zeros(len(obs), np.float64)
    rx = C.c_double(0.0)
    n = load_library().gpsx_wobs_pseudoranges(obs.ctypes.data, len(obs), float(offset_ms), pr.ctypes.data, C.byref(rx))
    if n < 0:
        raise GpsxError(f"gpsx_wobs_pseudoranges -> {n}: no observables, or an offset that is not finite")
    return pr, rx.value, n


def wobs_pseudoranges_rx(obs: np.ndarray, n_rx: int, ch_per_rx: int, offset_ms: float = 68.802):
    """wobs_pseudoranges on each receiver's slice of the WOBS_DTYPE [n_rx * ch_per_rx] observables of a multi-receiver chain, the
    reference channel chosen per receiver -> (pr_m float64 [n_rx * ch_per_rx], rx_tow_s float64 [n_rx], n_valid int32 [n_rx]).
    Host only."""
    obs = np.ascontiguousarray(obs, WOBS_DTYPE).reshape(-1)
    if n_rx < 1 or ch_per_rx < 1 or len(obs) != n_rx * ch_per_rx:
        raise GpsxError("wobs_pseudoranges_rx takes n_rx * ch_per_rx observables")
    pr, rx, n_valid = np.zeros(len(obs), np.float64), np.zeros(n_rx, np.float64), np.zeros(n_rx, np.int32)
    n = load_library().gpsx_wobs_pseudoranges_rx(obs.ctypes.data, n_rx, ch_per_rx, float(offset_ms), pr.ctypes.data, rx.ctypes.data,
                                                 n_valid.ctypes.data)
    if n < 0:
        raise GpsxError(f"gpsx_wobs_pseudoranges_rx -> {n}: no observables, or an offset that is not finite")
    return pr, rx, n_valid


# gpsx_weph_cfg_t / gpsx_weph_state_t / gpsx_weph_t (every channel's broadcast ephemeris from the words) and eph_t (include/gpsx_compat.h)
WEPH_FLAG_VALID, WEPH_FLAG_NEW = 1, 2
WEPH_CFG_DTYPE = np.dtype([("reserved0", "<i4"), ("reserved1", "<i4")])
WEPH_STATE_DTYPE = np.dtype([("blocks_seen", "<i8"), ("last_word_end_p1", "<i8"), ("cur", "<u4", (8,)), ("cur_mask", "<u4"), ("cur_next", "<u4"),
                             ("cur_id", "<u4"), ("cur_tow", "<u4"), ("sf", "<u4", (3, 8)), ("sf_tow", "<u4", (3,)), ("have", "<u4"), ("flags", "<u4"),
                             ("n_sets", "<u4"), ("n_subframes", "<u4"), ("reserved", "<u4")])
WEPH_DOUBLES = ("A", "e", "i0", "OMG0", "omg", "M0", "deln", "OMGd", "idot", "crc", "crs", "cuc", "cus", "cic", "cis", "toes", "fit", "f0", "f1", "f2", "tgd")
WEPH_DTYPE = np.dtype([("flags", "<u4")] + [(k, "<i4") for k in ("iode", "iodc", "sva", "svh", "week", "code", "flag")] +
                      [(k, "<i8") for k in ("toe_time", "toc_time", "ttr_time")] + [(k, "<f8") for k in ("toe_sec", "toc_sec", "ttr_sec")] +
                      [(k, "<f8") for k in WEPH_DOUBLES] + [("n_sets", "<u4"), ("have", "<u4")])
EPH_DTYPE = np.dtype([(k, "<i4") for k in ("sat", "iode", "iodc", "sva", "svh", "week", "code", "flag")] +
                     [(k, t) for g in ("toe", "toc", "ttr") for k, t in ((g + "_time", "<i8"), (g + "_sec", "<f8"))] +
                     [(k, "<f8") for k in WEPH_DOUBLES[:-1]] + [("tgd", "<f8", (4,))])
assert WEPH_CFG_DTYPE.itemsize == 8 and WEPH_STATE_DTYPE.itemsize == 192 and WEPH_DTYPE.itemsize == 256 and EPH_DTYPE.itemsize == 272


def weph_to_eph(rec, prn: int) -> np.ndarray:
    """one VALID WEPH_DTYPE record -> the reference's eph_t as EPH_DTYPE [1] (what gps_nav_data_decode_subframe leaves in a zeroed
    channel's eph_data.eph after subframes 1, 2, 3 of the record's bits, with sat = prn); GpsxError without VALID.  Host only."""
    rec = np.ascontiguousarray(rec, WEPH_DTYPE).reshape(-1)
    if len(rec) != 1:
        raise GpsxError("weph_to_eph takes one record")
    out = np.zeros(1, EPH_DTYPE)
    rc = load_library().gpsx_weph_to_eph(rec.ctypes.data, int(prn), out.ctypes.data)
    if rc != 0:
        raise GpsxError(f"gpsx_weph_to_eph -> {rc}: the record is not VALID")
    return out


# gpsx_wlock_cfg_t / gpsx_wlock_state_t / gpsx_wlock_t (every channel's code-lock, carrier-lock and C/N0 indicators from the records)
WLOCK_FLAG_CODE, WLOCK_FLAG_CARRIER, WLOCK_FLAG_PENDING, WLOCK_FLAG_OPEN_LOCKED, WLOCK_FLAG_EPOCH_LOCKED = 1, 2, 4, 8, 16
WLOCK_FLAG_LOST_CODE, WLOCK_FLAG_LOST_CARRIER, WLOCK_FLAG_REARMED, WLOCK_FLAG_RANGE = 32, 64, 128, 256
WLOCK_REARM_CODE_LOSS, WLOCK_REARM_NO_CARRIER = 1, 2
WLOCK_CFG_DTYPE = np.dtype([("epoch_search", "<i4"), ("epoch_lock", "<i4"), ("code_min", "<f4"), ("car_min", "<f4"), ("snr_min", "<f4"),
                            ("n_good", "<i4"), ("n_bad", "<i4"), ("rearm", "<i4"), ("patience", "<i4"), ("reserved", "<i4")])
WLOCK_STATE_DTYPE = np.dtype([("blocks_seen", "<i8"), ("last_epoch_end_p1", "<i8"), ("sum_a", "<i8"), ("sum_p", "<i8"), ("sum_d", "<i8"),
                              ("sum_e", "<i8"), ("sum_l", "<i8"), ("last_p", "<i8"), ("last_code_ratio", "<f4"), ("last_car_ratio", "<f4"),
                              ("last_snr", "<f4"), ("epoch_n", "<u4"), ("flags", "<u4"), ("last_k", "<u4"), ("code_good", "<u4"),
                              ("code_bad", "<u4"), ("car_good", "<u4"), ("car_bad", "<u4"), ("false_run", "<u4"), ("n_lost_code", "<u4"),
                              ("n_lost_carrier", "<u4"), ("n_rearm", "<u4"), ("n_range", "<u4"), ("reserved", "<u4")])
WLOCK_DTYPE = np.dtype([("flags", "<u4"), ("n_epochs", "<u4"), ("last_k", "<u4"), ("age_blocks", "<i4"), ("code_ratio", "<f4"),
                        ("car_ratio", "<f4"), ("snr", "<f4"), ("n_range", "<u4"), ("p", "<i8"), ("n_lost_code", "<u4"),
                        ("n_lost_carrier", "<u4"), ("n_rearm", "<u4"), ("reserved", "<u4", (3,))])
assert WLOCK_CFG_DTYPE.itemsize == 40 and WLOCK_STATE_DTYPE.itemsize == 128 and WLOCK_DTYPE.itemsize == 64


# gpsx_wfix_cfg_t / gpsx_wfix_t (every receiver's position fix from the observables and ephemeris records)
WFIX_FLAG_FIX, WFIX_FLAG_TOO_FEW, WFIX_FLAG_SINGULAR, WFIX_FLAG_NO_CONV, WFIX_FLAG_NONFINITE = 1, 2, 4, 8, 16
WFIX_CFG_DTYPE = np.dtype([("offset_ms", "<f8"), ("ion", "<f8", (8,)), ("ch_per_rx", "<i4"), ("min_sats", "<i4"), ("reserved0", "<i4"),
                           ("reserved1", "<i4"), ("reserved2", "<i4"), ("reserved3", "<i4")])
WFIX_DTYPE = np.dtype([("flags", "<u4"), ("n_used", "<i4"), ("n_iter", "<i4"), ("ref_slot", "<i4"), ("used_mask", "<u8"), ("rr", "<f8", (3,)),
                       ("dtr_s", "<f8"), ("rx_tow_s", "<f8"), ("geo", "<f8", (3,)), ("qr", "<f4", (6,)), ("resid_rms_m", "<f8"), ("week", "<i4"),
                       ("reserved", "<i4")])
assert WFIX_CFG_DTYPE.itemsize == 96 and WFIX_DTYPE.itemsize == 128


def wfix_cfg(offset_ms: float, ch_per_rx: int, min_sats: int = 4, ion=None) -> np.ndarray:
    """a gpsx_wfix_cfg_t as a one-element WFIX_CFG_DTYPE array (ion None: all zero, the solver's default Klobuchar set)"""
    cfg = np.zeros(1, WFIX_CFG_DTYPE)
    cfg["offset_ms"], cfg["ch_per_rx"], cfg["min_sats"] = offset_ms, ch_per_rx, min_sats
    if ion is not None:
        cfg["ion"][0] = ion
    return cfg


# gpsx_wfde_cfg_t / gpsx_wfde_t (the fixes with the ambiguous millisecond repaired and faulty slots detected and excluded)
WFDE_FLAG_PASSED, WFDE_FLAG_UNCHECKED, WFDE_FLAG_FAULT, WFDE_FLAG_NOFIX = 1, 2, 4, 8
WFDE_FLAG_EXCLUDED, WFDE_FLAG_REPAIRED, WFDE_FLAG_UNRESOLVED = 16, 32, 64
WFDE_CFG_DTYPE = np.dtype([("fix", WFIX_CFG_DTYPE), ("z_global", "<f8"), ("max_excl", "<i4"), ("repair", "<i4"), ("reserved", "<i4", (4,))])
WFDE_DTYPE = np.dtype([("flags", "<u4"), ("n_rounds", "<i4"), ("n_excluded", "<i4"), ("dof", "<i4"), ("excl_mask", "<u8"), ("plus_mask", "<u8"),
                       ("minus_mask", "<u8"), ("t_stat", "<f8"), ("t_limit", "<f8"), ("reserved", "<u8")])
assert WFDE_CFG_DTYPE.itemsize == 128 and WFDE_DTYPE.itemsize == 64


def wfde_cfg(offset_ms: float, ch_per_rx: int, min_sats: int = 4, ion=None, z_global: float = 3.09, max_excl: int = 2, repair: bool = True) -> np.ndarray:
    """a gpsx_wfde_cfg_t as a one-element WFDE_CFG_DTYPE array: wfix_cfg's fields, the global test's normal quantile (3.09: a false
    alarm in a thousand), the statistical exclusions allowed per receiver (0 .. 8) and whether the ambiguous millisecond is repaired"""
    cfg = np.zeros(1, WFDE_CFG_DTYPE)
    cfg["fix"] = wfix_cfg(offset_ms, ch_per_rx, min_sats, ion)
    cfg["z_global"], cfg["max_excl"], cfg["repair"] = z_global, max_excl, int(repair)
    return cfg


# gpsx_wvel_cfg_t / gpsx_wvel_t (every receiver's velocity and clock drift from the carrier frequencies and the position records)
WVEL_FLAG_VEL, WVEL_FLAG_NO_FIX, WVEL_FLAG_TOO_FEW, WVEL_FLAG_SINGULAR, WVEL_FLAG_NONFINITE = 1, 2, 4, 8, 16
WVEL_L1CA = -0.19029367279836487      # GPSX_WVEL_L1CA: -c / 1575.42e6, m/s of range rate per Hz of a frequency that is the Doppler
WVEL_L1CA_WLOOP = WVEL_L1CA * 1022.0 / 1023.0      # GPSX_WVEL_L1CA_WLOOP: per Hz of the weighted loops' if_freq_offset_hz, which rest at fd (1 + 1/1022)
WVEL_CFG_DTYPE = np.dtype([("mps_per_hz", "<f8"), ("ch_per_rx", "<i4"), ("min_sats", "<i4"), ("reserved", "<i4", (4,))])
WVEL_DTYPE = np.dtype([("flags", "<u4"), ("n_used", "<i4"), ("used_mask", "<u8"), ("vel", "<f8", (3,)), ("drift_s_s", "<f8"), ("enu", "<f8", (3,)),
                       ("qv", "<f4", (6,)), ("resid_rms_mps", "<f8"), ("reserved", "<u8")])
assert WVEL_CFG_DTYPE.itemsize == 32 and WVEL_DTYPE.itemsize == 112


def wvel_cfg(ch_per_rx: int, min_sats: int = 4, mps_per_hz: float = WVEL_L1CA) -> np.ndarray:
    """a gpsx_wvel_cfg_t as a one-element WVEL_CFG_DTYPE array.  mps_per_hz: the default is for frequencies that are the Doppler;
    observables of this library's weighted loops take WVEL_L1CA_WLOOP"""
    cfg = np.zeros(1, WVEL_CFG_DTYPE)
    cfg["mps_per_hz"], cfg["ch_per_rx"], cfg["min_sats"] = mps_per_hz, ch_per_rx, min_sats
    return cfg


# gpsx_wkf_cfg_t / gpsx_wkf_state_t / gpsx_wkf_t (every receiver's navigation filter: a resident eight-state Kalman filter)
WKF_FLAG_INIT, WKF_FLAG_NOT_INIT, WKF_FLAG_UPDATED, WKF_FLAG_COAST, WKF_FLAG_LOST, WKF_FLAG_BAD = 1, 2, 4, 8, 16, 32
WKF_FLAG_REPAIRED, WKF_FLAG_REJECTED, WKF_FLAG_STEERED = 64, 128, 256
WKF_STATE_INIT = 1
WKF_CFG_DTYPE = np.dtype([("ion", "<f8", (8,)), ("mps_per_hz", "<f8"), ("sig_pr_m", "<f8"), ("sig_dop_mps", "<f8"), ("gate", "<f8"), ("q_acc", "<f8"),
                          ("q_clk_f", "<f8"), ("q_clk_g", "<f8"), ("p0_pos", "<f8"), ("p0_clk", "<f8"), ("p0_vel", "<f8"), ("p0_drift", "<f8"),
                          ("ch_per_rx", "<i4"), ("max_coast", "<i4"), ("reserved", "<i4", (4,))])
WKF_STATE_DTYPE = np.dtype([("x", "<f8", (8,)), ("P", "<f8", (36,)), ("rcv_ms", "<i8"), ("week", "<i4"), ("flags", "<u4"), ("n_starved", "<u4"),
                            ("n_init", "<u4"), ("n_lost", "<u4"), ("reserved", "<u4")])
WKF_DTYPE = np.dtype([("flags", "<u4"), ("n_pr", "<i4"), ("n_dop", "<i4"), ("n_starved", "<u4"), ("pr_mask", "<u8"), ("dop_mask", "<u8"),
                      ("rej_pr_mask", "<u8"), ("rej_dop_mask", "<u8"), ("plus_mask", "<u8"), ("minus_mask", "<u8"), ("rr", "<f8", (3,)),
                      ("clk_m", "<f8"), ("vel", "<f8", (3,)), ("cdrift_mps", "<f8"), ("geo", "<f8", (3,)), ("enu", "<f8", (3,)), ("sigma", "<f4", (8,)),
                      ("nis_pr", "<f8"), ("nis_dop", "<f8"), ("rcv_ms", "<i8"), ("week", "<i4"), ("reserved", "<i4")])
assert WKF_CFG_DTYPE.itemsize == 176 and WKF_STATE_DTYPE.itemsize == 384 and WKF_DTYPE.itemsize == 240


def wkf_cfg(ch_per_rx: int, mps_per_hz: float = WVEL_L1CA, sig_pr_m: float = 3.0, sig_dop_mps: float = 0.1, gate: float = 5.0, q_acc: float = 1.0,
            q_clk_f: float = 0.04, q_clk_g: float = 0.4, p0=(30.0, 30.0, 10.0, 500.0), max_coast: int = 10, ion=None) -> np.ndarray:
    """a gpsx_wkf_cfg_t as a one-element WKF_CFG_DTYPE array: the row noises (m, m/s), the gate in standard deviations, the process
    noise (q_acc m^2/s^3 per axis; the clock's phase and frequency noise), the initial standard deviations p0 = (position, clock,
    velocity, drift) and the launches a receiver may go without a pseudorange row.  mps_per_hz as wvel_cfg's"""
    cfg = np.zeros(1, WKF_CFG_DTYPE)
    for name, v in (("mps_per_hz", mps_per_hz), ("sig_pr_m", sig_pr_m), ("sig_dop_mps", sig_dop_mps), ("gate", gate), ("q_acc", q_acc),
                    ("q_clk_f", q_clk_f), ("q_clk_g", q_clk_g), ("p0_pos", p0[0]), ("p0_clk", p0[1]), ("p0_vel", p0[2]), ("p0_drift", p0[3]),
                    ("ch_per_rx", ch_per_rx), ("max_coast", max_coast)):
        cfg[name] = v
    if ion is not None:
        cfg["ion"][0] = ion
    return cfg


# gpsx_wacq_cfg_t / gpsx_wacq_det_t / gpsx_wacq_t (acquisition decisions and slot hand-over between a weighted grid and the sync loop)
WACQ_DET_DETECTED, WACQ_DET_TRACKED, WACQ_DET_ASSIGNED, WACQ_DET_DROPPED = 1, 2, 4, 8
WACQ_FLAG_ASSIGNED, WACQ_FLAG_EVICTED, WACQ_FLAG_FULL = 1, 2, 4
WACQ_CFG_DTYPE = np.dtype([("ch_per_rx", "<i4"), ("det_num", "<i4"), ("det_den", "<i4"), ("min_peak", "<u4"), ("lead_blocks", "<i4"),
                           ("code_per_hz", "<f4"), ("evict_after_blocks", "<i4"), ("reserved", "<i4")])
WACQ_DET_DTYPE = np.dtype([("max_val", "<u4"), ("phase", "<u4"), ("dopp_hz", "<i4"), ("flags", "u1"), ("slot", "i1"), ("zero", "<u2")])
WACQ_DTYPE = np.dtype([("flags", "<u4"), ("n_detected", "<u4"), ("n_tracked", "<u4"), ("n_assigned", "<u4"), ("n_evicted", "<u4"),
                       ("n_dropped", "<u4"), ("assigned_mask", "<u8"), ("evicted_mask", "<u8"), ("kept_mask", "<u8"), ("free_mask", "<u8"),
                       ("reserved", "<u4", (2,))])
assert WACQ_CFG_DTYPE.itemsize == 32 and WACQ_DET_DTYPE.itemsize == 16 and WACQ_DTYPE.itemsize == 64


def wacq_cfg(ch_per_rx: int, det=(4, 1), min_peak: int = 0, lead_blocks: int = 0, code_per_hz: float = 0.0, evict_after_blocks: int = 0) -> np.ndarray:
    """a gpsx_wacq_cfg_t as a one-element WACQ_CFG_DTYPE array: a PRN is detected when its best record's peak is at least
    det[0] / det[1] times its mean over the phases (and at least min_peak); lead_blocks and code_per_hz (WAID_L1CA) project the
    record's phase to the loop's first block; a slot without code lock evict_after_blocks after its hand-over is freed (0: never)"""
    cfg = np.zeros(1, WACQ_CFG_DTYPE)
    for name, v in (("ch_per_rx", ch_per_rx), ("det_num", det[0]), ("det_den", det[1]), ("min_peak", min_peak), ("lead_blocks", lead_blocks),
                    ("code_per_hz", code_per_hz), ("evict_after_blocks", evict_after_blocks)):
        cfg[name] = v
    return cfg


# gpsx_wbank_cfg_t / gpsx_wbank_t (the ephemeris bank behind gpsx_weph: a receiver's newest VALID record per listed PRN, WEPH_DTYPE [n_rx, n_prn])
WBANK_CFG_DTYPE = np.dtype([("ch_per_rx", "<i4"), ("reserved", "<i4", (3,))])
WBANK_DTYPE = np.dtype([("stored_mask", "<u8"), ("have_mask", "<u8"), ("from_bank_mask", "<u8"), ("n_stored", "<u2"), ("n_have", "<u2"),
                        ("n_from_bank", "<u2"), ("zero", "<u2")])
assert WBANK_CFG_DTYPE.itemsize == 16 and WBANK_DTYPE.itemsize == 32


def wbank_cfg(ch_per_rx: int) -> np.ndarray:
    """a gpsx_wbank_cfg_t as a one-element WBANK_CFG_DTYPE array"""
    cfg = np.zeros(1, WBANK_CFG_DTYPE)
    cfg["ch_per_rx"] = ch_per_rx
    return cfg


# gpsx_wpred_cfg_t / gpsx_wpred_t / gpsx_wpred_rx_t (prediction and hot hand-over behind the navigation filter, from its state and the bank)
WPRED_HAVE_EPH, WPRED_PREDICTED, WPRED_VISIBLE, WPRED_CERTAIN, WPRED_TRACKED, WPRED_ASSIGNED, WPRED_DROPPED = 1, 2, 4, 8, 16, 32, 64
WPRED_RX_PREDICTED, WPRED_RX_NOT_INIT, WPRED_RX_BAD, WPRED_RX_ASSIGNED, WPRED_RX_EVICTED, WPRED_RX_FULL = 1, 2, 4, 8, 16, 32
WPRED_CFG_DTYPE = np.dtype([("ion", "<f8", (8,)), ("mps_per_hz", "<f8"), ("el_min_rad", "<f8"), ("max_sigma_m", "<f8"), ("max_sigma_hz", "<f8"),
                            ("ch_per_rx", "<i4"), ("lead_blocks", "<i4"), ("evict_after_blocks", "<i4"), ("handover", "<i4"), ("reserved", "<i4", (4,))])
WPRED_DTYPE = np.dtype([("flags", "<u4"), ("slot", "<i4"), ("tx_ms", "<i8"), ("pr_m", "<f8"), ("code_phase", "<f8"), ("f_hz", "<f8"), ("el", "<f8"),
                        ("az", "<f8"), ("sigma_m", "<f4"), ("sigma_hz", "<f4")])
WPRED_RX_DTYPE = np.dtype([("flags", "<u2"), ("week", "<i2"), ("t_ms", "<i4"), ("n_have", "u1"), ("n_visible", "u1"), ("n_tracked", "u1"),
                           ("n_assigned", "u1"), ("n_evicted", "u1"), ("n_dropped", "u1"), ("zero", "<u2"), ("visible_mask", "<u8"), ("have_mask", "<u8"),
                           ("assigned_mask", "<u8"), ("evicted_mask", "<u8"), ("kept_mask", "<u8"), ("free_mask", "<u8")])
assert WPRED_CFG_DTYPE.itemsize == 128 and WPRED_DTYPE.itemsize == 64 and WPRED_RX_DTYPE.itemsize == 64


def wpred_cfg(ch_per_rx: int, mps_per_hz: float = WVEL_L1CA, el_min_rad: float = 0.0873, max_sigma_m: float = 300.0, max_sigma_hz: float = 12.5,
              lead_blocks: int = 0, evict_after_blocks: int = 0, handover: int = 1, ion=None) -> np.ndarray:
    """a gpsx_wpred_cfg_t as a one-element WPRED_CFG_DTYPE array: a banked satellite is a candidate when it stands at least el_min_rad
    (5 degrees) above the horizon lead_blocks after the filter's rcv_ms and its predicted pseudorange and frequency are known to
    max_sigma_m and max_sigma_hz (one sigma, from the filter's covariance); handover 1 writes the candidates into free slots"""
    cfg = np.zeros(1, WPRED_CFG_DTYPE)
    for name, v in (("mps_per_hz", mps_per_hz), ("el_min_rad", el_min_rad), ("max_sigma_m", max_sigma_m), ("max_sigma_hz", max_sigma_hz),
                    ("ch_per_rx", ch_per_rx), ("lead_blocks", lead_blocks), ("evict_after_blocks", evict_after_blocks), ("handover", handover)):
        cfg[name] = v
    if ion is not None:
        cfg["ion"][0] = ion
    return cfg


# gpsx_wsnap_cfg_t / gpsx_wsnap_prior_t / gpsx_wsnap_t / gpsx_wsnap_sv_t (snapshot fixes from a weighted grid's records, a bank and a prior)
WSNAP_FIX, WSNAP_RESID, WSNAP_TOO_FEW, WSNAP_SINGULAR, WSNAP_NO_CONV, WSNAP_NONFINITE, WSNAP_NO_PRIOR = 1, 2, 4, 8, 16, 32, 64
WSNAP_PRIOR_HAVE = 1
WSNAP_SV_DETECTED, WSNAP_SV_HAVE_EPH, WSNAP_SV_CANDIDATE, WSNAP_SV_USED, WSNAP_SV_REFERENCE = 1, 2, 4, 8, 16
WSNAP_CFG_DTYPE = np.dtype([("ion", "<f8", (8,)), ("el_min_rad", "<f8"), ("epoch_offset_s", "<f8"), ("max_resid_m", "<f8"), ("det_num", "<i4"),
                            ("det_den", "<i4"), ("min_peak", "<u4"), ("min_sats", "<i4"), ("reserved", "<i4", (6,))])
WSNAP_PRIOR_DTYPE = np.dtype([("flags", "<u4"), ("week", "<i4"), ("rr", "<f8", (3,)), ("tow_s", "<f8"), ("reserved", "<u4", (2,))])
WSNAP_DTYPE = np.dtype([("flags", "<u4"), ("week", "<i4"), ("n_detected", "u1"), ("n_candidates", "u1"), ("n_used", "u1"), ("n_iter", "u1"),
                        ("ref", "<i4"), ("used_mask", "<u8"), ("rr", "<f8", (3,)), ("b_m", "<f8"), ("dt_s", "<f8"), ("tow_s", "<f8"),
                        ("geo", "<f8", (3,)), ("resid_rms_m", "<f8"), ("qr", "<f4", (6,))])
WSNAP_SV_DTYPE = np.dtype([("flags", "<u4"), ("n_ms", "<i4"), ("phase", "<u4"), ("dopp_hz", "<i4"), ("el", "<f8"), ("az", "<f8"), ("resid_m", "<f8"),
                           ("reserved", "<u4", (2,))])
assert WSNAP_CFG_DTYPE.itemsize == 128 and WSNAP_PRIOR_DTYPE.itemsize == 48 and WSNAP_DTYPE.itemsize == 128 and WSNAP_SV_DTYPE.itemsize == 48


def wsnap_cfg(epoch_offset_s: float, el_min_rad: float = 0.0873, max_resid_m: float = 1000.0, det=(4, 1), min_peak: int = 0, min_sats: int = 5,
              ion=None) -> np.ndarray:
    """a gpsx_wsnap_cfg_t as a one-element WSNAP_CFG_DTYPE array: a PRN counts when its best record is detected as gpsx_wacq detects
    (det, min_peak) and it stands at least el_min_rad above the prior's horizon; epoch_offset_s is half the search's span; a
    converged solution whose residuals' rms is above max_resid_m (a wrong millisecond is 300 km) is flagged RESID, not FIX"""
    cfg = np.zeros(1, WSNAP_CFG_DTYPE)
    for name, v in (("el_min_rad", el_min_rad), ("epoch_offset_s", epoch_offset_s), ("max_resid_m", max_resid_m), ("det_num", det[0]),
                    ("det_den", det[1]), ("min_peak", min_peak), ("min_sats", min_sats)):
        cfg[name] = v
    if ion is not None:
        cfg["ion"][0] = ion
    return cfg


def wsnap_prior(rr, week, tow_s) -> np.ndarray:
    """gpsx_wsnap_prior_t records with HAVE from rr [n, 3] (ECEF, m), the GPS week and the time of week of the search's first sample"""
    rr = np.asarray(rr, np.float64).reshape(-1, 3)
    out = np.zeros(len(rr), WSNAP_PRIOR_DTYPE)
    out["flags"], out["week"], out["rr"], out["tow_s"] = WSNAP_PRIOR_HAVE, week, rr, tow_s
    return out


# gpsx_wtow_cfg_t / gpsx_wtow_t / gpsx_wtow_rx_t (time-of-week aiding of the observable states from gpsx_wpred's records)
(WTOW_NO_PRED, WTOW_EMPTY, WTOW_UNLISTED, WTOW_BAD, WTOW_WAITING, WTOW_STALE, WTOW_UNCERTAIN, WTOW_INCONSISTENT, WTOW_OFF_GRID, WTOW_REARMED,
 WTOW_SHIFTED, WTOW_AIDED, WTOW_AGREES, WTOW_DISAGREES) = (1 << i for i in range(14))
WTOW_RX_NO_PRED, WTOW_RX_AIDED, WTOW_RX_SHIFTED, WTOW_RX_DISAGREES, WTOW_RX_OFF_GRID, WTOW_RX_REARMED = 1, 2, 4, 8, 16, 32
WTOW_CFG_DTYPE = np.dtype([("max_sigma_m", "<f8"), ("max_resid_samples", "<f4"), ("ch_per_rx", "<i4"), ("max_age_blocks", "<i4"), ("resolve", "<i4"),
                           ("rearm", "<i4"), ("reserved", "<i4")])
WTOW_DTYPE = np.dtype([("flags", "<u4"), ("prn_index", "<i4"), ("tx_ms", "<i8"), ("resid", "<f4"), ("m", "<i4"), ("shift", "<i4"), ("zero", "<u4")])
WTOW_RX_DTYPE = np.dtype([("flags", "<u2"), ("n_aided", "u1"), ("n_agrees", "u1"), ("n_disagrees", "u1"), ("n_off_grid", "u1"), ("n_shifted", "u1"),
                          ("n_inconsistent", "u1"), ("aided_mask", "<u8"), ("agrees_mask", "<u8"), ("disagrees_mask", "<u8"), ("off_grid_mask", "<u8"),
                          ("shifted_mask", "<u8"), ("inconsistent_mask", "<u8"), ("valid_after_mask", "<u8")])
assert WTOW_CFG_DTYPE.itemsize == 32 and WTOW_DTYPE.itemsize == 32 and WTOW_RX_DTYPE.itemsize == 64


def wtow_cfg(ch_per_rx: int, max_sigma_m: float = 300.0, max_resid_samples: float = 8.0, max_age_blocks: int = 40, resolve: int = 1,
             rearm: int = 0) -> np.ndarray:
    """a gpsx_wtow_cfg_t as a one-element WTOW_CFG_DTYPE array: a slot's time of week is anchored from a prediction known to max_sigma_m
    (one sigma) whose code phase lies within max_resid_samples of the loop's, that no older than max_age_blocks; resolve 1 moves the
    edge block of an AMBIGUOUS chain where the prediction says so, rearm 1 sends a slot whose bit edge is off the 20 ms grid back to
    its search"""
    cfg = np.zeros(1, WTOW_CFG_DTYPE)
    for name, v in (("max_sigma_m", max_sigma_m), ("max_resid_samples", max_resid_samples), ("ch_per_rx", ch_per_rx),
                    ("max_age_blocks", max_age_blocks), ("resolve", resolve), ("rearm", rearm)):
        cfg[name] = v
    return cfg


# gpsx_walm_cfg_t / gpsx_walm_slot_t / gpsx_walm_bank_t / gpsx_walm_rx_t / gpsx_walm_sv_t (almanac, ionosphere and UTC from subframes 4, 5)
WALM_IONUTC, WALM_PAGE25 = 1, 2
WALM_HELD, WALM_WEEK, WALM_HEALTHY, WALM_NEW = 1, 2, 4, 8
WALM_ENTRIES = 34
WALM_CFG_DTYPE = np.dtype([("ch_per_rx", "<i4"), ("reserved", "<i4", (3,))])
WALM_SLOT_DTYPE = np.dtype([("blocks_seen", "<i8"), ("last_word_end_p1", "<i8"), ("cur", "<u4", (8,)), ("cur_mask", "<u4"), ("cur_next", "<u4"),
                            ("cur_id", "<u4"), ("reserved", "<u4")])
WALM_BANK_DTYPE = np.dtype([("page", "<u4", (WALM_ENTRIES, 8)), ("have_mask", "<u8"), ("n_stored", "<u4"), ("n_changed", "<u4"), ("n_other", "<u4"),
                            ("reserved", "<u4", (3,))])
WALM_RX_DTYPE = np.dtype([("flags", "<u4"), ("n_stored", "<u4"), ("have_mask", "<u8"), ("new_mask", "<u8"), ("seen_mask", "<u8"), ("healthy_mask", "<u4"),
                          ("week_mask", "<u4"), ("p25_unhealthy_mask", "<u4"), ("toa_s", "<i4"), ("wna", "<i4"), ("tot_s", "<i4"), ("wnt", "<i4"),
                          ("dt_ls", "<i4"), ("wn_lsf", "<i4"), ("dn", "<i4"), ("dt_lsf", "<i4"), ("reserved", "<u4"), ("A0", "<f8"), ("A1", "<f8"),
                          ("ion", "<f8", (8,))])
WALM_SV_DOUBLES = ("toas", "e", "A", "i0", "OMG0", "omg", "M0", "OMGd", "f0", "f1")
WALM_SV_DTYPE = np.dtype([("flags", "<u4"), ("svid", "<i4"), ("svh", "<i4"), ("week", "<i4")] + [(k, "<f8") for k in WALM_SV_DOUBLES])
assert (WALM_CFG_DTYPE.itemsize, WALM_SLOT_DTYPE.itemsize, WALM_BANK_DTYPE.itemsize, WALM_RX_DTYPE.itemsize, WALM_SV_DTYPE.itemsize) == (16, 64, 1120, 160, 96)


def walm_cfg(ch_per_rx: int) -> np.ndarray:
    """a gpsx_walm_cfg_t as a one-element WALM_CFG_DTYPE array"""
    cfg = np.zeros(1, WALM_CFG_DTYPE)
    cfg["ch_per_rx"] = ch_per_rx
    return cfg


def walm_to_eph(rec) -> np.ndarray:
    """one WALM_SV_DTYPE record with WALM_HELD and WALM_WEEK -> a WEPH_FLAG_VALID WEPH_DTYPE [1] record of the almanac orbit (weph_to_eph
    and the solvers then evaluate it unchanged); GpsxError without the two flags.  Host only."""
    rec = np.ascontiguousarray(rec, WALM_SV_DTYPE).reshape(-1)
    if len(rec) != 1:
        raise GpsxError("walm_to_eph takes one record")
    out = np.zeros(1, WEPH_DTYPE)
    rc = load_library().gpsx_walm_to_eph(rec.ctypes.data, out.ctypes.data)
    if rc != 0:
        raise GpsxError(f"gpsx_walm_to_eph -> {rc}: the record is not HELD with WEEK")
    return out


def walm_gps_minus_utc(rx, week: int, tow_s: float) -> float:
    """GPS - UTC in seconds at GPS week `week`, second tow_s, from one WALM_RX_DTYPE record with WALM_IONUTC; GpsxError without it, with
    a day number outside 1 .. 7 or a tow_s that is not finite.  Host only."""
    rx = np.ascontiguousarray(rx, WALM_RX_DTYPE).reshape(-1)
    if len(rx) != 1:
        raise GpsxError("walm_gps_minus_utc takes one record")
    dt = C.c_double(0.0)
    rc = load_library().gpsx_walm_gps_minus_utc(rx.ctypes.data, int(week), float(tow_s), C.byref(dt))
    if rc != 0:
        raise GpsxError(f"gpsx_walm_gps_minus_utc -> {rc}: no page 18, a day number outside 1..7 or a time that is not finite")
    return dt.value


# gpsx_acq_window_t / gpsx_acq_window_rep_t (the weighted grid in a window around each of gpsx_wpred's predictions)
ACQ_WINDOW_SEARCHED, ACQ_WINDOW_SKIPPED, ACQ_WINDOW_BAD, ACQ_WINDOW_OFF_LATTICE, ACQ_WINDOW_CLIPPED = 1, 2, 4, 8, 16
ACQ_WINDOW_CFG_DTYPE = np.dtype([("n_coh", "<i4"), ("n_seg", "<i4"), ("half_width", "<i4"), ("half_bins", "<i4"), ("guard", "<i4"),
                                 ("need_flags", "<u4"), ("skip_flags", "<u4"), ("reserved", "<i4")])
ACQ_WINDOW_REP_DTYPE = np.dtype([("flags", "<u4"), ("first_bin", "<i4"), ("n_bins", "<i4"), ("centre", "<i4")])
assert ACQ_WINDOW_CFG_DTYPE.itemsize == 32 and ACQ_WINDOW_REP_DTYPE.itemsize == 16


def acq_window_cfg(n_coh: int, n_seg: int, half_width: int, half_bins: int, guard: int, need_flags: int = WPRED_PREDICTED | WPRED_VISIBLE,
                   skip_flags: int = WPRED_TRACKED | WPRED_ASSIGNED) -> np.ndarray:
    """a gpsx_acq_window_t as a one-element ACQ_WINDOW_CFG_DTYPE array: n_seg coherent segments of n_coh blocks, the half_width samples
    and half_bins Doppler bins either side of each prediction that has need_flags and none of skip_flags; phases within guard of the
    peak do not count as noise"""
    cfg = np.zeros(1, ACQ_WINDOW_CFG_DTYPE)
    for name, v in (("n_coh", n_coh), ("n_seg", n_seg), ("half_width", half_width), ("half_bins", half_bins), ("guard", guard),
                    ("need_flags", need_flags), ("skip_flags", skip_flags)):
        cfg[name] = v
    return cfg


def wlock_cfg(epoch_search, epoch_lock, code_min, car_min, snr_min, n_good, n_bad, rearm=0, patience=0) -> np.ndarray:
    """a gpsx_wlock_cfg_t as a one-element WLOCK_CFG_DTYPE array"""
    cfg = np.zeros(1, WLOCK_CFG_DTYPE)
    for name, v in (("epoch_search", epoch_search), ("epoch_lock", epoch_lock), ("code_min", code_min), ("car_min", car_min), ("snr_min", snr_min),
                    ("n_good", n_good), ("n_bad", n_bad), ("rearm", rearm), ("patience", patience)):
        cfg[name] = v
    return cfg


def wlock_cn0_dbhz(lock: np.ndarray, n_coh_lock: int) -> np.ndarray:
    """WLOCK_DTYPE records of one launch -> C/N0 in dB-Hz, float32 [n]: 10 log10(snr / (n_coh_lock ms)) where the newest epoch was a
    LOCKED one with snr > 0, else 0.  Host only."""
    lock = np.ascontiguousarray(lock, WLOCK_DTYPE).reshape(-1)
    out = np.zeros(len(lock), np.float32)
    rc = load_library().gpsx_wlock_cn0_dbhz(lock.ctypes.data, len(lock), int(n_coh_lock), out.ctypes.data)
    if rc != 0:
        raise GpsxError(f"gpsx_wlock_cn0_dbhz -> {rc}: no records, or n_coh_lock outside 1 .. 20")
    return out


TRK_DTYPE = np.dtype([("prn", "<i4"), ("code_phase_fine", "<f4"), ("if_freq_offset_hz", "<f4"),
                      ("if_freq_accum", "<u4")])
JOB_DTYPE = np.dtype([("block", "<i4"), ("n_ms", "<i4"), ("prn", "<i4"), ("freq_hz", "<f4"), ("offset_bits", "<i4"),
                      ("win_start", "<i4"), ("win_stop", "<i4")])


class AcqGrid(C.Structure):
    _fields_ = [("n_search", C.c_int32), ("n_ms", C.c_int32), ("search_stride_blocks", C.c_int32),
                ("n_prn", C.c_int32), ("prns", C.c_void_p), ("dopp_min_hz", C.c_int32), ("dopp_step_hz", C.c_int32),
                ("n_dopp", C.c_int32), ("phase_mode", C.c_int32), ("win_start", C.c_int32), ("win_stop", C.c_int32),
                ("shard_index", C.c_int32), ("shard_count", C.c_int32)]


class Config(C.Structure):   # gpsx_config_t
    _fields_ = [("sample_rate_hz", C.c_uint32), ("if_hz", C.c_int32)]


class AcqWeightedT(C.Structure):          # gpsx_acq_weighted_t
    _fields_ = [("n_search", C.c_int32), ("search_stride_blocks", C.c_int32), ("n_prn", C.c_int32), ("prns", C.POINTER(C.c_uint8)),
                ("dopp_min_hz", C.c_int32), ("dopp_step_hz", C.c_int32), ("n_dopp", C.c_int32), ("weights", C.c_int32)]


class GpsxError(RuntimeError):
    pass


CAPTURE_BLOCK_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_long)   # gpsx_capture_block_fn


def load_library(lab: bool | None = None) -> C.CDLL:
    """lib/libgpsx.so -- or, lab=True (or $GPSX_USE_LAB_LIBRARY=1 when lab is None): lib/libgpsx_lab.so, the same sources
    built with -DGPSX_LAB, the only build that reads the $GPSX_ACQ_* / $GPSX_TRACK_WAVE_FROM knobs forcing a kernel form."""
    if lab is None:
        lab = os.environ.get("GPSX_USE_LAB_LIBRARY") == "1"
    path = LAB_LIB_PATH if lab else LIB_PATH
    if os.environ.get("GPSX_LIB_PATH") and not lab:
        path = os.environ["GPSX_LIB_PATH"]      # another build of the product sources, e.g. lib/libgpsx_asan.so (tools/run_sanitizers.sh)
    if not os.path.exists(path):
        raise GpsxError(f"{path} is missing: run `python -m stm32f4_sdr_gps_amd.build` (needs hipcc)")
    lib = C.CDLL(path)
    assert lib.gpsx_is_lab_build() == (1 if lab else 0)
    lib.gpsx_last_error.restype = C.c_char_p
    lib.gpsx_strerror.restype = C.c_char_p
    lib.gpsx_last_kernel.restype = C.c_char_p
    lib.gpsx_last_kernel.argtypes = [C.c_void_p]
    lib.gpsx_acq_peaks_count.restype = C.c_size_t
    lib.gpsx_acq_keys_count.restype = C.c_size_t
    lib.gpsx_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_void_p]
    lib.gpsx_destroy.argtypes = [C.c_void_p]
    for name in ("gpsx_synchronize",):
        getattr(lib, name).argtypes = [C.c_void_p]
    lib.gpsx_last_error.argtypes = [C.c_void_p]
    lib.gpsx_malloc.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_size_t]
    lib.gpsx_free.argtypes = [C.c_void_p, C.c_void_p]
    lib.gpsx_host_alloc.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_size_t]
    lib.gpsx_bind_thread_to_device.argtypes = [C.c_void_p]
    lib.gpsx_host_free.argtypes = [C.c_void_p, C.c_void_p]
    lib.gpsx_memcpy_h2d.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    lib.gpsx_memcpy_d2h.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    lib.gpsx_event_create.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    lib.gpsx_event_record.argtypes = [C.c_void_p, C.c_void_p]
    lib.gpsx_event_elapsed_ms.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]
    lib.gpsx_event_destroy.argtypes = [C.c_void_p, C.c_void_p]
    lib.gpsx_device_info.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.gpsx_ca_codes.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.gpsx_acq_grid_dev.argtypes = [C.c_void_p, C.POINTER(AcqGrid), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p]
    lib.gpsx_acq_grid.argtypes = [C.c_void_p, C.POINTER(AcqGrid), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.gpsx_acq_grid_async.argtypes = lib.gpsx_acq_grid.argtypes
    lib.gpsx_acq_jobs.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.gpsx_track_epl_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.gpsx_track_epl_batch_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.gpsx_track_epl_batch_chunked.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                                 TRACK_CHUNK_FN, C.c_void_p]
    lib.gpsx_rewind.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.gpsx_track_loop.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p]
    lib.gpsx_track_loop_dev.argtypes = lib.gpsx_track_loop.argtypes
    lib.gpsx_loop_set_polarity.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    lib.gpsx_loop_reset_code_filter.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    lib.gpsx_loop_set_schedule.argtypes = [C.c_void_p, C.c_int]
    lib.gpsx_loop_set_word_sync.argtypes = [C.c_void_p, C.c_int]
    lib.gpsx_loop_set_draws.argtypes = [C.c_void_p, C.c_int]
    lib.gpsx_set_acq_path.argtypes = [C.c_void_p, C.c_int]
    lib.gpsx_acq_grid_weighted.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.gpsx_acq_grid_weighted_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.gpsx_acq_grid_weighted_ms.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    lib.gpsx_acq_grid_weighted_ms_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    lib.gpsx_acq_grid_weighted_coh.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    lib.gpsx_acq_grid_weighted_coh_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    lib.gpsx_acq_grid_weighted_hyb.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    lib.gpsx_acq_grid_weighted_hyb_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    lib.gpsx_track_epl_weighted.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    lib.gpsx_track_epl_weighted_dev.argtypes = lib.gpsx_track_epl_weighted.argtypes
    lib.gpsx_track_loop_weighted.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    lib.gpsx_track_loop_weighted_dev.argtypes = lib.gpsx_track_loop_weighted.argtypes
    lib.gpsx_track_loop_weighted_sync.argtypes = lib.gpsx_track_loop_weighted.argtypes
    lib.gpsx_track_loop_weighted_sync_dev.argtypes = lib.gpsx_track_loop_weighted.argtypes
    lib.gpsx_track_loop_weighted_aided.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    lib.gpsx_track_loop_weighted_aided_dev.argtypes = lib.gpsx_track_loop_weighted_aided.argtypes
    lib.gpsx_track_loop_weighted_sync_aided.argtypes = lib.gpsx_track_loop_weighted_aided.argtypes
    lib.gpsx_track_loop_weighted_sync_aided_dev.argtypes = lib.gpsx_track_loop_weighted_aided.argtypes
    lib.gpsx_track_loop_weighted_sync_multi.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.gpsx_track_loop_weighted_sync_multi_dev.argtypes = lib.gpsx_track_loop_weighted_sync_multi.argtypes
    lib.gpsx_wobs_pseudoranges_rx.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.gpsx_wnav_words.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    lib.gpsx_wnav_words_dev.argtypes = lib.gpsx_wnav_words.argtypes
    lib.gpsx_wnav_subframe_image.argtypes = [C.c_void_p, C.c_void_p]
    lib.gpsx_wobs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.gpsx_wobs_dev.argtypes = lib.gpsx_wobs.argtypes
    lib.gpsx_wobs_pseudoranges.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.POINTER(C.c_double)]
    lib.gpsx_weph.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    lib.gpsx_weph_dev.argtypes = lib.gpsx_weph.argtypes
    lib.gpsx_weph_to_eph.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.gpsx_wlock.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.gpsx_wlock_dev.argtypes = lib.gpsx_wlock.argtypes
    lib.gpsx_wfix.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.gpsx_wfix_dev.argtypes = lib.gpsx_wfix.argtypes
    lib.gpsx_wfde.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.gpsx_wfde_dev.argtypes = lib.gpsx_wfde.argtypes
    lib.gpsx_wvel.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.gpsx_wvel_dev.argtypes = lib.gpsx_wvel.argtypes
    lib.gpsx_wkf.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                             C.c_void_p]
    lib.gpsx_wkf_dev.argtypes = lib.gpsx_wkf.argtypes
    lib.gpsx_wacq.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                              C.c_void_p]
    lib.gpsx_wacq_dev.argtypes = lib.gpsx_wacq.argtypes
    lib.gpsx_wbank.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.gpsx_wbank_dev.argtypes = lib.gpsx_wbank.argtypes
    lib.gpsx_wpred.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.gpsx_wpred_dev.argtypes = lib.gpsx_wpred.argtypes
    lib.gpsx_wtow.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                              C.c_void_p, C.c_void_p]
    lib.gpsx_wtow_dev.argtypes = lib.gpsx_wtow.argtypes
    lib.gpsx_walm.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.gpsx_walm_dev.argtypes = lib.gpsx_walm.argtypes
    lib.gpsx_walm_to_eph.argtypes = [C.c_void_p, C.c_void_p]
    lib.gpsx_walm_gps_minus_utc.argtypes = [C.c_void_p, C.c_int, C.c_double, C.POINTER(C.c_double)]
    lib.gpsx_wsnap.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.gpsx_wsnap_dev.argtypes = lib.gpsx_wsnap.argtypes
    lib.gpsx_wsnap_to_fix.argtypes = [C.c_void_p, C.c_void_p]
    lib.gpsx_acq_window_weighted.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.gpsx_acq_window_weighted_dev.argtypes = lib.gpsx_acq_window_weighted.argtypes
    lib.gpsx_wlock_cn0_dbhz.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.gps_tracking_words_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_int]
    lib.gpsx_loop_state_from_channel.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    lib.gpsx_loop_state_from_channel.restype = None
    lib.gpsx_loop_state_to_channel.argtypes = [C.c_void_p, C.c_void_p]
    lib.gpsx_loop_state_to_channel.restype = None
    lib.gpsx_wipeoff.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.POINTER(C.c_uint32), C.c_void_p, C.c_void_p]
    lib.gpsx_replica.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_void_p]
    lib.gpsx_corr_offsets.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                      C.c_void_p, C.c_void_p, C.c_void_p]
    lib.gpsx_set_if_format.argtypes = [C.c_void_p, C.c_int]
    lib.gpsx_config_default.argtypes = [C.POINTER(Config)]
    lib.gpsx_config_default.restype = None
    lib.gpsx_set_config.argtypes = [C.c_void_p, C.POINTER(Config)]
    lib.gpsx_get_config.argtypes = [C.c_void_p, C.POINTER(Config)]
    lib.gpsx_if_unpack2.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.gpsx_mag8.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.gpsx_corr_search.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_void_p]
    # in-process multi-GPU group
    lib.gpsx_group_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_void_p)]
    lib.gpsx_group_destroy.argtypes = [C.c_void_p]
    lib.gpsx_group_destroy.restype = None
    lib.gpsx_acq_grid_sharded.argtypes = [C.c_void_p, C.POINTER(AcqGrid), C.POINTER(C.c_void_p), C.c_int,
                                          C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    # capture ring (IF ingest)
    lib.gpsx_capture_create.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
    lib.gpsx_capture_destroy.argtypes = [C.c_void_p]
    lib.gpsx_capture_destroy.restype = None
    lib.gpsx_capture_write_slot.argtypes = [C.c_void_p]
    lib.gpsx_capture_write_slot.restype = C.c_void_p
    lib.gpsx_capture_commit.argtypes = [C.c_void_p]
    lib.gpsx_capture_push.argtypes = [C.c_void_p, C.c_void_p]
    lib.gpsx_capture_ready_buf.argtypes = [C.c_void_p]
    lib.gpsx_capture_ready_buf.restype = C.c_void_p
    lib.gpsx_capture_window_dev.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
    lib.gpsx_capture_packet_cnt.argtypes = [C.c_void_p]
    lib.gpsx_capture_packet_cnt.restype = C.c_uint32
    lib.gpsx_capture_block_bytes.argtypes = [C.c_void_p]
    lib.gpsx_capture_block_bytes.restype = C.c_size_t
    lib.gpsx_capture_replay_file.argtypes = [C.c_void_p, C.c_char_p, C.c_long, C.c_long, CAPTURE_BLOCK_FN, C.c_void_p]
    lib.gpsx_capture_replay_file.restype = C.c_long
    for name in ("signal_capture_get_ready_buf", "signal_capture_get_copy_buf"):
        getattr(lib, name).restype = C.c_void_p
    for name in ("signal_capture_have_irq", "signal_capture_check_copied"):
        getattr(lib, name).restype = C.c_uint8
    lib.signal_capture_get_packet_cnt.restype = C.c_uint32
    lib.gpsx_compat_capture_push.argtypes = [C.c_void_p]
    lib.gpsx_compat_capture_push.restype = None
    # compat (reference names)
    lib.gps_generate_prn.argtypes = [C.c_void_p, C.c_int]
    lib.gps_channell_prepare.argtypes = [C.c_void_p]
    lib.gps_correlation8.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint16]
    lib.gps_correlation8.restype = C.c_int16
    lib.gps_correlation_iq.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint16, C.POINTER(C.c_int16),
                                       C.POINTER(C.c_int16)]
    lib.correlation_search.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint16, C.c_uint16,
                                       C.POINTER(C.c_uint16), C.POINTER(C.c_uint16)]
    lib.correlation_search.restype = C.c_uint16
    lib.gps_shift_to_zero_freq.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float]
    lib.gps_shift_to_zero_freq_track.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.gps_generate_prn_data2.argtypes = [C.c_void_p, C.c_void_p, C.c_uint16]
    lib.gps_rewind_if_phase.argtypes = [C.c_void_p, C.c_uint8]
    return lib


def _ptr(a):
    return None if a is None else a.ctypes.data


class Engine:
    """One gpsx context.  `stream` may be a raw hipStream_t handle (int), e.g. torch.cuda.current_stream().cuda_stream."""

    def __init__(self, device: int = 0, stream: int | None = None, lab: bool | None = None):
        self.lib = load_library(lab)
        h = C.c_void_p()
        rc = self.lib.gpsx_create(C.byref(h), device, C.c_void_p(stream) if stream else None)
        if rc != 0:
            raise GpsxError(f"gpsx_create(device={device}) -> {rc}: {self.lib.gpsx_strerror(rc).decode()} "
                            "(the correlator engine needs an MI355X; it has no CPU path)")
        self.h = h
        self.block_bytes = BYTES_PER_MS

    def close(self):
        if getattr(self, "h", None):
            for p in getattr(self, "_pinned", []):
                self.lib.gpsx_host_free(self.h, C.c_void_p(p))
            self._pinned = []
            self.lib.gpsx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc != 0:
            raise GpsxError(f"{what} -> {rc}: {self.lib.gpsx_strerror(rc).decode()}: "
                            f"{self.lib.gpsx_last_error(self.h).decode()}")

    # -- plumbing ----------------------------------------------------------------------------------------------
    def device_info(self):
        name = C.create_string_buffer(128)
        cus, khz = C.c_int(), C.c_int()
        self.lib.gpsx_device_info(self.h, name, 128, C.byref(cus), C.byref(khz))
        return name.value.decode(), cus.value, khz.value

    def synchronize(self):
        self._chk(self.lib.gpsx_synchronize(self.h), "gpsx_synchronize")

    def malloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        self._chk(self.lib.gpsx_malloc(self.h, C.byref(p), nbytes), "gpsx_malloc")
        return p.value

    def bind_thread_to_device(self) -> bool:
        """Pin the calling thread to the CPUs local to this context's GPU; False when the topology is not exposed."""
        return self.lib.gpsx_bind_thread_to_device(self.h) == 0

    def host_array(self, shape, dtype) -> np.ndarray:
        """A numpy array in page-locked host memory (gpsx_host_alloc); lives until the engine is closed."""
        dtype = np.dtype(dtype)
        n = int(np.prod(shape)) * dtype.itemsize
        p = C.c_void_p()
        self._chk(self.lib.gpsx_host_alloc(self.h, C.byref(p), max(n, 1)), "gpsx_host_alloc")
        self._pinned = getattr(self, "_pinned", [])
        self._pinned.append(p.value)
        buf = (C.c_ubyte * max(n, 1)).from_address(p.value)
        return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def free(self, dptr: int):
        self._chk(self.lib.gpsx_free(self.h, dptr), "gpsx_free")

    def h2d(self, dptr: int, arr: np.ndarray):
        arr = np.ascontiguousarray(arr)
        self._chk(self.lib.gpsx_memcpy_h2d(self.h, dptr, arr.ctypes.data, arr.nbytes), "gpsx_memcpy_h2d")

    def d2h(self, arr: np.ndarray, dptr: int):
        assert arr.flags.c_contiguous
        self._chk(self.lib.gpsx_memcpy_d2h(self.h, arr.ctypes.data, dptr, arr.nbytes), "gpsx_memcpy_d2h")

    def event(self) -> int:
        e = C.c_void_p()
        self._chk(self.lib.gpsx_event_create(self.h, C.byref(e)), "gpsx_event_create")
        return e.value

    def record(self, ev: int):
        self._chk(self.lib.gpsx_event_record(self.h, ev), "gpsx_event_record")

    def elapsed_ms(self, ev0: int, ev1: int) -> float:
        ms = C.c_float()
        self._chk(self.lib.gpsx_event_elapsed_ms(self.h, ev0, ev1, C.byref(ms)), "gpsx_event_elapsed_ms")
        return ms.value

    # -- receiver constants (gpsx_config_t) ---------------------------------------------------------------------
    def get_config(self) -> Config:
        cfg = Config()
        self._chk(self.lib.gpsx_get_config(self.h, C.byref(cfg)), "gpsx_get_config")
        return cfg

    def set_config(self, if_hz: int = IF_HZ, sample_rate_hz: int = 16368000):
        cfg = Config(sample_rate_hz, if_hz)
        self._chk(self.lib.gpsx_set_config(self.h, C.byref(cfg)), "gpsx_set_config")

    # -- IF sample format (N3 ingest) ---------------------------------------------------------------------------
    def set_if_format(self, fmt: int):
        self._chk(self.lib.gpsx_set_if_format(self.h, fmt), "gpsx_set_if_format")
        self.block_bytes = BYTES_PER_MS_2BIT if fmt == IF_2BIT_SM else BYTES_PER_MS

    def if_unpack2(self, if_2bit: np.ndarray):
        blocks = np.ascontiguousarray(if_2bit, np.uint8).reshape(-1, BYTES_PER_MS_2BIT)
        sign = np.zeros((len(blocks), BYTES_PER_MS), np.uint8)
        mag = np.zeros((len(blocks), BYTES_PER_MS), np.uint8)
        self._chk(self.lib.gpsx_if_unpack2(self.h, blocks.ctypes.data, len(blocks), sign.ctypes.data, mag.ctypes.data),
                  "gpsx_if_unpack2")
        return sign, mag

    # -- K1 ---------------------------------------------------------------------------------------------------
    def ca_codes(self, prns) -> np.ndarray:
        prns = np.ascontiguousarray(prns, np.uint8)
        out = np.zeros((len(prns), 1023), np.uint8)
        self._chk(self.lib.gpsx_ca_codes(self.h, prns.ctypes.data, len(prns), out.ctypes.data), "gpsx_ca_codes")
        return out

    # -- acquisition ------------------------------------------------------------------------------------------
    @staticmethod
    def grid_desc(prns: np.ndarray, n_search=1, n_ms=1, search_stride_blocks=None, dopp_min_hz=-5000,
                  dopp_step_hz=500, n_dopp=21, phase_mode=PHASES_FINE, win=(0, 2046), shard=(0, 1)) -> AcqGrid:
        g = AcqGrid()
        g.n_search, g.n_ms = n_search, n_ms
        g.search_stride_blocks = n_ms if search_stride_blocks is None else search_stride_blocks
        g.n_prn, g.prns = len(prns), prns.ctypes.data
        g.dopp_min_hz, g.dopp_step_hz, g.n_dopp = dopp_min_hz, dopp_step_hz, n_dopp
        g.phase_mode = phase_mode
        g.win_start, g.win_stop = win
        g.shard_index, g.shard_count = shard
        return g

    def acq_grid(self, if_blocks: np.ndarray, prns, want_keys=True, **kw):
        """Host-buffer grid search.  Returns (peaks[n_search, n_prn, n_dopp, n_bits], keys[n_search, n_prn, n_dopp])."""
        prns = np.ascontiguousarray(prns, np.uint8)
        blocks = np.ascontiguousarray(if_blocks, np.uint8).reshape(-1, self.block_bytes)
        g = self.grid_desc(prns, **kw)
        n_bits = 8 if g.phase_mode == PHASES_FINE else 1
        peaks = np.zeros((g.n_search, g.n_prn, g.n_dopp, n_bits), PEAK_DTYPE)
        keys = np.zeros((g.n_search, g.n_prn, g.n_dopp), np.int64) if want_keys else None
        self._chk(self.lib.gpsx_acq_grid(self.h, C.byref(g), blocks.ctypes.data, len(blocks), peaks.ctypes.data,
                                         _ptr(keys)), "gpsx_acq_grid")
        return peaks, keys

    def acq_grid_debug(self, if_blocks: np.ndarray, prns, want_per_ms=False, want_energy=False, want_cnt=False, **kw):
        """Device-pointer path with the optional inspection outputs, staged through gpsx_malloc'ed buffers."""
        prns = np.ascontiguousarray(prns, np.uint8)
        blocks = np.ascontiguousarray(if_blocks, np.uint8).reshape(-1, BYTES_PER_MS)
        g = self.grid_desc(prns, **kw)
        n_bits = 8 if g.phase_mode == PHASES_FINE else 1
        shape = (g.n_search, g.n_prn, g.n_dopp, n_bits)
        peaks = np.zeros(shape, PEAK_DTYPE)
        keys = np.zeros(shape[:3], np.int64)
        per_ms = np.zeros(shape + (g.n_ms,), PEAK_DTYPE) if want_per_ms else None
        energy = np.zeros(shape + (2046,), np.uint32) if want_energy else None
        cnt = np.zeros(shape + (2046, 2), np.uint16) if want_cnt else None
        bufs = []

        def dev(arr):
            if arr is None:
                return None
            p = self.malloc(arr.nbytes)
            self.h2d(p, arr)
            bufs.append(p)
            return p

        try:
            d_if = dev(np.concatenate([blocks.reshape(-1), np.zeros(2, np.uint8)]))
            d_peaks, d_keys, d_per, d_en, d_cnt = dev(peaks), dev(keys), dev(per_ms), dev(energy), dev(cnt)
            self._chk(self.lib.gpsx_acq_grid_dev(self.h, C.byref(g), d_if, len(blocks), d_peaks, d_keys, d_per, d_en,
                                                 d_cnt), "gpsx_acq_grid_dev")
            self.synchronize()
            for arr, p in ((peaks, d_peaks), (keys, d_keys), (per_ms, d_per), (energy, d_en), (cnt, d_cnt)):
                if arr is not None:
                    self.d2h(arr, p)
        finally:
            for p in bufs:
                self.free(p)
        return dict(peaks=peaks, keys=keys, per_ms=per_ms, energy=energy, cnt=cnt)

    def acq_jobs(self, if_blocks: np.ndarray, jobs: np.ndarray, want_energy=False):
        blocks = np.ascontiguousarray(if_blocks, np.uint8).reshape(-1, self.block_bytes)
        jobs = np.ascontiguousarray(jobs, JOB_DTYPE)
        peaks = np.zeros(len(jobs), PEAK_DTYPE)
        energy = np.zeros((len(jobs), 2046), np.uint32) if want_energy else None
        self._chk(self.lib.gpsx_acq_jobs(self.h, jobs.ctypes.data, len(jobs), blocks.ctypes.data, len(blocks),
                                         peaks.ctypes.data, _ptr(energy)), "gpsx_acq_jobs")
        return peaks, energy

    # -- tracking ---------------------------------------------------------------------------------------------
    def track_epl(self, if_block: np.ndarray, states: np.ndarray, iq_out: np.ndarray | None = None) -> np.ndarray:
        """states: TRK_DTYPE array, updated in place (if_freq_accum).  Returns int16 [n_ch, 6] = IE,QE,IP,QP,IL,QL
        (written into iq_out when given, e.g. a page-locked array from host_array())."""
        assert states.dtype == TRK_DTYPE and states.flags.c_contiguous
        blk = np.ascontiguousarray(if_block, np.uint8)
        iq = np.zeros((len(states), 6), np.int16) if iq_out is None else iq_out
        self._chk(self.lib.gpsx_track_epl_batch(self.h, blk.ctypes.data, states.ctypes.data, len(states),
                                                iq.ctypes.data), "gpsx_track_epl_batch")
        return iq

    def track_epl_chunked(self, if_block: np.ndarray, states: np.ndarray, n_chunks: int, on_chunk,
                          iq_out: np.ndarray | None = None) -> np.ndarray:
        """track_epl in n_chunks pieces; on_chunk(first, n) is called on this thread as each piece's results land in
        `states` / the returned array while the GPU works on the next pieces (gpsx_track_epl_batch_chunked)."""
        assert states.dtype == TRK_DTYPE and states.flags.c_contiguous
        blk = np.ascontiguousarray(if_block, np.uint8)
        iq = np.zeros((len(states), 6), np.int16) if iq_out is None else iq_out
        assert iq.dtype == np.int16 and iq.flags.c_contiguous and iq.shape == (len(states), 6)
        raised = []

        def trampoline(user, first, n):   # (ctypes would print and swallow an exception raised inside the callback)
            if not raised:
                try:
                    on_chunk(first, n)
                except BaseException as exc:   # noqa: BLE001 -- re-raised below, on the caller's stack
                    raised.append(exc)

        cb = TRACK_CHUNK_FN(trampoline)
        rc = self.lib.gpsx_track_epl_batch_chunked(self.h, blk.ctypes.data, states.ctypes.data, len(states),
                                                   iq.ctypes.data, n_chunks, cb, None)
        if raised:
            raise raised[0]
        self._chk(rc, "gpsx_track_epl_batch_chunked")
        return iq

    def acq_grid_weighted(self, blocks_2bit: np.ndarray, prns, n_search: int, dopp_min_hz: int, dopp_step_hz: int, n_dopp: int,
                          use_magnitude: bool = True, stride_blocks: int = 1) -> np.ndarray:
        """EXTENSION (not in the reference): the acquisition grid on weighted two-bit samples -> PEAK_DTYPE [n_search, n_prn, n_dopp]"""
        blocks = np.ascontiguousarray(blocks_2bit, np.uint8).reshape(-1, BYTES_PER_MS_2BIT)
        prns = np.ascontiguousarray(prns, np.uint8)
        g = AcqWeightedT(n_search, stride_blocks, len(prns), prns.ctypes.data_as(C.POINTER(C.c_uint8)), dopp_min_hz, dopp_step_hz, n_dopp,
                         1 if use_magnitude else 0)
        peaks = np.zeros((n_search, len(prns), n_dopp), PEAK_DTYPE)
        self._chk(self.lib.gpsx_acq_grid_weighted(self.h, C.byref(g), blocks.ctypes.data, len(blocks), peaks.ctypes.data),
                  "gpsx_acq_grid_weighted")
        return peaks

    def acq_grid_weighted_ms(self, blocks_2bit: np.ndarray, prns, n_search: int, n_ms: int, dopp_min_hz: int, dopp_step_hz: int,
                             n_dopp: int, use_magnitude: bool = True, stride_blocks: int | None = None) -> np.ndarray:
        """EXTENSION: the weighted grid over n_ms blocks per search, magnitudes summed non-coherently (search s: blocks
        s * stride_blocks .. + n_ms - 1; the stride defaults to n_ms) -> PEAK_DTYPE [n_search, n_prn, n_dopp]"""
        blocks = np.ascontiguousarray(blocks_2bit, np.uint8).reshape(-1, BYTES_PER_MS_2BIT)
        prns = np.ascontiguousarray(prns, np.uint8)
        stride = n_ms if stride_blocks is None else stride_blocks
        g = AcqWeightedT(n_search, stride, len(prns), prns.ctypes.data_as(C.POINTER(C.c_uint8)), dopp_min_hz, dopp_step_hz, n_dopp,
                         1 if use_magnitude else 0)
        peaks = np.zeros((n_search, len(prns), n_dopp), PEAK_DTYPE)
        self._chk(self.lib.gpsx_acq_grid_weighted_ms(self.h, C.byref(g), n_ms, blocks.ctypes.data, len(blocks), peaks.ctypes.data),
                  "gpsx_acq_grid_weighted_ms")
        return peaks

    def acq_grid_weighted_coh(self, blocks_2bit: np.ndarray, prns, n_search: int, n_coh: int, dopp_min_hz: int, dopp_step_hz: int,
                              n_dopp: int, use_magnitude: bool = True, stride_blocks: int | None = None) -> np.ndarray:
        """EXTENSION: the weighted grid over n_coh blocks per search (1 .. 20), integrated coherently: I and Q summed over the
        blocks with the carrier NCO running on from block to block (search s: blocks s * stride_blocks .. + n_coh - 1; the
        stride defaults to n_coh) -> PEAK_DTYPE [n_search, n_prn, n_dopp]"""
        blocks = np.ascontiguousarray(blocks_2bit, np.uint8).reshape(-1, BYTES_PER_MS_2BIT)
        prns = np.ascontiguousarray(prns, np.uint8)
        stride = n_coh if stride_blocks is None else stride_blocks
        g = AcqWeightedT(n_search, stride, len(prns), prns.ctypes.data_as(C.POINTER(C.c_uint8)), dopp_min_hz, dopp_step_hz, n_dopp,
                         1 if use_magnitude else 0)
        peaks = np.zeros((n_search, len(prns), n_dopp), PEAK_DTYPE)
        self._chk(self.lib.gpsx_acq_grid_weighted_coh(self.h, C.byref(g), n_coh, blocks.ctypes.data, len(blocks), peaks.ctypes.data),
                  "gpsx_acq_grid_weighted_coh")
        return peaks

    def acq_grid_weighted_hyb(self, blocks_2bit: np.ndarray, prns, n_search: int, n_coh: int, n_seg: int, dopp_min_hz: int,
                              dopp_step_hz: int, n_dopp: int, use_magnitude: bool = True, stride_blocks: int | None = None) -> np.ndarray:
        """EXTENSION: the weighted grid over n_seg coherent windows of n_coh blocks each (1 .. 20 x 1 .. 128), the windows'
        magnitudes summed non-coherently (search s, window j: blocks s * stride_blocks + j * n_coh .. + n_coh - 1, the carrier
        NCO started from 0 at the window's first block; the stride defaults to n_coh * n_seg)
        -> PEAK_DTYPE [n_search, n_prn, n_dopp]"""
        blocks = np.ascontiguousarray(blocks_2bit, np.uint8).reshape(-1, BYTES_PER_MS_2BIT)
        prns = np.ascontiguousarray(prns, np.uint8)
        stride = n_coh * n_seg if stride_blocks is None else stride_blocks
        g = AcqWeightedT(n_search, stride, len(prns), prns.ctypes.data_as(C.POINTER(C.c_uint8)), dopp_min_hz, dopp_step_hz, n_dopp,
                         1 if use_magnitude else 0)
        peaks = np.zeros((n_search, len(prns), n_dopp), PEAK_DTYPE)
        self._chk(self.lib.gpsx_acq_grid_weighted_hyb(self.h, C.byref(g), n_coh, n_seg, blocks.ctypes.data, len(blocks),
                                                      peaks.ctypes.data), "gpsx_acq_grid_weighted_hyb")
        return peaks

    def track_epl_weighted(self, blocks_2bit: np.ndarray, states: np.ndarray, use_magnitude: bool = True, spacing: int = 8) -> np.ndarray:
        """EXTENSION: Early / Prompt / Late on weighted two-bit samples over the n_blocks consecutive 4092-byte blocks given, with
        the weighted grids' sample, carrier and replica definitions (a grid record hands over exactly: phase -> code_phase_fine,
        Doppler bin -> if_freq_offset_hz, accumulator 0 at the window's first block).  states: TRK_DTYPE array, updated in place
        (if_freq_accum advanced by n_blocks blocks).  Early and Late sit `spacing` samples (1 .. 15) around Prompt.
        -> int32 [n_blocks, n_ch, 6] = IE, QE, IP, QP, IL, QL"""
        assert states.dtype == TRK_DTYPE and states.flags.c_contiguous
        blocks = np.ascontiguousarray(blocks_2bit, np.uint8).reshape(-1, BYTES_PER_MS_2BIT)
        cfg = np.array([1 if use_magnitude else 0, spacing], np.int32)
        iq = np.zeros((len(blocks), len(states), 6), np.int32)
        self._chk(self.lib.gpsx_track_epl_weighted(self.h, cfg.ctypes.data, blocks.ctypes.data, len(blocks), states.ctypes.data,
                                                   len(states), iq.ctypes.data), "gpsx_track_epl_weighted")
        return iq

    def track_loop_weighted(self, blocks_2bit: np.ndarray, d_state: int, n_ch: int, n_coh: int, use_magnitude: bool = True,
                            spacing: int = 8, dll=(1.0, 300.0), pll=(4.0, 3000.0), fll: float = 0.0) -> np.ndarray:
        """EXTENSION: the closed DLL / Costas PLL / FLL on weighted two-bit samples over the n_blocks consecutive 4092-byte blocks
        given (a multiple of n_coh), on the n_ch WLOOP_STATE_DTYPE states at device address d_state: the loop is updated once per
        coherent window of n_coh blocks (1 .. 20).  dll / pll: the (c1, c2) gains of the PI forms, fll: the frequency loop's gain
        (0: none).  -> WLOOP_REC_DTYPE [n_blocks / n_coh, n_ch]"""
        blocks = np.ascontiguousarray(blocks_2bit, np.uint8).reshape(-1, BYTES_PER_MS_2BIT)
        cfg = wloop_cfg(n_coh, use_magnitude, spacing, dll, pll, fll)
        rec = np.zeros((len(blocks) // max(n_coh, 1), n_ch), WLOOP_REC_DTYPE)
        self._chk(self.lib.gpsx_track_loop_weighted(self.h, cfg.ctypes.data, blocks.ctypes.data, len(blocks), C.c_void_p(d_state), n_ch,
                                                    rec.ctypes.data), "gpsx_track_loop_weighted")
        return rec

    def track_loop_weighted_sync(self, blocks_2bit: np.ndarray, d_state: int, n_ch: int, cfg: np.ndarray) -> np.ndarray:
        """EXTENSION: the weighted loop with a 20 ms bit synchroniser per channel and bit-aligned windows over the n_blocks
        consecutive 4092-byte blocks given (any number from 1 to 4096: the open window lives in the state), on the n_ch
        WSYNC_STATE_DTYPE states at device address d_state.  cfg: wsync_cfg(...).  -> WSYNC_REC_DTYPE [slots, n_ch], slots =
        wsync_slots(n_blocks, n_coh_search, n_coh_lock); a slot without a window has end_block -1 and flags 0"""
        blocks = np.ascontiguousarray(blocks_2bit, np.uint8).reshape(-1, BYTES_PER_MS_2BIT)
        assert cfg.dtype == WSYNC_CFG_DTYPE and cfg.size == 1
        rec = np.zeros((wsync_slots(len(blocks), int(cfg["n_coh_search"][0]), int(cfg["n_coh_lock"][0])), n_ch), WSYNC_REC_DTYPE)
        self._chk(self.lib.gpsx_track_loop_weighted_sync(self.h, cfg.ctypes.data, blocks.ctypes.data, len(blocks), C.c_void_p(d_state),
                                                         n_ch, rec.ctypes.data), "gpsx_track_loop_weighted_sync")
        return rec

    def track_loop_weighted_aided(self, blocks_2bit: np.ndarray, d_state: int, n_ch: int, n_coh: int, code_per_hz: float = WAID_L1CA,
                                  use_magnitude: bool = True, spacing: int = 8, dll=(1.0, 300.0), pll=(4.0, 3000.0),
                                  fll: float = 0.0) -> np.ndarray:
        """EXTENSION: track_loop_weighted with carrier aiding of the code loop: per window the code phase also steps by
        -(code_per_hz * if_freq_offset_hz) * T, the offset the window ran with (code_per_hz 0: track_loop_weighted's bytes).
        -> WLOOP_REC_DTYPE [n_blocks / n_coh, n_ch]"""
        blocks = np.ascontiguousarray(blocks_2bit, np.uint8).reshape(-1, BYTES_PER_MS_2BIT)
        cfg, aid = wloop_cfg(n_coh, use_magnitude, spacing, dll, pll, fll), waid(code_per_hz)
        rec = np.zeros((len(blocks) // max(n_coh, 1), n_ch), WLOOP_REC_DTYPE)
        self._chk(self.lib.gpsx_track_loop_weighted_aided(self.h, cfg.ctypes.data, aid.ctypes.data, blocks.ctypes.data, len(blocks),
                                                          C.c_void_p(d_state), n_ch, rec.ctypes.data), "gpsx_track_loop_weighted_aided")
        return rec

    def track_loop_weighted_sync_aided(self, blocks_2bit: np.ndarray, d_state: int, n_ch: int, cfg: np.ndarray,
                                       code_per_hz: float = WAID_L1CA) -> np.ndarray:
        """EXTENSION: track_loop_weighted_sync with carrier aiding of the code loop (as track_loop_weighted_aided; the same factor in
        SEARCH and LOCKED windows, no step in WAIT).  -> WSYNC_REC_DTYPE [slots, n_ch]"""
        blocks = np.ascontiguousarray(blocks_2bit, np.uint8).reshape(-1, BYTES_PER_MS_2BIT)
        assert cfg.dtype == WSYNC_CFG_DTYPE and cfg.size == 1
        aid = waid(code_per_hz)
        rec = np.zeros((wsync_slots(len(blocks), int(cfg["n_coh_search"][0]), int(cfg["n_coh_lock"][0])), n_ch), WSYNC_REC_DTYPE)
        self._chk(self.lib.gpsx_track_loop_weighted_sync_aided(self.h, cfg.ctypes.data, aid.ctypes.data, blocks.ctypes.data, len(blocks),
                                                               C.c_void_p(d_state), n_ch, rec.ctypes.data), "gpsx_track_loop_weighted_sync_aided")
        return rec

    def track_loop_weighted_sync_multi(self, streams_2bit: np.ndarray, d_state: int, ch_per_rx: int, cfg: np.ndarray,
                                       code_per_hz: float | None = None) -> np.ndarray:
        """EXTENSION: track_loop_weighted_sync(_aided) for n_rx receivers in one launch, one IF stream each: streams_2bit is uint8
        [n_rx, n_blocks, 4092]; the n_rx * ch_per_rx WSYNC_STATE_DTYPE states at device address d_state, channel r * ch_per_rx + j
        slot j of receiver r (a slot without a satellite: prn = PRN_NONE).  code_per_hz None: unaided.
        -> WSYNC_REC_DTYPE [slots, n_rx * ch_per_rx], receiver r's columns the single-stream call's on its stream"""
        streams = np.ascontiguousarray(streams_2bit, np.uint8)
        assert streams.ndim == 3 and streams.shape[2] == BYTES_PER_MS_2BIT and cfg.dtype == WSYNC_CFG_DTYPE and cfg.size == 1
        n_rx, n_blocks = streams.shape[:2]
        rx, aid = wmulti(n_rx, ch_per_rx, n_blocks), (None if code_per_hz is None else waid(code_per_hz))
        rec = np.zeros((wsync_slots(n_blocks, int(cfg["n_coh_search"][0]), int(cfg["n_coh_lock"][0])), n_rx * ch_per_rx), WSYNC_REC_DTYPE)
        self._chk(self.lib.gpsx_track_loop_weighted_sync_multi(self.h, cfg.ctypes.data, None if aid is None else aid.ctypes.data, rx.ctypes.data,
                                                               streams.ctypes.data, n_blocks, C.c_void_p(d_state), rec.ctypes.data),
                  "gpsx_track_loop_weighted_sync_multi")
        return rec

    def wnav_words(self, d_rec: int, n_slots: int, n_blocks: int, d_state: int, n_ch: int, max_bad_words: int = 3) -> np.ndarray:
        """EXTENSION: LNAV frame sync and parity-checked words from the WSYNC_REC_DTYPE [n_slots, n_ch] records at device address
        d_rec that gpsx_track_loop_weighted_sync_dev wrote for n_blocks blocks, on the n_ch WNAV_STATE_DTYPE frame states at device
        address d_state (all zero: a fresh channel).  -> WNAV_WORD_DTYPE [n_blocks // 600 + 2, n_ch]; an empty slot has flags 0 and
        end_block -1"""
        cfg = np.zeros(1, WNAV_CFG_DTYPE)
        cfg["max_bad_words"] = max_bad_words
        words = np.zeros((wnav_word_slots(n_blocks), n_ch), WNAV_WORD_DTYPE)
        self._chk(self.lib.gpsx_wnav_words(self.h, cfg.ctypes.data, C.c_void_p(d_rec), n_slots, n_blocks, C.c_void_p(d_state), n_ch,
                                           words.ctypes.data), "gpsx_wnav_words")
        return words

    def wobs(self, d_rec: int, n_slots: int, n_blocks: int, d_words: int, d_state: int, n_ch: int, edge_guard: float = 512.0) -> np.ndarray:
        """EXTENSION: every channel's transmit time at the first sample of the block that follows the launch, from the WSYNC_REC_DTYPE
        [n_slots, n_ch] records at device address d_rec and the WNAV_WORD_DTYPE [n_blocks // 600 + 2, n_ch] words at d_words that the
        two earlier stages wrote for n_blocks blocks, on the n_ch WOBS_STATE_DTYPE states at device address d_state (all zero: a fresh
        channel).  -> WOBS_DTYPE [n_ch]"""
        cfg = np.zeros(1, WOBS_CFG_DTYPE)
        cfg["edge_guard"] = edge_guard
        obs = np.zeros(n_ch, WOBS_DTYPE)
        self._chk(self.lib.gpsx_wobs(self.h, cfg.ctypes.data, C.c_void_p(d_rec), n_slots, n_blocks, C.c_void_p(d_words), C.c_void_p(d_state), n_ch,
                                     obs.ctypes.data), "gpsx_wobs")
        return obs

    def weph(self, d_words: int, n_blocks: int, d_state: int, n_ch: int) -> np.ndarray:
        """EXTENSION: every channel's broadcast ephemeris from the WNAV_WORD_DTYPE [n_blocks // 600 + 2, n_ch] words at device address
        d_words that gpsx_wnav_words_dev wrote for n_blocks blocks, on the n_ch WEPH_STATE_DTYPE states at device address d_state (all
        zero: a fresh channel).  -> WEPH_DTYPE [n_ch]; a record with WEPH_FLAG_VALID holds the decoded ephemeris (weph_to_eph)"""
        cfg = np.zeros(1, WEPH_CFG_DTYPE)
        eph = np.zeros(n_ch, WEPH_DTYPE)
        self._chk(self.lib.gpsx_weph(self.h, cfg.ctypes.data, C.c_void_p(d_words), n_blocks, C.c_void_p(d_state), n_ch, eph.ctypes.data), "gpsx_weph")
        return eph

    def wlock(self, cfg: np.ndarray, d_rec: int, n_slots: int, n_blocks: int, d_state: int, n_ch: int, d_sync_state: int | None = None) -> np.ndarray:
        """EXTENSION: every channel's code-lock, carrier-lock and C/N0 indicators from the WSYNC_REC_DTYPE [n_slots, n_ch] records at
        device address d_rec that gpsx_track_loop_weighted_sync_dev wrote for n_blocks blocks, on the n_ch WLOCK_STATE_DTYPE states at
        device address d_state (all zero: a fresh channel); cfg from wlock_cfg.  d_sync_state: the sync loop's own states, needed when
        cfg's rearm is not 0 -- a channel whose re-arm falls due has its bit search restarted there.  -> WLOCK_DTYPE [n_ch]"""
        assert cfg.dtype == WLOCK_CFG_DTYPE and cfg.size == 1
        lock = np.zeros(n_ch, WLOCK_DTYPE)
        self._chk(self.lib.gpsx_wlock(self.h, cfg.ctypes.data, C.c_void_p(d_rec), n_slots, n_blocks, C.c_void_p(d_state),
                                      C.c_void_p(d_sync_state) if d_sync_state else None, n_ch, lock.ctypes.data), "gpsx_wlock")
        return lock

    def wfix(self, cfg: np.ndarray, obs: np.ndarray, eph: np.ndarray, n_rx: int, lock: np.ndarray | None = None,
             prev: np.ndarray | None = None, want_pr: bool = False):
        """EXTENSION: every receiver's position fix from the WOBS_DTYPE observables and WEPH_DTYPE ephemeris records [n_rx * ch_per_rx]
        of one launch of the weighted chain (receiver r owns slots r * ch_per_rx ...), host arrays; cfg from wfix_cfg.  lock: WLOCK_DTYPE
        records, a slot then also needs WLOCK_FLAG_CODE; prev: WFIX_DTYPE [n_rx], the start points (records with WFIX_FLAG_FIX).
        -> WFIX_DTYPE [n_rx], and with want_pr the pseudoranges float64 [n_rx * ch_per_rx] as well"""
        assert cfg.dtype == WFIX_CFG_DTYPE and cfg.size == 1
        n_ch = n_rx * int(cfg["ch_per_rx"][0])
        obs, eph = np.ascontiguousarray(obs, WOBS_DTYPE).reshape(-1), np.ascontiguousarray(eph, WEPH_DTYPE).reshape(-1)
        assert len(obs) == n_ch and len(eph) == n_ch
        lock = None if lock is None else np.ascontiguousarray(lock).view(WLOCK_DTYPE).reshape(n_ch)      # (any 64-byte record dtype)
        prev = None if prev is None else np.ascontiguousarray(prev, WFIX_DTYPE).reshape(n_rx)
        fix, pr = np.zeros(n_rx, WFIX_DTYPE), np.zeros(n_ch, np.float64)
        self._chk(self.lib.gpsx_wfix(self.h, cfg.ctypes.data, obs.ctypes.data, eph.ctypes.data, None if lock is None else lock.ctypes.data,
                                     None if prev is None else prev.ctypes.data, n_rx, fix.ctypes.data, pr.ctypes.data if want_pr else None),
                  "gpsx_wfix")
        return (fix, pr) if want_pr else fix

    def wfde(self, cfg: np.ndarray, obs: np.ndarray, eph: np.ndarray, n_rx: int, lock: np.ndarray | None = None,
             prev: np.ndarray | None = None, want_pr: bool = False):
        """EXTENSION: wfix with the ambiguous millisecond repaired and faulty slots detected and excluded (include/gpsx.h gpsx_wfde);
        the same host arrays, cfg from wfde_cfg.
        -> (WFIX_DTYPE [n_rx], WFDE_DTYPE [n_rx]), and with want_pr the last round's pseudoranges float64 [n_rx * ch_per_rx] as well"""
        assert cfg.dtype == WFDE_CFG_DTYPE and cfg.size == 1
        n_ch = n_rx * int(cfg["fix"]["ch_per_rx"][0])
        obs, eph = np.ascontiguousarray(obs, WOBS_DTYPE).reshape(-1), np.ascontiguousarray(eph, WEPH_DTYPE).reshape(-1)
        assert len(obs) == n_ch and len(eph) == n_ch
        lock = None if lock is None else np.ascontiguousarray(lock).view(WLOCK_DTYPE).reshape(n_ch)      # (any 64-byte record dtype)
        prev = None if prev is None else np.ascontiguousarray(prev, WFIX_DTYPE).reshape(n_rx)
        fix, fde, pr = np.zeros(n_rx, WFIX_DTYPE), np.zeros(n_rx, WFDE_DTYPE), np.zeros(n_ch, np.float64)
        self._chk(self.lib.gpsx_wfde(self.h, cfg.ctypes.data, obs.ctypes.data, eph.ctypes.data, None if lock is None else lock.ctypes.data,
                                     None if prev is None else prev.ctypes.data, n_rx, fix.ctypes.data, fde.ctypes.data,
                                     pr.ctypes.data if want_pr else None), "gpsx_wfde")
        return (fix, fde, pr) if want_pr else (fix, fde)

    def wvel(self, cfg: np.ndarray, obs: np.ndarray, eph: np.ndarray, fix: np.ndarray, n_rx: int, lock: np.ndarray | None = None) -> np.ndarray:
        """EXTENSION: every receiver's velocity and clock drift (include/gpsx.h gpsx_wvel) from wfix's / wfde's host arrays and their
        WFIX_DTYPE records fix [n_rx]; cfg from wvel_cfg.  lock: WLOCK_DTYPE records, a slot then also needs WLOCK_FLAG_CARRIER.
        -> WVEL_DTYPE [n_rx]"""
        assert cfg.dtype == WVEL_CFG_DTYPE and cfg.size == 1
        n_ch = n_rx * int(cfg["ch_per_rx"][0])
        obs, eph = np.ascontiguousarray(obs, WOBS_DTYPE).reshape(-1), np.ascontiguousarray(eph, WEPH_DTYPE).reshape(-1)
        assert len(obs) == n_ch and len(eph) == n_ch
        lock = None if lock is None else np.ascontiguousarray(lock).view(WLOCK_DTYPE).reshape(n_ch)      # (any 64-byte record dtype)
        fix = np.ascontiguousarray(fix, WFIX_DTYPE).reshape(n_rx)
        vel = np.zeros(n_rx, WVEL_DTYPE)
        self._chk(self.lib.gpsx_wvel(self.h, cfg.ctypes.data, obs.ctypes.data, eph.ctypes.data, None if lock is None else lock.ctypes.data,
                                     fix.ctypes.data, n_rx, vel.ctypes.data), "gpsx_wvel")
        return vel

    def wkf(self, cfg: np.ndarray, obs: np.ndarray, eph: np.ndarray, n_rx: int, n_blocks: int, d_state: int, fix: np.ndarray | None = None,
            vel: np.ndarray | None = None, lock: np.ndarray | None = None) -> np.ndarray:
        """EXTENSION: every receiver's navigation filter (include/gpsx.h gpsx_wkf), one call per launch of n_blocks blocks, on the n_rx
        WKF_STATE_DTYPE states at device address d_state (all zero: a fresh receiver); obs / eph / lock as wfix's host arrays, cfg from
        wkf_cfg.  fix (WFIX_DTYPE [n_rx]) and vel (WVEL_DTYPE [n_rx]) initialise the receivers that are not yet initialised.
        -> WKF_DTYPE [n_rx]"""
        assert cfg.dtype == WKF_CFG_DTYPE and cfg.size == 1
        n_ch = n_rx * int(cfg["ch_per_rx"][0])
        obs, eph = np.ascontiguousarray(obs, WOBS_DTYPE).reshape(-1), np.ascontiguousarray(eph, WEPH_DTYPE).reshape(-1)
        assert len(obs) == n_ch and len(eph) == n_ch
        lock = None if lock is None else np.ascontiguousarray(lock).view(WLOCK_DTYPE).reshape(n_ch)      # (any 64-byte record dtype)
        fix = None if fix is None else np.ascontiguousarray(fix, WFIX_DTYPE).reshape(n_rx)
        vel = None if vel is None else np.ascontiguousarray(vel, WVEL_DTYPE).reshape(n_rx)
        kf = np.zeros(n_rx, WKF_DTYPE)
        self._chk(self.lib.gpsx_wkf(self.h, cfg.ctypes.data, obs.ctypes.data, eph.ctypes.data, None if lock is None else lock.ctypes.data,
                                    None if fix is None else fix.ctypes.data, None if vel is None else vel.ctypes.data, n_rx, n_blocks,
                                    C.c_void_p(d_state), kf.ctypes.data), "gpsx_wkf")
        return kf

    def wacq(self, cfg: np.ndarray, peaks: np.ndarray, prns, dopp_min_hz: int, dopp_step_hz: int, d_sync_state: int, d_lock_state: int | None = None,
             d_nav_state: int | None = None, d_obs_state: int | None = None, d_eph_state: int | None = None, want_det: bool = True):
        """EXTENSION: acquisition decisions and slot hand-over (include/gpsx.h gpsx_wacq) from a weighted grid's records, PEAK_DTYPE
        [n_rx, n_prn, n_dopp] in host memory (search s is receiver s; prns and the Doppler grid are the grid call's), on the
        n_rx * ch_per_rx WSYNC_STATE_DTYPE states at device address d_sync_state and, where given, the lock, nav, obs and eph states of
        the same slots: a detected PRN that no slot tracks is handed to a free slot, whose states start afresh; cfg from wacq_cfg.
        -> (WACQ_DTYPE [n_rx], WACQ_DET_DTYPE [n_rx, n_prn]), or the first alone without want_det"""
        assert cfg.dtype == WACQ_CFG_DTYPE and cfg.size == 1
        peaks = np.ascontiguousarray(peaks, PEAK_DTYPE)
        prns = np.ascontiguousarray(prns, np.uint8)
        assert peaks.ndim == 3 and peaks.shape[1] == len(prns)
        n_rx, n_prn, n_dopp = peaks.shape
        g = AcqWeightedT(n_rx, 0, n_prn, prns.ctypes.data_as(C.POINTER(C.c_uint8)), dopp_min_hz, dopp_step_hz, n_dopp, 1)
        acq, det = np.zeros(n_rx, WACQ_DTYPE), np.zeros((n_rx, n_prn), WACQ_DET_DTYPE)
        opt = lambda d: C.c_void_p(d) if d else None   # noqa: E731
        self._chk(self.lib.gpsx_wacq(self.h, cfg.ctypes.data, C.addressof(g), peaks.ctypes.data, C.c_void_p(d_sync_state), opt(d_lock_state),
                                     opt(d_nav_state), opt(d_obs_state), opt(d_eph_state), acq.ctypes.data, det.ctypes.data if want_det else None),
                  "gpsx_wacq")
        return (acq, det) if want_det else acq

    def wbank(self, cfg: np.ndarray, prns, d_sync_state: int, eph: np.ndarray, d_bank: int, want_out: bool = True):
        """EXTENSION: the ephemeris bank (include/gpsx.h gpsx_wbank) behind a launch's WEPH_DTYPE records eph [n_rx * ch_per_rx] in host
        memory: the newest VALID record per receiver and PRN of the list prns goes into the WEPH_DTYPE [n_rx, len(prns)] bank at device
        address d_bank (all zero: empty), and a slot of the WSYNC_STATE_DTYPE states at d_sync_state that tracks a listed PRN without a
        VALID record of its own gets the bank's in the merged copy; cfg from wbank_cfg.
        -> (WBANK_DTYPE [n_rx], merged WEPH_DTYPE [n_rx * ch_per_rx]), or the first alone without want_out"""
        assert cfg.dtype == WBANK_CFG_DTYPE and cfg.size == 1
        eph = np.ascontiguousarray(eph, WEPH_DTYPE).reshape(-1)
        prns = np.ascontiguousarray(prns, np.uint8)
        ch = int(cfg["ch_per_rx"][0])
        assert ch >= 1 and eph.size % ch == 0
        n_rx = eph.size // ch
        rep, out = np.zeros(n_rx, WBANK_DTYPE), np.zeros(eph.size, WEPH_DTYPE)
        self._chk(self.lib.gpsx_wbank(self.h, cfg.ctypes.data, n_rx, len(prns), prns.ctypes.data, C.c_void_p(d_sync_state), eph.ctypes.data,
                                      C.c_void_p(d_bank), out.ctypes.data if want_out else None, rep.ctypes.data), "gpsx_wbank")
        return (rep, out) if want_out else rep

    def wpred(self, cfg: np.ndarray, prns, n_rx: int, d_kf_state: int, d_bank: int, d_sync_state: int, d_lock_state: int | None = None,
              d_nav_state: int | None = None, d_obs_state: int | None = None, d_eph_state: int | None = None, want_pred: bool = True):
        """EXTENSION: prediction and hot hand-over (include/gpsx.h gpsx_wpred) from the n_rx WKF_STATE_DTYPE filter states at device
        address d_kf_state and the WEPH_DTYPE [n_rx, len(prns)] bank at d_bank, on the n_rx * ch_per_rx WSYNC_STATE_DTYPE states at
        d_sync_state and, where given, the lock, nav, obs and eph states of the same slots; cfg from wpred_cfg.
        -> (WPRED_RX_DTYPE [n_rx], WPRED_DTYPE [n_rx, n_prn]), or the first alone without want_pred"""
        assert cfg.dtype == WPRED_CFG_DTYPE and cfg.size == 1
        prns = np.ascontiguousarray(prns, np.uint8)
        rx, pred = np.zeros(n_rx, WPRED_RX_DTYPE), np.zeros((n_rx, len(prns)), WPRED_DTYPE)
        opt = lambda d: C.c_void_p(d) if d else None   # noqa: E731
        self._chk(self.lib.gpsx_wpred(self.h, cfg.ctypes.data, n_rx, len(prns), prns.ctypes.data, C.c_void_p(d_kf_state), C.c_void_p(d_bank),
                                      C.c_void_p(d_sync_state), opt(d_lock_state), opt(d_nav_state), opt(d_obs_state), opt(d_eph_state), rx.ctypes.data,
                                      pred.ctypes.data if want_pred else None), "gpsx_wpred")
        return (rx, pred) if want_pred else rx

    def _wsnap_grid(self, n_rx, prns, dopp_min_hz, dopp_step_hz, n_dopp):
        prns = np.ascontiguousarray(prns, np.uint8)
        return prns, AcqWeightedT(n_rx, 0, len(prns), prns.ctypes.data_as(C.POINTER(C.c_uint8)), dopp_min_hz, dopp_step_hz, n_dopp, 1)

    def wsnap(self, cfg: np.ndarray, peaks: np.ndarray, prns, dopp_min_hz: int, dopp_step_hz: int, d_bank: int, bank_stride: int, prior: np.ndarray,
              want_sv: bool = True):
        """EXTENSION: snapshot fixes (include/gpsx.h gpsx_wsnap) from a weighted grid's records, PEAK_DTYPE [n_rx, n_prn, n_dopp] in host
        memory (search s is receiver s; prns and the Doppler grid are the grid call's), the WEPH_DTYPE bank at device address d_bank
        ([n_rx, n_prn] with bank_stride n_prn, one shared row [n_prn] with 0) and the WSNAP_PRIOR_DTYPE [n_rx] priors (wsnap_prior); cfg
        from wsnap_cfg.  -> (WSNAP_DTYPE [n_rx], WSNAP_SV_DTYPE [n_rx, n_prn]), or the first alone without want_sv"""
        assert cfg.dtype == WSNAP_CFG_DTYPE and cfg.size == 1
        peaks = np.ascontiguousarray(peaks, PEAK_DTYPE)
        assert peaks.ndim == 3 and peaks.shape[1] == len(prns)
        n_rx, n_prn, n_dopp = peaks.shape
        prior = np.ascontiguousarray(prior, WSNAP_PRIOR_DTYPE).reshape(n_rx)
        prns, g = self._wsnap_grid(n_rx, prns, dopp_min_hz, dopp_step_hz, n_dopp)
        snap, sv = np.zeros(n_rx, WSNAP_DTYPE), np.zeros((n_rx, n_prn), WSNAP_SV_DTYPE)
        self._chk(self.lib.gpsx_wsnap(self.h, cfg.ctypes.data, C.addressof(g), peaks.ctypes.data, C.c_void_p(d_bank), bank_stride, prior.ctypes.data,
                                      snap.ctypes.data, sv.ctypes.data if want_sv else None), "gpsx_wsnap")
        return (snap, sv) if want_sv else snap

    def wsnap_dev(self, cfg: np.ndarray, d_peaks: int, n_rx: int, prns, dopp_min_hz: int, dopp_step_hz: int, n_dopp: int, d_bank: int, bank_stride: int,
                  d_prior: int, d_snap: int, d_sv: int | None = None) -> None:
        """EXTENSION: gpsx_wsnap_dev on the records a weighted grid call left at device address d_peaks, enqueued behind it on the
        engine's stream: WSNAP_DTYPE [n_rx] to d_snap and, where given, WSNAP_SV_DTYPE [n_rx, len(prns)] to d_sv; nothing is read back"""
        assert cfg.dtype == WSNAP_CFG_DTYPE and cfg.size == 1
        prns, g = self._wsnap_grid(n_rx, prns, dopp_min_hz, dopp_step_hz, n_dopp)
        self._chk(self.lib.gpsx_wsnap_dev(self.h, cfg.ctypes.data, C.addressof(g), C.c_void_p(d_peaks), C.c_void_p(d_bank), bank_stride,
                                          C.c_void_p(d_prior), C.c_void_p(d_snap), C.c_void_p(d_sv) if d_sv else None), "gpsx_wsnap_dev")

    def wsnap_to_fix(self, snap: np.ndarray) -> np.ndarray:
        """EXTENSION: gpsx_wsnap_to_fix per record: WSNAP_DTYPE [n] -> WFIX_DTYPE [n]; a record without FIX gives an all-zero one"""
        snap = np.ascontiguousarray(snap, WSNAP_DTYPE).reshape(-1)
        fix = np.zeros(len(snap), WFIX_DTYPE)
        for k in range(len(snap)):
            self.lib.gpsx_wsnap_to_fix(snap[k:k + 1].ctypes.data, fix[k:k + 1].ctypes.data)
        return fix

    def wtow(self, cfg: np.ndarray, prns, n_rx: int, d_pred_rx: int, d_pred: int, d_sync_state: int, d_obs_state: int, d_obs: int | None = None):
        """EXTENSION: time-of-week aiding (include/gpsx.h gpsx_wtow) of the n_rx * ch_per_rx WOBS_STATE_DTYPE states at device address
        d_obs_state from the WPRED_RX_DTYPE [n_rx] and WPRED_DTYPE [n_rx, len(prns)] records a gpsx_wpred_dev call left at d_pred_rx and
        d_pred -- its epoch the block the states stand at: the caller's duty --, the slots' PRNs from the WSYNC_STATE_DTYPE states at
        d_sync_state; d_obs: that launch's WOBS_DTYPE records, patched where a state changed; cfg from wtow_cfg.
        -> (WTOW_DTYPE [n_rx * ch_per_rx], WTOW_RX_DTYPE [n_rx])"""
        assert cfg.dtype == WTOW_CFG_DTYPE and cfg.size == 1
        prns = np.ascontiguousarray(prns, np.uint8)
        tow, tow_rx = np.zeros(n_rx * int(cfg["ch_per_rx"][0]), WTOW_DTYPE), np.zeros(n_rx, WTOW_RX_DTYPE)
        self._chk(self.lib.gpsx_wtow(self.h, cfg.ctypes.data, n_rx, len(prns), prns.ctypes.data, C.c_void_p(d_pred_rx), C.c_void_p(d_pred),
                                     C.c_void_p(d_sync_state), C.c_void_p(d_obs_state), C.c_void_p(d_obs) if d_obs else None, tow.ctypes.data,
                                     tow_rx.ctypes.data), "gpsx_wtow")
        return tow, tow_rx

    def wtow_dev(self, cfg: np.ndarray, prns, n_rx: int, d_pred_rx: int, d_pred: int, d_sync_state: int, d_obs_state: int, d_obs: int | None,
                 d_tow: int, d_tow_rx: int) -> None:
        """the same with the two record arrays left in device memory at d_tow and d_tow_rx: enqueues on the context's stream and returns"""
        assert cfg.dtype == WTOW_CFG_DTYPE and cfg.size == 1
        prns = np.ascontiguousarray(prns, np.uint8)
        self._chk(self.lib.gpsx_wtow_dev(self.h, cfg.ctypes.data, n_rx, len(prns), prns.ctypes.data, C.c_void_p(d_pred_rx), C.c_void_p(d_pred),
                                         C.c_void_p(d_sync_state), C.c_void_p(d_obs_state), C.c_void_p(d_obs) if d_obs else None, C.c_void_p(d_tow),
                                         C.c_void_p(d_tow_rx)), "gpsx_wtow_dev")

    def walm(self, cfg: np.ndarray, d_words: int, n_blocks: int, n_rx: int, d_slot_state: int, d_bank: int, want_alm: bool = True):
        """EXTENSION: almanac, ionosphere and UTC (include/gpsx.h gpsx_walm) from the WNAV_WORD_DTYPE [n_blocks // 600 + 2, n_rx *
        ch_per_rx] words at device address d_words that gpsx_wnav_words_dev wrote for n_blocks blocks, on the n_rx * ch_per_rx
        WALM_SLOT_DTYPE states at d_slot_state and the n_rx WALM_BANK_DTYPE banks at d_bank (all zero: fresh); cfg from walm_cfg.
        -> (WALM_RX_DTYPE [n_rx], WALM_SV_DTYPE [n_rx, 32]), or the first alone without want_alm"""
        assert cfg.dtype == WALM_CFG_DTYPE and cfg.size == 1
        rx, alm = np.zeros(n_rx, WALM_RX_DTYPE), np.zeros((n_rx, 32), WALM_SV_DTYPE)
        self._chk(self.lib.gpsx_walm(self.h, cfg.ctypes.data, C.c_void_p(d_words), n_blocks, n_rx, C.c_void_p(d_slot_state), C.c_void_p(d_bank),
                                     rx.ctypes.data, alm.ctypes.data if want_alm else None), "gpsx_walm")
        return (rx, alm) if want_alm else rx

    def walm_dev(self, cfg: np.ndarray, d_words: int, n_blocks: int, n_rx: int, d_slot_state: int, d_bank: int, d_rx: int, d_alm: int | None) -> None:
        """the same with the record arrays left in device memory at d_rx and d_alm (None: not wanted): enqueues and returns"""
        assert cfg.dtype == WALM_CFG_DTYPE and cfg.size == 1
        self._chk(self.lib.gpsx_walm_dev(self.h, cfg.ctypes.data, C.c_void_p(d_words), n_blocks, n_rx, C.c_void_p(d_slot_state), C.c_void_p(d_bank),
                                         C.c_void_p(d_rx), C.c_void_p(d_alm) if d_alm else None), "gpsx_walm_dev")

    def acq_window(self, cfg: np.ndarray, pred: np.ndarray, blocks_2bit: np.ndarray, prns, dopp_min_hz: int, dopp_step_hz: int, n_dopp: int,
                   use_magnitude: bool = True, stride_blocks: int | None = None, want_rep: bool = True):
        """EXTENSION: the weighted grid in a window around each prediction (include/gpsx.h gpsx_acq_window_weighted): pred is gpsx_wpred's
        WPRED_DTYPE [n_rx, len(prns)] in host memory, prns THE SAME LIST that call was given; receiver r reads blocks r * stride_blocks
        .. + n_coh * n_seg - 1 (the stride defaults to n_coh * n_seg); cfg from acq_window_cfg.
        -> (PEAK_DTYPE [n_rx, n_prn, n_dopp], ACQ_WINDOW_REP_DTYPE [n_rx, n_prn]), or the first alone without want_rep"""
        assert cfg.dtype == ACQ_WINDOW_CFG_DTYPE and cfg.size == 1
        pred = np.ascontiguousarray(pred, WPRED_DTYPE)
        prns = np.ascontiguousarray(prns, np.uint8)
        assert pred.ndim == 2 and pred.shape[1] == len(prns)
        blocks = np.ascontiguousarray(blocks_2bit, np.uint8).reshape(-1, BYTES_PER_MS_2BIT)
        n_rx = pred.shape[0]
        stride = int(cfg["n_coh"][0]) * int(cfg["n_seg"][0]) if stride_blocks is None else stride_blocks
        g = AcqWeightedT(n_rx, stride, len(prns), prns.ctypes.data_as(C.POINTER(C.c_uint8)), dopp_min_hz, dopp_step_hz, n_dopp, 1 if use_magnitude else 0)
        peaks, rep = np.zeros((n_rx, len(prns), n_dopp), PEAK_DTYPE), np.zeros((n_rx, len(prns)), ACQ_WINDOW_REP_DTYPE)
        self._chk(self.lib.gpsx_acq_window_weighted(self.h, C.addressof(g), cfg.ctypes.data, pred.ctypes.data, blocks.ctypes.data, len(blocks),
                                                    peaks.ctypes.data, rep.ctypes.data if want_rep else None), "gpsx_acq_window_weighted")
        return (peaks, rep) if want_rep else peaks

    def acq_window_dev(self, cfg: np.ndarray, d_pred: int, d_blocks: int, n_blocks: int, n_rx: int, prns, dopp_min_hz: int, dopp_step_hz: int,
                       n_dopp: int, d_peaks: int, d_rep: int | None, use_magnitude: bool = True, stride_blocks: int | None = None) -> None:
        """the same with the predictions, the blocks, the records and the reports (None: not wanted) in device memory: enqueues and returns"""
        assert cfg.dtype == ACQ_WINDOW_CFG_DTYPE and cfg.size == 1
        prns = np.ascontiguousarray(prns, np.uint8)
        stride = int(cfg["n_coh"][0]) * int(cfg["n_seg"][0]) if stride_blocks is None else stride_blocks
        g = AcqWeightedT(n_rx, stride, len(prns), prns.ctypes.data_as(C.POINTER(C.c_uint8)), dopp_min_hz, dopp_step_hz, n_dopp, 1 if use_magnitude else 0)
        self._chk(self.lib.gpsx_acq_window_weighted_dev(self.h, C.addressof(g), cfg.ctypes.data, C.c_void_p(d_pred), C.c_void_p(d_blocks), n_blocks,
                                                        C.c_void_p(d_peaks), C.c_void_p(d_rep) if d_rep else None), "gpsx_acq_window_weighted_dev")

    def set_loop_schedule(self, schedule: int) -> None:
        """SCHED_EVERY_MS or SCHED_MUX17 (the reference's four-channel 17 ms multiplex) for this context's track_loop launches"""
        self._chk(self.lib.gpsx_loop_set_schedule(self.h, schedule), "gpsx_loop_set_schedule")

    def set_acq_path(self, path: int) -> None:
        """ACQ_PATH_MATRIX (default) or ACQ_PATH_VECTOR (no MFMA: the polyphase popcount kernel)"""
        self._chk(self.lib.gpsx_set_acq_path(self.h, path), "gpsx_set_acq_path")

    def set_loop_draws(self, draws: int) -> None:
        """DRAWS_XORSHIFT (default) or DRAWS_LIBC (the reference's rand(), drawn on the host in the reference's order)"""
        self._chk(self.lib.gpsx_loop_set_draws(self.h, draws), "gpsx_loop_set_draws")

    def set_loop_word_sync(self, owner: int) -> None:
        """WORDSYNC_DEVICE (default: the kernel decides the data polarity itself) or WORDSYNC_HOST (gpsx_loop_set_polarity only)"""
        self._chk(self.lib.gpsx_loop_set_word_sync(self.h, owner), "gpsx_loop_set_word_sync")

    def track_loop(self, if_blocks: np.ndarray, d_state: int, n_ch: int, first_tick: int, want_trace=False):
        """K = len(if_blocks) milliseconds of the device tracking loops on the n_ch states at device address d_state.
        Returns (flags uint8 [K, n_ch], trace LOOP_TRACE_DTYPE [K, n_ch] or None)."""
        blocks = np.ascontiguousarray(if_blocks, np.uint8).reshape(-1, self.block_bytes)
        flags = np.zeros((len(blocks), n_ch), np.uint8)
        trace = np.zeros((len(blocks), n_ch), LOOP_TRACE_DTYPE) if want_trace else None
        self._chk(self.lib.gpsx_track_loop(self.h, blocks.ctypes.data, len(blocks), d_state, n_ch, first_tick,
                                           flags.ctypes.data, _ptr(trace)), "gpsx_track_loop")
        return flags, trace

    def rewind(self, states: np.ndarray, steps) -> None:
        steps = np.ascontiguousarray(steps, np.uint8)
        self._chk(self.lib.gpsx_rewind(self.h, states.ctypes.data, len(states), steps.ctypes.data), "gpsx_rewind")

    # -- per-call primitives ------------------------------------------------------------------------------------
    def wipeoff(self, signal, freq_hz, accum=0, prefill=None):
        di = np.zeros(1024, np.uint16) if prefill is None else prefill[0].copy()
        dq = np.zeros(1024, np.uint16) if prefill is None else prefill[1].copy()
        acc = C.c_uint32(accum)
        sig = np.ascontiguousarray(signal, np.uint8)
        self._chk(self.lib.gpsx_wipeoff(self.h, sig.ctypes.data, np.float32(freq_hz), C.byref(acc), di.ctypes.data,
                                        dq.ctypes.data), "gpsx_wipeoff")
        return di, dq, acc.value

    def replica(self, chips, offset_bits, pad_in=0):
        out = np.zeros(1024, np.uint16)
        out[1023] = pad_in
        chips = np.ascontiguousarray(chips, np.uint8)
        self._chk(self.lib.gpsx_replica(self.h, chips.ctypes.data, offset_bits, out.ctypes.data), "gpsx_replica")
        return out

    def corr_offsets(self, rep, di, dq, offsets):
        offsets = np.ascontiguousarray(offsets, np.uint16)
        n = len(offsets)
        ci, cq, c8 = np.zeros(n, np.uint16), np.zeros(n, np.uint16), np.zeros(n, np.int16)
        self._chk(self.lib.gpsx_corr_offsets(self.h, rep.ctypes.data, di.ctypes.data, dq.ctypes.data,
                                             offsets.ctypes.data, n, ci.ctypes.data, cq.ctypes.data, c8.ctypes.data),
                  "gpsx_corr_offsets")
        return ci, cq, c8

    def mag8(self, cnt_i, cnt_q) -> np.ndarray:
        ci = np.ascontiguousarray(cnt_i, np.uint16)
        cq = np.ascontiguousarray(cnt_q, np.uint16)
        out = np.zeros(len(ci), np.int16)
        self._chk(self.lib.gpsx_mag8(self.h, ci.ctypes.data, cq.ctypes.data, len(ci), out.ctypes.data), "gpsx_mag8")
        return out

    def corr_search(self, rep, di, dq, start, stop):
        pk = np.zeros(1, PEAK_DTYPE)
        self._chk(self.lib.gpsx_corr_search(self.h, rep.ctypes.data, di.ctypes.data, dq.ctypes.data, start, stop,
                                            pk.ctypes.data), "gpsx_corr_search")
        return int(pk["max_val"][0]), int(pk["avr"][0]), int(pk["phase"][0])


class Capture:
    """A capture ring of `eng` (include/gpsx.h "IF ingest"): pinned host slots mirrored in HBM by asynchronous copies."""

    def __init__(self, eng: Engine, n_slots: int):
        self.eng, self.lib = eng, eng.lib
        h = C.c_void_p()
        eng._chk(self.lib.gpsx_capture_create(eng.h, n_slots, C.byref(h)), "gpsx_capture_create")
        self.h = h
        self.block_bytes = int(self.lib.gpsx_capture_block_bytes(h))

    def close(self):
        if getattr(self, "h", None) and getattr(self.eng, "h", None):
            self.lib.gpsx_capture_destroy(self.h)
        self.h = None

    def push(self, block: np.ndarray):
        block = np.ascontiguousarray(block, np.uint8).reshape(-1)
        assert block.size == self.block_bytes
        self.eng._chk(self.lib.gpsx_capture_push(self.h, _ptr(block)), "gpsx_capture_push")

    def ready_ptr(self) -> int:
        """Host address of the newest committed block (what signal_capture_get_ready_buf returns), 0 before the first."""
        return int(self.lib.gpsx_capture_ready_buf(self.h) or 0)

    def ready_view(self, n_blocks: int = 1) -> np.ndarray:
        """numpy view (no copy) of the pinned slot(s) ending at the newest block; only windows that do not wrap."""
        p = self.ready_ptr() - (n_blocks - 1) * self.block_bytes
        buf = (C.c_uint8 * (n_blocks * self.block_bytes)).from_address(p)
        return np.frombuffer(buf, np.uint8).reshape(n_blocks, self.block_bytes)

    def window_dev(self, n_blocks: int) -> int:
        d = C.c_void_p()
        self.eng._chk(self.lib.gpsx_capture_window_dev(self.h, n_blocks, C.byref(d)), "gpsx_capture_window_dev")
        return int(d.value)

    def packet_cnt(self) -> int:
        return int(self.lib.gpsx_capture_packet_cnt(self.h))

    def replay_file(self, path: str, first_block=0, max_blocks=-1, on_block=None) -> int:
        cb = CAPTURE_BLOCK_FN((lambda user, cap, idx: int(on_block(idx) or 0)) if on_block else 0)
        n = int(self.lib.gpsx_capture_replay_file(self.h, path.encode(), first_block, max_blocks, cb, None))
        if n < 0:
            self.eng._chk(n, "gpsx_capture_replay_file")
        return n
