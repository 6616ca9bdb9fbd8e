"""An exact CPU restatement of the closed DLL / Costas PLL / FLL on weighted two-bit samples (include/gpsx.h
gpsx_track_loop_weighted), for the tests.  Per window the correlators are weighted_track_ref.track on the state at the window's start
(already pinned to the weighted grids' restatements); the loop arithmetic is numpy float32, one operation per line in the order the
header writes it; the arctangent is csrc/gpsx_libm.hpp's atanf_fdlibm, called through a tiny shared object compiled with g++ the way
tests/test_libm_restatement.py compiles its program (that test pins the header to glibc's fdlibm arctangent).  Nothing of the
library's own kernel or loop code is included or imported here."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

import weighted_track_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STATE_DTYPE = np.dtype([("prn", "<i4"), ("code_phase_fine", "<f4"), ("if_freq_offset_hz", "<f4"), ("if_freq_accum", "<u4"),
                        ("dll_err", "<f4"), ("pll_err", "<f4"), ("prev_ip", "<i4"), ("prev_qp", "<i4"), ("n_updates", "<u4"),
                        ("reserved", "<u4")])
REC_DTYPE = np.dtype([("iq", "<i4", 6), ("code_phase_fine", "<f4"), ("if_freq_offset_hz", "<f4"), ("if_freq_accum", "<u4")])
TRK_DTYPE = np.dtype([("prn", "<i4"), ("code_phase_fine", "<f4"), ("if_freq_offset_hz", "<f4"), ("if_freq_accum", "<u4")])
assert STATE_DTYPE.itemsize == 40 and REC_DTYPE.itemsize == 36

F = np.float32
SPAN = F(16368.0)
CYCLES = F(0.15915494)

_SRC = r"""
#include "gpsx_libm.hpp"
extern "C" float wloop_atanf(float x) { return gpsx_libm::atanf_fdlibm(x); }
"""
_lib = None
_tmp = None


def atanf(x):
    """csrc/gpsx_libm.hpp atanf_fdlibm on a float32"""
    global _lib, _tmp
    if _lib is None:
        _tmp = tempfile.TemporaryDirectory(prefix="wloop_atanf_")
        src, so = os.path.join(_tmp.name, "atanf.cpp"), os.path.join(_tmp.name, "libwloop_atanf.so")
        with open(src, "w") as f:
            f.write(_SRC)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-I",
                               os.path.join(ROOT, "stm32f4_sdr_gps_amd", "csrc"), "-o", so, src])
        _lib = ctypes.CDLL(so)
        _lib.wloop_atanf.argtypes = [ctypes.c_float]
        _lib.wloop_atanf.restype = ctypes.c_float
    return F(_lib.wloop_atanf(float(F(x))))


def i64_to_f32(v):
    """(float)(int64): one rounding to nearest, ties to even (exact integer arithmetic, no double in between)"""
    v = int(v)
    a = abs(v)
    if a >= 1 << 24:
        sh = a.bit_length() - 24
        q, r = a >> sh, a & ((1 << sh) - 1)
        half = 1 << (sh - 1)
        if r > half or (r == half and (q & 1)):
            q += 1
        a = q << sh
    return F(-a if v < 0 else a)


def make_cfg(n_coh, use_magnitude=True, spacing=8, dll=(1.0, 300.0), pll=(4.0, 3000.0), fll=0.0):
    return dict(n_coh=int(n_coh), use_magnitude=bool(use_magnitude), spacing=int(spacing), dll_c1=F(dll[0]), dll_c2=F(dll[1]),
                pll_c1=F(pll[0]), pll_c2=F(pll[1]), fll_c=F(fll))


def update(state, iq, cfg):
    """the loop arithmetic of one window on one channel's state (a STATE_DTYPE scalar view, modified in place): DLL, Costas PLL,
    FLL, carrier update, end of window.  iq: the six window sums."""
    IE, QE, IP, QP, IL, QL = (int(v) for v in iq)
    T_ = F(F(cfg["n_coh"]) * F(0.001))
    # DLL
    e2, l2 = IE * IE + QE * QE, IL * IL + QL * QL
    d = F(0.0) if e2 + l2 == 0 else F(i64_to_f32(e2 - l2) / i64_to_f32(e2 + l2))
    a = F(d - state["dll_err"])
    a = F(cfg["dll_c1"] * a)
    b = F(cfg["dll_c2"] * T_)
    b = F(b * d)
    corr = F(a + b)
    phase = F(state["code_phase_fine"] - corr)
    if phase < F(0.0):
        phase = F(phase + SPAN)
    elif phase >= SPAN:
        phase = F(phase - SPAN)
    state["code_phase_fine"] = phase
    state["dll_err"] = d
    # Costas PLL, cycles
    if IP == 0:
        p = F(0.25) if QP > 0 else (F(-0.25) if QP < 0 else F(0.0))
    else:
        p = F(atanf(F(F(QP) / F(IP))) * CYCLES)
    # FLL, Hz
    fe = F(0.0)
    if cfg["fll_c"] != F(0.0) and int(state["n_updates"]) > 0:
        pi, pq = int(state["prev_ip"]), int(state["prev_qp"])
        cross, dot = pi * QP - pq * IP, pi * IP + pq * QP
        if dot != 0:
            fe = F(atanf(F(i64_to_f32(cross) / i64_to_f32(dot))) * CYCLES)
            fe = F(fe / T_)
    a = F(p - state["pll_err"])
    a = F(cfg["pll_c1"] * a)
    b = F(cfg["pll_c2"] * T_)
    b = F(b * p)
    c = F(a + b)
    c = F(c + F(cfg["fll_c"] * fe))
    state["if_freq_offset_hz"] = F(state["if_freq_offset_hz"] - c)
    state["pll_err"] = p
    state["prev_ip"] = IP
    state["prev_qp"] = QP
    state["n_updates"] = (int(state["n_updates"]) + 1) & 0xFFFFFFFF


def run(oracle, blocks_2bit, states, cfg, if_hz=4092000, channels=None):
    """n_blocks / n_coh windows on `states` (a STATE_DTYPE array, modified in place) -> REC_DTYPE [windows][n_ch].  `channels`:
    only these are advanced (the others' states and records are left alone / zero)."""
    blks = np.asarray(blocks_2bit, np.uint8).reshape(-1, 4092)
    n_coh = cfg["n_coh"]
    assert states.dtype == STATE_DTYPE and len(blks) % n_coh == 0
    todo = list(range(len(states))) if channels is None else sorted({int(c) for c in channels})
    n_win = len(blks) // n_coh
    rec = np.zeros((n_win, len(states)), REC_DTYPE)
    with np.errstate(all="ignore"):
        for u in range(n_win):
            trk = np.zeros(len(todo), TRK_DTYPE)
            for f in ("prn", "code_phase_fine", "if_freq_offset_hz", "if_freq_accum"):
                trk[f] = states[f][todo]
            iq, acc = T.track(oracle, blks[u * n_coh:(u + 1) * n_coh], trk, cfg["use_magnitude"], cfg["spacing"], if_hz)
            sums = iq.astype(np.int64).sum(axis=0)
            for j, ch in enumerate(todo):
                st = states[ch:ch + 1]
                st["if_freq_accum"][0] = acc[j]
                bad = T.tau_of(trk["code_phase_fine"][j]) is None or not 1 <= int(trk["prn"][j]) <= 210
                if not bad:
                    view = {name: st[name] for name in STATE_DTYPE.names}
                    update(_Scalar(view), sums[j], cfg)
                rec[u, ch] = (sums[j], st["code_phase_fine"][0], st["if_freq_offset_hz"][0], st["if_freq_accum"][0])
    return rec


class _Scalar:
    """one channel's fields of a structured array as a mapping (reads give numpy scalars, writes go to the array)"""

    def __init__(self, views):
        self.v = views

    def __getitem__(self, k):
        return self.v[k][0]

    def __setitem__(self, k, x):
        self.v[k][0] = x


def handover(prn, phase, offset_hz, accum=0):
    """a zeroed state with the four fields a grid record fills"""
    st = np.zeros(1, STATE_DTYPE)
    st[0]["prn"], st[0]["code_phase_fine"], st[0]["if_freq_offset_hz"], st[0]["if_freq_accum"] = prn, phase, offset_hz, accum
    return st
