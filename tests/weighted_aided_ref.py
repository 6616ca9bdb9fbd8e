"""An exact CPU restatement of the carrier-aided weighted loops (include/gpsx.h gpsx_track_loop_weighted_aided,
gpsx_track_loop_weighted_sync_aided), for the tests.  It stands on weighted_loop_ref and weighted_sync_ref as they are: the block
loops, the correlators, the synchroniser and everything of the window update but the code phase are theirs, run with this module's
`update` in the place of weighted_loop_ref.update for the duration of a call (weighted_sync_ref._channel calls it through its own
`L`, weighted_loop_ref.run through its module's name).  The aiding factor travels in the gains' dict as "code_per_hz"; the unaided
restatements never read that key and their outputs are what they were.  Nothing of the library's kernel code is included or
imported."""
import contextlib

import numpy as np

import weighted_loop_ref as L
import weighted_sync_ref as Y

F = np.float32
WAID_L1CA = F(0.010389610)     # GPSX_WAID_L1CA


def aided_phase(code_phase_fine, dll_err, iq, cfg, if_freq_offset_hz, code_per_hz):
    """the DLL step with the aiding clause: one IEEE single operation per line, in the header's order -> (phase, d)"""
    IE, QE, _, _, IL, QL = (int(v) for v in iq)
    T_ = F(F(cfg["n_coh"]) * F(0.001))
    e2, l2 = IE * IE + QE * QE, IL * IL + QL * QL
    d = F(0.0) if e2 + l2 == 0 else F(L.i64_to_f32(e2 - l2) / L.i64_to_f32(e2 + l2))
    a = F(d - F(dll_err))
    a = F(cfg["dll_c1"] * a)
    b = F(cfg["dll_c2"] * T_)
    b = F(b * d)
    corr = F(a + b)
    phase = F(F(code_phase_fine) - corr)
    k = F(code_per_hz)
    if k != F(0.0):
        step = F(k * F(if_freq_offset_hz))      # per window: the factor times the offset the window ran with ...
        step = F(step * T_)                     # ... times the window's length
        phase = F(phase - step)
    if phase < F(0.0):
        phase = F(phase + L.SPAN)
    elif phase >= L.SPAN:
        phase = F(phase - L.SPAN)
    return phase, d


_unaided_update = L.update


def update(state, iq, cfg):
    """weighted_loop_ref.update with the aiding clause in its DLL step.  cfg["code_per_hz"] absent or 0: that function, untouched."""
    k = F(cfg.get("code_per_hz", 0.0))
    if k == F(0.0):
        return _unaided_update(state, iq, cfg)
    with np.errstate(all="ignore"):
        phase, _ = aided_phase(state["code_phase_fine"], state["dll_err"], iq, cfg, state["if_freq_offset_hz"], k)   # (before the carrier step)
    _unaided_update(state, iq, cfg)        # dll_err, the carrier, the loop memory: as they are there
    state["code_phase_fine"] = phase


@contextlib.contextmanager
def _with_aided_update():
    assert L.update is _unaided_update
    L.update = update
    try:
        yield
    finally:
        L.update = _unaided_update


def loop_cfg(cfg, code_per_hz):
    """a weighted_loop_ref.make_cfg dict with the factor"""
    return dict(cfg, code_per_hz=F(code_per_hz))


def sync_cfg(cfg, code_per_hz):
    """a weighted_sync_ref.make_cfg dict with the factor in both gain sets (the same for SEARCH and LOCKED windows)"""
    return dict(cfg, search=dict(cfg["search"], code_per_hz=F(code_per_hz)), lock=dict(cfg["lock"], code_per_hz=F(code_per_hz)))


def run(oracle, blocks_2bit, states, cfg, code_per_hz, if_hz=4092000, channels=None):
    """weighted_loop_ref.run with the aiding clause: gpsx_track_loop_weighted_aided"""
    with _with_aided_update():
        return L.run(oracle, blocks_2bit, states, loop_cfg(cfg, code_per_hz), if_hz, channels)


def run_sync(oracle, blocks_2bit, states, cfg, code_per_hz, if_hz=4092000, channels=None, events=None):
    """weighted_sync_ref.run with the aiding clause: gpsx_track_loop_weighted_sync_aided.  A bad channel and a channel in WAIT end
    no window, so they take no step."""
    with _with_aided_update():
        return Y.run(oracle, blocks_2bit, states, sync_cfg(cfg, code_per_hz), if_hz, channels, events)
