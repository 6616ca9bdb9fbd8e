"""What the closed weighted loop's CPU and GPU tests share (include/gpsx.h gpsx_track_loop_weighted): the pull-in scenario, the loop
configurations it runs with, and the launch shapes of k_track_wloop with what csrc/gpsx_track_loop_weighted_plan.hpp makes of
each -- tests/test_track_loop_weighted_plan.py compiles that header with g++ and asserts every row without a GPU; the GPU tests ask
the same compiled function what they are running."""
import os
import subprocess
import tempfile

import numpy as np

import weighted_loop_ref as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- the pull-in scenario ------------------------------------------------------------------------------------------------------
PRN, FD, DELAY, CARRIER_PHASE = 7, 1310.0, 4321.0, 0.4
REST = FD * (1.0 + 1.0 / 1022.0)      # where the carrier loop rests: the NCO mixes 16 352 of a block's 16 368 samples
AMPLITUDE = 0.035                     # the lowest of {0.1, 0.07, 0.05, 0.035} at which n_coh = 20 decodes every bit on SEEDS
SEEDS = (1, 2, 3)
# the handover errors of a _coh-style record per seed: code phase within 3 samples, carrier within 250 / n_coh Hz (n_coh = 20)
HANDOVER = {1: (3.0, 12.5), 2: (-3.0, -12.5), 3: (2.0, 7.0)}
PULL_IN_MS = 200
# gains.  A window of T seconds turns the loops into sampled ones: omega_n T stays well below 1.  Carrier, steady state (T = 20 ms):
# omega_n = 15 rad/s, zeta = 0.7 -> c1 = 2 zeta omega_n = 21, c2 = omega_n^2 = 225; pull-in (T = 4 ms): omega_n = 40 -> 56, 1600,
# with a tenth of the measured frequency error fed back per window.  Code: the reference's PI form, slowed down as T grows.
PULL_IN = dict(n_coh=4, dll=(1.0, 100.0), pll=(56.0, 1600.0), fll=0.1)
STEADY = dict(n_coh=20, dll=(0.5, 40.0), pll=(21.0, 225.0), fll=0.0)
REFERENCE_1MS = dict(n_coh=1, dll=(1.0, 300.0), pll=(4.0, 3000.0), fll=0.0)   # the reference's gains, its 1 ms update


def scenario(amp, seed, n_ms):
    """n_ms two-bit blocks of PRN 7 with 20 ms data bits and the bits: window u of 20 blocks holds bit u (the bit edge sits DELAY
    samples into the window's first block, where the code period starts)"""
    from stm32f4_sdr_gps_amd import synth
    rng = np.random.default_rng(1000 + seed)
    bits = rng.integers(0, 2, n_ms // 20 + 1) * 2.0 - 1.0
    blocks = synth.make_if(n_ms, [synth.Sat(PRN, FD, DELAY, amp, CARRIER_PHASE, nav_bits=bits)], noise_amp=1.0, seed=seed, two_bit=True)
    return blocks, bits


def handover_state(seed, carrier_scale=1.0):
    d_phase, d_hz = HANDOVER[seed]
    return L.handover(PRN, DELAY + d_phase, FD + d_hz * carrier_scale)


def bit_errors(records, bits, first_bit, n_ms):
    """records: [(first block, n_coh, REC array)] of channel 0 -> mismatches between the signs of the 20 ms prompt sums and the data
    bits from `first_bit` on, up to one global polarity"""
    sums = {}
    for at, n_coh, r in records:
        for u in range(len(r)):
            b = (at + u * n_coh) // 20
            sums[b] = sums.get(b, 0) + int(r["iq"][u, 0, 2])
    n_bits = n_ms // 20
    got = np.array([1.0 if sums[b] > 0 else -1.0 for b in range(first_bit, n_bits)])
    want = bits[first_bit:n_bits]
    return min(int((got != want).sum()), int((got != -want).sum())), n_bits - first_bit


def tail_errors(records, n_ms):
    """(largest |code phase - DELAY|, largest |carrier - REST|) over the windows that start in the run's last quarter"""
    ph, hz = [], []
    for at, n_coh, r in records:
        for u in range(len(r)):
            if at + u * n_coh >= 0.75 * n_ms:
                ph.append(float(r["code_phase_fine"][u, 0]))
                hz.append(float(r["if_freq_offset_hz"][u, 0]))
    return float(np.abs(np.array(ph) - DELAY).max()), float(np.abs(np.array(hz) - REST).max())


# ---- launch shapes -------------------------------------------------------------------------------------------------------------
# (n_ch, cpw, workgroups, channels of the last active wave, idle waves of the last workgroup): every cpw the plan can choose,
# waves filled partly and fully, workgroups with idle waves
SHAPES = [
    (1, 1, 1, 1, 3), (3, 1, 1, 1, 1), (5, 1, 2, 1, 3), (64, 1, 16, 1, 0), (257, 1, 65, 1, 3),
    (8195, 2, 1025, 1, 2), (12291, 3, 1025, 3, 3), (16389, 4, 1025, 1, 2), (20490, 5, 1025, 5, 2), (24583, 6, 1025, 1, 2),
    (28700, 7, 1025, 7, 0), (32771, 8, 1025, 3, 3), (36870, 9, 1025, 6, 3), (40990, 10, 1025, 10, 1), (45058, 11, 1025, 2, 3),
    (49170, 12, 1025, 6, 2), (53250, 13, 1025, 2, 3), (57350, 14, 1025, 6, 3), (61475, 15, 1025, 5, 1), (65536, 16, 1024, 16, 0),
    (70003, 16, 1094, 3, 0),
]
ROWS = {r[0]: r[1:] for r in SHAPES}

DRIVER = r"""
#include "gpsx_track_loop_weighted_plan.hpp"
#include <stdio.h>
int main()
{
  int n_ch;
  while (scanf("%d", &n_ch) == 1) {
    const gpsx::TrackLoopWeightedPlan p = gpsx::plan_track_loop_weighted(n_ch);
    printf("%d %u\n", p.cpw, p.groups);
  }
  return 0;
}
"""

_exe = None
_tmp = None
_cache = {}


def plans(counts):
    """[(cpw, workgroups)] from the header itself (compiled once per process)"""
    global _exe, _tmp
    counts = [int(c) for c in counts]
    new = [c for c in dict.fromkeys(counts) if c not in _cache]
    if new:
        if _exe is None:
            _tmp = tempfile.TemporaryDirectory(prefix="track_loop_weighted_plan_")
            src, _exe = os.path.join(_tmp.name, "plan.cpp"), os.path.join(_tmp.name, "plan")
            with open(src, "w") as f:
                f.write(DRIVER)
            subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "stm32f4_sdr_gps_amd", "csrc"),
                                   "-o", _exe, src])
        out = subprocess.run([_exe], input="".join(f"{c}\n" for c in new), capture_output=True, text=True, check=True).stdout
        lines = out.splitlines()
        assert len(lines) == len(new)
        for c, line in zip(new, lines):
            cpw, groups = line.split()
            _cache[c] = (int(cpw), int(groups))
    return [_cache[c] for c in counts]


def tabled(n_ch):
    """cpw of a launch the GPU tests make -- which must be a row above, so that the CPU test has asserted its shape"""
    assert n_ch in ROWS, f"{n_ch} channels are launched but not in tests/weighted_loop_cases.py"
    cpw, groups = plans([n_ch])[0]
    assert (cpw, groups) == ROWS[n_ch][:2]
    return cpw


def geometry(n_ch, cpw, groups):
    """What the kernel's indexing makes of a plan: wave w of workgroup g starts at channel (4 g + w) cpw, is idle when that is
    >= n_ch and serves min(cpw, n_ch - start) channels otherwise -> (channels of the last active wave, idle waves)"""
    starts = [(4 * g + w) * cpw for g in range(groups) for w in range(4)]
    active = [s for s in starts if s < n_ch]
    assert sum(min(cpw, n_ch - s) for s in active) == n_ch
    idle = len(starts) - len(active)
    assert 0 <= idle < 4 and all(s >= n_ch for s in starts[len(active):])
    return min(cpw, n_ch - active[-1]), idle
