"""The launch shapes tests/test_gpu_weighted_track_shapes.py runs k_track_epl_weighted at, with what
csrc/gpsx_track_weighted_plan.hpp makes of each: cpw (channels a wave serves one after the other), the workgroups of four waves,
the channels of the last active wave (ragged when fewer than cpw), the idle waves of the last workgroup, and whether cpw was set
by the ceil(n_ch / 4) bound.  tests/test_track_weighted_plan.py compiles the header with g++ and asserts every row without a GPU;
the GPU tests ask the same compiled function what they are running."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (n_ch, n_blocks, cpw, workgroups, channels of the last active wave, idle waves of the last workgroup, set by the bound)
# every cpw from 2 to 16 with a ragged last wave, and the benchmark's 212 992 channels (cpw 16, nothing ragged)
SHAPES = [
    (8195, 1, 2, 1025, 1, 2, False),
    (4099, 3, 3, 342, 1, 1, False),
    (1367, 9, 3, 114, 2, 0, False),
    (1367, 12, 4, 86, 3, 2, False),
    (4099, 5, 5, 205, 4, 0, False),
    (2731, 9, 6, 114, 1, 0, False),
    (821, 35, 7, 30, 2, 2, False),
    (821, 40, 8, 26, 5, 1, False),
    (1171, 32, 9, 33, 1, 1, False),
    (1171, 35, 10, 30, 1, 2, False),
    (1171, 39, 11, 27, 5, 1, False),
    (1171, 42, 12, 25, 7, 2, False),
    (1171, 46, 13, 23, 1, 1, False),
    (1171, 49, 14, 21, 9, 0, False),
    (1171, 53, 15, 20, 1, 1, False),
    (70003, 1, 16, 1094, 3, 0, False),
    (212992, 1, 16, 3328, 16, 0, False),
]

# few channels, many blocks.  The first four: n_ch x n_blocks / 4096 exceeds ceil(n_ch / 4), which then IS cpw; the last two stay
# just below their bound (6 and 12)
FEW = [
    (61, 4096, 16, 1, 13, 0, True),
    (37, 4096, 10, 1, 7, 0, True),
    (5, 4096, 2, 1, 1, 1, True),
    (2, 4096, 1, 1, 1, 2, True),
    (23, 900, 5, 2, 3, 3, False),
    (45, 700, 7, 2, 3, 1, False),
]

# the other launches of the GPU tests: what the K-split identities of SHAPES and FEW launch (one block; ceil(K / 4) blocks;
# eight pieces of ceil(K / 8) blocks and the remainders 109 and 84 of the last piece), the seam matrix (8219 and 107 channels),
# the PRN sweep (210), bad channels (1367 x 12 above; 7 x 1), stream order (4099 x 20, x 4, x 1), both steps (300 and 8195, x 1)
OTHER = [
    (4099, 1, 1, 1025, 1, 1, False), (1367, 1, 1, 342, 1, 1, False), (2731, 1, 1, 683, 1, 1, False), (821, 1, 1, 206, 1, 3, False),
    (1171, 1, 1, 293, 1, 1, False),
    (1367, 3, 1, 342, 1, 1, False), (4099, 2, 2, 513, 1, 2, False), (2731, 3, 2, 342, 1, 2, False), (821, 9, 1, 206, 1, 3, False),
    (821, 8, 1, 206, 1, 3, False), (821, 10, 2, 103, 1, 1, False), (1171, 8, 2, 147, 1, 2, False), (1171, 9, 2, 147, 1, 2, False),
    (1171, 10, 2, 147, 1, 2, False), (1171, 11, 3, 98, 1, 1, False), (1171, 12, 3, 98, 1, 1, False), (1171, 13, 3, 98, 1, 1, False), (1171, 14, 4, 74, 3, 3, False),
    (61, 512, 7, 3, 5, 3, False), (37, 512, 4, 3, 1, 2, False), (5, 512, 1, 2, 1, 3, False), (2, 512, 1, 1, 1, 2, False),
    (23, 113, 1, 6, 1, 1, False), (23, 109, 1, 6, 1, 1, False), (45, 88, 1, 12, 1, 3, False), (45, 84, 1, 12, 1, 3, False),
    (8219, 1, 2, 1028, 1, 2, False), (107, 1, 1, 27, 1, 1, False), (210, 1, 1, 53, 1, 2, False), (7, 1, 1, 2, 1, 1, False),
    (4099, 20, 16, 65, 3, 3, False), (4099, 4, 4, 257, 3, 3, False), (300, 1, 1, 75, 1, 0, False),
]

DRIVER = r"""
#include "gpsx_track_weighted_plan.hpp"
#include <stdio.h>
int main()
{
  int n_ch, n_blocks;
  while (scanf("%d %d", &n_ch, &n_blocks) == 2) {
    const gpsx::TrackWeightedPlan p = gpsx::plan_track_weighted(n_ch, n_blocks);
    printf("%d %u %d\n", p.cpw, p.groups, (int)p.spread_bound);
  }
  return 0;
}
"""

ROWS = {(r[0], r[1]): r[2:] for r in SHAPES + FEW + OTHER}

_exe = None
_tmp = None     # the compiled driver's directory, removed when the process ends
_cache = {}


def tabled(n_ch, n_blocks):
    """cpw of a launch the GPU tests make -- which must be a row above, so that the CPU test has asserted its shape"""
    assert (n_ch, n_blocks) in ROWS, f"({n_ch}, {n_blocks}) is launched but not in tests/weighted_track_shapes.py"
    cpw, groups, bound = plan(n_ch, n_blocks)
    assert (cpw, groups, bound) == (ROWS[(n_ch, n_blocks)][0], ROWS[(n_ch, n_blocks)][1], ROWS[(n_ch, n_blocks)][4])
    return cpw


def plan(n_ch, n_blocks):
    """(cpw, workgroups, set by the bound) of one launch, from the header itself (compiled once per process)"""
    return plans([(n_ch, n_blocks)])[0]


def plans(pairs):
    global _exe, _tmp
    pairs = [(int(a), int(b)) for a, b in pairs]
    new = [p for p in dict.fromkeys(pairs) if p not in _cache]
    if new:
        if _exe is None:
            _tmp = tempfile.TemporaryDirectory(prefix="track_weighted_plan_")
            src, _exe = os.path.join(_tmp.name, "plan.cpp"), os.path.join(_tmp.name, "plan")
            with open(src, "w") as f:
                f.write(DRIVER)
            subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "stm32f4_sdr_gps_amd", "csrc"),
                                   "-o", _exe, src])
        out = subprocess.run([_exe], input="".join(f"{a} {b}\n" for a, b in new), capture_output=True, text=True, check=True).stdout
        lines = out.splitlines()
        assert len(lines) == len(new)
        for p, line in zip(new, lines):
            cpw, groups, bound = line.split()
            _cache[p] = (int(cpw), int(groups), bound == "1")
    return [_cache[p] for p in pairs]


def geometry(n_ch, cpw, groups):
    """What the kernel's indexing makes of a plan: wave w of workgroup g starts at channel ch0 = (4 g + w) cpw, is idle when
    ch0 >= n_ch and serves min(cpw, n_ch - ch0) channels otherwise -> (first channel of the last active wave, its channels,
    idle waves), after checking that the waves cover every channel once and only the last workgroup has idle waves"""
    starts = [(4 * g + w) * cpw for g in range(groups) for w in range(4)]
    active = [s for s in starts if s < n_ch]
    assert sum(min(cpw, n_ch - s) for s in active) == n_ch
    idle = len(starts) - len(active)
    assert 0 <= idle < 4 and all(s >= n_ch for s in starts[len(active):])
    return active[-1], min(cpw, n_ch - active[-1]), idle
