"""The weighted two-bit grid over n_ms blocks (include/gpsx.h gpsx_acq_grid_weighted_ms), without a GPU: the exact CPU
restatement its GPU tests compare against (tests/weighted_ms_ref.py) pinned three ways -- to the oracle's one-block weighted grid,
to the oracle's sample-by-sample I and Q, and to the record's fold rules on hand-made sums -- plus the host planner that picks the
kernels, grids, chunks and scratch (plan_acq_weighted, compiled with g++) and the library's exported entry points."""
import os
import subprocess

import numpy as np
import pytest

import weighted_ms_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _blocks(n_ms, amp=0.3, seed=3):
    from stm32f4_sdr_gps_amd import synth
    sats = [synth.Sat(7, 1310.0, 4321.0, amp, 0.4), synth.Sat(19, -2240.0, 12007.0, amp, 2.0)]
    return synth.make_if_static(n_ms, sats, noise_amp=1.0, seed=seed, two_bit=True)


@pytest.mark.parametrize("use_mag", [True, False])
def test_reference_at_one_block_is_the_oracle_grid(oracle, use_mag):
    blocks = _blocks(3)
    prns = np.array([7, 19, 3], np.uint8)
    want = oracle.acq_grid_weighted(blocks, 3, prns, 1000, 500, 2, use_mag, stride_blocks=1, n_threads=4, )
    got = R.grid(oracle, blocks, 3, prns, 1, 1000, 500, 2, use_mag, stride=1)
    for f in ("max_val", "phase", "sum", "avr"):
        assert np.array_equal(got[f], want[f]), f


def test_reference_iq_is_the_oracle_definition(oracle):
    blocks = _blocks(2, seed=9)
    rng = np.random.default_rng(4)
    for _ in range(6):
        b, prn, d = int(rng.integers(0, 2)), int(rng.integers(1, 33)), int(rng.integers(-10, 11))
        use_mag = bool(rng.integers(0, 2))
        i, q = R.iq(oracle, blocks[b], prn, 4092000 + 500 * d, use_mag)
        for tau in rng.integers(0, 16368, 5):
            assert oracle.weighted_iq(blocks[b], prn, 4092000 + 500 * d, int(tau), use_mag) == (int(i[tau]), int(q[tau]))


def test_fold_rules_on_hand_made_sums():
    e = np.zeros(16368, np.int64)
    assert R.fold(e) == (0, 0, 0, 0)
    e[[5, 900, 16367]] = 7                                  # ties: the smallest phase
    assert R.fold(e) == (7, 5, 21, 0)
    e[:] = 128 * 69375                                      # the top of E's range: the sum wraps at 2^32
    s = (16368 * 128 * 69375) % (1 << 32)
    assert R.fold(e) == (128 * 69375, 0, s, s // 16368)
    e[16000] += 1
    assert R.fold(e)[:2] == (128 * 69375 + 1, 16000)
    # the exact root at the edges of f64's square root
    x = np.array([0, 1, 2, 3, 4, 15, 16, 2896 ** 2 * 2, (1 << 32) + 5, 2 * 49056 ** 2, 2 * 49056 ** 2 - 1], np.int64)
    import math
    assert R.isqrt(x).tolist() == [math.isqrt(int(v)) for v in x]


DRIVER = r"""
#include "gpsx_acq_plan.hpp"
#include <stdio.h>
using namespace gpsx;
int main()
{
  AcqWShape g;
  AcqKnobs kn;
  int vec, refused;
  while (scanf("%d %d %d %d %d %d %d", &g.n_search, &g.n_ms, &g.n_prn, &g.n_dopp, &vec, &kn.wms_scratch_mb, &refused) == 7) {
    g.vector = vec;
    const AcqWPlan p = plan_acq_weighted(g, kn, 256, refused);
    if (p.enomem)
      printf("ENOMEM\n");
    else
      printf("%s %ld %ld %d %ld %zu\n", p.name, p.units, p.chunk, p.n_chunks, p.grid, p.scratch_bytes);
  }
  return 0;
}
"""

MB = 1 << 20
C = 2 * MB   # scratch per cluster of the matrix walk
# (n_search, n_ms, n_prn, n_dopp, vector, scratch cap MB (0: default 2048), refused) -> kernel units chunk n_chunks grid scratch
ROWS = [
    ((256, 1, 32, 21, 0, 0, 0), f"k_acq_mxw 5376 5376 1 5376 0"),                       # one block: the existing kernel
    ((256, 10, 32, 21, 0, 0, 0), f"k_acq_wmx_ms 5376 1024 6 1024 {1024 * C}"),          # 2 GB: four rounds of 256 CUs
    ((1, 10, 32, 21, 0, 0, 0), f"k_acq_wmx_ms 21 21 1 21 {21 * C}"),                    # a lone search
    ((1, 10, 40, 3, 0, 0, 0), f"k_acq_wmx_ms 6 6 1 6 {6 * C}"),                         # two 32-PRN sets
    ((64, 10, 32, 21, 0, 1024, 0), f"k_acq_wmx_ms 1344 512 3 512 {512 * C}"),           # the lab cap: three chunks
    ((64, 10, 32, 21, 0, 100, 0), f"k_acq_wmx_ms 1344 50 27 50 {50 * C}"),              # below a round: not rounded
    ((64, 10, 32, 21, 0, 1, 0), "ENOMEM"),                                               # not one cluster under the cap
    ((256, 10, 32, 21, 0, 0, 1), f"k_acq_wmx_ms 5376 512 11 512 {512 * C}"),            # refused: halves
    ((256, 10, 32, 21, 0, 0, 3), f"k_acq_wmx_ms 5376 128 42 128 {128 * C}"),
    ((256, 10, 32, 21, 0, 0, 10), f"k_acq_wmx_ms 5376 1 5376 1 {C}"),
    ((256, 10, 32, 21, 0, 0, 11), "ENOMEM"),
    ((1, 10, 32, 21, 0, 0, 4), f"k_acq_wmx_ms 21 1 21 1 {C}"),
    ((1, 10, 32, 21, 0, 0, 5), "ENOMEM"),
    ((256, 1, 32, 21, 1, 0, 0), "k_acq_weighted 21504 21504 1 21504 0"),                # vector ALU: 8-PRN groups
    ((256, 10, 32, 21, 1, 0, 0), "k_acq_weighted_ms 21504 21504 1 21504 0"),            # no scratch, one launch
    ((1, 128, 40, 3, 1, 1, 7), "k_acq_weighted_ms 15 15 1 15 0"),                       # (no scratch: cap and refusals moot)
]


def test_plan_acq_weighted_table(tmp_path):
    src, exe = tmp_path / "drv.cpp", tmp_path / "drv"
    src.write_text(DRIVER)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "stm32f4_sdr_gps_amd", "csrc"), str(src), "-o", str(exe)])
    stdin = "".join(" ".join(map(str, r[0])) + "\n" for r in ROWS)
    out = subprocess.run([str(exe)], input=stdin, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(ROWS)
    for (shape, want), got in zip(ROWS, out):
        assert got == want, (shape, got, want)


def test_library_exports_the_multi_block_entry_points(lib_path):
    syms = subprocess.check_output(["nm", "-D", "--defined-only", lib_path], text=True)
    names = {line.split()[-1] for line in syms.splitlines() if line.strip()}
    assert {"gpsx_acq_grid_weighted_ms", "gpsx_acq_grid_weighted_ms_dev", "gpsx_acq_grid_weighted", "gpsx_acq_grid_weighted_dev"} <= names
