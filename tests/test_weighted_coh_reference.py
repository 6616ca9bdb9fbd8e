"""The weighted two-bit grid over n_coh coherently integrated blocks (include/gpsx.h gpsx_acq_grid_weighted_coh), without a GPU:
the exact CPU restatement its GPU tests compare against (tests/weighted_coh_ref.py) pinned three ways -- to the oracle's one-block
weighted grid at n_coh = 1, to a direct sample-by-sample sum over the oracle's wipe-off with the NCO accumulator chained (checked
against its closed form), and to exact roots and the fold at the top of the range -- plus the host planner (plan_acq_coherent,
compiled with g++), the exported entry points and the kernels' resources."""
import math
import os
import subprocess

import numpy as np
import pytest

import weighted_coh_ref as R
import weighted_ms_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _blocks(n, amp=0.3, seed=3):
    from stm32f4_sdr_gps_amd import synth
    sats = [synth.Sat(7, 1310.0, 4321.0, amp, 0.4), synth.Sat(19, -2240.0, 12007.0, amp, 2.0)]
    return synth.make_if_static(n, sats, noise_amp=1.0, seed=seed, two_bit=True)


@pytest.mark.parametrize("use_mag", [True, False])
def test_reference_at_one_block_is_the_oracle_grid(oracle, use_mag):
    blocks = _blocks(3)
    prns = np.array([7, 19, 3], np.uint8)
    want = oracle.acq_grid_weighted(blocks, 3, prns, 1000, 500, 2, use_mag, stride_blocks=1, n_threads=4)
    got = R.grid(oracle, blocks, 3, prns, 1, 1000, 500, 2, use_mag, stride=1)
    for f in ("max_val", "phase", "sum", "avr"):
        assert np.array_equal(got[f], want[f]), f


@pytest.mark.parametrize("n_coh", [2, 7, 20])
def test_reference_is_the_chained_sample_sum(oracle, n_coh):
    blocks = _blocks(n_coh + 1, seed=9)
    rng = np.random.default_rng(n_coh)
    for _ in range(2):
        first, prn, d = int(rng.integers(0, 2)), int(rng.integers(1, 33)), int(rng.integers(-10, 11))
        use_mag = bool(rng.integers(0, 2))
        f = 4092000 + 500 * d
        step32 = (oracle.nco_step(f) * 32) & 0xFFFFFFFF
        # the direct sum: every block wiped from the closed-form accumulator b * 511 * step32, which is what the chain leaves
        vals = []
        for b in range(n_coh):
            acc_b = (b * 511 * step32) & 0xFFFFFFFF
            sign, mag = W.planes(blocks[first + b])
            di, dq, acc_out = oracle.wipeoff(np.packbits(sign, bitorder="little"), f, acc_b)
            assert acc_out == ((b + 1) * 511 * step32) & 0xFFFFFFFF
            w = 1 + 2 * mag.astype(np.int64) if use_mag else np.ones(16368, np.int64)
            vi = (2 * np.unpackbits(di.view(np.uint8), bitorder="little")[:16368].astype(np.int64) - 1) * w
            vq = (2 * np.unpackbits(dq.view(np.uint8), bitorder="little")[:16368].astype(np.int64) - 1) * w
            vi[16352:] = 0
            vq[16352:] = 0
            vals.append((vi, vq))
        c = np.repeat(1 - 2 * oracle.ca_code(prn).astype(np.int64), 16)
        i, q = R.iq(oracle, blocks, first, n_coh, prn, f, use_mag)
        for tau in rng.integers(0, 16368, 4):
            rep = c[(np.arange(16368) - int(tau)) % 16368]
            assert (int(i[tau]), int(q[tau])) == (sum(int(vi @ rep) for vi, _ in vals), sum(int(vq @ rep) for _, vq in vals))


@pytest.mark.parametrize("kind", ["all_ff", "code_matched"])
def test_root_and_fold_exact_at_the_top_of_the_range(oracle, kind):
    prn, f = 5, 4092000 + 1500
    blocks = np.full((20, 4092), 0xFF, np.uint8) if kind == "all_ff" else R.code_matched_blocks(oracle, prn, f, 20)
    i, q = R.iq(oracle, blocks, 0, 20, prn, f)
    if kind == "code_matched":
        assert i[0] == 3 * 16352 * 20
        assert int(i[0]) ** 2 + int(q[0]) ** 2 >= 1 << 39
    e = [int(a) * int(a) + int(b) * int(b) for a, b in zip(i, q)]
    assert max(e) < 1 << 41
    m = [math.isqrt(v) for v in e]
    assert W.isqrt(i * i + q * q).tolist() == m
    s = sum(m) % (1 << 32)
    want = (max(m), m.index(max(m)), s, s // 16368)
    got = R.grid(oracle, blocks, 1, [prn], 20, 1500, 500, 1)[0, 0, 0]
    assert tuple(int(got[k]) for k in ("max_val", "phase", "sum", "avr")) == want


DRIVER = r"""
#include "gpsx_acq_plan.hpp"
#include <stdio.h>
using namespace gpsx;
int main()
{
  AcqWShape g;
  int vec;
  while (scanf("%d %d %d %d %d", &g.n_search, &g.n_ms, &g.n_prn, &g.n_dopp, &vec) == 5) {
    g.vector = vec;
    const AcqWPlan p = plan_acq_coherent(g);
    printf("%s %d %ld %ld %d %zu\n", p.name, (int)p.mx, p.units, p.grid, p.n_chunks, p.scratch_bytes);
  }
  return 0;
}
"""

# (n_search, n_coh, n_prn, n_dopp, vector) -> kernel mx units grid n_chunks scratch
ROWS = [
    ((256, 10, 32, 21, 0), "k_acq_coh_mx 1 5376 5376 1 0"),          # the chip-filling launch: a workgroup per cluster
    ((256, 20, 32, 21, 0), "k_acq_coh_mx 1 5376 5376 1 0"),          # n_coh does not change the launch
    ((1, 10, 40, 3, 0), "k_acq_coh_mx 1 6 6 1 0"),                   # 40 PRNs: two 32-PRN sets
    ((1, 2, 1, 1, 0), "k_acq_coh_mx 1 1 1 1 0"),
    ((256, 10, 32, 21, 1), "k_acq_coh_vec 0 21504 21504 1 0"),       # vector ALU: 8-PRN groups
    ((1, 10, 40, 3, 1), "k_acq_coh_vec 0 15 15 1 0"),
    ((256, 1, 32, 21, 0), "k_acq_mxw 1 5376 5376 1 0"),              # n_coh = 1: the one-block kernels
    ((256, 1, 32, 21, 1), "k_acq_weighted 0 21504 21504 1 0"),
    ((1, 1, 40, 3, 0), "k_acq_mxw 1 6 6 1 0"),
]


def test_plan_acq_coherent_table(tmp_path):
    src, exe = tmp_path / "drv.cpp", tmp_path / "drv"
    src.write_text(DRIVER)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "stm32f4_sdr_gps_amd", "csrc"), str(src), "-o", str(exe)])
    stdin = "".join(" ".join(map(str, r[0])) + "\n" for r in ROWS)
    out = subprocess.run([str(exe)], input=stdin, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(ROWS)
    for (shape, want), got in zip(ROWS, out):
        assert got == want, (shape, got, want)


def test_library_exports_the_coherent_entry_points(lib_path):
    syms = subprocess.check_output(["nm", "-D", "--defined-only", lib_path], text=True)
    names = {line.split()[-1] for line in syms.splitlines() if line.strip()}
    assert {"gpsx_acq_grid_weighted_coh", "gpsx_acq_grid_weighted_coh_dev"} <= names


def test_coherent_kernels_have_no_scratch(lib_path):
    from stm32f4_sdr_gps_amd import build
    res = build.check_no_scratch()
    for name in ("k_acq_coh_mx", "k_acq_coh_vec"):
        hits = [v for k, v in res.items() if name in k]
        assert len(hits) == 1 and hits[0]["scratch_bytes"] == 0, (name, hits)
        assert hits[0]["lds_bytes"] <= 160 * 1024
