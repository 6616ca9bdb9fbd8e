"""The weighted two-bit grid over n_seg coherent windows of n_coh blocks, the windows' magnitudes summed (include/gpsx.h
gpsx_acq_grid_weighted_hyb), without a GPU: the exact CPU restatement its GPU tests compare against (tests/weighted_hyb_ref.py)
pinned three ways -- to the coherent restatement at n_seg = 1 and the non-coherent one at n_coh = 1, to a direct sample-by-sample
sum over the oracle's wipe-off with the NCO accumulator restarted at 0 at every segment's first block, and to Python-integer roots
and the fold at the top of the range -- plus the host planner (plan_acq_hybrid, compiled with g++), the exported entry points and
the kernels' resources."""
import math
import os
import subprocess

import numpy as np
import pytest

import weighted_coh_ref as R
import weighted_hyb_ref as H
import weighted_ms_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("max_val", "phase", "sum", "avr")


def _blocks(n, amp=0.3, seed=3):
    from stm32f4_sdr_gps_amd import synth
    sats = [synth.Sat(7, 1310.0, 4321.0, amp, 0.4), synth.Sat(19, -2240.0, 12007.0, amp, 2.0)]
    return synth.make_if_static(n, sats, noise_amp=1.0, seed=seed, two_bit=True)


@pytest.mark.parametrize("use_mag", [True, False])
def test_one_segment_is_the_coherent_restatement(oracle, use_mag):
    blocks = _blocks(6)
    prns = np.array([7, 19, 3], np.uint8)
    want = R.grid(oracle, blocks, 3, prns, 4, 1000, 250, 2, use_mag, stride=1)          # overlapping searches
    got = H.grid(oracle, blocks, 3, prns, 4, 1, 1000, 250, 2, use_mag, stride=1)
    for f in FIELDS:
        assert np.array_equal(got[f], want[f]), f


@pytest.mark.parametrize("use_mag", [True, False])
def test_one_block_windows_are_the_non_coherent_restatement(oracle, use_mag):
    blocks = _blocks(6)
    prns = np.array([7, 19, 3], np.uint8)
    want = W.grid(oracle, blocks, 3, prns, 4, 1000, 500, 2, use_mag, stride=1)
    got = H.grid(oracle, blocks, 3, prns, 1, 4, 1000, 500, 2, use_mag, stride=1)
    for f in FIELDS:
        assert np.array_equal(got[f], want[f]), f


@pytest.mark.parametrize("n_seg", [2, 3])
@pytest.mark.parametrize("n_coh", [2, 7, 20])
def test_reference_restarts_the_accumulator_at_every_segment(oracle, n_coh, n_seg):
    """E(tau) at a few random tau against the direct sum: every block of every segment wiped from b * 511 * step32, b counted from
    the SEGMENT's first block -- a restatement that chained the accumulator across segments would differ"""
    blocks = _blocks(n_coh * n_seg + 1, seed=9)
    rng = np.random.default_rng(100 * n_coh + n_seg)
    for _ in range(2):
        first, prn, d = int(rng.integers(0, 2)), int(rng.integers(1, 33)), int(rng.integers(-10, 11))
        use_mag = bool(rng.integers(0, 2))
        f = 4092000 + 500 * d + 37
        step32 = (oracle.nco_step(f) * 32) & 0xFFFFFFFF
        c = np.repeat(1 - 2 * oracle.ca_code(prn).astype(np.int64), 16)
        taus = [int(t) for t in rng.integers(0, 16368, 3)]
        want = [0] * len(taus)
        for j in range(n_seg):
            si, sq = [0] * len(taus), [0] * len(taus)
            for b in range(n_coh):
                sign, mag = W.planes(blocks[first + j * n_coh + b])
                di, dq, _ = oracle.wipeoff(np.packbits(sign, bitorder="little"), f, (b * 511 * step32) & 0xFFFFFFFF)
                w = 1 + 2 * mag.astype(np.int64) if use_mag else np.ones(16368, np.int64)
                vi = (2 * np.unpackbits(di.view(np.uint8), bitorder="little")[:16368].astype(np.int64) - 1) * w
                vq = (2 * np.unpackbits(dq.view(np.uint8), bitorder="little")[:16368].astype(np.int64) - 1) * w
                vi[16352:] = 0
                vq[16352:] = 0
                for k, tau in enumerate(taus):
                    rep = c[(np.arange(16368) - tau) % 16368]
                    si[k] += int(vi @ rep)
                    sq[k] += int(vq @ rep)
            for k in range(len(taus)):
                want[k] += math.isqrt(si[k] * si[k] + sq[k] * sq[k])
        e = H.energy(oracle, blocks, first, n_coh, n_seg, prn, f, use_mag)
        assert [int(e[t]) for t in taus] == want, (first, prn, d, use_mag)


def test_root_and_fold_exact_at_the_top_of_the_range(oracle):
    prn, f, n_seg = 5, 4092000 + 1500, 3
    blocks = np.concatenate([R.code_matched_blocks(oracle, prn, f, 20)] * n_seg)
    e = [0] * 16368
    for j in range(n_seg):
        i, q = R.iq(oracle, blocks, 20 * j, 20, prn, f)
        assert i[0] == 981120
        for t, (a, b) in enumerate(zip(i, q)):
            e[t] += math.isqrt(int(a) * int(a) + int(b) * int(b))
    assert e[0] >= n_seg * 981120 and max(e) < 1 << 28
    s = sum(e) % (1 << 32)
    want = (max(e), e.index(max(e)), s, s // 16368)
    got = H.grid(oracle, blocks, 1, [prn], 20, n_seg, 1500, 500, 1)[0, 0, 0]
    assert tuple(int(got[k]) for k in FIELDS) == want


DRIVER = r"""
#include "gpsx_acq_plan.hpp"
#include <stdio.h>
#include <string.h>
using namespace gpsx;
static bool same(const AcqWPlan &a, const AcqWPlan &b)
{
  return a.form == b.form && a.mx == b.mx && a.enomem == b.enomem && a.units == b.units && a.chunk == b.chunk &&
         a.n_chunks == b.n_chunks && a.grid == b.grid && a.scratch_bytes == b.scratch_bytes && !strcmp(a.name ? a.name : "", b.name ? b.name : "");
}
int main()
{
  AcqHShape g;
  int vec, cap_mb, n_cus, refused;
  while (scanf("%d %d %d %d %d %d %d %d %d", &g.n_search, &g.n_coh, &g.n_seg, &g.n_prn, &g.n_dopp, &vec, &cap_mb, &n_cus, &refused) == 9) {
    g.vector = vec;
    AcqKnobs k;
    k.wms_scratch_mb = cap_mb;
    const AcqWPlan p = plan_acq_hybrid(g, k, n_cus, refused);
    // the older calls' plans for the same shape: n_seg = 1 -> the coherent call's, n_coh = 1 -> the non-coherent call's
    int old = -1;
    if (g.n_seg == 1)
      old = same(p, plan_acq_coherent(AcqWShape{g.n_search, g.n_coh, g.n_prn, g.n_dopp, g.vector}));
    else if (g.n_coh == 1)
      old = same(p, plan_acq_weighted(AcqWShape{g.n_search, g.n_seg, g.n_prn, g.n_dopp, g.vector}, k, n_cus, refused));
    printf("%s %d %d %ld %ld %d %ld %zu %d\n", p.name ? p.name : "-", (int)p.mx, (int)p.enomem, p.units, p.chunk, p.n_chunks, p.grid,
           p.scratch_bytes, old);
  }
  return 0;
}
"""

MB = 1 << 20
# (n_search, n_coh, n_seg, n_prn, n_dopp, vector, cap MB (0: default 2048), CUs, refused)
#   -> kernel mx enomem units chunk n_chunks grid scratch same-as-the-older-call (-1: not a degenerate shape)
ROWS = [
    # the chip-filling shape: 5376 clusters of 2 MB; the default cap holds 1024 = four rounds of 256 CUs -> six launches
    ((256, 10, 8, 32, 21, 0, 0, 256, 0), f"k_acq_hyb_mx 1 0 5376 1024 6 1024 {2048 * MB} -1"),
    ((256, 10, 8, 32, 21, 1, 0, 256, 0), "k_acq_hyb_vec 0 0 21504 21504 1 21504 0 -1"),          # registers: one launch, no scratch
    ((256, 10, 8, 32, 21, 0, 0, 256, 1), f"k_acq_hyb_mx 1 0 5376 512 11 512 {1024 * MB} -1"),    # every refusal halves the chunk
    ((256, 10, 8, 32, 21, 0, 0, 256, 2), f"k_acq_hyb_mx 1 0 5376 256 21 256 {512 * MB} -1"),
    ((256, 10, 8, 32, 21, 0, 0, 256, 11), "k_acq_hyb_mx 1 1 5376 0 0 0 0 -1"),                   # 1024 >> 11 = 0: GPSX_ENOMEM
    ((256, 10, 8, 32, 21, 1, 0, 256, 11), "k_acq_hyb_vec 0 0 21504 21504 1 21504 0 -1"),         # (the vector form asks for none)
    ((256, 10, 8, 32, 21, 0, 1024, 256, 0), f"k_acq_hyb_mx 1 0 5376 512 11 512 {1024 * MB} -1"), # the lab knob's cap
    ((256, 10, 8, 32, 21, 0, 100, 256, 0), f"k_acq_hyb_mx 1 0 5376 50 108 50 {100 * MB} -1"),    # below one round: what the cap holds
    ((64, 20, 4, 32, 21, 0, 0, 256, 0), f"k_acq_hyb_mx 1 0 1344 1024 2 1024 {2048 * MB} -1"),    # exceeds the cap: two launches
    ((1, 2, 2, 40, 3, 0, 0, 256, 0), f"k_acq_hyb_mx 1 0 6 6 1 6 {12 * MB} -1"),                  # 40 PRNs: two sets per (search, bin)
    ((1, 2, 2, 40, 3, 1, 0, 256, 0), "k_acq_hyb_vec 0 0 15 15 1 15 0 -1"),
    # one window: the coherent call's plan (and at n_coh = 1 the one-block kernels)
    ((256, 10, 1, 32, 21, 0, 0, 256, 0), "k_acq_coh_mx 1 0 5376 5376 1 5376 0 1"),
    ((256, 10, 1, 32, 21, 1, 0, 256, 0), "k_acq_coh_vec 0 0 21504 21504 1 21504 0 1"),
    ((3, 1, 1, 40, 3, 0, 0, 256, 0), "k_acq_mxw 1 0 18 18 1 18 0 1"),
    ((3, 1, 1, 40, 3, 1, 0, 256, 0), "k_acq_weighted 0 0 45 45 1 45 0 1"),
    # windows of one block: the non-coherent call's plan with n_ms = n_seg, its chunks and its refusals
    ((256, 1, 20, 32, 21, 0, 0, 256, 0), f"k_acq_wmx_ms 1 0 5376 1024 6 1024 {2048 * MB} 1"),
    ((256, 1, 20, 32, 21, 0, 1024, 256, 1), f"k_acq_wmx_ms 1 0 5376 256 21 256 {512 * MB} 1"),
    ((256, 1, 20, 32, 21, 0, 0, 256, 11), "k_acq_wmx_ms 1 1 5376 0 0 0 0 1"),
    ((256, 1, 128, 32, 21, 1, 0, 256, 0), "k_acq_weighted_ms 0 0 21504 21504 1 21504 0 1"),
]


def test_plan_acq_hybrid_table(tmp_path):
    src, exe = tmp_path / "drv.cpp", tmp_path / "drv"
    src.write_text(DRIVER)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "stm32f4_sdr_gps_amd", "csrc"), str(src), "-o", str(exe)])
    stdin = "".join(" ".join(map(str, r[0])) + "\n" for r in ROWS)
    out = subprocess.run([str(exe)], input=stdin, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(ROWS)
    for (shape, want), got in zip(ROWS, out):
        assert got == want, (shape, got, want)


def test_library_exports_the_hybrid_entry_points(lib_path):
    syms = subprocess.check_output(["nm", "-D", "--defined-only", lib_path], text=True)
    names = {line.split()[-1] for line in syms.splitlines() if line.strip()}
    assert {"gpsx_acq_grid_weighted_hyb", "gpsx_acq_grid_weighted_hyb_dev"} <= names


def test_hybrid_kernels_have_no_scratch(lib_path):
    from stm32f4_sdr_gps_amd import build
    res = build.check_no_scratch()
    for name in ("k_acq_hyb_mx", "k_acq_hyb_vec"):
        hits = [v for k, v in res.items() if name in k]
        assert len(hits) == 1 and hits[0]["scratch_bytes"] == 0, (name, hits)
        assert hits[0]["lds_bytes"] <= 160 * 1024
