"""The cases that the shape tests of the eight weighted acquisition kernels share (tests/test_gpu_weighted_grid_shapes.py on the GPU,
tests/test_weighted_grid_cases_reference.py and tests/test_acq_weighted_plan.py without one): PRN lists whose lengths sit on the
kernels' edges -- groups of 8 on the vector ALU, sets of 32 on the matrix cores, the documented maximum of 255 -- with PRN 1 in
slot 0, PRN 210 in the last slot and duplicates across groups and sets; which records of such a list a test restates; the block
at the top of the one-block range; a capture whose hybrid sum passes 2^32; a call whose chunk edges fall inside a (search,
Doppler) pair's sets and across a search; and the g++ driver over csrc/gpsx_acq_plan.hpp's weighted planners.  The premises are
asserted in tests/test_weighted_grid_cases_reference.py, on the restatements alone."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IF_HZ = 4092000
GROUP, SET = 8, 32                      # PRNs per workgroup: k_acq_weighted* / k_acq_coh_vec / k_acq_hyb_vec, and the matrix kernels
LENGTHS = (1, 8, 9, 32, 33, 64, 65, 255)
SEED = 2046
CLUSTER_MB = 2                          # kMxwMsClusterBytes: a cluster's running sums in the scratch walks


def prn_list(n):
    """n PRNs drawn with a fixed seed from 2..209 (without repeats up to 208 of them, the rest drawn freely: the 255-list repeats
    PRNs by itself), then: PRN 1 into slot 0, PRN 210 into the last slot (a list of one is [210]: the table's last row in the
    only slot), from 9 on PRN 210 also into one of slots 1..7 -- the same PRN in the first group and the last, from 33 on in the
    first set and the last --, and from 65 on the PRN of one of slots 8..31 again in one of slots 32..63"""
    rng = np.random.default_rng([SEED, n])
    pool = rng.permutation(np.arange(2, 210))
    p = np.concatenate([pool, rng.integers(2, 210, max(n - len(pool), 0))])[:n].astype(np.uint8)
    p[0] = 1
    p[n - 1] = 210
    if n >= GROUP + 1:
        p[1 + int(rng.integers(0, 7))] = 210
    if n >= 2 * SET + 1:
        p[SET + int(rng.integers(0, SET))] = p[GROUP + int(rng.integers(0, SET - GROUP))]
    return p


def duplicates(prns):
    """[[slots of one PRN], ...] for every PRN the list holds more than once"""
    prns = np.asarray(prns)
    return [np.flatnonzero(prns == v).tolist() for v in np.unique(prns) if (prns == v).sum() > 1]


def edge_slots(prns):
    """the first and the last slot of every group of 8 (a set of 32 starts and ends with one), then every slot of a repeated PRN"""
    n = len(prns)
    slots = sorted({s for g in range(0, n, GROUP) for s in (g, min(g + GROUP - 1, n - 1))} | {s for d in duplicates(prns) for s in d})
    return slots


def sample_units(prns, n_search, n_dopp):
    """(search, slot, Doppler) triples to restate of a call on this list: every edge_slots slot -- the list's first and last slot
    in every (search, Doppler) pair, any other in one pair, the pairs taken in turn"""
    pairs = [(s, d) for s in range(n_search) for d in range(n_dopp)]
    units = []
    for i, slot in enumerate(edge_slots(prns)):
        for s, d in (pairs if slot in (0, len(prns) - 1) else [pairs[i % len(pairs)]]):
            units.append((s, slot, d))
    return units


def noisy_blocks(n, amp=0.3, seed=3):
    """the existing weighted-grid tests' capture: three weak satellites in noise"""
    from stm32f4_sdr_gps_amd import synth
    sats = [synth.Sat(7, 1310.0, 4321.0, amp, 0.4), synth.Sat(19, -2240.0, 12007.0, amp, 2.0), synth.Sat(30, 2018.0, 13000.0, amp, 4.0)]
    return synth.make_if_static(n, sats, noise_amp=1.0, seed=seed, two_bit=True)


# ---- the top of the one-block range -------------------------------------------------------------------------------------------
TOP_PRN, TOP_DOPP_HZ, TOP_I = 8, 1310, 3 * 16352          # include/gpsx.h: |I| <= 49 056 in one block


def matched_block(oracle):
    """one block whose wiped I samples are 3 x PRN 8's replica at phase 0 in the bin of 1310 Hz: I(0) = 49 056, Q(0) = 0"""
    import weighted_coh_ref as R
    return R.code_matched_blocks(oracle, TOP_PRN, IF_HZ + TOP_DOPP_HZ, 1)


# ---- a hybrid sum past 2^32 --------------------------------------------------------------------------------------------------
WRAP_N_COH, WRAP_N_SEG, WRAP_PRNS, WRAP_DOPP_HZ = 20, 128, (7, 8), 1310
WRAP_SEGS = (64, 128)      # at 64 windows the sum sits between 2^31 and 2^32 (the top bit of a u32 total), at 128 it has passed 2^32


def wrap_capture():
    """2560 blocks: twenty random blocks with every magnitude bit set, 128 times over -- every window of a 20 x 128 search is the
    same, so E = 128 m and the sum over the phases is 128 x (about 35 million)"""
    base = np.random.default_rng(7).integers(0, 256, (WRAP_N_COH, 4092), dtype=np.uint8) | np.uint8(0xAA)
    return np.tile(base, (WRAP_N_SEG, 1))


def wrap_energy(oracle, prn):
    """{n_seg: E(tau)} of the wrapping capture's one search at 64 and at 128 windows, int64 and unwrapped (the second 64 windows
    are restated as well and added to the first)"""
    import weighted_hyb_ref as H
    cap, half = wrap_capture(), WRAP_SEGS[0]
    first = H.energy(oracle, cap, 0, WRAP_N_COH, half, prn, IF_HZ + WRAP_DOPP_HZ)
    return {half: first, WRAP_N_SEG: first + H.energy(oracle, cap, half * WRAP_N_COH, WRAP_N_COH, WRAP_N_SEG - half, prn, IF_HZ + WRAP_DOPP_HZ)}


# ---- chunk edges inside a (search, Doppler) pair and across a search ----------------------------------------------------------
# 2 searches x 40 PRNs (two sets, the second partial) x 3 Doppler bins: 12 clusters, set fastest, then Doppler, then search
CHUNK = dict(n_search=2, n_prn=40, n_dopp=3, stride=1, dopp_min_hz=-2240, dopp_step_hz=1775, n_ms=3, n_coh=2, n_seg=3)
CHUNK_CAPS_MB = {2: 12, 6: 4, 10: 3, 14: 2}            # scratch cap -> launches
CHUNK_REFUSED_MB = 1                                   # not one cluster's scratch: GPSX_ENOMEM


def chunk_prns():
    return np.arange(1, CHUNK["n_prn"] + 1, dtype=np.uint8)


def decode_cluster(c, n_sets, n_dopp):
    """(search, Doppler bin, set) of cluster c (csrc/gpsx_mx_parts.hpp mx_decode_cluster)"""
    return c // n_sets // n_dopp, c // n_sets % n_dopp, c % n_sets


def launches(units, chunk):
    """[(first cluster, clusters)] of a walk planned at `chunk` clusters a launch: the last launch takes the rest"""
    return [(lo, min(chunk, units - lo)) for lo in range(0, units, chunk)]


# ---- the weighted planners on the host ------------------------------------------------------------------------------------------
PLAN_DRIVER = r"""
#include "gpsx_acq_plan.hpp"
#include <stdio.h>
using namespace gpsx;
static const char *form_name(AcqWForm f)
{
  switch (f) {
  case AcqWForm::kMxw: return "kMxw";
  case AcqWForm::kMxwWalk: return "kMxwWalk";
  case AcqWForm::kVec: return "kVec";
  case AcqWForm::kVecMs: return "kVecMs";
  case AcqWForm::kCohMx: return "kCohMx";
  case AcqWForm::kCohVec: return "kCohVec";
  case AcqWForm::kHybMx: return "kHybMx";
  case AcqWForm::kHybVec: return "kHybVec";
  }
  return "?";
}
int main()
{
  char call;
  int n_search, n_a, n_seg, n_prn, n_dopp, vector, cap_mb, refused;
  while (scanf(" %c %d %d %d %d %d %d %d %d", &call, &n_search, &n_a, &n_seg, &n_prn, &n_dopp, &vector, &cap_mb, &refused) == 9) {
    AcqKnobs kn;
    kn.wms_scratch_mb = cap_mb;
    const AcqWShape g{n_search, n_a, n_prn, n_dopp, vector != 0};
    const AcqWPlan p = call == 'w' ? plan_acq_weighted(g, kn, 256, refused)
                     : call == 'c' ? plan_acq_coherent(g)
                                   : plan_acq_hybrid(AcqHShape{n_search, n_a, n_seg, n_prn, n_dopp, vector != 0}, kn, 256, refused);
    printf("%s %d %d %ld %ld %d %ld %zu %s\n", form_name(p.form), (int)p.mx, (int)p.enomem, p.units, p.chunk, p.n_chunks, p.grid,
           p.scratch_bytes, p.name ? p.name : "-");
  }
  return 0;
}
"""
PLAN_FIELDS = ("form", "mx", "enomem", "units", "chunk", "n_chunks", "grid", "scratch_bytes", "name")


def plan_rows(tmp_path, rows):
    """rows of (call 'w' | 'c' | 'h', n_search, n_ms or n_coh, n_seg, n_prn, n_dopp, vector, scratch cap in MB or 0, refused)
    through plan_acq_weighted / plan_acq_coherent / plan_acq_hybrid at 256 CUs -> one dict of PLAN_FIELDS per row"""
    src = tmp_path / "acq_weighted_plan.cpp"
    src.write_text(PLAN_DRIVER)
    exe = tmp_path / "acq_weighted_plan"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "stm32f4_sdr_gps_amd", "csrc"),
                           "-o", str(exe), str(src)])
    lines = "".join(" ".join(map(str, row)) + "\n" for row in rows)
    out = subprocess.run([str(exe)], input=lines, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(rows)
    plans = []
    for line in out:
        f = line.split()
        plans.append(dict(form=f[0], mx=int(f[1]), enomem=int(f[2]), units=int(f[3]), chunk=int(f[4]), n_chunks=int(f[5]),
                          grid=int(f[6]), scratch_bytes=int(f[7]), name=f[8]))
    return plans


def chunk_plan_rows():
    """the chunk call under each cap and under the refused one, as _ms and as _hyb, for plan_rows"""
    c = CHUNK
    rows = []
    for cap in list(CHUNK_CAPS_MB) + [CHUNK_REFUSED_MB]:
        rows.append(("w", c["n_search"], c["n_ms"], 0, c["n_prn"], c["n_dopp"], 0, cap, 0))
        rows.append(("h", c["n_search"], c["n_coh"], c["n_seg"], c["n_prn"], c["n_dopp"], 0, cap, 0))
    return rows
