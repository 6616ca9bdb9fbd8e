"""The single-block fine grid with its chip operand resident in registers (k_acq_mx<0>, DESIGN.md 4.1 "resident chips";
csrc/gpsx_mx_parts.hpp: MxChipRegs).  A lane keeps the 16 x 32 chips of its own (PRN, K half) from the anchor pass to the last
recurrence pass of a cluster, so what can go wrong is a chip fragment in the wrong register, or registers that hold another PRN
set's chips -- the neighbouring set of a launch, or whatever the previous workgroup on the CU left.  Either is a wrong triplet
somewhere, so every record and key is compared bit for bit with the CPU oracle computed live.

Every case is 1 or 2 captures x 1 or 2 Doppler bins (the launch that reaches the split form repeats two captures 84 times).
"""
import numpy as np
import pytest

from conftest import oracle_threads
from golden_util import IF_HZ

ORC_THREADS = oracle_threads()
FIELDS = ("max_val", "phase", "sum", "avr")
DOPP2 = dict(dopp_min_hz=-1500, dopp_step_hz=4000, n_dopp=2)
DOPP1 = dict(dopp_min_hz=-1500, dopp_step_hz=4000, n_dopp=1)
# 32 PRNs of set 0, five of a second, partly filled set; and a second full set for the launches that alternate
PRNS37 = np.concatenate([np.arange(1, 33), [33, 61, 120, 150, 210]]).astype(np.uint8)
PRNS_B = np.arange(64, 96, dtype=np.uint8)
# chip offsets whose two byte offsets are a window: the first and last column of a fragment's K half (kappa = 0 / 7 | 8), the
# fold's columns 1021 / 1022 (kappa = 15)
EDGE_Q = (0, 1, 511, 512, 1021, 1022)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def monkeypatch_module():
    mp = pytest.MonkeyPatch()
    yield mp
    mp.undo()


@pytest.fixture(scope="module")
def eng(monkeypatch_module):
    """The lab library with $GPSX_ACQ_NO_SPLIT: launches of a handful of clusters stay one workgroup per cluster (k_acq_mx<0>)."""
    from stm32f4_sdr_gps_amd import capi
    monkeypatch_module.setenv("GPSX_ACQ_NO_SPLIT", "1")
    e = capi.Engine(0, lab=True)
    monkeypatch_module.delenv("GPSX_ACQ_NO_SPLIT")
    yield e
    e.close()


@pytest.fixture(scope="module")
def orc():
    from oracle import pyoracle
    return pyoracle.Oracle()


@pytest.fixture(scope="module")
def caps():
    """Two captures at the bench's amplitude: (sign planes, the same samples as 2-bit IF)"""
    from stm32f4_sdr_gps_amd import synth
    return synth.cold_start_block(2, seed=83, amp_scale=0.25), synth.cold_start_block(2, seed=83, amp_scale=0.25, two_bit=True)


@pytest.fixture(scope="module")
def want37(orc, caps):
    """The oracle's triplets of both captures for the 37 PRNs, computed once: a PRN's rows do not depend on its place in a list, so
    every PRN list below is a selection of these rows.  -> [capture][PRN index in PRNS37, bin, bit shift]"""
    sign = caps[0]
    return [orc.acq_grid(sign[i:i + 1], 1, PRNS37, DOPP2["dopp_min_hz"], DOPP2["dopp_step_hz"], 2, 8, n_threads=ORC_THREADS, live=True)
            for i in range(2)]


def _keys(want):
    from stm32f4_sdr_gps_amd import sharding
    return sharding.pack_keys(want["max_val"], want["phase"])


def _grid(e, blocks, prns, two_bit=False, **kw):
    from stm32f4_sdr_gps_amd import capi
    if two_bit:
        e.set_if_format(capi.IF_2BIT_SM)
    try:
        pk, keys = e.acq_grid(blocks, prns, n_search=len(blocks), **kw)
    finally:
        e.set_if_format(capi.IF_1BIT)
    assert e.lib.gpsx_last_kernel(e.h) == b"k_acq_mx<0>"
    return pk, keys


def _check(pk, keys, want):
    assert len(pk) == len(want)
    for i, w in enumerate(want):
        for f in FIELDS:
            assert np.array_equal(pk[i][f], w[f]), (i, f)
        assert np.array_equal(keys[i], _keys(w)), i


def _rows_differ(a, b):
    return any(not np.array_equal(a[f], b[f]) for f in FIELDS)


# ---- 1. PRN lists: whose chips are in the registers ---------------------------------------------------------------------------------------
def _prn_lists():
    rng = np.random.default_rng(5)
    return {"1": np.arange(1), "31": np.arange(31), "32": np.arange(32), "33": np.arange(33), "37": np.arange(37),
            "32_reversed": np.arange(32)[::-1].copy(), "32_shuffled": rng.permutation(32)}


@pytest.mark.parametrize("name", list(_prn_lists()))
def test_prn_lists(eng, caps, want37, name):
    """One capture x 2 bins: lists of 1, 31, 32, 33 and 37 PRNs -- lanes without a PRN, a second set of one and of five PRNs, whose
    registers must hold THAT set's chips -- and the 32 PRNs of a set reversed and shuffled: PRN p of the list is lane p's."""
    pick = _prn_lists()[name]
    want = want37[0][pick]
    # the premises, from the oracle alone: no two PRNs of the list share their rows, so a lane with another lane's chips -- the
    # same lane of the other set, or the lane a permutation moved -- is a mismatch
    for a in range(len(pick)):
        for b in range(a + 1, len(pick)):
            assert _rows_differ(want[a], want[b]), (a, b)
    pk, keys = _grid(eng, caps[0][:1], PRNS37[pick], **DOPP2)
    _check(pk, keys, [want])


# ---- 2. the edges of kappa -------------------------------------------------------------------------------------------------------------------
def _windowed(orc, block, prns, dopp, win):
    """The oracle's windowed search_job per (PRN, bin, bit shift) -> triplets [n_prn, n_dopp, 8]"""
    from stm32f4_sdr_gps_amd import capi
    want = np.zeros((len(prns), dopp["n_dopp"], 8), capi.PEAK_DTYPE)
    for p in range(len(prns)):
        code = orc.ca_code(int(prns[p]))
        for d in range(dopp["n_dopp"]):
            freq = float(IF_HZ + dopp["dopp_min_hz"] + dopp["dopp_step_hz"] * d)
            for b in range(8):
                peak, _, _ = orc.search_job(block, 1, code, freq, b, win[0], win[1])
                want[p, d, b] = tuple(peak[f] for f in FIELDS)
    return want


@pytest.mark.parametrize("q", EDGE_Q)
def test_kappa_edges(eng, orc, caps, q):
    """Windows of the two byte offsets of ONE chip offset q: every record of the launch is the correlation at q alone, where chip
    column c meets vector entry q + c -- at q = 0 column 0 of kappa = 0 meets entry 0, at q = 1021 / 1022 the fold's columns meet the
    wrap.  32 PRNs x 2 bins x 8 bit shifts, each a sum over all sixteen fragments of its lane."""
    prns = PRNS37[:32]
    win = (2 * q, 2 * q + 2)
    want = _windowed(orc, caps[0][:1], prns, DOPP2, win)
    assert (want["max_val"] > 0).any(axis=(1, 2)).all()   # (from the oracle alone: every PRN has a window whose maximum is not zero)
    pk, keys = _grid(eng, caps[0][:1], prns, win=win, **DOPP2)
    _check(pk, keys, [want])


# ---- 3. the preamble's paths -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("two_bit", [False, True], ids=["if_1bit", "if_2bit"])
def test_both_if_formats(eng, caps, want37, two_bit):
    """Two captures x 2 bins x 37 PRNs = 8 clusters, as sign planes and as 2-bit IF: the block's load differs, the chips do not."""
    pk, keys = _grid(eng, caps[1] if two_bit else caps[0], PRNS37, two_bit=two_bit, **DOPP2)
    _check(pk, keys, want37)


def test_a_shard_that_cuts_a_cluster(eng, caps, want37):
    """One capture x 2 bins x 32 PRNs = 8 units: the second third of them leaves a workgroup with some of its four 8-PRN groups --
    all 32 lanes keep their chips, the foreign groups' results are not published."""
    from stm32f4_sdr_gps_amd import sharding
    want = want37[0][:32]
    mine = sharding.owned_mask(1, 32, 2, 1, 3)[0]                  # [n_prn, n_dopp]
    assert mine.any() and not mine.all()
    assert any(0 < mine[:, d].sum() < 32 for d in range(2))       # (a cluster -- one bin's 32 PRNs -- is cut)
    pk, keys = _grid(eng, caps[0][:1], PRNS37[:32], shard=(1, 3), **DOPP2)
    for f in FIELDS:
        assert np.array_equal(pk[0][f][mine], want[f][mine]), f
        assert not pk[0][f][~mine].any(), f
    assert np.array_equal(keys[0][mine], _keys(want)[mine]) and not keys[0][~mine].any()


PLAN_DRIVER = r"""
#include "gpsx_acq_plan.hpp"
#include <stdio.h>
#include <stdlib.h>
using namespace gpsx;
int main(int argc, char **argv)
{
  AcqShape g{};
  g.n_search = 168, g.n_ms = 1, g.n_prn = 32, g.n_dopp = 2, g.n_bits = 8;
  AcqKnobs kn{};
  kn.algo = 4;
  const AcqPlan p = plan_acq(g, kn, atoi(argv[1]), 0);
  printf("%d %ld %ld %d %s\n", p.form == AcqForm::kMxTail, p.grid, p.grid_tail, p.split_segs, p.name);
  return 0;
}
"""


def _plan_of_the_tail_launch(tmp_path, n_cus):
    """What the library's own planner (csrc/gpsx_acq_plan.hpp, compiled for the host as tests/test_acq_plan.py does) makes of
    168 searches x 2 bins x 32 PRNs on n_cus compute units -> (is the tail form, workgroups of k_acq_mx<0>, of k_acq_mx<5>, segments)"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src, exe = tmp_path / "plan.cpp", tmp_path / "plan"
    src.write_text(PLAN_DRIVER)
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-I", os.path.join(root, "stm32f4_sdr_gps_amd", "csrc"), str(src), "-o", str(exe)])
    tail, grid, grid_tail, segs, name = subprocess.check_output([str(exe), str(n_cus)], text=True).split()
    assert name == "k_acq_mx<0>"
    return bool(int(tail)), int(grid), int(grid_tail), int(segs)


def test_last_round_in_the_split_form(caps, want37, tmp_path):
    """The product library, 168 searches x 2 bins x 32 PRNs = 336 clusters on 256 CUs: 256 workgroups of k_acq_mx<0> and the 80
    clusters of the last round in the split form (k_acq_mx<5>, which reads its chips from LDS in every pass) in ONE launch.  The
    searches are the two captures in turn, so every record of all 168 is compared with the oracle's two.  gpsx_last_kernel names
    the launch's first kernel only, so the premise -- this shape is planned as full rounds plus a split tail -- is taken from the
    library's planner itself, at the device's own number of compute units."""
    from stm32f4_sdr_gps_amd import capi
    blocks = np.tile(caps[0], (84, 1))
    e = capi.Engine(0)
    try:
        n_cus = e.device_info()[1]   # (what gpsx_acq_grid_dev hands the planner)
        assert _plan_of_the_tail_launch(tmp_path, n_cus) == (True, 256, 160, 2), n_cus
        pk, keys = _grid(e, blocks, PRNS37[:32], **DOPP2)
    finally:
        e.close()
    _check(pk, keys, [want37[i & 1][:32] for i in range(168)])


# ---- 4. registers left over from another workgroup ------------------------------------------------------------------------------------------------
def test_ten_identical_launches(eng, caps, want37):
    """The 2-bit launch of both captures ten times: byte-identical peaks and keys, the first run's equal to the oracle's."""
    first = None
    for run in range(10):
        pk, keys = _grid(eng, caps[1], PRNS37, two_bit=True, **DOPP2)
        if first is None:
            first = (pk.tobytes(), keys.tobytes())
            _check(pk, keys, want37)
        else:
            assert pk.tobytes() == first[0] and keys.tobytes() == first[1], run


def test_set_a_then_b_then_a(eng, orc, caps, want37):
    """PRN set A, then another 32 PRNs on the same capture, then A again: the first and third launch are byte-identical and equal
    to the oracle, and so is the second -- a workgroup that met a CU's registers as the previous set left them shows here."""
    sign = caps[0][:1]
    want_a = want37[0][:32]
    want_b = orc.acq_grid(sign, 1, PRNS_B, DOPP1["dopp_min_hz"], DOPP1["dopp_step_hz"], 1, 8, n_threads=ORC_THREADS, live=True)
    assert all(_rows_differ(want_a[p][:1], want_b[p]) for p in range(32))   # (a lane's two PRNs never agree)
    runs = []
    for prns, want in ((PRNS37[:32], want_a[:, :1]), (PRNS_B, want_b), (PRNS37[:32], want_a[:, :1])):
        pk, keys = _grid(eng, sign, prns, **DOPP1)
        _check(pk, keys, [want])
        runs.append((pk.tobytes(), keys.tobytes()))
    assert runs[0] == runs[2]
