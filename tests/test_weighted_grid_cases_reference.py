"""The premises of tests/weighted_grid_cases.py, without a GPU and on the restatements alone: the PRN lists sit where they claim to
(lengths on the groups' and sets' edges, PRN 1 first, PRN 210 last, the same PRN in two groups and in two sets), the sampled
records hold every group's and set's first and last slot and every repeat, the matched block reaches the header's bound of one
block, the wrapping capture's sum passes 2^32, and the chunk call's launches -- from the host planner -- cut where the GPU test
needs them cut: inside a (search, Doppler) pair's sets and across a search."""
import numpy as np
import pytest

import weighted_grid_cases as G
import weighted_ms_ref as W


def test_lengths_sit_on_group_and_set_edges():
    assert G.LENGTHS == (1, 8, 9, 32, 33, 64, 65, 255)
    for k in (1, 4, 8):                                  # a full last group / set and one slot more, at 8 and at 32 PRNs
        assert G.GROUP * k in G.LENGTHS and G.GROUP * k + 1 in G.LENGTHS
    assert max(G.LENGTHS) == 255 and 255 % G.SET == 31 and 255 % G.GROUP == 7       # the maximum: a last set of 31, a last group of 7


@pytest.mark.parametrize("n", G.LENGTHS)
def test_prn_lists(n):
    p = G.prn_list(n)
    assert p.dtype == np.uint8 and len(p) == n and p.min() >= 1 and p.max() == 210
    assert np.array_equal(p, G.prn_list(n))                                         # a fixed seed
    assert p[-1] == 210 and (n == 1 or p[0] == 1)
    dups = G.duplicates(p)
    assert all(len(d) >= 2 and len(set(p[d].tolist())) == 1 for d in dups)
    assert sorted(s for d in dups for s in d) == [s for s in range(n) if (p == p[s]).sum() > 1]
    if n > G.GROUP:
        assert any(len({s // G.GROUP for s in d}) > 1 for d in dups), "no PRN in two groups of 8"
    if n > G.SET:
        assert any(len({s // G.SET for s in d}) > 1 for d in dups), "no PRN in two sets of 32"
    if n > 210:
        assert sum(len(d) - 1 for d in dups) >= n - 210                             # 255 slots from 210 PRNs
    if n > 2 * G.SET:
        assert any(p[d[0]] != 210 and len({s // G.SET for s in d}) > 1 for d in dups)   # a repeat that is not the forced 210


@pytest.mark.parametrize("n", G.LENGTHS)
def test_sampled_units_hold_every_edge_and_repeat(n):
    p = G.prn_list(n)
    units = G.sample_units(p, 2, 2)
    assert len(set(units)) == len(units) and all(0 <= s < 2 and 0 <= k < n and 0 <= d < 2 for s, k, d in units)
    slots = {k for _, k, _ in units}
    for first in range(0, n, G.GROUP):
        assert first in slots and min(first + G.GROUP - 1, n - 1) in slots
    for first in range(0, n, G.SET):
        assert first in slots and min(first + G.SET - 1, n - 1) in slots
    assert all(s in slots for d in G.duplicates(p) for s in d)
    for k in (0, n - 1):
        assert {(s, d) for s, kk, d in units if kk == k} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {(s, d) for s, _, d in units} == {(0, 0), (0, 1), (1, 0), (1, 1)}


def test_matched_block_is_the_top_of_the_one_block_range(oracle):
    blk = G.matched_block(oracle)
    assert blk.shape == (1, 4092)
    i, q = W.iq(oracle, blk[0], G.TOP_PRN, G.IF_HZ + G.TOP_DOPP_HZ)
    m = W.isqrt(i * i + q * q)
    assert G.TOP_I == 49056 and int(i[0]) == G.TOP_I and int(q[0]) == 0
    assert int(m.max()) == G.TOP_I and int(np.argmax(m)) == 0
    four = W.energy(oracle, np.tile(blk, (4, 1)), 0, G.TOP_PRN, G.IF_HZ + G.TOP_DOPP_HZ, 4, 0)
    assert W.fold(four)[:2] == (4 * G.TOP_I, 0)


def test_wrapping_capture_passes_2_to_the_32(oracle):
    cap = G.wrap_capture()
    assert cap.shape == (G.WRAP_N_COH * G.WRAP_N_SEG, 4092) and (cap & 0xAA == 0xAA).all()
    assert all((cap[k * G.WRAP_N_COH:(k + 1) * G.WRAP_N_COH] == cap[:G.WRAP_N_COH]).all() for k in range(G.WRAP_N_SEG))
    import weighted_hyb_ref as H
    by_seg = G.wrap_energy(oracle, G.WRAP_PRNS[0])
    e = by_seg[G.WRAP_N_SEG]
    assert np.array_equal(e, H.energy(oracle, cap, 0, G.WRAP_N_COH, G.WRAP_N_SEG, G.WRAP_PRNS[0], G.IF_HZ + G.WRAP_DOPP_HZ))
    total = int(e.sum())
    assert total >> 32 >= 1, total
    assert int(e.max()) < 1 << 28                                                    # E itself stays inside the header's bound
    assert W.fold(e)[2] == total - (total >> 32 << 32) != total
    half = int(by_seg[G.WRAP_SEGS[0]].sum())                                         # not wrapped, the top bit of a u32 set
    assert G.WRAP_SEGS == (64, 128) and 1 << 31 <= half < 1 << 32 and W.fold(by_seg[G.WRAP_SEGS[0]])[2] == half, half


def test_chunk_call_launches_cut_inside_pairs_and_across_a_search(tmp_path):
    c = G.CHUNK
    n_sets = -(-c["n_prn"] // G.SET)
    units = c["n_search"] * c["n_dopp"] * n_sets
    assert (n_sets, c["n_prn"] % G.SET, units) == (2, 8, 12)                         # two sets, the second partial
    assert c["n_ms"] > 1 and c["n_coh"] > 1 and c["n_seg"] == 3                      # both scratch walks; one middle segment
    order = [G.decode_cluster(k, n_sets, c["n_dopp"]) for k in range(units)]
    assert order[:4] == [(0, 0, 0), (0, 0, 1), (0, 1, 0), (0, 1, 1)] and order[6] == (1, 0, 0)      # set fastest, then Doppler, then search
    plans = G.plan_rows(tmp_path, G.chunk_plan_rows())
    caps = list(G.CHUNK_CAPS_MB) + [G.CHUNK_REFUSED_MB]
    assert caps == [2, 6, 10, 14, 1]
    for k, cap in enumerate(caps):
        for plan, form, name in ((plans[2 * k], "kMxwWalk", "k_acq_wmx_ms"), (plans[2 * k + 1], "kHybMx", "k_acq_hyb_mx")):
            assert (plan["form"], plan["name"], plan["mx"], plan["units"]) == (form, name, 1, units)
            if cap == G.CHUNK_REFUSED_MB:
                assert plan["enomem"] == 1
                continue
            per = cap // G.CLUSTER_MB
            assert (plan["enomem"], plan["chunk"], plan["n_chunks"]) == (0, per, G.CHUNK_CAPS_MB[cap])
            runs = G.launches(plan["units"], plan["chunk"])
            assert len(runs) == plan["n_chunks"] and sum(n for _, n in runs) == units
            searches = [{order[lo + j][0] for j in range(n)} for lo, n in runs]
            odd_start = [order[lo][2] == 1 for lo, _ in runs]
            assert any(len(s) == 2 for s in searches) == (per in (5, 7)), (per, runs)   # a launch holding a search boundary
            assert any(odd_start[1:]), (per, runs)                                      # a launch starting on the second set
            assert any(n > 1 for _, n in runs) == (per > 1)
    assert [G.launches(units, p) for p in (5, 7)] == [[(0, 5), (5, 5), (10, 2)], [(0, 7), (7, 5)]]
