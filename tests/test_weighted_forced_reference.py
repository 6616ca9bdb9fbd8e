"""The table of forced cases of the weighted loops' window update and bit-sync decision (tests/weighted_forced_cases.py), on the
CPU restatement alone: every row reaches the branch it names -- its predicate, evaluated on the integers and on the bits of the
restatement's outcome, proves it --, every window forced to a target has exactly the target's sums, every class of case is present,
nothing exceeds the 2^30 bound under which the definition's int64 expressions are exact, and the rows that are to end no window
end none.  tests/test_gpu_weighted_forced.py runs the same states through k_track_wsync, tests/test_gpu_weighted_loop.py the
k_track_wloop rows."""
import numpy as np
import pytest

import weighted_forced_cases as W
import weighted_sync_ref as Y


@pytest.mark.parametrize("group", sorted(W.GROUPS))
def test_every_row_takes_its_branch(oracle, group):
    rows, st0, cfg, rec, after, outcomes = W.restated(oracle, group)
    failed = []
    for o in outcomes:
        if not o.row.check(o):
            failed.append(o.row.name)
        window = (o.rec["flags"] & Y.F_WINDOW) != 0
        if o.row.target is not None:
            assert tuple(int(v) for v in W.first(o)["w"]["iq"]) == o.row.target, o.row.name
        assert window.any() == o.row.ends, o.row.name
    print(group, len(rows), "rows,", int(sum(o.row.ends for o in outcomes)), "end a window")
    assert not failed, failed     # 100 % of the rows: one that cannot meet its predicate is taken out of the table, not skipped


def test_every_class_of_case_is_present():
    tags = set()
    for group in W.GROUPS:
        for row in W.table(group):
            tags |= row.tags
    missing = [t for t in W.REQUIRED if t not in tags]
    assert not missing, missing
    assert len(W.REQUIRED) == len(set(W.REQUIRED)) and len(W.REQUIRED) > 100


def test_nothing_exceeds_the_bound(oracle):
    """|target|, |prev| <= 2^30: e2 + l2 <= 2^62 and |cross|, |dot| <= 2^61, no int64 expression of the definition overflows; and
    the preloaded win_iq = target - r is an int32"""
    for group in W.GROUPS:
        rows, st0, *_ = W.restated(oracle, group)
        for i, row in enumerate(rows):
            assert max(abs(row.prev[0]), abs(row.prev[1])) <= W.BOUND, row.name
            if row.target is not None:
                assert max(abs(v) for v in row.target) <= W.BOUND, row.name
                assert all(abs(t - int(w)) <= 49056 for t, w in zip(row.target, st0["win_iq"][i])), row.name
    assert any(row.target is not None and max(map(abs, row.target)) == W.BOUND for row in W.table("A"))


def test_the_masks_are_partial(oracle):
    """among any sixteen consecutive rows of a group (what a wave holds at most) some end a window and some do not; a bad channel
    sits in every dozen of group A's rows"""
    for group in W.GROUPS:
        rows, _, _, rec, _, _ = W.restated(oracle, group)
        ended = ((rec["flags"] & Y.F_WINDOW) != 0).any(axis=0)
        for at in range(0, max(1, len(rows) - 15)):
            part = ended[at:at + 16]
            assert part.any() and not part.all(), (group, at)
    bad = ["bad" in row.tags for row in W.table("A")]
    assert all(any(bad[at:at + 12]) for at in range(len(bad) - 11))


def test_the_table_cut_one_block_earlier(oracle):
    """the same targets reached over two launches of one block: the first ends no window, the second ends the target's"""
    cut = W.cut_rows("A")
    rows, cfg = W.table("A"), W.cfg_of("A")
    assert len(cut) > 60
    st = np.concatenate([W.state_of(oracle, rows[i], i, cfg, lead=2)[0] for i in cut])
    one = Y.run(oracle, W.blocks()[0:1], st, cfg)
    assert not one["flags"].any()
    two = Y.run(oracle, W.blocks()[1:2], st, cfg)
    for j, i in enumerate(cut):
        assert int(two[0, j]["flags"]) & Y.F_WINDOW and tuple(int(v) for v in two[0, j]["w"]["iq"]) == rows[i].target, rows[i].name


def test_the_tiling_moves_the_rows_through_the_lanes():
    for cpw, n_ch in ((1, 257), (2, 8195), (7, 28700), (16, 70003)):
        for n_rows in (len(W.table(g)) for g in W.GROUPS):
            idx = W.tiled(n_ch, n_rows, cpw)
            assert set(idx[:n_rows]) == set(range(n_rows)) and idx.max() == n_rows - 1
            if cpw > 1 and n_rows >= cpw:
                lanes = {(int(c) % cpw) for c in np.nonzero(idx == 0)[0][:4 * cpw]}
                assert len(lanes) == cpw, (cpw, n_rows)


def test_the_wloop_rows_hit_their_intervals(oracle):
    """k_track_wloop's rows (the FLL through a rotated prev, the wrap through phase and dll_err): what the first window's FLL and
    code-phase update meet, asserted on the integers"""
    names, st0, want, want_st, facts = W.wloop_table(oracle)
    seen = set()
    for f in facts:
        kind = f.name.split(":")
        if kind[0] == "fll" and f.c is not None:
            assert f.n > 0 and (f.cross, f.dot) == (-f.s * f.n, f.c * f.n), f.name
            if f.c == 0:
                assert f.dot == 0 and f.cross != 0
            elif f.s == 0:
                assert f.cross == 0 and (f.dot < 0) == (f.c < 0)
            elif len(kind) == 4:
                lim, side, sign = kind[1:]
                assert W.interval(f.q) == W.WLOOP_INTERVAL[lim][side == "above"] and (f.q < 0) == (sign == "-"), (f.name, f.q)
                seen.add(W.interval(f.q))
        elif f.name == "fll:prev=0":
            assert (f.cross, f.dot) == (0, 0) and int(st0["n_updates"][names.index(f.name)]) > 0
        elif kind[0] == "wrap":
            down = kind[1] == "down"
            assert (f.phase0 < 1 and f.phase1 > 16360) if down else (f.phase0 > 16367 and f.phase1 < 8), (f.name, f.phase0, f.phase1)
    assert seen == {"poly", "hi0", "hi1", "hi2", "hi3"}
    j = names.index("fll:n_updates=0xFFFFFFFF")
    assert int(st0["n_updates"][j]) == 0xFFFFFFFF and int(want_st["n_updates"][j]) == 1
    assert {"fll:dot=0", "fll:half_turn", "fll:prev=0", "wrap:down", "wrap:up"} <= set(names)
