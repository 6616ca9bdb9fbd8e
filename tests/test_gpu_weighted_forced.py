"""Every branch of the weighted loops' window update and of the bit synchroniser's decision, forced on the device (include/gpsx.h
gpsx_track_loop_weighted_sync; k_track_wsync): the table of tests/weighted_forced_cases.py -- states whose open window makes the
launch's first block end a window with chosen sums, asserted branch by branch on the restatement in
tests/test_weighted_forced_reference.py -- through gpsx_track_loop_weighted_sync_dev against the exact CPU restatement
(tests/weighted_sync_ref.py).  Every comparison is for equality, byte for byte, on the records and on the full 448-byte states, with
canaries around both: the table at one channel per wave; at 2, 7 and 16 channels per wave with the rows moving through the lanes;
the host variant; and the same targets reached over two launches, the open window passing through HBM between them.  Every launch
runs one or two blocks; the restatement runs the distinct rows only."""
import numpy as np
import pytest

import weighted_forced_cases as W
import weighted_gpu as G
import weighted_loop_cases as S
import weighted_sync_ref as Y
from weighted_gpu import EINVAL, eng  # noqa: F401

pytestmark = pytest.mark.gpu


def _launches(eng, pieces, st, cfg, has_bad, host=False):
    """the library on a copy of `st` in device memory, one launch per entry of `pieces` (arrays of blocks) -> ([records per launch],
    [states after each launch]).  has_bad: GPSX_EINVAL is due (from the next synchronize after the device variant, from the host
    variant itself)"""
    n_ch, c = len(st), G.sync_cfg(cfg)
    fn = eng.lib.gpsx_track_loop_weighted_sync if host else eng.lib.gpsx_track_loop_weighted_sync_dev
    parts = [np.ascontiguousarray(part, np.uint8).reshape(-1, 4092) for part in pieces]

    def call(ins, sts, out, k):
        return fn(eng.h, c.ctypes.data, ins[0], len(parts[k]), sts[0], n_ch, out)
    recs, states, codes = G.run_stage(eng, call, b"k_track_wsync", st, [([part], Y.REC_DTYPE, (Y.slots(len(part), cfg), n_ch)) for part in parts],
                                      not host, host_inputs=True, after_each=True)
    assert codes == [EINVAL if has_bad else 0] * len(parts), (codes, eng.lib.gpsx_last_error(eng.h))
    assert eng.lib.gpsx_synchronize(eng.h) == 0
    return recs, states


def _same(rec, after, want_rec, want_st, channels, names, what):
    assert rec.dtype == Y.REC_DTYPE, what
    G.same_columns(rec, want_rec, (what, "record"), list(channels), names)
    G.same_rows(after, want_st, (what, "state"), list(channels), names)


def _group(oracle, group, n_ch, cpw):
    """(blocks, states [n_ch], cfg, records wanted, states wanted, row name per channel, a bad channel among them)"""
    rows, st0, cfg, rec, after, _ = W.restated(oracle, group)
    idx = W.tiled(n_ch, len(rows), cpw)
    names = [rows[i].name for i in idx]
    return (W.blocks(W.GROUPS[group][1]), st0[idx].copy(), cfg, np.ascontiguousarray(rec[:, idx]), after[idx].copy(), names,
            any("bad" in rows[i].tags for i in set(idx.tolist())))


@pytest.mark.parametrize("group", sorted(W.GROUPS))
def test_the_table_at_one_channel_per_wave(eng, oracle, group):
    """(a) 257 channels, the rows tiled: every channel's records and full state are the restatement's"""
    n_ch = 257
    assert S.tabled(n_ch) == 1
    blocks, st, cfg, want, want_st, names, has_bad = _group(oracle, group, n_ch, 1)
    recs, states = _launches(eng, [blocks], st, cfg, has_bad)
    _same(recs[0], states[0], want, want_st, range(n_ch), names, group)
    assert recs[0].tobytes() == want.tobytes() and states[0].tobytes() == want_st.tobytes()


@pytest.mark.parametrize("n_ch", [8195, 28700, 70003])
def test_the_table_at_several_channels_per_wave(eng, oracle, n_ch):
    """(b) cpw 2, 7 and 16: the table tiled with a period coprime to the cpw, so that every row passes through every lane and --
    in group A, which has more rows than a wave has channels -- the channels of a wave sit on different rows (groups B and C have
    3 and 6 rows: their waves repeat rows at cpw 7 and 16); a sample (the first, the last, the wave boundaries, the ragged last
    wave, 15 random channels) against the restatement, and equal states give equal results wherever they sit"""
    cpw = S.tabled(n_ch)
    assert cpw == {8195: 2, 28700: 7, 70003: 16}[n_ch]
    last = S.ROWS[n_ch][2]
    rng = np.random.default_rng(n_ch)
    sample = sorted({0, 1, cpw - 1, cpw, 4 * cpw - 1, 4 * cpw, n_ch - 1, n_ch - last, n_ch - last - 1} | {int(x) for x in rng.integers(0, n_ch, 15)})
    for group in sorted(W.GROUPS):
        blocks, st, cfg, want, want_st, names, has_bad = _group(oracle, group, n_ch, cpw)
        recs, states = _launches(eng, [blocks], st, cfg, has_bad)
        _same(recs[0], states[0], want, want_st, sample, names, (group, n_ch))
        idx = W.tiled(n_ch, len(W.table(group)), cpw)      # channel idx[c] < n_rows holds the same state as channel c
        assert recs[0].tobytes() == np.ascontiguousarray(recs[0][:, idx]).tobytes() and states[0].tobytes() == states[0][idx].tobytes(), (group, n_ch)
        assert recs[0].tobytes() == want.tobytes() and states[0].tobytes() == want_st.tobytes(), (group, n_ch)


@pytest.mark.parametrize("group", sorted(W.GROUPS))
def test_the_host_variant(eng, oracle, group):
    """(c) 257 channels through gpsx_track_loop_weighted_sync: the device variant's records and states"""
    blocks, st, cfg, want, want_st, names, has_bad = _group(oracle, group, 257, 1)
    dev = _launches(eng, [blocks], st, cfg, has_bad)
    host = _launches(eng, [blocks], st, cfg, has_bad, host=True)
    assert host[0][0].tobytes() == dev[0][0].tobytes() and host[1][0].tobytes() == dev[1][0].tobytes()
    _same(host[0][0], host[1][0], want, want_st, range(257), names, (group, "host"))


def test_the_table_cut_one_block_earlier(eng, oracle):
    """(d) the rows of group A whose window has a block in it, preloaded with win_n one less and win_iq = target - r_0 - r_1, over
    two launches of one block: the first ends no window and leaves the open window in HBM, the second ends the target's; records
    and states of both launches are the restatement's of the same two launches"""
    n_ch = 257
    cut = W.cut_rows("A")
    rows, cfg = W.table("A"), W.cfg_of("A")
    distinct = np.concatenate([W.state_of(oracle, rows[i], i, cfg, lead=2)[0] for i in cut])
    idx = np.arange(n_ch) % len(cut)
    names = [rows[cut[i]].name for i in idx]
    st = distinct[idx].copy()
    pieces = [W.blocks()[0:1], W.blocks()[1:2]]
    want_st = distinct.copy()
    want = []
    for part in pieces:
        want.append(np.ascontiguousarray(Y.run(oracle, part, want_st, cfg)[:, idx]))
        want.append(want_st[idx].copy())
    recs, states = _launches(eng, pieces, st, cfg, False)
    _same(recs[0], states[0], want[0], want[1], range(n_ch), names, "first launch")
    _same(recs[1], states[1], want[2], want[3], range(n_ch), names, "second launch")
    assert not recs[0]["flags"].any() and (states[0]["win_n"] == st["win_n"] + 1).all() and states[0]["win_iq"].any(axis=1).all()
    assert (recs[1]["flags"][0] & Y.F_WINDOW).all() and not states[1]["win_iq"].any()
    for c in range(len(cut)):
        assert tuple(int(v) for v in recs[1][0, c]["w"]["iq"]) == rows[cut[c]].target, names[c]
