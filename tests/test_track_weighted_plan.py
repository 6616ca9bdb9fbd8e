"""csrc/gpsx_track_weighted_plan.hpp -- the launch shape of k_track_epl_weighted: channels per wave (cpw) and workgroups from
(n_ch, n_blocks) -- compiled for the HOST with g++ and checked on every launch tests/test_gpu_weighted_track_shapes.py makes
(tests/weighted_track_shapes.py): cpw, the workgroup count, whether the last active wave is ragged, how many waves of the last
workgroup are idle, whether cpw was set by the ceil(n_ch / 4) bound -- so that the GPU tests cover the shapes they claim to."""
import weighted_track_shapes as S


def _check(rows):
    got = S.plans([(r[0], r[1]) for r in rows])
    bad = []
    for (n_ch, n_blocks, cpw, groups, last, idle, bound), (g_cpw, g_groups, g_bound) in zip(rows, got):
        first, g_last, g_idle = S.geometry(n_ch, g_cpw, g_groups)
        if (g_cpw, g_groups, g_last, g_idle, g_bound) != (cpw, groups, last, idle, bound):
            bad.append(f"({n_ch}, {n_blocks}): plan {(g_cpw, g_groups, g_last, g_idle, g_bound)}, table {(cpw, groups, last, idle, bound)}")
        assert first + g_last == n_ch and 1 <= g_cpw <= 16 and 4 * g_cpw * g_groups >= n_ch > 4 * g_cpw * (g_groups - 1)
    assert not bad, "\n".join(bad)


def test_every_channels_per_wave_table():
    _check(S.SHAPES)
    assert {r[2] for r in S.SHAPES} | {1} == set(range(1, 17))
    assert {S.ROWS[k][0] for k in S.ROWS} == set(range(1, 17))           # cpw = 1 is reached by the other launches
    ragged = [r for r in S.SHAPES if r[4] < r[2]]
    assert len(ragged) == len(S.SHAPES) - 1 and S.SHAPES[-1][:2] == (212992, 1)   # every entry but the benchmark's shape
    assert {r[2] for r in ragged} == set(range(2, 17))                  # a ragged last wave at every cpw above 1
    assert sum(1 for r in ragged if r[5] > 0) >= 8 and {r[5] for r in ragged} == {0, 1, 2}
    assert (70003, 1, 16) == S.SHAPES[-2][:3] and S.SHAPES[-2][4] == 3   # cpw 16 with a last wave of 3
    assert not any(r[6] for r in S.SHAPES)


def test_few_channels_many_blocks_table():
    _check(S.FEW)
    assert [(r[0], r[1], r[2]) for r in S.FEW] == [(61, 4096, 16), (37, 4096, 10), (5, 4096, 2), (2, 4096, 1), (23, 900, 5), (45, 700, 7)]
    for n_ch, n_blocks, cpw, _, _, _, bound in S.FEW:
        spread = (n_ch + 3) // 4
        assert bound == (n_ch * n_blocks // 4096 > spread) and (cpw == spread if bound else cpw < spread)
    assert sum(r[6] for r in S.FEW) == 4
    # the eight-piece calls they are compared with run at another cpw wherever there is one to run at (2 channels: cpw is 1)
    for n_ch, n_blocks, cpw, *_ in S.FEW:
        piece = -(-n_blocks // 8)
        assert (S.ROWS[(n_ch, piece)][0] != cpw) == (n_ch != 2)


def test_other_launches_table():
    _check(S.OTHER)
    assert len(S.ROWS) == len(S.SHAPES) + len(S.FEW) + len(S.OTHER)      # no pair twice
    # the K-split identities change cpw: one-block calls and ceil(K / 4)-block pieces against the K-block call
    for n_ch, n_blocks, cpw, *_ in S.SHAPES:
        if n_blocks > 1:
            assert S.ROWS[(n_ch, 1)][0] == 1 != cpw and S.ROWS[(n_ch, -(-n_blocks // 4))][0] != cpw
    assert S.ROWS[(8219, 1)][0] == 2 and S.ROWS[(4099, 20)][0] == 16 and S.ROWS[(4099, 4)][0] == 4 and S.ROWS[(1367, 12)][0] == 4
