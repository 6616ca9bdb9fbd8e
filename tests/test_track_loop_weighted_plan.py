"""csrc/gpsx_track_loop_weighted_plan.hpp -- the launch shape of k_track_wloop: channels per wave (cpw) and workgroups from n_ch
alone (the blocks run inside the kernel) -- compiled for the HOST with g++ and checked on every launch
tests/test_gpu_weighted_loop.py makes (tests/weighted_loop_cases.py): cpw, the workgroup count, the channels of the last active
wave and the idle waves of the last workgroup -- so that the GPU tests cover the shapes they claim to."""
import weighted_loop_cases as S


def test_every_shape_of_the_table():
    got = S.plans([r[0] for r in S.SHAPES])
    bad = []
    for (n_ch, cpw, groups, last, idle), (g_cpw, g_groups) in zip(S.SHAPES, got):
        g_last, g_idle = S.geometry(n_ch, g_cpw, g_groups)
        if (g_cpw, g_groups, g_last, g_idle) != (cpw, groups, last, idle):
            bad.append(f"{n_ch}: plan {(g_cpw, g_groups, g_last, g_idle)}, table {(cpw, groups, last, idle)}")
        assert 1 <= g_cpw <= 16 and 4 * g_cpw * g_groups >= n_ch > 4 * g_cpw * (g_groups - 1)
    assert not bad, "\n".join(bad)


def test_the_table_covers_what_it_claims():
    assert {r[1] for r in S.SHAPES} == set(range(1, 17))                    # every cpw the plan can choose
    assert {r[4] for r in S.SHAPES} == {0, 1, 2, 3}                         # workgroups with no, one, two and three idle waves
    ragged = [r for r in S.SHAPES if r[3] < r[1]]
    full = [r for r in S.SHAPES if r[3] == r[1] and r[1] > 1]
    assert len(ragged) >= 10 and len(full) >= 3                             # waves filled partly and fully
    assert (65536, 16, 1024, 16, 0) in S.SHAPES                             # the benchmark's shape: nothing ragged, nothing idle
    assert len(S.ROWS) == len(S.SHAPES)                                     # no channel count twice


def test_the_plan_depends_on_the_channel_count_as_the_sign_plane_loops_does():
    """cpw = n_ch / 4096 clamped to 1 .. 16: ~4 workgroups of four waves per compute unit, launch_track_loop's rule"""
    counts = [1, 4095, 4096, 8191, 8192, 65535, 65536, 212992, 1 << 22]
    for n_ch, (cpw, groups) in zip(counts, S.plans(counts)):
        assert cpw == max(1, min(16, n_ch // 4096)) and groups == -(-n_ch // (4 * cpw))
