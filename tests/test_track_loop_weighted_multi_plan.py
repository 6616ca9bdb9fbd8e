"""csrc/gpsx_track_loop_weighted_plan.hpp plan_track_loop_weighted_multi -- the launch shape of k_track_wsync_multi: one workgroup
of four waves per receiver, cpw = ceil(ch_per_rx / 4) slots per wave -- compiled for the HOST with g++ and checked for every
ch_per_rx and on every launch tests/test_gpu_weighted_multi.py makes (tests/weighted_multi_cases.py SHAPES), so that the GPU tests
cover the wave geometries they claim to."""
import weighted_multi_cases as M


def test_every_slot_count():
    shapes = [(n_rx, ch) for ch in range(1, 65) for n_rx in (1, 7, 1 << 20)]
    for (n_rx, ch), (cpw, groups) in zip(shapes, M.plans(shapes)):
        assert cpw == -(-ch // 4) and 4 * cpw >= ch and 1 <= cpw <= 16 and groups == n_rx, (n_rx, ch, cpw, groups)
        w = M.waves(ch, cpw)
        assert sum(w) == ch and w[0] >= 1 and all(a >= b for a, b in zip(w, w[1:]))      # every slot in one wave, the first never idle


def test_what_the_plan_refuses():
    for shape, got in zip([(1, 0), (1, 65), (0, 4), (-1, 4), (1, -3)], M.plans([(1, 0), (1, 65), (0, 4), (-1, 4), (1, -3)])):
        assert got == (0, 0), shape


def test_every_shape_the_gpu_tests_run():
    got = M.plans([s[:2] for s in M.SHAPES])
    for (n_rx, ch, cpw, waves), (g_cpw, g_groups) in zip(M.SHAPES, got):
        assert (g_cpw, g_groups) == (cpw, n_rx) and M.waves(ch, g_cpw) == waves, (n_rx, ch)
    by = {s[:2]: s for s in M.SHAPES}
    assert by[(3, 5)][3].count(0) == 1 and by[(9, 1)][3].count(0) == 3            # an idle wave; three idle waves
    assert by[(2, 17)][3] == (5, 5, 5, 2) and by[(2, 64)][3] == (16,) * 4        # a ragged last wave; full waves
    assert by[(5, 4)][3] == (1,) * 4                                             # the four-channel receiver
    assert M.N_BLOCKS % 20 and M.N_BLOCKS % 5 and M.N_BLOCKS % 4 and sum(M.PIECES) == M.N_BLOCKS
