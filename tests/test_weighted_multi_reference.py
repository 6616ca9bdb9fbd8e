"""The sync loop for many receivers per launch, without a GPU (include/gpsx.h gpsx_track_loop_weighted_sync_multi,
gpsx_wobs_pseudoranges_rx): the interface as a C compiler, nm and capi.py see it; the new kernel's resources; the grounds the case
table of tests/weighted_multi_cases.py stands on, asserted on the restatement so that a case cannot stop covering one unnoticed;
gpsx_wobs_pseudoranges_rx against per-slice calls of gpsx_wobs_pseudoranges, bitwise; and the two-receiver chain scenario on the
restatements, which shows that weighted_lock_cases' thresholds separate a PRN that is only on the other receiver's stream from the
satellites that are present.  The arithmetic is weighted_sync_ref's with weighted_aided_ref's clause: nothing is restated here."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import weighted_lock_cases as X
import weighted_lock_ref as R
import weighted_multi_cases as M
import weighted_obs_ref as O
import weighted_sync_cases as K
import weighted_sync_ref as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"gpsx_track_loop_weighted_sync_multi", "gpsx_track_loop_weighted_sync_multi_dev", "gpsx_wobs_pseudoranges_rx"}

LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "gpsx.h"
typedef int (*multi_dev)(gpsx_ctx *, const gpsx_wsync_cfg_t *, const gpsx_waid_t *, const gpsx_wmulti_t *, const void *, int, gpsx_wsync_state_t *,
                         gpsx_wsync_rec_t *);
typedef int (*multi_host)(gpsx_ctx *, const gpsx_wsync_cfg_t *, const gpsx_waid_t *, const gpsx_wmulti_t *, const uint8_t *, int, gpsx_wsync_state_t *,
                          gpsx_wsync_rec_t *);
typedef int (*pr_rx)(const gpsx_wobs_t *, int, int, double, double *, double *, int *);
_Static_assert(__builtin_types_compatible_p(__typeof__(&gpsx_track_loop_weighted_sync_multi_dev), multi_dev), "the _dev entry point");
_Static_assert(__builtin_types_compatible_p(__typeof__(&gpsx_track_loop_weighted_sync_multi), multi_host), "the host entry point");
_Static_assert(__builtin_types_compatible_p(__typeof__(&gpsx_wobs_pseudoranges_rx), pr_rx), "the per-receiver pseudorange step");
int main(void)
{
  printf("sizeof %zu\nn_rx %zu\nch_per_rx %zu\nrx_stride_blocks %zu\nreserved %zu\nversion %d\nnone %d\n", sizeof(gpsx_wmulti_t),
         offsetof(gpsx_wmulti_t, n_rx), offsetof(gpsx_wmulti_t, ch_per_rx), offsetof(gpsx_wmulti_t, rx_stride_blocks),
         offsetof(gpsx_wmulti_t, reserved), GPSX_VERSION, GPSX_PRN_NONE);
  return 0;
}
"""


# ---- the interface ---------------------------------------------------------------------------------------------------------------------
def test_the_struct_and_the_entry_points_as_a_c_compiler_sees_them():
    with tempfile.TemporaryDirectory(prefix="wmulti_layout_") as tmp:
        src, exe = os.path.join(tmp, "layout.c"), os.path.join(tmp, "layout")
        with open(src, "w") as f:
            f.write(LAYOUT_C)
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
        got = {k: int(v) for k, v in (line.split() for line in subprocess.check_output([exe], text=True).splitlines())}
    assert got == dict(sizeof=16, n_rx=0, ch_per_rx=4, rx_stride_blocks=8, reserved=12, version=110, none=-2147483648)
    from stm32f4_sdr_gps_amd import capi
    assert capi.WMULTI_DTYPE.itemsize == 16 and [capi.WMULTI_DTYPE.fields[f][1] for f in ("n_rx", "ch_per_rx", "rx_stride_blocks", "reserved")] == [0, 4, 8, 12]
    assert capi.wmulti(3, 5, 64).tobytes() == np.array([3, 5, 64, 0], "<i4").tobytes() and capi.PRN_NONE == M.PRN_NONE == got["none"]


def test_library_exports_the_entry_points(lib_path):
    syms = subprocess.check_output(["nm", "-D", "--defined-only", lib_path], text=True)
    names = {line.split()[-1] for line in syms.splitlines() if line.strip()}
    assert SYMBOLS <= names
    from stm32f4_sdr_gps_amd import capi
    import __graft_entry__ as entry
    assert SYMBOLS <= set(entry.ABI_SYMBOLS)
    assert callable(getattr(capi.Engine, "track_loop_weighted_sync_multi", None)) and callable(capi.wobs_pseudoranges_rx)
    lib = capi.load_library()
    assert len(lib.gpsx_track_loop_weighted_sync_multi.argtypes) == len(lib.gpsx_track_loop_weighted_sync_multi_dev.argtypes) == 8
    assert len(lib.gpsx_wobs_pseudoranges_rx.argtypes) == 7 and lib.gpsx_version() == 110


def test_the_kernels_resources(lib_path):
    from stm32f4_sdr_gps_amd import build
    res = build.check_no_scratch()          # (runs check_wmulti too)
    hits = list(build.check_wmulti().values())
    assert len(hits) == 1 and hits[0]["scratch_bytes"] == 0 and hits[0]["vgprs"] <= 128, hits
    assert 8192 <= hits[0]["lds_bytes"] <= 8192 + 64          # one receiver's two plane buffers
    for name in ("k_track_wloop", "k_track_wsync", "k_track_waid_loop", "k_track_waid_sync"):      # the single-stream kernels: still one of each
        assert len([k for k in res if name in k]) == 1, name


# ---- the case table ------------------------------------------------------------------------------------------------------------------------
def test_the_case_table_stands_on_every_ground(oracle):
    seen = M.grounds(oracle)
    print({k: len(v) for k, v in seen.items()})
    for ground, hits in seen.items():
        assert hits, ground
    cases = {h[0] for h in seen["accept"]}
    assert {k for _, k in cases} == set(M.AIDS)                                     # an accept with and without aiding
    assert {n for _, _, n in seen["bad"]} == set(M.BAD)
    # hand-overs in all three modes on every shape with more than one slot; the one-slot shape takes them receiver by receiver
    for i, (n_rx, ch, _, _) in enumerate(M.SHAPES):
        assert {int(m) for m in M.shape_inputs(i)[1]["mode"]} == {Y.SEARCH, Y.WAIT, Y.LOCKED}, (n_rx, ch)
    # every receiver has satellites and a stream of its own
    blocks = M.shape_inputs(0)[0]
    assert len({b.tobytes() for b in blocks}) == len(blocks) and len({tuple(s[0] for s in M.rx_sats(r)) for r in range(9)}) == 9


def test_aiding_changes_the_bytes_and_a_zero_factor_does_not(oracle):
    """the two factors of the table differ in their bytes on every shape (so the GPU comparison tells them apart), and the factor 0
    is weighted_sync_ref's own run: receiver 1 of shape 0 through it directly"""
    ref = M.shapes_on_restatement()
    for i in range(len(M.SHAPES)):
        assert ref[(i, M.AIDS[0])][1].tobytes() != ref[(i, M.AIDS[1])][1].tobytes(), i
    blocks, st0, cfg = M.shape_inputs(0)
    ch = M.SHAPES[0][1]
    st = st0[ch:2 * ch].copy()
    rec = Y.run(oracle, blocks[1], st, cfg)
    want_rec, want_st, _ = ref[(0, 0.0)]
    assert rec.tobytes() == np.ascontiguousarray(want_rec[:, ch:2 * ch]).tobytes() and st.tobytes() == want_st[ch:2 * ch].tobytes()


def test_the_holes_leave_their_neighbours_alone(oracle):
    for k in M.AIDS:
        base_rec, base_st, _ = M.shapes_on_restatement()[(0, k)]
        st0, rec, st = M.patched(oracle, 0, k, M.HOLES)
        for ch in range(len(st)):
            same = rec[:, ch].tobytes() == base_rec[:, ch].tobytes() and st[ch:ch + 1].tobytes() == base_st[ch:ch + 1].tobytes()
            assert same == (ch not in M.HOLES), ch
        for ch in M.HOLES:                 # only if_freq_accum moved
            for f in Y.STATE_DTYPE.names:
                if f != "loop":
                    assert st[f][ch:ch + 1].tobytes() == st0[f][ch:ch + 1].tobytes(), (ch, f)
            for f in st["loop"].dtype.names:
                assert (st["loop"][f][ch:ch + 1].tobytes() == st0["loop"][f][ch:ch + 1].tobytes()) == (f != "if_freq_accum"), (ch, f)
    assert sorted(ch % 5 for ch in M.HOLES) == [0, 2, 4] and sorted(ch // 5 for ch in M.HOLES) == [0, 1, 2]     # front, middle, end


# ---- gpsx_wobs_pseudoranges_rx ---------------------------------------------------------------------------------------------------------------
def _obs(rows):
    obs = np.zeros(len(rows), O.OBS_DTYPE)
    for k, (tx_ms, phase, flags) in enumerate(rows):
        obs[k] = (tx_ms, phase, 0.0, flags, 0, 0, 0)
    return obs


def test_pseudoranges_per_receiver_are_the_per_slice_calls(lib_path):
    from stm32f4_sdr_gps_amd import capi
    v = O.F_VALID | 7
    rows = [(1000, 5000.0, v), (1003, 16000.0, v), (1003, 200.5, v), (2000, 0.0, 7),               # receiver 0: the reference is slot 2
            (604799990, 100.0, v), (15, 300.0, v), (5, 100.0, v), (9, 1.0, 0),                     # receiver 1: across the week's end, slot 1
            (7, 1.0, 7), (9, 1.0, 0), (11, 3.0, 7 | O.F_AMBIGUOUS), (0, 0.0, 0),                   # receiver 2: no VALID observable
            (500, 9000.0, v), (400, 1.0, v | O.F_AMBIGUOUS), (2, 2.0, 7), (499, 16367.0, v)]       # receiver 3: slot 0
    obs = _obs(rows)
    rng = np.random.default_rng(5)
    more = _obs([(int(rng.integers(0, 604800000)), float(rng.uniform(0, 16368)), v if rng.integers(0, 3) else 7) for _ in range(40 * 6)])
    for o, n_rx, ch in ((obs, 4, 4), (obs, 1, 16), (obs, 16, 1), (obs, 2, 8), (more, 40, 6), (more, 6, 40)):
        for offset in (68.802, 0.0, -3.5):
            pr, rx, n_valid = capi.wobs_pseudoranges_rx(o, n_rx, ch, offset)
            refs = []
            for r in range(n_rx):
                want_pr, want_rx, want_n = capi.wobs_pseudoranges(o[r * ch:(r + 1) * ch], offset)
                assert pr[r * ch:(r + 1) * ch].tobytes() == want_pr.tobytes() and np.float64(rx[r]).tobytes() == np.float64(want_rx).tobytes()
                assert int(n_valid[r]) == want_n
                refs.append(int(np.argmin(np.where(want_pr > 0, want_pr, np.inf))) if want_n else -1)
            if o is obs and (n_rx, ch) == (4, 4) and offset == 68.802:      # (the reference channel has the smallest pseudorange)
                assert refs == [2, 1, -1, 0] and n_valid.tolist() == [3, 3, 0, 3] and rx[2] == 0.0 and not pr[8:12].any(), (refs, n_valid)
    # refusals: nothing written
    lib = capi.load_library()
    pr1, rx1, nv1 = np.full(16, 5.0), np.full(4, 5.0), np.full(4, 5, np.int32)
    good = [obs.ctypes.data, 4, 4, 1.0, pr1.ctypes.data, rx1.ctypes.data, nv1.ctypes.data]
    assert lib.gpsx_wobs_pseudoranges_rx(*good) == 9
    pr1[:], rx1[:], nv1[:] = 5.0, 5.0, 5
    for at, bad in ((0, None), (4, None), (5, None), (6, None), (1, 0), (1, -1), (2, 0), (2, -4), (3, float("nan")), (3, float("inf")), (1, 1 << 30)):
        args = list(good)
        args[at] = bad
        if bad == 1 << 30:
            args[2] = 4                                                              # n_rx * ch_per_rx = 2^32
        assert lib.gpsx_wobs_pseudoranges_rx(*args) == -22 and (pr1 == 5.0).all() and (rx1 == 5.0).all() and (nv1 == 5).all(), (at, bad)
    with pytest.raises(capi.GpsxError):
        capi.wobs_pseudoranges_rx(obs, 3, 4)


# ---- the chain on the restatements -----------------------------------------------------------------------------------------------------------
def test_the_chain_scenario_separates_the_cross_stream_prn():
    """two receivers, three satellites each, a slot with the other receiver's PRN and an empty one: on the restatements every present
    satellite is LOCKED and decodes its bits, the cross-stream PRN never gets CODE, and weighted_lock_cases.CODE_MIN lies between"""
    recs, st, locks, _ = M.chain_on_restatement()
    got = M.chain_measure()
    print("chain, code ratios:", got)
    assert got == M.MEASURED, got
    assert got["code_cross_max"] < X.CODE_MIN < got["code_present_min"]
    both = R.F_CODE | R.F_CARRIER
    flags = np.array([l["flags"] for l in locks])
    for ch in M.chain_slots("sat"):
        r, j = divmod(ch, M.CHAIN_CH)
        sat = M.CHAIN_SLOTS[r][j][1]
        assert int(st["mode"][ch]) == Y.LOCKED and (flags[-1, ch] & both) == both, ch
        bits = Y.bits_after_lock([(at, rec[:, ch]) for at, rec in zip(range(0, M.CHAIN_MS, M.CHAIN_LAUNCH), recs)])
        edge = int(st["edge"][ch])
        assert edge - M.CHAIN_SATS[r][sat][3] in (0, 1), (ch, edge)
        errors, n = K.bit_errors(bits, M.chain_blocks(r)[1][sat], edge)
        assert errors == 0 and n >= 40, (ch, errors, n)
    for ch in M.chain_slots("cross"):
        assert not (flags[:, ch] & R.F_CODE).any(), (ch, flags[:, ch])
    empty = Y.empty_records(recs[0].shape[0], 1)[:, 0]
    for ch in M.chain_slots("none"):
        assert all(rec[:, ch].tobytes() == empty.tobytes() for rec in recs) and not flags[:, ch].any()
