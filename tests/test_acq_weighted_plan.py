"""csrc/gpsx_acq_plan.hpp's weighted planners -- plan_acq_weighted, plan_acq_coherent, plan_acq_hybrid and the chunk rule they share,
plan_wms_chunks -- compiled for the HOST with g++ (tests/weighted_grid_cases.py's driver) and checked on a table at 256 CUs (the
MI355X), tests/test_acq_plan.py's method: per call the form, the path, GPSX_ENOMEM, the units, the units per launch, the launches,
the grid, the scratch of one launch and the gpsx_last_kernel name.  The rows follow from the header's rules, not from its output:
a cluster of the two scratch walks keeps 2 MB, the default cap is 2048 MB; a launch takes cap / 2 MB clusters, whole rounds of the
chip when that is at least one round, never more than the call has, and every refusal halves what is left after that; the vector
forms take a workgroup per (search, Doppler, 8 PRNs) in one launch without scratch; the matrix forms count 32 PRNs per cluster."""
import weighted_grid_cases as G

MB = 1 << 20
CL = 2 * MB                       # kMxwMsClusterBytes
W, C, H = "w", "c", "h"           # gpsx_acq_grid_weighted_ms (n_ms = 1: gpsx_acq_grid_weighted), _coh, _hyb


def walk(form, name, units, chunk):
    """a scratch walk at `chunk` clusters a launch"""
    return dict(form=form, mx=1, enomem=0, units=units, chunk=chunk, n_chunks=-(-units // chunk), grid=chunk, scratch_bytes=chunk * CL, name=name)


def refused(form, name, units):
    return dict(form=form, mx=1, enomem=1, units=units, chunk=0, n_chunks=0, grid=0, scratch_bytes=0, name=name)


def once(form, name, units, mx):
    """one launch, no scratch"""
    return dict(form=form, mx=mx, enomem=0, units=units, chunk=units, n_chunks=1, grid=units, scratch_bytes=0, name=name)


MS, HY = ("kMxwWalk", "k_acq_wmx_ms"), ("kHybMx", "k_acq_hyb_mx")
# 32 PRNs x 21 Doppler bins: 21 clusters and 84 vector workgroups per search
# (what, (call, n_search, n_ms | n_coh, n_seg, n_prn, n_dopp, vector, cap in MB or 0, refused), the plan)
ROWS = [
    # clusters and launches at the default and at capped scratch sizes
    ("hyb 256 x 10 x 8, default cap: 2048 MB / 2 MB = 1024, four rounds", (H, 256, 10, 8, 32, 21, 0, 0, 0), walk(*HY, 5376, 1024)),
    ("hyb 256 x 10 x 8 at 1024 MB: 512 a launch", (H, 256, 10, 8, 32, 21, 0, 1024, 0), walk(*HY, 5376, 512)),
    ("ms 64 x 10 at 1024 MB", (W, 64, 10, 0, 32, 21, 0, 1024, 0), walk(*MS, 1344, 512)),
    ("ms 256 x 10, default cap", (W, 256, 10, 0, 32, 21, 0, 0, 0), walk(*MS, 5376, 1024)),
    # whole rounds from one round up, the bare quotient below
    ("ms at 700 MB: 350 -> 256", (W, 64, 10, 0, 32, 21, 0, 700, 0), walk(*MS, 1344, 256)),
    ("hyb at 700 MB: 350 -> 256", (H, 64, 2, 3, 32, 21, 0, 700, 0), walk(*HY, 1344, 256)),
    ("ms at 100 MB: 50, below a round", (W, 64, 10, 0, 32, 21, 0, 100, 0), walk(*MS, 1344, 50)),
    ("ms at 512 MB: exactly one round", (W, 64, 10, 0, 32, 21, 0, 512, 0), walk(*MS, 1344, 256)),
    ("ms at 510 MB: 255, one short of a round", (W, 64, 10, 0, 32, 21, 0, 510, 0), walk(*MS, 1344, 255)),
    ("ms at 2 MB: one cluster a launch", (W, 2, 3, 0, 40, 3, 0, 2, 0), walk(*MS, 12, 1)),
    # never more than the call has -- and the call's count is not rounded
    ("ms 1 x 10: 21 clusters", (W, 1, 10, 0, 32, 21, 0, 0, 0), walk(*MS, 21, 21)),
    ("ms 16 x 10: 336 clusters, more than a round, fewer than the cap", (W, 16, 10, 0, 32, 21, 0, 0, 0), walk(*MS, 336, 336)),
    ("hyb 16 x 2 x 2: 336 clusters", (H, 16, 2, 2, 32, 21, 0, 0, 0), walk(*HY, 336, 336)),
    ("ms 16 x 10 at 700 MB: 256 + 80", (W, 16, 10, 0, 32, 21, 0, 700, 0), walk(*MS, 336, 256)),
    ("ms, 33 PRNs: two clusters per (search, Doppler)", (W, 3, 2, 0, 33, 5, 0, 0, 0), walk(*MS, 30, 30)),
    ("hyb, 255 PRNs: eight", (H, 2, 2, 2, 255, 3, 0, 0, 0), walk(*HY, 48, 48)),
    # every refusal halves, after the rounding and after the call's count
    ("ms 256 x 10, refused once: 1024 -> 512", (W, 256, 10, 0, 32, 21, 0, 0, 1), walk(*MS, 5376, 512)),
    ("ms 256 x 10, refused three times: 1024 -> 128", (W, 256, 10, 0, 32, 21, 0, 0, 3), walk(*MS, 5376, 128)),
    ("hyb 256 x 10 x 8, refused once", (H, 256, 10, 8, 32, 21, 0, 0, 1), walk(*HY, 5376, 512)),
    ("hyb 256 x 10 x 8, refused three times", (H, 256, 10, 8, 32, 21, 0, 0, 3), walk(*HY, 5376, 128)),
    ("ms at 700 MB, refused once: 350 -> 256 -> 128", (W, 64, 10, 0, 32, 21, 0, 700, 1), walk(*MS, 1344, 128)),
    ("ms 1 x 10, refused once: 21 -> 10", (W, 1, 10, 0, 32, 21, 0, 0, 1), walk(*MS, 21, 10)),
    ("ms 256 x 10, refused ten times: one cluster", (W, 256, 10, 0, 32, 21, 0, 0, 10), walk(*MS, 5376, 1)),
    # GPSX_ENOMEM: the shift leaves nothing, the refusals run out, the cap holds no cluster
    ("ms 256 x 10, refused eleven times", (W, 256, 10, 0, 32, 21, 0, 0, 11), refused(*MS, 5376)),
    ("ms 1 x 10, refused five times: 21 >> 5", (W, 1, 10, 0, 32, 21, 0, 0, 5), refused(*MS, 21)),
    ("ms, refused 62 times", (W, 256, 10, 0, 32, 21, 0, 0, 62), refused(*MS, 5376)),
    ("ms, refused 63 times", (W, 256, 10, 0, 32, 21, 0, 0, 63), refused(*MS, 5376)),
    ("ms, refused 64 times (no shift by the word size)", (W, 256, 10, 0, 32, 21, 0, 0, 64), refused(*MS, 5376)),
    ("hyb, refused 62 times", (H, 256, 10, 8, 32, 21, 0, 0, 62), refused(*HY, 5376)),
    ("ms at 1 MB", (W, 2, 3, 0, 40, 3, 0, 1, 0), refused(*MS, 12)),
    ("hyb at 1 MB", (H, 2, 2, 3, 40, 3, 0, 1, 0), refused(*HY, 12)),
    # one block: a launch of clusters, no scratch, whatever the cap
    ("one block", (W, 256, 1, 0, 32, 21, 0, 0, 0), once("kMxw", "k_acq_mxw", 5376, 1)),
    ("one block, 33 PRNs, at 1 MB and refused", (W, 2, 1, 0, 33, 3, 0, 1, 5), once("kMxw", "k_acq_mxw", 12, 1)),
    ("coherent", (C, 256, 20, 0, 32, 21, 0, 0, 0), once("kCohMx", "k_acq_coh_mx", 5376, 1)),
    ("coherent, 65 PRNs: three clusters", (C, 2, 2, 0, 65, 3, 0, 0, 0), once("kCohMx", "k_acq_coh_mx", 18, 1)),
    # the vector forms: n_search x n_dopp x ceil(n_prn / 8) workgroups, one launch, no scratch, no cap, no refusal
    ("vector, one block", (W, 3, 1, 0, 40, 21, 1, 0, 0), once("kVec", "k_acq_weighted", 315, 0)),
    ("vector ms", (W, 3, 10, 0, 40, 21, 1, 0, 0), once("kVecMs", "k_acq_weighted_ms", 315, 0)),
    ("vector ms, 9 PRNs, at 1 MB and refused", (W, 2, 128, 0, 9, 3, 1, 1, 62), once("kVecMs", "k_acq_weighted_ms", 12, 0)),
    ("vector ms, 255 PRNs", (W, 256, 10, 0, 255, 21, 1, 0, 0), once("kVecMs", "k_acq_weighted_ms", 256 * 21 * 32, 0)),
    ("vector coherent", (C, 3, 20, 0, 33, 21, 1, 0, 0), once("kCohVec", "k_acq_coh_vec", 315, 0)),
    ("vector coherent, 8 PRNs", (C, 3, 2, 0, 8, 21, 1, 0, 0), once("kCohVec", "k_acq_coh_vec", 63, 0)),
    ("vector hyb", (H, 3, 10, 8, 64, 21, 1, 0, 0), once("kHybVec", "k_acq_hyb_vec", 504, 0)),
    ("vector hyb, 65 PRNs, at 1 MB and refused", (H, 3, 2, 2, 65, 21, 1, 1, 62), once("kHybVec", "k_acq_hyb_vec", 567, 0)),
    # the delegations: one window is the coherent call, windows of one block the non-coherent one (n_ms = n_seg), one block of
    # either the one-block call
    ("hyb 5 x 1 = coherent 5", (H, 4, 5, 1, 40, 3, 0, 0, 0), once("kCohMx", "k_acq_coh_mx", 24, 1)),
    ("vector hyb 5 x 1", (H, 4, 5, 1, 40, 3, 1, 0, 0), once("kCohVec", "k_acq_coh_vec", 60, 0)),
    ("hyb 1 x 6 = ms 6", (H, 4, 1, 6, 40, 3, 0, 0, 0), walk(*MS, 24, 24)),
    ("hyb 1 x 6 at 10 MB: the ms walk's chunks", (H, 4, 1, 6, 40, 3, 0, 10, 0), walk(*MS, 24, 5)),
    ("hyb 1 x 6 at 1 MB: the ms walk's refusal", (H, 4, 1, 6, 40, 3, 0, 1, 0), refused(*MS, 24)),
    ("vector hyb 1 x 6", (H, 4, 1, 6, 40, 3, 1, 0, 0), once("kVecMs", "k_acq_weighted_ms", 60, 0)),
    ("hyb 1 x 1", (H, 4, 1, 1, 40, 3, 0, 0, 0), once("kMxw", "k_acq_mxw", 24, 1)),
    ("vector hyb 1 x 1", (H, 4, 1, 1, 40, 3, 1, 0, 0), once("kVec", "k_acq_weighted", 60, 0)),
    ("coherent 1", (C, 4, 1, 0, 40, 3, 0, 0, 0), once("kMxw", "k_acq_mxw", 24, 1)),
    ("vector coherent 1", (C, 4, 1, 0, 40, 3, 1, 0, 0), once("kVec", "k_acq_weighted", 60, 0)),
    ("ms 1", (W, 4, 1, 0, 40, 3, 0, 0, 0), once("kMxw", "k_acq_mxw", 24, 1)),
]


def test_acq_weighted_plan_table(tmp_path):
    plans = G.plan_rows(tmp_path, [row for _, row, _ in ROWS])
    bad = [f"{what}:\n  plan {plan}\n  want {want}" for (what, _, want), plan in zip(ROWS, plans) if plan != want]
    assert not bad, "\n".join(bad)


def test_scratch_is_chunk_times_two_megabytes_and_launches_cover_the_call(tmp_path):
    plans = G.plan_rows(tmp_path, [row for _, row, _ in ROWS])
    walks = [p for p in plans if p["form"] in ("kMxwWalk", "kHybMx") and not p["enomem"]]
    assert len(walks) >= 20
    for p in walks:
        assert p["scratch_bytes"] == p["chunk"] * 2 * MB and p["grid"] == p["chunk"] <= p["units"]
        runs = G.launches(p["units"], p["chunk"])
        assert len(runs) == p["n_chunks"] and sum(n for _, n in runs) == p["units"] and 1 <= runs[-1][1] <= p["chunk"]
    assert all(p["scratch_bytes"] == 0 and p["n_chunks"] == 1 for p in plans if p["form"] not in ("kMxwWalk", "kHybMx"))


def test_acq_weighted_plan_covers_every_form():
    """every AcqWForm and every gpsx_last_kernel name of the weighted grids appears in the table, each walk also refused"""
    forms, names = {want["form"] for _, _, want in ROWS}, {want["name"] for _, _, want in ROWS}
    assert forms == {"kMxw", "kMxwWalk", "kVec", "kVecMs", "kCohMx", "kCohVec", "kHybMx", "kHybVec"}
    assert names == {"k_acq_mxw", "k_acq_wmx_ms", "k_acq_weighted", "k_acq_weighted_ms", "k_acq_coh_mx", "k_acq_coh_vec", "k_acq_hyb_mx",
                     "k_acq_hyb_vec"}
    assert {want["form"] for _, _, want in ROWS if want["enomem"]} == {"kMxwWalk", "kHybMx"}
    header = open(G.os.path.join(G.ROOT, "stm32f4_sdr_gps_amd", "csrc", "gpsx_acq_plan.hpp")).read()
    listed = header.split("enum class AcqWForm {")[1].split("};")[0]
    assert {line.split(",")[0].strip() for line in listed.splitlines() if line.strip().startswith("k")} == forms
