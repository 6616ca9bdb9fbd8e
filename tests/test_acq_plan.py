"""csrc/gpsx_acq_plan.hpp -- the planner that decides which kernels serve one gpsx_acq_grid_dev call -- compiled for the HOST with
g++ and checked on a table of launch shapes at 256 CUs (the MI355X): per call the kernel sequence with grids (k_acq_keys when
the kernels do not write the keys themselves; the caller asked for keys), split_segs, the HBM scratch, whether the merge planes
are taken, and the gpsx_last_kernel name.  The rows were read from the launch code the planner replaced and confirmed under
rocprofv3 --kernel-trace on an MI355X (the rows without refused scratch), through both libraries."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
#include "gpsx_acq_plan.hpp"
#include <stdio.h>
#include <string>
using namespace gpsx;
static std::string k(const char *name, long grid) { return std::string(name) + ":" + std::to_string(grid) + " "; }
int main()
{
  AcqShape g;
  AcqKnobs kn;
  int inspect, no_split, refused;
  while (scanf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d", &g.n_search, &g.n_ms, &g.n_prn, &g.n_dopp, &g.n_bits, &g.shard_index,
               &g.shard_count, &inspect, &kn.algo, &kn.seg, &kn.split, &no_split, &kn.ms_mode, &refused) == 14) {
    g.inspect = inspect;
    kn.no_split = no_split;
    const AcqPlan p = plan_acq(g, kn, 256, refused);
    const long n = (long)p.n_peaks, fin = (n + 255) / 256;
    std::string seq;
    char poly[32];
    snprintf(poly, sizeof poly, "k_acq_poly<8,%d,%d>", p.seg, p.form == AcqForm::kPolyWalk ? 1 : p.form == AcqForm::kPolyStore ? 2 : 0);
    if (p.unit_hi > p.unit_lo) {
      switch (p.form) {
      case AcqForm::kMxSingle: seq = k("k_acq_mx<0>", p.grid); break;
      case AcqForm::kMxSplit: seq = k("k_acq_mx<5>", p.grid) + k("k_acq_finalize", fin); break;
      case AcqForm::kMxTail:
        seq = k("k_acq_mx<0>", p.grid) + k("k_acq_mx<5>", p.grid_tail) + k("k_acq_finalize_from", (n - (long)p.first_peak + 255) / 256);
        break;
      case AcqForm::kMxByte: seq = k("k_acq_mx<4>", p.grid); break;
      case AcqForm::kMxWalk: seq = "memset " + k("k_acq_mx<3>", p.grid) + (p.walk24 ? k("k_acq_mx<1>", p.grid) : ""); break;
      case AcqForm::kMxStore: seq = k("k_acq_mx<2>", p.grid) + k("k_acq_vals_search", n / 8); break;
      case AcqForm::kPoly: seq = k(poly, p.grid) + (p.seg < 16 ? k("k_acq_finalize", fin) : ""); break;
      case AcqForm::kPolyWalk: seq = k(poly, p.grid); break;
      case AcqForm::kPolyStore: seq = k(poly, p.grid) + k("k_acq_vals_search", n / 8); break;
      case AcqForm::kDot8: seq = k(g.n_ms > 1 ? (inspect ? "k_acq<8,true,true>" : "k_acq<8,true,false>")
                                               : (inspect ? "k_acq<8,false,true>" : "k_acq<8,false,false>"), p.grid); break;
      }
    }
    if (p.keys_kernel)
      seq += k("k_acq_keys", ((long)g.n_search * g.n_prn * g.n_dopp + 255) / 256);
    printf("%s| %d %zu %d %s\n", seq.c_str(), p.split_segs, p.energy_bytes, (int)p.planes, p.name[0] ? p.name : "-");
  }
  return 0;
}
"""

MX, POLY, DOT8 = 4, 2, 1
NO_MX, NO_POLY, NO_PLANES = 1, 2, 4


def mx_energy(clusters):
    return clusters * 8 * (16 * 4 * 4 * 64) * 12 + 16384 + clusters * 4


# (call, (n_search, n_ms, n_prn, n_dopp, n_bits, shard_index, shard_count, inspect), knobs (algo, seg, split, no_split, ms_mode),
#  refused scratch, kernel sequence with grids, split_segs, energy bytes, planes, gpsx_last_kernel).  32 PRN x 21 Doppler: 84 units and
#  21 clusters per search.
FINE, BYTE = 8, 1
D = (MX, 0, 0, 0, 0)
ROWS = [
    # the matrix-core forms, default knobs
    ("256 captures (bench headline)", (256, 1, 32, 21, FINE, 0, 0, 0), D, 0, "k_acq_mx<0>:5376", 0, 0, 0, "k_acq_mx<0>"),
    ("1 capture", (1, 1, 32, 21, FINE, 0, 0, 0), D, 0, "k_acq_mx<5>:168 k_acq_finalize:21", 8, 0, 1, "k_acq_mx<5>"),
    ("3 captures", (3, 1, 32, 21, FINE, 0, 0, 0), D, 0, "k_acq_mx<5>:252 k_acq_finalize:63", 4, 0, 1, "k_acq_mx<5>"),
    ("6 captures", (6, 1, 32, 21, FINE, 0, 0, 0), D, 0, "k_acq_mx<5>:252 k_acq_finalize:126", 2, 0, 1, "k_acq_mx<5>"),
    ("8 captures: 168 clusters, more than half a round", (8, 1, 32, 21, FINE, 0, 0, 0), D, 0, "k_acq_mx<0>:168", 0, 0, 0, "k_acq_mx<0>"),
    ("16 captures: full round + split tail", (16, 1, 32, 21, FINE, 0, 0, 0), D, 0,
     "k_acq_mx<0>:256 k_acq_mx<5>:160 k_acq_finalize_from:84", 2, 0, 1, "k_acq_mx<0>"),
    ("64 captures: full rounds + split tail", (64, 1, 32, 21, FINE, 0, 0, 0), D, 0,
     "k_acq_mx<0>:1280 k_acq_mx<5>:256 k_acq_finalize_from:84", 4, 0, 1, "k_acq_mx<0>"),
    ("20 captures: tail of 164 clusters, more than half a round", (20, 1, 32, 21, FINE, 0, 0, 0), D, 0, "k_acq_mx<0>:420", 0, 0, 0,
     "k_acq_mx<0>"),
    ("1 capture, shard 0 of 2", (1, 1, 32, 21, FINE, 0, 2, 0), D, 0, "k_acq_mx<0>:11 k_acq_keys:3", 0, 0, 0, "k_acq_mx<0>"),
    ("1 capture, shard 1 of 2", (1, 1, 32, 21, FINE, 1, 2, 0), D, 0, "k_acq_mx<0>:11 k_acq_keys:3", 0, 0, 0, "k_acq_mx<0>"),
    ("1 unit, shard 0 of 2: nothing to launch", (1, 1, 1, 1, FINE, 0, 2, 0), D, 0, "k_acq_keys:1", 0, 0, 0, "-"),
    ("1 search x 10 blocks: store form", (1, 10, 32, 21, FINE, 0, 0, 0), D, 0, "k_acq_mx<2>:210 k_acq_vals_search:672 k_acq_keys:3", 0,
     10 * 32 * 21 * 32768, 0, "k_acq_mx<2>"),
    ("256 searches x 10 blocks: walk16 + walk24", (256, 10, 32, 21, FINE, 0, 0, 0), D, 0, "memset k_acq_mx<3>:5376 k_acq_mx<1>:5376", 0,
     mx_energy(5376), 0, "k_acq_mx<3>"),
    ("64 searches x 5 blocks: walk16 alone", (64, 5, 32, 21, FINE, 0, 0, 0), D, 0, "memset k_acq_mx<3>:1344", 0, mx_energy(1344), 0,
     "k_acq_mx<3>"),
    ("256 searches x 10 blocks, shard 0 of 2", (256, 10, 32, 21, FINE, 0, 2, 0), D, 0,
     "memset k_acq_mx<3>:2688 k_acq_mx<1>:2688 k_acq_keys:672", 0, mx_energy(2688), 0, "k_acq_mx<3>"),
    ("256 captures, byte phases", (256, 1, 32, 21, BYTE, 0, 0, 0), D, 0, "k_acq_mx<4>:256", 0, 0, 0, "k_acq_mx<4>"),
    ("1 capture, byte phases", (1, 1, 32, 21, BYTE, 0, 0, 0), D, 0, "k_acq_mx<4>:21", 0, 0, 0, "k_acq_mx<4>"),
    ("24 captures, 72 PRNs, byte phases: 3 PRN sets", (24, 1, 72, 21, BYTE, 0, 0, 0), D, 0, "k_acq_mx<4>:255", 0, 0, 0, "k_acq_mx<4>"),
    ("1 search x 10 blocks, byte phases: dot8", (1, 10, 32, 21, BYTE, 0, 0, 0), D, 0, "k_acq<8,true,false>:84 k_acq_keys:3", 0, 0, 0,
     "k_acq<8,true,dot8>"),
    ("1 capture, inspection outputs: dot8", (1, 1, 32, 21, FINE, 0, 0, 1), D, 0, "k_acq<8,false,true>:672 k_acq_keys:3", 0, 0, 0,
     "k_acq<8,false,dot8>"),
    ("1 search x 10 blocks, inspection outputs", (1, 10, 32, 21, FINE, 0, 0, 1), D, 0, "k_acq<8,true,true>:672 k_acq_keys:3", 0, 0, 0,
     "k_acq<8,true,dot8>"),
    # the lab knobs
    ("1 capture, $GPSX_ACQ_SPLIT=4", (1, 1, 32, 21, FINE, 0, 0, 0), (MX, 0, 4, 0, 0), 0, "k_acq_mx<5>:84 k_acq_finalize:21", 4, 0, 1,
     "k_acq_mx<5>"),
    ("16 captures, $GPSX_ACQ_SPLIT=8: the tail would not fit", (16, 1, 32, 21, FINE, 0, 0, 0), (MX, 0, 8, 0, 0), 0,
     "k_acq_mx<0>:256 k_acq_mx<5>:160 k_acq_finalize_from:84", 2, 0, 1, "k_acq_mx<0>"),
    ("64 captures, $GPSX_ACQ_SPLIT=2", (64, 1, 32, 21, FINE, 0, 0, 0), (MX, 0, 2, 0, 0), 0,
     "k_acq_mx<0>:1280 k_acq_mx<5>:128 k_acq_finalize_from:84", 2, 0, 1, "k_acq_mx<0>"),
    ("1 capture, $GPSX_ACQ_NO_SPLIT", (1, 1, 32, 21, FINE, 0, 0, 0), (MX, 0, 0, 1, 0), 0, "k_acq_mx<0>:21", 0, 0, 0, "k_acq_mx<0>"),
    ("1 search x 10 blocks, $GPSX_ACQ_MS_MODE=walk", (1, 10, 32, 21, FINE, 0, 0, 0), (MX, 0, 0, 0, 1), 0,
     "memset k_acq_mx<3>:21 k_acq_mx<1>:21", 0, mx_energy(21), 0, "k_acq_mx<3>"),
    ("256 searches x 10 blocks, $GPSX_ACQ_MS_MODE=blocks", (256, 10, 32, 21, FINE, 0, 0, 0), (MX, 0, 0, 0, 2), 0,
     "k_acq_mx<2>:53760 k_acq_vals_search:172032 k_acq_keys:672", 0, 256 * 10 * 32 * 21 * 32768, 0, "k_acq_mx<2>"),
    ("1 capture, $GPSX_ACQ_ALGO=dot8", (1, 1, 32, 21, FINE, 0, 0, 0), (DOT8, 0, 0, 0, 0), 0, "k_acq<8,false,false>:672 k_acq_keys:3", 0,
     0, 0, "k_acq<8,false,dot8>"),
    ("1 search x 10 blocks, $GPSX_ACQ_ALGO=dot8", (1, 10, 32, 21, FINE, 0, 0, 0), (DOT8, 0, 0, 0, 0), 0,
     "k_acq<8,true,false>:672 k_acq_keys:3", 0, 0, 0, "k_acq<8,true,dot8>"),
    ("256 captures, $GPSX_ACQ_SEG=4 (selects the polyphase kernel)", (256, 1, 32, 21, FINE, 0, 0, 0), (POLY, 4, 0, 0, 0), 0,
     "k_acq_poly<8,4,0>:86016 k_acq_finalize:5376 k_acq_keys:672", 0, 0, 1, "k_acq_poly<8,4,0>"),
    ("1 capture, $GPSX_ACQ_SEG=16", (1, 1, 32, 21, FINE, 0, 0, 0), (POLY, 16, 0, 0, 0), 0, "k_acq_poly<8,16,0>:84 k_acq_keys:3", 0, 0,
     1, "k_acq_poly<8,16,0>"),
    ("1 capture, $GPSX_ACQ_SEG=8", (1, 1, 32, 21, FINE, 0, 0, 0), (POLY, 8, 0, 0, 0), 0,
     "k_acq_poly<8,8,0>:168 k_acq_finalize:21 k_acq_keys:3", 0, 0, 1, "k_acq_poly<8,8,0>"),
    # the vector path (gpsx_set_acq_path(VECTOR))
    ("vector: 256 captures", (256, 1, 32, 21, FINE, 0, 0, 0), (POLY, 0, 0, 0, 0), 0, "k_acq_poly<8,16,0>:21504 k_acq_keys:672", 0, 0,
     1, "k_acq_poly<8,16,0>"),
    ("vector: 16 captures", (16, 1, 32, 21, FINE, 0, 0, 0), (POLY, 0, 0, 0, 0), 0,
     "k_acq_poly<8,8,0>:2688 k_acq_finalize:336 k_acq_keys:42", 0, 0, 1, "k_acq_poly<8,8,0>"),
    ("vector: 1 capture", (1, 1, 32, 21, FINE, 0, 0, 0), (POLY, 0, 0, 0, 0), 0, "k_acq_poly<8,4,0>:336 k_acq_finalize:21 k_acq_keys:3",
     0, 0, 1, "k_acq_poly<8,4,0>"),
    ("vector: 1 capture, shard 1 of 2", (1, 1, 32, 21, FINE, 1, 2, 0), (POLY, 0, 0, 0, 0), 0,
     "k_acq_poly<8,4,0>:168 k_acq_finalize:21 k_acq_keys:3", 0, 0, 1, "k_acq_poly<8,4,0>"),
    ("vector: 1 search x 10 blocks, store form", (1, 10, 32, 21, FINE, 0, 0, 0), (POLY, 0, 0, 0, 0), 0,
     "k_acq_poly<8,8,2>:1680 k_acq_vals_search:672 k_acq_keys:3", 0, 10 * 32 * 21 * 32768, 1, "k_acq_poly<8,8,2>"),
    ("vector: 8 searches x 10 blocks, store form", (8, 10, 32, 21, FINE, 0, 0, 0), (POLY, 0, 0, 0, 0), 0,
     "k_acq_poly<8,16,2>:6720 k_acq_vals_search:5376 k_acq_keys:21", 0, 8 * 10 * 32 * 21 * 32768, 1, "k_acq_poly<8,16,2>"),
    ("vector: 64 searches x 10 blocks, walk form", (64, 10, 32, 21, FINE, 0, 0, 0), (POLY, 0, 0, 0, 0), 0,
     "k_acq_poly<8,16,1>:5376 k_acq_keys:168", 0, 5376 * 8 * 16384 * 4, 1, "k_acq_poly<8,16,1>"),
    ("vector: 1 search x 10 blocks, $GPSX_ACQ_MS_MODE=walk", (1, 10, 32, 21, FINE, 0, 0, 0), (POLY, 0, 0, 0, 1), 0,
     "k_acq_poly<8,16,1>:84 k_acq_keys:3", 0, 84 * 8 * 16384 * 4, 1, "k_acq_poly<8,16,1>"),
    ("vector: 1 capture, byte phases: dot8", (1, 1, 32, 21, BYTE, 0, 0, 0), (POLY, 0, 0, 0, 0), 0,
     "k_acq<8,false,false>:84 k_acq_keys:3", 0, 0, 0, "k_acq<8,false,dot8>"),
    ("vector: 1 unit, shard 0 of 2: nothing to launch", (1, 1, 1, 1, FINE, 0, 2, 0), (POLY, 0, 0, 0, 0), 0, "k_acq_keys:1", 0, 0, 1,
     "-"),
    ("dot8: 1 unit, shard 0 of 2: nothing to launch", (1, 1, 1, 1, FINE, 0, 2, 0), (DOT8, 0, 0, 0, 0), 0, "k_acq_keys:1", 0, 0, 0,
     "k_acq<8,false,dot8>"),
    # scratch refused: matrix -> polyphase -> dot8; no planes -> unsplit
    ("256 searches x 10 blocks, matrix scratch refused", (256, 10, 32, 21, FINE, 0, 0, 0), D, NO_MX,
     "k_acq_poly<8,16,1>:21504 k_acq_keys:672", 0, 21504 * 8 * 16384 * 4, 1, "k_acq_poly<8,16,1>"),
    ("1 search x 10 blocks, matrix scratch refused", (1, 10, 32, 21, FINE, 0, 0, 0), D, NO_MX,
     "k_acq_poly<8,8,2>:1680 k_acq_vals_search:672 k_acq_keys:3", 0, 10 * 32 * 21 * 32768, 1, "k_acq_poly<8,8,2>"),
    ("256 searches x 10 blocks, both refused", (256, 10, 32, 21, FINE, 0, 0, 0), D, NO_MX | NO_POLY,
     "k_acq<8,true,false>:172032 k_acq_keys:672", 0, 0, 0, "k_acq<8,true,dot8>"),
    ("vector: 64 searches x 10 blocks, scratch refused", (64, 10, 32, 21, FINE, 0, 0, 0), (POLY, 0, 0, 0, 0), NO_POLY,
     "k_acq<8,true,false>:43008 k_acq_keys:168", 0, 0, 0, "k_acq<8,true,dot8>"),
    ("1 capture, planes refused", (1, 1, 32, 21, FINE, 0, 0, 0), D, NO_PLANES, "k_acq_mx<0>:21", 0, 0, 0, "k_acq_mx<0>"),
    ("16 captures, planes refused", (16, 1, 32, 21, FINE, 0, 0, 0), D, NO_PLANES, "k_acq_mx<0>:336", 0, 0, 0, "k_acq_mx<0>"),
]


def plan_rows(tmp_path, rows):
    src = tmp_path / "acq_plan.cpp"
    src.write_text(DRIVER)
    exe = tmp_path / "acq_plan"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "stm32f4_sdr_gps_amd", "csrc"),
                           "-o", str(exe), str(src)])
    lines = "".join(" ".join(map(str, shape + knobs + (refused,))) + "\n" for _, shape, knobs, refused, *_ in rows)
    return subprocess.run([str(exe)], input=lines, capture_output=True, text=True, check=True).stdout.splitlines()


def test_acq_plan_table(tmp_path):
    out = plan_rows(tmp_path, ROWS)
    assert len(out) == len(ROWS)
    bad = []
    for (call, _, _, _, seq, segs, energy, planes, name), line in zip(ROWS, out):
        want = f"{seq + ' ' if seq else ''}| {segs} {energy} {planes} {name}"
        if line != want:
            bad.append(f"{call}:\n  plan {line}\n  want {want}")
    assert not bad, "\n".join(bad)


def test_acq_plan_covers_every_form(tmp_path):
    """Every kernel the grid call can launch appears in the table, and every form's name."""
    seqs = " ".join(r[4] for r in ROWS)
    for kernel in ["k_acq_mx<0>", "k_acq_mx<1>", "k_acq_mx<2>", "k_acq_mx<3>", "k_acq_mx<4>", "k_acq_mx<5>", "k_acq_finalize:",
                   "k_acq_finalize_from", "k_acq_vals_search", "k_acq_poly<8,4,0>", "k_acq_poly<8,8,0>", "k_acq_poly<8,16,0>",
                   "k_acq_poly<8,16,1>", "k_acq_poly<8,8,2>", "k_acq_poly<8,16,2>", "k_acq<8,false,false>", "k_acq<8,true,false>",
                   "k_acq<8,false,true>", "k_acq<8,true,true>", "k_acq_keys", "memset"]:
        assert kernel in seqs, kernel
