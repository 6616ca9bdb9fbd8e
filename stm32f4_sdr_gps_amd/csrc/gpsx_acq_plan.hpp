// gpsx_acq_plan.hpp -- which kernels serve one acquisition grid call (gpsx_acq_grid_dev), with what grids and scratch: the one
// place that decides.  Pure host C++ (no HIP): tests/test_acq_plan.py compiles it with g++ and checks a table of launch shapes.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace gpsx {

constexpr int kAcqGroup = 8;      // PRNs per accumulator set (one main-loop pass) in the grid kernel.  A sharding unit is (search,
                                  // Doppler bin, 8-PRN group) -- 84 units per 32 PRN x 21 Doppler search, SURVEY.md 8(e).  Unit
                                  // index u = (search * n_dopp + dopp) * n_groups + group (group fastest); shard r of W owns the
                                  // contiguous run [r * U / W, (r + 1) * U / W) -- balanced to one unit, and the four groups of a
                                  // (search, Doppler) pair stay on one GPU (the matrix-core kernel sweeps 32 PRNs at once)
constexpr int kMaxMs = 128;       // keeps (energy << 11 | phase) and the window sum inside 32 bits
constexpr int kAlgoDot8 = 1;      // main loop: v_dot8_u32_u4 on 4-bit block sums, 8 chips per instruction
constexpr int kAlgoPoly = 2;      // fine grid only: polyphase recurrence across the 16 sample offsets, AND + popcount
constexpr int kAlgoMx = 4;        // the same recurrence as a Toeplitz GEMM on the matrix cores, MX-FP4: the default at every
                                  // launch size, for fine grids and single-block byte-phase grids without inspection outputs

// scratch of the block-parallel multi-block forms: every block's magnitudes, u16 per hypothesis
inline size_t acq_poly_vals_bytes(int n_search, int n_ms, int n_prn, int n_dopp)
{
  return (size_t)n_search * n_ms * n_prn * n_dopp * 16 * 1024 * sizeof(uint16_t);
}
// scratch of k_acq_poly's walk: the running per-hypothesis sums between blocks
inline size_t acq_poly_energy_bytes(long local_units) { return (size_t)local_units * kAcqGroup * 16 * 1024 * sizeof(uint32_t); }
constexpr size_t kMxZeroRecBytes = 16384;          // a tile-row's worth of all-zero records in front of the flags: what the walk
                                                   // forms "read back" in the first block of a search (16 offsets x ... of the
                                                   // same addresses: 4 tiles x 64 lanes x 4 groups x 12 B = 12 KB, rounded up)
inline size_t acq_mx_energy_bytes(long clusters)   // per workgroup: 8 waves x 16 offsets x 4 tiles x 4 groups x 64 lanes x 12 B
{                                                  // (the 24-bit records of the fallback form), + the zero records + one overflow flag
  return (size_t)clusters * 8 * (16 * 4 * 4 * 64) * 12 + kMxZeroRecBytes + (size_t)clusters * 4;
}

// The lab knobs (lib/libgpsx_lab.so reads them from the environment in gpsx_create; the product only sets `algo`, through
// gpsx_set_acq_path): forced kernel forms for the parity tests of the alternative kernels and for A/B measurements.
struct AcqKnobs {
  int algo = kAlgoMx;     // $GPSX_ACQ_ALGO = mx (default: the matrix-core kernel, at every launch size) | poly | dot8
  int seg = 0;            // $GPSX_ACQ_SEG = 4 | 8 | 16: the polyphase kernel at that many offsets per workgroup (implies
                          // $GPSX_ACQ_ALGO=poly unless another algorithm was named)
  int split = 0;          // $GPSX_ACQ_SPLIT: workgroups per cluster of the split form (2, 4, 8; 0 = by launch size)
  bool no_split = false;  // $GPSX_ACQ_NO_SPLIT: small single-block fine grids stay one workgroup per cluster
  int ms_mode = 0;        // $GPSX_ACQ_MS_MODE = walk (1) | blocks (2): force one multi-block form; 0 = by size
  int wms_scratch_mb = 0; // $GPSX_ACQ_WMS_SCRATCH_MB: cap on the weighted multi-block walk's scratch per launch (0 = the default)
};

struct AcqShape {
  int n_search, n_ms, n_prn, n_dopp, n_bits;   // n_bits: 8 (fine phases) or 1 (byte phases)
  int shard_index, shard_count;                // as in gpsx_acq_grid_t (shard_count 0: unsharded)
  bool inspect;                                // per-block triplets, energy plane or raw counts asked for
};

// Scratch the caller could not get (plan_acq's `refused`): the form that needs it is passed over for the next one.
constexpr int kNoMxScratch = 1, kNoPolyScratch = 2, kNoPlanes = 4;

enum class AcqForm {
  kMxSingle,   // k_acq_mx<0>: a workgroup per cluster
  kMxSplit,    // k_acq_mx<5> (split_segs workgroups per cluster) + k_acq_finalize
  kMxTail,     // k_acq_mx<0> on the full rounds, k_acq_mx<5> on the last (grid_tail, from c_tail), k_acq_finalize_from
  kMxByte,     // k_acq_mx<4>: persistent workgroups, byte phases
  kMxWalk,     // zero records, k_acq_mx<3> (16-bit sums), k_acq_mx<1> behind it when walk24
  kMxStore,    // k_acq_mx<2>, a workgroup per (cluster, block), + k_acq_vals_search
  kPoly,       // k_acq_poly<8,seg,0> (+ k_acq_finalize for seg 4 and 8)
  kPolyWalk,   // k_acq_poly<8,16,1>
  kPolyStore,  // k_acq_poly<8,seg,2> + k_acq_vals_search
  kDot8,       // k_acq<8, n_ms > 1, inspect>
};

struct AcqPlan {
  AcqForm form;
  bool mx;                   // a k_acq_mx form (launch_acq_mx)
  long unit_lo, unit_hi;     // this shard's run of sharding units
  int n_groups;
  int c_lo, c_hi, c_tail;    // the clusters (32-PRN sets of one search and Doppler) that meet the units; kMxTail: first of the tail
  long grid, grid_tail;      // workgroups of the form's main kernel; kMxTail: of k_acq_mx<5>
  int split_segs, seg;       // k_acq_mx<5>: workgroups per cluster; k_acq_poly: sample offsets per workgroup
  bool walk24;               // kMxWalk: the 24-bit walk follows the 16-bit one
  size_t n_peaks, first_peak;   // the call's peaks; kMxTail: the first one k_acq_finalize_from converts
  size_t energy_bytes;       // HBM scratch (gpsx_ctx::d_energy) the form needs, 0: none
  bool planes;               // the two u32 planes of n_peaks entries (gpsx_ctx::d_acc)
  bool keys_in_kernels;      // AcqParams::keys = the caller's keys (unsharded k_acq_mx launches)
  bool keys_kernel;          // k_acq_keys must write the keys
  const char *name;          // gpsx_last_kernel
};

inline AcqPlan plan_acq(const AcqShape &g, const AcqKnobs &k, int n_cus, int refused)
{
  AcqPlan p{};
  const int shards = g.shard_count > 0 ? g.shard_count : 1, shard = g.shard_count > 0 ? g.shard_index : 0;
  p.n_groups = (g.n_prn + kAcqGroup - 1) / kAcqGroup;
  const long n_units = (long)g.n_search * p.n_groups * g.n_dopp;
  p.unit_lo = n_units * shard / shards, p.unit_hi = n_units * (shard + 1) / shards;
  const long units = p.unit_hi - p.unit_lo;
  const int n_sets = (p.n_groups + 3) / 4;
  if (units > 0) {
    auto cluster_of = [&](long unit) { return (int)((unit / p.n_groups) * n_sets + (unit % p.n_groups) / 4); };
    p.c_lo = cluster_of(p.unit_lo);
    p.c_hi = cluster_of(p.unit_hi - 1) + 1;
  }
  const long nc = p.c_hi - p.c_lo;
  p.n_peaks = (size_t)g.n_search * g.n_prn * g.n_dopp * g.n_bits;
  const size_t vals_bytes = acq_poly_vals_bytes(g.n_search, g.n_ms, g.n_prn, g.n_dopp);
  p.keys_kernel = true;
  // The matrix-core kernel (one 512-thread workgroup per (search, Doppler, 32 PRNs), one per CU) is the faster one at
  // every launch size measured, a single capture included (0.155 ms against 0.166 ms, profiles/r02_launch_size_sweep.json).
  // (and serves the byte-phase grid as sample offsets 0 and 8 of the fine one: ten of its seventeen passes, two epilogues)
  p.mx = k.algo == kAlgoMx && !g.inspect && (g.n_bits == 8 || g.n_ms == 1) && !(refused & kNoMxScratch);
  if (p.mx) {
    p.keys_in_kernels = shards == 1;   // (a shard's foreign units must read as zero: k_acq_keys sees to that)
    p.keys_kernel = !p.keys_in_kernels || units <= 0;
    p.name = "k_acq_mx<0>";
    auto ladder = [&](long clusters) { return 8 * clusters <= n_cus ? 8 : 4 * clusters <= n_cus ? 4 : 2; };
    const long tail = nc % n_cus;
    const bool split = g.n_ms == 1 && g.n_bits == 8 && shards == 1 && !k.no_split && !(refused & kNoPlanes);
    if (g.n_ms > 1) {
      // n_ms > 1, few searches: a workgroup per (cluster, block) instead of a workgroup walking its cluster's blocks -- a lone
      // ten-block search is 210 workgroups (one round of the chip) instead of 21 doing ten blocks each
      const bool store = k.ms_mode ? k.ms_mode == 2 : nc < n_cus && vals_bytes <= ((size_t)8 << 30);
      p.form = store ? AcqForm::kMxStore : AcqForm::kMxWalk;
      p.grid = store ? nc * g.n_ms : nc;
      p.energy_bytes = store ? vals_bytes : acq_mx_energy_bytes(nc);
      // 16-bit running sums first; where they cannot overflow (n_ms x 11573 < 2^16) that is all, otherwise the 24-bit form
      // follows and redoes the clusters whose flag went up
      p.walk24 = !store && g.n_ms * 11573 > 65535;
      p.keys_kernel |= store;
      p.name = store ? "k_acq_mx<2>" : "k_acq_mx<3>";
    } else if (g.n_bits == 1) {
      // byte-phase grid: sample offsets 0 and 8, each started from its own block sums; one software pipeline per persistent
      // workgroup, and a workgroup keeps ONE PRN set's tables: the grid is a multiple of n_sets
      p.form = AcqForm::kMxByte;
      p.grid = nc < n_cus ? nc : n_cus - n_cus % n_sets;
      p.name = "k_acq_mx<4>";
    } else if (split && 2 * nc <= n_cus) {
      // fewer clusters than half the chip (a lone cold start is 21): two workgroups per cluster with eight sample offsets each,
      // four with four each from a quarter of the chip down (a lone cold start: 21 clusters -> 168 workgroups); merged through
      // the planes + k_acq_finalize.  $GPSX_ACQ_SPLIT: 2, 4 or 8 whatever the launch size.
      p.form = AcqForm::kMxSplit;
      p.split_segs = k.split ? k.split : ladder(nc);
      p.grid = p.split_segs * nc;
      p.planes = true;
      p.name = "k_acq_mx<5>";
    } else if (split && nc > n_cus && tail > 0 && 2 * tail <= n_cus) {
      // One workgroup per cluster and CU: a launch is rounds of n_cus clusters, and a last round that fills at most half of the
      // chip takes as long as a full one.  Then the full rounds go out as they are and the leftover clusters in the split form
      // behind them -- 2, 4 or 8 workgroups per cluster, as many as still fit ONE round, each with a run of sample offsets it
      // starts directly (16 captures = 336 clusters: 256 + 80 x 2; 64 captures = 1344: 1280 + 64 x 4).  $GPSX_ACQ_SPLIT here
      // too, as long as the tail still fits one round.
      p.form = AcqForm::kMxTail;
      p.grid = nc - tail;
      p.c_tail = (int)(p.c_hi - tail);
      p.split_segs = k.split && k.split * tail <= n_cus ? k.split : ladder(tail);
      p.grid_tail = p.split_segs * tail;
      // the planes of the tail's peaks only: from the first peak of the search the tail begins in
      p.first_peak = (size_t)(p.c_tail / (n_sets * g.n_dopp)) * g.n_prn * g.n_dopp * g.n_bits;
      p.planes = true;
    } else {
      p.form = AcqForm::kMxSingle;
      p.grid = nc;
    }
  } else if ((k.algo == kAlgoPoly || k.algo == kAlgoMx) && g.n_bits == 8 && !g.inspect && !(refused & kNoPolyScratch)) {
    p.planes = true;   // (zeroed when allocated, kept zero by k_acq_finalize; taken by every polyphase form)
    if (g.n_ms > 1) {
      // Scratch in HBM between blocks.  Many searches: each workgroup walks the blocks of its unit and keeps 64 KB of
      // running sums per (PRN, Doppler) pair of this shard (2.7 GB for 64 simultaneous cold-start searches).  Fewer
      // searches (fewer workgroups than six rounds of the chip's 768 slots): a workgroup per (unit, block) instead, all
      // blocks' magnitudes as u16 (32 KB per pair and block), summed and searched by a second small kernel -- a single
      // 10-block cold-start search then takes 0.84 ms instead of 2.8, and the form stays ahead up to ~40 searches.
      // Eight-offset workgroups when that is still a small launch: no merge is needed there, every hypothesis is stored on
      // its own.  When the scratch cannot be had, the register-resident dot8 kernel does the job.
      const bool store = k.ms_mode ? k.ms_mode == 2 : units < 6 * 768 && vals_bytes <= ((size_t)8 << 30);
      p.form = store ? AcqForm::kPolyStore : AcqForm::kPolyWalk;
      p.seg = store && units * g.n_ms < 6 * 768 ? 8 : 16;
      p.grid = (store ? units * g.n_ms : units) * (16 / p.seg);
      p.energy_bytes = store ? vals_bytes : acq_poly_energy_bytes(units);
      p.name = !store ? "k_acq_poly<8,16,1>" : p.seg == 16 ? "k_acq_poly<8,16,2>" : "k_acq_poly<8,8,2>";
    } else {
      // One workgroup per chip (16 offsets: one direct step + 15 recurrence steps; results merged in LDS and written once)
      // when that still leaves several waves of workgroups per CU slot; otherwise two (8 offsets each) or, for launches of
      // a capture or two, four (4 offsets each), merged through global atomics on the planes and converted by
      // k_acq_finalize -- balance and latency against the extra direct steps.  $GPSX_ACQ_SEG forces one.
      p.form = AcqForm::kPoly;
      p.seg = k.seg ? k.seg : units >= 6 * 768 ? 16 : units >= 768 ? 8 : 4;
      p.grid = units * (16 / p.seg);
      p.name = p.seg == 16 ? "k_acq_poly<8,16,0>" : p.seg == 8 ? "k_acq_poly<8,8,0>" : "k_acq_poly<8,4,0>";
    }
  } else {
    p.form = AcqForm::kDot8;
    p.grid = units * g.n_bits;
    p.name = g.n_ms > 1 ? "k_acq<8,true,dot8>" : "k_acq<8,false,dot8>";
  }
  if (units <= 0 && p.form != AcqForm::kDot8)
    p.name = "";   // (nothing of the grid is this shard's: nothing is launched)
  return p;
}

// ---- the weighted two-bit grid (gpsx_acq_grid_weighted_ms; n_ms = 1 is gpsx_acq_grid_weighted) ------------------------------
// The matrix-core walk (k_acq_wmx_ms): a workgroup per cluster (search, Doppler bin, 32-PRN set) walks the search's blocks and keeps
// its running sums E(tau) as u32 in HBM between them: 16 sample offsets x 8 waves x 16 (tile, quad of PRN rows) x 64 lanes x 16 B.
constexpr size_t kMxwMsClusterBytes = (size_t)16 * 8 * 16 * 64 * 16;   // 2 MB per cluster in flight
constexpr int kWmsScratchMbDefault = 2048;                               // 1024 clusters per launch: four rounds of 256 CUs

struct AcqWShape {
  int n_search, n_ms, n_prn, n_dopp;
  bool vector;                 // GPSX_ACQ_PATH_VECTOR
};

enum class AcqWForm {
  kMxw,        // k_acq_mxw: one block (n_ms = 1), a workgroup per cluster
  kMxwWalk,    // k_acq_wmx_ms: a workgroup per cluster walks n_ms blocks, running sums through HBM scratch, in chunks of clusters
  kVec,        // k_acq_weighted: one block, a workgroup per (search, Doppler, 8 PRNs)
  kVecMs,      // k_acq_weighted_ms: the same workgroups, running sums in registers (no scratch)
  kCohMx,      // k_acq_coh_mx: n_coh blocks summed sample by sample, one correlation; a workgroup per cluster (no scratch)
  kCohVec,     // k_acq_coh_vec: the same on the vector ALU, a workgroup per (search, Doppler, 8 PRNs) (no scratch)
  kHybMx,      // k_acq_hyb_mx: a workgroup per cluster walks n_seg coherent windows, running sums through HBM scratch, in chunks
  kHybVec,     // k_acq_hyb_vec: a workgroup per (search, Doppler, 8 PRNs), running sums in registers (no scratch)
};

struct AcqWPlan {
  AcqWForm form;
  bool mx;
  bool enomem;           // not even one cluster's scratch could be had: GPSX_ENOMEM
  long units;            // clusters (matrix) or workgroups (vector) of the whole call
  long chunk;            // units per launch (the last launch takes the rest)
  int n_chunks;
  long grid;             // workgroups of a full chunk's launch
  size_t scratch_bytes;  // HBM scratch (gpsx_ctx::d_energy) of one chunk, 0: none
  const char *name;      // gpsx_last_kernel
};

// The chunks of a walk whose clusters keep kMxwMsClusterBytes of running sums each: as many clusters per launch as the cap holds,
// whole rounds of the chip when that is at least one (a launch is rounds of one workgroup per CU), never more than the call has;
// every refusal halves it.  p.units is set; p.enomem if not even one cluster is left.
inline void plan_wms_chunks(AcqWPlan &p, const AcqKnobs &k, int n_cus, int refused)
{
  const size_t cap = (size_t)(k.wms_scratch_mb > 0 ? k.wms_scratch_mb : kWmsScratchMbDefault) << 20;
  long chunk = (long)(cap / kMxwMsClusterBytes);
  if (chunk >= n_cus)
    chunk -= chunk % n_cus;
  chunk = chunk < p.units ? chunk : p.units;
  chunk = refused < 62 ? chunk >> refused : 0;
  if (chunk < 1) {
    p.enomem = true;
    return;
  }
  p.chunk = p.grid = chunk;
  p.n_chunks = (int)((p.units + chunk - 1) / chunk);
  p.scratch_bytes = (size_t)chunk * kMxwMsClusterBytes;
}

// `refused`: how many scratch requests of this call were refused so far -- each halves the chunk.
inline AcqWPlan plan_acq_weighted(const AcqWShape &g, const AcqKnobs &k, int n_cus, int refused)
{
  AcqWPlan p{};
  p.mx = !g.vector;
  if (!p.mx) {
    // vector ALU: the running sums of a thread's 4 chip offsets x 8 PRNs stay in registers; blocks inner, sample offsets outer
    p.form = g.n_ms == 1 ? AcqWForm::kVec : AcqWForm::kVecMs;
    p.units = (long)g.n_search * g.n_dopp * ((g.n_prn + 7) / 8);
    p.chunk = p.grid = p.units;
    p.n_chunks = 1;
    p.name = g.n_ms == 1 ? "k_acq_weighted" : "k_acq_weighted_ms";
    return p;
  }
  p.units = (long)g.n_search * g.n_dopp * ((g.n_prn + 31) / 32);
  if (g.n_ms == 1) {
    p.form = AcqWForm::kMxw;
    p.chunk = p.grid = p.units;
    p.n_chunks = 1;
    p.name = "k_acq_mxw";
    return p;
  }
  p.form = AcqWForm::kMxwWalk;
  p.name = "k_acq_wmx_ms";
  plan_wms_chunks(p, k, n_cus, refused);
  return p;
}

// ---- the weighted grid over n_coh blocks integrated coherently (gpsx_acq_grid_weighted_coh; g.n_ms = n_coh) -----------------
// Twenty blocks are one navigation-data bit, and the limit of the pre-summed samples' int8 differences (|dM| <= 6 n_coh <= 120).
constexpr int kMaxCoh = 20;

// One launch, no scratch: a workgroup adds its search's blocks in LDS and correlates the sum once.  n_coh = 1 is the one-block
// call's plan (its kernels: byte-identical records by construction).
inline AcqWPlan plan_acq_coherent(const AcqWShape &g)
{
  if (g.n_ms == 1)
    return plan_acq_weighted(g, AcqKnobs{}, 1, 0);
  AcqWPlan p{};
  p.mx = !g.vector;
  p.form = p.mx ? AcqWForm::kCohMx : AcqWForm::kCohVec;
  p.units = (long)g.n_search * g.n_dopp * (p.mx ? (g.n_prn + 31) / 32 : (g.n_prn + 7) / 8);
  p.chunk = p.grid = p.units;
  p.n_chunks = 1;
  p.name = p.mx ? "k_acq_coh_mx" : "k_acq_coh_vec";
  return p;
}

// ---- n_seg coherent windows of n_coh blocks each, their magnitudes summed (gpsx_acq_grid_weighted_hyb) ------------------------
struct AcqHShape {
  int n_search, n_coh, n_seg, n_prn, n_dopp;
  bool vector;                 // GPSX_ACQ_PATH_VECTOR
};

// One window is the coherent call's plan, windows of one block are the non-coherent call's (n_ms = n_seg): their kernels, their
// records.  Otherwise the matrix form keeps a cluster's running sums in k_acq_wmx_ms's scratch layout and is chunked by its rule;
// the vector form keeps them in registers: one launch, no scratch.
inline AcqWPlan plan_acq_hybrid(const AcqHShape &g, const AcqKnobs &k, int n_cus, int refused)
{
  if (g.n_seg == 1)
    return plan_acq_coherent(AcqWShape{g.n_search, g.n_coh, g.n_prn, g.n_dopp, g.vector});
  if (g.n_coh == 1)
    return plan_acq_weighted(AcqWShape{g.n_search, g.n_seg, g.n_prn, g.n_dopp, g.vector}, k, n_cus, refused);
  AcqWPlan p{};
  p.mx = !g.vector;
  p.form = p.mx ? AcqWForm::kHybMx : AcqWForm::kHybVec;
  p.name = p.mx ? "k_acq_hyb_mx" : "k_acq_hyb_vec";
  p.units = (long)g.n_search * g.n_dopp * (p.mx ? (g.n_prn + 31) / 32 : (g.n_prn + 7) / 8);
  if (p.mx) {
    plan_wms_chunks(p, k, n_cus, refused);
    return p;
  }
  p.chunk = p.grid = p.units;
  p.n_chunks = 1;
  return p;
}

}  // namespace gpsx
