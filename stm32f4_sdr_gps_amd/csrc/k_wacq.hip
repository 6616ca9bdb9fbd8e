// k_wacq.hip -- EXTENSION, not in the reference: acquisition decisions and slot hand-over, the stage between a weighted grid's peak
// records and the sync loop's channel states (include/gpsx.h gpsx_wacq).
//
// One wave per receiver, four receivers per 256-thread workgroup; no LDS, no barrier, no scratch.  What decides the time is the read
// of the receiver's n_prn x n_dopp records (16 bytes each): per PRN row the 64 lanes stride over the bins (a record's max_val
// decides; the row's winner is read whole afterwards, one record per lane), keep the greatest 64-bit key (max_val << 32 | ~bin: the
// greater max_val, then the lower bin), and a butterfly of six __shfl_xor steps leaves the row's key in every lane; lane p keeps
// row p's.  Two rows a turn and four bins per lane and row are requested together, so that a wave that has a CU to itself (256
// receivers are 256 waves) keeps eight loads in flight.  Behind that the wave works on two small sets, a PRN
// per lane and a slot per lane: which PRNs a kept slot holds, the candidates' ranks and the slots they go to are ballots, popcounts
// of masks and shuffles from a wave-uniform lane.  Every ballot and shuffle runs under wave-uniform control flow (a wave whose
// receiver does not exist leaves as a whole; the loops around them have wave-uniform bounds; lane-dependent conditions are
// selects).  The states of a slot that is handed over or evicted are written by the wave together, 8 bytes per lane: the sync
// state's 56 words in one store, the lock, nav, obs and eph states' 16 + 8 + 10 + 24 = 58 in a second.
#include <hip/hip_runtime.h>

#include <cstddef>

#include "gpsx_device.hpp"
#include "gpsx_kernels.hpp"

namespace gpsx {

namespace {

static_assert(sizeof(gpsx_wacq_cfg_t) == 32 && offsetof(gpsx_wacq_cfg_t, det_num) == 4 && offsetof(gpsx_wacq_cfg_t, min_peak) == 12 &&
              offsetof(gpsx_wacq_cfg_t, lead_blocks) == 16 && offsetof(gpsx_wacq_cfg_t, code_per_hz) == 20 &&
              offsetof(gpsx_wacq_cfg_t, evict_after_blocks) == 24 && offsetof(gpsx_wacq_cfg_t, reserved) == 28, "gpsx_wacq_cfg_t layout");
static_assert(sizeof(gpsx_wacq_det_t) == 16 && offsetof(gpsx_wacq_det_t, phase) == 4 && offsetof(gpsx_wacq_det_t, dopp_hz) == 8 &&
              offsetof(gpsx_wacq_det_t, flags) == 12 && offsetof(gpsx_wacq_det_t, slot) == 13 && offsetof(gpsx_wacq_det_t, zero) == 14,
              "gpsx_wacq_det_t layout");
static_assert(sizeof(gpsx_wacq_t) == 64 && offsetof(gpsx_wacq_t, n_dropped) == 20 && offsetof(gpsx_wacq_t, assigned_mask) == 24 &&
              offsetof(gpsx_wacq_t, free_mask) == 48 && offsetof(gpsx_wacq_t, reserved) == 56, "gpsx_wacq_t layout");
static_assert(sizeof(gpsx_peak_t) == 16 && offsetof(gpsx_peak_t, max_val) == 0 && offsetof(gpsx_peak_t, phase) == 4 && offsetof(gpsx_peak_t, sum) == 8,
              "gpsx_peak_t layout");
static_assert(sizeof(gpsx_wsync_state_t) == 448 && offsetof(gpsx_wsync_state_t, loop) == 0 && offsetof(gpsx_wloop_state_t, prn) == 0 &&
              offsetof(gpsx_wloop_state_t, code_phase_fine) == 4 && offsetof(gpsx_wloop_state_t, if_freq_offset_hz) == 8 &&
              offsetof(gpsx_wloop_state_t, if_freq_accum) == 12, "gpsx_wsync_state_t layout");
static_assert(sizeof(gpsx_wlock_state_t) == 128 && offsetof(gpsx_wlock_state_t, blocks_seen) == 0 && offsetof(gpsx_wlock_state_t, flags) == 80 &&
              sizeof(gpsx_wnav_state_t) == 64 && sizeof(gpsx_wobs_state_t) == 80 && sizeof(gpsx_weph_state_t) == 192, "the four stage states");
static_assert(alignof(gpsx_wsync_state_t) == 8 && alignof(gpsx_wlock_state_t) == 8 && alignof(gpsx_wnav_state_t) == 8 &&
              alignof(gpsx_wobs_state_t) == 8 && alignof(gpsx_weph_state_t) == 8, "the states are written in 8-byte words");

constexpr int kSyncWords = 56;                                      // 8-byte words of a sync state
constexpr int kLockWords = 16, kNavWords = 8, kObsWords = 10;       // ... of the other four: 16 + 8 + 10 + 24 = 58 lanes
constexpr int kEphWords = 24;
constexpr u32 kPhases = 16368u;

struct alignas(4) Quad { u32 a, b, c, d; };   // a record at a dword-aligned address: one global_load_dwordx4

__device__ __forceinline__ u64 below(int lane) { return (1ull << lane) - 1ull; }   // the lanes under this one (lane 0 .. 63)

}  // namespace

// PRN numbers by value, eight per word (n_prn <= 64): lane p's is a select among eight scalars, never an indexed copy
struct WacqPrns { u64 w[8]; };

__global__ __launch_bounds__(256) void k_wacq(gpsx_wacq_cfg_t cfg, int n_rx, int n_prn, int n_dopp, int dopp_min_hz, int dopp_step_hz, WacqPrns prns,
                                              const gpsx_peak_t *__restrict__ peaks, gpsx_wsync_state_t *sync, gpsx_wlock_state_t *lock,
                                              gpsx_wnav_state_t *nav, gpsx_wobs_state_t *obs, gpsx_weph_state_t *eph,
                                              gpsx_wacq_t *__restrict__ acq, gpsx_wacq_det_t *__restrict__ det)
{
  const int lane = (int)threadIdx.x & 63;
  const int r = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
  if (r >= n_rx)          // (the whole wave: r is the same in its 64 lanes)
    return;
  const int ch = cfg.ch_per_rx;

  // 1 the best record per PRN: lane p keeps row p's key
  const gpsx_peak_t *rows = peaks + (size_t)r * (size_t)n_prn * (size_t)n_dopp;
  u64 key = 0;            // (below every record's: a key's low word is ~bin >= 2^31)
  // (two rows a turn, four bins per lane and row requested before the first is looked at: eight loads in flight per lane)
  auto wave_key = [](u64 k) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const u64 o = (u64)__shfl_xor((long long)k, m, 64);
      k = o > k ? o : k;
    }
    return k;
  };
#pragma unroll 1
  for (int p = 0; p < n_prn; p += 2) {
    const bool two = p + 1 < n_prn;                        // (wave-uniform; a last odd row is read twice)
    const gpsx_peak_t *row0 = rows + (size_t)p * (size_t)n_dopp, *row1 = rows + (size_t)(two ? p + 1 : p) * (size_t)n_dopp;
    u64 k0 = 0, k1 = 0;
#pragma unroll 1
    for (int d0 = lane; d0 < n_dopp; d0 += 4 * 64) {     // (lane-dependent by one turn at most; no cross-lane operation in here)
      u32 v0[4], v1[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const bool in = d0 + 64 * u < n_dopp;
        v0[u] = in ? row0[d0 + 64 * u].max_val : 0u;
        v1[u] = in ? row1[d0 + 64 * u].max_val : 0u;
      }
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const bool in = d0 + 64 * u < n_dopp;
        const u64 low = (u64)(0xFFFFFFFFu - (u32)(d0 + 64 * u));
        const u64 a = in ? ((u64)v0[u] << 32) | low : 0ull, b = in ? ((u64)v1[u] << 32) | low : 0ull;
        k0 = a > k0 ? a : k0;
        k1 = b > k1 ? b : k1;
      }
    }
    k0 = wave_key(k0);
    k1 = wave_key(k1);
    key = lane == p ? k0 : (two && lane == p + 1 ? k1 : key);
  }
  const bool is_prn = lane < n_prn;
  const u32 M = is_prn ? (u32)(key >> 32) : 0u;
  const u32 bin = is_prn ? 0xFFFFFFFFu - (u32)key : 0u;
  const Quad best = *reinterpret_cast<const Quad *>(rows + (is_prn ? (size_t)lane * (size_t)n_dopp + bin : 0));
  const u32 tau = best.b, S = best.c;
  const int dopp_hz = (int)((u32)dopp_min_hz + bin * (u32)dopp_step_hz);   // (inside int32: the host checked both ends of the grid)
  const u64 word = lane < 8 ? prns.w[0] : lane < 16 ? prns.w[1] : lane < 24 ? prns.w[2] : lane < 32 ? prns.w[3] :
                   lane < 40 ? prns.w[4] : lane < 48 ? prns.w[5] : lane < 56 ? prns.w[6] : prns.w[7];
  const int my_prn = (int)((word >> ((lane & 7) * 8)) & 0xFFull);

  // 2 detection
  const bool detected = is_prn && M >= (cfg.min_peak > 1u ? cfg.min_peak : 1u) &&
                        (u64)M * (u64)kPhases * (u64)cfg.det_den >= (u64)cfg.det_num * (u64)S;

  // 3 slots: lane j is slot j
  const bool is_slot = lane < ch;
  const size_t ch0 = (size_t)r * (size_t)ch;
  const int slot_prn = is_slot ? sync[ch0 + lane].loop.prn : GPSX_PRN_NONE;
  const bool holds = is_slot && slot_prn != GPSX_PRN_NONE;
  bool evicted = false;
  if (cfg.evict_after_blocks > 0) {     // (then lock is not null: the host checked)
    const gpsx_wlock_state_t *ls = lock + ch0 + (is_slot ? lane : 0);
    const long long seen = ls->blocks_seen;
    const u32 lflags = ls->flags;
    evicted = holds && (lflags & GPSX_WLOCK_CODE) == 0 && seen >= (long long)cfg.evict_after_blocks;
  }
  const bool kept = holds && !evicted;
  const u64 kept_mask = __ballot(kept), evicted_mask = __ballot(evicted), free_before = __ballot(is_slot && !kept);

  // 4 candidates: the detected PRNs that no kept slot holds, ranked by M (equal: the lower index), the k-th to the k-th free slot
  bool tracked = false;
#pragma unroll 1
  for (int j = 0; j < ch; j++) {
    const int v = __shfl(slot_prn, j, 64);
    tracked = tracked || (((kept_mask >> j) & 1ull) != 0 && v == my_prn);
  }
  tracked = tracked && detected;
  const bool cand = detected && !tracked;
  const u64 cand_mask = __ballot(cand);
  int rank = 0;
#pragma unroll 1
  for (int q = 0; q < n_prn; q++) {
    const u32 mq = (u32)__shfl((int)M, q, 64);
    rank += (((cand_mask >> q) & 1ull) != 0 && (mq > M || (mq == M && q < lane))) ? 1 : 0;
  }
  const int n_free = __popcll(free_before);
  const bool assigned = cand && rank < n_free;
  const bool dropped = cand && !assigned;
  int slot = -1;
  if (assigned) {                        // the rank-th set bit of free_before (no cross-lane operation in here)
    u64 m = free_before;
    for (int i = 0; i < rank; i++)
      m &= m - 1ull;
    slot = __ffsll((long long)m) - 1;
  }
  const u64 assigned_mask = __ballot(is_slot && ((free_before >> lane) & 1ull) != 0 && __popcll(free_before & below(lane)) < __popcll(cand_mask));
  const u64 tracked_mask = __ballot(tracked), detected_mask = __ballot(detected), dropped_mask = __ballot(dropped);

  // 5 the hand-over's floats, in the candidate's lane
  const float f = (float)dopp_hz;
  float phase = (float)tau;
  if (cfg.code_per_hz != 0.0f && cfg.lead_blocks != 0) {
    const float per_s = cfg.code_per_hz * f;
    const float span_s = (float)cfg.lead_blocks * 0.001f;
    const float step = per_s * span_s;
    phase = phase - step;
    if (phase < 0.0f)
      phase = phase + 16368.0f;
    else if (phase >= 16368.0f)
      phase = phase - 16368.0f;
  }

  // ... and the states of every slot that is handed over or evicted, the wave together
  u64 todo = assigned_mask | evicted_mask;      // (wave-uniform: ballots)
#pragma unroll 1
  while (todo != 0) {
    const int j = __ffsll((long long)todo) - 1;
    todo &= todo - 1ull;
    const u64 from = __ballot(assigned && slot == j);       // the candidate that goes there: one lane, or none
    const int src = from != 0 ? __ffsll((long long)from) - 1 : 0;
    const int h_prn = __shfl(my_prn, src, 64);
    const u32 h_phase = (u32)__shfl((int)__float_as_uint(phase), src, 64);
    const u32 h_freq = (u32)__shfl((int)__float_as_uint(f), src, 64);
    const u64 w0 = from != 0 ? ((u64)h_phase << 32) | (u64)(u32)h_prn : (u64)(u32)GPSX_PRN_NONE;
    const u64 w1 = from != 0 ? (u64)h_freq : 0ull;          // (if_freq_accum, the high half: 0)
    const size_t c = ch0 + (size_t)j;
    if (lane < kSyncWords)
      reinterpret_cast<u64 *>(sync + c)[lane] = lane == 0 ? w0 : lane == 1 ? w1 : 0ull;
    u64 *dst = nullptr;
    if (lane < kLockWords)
      dst = lock ? reinterpret_cast<u64 *>(lock + c) + lane : nullptr;
    else if (lane < kLockWords + kNavWords)
      dst = nav ? reinterpret_cast<u64 *>(nav + c) + (lane - kLockWords) : nullptr;
    else if (lane < kLockWords + kNavWords + kObsWords)
      dst = obs ? reinterpret_cast<u64 *>(obs + c) + (lane - kLockWords - kNavWords) : nullptr;
    else if (lane < kLockWords + kNavWords + kObsWords + kEphWords)
      dst = eph ? reinterpret_cast<u64 *>(eph + c) + (lane - kLockWords - kNavWords - kObsWords) : nullptr;
    if (dst)
      *dst = 0ull;
  }

  // 6 the records
  if (det && is_prn) {
    const u32 fl = (detected ? GPSX_WACQ_DET_DETECTED : 0u) | (tracked ? GPSX_WACQ_DET_TRACKED : 0u) |
                   (assigned ? GPSX_WACQ_DET_ASSIGNED : 0u) | (dropped ? GPSX_WACQ_DET_DROPPED : 0u);
    const Quad o = {M, tau, (u32)dopp_hz, fl | (((u32)slot & 0xFFu) << 8)};
    *reinterpret_cast<Quad *>(det + ((size_t)r * (size_t)n_prn + (size_t)lane)) = o;
  }
  if (lane == 0) {
    const u32 n_assigned = (u32)__popcll(assigned_mask), n_evicted = (u32)__popcll(evicted_mask), n_dropped = (u32)__popcll(dropped_mask);
    gpsx_wacq_t a;
    a.flags = (n_assigned ? GPSX_WACQ_ASSIGNED : 0u) | (n_evicted ? GPSX_WACQ_EVICTED : 0u) | (n_dropped ? GPSX_WACQ_FULL : 0u);
    a.n_detected = (u32)__popcll(detected_mask);
    a.n_tracked = (u32)__popcll(tracked_mask);
    a.n_assigned = n_assigned;
    a.n_evicted = n_evicted;
    a.n_dropped = n_dropped;
    a.assigned_mask = assigned_mask;
    a.evicted_mask = evicted_mask;
    a.kept_mask = kept_mask;
    a.free_mask = free_before & ~assigned_mask;
    a.reserved[0] = a.reserved[1] = 0u;
    acq[r] = a;
  }
}

void launch_wacq(hipStream_t s, const gpsx_wacq_cfg_t &cfg, int n_rx, int n_prn, const uint8_t *prns, int dopp_min_hz, int dopp_step_hz, int n_dopp,
                 const gpsx_peak_t *d_peaks, gpsx_wsync_state_t *d_sync_st, gpsx_wlock_state_t *d_lock_st, gpsx_wnav_state_t *d_nav_st,
                 gpsx_wobs_state_t *d_obs_st, gpsx_weph_state_t *d_eph_st, gpsx_wacq_t *d_acq, gpsx_wacq_det_t *d_det)
{
  // (no checks of its own: gpsx_api_wtrack.hip's wacq() is the one list of what a launch needs -- 1 .. 2^20 receivers and bins, 1 .. 64
  //  PRNs and slots, lock states where slots can be evicted -- and refuses with a text before it comes here)
  WacqPrns list = {};
  for (int p = 0; p < n_prn; p++)
    list.w[p >> 3] |= (u64)prns[p] << ((p & 7) * 8);
  hipLaunchKernelGGL(k_wacq, dim3(((unsigned)n_rx + 3u) / 4u), dim3(256), 0, s, cfg, n_rx, n_prn, n_dopp, dopp_min_hz, dopp_step_hz, list, d_peaks,
                     d_sync_st, d_lock_st, d_nav_st, d_obs_st, d_eph_st, d_acq, d_det);
}

}  // namespace gpsx
