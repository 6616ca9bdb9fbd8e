// k_wtow.hip -- EXTENSION, not in the reference: time-of-week aiding of the observables, the stage behind gpsx_wobs and gpsx_wpred that
// anchors a running bit chain's time of week from the prediction's transmit millisecond before a HOW has done it, and resolves
// GPSX_WOBS_AMBIGUOUS where the prediction names the other edge block (include/gpsx.h gpsx_wtow).
//
// k_wacq's geometry: one wave per receiver, four receivers per 256-thread workgroup, lane j is slot j; no LDS, no barrier, no scratch.
// A slot's index in the list is a wave-uniform loop of shuffles over the list, the receiver's masks are ballots; every ballot and
// shuffle runs under wave-uniform control flow (a wave whose receiver does not exist or has no prediction leaves as a whole; lane-
// dependent conditions are selects, and the few stores they guard contain no cross-lane operation).  The stage moves a few words per
// slot: the 80-byte state comes in as five 16-byte loads, the prediction's record as three, and only the words that change go back.
// Step 3 is three double operations; everything else is integer.  Absolute block counts go up to 2^62 and Z down to -2^62: they are
// taken modulo the week before they are subtracted, which is all the definition needs of them.
#include <hip/hip_runtime.h>

#include <cstddef>

#include "gpsx_device.hpp"
#include "gpsx_kernels.hpp"

namespace gpsx {

namespace {

static_assert(sizeof(gpsx_wtow_cfg_t) == 32 && offsetof(gpsx_wtow_cfg_t, max_sigma_m) == 0 && offsetof(gpsx_wtow_cfg_t, max_resid_samples) == 8 &&
              offsetof(gpsx_wtow_cfg_t, ch_per_rx) == 12 && offsetof(gpsx_wtow_cfg_t, max_age_blocks) == 16 && offsetof(gpsx_wtow_cfg_t, resolve) == 20 &&
              offsetof(gpsx_wtow_cfg_t, rearm) == 24 && offsetof(gpsx_wtow_cfg_t, reserved) == 28, "gpsx_wtow_cfg_t layout");
static_assert(sizeof(gpsx_wtow_t) == 32 && offsetof(gpsx_wtow_t, flags) == 0 && offsetof(gpsx_wtow_t, prn_index) == 4 && offsetof(gpsx_wtow_t, tx_ms) == 8 &&
              offsetof(gpsx_wtow_t, resid) == 16 && offsetof(gpsx_wtow_t, m) == 20 && offsetof(gpsx_wtow_t, shift) == 24 && offsetof(gpsx_wtow_t, zero) == 28,
              "gpsx_wtow_t layout");
static_assert(sizeof(gpsx_wtow_rx_t) == 64 && offsetof(gpsx_wtow_rx_t, flags) == 0 && offsetof(gpsx_wtow_rx_t, n_aided) == 2 &&
              offsetof(gpsx_wtow_rx_t, n_inconsistent) == 7 && offsetof(gpsx_wtow_rx_t, aided_mask) == 8 && offsetof(gpsx_wtow_rx_t, inconsistent_mask) == 48 &&
              offsetof(gpsx_wtow_rx_t, valid_after_mask) == 56, "gpsx_wtow_rx_t layout");
static_assert(sizeof(gpsx_wobs_state_t) == 80 && offsetof(gpsx_wobs_state_t, blocks_seen) == 0 && offsetof(gpsx_wobs_state_t, last_bit_end_p1) == 8 &&
              offsetof(gpsx_wobs_state_t, chain_first_p1) == 16 && offsetof(gpsx_wobs_state_t, edge_block) == 24 &&
              offsetof(gpsx_wobs_state_t, tx_ms_at_edge) == 32 && offsetof(gpsx_wobs_state_t, last_win_end_p1) == 40 &&
              offsetof(gpsx_wobs_state_t, last_phase) == 48 && offsetof(gpsx_wobs_state_t, flags) == 56 && offsetof(gpsx_wobs_state_t, reserved) == 76,
              "gpsx_wobs_state_t layout: five 16-byte words");
static_assert(sizeof(gpsx_wobs_t) == 32 && offsetof(gpsx_wobs_t, tx_ms) == 0 && offsetof(gpsx_wobs_t, flags) == 16, "gpsx_wobs_t layout");
static_assert(sizeof(gpsx_wpred_t) == 64 && offsetof(gpsx_wpred_t, flags) == 0 && offsetof(gpsx_wpred_t, tx_ms) == 8 && offsetof(gpsx_wpred_t, code_phase) == 24 &&
              offsetof(gpsx_wpred_t, sigma_m) == 56 && sizeof(gpsx_wpred_rx_t) == 64 && offsetof(gpsx_wpred_rx_t, flags) == 0, "gpsx_wpred_t layout");
static_assert(sizeof(gpsx_wsync_state_t) == 448 && offsetof(gpsx_wsync_state_t, loop) == 0 && offsetof(gpsx_wloop_state_t, prn) == 0 &&
              offsetof(gpsx_wsync_state_t, mode) == 72 && offsetof(gpsx_wsync_state_t, search_n) == 84 && offsetof(gpsx_wsync_state_t, prev_best_p1) == 88,
              "gpsx_wsync_state_t layout");

constexpr long long kMaxCount = 1ll << 62;     // k_wobs' bounds of a state
constexpr long long kWeekMs = 604800000ll;
constexpr u32 kStateFlags = GPSX_WOBS_PHASE | GPSX_WOBS_EDGE | GPSX_WOBS_TOW | GPSX_WOBS_CONFIRMED | GPSX_WOBS_AMBIGUOUS;

struct alignas(16) Quad { u32 a, b, c, d; };   // 16 bytes at a 16-byte aligned address: one global_load_dwordx4

__device__ __forceinline__ long long pair(u32 lo, u32 hi) { return (long long)(((u64)hi << 32) | (u64)lo); }
__device__ __forceinline__ long long week_pos(long long x) { const long long r = x % kWeekMs; return r < 0 ? r + kWeekMs : r; }
// x in (-W, 2 W) folded into 0 .. W - 1
__device__ __forceinline__ long long week_fold(long long x) { return x < 0 ? x + kWeekMs : (x >= kWeekMs ? x - kWeekMs : x); }

}  // namespace

// PRN numbers by value, eight per word (n_prn <= 64): lane p's is a select among eight scalars, never an indexed copy
struct WtowPrns { u64 w[8]; };

__global__ __launch_bounds__(256) void k_wtow(gpsx_wtow_cfg_t cfg, int n_rx, int n_prn, WtowPrns prns, const gpsx_wpred_rx_t *__restrict__ pred_rx,
                                              const gpsx_wpred_t *__restrict__ pred, gpsx_wsync_state_t *sync, gpsx_wobs_state_t *st, gpsx_wobs_t *obs,
                                              gpsx_wtow_t *__restrict__ tow, gpsx_wtow_rx_t *__restrict__ tow_rx)
{
  const int lane = (int)threadIdx.x & 63;
  const int r = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
  if (r >= n_rx)          // (the whole wave: r is the same in its 64 lanes)
    return;
  const int ch = cfg.ch_per_rx;
  const bool is_slot = lane < ch;
  const size_t ch0 = (size_t)r * (size_t)ch;

  // 0 receiver (the whole wave again: one record, the same in its 64 lanes)
  if ((pred_rx[r].flags & GPSX_WPRED_RX_PREDICTED) == 0) {
    if (is_slot) {
      gpsx_wtow_t o = {};
      o.flags = GPSX_WTOW_NO_PRED;
      tow[ch0 + lane] = o;
    }
    if (lane == 0) {
      gpsx_wtow_rx_t o = {};
      o.flags = GPSX_WTOW_RX_NO_PRED;
      tow_rx[r] = o;
    }
    return;
  }

  // 1 slot: lane j is slot j; the state in five words, whatever becomes of the slot (an idle lane reads slot 0's)
  const size_t at = ch0 + (is_slot ? lane : 0);
  const int slot_prn = is_slot ? sync[at].loop.prn : GPSX_PRN_NONE;
  const Quad *sq = reinterpret_cast<const Quad *>(st + at);
  const Quad q0 = sq[0], q1 = sq[1], q2 = sq[2], q3 = sq[3], q4 = sq[4];
  const u64 word = lane < 8 ? prns.w[0] : lane < 16 ? prns.w[1] : lane < 24 ? prns.w[2] : lane < 32 ? prns.w[3] :
                   lane < 40 ? prns.w[4] : lane < 48 ? prns.w[5] : lane < 56 ? prns.w[6] : prns.w[7];
  const int my_prn = (int)((word >> ((lane & 7) * 8)) & 0xFFull);
  int idx = -1;
#pragma unroll 1
  for (int q = 0; q < n_prn; q++) {
    const int v = __shfl(my_prn, q, 64);        // (1 .. 210: never GPSX_PRN_NONE)
    idx = is_slot && slot_prn == v ? q : idx;
  }
  const long long B = pair(q0.a, q0.b), last_bit_p1 = pair(q0.c, q0.d), first_p1 = pair(q1.a, q1.b), Z = pair(q1.c, q1.d);
  const long long Tz = pair(q2.a, q2.b), last_win_p1 = pair(q2.c, q2.d);
  const float last_phase = __uint_as_float(q3.a);
  const u32 s_flags = q3.c;
  const bool good = (s_flags & ~kStateFlags) == 0 && q4.d == 0 && (u64)B <= (u64)kMaxCount && (u64)last_bit_p1 <= (u64)kMaxCount &&
                    (u64)first_p1 <= (u64)kMaxCount && (u64)last_win_p1 <= (u64)kMaxCount && Z >= -kMaxCount && Z <= kMaxCount &&
                    (u64)Tz < (u64)kWeekMs && (!(s_flags & GPSX_WOBS_PHASE) || (last_phase >= 0.0f && last_phase < 16368.0f));
  const bool empty = !is_slot || slot_prn == GPSX_PRN_NONE;
  const bool unlisted = !empty && idx < 0;
  const bool listed = !empty && idx >= 0;
  const bool bad = listed && !good;
  const bool chain = (s_flags & (GPSX_WOBS_PHASE | GPSX_WOBS_EDGE)) == (GPSX_WOBS_PHASE | GPSX_WOBS_EDGE);
  const bool waiting = listed && good && !chain;
  const bool stale = listed && good && chain && (long long)((u64)B - (u64)last_win_p1) > (long long)cfg.max_age_blocks;   // (good: both within 0 .. 2^62)
  const bool live = listed && good && chain && !stale;

  // 2 prediction: the slot's PRN's record (an idle or unlisted lane reads index 0's)
  const gpsx_wpred_t *w = pred + (size_t)r * (size_t)n_prn + (size_t)(idx >= 0 ? idx : 0);
  const Quad w0 = *reinterpret_cast<const Quad *>(w);
  const double w_phase = w->code_phase;
  const float w_sigma = w->sigma_m;
  const bool uncertain = live && ((w0.a & GPSX_WPRED_PREDICTED) == 0 || (double)w_sigma > cfg.max_sigma_m);
  const bool known = live && !uncertain;

  // 3 millisecond
  const double d = (double)last_phase - w_phase;
  const int k = d > 8184.0 ? 1 : (d < -8184.0 ? -1 : 0);
  const double rho = d - (k > 0 ? 16368.0 : (k < 0 ? -16368.0 : 0.0));      // (16368 k: a select, not a product)
  const bool fits = __builtin_fabs(rho) <= (double)cfg.max_resid_samples;   // (a NaN fails it)
  const bool inconsistent = known && !fits;
  const bool timed = known && fits;
  const long long tx = week_fold(week_pos(pair(w0.c, w0.d)) + k);
  const long long span = week_pos(B) - week_pos(Z);            // (-W, W)
  const long long tz1 = week_fold(tx - span);
  const int m = (int)(tz1 % 20);

  // 4 grid
  const bool may_shift = (s_flags & GPSX_WOBS_AMBIGUOUS) != 0 && cfg.resolve != 0;
  const int s = may_shift && m == 1 ? -1 : (may_shift && m == 19 ? 1 : 0);
  const bool on_grid = timed && (m == 0 || s != 0);
  const bool off_grid = timed && !on_grid;
  const bool shifted = on_grid && s != 0;
  const long long z_new = (long long)((u64)Z + (u64)(long long)s), tz_new = week_fold(tz1 + s);   // (good: |Z| <= 2^62)
  bool rearmed = false;
  if (cfg.rearm != 0) {       // (uniform over the launch)
    gpsx_wsync_state_t *y = sync + at;
    rearmed = off_grid && y->mode != GPSX_WSYNC_SEARCH;
    if (rearmed) {
      y->mode = GPSX_WSYNC_SEARCH;
      y->search_n = 0;
      y->prev_best_p1 = 0;
    }
  }

  // 5 anchor
  const bool has_tow = (s_flags & GPSX_WOBS_TOW) != 0;
  const bool aided = on_grid && !has_tow;
  const bool agrees = on_grid && has_tow && Tz == tz_new;
  const bool disagrees = on_grid && has_tow && Tz != tz_new;
  const bool settle = cfg.resolve != 0 && (aided || agrees);
  const u32 n_flags = (aided ? s_flags | GPSX_WOBS_TOW : s_flags) & (settle ? ~GPSX_WOBS_AMBIGUOUS : ~0u);
  const bool changed = aided || n_flags != s_flags;           // (a shift needs AMBIGUOUS, and clears it)
  gpsx_wobs_state_t *mine = st + at;
  if (settle && s != 0)
    mine->edge_block = z_new;
  if (aided)
    mine->tx_ms_at_edge = tz_new;
  if (changed)
    mine->flags = n_flags;

  // 6 observable: gpsx_wobs' output clause on the new state (PHASE, EDGE and TOW hold)
  if (obs && changed) {
    const long long tz = aided ? tz_new : Tz, z = settle ? z_new : Z;
    gpsx_wobs_t *o = obs + at;
    o->tx_ms = week_fold(tz + (week_pos(B) - week_pos(z)));
    o->flags = n_flags | GPSX_WOBS_VALID;
  }

  // 7 records
  const bool counted = listed && good;
  const u32 after = changed ? n_flags : s_flags;
  constexpr u32 need = GPSX_WOBS_PHASE | GPSX_WOBS_EDGE | GPSX_WOBS_TOW;
  const u64 aided_mask = __ballot(aided), agrees_mask = __ballot(agrees), disagrees_mask = __ballot(disagrees), off_grid_mask = __ballot(off_grid);
  const u64 shifted_mask = __ballot(shifted), inconsistent_mask = __ballot(inconsistent), rearmed_mask = __ballot(rearmed);
  const u64 valid_after_mask = __ballot(counted && (after & need) == need);
  if (is_slot) {
    gpsx_wtow_t o;
    o.flags = (empty ? GPSX_WTOW_EMPTY : 0u) | (unlisted ? GPSX_WTOW_UNLISTED : 0u) | (bad ? GPSX_WTOW_BAD : 0u) | (waiting ? GPSX_WTOW_WAITING : 0u) |
              (stale ? GPSX_WTOW_STALE : 0u) | (uncertain ? GPSX_WTOW_UNCERTAIN : 0u) | (inconsistent ? GPSX_WTOW_INCONSISTENT : 0u) |
              (off_grid ? GPSX_WTOW_OFF_GRID : 0u) | (rearmed ? GPSX_WTOW_REARMED : 0u) | (shifted ? GPSX_WTOW_SHIFTED : 0u) |
              (aided ? GPSX_WTOW_AIDED : 0u) | (agrees ? GPSX_WTOW_AGREES : 0u) | (disagrees ? GPSX_WTOW_DISAGREES : 0u);
    o.prn_index = idx;
    o.tx_ms = timed ? tx : 0;
    const float resid = (float)rho;
    o.resid = known ? (resid != resid ? __uint_as_float(0x7FC00000u) : resid) : 0.0f;
    o.m = timed ? m : -1;
    o.shift = shifted ? s : 0;
    o.zero = 0;
    tow[ch0 + lane] = o;
  }
  if (lane == 0) {
    gpsx_wtow_rx_t o;
    o.flags = (uint16_t)((aided_mask ? GPSX_WTOW_RX_AIDED : 0u) | (shifted_mask ? GPSX_WTOW_RX_SHIFTED : 0u) | (disagrees_mask ? GPSX_WTOW_RX_DISAGREES : 0u) |
                         (off_grid_mask ? GPSX_WTOW_RX_OFF_GRID : 0u) | (rearmed_mask ? GPSX_WTOW_RX_REARMED : 0u));
    o.n_aided = (uint8_t)__popcll(aided_mask);
    o.n_agrees = (uint8_t)__popcll(agrees_mask);
    o.n_disagrees = (uint8_t)__popcll(disagrees_mask);
    o.n_off_grid = (uint8_t)__popcll(off_grid_mask);
    o.n_shifted = (uint8_t)__popcll(shifted_mask);
    o.n_inconsistent = (uint8_t)__popcll(inconsistent_mask);
    o.aided_mask = aided_mask;
    o.agrees_mask = agrees_mask;
    o.disagrees_mask = disagrees_mask;
    o.off_grid_mask = off_grid_mask;
    o.shifted_mask = shifted_mask;
    o.inconsistent_mask = inconsistent_mask;
    o.valid_after_mask = valid_after_mask;
    tow_rx[r] = o;
  }
}

void launch_wtow(hipStream_t s, const gpsx_wtow_cfg_t &cfg, int n_rx, int n_prn, const uint8_t *prns, const gpsx_wpred_rx_t *d_pred_rx,
                 const gpsx_wpred_t *d_pred, gpsx_wsync_state_t *d_sync_st, gpsx_wobs_state_t *d_obs_st, gpsx_wobs_t *d_obs, gpsx_wtow_t *d_tow,
                 gpsx_wtow_rx_t *d_tow_rx)
{
  // (no checks of its own: gpsx_api_wtrack.hip's wtow() is the one list of what a launch needs and refuses with a text before it comes here)
  WtowPrns list = {};
  for (int p = 0; p < n_prn; p++)
    list.w[p >> 3] |= (u64)prns[p] << ((p & 7) * 8);
  hipLaunchKernelGGL(k_wtow, dim3(((unsigned)n_rx + 3u) / 4u), dim3(256), 0, s, cfg, n_rx, n_prn, list, d_pred_rx, d_pred, d_sync_st, d_obs_st, d_obs, d_tow,
                     d_tow_rx);
}

}  // namespace gpsx
