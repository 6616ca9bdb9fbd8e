// k_wbank.hip -- EXTENSION, not in the reference: the ephemeris bank, the stage behind gpsx_weph that keeps every receiver's newest
// VALID ephemeris per listed PRN across slot changes and merges it into the launch's records (include/gpsx.h gpsx_wbank; DESIGN.md
// 4.6.14).
//
// One wave per receiver, four receivers per 256-thread workgroup; no LDS, no barrier, no scratch.  The wave works on two small sets,
// a slot per lane and a PRN index per lane: a slot's index in the list is a loop of shuffles over the list, an index's winning offer
// a loop of shuffles over the slots, what was stored and what the bank holds are ballots.  Every ballot and shuffle runs under
// wave-uniform control flow (a wave whose receiver does not exist leaves as a whole; the loops around them have wave-uniform bounds;
// lane-dependent conditions are selects).  What decides the time is moving the 256-byte records: half a wave moves one, 8 bytes per
// lane, two records a turn.  No record is read from memory in the call that stored it: a merged record whose bank entry was replaced
// in this call is read from the slot that was stored, so no load depends on another lane's store.
#include <hip/hip_runtime.h>

#include <cstddef>

#include "gpsx_device.hpp"
#include "gpsx_kernels.hpp"

namespace gpsx {

namespace {

static_assert(sizeof(gpsx_wbank_cfg_t) == 16 && offsetof(gpsx_wbank_cfg_t, reserved) == 4, "gpsx_wbank_cfg_t layout");
static_assert(sizeof(gpsx_wbank_t) == 32 && offsetof(gpsx_wbank_t, have_mask) == 8 && offsetof(gpsx_wbank_t, from_bank_mask) == 16 &&
              offsetof(gpsx_wbank_t, n_stored) == 24 && offsetof(gpsx_wbank_t, zero) == 30, "gpsx_wbank_t layout");
static_assert(sizeof(gpsx_weph_t) == 256 && offsetof(gpsx_weph_t, flags) == 0 && offsetof(gpsx_weph_t, toe_time) == 32 && alignof(gpsx_weph_t) == 8,
              "gpsx_weph_t layout: 32 words of 8 bytes, flags in the low half of the first");
static_assert(sizeof(gpsx_wsync_state_t) == 448 && offsetof(gpsx_wsync_state_t, loop) == 0 && offsetof(gpsx_wloop_state_t, prn) == 0,
              "gpsx_wsync_state_t layout");

constexpr int kRecWords = 32;     // 8-byte words of an ephemeris record: half a wave

__device__ __forceinline__ u64 as_stored(u64 word0) { return (word0 & 0xFFFFFFFF00000000ull) | (u64)GPSX_WEPH_VALID; }   // flags = VALID

}  // namespace

// PRN numbers by value, eight per word (n_prn <= 64): lane p's is a select among eight scalars, never an indexed copy
struct WbankPrns { u64 w[8]; };

__global__ __launch_bounds__(256) void k_wbank(int ch, int n_rx, int n_prn, WbankPrns prns, const gpsx_wsync_state_t *__restrict__ sync,
                                               const gpsx_weph_t *eph, gpsx_weph_t *bank, gpsx_weph_t *eph_out, gpsx_wbank_t *__restrict__ rep)
{
  const int lane = (int)threadIdx.x & 63;
  const int r = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
  if (r >= n_rx)          // (the whole wave: r is the same in its 64 lanes)
    return;
  const size_t ch0 = (size_t)r * (size_t)ch, b0 = (size_t)r * (size_t)n_prn;
  const u64 word = lane < 8 ? prns.w[0] : lane < 16 ? prns.w[1] : lane < 24 ? prns.w[2] : lane < 32 ? prns.w[3] :
                   lane < 40 ? prns.w[4] : lane < 48 ? prns.w[5] : lane < 56 ? prns.w[6] : prns.w[7];
  const int my_prn = (int)((word >> ((lane & 7) * 8)) & 0xFFull);

  // 1 offers: lane j is slot j
  const bool is_slot = lane < ch;
  const int slot_prn = is_slot ? sync[ch0 + lane].loop.prn : GPSX_PRN_NONE;
  const gpsx_weph_t *mine = eph + ch0 + (is_slot ? lane : 0);
  const u32 s_flags = mine->flags;
  const long long s_toe = mine->toe_time;
  const bool s_valid = is_slot && (s_flags & GPSX_WEPH_VALID) != 0;
  int idx = -1;
#pragma unroll 1
  for (int q = 0; q < n_prn; q++) {
    const int v = __shfl(my_prn, q, 64);        // (1 .. 210: never GPSX_PRN_NONE)
    idx = is_slot && slot_prn == v ? q : idx;
  }
  const bool offers = s_valid && idx >= 0;

  // 2 store: lane p is PRN index p
  const bool is_prn = lane < n_prn;
  const gpsx_weph_t *held = bank + b0 + (is_prn ? lane : 0);
  const u32 b_flags = held->flags;
  const long long b_toe = held->toe_time;
  const bool b_valid = is_prn && (b_flags & GPSX_WEPH_VALID) != 0;
  int win = -1;
  long long win_toe = 0;
#pragma unroll 1
  for (int j = 0; j < ch; j++) {
    const int o = __shfl(offers ? idx : -1, j, 64);     // (an index is below n_prn: lanes from n_prn on never match)
    const long long t = __shfl(s_toe, j, 64);
    const bool take = o == lane && (win < 0 || t > win_toe);      // (ascending slots, strictly greater: the lowest among equals)
    win = take ? j : win;
    win_toe = take ? t : win_toe;
  }
  const bool store = win >= 0 && (!b_valid || win_toe >= b_toe);
  const u64 stored_mask = __ballot(store), have_mask = __ballot(b_valid || store);

  // 3 merge: lane j again
  const int ixc = idx >= 0 ? idx : 0;
  const int win_of = __shfl(win, ixc, 64);                         // the slot stored for this slot's index, where one was
  const bool stored_p = ((stored_mask >> ixc) & 1ull) != 0;
  const bool from_bank = is_slot && !s_valid && idx >= 0 && ((have_mask >> ixc) & 1ull) != 0;
  const u64 from_bank_mask = __ballot(from_bank);

  // ... the records, two a turn: lanes 0 .. 31 the first, lanes 32 .. 63 the second, word w each
  const int half = lane / kRecWords, w = lane % kRecWords;
  u64 todo = stored_mask;                                          // (wave-uniform: a ballot)
#pragma unroll 1
  while (todo != 0) {
    const int p0 = __ffsll((long long)todo) - 1;
    todo &= todo - 1ull;
    const bool two = todo != 0;
    const int p1 = two ? __ffsll((long long)todo) - 1 : p0;
    todo &= todo - 1ull;
    const int p = half ? p1 : p0;
    const int s = __shfl(win, p, 64);                              // (stored: a slot of this receiver)
    if (half == 0 || two) {
      const u64 v = reinterpret_cast<const u64 *>(eph + ch0 + (size_t)s)[w];
      reinterpret_cast<u64 *>(bank + b0 + (size_t)p)[w] = w == 0 ? as_stored(v) : v;
    }
  }
  if (eph_out) {
    // (in place only the records that come from the bank change; they are never a slot that was stored: that one has VALID)
    todo = eph_out == eph ? from_bank_mask : (ch == 64 ? ~0ull : (1ull << ch) - 1ull);
#pragma unroll 1
    while (todo != 0) {
      const int j0 = __ffsll((long long)todo) - 1;
      todo &= todo - 1ull;
      const bool two = todo != 0;
      const int j1 = two ? __ffsll((long long)todo) - 1 : j0;
      todo &= todo - 1ull;
      const int j = half ? j1 : j0;
      const bool fb = ((from_bank_mask >> j) & 1ull) != 0;
      const bool st = __shfl(stored_p ? 1 : 0, j, 64) != 0;
      const int ix = __shfl(ixc, j, 64), wn = __shfl(win_of, j, 64);
      if (half == 0 || two) {
        const gpsx_weph_t *src = fb ? (st ? eph + ch0 + (size_t)(wn >= 0 ? wn : 0) : bank + b0 + (size_t)ix) : eph + ch0 + (size_t)j;
        const u64 v = reinterpret_cast<const u64 *>(src)[w];
        reinterpret_cast<u64 *>(eph_out + ch0 + (size_t)j)[w] = fb && st && w == 0 ? as_stored(v) : v;
      }
    }
  }

  // 4 the report
  if (lane == 0) {
    gpsx_wbank_t o;
    o.stored_mask = stored_mask;
    o.have_mask = have_mask;
    o.from_bank_mask = from_bank_mask;
    o.n_stored = (uint16_t)__popcll(stored_mask);
    o.n_have = (uint16_t)__popcll(have_mask);
    o.n_from_bank = (uint16_t)__popcll(from_bank_mask);
    o.zero = 0;
    rep[r] = o;
  }
}

void launch_wbank(hipStream_t s, const gpsx_wbank_cfg_t &cfg, int n_rx, int n_prn, const uint8_t *prns, const gpsx_wsync_state_t *d_sync_st,
                  const gpsx_weph_t *d_eph, gpsx_weph_t *d_bank, gpsx_weph_t *d_eph_out, gpsx_wbank_t *d_rep)
{
  // (no checks of its own: gpsx_api_wtrack.hip's wbank() is the one list of what a launch needs and refuses with a text before it comes here)
  WbankPrns list = {};
  for (int p = 0; p < n_prn; p++)
    list.w[p >> 3] |= (u64)prns[p] << ((p & 7) * 8);
  hipLaunchKernelGGL(k_wbank, dim3(((unsigned)n_rx + 3u) / 4u), dim3(256), 0, s, cfg.ch_per_rx, n_rx, n_prn, list, d_sync_st, d_eph, d_bank, d_eph_out,
                     d_rep);
}

}  // namespace gpsx
