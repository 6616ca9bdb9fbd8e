// k_wlock.hip -- EXTENSION, not in the reference: every channel's code-lock, carrier-lock and C/N0 indicators from the window records
// of the weighted loop with bit sync, with the re-arm of its bit search (include/gpsx.h gpsx_wlock).
//
// k_wobs' shape, since it is the same problem: one channel per lane, a serial recurrence over the channel's records, and what
// decides the time is the read of d_rec.  A lane needs 32 of a record's 48 bytes: iq[6] at offset 0 (16 + 8 bytes) and end_block /
// flags at offset 36 (4-byte aligned) -- three loads per slot, eight registers, loaded kAhead slots before the recurrence needs
// them in two register sets that take turns (2 x 4 x 8 = 64 registers, as k_wobs' 2 x 8 x 4).  The five epoch sums are int64 in
// registers; the three ratios of an epoch's end are plain divisions, correctly rounded and uncontracted by this object's flags
// (csrc/Makefile), as the loop kernels' are.  No LDS.  The sync states are touched by the lanes whose channel has a re-arm pending,
// at the very end: one word read, eleven written.
#include <hip/hip_runtime.h>

#include <cstddef>

#include "gpsx_device.hpp"
#include "gpsx_kernels.hpp"
#include "gpsx_wstage_parts.hpp"

namespace gpsx {

namespace {

static_assert(sizeof(gpsx_wlock_cfg_t) == 40 && offsetof(gpsx_wlock_cfg_t, code_min) == 8 && offsetof(gpsx_wlock_cfg_t, n_good) == 20 &&
              offsetof(gpsx_wlock_cfg_t, rearm) == 28 && offsetof(gpsx_wlock_cfg_t, reserved) == 36, "gpsx_wlock_cfg_t layout");
static_assert(sizeof(gpsx_wlock_state_t) == 128 && offsetof(gpsx_wlock_state_t, blocks_seen) == 0 && offsetof(gpsx_wlock_state_t, last_epoch_end_p1) == 8 &&
              offsetof(gpsx_wlock_state_t, sum_a) == 16 && offsetof(gpsx_wlock_state_t, sum_l) == 48 && offsetof(gpsx_wlock_state_t, last_p) == 56 &&
              offsetof(gpsx_wlock_state_t, last_code_ratio) == 64 && offsetof(gpsx_wlock_state_t, last_snr) == 72 &&
              offsetof(gpsx_wlock_state_t, epoch_n) == 76 && offsetof(gpsx_wlock_state_t, flags) == 80 && offsetof(gpsx_wlock_state_t, last_k) == 84 &&
              offsetof(gpsx_wlock_state_t, code_good) == 88 && offsetof(gpsx_wlock_state_t, car_bad) == 100 &&
              offsetof(gpsx_wlock_state_t, false_run) == 104 && offsetof(gpsx_wlock_state_t, n_lost_code) == 108 &&
              offsetof(gpsx_wlock_state_t, n_range) == 120 && offsetof(gpsx_wlock_state_t, reserved) == 124, "gpsx_wlock_state_t layout");
static_assert(sizeof(gpsx_wlock_t) == 64 && offsetof(gpsx_wlock_t, flags) == 0 && offsetof(gpsx_wlock_t, n_epochs) == 4 && offsetof(gpsx_wlock_t, last_k) == 8 &&
              offsetof(gpsx_wlock_t, age_blocks) == 12 && offsetof(gpsx_wlock_t, code_ratio) == 16 && offsetof(gpsx_wlock_t, snr) == 24 &&
              offsetof(gpsx_wlock_t, n_range) == 28 && offsetof(gpsx_wlock_t, p) == 32 && offsetof(gpsx_wlock_t, n_lost_code) == 40 &&
              offsetof(gpsx_wlock_t, n_rearm) == 48 && offsetof(gpsx_wlock_t, reserved) == 52, "gpsx_wlock_t layout");
static_assert(sizeof(gpsx_wsync_state_t) == 448 && offsetof(gpsx_wsync_state_t, loop) == 0 && offsetof(gpsx_wloop_state_t, n_updates) == 32 &&
              offsetof(gpsx_wsync_state_t, win_iq) == 40 && offsetof(gpsx_wsync_state_t, win_n) == 64 && offsetof(gpsx_wsync_state_t, mode) == 72 &&
              offsetof(gpsx_wsync_state_t, bit_ip) == 80 && offsetof(gpsx_wsync_state_t, search_n) == 84 &&
              offsetof(gpsx_wsync_state_t, prev_best_p1) == 88, "gpsx_wsync_state_t layout");

constexpr int kAhead = 4;                    // slots a lane's loads run ahead of its recurrence
constexpr long long kMaxCount = 1ll << 62;
constexpr long long kMaxSum = 1ll << 51;     // a state's P, E, L, |D|
constexpr long long kMaxA = 1ll << 30;       // a state's A
constexpr u32 kRange = 1u << 20;             // a sum of this magnitude is not accumulated
constexpr u32 kStateFlags = GPSX_WLOCK_CODE | GPSX_WLOCK_CARRIER | GPSX_WLOCK_PENDING | GPSX_WLOCK_OPEN_LOCKED | GPSX_WLOCK_EPOCH_LOCKED;
constexpr u32 kOutFlags = GPSX_WLOCK_CODE | GPSX_WLOCK_CARRIER | GPSX_WLOCK_EPOCH_LOCKED;

struct alignas(4) Quad { int a, b, c, d; };  // words at a dword-aligned address: one global_load_dwordx4 / _dwordx2
struct alignas(4) Pair { int a, b; };
struct Win { int ie, qe, ip, qp, il, ql, end_block; u32 flags; };   // what a window is here

__device__ __forceinline__ u32 mag(int v) { return v < 0 ? 0u - (u32)v : (u32)v; }
__device__ __forceinline__ long long sq(int v) { return (long long)v * (long long)v; }
__device__ __forceinline__ u32 run_up(u32 n) { return n < 255u ? n + 1u : 255u; }
// one verdict on an indicator's two runs and its flag, in selects (no branch: the two indicators' steps stay two sets of registers)
// -> the flag was cleared
__device__ __forceinline__ bool verdict(bool good, u32 &good_run, u32 &bad_run, u32 &flags, u32 bit, u32 n_good, u32 n_bad)
{
  good_run = good ? run_up(good_run) : 0u;
  bad_run = good ? 0u : run_up(bad_run);
  const bool set = good && good_run >= n_good, lost = !good && (flags & bit) != 0 && bad_run >= n_bad;
  flags = set ? flags | bit : (lost ? flags & ~bit : flags);
  return lost;
}

}  // namespace

__global__ __launch_bounds__(64) void k_wlock(const gpsx_wsync_rec_t *__restrict__ rec, int n_slots, int n_blocks, gpsx_wlock_cfg_t cfg,
                                              gpsx_wlock_state_t *__restrict__ st, gpsx_wsync_state_t *__restrict__ sync, int n_ch,
                                              gpsx_wlock_t *__restrict__ lock, u32 *__restrict__ bad_state)
{
  const int lane = threadIdx.x;
  const int ch0 = (int)blockIdx.x * 64;
  const bool active = lane < n_ch - ch0;
  const int ch = active ? ch0 + lane : n_ch - 1;   // (always a channel below n_ch: the idle lanes of the last wave load, nothing else)
  const gpsx_wlock_state_t s0 = st[ch];
  const bool valid = (s0.flags & ~kStateFlags) == 0 && s0.reserved == 0 && (u64)s0.blocks_seen <= (u64)kMaxCount &&
                     (u64)s0.last_epoch_end_p1 <= (u64)kMaxCount && s0.epoch_n <= 1023u && s0.last_k <= 1024u && s0.code_good <= 255u &&
                     s0.code_bad <= 255u && s0.car_good <= 255u && s0.car_bad <= 255u && (u64)s0.sum_a <= (u64)kMaxA &&
                     (u64)s0.sum_p <= (u64)kMaxSum && (u64)s0.sum_e <= (u64)kMaxSum && (u64)s0.sum_l <= (u64)kMaxSum &&
                     s0.sum_d >= -kMaxSum && s0.sum_d <= kMaxSum;
  if (active && !valid && bad_state)
    *bad_state = 1u;
  const bool run = active && valid;

  // the state in registers; the newest epoch's end is kept launch-relative, as end_block + 1 (-1: it is an earlier launch's)
  long long A = s0.sum_a, P = s0.sum_p, D = s0.sum_d, E = s0.sum_e, L = s0.sum_l, last_p = s0.last_p;
  float code_ratio = s0.last_code_ratio, car_ratio = s0.last_car_ratio, snr = s0.last_snr;
  u32 epoch_n = s0.epoch_n, flags = s0.flags, last_k = s0.last_k;
  u32 code_good = s0.code_good, code_bad = s0.code_bad, car_good = s0.car_good, car_bad = s0.car_bad, false_run = s0.false_run;
  u32 n_lost_code = s0.n_lost_code, n_lost_carrier = s0.n_lost_carrier, n_rearm = s0.n_rearm, n_range = s0.n_range;
  u32 events = 0, n_epochs = 0;
  int last_end = -1;

  auto step = [&](const Win &w) {
    if (!(run && (w.flags & GPSX_WSYNC_WINDOW) && (u32)w.end_block < (u32)n_blocks))
      return;
    // 1 range
    if ((mag(w.ie) | mag(w.qe) | mag(w.ip) | mag(w.qp) | mag(w.il) | mag(w.ql)) >= kRange) {   // (an OR reaches 2^20 iff one of them does)
      n_range++;
      events |= GPSX_WLOCK_RANGE;
      return;
    }
    const bool locked = (w.flags & GPSX_WSYNC_LOCKED_FLAG) != 0;
    // 2 a SEARCH window
    if (!locked) {
      if (flags & GPSX_WLOCK_CARRIER) {
        flags &= ~GPSX_WLOCK_CARRIER;
        n_lost_carrier++;
        events |= GPSX_WLOCK_LOST_CARRIER;
      }
      car_good = car_bad = false_run = 0;
    }
    // 3 the open epoch's kind
    if (epoch_n > 0 && ((flags & GPSX_WLOCK_OPEN_LOCKED) != 0) != locked) {
      A = P = D = E = L = 0;
      epoch_n = 0;
    }
    flags = locked ? flags | GPSX_WLOCK_OPEN_LOCKED : flags & ~GPSX_WLOCK_OPEN_LOCKED;
    // 4 the sums
    const long long ip2 = sq(w.ip), qp2 = sq(w.qp);
    A += (long long)mag(w.ip);
    P += ip2 + qp2;
    D += ip2 - qp2;
    E += sq(w.ie) + sq(w.qe);
    L += sq(w.il) + sq(w.ql);
    epoch_n++;
    // 5 the epoch's end
    if (epoch_n < (u32)(locked ? cfg.epoch_lock : cfg.epoch_search))
      return;
    const long long el = E + L, aa = A * A, den = (long long)epoch_n * P - aa;
    code_ratio = el == 0 ? 0.0f : (float)(2 * P) / (float)el;
    car_ratio = P == 0 ? 0.0f : (float)D / (float)P;
    snr = den == 0 ? 0.0f : (float)aa / (float)den;
    last_p = P;
    last_k = epoch_n;
    last_end = w.end_block + 1;
    flags = locked ? flags | GPSX_WLOCK_EPOCH_LOCKED : flags & ~GPSX_WLOCK_EPOCH_LOCKED;
    n_epochs++;
    // 5a the code verdict
    if (verdict(code_ratio >= cfg.code_min, code_good, code_bad, flags, GPSX_WLOCK_CODE, (u32)cfg.n_good, (u32)cfg.n_bad)) {
      n_lost_code++;
      events |= GPSX_WLOCK_LOST_CODE;
      flags |= (cfg.rearm & 1) ? GPSX_WLOCK_PENDING : 0u;
    }
    // 5b the carrier verdict
    if (locked) {
      const bool good = car_ratio >= cfg.car_min && snr >= cfg.snr_min, was = (flags & GPSX_WLOCK_CARRIER) != 0;
      if (verdict(good, car_good, car_bad, flags, GPSX_WLOCK_CARRIER, (u32)cfg.n_good, (u32)cfg.n_bad)) {
        n_lost_carrier++;
        events |= GPSX_WLOCK_LOST_CARRIER;
      }
      false_run = good || was ? 0u : false_run + 1u;
      if (!good && !was && (cfg.rearm & 2) && false_run >= (u32)cfg.patience) {
        flags |= GPSX_WLOCK_PENDING;
        false_run = 0;
      }
    }
    A = P = D = E = L = 0;
    epoch_n = 0;
  };

  auto load_one = [&](int slot) {
    const char *r = reinterpret_cast<const char *>(rec + ((size_t)slot * (size_t)n_ch + (size_t)ch));
    const Quad q = *reinterpret_cast<const Quad *>(r);
    const Pair l = *reinterpret_cast<const Pair *>(r + 16), ef = *reinterpret_cast<const Pair *>(r + 36);
    return Win{q.a, q.b, q.c, q.d, l.a, l.b, ef.a, (u32)ef.b};
  };
  Win even[kAhead], odd[kAhead];
  wstage::load_ahead(even, 0, n_slots, load_one);
#pragma unroll 1
  for (int at = 0; at < n_slots; at += 2 * kAhead)
    wstage::turn(even, odd, at, n_slots, load_one, step);

  if (!run) {
    if (active) {
      lock[ch] = gpsx_wlock_t{0u, 0u, 0u, -1, 0.0f, 0.0f, 0.0f, 0u, 0, 0u, 0u, 0u, {0u, 0u, 0u}};
    }
    return;
  }

  // the launch's end: the re-arm, on the sync state as the sync launch before this one left it
  if (flags & GPSX_WLOCK_PENDING) {
    if (cfg.rearm != 0) {          // (then sync is not null: the host checked)
      gpsx_wsync_state_t *y = sync + ch;
      if (y->mode == GPSX_WSYNC_LOCKED) {
        y->mode = GPSX_WSYNC_SEARCH;
        y->search_n = 0;
        y->prev_best_p1 = 0;
#pragma unroll
        for (int k = 0; k < 6; k++)
          y->win_iq[k] = 0;
        y->win_n = 0;
        y->bit_ip = 0;
        y->loop.n_updates = 0;
        events |= GPSX_WLOCK_REARMED;
        n_rearm++;
        flags &= ~(GPSX_WLOCK_CODE | GPSX_WLOCK_CARRIER | GPSX_WLOCK_OPEN_LOCKED);
        code_good = code_bad = car_good = car_bad = false_run = 0;
        A = P = D = E = L = 0;
        epoch_n = 0;
      }
    }
    flags &= ~GPSX_WLOCK_PENDING;
  }

  const long long b = s0.blocks_seen + n_blocks;
  const long long end_p1 = last_end >= 0 ? s0.blocks_seen + last_end : s0.last_epoch_end_p1;
  gpsx_wlock_state_t s;
  s.blocks_seen = b;
  s.last_epoch_end_p1 = end_p1;
  s.sum_a = A; s.sum_p = P; s.sum_d = D; s.sum_e = E; s.sum_l = L;
  s.last_p = last_p;
  s.last_code_ratio = code_ratio; s.last_car_ratio = car_ratio; s.last_snr = snr;
  s.epoch_n = epoch_n; s.flags = flags; s.last_k = last_k;
  s.code_good = code_good; s.code_bad = code_bad; s.car_good = car_good; s.car_bad = car_bad;
  s.false_run = false_run;
  s.n_lost_code = n_lost_code; s.n_lost_carrier = n_lost_carrier; s.n_rearm = n_rearm; s.n_range = n_range;
  s.reserved = 0;
  st[ch] = s;

  const long long age = b - end_p1;
  const int age_blocks = last_k != 0 ? (int)(age < 0 ? 0 : (age > 0x7FFFFFFFll ? 0x7FFFFFFFll : age)) : -1;
  const gpsx_wlock_t o = {(flags & kOutFlags) | events, n_epochs, last_k, age_blocks, code_ratio, car_ratio, snr, n_range, last_p,
                          n_lost_code, n_lost_carrier, n_rearm, {0u, 0u, 0u}};
  lock[ch] = o;
}

void launch_wlock(hipStream_t s, const gpsx_wsync_rec_t *d_rec, int n_slots, int n_blocks, const gpsx_wlock_cfg_t &cfg, gpsx_wlock_state_t *d_st,
                  gpsx_wsync_state_t *d_sync_st, int n_ch, gpsx_wlock_t *d_lock, uint32_t *d_bad_state)
{
  if (n_ch <= 0 || n_blocks <= 0 || n_blocks > 4096 || n_slots <= 0 || (cfg.rearm != 0 && !d_sync_st))
    return;
  hipLaunchKernelGGL(k_wlock, dim3(((unsigned)n_ch + 63u) / 64u), dim3(64), 0, s, d_rec, n_slots, n_blocks, cfg, d_st, d_sync_st, n_ch, d_lock,
                     d_bad_state);
}

}  // namespace gpsx
