// k_wobs.hip -- EXTENSION, not in the reference: every channel's transmit time at the launch's end, from the window records of the
// weighted loop with bit sync and the word records of the word layer (include/gpsx.h gpsx_wobs).
//
// k_wnav_words' shape, since it is the same problem: one channel per lane, a serial recurrence over the channel's records (a
// dozen operations each), and what decides the time is the read of d_rec.  A lane needs 16 of a record's 48 bytes: code_phase_fine
// and if_freq_offset_hz at offset 24 (8-byte aligned: 48 k + 24), end_block and flags at offset 36 (4-byte aligned) -- two
// global_load_dwordx2 per slot, loaded kAhead slots before the recurrence needs them in two register sets that take turns.
// The word pass is at most eight 16-byte records per channel (12 bytes of each), all in flight at once.
// Absolute block counts go up to 2^62 and Z down to -2^62: every sum of two of them that could leave an int64 is taken modulo
// 20 and modulo the week instead, which is all the definition needs of it.
#include <hip/hip_runtime.h>

#include <cstddef>

#include "gpsx_device.hpp"
#include "gpsx_kernels.hpp"
#include "gpsx_wstage_parts.hpp"

namespace gpsx {

namespace {

static_assert(sizeof(gpsx_wobs_cfg_t) == 8, "gpsx_wobs_cfg_t layout");
static_assert(sizeof(gpsx_wobs_state_t) == 80 && offsetof(gpsx_wobs_state_t, blocks_seen) == 0 && offsetof(gpsx_wobs_state_t, last_bit_end_p1) == 8 &&
              offsetof(gpsx_wobs_state_t, chain_first_p1) == 16 && offsetof(gpsx_wobs_state_t, edge_block) == 24 &&
              offsetof(gpsx_wobs_state_t, tx_ms_at_edge) == 32 && offsetof(gpsx_wobs_state_t, last_win_end_p1) == 40 &&
              offsetof(gpsx_wobs_state_t, last_phase) == 48 && offsetof(gpsx_wobs_state_t, last_freq) == 52 && offsetof(gpsx_wobs_state_t, flags) == 56 &&
              offsetof(gpsx_wobs_state_t, n_wraps) == 60 && offsetof(gpsx_wobs_state_t, n_anchor) == 64 && offsetof(gpsx_wobs_state_t, n_mismatch) == 68 &&
              offsetof(gpsx_wobs_state_t, n_break) == 72 && offsetof(gpsx_wobs_state_t, reserved) == 76, "gpsx_wobs_state_t layout");
static_assert(sizeof(gpsx_wobs_t) == 32 && offsetof(gpsx_wobs_t, tx_ms) == 0 && offsetof(gpsx_wobs_t, code_phase_fine) == 8 &&
              offsetof(gpsx_wobs_t, if_freq_offset_hz) == 12 && offsetof(gpsx_wobs_t, flags) == 16 && offsetof(gpsx_wobs_t, age_blocks) == 20 &&
              offsetof(gpsx_wobs_t, n_wraps) == 24 && offsetof(gpsx_wobs_t, reserved) == 28, "gpsx_wobs_t layout");

constexpr int kAhead = 8;                    // slots a lane's loads run ahead of its recurrence
constexpr int kMaxWords = 4096 / 600 + 2;    // word slots of the longest launch
constexpr long long kMaxCount = 1ll << 62;
constexpr long long kWeekMs = 604800000ll;
constexpr u32 kChainFlags = GPSX_WOBS_EDGE | GPSX_WOBS_TOW | GPSX_WOBS_CONFIRMED | GPSX_WOBS_AMBIGUOUS;
constexpr u32 kStateFlags = GPSX_WOBS_PHASE | kChainFlags;

struct alignas(4) Pair { u32 a, b; };        // two words at a dword-aligned address: one global_load_dwordx2
struct How { u32 end_block, index_flags, aux; };   // what a word record is here: its words 0, 2 and 3
struct Win { float phase, freq; int end_block; u32 flags; };   // what a window is here

__device__ __forceinline__ int mod_pos(long long x, int m) { const int r = (int)(x % m); return r < 0 ? r + m : r; }

}  // namespace

__global__ __launch_bounds__(64) void k_wobs(const gpsx_wsync_rec_t *__restrict__ rec, int n_slots, int n_blocks, float edge_guard,
                                             const gpsx_wnav_word_t *__restrict__ words, int max_words, gpsx_wobs_state_t *__restrict__ st,
                                             int n_ch, gpsx_wobs_t *__restrict__ obs, u32 *__restrict__ bad_state)
{
  const int lane = threadIdx.x;
  const int ch0 = (int)blockIdx.x * 64;
  const bool active = lane < n_ch - ch0;
  const int ch = active ? ch0 + lane : n_ch - 1;   // (always a channel below n_ch: the idle lanes of the last wave load, nothing else)
  const gpsx_wobs_state_t s0 = st[ch];
  const bool valid = (s0.flags & ~kStateFlags) == 0 && s0.reserved == 0 && (u64)s0.blocks_seen <= (u64)kMaxCount &&
                     (u64)s0.last_bit_end_p1 <= (u64)kMaxCount && (u64)s0.chain_first_p1 <= (u64)kMaxCount &&
                     (u64)s0.last_win_end_p1 <= (u64)kMaxCount && s0.edge_block >= -kMaxCount && s0.edge_block <= kMaxCount &&
                     (u64)s0.tx_ms_at_edge < (u64)kWeekMs &&
                     (!(s0.flags & GPSX_WOBS_PHASE) || (s0.last_phase >= 0.0f && s0.last_phase < 16368.0f));
  if (active && !valid && bad_state)
    *bad_state = 1u;
  const bool run = active && valid;

  // the state in registers.  Ends of bits and windows are kept launch-relative, as end_block + 1: last_bit the newest bit's (a value
  // far outside a launch when that bit is older than the launch: it then equals no end_block + 1 - 20), last_win / first the newest
  // window's and the chain's first bit's when they fell into this launch, else -1
  u32 flags = s0.flags, n_wraps = s0.n_wraps, n_break = s0.n_break;
  float last_phase = s0.last_phase, last_freq = s0.last_freq;
  long long z = s0.edge_block;
  const long long base = s0.blocks_seen;
  bool have_bit = s0.last_bit_end_p1 != 0;
  const long long rel = s0.last_bit_end_p1 - base;
  int last_bit = (int)(rel < -100000 ? -100000 : (rel > 100000 ? 100000 : rel));
  int last_win = -1, first = -1;
  bool any_bit = false;      // last_bit is this launch's (or was cleared in it)

  auto step = [&](const Win &w) {
    const float p = w.phase;
    if (!(run && (w.flags & GPSX_WSYNC_WINDOW) && (u32)w.end_block < (u32)n_blocks && p >= 0.0f && p < 16368.0f))
      return;
    const int w_p1 = w.end_block + 1;
    const bool locked = (w.flags & GPSX_WSYNC_LOCKED_FLAG) != 0;
    // 1 a SEARCH window
    if (!locked) {
      n_break += (flags >> 1) & 1u;
      flags &= ~kChainFlags;
      have_bit = false;
      any_bit = true;
    }
    // 2 wrap
    if ((flags & (GPSX_WOBS_EDGE | GPSX_WOBS_PHASE)) == (GPSX_WOBS_EDGE | GPSX_WOBS_PHASE)) {
      const float d = p - last_phase;
      const int dz = d > 8184.0f ? -1 : (d < -8184.0f ? 1 : 0);
      z += dz;
      n_wraps += (u32)(dz != 0);
    }
    // 3 the newest record
    last_phase = p;
    last_freq = w.freq;
    last_win = w_p1;
    flags |= GPSX_WOBS_PHASE;
    // 4 a bit
    if (locked && (w.flags & GPSX_WSYNC_BIT)) {
      if (have_bit && w_p1 != last_bit + 20) {
        n_break += (flags >> 1) & 1u;
        flags &= ~kChainFlags;
      }
      if (!(flags & GPSX_WOBS_EDGE)) {
        z = base + (long long)(w_p1 - (p >= 8184.0f ? 1 : 0));
        first = w_p1;
        flags |= GPSX_WOBS_EDGE | (fabsf(p - 8184.0f) < edge_guard ? GPSX_WOBS_AMBIGUOUS : 0u);
      }
      last_bit = w_p1;
      have_bit = any_bit = true;
    }
  };

  auto load_one = [&](int slot) {
    const char *r = reinterpret_cast<const char *>(rec + ((size_t)slot * (size_t)n_ch + (size_t)ch));
    const Pair pf = *reinterpret_cast<const Pair *>(r + 24), ef = *reinterpret_cast<const Pair *>(r + 36);
    return Win{__uint_as_float(pf.a), __uint_as_float(pf.b), (int)ef.a, ef.b};
  };
  Win even[kAhead], odd[kAhead];
  wstage::load_ahead(even, 0, n_slots, load_one);
#pragma unroll 1
  for (int at = 0; at < n_slots; at += 2 * kAhead)
    wstage::turn(even, odd, at, n_slots, load_one, step);

  // the word records, all in flight before the first is looked at (loaded here, not beside pass 1: their 24 registers there cost
  // the fourth wave per SIMD, and one round trip per wave at the end costs a hundredth of the kernel)
  How wd[kMaxWords];
#pragma unroll
  for (int k = 0; k < kMaxWords; k++) {
    const char *r = reinterpret_cast<const char *>(words + ((size_t)min(k, max_words - 1) * (size_t)n_ch + (size_t)ch));
    const Pair ia = *reinterpret_cast<const Pair *>(r + 8);
    wd[k] = How{*reinterpret_cast<const u32 *>(r), ia.a, ia.b};
  }
  if (!run) {
    if (active)
      obs[ch] = gpsx_wobs_t{0, 0.0f, 0.0f, 0u, -1, 0u, 0u};
    return;
  }
  const long long last_bit_p1 = any_bit ? (have_bit ? base + last_bit : 0) : s0.last_bit_end_p1;
  const long long first_p1 = first >= 0 ? base + first : s0.chain_first_p1;

  // pass 2: the HOWs, on sums taken modulo 20 and modulo the week
  long long tz = s0.tx_ms_at_edge;
  u32 n_anchor = s0.n_anchor, n_mismatch = s0.n_mismatch;
  const int base20 = mod_pos(base, 20), z20 = mod_pos(z, 20), base_wk = mod_pos(base, (int)kWeekMs), z_wk = mod_pos(z, (int)kWeekMs);
#pragma unroll
  for (int k = 0; k < kMaxWords; k++) {
    const u32 end_block = wd[k].end_block, index = wd[k].index_flags & 0xFFu, wflags = (wd[k].index_flags >> 8) & 0xFFu, aux = wd[k].aux;
    if (!(k < max_words && (wflags & (GPSX_WNAV_WORD | GPSX_WNAV_OK)) == (GPSX_WNAV_WORD | GPSX_WNAV_OK) && index == 2u && aux < 100800u &&
          end_block < (u32)n_blocks && (flags & GPSX_WOBS_EDGE)))
      continue;
    const int e1 = (int)end_block + 1;
    const long long e_p1 = base + e1;
    if (!(e_p1 >= first_p1 + 1220 && e_p1 <= last_bit_p1 && (last_bit_p1 - e_p1) % 20 == 0))
      continue;
    const int t = 6000 * (int)((aux + 100799u) % 100800u) + 1200;
    const int r = (base20 + e1 % 20 + 20 - z20 + 10) % 20 - 10;      // E + 1 - Z - 20 j
    if (r > 5 || r < -5) {
      n_mismatch++;
      continue;
    }
    // Tc = (T - 20 j) mod week, with 20 j = E + 1 - Z - r
    long long tc = ((long long)t + r - base_wk - e1 + z_wk) % kWeekMs;
    tc = tc < 0 ? tc + kWeekMs : tc;
    if (!(flags & GPSX_WOBS_TOW)) {
      tz = tc;
      flags |= GPSX_WOBS_TOW;
      n_anchor++;
    } else if (tc == tz) {
      flags |= GPSX_WOBS_CONFIRMED;
    } else {
      tz = tc;
      flags &= ~GPSX_WOBS_CONFIRMED;
      n_mismatch++;
    }
  }

  // the state, and the observable at the first sample of block B
  const long long b = base + n_blocks;
  const long long last_win_p1 = last_win >= 0 ? base + last_win : s0.last_win_end_p1;
  gpsx_wobs_state_t s;
  s.blocks_seen = b;
  s.last_bit_end_p1 = last_bit_p1;
  s.chain_first_p1 = first_p1;
  s.edge_block = z;
  s.tx_ms_at_edge = tz;
  s.last_win_end_p1 = last_win_p1;
  s.last_phase = last_phase; s.last_freq = last_freq;
  s.flags = flags; s.n_wraps = n_wraps;
  s.n_anchor = n_anchor; s.n_mismatch = n_mismatch; s.n_break = n_break; s.reserved = 0;
  st[ch] = s;

  constexpr u32 need = GPSX_WOBS_PHASE | GPSX_WOBS_EDGE | GPSX_WOBS_TOW;
  const bool ok = (flags & need) == need, phase = (flags & GPSX_WOBS_PHASE) != 0;
  long long tx = (tz + base_wk + n_blocks - z_wk) % kWeekMs;
  tx = tx < 0 ? tx + kWeekMs : tx;
  const long long age = b - last_win_p1;
  gpsx_wobs_t o;
  o.tx_ms = ok ? tx : 0;
  o.code_phase_fine = phase ? last_phase : 0.0f;
  o.if_freq_offset_hz = phase ? last_freq : 0.0f;
  o.flags = flags | (ok ? GPSX_WOBS_VALID : 0u);
  o.age_blocks = phase ? (int)(age < 0 ? 0 : (age > 0x7FFFFFFFll ? 0x7FFFFFFFll : age)) : -1;
  o.n_wraps = n_wraps;
  o.reserved = 0;
  obs[ch] = o;
}

void launch_wobs(hipStream_t s, const gpsx_wsync_rec_t *d_rec, int n_slots, int n_blocks, float edge_guard, const gpsx_wnav_word_t *d_words,
                 gpsx_wobs_state_t *d_st, int n_ch, gpsx_wobs_t *d_obs, uint32_t *d_bad_state)
{
  if (n_ch <= 0 || n_blocks <= 0 || n_blocks > 4096 || n_slots <= 0)
    return;
  hipLaunchKernelGGL(k_wobs, dim3(((unsigned)n_ch + 63u) / 64u), dim3(64), 0, s, d_rec, n_slots, n_blocks, edge_guard, d_words,
                     n_blocks / 600 + 2, d_st, n_ch, d_obs, d_bad_state);
}

}  // namespace gpsx
