// k_wnav_words.hip -- EXTENSION, not in the reference: LNAV frame sync and parity-checked words from the bit records of the weighted
// loop with bit sync (include/gpsx.h gpsx_wnav_words).
//
// One channel per lane: the frame state is a serial recurrence over the channel's bits, a few dozen integer operations per bit
// and a parity test once per word.  What decides the time is the read of d_rec: a bit is 12 of a record's 48 bytes (end_block,
// flags, bit_ip at offset 36), the lanes of a wave sit 48 bytes apart, and every cache line of the array is touched once.  The
// three words do not depend on the state, so a lane loads them kAhead slots before the recurrence needs them (two register
// sets that take turns: the slots in work and the slots in flight); with one 3 KB row in flight per wave and slot ahead, a full device holds
// tens of megabytes in flight and the kernel runs at the memory's pace, not at one round trip per slot.
// A word is one 16-byte store to the channel's next slot; the slots a channel did not fill get the empty pattern at the end.
// (The other load shape -- the wave loads whole rows in 16-byte pieces as k_track_wsync stored them and passes them through LDS --
//  was built and measured: 9 to 11 % slower, 145 VGPRs and 24 KB of LDS.  EXPERIMENTS.md.)
#include <hip/hip_runtime.h>

#include <cstddef>
#include <initializer_list>

#include "gpsx_device.hpp"
#include "gpsx_kernels.hpp"
#include "gpsx_wstage_parts.hpp"

namespace gpsx {

namespace {

static_assert(sizeof(gpsx_wnav_cfg_t) == 8, "gpsx_wnav_cfg_t layout");
static_assert(sizeof(gpsx_wnav_state_t) == 64 && offsetof(gpsx_wnav_state_t, hist) == 0 && offsetof(gpsx_wnav_state_t, blocks_seen) == 8 &&
              offsetof(gpsx_wnav_state_t, last_bit_end_p1) == 16 && offsetof(gpsx_wnav_state_t, fresh) == 24 &&
              offsetof(gpsx_wnav_state_t, mode) == 28 && offsetof(gpsx_wnav_state_t, inv) == 32 && offsetof(gpsx_wnav_state_t, word_idx) == 36 &&
              offsetof(gpsx_wnav_state_t, bit_idx) == 40 && offsetof(gpsx_wnav_state_t, bad_run) == 44 &&
              offsetof(gpsx_wnav_state_t, ok_mask) == 48 && offsetof(gpsx_wnav_state_t, n_sync) == 52 && offsetof(gpsx_wnav_state_t, n_drop) == 56 &&
              offsetof(gpsx_wnav_state_t, n_subframes) == 60, "gpsx_wnav_state_t layout");

constexpr int kAhead = 8;                    // slots a lane's loads run ahead of its recurrence
constexpr u32 kWord30 = 0x3FFFFFFFu;
constexpr long long kMaxCount = 1ll << 62;   // blocks_seen and last_bit_end_p1 lie in 0 .. 2^62

struct Bit3 { int end_block; u32 flags; int bit_ip; };   // what a bit is: a record's last three words
struct alignas(4) Word16 { u32 w[4]; };                   // a word record at a dword-aligned address: one global_store_dwordx4

// IS-GPS-200 table 20-XIV (kParityMask of gpsx_steps.cpp, with d1 in bit 23 here)
constexpr u32 taps(std::initializer_list<int> bits)
{
  u32 m = 0;
  for (int b : bits)
    m |= 1u << (24 - b);
  return m;
}

__device__ __forceinline__ u32 source_bits(u32 w, u32 p30) { return ((w >> 6) ^ (0u - p30)) & 0xFFFFFFu; }

__device__ __forceinline__ bool parity_ok(u32 w, u32 p29, u32 p30)
{
  constexpr u32 m0 = taps({1, 2, 3, 5, 6, 10, 11, 12, 13, 14, 17, 18, 20, 23}), m1 = taps({2, 3, 4, 6, 7, 11, 12, 13, 14, 15, 18, 19, 21, 24});
  constexpr u32 m2 = taps({1, 3, 4, 5, 7, 8, 12, 13, 14, 15, 16, 19, 20, 22}), m3 = taps({2, 4, 5, 6, 8, 9, 13, 14, 15, 16, 17, 20, 21, 23});
  constexpr u32 m4 = taps({1, 3, 5, 6, 7, 9, 10, 14, 15, 16, 17, 18, 21, 22, 24}), m5 = taps({3, 5, 6, 8, 9, 10, 11, 13, 15, 19, 22, 23, 24});
  const u32 d = source_bits(w, p30);
  const u32 odd = ((u32)__popc(d & m0) & 1u) << 5 | ((u32)__popc(d & m1) & 1u) << 4 | ((u32)__popc(d & m2) & 1u) << 3 |
                  ((u32)__popc(d & m3) & 1u) << 2 | ((u32)__popc(d & m4) & 1u) << 1 | ((u32)__popc(d & m5) & 1u);
  return (odd ^ ((0u - p29) & 0x29u) ^ ((0u - p30) & 0x16u)) == (w & 63u);   // D25, D27, D30 start from D29*; D26, D28, D29 from D30*
}

}  // namespace

__global__ __launch_bounds__(64) void k_wnav_words(const gpsx_wsync_rec_t *__restrict__ rec, int n_slots, int n_blocks, int max_bad_words,
                                                   gpsx_wnav_state_t *__restrict__ st, int n_ch, gpsx_wnav_word_t *__restrict__ words,
                                                   int max_words, u32 *__restrict__ bad_state)
{
  const int lane = threadIdx.x;
  const int ch0 = (int)blockIdx.x * 64;
  const bool active = lane < n_ch - ch0;
  const int ch = active ? ch0 + lane : n_ch - 1;   // (always a channel below n_ch: the idle lanes of the last wave load, nothing else)
  const gpsx_wnav_state_t s0 = st[ch];
  const bool valid = (u32)s0.mode <= 1u && (u32)s0.inv <= 1u && (u32)s0.word_idx <= 9u && (u32)s0.bit_idx <= 29u && (u32)s0.fresh <= 62u &&
                     (u32)s0.bad_run <= 10u && (u64)s0.blocks_seen <= (u64)kMaxCount && (u64)s0.last_bit_end_p1 <= (u64)kMaxCount;
  if (active && !valid && bad_state)
    *bad_state = 1u;
  const bool run = active && valid;

  // the state in registers.  The time base is kept launch-relative: last_rel = the newest bit's end block counted from this
  // launch's first (a value far outside a launch when the newest bit is older than that: it then equals no end_block - 20)
  u64 hist = s0.hist;
  int fresh = s0.fresh, mode = s0.mode, inv = s0.inv, word_idx = s0.word_idx, bit_idx = s0.bit_idx, bad_run = s0.bad_run;
  u32 ok_mask = s0.ok_mask, n_sync = s0.n_sync, n_drop = s0.n_drop, n_subframes = s0.n_subframes;
  bool have_last = s0.last_bit_end_p1 != 0, any_bit = false;
  const long long rel = s0.last_bit_end_p1 - (s0.blocks_seen + 1);
  int last_rel = (int)(rel < -100000 ? -100000 : (rel > 100000 ? 100000 : rel));
  int n_out = 0;

  auto emit = [&](int end_block, u32 word, u32 index, u32 flags, u32 id, u32 aux) {
    if (n_out < max_words) {   // (the header's bound: never false)
      reinterpret_cast<Word16 *>(words)[(size_t)n_out * (size_t)n_ch + (size_t)ch] = Word16{{(u32)end_block, word, index | flags << 8 | id << 16, aux}};
      n_out++;
    }
  };

  auto step = [&](const Bit3 &b) {
    if (!(run && (b.flags & (GPSX_WSYNC_WINDOW | GPSX_WSYNC_BIT)) == (GPSX_WSYNC_WINDOW | GPSX_WSYNC_BIT) && (u32)b.end_block < (u32)n_blocks))
      return;
    // 1 continuity
    if (have_last && b.end_block != last_rel + 20) {
      n_drop += (u32)mode;
      mode = GPSX_WNAV_HUNT;
      fresh = word_idx = bit_idx = bad_run = 0;
      ok_mask = 0;
    }
    last_rel = b.end_block;
    have_last = any_bit = true;
    // 2 shift
    hist = hist << 1 | (u64)((u32)b.bit_ip >> 31);
    fresh = min(fresh + 1, 62);
    if (mode == GPSX_WNAV_HUNT) {
      // 3 TLM + HOW as a whole; parity does not see the polarity, so the preamble alone says which inv' can pass
      const u32 t = (u32)(hist >> 52) & 0xFFu;
      if (fresh == 62 && (t == 0x8Bu || t == 0x74u)) {
        const u32 inv1 = t == 0x74u;
        const u64 x = inv1 ? ~hist : hist;
        const u32 w1 = (u32)(x >> 30) & kWord30, w2 = (u32)x & kWord30;
        const u32 p29 = (u32)(x >> 61) & 1u, p30 = (u32)(x >> 60) & 1u;
        const u32 d2 = source_bits(w2, w1 & 1u);
        const u32 id = (d2 >> 2) & 7u;
        if (parity_ok(w1, p29, p30) && parity_ok(w2, (w1 >> 1) & 1u, w1 & 1u) && (w2 & 3u) == 0 && id >= 1 && id <= 5) {
          inv = (int)inv1;
          mode = GPSX_WNAV_SYNCED;
          word_idx = 2;
          bit_idx = bad_run = 0;
          ok_mask = 3u | id << 16;
          n_sync++;
          const u32 flags = GPSX_WNAV_WORD | GPSX_WNAV_OK | GPSX_WNAV_SYNC | (inv1 ? GPSX_WNAV_INVERTED : 0u);
          emit(b.end_block - 600, source_bits(w1, p30) << 6 | (w1 & 63u), 1, flags, id, 0);
          emit(b.end_block, d2 << 6 | (w2 & 63u), 2, flags, id, (d2 >> 7) & 0x1FFFFu);
        }
      }
      return;
    }
    // 4 SYNCED
    if (++bit_idx < 30)
      return;
    const u32 w = (u32)hist & kWord30, p29 = (u32)(hist >> 31) & 1u, p30 = (u32)(hist >> 30) & 1u;
    const int index = word_idx + 1;
    const u32 d = source_bits(w, p30);
    bool passed = parity_ok(w, p29, p30);
    u32 flags = GPSX_WNAV_WORD, aux = 0;
    if (index == 1) {
      const u32 t = ((w ^ (0u - (u32)inv)) & kWord30) >> 22;
      if (t == 0x74u && passed) {
        inv ^= 1;
        flags |= GPSX_WNAV_FLIPPED;
      } else if (t != 0x8Bu) {
        passed = false;
      }
    }
    const u32 x = (w ^ (0u - (u32)inv)) & kWord30;
    if (index == 2) {
      const u32 id = (d >> 2) & 7u;
      passed = passed && (x & 3u) == 0 && id >= 1 && id <= 5;
      ok_mask = (ok_mask & 0x3FFu) | (passed ? id << 16 : 0u);
      if (passed)
        aux = (d >> 7) & 0x1FFFFu;
    }
    if (passed) {
      flags |= GPSX_WNAV_OK;
      ok_mask |= 1u << (index - 1);
    }
    if (inv)
      flags |= GPSX_WNAV_INVERTED;
    const u32 id_out = (ok_mask >> 16) & 7u;
    bad_run = passed ? 0 : min(bad_run + 1, 10);
    bit_idx = 0;
    word_idx = index == 10 ? 0 : index;
    if (index == 10) {
      if ((ok_mask & 0x3FFu) == 0x3FFu) {
        flags |= GPSX_WNAV_SUBFRAME;
        n_subframes++;
      }
      ok_mask = 0;
    }
    if (bad_run >= max_bad_words) {
      flags |= GPSX_WNAV_DROPPED;
      n_drop++;
      mode = GPSX_WNAV_HUNT;
      fresh = word_idx = 0;
    }
    emit(b.end_block, d << 6 | (x & 63u), (u32)index, flags, id_out, aux);
  };

  auto load_one = [&](int slot) {
    const gpsx_wsync_rec_t &r = rec[(size_t)slot * (size_t)n_ch + (size_t)ch];
    return Bit3{r.end_block, r.flags, r.bit_ip};
  };
  Bit3 even[kAhead], odd[kAhead];
  wstage::load_ahead(even, 0, n_slots, load_one);
#pragma unroll 1
  for (int at = 0; at < n_slots; at += 2 * kAhead)
    wstage::turn(even, odd, at, n_slots, load_one, step);

  if (active) {
#pragma unroll 1
    for (int k = n_out; k < max_words; k++)   // (a bad channel: every slot)
      reinterpret_cast<Word16 *>(words)[(size_t)k * (size_t)n_ch + (size_t)ch] = Word16{{~0u, 0u, 0u, 0u}};
  }
  if (run) {
    gpsx_wnav_state_t s;
    s.hist = hist;
    s.blocks_seen = s0.blocks_seen + n_blocks;
    s.last_bit_end_p1 = any_bit ? s0.blocks_seen + 1 + last_rel : s0.last_bit_end_p1;
    s.fresh = fresh; s.mode = mode; s.inv = inv; s.word_idx = word_idx; s.bit_idx = bit_idx; s.bad_run = bad_run;
    s.ok_mask = ok_mask; s.n_sync = n_sync; s.n_drop = n_drop; s.n_subframes = n_subframes;
    st[ch] = s;
  }
}

void launch_wnav_words(hipStream_t s, const gpsx_wsync_rec_t *d_rec, int n_slots, int n_blocks, int max_bad_words, gpsx_wnav_state_t *d_st,
                       int n_ch, gpsx_wnav_word_t *d_words, uint32_t *d_bad_state)
{
  if (n_ch <= 0 || n_blocks <= 0 || n_slots <= 0)
    return;
  hipLaunchKernelGGL(k_wnav_words, dim3(((unsigned)n_ch + 63u) / 64u), dim3(64), 0, s, d_rec, n_slots, n_blocks, max_bad_words, d_st, n_ch,
                     d_words, n_blocks / 600 + 2, d_bad_state);
}

}  // namespace gpsx
