// gpsx_wstage_parts.hpp -- what the stage kernels behind the weighted loop with bit sync share, one channel per lane in all four:
// k_wnav_words, k_wobs and k_wlock walk a channel's window records slot by slot, k_weph reads the word records the first of them wrote.
// Here: the layout of the two record types (once, for all four) and the slot walk's body.  A kernel keeps the asserts on its own
// cfg, state and output structs, what it takes out of a record (its item type, its loads), its look-ahead kAhead and its recurrence.
// The kernels are, instruction for instruction, what they were before this header (profiles/r20_wstage_parts_isa.txt).
#pragma once
#include <cstddef>
#include "gpsx_device.hpp"
namespace gpsx {
namespace wstage {

static_assert(sizeof(gpsx_wsync_rec_t) == 48 && offsetof(gpsx_wsync_rec_t, w) == 0 && offsetof(gpsx_wloop_rec_t, iq) == 0 &&
              offsetof(gpsx_wloop_rec_t, code_phase_fine) == 24 && offsetof(gpsx_wloop_rec_t, if_freq_offset_hz) == 28 &&
              offsetof(gpsx_wsync_rec_t, end_block) == 36 && offsetof(gpsx_wsync_rec_t, flags) == 40 && offsetof(gpsx_wsync_rec_t, bit_ip) == 44,
              "gpsx_wsync_rec_t layout");
static_assert(sizeof(gpsx_wnav_word_t) == 16 && offsetof(gpsx_wnav_word_t, end_block) == 0 && offsetof(gpsx_wnav_word_t, word) == 4 &&
              offsetof(gpsx_wnav_word_t, index) == 8 && offsetof(gpsx_wnav_word_t, flags) == 9 && offsetof(gpsx_wnav_word_t, subframe_id) == 10 &&
              offsetof(gpsx_wnav_word_t, zero) == 11 && offsetof(gpsx_wnav_word_t, aux) == 12, "gpsx_wnav_word_t layout");

// The slot walk: step(load_one(slot)) for a channel's n_slots records in order, the loads kAhead slots ahead of the steps in two
// register sets that take turns -- never copied: a copy would have to wait for the loads it copies.  load_one(slot) -> what the
// kernel takes out of that slot's record, an Item (its loads do not depend on the recurrence's state).  A kernel loads `even` from
// slot 0 and calls turn() for at = 0, 2 kAhead, .. under #pragma unroll 1.  That loop statement stays in the kernel: a loop the
// compiler first meets inside a helper is optimised there, against opaque closures, and again in the kernel, and comes out as other
// instructions.  load_ahead and step_through are plain inline functions for the same reason: the lambdas they replace were.

// kAhead slots from slot `from` on; slots past the launch's last repeat it (in bounds, and not stepped through)
template <int kAhead, typename Item, typename LoadOne>
__device__ inline void load_ahead(Item (&to)[kAhead], int from, int n_slots, const LoadOne &load_one)
{
#pragma unroll
  for (int u = 0; u < kAhead; u++)
    to[u] = load_one(min(from + u, n_slots - 1));
}
template <int kAhead, typename Item, typename Step>
__device__ inline void step_through(const Item (&from)[kAhead], int at, int n_slots, Step &step)
{
#pragma unroll
  for (int u = 0; u < kAhead; u++)
    if (at + u < n_slots)   // (uniform over the launch)
      step(from[u]);
}

// one round of the walk: slots at .. at + 2 kAhead - 1 stepped through, the 2 kAhead behind them loaded
template <int kAhead, typename Item, typename LoadOne, typename Step>
__device__ __forceinline__ void turn(Item (&even)[kAhead], Item (&odd)[kAhead], int at, int n_slots, const LoadOne &load_one, Step &step)
{
  load_ahead(odd, at + kAhead, n_slots, load_one);   // (unconditional: a set that is loaded on one path only is merged by copies, which wait)
  step_through(even, at, n_slots, step);
  load_ahead(even, at + 2 * kAhead, n_slots, load_one);
  step_through(odd, at + kAhead, n_slots, step);
}

}  // namespace wstage
}  // namespace gpsx
