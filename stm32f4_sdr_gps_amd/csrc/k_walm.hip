// k_walm.hip -- EXTENSION, not in the reference: almanac, ionosphere and UTC from subframes 4 and 5 of the word records (include/gpsx.h
// gpsx_walm): every slot's subframes assembled across launches as k_weph assembles them, the newest copy of the 32
// almanac pages, of subframe 4 page 18 and of subframe 5 page 25 kept per receiver in a device-resident bank, and decoded per launch.
//
// k_wbank's geometry: one wave per receiver, four receivers per 256-thread workgroup; no LDS, no barrier, no scratch.  The wave works
// on two small sets.  First lane j is slot j: its up-to-eight word records (one 16-byte load each), its 64-byte state, and -- lane e
// is bank entry e -- the entry's eight words and the bank's tail are all requested before the first is looked at; then k_weph's
// recurrence.  Second lane e is entry e: the slots that completed a page are a ballot, and each is applied in ascending slot order by
// nine lane broadcasts (the entry number, the eight words), so the highest slot's words stand.  An entry is written back only if its
// words changed, and none is read back.  Every ballot and broadcast runs under wave-uniform control flow (a wave whose receiver does
// not exist leaves as a whole; the commit loop walks a ballot; lane-dependent conditions are selects).  cur[] is indexed by data (the
// word's index): a chain of selects over constant indices, as in k_weph, so nothing goes to scratch.  FP64 only scales integers.
// The 96-byte almanac records leave directly, six 16-byte stores per lane of lanes 0 .. 31: a receiver's 32 records are 3 KiB of
// consecutive addresses, every line of which the wave's six store instructions fill between them (EXPERIMENTS.md).
#include <hip/hip_runtime.h>

#include <cstddef>

#include "gpsx_device.hpp"
#include "gpsx_kernels.hpp"

namespace gpsx {

namespace {

static_assert(sizeof(gpsx_walm_cfg_t) == 16 && offsetof(gpsx_walm_cfg_t, reserved) == 4, "gpsx_walm_cfg_t layout");
static_assert(sizeof(gpsx_walm_slot_t) == 64 && offsetof(gpsx_walm_slot_t, last_word_end_p1) == 8 && offsetof(gpsx_walm_slot_t, cur) == 16 &&
              offsetof(gpsx_walm_slot_t, cur_mask) == 48 && offsetof(gpsx_walm_slot_t, cur_next) == 52 && offsetof(gpsx_walm_slot_t, cur_id) == 56 &&
              offsetof(gpsx_walm_slot_t, reserved) == 60, "gpsx_walm_slot_t layout");
static_assert(sizeof(gpsx_walm_bank_t) == 1120 && offsetof(gpsx_walm_bank_t, have_mask) == 1088 && offsetof(gpsx_walm_bank_t, n_stored) == 1096 &&
              offsetof(gpsx_walm_bank_t, n_other) == 1104 && offsetof(gpsx_walm_bank_t, reserved) == 1108, "gpsx_walm_bank_t layout");
static_assert(sizeof(gpsx_walm_rx_t) == 160 && offsetof(gpsx_walm_rx_t, have_mask) == 8 && offsetof(gpsx_walm_rx_t, healthy_mask) == 32 &&
              offsetof(gpsx_walm_rx_t, toa_s) == 44 && offsetof(gpsx_walm_rx_t, tot_s) == 52 && offsetof(gpsx_walm_rx_t, reserved) == 76 &&
              offsetof(gpsx_walm_rx_t, A0) == 80 && offsetof(gpsx_walm_rx_t, ion) == 96, "gpsx_walm_rx_t layout");
static_assert(sizeof(gpsx_walm_sv_t) == 96 && offsetof(gpsx_walm_sv_t, svid) == 4 && offsetof(gpsx_walm_sv_t, toas) == 16 &&
              offsetof(gpsx_walm_sv_t, f1) == 88, "gpsx_walm_sv_t layout");
static_assert(sizeof(gpsx_wnav_word_t) == 16 && offsetof(gpsx_wnav_word_t, end_block) == 0 && offsetof(gpsx_wnav_word_t, word) == 4 &&
              offsetof(gpsx_wnav_word_t, index) == 8 && offsetof(gpsx_wnav_word_t, flags) == 9 && offsetof(gpsx_wnav_word_t, subframe_id) == 10 &&
              offsetof(gpsx_wnav_word_t, aux) == 12, "gpsx_wnav_word_t layout");

constexpr int kMaxWords = 4096 / 600 + 2;    // word slots of the longest launch
constexpr long long kMaxCount = 1ll << 62;
constexpr u32 kTowCounts = 100800u;          // six-second counts of a week
constexpr int kEntries = GPSX_WALM_ENTRIES, kPage18 = 32, kPage25 = 33;
constexpr u32 kToaMax = 147u;                // 147 * 4096 s = 602 112 s: the last toa inside a week

struct alignas(16) Quad { u32 a, b, c, d; };   // 16 bytes as one global_load_dwordx4 / global_store_dwordx4

constexpr double kSemiCircle = 3.1415926535898;
constexpr int kBuildWeek = 2290;

// `len` bits from subframe bit `pos`, first bit most significant, out of the eight words 3 .. 10 (d1 in bit 23): k_weph's
template <int pos, int len>
__device__ __forceinline__ u32 take(const u32 (&w)[8])
{
  static_assert(pos >= 60 && pos % 30 + len <= 24 && len >= 1 && len <= 24, "a run inside one word's source bits");
  return (w[pos / 30 - 2] >> (24 - pos % 30 - len)) & ((1u << len) - 1u);
}
template <int len>
__device__ __forceinline__ int as_int(u32 raw)   // two's complement of `len` bits (len 32: the word itself)
{
  return (int)(len < 32 && (raw >> (len - 1)) ? raw | (~0u << (len & 31)) : raw);
}
__device__ __forceinline__ int week8(u32 w) { return (int)w + (kBuildWeek - (int)w + 128) / 256 * 256; }
__device__ __forceinline__ u32 lane_word(u32 v, int lane) { return (u32)__builtin_amdgcn_readlane((int)v, lane); }   // (lane: wave-uniform)

}  // namespace

__global__ __launch_bounds__(256) void k_walm(const gpsx_wnav_word_t *__restrict__ words, int max_words, int n_blocks, int ch, int n_rx,
                                              gpsx_walm_slot_t *__restrict__ st, gpsx_walm_bank_t *__restrict__ bank,
                                              gpsx_walm_rx_t *__restrict__ rx, gpsx_walm_sv_t *__restrict__ alm, u32 *__restrict__ bad_state)
{
  const int lane = (int)threadIdx.x & 63;
  const int r = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
  if (r >= n_rx)          // (the whole wave: r is the same in its 64 lanes)
    return;
  const size_t n_ch = (size_t)n_rx * (size_t)ch;
  const bool is_slot = lane < ch, is_entry = lane < kEntries;
  const size_t c = (size_t)r * (size_t)ch + (size_t)(is_slot ? lane : 0);   // (always a slot of this receiver: idle lanes load, nothing else)
  gpsx_walm_bank_t *const bk = bank + r;

  // everything the wave reads, in flight before the first is looked at; word slots past the launch's last repeat it (in bounds)
  Quad wd[kMaxWords];
#pragma unroll
  for (int k = 0; k < kMaxWords; k++)
    wd[k] = *reinterpret_cast<const Quad *>(words + ((size_t)min(k, max_words - 1) * n_ch + c));
  Quad sq[4];
#pragma unroll
  for (int k = 0; k < 4; k++)
    sq[k] = reinterpret_cast<const Quad *>(st + c)[k];
  const Quad *const my_page = reinterpret_cast<const Quad *>(bk->page[is_entry ? lane : 0]);
  const Quad pq0 = my_page[0], pq1 = my_page[1];
  const Quad t0 = reinterpret_cast<const Quad *>(&bk->have_mask)[0], t1 = reinterpret_cast<const Quad *>(&bk->have_mask)[1];   // (one address for the wave)

  // the bank
  const u32 before[8] = {pq0.a, pq0.b, pq0.c, pq0.d, pq1.a, pq1.b, pq1.c, pq1.d};
  const u64 have0 = (u64)t0.a | (u64)t0.b << 32;
  const u32 bank_stored = t0.c, bank_changed = t0.d, bank_other = t1.a;
  const bool words_ok = !is_entry || (before[0] | before[1] | before[2] | before[3] | before[4] | before[5] | before[6] | before[7]) < (1u << 24);
  const bool bank_ok = __ballot(!words_ok) == 0ull && (have0 >> kEntries) == 0ull && (t1.b | t1.c | t1.d) == 0u;   // (wave-uniform)

  // the slot
  const long long blocks_seen = (long long)((u64)sq[0].a | (u64)sq[0].b << 32), last0 = (long long)((u64)sq[0].c | (u64)sq[0].d << 32);
  u32 cur[8] = {sq[1].a, sq[1].b, sq[1].c, sq[1].d, sq[2].a, sq[2].b, sq[2].c, sq[2].d};
  u32 cur_mask = sq[3].a, cur_next = sq[3].b, cur_id = sq[3].c;
  const bool slot_ok = (u64)blocks_seen <= (u64)kMaxCount && (u64)last0 <= (u64)kMaxCount && cur_next <= 10u && cur_next != 1u && cur_mask <= 0x3FFu &&
                       cur_id <= 5u && (cur[0] | cur[1] | cur[2] | cur[3] | cur[4] | cur[5] | cur[6] | cur[7]) < (1u << 24) && sq[3].d == 0u;
  if (bad_state && (!bank_ok || (is_slot && !slot_ok)) && (is_slot || lane == 0))
    *bad_state = 1u;
  const bool run = is_slot && slot_ok && bank_ok;   // (the other lanes go along: they complete nothing, their states stay)

  // 1 the records: k_weph's recurrence
  const long long base = run ? blocks_seen : 0;
  long long last = run ? last0 : 0;
  u32 done[8], done_id = 0;   // the subframe 4 or 5 that completed in this launch
#pragma unroll
  for (int j = 0; j < 8; j++)
    done[j] = 0;
#pragma unroll
  for (int k = 0; k < kMaxWords; k++) {
    const int end_block = (int)wd[k].a;
    const u32 index = wd[k].c & 0xFFu, wflags = (wd[k].c >> 8) & 0xFFu, sub_id = (wd[k].c >> 16) & 0xFFu, aux = wd[k].d;
    const long long e1 = base + end_block + 1;
    if (!(k < max_words && (wflags & GPSX_WNAV_WORD) && index >= 1u && index <= 10u && end_block >= -600 && end_block < n_blocks && e1 >= 1))
      continue;
    const bool passed = (wflags & GPSX_WNAV_OK) && (index != 2u || (sub_id >= 1u && sub_id <= 5u && aux < kTowCounts));
    if (index == 1u) {
      cur_mask = passed ? 1u : 0u;
      cur_next = 2u;
      cur_id = 0u;
    } else if (index == cur_next && e1 == last + 600) {
      if (passed) {
        cur_mask |= 1u << (index - 1u);
        if (index == 2u)
          cur_id = sub_id;
        const u32 data = (wd[k].b >> 6) & 0xFFFFFFu;
#pragma unroll
        for (int j = 0; j < 8; j++)
          cur[j] = index == (u32)(j + 3) ? data : cur[j];
      }
      cur_next = index == 10u ? 0u : index + 1u;
      if (index == 10u && cur_mask == 0x3FFu && cur_id >= 4u) {
        done_id = cur_id;
#pragma unroll
        for (int j = 0; j < 8; j++)
          done[j] = cur[j];
      }
    } else {
      cur_next = 0u;
      cur_mask = 0u;
    }
    last = e1;
  }
  if (run) {
    const u64 seen = (u64)(base + n_blocks), l = (u64)last;
    Quad *dst = reinterpret_cast<Quad *>(st + c);
    dst[0] = Quad{(u32)seen, (u32)(seen >> 32), (u32)l, (u32)(l >> 32)};
    dst[1] = Quad{cur[0], cur[1], cur[2], cur[3]};
    dst[2] = Quad{cur[4], cur[5], cur[6], cur[7]};
    dst[3] = Quad{cur_mask, cur_next, cur_id, 0u};
  }

  // ... where a complete subframe goes: an entry, or nowhere
  int entry = -1;
  {
    const u32 data_id = take<60, 2>(done), sv = take<62, 6>(done), toa = take<90, 8>(done);
    const bool almanac = toa <= kToaMax && (done_id == 5u ? sv >= 1u && sv <= 24u : sv >= 25u && sv <= 32u);
    entry = almanac ? (int)sv - 1 : entry;
    entry = done_id == 4u && sv == 56u ? kPage18 : entry;
    entry = done_id == 5u && sv == 51u ? kPage25 : entry;
    entry = data_id == 1u ? entry : -1;
  }
  const bool complete = run && done_id != 0u;
  const u64 commits = __ballot(complete && entry >= 0);
  const u32 n_other = (u32)__popcll(__ballot(complete && entry < 0));

  // 2 the commits: lane e is entry e
  u32 page[8];
#pragma unroll
  for (int j = 0; j < 8; j++)
    page[j] = before[j];
  bool seen_e = false;
  u64 todo = commits;                                              // (wave-uniform: a ballot)
#pragma unroll 1
  while (todo != 0) {
    const int j = __ffsll((long long)todo) - 1;
    todo &= todo - 1ull;
    const bool mine = (int)lane_word((u32)entry, j) == lane;      // (an entry is below 34: lanes from 34 on never match)
    seen_e = seen_e || mine;
#pragma unroll
    for (int w = 0; w < 8; w++) {
      const u32 v = lane_word(done[w], j);
      page[w] = mine ? v : page[w];
    }
  }
  bool differs = false;
#pragma unroll
  for (int w = 0; w < 8; w++)
    differs = differs || page[w] != before[w];
  const bool held0 = is_entry && ((have0 >> lane) & 1ull) != 0;
  const bool is_new = seen_e && (!held0 || differs);
  const u64 seen_mask = __ballot(seen_e), new_mask = __ballot(is_new), have_mask = bank_ok ? have0 | seen_mask : 0ull;
  const u32 n_stored = (u32)__popcll(commits);
  if (is_entry && differs) {
    Quad *dst = reinterpret_cast<Quad *>(bk->page[lane]);
    dst[0] = Quad{page[0], page[1], page[2], page[3]};
    dst[1] = Quad{page[4], page[5], page[6], page[7]};
  }
  if (lane == 0 && (n_stored | n_other) != 0u) {
    Quad *dst = reinterpret_cast<Quad *>(&bk->have_mask);
    dst[0] = Quad{(u32)have_mask, (u32)(have_mask >> 32), bank_stored + n_stored, bank_changed + (u32)__popcll(new_mask)};
    dst[1] = Quad{bank_other + n_other, 0u, 0u, 0u};
  }

  // 3 the records: pages 18 and 25 to every lane (scalars), lanes 0 .. 31 their SV
  u32 p18[8], p25[8];
#pragma unroll
  for (int w = 0; w < 8; w++) {
    p18[w] = lane_word(page[w], kPage18);
    p25[w] = lane_word(page[w], kPage25);
  }
  const bool has18 = ((have_mask >> kPage18) & 1ull) != 0, has25 = ((have_mask >> kPage25) & 1ull) != 0;   // (a BAD bank: neither)
  const bool held = lane < 32 && ((have_mask >> lane) & 1ull) != 0;
  const u32 svh = take<136, 8>(page), toa = take<90, 8>(page);
  const bool healthy = held && svh == 0u, week_ok = held && has25 && toa == take<68, 8>(p25);
  const int wna = week8(take<76, 8>(p25));
  const u64 healthy_mask = __ballot(healthy), week_mask = __ballot(week_ok);

  if (alm && lane < 32) {
    gpsx_walm_sv_t o = gpsx_walm_sv_t{};
    if (held) {
      o.flags = GPSX_WALM_HELD | (week_ok ? GPSX_WALM_WEEK : 0u) | (healthy ? GPSX_WALM_HEALTHY : 0u) | (is_new ? GPSX_WALM_NEW : 0u);
      o.svid = (int)take<62, 6>(page);
      o.svh = (int)svh;
      o.week = week_ok ? wna : 0;
      o.toas = (double)(toa * 4096u);
      o.e = (double)take<68, 16>(page) * 0x1p-21;
      const double root_a = (double)take<150, 24>(page) * 0x1p-11;
      o.A = root_a * root_a;
      const double di = (double)as_int<16>(take<98, 16>(page)) * 0x1p-19;
      const double i_sc = 0.3 + di;
      o.i0 = i_sc * kSemiCircle;
      o.OMG0 = (double)as_int<24>(take<180, 24>(page)) * 0x1p-23 * kSemiCircle;
      o.omg = (double)as_int<24>(take<210, 24>(page)) * 0x1p-23 * kSemiCircle;
      o.M0 = (double)as_int<24>(take<240, 24>(page)) * 0x1p-23 * kSemiCircle;
      o.OMGd = (double)as_int<16>(take<120, 16>(page)) * 0x1p-38 * kSemiCircle;
      o.f0 = (double)as_int<11>(take<270, 8>(page) << 3 | take<289, 3>(page)) * 0x1p-20;
      o.f1 = (double)as_int<11>(take<278, 11>(page)) * 0x1p-38;
    }
    const Quad *src = reinterpret_cast<const Quad *>(&o);
    Quad *dst = reinterpret_cast<Quad *>(alm + ((size_t)r * 32u + (size_t)lane));
#pragma unroll
    for (int k = 0; k < 6; k++)
      dst[k] = src[k];
  }

  if (lane == 0) {
    gpsx_walm_rx_t o = gpsx_walm_rx_t{};
    if (bank_ok) {
      o.flags = (has18 ? GPSX_WALM_IONUTC : 0u) | (has25 ? GPSX_WALM_PAGE25 : 0u);
      o.n_stored = n_stored;
      o.have_mask = have_mask;
      o.new_mask = new_mask;
      o.seen_mask = seen_mask;
      o.healthy_mask = (u32)healthy_mask;
      o.week_mask = (u32)week_mask;
    }
    if (has25) {
      const u32 h[6] = {p25[1], p25[2], p25[3], p25[4], p25[5], p25[6]};   // words 4 .. 9: four six-bit health words each
      u32 unhealthy = 0;
#pragma unroll
      for (int n = 0; n < 24; n++)
        unhealthy |= ((h[n / 4] >> (18 - 6 * (n % 4))) & 63u) != 0u ? 1u << n : 0u;
      o.p25_unhealthy_mask = unhealthy;
      o.toa_s = (int)(take<68, 8>(p25) * 4096u);
      o.wna = wna;
    }
    if (has18) {
      o.tot_s = (int)(take<218, 8>(p18) * 4096u);
      o.wnt = week8(take<226, 8>(p18));
      o.dt_ls = as_int<8>(take<240, 8>(p18));
      o.wn_lsf = week8(take<248, 8>(p18));
      o.dn = (int)take<256, 8>(p18);
      o.dt_lsf = as_int<8>(take<270, 8>(p18));
      o.A0 = (double)as_int<32>(take<180, 24>(p18) << 8 | take<210, 8>(p18)) * 0x1p-30;
      o.A1 = (double)as_int<24>(take<150, 24>(p18)) * 0x1p-50;
      o.ion[0] = (double)as_int<8>(take<68, 8>(p18)) * 0x1p-30;
      o.ion[1] = (double)as_int<8>(take<76, 8>(p18)) * 0x1p-27;
      o.ion[2] = (double)as_int<8>(take<90, 8>(p18)) * 0x1p-24;
      o.ion[3] = (double)as_int<8>(take<98, 8>(p18)) * 0x1p-24;
      o.ion[4] = (double)as_int<8>(take<106, 8>(p18)) * 0x1p11;
      o.ion[5] = (double)as_int<8>(take<120, 8>(p18)) * 0x1p14;
      o.ion[6] = (double)as_int<8>(take<128, 8>(p18)) * 0x1p16;
      o.ion[7] = (double)as_int<8>(take<136, 8>(p18)) * 0x1p16;
    }
    const Quad *src = reinterpret_cast<const Quad *>(&o);
    Quad *dst = reinterpret_cast<Quad *>(rx + r);
#pragma unroll
    for (int k = 0; k < 10; k++)
      dst[k] = src[k];
  }
}

void launch_walm(hipStream_t s, const gpsx_walm_cfg_t &cfg, const gpsx_wnav_word_t *d_words, int n_blocks, int n_rx, gpsx_walm_slot_t *d_slot_st,
                 gpsx_walm_bank_t *d_bank, gpsx_walm_rx_t *d_rx, gpsx_walm_sv_t *d_alm, uint32_t *d_bad_state)
{
  // (no checks of its own: gpsx_api_wtrack.hip's walm() is the one list of what a launch needs and refuses with a text before it comes here)
  hipLaunchKernelGGL(k_walm, dim3(((unsigned)n_rx + 3u) / 4u), dim3(256), 0, s, d_words, n_blocks / 600 + 2, n_blocks, cfg.ch_per_rx, n_rx, d_slot_st,
                     d_bank, d_rx, d_alm, d_bad_state);
}

}  // namespace gpsx
