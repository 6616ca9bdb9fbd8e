// k_weph.hip -- EXTENSION, not in the reference: every channel's broadcast ephemeris from the word records of the word layer
// (include/gpsx.h gpsx_weph): subframes assembled across launches, the newest complete subframes 1, 2 and 3 kept,
// and -- when the three are of one issue of data -- decoded as gps_nav_data_decode_subframe (gpsx_ephemeris.cpp) decodes them.
//
// k_wobs' shape: one channel per lane, 64 lanes per workgroup.  A lane reads at most eight word records (one 16-byte load each, all
// in flight before the first is looked at) and its 192-byte state, a per-lane struct access, strided.  The 256-byte records leave
// through LDS: a lane puts its own there, and each of the wave's sixteen store instructions then covers 1 KiB of consecutive
// addresses, four whole records (16 % faster at 212 992 channels than sixteen strided stores per lane: EXPERIMENTS.md).
// cur[] and sf[][] are indexed by data (the word's index, the subframe's ID): they live in registers and every such access is a
// chain of selects over constant indices, so that nothing goes to scratch.  A launch holds at most eight records and a subframe has
// ten: at most one subframe completes per launch, so the words it completed with are set aside in the loop and committed once behind it.
// The decoder's doubles: an integer conversion and one or two IEEE multiplies per field, in the decoder's order (-ffp-contract=off:
// there is no sum behind a product here anyway); its scale factors are the decoder's decimal literals.
#include <hip/hip_runtime.h>

#include <cstddef>

#include "gpsx_device.hpp"
#include "gpsx_kernels.hpp"
#include "gpsx_wstage_parts.hpp"

namespace gpsx {

namespace {

static_assert(sizeof(gpsx_weph_cfg_t) == 8, "gpsx_weph_cfg_t layout");
static_assert(sizeof(gpsx_weph_state_t) == 192 && offsetof(gpsx_weph_state_t, blocks_seen) == 0 && offsetof(gpsx_weph_state_t, last_word_end_p1) == 8 &&
              offsetof(gpsx_weph_state_t, cur) == 16 && offsetof(gpsx_weph_state_t, cur_mask) == 48 && offsetof(gpsx_weph_state_t, cur_next) == 52 &&
              offsetof(gpsx_weph_state_t, cur_id) == 56 && offsetof(gpsx_weph_state_t, cur_tow) == 60 && offsetof(gpsx_weph_state_t, sf) == 64 &&
              offsetof(gpsx_weph_state_t, sf_tow) == 160 && offsetof(gpsx_weph_state_t, have) == 172 && offsetof(gpsx_weph_state_t, flags) == 176 &&
              offsetof(gpsx_weph_state_t, n_sets) == 180 && offsetof(gpsx_weph_state_t, n_subframes) == 184 && offsetof(gpsx_weph_state_t, reserved) == 188,
              "gpsx_weph_state_t layout");
static_assert(sizeof(gpsx_weph_t) == 256 && offsetof(gpsx_weph_t, flags) == 0 && offsetof(gpsx_weph_t, iode) == 4 && offsetof(gpsx_weph_t, flag) == 28 &&
              offsetof(gpsx_weph_t, toe_time) == 32 && offsetof(gpsx_weph_t, toe_sec) == 56 && offsetof(gpsx_weph_t, A) == 80 &&
              offsetof(gpsx_weph_t, tgd) == 240 && offsetof(gpsx_weph_t, n_sets) == 248 && offsetof(gpsx_weph_t, have) == 252, "gpsx_weph_t layout");

constexpr int kMaxWords = 4096 / 600 + 2;    // word slots of the longest launch
constexpr long long kMaxCount = 1ll << 62;
constexpr u32 kTowCounts = 100800u;          // six-second counts of a week

struct alignas(16) Quad { u32 a, b, c, d; };   // a word record as one global_load_dwordx4

// the decoder's constants (gpsx_ephemeris.cpp)
constexpr double kSemiCircle = 3.1415926535898;
constexpr int kBuildWeek = 2290;
constexpr long long kUnixToGps = 315964800ll;
constexpr double kP4 = 16.0, kM5 = 0.03125, kM19 = 1.907348632812500E-06, kM29 = 1.862645149230957E-09, kM31 = 4.656612873077393E-10,
                 kM33 = 1.164153218269348E-10, kM43 = 1.136868377216160E-13, kM55 = 2.775557561562891E-17;

// `len` bits from subframe bit `pos`, first bit most significant, out of the eight words 3 .. 10 (d1 in bit 23): bit n lies in word
// n / 30, and a run never leaves its word's 24 source bits
template <int pos, int len>
__device__ __forceinline__ u32 take(const u32 (&w)[8])
{
  static_assert(pos >= 60 && pos % 30 + len <= 24 && len >= 1 && len <= 24, "a run inside one word's source bits");
  return (w[pos / 30 - 2] >> (24 - pos % 30 - len)) & ((1u << len) - 1u);
}
template <int len>
__device__ __forceinline__ double as_signed(u32 raw)   // two's complement of `len` bits (len 32: the word itself)
{
  return (double)(int)(len < 32 && (raw >> (len - 1)) ? raw | (~0u << (len & 31)) : raw);
}
template <int p1, int p2>
__device__ __forceinline__ u32 take_8_24(const u32 (&w)[8]) { return take<p1, 8>(w) << 24 | take<p2, 24>(w); }

struct Time { long long time; double sec; };
__device__ __forceinline__ Time gps_time(int week, double sec)   // the decoder's, with its (int)sec split
{
  if (sec < -1e9 || 1e9 < sec)
    sec = 0.0;
  return Time{kUnixToGps + (long long)(86400 * 7 * week + (int)sec), sec - (int)sec};
}

}  // namespace

__global__ __launch_bounds__(64) void k_weph(const gpsx_wnav_word_t *__restrict__ words, int max_words, int n_blocks,
                                             gpsx_weph_state_t *__restrict__ st, int n_ch, gpsx_weph_t *__restrict__ eph,
                                             u32 *__restrict__ bad_state)
{
  const int lane = threadIdx.x;
  const int ch0 = (int)blockIdx.x * 64;
  const bool active = lane < n_ch - ch0;
  const int ch = active ? ch0 + lane : n_ch - 1;   // (always a channel below n_ch: the idle lanes of the last wave load, nothing else)

  // the word records, all in flight before the first is looked at; slots past the launch's last repeat it (in bounds, not stepped through)
  Quad wd[kMaxWords];
#pragma unroll
  for (int k = 0; k < kMaxWords; k++)
    wd[k] = *reinterpret_cast<const Quad *>(words + ((size_t)min(k, max_words - 1) * (size_t)n_ch + (size_t)ch));
  const gpsx_weph_state_t s0 = st[ch];

  bool valid = (u64)s0.blocks_seen <= (u64)kMaxCount && (u64)s0.last_word_end_p1 <= (u64)kMaxCount && s0.cur_next <= 10u && s0.cur_next != 1u &&
               s0.cur_mask <= 0x3FFu && s0.cur_id <= 5u && s0.cur_tow < kTowCounts && s0.have <= 7u && (s0.flags & ~GPSX_WEPH_VALID) == 0 &&
               (!(s0.flags & GPSX_WEPH_VALID) || s0.have == 7u) && s0.reserved == 0;
  u32 cur[8], sf[3][8], sf_tow[3];
  u32 all = 0;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    cur[j] = s0.cur[j];
    all |= cur[j];
  }
#pragma unroll
  for (int k = 0; k < 3; k++) {
    sf_tow[k] = s0.sf_tow[k];
    valid = valid && sf_tow[k] < kTowCounts;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      sf[k][j] = s0.sf[k][j];
      all |= sf[k][j];
    }
  }
  valid = valid && all < (1u << 24);
  if (active && !valid && bad_state)
    *bad_state = 1u;
  const bool run = active && valid;   // (the other lanes go along to the stores: their records are zero, their states stay)

  // the records
  const long long base = run ? s0.blocks_seen : 0;
  long long last = run ? s0.last_word_end_p1 : 0;
  u32 cur_mask = s0.cur_mask, cur_next = s0.cur_next, cur_id = s0.cur_id, cur_tow = s0.cur_tow, n_subframes = s0.n_subframes;
  u32 done[8], done_id = 0, done_tow = 0;   // the subframe that completed in this launch (done_id 1 .. 3: to be committed)
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
      cur_id = cur_tow = 0u;
    } else if (index == cur_next && e1 == last + 600) {
      if (passed) {
        cur_mask |= 1u << (index - 1u);
        if (index == 2u) {
          cur_id = sub_id;
          cur_tow = aux;
        }
        const u32 data = (wd[k].b >> 6) & 0xFFFFFFu;
#pragma unroll
        for (int j = 0; j < 8; j++)
          cur[j] = index == (u32)(j + 3) ? data : cur[j];
      }
      cur_next = index == 10u ? 0u : index + 1u;
      if (index == 10u && cur_mask == 0x3FFu) {
        n_subframes++;
        done_id = cur_id;
        done_tow = cur_tow;
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

  // the commit
  u32 have = s0.have, flags = s0.flags, n_sets = s0.n_sets, is_new = 0u;
  if (done_id >= 1u && done_id <= 3u) {
    const u32 k = done_id - 1u;
    bool changed = !((have >> k) & 1u);
#pragma unroll
    for (int i = 0; i < 3; i++) {
      const bool here = k == (u32)i;
#pragma unroll
      for (int j = 0; j < 8; j++) {
        changed = changed || (here && sf[i][j] != done[j]);
        sf[i][j] = here ? done[j] : sf[i][j];
      }
      sf_tow[i] = here ? done_tow : sf_tow[i];
    }
    have |= 1u << k;
    const bool consistent = have == 7u && (sf[1][0] >> 16) == (sf[2][7] >> 16) && (sf[1][0] >> 16) == (sf[0][5] >> 16);
    if (consistent) {
      if (!(flags & GPSX_WEPH_VALID) || changed) {
        n_sets++;
        is_new = GPSX_WEPH_NEW;
      }
      flags |= GPSX_WEPH_VALID;
    } else {
      flags &= ~GPSX_WEPH_VALID;
    }
  }

  gpsx_weph_state_t s;
  s.blocks_seen = base + n_blocks;
  s.last_word_end_p1 = last;
#pragma unroll
  for (int j = 0; j < 8; j++)
    s.cur[j] = cur[j];
  s.cur_mask = cur_mask; s.cur_next = cur_next; s.cur_id = cur_id; s.cur_tow = cur_tow;
#pragma unroll
  for (int i = 0; i < 3; i++) {
#pragma unroll
    for (int j = 0; j < 8; j++)
      s.sf[i][j] = sf[i][j];
    s.sf_tow[i] = sf_tow[i];
  }
  s.have = have; s.flags = flags; s.n_sets = n_sets; s.n_subframes = n_subframes; s.reserved = 0;
  if (run)
    st[ch] = s;

  // the record: subframes 1, 2, 3 as the decoder reads them, in this order
  gpsx_weph_t o = gpsx_weph_t{};
  if (run) {
    o.flags = flags | is_new;
    o.n_sets = n_sets;
    o.have = have;
  }
  if (run && (flags & GPSX_WEPH_VALID)) {
    const u32(&s1)[8] = sf[0], (&s2)[8] = sf[1], (&s3)[8] = sf[2];
    // subframe 1
    const int week10 = (int)take<60, 10>(s1) + 1024;
    o.code = (int)take<70, 2>(s1);
    o.sva = (int)take<72, 4>(s1);
    o.svh = (int)take<76, 6>(s1);
    o.flag = (int)take<90, 1>(s1);
    o.tgd = as_signed<8>(take<196, 8>(s1)) * kM31;
    o.f2 = as_signed<8>(take<240, 8>(s1)) * kM55;
    o.f1 = as_signed<16>(take<248, 16>(s1)) * kM43;
    o.f0 = as_signed<22>(take<270, 22>(s1)) * kM31;
    o.iodc = (int)((take<82, 2>(s1) << 8) + take<210, 8>(s1));
    const double toc = (double)take<218, 16>(s1) * 16.0;
    o.week = week10 + (kBuildWeek - week10 + 512) / 1024 * 1024;
    const Time ttr = gps_time(o.week, (double)sf_tow[0] * 6.0), t_oc = gps_time(o.week, toc);
    o.ttr_time = ttr.time; o.ttr_sec = ttr.sec;
    o.toc_time = t_oc.time; o.toc_sec = t_oc.sec;
    // subframe 2
    o.crs = as_signed<16>(take<68, 16>(s2)) * kM5;
    o.deln = as_signed<16>(take<90, 16>(s2)) * kM43 * kSemiCircle;
    o.M0 = as_signed<32>(take_8_24<106, 120>(s2)) * kM31 * kSemiCircle;
    o.cuc = as_signed<16>(take<150, 16>(s2)) * kM29;
    o.e = (double)take_8_24<166, 180>(s2) * kM33;
    o.cus = as_signed<16>(take<210, 16>(s2)) * kM29;
    o.toes = (double)take<270, 16>(s2) * kP4;
    o.fit = (double)take<286, 1>(s2);
    const double sqrt_a = (double)take_8_24<226, 240>(s2) * kM19;
    o.A = sqrt_a * sqrt_a;
    const Time toe = gps_time(o.week, o.toes);
    o.toe_time = toe.time; o.toe_sec = toe.sec;
    // subframe 3 (its IODE is the one that stays)
    o.cic = as_signed<16>(take<60, 16>(s3)) * kM29;
    o.OMG0 = as_signed<32>(take_8_24<76, 90>(s3)) * kM31 * kSemiCircle;
    o.cis = as_signed<16>(take<120, 16>(s3)) * kM29;
    o.i0 = as_signed<32>(take_8_24<136, 150>(s3)) * kM31 * kSemiCircle;
    o.crc = as_signed<16>(take<180, 16>(s3)) * kM5;
    o.omg = as_signed<32>(take_8_24<196, 210>(s3)) * kM31 * kSemiCircle;
    o.OMGd = as_signed<24>(take<240, 24>(s3)) * kM43 * kSemiCircle;
    o.iode = (int)take<270, 8>(s3);
    o.idot = as_signed<14>(take<278, 14>(s3)) * kM43 * kSemiCircle;
  }
  // the 64 records of the workgroup through LDS: a lane writes its own (rows of 68 dwords: 16-byte aligned, the rows' banks staggered),
  // then every store instruction of the wave covers 1 KiB of consecutive addresses -- four whole records
  __shared__ __attribute__((aligned(16))) u32 stage[64 * 68];
  {
    const uint4 *src = reinterpret_cast<const uint4 *>(&o);
    uint4 *row = reinterpret_cast<uint4 *>(stage + lane * 68);
#pragma unroll
    for (int j = 0; j < 16; j++)
      row[j] = src[j];
  }
  __syncthreads();
  const int rows = min(64, n_ch - ch0);
  uint4 *dst = reinterpret_cast<uint4 *>(eph + ch0);
#pragma unroll
  for (int i = 0; i < 16; i++) {
    const int q = i * 64 + lane;
    if ((q >> 4) < rows)
      dst[q] = *reinterpret_cast<const uint4 *>(stage + (q >> 4) * 68 + (q & 15) * 4);
  }
}

void launch_weph(hipStream_t s, const gpsx_wnav_word_t *d_words, int n_blocks, gpsx_weph_state_t *d_st, int n_ch, gpsx_weph_t *d_eph,
                 uint32_t *d_bad_state)
{
  if (n_ch <= 0 || n_blocks <= 0 || n_blocks > 4096)
    return;
  hipLaunchKernelGGL(k_weph, dim3(((unsigned)n_ch + 63u) / 64u), dim3(64), 0, s, d_words, n_blocks / 600 + 2, n_blocks, d_st, n_ch, d_eph,
                     d_bad_state);
}

}  // namespace gpsx
