// k_acq_mx_byte.hip -- k_acq_mx<4>, the byte-phase form of the matrix-core grid (gpsx_mx_parts.hpp): sample offsets 0 and 8 only,
// each started directly from its own block sums; one persistent workgroup per CU runs its clusters as one software pipeline.
#include "gpsx_mx_parts.hpp"

namespace gpsx {

namespace {

// The byte-phase form's two passes of a stage (low vector at 2^0, high vector at 2^3) as ONE walk over the anti-diagonals: the
// A fragments are fetched once instead of twice, there is no gap between the passes, and every fragment is requested into the
// registers of its predecessor as soon as that one's MFMAs have been issued -- under the twelve MFMAs of the other three streams.
template <int S, int NT>
__device__ __forceinline__ void mx_pass2_step(lds_cu32 *const (&w)[4], const v4i *ca, v4i (&a)[16], v4i (&f)[4], v16f (&acc)[2][NT])
{
  constexpr int kSteps = 16 + NT - 1;
  constexpr bool more = S + 1 < kSteps;
  if constexpr (more && S + 1 < 16)
    a[S + 1] = ca[(S + 1) * 64];                           // chips_a[S + 1][h][n]
  constexpr int j_lo = S - 15 > 0 ? S - 15 : 0, j_hi = S < NT - 1 ? S : NT - 1;
#pragma unroll
  for (int v = 0; v < 4; v++) {   // I low, Q low, I high, Q high
#pragma unroll
    for (int j = j_lo; j <= j_hi; j++)
      acc[v & 1][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(widen(a[S - j]), widen(f[v]), acc[v & 1][j], 4, 4, 0, kScaleA, 0,
                                                                      v < 2 ? kScaleOne : kScaleEight);
    if constexpr (more)
      f[v] = lds_frag(w[v], 8 * (S + 1));
  }
  if constexpr (more) {
    if constexpr (S + 1 < 16)
      __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                 // DS read: the A fragment
#pragma unroll
    for (int v = 0; v < 4; v++) {
      __builtin_amdgcn_sched_group_barrier(0x008, j_hi - j_lo + 1, 0);   // MFMAs of one stream
      __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);                 // DS reads: its next fragment
    }
  }
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (more)
    mx_pass2_step<S + 1, NT>(w, ca, a, f, acc);
}
template <int NT>
__device__ __forceinline__ void mx_pass2(const MxShared &sh, int lane, int q0_tile, v16f (&acc)[2][NT], const u32 *e8_low,
                                         const u32 *e8_high)
{
  const int n = lane & 31, h = lane >> 5;
  const int off = (n & 7) * kCopyDwords + 4 * (q0_tile + h) + (n >> 3);
  lds_cu32 *const w[4] = {lds_opaque(e8_low + off), lds_opaque(e8_low + 8 * kCopyDwords + off), lds_opaque(e8_high + off),
                          lds_opaque(e8_high + 8 * kCopyDwords + off)};
  const v4i *ca = &sh.chips_a[0][h][n];
  v4i a[16];
  v4i f[4] = {lds_frag(w[0], 0), lds_frag(w[1], 0), lds_frag(w[2], 0), lds_frag(w[3], 0)};
  a[0] = ca[0];
  mx_pass2_step<0, NT>(w, ca, a, f, acc);
}

// ---- sample offset 8 started directly, with the odd byte offset's terms in the start values and in ONE extra K step per pass -----
// (the byte-phase form, mx_byte_pipe; the formula is the one in front of mx_half_switch at b = 0, without the A_7 that a walk
//  from the even offsets would have left in the accumulators.)
//   extra(q, p) = - pop(W) - chip_p[1022 - q] beta_0 + T(q) [ (2 c1022_p - 1) S_8[q - 1] - 16 c1022_p ]
// because P = data bytes (2 q - 1, 2 q) IS the block D[16 (q - 1) + 8, +16) whose popcount the offset-8 vectors already carry
// as entry q - 1: the tail word acts as one more chip, "chip -1" = chip 1022 in +-1 form.  So
//   * start values:  base - pop(W)   (mx_init_acc_odd);
//   * - chip_p[1022 - q] beta_0 is entry 1022 of the offset-8 vectors' first period lowered by beta_0 = 16 - 2 pop(W) -- and
//     pop(W) is that entry's own block sum: the entry is the constant -16 (mx_byte_wipe_codes): nothing to compute at all;
//   * per pass one MFMA per tile and stream (mx_odd_tail_steps): A column 0 of lane half 0 = -(2 c1022 - 1) / 2 against nibble
//     q - 1 of the pass's own vector (-2 (S & 3), then -(S >> 2) at 2^3), and in the high pass column 0 of lane half 1 = c1022
//     against -2 at 2^3; both B entries zero for q = 0.
template <int NT>
__device__ __forceinline__ void mx_init_acc_odd(const u32 *ones, const u32 *d_i, const u32 *d_q, int lane, int q0_tile,
                                                v16f (&acc)[2][NT], int win_start, int win_stop)
{
  const int n = lane & 31;
  const float base_i = (float)((int)ones[0] + 8192 - kHalf - (int)__popc(d_i[0] & 0xFFu)) * kAccScale;
  const float base_q = (float)((int)ones[1] + 8192 - kHalf - (int)__popc(d_q[0] & 0xFFu)) * kAccScale;
#pragma unroll
  for (int j = 0; j < NT; j++) {
    const int q = 32 * (q0_tile + 2 * j) + n;
    const bool in1 = q < kChips && 2 * q + 1 >= win_start && 2 * q + 1 < win_stop;
#pragma unroll
    for (int r = 0; r < 16; r++) {
      acc[0][j][r] = in1 ? base_i : base_i + kOutside;
      acc[1][j][r] = in1 ? base_q : base_q + kOutside;
    }
  }
}
// (both passes' extra steps in one go, BEFORE the passes: their operands come from LDS under the start values' moves)
template <int NT>
__device__ __forceinline__ void mx_odd_tail_operands(const u32 *v_low, const u32 *v_high, int lane, int q0_tile, u32 (&b_low)[2][NT],
                                                     u32 (&b_high)[2][NT])
{
  const int n = lane & 31, h = lane >> 5;
#pragma unroll
  for (int j = 0; j < NT; j++) {
    const int q = 32 * (q0_tile + 2 * j) + n;
    const int e = q > 0 ? q - 1 : 0;
    // entry q - 1 of a vector (copy 0, dword e / 8) moved to nibble 0; what is left above it meets zero columns of A
#pragma unroll
    for (int s = 0; s < 2; s++) {
      const u32 lo = v_low[s * 8 * kCopyDwords + (e >> 3)] >> (4 * (e & 7)), hi = v_high[s * 8 * kCopyDwords + (e >> 3)] >> (4 * (e & 7));
      b_low[s][j] = h || q == 0 ? 0u : lo;
      b_high[s][j] = q == 0 ? 0u : h ? 0xCu /* FP4 -2 */ : hi;
    }
  }
}
template <int NT>
__device__ __forceinline__ void mx_odd_tail_steps(const MxShared &sh, int lane, const u32 (&b_low)[2][NT], const u32 (&b_high)[2][NT],
                                                  v16f (&acc)[2][NT])
{
  const int n = lane & 31, h = lane >> 5;
  const u32 c22 = (sh.chip_t[1022 + 1] >> n) & 1u;   // A row n = PRN n of the cluster
  const v4i a_low = v4i{(int)(h ? 0u : c22 ? 0x9u : 0x1u), 0, 0, 0};             // FP4 -0.5 / +0.5
  const v4i a_high = v4i{(int)(h ? c22 << 1 : c22 ? 0x9u : 0x1u), 0, 0, 0};      // lane half 1: 1.0 where chip 1022 is set
#pragma unroll
  for (int j = 0; j < NT; j++)
#pragma unroll
    for (int s = 0; s < 2; s++) {
      acc[s][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(widen(a_low), widen(v4i{(int)b_low[s][j], 0, 0, 0}), acc[s][j], 4, 4, 0,
                                                                  kScaleA, 0, kScaleOne);
      acc[s][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(widen(a_high), widen(v4i{(int)b_high[s][j], 0, 0, 0}), acc[s][j], 4, 4,
                                                                  0, kScaleA, 0, kScaleEight);
    }
}

// ---- the byte-phase grid as ONE software pipeline over the clusters of a persistent workgroup (k_acq_mx<4>) -----------------
// Per cluster and wave two stages -- sample offset 0, sample offset 8, each started from its own block sums: start values, two
// passes on the wave's four q-tiles, an epilogue of 64 hypotheses per lane -- the two waves of a SIMD half a stage apart, one
// barrier per stage.  The clusters follow each other WITHOUT a fill and a drain half stage and without a preamble between them:
// what cluster c + 1 and c + 2 need is made by all eight waves behind the barriers of cluster c's stages, each piece in a buffer
// nobody reads then (mx_byte_pipe).  Two copies of what a stage reads of its block (d), of the sums' bytes and of the result
// slots (sh.part[0] / [6]) by the cluster's parity; three of pop(D).
struct MxBlockRegs {
  u32 v[4];
};
__device__ __forceinline__ MxBlockRegs mx_block_request(const uint8_t *blk, int if_format, int tid)
{
  // thread t: 16-bit words 2 t and 2 t + 1 of the sign plane (1023 exist), as load_sign16 reads them
  MxBlockRegs r;
  const uint16_t *p = reinterpret_cast<const uint16_t *>(blk);
  const bool second = 2 * tid + 1 < kWords16;
  if (if_format == GPSX_IF_2BIT_SM) {
    r.v[0] = p[4 * tid];
    r.v[1] = p[4 * tid + 1];
    r.v[2] = second ? p[4 * tid + 2] : 0;
    r.v[3] = second ? p[4 * tid + 3] : 0;
  } else {
    r.v[0] = p[2 * tid];
    r.v[1] = second ? p[2 * tid + 1] : 0;
    r.v[2] = r.v[3] = 0;
  }
  return r;
}
__device__ __forceinline__ void mx_block_commit(MxShared &sh, const MxBlockRegs &r, int if_format, int tid)
{
  u32 lo = r.v[0], hi = r.v[1];
  if (if_format == GPSX_IF_2BIT_SM) {
    lo = even_bits16(r.v[0] | (r.v[1] << 16));
    hi = even_bits16(r.v[2] | (r.v[3] << 16));
  }
  reinterpret_cast<u32 *>(sh.x)[tid] = (lo & 0xFFFFu) | (hi << 16);
}

// FP4 codes of the two parts of a block sum S = 0 .. 16: -2 (S & 3) -> 0, C, E, F; -(S >> 2) -> 0, A, C, D, E
__device__ __forceinline__ u32 sum_code_low(u32 s) { return (0xFEC0u >> ((s << 2) & 0xCu)) & 0xFu; }
__device__ __forceinline__ u32 sum_code_high(u32 s) { return (0xEDCA0u >> (s & 0x1Cu)) & 0xFu; }

// Table for the wipe-off piece (in the recurrence's lookup tables' LDS, which this form does not use): two block sums
// (a | b << 5, each 0 .. 16) -> the byte of their low codes and, above it, the byte of their high codes
__device__ __forceinline__ void mx_byte_fill_code_table(MxShared &sh, int tid)
{
  uint16_t *lut = reinterpret_cast<uint16_t *>(sh.t_lut);
  static_assert(sizeof(sh.t_lut) >= 1024 * sizeof(uint16_t), "code table fits");
  for (int i = tid; i < 1024; i += kMxThreads) {
    const u32 sa = (u32)i & 31u, sb = (u32)i >> 5;
    lut[i] = (uint16_t)(sum_code_low(sa) | (sum_code_low(sb) << 4) | (sum_code_high(sa) << 8) | (sum_code_high(sb) << 12));
  }
}

// Wipe-off of the block in sh.x -> d[2][514] (word 511 = the wrap-around copy), pop(D) -> ones (zeroed beforehand), and copy 0
// of the four vectors of each stream -- entry k = the FP4 code of a part of the block sum S_t0[k mod 1023], k < 2056 -- as bytes
// of two entries: thread w has word w and wipes word w + 1 a second time (no barrier between the stream and its sums), i.e.
// sums 2 w, 2 w + 1, 2 w + 2 of either sample offset: byte w of the first period, byte 512 + w of the second (which starts at
// the odd entry 1023), and bytes 0..4 again as 1023..1027 (entries from 2046).  Entry 1023 = entry 0.  The four bytes of a
// thread (low / high vector, first / second period) are transposed over its quad, so that each lane writes ONE dword.
__device__ __forceinline__ void mx_byte_wipe_codes(const MxShared &sh, u32 *d, u32 *ones, u32 *base0, u32 *base8, u32 step_word,
                                                   int tid, int lane)
{
  const u32 *x32 = reinterpret_cast<const u32 *>(sh.x);
  const uint16_t *lut = reinterpret_cast<const uint16_t *>(sh.t_lut);
  const int w = tid, k = tid & 3;
  const u32 x_first = x32[0], x_cur = x32[w], x_next = x32[w < 511 ? w + 1 : 0];
  const u32 quad_cur = (step_word * (u32)w) >> 30, quad_next = (step_word * (u32)(w + 1)) >> 30;
  const u32 sel = (u32)k * 0x0101u + 0x0400u;   // v_perm_b32: byte k of the second source, byte k of the first
  // lane k of a quad writes item k: low / high vector (k & 1), first / second period (k >> 1), dword w / 4 of it
  const int item_dword = (k & 1) * 258 + (k >> 1) * 128 + (w >> 2);
  u32 cnt = 0;   // both streams' counts in one register (each below 2^16 per wave)
#pragma unroll
  for (int s = 0; s < 2; s++) {
    const u32 first = (s ? carrier_q(0u) : carrier_i(0u)) ^ x_first;
    const u32 wrap = first << 16;   // samples 16352..16367 are zero, then sample 0 again
    const u32 cur = w < kWords32 ? (s ? carrier_q(quad_cur) : carrier_i(quad_cur)) ^ x_cur : wrap;
    const u32 nxt = w + 1 < kWords32 ? (s ? carrier_q(quad_next) : carrier_i(quad_next)) ^ x_next : (w + 1 == kWords32 ? wrap : 0u);
    d[s * 514 + w] = cur;
    cnt += (w < kWords32 ? (u32)__popc(cur) : 0u) << (16 * s);
    const u32 x8 = __builtin_amdgcn_alignbit(nxt, cur, 8u);
#pragma unroll
    for (int o = 0; o < 2; o++) {
      u32 s0 = pop16(o ? x8 : cur), s1 = (u32)__popc((o ? x8 : cur) >> 16);
      const u32 s2 = pop16(o ? nxt >> 8 : nxt);
      if (o && w == 511) {
        s1 = pop16(first >> 8);   // entry 1023 = entry 0 (offset 0: the wrap word's upper half already is D[0, 16))
        // Offset 8, entry 1022 of the FIRST period (the only one chip 1022 - q ever meets): the odd byte offsets skip the
        // replica word at the wrap (quirk Q3) -- - chip[1022 - q] beta_0 with beta_0 = 16 - 2 pop(W), and pop(W) IS this
        // entry's block sum S_8[1022] = pop(D[0, 8)): entry -2 S - beta_0 = -16 whatever the data, i.e. "S = 8".
        s0 = 8;
      }
      // bytes: [0] low vector, first period; [1] high, first; [2] low, second period; [3] high, second
      const u32 pk = (u32)lut[s0 | (s1 << 5)] | ((u32)lut[s1 | (s2 << 5)] << 16);
      u32 *base = (o ? base8 : base0) + s * (2 * 258);   // [stream][low / high][258 dwords]
      const u32 p0 = (u32)__builtin_amdgcn_mov_dpp((int)pk, 0x00, 0xF, 0xF, true), p1 = (u32)__builtin_amdgcn_mov_dpp((int)pk, 0x55, 0xF, 0xF, true);
      const u32 p2 = (u32)__builtin_amdgcn_mov_dpp((int)pk, 0xAA, 0xF, 0xF, true), p3 = (u32)__builtin_amdgcn_mov_dpp((int)pk, 0xFF, 0xF, 0xF, true);
      const u32 out = (__builtin_amdgcn_perm(p1, p0, sel) & 0xFFFFu) | (__builtin_amdgcn_perm(p3, p2, sel) << 16);
      if (w < 508 || k < 2)
        base[item_dword] = out;
      uint8_t *bytes = reinterpret_cast<uint8_t *>(base);
      if (w >= 508 && w < 511) {   // the last dword of the second period also holds byte 1023, which is entry 2046's
        bytes[512 + w] = (uint8_t)(pk >> 16);
        bytes[258 * 4 + 512 + w] = (uint8_t)(pk >> 24);
      }
      if (w < 5) {
        bytes[1023 + w] = (uint8_t)pk;
        bytes[258 * 4 + 1023 + w] = (uint8_t)(pk >> 8);
      }
    }
  }
  cnt = wave_sum_to_lane63(cnt);
  if (lane == 63) {
    atomicAdd(&ones[0], cnt & 0xFFFFu);
    atomicAdd(&ones[1], cnt >> 16);
  }
}

// the low and the high vector of one sample offset: the eight shifted copies of each from its copy 0
__device__ __forceinline__ void mx_byte_vector_pair(const u32 *base, u32 *dst_low, u32 *dst_high, int tid)
{
  const int iq = tid >> 8, j = tid & 255;
#pragma unroll
  for (int which = 0; which < 2; which++) {
    const u32 *v = base + (iq * 2 + which) * 258 + j;
    const u32 lo = v[0], hi = v[1];
    u32 *dst = (which ? dst_high : dst_low) + (iq * 8) * kCopyDwords + j;
#pragma unroll
    for (int c = 0; c < 8; c++)
      dst[c * kCopyDwords] = c ? __builtin_amdgcn_alignbit(hi, lo, 4u * (u32)c) : lo;
  }
}

// the triplets of one cluster from result slots `slots` of sh.part (bit shift 0 only), and the slots back to zero: thread
// (which, PRN, eighth) folds four lane slots, the eight threads of a PRN meet over DPP / permutes
__device__ __forceinline__ void mx_byte_fold(MxShared &sh, int slots, u32 group_mask, int set, int search, int dopp,
                                             const AcqParams &prm, gpsx_peak_t *__restrict__ peaks, int tid)
{
  const int which = tid >> 8, p = (tid >> 3) & 31, part = tid & 7;
  uint4 *row = reinterpret_cast<uint4 *>(&sh.part[slots][p][which][4 * part]);
  const uint4 v = *row;
  *row = make_uint4(0, 0, 0, 0);
  u32 k = max(max(v.x, v.y), max(v.z, v.w)), t = v.x + v.y + v.z + v.w;
  // the eight lanes of a PRN: neighbours, pairs (quad permutes), then the other half of the eight (mirrored: all four alike by then)
#define MX_FOLD8(ctrl)                                                                          \
  {                                                                                             \
    const u32 ko = (u32)__builtin_amdgcn_mov_dpp((int)k, ctrl, 0xF, 0xF, true);                 \
    const u32 to = (u32)__builtin_amdgcn_mov_dpp((int)t, ctrl, 0xF, 0xF, true);                 \
    k = ko > k ? ko : k;                                                                        \
    t += to;                                                                                    \
  }
  MX_FOLD8(0xB1)    // quad_perm [1, 0, 3, 2]
  MX_FOLD8(0x4E)    // quad_perm [2, 3, 0, 1]
  MX_FOLD8(0x141)   // row_half_mirror
#undef MX_FOLD8
  const int slot = 32 * set + p;
  if (part == 0 && ((group_mask >> (p >> 3)) & 1u) && slot < prm.n_prn) {
    const size_t idx = ((size_t)(search * prm.n_prn + slot) * prm.n_dopp + dopp) * prm.n_bits;
    uint2 *pk = reinterpret_cast<uint2 *>(&peaks[idx]);
    if (which == 0) {
      const u32 max_val = k >> 11, phase = max_val ? 2047u - (k & 2047u) : 0u;
      pk[0] = make_uint2(max_val, phase);                                // gpsx_peak_t: max_val, phase
      if (prm.keys)   // (the packed key k_acq_keys would make of it: one bit shift)
        prm.keys[idx] = (int64_t)(((unsigned long long)max_val << 14) | (unsigned long long)(16383u - 8u * phase));
    } else {
      pk[1] = make_uint2(t, t / (2u * kChips));                          //              sum, avr
    }
  }
}

__device__ __forceinline__ void mx_byte_pipe(MxShared &sh, const AcqParams &prm, int cluster_lo,
                                             const uint8_t *__restrict__ if_blocks, const u32 *__restrict__ mx_a,
                                             const u32 *__restrict__ mx_t, gpsx_peak_t *__restrict__ peaks)
{
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int role = wave >> 2;                            // waves w and w + 4 share a SIMD: half a stage apart
  const int q0_tile = 8 * (wave >> 1) + (wave & 1);      // this wave owns q-tiles q0_tile + 2 j
  const int n_sets = (prm.n_groups + 3) / 4;
  const int stride = (int)gridDim.x, first = cluster_lo + (int)blockIdx.x;
  const int n_my = (prm.n_clusters - (int)blockIdx.x + stride - 1) / stride;   // clusters first, first + stride, ...: >= 1
  if (n_my <= 0)                                         // (a grid larger than the launch's clusters: the launcher never makes one)
    return;
  const int set = first % n_sets;                        // (the launcher's grid is a multiple of n_sets: one PRN set per workgroup)
  const size_t block_bytes = prm.if_format == GPSX_IF_2BIT_SM ? GPSX_BYTES_PER_MS_2BIT : kBytes;

  // LDS this form has to itself: the polyphase planes (second copy of d, three of ones), the lookup tables (code table, step
  // table), and of the result slots of bit shifts 1..7: the offset-8 vectors, behind them copy 0 of the vectors as the wipe-off
  // piece leaves them ([offset 0 | offset 8 of even / odd clusters][stream][low / high][258 dwords]), slot 7 = odd clusters' results
  u32 *d_alt = &sh.plane[0][0][0], *ones3 = d_alt + 2 * 514;   // ones3[3][2]
  static_assert(sizeof(sh.plane) >= (2 * 514 + 6) * sizeof(u32), "overlays fit");
  u32 *e8x = &sh.part[1][0][0][0];
  constexpr int kVec = 2 * 8 * kCopyDwords, kBase = 2 * 2 * 258, kSlotsEven = 0, kSlotsOdd = 7;
  u32 *bbase = e8x + 2 * kVec;
  static_assert((2 * kVec + 3 * kBase) * sizeof(u32) <= 6 * sizeof(sh.part[0]), "two vectors and three sets of their copy 0 below result slots 7");

  // (search, Doppler bin) of this workgroup's clusters c - 1 .. c + 2 around the cluster c the pieces are at: moved on by
  // additions, one division when the workgroup starts (a cluster's pieces need three decodes; divisions cost them a third)
  const int sd_step = stride / n_sets, search_step = sd_step / prm.n_dopp, dopp_step = sd_step % prm.n_dopp;
  int w_sd[4], w_search[4], w_dopp[4], w_at = 0;   // [k]: cluster w_at - 1 + k
  w_sd[1] = first / n_sets;
  w_search[1] = w_sd[1] / prm.n_dopp;
  w_dopp[1] = w_sd[1] % prm.n_dopp;
  w_sd[0] = w_sd[1], w_search[0] = w_search[1], w_dopp[0] = w_dopp[1];
#pragma unroll
  for (int k = 2; k < 4; k++) {
    w_sd[k] = w_sd[k - 1] + sd_step;
    w_dopp[k] = w_dopp[k - 1] + dopp_step;
    w_search[k] = w_search[k - 1] + search_step + (w_dopp[k] >= prm.n_dopp ? 1 : 0);
    w_dopp[k] -= w_dopp[k] >= prm.n_dopp ? prm.n_dopp : 0;
  }
  auto window_to = [&](int c) {   // (at most one step per call)
    if (w_at < c) {
#pragma unroll
      for (int k = 0; k < 3; k++)
        w_sd[k] = w_sd[k + 1], w_search[k] = w_search[k + 1], w_dopp[k] = w_dopp[k + 1];
      w_sd[3] = w_sd[2] + sd_step;
      w_dopp[3] = w_dopp[2] + dopp_step;
      w_search[3] = w_search[2] + search_step + (w_dopp[3] >= prm.n_dopp ? 1 : 0);
      w_dopp[3] -= w_dopp[3] >= prm.n_dopp ? prm.n_dopp : 0;
      w_at++;
    }
  };
  auto decode = [&](int i, int &search, int &dopp, u32 &mask) {   // i in w_at - 1 .. w_at + 2
    const int k = i - w_at + 1;
    const int sd = k == 0 ? w_sd[0] : k == 1 ? w_sd[1] : k == 2 ? w_sd[2] : w_sd[3];
    search = k == 0 ? w_search[0] : k == 1 ? w_search[1] : k == 2 ? w_search[2] : w_search[3];
    dopp = k == 0 ? w_dopp[0] : k == 1 ? w_dopp[1] : k == 2 ? w_dopp[2] : w_dopp[3];
    mask = 0;
#pragma unroll
    for (int g = 0; g < 4; g++) {
      const int group = 4 * set + g, unit = sd * prm.n_groups + group;
      if (group < prm.n_groups && unit >= prm.unit_lo && unit < prm.unit_hi)
        mask |= 1u << g;
    }
  };
  auto block_of = [&](int i) {
    int search, dopp;
    u32 mask;
    decode(i, search, dopp, mask);
    return if_blocks + (size_t)(search * prm.search_stride_blocks) * block_bytes;
  };
  // the carrier's step per 32-sample word for the first 256 Doppler bins (one correctly rounded division each: once per
  // workgroup instead of once per cluster, where everything in the wipe-off piece waits for it); behind the code table
  u32 *step_tab = sh.t_lut + 512;
  static_assert(sizeof(sh.t_lut) >= (512 + 256) * sizeof(u32), "step table fits");
  auto step_of_bin = [&](int dopp) {
    return mx_step_word(dopp, prm.if_hz, prm.dopp_min_hz, prm.dopp_step_hz);
  };
  auto step_of = [&](int i) {
    int search, dopp;
    u32 mask;
    decode(i, search, dopp, mask);
    return dopp < 256 ? step_tab[dopp] : step_of_bin(dopp);
  };
  auto d_of = [&](int i) { return i & 1 ? d_alt : &sh.d[0][0]; };
  auto ones_of = [&](int i) { return ones3 + 2 * (i % 3); };
  u32 *base0 = bbase;
  auto base8_of = [&](int i) { return bbase + (1 + (i & 1)) * kBase; };

  // ---- fill: tables of the PRN set, cluster 0 up to its offset-0 vectors, cluster 1's block in LDS ------------------------------
  {
    MxBlockRegs b0 = mx_block_request(block_of(0), prm.if_format, tid);
    MxBlockRegs b1 = n_my > 1 ? mx_block_request(block_of(1), prm.if_format, tid) : b0;
    mx_load_tables(sh, mx_a, mx_t, set, tid);
    constexpr int kSlotVecs = (int)(sizeof(sh.part[0]) / sizeof(uint4));
    for (int i = tid; i < 2 * kSlotVecs; i += kMxThreads)
      reinterpret_cast<uint4 *>(&sh.part[i / kSlotVecs ? kSlotsOdd : kSlotsEven][0][0][0])[i % kSlotVecs] = make_uint4(0, 0, 0, 0);
    mx_byte_fill_code_table(sh, tid);
    if (tid < 256 && tid < prm.n_dopp)
      step_tab[tid] = step_of_bin(tid);
    if (tid < 6)
      ones3[tid] = 0;
    if (tid < 4) {   // the zero pad behind the wrap-around word, both copies
      sh.d[tid >> 1][512 + (tid & 1)] = 0;
      d_alt[(tid >> 1) * 514 + 512 + (tid & 1)] = 0;
    }
    mx_block_commit(sh, b0, prm.if_format, tid);
    __syncthreads();
    mx_byte_wipe_codes(sh, d_of(0), ones_of(0), base0, base8_of(0), step_of(0), tid, lane);
    __syncthreads();
    mx_byte_vector_pair(base0, &sh.e8[0][0][0][0], &sh.e8[1][0][0][0], tid);
    mx_block_commit(sh, b1, prm.if_format, tid);
  }
  u32 kq[kMxTiles];   // 2047 - (even byte offset of the lane's chip offset in tile j): the low field of its search keys
#pragma unroll
  for (int j = 0; j < kMxTiles; j++)
    kq[j] = (u32)(2047 - 2 * (32 * (q0_tile + 2 * j) + (lane & 31)));

  // Half stages: per cluster four -- passes of sample offset 0 (start values, two passes on the wave's four q-tiles), its epilogue
  // (64 hypotheses per lane), passes of offset 8 (with the odd offset's extra K step), its epilogue; role 1 one half stage
  // behind role 0.  One barrier per stage, i.e. two per cluster, and behind them by everybody (c = the cluster role 0 is in):
  //   start of the offset-0 stage:  the offset-8 vectors of c (read until the half stage before); wipe-off / pop(D) / sums of
  //                                 c + 1 into the copies c - 1 had; the request for c + 2's block (registers);
  //   start of the offset-8 stage:  the offset-0 vectors of c + 1; c + 2's block -> LDS, its pop(D) counters zeroed; the
  //                                 triplets of c - 1 (its last epilogue ran in the half stage before), its slots zeroed.
  MxBlockRegs next_block = {{0, 0, 0, 0}};
  v16f acc[2][kMxTiles];
  const int n_half = 4 * n_my;
  // the pieces behind the barrier of even half stage hs_even, thread t's share
  auto piece = [&](int hs_even, int t) {
    asm volatile("" : "+v"(t));   // (per-thread addresses of these pieces are recomputed, not kept across the stages)
    const int c = hs_even >> 2;
    window_to(c);
    const bool steady = c >= 1 && c + 2 < n_my;   // every piece exists: one straight run, their LDS round trips overlap
    if ((hs_even & 2) == 0) {
      if (steady) {
        const u32 step = step_of(c + 1);
        const uint8_t *blk = block_of(c + 2);
        next_block = mx_block_request(blk, prm.if_format, t);
        mx_byte_vector_pair(base8_of(c), e8x, e8x + kVec, t);
        mx_byte_wipe_codes(sh, d_of(c + 1), ones_of(c + 1), base0, base8_of(c + 1), step, t, t & 63);
      } else {
        if (c < n_my)
          mx_byte_vector_pair(base8_of(c), e8x, e8x + kVec, t);
        if (c + 1 < n_my)
          mx_byte_wipe_codes(sh, d_of(c + 1), ones_of(c + 1), base0, base8_of(c + 1), step_of(c + 1), t, t & 63);
        if (c + 2 < n_my)
          next_block = mx_block_request(block_of(c + 2), prm.if_format, t);
      }
    } else {
      int search, dopp;
      u32 mask;
      if (steady) {
        decode(c - 1, search, dopp, mask);
        mx_block_commit(sh, next_block, prm.if_format, t);
        if (t < 2)
          ones_of(c + 2)[t] = 0;
        mx_byte_fold(sh, (c - 1) & 1 ? kSlotsOdd : kSlotsEven, mask, set, search, dopp, prm, peaks, t);
        mx_byte_vector_pair(base0, &sh.e8[0][0][0][0], &sh.e8[1][0][0][0], t);
      } else {
        if (c + 1 < n_my)
          mx_byte_vector_pair(base0, &sh.e8[0][0][0][0], &sh.e8[1][0][0][0], t);
        if (c + 2 < n_my) {
          mx_block_commit(sh, next_block, prm.if_format, t);
          if (t < 2)
            ones_of(c + 2)[t] = 0;
        }
        if (c >= 1) {
          decode(c - 1, search, dopp, mask);
          mx_byte_fold(sh, (c - 1) & 1 ? kSlotsOdd : kSlotsEven, mask, set, search, dopp, prm, peaks, t);
        }
      }
    }
  };
#pragma unroll 1
  for (int hs = 0; hs <= n_half; hs++) {
    if ((hs & 1) == 0)
      __syncthreads();
    // A stage's pieces only have to be done before the NEXT barrier, and what they write nobody reads before it: role 1 does
    // its threads' share at once (pieces, epilogue, passes), role 0 at the end of its stage (passes, epilogue, pieces) -- the
    // two waves of a SIMD are then on the matrix pipe one after the other from the barrier on.
    if (role == 1 && (hs & 1) == 0)
      piece(hs, tid);
    const int x = hs - role;   // this role's half stage
    if (x >= 0 && x < n_half) {
      const int cc = x >> 2, o = (x >> 1) & 1;   // sample offset 8 o
      if ((x & 1) == 0) {
        const u32 *dd = d_of(cc), *ones = ones_of(cc);
        const u32 *va = o ? e8x : &sh.e8[0][0][0][0], *vb = o ? e8x + kVec : &sh.e8[1][0][0][0];
        if (o) {
          u32 b_low[2][kMxTiles], b_high[2][kMxTiles];
          mx_odd_tail_operands(va, vb, lane, q0_tile, b_low, b_high);
          mx_init_acc_odd(ones, dd, dd + 514, lane, q0_tile, acc, prm.win_start, prm.win_stop);
          mx_odd_tail_steps(sh, lane, b_low, b_high, acc);
        } else {
          mx_init_acc(ones, lane, q0_tile, acc, prm.win_start, prm.win_stop);
        }
        mx_pass2(sh, lane, q0_tile, acc, va, vb);
      } else {
        mx_epilogue_single(sh, lane, kq, 8 * o, acc, cc & 1 ? kSlotsOdd : kSlotsEven);
      }
    }
    if (role == 0 && (hs & 1) != 0)
      piece(hs - 1, tid);
  }
  __syncthreads();
  {
    int search, dopp;
    u32 mask;
    decode(n_my - 1, search, dopp, mask);
    mx_byte_fold(sh, (n_my - 1) & 1 ? kSlotsOdd : kSlotsEven, mask, set, search, dopp, prm, peaks, tid);
  }
}

}  // namespace

template <>
__global__ __launch_bounds__(kMxThreads, 1) void k_acq_mx<kMxByte>(GPSX_K_ACQ_MX_PARAMS)
{
  __shared__ MxShared sh;
  mx_byte_pipe(sh, prm, cluster_lo, if_blocks, mx_a, mx_t, peaks);
}

void launch_acq_mx_byte(hipStream_t s, unsigned grid, const AcqParams &prm, int cluster_lo, const uint8_t *d_if, const uint32_t *d_mx_a,
                        const uint32_t *d_mx_t)
{
  hipLaunchKernelGGL(k_acq_mx<kMxByte>, dim3(grid), dim3(kMxThreads), 0, s, prm, cluster_lo, d_if, d_mx_a, d_mx_t, prm.peaks, (u32 *)nullptr,
                     (u32 *)nullptr);
}

}  // namespace gpsx
