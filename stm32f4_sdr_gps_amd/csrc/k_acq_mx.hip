// k_acq_mx.hip -- the matrix-core grid (gpsx_mx_parts.hpp: formulation, data movement, work split): the table builder, the
// single-block form k_acq_mx<0> (mx_single) and the forms mx_unit serves -- <3> / <1> walk, <2> store, <5> split -- with the
// pieces only they use.
// (k_acq_mx<4>, the byte-phase form: k_acq_mx_byte.hip; the weighted kernels on the same parts: k_acq_mxw.hip.)
#include "gpsx_mx_parts.hpp"
#include "gpsx_mx_transposed.hpp"

namespace gpsx {

// mx_a [set][16][2][32][4]: the A fragments of a 32-slot cluster; mx_t [set][1032]: its transposed chip words
__global__ void k_build_mx_tables(const u32 *__restrict__ chipbits, int n_slots, u32 *__restrict__ mx_a, u32 *__restrict__ mx_t)
{
  const int n_sets = (n_slots + 31) / 32;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  const int per_set = 16 * 2 * 32 * 4 + 1032;
  if (idx >= n_sets * per_set)
    return;
  const int set = idx / per_set, r = idx - set * per_set;
  if (r < 16 * 2 * 32 * 4) {
    const int dw = r & 3, p = (r >> 2) & 31, h = (r >> 7) & 1, kappa = r >> 8;
    const int slot = 32 * set + p;
    const u32 word = slot < n_slots ? chipbits[(size_t)slot * 32 + 2 * kappa + h] : 0u;   // chips 64 kappa + 32 h ..
    mx_a[(size_t)set * (16 * 2 * 32 * 4) + r] = spread8((word >> (8 * dw)) & 0xFFu) << 1;   // chip 1 -> FP4 code 2 (= 1.0)
  } else {
    const int c = r - 16 * 2 * 32 * 4 - 1;   // -1 .. 1030
    u32 w = 0;
    if (c >= 0 && c < kChips)
      for (int p = 0; p < 32; p++) {
        const int slot = 32 * set + p;
        if (slot < n_slots)
          w |= ((chipbits[(size_t)slot * 32 + (c >> 5)] >> (c & 31)) & 1u) << p;
      }
    mx_t[(size_t)set * 1032 + (c + 1)] = w;
  }
}

void launch_build_mx_tables(hipStream_t s, const uint32_t *d_chipbits, int n_slots, uint32_t *d_mx_a, uint32_t *d_mx_t)
{
  const int n_sets = (n_slots + 31) / 32;
  const int n = n_sets * (16 * 2 * 32 * 4 + 1032);
  hipLaunchKernelGGL(k_build_mx_tables, dim3((n + 255) / 256), dim3(256), 0, s, d_chipbits, n_slots, d_mx_a, d_mx_t);
}

namespace {

// No PRN set's tables are in LDS when a workgroup starts.  mx_single and mx_unit test their set against this before they load them:
// a set is a remainder, negative for all the compiler knows, so the test is a compare and a branch in the instruction streams
// of k_acq_mx<0> <1> <2> <3> <5> (it never fails).
constexpr int kMxNoSet = -1;
constexpr int kPasses = 17;            // 2 for the first offset + 15 recurrence steps
constexpr int kPassesAnchor = 16;      // the single-block form: 1 (E3M2 anchor) + 15
constexpr int kAnchorDwords = 392;     // one stream's anchor vector: 2048 six-bit codes = 384 dwords, + slack

// Eight of the sixteen planes (sample offsets t0_lo .. t0_lo + 7, both streams) with their circular extension, by the four waves
// of ONE role while the other role is inside an MFMA pass (the single-block form's start-up, mx_single): wave v owns the four rows
// (stream v >> 1, t0 = t0_lo + 4 (v & 1) + 0..3) WHOLE, so that an extension word depends only on words its own wave wrote -- a
// wavefront-scope fence and a wait for the LDS order them, where mx_wipe_block needs a workgroup barrier that the other role,
// inside its pass, would not arrive at.  Lane (t0 = lane & 3, w = lane >> 2 (+ 16)): the four lanes of a word read the same
// sixteen stream words (LDS broadcast), the sixteen words of a wave in rotated order -- 16 w + (k + w) mod 16: sixteen banks per
// parity of w -- where the plain order would put all sixteen on two banks.
__device__ __forceinline__ void mx_planes_half(MxSharedCore &sh, int t0_lo, int v, int lane)
{
  const int iq = v >> 1, t0_first = t0_lo + 4 * (v & 1);
  const int t0 = t0_first + (lane & 3), rot = lane >> 2;
#pragma unroll 1
  for (int it = 0; it < 2; it++) {
    const int w = rot + 16 * it;
    const u32 *src = &sh.d[iq][16 * w];
    u32 bits = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) {
      const int kk = (k + rot) & 15;
      const u32 sk = src[kk];
      bits |= ((sk >> t0) & 1u) << (2 * kk);
      bits |= ((sk >> (16 + t0)) & 1u) << (2 * kk + 1);
    }
    sh.plane[iq][t0][w] = bits;
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave's words 0..31 of its four rows are in LDS
#pragma unroll 1
  for (int m = lane; m < 4 * (kPlaneWordsMx - 32); m += 64) {
    const int r = m / (kPlaneWordsMx - 32), w = 32 + m % (kPlaneWordsMx - 32);
    u32 *pl = sh.plane[iq][t0_first + r];
    pl[w] = mx_plane_ext_word(pl, w);
  }
}

// ---- the single-block form's anchor: sample offset 0 in ONE pass ---------------------------------------------------------------
// The vector holds 8 - S_0[k] as E3M2 codes (gpsx_anchor_codes.hpp) at block scale 2^1: against chips in {0, 1} the pass adds
// 2 sum_c chip[c] (8 - S_0[q + c]) = 8192 - 2 M_0(q) (512 ones per code), so the start values are the two-pass form's less 8192.
// ONE copy per stream, 2048 codes in 384 dwords: a lane's window starts at bit 6 (32 f + n), dword aligned only every 16 lanes,
// and is cut out in registers (mx_anchor_pass).  Thread (stream, j): the codes of entries 8 j .. 8 j + 7, 48 bits; the two lanes
// of a pair write the three dwords they fill.
__device__ __forceinline__ void mx_anchor_build(MxSharedCore &sh, u32 *dst, int tid)
{
  const int iq = tid >> 8, j = tid & 255;
  const u32 *dd = sh.d[iq];
  u64 bits = 0;
#pragma unroll
  for (int e = 0; e < 8; e++) {
    const int pos = 16 * wrap1023(8 * j + e);
    const u32 sum = pop16(__builtin_amdgcn_alignbit(dd[(pos >> 5) + 1], dd[pos >> 5], (u32)(pos & 31)));
    bits |= (u64)gpsx_anchor_code((int)sum) << (6 * e);
  }
  const u32 lo = (u32)bits, hi = (u32)(bits >> 32);   // (hi: 16 bits)
  const u32 lo_pair = dpp<0xB1>(lo, lo);              // quad_perm [1,0,3,2]: the other lane of the pair
  u32 *d3 = dst + iq * kAnchorDwords + 3 * (j >> 1);
  if (j & 1) {
    d3[2] = (lo >> 16) | (hi << 16);
  } else {
    d3[0] = lo;
    d3[1] = hi | (lo_pair << 16);
  }
}

// Seven dwords from the window's dword, shifted down by 6 n mod 32: the lane's 32 codes in six dwords (v_alignbit_b32)
struct AnchorRaw {
  u32 d[7];
};
__device__ __forceinline__ AnchorRaw mx_anchor_raw(lds_cu32 *w, int dw)
{
  AnchorRaw r;
#pragma unroll
  for (int i = 0; i < 7; i++)
    r.d[i] = w[dw + i];
  return r;
}
__device__ __forceinline__ v8i mx_anchor_frag(const AnchorRaw &r, u32 shift)
{
  v8i f = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < 6; i++)
    f[i] = (int)__builtin_amdgcn_alignbit(r.d[i + 1], r.d[i], shift);
  return f;
}
// One anti-diagonal, as mx_pass_step: the raw dwords of the next one are requested first, then this one's MFMAs go out, and the
// shifts that make the next fragments run under them.
template <int S, int NT>
__device__ __forceinline__ void mx_anchor_step(lds_cu32 *wi, lds_cu32 *wq, const v4i *ca, v4i (&a)[16], v8i &fi, v8i &fq,
                                               v16f (&acc)[2][NT], u32 shift)
{
  constexpr int kSteps = 16 + NT - 1;
  constexpr bool more = S + 1 < kSteps;
  AnchorRaw ri, rq;
  if constexpr (more) {
    ri = mx_anchor_raw(wi, 12 * (S + 1));                  // fragment Q0 + 2 (S + 1): six dwords per fragment
    rq = mx_anchor_raw(wq, 12 * (S + 1));
    if constexpr (S + 1 < 16)
      a[S + 1] = ca[(S + 1) * 64];                         // chips_a[S + 1][h][n]
  }
  constexpr int j_lo = S - 15 > 0 ? S - 15 : 0, j_hi = S < NT - 1 ? S : NT - 1;
#pragma unroll
  for (int j = j_lo; j <= j_hi; j++) {
    // (transposed, as the recurrence passes -- mx_mfma: the E3M2 vector is A, format code 3 in cbsz, its 2^1 on the A side)
    acc[0][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(fi, widen(a[S - j]), acc[0][j], 3, 4, 0, kScaleTwo, 0, kScaleA);
    acc[1][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(fq, widen(a[S - j]), acc[1][j], 3, 4, 0, kScaleTwo, 0, kScaleA);
  }
  if constexpr (more) {
    __builtin_amdgcn_sched_group_barrier(0x100, S + 1 < 16 ? 9 : 8, 0);      // DS reads
    __builtin_amdgcn_sched_group_barrier(0x008, 2 * (j_hi - j_lo + 1), 0);   // MFMAs
  }
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (more) {
    fi = mx_anchor_frag(ri, shift);
    fq = mx_anchor_frag(rq, shift);
    __builtin_amdgcn_sched_barrier(0);
    mx_anchor_step<S + 1, NT>(wi, wq, ca, a, fi, fq, acc, shift);
  }
}
// The chips it reads -- every kappa, each a step ahead of its first MFMA -- are the lane's for the whole cluster: they go into
// `chips`, where the recurrence passes find those of kappa < kMxChipsResident (MxChipRegs).
template <int NT>
__device__ __forceinline__ void mx_anchor_pass(const MxSharedCore &sh, const u32 *anchor, int lane, int q0_tile, v16f (&acc)[2][NT],
                                               MxChipRegs &chips)
{
  const int n = lane & 31, h = lane >> 5;
  const u32 shift = (u32)(6 * n) & 31u;
  lds_cu32 *wi = lds_opaque(anchor + 6 * (q0_tile + h) + ((6 * n) >> 5));
  lds_cu32 *wq = lds_opaque(anchor + kAnchorDwords + 6 * (q0_tile + h) + ((6 * n) >> 5));
  const v4i *ca = &sh.chips_a[0][h][n];
  v8i fi = mx_anchor_frag(mx_anchor_raw(wi, 0), shift), fq = mx_anchor_frag(mx_anchor_raw(wq, 0), shift);
  chips.k[0] = ca[0];
  mx_anchor_step<0, NT>(wi, wq, ca, chips.k, fi, fq, acc, shift);
}

// ---- the two vectors of a DIRECT start at sample offset t0s, in one phase ---------------------------------------------------
// M_t0s(q) = sum_c chip[c] S_t0s[q + c] from the block sums S_t0s[k] = pop(D[16 k + t0s, +16)) themselves, as passes 0 and 1
// do it for t0s = 0 (mx_vector_phase1): which = 0: -2 (S & 3), which = 1: -(S >> 2) at block scale 2^3.  Thread (stream, j)
// builds dwords j and j + 1 of copy 0 (sixteen block sums) and writes dword j of the eight shifted copies -- no round trip
// through sh.base, no second barrier.  Used where a workgroup does not walk to an offset but starts there: offset 8 of the
// byte-phase grid (the reference's own search, PM/GPS/acquisition.c:280-312) and the second half of a split fine grid.
__device__ __forceinline__ void mx_vector_build_direct(MxShared &sh, int which, int t0s, u32 *e8_dst, int tid)
{
  const int iq = tid >> 8, j = tid & 255;
  const u32 *dd = sh.d[iq];
  u32 w2[2] = {0, 0};
#pragma unroll
  for (int e = 0; e < 16; e++) {
    const int k = wrap1023(8 * j + e);
    const int pos = 16 * k + t0s;
    const u32 sum = pop16(__builtin_amdgcn_alignbit(dd[(pos >> 5) + 1], dd[pos >> 5], (u32)(pos & 31)));
    const u32 code = which == 0 ? (0xFEC0u >> (4u * (sum & 3u))) & 0xFu : (0xEDCA0u >> (4u * (sum >> 2))) & 0xFu;
    w2[e >> 3] |= code << (4 * (e & 7));
  }
  u32 *dst = e8_dst + (iq * 8) * kCopyDwords + j;   // [stream][copy][dword]
#pragma unroll
  for (int c = 0; c < 8; c++)
    dst[c * kCopyDwords] = c ? __builtin_amdgcn_alignbit(w2[1], w2[0], 4u * (u32)c) : w2[0];
}

// The general form of the above for a workgroup that STARTS at sample offset t0s = 8 half + b (mx_vector_build_direct gave
// it C0): everything the walk would have accumulated or patched in by then, as start values --
//   + c1022 A_b(q),  A_b = 2 pop(byte_o & low_b) - b                                                     (quirk Q5)
//   - half [ pop(W) + chip[1021 - q] b + chip[1022 - q] (16 - b - 2 pop(W))                               (Q3, wrap word)
//            + T(q) ( pop(P) + c1021 (b - 2 pop(P & low_b)) + c1022 (16 - b - 2 pop(P & high_b)) ) ]      (Q3, tail word)
// with o = 2 q + half, W = data bytes (2045, 0), P = data bytes (o - 2, o - 1), T = [q > 0] (the formula in front of
// mx_half_switch; tests/test_formulation.py).  Five multiply-adds per hypothesis, once per workgroup.
__device__ __forceinline__ void mx_direct_terms(const MxShared &sh, int lane, int q0_tile, v16f (&acc)[2][kMxTiles], int t0s,
                                                int win_start, int win_stop)
{
  const int n = lane & 31, h = lane >> 5;
  const int b = t0s & 7, half = t0s >> 3;
  const u32 low = (1u << b) - 1u, high = (0xFFFFu << b) & 0xFFFFu;
  const float fh = (float)half;
  const u32 f22 = sh.chip_t[1022 + 1] >> (4 * h), f21 = sh.chip_t[1021 + 1] >> (4 * h);
  float popw[2], beta[2];
#pragma unroll
  for (int s = 0; s < 2; s++) {
    const int pw = (int)__popc(sh.d[s][0] & 0xFFu);   // W = byte 0 << 8: its low byte (data byte 2045) is never mixed
    popw[s] = (float)pw;
    beta[s] = (float)(16 - b - 2 * pw);
  }
#pragma unroll
  for (int j = 0; j < kMxTiles; j++) {
    const int q = 32 * (q0_tile + 2 * j) + n;
    const bool exists = q < kChips;
    const int qc = exists ? q : 0;
    const int o = 2 * qc + half;
    const float tq = (qc > 0) ? fh : 0.0f;            // half * T(q)
    float k0[2], k21[2], k22[2], kb[2];
#pragma unroll
    for (int s = 0; s < 2; s++) {
      const int fa = 2 * (int)__popc(lds_byte(sh.d[s], o) & low) - b;
      int fp = 0, gl = 0, gh = 0;
      if (qc > 0 || half == 0) {   // (o >= 2 wherever the tail term counts; for half == 0 the values are multiplied by 0)
        const int o2 = o >= 2 ? o : 2;
        const u32 prev = lds_byte(sh.d[s], o2 - 2) | (lds_byte(sh.d[s], o2 - 1) << 8);
        fp = (int)__popc(prev);
        gl = b - 2 * (int)__popc(prev & low);
        gh = 16 - b - 2 * (int)__popc(prev & high);
      }
      k0[s] = -(fh * popw[s] + tq * (float)fp) * kAccScale;
      k21[s] = -tq * (float)gl * kAccScale;
      k22[s] = ((float)fa - tq * (float)gh) * kAccScale;
      kb[s] = -fh * beta[s] * kAccScale;
    }
    const float ka = -fh * (float)b * kAccScale;
    if (half) {   // the accumulators were started for the even byte offset's window position
      const bool in0 = exists && 2 * q >= win_start && 2 * q < win_stop;
      const bool in1 = exists && 2 * q + 1 >= win_start && 2 * q + 1 < win_stop;
      if (in0 != in1) {
        k0[0] += in1 ? -kOutside : kOutside;
        k0[1] += in1 ? -kOutside : kOutside;
      }
    }
    const u32 w1 = sh.chip_t[(exists ? kChips - 1 - q : 0) + 1] >> (4 * h);   // chip 1022 - q of the lane's PRNs
    const u32 w0 = sh.chip_t[(exists ? kChips - 2 - q : -1) + 1] >> (4 * h);  // chip 1021 - q (chip -1 = 0)
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int pb = (r & 3) + 8 * (r >> 2);
      const float c22 = (float)((f22 >> pb) & 1u), c21 = (float)((f21 >> pb) & 1u);
      const float ca = (float)((w0 >> pb) & 1u), cb = (float)((w1 >> pb) & 1u);
      acc[0][j][r] += k0[0] + ca * ka + cb * kb[0] + c21 * k21[0] + c22 * k22[0];
      acc[1][j][r] += k0[1] + ca * ka + cb * kb[1] + c21 * k21[1] + c22 * k22[1];
    }
  }
}

// MULTI: the running sums between blocks: the scratch stream is what binds this form (bench.py `roofline` of the
// multi-block run), so its records are as small as exactness allows.
//   S16 = true  (kMxWalk16, the form that runs first): four 16-bit sums in two dwords, moved on by SATURATING packed adds
//               (v_pk_add_u16 clamp: two sums per instruction, no unpacking).  n_ms x 11573 fits 16 bits up to 5 blocks;
//               beyond that only hypotheses with magnitudes above 6553 in every block -- clean carriers, not signals in
//               noise -- can reach 0xFFFF, where a sum then stays: the last block's epilogue, which unpacks the sums for
//               its keys, raises the workgroup's flag when it meets one, and the launcher's second kernel (kMxWalk,
//               below), whose workgroups leave at once where no flag is up, does such a cluster again with
//   S16 = false (kMxWalk): four sums of 24 bits (128 x 11573 < 2^21) in three dwords.
template <bool S16>
struct SumRecT {
  u32 w[S16 ? 2 : 3];
};
// (The records are a stream: written once per block, read once a block later, a megabyte per workgroup in between -- nothing
//  a cache keeps.)
template <bool S16>
__device__ __forceinline__ void sums_unpack(const SumRecT<S16> &r, u32 (&s)[4])
{
  if constexpr (S16) {
    s[0] = r.w[0] & 0xFFFFu;
    s[1] = r.w[0] >> 16;
    s[2] = r.w[1] & 0xFFFFu;
    s[3] = r.w[1] >> 16;
  } else {
    s[0] = r.w[0] & 0xFFFFFFu;
    s[1] = __builtin_amdgcn_alignbit(r.w[1], r.w[0], 24u) & 0xFFFFFFu;
    s[2] = __builtin_amdgcn_alignbit(r.w[2], r.w[1], 16u) & 0xFFFFFFu;
    s[3] = r.w[2] >> 8;
  }
}
template <bool S16>
__device__ __forceinline__ SumRecT<S16> sums_pack(const u32 (&s)[4])
{
  SumRecT<S16> r;
  if constexpr (S16) {
    // (the low halves of two sums; a sum that does not fit has raised the workgroup's flag, what is stored is not used)
    r.w[0] = __builtin_amdgcn_perm(s[1], s[0], 0x05040100u);
    r.w[1] = __builtin_amdgcn_perm(s[3], s[2], 0x05040100u);
  } else {
    r.w[0] = s[0] | (s[1] << 24);
    r.w[1] = (s[1] >> 8) | (s[2] << 16);
    r.w[2] = (s[2] >> 16) | (s[3] << 8);
  }
  return r;
}

// two 16-bit sums + two magnitudes in one instruction, saturating: a half that reaches 0xFFFF stays there, and the last
// block's epilogue, which unpacks the sums anyway, raises the flag when it meets one
typedef unsigned short us2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ u32 pk_add_sat_u16(u32 a, u32 b)
{
  return __builtin_bit_cast(u32, __builtin_elementwise_add_sat(__builtin_bit_cast(us2, a), __builtin_bit_cast(us2, b)));
}

// MULTI: request the running sums of sample offset t0, records [first, first + count) of this lane's 16; zero for the first
// block.  The first two tiles' records are requested before the wave's MFMA pass, the other two's at the start of the
// epilogue: a pass or two tiles of epilogue ahead of their use, never more than 12 records in registers.
// Record layout of a wave's slice: [sample offset][tile][lane][8-PRN group] -- a lane's four records of a tile are contiguous
// (32 bytes with the 16-bit records), so two of them move per instruction: half the loads and stores of the
// [offset][tile][group][lane] layout of round 2, still 1 KB contiguous per wave instruction.
template <bool S16>
struct alignas(8) RecPairT {
  SumRecT<S16> a, b;
};
template <int FIRST, int COUNT, bool S16>
__device__ __forceinline__ void mx_prefetch_sums(const u32 *__restrict__ energy, const u32 *__restrict__ zero_recs, int lane,
                                                 int t0, bool ms_first, SumRecT<S16> (&pre)[16])
{
  static_assert(FIRST % 2 == 0 && COUNT % 2 == 0, "records move in pairs");
  // (first block of a search: the running sums are zero -- read from a small all-zero region, `zero_recs`, instead of being
  //  set by the vector ALU: register writes into the prefetch array made the compiler drain every outstanding store first,
  //  an s_waitcnt vmcnt(0) per step; a load is ordered behind them by the memory system and costs nothing)
  if constexpr (S16) {
    // 16-bit records: [sample offset][tile][group pair][lane][2] -- a wave's 16-byte loads and stores of a pair cover ONE
    // contiguous kilobyte (whole 128-byte lines per instruction, not half lines twice)
    const SumRecT<S16> *e2 = ms_first ? reinterpret_cast<const SumRecT<S16> *>(zero_recs) + (size_t)lane * 2
                                      : reinterpret_cast<const SumRecT<S16> *>(energy) + (size_t)(t0 * kMxTiles) * 256 + (size_t)lane * 2;
#pragma unroll
    for (int i = FIRST; i < FIRST + COUNT; i += 2) {
      const RecPairT<S16> rp = *reinterpret_cast<const RecPairT<S16> *>(&e2[(size_t)(i >> 2) * 256 + (size_t)((i & 3) >> 1) * 128]);
      pre[i] = rp.a;
      pre[i + 1] = rp.b;
    }
    return;
  }
  const SumRecT<S16> *e4 = ms_first ? reinterpret_cast<const SumRecT<S16> *>(zero_recs) + (size_t)lane * 4
                                    : reinterpret_cast<const SumRecT<S16> *>(energy) + ((size_t)(t0 * kMxTiles) * 64 + lane) * 4;
#pragma unroll
  for (int i = FIRST; i < FIRST + COUNT; i += 2) {
    const RecPairT<S16> rp = *reinterpret_cast<const RecPairT<S16> *>(&e4[(size_t)(i >> 2) * 256 + (i & 3)]);
    pre[i] = rp.a;
    pre[i + 1] = rp.b;
  }
}

// ---- epilogue of one sample offset: magnitude, windowed max / sum -------------------------------------------------------
// SEARCH = false (MULTI, not the last block): only the running sums move on -- no key, no maximum, no window sum
template <bool MULTI, bool SEARCH, bool S16>
__device__ __forceinline__ void mx_epilogue(MxShared &sh, int lane, int q0_tile, int t0, const v16f (&acc)[2][kMxTiles],
                                            u32 group_mask, u32 *__restrict__ energy, const u32 *__restrict__ zero_recs,
                                            SumRecT<S16> (&pre)[MULTI ? 16 : 1], bool ms_first, u32 &witness)
{
  typedef SumRecT<S16> SumRec;
  constexpr bool ms_last = SEARCH;
  const int n = lane & 31, h = lane >> 5;
  const int b = t0 & 7, half = t0 >> 3;
  // Search results: every lane owns a (bit shift, PRN) slot pair of LDS -- atomics without a return value at per-PRN
  // constant offsets from one address, no conflicts.  Single-block searches keep a running maximum / sum per PRN in
  // registers and fold them in once per sample offset (32 atomics); the multi-block form, short of registers next to its
  // prefetched sums, folds every hypothesis in directly (measured: 3 % slower for the single-block form, 4 % faster here).
  constexpr bool DIRECT = MULTI;
  u32 *slot = SEARCH ? &sh.part[b][4 * h][0][n] : nullptr;
  u32 best[SEARCH && !DIRECT ? 16 : 1], total[SEARCH && !DIRECT ? 16 : 1];
#pragma unroll
  for (int r = 0; r < (SEARCH && !DIRECT ? 16 : 1); r++) {
    best[r] = 0;
    total[r] = 0;
  }
  // MULTI: the running sums of a lane's four hypotheses of a group are one 12-byte record ([offset][tile][group][lane]: a
  // wave reads / writes 768 contiguous bytes per instruction); the first records of this offset were requested before
  // the wave's MFMA pass (mx_prefetch_sums) -- the scratch is HBM, the pass hides its latency
  SumRec *e4 = reinterpret_cast<SumRec *>(energy) + ((size_t)(t0 * kMxTiles) * 64 + lane) * 4;   // [tile][lane][group]
  mx_round_toward_zero();
#pragma unroll
  for (int j = 0; j < kMxTiles; j++) {
    const int q = 32 * (q0_tile + 2 * j) + n;
    const u32 key_lo = (u32)(2047 - (2 * q + half));   // 0 .. 2047 (q = 1023 does not exist: its magnitude is 0)
    if constexpr (MULTI) {
      // (deeper -- two tiles ahead with the 16-bit records -- measured 3 % slower: more registers, nothing gained)
      // (two tiles ahead: with the spilled registers gone -- round 3 -- the deeper request is 2 % faster; round 2 measured it
      //  1-3 % slower, next to 46 spilled registers)
      if (j == 0)
        mx_prefetch_sums<8, 8, S16>(energy, zero_recs, lane, t0, ms_first, pre);
    }
    // (all four 8-PRN groups, whether this shard owns them or not: a workgroup that owns only some -- at the ends of a
    //  shard's run, or a ragged PRN list -- does a little unused work here instead of branching around register arrays;
    //  group_mask decides below what is published)
    // GS hypotheses at a time: enough independent chains for a wave that has its SIMD's vector ALU to itself (its partner
    // is in the MFMA pass) to cover the ALU, transcendental and branch latencies, few enough to stay in registers next to
    // the 128 accumulators.
    constexpr int GS = MULTI ? 4 : 8;
    SumRec held{};   // (16-bit records, not the last block: the even group's new record, until the odd group's is there)
#pragma unroll
    for (int r0 = 0; r0 < 16; r0 += GS) {
      u32 prev[GS];
#pragma unroll
      for (int i = 0; i < GS; i++)
        prev[i] = 0;
      if (MULTI && !(S16 && !SEARCH)) {
#pragma unroll
        for (int g = 0; g < GS / 4; g++) {
          u32 p4[4];
          sums_unpack<S16>(pre[MULTI ? j * 4 + r0 / 4 + g : 0], p4);
#pragma unroll
          for (int i = 0; i < 4; i++) {
            prev[4 * g + i] = p4[i];
            if constexpr (S16)
              witness = max(witness, p4[i]);   // (last block: a saturated sum, 0xFFFF, shows here)
          }
        }
      }
      SumRec *e_rec = e4 + (size_t)j * 256 + r0 / 4;
      u32 out[GS];
      // Magnitudes of the group's hypotheses.  When all of them (GS x 64 lanes) lie below radius 1024 -- noise hypotheses
      // sit at a few hundred -- e < 2^20 is an exact integer and trunc(v_sqrt_f32(e + 1/2)) is its integer root with no
      // fix-up (the true root of n^2 + r + 1/2 keeps 1 / (4 (n + 1)) away from the integers around it, one ulp below 1024
      // is half of that; gps_mag8 checks every pair of that domain on the device): one wave-uniform test per group
      // instead of GS neighbour tests.
      float ev[GS];
      u32 e_max = 0;
#pragma unroll
      for (int i = 0; i < GS; i++) {
        ev[i] = clip_square_sum(acc[0][j][r0 + i], acc[1][j][r0 + i]);
        e_max = max(e_max, __float_as_uint(ev[i]));   // (on the bit patterns: non-negative floats order like integers)
      }
      const bool small = __builtin_amdgcn_ballot_w64(e_max >= 0x3C800000u /* 2^20 / 2^26 as f32 */) == 0;
      u32 mag[GS];
      constexpr bool PACKED = MULTI && S16 && !SEARCH;   // 16-bit records, not the last block: sums move on in packed form
      if (small) {
#pragma unroll
        for (int i = 0; i < GS; i++)
          mag[i] = PACKED ? root_bits_small(ev[i]) : (u32)(int)(__builtin_amdgcn_sqrtf(ev[i]) * kRootGuard);
      } else {
        float ci[GS], cq[GS];
#pragma unroll
        for (int i = 0; i < GS; i++) {
          ci[i] = acc[0][j][r0 + i];
          cq[i] = acc[1][j][r0 + i];
        }
        mx_roots_exact<GS>(ci, cq, mag);
      }
      if constexpr (PACKED) {
        // (magnitudes in the low halves of mag[] -- the rounding add's 0x4B000000 sits above them --, two per v_perm_b32,
        //  then one saturating packed add per pair: 1 instruction per hypothesis instead of unpack, add, pack and witness)
        const SumRec &pr = pre[j * 4 + r0 / 4];
        SumRec nr;
        nr.w[0] = pk_add_sat_u16(pr.w[0], __builtin_amdgcn_perm(mag[1], mag[0], 0x05040100u));
        nr.w[1] = pk_add_sat_u16(pr.w[1], __builtin_amdgcn_perm(mag[3], mag[2], 0x05040100u));
        // (a lane's records of a tile are contiguous: the even group's waits for the odd one, both leave in one 16-byte store)
        if ((r0 / 4) & 1) {
          RecPairT<S16> both;
          both.a = held;
          both.b = nr;
          // ([offset][tile][pair][lane][2]: see mx_prefetch_sums)
          SumRec *e_pair = reinterpret_cast<SumRec *>(energy) + (size_t)(t0 * kMxTiles + j) * 256 + (size_t)(r0 / 8) * 128 + (size_t)lane * 2;
          *reinterpret_cast<RecPairT<S16> *>(e_pair) = both;
        } else {
          held = nr;
        }
        __builtin_amdgcn_sched_barrier(0);
        continue;
      }
#pragma unroll
      for (int i = 0; i < GS; i++) {
        const int r = r0 + i;
        u32 val = mag[i];
        if (MULTI)
          val += prev[i];
        out[i] = val;
        if (SEARCH && DIRECT) {
          const int p_off = ((r & 3) + 8 * (r >> 2)) * 64;   // PRN (r & 3) + 8 (r >> 2) + 4 h: 2 x 32 words per PRN
          atomicMax(slot + p_off, (val << 11) | key_lo);
          atomicAdd(slot + p_off + 32, val);
        } else if (SEARCH) {
          const u32 key = (val << 11) | key_lo;
          best[DIRECT ? 0 : r] = key > best[DIRECT ? 0 : r] ? key : best[DIRECT ? 0 : r];
          total[DIRECT ? 0 : r] += val;
        }
      }
      if (MULTI && !ms_last) {
#pragma unroll
        for (int g = 0; g < GS / 4; g++) {
          const u32 o4[4] = {out[4 * g], out[4 * g + 1], out[4 * g + 2], out[4 * g + 3]};
          e_rec[g] = sums_pack<S16>(o4);
        }
      }
      if (SEARCH && !DIRECT) {   // (pinned in program order: left alone, the compiler sinks all 64 chains to the end and spills)
#pragma unroll
        for (int i = 0; i < GS; i++)
          asm volatile("" : "+v"(best[DIRECT ? 0 : r0 + i]), "+v"(total[DIRECT ? 0 : r0 + i]));
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  mx_round_to_nearest();
  if (SEARCH && !DIRECT) {
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int p_off = ((r & 3) + 8 * (r >> 2)) * 64;
      atomicMax(slot + p_off, best[DIRECT ? 0 : r]);
      atomicAdd(slot + p_off + 32, total[DIRECT ? 0 : r]);
    }
  }
}

// Block-parallel form of a multi-block search (kMxStore): this workgroup handled ONE block; its magnitudes go out as
// u16 in the layout k_acq_vals_search (k_acq_poly.hip) sums and searches: per (search, block, PRN, Doppler) a plane of
// [sample offset][q & 3][q >> 2].
__device__ __forceinline__ void mx_epilogue_store(int lane, int q0_tile, int t0, const v16f (&acc)[2][kMxTiles], u32 group_mask,
                                                  uint16_t *__restrict__ plane0, size_t prn_stride, int slot0, int n_prn)
{
  const int n = lane & 31, h = lane >> 5;
#pragma unroll
  for (int j = 0; j < kMxTiles; j++) {
    const int q = 32 * (q0_tile + 2 * j) + n;
    uint16_t *v = plane0 + (size_t)t0 * 1024 + (size_t)(q & 3) * 256 + (size_t)(q >> 2);
#pragma unroll
    for (int g = 0; g < 4; g++) {
#pragma unroll
      for (int rr = 0; rr < 4; rr++) {
        const int r = 4 * g + rr;
        const int p = (r & 3) + 8 * (r >> 2) + 4 * h;
        const u32 val = mag8_f32(acc[0][j][r], acc[1][j][r]);
        if (((group_mask >> g) & 1u) && slot0 + p < n_prn)
          v[(size_t)p * prn_stride] = (uint16_t)val;
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

// ---- the single-block form (k_acq_mx<0>, n_ms == 1: the headline sweep): one workgroup per cluster -----------------------------
// Sample offset 0 in ONE pass (the E3M2 anchor, mx_anchor_pass), so kPassesAnchor passes; pass p >= 1 produces sample offset p and is
// pass p + 1 of the two-pass forms (mx_unit), the number that mx_vector_build, the vector buffers and the quirk steps go by.
// Steps of two halves: role 0 runs a pass, then the epilogue of the sample offset it produced; role 1 the epilogue first, then the
// pass -- one wave of a SIMD on the matrix pipe while the other has the vector ALU, with nothing but their own pace between the
// halves: ONE barrier per step, behind which all eight waves build the vector of the next step's pass into the buffer that both
// roles read during the step before.  (Behind the barrier, not behind the epilogue as in the walk forms: same-box A/B, 1.8 % faster
// here -- the step is bound by the SIMD's issue port, not by the barrier: moving the work does not shorten it.)
//
// The anchor pass leaves the role that waits for it without an epilogue, so half steps 0 and 1 are straight-line code and the loop
// starts at half step 2.  The preamble builds only what the anchor pass reads and the first epilogue writes; role 1 fills its empty
// half step 0 with the rest of it, next to a partner that issues MFMAs, LDS reads and the fragments' shifts only:
//   piece, maker                                    first reader                                  published by the barrier of
//   anchor vector (in e8[0]), zeroes of the result  the anchor passes; role 0's epilogue of       half step 0
//   slots, block, pop(D), chips:       all, preamble   offset 0 in half step 1
//   role 1's start values:             role 1, 0    its anchor pass                               (its own)
//   planes t0 0..7 + extension, t_lut: role 1, 0    mx_vector_build(2), behind that barrier       half step 2
//   planes t0 8..15 + extension:       role 1, 0    mx_vector_build(10), half step 16             half step 2
//   the half switch's table hs:        role 1, 0    mxt_half_switch, half steps 16 / 17           half step 2
//   vector of pass 1 (e8[0], over the anchor): all, 2   pass 1, half steps 2 / 3                  the loop's first (half step 2)
// The barrier of half step 2 is taken twice: once to end the anchor passes and publish the planes, once -- the loop's own --
// behind the build of pass 1's vector, where the loop goes on to build pass 2's next to pass 1 as in every later step.
//
// The quirk terms ride in chip columns 1021 / 1022 of the recurrence passes (MxFold, gpsx_fold_codes.hpp): no extra K step here.
// The pairs of a pass are built with its vector and published with it; their look-up table is one more piece of role 1's half
// step 0, published like t_lut.
//
// The accumulator tile is TRANSPOSED here (gpsx_mx_transposed.hpp): the fragment is the MFMA's A operand and the chips are B, so a
// lane holds ONE PRN, lane & 31, and its 4 x 16 registers 64 chip offsets of it.  The windowed maximum and sum of a sample offset
// are register chains of the lane that end in two LDS atomics per wave (mxt_epilogue), the result slots are one word per
// (bit shift, field, lane half, PRN), and what the even-to-odd switch adds per chip offset comes from a table built once per
// workgroup (mxt_half_switch_build).  The other forms keep one chip offset per lane and 16 PRNs in its registers.
constexpr int kHsStride = 1026;          // a row of the half switch's table: 1024 entries + 16 bytes, so that the two rows a wave
                                         // reads at the same chip offset lie in different banks
struct MxSingleShared {
  MxSharedCore mx;
  MxFold fold;
  alignas(16) u32 part[8][2][2][32];     // [bit shift][best key / sum][lane half][PRN]: a wave's atomic hits 64 different words
  alignas(16) float2 hs[2][kHsStride];   // [chip 1022 of the PRN][q]: (I, Q) terms of the even-to-odd switch (mxt_half_switch)
};

// The search window in chip offsets: the even byte offset 2 q of an existing q lies inside for q in [lo0, hi0), the odd one,
// 2 q + 1, for q in [lo1, hi1); lo1 <= lo0 <= lo1 + 1 and hi1 <= hi0 <= hi1 + 1.
struct MxtWindow {
  int lo0, hi0, lo1, hi1;
};
__device__ __forceinline__ MxtWindow mxt_window(int win_start, int win_stop)
{
  MxtWindow w;
  w.lo0 = (win_start + 1) >> 1;
  w.hi0 = min(kChips, (win_stop + 1) >> 1);
  w.lo1 = win_start >> 1;
  w.hi1 = min(kChips, win_stop >> 1);
  return w;
}
// Do all 128 chip offsets of this wave exist and lie, with both their byte offsets, inside the search window?  Wave-uniform; true
// for every wave of an unwindowed search but the one that holds q = 1023.
__device__ __forceinline__ bool mxt_wave_whole(int q0_tile, int win_start, int win_stop)
{
  const MxtWindow w = mxt_window(win_start, win_stop);
  const int q_lo = 32 * q0_tile, q_hi = 32 * (q0_tile + 2 * (kMxTiles - 1)) + 31;
  return q_lo >= w.lo0 && q_hi < w.hi1;
}

// mx_init_acc for the transposed tile: the window test is per register, or -- one test for the wave -- not needed at all
__device__ __forceinline__ void mxt_init_acc(const u32 *ones, int lane, int q0_tile, v16f (&acc)[2][kMxTiles], int win_start,
                                             int win_stop, int pass_bias)
{
  const float base_i = (float)((int)ones[0] + 8192 - kHalf - pass_bias) * kAccScale,
              base_q = (float)((int)ones[1] + 8192 - kHalf - pass_bias) * kAccScale;
  if (mxt_wave_whole(q0_tile, win_start, win_stop)) {
#pragma unroll
    for (int j = 0; j < kMxTiles; j++)
#pragma unroll
      for (int r = 0; r < 16; r++) {
        acc[0][j][r] = base_i;
        acc[1][j][r] = base_q;
      }
  } else {
    const MxtWindow w = mxt_window(win_start, win_stop);
    const int h = lane >> 5;
    const u32 span = (u32)max(w.hi0 - w.lo0, 0);
#pragma unroll
    for (int j = 0; j < kMxTiles; j++)
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int q = 32 * (q0_tile + 2 * j) + gpsx_mxt_row(h, r);
        const bool in_win = (u32)(q - w.lo0) < span;   // lo0 <= q < hi0
        acc[0][j][r] = in_win ? base_i : base_i + kOutside;
        acc[1][j][r] = in_win ? base_q : base_q + kOutside;
      }
  }
}

// The even-to-odd switch (the formula in front of mx_half_switch, at b = 0) per chip offset, once per workgroup: what does not
// depend on the PRN but through its chip 1022, hs[c22][q] = (fk + c22 fa) / 8192 for both streams.  Thread t of n: the chip offset
// pairs m = t, t + n, ..: q = 2 m and 2 m + 1 read data bytes 4 m - 1 .. 4 m + 2, one stream word and the one before it, and
// leave as one 16-byte store per row.  (q = 1023 does not exist: its entry is as small as the others, and its hypothesis, started
// outside the window, still clips to zero.)
__device__ __forceinline__ void mxt_half_switch_build(const MxSharedCore &sh, float2 (*hs)[kHsStride], int t, int n)
{
  const int popw[2] = {(int)__popc(sh.d[0][0] & 0xFFu), (int)__popc(sh.d[1][0] & 0xFFu)};
#pragma unroll 1
  for (int m = t; m < 512; m += n) {
    float row[2][2][2];   // [c22][q & 1][stream]
#pragma unroll
    for (int s = 0; s < 2; s++) {
      const u32 w = sh.d[s][m], before = sh.d[s][m > 0 ? m - 1 : 0] >> 24;   // data bytes 4 m .. 4 m + 3; 4 m - 1
#pragma unroll
      for (int k = 0; k < 2; k++) {
        const u32 cur = (w >> (16 * k)) & 0xFFu;                              // data byte 2 q
        // A_7 of the even offset goes, A_0 = 0 of the odd one comes
        int fa = -(2 * (int)__popc(cur & 0x7Fu) - 7);
        int fk = -popw[s];
        if (2 * m + k > 0) {                                                  // T(q): the tail word, data bytes (2 q - 1, 2 q)
          const u32 prev = (k ? (w >> 8) & 0xFFu : before) | (cur << 8);
          fk -= (int)__popc(prev);
          fa -= 16 - 2 * (int)__popc(prev);
        }
        row[0][k][s] = (float)fk * kAccScale;
        row[1][k][s] = (float)(fk + fa) * kAccScale;
      }
    }
#pragma unroll
    for (int c = 0; c < 2; c++)
      *reinterpret_cast<float4 *>(&hs[c][2 * m]) = make_float4(row[c][0][0], row[c][0][1], row[c][1][0], row[c][1][1]);
  }
}

// mx_half_switch for the transposed tile.  A lane's chip 1022 picks its row of the table; the entries of four adjacent chip
// offsets (registers 4 g .. 4 g + 3) are two 16-byte reads, the same address in all lanes of a half and row.  Left per lane: the
// chip[1022 - q] beta_0 term -- chip 1022 - q of PRN lane & 31 is bit lane & 31 of chip_t[1023 - q], four words per read.
// Every term is a multiple of 2^-13 below 2^8 in magnitude: the sums are exact in any order.
__device__ __forceinline__ void mxt_half_switch(const MxSharedCore &sh, const float2 (*hs)[kHsStride], int lane, int q0_tile,
                                                v16f (&acc)[2][kMxTiles], int win_start, int win_stop)
{
  asm volatile("" : "+v"(lane));   // (the addresses below are computed here, not hoisted over the passes into registers they lack)
  const int prn = lane & 31, h = lane >> 5;
  const u32 wrap_i = (sh.d[0][0] & 0xFFu) << 8, wrap_q = (sh.d[1][0] & 0xFFu) << 8;
  const float nbeta_i = -(float)(16 - 2 * (int)__popc(wrap_i)) * kAccScale, nbeta_q = -(float)(16 - 2 * (int)__popc(wrap_q)) * kAccScale;
  // one address per table, constant offsets per (tile, register quad): the chip words run DOWN with q, so theirs is the last quad's
  const int q4_first = 32 * q0_tile + 4 * h, q4_last = q4_first + 64 * (kMxTiles - 1) + 24;
  const float2 *tab = &hs[(sh.chip_t[1022 + 1] >> prn) & 1u][q4_first];
  const u32 *cw = &sh.chip_t[kChips - 3 - q4_last];          // chip_t[1020 - q4 .. 1023 - q4] of the last quad
#pragma unroll
  for (int j = 0; j < kMxTiles; j++) {
#pragma unroll
    for (int g = 0; g < 4; g++) {
      const int dq = 64 * j + 8 * g;                         // registers 4 g + i: chip offsets q4_first + dq + i
      const float4 t01 = *reinterpret_cast<const float4 *>(&tab[dq]), t23 = *reinterpret_cast<const float4 *>(&tab[dq + 2]);
      const uint4 w = *reinterpret_cast<const uint4 *>(&cw[64 * (kMxTiles - 1) + 24 - dq]);
      const float ti[4] = {t01.x, t01.z, t23.x, t23.z}, tq[4] = {t01.y, t01.w, t23.y, t23.w};
      const u32 wi[4] = {w.w, w.z, w.y, w.x};                  // chip_t[1023 - (q4 + i)]
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const float c1 = (float)((wi[i] >> prn) & 1u);
        acc[0][j][4 * g + i] += __builtin_fmaf(c1, nbeta_i, ti[i]);
        acc[1][j][4 * g + i] += __builtin_fmaf(c1, nbeta_q, tq[i]);
      }
    }
  }
  if (!mxt_wave_whole(q0_tile, win_start, win_stop)) {
    // A window edge may fall between the two byte offsets of a chip offset; the accumulators were started for the even one's
    // place.  That happens at two chip offsets at the most: lo1, if only its odd byte offset is inside (an odd win_start), and
    // hi1, if only its even one is (an odd win_stop).  A tile that holds neither is skipped (wave-uniform).
    const MxtWindow w = mxt_window(win_start, win_stop);
    const bool any = win_start < win_stop;
    const int q_in = any && w.lo1 != w.lo0 ? w.lo1 : -1, q_out = any && w.hi1 != w.hi0 ? w.hi1 : -1;
#pragma unroll
    for (int j = 0; j < kMxTiles; j++) {
      const int tile = q0_tile + 2 * j;
      if ((q_in >> 5) != tile && (q_out >> 5) != tile)
        continue;
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int q = 32 * tile + gpsx_mxt_row(h, r);
        const float edge = (q == q_in ? -kOutside : 0.0f) + (q == q_out ? kOutside : 0.0f);
        acc[0][j][r] += edge;
        acc[1][j][r] += edge;
      }
    }
  }
}

// mx_epilogue_single for the transposed tile: the same groups of eight hypotheses (two tiles x four registers), radius test, small
// and exact paths and rounding modes.  The keys are LOCAL -- (root bits << 6) | the register's compile-time code, one
// v_lshl_or_b32 with an inline constant -- and all 64 of a lane belong to ONE (bit shift, PRN): four interleaved chains of
// v_max3_u32 / v_add3_u32 (register rr of every group feeds chain rr: a chain's links are a whole group apart, as the 16 chains
// of mx_epilogue_single are), joined at the end; the winner becomes the global key once, and the wave issues one ds_max_u32 and
// one ds_add_u32, each lane at its own word.  The root bits carry 0x4B000000: it leaves a global key in the shift, and the sum
// starts at -64 x 0x4B000000 (mod 2^32).
//
// TRUST, VERIFY, REDO.  The radius test costs 5 vector instructions and two branches per group and fires only next to a satellite,
// so the lane's 64 hypotheses first go down the small path WITHOUT it (TRUST = true: 7 instructions per hypothesis, issued phase
// by phase -- sixteen clip-squares, eight sums, eight roots, eight fmas, eight keys, the chains -- so that only the chain links
// follow their producers directly), and the joined winner is compared ONCE with the local key of magnitude 1024
// (gpsx_mxt_trust_limit_key).  A hypothesis at or beyond radius 1024 leaves root bits >= kRootBias + 1024 on the small path whatever
// else is wrong with them (the guard factor: the product is never below the true root), and local keys are monotone in the root
// bits below 2^14, so a winner below the limit says that every hypothesis of the lane was inside the small path's proven range.
// If any lane of the wave is at or above it, the wave throws the chains away and runs the group-tested code (TRUST = false: the
// careful path, 7 5/8 per hypothesis) over the same accumulators -- an epilogue changes none of them, and nothing has left the
// registers before the check.  A satellite's peak region spans some 32 consecutive sample offsets of one lane: `hot`, wave-uniform
// and carried from one epilogue of the wave to its next, says that some winner reached magnitude kGpsxMxtHotRadius last time, and
// sends this one down the careful path at once, so a strong signal costs one redo on entry and the careful path's price inside.
// Results never depend on it.
static_assert(kGpsxMxtRootBias == kRootBias, "gpsx_mx_transposed.hpp's limit keys carry the small path's bias");
static_assert(kGpsxMxtHotRadius <= kGpsxMxtTrustRadius, "mxt_epilogue tests the limit only where the predictor's radius is reached");
// The end of a phase of the trust path: all eight values pass through one empty asm statement, so every instruction of the
// next phase is behind every instruction of this one (__builtin_amdgcn_sched_barrier alone does not order the arithmetic, which
// is placed before the scheduler sees it).  With the branch gone the compiler emits the phases in this order by itself; what the
// statement adds is the s_nop 0 the hazard recogniser puts behind an asm statement, five per group.  Measured, not explained
// (EXPERIMENTS round 14, same-box A/B on three boxes): without the fences the kernel is 2.0 % faster than the parent at amplitude
// 0.25 but 0.9 - 1.1 % SLOWER at 1.0; with them 1.6 % faster at 0.25, 1.2 % at 0.5 and 0.2 - 0.4 % at 1.0 -- the form that is
// never slower is the one kept.
template <typename T>
__device__ __forceinline__ void mxt_phase(T (&v)[8])
{
  asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7]));
  __builtin_amdgcn_sched_barrier(0);
}
template <bool TRUST>
__device__ __forceinline__ u32 mxt_chains(const v16f (&acc)[2][kMxTiles], u32 &sum)
{
  u32 best[4], total[4];
#pragma unroll
  for (int c = 0; c < 4; c++) {
    best[c] = 0;
    total[c] = c ? 0u : 0u - (u32)kGpsxMxtLocals * kRootBias;
  }
#pragma unroll
  for (int jp = 0; jp < kMxTiles; jp += 2) {
#pragma unroll
    for (int r0 = 0; r0 < 16; r0 += 4) {
      u32 bits[8];
      if constexpr (TRUST) {
        float si[8], sq[8], ev[8], rt[8];
#pragma unroll
        for (int i = 0; i < 8; i++) {
          si[i] = mx_clip_square(acc[0][jp + (i >> 2)][r0 + (i & 3)]);
          sq[i] = mx_clip_square(acc[1][jp + (i >> 2)][r0 + (i & 3)]);
        }
        mxt_phase(si);
        mxt_phase(sq);
#pragma unroll
        for (int i = 0; i < 8; i++)
          ev[i] = si[i] + sq[i];
        mxt_phase(ev);
#pragma unroll
        for (int i = 0; i < 8; i++)
          rt[i] = __builtin_amdgcn_sqrtf(ev[i]);
        mxt_phase(rt);
#pragma unroll
        for (int i = 0; i < 8; i++)
          bits[i] = __float_as_uint(__builtin_fmaf(rt[i], kRootGuard, 8388608.0f));   // (root_bits_small, a phase apart)
        mxt_phase(bits);
      } else {
        float ev[8];
        u32 e_max = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) {
          ev[i] = clip_square_sum(acc[0][jp + (i >> 2)][r0 + (i & 3)], acc[1][jp + (i >> 2)][r0 + (i & 3)]);
          e_max = max(e_max, __float_as_uint(ev[i]));
        }
        const bool small = __builtin_amdgcn_ballot_w64(e_max >= 0x3C800000u /* 2^20 / 2^26 as f32 */) == 0;
        if (__builtin_expect(small, 1)) {
#pragma unroll
          for (int i = 0; i < 8; i++)
            bits[i] = root_bits_small(ev[i]);
        } else {
          float ci[8], cq[8];
#pragma unroll
          for (int i = 0; i < 8; i++) {
            ci[i] = acc[0][jp + (i >> 2)][r0 + (i & 3)];
            cq[i] = acc[1][jp + (i >> 2)][r0 + (i & 3)];
          }
          mx_roots_exact<8>(ci, cq, bits);
#pragma unroll
          for (int i = 0; i < 8; i++)
            bits[i] += kRootBias;
        }
      }
      u32 key[8];
#pragma unroll
      for (int i = 0; i < 8; i++)
        key[i] = gpsx_mxt_local_key(bits[i], jp + (i >> 2), r0 + (i & 3));
      if constexpr (TRUST)
        mxt_phase(key);
#pragma unroll
      for (int rr = 0; rr < 4; rr++) {
        best[rr] = max(max(best[rr], key[rr]), key[4 + rr]);
        total[rr] = total[rr] + bits[rr] + bits[4 + rr];
      }
      // (pinned in program order, as in mx_epilogue_single)
#pragma unroll
      for (int rr = 0; rr < 4; rr++)
        asm volatile("" : "+v"(best[rr]), "+v"(total[rr]));
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  sum = total[0] + total[1] + total[2] + total[3];
  return max(max(best[0], best[1]), max(best[2], best[3]));
}
// `hot`: in, take the careful path at once; out, some lane's winner reached kGpsxMxtHotRadius (both wave-uniform)
__device__ __forceinline__ void mxt_epilogue(u32 *part, int lane, int q0_tile, int t0, v16f (&acc)[2][kMxTiles], bool &hot)
{
  const int b = t0 & 7, half = t0 >> 3;
  u32 winner = 0, sum = 0;
  bool careful = hot;
  mx_round_toward_zero();
  if (!careful) {
    winner = mxt_chains<true>(acc, sum);
    // (one compare where nothing is near: a winner below the predictor's radius is below the limit)
    hot = __builtin_amdgcn_ballot_w64(winner >= gpsx_mxt_hot_limit_key()) != 0;
    careful = hot && __builtin_amdgcn_ballot_w64(winner >= gpsx_mxt_trust_limit_key()) != 0;
  }
  if (careful) {
    // (the accumulators made opaque: left alone, the compiler keeps the trust path's 64 sums of squares for this path -- in scratch)
#pragma unroll
    for (int s = 0; s < 2; s++)
#pragma unroll
      for (int j = 0; j < kMxTiles; j++)
        asm volatile("" : "+v"(acc[s][j]));
    winner = mxt_chains<false>(acc, sum);
    hot = __builtin_amdgcn_ballot_w64(winner >= gpsx_mxt_hot_limit_key()) != 0;
  }
  mx_round_to_nearest();
  const u32 key = gpsx_mxt_global_key(winner, 32 * q0_tile + 4 * (lane >> 5), half);
  u32 *slot = part + (2 * b) * 64 + lane;   // part[b][0][h][PRN]; the sum 64 words on
  atomicMax(slot, key);
  atomicAdd(slot + 64, sum);
}
__device__ __forceinline__ void mx_fill_fold_lut(MxFold &fold, int t)   // threads 0..63
{
  if (t < 64) {
    const int late = t >> 5, z = t & 31;
    v4i e;
#pragma unroll
    for (int i = 0; i < 4; i++)
      e[i] = (int)(gpsx_fold_pair(late != 0, 2, (z >> i) & 1, (z >> (i + 1)) & 1) << kGpsxFoldShift);
    fold.lut[late][z] = e;
  }
}

__device__ __forceinline__ void mx_single(MxSingleShared &shs, const AcqParams &prm, int cluster_lo,
                                          const uint8_t *__restrict__ if_blocks, const u32 *__restrict__ mx_a,
                                          const u32 *__restrict__ mx_t, gpsx_peak_t *__restrict__ peaks)
{
  MxSharedCore &sh = shs.mx;
  MxFold &fold = shs.fold;
  u32 *part = &shs.part[0][0][0][0];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // (wave-uniform values in SGPRs)
  const int role = wave >> 2;                            // waves w and w + 4 share a SIMD: half a step apart
  const int q0_tile = 8 * (wave >> 1) + (wave & 1);      // this wave owns q-tiles q0_tile + 2 j

  // ---- decode, tables, result slots, block ---------------------------------------------------------------------------------
  const int n_sets = (prm.n_groups + 3) / 4;
  const MxCluster c = mx_decode_cluster(cluster_lo + (int)blockIdx.x, n_sets, prm.n_dopp);
  const int set = c.set, sd = c.sd, dopp = c.dopp, search = c.search;
  u32 group_mask = 0;
#pragma unroll
  for (int g = 0; g < 4; g++) {
    const int group = 4 * set + g;
    const int unit = sd * prm.n_groups + group;
    if (group < prm.n_groups && unit >= prm.unit_lo && unit < prm.unit_hi)
      group_mask |= 1u << g;
  }
  group_mask = (u32)__builtin_amdgcn_readfirstlane((int)group_mask);
  if (group_mask == 0)
    return;
  const u32 step_word = mx_step_word(dopp, prm.if_hz, prm.dopp_min_hz, prm.dopp_step_hz);

  if (set != kMxNoSet) {
    mx_load_tables(sh, mx_a, mx_t, set, tid);   // (t_lut: role 1 fills it in half step 0)
  }
  // (role 0's first epilogue runs in half step 1 -- the zeroes are published by the barrier of half step 0, like the block)
  if (tid < (int)(sizeof(shs.part) / sizeof(uint4)))
    reinterpret_cast<uint4 *>(part)[tid] = make_uint4(0, 0, 0, 0);
  const size_t block_bytes = prm.if_format == GPSX_IF_2BIT_SM ? GPSX_BYTES_PER_MS_2BIT : kBytes;
  const uint8_t *block0 = if_blocks + (size_t)(search * prm.search_stride_blocks) * block_bytes;
  mx_load_block(sh, block0, prm.if_format, tid);

  __syncthreads();
  const int n_pass = kPassesAnchor;
  // (One trip.  Inside a loop the compiler hoists the preamble's per-thread address arithmetic above the barriers, as it does in
  //  mx_unit's block loop, which this form used to run once; without it k_acq_mx<0> comes out 14 instructions longer.)
#pragma unroll 1
  for (int once = 0; once < 1; once++) {
    // all that pass 0 reads: the chips (above), the anchor vector -- from the block sums themselves, in sh.e8[0], which the
    // recurrence's vectors take over behind the barrier that ends the anchor passes -- and pop(D) for the start values
    mx_wipe_stream<true>(sh, step_word, tid, lane);
    __syncthreads();
    mx_anchor_build(sh, &sh.e8[0][0][0][0], tid);

    v16f acc[2][kMxTiles];
    if (role == 0)   // (role 1's start values wait until role 0 is inside pass 0)
      mxt_init_acc(sh.ones, lane, q0_tile, acc, prm.win_start, prm.win_stop, kGpsxAnchorPassBias);

    // (thread indices made opaque per piece: a piece's per-thread addresses are computed where it runs, not hoisted over the
    //  passes into registers that the passes do not have)
    auto opaque = [](int v) {
      asm volatile("" : "+v"(v));
      return v;
    };
    __syncthreads();               // half step 0: the anchor vector, the chips, the block and the result slots' zeroes are in LDS
    if (role) {                    // (threads 256..511; all of it is done before role 0, alone on the matrix pipe, ends its pass)
      mx_planes_half(sh, 0, wave & 3, opaque(lane));
      mx_fill_tables(sh, opaque(tid) & 255, 256);
      mx_fill_fold_lut(fold, opaque(tid) & 255);
      mx_planes_half(sh, 8, wave & 3, opaque(lane));
      mxt_half_switch_build(sh, shs.hs, opaque(tid) & 255, 256);
      mxt_init_acc(sh.ones, opaque(lane), q0_tile, acc, prm.win_start, prm.win_stop, kGpsxAnchorPassBias);
    }
    MxChipRegs chips;              // (filled by the anchor pass, read by every pass after it)
    mx_anchor_pass(sh, &sh.e8[0][0][0][0], lane, q0_tile, acc, chips);
    bool hot = false;              // (the epilogues' predictor: per wave, clear for its first one)
    if (!role)                     // half step 1 of role 0, under role 1's pass
      mxt_epilogue(part, lane, q0_tile, 0, acc, hot);
    __syncthreads();               // half step 2: everybody is done with the anchor vector; the planes, t_lut and hs are published
    mx_vector_build<true>(sh, 2, opaque(tid), &fold);
#pragma unroll 1
    for (int hs = 2; hs <= 2 * n_pass; hs++) {
      if ((hs & 1) == 0) {
        __syncthreads();
        const int p_vec = (hs >> 1) + 1;   // the next step's pass
        if (p_vec < n_pass)
          mx_vector_build<true>(sh, p_vec + 1, tid, &fold);
      }
      const int x = hs - role;   // role-local half step: even = MFMA pass x / 2, odd = epilogue after pass (x - 1) / 2
      const bool active = x >= 0 && x < 2 * n_pass;
      // (pass and epilogue go by the two-pass number p; p == 1 and p < 2 never occur here, but without the tests on them
      //  the compiler schedules the kernel differently: 7728 instructions against 7732)
      const int p = (x >> 1) + 1;
      if (active && (x & 1) == 0) {
        mx_pass<true, kMxTiles, kScaleA, true, kMxChipsResident>(sh, p & 1, lane, q0_tile, acc, p == 1 ? kScaleEight : kScaleOne,
                                                                 v4i{0, 0, 0, 0}, p >= 2 && p != 9, &fold.pair[p & 1][0][0], &chips);
        if (p == 9)
          mxt_half_switch(sh, shs.hs, lane, q0_tile, acc, prm.win_start, prm.win_stop);
      }
      if (active && (x & 1) && p >= 1)
        mxt_epilogue(part, lane, q0_tile, p - 1, acc, hot);
    }
  }
  __syncthreads();
  // the finished triplets and packed keys, as at the end of mx_unit without its SPLIT half; a (bit shift, PRN) cell is two words
  // per field, one per lane half, read directly
  {
    const int which = tid >> 8, p = (tid >> 3) & 31, b = tid & 7;
    const int slot = 32 * set + p;
    const u32 v0 = shs.part[b][which][0][p], v1 = shs.part[b][which][1][p];
    const u32 k = v0 > v1 ? v0 : v1, t = v0 + v1;   // (which = 0: the keys' maximum counts, which = 1: the sums' sum)
    if (((group_mask >> (p >> 3)) & 1u) && slot < prm.n_prn && b < prm.n_bits) {
      const size_t idx = ((size_t)(search * prm.n_prn + slot) * prm.n_dopp + dopp) * prm.n_bits + b;
      uint2 *pk = reinterpret_cast<uint2 *>(&peaks[idx]);
      if (which == 0) {
        const u32 max_val = k >> 11;
        pk[0] = make_uint2(max_val, max_val ? 2047u - (k & 2047u) : 0u);   // gpsx_peak_t: max_val, phase
      } else {
        pk[1] = make_uint2(t, t / (2u * kChips));                          //              sum, avr
      }
    }
    // the packed key of (search, PRN, Doppler) -- (energy << 14) | (16383 - fine phase) of the best bit shift, what k_acq_keys
    // makes of the triplets -- while they are in registers (unsharded launches: prm.keys is null otherwise)
    if (prm.keys && which == 0) {   // (wave-uniform: waves 0..3; a PRN's eight bit shifts are eight adjacent lanes)
      unsigned long long key = 0;
      if (b < prm.n_bits) {
        const u32 max_val = k >> 11, phase = max_val ? 2047u - (k & 2047u) : 0u;
        key = ((unsigned long long)max_val << 14) | (unsigned long long)(16383u - (8u * phase + (u32)b));
      }
      key = mx_max8_u64(key);
      if (b == 0 && ((group_mask >> (p >> 3)) & 1u) && slot < prm.n_prn)
        prm.keys[(size_t)(search * prm.n_prn + slot) * prm.n_dopp + dopp] = (int64_t)key;
    }
  }
}

// ---- the forms that start a block in two passes (kPasses): kMxSplit, kMxWalk16, kMxWalk, kMxStore --------------------------------
// kMxWalk16: the workgroup walks the blocks of its search, running sums as 16-bit records in HBM scratch; `flags`[workgroup] tells
// whether a sum outgrew them.  kMxWalk: the same with 24-bit records: launched behind kMxWalk16, a workgroup does its cluster again
// if its flag is up and leaves otherwise.  kMxStore: a workgroup per (cluster, block), magnitudes out as u16 for k_acq_vals_search:
// the form for few multi-block searches.  kMxSplit: see SPLIT below.
template <int MODE>
__device__ __forceinline__ void mx_unit(MxShared &sh, const AcqParams &prm, int cluster_lo,
                                        const uint8_t *__restrict__ if_blocks, const u32 *__restrict__ mx_a,
                                        const u32 *__restrict__ mx_t, gpsx_peak_t *__restrict__ peaks, u32 *__restrict__ energy,
                                        u32 *__restrict__ flags)
{
  constexpr bool MULTI = MODE == kMxWalk || MODE == kMxWalk16, STORE = MODE == kMxStore, S16 = MODE == kMxWalk16;
  // SPLIT: the single-block fine grid for launches that leave most of the chip idle -- two workgroups per cluster, sample offsets
  // 0..7 and 8..15, the second one started directly at offset 8 (as the byte-phase form does); their search results meet in
  // two global u32 planes (`energy` = packed keys, behind them the sums: atomicMax / atomicAdd) that k_acq_finalize converts
  constexpr bool SPLIT = MODE == kMxSplit;
  typedef SumRecT<S16> SumRec;
  const int wg = (int)blockIdx.x;
  if constexpr (MODE == kMxWalk) {
    if (flags && flags[wg] == 0)   // (uniform: the 16-bit run of this cluster was exact)
      return;
  }
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // (wave-uniform values in SGPRs)
  const int role = wave >> 2;                            // waves w and w + 4 share a SIMD: half a step apart
  const int q0_tile = 8 * (wave >> 1) + (wave & 1);      // this wave owns q-tiles q0_tile + 2 j

  // ---- decode: cluster = (search, Doppler, set of 32 PRN slots); its four 8-PRN groups are sharding units -----------
  const int n_sets = (prm.n_groups + 3) / 4;
  const int ms_store = STORE ? wg % prm.n_ms : 0;
  const int n_seg = SPLIT ? prm.split_segs : 1;          // SPLIT: workgroups per cluster (2, 4 or 8) ...
  const int seg = SPLIT ? wg % n_seg : 0;   // ... and which run of 16 / n_seg sample offsets this one has
  const MxCluster c = mx_decode_cluster(cluster_lo + (STORE ? wg / prm.n_ms : SPLIT ? wg / n_seg : wg), n_sets, prm.n_dopp);
  const int set = c.set, sd = c.sd, dopp = c.dopp, search = c.search;
  u32 group_mask = 0;
#pragma unroll
  for (int g = 0; g < 4; g++) {
    const int group = 4 * set + g;
    const int unit = sd * prm.n_groups + group;
    if (group < prm.n_groups && unit >= prm.unit_lo && unit < prm.unit_hi)
      group_mask |= 1u << g;
  }
  group_mask = (u32)__builtin_amdgcn_readfirstlane((int)group_mask);
  if (group_mask == 0)
    return;
  const u32 step_word = mx_step_word(dopp, prm.if_hz, prm.dopp_min_hz, prm.dopp_step_hz);

  // tables of the cluster (the persistent form keeps them while the set stays the same)
  if (set != kMxNoSet) {
    mx_load_tables(sh, mx_a, mx_t, set, tid);
    mx_fill_tables(sh, tid);
  }
  for (int i = tid; i < 8 * 32 * 2 * 32 / 4; i += kMxThreads)
    reinterpret_cast<uint4 *>(&sh.part[0][0][0][0])[i] = make_uint4(0, 0, 0, 0);
  const size_t block_bytes = prm.if_format == GPSX_IF_2BIT_SM ? GPSX_BYTES_PER_MS_2BIT : kBytes;
  const uint8_t *block0 = if_blocks + (size_t)(search * prm.search_stride_blocks + (STORE ? wg % prm.n_ms : 0)) * block_bytes;
  mx_load_block(sh, block0, prm.if_format, tid);

  __syncthreads();
  // A operand of the extra K step: column 0 of lane half 0 = chip 1022 of PRN (lane & 31), of half 1 = chip 1021
  const v4i a_corr = v4i{(int)(((sh.chip_t[(lane >> 5 ? 1021 : 1022) + 1] >> (lane & 31)) & 1u) << 1), 0, 0, 0};
  u32 kq[kMxTiles];   // 2047 - (even byte offset of the lane's chip offset in tile j): the low field of its search keys
#pragma unroll
  for (int j = 0; j < kMxTiles; j++) {
    kq[j] = (u32)(2047 - 2 * (32 * (q0_tile + 2 * j) + (lane & 31)));
    if constexpr (!MULTI && !STORE)
      asm volatile("" : "+v"(kq[j]));   // (kept in registers, not rebuilt per group; the other forms do not use them)
  }
  u32 *e_wave = MULTI ? energy + ((size_t)wg * 8 + wave) * (16 * kMxTiles * 4 * 64 * (S16 ? 2 : 3)) : nullptr;   // dwords per record
  const u32 *zero_recs = MULTI ? flags - kMxZeroRecBytes / sizeof(u32) : nullptr;   // (the launcher put them in front of the flags)
  u32 witness = 0;   // S16: OR of every sum this lane stored
  const int n_ms = MULTI ? prm.n_ms : 1;
  // SPLIT: two direct passes at sample offset t0s, then 16 / n_seg - 1 steps of the walk (local pass lp >= 2 is pass t0s + lp)
  const int t0s = SPLIT ? seg * (16 / n_seg) : 0;
  const int n_pass = SPLIT ? 16 / n_seg + 1 : kPasses;
  const int pbase = t0s;
#pragma unroll 1
  for (int ms = 0; ms < n_ms; ms++) {
    const bool ms_first = ms == 0, ms_last = ms == n_ms - 1;
    // (the walk forms: thread indices made opaque per block, so that the preamble's per-thread address arithmetic is redone
    //  per block instead of being hoisted out of this loop into registers that the step loop below then has to spill)
    int tid_p = tid, lane_p = lane;
    if constexpr (MULTI)
      asm volatile("" : "+v"(tid_p), "+v"(lane_p));
    if (ms > 0) {
      __syncthreads();   // the previous block's readers are done
      mx_load_block(sh, block0 + (size_t)ms * block_bytes, prm.if_format, tid_p);
      __syncthreads();
    }
    if (SPLIT && seg) {
      mx_wipe_block(sh, step_word, tid_p, lane_p);
      // not the first run: the first two vectors from the block sums of sample offset t0s (the planes' barrier is the loop's first)
      mx_vector_build_direct(sh, 0, t0s, &sh.e8[0][0][0][0], tid);
      mx_vector_build_direct(sh, 1, t0s, &sh.e8[1][0][0][0], tid);
      for (int i = tid; i < 2 * 2 * 2 * 128; i += kMxThreads)
        (&sh.corr[0][0][0][0])[i] = 0;
    } else {
      mx_wipe_block(sh, step_word, tid_p, lane_p);
      __syncthreads();
      // the first two vectors (from the popcounts of sample offset 0), by the two-phase builders
      mx_vector_phase1(sh, 0, 0, tid_p);
      __syncthreads();
      mx_vector_phase2(sh, 0, tid_p);
      __syncthreads();
      mx_vector_phase1(sh, 1, 1, tid_p);
      __syncthreads();
      mx_vector_phase2(sh, 1, tid_p);
    }

    v16f acc[2][kMxTiles];
    mx_init_acc(sh.ones, lane_p, q0_tile, acc, prm.win_start, prm.win_stop);
    SumRec pre[MULTI ? 16 : 1];

    // Steps of two halves: role 0 runs pass p, then the epilogue of sample offset p - 1; role 1 the epilogue of sample
    // offset p - 2, then pass p -- one wave of a SIMD on the matrix pipe while the other has the vector ALU, with nothing
    // but their own pace between the halves: ONE barrier per step, where all eight waves build the vector of pass p + 1
    // into the buffer that both roles read during step p - 1.
    //
    // Passes 0 and 1 produce no sample offset, so in half steps 0..3 the roles take strict turns and each has slots with no work.
#pragma unroll 1
    for (int hs = 0; hs <= 2 * n_pass; hs++) {
      if ((hs & 1) == 0)
        __syncthreads();
      // The vector of the next step: built behind the barrier by everybody (single-block forms), or behind this step's epilogue
      // by the role that just finished one (walk forms: each role's threads own one stream of the vector -- threads 0..255 =
      // waves 0..3 = I, 256..511 = Q --, the buffer it goes into was last read in the previous step, and the barrier that opens
      // the next step publishes it).  Same-box A/B: behind the epilogue is 1.5 % faster for the walk form (whose epilogue waits
      // on HBM anyway) and 1.8 % slower for the single-block form -- the step is bound by the SIMD's issue port, not by the
      // barrier: moving the work does not shorten it.
      constexpr bool kBuildBehindEpilogue = MULTI;
      if (!kBuildBehindEpilogue && (hs & 1) == 0) {
        const int p_vec = (hs >> 1) + 1;
        if (p_vec >= 2 && p_vec < n_pass) {
          int tid_v = tid;
          if constexpr (MULTI)
            asm volatile("" : "+v"(tid_v));   // (as above: the builder's addresses are not worth registers across the passes)
          mx_vector_build(sh, pbase + p_vec, tid_v);
        }
      }
      int lane_s = lane;         // (walk forms: opaque per half step, see tid_p -- record addresses are recomputed, not spilled)
      if constexpr (MULTI)
        asm volatile("" : "+v"(lane_s));
      const int x = hs - role;   // role-local half step: even = MFMA pass x / 2, odd = epilogue after pass (x - 1) / 2
      const bool active = x >= 0 && x < 2 * n_pass;
      const int p = x >> 1;
      if (active && (x & 1) == 0) {
        if constexpr (MULTI) {
          if (p >= 1)
            mx_prefetch_sums<0, 8, S16>(e_wave, zero_recs, lane_s, p - 1, ms_first, pre);
        }
        mx_pass<!MULTI>(sh, p & 1, lane, q0_tile, acc, p == 1 ? kScaleEight : kScaleOne, a_corr, p >= 2 && (SPLIT || p != 9));
        if constexpr (SPLIT) {
          if (p == 1 && seg) {
            int lane_d = lane;   // (opaque: the terms' per-lane addresses are not worth registers across the step loop)
            asm volatile("" : "+v"(lane_d));
            mx_direct_terms(sh, lane_d, q0_tile, acc, t0s, prm.win_start, prm.win_stop);
          }
        } else {
          if (p == 9)
            mx_half_switch(sh, lane_s, q0_tile, acc, prm.win_start, prm.win_stop);
        }
      }
      if (STORE) {
        if (active && (x & 1) && p >= 1) {
          uint16_t *plane0 = reinterpret_cast<uint16_t *>(energy) +
                             ((size_t)((search * prm.n_ms + ms_store) * prm.n_prn + 32 * set) * prm.n_dopp + dopp) * (16 * 1024);
          mx_epilogue_store(lane, q0_tile, p - 1, acc, group_mask, plane0, (size_t)prm.n_dopp * (16 * 1024), 32 * set, prm.n_prn);
        }
      } else if (active && (x & 1) && p >= 1) {
        if (!MULTI)
          mx_epilogue_single(sh, lane, kq, t0s + p - 1, acc);
        else if (!ms_last)
          mx_epilogue<MULTI, false, S16>(sh, lane_s, q0_tile, p - 1, acc, group_mask, e_wave, zero_recs, pre, ms_first, witness);
        else
          mx_epilogue<MULTI, true, S16>(sh, lane_s, q0_tile, p - 1, acc, group_mask, e_wave, zero_recs, pre, ms_first, witness);
      }
      if (kBuildBehindEpilogue && (x & 1) != 0) {
        const int p_vec = (hs >> 1) + 1;
        if (p_vec >= 2 && p_vec < n_pass) {
          int tid_v = tid;
          if constexpr (MULTI)
            asm volatile("" : "+v"(tid_v));
          mx_vector_build(sh, pbase + p_vec, tid_v);
        }
      }
    }
  }
  if (STORE)
    return;   // k_acq_vals_search sums the blocks and searches
  if constexpr (S16) {
    // did any stored sum need more than 16 bits?  (sh.ones is free after the last block's preamble)
    if (tid == 0)
      sh.ones[0] = 0;
    __syncthreads();
    if (__builtin_amdgcn_ballot_w64(witness >= 0xFFFFu) != 0 && lane == 0)
      atomicOr(&sh.ones[0], 1u);
  }
  __syncthreads();
  if constexpr (S16) {
    if (tid == 0)
      flags[wg] = sh.ones[0];
    if (sh.ones[0])
      return;   // (uniform) the second kernel does this cluster again and writes its triplets
  }
  // the finished triplets: one per (PRN, bit shift); threads 0..255 fold the 32 lane slots of the maxima and write
  // (max, phase), threads 256..511 those of the sums and write (sum, avr)
  {
    const int which = tid >> 8, p = (tid >> 3) & 31, b = tid & 7;
    const int slot = 32 * set + p;
    const u32 *row = sh.part[b][p][which];
    u32 vals[32];
#pragma unroll
    for (int l = 0; l < 32; l++)
      vals[l] = row[(l + tid) & 31];   // (rotated start: the threads of a wave spread over the banks)
    u32 k = 0, t = 0;
#pragma unroll
    for (int l = 0; l < 32; l++) {
      k = vals[l] > k ? vals[l] : k;
      t += vals[l];
    }
    if (((group_mask >> (p >> 3)) & 1u) && slot < prm.n_prn && b < prm.n_bits) {
      const size_t idx = ((size_t)(search * prm.n_prn + slot) * prm.n_dopp + dopp) * prm.n_bits + b;
      uint2 *pk = reinterpret_cast<uint2 *>(&peaks[idx]);
      if constexpr (SPLIT) {   // the runs of a cluster meet in the planes: keys [0, n), sums [n, 2 n)
        const size_t n_planes = (size_t)prm.n_planes;
        if (which == 0)
          atomicMax(&energy[idx], k);
        else
          atomicAdd(&energy[n_planes + idx], t);
      } else if (which == 0) {
        const u32 max_val = k >> 11;
        pk[0] = make_uint2(max_val, max_val ? 2047u - (k & 2047u) : 0u);   // gpsx_peak_t: max_val, phase
      } else {
        pk[1] = make_uint2(t, t / (2u * kChips));                          //              sum, avr
      }
    }
    // the packed key of (search, PRN, Doppler) -- (energy << 14) | (16383 - fine phase) of the best bit shift, what k_acq_keys
    // makes of the triplets -- while they are in registers (unsharded launches: prm.keys is null otherwise)
    if constexpr (!SPLIT) {
      if (prm.keys && which == 0) {   // (wave-uniform: waves 0..3; a PRN's eight bit shifts are eight adjacent lanes)
        unsigned long long key = 0;
        if (b < prm.n_bits) {
          const u32 max_val = k >> 11, phase = max_val ? 2047u - (k & 2047u) : 0u;
          key = ((unsigned long long)max_val << 14) | (unsigned long long)(16383u - (8u * phase + (u32)b));
        }
        key = mx_max8_u64(key);
        if (b == 0 && ((group_mask >> (p >> 3)) & 1u) && slot < prm.n_prn)
          prm.keys[(size_t)(search * prm.n_prn + slot) * prm.n_dopp + dopp] = (int64_t)key;
      }
    }
  }
}

}  // namespace

template <int MODE>
__global__ __launch_bounds__(kMxThreads, 1) void k_acq_mx(GPSX_K_ACQ_MX_PARAMS)
{
  if constexpr (MODE == kMxSingle) {
    __shared__ MxSingleShared sh;
    mx_single(sh, prm, cluster_lo, if_blocks, mx_a, mx_t, peaks);
  } else {
    __shared__ MxShared sh;
    mx_unit<MODE>(sh, prm, cluster_lo, if_blocks, mx_a, mx_t, peaks, energy, flags);
  }
}

// plan_acq (gpsx_acq_plan.hpp) decides the form, its grids and split_segs (in prm); this issues its launch sequence
void launch_acq_mx(hipStream_t s, const AcqPlan &p, const AcqParams &prm, const uint8_t *d_if, const uint32_t *d_mx_a,
                   const uint32_t *d_mx_t, uint32_t *d_planes, uint32_t *d_energy)
{
  if (p.c_hi <= p.c_lo)
    return;
  const dim3 grid((unsigned)p.grid), block(kMxThreads);
  gpsx_peak_t *d_peaks = prm.peaks;
  switch (p.form) {
  case AcqForm::kMxStore:
    hipLaunchKernelGGL(k_acq_mx<kMxStore>, grid, block, 0, s, prm, p.c_lo, d_if, d_mx_a, d_mx_t, d_peaks, d_energy, (u32 *)nullptr);
    launch_acq_vals_search(s, prm, reinterpret_cast<const uint16_t *>(d_energy), d_peaks, p.n_peaks);
    break;
  case AcqForm::kMxWalk: {
    u32 *d_flags = d_energy + acq_mx_energy_bytes(p.grid) / sizeof(u32) - p.grid;   // (the flags sit behind the records)
    (void)hipMemsetAsync(d_flags - kMxZeroRecBytes / sizeof(u32), 0, kMxZeroRecBytes, s);   // the first block's "previous sums"
    hipLaunchKernelGGL(k_acq_mx<kMxWalk16>, grid, block, 0, s, prm, p.c_lo, d_if, d_mx_a, d_mx_t, d_peaks, d_energy, d_flags);
    if (p.walk24)   // redoes the clusters whose flag went up
      hipLaunchKernelGGL(k_acq_mx<kMxWalk>, grid, block, 0, s, prm, p.c_lo, d_if, d_mx_a, d_mx_t, d_peaks, d_energy, d_flags);
    break;
  }
  case AcqForm::kMxByte:
    launch_acq_mx_byte(s, (unsigned)p.grid, prm, p.c_lo, d_if, d_mx_a, d_mx_t);
    break;
  case AcqForm::kMxSplit:
    hipLaunchKernelGGL(k_acq_mx<kMxSplit>, grid, block, 0, s, prm, p.c_lo, d_if, d_mx_a, d_mx_t, d_peaks, d_planes, (u32 *)nullptr);
    launch_acq_finalize(s, d_planes, d_planes + p.n_peaks, p.n_peaks, d_peaks, prm.keys);
    break;
  default:   // kMxSingle, and kMxTail's full rounds (their workgroups write their keys in their folds, k_acq_finalize_from the tail's)
    hipLaunchKernelGGL(k_acq_mx<kMxSingle>, grid, block, 0, s, prm, p.c_lo, d_if, d_mx_a, d_mx_t, d_peaks, (u32 *)nullptr,
                       (u32 *)nullptr);
    if (p.form != AcqForm::kMxTail)
      break;
    hipLaunchKernelGGL(k_acq_mx<kMxSplit>, dim3((unsigned)p.grid_tail), block, 0, s, prm, p.c_tail, d_if, d_mx_a, d_mx_t, d_peaks,
                       d_planes, (u32 *)nullptr);
    launch_acq_finalize_from(s, d_planes, d_planes + p.n_peaks, p.first_peak, p.n_peaks, d_peaks, prm.n_prn, prm.n_dopp,
                             prm.n_bits, (prm.n_groups + 3) / 4, p.c_tail, prm.keys);
  }
}

}  // namespace gpsx
