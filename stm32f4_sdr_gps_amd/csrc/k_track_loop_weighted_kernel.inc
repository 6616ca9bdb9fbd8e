// k_track_loop_weighted_kernel.inc -- the text of k_track_wloop and of its carrier-aided twin k_track_waid_loop:
// k_track_loop_weighted.hip includes it twice,
// with GPSX_WLOOP_KERNEL the kernel's name and GPSX_WLOOP_AIDED 0 / 1.  One copy of the block loop; the aided kernel has one more
// argument (code_per_hz) and window_update's aiding clause (gpsx_track_wloop_parts.hpp), nothing else.  A text, not a template
// function that two thin kernels call: inlined into a kernel that form changed k_track_wsync's block loop (other exec-mask
// handling around the record stores; profiles/r16_waid_unaided_isa.txt), and this one leaves both unaided kernels as they were.
__global__ __launch_bounds__(256, 4) void GPSX_WLOOP_KERNEL(const uint8_t *__restrict__ if_blocks, int n_blocks, int if_hz, gpsx_wloop_cfg_t cfg,
                                                     gpsx_wloop_state_t *__restrict__ st, int n_ch, int cpw,
                                                     const u32 *__restrict__ rep_all, gpsx_wloop_rec_t *__restrict__ rec,
                                                     u32 *__restrict__ bad_prn
#if GPSX_WLOOP_AIDED
                                                     , float code_per_hz
#endif
)
{
#if !GPSX_WLOOP_AIDED
  constexpr float code_per_hz = 0.0f;   // (not read: window_update<false> has no aiding clause)
#endif
  using namespace trkweighted;
  using namespace trkwloop;
  __shared__ __attribute__((aligned(16))) u32 s_x[2][512], s_m[2][512];   // this and the next block's planes
  __shared__ uint2 s_carrier[4];
  const Lanes l = lanes_of(n_ch, cpw);   // gpsx_track_wloop_parts.hpp, like everything the two loops share
  const int lane = l.lane, k_l = l.k_l, n_here = l.n_here, ch_l = l.ch_l;
  const bool in_wave = l.in_wave(), mine = l.mine();
  const int use_magnitude = cfg.weights == GPSX_WEIGHTS_SIGN_MAGNITUDE;
  const int n_coh = cfg.n_coh;
  const float T = (float)n_coh * 0.001f;
  const Gains gains = {cfg.dll_c1, cfg.dll_c2, cfg.pll_c1, cfg.pll_c2, cfg.fll_c, T};   // (launch constants: so are dll_c2 * T and pll_c2 * T)

  fill_carrier(s_carrier);

  Live s = {};
  int prn_ok = 0;   // the validated PRN; 0: outside 1 .. 210 (reported here); -1: a padding channel (never reported)
  if (n_here)
    prn_ok = load_state(&st[ch_l], l, bad_prn, s);

  // a window's tau, PRN and step.  This kernel's rule: every lane of the wave keeps its channel's PRN (those beyond the wave's
  // channels mirror its first), and a bad phase is reported for every channel but a padding one (prn_ok >= 0).
  Window w;
  auto rule = [&](bool phase_ok) {
    w.prn = phase_ok && prn_ok > 0 ? prn_ok : 0;
    if (!phase_ok && mine && k_l == 0 && bad_prn && prn_ok >= 0)
      *bad_prn = 1u;
  };
  begin_window(w, s, if_hz, rule);
  int sum_i = 0, sum_q = 0;   // lane 4 c + k: tap k's window sums
  int in_win = 0, window = 0;

#pragma unroll 1
  for (int b = 0; b < n_blocks; b++) {
    stage_planes(if_blocks + (size_t)b * GPSX_BYTES_PER_MS_2BIT, use_magnitude, s_x[b & 1], s_m[b & 1]);
    __syncthreads();
    if (!n_here)   // (wave-uniform)
      continue;
    u32 pop_m;
    const u32 counts = wave_counts(s_x[b & 1], s_m[b & 1], s_carrier, lane, n_here, w.prn, w.tau, cfg.spacing, w.step, s.if_freq_accum, rep_all, pop_m);
    int res_i = 0, res_q = 0;
    if (mine)
      finish_tap(s_carrier, lane, w.prn, w.tau, cfg.spacing, w.step, s.if_freq_accum, rep_all, counts, pop_m, res_i, res_q);
    sum_i += res_i;
    sum_q += res_q;
    s.if_freq_accum += w.step * (u32)kWords32;
    if (++in_win < n_coh)   // (uniform over the launch)
      continue;

    // ---- the window's end: the quad gathers its six sums, every lane of it runs the loop ---------------------------------------
    const int IE = quad_get<0>(sum_i), QE = quad_get<0>(sum_q), IP = quad_get<1>(sum_i), QP = quad_get<1>(sum_q);
    const int IL = quad_get<2>(sum_i), QL = quad_get<2>(sum_q);
    if (w.prn != 0)   // (a bad channel: floats and loop memory stay as they were)
      window_update<GPSX_WLOOP_AIDED != 0>(s, gains, IE, QE, IP, QP, IL, QL, code_per_hz);
    if (in_wave && k_l == 0) {
      gpsx_wloop_rec_t r;
      r.iq[0] = IE; r.iq[1] = QE; r.iq[2] = IP; r.iq[3] = QP; r.iq[4] = IL; r.iq[5] = QL;
      r.code_phase_fine = s.code_phase_fine;
      r.if_freq_offset_hz = s.if_freq_offset_hz;
      r.if_freq_accum = s.if_freq_accum;
      rec[(size_t)window * (size_t)n_ch + (size_t)ch_l] = r;
    }
    window++;
    in_win = 0;
    sum_i = sum_q = 0;
    begin_window(w, s, if_hz, rule);   // the next window
  }
  if (in_wave && k_l == 0)
    __builtin_memcpy(&st[ch_l].code_phase_fine, &s, sizeof s);
}
