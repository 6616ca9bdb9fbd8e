// k_track_loop_weighted_sync_kernel.inc -- the text of k_track_wsync and of its carrier-aided twin k_track_waid_sync:
// k_track_loop_weighted_sync.hip includes it twice,
// with GPSX_WSYNC_KERNEL the kernel's name and GPSX_WSYNC_AIDED 0 / 1.  One copy of the block loop; the aided kernel has one more
// argument (code_per_hz) and window_update's aiding clause (gpsx_track_wloop_parts.hpp), nothing else.
// k_track_loop_weighted_sync_multi.hip includes it a third time, as k_track_wsync_multi, with GPSX_WSYNC_AIDED 1 and GPSX_WSYNC_MULTI
// defined: two more arguments and other PLACES -- a workgroup is a receiver, its lanes' channels come from that file's lanes_of_rx, the
// blocks are the receiver's own -- and no other line.  There n_ch is the record pitch alone (n_rx ch_per_rx), not the lanes' bound.
// A text, not a template
// function that two thin kernels call: inlined into a kernel that form changed k_track_wsync's block loop (other exec-mask
// handling around the record stores; profiles/r16_waid_unaided_isa.txt), and this one leaves both unaided kernels as they were.
__global__ __launch_bounds__(256, 4) void GPSX_WSYNC_KERNEL(const uint8_t *__restrict__ if_blocks, int n_blocks, int if_hz, gpsx_wsync_cfg_t cfg,
                                                     gpsx_wsync_state_t *__restrict__ st, int n_ch, int cpw,
                                                     const u32 *__restrict__ rep_all, gpsx_wsync_rec_t *__restrict__ rec,
                                                     u32 *__restrict__ bad_prn
#if GPSX_WSYNC_AIDED
                                                     , float code_per_hz
#endif
#ifdef GPSX_WSYNC_MULTI
                                                     , int ch_per_rx, size_t rx_stride_bytes
#endif
)
{
#if !GPSX_WSYNC_AIDED
  constexpr float code_per_hz = 0.0f;   // (not read: window_update<false> has no aiding clause)
#endif
  using namespace trkweighted;
  using namespace trkwloop;
  __shared__ __attribute__((aligned(16))) u32 s_x[2][512], s_m[2][512];   // this and the next block's planes
  __shared__ uint2 s_carrier[4];
#ifdef GPSX_WSYNC_MULTI
  const Lanes l = lanes_of_rx(ch_per_rx, cpw);   // ch_l counts over all receivers: the state and record bases are in it
  if_blocks += (size_t)blockIdx.x * rx_stride_bytes;
#else
  const Lanes l = lanes_of(n_ch, cpw);   // gpsx_track_wloop_parts.hpp, like everything the two loops share
#endif
  const int lane = l.lane, k_l = l.k_l, n_here = l.n_here, ch_l = l.ch_l;
  const bool in_wave = l.in_wave(), mine = l.mine();
  const int use_magnitude = cfg.weights == GPSX_WEIGHTS_SIGN_MAGNITUDE;
  const int span = min(cfg.n_coh_search, cfg.n_coh_lock);
  const int decide_at = 20 * (cfg.sync_bits + 1);
  gpsx_wsync_state_t *const my = st + ch_l;

  fill_carrier(s_carrier);

  Live s = {};
  int sum_i = 0, sum_q = 0;   // lane 4 c + k: tap k's sums over the open window (win_iq[2 k], [2 k + 1])
  int win_n = 0, ms = 0, mode = 0, edge = 0, bit_ip = 0, search_n = 0;
  int p_i = 0, p_q = 0;       // the round's running prompt: the quad's Prompt lane (k = 1) alone keeps it
  int prn_ok = 0;             // the validated PRN; 0: a bad channel (reported here); -1: a padding channel (never reported)
  if (n_here) {
    prn_ok = load_state(&my->loop, l, bad_prn, s);
    if (k_l < 3) {
      sum_i = my->win_iq[2 * k_l];
      sum_q = my->win_iq[2 * k_l + 1];
    }
    win_n = my->win_n; ms = my->ms_count; mode = my->mode; edge = my->edge;
    bit_ip = my->bit_ip; search_n = my->search_n;
    p_i = my->p_i; p_q = my->p_q;
    // the caller's words: out of range -> a bad channel, like a bad PRN
    if ((unsigned)mode > 2u || (unsigned)ms >= 20u || (unsigned)edge >= 20u || (unsigned)win_n > 20u || (unsigned)search_n > 4020u) {
      if (prn_ok > 0 && mine && k_l == 0 && bad_prn)
        *bad_prn = 1u;
      prn_ok = prn_ok < 0 ? -1 : 0;
    }
  }

  // tau, PRN and step of a window, in registers: from the state's floats, which change at a window's end only.  This kernel's rule,
  // unlike k_track_wloop's: the lanes beyond the wave's channels (they mirror its first) get PRN 0 -- they must not act -- and a bad
  // phase is reported for a good channel only (prn_ok > 0).
  Window w;
  auto rule = [&](bool phase_ok) {
    w.prn = in_wave && phase_ok && prn_ok > 0 ? prn_ok : 0;
    if (!phase_ok && mine && k_l == 0 && bad_prn && prn_ok > 0)
      *bad_prn = 1u;
  };
  begin_window(w, s, if_hz, rule);
  int slot = 0, in_slot = 0;
  bool wrote = false;   // a window of this channel ended in the current slot

#pragma unroll 1
  for (int b = 0; b < n_blocks; b++) {
    stage_planes(if_blocks + (size_t)b * GPSX_BYTES_PER_MS_2BIT, use_magnitude, s_x[b & 1], s_m[b & 1]);
    __syncthreads();
    if (!n_here)   // (wave-uniform)
      continue;
    const bool ok = w.prn != 0;
    if (ok && mode == GPSX_WSYNC_WAIT && ms == edge)
      mode = GPSX_WSYNC_LOCKED;   // this block is a bit's first
    const bool corr = ok && mode != GPSX_WSYNC_WAIT;
    u32 pop_m;
    const u32 counts = wave_counts(s_x[b & 1], s_m[b & 1], s_carrier, lane, n_here, w.prn, w.tau, cfg.spacing, w.step, s.if_freq_accum, rep_all, pop_m);
    int res_i = 0, res_q = 0;
    if (mine)
      finish_tap(s_carrier, lane, w.prn, w.tau, cfg.spacing, w.step, s.if_freq_accum, rep_all, counts, pop_m, res_i, res_q);
    if (corr) {
      sum_i += res_i;
      sum_q += res_q;
      win_n++;
    }
    s.if_freq_accum += w.step * (u32)kWords32;
    bool ends = false, decide = false;
    if (ok) {
      ms = ms == 19 ? 0 : ms + 1;
      if (mode == GPSX_WSYNC_SEARCH) {
        if (k_l == 1) {   // this lane's res_i, res_q ARE the block's prompt: the prefix form touches one candidate per block
          p_i = (int)((u32)p_i + (u32)res_i);
          p_q = (int)((u32)p_q + (u32)res_q);
          int2 *bp = reinterpret_cast<int2 *>(&my->base[ms][0]);
          if (search_n >= 20) {
            const int2 old = *bp;
            const long long di = (int)((u32)p_i - (u32)old.x), dq = (int)((u32)p_q - (u32)old.y);
            unsigned long long *ep = reinterpret_cast<unsigned long long *>(&my->e[ms]);
            *ep = *ep + (unsigned long long)(di * di) + (unsigned long long)(dq * dq);
          }
          *bp = int2{p_i, p_q};
        }
        search_n++;
        decide = search_n >= decide_at;
      }
      const bool locked = mode == GPSX_WSYNC_LOCKED;
      ends = corr && (win_n >= (locked ? cfg.n_coh_lock : cfg.n_coh_search) || (locked && ms == edge));
    }

    // ---- a window's end, for the lanes whose channel has one: the quad gathers its six sums, every lane of it runs the loop ------
    if (__builtin_amdgcn_ballot_w64(ends) != 0) {   // (wave-uniform: every lane is active for the quad exchanges)
      const int IE = quad_get<0>(sum_i), QE = quad_get<0>(sum_q), IP = quad_get<1>(sum_i), QP = quad_get<1>(sum_q);
      const int IL = quad_get<2>(sum_i), QL = quad_get<2>(sum_q);
      if (ends) {
        const bool locked = mode == GPSX_WSYNC_LOCKED;
        const gpsx_wsync_gains_t g = locked ? cfg.lock : cfg.search;
        const float T = (float)win_n * 0.001f;
        window_update<GPSX_WSYNC_AIDED != 0>(s, Gains{g.dll_c1, g.dll_c2, g.pll_c1, g.pll_c2, g.fll_c, T}, IE, QE, IP, QP, IL, QL, code_per_hz);
        // the bit's prompt sum and the record
        u32 flags = GPSX_WSYNC_WINDOW;
        int bit_out = 0;
        if (locked) {
          flags |= GPSX_WSYNC_LOCKED_FLAG;
          bit_ip = (int)((u32)bit_ip + (u32)IP);
          if (ms == edge) {
            flags |= GPSX_WSYNC_BIT;
            bit_out = bit_ip;
            bit_ip = 0;
          }
        }
        if (k_l < 3) {
          Rec16 v;
          if (k_l == 0)
            v = Rec16{{(u32)IE, (u32)QE, (u32)IP, (u32)QP}};
          else if (k_l == 1)
            v = Rec16{{(u32)IL, (u32)QL, __float_as_uint(s.code_phase_fine), __float_as_uint(s.if_freq_offset_hz)}};
          else
            v = Rec16{{s.if_freq_accum, (u32)b, flags, (u32)bit_out}};
          reinterpret_cast<Rec16 *>(&rec[(size_t)slot * (size_t)n_ch + (size_t)ch_l])[k_l] = v;
        }
        wrote = true;
        sum_i = sum_q = 0;
        win_n = 0;
        begin_window(w, s, if_hz, rule);   // the next window
      }
    }

    // ---- the search's decision, for the lanes whose channel has seen 20 (sync_bits + 1) blocks ---------------------------------
    if (__builtin_amdgcn_ballot_w64(decide) != 0) {   // (wave-uniform)
      int best = 0, accept = 0;
      if (decide && k_l == 1) {
        long long e_best = my->e[0];
#pragma unroll 1
        for (int c = 1; c < 20; c++) {
          const long long v = my->e[c];
          if (v > e_best) {
            e_best = v;
            best = c;
          }
        }
        const long long opp = my->e[best < 10 ? best + 10 : best - 10];
        accept = best + 1 == my->prev_best_p1 && (long long)((unsigned long long)e_best * (unsigned long long)cfg.sync_den) >=
                                                     (long long)((unsigned long long)opp * (unsigned long long)cfg.sync_num);
        my->last_best_e = e_best;
        my->last_opp_e = opp;
        my->prev_best_p1 = best + 1;
        my->sync_rounds = (int)((u32)my->sync_rounds + 1u);
#pragma unroll 1
        for (int c = 0; c < 20; c++)
          my->e[c] = 0;
        p_i = p_q = 0;
      }
      best = quad_get<1>(best);
      accept = quad_get<1>(accept);
      if (decide) {
        search_n = 0;
        if (accept) {   // wait for the edge; the open window is discarded
          edge = best;
          mode = GPSX_WSYNC_WAIT;
          sum_i = sum_q = 0;
          win_n = 0;
          bit_ip = 0;
          s.n_updates = 0;
        }
      }
    }

    // ---- the slot's end: a channel without a window in it gets the empty pattern -------------------------------------------------
    if (++in_slot == span || b == n_blocks - 1) {   // (uniform over the launch)
      if (mine && !wrote)
        reinterpret_cast<Rec16 *>(&rec[(size_t)slot * (size_t)n_ch + (size_t)ch_l])[k_l] = Rec16{{0u, k_l == 2 ? ~0u : 0u, 0u, 0u}};
      wrote = false;
      in_slot = 0;
      slot++;
    }
  }

  if (mine) {
    my->win_iq[2 * k_l] = sum_i;
    my->win_iq[2 * k_l + 1] = sum_q;
    if (k_l == 0) {
      __builtin_memcpy(&my->loop.code_phase_fine, &s, sizeof s);
      my->win_n = win_n; my->ms_count = ms; my->mode = mode; my->edge = edge;
      my->bit_ip = bit_ip; my->search_n = search_n;
    }
    if (k_l == 1) {
      my->p_i = p_i;
      my->p_q = p_q;
    }
  }
}
