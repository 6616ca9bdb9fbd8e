// gpsx_kernels.hpp -- host-visible launch interface of the HIP kernels (implemented in k_*.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/gpsx.h"
#include "gpsx_acq_plan.hpp"

namespace gpsx {

constexpr int kCodeWords = 256;   // 4-chip code words per PRN (1023 chips + 1 masked pad)

// One search = one workgroup pass: `count` (<= group size) consecutive code-table slots, one carrier frequency,
// one replica bit shift, n_ms consecutive blocks.
struct AcqJobRec {
  int32_t block;        // first IF block
  int32_t slot;         // first code-table slot
  float freq_hz;        // IF + Doppler
  int32_t offset_bits;  // replica shift b
  int32_t win_start, win_stop;
  int32_t out_index;    // index of slot 0's result
};

struct AcqParams {
  // arithmetic job decode (grid mode, jobs == nullptr)
  int32_t n_ms;
  int32_t search_stride_blocks;
  int32_t n_prn, n_groups, n_dopp, dopp_min_hz, dopp_step_hz;
  int32_t n_bits;
  int32_t unit_lo, unit_hi;   // this shard's run of sharding units
  int32_t win_start, win_stop;
  int32_t if_format;        // GPSX_IF_1BIT / GPSX_IF_2BIT_SM
  int32_t if_hz;            // gpsx_config_t.if_hz: centre of the Doppler axis
  // from the plan (gpsx_acq_plan.hpp), read by the k_acq_mx forms named:
  int32_t split_segs;       //   k_acq_mx<5>: workgroups per cluster (2, 4 or 8)
  int32_t n_clusters;       //   k_acq_mx<4>: clusters of the launch (one persistent workgroup per CU walks them)
  uint64_t n_planes;        //   k_acq_mx<5>: entries per result plane (packed keys [0, n), sums [n, 2 n) behind `energy`)
  // explicit job list (job mode)
  const AcqJobRec *jobs;
  // outputs (optional ones may be null)
  gpsx_peak_t *peaks;
  int64_t *keys;            // k_acq_mx: packed keys written next to the triplets (unsharded launches; null: k_acq_keys follows)
  gpsx_peak_t *per_ms;
  uint32_t *energy;
  uint16_t *cnt;
};

// K1: Gold codes + derived tables for `n_slots` code-table slots (padded slots have prn 0 -> all-zero tables).
//   chips    [n_slots][1024]  0/1 bytes
//   chipbits [n_slots][32]    packed, bit (i & 31) of word (i >> 5) = chip i
//   cw8      [n_slots/group][128][group]  8 chips per word as 0/1 nibbles (pad chip 1023 = 0)
void launch_build_codes(hipStream_t s, const uint8_t *d_prns, int n_slots, int group, uint8_t *d_chips,
                        uint32_t *d_chipbits, uint32_t *d_cw8);

// K2+K3+K4 fused acquisition search.  group = kAcqGroup (grid; local_units = sharding units of this rank) or 1 (job
// list; local_units = jobs).  d_cw8: the cw8 table of launch_build_codes.
void launch_acq(hipStream_t s, int group, long local_units, const AcqParams &prm, const uint8_t *d_if, const uint32_t *d_cw8,
                const uint32_t *d_chipbits);
// The fine grid (and k_acq_mx's byte-phase grid) without inspection outputs: plan_acq (gpsx_acq_plan.hpp) decides the form, its
// grids and scratch; these launchers issue the plan's launch sequence.  d_planes: 2 * plan.n_peaks u32 (keys, then sums; all-zero
// between launches: k_acq_finalize* puts back what it reads), d_energy: plan.energy_bytes.  d_peaks = prm.peaks.
// Polyphase variant (k_acq_poly.hip): AND + popcount recurrence across the 16 sample offsets.
void launch_acq_poly(hipStream_t s, const AcqPlan &plan, const AcqParams &prm, const uint8_t *d_if, const uint32_t *d_cw8,
                     const uint32_t *d_chipbits, uint32_t *d_planes, uint32_t *d_energy);
// Matrix-core variant (k_acq_mx.hip, k_acq_mx_byte.hip): one 512-thread workgroup per (search, Doppler, 32 PRN slots).  Tables: mx_a [sets][4096]
// A fragments, mx_t [sets][1032] transposed chip words (launch_build_mx_tables).
void launch_build_mx_tables(hipStream_t s, const uint32_t *d_chipbits, int n_slots, uint32_t *d_mx_a, uint32_t *d_mx_t);
void launch_acq_mx(hipStream_t s, const AcqPlan &plan, const AcqParams &prm, const uint8_t *d_if, const uint32_t *d_mx_a,
                   const uint32_t *d_mx_t, uint32_t *d_planes, uint32_t *d_energy);
void launch_acq_finalize_from(hipStream_t s, uint32_t *d_keyacc, uint32_t *d_sumacc, size_t first, size_t n_peaks,
                              gpsx_peak_t *d_peaks, int n_prn, int n_dopp, int n_bits, int n_sets, int cluster_from,
                              int64_t *d_keys_opt = nullptr);   // d_keys_opt (n_bits = 8): the packed keys as well
void launch_acq_vals_search(hipStream_t s, const AcqParams &prm, const uint16_t *d_vals, gpsx_peak_t *d_peaks, size_t n_peaks);
void launch_acq_finalize(hipStream_t s, uint32_t *d_keyacc, uint32_t *d_sumacc, size_t n_peaks,
                         gpsx_peak_t *d_peaks, int64_t *d_keys_opt = nullptr);

// keys[unit pair] = max over bit shifts of (max_val << 14 | 16383 - (8 * phase + b)); 0 for pairs of other shards
void launch_acq_keys(hipStream_t s, const gpsx_peak_t *d_peaks, int64_t *d_keys, int n_search, int n_prn, int n_groups,
                     int n_dopp, int n_bits, int unit_lo, int unit_hi);

// generic per-call primitives on caller-shaped buffers
void launch_wipeoff(hipStream_t s, const uint8_t *d_signal, float freq_hz, uint32_t accum_in, uint8_t *d_i,
                    uint8_t *d_q, uint32_t *d_accum_out);
void launch_replica(hipStream_t s, const uint8_t *d_chips, unsigned offset_bits, uint16_t *d_out);
void launch_corr_offsets(hipStream_t s, const uint8_t *d_rep, const uint8_t *d_i, const uint8_t *d_q,
                         const uint16_t *d_offsets, int first_offset, int n, uint16_t *d_cnt_i, uint16_t *d_cnt_q,
                         int16_t *d_corr8);
void launch_mag8(hipStream_t s, const uint16_t *d_cnt_i, const uint16_t *d_cnt_q, int n, int16_t *d_out,
                 uint32_t *d_disagree);
void launch_search_reduce(hipStream_t s, const int16_t *d_corr8, int n, int first_offset, gpsx_peak_t *d_peak);

// K2+K3+K5 tracking correlators, one workgroup per channel
// d_bad_prn (may be null): set to 1 by a channel whose PRN is outside 1..210 (it correlates against the empty code)
// d_trk_rep: the replica bit streams of every PRN slot (launch_build_track_rep), read by the wave-per-channel form
void launch_track_epl(hipStream_t s, const uint8_t *d_if_block, int if_format, int if_hz, gpsx_trk_state_t *d_st, int n_ch,
                      const uint8_t *d_chips, const uint32_t *d_chipbits, const uint32_t *d_trk_rep, int16_t *d_iq,
                      uint32_t *d_bad_prn, int wave_from);
constexpr int kTrackRepStride = 1032;   // words per PRN row of d_trk_rep
void launch_build_track_rep(hipStream_t s, const uint32_t *d_chipbits_all, int n_slots, uint32_t *d_rep);
// extension: the acquisition grid on weighted two-bit samples (k_acq_weighted.hip); -1 if the kernel's LDS size is refused
int launch_acq_weighted(hipStream_t s, const uint8_t *d_if_blocks, int n_search, int stride_blocks, int n_prn,
                        const uint8_t *d_chips_all, const uint8_t *d_prns, int if_hz, int dopp_min_hz, int dopp_step_hz, int n_dopp,
                        int use_magnitude, gpsx_peak_t *d_peaks);
// the same grid on the matrix cores (k_acq_mxw.hip: k_acq_mxw): d_mx_a = the chip tables of the sign-only grid (launch_build_mx_tables)
void launch_acq_mxw(hipStream_t s, const uint8_t *d_if_blocks, int n_search, int stride_blocks, int n_prn, const uint32_t *d_mx_a,
                    int if_hz, int dopp_min_hz, int dopp_step_hz, int n_dopp, int use_magnitude, gpsx_peak_t *d_peaks);
// gpsx_acq_grid_weighted_ms (plan_acq_weighted): clusters [cluster_lo, + n_clusters) walk n_ms blocks each, d_scratch = n_clusters x
// kMxwMsClusterBytes (k_acq_wmx_ms) / the vector-ALU form, running sums in registers (k_acq_weighted_ms; -1: LDS size refused)
void launch_acq_mxw_ms(hipStream_t s, const uint8_t *d_if_blocks, int stride_blocks, int n_ms, int n_prn, const uint32_t *d_mx_a, int if_hz,
                       int dopp_min_hz, int dopp_step_hz, int n_dopp, int use_magnitude, int cluster_lo, int n_clusters, void *d_scratch,
                       gpsx_peak_t *d_peaks);
int launch_acq_weighted_ms(hipStream_t s, const uint8_t *d_if_blocks, int n_search, int stride_blocks, int n_ms, int n_prn,
                           const uint8_t *d_chips_all, const uint8_t *d_prns, int if_hz, int dopp_min_hz, int dopp_step_hz, int n_dopp,
                           int use_magnitude, gpsx_peak_t *d_peaks);
// gpsx_acq_grid_weighted_coh (plan_acq_coherent, n_coh >= 2): k_acq_coh_mx (mx: a workgroup per 32-PRN cluster) or k_acq_coh_vec
// (a workgroup per 8 PRNs); neither needs scratch
void launch_acq_coh(hipStream_t s, bool mx, const uint8_t *d_if_blocks, int n_search, int stride_blocks, int n_coh, int n_prn,
                    const uint8_t *d_chips_all, const uint8_t *d_prns, int if_hz, int dopp_min_hz, int dopp_step_hz, int n_dopp,
                    int use_magnitude, gpsx_peak_t *d_peaks);
// gpsx_acq_grid_weighted_hyb (plan_acq_hybrid, n_coh >= 2 and n_seg >= 2; k_acq_hyb.hip): k_acq_hyb_mx -- clusters [cluster_lo,
// + n_clusters) walk n_seg windows of n_coh blocks each, d_scratch = n_clusters x kMxwMsClusterBytes -- or k_acq_hyb_vec, running
// sums in registers, no scratch
void launch_acq_hyb_mx(hipStream_t s, const uint8_t *d_if_blocks, int stride_blocks, int n_coh, int n_seg, int n_prn,
                       const uint8_t *d_chips_all, const uint8_t *d_prns, int if_hz, int dopp_min_hz, int dopp_step_hz, int n_dopp,
                       int use_magnitude, int cluster_lo, int n_clusters, void *d_scratch, gpsx_peak_t *d_peaks);
void launch_acq_hyb_vec(hipStream_t s, const uint8_t *d_if_blocks, int n_search, int stride_blocks, int n_coh, int n_seg, int n_prn,
                        const uint8_t *d_chips_all, const uint8_t *d_prns, int if_hz, int dopp_min_hz, int dopp_step_hz, int n_dopp,
                        int use_magnitude, gpsx_peak_t *d_peaks);
// extension: gpsx_track_epl_weighted (k_track_weighted.hip) -- E/P/L on weighted two-bit samples, n_blocks 4092-byte blocks x n_ch
// channels in one launch, d_iq [n_blocks][n_ch][6] int32; every channel's accumulator is advanced by n_blocks blocks (at
// n_blocks >= 2 by k_track_weighted_advance behind the correlators).  d_bad_prn as launch_track_epl's.
void launch_track_epl_weighted(hipStream_t s, const uint8_t *d_if_blocks_2bit, int n_blocks, int if_hz, int use_magnitude, int spacing,
                               gpsx_trk_state_t *d_st, int n_ch, const uint32_t *d_trk_rep, int32_t *d_iq, uint32_t *d_bad_prn);
// extension: gpsx_track_loop_weighted (k_track_loop_weighted.hip: k_track_wloop) -- the closed DLL / PLL / FLL on weighted two-bit
// samples: n_blocks 4092-byte blocks (a multiple of cfg.n_coh) one after the other inside one launch, d_rec [n_blocks / n_coh][n_ch];
// the states are read once and written once.  d_bad_prn as launch_track_epl's.
void launch_track_loop_weighted(hipStream_t s, const uint8_t *d_if_blocks_2bit, int n_blocks, int if_hz, const gpsx_wloop_cfg_t &cfg,
                                gpsx_wloop_state_t *d_st, int n_ch, const uint32_t *d_trk_rep, gpsx_wloop_rec_t *d_rec,
                                uint32_t *d_bad_prn);
// extension: gpsx_track_loop_weighted_sync (k_track_loop_weighted_sync.hip: k_track_wsync) -- the same loop with a 20 ms bit
// synchroniser per channel and bit-aligned windows: any n_blocks, the open window in the state (448 bytes per channel),
// d_rec [ceil(n_blocks / min(n_coh_search, n_coh_lock))][n_ch], every byte of it written.  d_bad_prn as launch_track_epl's.
void launch_track_loop_weighted_sync(hipStream_t s, const uint8_t *d_if_blocks_2bit, int n_blocks, int if_hz, const gpsx_wsync_cfg_t &cfg,
                                     gpsx_wsync_state_t *d_st, int n_ch, const uint32_t *d_trk_rep, gpsx_wsync_rec_t *d_rec,
                                     uint32_t *d_bad_prn);
// extension: gpsx_track_loop_weighted_aided / _sync_aided (k_track_waid_loop, k_track_waid_sync: the two kernels' bodies instantiated
// with the carrier aiding clause of gpsx_track_wloop_parts.hpp's window_update, in the same files) -- everything as the two launches
// above; code_per_hz: samples of code phase per second and Hz of carrier offset (0: the unaided bytes).
void launch_track_loop_weighted_aided(hipStream_t s, const uint8_t *d_if_blocks_2bit, int n_blocks, int if_hz, const gpsx_wloop_cfg_t &cfg,
                                      float code_per_hz, gpsx_wloop_state_t *d_st, int n_ch, const uint32_t *d_trk_rep, gpsx_wloop_rec_t *d_rec,
                                      uint32_t *d_bad_prn);
void launch_track_loop_weighted_sync_aided(hipStream_t s, const uint8_t *d_if_blocks_2bit, int n_blocks, int if_hz, const gpsx_wsync_cfg_t &cfg,
                                           float code_per_hz, gpsx_wsync_state_t *d_st, int n_ch, const uint32_t *d_trk_rep,
                                           gpsx_wsync_rec_t *d_rec, uint32_t *d_bad_prn);
// extension: gpsx_track_loop_weighted_sync_multi (k_track_loop_weighted_sync_multi.hip: k_track_wsync_multi, the sync kernel's text a
// third time) -- n_rx receivers with ch_per_rx (1 .. 64) channel slots each in one launch, a workgroup per receiver: receiver r reads
// the n_blocks blocks that start rx_stride_blocks (>= n_blocks) 4092-byte blocks behind receiver r - 1's.  d_st [n_rx ch_per_rx] and
// d_rec [slots][n_rx ch_per_rx] are the single-stream launch's arrays; code_per_hz 0: the unaided bytes.
void launch_track_loop_weighted_sync_multi(hipStream_t s, const uint8_t *d_if_blocks_2bit, int n_blocks, int if_hz, const gpsx_wsync_cfg_t &cfg,
                                           float code_per_hz, int n_rx, int ch_per_rx, int rx_stride_blocks, gpsx_wsync_state_t *d_st,
                                           const uint32_t *d_trk_rep, gpsx_wsync_rec_t *d_rec, uint32_t *d_bad_prn);
// extension: gpsx_wnav_words (k_wnav_words.hip: k_wnav_words) -- LNAV frame sync and parity-checked words from the [n_slots][n_ch]
// records launch_track_loop_weighted_sync wrote for n_blocks blocks: one channel per lane, 64-byte frame states in HBM,
// d_words [n_blocks / 600 + 2][n_ch], every byte of it written.  d_bad_state (may be null): set to 1 by a channel whose state
// words are out of range.
void launch_wnav_words(hipStream_t s, const gpsx_wsync_rec_t *d_rec, int n_slots, int n_blocks, int max_bad_words, gpsx_wnav_state_t *d_st,
                       int n_ch, gpsx_wnav_word_t *d_words, uint32_t *d_bad_state);
// extension: gpsx_wobs (k_wobs.hip: k_wobs) -- every channel's transmit time at the launch's end, from the same [n_slots][n_ch]
// records and the [n_blocks / 600 + 2][n_ch] word records launch_wnav_words made of them: one channel per lane, 80-byte states in
// HBM, d_obs [n_ch], every byte of it written.  d_bad_state (may be null): set to 1 by a channel whose state is out of range.
void launch_wobs(hipStream_t s, const gpsx_wsync_rec_t *d_rec, int n_slots, int n_blocks, float edge_guard, const gpsx_wnav_word_t *d_words,
                 gpsx_wobs_state_t *d_st, int n_ch, gpsx_wobs_t *d_obs, uint32_t *d_bad_state);
// extension: gpsx_weph (k_weph.hip: k_weph) -- every channel's broadcast ephemeris from the [n_blocks / 600 + 2][n_ch] word records
// launch_wnav_words wrote: one channel per lane, 192-byte states in HBM, d_eph [n_ch] 256-byte records, every byte of them written.
// d_bad_state (may be null): set to 1 by a channel whose state is out of range.
void launch_weph(hipStream_t s, const gpsx_wnav_word_t *d_words, int n_blocks, gpsx_weph_state_t *d_st, int n_ch, gpsx_weph_t *d_eph,
                 uint32_t *d_bad_state);
// extension: gpsx_wlock (k_wlock.hip: k_wlock) -- every channel's code-lock, carrier-lock and C/N0 indicators from the same
// [n_slots][n_ch] records: one channel per lane, 128-byte states in HBM, d_lock [n_ch] 64-byte records, every byte of them written.
// d_sync_st (null unless cfg.rearm): the sync loop's states, written where a re-arm is due.  d_bad_state (may be null): set to 1 by
// a channel whose state is out of range.
void launch_wlock(hipStream_t s, const gpsx_wsync_rec_t *d_rec, int n_slots, int n_blocks, const gpsx_wlock_cfg_t &cfg, gpsx_wlock_state_t *d_st,
                  gpsx_wsync_state_t *d_sync_st, int n_ch, gpsx_wlock_t *d_lock, uint32_t *d_bad_state);
// extension: gpsx_wfix (k_wfix.hip: k_wfix) -- every receiver's position fix from the [n_rx * ch_per_rx] observables and ephemeris
// records (and lock records, d_lock may be null) of the stages above: one slot per lane, a receiver a group of lanes, no state;
// d_prev (may be null, may be d_fix) [n_rx] start points, d_fix [n_rx] 128-byte records and d_pr_m (may be null) [n_rx * ch_per_rx],
// every byte of them written.  cfg as the host checked it.
void launch_wfix(hipStream_t s, const gpsx_wfix_cfg_t &cfg, const gpsx_wobs_t *d_obs, const gpsx_weph_t *d_eph, const gpsx_wlock_t *d_lock,
                 const gpsx_wfix_t *d_prev, int n_rx, gpsx_wfix_t *d_fix, double *d_pr_m);
// extension: gpsx_wfde (k_wfde.hip: k_wfde) -- launch_wfix's fixes with the ambiguous millisecond repaired and faulty slots excluded:
// the same arrays and lane layout, rounds of the solver per receiver; d_fde [n_rx] 64-byte records, every byte of them written.
// cfg as the host checked it.
void launch_wfde(hipStream_t s, const gpsx_wfde_cfg_t &cfg, const gpsx_wobs_t *d_obs, const gpsx_weph_t *d_eph, const gpsx_wlock_t *d_lock,
                 const gpsx_wfix_t *d_prev, int n_rx, gpsx_wfix_t *d_fix, gpsx_wfde_t *d_fde, double *d_pr_m);
// extension: gpsx_wvel (k_wvel.hip: k_wvel) -- every receiver's velocity and clock drift from the same [n_rx * ch_per_rx] arrays and
// the [n_rx] position records of launch_wfix / launch_wfde: the same lane layout, one linear solve, no state; d_vel [n_rx] 112-byte
// records, every byte of them written.  cfg as the host checked it.
void launch_wvel(hipStream_t s, const gpsx_wvel_cfg_t &cfg, const gpsx_wobs_t *d_obs, const gpsx_weph_t *d_eph, const gpsx_wlock_t *d_lock,
                 const gpsx_wfix_t *d_fix, int n_rx, gpsx_wvel_t *d_vel);
// extension: gpsx_wkf (k_wkf.hip: k_wkf) -- every receiver's navigation filter on the same [n_rx * ch_per_rx] arrays: the same lane
// layout, a resident 384-byte state per receiver in d_state [n_rx]; d_fix and d_vel (each may be null) [n_rx] are read by receivers
// that are not initialised; d_kf [n_rx] 240-byte records, every byte of them written.  A state that is out of range raises
// *d_bad_state.  cfg and n_blocks as the host checked them.
void launch_wkf(hipStream_t s, const gpsx_wkf_cfg_t &cfg, const gpsx_wobs_t *d_obs, const gpsx_weph_t *d_eph, const gpsx_wlock_t *d_lock,
                const gpsx_wfix_t *d_fix, const gpsx_wvel_t *d_vel, int n_rx, int n_blocks, gpsx_wkf_state_t *d_state, gpsx_wkf_t *d_kf,
                uint32_t *d_bad_state);
// extension: gpsx_wacq (k_wacq.hip: k_wacq) -- acquisition decisions and slot hand-over between a weighted grid's records d_peaks
// [n_rx][n_prn][n_dopp] and the [n_rx * ch_per_rx] states of the sync loop and of the four stages behind it (d_lock_st null only
// with evict_after_blocks == 0; d_nav_st, d_obs_st, d_eph_st may be null): a wave per receiver, no state of its own; prns: the
// grid's n_prn (<= 64) PRN numbers in HOST memory, passed by value; d_acq [n_rx] 64-byte records and d_det (may be null)
// [n_rx][n_prn] 16-byte records, every byte of them written.  cfg and the grid as the host checked them: the launcher checks nothing again.
void launch_wacq(hipStream_t s, const gpsx_wacq_cfg_t &cfg, int n_rx, int n_prn, const uint8_t *prns, int dopp_min_hz, int dopp_step_hz, int n_dopp,
                 const gpsx_peak_t *d_peaks, gpsx_wsync_state_t *d_sync_st, gpsx_wlock_state_t *d_lock_st, gpsx_wnav_state_t *d_nav_st,
                 gpsx_wobs_state_t *d_obs_st, gpsx_weph_state_t *d_eph_st, gpsx_wacq_t *d_acq, gpsx_wacq_det_t *d_det);
// extension: gpsx_wbank (k_wbank.hip: k_wbank) -- the ephemeris bank behind gpsx_weph: d_bank [n_rx][n_prn] takes the newest VALID record
// of d_eph [n_rx * ch_per_rx] per listed PRN (the slots' PRNs from d_sync_st, read only), d_eph_out (may be null, may be d_eph) the
// records with the bank's where a slot has none of its own, d_rep [n_rx] 32-byte records, every byte written.  A wave per receiver;
// prns: n_prn (<= 64) PRN numbers in HOST memory, passed by value.  The launcher checks nothing again.
void launch_wbank(hipStream_t s, const gpsx_wbank_cfg_t &cfg, int n_rx, int n_prn, const uint8_t *prns, const gpsx_wsync_state_t *d_sync_st,
                  const gpsx_weph_t *d_eph, gpsx_weph_t *d_bank, gpsx_weph_t *d_eph_out, gpsx_wbank_t *d_rep);
// extension: gpsx_wpred (k_wpred.hip: k_wpred) -- prediction and hot hand-over behind gpsx_wkf: from the filter states d_kf_state [n_rx]
// and the bank d_bank [n_rx][n_prn] (both read only) every listed PRN's elevation, pseudorange, code phase and Doppler lead_blocks after
// the state's rcv_ms; with cfg.handover the visible, certain and untracked ones go to free slots of the five state arrays (as
// launch_wacq's: d_lock_st null only with evict_after_blocks == 0; d_nav_st, d_obs_st, d_eph_st may be null).  d_rx [n_rx] and d_pred
// (may be null) [n_rx][n_prn] 64-byte records, every byte written.  A wave per receiver; prns in HOST memory, by value.  No checks.
void launch_wpred(hipStream_t s, const gpsx_wpred_cfg_t &cfg, int n_rx, int n_prn, const uint8_t *prns, const gpsx_wkf_state_t *d_kf_state,
                  const gpsx_weph_t *d_bank, gpsx_wsync_state_t *d_sync_st, gpsx_wlock_state_t *d_lock_st, gpsx_wnav_state_t *d_nav_st,
                  gpsx_wobs_state_t *d_obs_st, gpsx_weph_state_t *d_eph_st, gpsx_wpred_rx_t *d_rx, gpsx_wpred_t *d_pred);
// extension: gpsx_wtow (k_wtow.hip: k_wtow) -- time-of-week aiding behind gpsx_wobs and gpsx_wpred: from launch_wpred's records d_pred_rx
// [n_rx] and d_pred [n_rx][n_prn] (read only) the anchor of every [n_rx * ch_per_rx] observable state d_obs_st whose chain runs without
// one; d_sync_st is read for the slots' PRNs and written only with cfg.rearm; d_obs (may be null) [n_rx * ch_per_rx]: tx_ms and flags of
// the slots whose state changed.  d_tow [n_rx * ch_per_rx] 32-byte and d_tow_rx [n_rx] 64-byte records, every byte written.  A wave
// per receiver; prns in HOST memory, by value.  No checks.
void launch_wtow(hipStream_t s, const gpsx_wtow_cfg_t &cfg, int n_rx, int n_prn, const uint8_t *prns, const gpsx_wpred_rx_t *d_pred_rx,
                 const gpsx_wpred_t *d_pred, gpsx_wsync_state_t *d_sync_st, gpsx_wobs_state_t *d_obs_st, gpsx_wobs_t *d_obs, gpsx_wtow_t *d_tow,
                 gpsx_wtow_rx_t *d_tow_rx);
// extension: gpsx_walm (k_walm.hip: k_walm) -- almanac, ionosphere and UTC behind gpsx_wnav_words, beside launch_weph on the same word
// records d_words [n_blocks / 600 + 2][n_rx * ch_per_rx]: a resident 64-byte state per slot in d_slot_st [n_rx * ch_per_rx], a
// resident 1120-byte bank per receiver in d_bank [n_rx]; d_rx [n_rx] 160-byte and d_alm (may be null) [n_rx][32] 96-byte records,
// every byte of them written.  A wave per receiver.  A slot state or a bank that is out of range raises *d_bad_state.  No checks.
void launch_walm(hipStream_t s, const gpsx_walm_cfg_t &cfg, const gpsx_wnav_word_t *d_words, int n_blocks, int n_rx, gpsx_walm_slot_t *d_slot_st,
                 gpsx_walm_bank_t *d_bank, gpsx_walm_rx_t *d_rx, gpsx_walm_sv_t *d_alm, uint32_t *d_bad_state);
// extension: gpsx_acq_window_weighted (k_acq_win.hip: k_acq_win) -- the weighted grid's energy in a window around each prediction: from
// launch_wpred's records d_pred [n_rx][n_prn] (read only) and the receivers' blocks (receiver r from block r * stride_blocks, cfg.n_coh *
// cfg.n_seg of them) the records d_peaks [n_rx][n_prn][n_dopp] and the reports d_rep (may be null) [n_rx][n_prn], every byte of them
// written.  A workgroup per (receiver, PRN index, bin of the 2 * half_bins + 1), receivers in chunks where a launch would count more
// than 2^32 - 1 threads (2^24 - 1 workgroups); prns: n_prn (<= 64) PRN numbers in HOST memory, passed by value.  No HBM scratch.  The launcher checks nothing again.
void launch_acq_win(hipStream_t s, const gpsx_acq_window_t &cfg, const uint8_t *d_if_blocks, int n_rx, int stride_blocks, int n_prn,
                    const uint8_t *prns, const uint8_t *d_chips_all, int if_hz, int dopp_min_hz, int dopp_step_hz, int n_dopp, int use_magnitude,
                    const gpsx_wpred_t *d_pred, gpsx_peak_t *d_peaks, gpsx_acq_window_rep_t *d_rep);
// extension: gpsx_wsnap (k_wsnap.hip: k_wsnap) -- snapshot fixes behind a weighted grid: from the records d_peaks [n_rx][n_prn][n_dopp], the
// bank d_bank (record (r, p) at r * bank_stride + p; bank_stride n_prn or 0) and the priors d_prior [n_rx] (all read only) a position, a
// common bias and a corrected time of week per receiver: d_snap [n_rx] 128-byte and d_sv (may be null) [n_rx][n_prn] 48-byte records,
// every byte of them written.  A wave per receiver, no state of its own.  cfg and the grid as the host checked them.  No checks.
void launch_wsnap(hipStream_t s, const gpsx_wsnap_cfg_t &cfg, int n_rx, int n_prn, int dopp_min_hz, int dopp_step_hz, int n_dopp,
                  const gpsx_peak_t *d_peaks, const gpsx_weph_t *d_bank, int bank_stride, const gpsx_wsnap_prior_t *d_prior, gpsx_wsnap_t *d_snap,
                  gpsx_wsnap_sv_t *d_sv);
// GPSX_DRAWS_LIBC (include/gpsx.h): a channel's false-lock jump reported by the first pass / its carrier candidate for the second
// (ms_from: the millisecond of the launch at which the channel's state in HBM is valid -- 0, or, under the multiplex, the first
//  millisecond of the slot it stopped in: its earlier slots of the launch were stored when they ended -- the replay starts there)
struct gpsx_loop_event_t { int32_t channel, ms, if_freq_i16, found_freq_hz, ms_from; };
struct gpsx_loop_reseed_t { int32_t ms, candidate, ms_from; };   // ms < 0: none
void launch_loop_scatter_reseeds(hipStream_t s, gpsx_loop_reseed_t *d_table, const int *d_channels, const gpsx_loop_reseed_t *d_cand, int n);
void launch_track_loop(hipStream_t s, const uint8_t *d_if_blocks, uint32_t block_stride, int n_blocks, int if_format, int if_hz,
                       gpsx_loop_state_t *d_st, int n_ch, uint32_t first_tick, int schedule, int word_sync,
                       const uint32_t *d_chipbits, const uint32_t *d_trk_rep, uint8_t *d_flags, gpsx_loop_trace_t *d_trace,
                       uint32_t *d_bad_prn, const int *d_ch_map, int n_map, const gpsx_loop_reseed_t *d_reseeds,
                       gpsx_loop_event_t *d_events, uint32_t *d_n_events);
void launch_loop_set_polarity(hipStream_t s, gpsx_loop_state_t *d_st, const int *d_channels, const uint8_t *d_values, int n);
constexpr int kTrackPadPrn = -2147483647 - 1;   // gpsx_trk_state_t.prn of a padding channel: the empty code, not an error
// N3: 2-bit sign/magnitude samples -> two 1-bit planes
void launch_unpack2(hipStream_t s, const uint8_t *d_in, int n_blocks, uint8_t *d_sign, uint8_t *d_mag);
void launch_rewind(hipStream_t s, int if_hz, gpsx_trk_state_t *d_st, int n_ch, const uint8_t *d_steps);

}  // namespace gpsx
