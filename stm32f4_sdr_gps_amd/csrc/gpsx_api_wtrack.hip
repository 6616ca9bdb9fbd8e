// gpsx_api_wtrack.hip -- the C ABI of the weighted two-bit tracking chain (include/gpsx.h): gpsx_track_epl_weighted,
// gpsx_track_loop_weighted, gpsx_track_loop_weighted_sync (and the carrier-aided form of each, _aided), gpsx_track_loop_weighted_sync_multi, gpsx_wnav_words, gpsx_wobs, gpsx_weph, gpsx_wlock, gpsx_wfix, gpsx_wfde, gpsx_wvel, gpsx_wkf, gpsx_wacq, gpsx_wbank, gpsx_wpred, gpsx_wtow, gpsx_walm, gpsx_wsnap, gpsx_acq_window_weighted (the grid in a window around gpsx_wpred's records: it stands in the chain, between the prediction and gpsx_wacq), each with its _dev twin, and the three
// host helpers behind them (gpsx_weph_to_eph, gpsx_walm_to_eph and gpsx_walm_gps_minus_utc are gpsx_ephemeris.cpp's, beside the decoder they restate).  Host code only, like gpsx_api.hip; it reads no lab knob, so lib/libgpsx_lab.so links this object as it is.
//
// A pair is ONE function with a `bool host`.  host: the capture and the results are host memory, staged through the arena; the call
// waits for its kernel and reports a bad channel itself (flag 0).  Otherwise (_dev) they are device memory, the call returns after
// the launch and the next gpsx_synchronize reports (flag 1).  The refusals come first; the first clause that fails decides the text.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <initializer_list>

#include "gpsx_ctx.hpp"

using namespace gpsx;
using namespace gpsx_host;

namespace {

// ---- the clauses the refusals share, the overflow-checked count x n_ch x sizeof -------------------------------------------------------
int check_weights_spacing(gpsx_ctx *ctx, int weights, int spacing)
{
  if (weights != GPSX_WEIGHTS_SIGN_ONLY && weights != GPSX_WEIGHTS_SIGN_MAGNITUDE)
    return fail(ctx, GPSX_EINVAL, "unknown weights");
  return spacing < 1 || spacing > 15 ? fail(ctx, GPSX_EINVAL, "spacing must be 1..15 samples") : GPSX_OK;
}
int check_n_blocks(gpsx_ctx *ctx, int n) { return n < 1 || n > 4096 ? fail(ctx, GPSX_EINVAL, "n_blocks must be 1..4096") : GPSX_OK; }
int check_n_slots(gpsx_ctx *ctx, int n, int n_blocks) { return n < 1 || n > n_blocks ? fail(ctx, GPSX_EINVAL, "n_slots must be 1..n_blocks") : GPSX_OK; }
int check_n_ch(gpsx_ctx *ctx, int n) { return n < 1 ? fail(ctx, GPSX_EINVAL, "n_ch must be at least 1") : GPSX_OK; }
int check_gains(gpsx_ctx *ctx, std::initializer_list<float> gains)
{
  for (float g : gains)
    if (!(__builtin_fabsf(g) <= 3.402823466e+38f))
      return fail(ctx, GPSX_EINVAL, "a loop gain is not finite");
  return GPSX_OK;
}
// the aided calls' own clauses (aided: the call has an `aid` argument at all)
int check_aid(gpsx_ctx *ctx, const gpsx_waid_t *aid)
{
  if (!(__builtin_fabsf(aid->code_per_hz) <= 1.0f))   // (a NaN fails it)
    return fail(ctx, GPSX_EINVAL, "code_per_hz must be finite and -1..1");
  return aid->reserved != 0 ? fail(ctx, GPSX_EINVAL, "reserved must be 0") : GPSX_OK;
}
bool records_overflow(size_t count, int n_ch, size_t each, size_t *bytes)
{
  size_t recs = 0;   // (true: the product overflows a size)
  return __builtin_mul_overflow(count, (size_t)n_ch, &recs) || __builtin_mul_overflow(recs, each, bytes);
}

// ---- the launch and what follows it -----------------------------------------------------------------------------------------------
// `launch(flag)` starts the kernel with the flag it raises for a bad channel; `copy_back()` (host calls only) enqueues the copies of
// the results.  `bad_state`: what a host call says when the flag was raised; nullptr: the tracking calls' PRN verdict.
template <typename Launch, typename CopyBack>
int launch_and_report(gpsx_ctx *ctx, bool host, const char *kernel, const char *bad_state, Launch launch, CopyBack copy_back)
{
  if (host)
    ctx->h_bad_prn[0] = 0;   // (flag 0 is the waiting calls' own: each reads it before it returns, so nothing can be pending in it)
  launch(ctx->d_bad_prn + (host ? 0 : 1));
  LAUNCHCHK(ctx, kernel);
  ctx->last_kernel = kernel;
  if (!host)
    return GPSX_OK;
  if (int rc = copy_back()) return rc;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (!bad_state)
    return track_prn_verdict(ctx);
  if (*ctx->h_bad_prn == 0)
    return GPSX_OK;
  *ctx->h_bad_prn = 0;
  return fail(ctx, GPSX_EINVAL, bad_state);
}

// ---- E/P/L on weighted two-bit samples, K blocks per launch -------------------------------------------------------------------------
int track_epl_weighted(gpsx_ctx *ctx, const gpsx_trk_weighted_t *cfg, const void *if_blocks_2bit, int n_blocks, gpsx_trk_state_t *st,
                       int n_ch, int32_t *iq_out, bool host)
{
  if (int rc = use_device(ctx)) return rc;
  if (!cfg || !if_blocks_2bit || !st || !iq_out)
    return fail(ctx, GPSX_EINVAL, "null argument");
  if (int rc = check_weights_spacing(ctx, cfg->weights, cfg->spacing)) return rc;
  if (int rc = check_n_blocks(ctx, n_blocks)) return rc;
  if (int rc = check_n_ch(ctx, n_ch)) return rc;
  size_t iq_bytes = 0;
  if (records_overflow((size_t)n_blocks, n_ch, 6 * sizeof(int32_t), &iq_bytes))
    return fail(ctx, GPSX_EINVAL, "n_blocks x n_ch records overflow a size");
  const size_t if_bytes = (size_t)n_blocks * GPSX_BYTES_PER_MS_2BIT, st_bytes = (size_t)n_ch * sizeof(gpsx_trk_state_t);
  const uint8_t *d_blocks = static_cast<const uint8_t *>(if_blocks_2bit);
  gpsx_trk_state_t *d_st = st;
  int32_t *d_iq = iq_out;
  if (host) {
    if (int rc = arena_reset(ctx, arena_size(if_bytes + 2) + arena_size(st_bytes) + arena_size(iq_bytes))) return rc;
    uint8_t *d_if = arena_take<uint8_t>(ctx, if_bytes + 2);
    d_st = arena_take<gpsx_trk_state_t>(ctx, n_ch);
    d_iq = arena_take<int32_t>(ctx, iq_bytes / sizeof(int32_t));
    HIPCHK(ctx, hipMemcpyAsync(d_if, if_blocks_2bit, if_bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_st, st, st_bytes, hipMemcpyHostToDevice, ctx->stream));
    d_blocks = d_if;
  }
  return launch_and_report(
      ctx, host, "k_track_epl_weighted", nullptr,
      [&](uint32_t *flag) { launch_track_epl_weighted(ctx->stream, d_blocks, n_blocks, ctx->if_hz, cfg->weights == GPSX_WEIGHTS_SIGN_MAGNITUDE,
                                                      cfg->spacing, d_st, n_ch, ctx->d_trk_rep, d_iq, flag); },
      [&]() -> int {
        HIPCHK(ctx, hipMemcpyAsync(st, d_st, st_bytes, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(iq_out, d_iq, iq_bytes, hipMemcpyDeviceToHost, ctx->stream));
        return GPSX_OK;
      });
}

// ---- the closed loops: DLL / PLL / FLL, K blocks per launch; the second with a bit synchroniser and bit-aligned windows -------------
// what a host call of either stages: the capture into the arena, room for the records.  The state is device memory in both variants.
// n_rx > 1 (the _multi call): n_rx streams of n_blocks blocks, rx_stride_blocks apart in host memory, packed n_blocks apart in the
// arena -- only the blocks themselves are read.
template <typename Rec>
int stage_loop_call(gpsx_ctx *ctx, const uint8_t *if_blocks_2bit, int n_blocks, size_t rec_bytes, const uint8_t **d_blocks, Rec **d_rec,
                    int n_rx = 1, int rx_stride_blocks = 0)
{
  const size_t rx_bytes = (size_t)n_blocks * GPSX_BYTES_PER_MS_2BIT, if_bytes = (size_t)n_rx * rx_bytes;
  if (int rc = arena_reset(ctx, arena_size(if_bytes + 2) + arena_size(rec_bytes))) return rc;
  uint8_t *d_if = arena_take<uint8_t>(ctx, if_bytes + 2);
  *d_rec = arena_take<Rec>(ctx, rec_bytes / sizeof(Rec));
  if (n_rx == 1 || rx_stride_blocks == n_blocks)
    HIPCHK(ctx, hipMemcpyAsync(d_if, if_blocks_2bit, if_bytes, hipMemcpyHostToDevice, ctx->stream));
  else
    HIPCHK(ctx, hipMemcpy2DAsync(d_if, rx_bytes, if_blocks_2bit, (size_t)rx_stride_blocks * GPSX_BYTES_PER_MS_2BIT, rx_bytes, (size_t)n_rx,
                                 hipMemcpyHostToDevice, ctx->stream));
  *d_blocks = d_if;
  return GPSX_OK;
}

// `aided`: the _aided pair (k_track_waid_loop with aid's factor); otherwise aid is not looked at
int track_loop_weighted(gpsx_ctx *ctx, const gpsx_wloop_cfg_t *cfg, bool aided, const gpsx_waid_t *aid, const void *if_blocks_2bit, int n_blocks,
                        gpsx_wloop_state_t *d_state, int n_ch, gpsx_wloop_rec_t *rec, bool host)
{
  if (int rc = use_device(ctx)) return rc;
  if (!cfg || (aided && !aid) || !if_blocks_2bit || !d_state || !rec)
    return fail(ctx, GPSX_EINVAL, "null argument");
  if (int rc = check_weights_spacing(ctx, cfg->weights, cfg->spacing)) return rc;
  if (cfg->n_coh < 1 || cfg->n_coh > 20)
    return fail(ctx, GPSX_EINVAL, "n_coh must be 1..20 blocks");
  if (int rc = check_n_blocks(ctx, n_blocks)) return rc;
  if (n_blocks % cfg->n_coh != 0)
    return fail(ctx, GPSX_EINVAL, "n_blocks must be a multiple of n_coh");
  if (int rc = check_n_ch(ctx, n_ch)) return rc;
  if (int rc = check_gains(ctx, {cfg->dll_c1, cfg->dll_c2, cfg->pll_c1, cfg->pll_c2, cfg->fll_c})) return rc;
  if (aided)
    if (int rc = check_aid(ctx, aid)) return rc;
  size_t rec_bytes = 0;
  if (records_overflow((size_t)(n_blocks / cfg->n_coh), n_ch, sizeof(gpsx_wloop_rec_t), &rec_bytes))
    return fail(ctx, GPSX_EINVAL, "windows x n_ch records overflow a size");
  const uint8_t *d_if = static_cast<const uint8_t *>(if_blocks_2bit);
  gpsx_wloop_rec_t *d_rec = rec;
  if (host)
    if (int rc = stage_loop_call(ctx, d_if, n_blocks, rec_bytes, &d_if, &d_rec)) return rc;
  return launch_and_report(
      ctx, host, aided ? "k_track_waid_loop" : "k_track_wloop", nullptr,
      [&](uint32_t *flag) {
        if (aided)
          launch_track_loop_weighted_aided(ctx->stream, d_if, n_blocks, ctx->if_hz, *cfg, aid->code_per_hz, d_state, n_ch, ctx->d_trk_rep, d_rec, flag);
        else
          launch_track_loop_weighted(ctx->stream, d_if, n_blocks, ctx->if_hz, *cfg, d_state, n_ch, ctx->d_trk_rep, d_rec, flag);
      },
      [&]() -> int { HIPCHK(ctx, hipMemcpyAsync(rec, d_rec, rec_bytes, hipMemcpyDeviceToHost, ctx->stream)); return GPSX_OK; });
}

// the sync loop's clauses on cfg and n_blocks, in the order both of its callers report them (between "null argument" and the channel counts)
int check_wsync_cfg(gpsx_ctx *ctx, const gpsx_wsync_cfg_t *cfg, int n_blocks)
{
  if (int rc = check_weights_spacing(ctx, cfg->weights, cfg->spacing)) return rc;
  for (int n : {cfg->n_coh_search, cfg->n_coh_lock})
    if (n < 1 || n > 20 || 20 % n != 0)
      return fail(ctx, GPSX_EINVAL, "n_coh_search and n_coh_lock must be 1, 2, 4, 5, 10 or 20 blocks");
  if (cfg->sync_bits < 1 || cfg->sync_bits > 200)
    return fail(ctx, GPSX_EINVAL, "sync_bits must be 1..200");
  if (cfg->sync_num < 1 || cfg->sync_num > 1024 || cfg->sync_den < 1 || cfg->sync_den > 1024)
    return fail(ctx, GPSX_EINVAL, "sync_num and sync_den must be 1..1024");
  if (cfg->sync_num < cfg->sync_den)
    return fail(ctx, GPSX_EINVAL, "sync_num must not be below sync_den");
  return check_n_blocks(ctx, n_blocks);
}
// ... and behind the channel counts: the gains, the aiding factor
int check_wsync_gains(gpsx_ctx *ctx, const gpsx_wsync_cfg_t *cfg, const gpsx_waid_t *aid)
{
  for (const gpsx_wsync_gains_t *g : {&cfg->search, &cfg->lock})
    if (int rc = check_gains(ctx, {g->dll_c1, g->dll_c2, g->pll_c1, g->pll_c2, g->fll_c})) return rc;
  return aid ? check_aid(ctx, aid) : GPSX_OK;
}

int track_loop_weighted_sync(gpsx_ctx *ctx, const gpsx_wsync_cfg_t *cfg, bool aided, const gpsx_waid_t *aid, const void *if_blocks_2bit,
                             int n_blocks, gpsx_wsync_state_t *d_state, int n_ch, gpsx_wsync_rec_t *rec, bool host)
{
  if (int rc = use_device(ctx)) return rc;
  if (!cfg || (aided && !aid) || !if_blocks_2bit || !d_state || !rec)
    return fail(ctx, GPSX_EINVAL, "null argument");
  if (int rc = check_wsync_cfg(ctx, cfg, n_blocks)) return rc;
  if (int rc = check_n_ch(ctx, n_ch)) return rc;
  if (int rc = check_wsync_gains(ctx, cfg, aided ? aid : nullptr)) return rc;
  const int span = cfg->n_coh_search < cfg->n_coh_lock ? cfg->n_coh_search : cfg->n_coh_lock;
  size_t rec_bytes = 0;
  if (records_overflow((size_t)((n_blocks + span - 1) / span), n_ch, sizeof(gpsx_wsync_rec_t), &rec_bytes))
    return fail(ctx, GPSX_EINVAL, "slots x n_ch records overflow a size");
  const uint8_t *d_if = static_cast<const uint8_t *>(if_blocks_2bit);
  gpsx_wsync_rec_t *d_rec = rec;
  if (host)
    if (int rc = stage_loop_call(ctx, d_if, n_blocks, rec_bytes, &d_if, &d_rec)) return rc;
  return launch_and_report(
      ctx, host, aided ? "k_track_waid_sync" : "k_track_wsync", nullptr,
      [&](uint32_t *flag) {
        if (aided)
          launch_track_loop_weighted_sync_aided(ctx->stream, d_if, n_blocks, ctx->if_hz, *cfg, aid->code_per_hz, d_state, n_ch, ctx->d_trk_rep, d_rec, flag);
        else
          launch_track_loop_weighted_sync(ctx->stream, d_if, n_blocks, ctx->if_hz, *cfg, d_state, n_ch, ctx->d_trk_rep, d_rec, flag);
      },
      [&]() -> int { HIPCHK(ctx, hipMemcpyAsync(rec, d_rec, rec_bytes, hipMemcpyDeviceToHost, ctx->stream)); return GPSX_OK; });
}

// n_rx receivers, one stream each, in one launch (k_track_wsync_multi).  aid NULL: unaided -- the one kernel with a factor of 0, which
// by the aided call's definition gives the unaided bytes.  The single-stream call's clauses in its order, rx's in the place of n_ch's.
int track_loop_weighted_sync_multi(gpsx_ctx *ctx, const gpsx_wsync_cfg_t *cfg, const gpsx_waid_t *aid, const gpsx_wmulti_t *rx,
                                   const void *if_blocks_2bit, int n_blocks, gpsx_wsync_state_t *d_state, gpsx_wsync_rec_t *rec, bool host)
{
  if (int rc = use_device(ctx)) return rc;
  if (!cfg || !rx || !if_blocks_2bit || !d_state || !rec)
    return fail(ctx, GPSX_EINVAL, "null argument");
  if (int rc = check_wsync_cfg(ctx, cfg, n_blocks)) return rc;
  if (rx->n_rx < 1 || rx->n_rx > (1 << 20))
    return fail(ctx, GPSX_EINVAL, "n_rx must be 1..1048576");
  if (rx->ch_per_rx < 1 || rx->ch_per_rx > 64)
    return fail(ctx, GPSX_EINVAL, "ch_per_rx must be 1..64");
  if (rx->rx_stride_blocks < n_blocks)
    return fail(ctx, GPSX_EINVAL, "rx_stride_blocks must not be below n_blocks");
  if (rx->reserved != 0)
    return fail(ctx, GPSX_EINVAL, "reserved must be 0");
  int n_ch = 0;
  if (__builtin_mul_overflow(rx->n_rx, rx->ch_per_rx, &n_ch))
    return fail(ctx, GPSX_EINVAL, "n_rx x ch_per_rx must not exceed INT32_MAX");
  if (int rc = check_wsync_gains(ctx, cfg, aid)) return rc;
  const int span = cfg->n_coh_search < cfg->n_coh_lock ? cfg->n_coh_search : cfg->n_coh_lock;
  size_t rec_bytes = 0, bytes = 0;
  if (records_overflow((size_t)((n_blocks + span - 1) / span), n_ch, sizeof(gpsx_wsync_rec_t), &rec_bytes) ||
      records_overflow(1, n_ch, sizeof(gpsx_wsync_state_t), &bytes) ||
      records_overflow((size_t)rx->rx_stride_blocks, rx->n_rx, GPSX_BYTES_PER_MS_2BIT, &bytes))
    return fail(ctx, GPSX_EINVAL, "slots x n_ch records, states or streams overflow a size");
  const uint8_t *d_if = static_cast<const uint8_t *>(if_blocks_2bit);
  gpsx_wsync_rec_t *d_rec = rec;
  int stride = rx->rx_stride_blocks;
  if (host) {
    if (int rc = stage_loop_call(ctx, d_if, n_blocks, rec_bytes, &d_if, &d_rec, rx->n_rx, stride)) return rc;
    stride = n_blocks;   // (packed in the arena)
  }
  return launch_and_report(
      ctx, host, "k_track_wsync_multi", nullptr,
      [&](uint32_t *flag) {
        launch_track_loop_weighted_sync_multi(ctx->stream, d_if, n_blocks, ctx->if_hz, *cfg, aid ? aid->code_per_hz : 0.0f, rx->n_rx, rx->ch_per_rx,
                                              stride, d_state, ctx->d_trk_rep, d_rec, flag);
      },
      [&]() -> int { HIPCHK(ctx, hipMemcpyAsync(rec, d_rec, rec_bytes, hipMemcpyDeviceToHost, ctx->stream)); return GPSX_OK; });
}

// ---- LNAV frame sync and parity-checked words from the sync loop's bit records; the observables behind both -------------------------
// (d_rec, d_words as input and the states are device memory in both variants; only the results are staged)
int wnav_words(gpsx_ctx *ctx, const gpsx_wnav_cfg_t *cfg, const gpsx_wsync_rec_t *d_rec, int n_slots, int n_blocks,
               gpsx_wnav_state_t *d_state, int n_ch, gpsx_wnav_word_t *words, bool host)
{
  if (int rc = use_device(ctx)) return rc;
  if (!cfg || !d_rec || !d_state || !words)
    return fail(ctx, GPSX_EINVAL, "null argument");
  if (cfg->max_bad_words < 1 || cfg->max_bad_words > 10)
    return fail(ctx, GPSX_EINVAL, "max_bad_words must be 1..10");
  if (cfg->reserved != 0)
    return fail(ctx, GPSX_EINVAL, "reserved must be 0");
  if (int rc = check_n_blocks(ctx, n_blocks)) return rc;
  if (int rc = check_n_slots(ctx, n_slots, n_blocks)) return rc;
  if (int rc = check_n_ch(ctx, n_ch)) return rc;
  size_t rec_bytes = 0, words_bytes = 0;
  if (records_overflow((size_t)n_slots, n_ch, sizeof(gpsx_wsync_rec_t), &rec_bytes) ||
      records_overflow((size_t)(n_blocks / 600 + 2), n_ch, sizeof(gpsx_wnav_word_t), &words_bytes))
    return fail(ctx, GPSX_EINVAL, "slots x n_ch records overflow a size");
  gpsx_wnav_word_t *d_words = words;
  if (host) {
    if (int rc = arena_reset(ctx, arena_size(words_bytes))) return rc;
    d_words = arena_take<gpsx_wnav_word_t>(ctx, words_bytes / sizeof(gpsx_wnav_word_t));
  }
  return launch_and_report(
      ctx, host, "k_wnav_words", "a channel's frame state is out of range (its state is untouched, its slots are empty)",
      [&](uint32_t *flag) { launch_wnav_words(ctx->stream, d_rec, n_slots, n_blocks, cfg->max_bad_words, d_state, n_ch, d_words, flag); },
      [&]() -> int { HIPCHK(ctx, hipMemcpyAsync(words, d_words, words_bytes, hipMemcpyDeviceToHost, ctx->stream)); return GPSX_OK; });
}

int wobs(gpsx_ctx *ctx, const gpsx_wobs_cfg_t *cfg, const gpsx_wsync_rec_t *d_rec, int n_slots, int n_blocks, const gpsx_wnav_word_t *d_words,
         gpsx_wobs_state_t *d_state, int n_ch, gpsx_wobs_t *obs, bool host)
{
  if (int rc = use_device(ctx)) return rc;
  if (!cfg || !d_rec || !d_words || !d_state || !obs)
    return fail(ctx, GPSX_EINVAL, "null argument");
  if (!(cfg->edge_guard >= 0.0f && cfg->edge_guard <= 8184.0f))   // (a NaN fails both)
    return fail(ctx, GPSX_EINVAL, "edge_guard must be finite and 0..8184");
  if (cfg->reserved != 0)
    return fail(ctx, GPSX_EINVAL, "reserved must be 0");
  if (int rc = check_n_blocks(ctx, n_blocks)) return rc;
  if (int rc = check_n_slots(ctx, n_slots, n_blocks)) return rc;
  if (int rc = check_n_ch(ctx, n_ch)) return rc;
  size_t bytes = 0, obs_bytes = 0;
  if (records_overflow((size_t)n_slots, n_ch, sizeof(gpsx_wsync_rec_t), &bytes) ||
      records_overflow((size_t)(n_blocks / 600 + 2), n_ch, sizeof(gpsx_wnav_word_t), &bytes) ||
      records_overflow(1, n_ch, sizeof(gpsx_wobs_state_t), &bytes) || records_overflow(1, n_ch, sizeof(gpsx_wobs_t), &obs_bytes))
    return fail(ctx, GPSX_EINVAL, "slots x n_ch records overflow a size");
  gpsx_wobs_t *d_obs = obs;
  if (host) {
    if (int rc = arena_reset(ctx, arena_size(obs_bytes))) return rc;
    d_obs = arena_take<gpsx_wobs_t>(ctx, (size_t)n_ch);
  }
  return launch_and_report(
      ctx, host, "k_wobs", "a channel's observable state is out of range (its state is untouched, its observable is zero)",
      [&](uint32_t *flag) { launch_wobs(ctx->stream, d_rec, n_slots, n_blocks, cfg->edge_guard, d_words, d_state, n_ch, d_obs, flag); },
      [&]() -> int { HIPCHK(ctx, hipMemcpyAsync(obs, d_obs, obs_bytes, hipMemcpyDeviceToHost, ctx->stream)); return GPSX_OK; });
}

// ---- the broadcast ephemerides from the words (d_words and the states are device memory in both variants) -----------------------------
int weph(gpsx_ctx *ctx, const gpsx_weph_cfg_t *cfg, const gpsx_wnav_word_t *d_words, int n_blocks, gpsx_weph_state_t *d_state, int n_ch,
         gpsx_weph_t *eph, bool host)
{
  if (int rc = use_device(ctx)) return rc;
  if (!cfg || !d_words || !d_state || !eph)
    return fail(ctx, GPSX_EINVAL, "null argument");
  if (cfg->reserved0 != 0 || cfg->reserved1 != 0)
    return fail(ctx, GPSX_EINVAL, "reserved must be 0");
  if (int rc = check_n_blocks(ctx, n_blocks)) return rc;
  if (int rc = check_n_ch(ctx, n_ch)) return rc;
  if (!host && (reinterpret_cast<uintptr_t>(eph) & 15u) != 0)   // (k_weph stores the records 16 bytes at a time)
    return fail(ctx, GPSX_EINVAL, "d_eph must be 16-byte aligned");
  size_t bytes = 0, eph_bytes = 0;
  if (records_overflow((size_t)(n_blocks / 600 + 2), n_ch, sizeof(gpsx_wnav_word_t), &bytes) ||
      records_overflow(1, n_ch, sizeof(gpsx_weph_state_t), &bytes) || records_overflow(1, n_ch, sizeof(gpsx_weph_t), &eph_bytes))
    return fail(ctx, GPSX_EINVAL, "slots x n_ch records overflow a size");
  gpsx_weph_t *d_eph = eph;
  if (host) {
    if (int rc = arena_reset(ctx, arena_size(eph_bytes))) return rc;
    d_eph = arena_take<gpsx_weph_t>(ctx, (size_t)n_ch);
  }
  return launch_and_report(
      ctx, host, "k_weph", "a channel's ephemeris state is out of range (its state is untouched, its record is zero)",
      [&](uint32_t *flag) { launch_weph(ctx->stream, d_words, n_blocks, d_state, n_ch, d_eph, flag); },
      [&]() -> int { HIPCHK(ctx, hipMemcpyAsync(eph, d_eph, eph_bytes, hipMemcpyDeviceToHost, ctx->stream)); return GPSX_OK; });
}

// ---- almanac, ionosphere and UTC from the same words (host: rx and alm are host memory, staged through the arena; the words, the slot
//      states and the banks are device memory in both variants) --------------------------------------------------------------------------
int walm(gpsx_ctx *ctx, const gpsx_walm_cfg_t *cfg, const gpsx_wnav_word_t *d_words, int n_blocks, int n_rx, gpsx_walm_slot_t *d_slot_state,
         gpsx_walm_bank_t *d_bank, gpsx_walm_rx_t *rx, gpsx_walm_sv_t *alm, bool host)
{
  if (int rc = use_device(ctx)) return rc;
  if (!cfg || !d_words || !d_slot_state || !d_bank || !rx)
    return fail(ctx, GPSX_EINVAL, "null argument");
  if (cfg->ch_per_rx < 1 || cfg->ch_per_rx > 64)
    return fail(ctx, GPSX_EINVAL, "ch_per_rx must be 1..64");
  if (cfg->reserved[0] != 0 || cfg->reserved[1] != 0 || cfg->reserved[2] != 0)
    return fail(ctx, GPSX_EINVAL, "reserved must be 0");
  if (int rc = check_n_blocks(ctx, n_blocks)) return rc;
  if (n_rx < 1 || n_rx > (1 << 20))
    return fail(ctx, GPSX_EINVAL, "n_rx must be 1..1048576");
  if (((reinterpret_cast<uintptr_t>(d_words) | reinterpret_cast<uintptr_t>(d_slot_state) | reinterpret_cast<uintptr_t>(d_bank)) & 15u) != 0)
    return fail(ctx, GPSX_EINVAL, "d_words, d_slot_state and d_bank must be 16-byte aligned");
  if (!host && ((reinterpret_cast<uintptr_t>(rx) | reinterpret_cast<uintptr_t>(alm)) & 15u) != 0)
    return fail(ctx, GPSX_EINVAL, "d_rx and d_alm must be 16-byte aligned");
  size_t words_bytes = 0, slot_bytes = 0, bank_bytes = 0, rx_bytes = 0, alm_bytes = 0;
  if (records_overflow((size_t)n_rx * (size_t)(n_blocks / 600 + 2), cfg->ch_per_rx, sizeof(gpsx_wnav_word_t), &words_bytes) ||
      records_overflow((size_t)n_rx, cfg->ch_per_rx, sizeof(gpsx_walm_slot_t), &slot_bytes) ||
      records_overflow((size_t)n_rx, 1, sizeof(gpsx_walm_bank_t), &bank_bytes) || records_overflow((size_t)n_rx, 1, sizeof(gpsx_walm_rx_t), &rx_bytes) ||
      records_overflow((size_t)n_rx, 32, sizeof(gpsx_walm_sv_t), &alm_bytes))
    return fail(ctx, GPSX_EINVAL, "n_rx x ch_per_rx records overflow a size");
  // (host and device addresses share one space here: one list of pairs serves both variants)
  const struct { const void *p; size_t n; } span[5] = {{d_words, words_bytes}, {d_slot_state, slot_bytes}, {d_bank, bank_bytes}, {rx, rx_bytes}, {alm, alm_bytes}};
  for (int a = 0; a < 5; a++)
    for (int b = a + 1; b < 5; b++) {
      const uintptr_t pa = reinterpret_cast<uintptr_t>(span[a].p), pb = reinterpret_cast<uintptr_t>(span[b].p);
      if (pa && pb && pa < pb + span[b].n && pb < pa + span[a].n)
        return fail(ctx, GPSX_EINVAL, "two arrays overlap");
    }
  gpsx_walm_rx_t *d_rx = rx;
  gpsx_walm_sv_t *d_alm = alm;
  if (host) {
    if (int rc = arena_reset(ctx, arena_size(rx_bytes) + (alm ? arena_size(alm_bytes) : 0))) return rc;
    d_rx = arena_take<gpsx_walm_rx_t>(ctx, (size_t)n_rx);
    if (alm)
      d_alm = arena_take<gpsx_walm_sv_t>(ctx, (size_t)n_rx * 32u);
  }
  return launch_and_report(
      ctx, host, "k_walm", "a slot's almanac state or a receiver's almanac bank is out of range (it is untouched, a bad bank's records are zero)",
      [&](uint32_t *flag) { launch_walm(ctx->stream, *cfg, d_words, n_blocks, n_rx, d_slot_state, d_bank, d_rx, d_alm, flag); },
      [&]() -> int {
        HIPCHK(ctx, hipMemcpyAsync(rx, d_rx, rx_bytes, hipMemcpyDeviceToHost, ctx->stream));
        if (alm)
          HIPCHK(ctx, hipMemcpyAsync(alm, d_alm, alm_bytes, hipMemcpyDeviceToHost, ctx->stream));
        return GPSX_OK;
      });
}

// ---- the lock monitor on the sync loop's records (d_rec and all states are device memory in both variants) ----------------------------
int wlock(gpsx_ctx *ctx, const gpsx_wlock_cfg_t *cfg, const gpsx_wsync_rec_t *d_rec, int n_slots, int n_blocks, gpsx_wlock_state_t *d_state,
          gpsx_wsync_state_t *d_sync_state, int n_ch, gpsx_wlock_t *lock, bool host)
{
  if (int rc = use_device(ctx)) return rc;
  if (!cfg || !d_rec || !d_state || !lock)
    return fail(ctx, GPSX_EINVAL, "null argument");
  if (cfg->epoch_search < 1 || cfg->epoch_search > 1024 || cfg->epoch_lock < 1 || cfg->epoch_lock > 1024)
    return fail(ctx, GPSX_EINVAL, "epoch_search and epoch_lock must be 1..1024 windows");
  if (cfg->n_good < 1 || cfg->n_good > 255 || cfg->n_bad < 1 || cfg->n_bad > 255)
    return fail(ctx, GPSX_EINVAL, "n_good and n_bad must be 1..255");
  for (float t : {cfg->code_min, cfg->car_min, cfg->snr_min})
    if (!(__builtin_fabsf(t) <= 3.402823466e+38f))
      return fail(ctx, GPSX_EINVAL, "a threshold is not finite");
  if (cfg->rearm < 0 || cfg->rearm > 3)
    return fail(ctx, GPSX_EINVAL, "rearm must be 0..3");
  if (cfg->patience < 0)
    return fail(ctx, GPSX_EINVAL, "patience must not be negative");
  if (cfg->reserved != 0)
    return fail(ctx, GPSX_EINVAL, "reserved must be 0");
  if (cfg->rearm != 0 && !d_sync_state)
    return fail(ctx, GPSX_EINVAL, "rearm needs d_sync_state");
  if (int rc = check_n_blocks(ctx, n_blocks)) return rc;
  if (int rc = check_n_slots(ctx, n_slots, n_blocks)) return rc;
  if (int rc = check_n_ch(ctx, n_ch)) return rc;
  size_t bytes = 0, lock_bytes = 0;
  if (records_overflow((size_t)n_slots, n_ch, sizeof(gpsx_wsync_rec_t), &bytes) || records_overflow(1, n_ch, sizeof(gpsx_wsync_state_t), &bytes) ||
      records_overflow(1, n_ch, sizeof(gpsx_wlock_state_t), &bytes) || records_overflow(1, n_ch, sizeof(gpsx_wlock_t), &lock_bytes))
    return fail(ctx, GPSX_EINVAL, "slots x n_ch records overflow a size");
  gpsx_wlock_t *d_lock = lock;
  if (host) {
    if (int rc = arena_reset(ctx, arena_size(lock_bytes))) return rc;
    d_lock = arena_take<gpsx_wlock_t>(ctx, (size_t)n_ch);
  }
  return launch_and_report(
      ctx, host, "k_wlock", "a channel's lock state is out of range (its state is untouched, its record is zero)",
      [&](uint32_t *flag) { launch_wlock(ctx->stream, d_rec, n_slots, n_blocks, *cfg, d_state, cfg->rearm != 0 ? d_sync_state : nullptr, n_ch, d_lock, flag); },
      [&]() -> int { HIPCHK(ctx, hipMemcpyAsync(lock, d_lock, lock_bytes, hipMemcpyDeviceToHost, ctx->stream)); return GPSX_OK; });
}

// ---- the solvers at the chain's end (host: every array is host memory, staged through the arena; _dev: all device memory) ------------
// a host call's input array of n records, which may be absent: room in the arena, the copy enqueued, *d the staged copy (src ==
// nullptr: nothing is taken, *d stays null).  The takes follow the order of the calls, as arena_reset's sum does.
template <typename T>
int stage_in(gpsx_ctx *ctx, const T *src, size_t n, const T **d)
{
  if (!src)
    return GPSX_OK;
  T *staged = arena_take<T>(ctx, n);
  HIPCHK(ctx, hipMemcpyAsync(staged, src, n * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
  *d = staged;
  return GPSX_OK;
}

// ---- the position fixes ---------------------------------------------------------------------------------------------------------------
int wfix(gpsx_ctx *ctx, const gpsx_wfix_cfg_t *cfg, const gpsx_wobs_t *obs, const gpsx_weph_t *eph, const gpsx_wlock_t *lock, const gpsx_wfix_t *prev,
         int n_rx, gpsx_wfix_t *fix, double *pr_m, bool host)
{
  if (int rc = use_device(ctx)) return rc;
  if (!cfg || !obs || !eph || !fix)
    return fail(ctx, GPSX_EINVAL, "null argument");
  if (!(cfg->offset_ms - cfg->offset_ms == 0.0))   // (not finite: the difference is a NaN)
    return fail(ctx, GPSX_EINVAL, "offset_ms is not finite");
  for (double v : cfg->ion)
    if (!(v - v == 0.0))
      return fail(ctx, GPSX_EINVAL, "an ionosphere coefficient is not finite");
  if (cfg->ch_per_rx < 1 || cfg->ch_per_rx > 64)
    return fail(ctx, GPSX_EINVAL, "ch_per_rx must be 1..64");
  if (cfg->min_sats < 4 || cfg->min_sats > 64)
    return fail(ctx, GPSX_EINVAL, "min_sats must be 4..64");
  if (cfg->reserved0 != 0 || cfg->reserved1 != 0 || cfg->reserved2 != 0 || cfg->reserved3 != 0)
    return fail(ctx, GPSX_EINVAL, "reserved must be 0");
  if (n_rx < 1 || n_rx > (1 << 20))
    return fail(ctx, GPSX_EINVAL, "n_rx must be 1..1048576");
  if (!host && (reinterpret_cast<uintptr_t>(fix) & 15u) != 0)
    return fail(ctx, GPSX_EINVAL, "d_fix must be 16-byte aligned");
  size_t obs_bytes = 0, eph_bytes = 0, lock_bytes = 0, fix_bytes = 0, pr_bytes = 0;
  if (records_overflow((size_t)n_rx, cfg->ch_per_rx, sizeof(gpsx_wobs_t), &obs_bytes) ||
      records_overflow((size_t)n_rx, cfg->ch_per_rx, sizeof(gpsx_weph_t), &eph_bytes) ||
      records_overflow((size_t)n_rx, cfg->ch_per_rx, sizeof(gpsx_wlock_t), &lock_bytes) ||
      records_overflow((size_t)n_rx, cfg->ch_per_rx, sizeof(double), &pr_bytes) || records_overflow((size_t)n_rx, 1, sizeof(gpsx_wfix_t), &fix_bytes))
    return fail(ctx, GPSX_EINVAL, "n_rx x ch_per_rx records overflow a size");
  const size_t n_ch = (size_t)n_rx * (size_t)cfg->ch_per_rx;
  const gpsx_wobs_t *d_obs = obs;
  const gpsx_weph_t *d_eph = eph;
  const gpsx_wlock_t *d_lock = lock;
  const gpsx_wfix_t *d_prev = prev;
  gpsx_wfix_t *d_fix = fix;
  double *d_pr = pr_m;
  if (host) {
    if (int rc = arena_reset(ctx, arena_size(obs_bytes) + arena_size(eph_bytes) + (lock ? arena_size(lock_bytes) : 0) +
                                      (prev ? arena_size(fix_bytes) : 0) + arena_size(fix_bytes) + (pr_m ? arena_size(pr_bytes) : 0)))
      return rc;
    if (int rc = stage_in(ctx, obs, n_ch, &d_obs)) return rc;
    if (int rc = stage_in(ctx, eph, n_ch, &d_eph)) return rc;
    if (int rc = stage_in(ctx, lock, n_ch, &d_lock)) return rc;
    if (int rc = stage_in(ctx, prev, (size_t)n_rx, &d_prev)) return rc;
    d_fix = arena_take<gpsx_wfix_t>(ctx, (size_t)n_rx);
    if (pr_m)
      d_pr = arena_take<double>(ctx, n_ch);
  }
  return launch_and_report(
      ctx, host, "k_wfix", "k_wfix raised the bad-state flag, which it never does",
      [&](uint32_t *) { launch_wfix(ctx->stream, *cfg, d_obs, d_eph, d_lock, d_prev, n_rx, d_fix, d_pr); },
      [&]() -> int {
        HIPCHK(ctx, hipMemcpyAsync(fix, d_fix, fix_bytes, hipMemcpyDeviceToHost, ctx->stream));
        if (pr_m)
          HIPCHK(ctx, hipMemcpyAsync(pr_m, d_pr, pr_bytes, hipMemcpyDeviceToHost, ctx->stream));
        return GPSX_OK;
      });
}

// ---- the position fixes with millisecond repair and fault exclusion (staged as wfix stages its arrays) --------------------------------
int wfde(gpsx_ctx *ctx, const gpsx_wfde_cfg_t *fc, const gpsx_wobs_t *obs, const gpsx_weph_t *eph, const gpsx_wlock_t *lock, const gpsx_wfix_t *prev,
         int n_rx, gpsx_wfix_t *fix, gpsx_wfde_t *fde, double *pr_m, bool host)
{
  if (int rc = use_device(ctx)) return rc;
  if (!fc || !obs || !eph || !fix || !fde)
    return fail(ctx, GPSX_EINVAL, "null argument");
  const gpsx_wfix_cfg_t *cfg = &fc->fix;
  if (!(cfg->offset_ms - cfg->offset_ms == 0.0))   // (not finite: the difference is a NaN)
    return fail(ctx, GPSX_EINVAL, "offset_ms is not finite");
  for (double v : cfg->ion)
    if (!(v - v == 0.0))
      return fail(ctx, GPSX_EINVAL, "an ionosphere coefficient is not finite");
  if (cfg->ch_per_rx < 1 || cfg->ch_per_rx > 64)
    return fail(ctx, GPSX_EINVAL, "ch_per_rx must be 1..64");
  if (cfg->min_sats < 4 || cfg->min_sats > 64)
    return fail(ctx, GPSX_EINVAL, "min_sats must be 4..64");
  if (cfg->reserved0 != 0 || cfg->reserved1 != 0 || cfg->reserved2 != 0 || cfg->reserved3 != 0)
    return fail(ctx, GPSX_EINVAL, "reserved must be 0");
  if (!(fc->z_global >= 0.0 && fc->z_global <= 10.0))   // (a NaN fails it)
    return fail(ctx, GPSX_EINVAL, "z_global must be finite and 0..10");
  if (fc->max_excl < 0 || fc->max_excl > 8)
    return fail(ctx, GPSX_EINVAL, "max_excl must be 0..8");
  if (fc->repair != 0 && fc->repair != 1)
    return fail(ctx, GPSX_EINVAL, "repair must be 0 or 1");
  for (int32_t v : fc->reserved)
    if (v != 0)
      return fail(ctx, GPSX_EINVAL, "reserved must be 0");
  if (n_rx < 1 || n_rx > (1 << 20))
    return fail(ctx, GPSX_EINVAL, "n_rx must be 1..1048576");
  if (!host && (reinterpret_cast<uintptr_t>(fix) & 15u) != 0)
    return fail(ctx, GPSX_EINVAL, "d_fix must be 16-byte aligned");
  if (!host && (reinterpret_cast<uintptr_t>(fde) & 15u) != 0)
    return fail(ctx, GPSX_EINVAL, "d_fde must be 16-byte aligned");
  size_t obs_bytes = 0, eph_bytes = 0, lock_bytes = 0, fix_bytes = 0, fde_bytes = 0, pr_bytes = 0;
  if (records_overflow((size_t)n_rx, cfg->ch_per_rx, sizeof(gpsx_wobs_t), &obs_bytes) ||
      records_overflow((size_t)n_rx, cfg->ch_per_rx, sizeof(gpsx_weph_t), &eph_bytes) ||
      records_overflow((size_t)n_rx, cfg->ch_per_rx, sizeof(gpsx_wlock_t), &lock_bytes) ||
      records_overflow((size_t)n_rx, cfg->ch_per_rx, sizeof(double), &pr_bytes) || records_overflow((size_t)n_rx, 1, sizeof(gpsx_wfix_t), &fix_bytes) ||
      records_overflow((size_t)n_rx, 1, sizeof(gpsx_wfde_t), &fde_bytes))
    return fail(ctx, GPSX_EINVAL, "n_rx x ch_per_rx records overflow a size");
  const size_t n_ch = (size_t)n_rx * (size_t)cfg->ch_per_rx;
  const gpsx_wobs_t *d_obs = obs;
  const gpsx_weph_t *d_eph = eph;
  const gpsx_wlock_t *d_lock = lock;
  const gpsx_wfix_t *d_prev = prev;
  gpsx_wfix_t *d_fix = fix;
  gpsx_wfde_t *d_fde = fde;
  double *d_pr = pr_m;
  if (host) {
    if (int rc = arena_reset(ctx, arena_size(obs_bytes) + arena_size(eph_bytes) + (lock ? arena_size(lock_bytes) : 0) +
                                      (prev ? arena_size(fix_bytes) : 0) + arena_size(fix_bytes) + arena_size(fde_bytes) +
                                      (pr_m ? arena_size(pr_bytes) : 0)))
      return rc;
    if (int rc = stage_in(ctx, obs, n_ch, &d_obs)) return rc;
    if (int rc = stage_in(ctx, eph, n_ch, &d_eph)) return rc;
    if (int rc = stage_in(ctx, lock, n_ch, &d_lock)) return rc;
    if (int rc = stage_in(ctx, prev, (size_t)n_rx, &d_prev)) return rc;
    d_fix = arena_take<gpsx_wfix_t>(ctx, (size_t)n_rx);
    d_fde = arena_take<gpsx_wfde_t>(ctx, (size_t)n_rx);
    if (pr_m)
      d_pr = arena_take<double>(ctx, n_ch);
  }
  return launch_and_report(
      ctx, host, "k_wfde", "k_wfde raised the bad-state flag, which it never does",
      [&](uint32_t *) { launch_wfde(ctx->stream, *fc, d_obs, d_eph, d_lock, d_prev, n_rx, d_fix, d_fde, d_pr); },
      [&]() -> int {
        HIPCHK(ctx, hipMemcpyAsync(fix, d_fix, fix_bytes, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(fde, d_fde, fde_bytes, hipMemcpyDeviceToHost, ctx->stream));
        if (pr_m)
          HIPCHK(ctx, hipMemcpyAsync(pr_m, d_pr, pr_bytes, hipMemcpyDeviceToHost, ctx->stream));
        return GPSX_OK;
      });
}

// ---- the velocity fixes behind either (staged as wfix stages its arrays; the position records are an input here) ---------------------
int wvel(gpsx_ctx *ctx, const gpsx_wvel_cfg_t *cfg, const gpsx_wobs_t *obs, const gpsx_weph_t *eph, const gpsx_wlock_t *lock, const gpsx_wfix_t *fix,
         int n_rx, gpsx_wvel_t *vel, bool host)
{
  if (int rc = use_device(ctx)) return rc;
  if (!cfg || !obs || !eph || !fix || !vel)
    return fail(ctx, GPSX_EINVAL, "null argument");
  if (!(cfg->mps_per_hz - cfg->mps_per_hz == 0.0) || cfg->mps_per_hz == 0.0)   // (not finite: the difference is a NaN)
    return fail(ctx, GPSX_EINVAL, "mps_per_hz must be finite and not 0");
  if (cfg->ch_per_rx < 1 || cfg->ch_per_rx > 64)
    return fail(ctx, GPSX_EINVAL, "ch_per_rx must be 1..64");
  if (cfg->min_sats < 4 || cfg->min_sats > 64)
    return fail(ctx, GPSX_EINVAL, "min_sats must be 4..64");
  for (int32_t v : cfg->reserved)
    if (v != 0)
      return fail(ctx, GPSX_EINVAL, "reserved must be 0");
  if (n_rx < 1 || n_rx > (1 << 20))
    return fail(ctx, GPSX_EINVAL, "n_rx must be 1..1048576");
  if (!host && (reinterpret_cast<uintptr_t>(vel) & 15u) != 0)
    return fail(ctx, GPSX_EINVAL, "d_vel must be 16-byte aligned");
  size_t obs_bytes = 0, eph_bytes = 0, lock_bytes = 0, fix_bytes = 0, vel_bytes = 0;
  if (records_overflow((size_t)n_rx, cfg->ch_per_rx, sizeof(gpsx_wobs_t), &obs_bytes) ||
      records_overflow((size_t)n_rx, cfg->ch_per_rx, sizeof(gpsx_weph_t), &eph_bytes) ||
      records_overflow((size_t)n_rx, cfg->ch_per_rx, sizeof(gpsx_wlock_t), &lock_bytes) ||
      records_overflow((size_t)n_rx, 1, sizeof(gpsx_wfix_t), &fix_bytes) || records_overflow((size_t)n_rx, 1, sizeof(gpsx_wvel_t), &vel_bytes))
    return fail(ctx, GPSX_EINVAL, "n_rx x ch_per_rx records overflow a size");
  const size_t n_ch = (size_t)n_rx * (size_t)cfg->ch_per_rx;
  const gpsx_wobs_t *d_obs = obs;
  const gpsx_weph_t *d_eph = eph;
  const gpsx_wlock_t *d_lock = lock;
  const gpsx_wfix_t *d_fix = fix;
  gpsx_wvel_t *d_vel = vel;
  if (host) {
    if (int rc = arena_reset(ctx, arena_size(obs_bytes) + arena_size(eph_bytes) + (lock ? arena_size(lock_bytes) : 0) + arena_size(fix_bytes) +
                                      arena_size(vel_bytes)))
      return rc;
    if (int rc = stage_in(ctx, obs, n_ch, &d_obs)) return rc;
    if (int rc = stage_in(ctx, eph, n_ch, &d_eph)) return rc;
    if (int rc = stage_in(ctx, lock, n_ch, &d_lock)) return rc;
    if (int rc = stage_in(ctx, fix, (size_t)n_rx, &d_fix)) return rc;
    d_vel = arena_take<gpsx_wvel_t>(ctx, (size_t)n_rx);
  }
  return launch_and_report(
      ctx, host, "k_wvel", "k_wvel raised the bad-state flag, which it never does",
      [&](uint32_t *) { launch_wvel(ctx->stream, *cfg, d_obs, d_eph, d_lock, d_fix, n_rx, d_vel); },
      [&]() -> int {
        HIPCHK(ctx, hipMemcpyAsync(vel, d_vel, vel_bytes, hipMemcpyDeviceToHost, ctx->stream));
        return GPSX_OK;
      });
}

// ---- the navigation filter behind them (staged as wfix stages its arrays; the state is device memory in both variants) ----------------
int wkf(gpsx_ctx *ctx, const gpsx_wkf_cfg_t *cfg, const gpsx_wobs_t *obs, const gpsx_weph_t *eph, const gpsx_wlock_t *lock, const gpsx_wfix_t *fix,
        const gpsx_wvel_t *vel, int n_rx, int n_blocks, gpsx_wkf_state_t *d_state, gpsx_wkf_t *kf, bool host)
{
  if (int rc = use_device(ctx)) return rc;
  if (!cfg || !obs || !eph || !d_state || !kf)
    return fail(ctx, GPSX_EINVAL, "null argument");
  if (cfg->ch_per_rx < 1 || cfg->ch_per_rx > 64)
    return fail(ctx, GPSX_EINVAL, "ch_per_rx must be 1..64");
  if (n_rx < 1 || n_rx > (1 << 20))
    return fail(ctx, GPSX_EINVAL, "n_rx must be 1..1048576");
  if (int rc = check_n_blocks(ctx, n_blocks)) return rc;
  if (cfg->max_coast < 0 || cfg->max_coast > 1000000)
    return fail(ctx, GPSX_EINVAL, "max_coast must be 0..1000000");
  if (!(cfg->gate > 0.0 && cfg->gate <= 100.0))   // (a NaN fails it)
    return fail(ctx, GPSX_EINVAL, "gate must be finite, above 0 and at most 100");
  if (!(cfg->sig_dop_mps - cfg->sig_dop_mps == 0.0) || !(cfg->sig_dop_mps > 0.0))   // (not finite: the difference is a NaN)
    return fail(ctx, GPSX_EINVAL, "sig_dop_mps must be finite and above 0");
  for (double v : {cfg->sig_pr_m, cfg->q_acc, cfg->q_clk_f, cfg->q_clk_g, cfg->p0_pos, cfg->p0_clk, cfg->p0_vel, cfg->p0_drift})
    if (!(v - v == 0.0) || v < 0.0)
      return fail(ctx, GPSX_EINVAL, "sig_pr_m, q_* and p0_* must be finite and not negative");
  for (double v : {cfg->p0_pos, cfg->p0_clk, cfg->p0_vel, cfg->p0_drift})
    if (v == 0.0)
      return fail(ctx, GPSX_EINVAL, "p0_* must not be 0");
  if (!(cfg->mps_per_hz - cfg->mps_per_hz == 0.0) || cfg->mps_per_hz == 0.0)
    return fail(ctx, GPSX_EINVAL, "mps_per_hz must be finite and not 0");
  for (double v : cfg->ion)
    if (!(v - v == 0.0))
      return fail(ctx, GPSX_EINVAL, "an ionosphere coefficient is not finite");
  for (int32_t v : cfg->reserved)
    if (v != 0)
      return fail(ctx, GPSX_EINVAL, "reserved must be 0");
  if ((reinterpret_cast<uintptr_t>(d_state) & 15u) != 0)
    return fail(ctx, GPSX_EINVAL, "d_state must be 16-byte aligned");
  if (!host && (reinterpret_cast<uintptr_t>(kf) & 15u) != 0)
    return fail(ctx, GPSX_EINVAL, "d_kf must be 16-byte aligned");
  size_t obs_bytes = 0, eph_bytes = 0, lock_bytes = 0, fix_bytes = 0, vel_bytes = 0, kf_bytes = 0, bytes = 0;
  if (records_overflow((size_t)n_rx, cfg->ch_per_rx, sizeof(gpsx_wobs_t), &obs_bytes) ||
      records_overflow((size_t)n_rx, cfg->ch_per_rx, sizeof(gpsx_weph_t), &eph_bytes) ||
      records_overflow((size_t)n_rx, cfg->ch_per_rx, sizeof(gpsx_wlock_t), &lock_bytes) ||
      records_overflow((size_t)n_rx, 1, sizeof(gpsx_wfix_t), &fix_bytes) || records_overflow((size_t)n_rx, 1, sizeof(gpsx_wvel_t), &vel_bytes) ||
      records_overflow((size_t)n_rx, 1, sizeof(gpsx_wkf_state_t), &bytes) || records_overflow((size_t)n_rx, 1, sizeof(gpsx_wkf_t), &kf_bytes))
    return fail(ctx, GPSX_EINVAL, "n_rx x ch_per_rx records overflow a size");
  const size_t n_ch = (size_t)n_rx * (size_t)cfg->ch_per_rx;
  const gpsx_wobs_t *d_obs = obs;
  const gpsx_weph_t *d_eph = eph;
  const gpsx_wlock_t *d_lock = lock;
  const gpsx_wfix_t *d_fix = fix;
  const gpsx_wvel_t *d_vel = vel;
  gpsx_wkf_t *d_kf = kf;
  if (host) {
    if (int rc = arena_reset(ctx, arena_size(obs_bytes) + arena_size(eph_bytes) + (lock ? arena_size(lock_bytes) : 0) +
                                      (fix ? arena_size(fix_bytes) : 0) + (vel ? arena_size(vel_bytes) : 0) + arena_size(kf_bytes)))
      return rc;
    if (int rc = stage_in(ctx, obs, n_ch, &d_obs)) return rc;
    if (int rc = stage_in(ctx, eph, n_ch, &d_eph)) return rc;
    if (int rc = stage_in(ctx, lock, n_ch, &d_lock)) return rc;
    if (int rc = stage_in(ctx, fix, (size_t)n_rx, &d_fix)) return rc;
    if (int rc = stage_in(ctx, vel, (size_t)n_rx, &d_vel)) return rc;
    d_kf = arena_take<gpsx_wkf_t>(ctx, (size_t)n_rx);
  }
  return launch_and_report(
      ctx, host, "k_wkf", "a receiver's filter state is out of range (its state is untouched, its record is zero but for the flag)",
      [&](uint32_t *flag) { launch_wkf(ctx->stream, *cfg, d_obs, d_eph, d_lock, d_fix, d_vel, n_rx, n_blocks, d_state, d_kf, flag); },
      [&]() -> int {
        HIPCHK(ctx, hipMemcpyAsync(kf, d_kf, kf_bytes, hipMemcpyDeviceToHost, ctx->stream));
        return GPSX_OK;
      });
}

// ---- acquisition decisions and slot hand-over (host: peaks, acq and det are host memory, staged through the arena; the five state
//      arrays are device memory in both variants) -----------------------------------------------------------------------------------------
int wacq(gpsx_ctx *ctx, const gpsx_wacq_cfg_t *cfg, const gpsx_acq_weighted_t *g, const gpsx_peak_t *peaks, gpsx_wsync_state_t *d_sync_state,
         gpsx_wlock_state_t *d_lock_state, gpsx_wnav_state_t *d_nav_state, gpsx_wobs_state_t *d_obs_state, gpsx_weph_state_t *d_eph_state,
         gpsx_wacq_t *acq, gpsx_wacq_det_t *det, bool host)
{
  if (int rc = use_device(ctx)) return rc;
  if (!cfg || !g || !g->prns || !peaks || !d_sync_state || !acq)
    return fail(ctx, GPSX_EINVAL, "null argument");
  if (cfg->ch_per_rx < 1 || cfg->ch_per_rx > 64)
    return fail(ctx, GPSX_EINVAL, "ch_per_rx must be 1..64");
  if (cfg->det_num < 1 || cfg->det_num > 1024 || cfg->det_den < 1 || cfg->det_den > 1024 || cfg->det_num < cfg->det_den)
    return fail(ctx, GPSX_EINVAL, "det_num and det_den must be 1..1024, det_num >= det_den");
  if (cfg->lead_blocks < 0 || cfg->lead_blocks > 4096)
    return fail(ctx, GPSX_EINVAL, "lead_blocks must be 0..4096");
  if (!(__builtin_fabsf(cfg->code_per_hz) <= 1.0f))   // (a NaN fails it)
    return fail(ctx, GPSX_EINVAL, "code_per_hz must be finite and -1..1");
  if (cfg->evict_after_blocks < 0 || cfg->evict_after_blocks > (1 << 30))
    return fail(ctx, GPSX_EINVAL, "evict_after_blocks must be 0..1073741824");
  if (cfg->reserved != 0)
    return fail(ctx, GPSX_EINVAL, "reserved must be 0");
  if (cfg->evict_after_blocks != 0 && !d_lock_state)
    return fail(ctx, GPSX_EINVAL, "evict_after_blocks needs d_lock_state");
  if (g->n_search < 1 || g->n_search > (1 << 20))
    return fail(ctx, GPSX_EINVAL, "n_search must be 1..1048576");
  if (g->n_prn < 1 || g->n_prn > 64)
    return fail(ctx, GPSX_EINVAL, "n_prn must be 1..64");
  if (g->n_dopp < 1 || g->n_dopp > (1 << 20))   // (the kernel counts bins in int32, four turns of 64 ahead)
    return fail(ctx, GPSX_EINVAL, "n_dopp must be 1..1048576");
  bool listed[GPSX_MAX_PRN + 1] = {};
  for (int i = 0; i < g->n_prn; i++) {
    if (g->prns[i] < 1 || g->prns[i] > GPSX_MAX_PRN)
      return fail(ctx, GPSX_EINVAL, "PRN outside 1..210");
    if (listed[g->prns[i]])
      return fail(ctx, GPSX_EINVAL, "a PRN is listed twice");
    listed[g->prns[i]] = true;
  }
  const long long f_first = g->dopp_min_hz, f_last = f_first + (long long)(g->n_dopp - 1) * (long long)g->dopp_step_hz;
  if (f_last < -2147483647ll - 1 || f_last > 2147483647ll)
    return fail(ctx, GPSX_EINVAL, "a Doppler bin lies outside int32");
  const double f_max = (double)std::max(f_first < 0 ? -f_first : f_first, f_last < 0 ? -f_last : f_last);
  if (std::fabs((double)cfg->code_per_hz) * f_max * (double)cfg->lead_blocks * 0.001 >= 16368.0)
    return fail(ctx, GPSX_EINVAL, "the projection must stay below one code period (|code_per_hz| x max |Doppler| x lead_blocks x 0.001 < 16368)");
  size_t peak_bytes = 0, acq_bytes = 0, det_bytes = 0, bytes = 0;
  if (records_overflow((size_t)g->n_search * (size_t)g->n_prn, g->n_dopp, sizeof(gpsx_peak_t), &peak_bytes) ||
      records_overflow((size_t)g->n_search, cfg->ch_per_rx, sizeof(gpsx_wsync_state_t), &bytes) ||
      records_overflow((size_t)g->n_search, g->n_prn, sizeof(gpsx_wacq_det_t), &det_bytes) ||
      records_overflow((size_t)g->n_search, 1, sizeof(gpsx_wacq_t), &acq_bytes))
    return fail(ctx, GPSX_EINVAL, "n_search x n_prn x n_dopp records overflow a size");
  const gpsx_peak_t *d_peaks = peaks;
  gpsx_wacq_t *d_acq = acq;
  gpsx_wacq_det_t *d_det = det;
  if (host) {
    if (int rc = arena_reset(ctx, arena_size(peak_bytes) + arena_size(acq_bytes) + (det ? arena_size(det_bytes) : 0))) return rc;
    if (int rc = stage_in(ctx, peaks, peak_bytes / sizeof(gpsx_peak_t), &d_peaks)) return rc;
    d_acq = arena_take<gpsx_wacq_t>(ctx, (size_t)g->n_search);
    if (det)
      d_det = arena_take<gpsx_wacq_det_t>(ctx, det_bytes / sizeof(gpsx_wacq_det_t));
  }
  return launch_and_report(
      ctx, host, "k_wacq", "k_wacq raised the bad-state flag, which it never does",
      [&](uint32_t *) {
        launch_wacq(ctx->stream, *cfg, g->n_search, g->n_prn, g->prns, g->dopp_min_hz, g->dopp_step_hz, g->n_dopp, d_peaks, d_sync_state, d_lock_state,
                    d_nav_state, d_obs_state, d_eph_state, d_acq, d_det);
      },
      [&]() -> int {
        HIPCHK(ctx, hipMemcpyAsync(acq, d_acq, acq_bytes, hipMemcpyDeviceToHost, ctx->stream));
        if (det)
          HIPCHK(ctx, hipMemcpyAsync(det, d_det, det_bytes, hipMemcpyDeviceToHost, ctx->stream));
        return GPSX_OK;
      });
}

// ---- the ephemeris bank (host: eph, eph_out and rep are host memory, staged through the arena; the sync states and the bank are device
//      memory in both variants) ------------------------------------------------------------------------------------------------------
int wbank(gpsx_ctx *ctx, const gpsx_wbank_cfg_t *cfg, int n_rx, int n_prn, const uint8_t *prns, const gpsx_wsync_state_t *d_sync_state,
          const gpsx_weph_t *eph, gpsx_weph_t *d_bank, gpsx_weph_t *eph_out, gpsx_wbank_t *rep, bool host)
{
  if (int rc = use_device(ctx)) return rc;
  if (!cfg || !prns || !d_sync_state || !eph || !d_bank || !rep)
    return fail(ctx, GPSX_EINVAL, "null argument");
  if (cfg->ch_per_rx < 1 || cfg->ch_per_rx > 64)
    return fail(ctx, GPSX_EINVAL, "ch_per_rx must be 1..64");
  if (cfg->reserved[0] != 0 || cfg->reserved[1] != 0 || cfg->reserved[2] != 0)
    return fail(ctx, GPSX_EINVAL, "reserved must be 0");
  if (n_rx < 1 || n_rx > (1 << 20))
    return fail(ctx, GPSX_EINVAL, "n_rx must be 1..1048576");
  if (n_prn < 1 || n_prn > 64)
    return fail(ctx, GPSX_EINVAL, "n_prn must be 1..64");
  bool listed[GPSX_MAX_PRN + 1] = {};
  for (int i = 0; i < n_prn; i++) {
    if (prns[i] < 1 || prns[i] > GPSX_MAX_PRN)
      return fail(ctx, GPSX_EINVAL, "PRN outside 1..210");
    if (listed[prns[i]])
      return fail(ctx, GPSX_EINVAL, "a PRN is listed twice");
    listed[prns[i]] = true;
  }
  if ((reinterpret_cast<uintptr_t>(d_sync_state) & 7u) != 0)
    return fail(ctx, GPSX_EINVAL, "d_sync_state must be 8-byte aligned");
  if ((reinterpret_cast<uintptr_t>(d_bank) & 15u) != 0)
    return fail(ctx, GPSX_EINVAL, "d_bank must be 16-byte aligned");
  if (!host && ((reinterpret_cast<uintptr_t>(eph) | reinterpret_cast<uintptr_t>(eph_out) | reinterpret_cast<uintptr_t>(rep)) & 15u) != 0)
    return fail(ctx, GPSX_EINVAL, "d_eph, d_eph_out and d_rep must be 16-byte aligned");
  size_t sync_bytes = 0, eph_bytes = 0, bank_bytes = 0, rep_bytes = 0;
  if (records_overflow((size_t)n_rx, cfg->ch_per_rx, sizeof(gpsx_wsync_state_t), &sync_bytes) ||
      records_overflow((size_t)n_rx, cfg->ch_per_rx, sizeof(gpsx_weph_t), &eph_bytes) ||
      records_overflow((size_t)n_rx, n_prn, sizeof(gpsx_weph_t), &bank_bytes) || records_overflow((size_t)n_rx, 1, sizeof(gpsx_wbank_t), &rep_bytes))
    return fail(ctx, GPSX_EINVAL, "n_rx x n_prn records overflow a size");
  // (host and device addresses share one space here: one list of pairs serves both variants)
  const struct { const void *p; size_t n; } span[5] = {{d_sync_state, sync_bytes}, {eph, eph_bytes}, {d_bank, bank_bytes}, {eph_out, eph_bytes}, {rep, rep_bytes}};
  for (int a = 0; a < 5; a++)
    for (int b = a + 1; b < 5; b++) {
      const uintptr_t pa = reinterpret_cast<uintptr_t>(span[a].p), pb = reinterpret_cast<uintptr_t>(span[b].p);
      if (!pa || !pb || (a == 1 && b == 3 && pa == pb))
        continue;
      if (pa < pb + span[b].n && pb < pa + span[a].n)
        return fail(ctx, GPSX_EINVAL, "two arrays overlap (only d_eph_out == d_eph may)");
    }
  const size_t n_ch = (size_t)n_rx * (size_t)cfg->ch_per_rx;
  const gpsx_weph_t *d_eph = eph;
  gpsx_weph_t *d_out = eph_out;
  gpsx_wbank_t *d_rep = rep;
  if (host) {
    const bool own_out = eph_out && eph_out != eph;
    if (int rc = arena_reset(ctx, arena_size(eph_bytes) + (own_out ? arena_size(eph_bytes) : 0) + arena_size(rep_bytes))) return rc;
    if (int rc = stage_in(ctx, eph, n_ch, &d_eph)) return rc;
    if (eph_out)
      d_out = own_out ? arena_take<gpsx_weph_t>(ctx, n_ch) : const_cast<gpsx_weph_t *>(d_eph);     // (in place: on the staged copy)
    d_rep = arena_take<gpsx_wbank_t>(ctx, (size_t)n_rx);
  }
  return launch_and_report(
      ctx, host, "k_wbank", "k_wbank raised the bad-state flag, which it never does",
      [&](uint32_t *) { launch_wbank(ctx->stream, *cfg, n_rx, n_prn, prns, d_sync_state, d_eph, d_bank, d_out, d_rep); },
      [&]() -> int {
        HIPCHK(ctx, hipMemcpyAsync(rep, d_rep, rep_bytes, hipMemcpyDeviceToHost, ctx->stream));
        if (eph_out)
          HIPCHK(ctx, hipMemcpyAsync(eph_out, d_out, eph_bytes, hipMemcpyDeviceToHost, ctx->stream));
        return GPSX_OK;
      });
}

// ---- prediction and hot hand-over (host: rx and pred are host memory, staged through the arena; the filter states, the bank and the
//      five state arrays are device memory in both variants) ---------------------------------------------------------------------------
int wpred(gpsx_ctx *ctx, const gpsx_wpred_cfg_t *cfg, int n_rx, int n_prn, const uint8_t *prns, const gpsx_wkf_state_t *d_kf_state,
          const gpsx_weph_t *d_bank, gpsx_wsync_state_t *d_sync_state, gpsx_wlock_state_t *d_lock_state, gpsx_wnav_state_t *d_nav_state,
          gpsx_wobs_state_t *d_obs_state, gpsx_weph_state_t *d_eph_state, gpsx_wpred_rx_t *rx, gpsx_wpred_t *pred, bool host)
{
  if (int rc = use_device(ctx)) return rc;
  if (!cfg || !prns || !d_kf_state || !d_bank || !d_sync_state || !rx)
    return fail(ctx, GPSX_EINVAL, "null argument");
  for (double v : cfg->ion)
    if (!(v - v == 0.0))   // (not finite: the difference is a NaN)
      return fail(ctx, GPSX_EINVAL, "an ionosphere coefficient is not finite");
  if (!(cfg->mps_per_hz - cfg->mps_per_hz == 0.0) || cfg->mps_per_hz == 0.0)
    return fail(ctx, GPSX_EINVAL, "mps_per_hz must be finite and not 0");
  if (!(std::fabs(cfg->el_min_rad) <= 1.5707963267948966))   // (a NaN fails it)
    return fail(ctx, GPSX_EINVAL, "el_min_rad must be finite and within -pi/2..pi/2");
  if (!(cfg->max_sigma_m - cfg->max_sigma_m == 0.0) || !(cfg->max_sigma_m > 0.0) || !(cfg->max_sigma_hz - cfg->max_sigma_hz == 0.0) ||
      !(cfg->max_sigma_hz > 0.0))
    return fail(ctx, GPSX_EINVAL, "max_sigma_m and max_sigma_hz must be finite and above 0");
  if (cfg->ch_per_rx < 1 || cfg->ch_per_rx > 64)
    return fail(ctx, GPSX_EINVAL, "ch_per_rx must be 1..64");
  if (cfg->lead_blocks < 0 || cfg->lead_blocks > 4096)
    return fail(ctx, GPSX_EINVAL, "lead_blocks must be 0..4096");
  if (cfg->evict_after_blocks < 0 || cfg->evict_after_blocks > (1 << 30))
    return fail(ctx, GPSX_EINVAL, "evict_after_blocks must be 0..1073741824");
  if (cfg->handover != 0 && cfg->handover != 1)
    return fail(ctx, GPSX_EINVAL, "handover must be 0 or 1");
  if (cfg->reserved[0] != 0 || cfg->reserved[1] != 0 || cfg->reserved[2] != 0 || cfg->reserved[3] != 0)
    return fail(ctx, GPSX_EINVAL, "reserved must be 0");
  if (cfg->evict_after_blocks != 0 && !d_lock_state)
    return fail(ctx, GPSX_EINVAL, "evict_after_blocks needs d_lock_state");
  if (n_rx < 1 || n_rx > (1 << 20))
    return fail(ctx, GPSX_EINVAL, "n_rx must be 1..1048576");
  if (n_prn < 1 || n_prn > 64)
    return fail(ctx, GPSX_EINVAL, "n_prn must be 1..64");
  bool listed[GPSX_MAX_PRN + 1] = {};
  for (int i = 0; i < n_prn; i++) {
    if (prns[i] < 1 || prns[i] > GPSX_MAX_PRN)
      return fail(ctx, GPSX_EINVAL, "PRN outside 1..210");
    if (listed[prns[i]])
      return fail(ctx, GPSX_EINVAL, "a PRN is listed twice");
    listed[prns[i]] = true;
  }
  if (((reinterpret_cast<uintptr_t>(d_kf_state) | reinterpret_cast<uintptr_t>(d_bank)) & 15u) != 0)
    return fail(ctx, GPSX_EINVAL, "d_kf_state and d_bank must be 16-byte aligned");
  if (!host && ((reinterpret_cast<uintptr_t>(rx) | reinterpret_cast<uintptr_t>(pred)) & 15u) != 0)
    return fail(ctx, GPSX_EINVAL, "d_rx and d_pred must be 16-byte aligned");
  size_t bytes = 0, rx_bytes = 0, pred_bytes = 0;
  if (records_overflow((size_t)n_rx, cfg->ch_per_rx, sizeof(gpsx_wsync_state_t), &bytes) ||
      records_overflow((size_t)n_rx, n_prn, sizeof(gpsx_weph_t), &bytes) || records_overflow((size_t)n_rx, n_prn, sizeof(gpsx_wpred_t), &pred_bytes) ||
      records_overflow((size_t)n_rx, 1, sizeof(gpsx_wpred_rx_t), &rx_bytes))
    return fail(ctx, GPSX_EINVAL, "n_rx x n_prn records overflow a size");
  gpsx_wpred_rx_t *d_rx = rx;
  gpsx_wpred_t *d_pred = pred;
  if (host) {
    if (int rc = arena_reset(ctx, arena_size(rx_bytes) + (pred ? arena_size(pred_bytes) : 0))) return rc;
    d_rx = arena_take<gpsx_wpred_rx_t>(ctx, (size_t)n_rx);
    if (pred)
      d_pred = arena_take<gpsx_wpred_t>(ctx, pred_bytes / sizeof(gpsx_wpred_t));
  }
  return launch_and_report(
      ctx, host, "k_wpred", "k_wpred raised the bad-state flag, which it never does",
      [&](uint32_t *) {
        launch_wpred(ctx->stream, *cfg, n_rx, n_prn, prns, d_kf_state, d_bank, d_sync_state, d_lock_state, d_nav_state, d_obs_state, d_eph_state, d_rx,
                     d_pred);
      },
      [&]() -> int {
        HIPCHK(ctx, hipMemcpyAsync(rx, d_rx, rx_bytes, hipMemcpyDeviceToHost, ctx->stream));
        if (pred)
          HIPCHK(ctx, hipMemcpyAsync(pred, d_pred, pred_bytes, hipMemcpyDeviceToHost, ctx->stream));
        return GPSX_OK;
      });
}

// ---- snapshot fixes (host: peaks, prior, snap and sv are host memory, staged through the arena; the bank is device memory in both
//      variants) ------------------------------------------------------------------------------------------------------------------------
int wsnap(gpsx_ctx *ctx, const gpsx_wsnap_cfg_t *cfg, const gpsx_acq_weighted_t *g, const gpsx_peak_t *peaks, const gpsx_weph_t *d_bank,
          int bank_stride, const gpsx_wsnap_prior_t *prior, gpsx_wsnap_t *snap, gpsx_wsnap_sv_t *sv, bool host)
{
  if (int rc = use_device(ctx)) return rc;
  if (!cfg || !g || !g->prns || !peaks || !d_bank || !prior || !snap)
    return fail(ctx, GPSX_EINVAL, "null argument");
  for (double v : cfg->ion)
    if (!(v - v == 0.0))   // (not finite: the difference is a NaN)
      return fail(ctx, GPSX_EINVAL, "an ionosphere coefficient is not finite");
  if (!(std::fabs(cfg->el_min_rad) <= 1.5707963267948966))   // (a NaN fails it)
    return fail(ctx, GPSX_EINVAL, "el_min_rad must be finite and within -pi/2..pi/2");
  if (!(cfg->epoch_offset_s >= 0.0 && cfg->epoch_offset_s <= 4.096))
    return fail(ctx, GPSX_EINVAL, "epoch_offset_s must be finite and 0..4.096");
  if (!(cfg->max_resid_m - cfg->max_resid_m == 0.0) || !(cfg->max_resid_m > 0.0))
    return fail(ctx, GPSX_EINVAL, "max_resid_m must be finite and above 0");
  if (cfg->det_num < 1 || cfg->det_num > 1024 || cfg->det_den < 1 || cfg->det_den > 1024 || cfg->det_num < cfg->det_den)
    return fail(ctx, GPSX_EINVAL, "det_num and det_den must be 1..1024, det_num >= det_den");
  if (cfg->min_sats < 5 || cfg->min_sats > 64)
    return fail(ctx, GPSX_EINVAL, "min_sats must be 5..64");
  for (int32_t v : cfg->reserved)
    if (v != 0)
      return fail(ctx, GPSX_EINVAL, "reserved must be 0");
  if (g->n_search < 1 || g->n_search > (1 << 20))
    return fail(ctx, GPSX_EINVAL, "n_search must be 1..1048576");
  if (g->n_prn < 1 || g->n_prn > 64)
    return fail(ctx, GPSX_EINVAL, "n_prn must be 1..64");
  if (g->n_dopp < 1 || g->n_dopp > (1 << 20))   // (the kernel counts bins in int32, four turns of 64 ahead)
    return fail(ctx, GPSX_EINVAL, "n_dopp must be 1..1048576");
  bool listed[GPSX_MAX_PRN + 1] = {};
  for (int i = 0; i < g->n_prn; i++) {
    if (g->prns[i] < 1 || g->prns[i] > GPSX_MAX_PRN)
      return fail(ctx, GPSX_EINVAL, "PRN outside 1..210");
    if (listed[g->prns[i]])
      return fail(ctx, GPSX_EINVAL, "a PRN is listed twice");
    listed[g->prns[i]] = true;
  }
  const long long f_first = g->dopp_min_hz, f_last = f_first + (long long)(g->n_dopp - 1) * (long long)g->dopp_step_hz;
  if (f_last < -2147483647ll - 1 || f_last > 2147483647ll)
    return fail(ctx, GPSX_EINVAL, "a Doppler bin lies outside int32");
  if (bank_stride != 0 && bank_stride != g->n_prn)
    return fail(ctx, GPSX_EINVAL, "bank_stride must be 0 or n_prn");
  if ((reinterpret_cast<uintptr_t>(d_bank) & 15u) != 0)
    return fail(ctx, GPSX_EINVAL, "d_bank must be 16-byte aligned");
  if (!host && ((reinterpret_cast<uintptr_t>(peaks) & 3u) != 0 || (reinterpret_cast<uintptr_t>(prior) & 7u) != 0))
    return fail(ctx, GPSX_EINVAL, "d_peaks must be 4-byte and d_prior 8-byte aligned");
  if (!host && ((reinterpret_cast<uintptr_t>(snap) | reinterpret_cast<uintptr_t>(sv)) & 15u) != 0)
    return fail(ctx, GPSX_EINVAL, "d_snap and d_sv must be 16-byte aligned");
  size_t peak_bytes = 0, bank_bytes = 0, prior_bytes = 0, snap_bytes = 0, sv_bytes = 0;
  if (records_overflow((size_t)g->n_search * (size_t)g->n_prn, g->n_dopp, sizeof(gpsx_peak_t), &peak_bytes) ||
      records_overflow((size_t)(bank_stride ? g->n_search : 1), g->n_prn, sizeof(gpsx_weph_t), &bank_bytes) ||
      records_overflow((size_t)g->n_search, 1, sizeof(gpsx_wsnap_prior_t), &prior_bytes) ||
      records_overflow((size_t)g->n_search, 1, sizeof(gpsx_wsnap_t), &snap_bytes) ||
      records_overflow((size_t)g->n_search, g->n_prn, sizeof(gpsx_wsnap_sv_t), &sv_bytes))
    return fail(ctx, GPSX_EINVAL, "n_search x n_prn x n_dopp records overflow a size");
  if (!host) {
    // (the two outputs against each other and against the three inputs)
    const struct { const void *p; size_t n; } span[5] = {{snap, snap_bytes}, {sv, sv_bytes}, {peaks, peak_bytes}, {d_bank, bank_bytes}, {prior, prior_bytes}};
    for (int a = 0; a < 2; a++)
      for (int b = a + 1; b < 5; b++) {
        const uintptr_t pa = reinterpret_cast<uintptr_t>(span[a].p), pb = reinterpret_cast<uintptr_t>(span[b].p);
        if (!pa || !pb)
          continue;
        if (pa < pb + span[b].n && pb < pa + span[a].n)
          return fail(ctx, GPSX_EINVAL, "d_snap or d_sv overlaps another array");
      }
  }
  const gpsx_peak_t *d_peaks = peaks;
  const gpsx_wsnap_prior_t *d_prior = prior;
  gpsx_wsnap_t *d_snap = snap;
  gpsx_wsnap_sv_t *d_sv = sv;
  if (host) {
    if (int rc = arena_reset(ctx, arena_size(peak_bytes) + arena_size(prior_bytes) + arena_size(snap_bytes) + (sv ? arena_size(sv_bytes) : 0))) return rc;
    if (int rc = stage_in(ctx, peaks, peak_bytes / sizeof(gpsx_peak_t), &d_peaks)) return rc;
    if (int rc = stage_in(ctx, prior, (size_t)g->n_search, &d_prior)) return rc;
    d_snap = arena_take<gpsx_wsnap_t>(ctx, (size_t)g->n_search);
    if (sv)
      d_sv = arena_take<gpsx_wsnap_sv_t>(ctx, sv_bytes / sizeof(gpsx_wsnap_sv_t));
  }
  return launch_and_report(
      ctx, host, "k_wsnap", "k_wsnap raised the bad-state flag, which it never does",
      [&](uint32_t *) {
        launch_wsnap(ctx->stream, *cfg, g->n_search, g->n_prn, g->dopp_min_hz, g->dopp_step_hz, g->n_dopp, d_peaks, d_bank, bank_stride, d_prior, d_snap,
                     d_sv);
      },
      [&]() -> int {
        HIPCHK(ctx, hipMemcpyAsync(snap, d_snap, snap_bytes, hipMemcpyDeviceToHost, ctx->stream));
        if (sv)
          HIPCHK(ctx, hipMemcpyAsync(sv, d_sv, sv_bytes, hipMemcpyDeviceToHost, ctx->stream));
        return GPSX_OK;
      });
}

// ---- time-of-week aiding of the observables (host: tow and tow_rx are host memory, staged through the arena; the prediction's records,
//      the sync and observable states and the observables are device memory in both variants) ------------------------------------------
int wtow(gpsx_ctx *ctx, const gpsx_wtow_cfg_t *cfg, int n_rx, int n_prn, const uint8_t *prns, const gpsx_wpred_rx_t *d_pred_rx,
         const gpsx_wpred_t *d_pred, gpsx_wsync_state_t *d_sync_state, gpsx_wobs_state_t *d_obs_state, gpsx_wobs_t *d_obs, gpsx_wtow_t *tow,
         gpsx_wtow_rx_t *tow_rx, bool host)
{
  if (int rc = use_device(ctx)) return rc;
  if (!cfg || !prns || !d_pred_rx || !d_pred || !d_sync_state || !d_obs_state || !tow || !tow_rx)
    return fail(ctx, GPSX_EINVAL, "null argument");
  if (!(cfg->max_sigma_m - cfg->max_sigma_m == 0.0) || !(cfg->max_sigma_m > 0.0))   // (not finite: the difference is a NaN)
    return fail(ctx, GPSX_EINVAL, "max_sigma_m must be finite and above 0");
  if (!(cfg->max_resid_samples > 0.0f && cfg->max_resid_samples <= 4092.0f))   // (a NaN fails it)
    return fail(ctx, GPSX_EINVAL, "max_resid_samples must be finite, above 0 and at most 4092");
  if (cfg->ch_per_rx < 1 || cfg->ch_per_rx > 64)
    return fail(ctx, GPSX_EINVAL, "ch_per_rx must be 1..64");
  if (cfg->max_age_blocks < 0 || cfg->max_age_blocks > 4096)
    return fail(ctx, GPSX_EINVAL, "max_age_blocks must be 0..4096");
  if ((cfg->resolve != 0 && cfg->resolve != 1) || (cfg->rearm != 0 && cfg->rearm != 1))
    return fail(ctx, GPSX_EINVAL, "resolve and rearm must be 0 or 1");
  if (cfg->reserved != 0)
    return fail(ctx, GPSX_EINVAL, "reserved must be 0");
  if (n_rx < 1 || n_rx > (1 << 20))
    return fail(ctx, GPSX_EINVAL, "n_rx must be 1..1048576");
  if (n_prn < 1 || n_prn > 64)
    return fail(ctx, GPSX_EINVAL, "n_prn must be 1..64");
  bool listed[GPSX_MAX_PRN + 1] = {};
  for (int i = 0; i < n_prn; i++) {
    if (prns[i] < 1 || prns[i] > GPSX_MAX_PRN)
      return fail(ctx, GPSX_EINVAL, "PRN outside 1..210");
    if (listed[prns[i]])
      return fail(ctx, GPSX_EINVAL, "a PRN is listed twice");
    listed[prns[i]] = true;
  }
  if (((reinterpret_cast<uintptr_t>(d_pred_rx) | reinterpret_cast<uintptr_t>(d_pred) | reinterpret_cast<uintptr_t>(d_obs_state) |
        reinterpret_cast<uintptr_t>(d_obs)) & 15u) != 0)
    return fail(ctx, GPSX_EINVAL, "d_pred_rx, d_pred, d_obs_state and d_obs must be 16-byte aligned");
  if ((reinterpret_cast<uintptr_t>(d_sync_state) & 7u) != 0)
    return fail(ctx, GPSX_EINVAL, "d_sync_state must be 8-byte aligned");
  if (!host && ((reinterpret_cast<uintptr_t>(tow) | reinterpret_cast<uintptr_t>(tow_rx)) & 15u) != 0)
    return fail(ctx, GPSX_EINVAL, "d_tow and d_tow_rx must be 16-byte aligned");
  size_t rx_bytes = 0, pred_bytes = 0, sync_bytes = 0, st_bytes = 0, obs_bytes = 0, tow_bytes = 0, tow_rx_bytes = 0;
  if (records_overflow((size_t)n_rx, 1, sizeof(gpsx_wpred_rx_t), &rx_bytes) || records_overflow((size_t)n_rx, n_prn, sizeof(gpsx_wpred_t), &pred_bytes) ||
      records_overflow((size_t)n_rx, cfg->ch_per_rx, sizeof(gpsx_wsync_state_t), &sync_bytes) ||
      records_overflow((size_t)n_rx, cfg->ch_per_rx, sizeof(gpsx_wobs_state_t), &st_bytes) ||
      records_overflow((size_t)n_rx, cfg->ch_per_rx, sizeof(gpsx_wobs_t), &obs_bytes) ||
      records_overflow((size_t)n_rx, cfg->ch_per_rx, sizeof(gpsx_wtow_t), &tow_bytes) || records_overflow((size_t)n_rx, 1, sizeof(gpsx_wtow_rx_t), &tow_rx_bytes))
    return fail(ctx, GPSX_EINVAL, "n_rx x n_prn records overflow a size");
  // (host and device addresses share one space here: one list of spans serves both variants)
  const struct { const void *p; size_t n; } span[7] = {{tow, tow_bytes},           {tow_rx, tow_rx_bytes},    {d_pred_rx, rx_bytes}, {d_pred, pred_bytes},
                                                      {d_sync_state, sync_bytes}, {d_obs_state, st_bytes}, {d_obs, obs_bytes}};
  for (int a = 0; a < 2; a++)
    for (int b = a + 1; b < 7; b++) {
      const uintptr_t pa = reinterpret_cast<uintptr_t>(span[a].p), pb = reinterpret_cast<uintptr_t>(span[b].p);
      if (pb && pa < pb + span[b].n && pb < pa + span[a].n)
        return fail(ctx, GPSX_EINVAL, "d_tow or d_tow_rx overlaps another array");
    }
  gpsx_wtow_t *d_tow = tow;
  gpsx_wtow_rx_t *d_tow_rx = tow_rx;
  if (host) {
    if (int rc = arena_reset(ctx, arena_size(tow_bytes) + arena_size(tow_rx_bytes))) return rc;
    d_tow = arena_take<gpsx_wtow_t>(ctx, tow_bytes / sizeof(gpsx_wtow_t));
    d_tow_rx = arena_take<gpsx_wtow_rx_t>(ctx, (size_t)n_rx);
  }
  return launch_and_report(
      ctx, host, "k_wtow", "k_wtow raised the bad-state flag, which it never does",
      [&](uint32_t *) { launch_wtow(ctx->stream, *cfg, n_rx, n_prn, prns, d_pred_rx, d_pred, d_sync_state, d_obs_state, d_obs, d_tow, d_tow_rx); },
      [&]() -> int {
        HIPCHK(ctx, hipMemcpyAsync(tow, d_tow, tow_bytes, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(tow_rx, d_tow_rx, tow_rx_bytes, hipMemcpyDeviceToHost, ctx->stream));
        return GPSX_OK;
      });
}

// ---- the weighted grid in a window around each prediction (host: pred, the blocks, peaks and rep are host memory, staged through the
//      arena) ---------------------------------------------------------------------------------------------------------------------------
int acq_window(gpsx_ctx *ctx, const gpsx_acq_weighted_t *g, const gpsx_acq_window_t *cfg, const gpsx_wpred_t *pred, const void *if_blocks_2bit,
               int n_blocks, gpsx_peak_t *peaks, gpsx_acq_window_rep_t *rep, bool host)
{
  if (int rc = use_device(ctx)) return rc;
  if (!g || !cfg || !g->prns || !pred || !if_blocks_2bit || !peaks)
    return fail(ctx, GPSX_EINVAL, "null argument");
  if (cfg->n_coh < 1 || cfg->n_coh > 20)
    return fail(ctx, GPSX_EINVAL, "n_coh outside 1..20");
  if (cfg->n_seg < 1 || cfg->n_seg > 128)
    return fail(ctx, GPSX_EINVAL, "n_seg outside 1..128");
  if (cfg->half_width < 1 || cfg->half_width > 2047)
    return fail(ctx, GPSX_EINVAL, "half_width must be 1..2047");
  if (cfg->half_bins < 0 || cfg->half_bins > 32)
    return fail(ctx, GPSX_EINVAL, "half_bins must be 0..32");
  if (cfg->guard < 0 || cfg->guard > cfg->half_width - 1)
    return fail(ctx, GPSX_EINVAL, "guard must be 0..half_width - 1");
  if (((cfg->need_flags | cfg->skip_flags) & ~0x7Fu) != 0)
    return fail(ctx, GPSX_EINVAL, "need_flags and skip_flags must be GPSX_WPRED_* bits");
  if ((cfg->need_flags & GPSX_WPRED_PREDICTED) == 0)
    return fail(ctx, GPSX_EINVAL, "need_flags must contain GPSX_WPRED_PREDICTED");
  if (cfg->reserved != 0)
    return fail(ctx, GPSX_EINVAL, "reserved must be 0");
  if (g->weights != GPSX_WEIGHTS_SIGN_ONLY && g->weights != GPSX_WEIGHTS_SIGN_MAGNITUDE)
    return fail(ctx, GPSX_EINVAL, "unknown weights");
  if (g->dopp_step_hz < 1)
    return fail(ctx, GPSX_EINVAL, "dopp_step_hz must be at least 1");
  if (g->n_search < 1 || g->n_search > (1 << 20))
    return fail(ctx, GPSX_EINVAL, "n_search must be 1..1048576");
  if (g->n_prn < 1 || g->n_prn > 64)
    return fail(ctx, GPSX_EINVAL, "n_prn must be 1..64");
  if (g->n_dopp < 1 || g->n_dopp > (1 << 20))
    return fail(ctx, GPSX_EINVAL, "n_dopp must be 1..1048576");
  if (g->search_stride_blocks < 0)
    return fail(ctx, GPSX_EINVAL, "search_stride_blocks must be at least 0");
  bool listed[GPSX_MAX_PRN + 1] = {};
  for (int i = 0; i < g->n_prn; i++) {
    if (g->prns[i] < 1 || g->prns[i] > GPSX_MAX_PRN)
      return fail(ctx, GPSX_EINVAL, "PRN outside 1..210");
    if (listed[g->prns[i]])
      return fail(ctx, GPSX_EINVAL, "a PRN is listed twice");
    listed[g->prns[i]] = true;
  }
  const long long f_last = (long long)g->dopp_min_hz + (long long)(g->n_dopp - 1) * (long long)g->dopp_step_hz;
  if (f_last > 2147483647ll)
    return fail(ctx, GPSX_EINVAL, "a Doppler bin lies outside int32");
  if (n_blocks < 1 || (long long)(g->n_search - 1) * g->search_stride_blocks + (long long)cfg->n_coh * cfg->n_seg > n_blocks)
    return fail(ctx, GPSX_EINVAL, "not enough blocks for the searches");
  if (!host && ((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(rep)) & 15u) != 0)
    return fail(ctx, GPSX_EINVAL, "d_pred and d_rep must be 16-byte aligned");
  size_t peak_bytes = 0, pred_bytes = 0, rep_bytes = 0, if_bytes = 0;
  if (records_overflow((size_t)g->n_search * (size_t)g->n_prn, g->n_dopp, sizeof(gpsx_peak_t), &peak_bytes) ||
      records_overflow((size_t)g->n_search, g->n_prn, sizeof(gpsx_wpred_t), &pred_bytes) ||
      records_overflow((size_t)g->n_search, g->n_prn, sizeof(gpsx_acq_window_rep_t), &rep_bytes) ||
      records_overflow((size_t)n_blocks, 1, (size_t)GPSX_BYTES_PER_MS_2BIT, &if_bytes))
    return fail(ctx, GPSX_EINVAL, "n_search x n_prn x n_dopp records overflow a size");
  const size_t n_rows = (size_t)g->n_search * (size_t)g->n_prn;
  const gpsx_wpred_t *d_pred = pred;
  const uint8_t *d_if = static_cast<const uint8_t *>(if_blocks_2bit);
  gpsx_peak_t *d_peaks = peaks;
  gpsx_acq_window_rep_t *d_rep = rep;
  if (host) {
    if (int rc = arena_reset(ctx, arena_size(pred_bytes) + arena_size(if_bytes) + arena_size(peak_bytes) + (rep ? arena_size(rep_bytes) : 0))) return rc;
    if (int rc = stage_in(ctx, pred, n_rows, &d_pred)) return rc;
    if (int rc = stage_in(ctx, static_cast<const uint8_t *>(if_blocks_2bit), if_bytes, &d_if)) return rc;
    d_peaks = arena_take<gpsx_peak_t>(ctx, peak_bytes / sizeof(gpsx_peak_t));
    if (rep)
      d_rep = arena_take<gpsx_acq_window_rep_t>(ctx, n_rows);
  }
  return launch_and_report(
      ctx, host, "k_acq_win", "k_acq_win raised the bad-state flag, which it never does",
      [&](uint32_t *) {
        launch_acq_win(ctx->stream, *cfg, d_if, g->n_search, g->search_stride_blocks, g->n_prn, g->prns, ctx->d_chips_all, ctx->if_hz, g->dopp_min_hz,
                       g->dopp_step_hz, g->n_dopp, g->weights == GPSX_WEIGHTS_SIGN_MAGNITUDE, d_pred, d_peaks, d_rep);
      },
      [&]() -> int {
        HIPCHK(ctx, hipMemcpyAsync(peaks, d_peaks, peak_bytes, hipMemcpyDeviceToHost, ctx->stream));
        if (rep)
          HIPCHK(ctx, hipMemcpyAsync(rep, d_rep, rep_bytes, hipMemcpyDeviceToHost, ctx->stream));
        return GPSX_OK;
      });
}

}  // namespace

extern "C" {

int gpsx_acq_window_weighted_dev(gpsx_ctx *ctx, const gpsx_acq_weighted_t *g, const gpsx_acq_window_t *cfg, const gpsx_wpred_t *d_pred,
                                 const void *d_if_blocks_2bit, int n_blocks, gpsx_peak_t *d_peaks, gpsx_acq_window_rep_t *d_rep)
{
  return acq_window(ctx, g, cfg, d_pred, d_if_blocks_2bit, n_blocks, d_peaks, d_rep, false);
}

int gpsx_acq_window_weighted(gpsx_ctx *ctx, const gpsx_acq_weighted_t *g, const gpsx_acq_window_t *cfg, const gpsx_wpred_t *pred,
                             const uint8_t *if_blocks_2bit, int n_blocks, gpsx_peak_t *peaks, gpsx_acq_window_rep_t *rep)
{
  return acq_window(ctx, g, cfg, pred, if_blocks_2bit, n_blocks, peaks, rep, true);
}

int gpsx_wtow_dev(gpsx_ctx *ctx, const gpsx_wtow_cfg_t *cfg, int n_rx, int n_prn, const uint8_t *prns, const gpsx_wpred_rx_t *d_pred_rx,
                  const gpsx_wpred_t *d_pred, gpsx_wsync_state_t *d_sync_state, gpsx_wobs_state_t *d_obs_state, gpsx_wobs_t *d_obs,
                  gpsx_wtow_t *d_tow, gpsx_wtow_rx_t *d_tow_rx)
{
  return wtow(ctx, cfg, n_rx, n_prn, prns, d_pred_rx, d_pred, d_sync_state, d_obs_state, d_obs, d_tow, d_tow_rx, false);
}

int gpsx_wtow(gpsx_ctx *ctx, const gpsx_wtow_cfg_t *cfg, int n_rx, int n_prn, const uint8_t *prns, const gpsx_wpred_rx_t *d_pred_rx,
              const gpsx_wpred_t *d_pred, gpsx_wsync_state_t *d_sync_state, gpsx_wobs_state_t *d_obs_state, gpsx_wobs_t *d_obs, gpsx_wtow_t *tow,
              gpsx_wtow_rx_t *tow_rx)
{
  return wtow(ctx, cfg, n_rx, n_prn, prns, d_pred_rx, d_pred, d_sync_state, d_obs_state, d_obs, tow, tow_rx, true);
}

int gpsx_walm_dev(gpsx_ctx *ctx, const gpsx_walm_cfg_t *cfg, const gpsx_wnav_word_t *d_words, int n_blocks, int n_rx,
                  gpsx_walm_slot_t *d_slot_state, gpsx_walm_bank_t *d_bank, gpsx_walm_rx_t *d_rx, gpsx_walm_sv_t *d_alm)
{
  return walm(ctx, cfg, d_words, n_blocks, n_rx, d_slot_state, d_bank, d_rx, d_alm, false);
}

int gpsx_walm(gpsx_ctx *ctx, const gpsx_walm_cfg_t *cfg, const gpsx_wnav_word_t *d_words, int n_blocks, int n_rx,
              gpsx_walm_slot_t *d_slot_state, gpsx_walm_bank_t *d_bank, gpsx_walm_rx_t *rx, gpsx_walm_sv_t *alm)
{
  return walm(ctx, cfg, d_words, n_blocks, n_rx, d_slot_state, d_bank, rx, alm, true);
}

int gpsx_wpred_dev(gpsx_ctx *ctx, const gpsx_wpred_cfg_t *cfg, int n_rx, int n_prn, const uint8_t *prns, const gpsx_wkf_state_t *d_kf_state,
                   const gpsx_weph_t *d_bank, gpsx_wsync_state_t *d_sync_state, gpsx_wlock_state_t *d_lock_state, gpsx_wnav_state_t *d_nav_state,
                   gpsx_wobs_state_t *d_obs_state, gpsx_weph_state_t *d_eph_state, gpsx_wpred_rx_t *d_rx, gpsx_wpred_t *d_pred)
{
  return wpred(ctx, cfg, n_rx, n_prn, prns, d_kf_state, d_bank, d_sync_state, d_lock_state, d_nav_state, d_obs_state, d_eph_state, d_rx, d_pred, false);
}

int gpsx_wpred(gpsx_ctx *ctx, const gpsx_wpred_cfg_t *cfg, int n_rx, int n_prn, const uint8_t *prns, const gpsx_wkf_state_t *d_kf_state,
               const gpsx_weph_t *d_bank, gpsx_wsync_state_t *d_sync_state, gpsx_wlock_state_t *d_lock_state, gpsx_wnav_state_t *d_nav_state,
               gpsx_wobs_state_t *d_obs_state, gpsx_weph_state_t *d_eph_state, gpsx_wpred_rx_t *rx, gpsx_wpred_t *pred)
{
  return wpred(ctx, cfg, n_rx, n_prn, prns, d_kf_state, d_bank, d_sync_state, d_lock_state, d_nav_state, d_obs_state, d_eph_state, rx, pred, true);
}

int gpsx_wsnap_dev(gpsx_ctx *ctx, const gpsx_wsnap_cfg_t *cfg, const gpsx_acq_weighted_t *g, const gpsx_peak_t *d_peaks, const gpsx_weph_t *d_bank,
                   int bank_stride, const gpsx_wsnap_prior_t *d_prior, gpsx_wsnap_t *d_snap, gpsx_wsnap_sv_t *d_sv)
{
  return wsnap(ctx, cfg, g, d_peaks, d_bank, bank_stride, d_prior, d_snap, d_sv, false);
}

int gpsx_wsnap(gpsx_ctx *ctx, const gpsx_wsnap_cfg_t *cfg, const gpsx_acq_weighted_t *g, const gpsx_peak_t *peaks, const gpsx_weph_t *d_bank,
               int bank_stride, const gpsx_wsnap_prior_t *prior, gpsx_wsnap_t *snap, gpsx_wsnap_sv_t *sv)
{
  return wsnap(ctx, cfg, g, peaks, d_bank, bank_stride, prior, snap, sv, true);
}

// host only: a snapshot with FIX as the gpsx_wfix_t record gpsx_wkf's INIT reads
int gpsx_wsnap_to_fix(const gpsx_wsnap_t *in, gpsx_wfix_t *out)
{
  if (!in || !out || in->flags != GPSX_WSNAP_FIX)
    return GPSX_EINVAL;
  gpsx_wfix_t f;
  std::memset(&f, 0, sizeof f);
  f.flags = GPSX_WFIX_FIX;
  f.n_used = in->n_used;
  f.n_iter = in->n_iter;
  f.ref_slot = in->ref;
  f.used_mask = in->used_mask;
  f.dtr_s = in->b_m / 299792458.0;
  f.rx_tow_s = in->tow_s + f.dtr_s;
  f.week = in->week;
  for (int i = 0; i < 3; i++) {
    f.rr[i] = in->rr[i];
    f.geo[i] = in->geo[i];
  }
  for (int i = 0; i < 6; i++)
    f.qr[i] = in->qr[i];
  f.resid_rms_m = in->resid_rms_m;
  *out = f;
  return GPSX_OK;
}

int gpsx_wbank_dev(gpsx_ctx *ctx, const gpsx_wbank_cfg_t *cfg, int n_rx, int n_prn, const uint8_t *prns, const gpsx_wsync_state_t *d_sync_state,
                   const gpsx_weph_t *d_eph, gpsx_weph_t *d_bank, gpsx_weph_t *d_eph_out, gpsx_wbank_t *d_rep)
{
  return wbank(ctx, cfg, n_rx, n_prn, prns, d_sync_state, d_eph, d_bank, d_eph_out, d_rep, false);
}

int gpsx_wbank(gpsx_ctx *ctx, const gpsx_wbank_cfg_t *cfg, int n_rx, int n_prn, const uint8_t *prns, const gpsx_wsync_state_t *d_sync_state,
               const gpsx_weph_t *eph, gpsx_weph_t *d_bank, gpsx_weph_t *eph_out, gpsx_wbank_t *rep)
{
  return wbank(ctx, cfg, n_rx, n_prn, prns, d_sync_state, eph, d_bank, eph_out, rep, true);
}

int gpsx_wacq_dev(gpsx_ctx *ctx, const gpsx_wacq_cfg_t *cfg, const gpsx_acq_weighted_t *g, const gpsx_peak_t *d_peaks,
                  gpsx_wsync_state_t *d_sync_state, gpsx_wlock_state_t *d_lock_state, gpsx_wnav_state_t *d_nav_state,
                  gpsx_wobs_state_t *d_obs_state, gpsx_weph_state_t *d_eph_state, gpsx_wacq_t *d_acq, gpsx_wacq_det_t *d_det)
{
  return wacq(ctx, cfg, g, d_peaks, d_sync_state, d_lock_state, d_nav_state, d_obs_state, d_eph_state, d_acq, d_det, false);
}

int gpsx_wacq(gpsx_ctx *ctx, const gpsx_wacq_cfg_t *cfg, const gpsx_acq_weighted_t *g, const gpsx_peak_t *peaks,
              gpsx_wsync_state_t *d_sync_state, gpsx_wlock_state_t *d_lock_state, gpsx_wnav_state_t *d_nav_state,
              gpsx_wobs_state_t *d_obs_state, gpsx_weph_state_t *d_eph_state, gpsx_wacq_t *acq, gpsx_wacq_det_t *det)
{
  return wacq(ctx, cfg, g, peaks, d_sync_state, d_lock_state, d_nav_state, d_obs_state, d_eph_state, acq, det, true);
}

int gpsx_wkf_dev(gpsx_ctx *ctx, const gpsx_wkf_cfg_t *cfg, const gpsx_wobs_t *d_obs, const gpsx_weph_t *d_eph, const gpsx_wlock_t *d_lock,
                 const gpsx_wfix_t *d_fix, const gpsx_wvel_t *d_vel, int n_rx, int n_blocks, gpsx_wkf_state_t *d_state, gpsx_wkf_t *d_kf)
{
  return wkf(ctx, cfg, d_obs, d_eph, d_lock, d_fix, d_vel, n_rx, n_blocks, d_state, d_kf, false);
}

int gpsx_wkf(gpsx_ctx *ctx, const gpsx_wkf_cfg_t *cfg, const gpsx_wobs_t *obs, const gpsx_weph_t *eph, const gpsx_wlock_t *lock,
             const gpsx_wfix_t *fix, const gpsx_wvel_t *vel, int n_rx, int n_blocks, gpsx_wkf_state_t *d_state, gpsx_wkf_t *kf)
{
  return wkf(ctx, cfg, obs, eph, lock, fix, vel, n_rx, n_blocks, d_state, kf, true);
}

int gpsx_wvel_dev(gpsx_ctx *ctx, const gpsx_wvel_cfg_t *cfg, const gpsx_wobs_t *d_obs, const gpsx_weph_t *d_eph, const gpsx_wlock_t *d_lock,
                  const gpsx_wfix_t *d_fix, int n_rx, gpsx_wvel_t *d_vel)
{
  return wvel(ctx, cfg, d_obs, d_eph, d_lock, d_fix, n_rx, d_vel, false);
}

int gpsx_wvel(gpsx_ctx *ctx, const gpsx_wvel_cfg_t *cfg, const gpsx_wobs_t *obs, const gpsx_weph_t *eph, const gpsx_wlock_t *lock,
              const gpsx_wfix_t *fix, int n_rx, gpsx_wvel_t *vel)
{
  return wvel(ctx, cfg, obs, eph, lock, fix, n_rx, vel, true);
}

int gpsx_wfde_dev(gpsx_ctx *ctx, const gpsx_wfde_cfg_t *cfg, const gpsx_wobs_t *d_obs, const gpsx_weph_t *d_eph, const gpsx_wlock_t *d_lock,
                  const gpsx_wfix_t *d_prev, int n_rx, gpsx_wfix_t *d_fix, gpsx_wfde_t *d_fde, double *d_pr_m)
{
  return wfde(ctx, cfg, d_obs, d_eph, d_lock, d_prev, n_rx, d_fix, d_fde, d_pr_m, false);
}

int gpsx_wfde(gpsx_ctx *ctx, const gpsx_wfde_cfg_t *cfg, const gpsx_wobs_t *obs, const gpsx_weph_t *eph, const gpsx_wlock_t *lock,
              const gpsx_wfix_t *prev, int n_rx, gpsx_wfix_t *fix, gpsx_wfde_t *fde, double *pr_m)
{
  return wfde(ctx, cfg, obs, eph, lock, prev, n_rx, fix, fde, pr_m, true);
}

int gpsx_wfix_dev(gpsx_ctx *ctx, const gpsx_wfix_cfg_t *cfg, const gpsx_wobs_t *d_obs, const gpsx_weph_t *d_eph, const gpsx_wlock_t *d_lock,
                  const gpsx_wfix_t *d_prev, int n_rx, gpsx_wfix_t *d_fix, double *d_pr_m)
{
  return wfix(ctx, cfg, d_obs, d_eph, d_lock, d_prev, n_rx, d_fix, d_pr_m, false);
}

int gpsx_wfix(gpsx_ctx *ctx, const gpsx_wfix_cfg_t *cfg, const gpsx_wobs_t *obs, const gpsx_weph_t *eph, const gpsx_wlock_t *lock,
              const gpsx_wfix_t *prev, int n_rx, gpsx_wfix_t *fix, double *pr_m)
{
  return wfix(ctx, cfg, obs, eph, lock, prev, n_rx, fix, pr_m, true);
}

int gpsx_track_epl_weighted_dev(gpsx_ctx *ctx, const gpsx_trk_weighted_t *cfg, const void *d_if_blocks_2bit, int n_blocks,
                                gpsx_trk_state_t *d_st, int n_ch, int32_t *d_iq_out)
{
  return track_epl_weighted(ctx, cfg, d_if_blocks_2bit, n_blocks, d_st, n_ch, d_iq_out, false);
}

int gpsx_track_epl_weighted(gpsx_ctx *ctx, const gpsx_trk_weighted_t *cfg, const uint8_t *if_blocks_2bit, int n_blocks,
                            gpsx_trk_state_t *st, int n_ch, int32_t *iq_out)
{
  return track_epl_weighted(ctx, cfg, if_blocks_2bit, n_blocks, st, n_ch, iq_out, true);
}

int gpsx_track_loop_weighted_dev(gpsx_ctx *ctx, const gpsx_wloop_cfg_t *cfg, const void *d_if_blocks_2bit, int n_blocks,
                                 gpsx_wloop_state_t *d_state, int n_ch, gpsx_wloop_rec_t *d_rec)
{
  return track_loop_weighted(ctx, cfg, false, nullptr, d_if_blocks_2bit, n_blocks, d_state, n_ch, d_rec, false);
}

int gpsx_track_loop_weighted(gpsx_ctx *ctx, const gpsx_wloop_cfg_t *cfg, const uint8_t *if_blocks_2bit, int n_blocks,
                             gpsx_wloop_state_t *d_state, int n_ch, gpsx_wloop_rec_t *rec)
{
  return track_loop_weighted(ctx, cfg, false, nullptr, if_blocks_2bit, n_blocks, d_state, n_ch, rec, true);
}

int gpsx_track_loop_weighted_aided_dev(gpsx_ctx *ctx, const gpsx_wloop_cfg_t *cfg, const gpsx_waid_t *aid, const void *d_if_blocks_2bit,
                                       int n_blocks, gpsx_wloop_state_t *d_state, int n_ch, gpsx_wloop_rec_t *d_rec)
{
  return track_loop_weighted(ctx, cfg, true, aid, d_if_blocks_2bit, n_blocks, d_state, n_ch, d_rec, false);
}

int gpsx_track_loop_weighted_aided(gpsx_ctx *ctx, const gpsx_wloop_cfg_t *cfg, const gpsx_waid_t *aid, const uint8_t *if_blocks_2bit,
                                   int n_blocks, gpsx_wloop_state_t *d_state, int n_ch, gpsx_wloop_rec_t *rec)
{
  return track_loop_weighted(ctx, cfg, true, aid, if_blocks_2bit, n_blocks, d_state, n_ch, rec, true);
}

int gpsx_track_loop_weighted_sync_dev(gpsx_ctx *ctx, const gpsx_wsync_cfg_t *cfg, const void *d_if_blocks_2bit, int n_blocks,
                                      gpsx_wsync_state_t *d_state, int n_ch, gpsx_wsync_rec_t *d_rec)
{
  return track_loop_weighted_sync(ctx, cfg, false, nullptr, d_if_blocks_2bit, n_blocks, d_state, n_ch, d_rec, false);
}

int gpsx_track_loop_weighted_sync(gpsx_ctx *ctx, const gpsx_wsync_cfg_t *cfg, const uint8_t *if_blocks_2bit, int n_blocks,
                                  gpsx_wsync_state_t *d_state, int n_ch, gpsx_wsync_rec_t *rec)
{
  return track_loop_weighted_sync(ctx, cfg, false, nullptr, if_blocks_2bit, n_blocks, d_state, n_ch, rec, true);
}

int gpsx_track_loop_weighted_sync_aided_dev(gpsx_ctx *ctx, const gpsx_wsync_cfg_t *cfg, const gpsx_waid_t *aid, const void *d_if_blocks_2bit,
                                            int n_blocks, gpsx_wsync_state_t *d_state, int n_ch, gpsx_wsync_rec_t *d_rec)
{
  return track_loop_weighted_sync(ctx, cfg, true, aid, d_if_blocks_2bit, n_blocks, d_state, n_ch, d_rec, false);
}

int gpsx_track_loop_weighted_sync_aided(gpsx_ctx *ctx, const gpsx_wsync_cfg_t *cfg, const gpsx_waid_t *aid, const uint8_t *if_blocks_2bit,
                                        int n_blocks, gpsx_wsync_state_t *d_state, int n_ch, gpsx_wsync_rec_t *rec)
{
  return track_loop_weighted_sync(ctx, cfg, true, aid, if_blocks_2bit, n_blocks, d_state, n_ch, rec, true);
}

int gpsx_track_loop_weighted_sync_multi_dev(gpsx_ctx *ctx, const gpsx_wsync_cfg_t *cfg, const gpsx_waid_t *aid, const gpsx_wmulti_t *rx,
                                            const void *d_if_blocks_2bit, int n_blocks, gpsx_wsync_state_t *d_state, gpsx_wsync_rec_t *d_rec)
{
  return track_loop_weighted_sync_multi(ctx, cfg, aid, rx, d_if_blocks_2bit, n_blocks, d_state, d_rec, false);
}

int gpsx_track_loop_weighted_sync_multi(gpsx_ctx *ctx, const gpsx_wsync_cfg_t *cfg, const gpsx_waid_t *aid, const gpsx_wmulti_t *rx,
                                        const uint8_t *if_blocks_2bit, int n_blocks, gpsx_wsync_state_t *d_state, gpsx_wsync_rec_t *rec)
{
  return track_loop_weighted_sync_multi(ctx, cfg, aid, rx, if_blocks_2bit, n_blocks, d_state, rec, true);
}

int gpsx_wnav_words_dev(gpsx_ctx *ctx, const gpsx_wnav_cfg_t *cfg, const gpsx_wsync_rec_t *d_rec, int n_slots, int n_blocks,
                        gpsx_wnav_state_t *d_state, int n_ch, gpsx_wnav_word_t *d_words)
{
  return wnav_words(ctx, cfg, d_rec, n_slots, n_blocks, d_state, n_ch, d_words, false);
}

int gpsx_wnav_words(gpsx_ctx *ctx, const gpsx_wnav_cfg_t *cfg, const gpsx_wsync_rec_t *d_rec, int n_slots, int n_blocks,
                    gpsx_wnav_state_t *d_state, int n_ch, gpsx_wnav_word_t *words)
{
  return wnav_words(ctx, cfg, d_rec, n_slots, n_blocks, d_state, n_ch, words, true);
}

int gpsx_wobs_dev(gpsx_ctx *ctx, const gpsx_wobs_cfg_t *cfg, const gpsx_wsync_rec_t *d_rec, int n_slots, int n_blocks,
                  const gpsx_wnav_word_t *d_words, gpsx_wobs_state_t *d_state, int n_ch, gpsx_wobs_t *d_obs)
{
  return wobs(ctx, cfg, d_rec, n_slots, n_blocks, d_words, d_state, n_ch, d_obs, false);
}

int gpsx_wobs(gpsx_ctx *ctx, const gpsx_wobs_cfg_t *cfg, const gpsx_wsync_rec_t *d_rec, int n_slots, int n_blocks,
              const gpsx_wnav_word_t *d_words, gpsx_wobs_state_t *d_state, int n_ch, gpsx_wobs_t *obs)
{
  return wobs(ctx, cfg, d_rec, n_slots, n_blocks, d_words, d_state, n_ch, obs, true);
}

int gpsx_weph_dev(gpsx_ctx *ctx, const gpsx_weph_cfg_t *cfg, const gpsx_wnav_word_t *d_words, int n_blocks, gpsx_weph_state_t *d_state,
                  int n_ch, gpsx_weph_t *d_eph)
{
  return weph(ctx, cfg, d_words, n_blocks, d_state, n_ch, d_eph, false);
}

int gpsx_weph(gpsx_ctx *ctx, const gpsx_weph_cfg_t *cfg, const gpsx_wnav_word_t *d_words, int n_blocks, gpsx_weph_state_t *d_state,
              int n_ch, gpsx_weph_t *eph)
{
  return weph(ctx, cfg, d_words, n_blocks, d_state, n_ch, eph, true);
}

int gpsx_wlock_dev(gpsx_ctx *ctx, const gpsx_wlock_cfg_t *cfg, const gpsx_wsync_rec_t *d_rec, int n_slots, int n_blocks,
                   gpsx_wlock_state_t *d_state, gpsx_wsync_state_t *d_sync_state, int n_ch, gpsx_wlock_t *d_lock)
{
  return wlock(ctx, cfg, d_rec, n_slots, n_blocks, d_state, d_sync_state, n_ch, d_lock, false);
}

int gpsx_wlock(gpsx_ctx *ctx, const gpsx_wlock_cfg_t *cfg, const gpsx_wsync_rec_t *d_rec, int n_slots, int n_blocks,
               gpsx_wlock_state_t *d_state, gpsx_wsync_state_t *d_sync_state, int n_ch, gpsx_wlock_t *lock)
{
  return wlock(ctx, cfg, d_rec, n_slots, n_blocks, d_state, d_sync_state, n_ch, lock, true);
}

int gpsx_wlock_cn0_dbhz(const gpsx_wlock_t *lock, int n, int n_coh_lock, float *cn0_dbhz)
{
  if (!lock || !cn0_dbhz || n < 1 || n_coh_lock < 1 || n_coh_lock > 20)
    return GPSX_EINVAL;
  const double t = n_coh_lock * 0.001;
  for (int i = 0; i < n; i++) {
    const bool have = (lock[i].flags & GPSX_WLOCK_EPOCH_LOCKED) && lock[i].last_k > 0 && lock[i].snr > 0.0f;
    cn0_dbhz[i] = have ? (float)(10.0 * std::log10((double)lock[i].snr / t)) : 0.0f;
  }
  return GPSX_OK;
}

int gpsx_wnav_subframe_image(const gpsx_wnav_word_t *ten, uint8_t image[38])
{
  if (!ten || !image)
    return GPSX_EINVAL;
  for (int w = 0; w < 10; w++)
    if (ten[w].index != w + 1 || (ten[w].flags & (GPSX_WNAV_WORD | GPSX_WNAV_OK)) != (GPSX_WNAV_WORD | GPSX_WNAV_OK))
      return GPSX_EINVAL;
  std::memset(image, 0, 38);
  for (int w = 0; w < 10; w++)
    for (int i = 0; i < 30; i++) {
      const int bit = 30 * w + i;
      image[bit >> 3] |= (uint8_t)(((ten[w].word >> (29 - i)) & 1u) << (bit & 7));
    }
  return GPSX_OK;
}

int gpsx_wobs_pseudoranges(const gpsx_wobs_t *obs, int n, double offset_ms, double *pr_m, double *rx_tow_s)
{
  if (!obs || !pr_m || !rx_tow_s || n < 1 || !(offset_ms - offset_ms == 0.0))   // (not finite: the difference is a NaN)
    return GPSX_EINVAL;
  constexpr int64_t kWeek = 604800000, kHalf = kWeek / 2;
  auto fold = [](int64_t d) { return ((d + kHalf) % kWeek + kWeek) % kWeek - kHalf; };   // into -302 400 000 .. 302 399 999
  int ref = -1, count = 0;
  for (int i = 0; i < n; i++) {
    pr_m[i] = 0.0;
    if (!(obs[i].flags & GPSX_WOBS_VALID))
      continue;
    count++;
    // later than the reference so far: more whole milliseconds, or a smaller code phase
    if (ref < 0 || (double)fold(obs[i].tx_ms - obs[ref].tx_ms) - ((double)obs[i].code_phase_fine - (double)obs[ref].code_phase_fine) / 16368.0 > 0.0)
      ref = i;
  }
  *rx_tow_s = 0.0;
  if (ref < 0)
    return 0;
  for (int i = 0; i < n; i++)
    if (obs[i].flags & GPSX_WOBS_VALID)
      pr_m[i] = 299792458e-3 * ((double)fold(obs[ref].tx_ms - obs[i].tx_ms) +
                                ((double)obs[i].code_phase_fine - (double)obs[ref].code_phase_fine) / 16368.0 + offset_ms);
  const double rx = ((double)obs[ref].tx_ms - (double)obs[ref].code_phase_fine / 16368.0 + offset_ms) / 1000.0;
  *rx_tow_s = rx >= 604800.0 ? rx - 604800.0 : (rx < 0.0 ? rx + 604800.0 : rx);
  return count;
}

int gpsx_wobs_pseudoranges_rx(const gpsx_wobs_t *obs, int n_rx, int ch_per_rx, double offset_ms, double *pr_m, double *rx_tow_s, int *n_valid)
{
  int n_ch = 0, total = 0;
  if (!obs || !pr_m || !rx_tow_s || !n_valid || n_rx < 1 || ch_per_rx < 1 || __builtin_mul_overflow(n_rx, ch_per_rx, &n_ch) ||
      !(offset_ms - offset_ms == 0.0))
    return GPSX_EINVAL;
  for (int r = 0; r < n_rx; r++) {   // (the arguments are good: a slice's call returns its count)
    const size_t at = (size_t)r * (size_t)ch_per_rx;
    n_valid[r] = gpsx_wobs_pseudoranges(obs + at, ch_per_rx, offset_ms, pr_m + at, rx_tow_s + r);
    total += n_valid[r];
  }
  return total;
}

}  // extern "C"
