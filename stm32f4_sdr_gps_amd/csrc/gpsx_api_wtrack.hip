// gpsx_api_wtrack.hip -- the C ABI of the weighted two-bit chain (include/gpsx.h).  Host code only, like gpsx_api.hip; it reads no lab
// knob, so lib/libgpsx_lab.so links this object as it is.  The stages in chain order, each a host call with its _dev twin:
//   gpsx_track_epl_weighted                               E/P/L correlators, K blocks per launch
//   gpsx_track_loop_weighted (_aided)                     the closed DLL / PLL / FLL loop
//   gpsx_track_loop_weighted_sync (_aided, _multi)        ... with bit sync and bit-aligned windows; many receivers per launch
//   gpsx_wnav_words, gpsx_wobs, gpsx_weph, gpsx_wlock     words, observables, ephemerides, lock monitor
//   gpsx_wfix, gpsx_wfde, gpsx_wvel, gpsx_wkf             position, fault exclusion, velocity, navigation filter
//   gpsx_wacq, gpsx_wbank, gpsx_wpred, gpsx_wtow          acquisition decisions, ephemeris bank, prediction, time-of-week aiding
//   gpsx_walm, gpsx_acq_window_weighted, gpsx_wsnap       almanac, the grid in a window around gpsx_wpred's records, snapshot fixes
// and the host helpers behind them (gpsx_weph_to_eph, gpsx_walm_to_eph and gpsx_walm_gps_minus_utc are gpsx_ephemeris.cpp's, beside
// the decoder they restate).
//
// A pair is ONE function with a `bool host`.  host: the capture and the results are host memory, staged through the arena; the call
// waits for its kernel and reports a bad channel itself (flag 0).  Otherwise (_dev) they are device memory, the call returns after
// the launch and the next gpsx_synchronize reports (flag 1).  The refusals come first, one line per clause; the first clause that
// fails decides the text.  Then one staging list says what a host call puts into the arena, copies in and copies back.
#include <hip/hip_runtime.h>

#include <cassert>
#include <cmath>
#include <cstring>
#include <initializer_list>

#include "gpsx_ctx.hpp"

using namespace gpsx;
using namespace gpsx_host;

namespace {

// ---- the clauses the refusals share, the overflow-checked count x n_ch x sizeof -------------------------------------------------------
// Each holds one text.  Where two stages word a condition differently the clause takes the text or stays in its stage.
bool is_finite(float v) { return __builtin_fabsf(v) <= 3.402823466e+38f; }   // (a NaN fails it)
bool is_finite(double v) { return v - v == 0.0; }                            // (not finite: the difference is a NaN)

int check_weights_spacing(gpsx_ctx *ctx, int weights, int spacing)
{
  if (weights != GPSX_WEIGHTS_SIGN_ONLY && weights != GPSX_WEIGHTS_SIGN_MAGNITUDE)
    return fail(ctx, GPSX_EINVAL, "unknown weights");
  return spacing < 1 || spacing > 15 ? fail(ctx, GPSX_EINVAL, "spacing must be 1..15 samples") : GPSX_OK;
}
int check_n_blocks(gpsx_ctx *ctx, int n) { return n < 1 || n > 4096 ? fail(ctx, GPSX_EINVAL, "n_blocks must be 1..4096") : GPSX_OK; }
int check_n_slots(gpsx_ctx *ctx, int n, int n_blocks) { return n < 1 || n > n_blocks ? fail(ctx, GPSX_EINVAL, "n_slots must be 1..n_blocks") : GPSX_OK; }
int check_n_ch(gpsx_ctx *ctx, int n) { return n < 1 ? fail(ctx, GPSX_EINVAL, "n_ch must be at least 1") : GPSX_OK; }
int check_ch_per_rx(gpsx_ctx *ctx, int n) { return n < 1 || n > 64 ? fail(ctx, GPSX_EINVAL, "ch_per_rx must be 1..64") : GPSX_OK; }
int check_n_rx(gpsx_ctx *ctx, int n) { return n < 1 || n > (1 << 20) ? fail(ctx, GPSX_EINVAL, "n_rx must be 1..1048576") : GPSX_OK; }
int check_n_prn(gpsx_ctx *ctx, int n) { return n < 1 || n > 64 ? fail(ctx, GPSX_EINVAL, "n_prn must be 1..64") : GPSX_OK; }
// (behind check_n_prn: n is 1..64)
int check_prn_list(gpsx_ctx *ctx, const uint8_t *prns, int n)
{
  bool listed[GPSX_MAX_PRN + 1] = {};
  for (int i = 0; i < n; i++) {
    if (prns[i] < 1 || prns[i] > GPSX_MAX_PRN)
      return fail(ctx, GPSX_EINVAL, "PRN outside 1..210");
    if (listed[prns[i]])
      return fail(ctx, GPSX_EINVAL, "a PRN is listed twice");
    listed[prns[i]] = true;
  }
  return GPSX_OK;
}
int check_grid_shape(gpsx_ctx *ctx, const gpsx_acq_weighted_t *g)
{
  if (g->n_search < 1 || g->n_search > (1 << 20))
    return fail(ctx, GPSX_EINVAL, "n_search must be 1..1048576");
  if (int rc = check_n_prn(ctx, g->n_prn)) return rc;
  if (g->n_dopp < 1 || g->n_dopp > (1 << 20))   // (the kernel counts bins in int32, four turns of 64 ahead)
    return fail(ctx, GPSX_EINVAL, "n_dopp must be 1..1048576");
  return GPSX_OK;
}
// (behind check_grid_shape: the product stays far inside a long long)
long long last_doppler_bin(const gpsx_acq_weighted_t *g) { return (long long)g->dopp_min_hz + (long long)(g->n_dopp - 1) * (long long)g->dopp_step_hz; }
// Both bounds for every caller.  acq_window has refused dopp_step_hz < 1 and n_dopp < 1 by then, so its last bin is at least
// dopp_min_hz, an int32: the lower bound cannot trip there, as when that stage tested the upper bound alone.
int check_doppler_bins(gpsx_ctx *ctx, const gpsx_acq_weighted_t *g)
{
  const long long f_last = last_doppler_bin(g);
  return f_last < -2147483647ll - 1 || f_last > 2147483647ll ? fail(ctx, GPSX_EINVAL, "a Doppler bin lies outside int32") : GPSX_OK;
}
int check_gains(gpsx_ctx *ctx, std::initializer_list<float> gains)
{
  for (float g : gains)
    if (!is_finite(g))
      return fail(ctx, GPSX_EINVAL, "a loop gain is not finite");
  return GPSX_OK;
}
int check_code_per_hz(gpsx_ctx *ctx, float v)
{
  return !(__builtin_fabsf(v) <= 1.0f) ? fail(ctx, GPSX_EINVAL, "code_per_hz must be finite and -1..1") : GPSX_OK;   // (a NaN fails it)
}
// the aided calls' own clauses (aided: the call has an `aid` argument at all)
int check_aid(gpsx_ctx *ctx, const gpsx_waid_t *aid)
{
  if (int rc = check_code_per_hz(ctx, aid->code_per_hz)) return rc;
  return aid->reserved != 0 ? fail(ctx, GPSX_EINVAL, "reserved must be 0") : GPSX_OK;
}
int check_ion(gpsx_ctx *ctx, const double (&ion)[8])
{
  for (double v : ion)
    if (!is_finite(v))
      return fail(ctx, GPSX_EINVAL, "an ionosphere coefficient is not finite");
  return GPSX_OK;
}
int check_mps_per_hz(gpsx_ctx *ctx, double v)
{
  return !is_finite(v) || v == 0.0 ? fail(ctx, GPSX_EINVAL, "mps_per_hz must be finite and not 0") : GPSX_OK;
}
int check_el_min(gpsx_ctx *ctx, double v)
{
  return !(std::fabs(v) <= 1.5707963267948966) ? fail(ctx, GPSX_EINVAL, "el_min_rad must be finite and within -pi/2..pi/2") : GPSX_OK;   // (a NaN fails it)
}
int check_det_ratio(gpsx_ctx *ctx, int num, int den)
{
  return num < 1 || num > 1024 || den < 1 || den > 1024 || num < den ? fail(ctx, GPSX_EINVAL, "det_num and det_den must be 1..1024, det_num >= det_den")
                                                                     : GPSX_OK;
}
// lo: 4 (the fixes on observables) or 5 (the snapshot's fifth unknown)
int check_min_sats(gpsx_ctx *ctx, int v, int lo)
{
  if (v >= lo && v <= 64)
    return GPSX_OK;
  return lo == 4 ? fail(ctx, GPSX_EINVAL, "min_sats must be 4..64") : fail(ctx, GPSX_EINVAL, "min_sats must be 5..64");
}
int check_lead_blocks(gpsx_ctx *ctx, int n) { return n < 0 || n > 4096 ? fail(ctx, GPSX_EINVAL, "lead_blocks must be 0..4096") : GPSX_OK; }
// the eviction pair: the range, and (behind the stage's reserved words) the array it reads
int check_evict_after(gpsx_ctx *ctx, int n)
{
  return n < 0 || n > (1 << 30) ? fail(ctx, GPSX_EINVAL, "evict_after_blocks must be 0..1073741824") : GPSX_OK;
}
int check_evict_lock_state(gpsx_ctx *ctx, int n, const void *d_lock_state)
{
  return n != 0 && !d_lock_state ? fail(ctx, GPSX_EINVAL, "evict_after_blocks needs d_lock_state") : GPSX_OK;
}
// wfix's clauses on its config; wfde's begin with them, on its cfg->fix
int check_wfix_cfg(gpsx_ctx *ctx, const gpsx_wfix_cfg_t *cfg)
{
  if (!is_finite(cfg->offset_ms))
    return fail(ctx, GPSX_EINVAL, "offset_ms is not finite");
  if (int rc = check_ion(ctx, cfg->ion)) return rc;
  if (int rc = check_ch_per_rx(ctx, cfg->ch_per_rx)) return rc;
  if (int rc = check_min_sats(ctx, cfg->min_sats, 4)) return rc;
  if (cfg->reserved0 != 0 || cfg->reserved1 != 0 || cfg->reserved2 != 0 || cfg->reserved3 != 0)
    return fail(ctx, GPSX_EINVAL, "reserved must be 0");
  return GPSX_OK;
}
// every pointer a multiple of `bytes` (a power of two; a null one passes).  Host memory is staged, so a clause on arrays that are the
// caller's in the host call stands behind `if (!host)`.
int check_aligned(gpsx_ctx *ctx, std::initializer_list<const void *> pointers, unsigned bytes, const char *text)
{
  uintptr_t low = 0;
  for (const void *p : pointers)
    low |= reinterpret_cast<uintptr_t>(p);
  return (low & (bytes - 1u)) != 0 ? fail(ctx, GPSX_EINVAL, text) : GPSX_OK;
}
// the first n_lead spans against every span behind them; a null span is skipped.  (Host and device addresses share one space here:
// one list serves both variants.)
struct Span { const void *p; size_t n; };
int check_no_overlap(gpsx_ctx *ctx, std::initializer_list<Span> spans, int n_lead, const char *text)
{
  const Span *s = spans.begin();
  for (int a = 0; a < n_lead; a++)
    for (int b = a + 1; b < (int)spans.size(); b++) {
      const uintptr_t pa = reinterpret_cast<uintptr_t>(s[a].p), pb = reinterpret_cast<uintptr_t>(s[b].p);
      if (pa && pb && pa < pb + s[b].n && pb < pa + s[a].n)
        return fail(ctx, GPSX_EINVAL, text);
    }
  return GPSX_OK;
}
bool records_overflow(size_t count, int n_ch, size_t each, size_t *bytes)
{
  size_t recs = 0;   // (true: the product overflows a size)
  return __builtin_mul_overflow(count, (size_t)n_ch, &recs) || __builtin_mul_overflow(recs, each, bytes);
}

// ---- what a host call stages: one list per call ----------------------------------------------------------------------------------------
// A stage adds every array that is host memory in its host call, in arena order, with the device-pointer variable its launch reads
// (which holds the caller's pointer: a _dev call launches with it as it is).  `stage`, called only when host, sizes the arena from the
// list, takes each entry's room in list order (256-byte rounding; `pad` bytes of slack behind the array), points the variable at it
// and enqueues the copies in; launch_and_report enqueues the copies out from the same list.  An array that is NULL adds nothing and
// its variable stays null.
enum { COPY_NONE = 0, COPY_IN = 1, COPY_OUT = 2, COPY_BOTH = 3 };
struct Staging {
  struct Entry {
    void *d_var;   // the address of the launch's pointer variable
    void *host;
    char *dev;
    size_t bytes, pad;
    int copy;
  };
  Entry e[8];
  int n = 0;
  template <typename T>
  void add(T **d_var, const void *host, size_t bytes, int copy, size_t pad = 0)
  {
    assert(n < 8);
    if (host)
      e[n++] = {d_var, const_cast<void *>(host), nullptr, bytes, pad, copy};
  }
};

int stage(gpsx_ctx *ctx, Staging *s)
{
  size_t need = 0;
  for (int i = 0; i < s->n; i++)
    need += arena_size(s->e[i].bytes + s->e[i].pad);
  if (int rc = arena_reset(ctx, need)) return rc;
  for (int i = 0; i < s->n; i++) {
    Staging::Entry &e = s->e[i];
    e.dev = arena_take<char>(ctx, e.bytes + e.pad);
    if (e.copy & COPY_IN)
      HIPCHK(ctx, hipMemcpyAsync(e.dev, e.host, e.bytes, hipMemcpyHostToDevice, ctx->stream));
    std::memcpy(e.d_var, &e.dev, sizeof e.dev);   // (the variable is a T * of some record type: every object pointer is one address here)
  }
  return GPSX_OK;
}

// ---- the launch and what follows it -----------------------------------------------------------------------------------------------
// `launch(flag)` starts the kernel with the flag it raises for a bad channel; a host call then copies back what its list marks.
// `bad_state`: what a host call says when the flag was raised; nullptr: the tracking calls' PRN verdict.
template <typename Launch>
int launch_and_report(gpsx_ctx *ctx, bool host, const Staging &s, const char *kernel, const char *bad_state, Launch launch)
{
  if (host)
    ctx->h_bad_prn[0] = 0;   // (flag 0 is the waiting calls' own: each reads it before it returns, so nothing can be pending in it)
  launch(ctx->d_bad_prn + (host ? 0 : 1));
  LAUNCHCHK(ctx, kernel);
  ctx->last_kernel = kernel;
  if (!host)
    return GPSX_OK;
  for (int i = 0; i < s.n; i++)
    if (s.e[i].copy & COPY_OUT)
      HIPCHK(ctx, hipMemcpyAsync(s.e[i].host, s.e[i].dev, s.e[i].bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (!bad_state)
    return track_prn_verdict(ctx);
  if (*ctx->h_bad_prn == 0)
    return GPSX_OK;
  *ctx->h_bad_prn = 0;
  return fail(ctx, GPSX_EINVAL, bad_state);
}

// ---- E/P/L on weighted two-bit samples, K blocks per launch -------------------------------------------------------------------------
// (the three tracking calls leave two bytes of slack behind a staged capture)
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
  const uint8_t *d_blocks = static_cast<const uint8_t *>(if_blocks_2bit);
  gpsx_trk_state_t *d_st = st;
  int32_t *d_iq = iq_out;
  Staging s;
  s.add(&d_blocks, if_blocks_2bit, (size_t)n_blocks * GPSX_BYTES_PER_MS_2BIT, COPY_IN, 2);
  s.add(&d_st, st, (size_t)n_ch * sizeof(gpsx_trk_state_t), COPY_BOTH);
  s.add(&d_iq, iq_out, iq_bytes, COPY_OUT);
  if (host)
    if (int rc = stage(ctx, &s)) return rc;
  return launch_and_report(ctx, host, s, "k_track_epl_weighted", nullptr, [&](uint32_t *flag) {
    launch_track_epl_weighted(ctx->stream, d_blocks, n_blocks, ctx->if_hz, cfg->weights == GPSX_WEIGHTS_SIGN_MAGNITUDE, cfg->spacing, d_st, n_ch,
                              ctx->d_trk_rep, d_iq, flag);
  });
}

// ---- the closed loops: DLL / PLL / FLL, K blocks per launch; the second with a bit synchroniser and bit-aligned windows -------------
// A host call of either stages the capture and room for the records.  The state is device memory in both variants.
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
  Staging s;
  s.add(&d_if, if_blocks_2bit, (size_t)n_blocks * GPSX_BYTES_PER_MS_2BIT, COPY_IN, 2);
  s.add(&d_rec, rec, rec_bytes, COPY_OUT);
  if (host)
    if (int rc = stage(ctx, &s)) return rc;
  return launch_and_report(ctx, host, s, aided ? "k_track_waid_loop" : "k_track_wloop", nullptr, [&](uint32_t *flag) {
    if (aided)
      launch_track_loop_weighted_aided(ctx->stream, d_if, n_blocks, ctx->if_hz, *cfg, aid->code_per_hz, d_state, n_ch, ctx->d_trk_rep, d_rec, flag);
    else
      launch_track_loop_weighted(ctx->stream, d_if, n_blocks, ctx->if_hz, *cfg, d_state, n_ch, ctx->d_trk_rep, d_rec, flag);
  });
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
  Staging s;
  s.add(&d_if, if_blocks_2bit, (size_t)n_blocks * GPSX_BYTES_PER_MS_2BIT, COPY_IN, 2);
  s.add(&d_rec, rec, rec_bytes, COPY_OUT);
  if (host)
    if (int rc = stage(ctx, &s)) return rc;
  return launch_and_report(ctx, host, s, aided ? "k_track_waid_sync" : "k_track_wsync", nullptr, [&](uint32_t *flag) {
    if (aided)
      launch_track_loop_weighted_sync_aided(ctx->stream, d_if, n_blocks, ctx->if_hz, *cfg, aid->code_per_hz, d_state, n_ch, ctx->d_trk_rep, d_rec, flag);
    else
      launch_track_loop_weighted_sync(ctx->stream, d_if, n_blocks, ctx->if_hz, *cfg, d_state, n_ch, ctx->d_trk_rep, d_rec, flag);
  });
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
  if (int rc = check_n_rx(ctx, rx->n_rx)) return rc;
  if (int rc = check_ch_per_rx(ctx, rx->ch_per_rx)) return rc;
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
  // a host call's n_rx streams are rx_stride_blocks apart in host memory and packed n_blocks apart in the arena -- only the blocks
  // themselves are read: where the two differ the list only takes the room, and the strided copy is a line of its own
  const size_t rx_bytes = (size_t)n_blocks * GPSX_BYTES_PER_MS_2BIT;
  const bool strided = rx->n_rx > 1 && stride != n_blocks;
  Staging s;
  s.add(&d_if, if_blocks_2bit, (size_t)rx->n_rx * rx_bytes, strided ? COPY_NONE : COPY_IN, 2);
  s.add(&d_rec, rec, rec_bytes, COPY_OUT);
  if (host) {
    if (int rc = stage(ctx, &s)) return rc;
    if (strided)
      HIPCHK(ctx, hipMemcpy2DAsync(const_cast<uint8_t *>(d_if), rx_bytes, if_blocks_2bit, (size_t)stride * GPSX_BYTES_PER_MS_2BIT, rx_bytes,
                                   (size_t)rx->n_rx, hipMemcpyHostToDevice, ctx->stream));
    stride = n_blocks;
  }
  return launch_and_report(ctx, host, s, "k_track_wsync_multi", nullptr, [&](uint32_t *flag) {
    launch_track_loop_weighted_sync_multi(ctx->stream, d_if, n_blocks, ctx->if_hz, *cfg, aid ? aid->code_per_hz : 0.0f, rx->n_rx, rx->ch_per_rx, stride,
                                          d_state, ctx->d_trk_rep, d_rec, flag);
  });
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
  Staging s;
  s.add(&d_words, words, words_bytes, COPY_OUT);
  if (host)
    if (int rc = stage(ctx, &s)) return rc;
  return launch_and_report(ctx, host, s, "k_wnav_words", "a channel's frame state is out of range (its state is untouched, its slots are empty)",
                           [&](uint32_t *flag) { launch_wnav_words(ctx->stream, d_rec, n_slots, n_blocks, cfg->max_bad_words, d_state, n_ch, d_words, flag); });
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
  Staging s;
  s.add(&d_obs, obs, obs_bytes, COPY_OUT);
  if (host)
    if (int rc = stage(ctx, &s)) return rc;
  return launch_and_report(ctx, host, s, "k_wobs", "a channel's observable state is out of range (its state is untouched, its observable is zero)",
                           [&](uint32_t *flag) { launch_wobs(ctx->stream, d_rec, n_slots, n_blocks, cfg->edge_guard, d_words, d_state, n_ch, d_obs, flag); });
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
  if (!host)   // (k_weph stores the records 16 bytes at a time)
    if (int rc = check_aligned(ctx, {eph}, 16, "d_eph must be 16-byte aligned")) return rc;
  size_t bytes = 0, eph_bytes = 0;
  if (records_overflow((size_t)(n_blocks / 600 + 2), n_ch, sizeof(gpsx_wnav_word_t), &bytes) ||
      records_overflow(1, n_ch, sizeof(gpsx_weph_state_t), &bytes) || records_overflow(1, n_ch, sizeof(gpsx_weph_t), &eph_bytes))
    return fail(ctx, GPSX_EINVAL, "slots x n_ch records overflow a size");
  gpsx_weph_t *d_eph = eph;
  Staging s;
  s.add(&d_eph, eph, eph_bytes, COPY_OUT);
  if (host)
    if (int rc = stage(ctx, &s)) return rc;
  return launch_and_report(ctx, host, s, "k_weph", "a channel's ephemeris state is out of range (its state is untouched, its record is zero)",
                           [&](uint32_t *flag) { launch_weph(ctx->stream, d_words, n_blocks, d_state, n_ch, d_eph, flag); });
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
    if (!is_finite(t))
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
  Staging s;
  s.add(&d_lock, lock, lock_bytes, COPY_OUT);
  if (host)
    if (int rc = stage(ctx, &s)) return rc;
  return launch_and_report(ctx, host, s, "k_wlock", "a channel's lock state is out of range (its state is untouched, its record is zero)", [&](uint32_t *flag) {
    launch_wlock(ctx->stream, d_rec, n_slots, n_blocks, *cfg, d_state, cfg->rearm != 0 ? d_sync_state : nullptr, n_ch, d_lock, flag);
  });
}

// ---- the solvers at the chain's end (host: every array is host memory, staged through the arena; _dev: all device memory) ------------
// ---- the position fixes ---------------------------------------------------------------------------------------------------------------
int wfix(gpsx_ctx *ctx, const gpsx_wfix_cfg_t *cfg, const gpsx_wobs_t *obs, const gpsx_weph_t *eph, const gpsx_wlock_t *lock, const gpsx_wfix_t *prev,
         int n_rx, gpsx_wfix_t *fix, double *pr_m, bool host)
{
  if (int rc = use_device(ctx)) return rc;
  if (!cfg || !obs || !eph || !fix)
    return fail(ctx, GPSX_EINVAL, "null argument");
  if (int rc = check_wfix_cfg(ctx, cfg)) return rc;
  if (int rc = check_n_rx(ctx, n_rx)) return rc;
  if (!host)
    if (int rc = check_aligned(ctx, {fix}, 16, "d_fix must be 16-byte aligned")) return rc;
  size_t obs_bytes = 0, eph_bytes = 0, lock_bytes = 0, fix_bytes = 0, pr_bytes = 0;
  if (records_overflow((size_t)n_rx, cfg->ch_per_rx, sizeof(gpsx_wobs_t), &obs_bytes) ||
      records_overflow((size_t)n_rx, cfg->ch_per_rx, sizeof(gpsx_weph_t), &eph_bytes) ||
      records_overflow((size_t)n_rx, cfg->ch_per_rx, sizeof(gpsx_wlock_t), &lock_bytes) ||
      records_overflow((size_t)n_rx, cfg->ch_per_rx, sizeof(double), &pr_bytes) || records_overflow((size_t)n_rx, 1, sizeof(gpsx_wfix_t), &fix_bytes))
    return fail(ctx, GPSX_EINVAL, "n_rx x ch_per_rx records overflow a size");
  const gpsx_wobs_t *d_obs = obs;
  const gpsx_weph_t *d_eph = eph;
  const gpsx_wlock_t *d_lock = lock;
  const gpsx_wfix_t *d_prev = prev;
  gpsx_wfix_t *d_fix = fix;
  double *d_pr = pr_m;
  Staging s;
  s.add(&d_obs, obs, obs_bytes, COPY_IN);
  s.add(&d_eph, eph, eph_bytes, COPY_IN);
  s.add(&d_lock, lock, lock_bytes, COPY_IN);
  s.add(&d_prev, prev, fix_bytes, COPY_IN);
  s.add(&d_fix, fix, fix_bytes, COPY_OUT);
  s.add(&d_pr, pr_m, pr_bytes, COPY_OUT);
  if (host)
    if (int rc = stage(ctx, &s)) return rc;
  return launch_and_report(ctx, host, s, "k_wfix", "k_wfix raised the bad-state flag, which it never does",
                           [&](uint32_t *) { launch_wfix(ctx->stream, *cfg, d_obs, d_eph, d_lock, d_prev, n_rx, d_fix, d_pr); });
}

// ---- the position fixes with millisecond repair and fault exclusion -------------------------------------------------------------------
int wfde(gpsx_ctx *ctx, const gpsx_wfde_cfg_t *fc, const gpsx_wobs_t *obs, const gpsx_weph_t *eph, const gpsx_wlock_t *lock, const gpsx_wfix_t *prev,
         int n_rx, gpsx_wfix_t *fix, gpsx_wfde_t *fde, double *pr_m, bool host)
{
  if (int rc = use_device(ctx)) return rc;
  if (!fc || !obs || !eph || !fix || !fde)
    return fail(ctx, GPSX_EINVAL, "null argument");
  const gpsx_wfix_cfg_t *cfg = &fc->fix;
  if (int rc = check_wfix_cfg(ctx, cfg)) return rc;
  if (!(fc->z_global >= 0.0 && fc->z_global <= 10.0))   // (a NaN fails it)
    return fail(ctx, GPSX_EINVAL, "z_global must be finite and 0..10");
  if (fc->max_excl < 0 || fc->max_excl > 8)
    return fail(ctx, GPSX_EINVAL, "max_excl must be 0..8");
  if (fc->repair != 0 && fc->repair != 1)
    return fail(ctx, GPSX_EINVAL, "repair must be 0 or 1");
  for (int32_t v : fc->reserved)
    if (v != 0)
      return fail(ctx, GPSX_EINVAL, "reserved must be 0");
  if (int rc = check_n_rx(ctx, n_rx)) return rc;
  if (!host) {
    if (int rc = check_aligned(ctx, {fix}, 16, "d_fix must be 16-byte aligned")) return rc;
    if (int rc = check_aligned(ctx, {fde}, 16, "d_fde must be 16-byte aligned")) return rc;
  }
  size_t obs_bytes = 0, eph_bytes = 0, lock_bytes = 0, fix_bytes = 0, fde_bytes = 0, pr_bytes = 0;
  if (records_overflow((size_t)n_rx, cfg->ch_per_rx, sizeof(gpsx_wobs_t), &obs_bytes) ||
      records_overflow((size_t)n_rx, cfg->ch_per_rx, sizeof(gpsx_weph_t), &eph_bytes) ||
      records_overflow((size_t)n_rx, cfg->ch_per_rx, sizeof(gpsx_wlock_t), &lock_bytes) ||
      records_overflow((size_t)n_rx, cfg->ch_per_rx, sizeof(double), &pr_bytes) || records_overflow((size_t)n_rx, 1, sizeof(gpsx_wfix_t), &fix_bytes) ||
      records_overflow((size_t)n_rx, 1, sizeof(gpsx_wfde_t), &fde_bytes))
    return fail(ctx, GPSX_EINVAL, "n_rx x ch_per_rx records overflow a size");
  const gpsx_wobs_t *d_obs = obs;
  const gpsx_weph_t *d_eph = eph;
  const gpsx_wlock_t *d_lock = lock;
  const gpsx_wfix_t *d_prev = prev;
  gpsx_wfix_t *d_fix = fix;
  gpsx_wfde_t *d_fde = fde;
  double *d_pr = pr_m;
  Staging s;
  s.add(&d_obs, obs, obs_bytes, COPY_IN);
  s.add(&d_eph, eph, eph_bytes, COPY_IN);
  s.add(&d_lock, lock, lock_bytes, COPY_IN);
  s.add(&d_prev, prev, fix_bytes, COPY_IN);
  s.add(&d_fix, fix, fix_bytes, COPY_OUT);
  s.add(&d_fde, fde, fde_bytes, COPY_OUT);
  s.add(&d_pr, pr_m, pr_bytes, COPY_OUT);
  if (host)
    if (int rc = stage(ctx, &s)) return rc;
  return launch_and_report(ctx, host, s, "k_wfde", "k_wfde raised the bad-state flag, which it never does",
                           [&](uint32_t *) { launch_wfde(ctx->stream, *fc, d_obs, d_eph, d_lock, d_prev, n_rx, d_fix, d_fde, d_pr); });
}

// ---- the velocity fixes behind either (the position records are an input here) -------------------------------------------------------
int wvel(gpsx_ctx *ctx, const gpsx_wvel_cfg_t *cfg, const gpsx_wobs_t *obs, const gpsx_weph_t *eph, const gpsx_wlock_t *lock, const gpsx_wfix_t *fix,
         int n_rx, gpsx_wvel_t *vel, bool host)
{
  if (int rc = use_device(ctx)) return rc;
  if (!cfg || !obs || !eph || !fix || !vel)
    return fail(ctx, GPSX_EINVAL, "null argument");
  if (int rc = check_mps_per_hz(ctx, cfg->mps_per_hz)) return rc;
  if (int rc = check_ch_per_rx(ctx, cfg->ch_per_rx)) return rc;
  if (int rc = check_min_sats(ctx, cfg->min_sats, 4)) return rc;
  for (int32_t v : cfg->reserved)
    if (v != 0)
      return fail(ctx, GPSX_EINVAL, "reserved must be 0");
  if (int rc = check_n_rx(ctx, n_rx)) return rc;
  if (!host)
    if (int rc = check_aligned(ctx, {vel}, 16, "d_vel must be 16-byte aligned")) return rc;
  size_t obs_bytes = 0, eph_bytes = 0, lock_bytes = 0, fix_bytes = 0, vel_bytes = 0;
  if (records_overflow((size_t)n_rx, cfg->ch_per_rx, sizeof(gpsx_wobs_t), &obs_bytes) ||
      records_overflow((size_t)n_rx, cfg->ch_per_rx, sizeof(gpsx_weph_t), &eph_bytes) ||
      records_overflow((size_t)n_rx, cfg->ch_per_rx, sizeof(gpsx_wlock_t), &lock_bytes) ||
      records_overflow((size_t)n_rx, 1, sizeof(gpsx_wfix_t), &fix_bytes) || records_overflow((size_t)n_rx, 1, sizeof(gpsx_wvel_t), &vel_bytes))
    return fail(ctx, GPSX_EINVAL, "n_rx x ch_per_rx records overflow a size");
  const gpsx_wobs_t *d_obs = obs;
  const gpsx_weph_t *d_eph = eph;
  const gpsx_wlock_t *d_lock = lock;
  const gpsx_wfix_t *d_fix = fix;
  gpsx_wvel_t *d_vel = vel;
  Staging s;
  s.add(&d_obs, obs, obs_bytes, COPY_IN);
  s.add(&d_eph, eph, eph_bytes, COPY_IN);
  s.add(&d_lock, lock, lock_bytes, COPY_IN);
  s.add(&d_fix, fix, fix_bytes, COPY_IN);
  s.add(&d_vel, vel, vel_bytes, COPY_OUT);
  if (host)
    if (int rc = stage(ctx, &s)) return rc;
  return launch_and_report(ctx, host, s, "k_wvel", "k_wvel raised the bad-state flag, which it never does",
                           [&](uint32_t *) { launch_wvel(ctx->stream, *cfg, d_obs, d_eph, d_lock, d_fix, n_rx, d_vel); });
}

// ---- the navigation filter behind them (the state is device memory in both variants) --------------------------------------------------
int wkf(gpsx_ctx *ctx, const gpsx_wkf_cfg_t *cfg, const gpsx_wobs_t *obs, const gpsx_weph_t *eph, const gpsx_wlock_t *lock, const gpsx_wfix_t *fix,
        const gpsx_wvel_t *vel, int n_rx, int n_blocks, gpsx_wkf_state_t *d_state, gpsx_wkf_t *kf, bool host)
{
  if (int rc = use_device(ctx)) return rc;
  if (!cfg || !obs || !eph || !d_state || !kf)
    return fail(ctx, GPSX_EINVAL, "null argument");
  if (int rc = check_ch_per_rx(ctx, cfg->ch_per_rx)) return rc;
  if (int rc = check_n_rx(ctx, n_rx)) return rc;
  if (int rc = check_n_blocks(ctx, n_blocks)) return rc;
  if (cfg->max_coast < 0 || cfg->max_coast > 1000000)
    return fail(ctx, GPSX_EINVAL, "max_coast must be 0..1000000");
  if (!(cfg->gate > 0.0 && cfg->gate <= 100.0))   // (a NaN fails it)
    return fail(ctx, GPSX_EINVAL, "gate must be finite, above 0 and at most 100");
  if (!is_finite(cfg->sig_dop_mps) || !(cfg->sig_dop_mps > 0.0))
    return fail(ctx, GPSX_EINVAL, "sig_dop_mps must be finite and above 0");
  for (double v : {cfg->sig_pr_m, cfg->q_acc, cfg->q_clk_f, cfg->q_clk_g, cfg->p0_pos, cfg->p0_clk, cfg->p0_vel, cfg->p0_drift})
    if (!is_finite(v) || v < 0.0)
      return fail(ctx, GPSX_EINVAL, "sig_pr_m, q_* and p0_* must be finite and not negative");
  for (double v : {cfg->p0_pos, cfg->p0_clk, cfg->p0_vel, cfg->p0_drift})
    if (v == 0.0)
      return fail(ctx, GPSX_EINVAL, "p0_* must not be 0");
  if (int rc = check_mps_per_hz(ctx, cfg->mps_per_hz)) return rc;
  if (int rc = check_ion(ctx, cfg->ion)) return rc;
  for (int32_t v : cfg->reserved)
    if (v != 0)
      return fail(ctx, GPSX_EINVAL, "reserved must be 0");
  if (int rc = check_aligned(ctx, {d_state}, 16, "d_state must be 16-byte aligned")) return rc;
  if (!host)
    if (int rc = check_aligned(ctx, {kf}, 16, "d_kf must be 16-byte aligned")) return rc;
  size_t obs_bytes = 0, eph_bytes = 0, lock_bytes = 0, fix_bytes = 0, vel_bytes = 0, kf_bytes = 0, bytes = 0;
  if (records_overflow((size_t)n_rx, cfg->ch_per_rx, sizeof(gpsx_wobs_t), &obs_bytes) ||
      records_overflow((size_t)n_rx, cfg->ch_per_rx, sizeof(gpsx_weph_t), &eph_bytes) ||
      records_overflow((size_t)n_rx, cfg->ch_per_rx, sizeof(gpsx_wlock_t), &lock_bytes) ||
      records_overflow((size_t)n_rx, 1, sizeof(gpsx_wfix_t), &fix_bytes) || records_overflow((size_t)n_rx, 1, sizeof(gpsx_wvel_t), &vel_bytes) ||
      records_overflow((size_t)n_rx, 1, sizeof(gpsx_wkf_state_t), &bytes) || records_overflow((size_t)n_rx, 1, sizeof(gpsx_wkf_t), &kf_bytes))
    return fail(ctx, GPSX_EINVAL, "n_rx x ch_per_rx records overflow a size");
  const gpsx_wobs_t *d_obs = obs;
  const gpsx_weph_t *d_eph = eph;
  const gpsx_wlock_t *d_lock = lock;
  const gpsx_wfix_t *d_fix = fix;
  const gpsx_wvel_t *d_vel = vel;
  gpsx_wkf_t *d_kf = kf;
  Staging s;
  s.add(&d_obs, obs, obs_bytes, COPY_IN);
  s.add(&d_eph, eph, eph_bytes, COPY_IN);
  s.add(&d_lock, lock, lock_bytes, COPY_IN);
  s.add(&d_fix, fix, fix_bytes, COPY_IN);
  s.add(&d_vel, vel, vel_bytes, COPY_IN);
  s.add(&d_kf, kf, kf_bytes, COPY_OUT);
  if (host)
    if (int rc = stage(ctx, &s)) return rc;
  return launch_and_report(ctx, host, s, "k_wkf", "a receiver's filter state is out of range (its state is untouched, its record is zero but for the flag)",
                           [&](uint32_t *flag) { launch_wkf(ctx->stream, *cfg, d_obs, d_eph, d_lock, d_fix, d_vel, n_rx, n_blocks, d_state, d_kf, flag); });
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
  if (int rc = check_ch_per_rx(ctx, cfg->ch_per_rx)) return rc;
  if (int rc = check_det_ratio(ctx, cfg->det_num, cfg->det_den)) return rc;
  if (int rc = check_lead_blocks(ctx, cfg->lead_blocks)) return rc;
  if (int rc = check_code_per_hz(ctx, cfg->code_per_hz)) return rc;
  if (int rc = check_evict_after(ctx, cfg->evict_after_blocks)) return rc;
  if (cfg->reserved != 0)
    return fail(ctx, GPSX_EINVAL, "reserved must be 0");
  if (int rc = check_evict_lock_state(ctx, cfg->evict_after_blocks, d_lock_state)) return rc;
  if (int rc = check_grid_shape(ctx, g)) return rc;
  if (int rc = check_prn_list(ctx, g->prns, g->n_prn)) return rc;
  if (int rc = check_doppler_bins(ctx, g)) return rc;
  const long long f_first = g->dopp_min_hz, f_last = last_doppler_bin(g);
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
  Staging s;
  s.add(&d_peaks, peaks, peak_bytes, COPY_IN);
  s.add(&d_acq, acq, acq_bytes, COPY_OUT);
  s.add(&d_det, det, det_bytes, COPY_OUT);
  if (host)
    if (int rc = stage(ctx, &s)) return rc;
  return launch_and_report(ctx, host, s, "k_wacq", "k_wacq raised the bad-state flag, which it never does", [&](uint32_t *) {
    launch_wacq(ctx->stream, *cfg, g->n_search, g->n_prn, g->prns, g->dopp_min_hz, g->dopp_step_hz, g->n_dopp, d_peaks, d_sync_state, d_lock_state,
                d_nav_state, d_obs_state, d_eph_state, d_acq, d_det);
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
  if (int rc = check_ch_per_rx(ctx, cfg->ch_per_rx)) return rc;
  if (cfg->reserved[0] != 0 || cfg->reserved[1] != 0 || cfg->reserved[2] != 0)
    return fail(ctx, GPSX_EINVAL, "reserved must be 0");
  if (int rc = check_n_rx(ctx, n_rx)) return rc;
  if (int rc = check_n_prn(ctx, n_prn)) return rc;
  if (int rc = check_prn_list(ctx, prns, n_prn)) return rc;
  if (int rc = check_aligned(ctx, {d_sync_state}, 8, "d_sync_state must be 8-byte aligned")) return rc;
  if (int rc = check_aligned(ctx, {d_bank}, 16, "d_bank must be 16-byte aligned")) return rc;
  if (!host)
    if (int rc = check_aligned(ctx, {eph, eph_out, rep}, 16, "d_eph, d_eph_out and d_rep must be 16-byte aligned")) return rc;
  size_t sync_bytes = 0, eph_bytes = 0, bank_bytes = 0, rep_bytes = 0;
  if (records_overflow((size_t)n_rx, cfg->ch_per_rx, sizeof(gpsx_wsync_state_t), &sync_bytes) ||
      records_overflow((size_t)n_rx, cfg->ch_per_rx, sizeof(gpsx_weph_t), &eph_bytes) ||
      records_overflow((size_t)n_rx, n_prn, sizeof(gpsx_weph_t), &bank_bytes) || records_overflow((size_t)n_rx, 1, sizeof(gpsx_wbank_t), &rep_bytes))
    return fail(ctx, GPSX_EINVAL, "n_rx x n_prn records overflow a size");
  // in place (eph_out == eph): the one array is eph's span, and a host call runs on the staged copy of eph and copies that back
  const bool in_place = eph_out == eph;
  if (int rc = check_no_overlap(ctx, {{d_sync_state, sync_bytes}, {eph, eph_bytes}, {d_bank, bank_bytes}, {in_place ? nullptr : eph_out, eph_bytes}, {rep, rep_bytes}},
                                5, "two arrays overlap (only d_eph_out == d_eph may)"))
    return rc;
  const gpsx_weph_t *d_eph = eph;
  gpsx_weph_t *d_out = eph_out;
  gpsx_wbank_t *d_rep = rep;
  Staging s;
  s.add(&d_eph, eph, eph_bytes, in_place ? COPY_BOTH : COPY_IN);
  s.add(&d_out, in_place ? nullptr : eph_out, eph_bytes, COPY_OUT);
  s.add(&d_rep, rep, rep_bytes, COPY_OUT);
  if (host) {
    if (int rc = stage(ctx, &s)) return rc;
    if (in_place)
      d_out = const_cast<gpsx_weph_t *>(d_eph);
  }
  return launch_and_report(ctx, host, s, "k_wbank", "k_wbank raised the bad-state flag, which it never does",
                           [&](uint32_t *) { launch_wbank(ctx->stream, *cfg, n_rx, n_prn, prns, d_sync_state, d_eph, d_bank, d_out, d_rep); });
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
  if (int rc = check_ion(ctx, cfg->ion)) return rc;
  if (int rc = check_mps_per_hz(ctx, cfg->mps_per_hz)) return rc;
  if (int rc = check_el_min(ctx, cfg->el_min_rad)) return rc;
  if (!is_finite(cfg->max_sigma_m) || !(cfg->max_sigma_m > 0.0) || !is_finite(cfg->max_sigma_hz) || !(cfg->max_sigma_hz > 0.0))
    return fail(ctx, GPSX_EINVAL, "max_sigma_m and max_sigma_hz must be finite and above 0");
  if (int rc = check_ch_per_rx(ctx, cfg->ch_per_rx)) return rc;
  if (int rc = check_lead_blocks(ctx, cfg->lead_blocks)) return rc;
  if (int rc = check_evict_after(ctx, cfg->evict_after_blocks)) return rc;
  if (cfg->handover != 0 && cfg->handover != 1)
    return fail(ctx, GPSX_EINVAL, "handover must be 0 or 1");
  if (cfg->reserved[0] != 0 || cfg->reserved[1] != 0 || cfg->reserved[2] != 0 || cfg->reserved[3] != 0)
    return fail(ctx, GPSX_EINVAL, "reserved must be 0");
  if (int rc = check_evict_lock_state(ctx, cfg->evict_after_blocks, d_lock_state)) return rc;
  if (int rc = check_n_rx(ctx, n_rx)) return rc;
  if (int rc = check_n_prn(ctx, n_prn)) return rc;
  if (int rc = check_prn_list(ctx, prns, n_prn)) return rc;
  if (int rc = check_aligned(ctx, {d_kf_state, d_bank}, 16, "d_kf_state and d_bank must be 16-byte aligned")) return rc;
  if (!host)
    if (int rc = check_aligned(ctx, {rx, pred}, 16, "d_rx and d_pred must be 16-byte aligned")) return rc;
  size_t bytes = 0, rx_bytes = 0, pred_bytes = 0;
  if (records_overflow((size_t)n_rx, cfg->ch_per_rx, sizeof(gpsx_wsync_state_t), &bytes) ||
      records_overflow((size_t)n_rx, n_prn, sizeof(gpsx_weph_t), &bytes) || records_overflow((size_t)n_rx, n_prn, sizeof(gpsx_wpred_t), &pred_bytes) ||
      records_overflow((size_t)n_rx, 1, sizeof(gpsx_wpred_rx_t), &rx_bytes))
    return fail(ctx, GPSX_EINVAL, "n_rx x n_prn records overflow a size");
  gpsx_wpred_rx_t *d_rx = rx;
  gpsx_wpred_t *d_pred = pred;
  Staging s;
  s.add(&d_rx, rx, rx_bytes, COPY_OUT);
  s.add(&d_pred, pred, pred_bytes, COPY_OUT);
  if (host)
    if (int rc = stage(ctx, &s)) return rc;
  return launch_and_report(ctx, host, s, "k_wpred", "k_wpred raised the bad-state flag, which it never does", [&](uint32_t *) {
    launch_wpred(ctx->stream, *cfg, n_rx, n_prn, prns, d_kf_state, d_bank, d_sync_state, d_lock_state, d_nav_state, d_obs_state, d_eph_state, d_rx, d_pred);
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
  if (!is_finite(cfg->max_sigma_m) || !(cfg->max_sigma_m > 0.0))
    return fail(ctx, GPSX_EINVAL, "max_sigma_m must be finite and above 0");
  if (!(cfg->max_resid_samples > 0.0f && cfg->max_resid_samples <= 4092.0f))   // (a NaN fails it)
    return fail(ctx, GPSX_EINVAL, "max_resid_samples must be finite, above 0 and at most 4092");
  if (int rc = check_ch_per_rx(ctx, cfg->ch_per_rx)) return rc;
  if (cfg->max_age_blocks < 0 || cfg->max_age_blocks > 4096)
    return fail(ctx, GPSX_EINVAL, "max_age_blocks must be 0..4096");
  if ((cfg->resolve != 0 && cfg->resolve != 1) || (cfg->rearm != 0 && cfg->rearm != 1))
    return fail(ctx, GPSX_EINVAL, "resolve and rearm must be 0 or 1");
  if (cfg->reserved != 0)
    return fail(ctx, GPSX_EINVAL, "reserved must be 0");
  if (int rc = check_n_rx(ctx, n_rx)) return rc;
  if (int rc = check_n_prn(ctx, n_prn)) return rc;
  if (int rc = check_prn_list(ctx, prns, n_prn)) return rc;
  if (int rc = check_aligned(ctx, {d_pred_rx, d_pred, d_obs_state, d_obs}, 16, "d_pred_rx, d_pred, d_obs_state and d_obs must be 16-byte aligned")) return rc;
  if (int rc = check_aligned(ctx, {d_sync_state}, 8, "d_sync_state must be 8-byte aligned")) return rc;
  if (!host)
    if (int rc = check_aligned(ctx, {tow, tow_rx}, 16, "d_tow and d_tow_rx must be 16-byte aligned")) return rc;
  size_t rx_bytes = 0, pred_bytes = 0, sync_bytes = 0, st_bytes = 0, obs_bytes = 0, tow_bytes = 0, tow_rx_bytes = 0;
  if (records_overflow((size_t)n_rx, 1, sizeof(gpsx_wpred_rx_t), &rx_bytes) || records_overflow((size_t)n_rx, n_prn, sizeof(gpsx_wpred_t), &pred_bytes) ||
      records_overflow((size_t)n_rx, cfg->ch_per_rx, sizeof(gpsx_wsync_state_t), &sync_bytes) ||
      records_overflow((size_t)n_rx, cfg->ch_per_rx, sizeof(gpsx_wobs_state_t), &st_bytes) ||
      records_overflow((size_t)n_rx, cfg->ch_per_rx, sizeof(gpsx_wobs_t), &obs_bytes) ||
      records_overflow((size_t)n_rx, cfg->ch_per_rx, sizeof(gpsx_wtow_t), &tow_bytes) || records_overflow((size_t)n_rx, 1, sizeof(gpsx_wtow_rx_t), &tow_rx_bytes))
    return fail(ctx, GPSX_EINVAL, "n_rx x n_prn records overflow a size");
  // (the two outputs against each other and against the five arrays the kernel reads or updates)
  if (int rc = check_no_overlap(ctx, {{tow, tow_bytes}, {tow_rx, tow_rx_bytes}, {d_pred_rx, rx_bytes}, {d_pred, pred_bytes}, {d_sync_state, sync_bytes},
                                      {d_obs_state, st_bytes}, {d_obs, obs_bytes}},
                                2, "d_tow or d_tow_rx overlaps another array"))
    return rc;
  gpsx_wtow_t *d_tow = tow;
  gpsx_wtow_rx_t *d_tow_rx = tow_rx;
  Staging s;
  s.add(&d_tow, tow, tow_bytes, COPY_OUT);
  s.add(&d_tow_rx, tow_rx, tow_rx_bytes, COPY_OUT);
  if (host)
    if (int rc = stage(ctx, &s)) return rc;
  return launch_and_report(ctx, host, s, "k_wtow", "k_wtow raised the bad-state flag, which it never does", [&](uint32_t *) {
    launch_wtow(ctx->stream, *cfg, n_rx, n_prn, prns, d_pred_rx, d_pred, d_sync_state, d_obs_state, d_obs, d_tow, d_tow_rx);
  });
}

// ---- almanac, ionosphere and UTC from the same words as weph's (host: rx and alm are host memory, staged through the arena; the words,
//      the slot states and the banks are device memory in both variants) ----------------------------------------------------------------
int walm(gpsx_ctx *ctx, const gpsx_walm_cfg_t *cfg, const gpsx_wnav_word_t *d_words, int n_blocks, int n_rx, gpsx_walm_slot_t *d_slot_state,
         gpsx_walm_bank_t *d_bank, gpsx_walm_rx_t *rx, gpsx_walm_sv_t *alm, bool host)
{
  if (int rc = use_device(ctx)) return rc;
  if (!cfg || !d_words || !d_slot_state || !d_bank || !rx)
    return fail(ctx, GPSX_EINVAL, "null argument");
  if (int rc = check_ch_per_rx(ctx, cfg->ch_per_rx)) return rc;
  if (cfg->reserved[0] != 0 || cfg->reserved[1] != 0 || cfg->reserved[2] != 0)
    return fail(ctx, GPSX_EINVAL, "reserved must be 0");
  if (int rc = check_n_blocks(ctx, n_blocks)) return rc;
  if (int rc = check_n_rx(ctx, n_rx)) return rc;
  if (int rc = check_aligned(ctx, {d_words, d_slot_state, d_bank}, 16, "d_words, d_slot_state and d_bank must be 16-byte aligned")) return rc;
  if (!host)
    if (int rc = check_aligned(ctx, {rx, alm}, 16, "d_rx and d_alm must be 16-byte aligned")) return rc;
  size_t words_bytes = 0, slot_bytes = 0, bank_bytes = 0, rx_bytes = 0, alm_bytes = 0;
  if (records_overflow((size_t)n_rx * (size_t)(n_blocks / 600 + 2), cfg->ch_per_rx, sizeof(gpsx_wnav_word_t), &words_bytes) ||
      records_overflow((size_t)n_rx, cfg->ch_per_rx, sizeof(gpsx_walm_slot_t), &slot_bytes) ||
      records_overflow((size_t)n_rx, 1, sizeof(gpsx_walm_bank_t), &bank_bytes) || records_overflow((size_t)n_rx, 1, sizeof(gpsx_walm_rx_t), &rx_bytes) ||
      records_overflow((size_t)n_rx, 32, sizeof(gpsx_walm_sv_t), &alm_bytes))
    return fail(ctx, GPSX_EINVAL, "n_rx x ch_per_rx records overflow a size");
  if (int rc = check_no_overlap(ctx, {{d_words, words_bytes}, {d_slot_state, slot_bytes}, {d_bank, bank_bytes}, {rx, rx_bytes}, {alm, alm_bytes}}, 5,
                                "two arrays overlap"))
    return rc;
  gpsx_walm_rx_t *d_rx = rx;
  gpsx_walm_sv_t *d_alm = alm;
  Staging s;
  s.add(&d_rx, rx, rx_bytes, COPY_OUT);
  s.add(&d_alm, alm, alm_bytes, COPY_OUT);
  if (host)
    if (int rc = stage(ctx, &s)) return rc;
  return launch_and_report(ctx, host, s, "k_walm",
                           "a slot's almanac state or a receiver's almanac bank is out of range (it is untouched, a bad bank's records are zero)",
                           [&](uint32_t *flag) { launch_walm(ctx->stream, *cfg, d_words, n_blocks, n_rx, d_slot_state, d_bank, d_rx, d_alm, flag); });
}

// ---- the weighted grid in a window around each prediction (host: pred, the blocks, peaks and rep are host memory, staged through the
//      arena; the capture without the tracking calls' slack) ----------------------------------------------------------------------------
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
  if (int rc = check_grid_shape(ctx, g)) return rc;
  if (g->search_stride_blocks < 0)
    return fail(ctx, GPSX_EINVAL, "search_stride_blocks must be at least 0");
  if (int rc = check_prn_list(ctx, g->prns, g->n_prn)) return rc;
  if (int rc = check_doppler_bins(ctx, g)) return rc;
  if (n_blocks < 1 || (long long)(g->n_search - 1) * g->search_stride_blocks + (long long)cfg->n_coh * cfg->n_seg > n_blocks)
    return fail(ctx, GPSX_EINVAL, "not enough blocks for the searches");
  if (!host)
    if (int rc = check_aligned(ctx, {pred, rep}, 16, "d_pred and d_rep must be 16-byte aligned")) return rc;
  size_t peak_bytes = 0, pred_bytes = 0, rep_bytes = 0, if_bytes = 0;
  if (records_overflow((size_t)g->n_search * (size_t)g->n_prn, g->n_dopp, sizeof(gpsx_peak_t), &peak_bytes) ||
      records_overflow((size_t)g->n_search, g->n_prn, sizeof(gpsx_wpred_t), &pred_bytes) ||
      records_overflow((size_t)g->n_search, g->n_prn, sizeof(gpsx_acq_window_rep_t), &rep_bytes) ||
      records_overflow((size_t)n_blocks, 1, (size_t)GPSX_BYTES_PER_MS_2BIT, &if_bytes))
    return fail(ctx, GPSX_EINVAL, "n_search x n_prn x n_dopp records overflow a size");
  const gpsx_wpred_t *d_pred = pred;
  const uint8_t *d_if = static_cast<const uint8_t *>(if_blocks_2bit);
  gpsx_peak_t *d_peaks = peaks;
  gpsx_acq_window_rep_t *d_rep = rep;
  Staging s;
  s.add(&d_pred, pred, pred_bytes, COPY_IN);
  s.add(&d_if, if_blocks_2bit, if_bytes, COPY_IN);
  s.add(&d_peaks, peaks, peak_bytes, COPY_OUT);
  s.add(&d_rep, rep, rep_bytes, COPY_OUT);
  if (host)
    if (int rc = stage(ctx, &s)) return rc;
  return launch_and_report(ctx, host, s, "k_acq_win", "k_acq_win raised the bad-state flag, which it never does", [&](uint32_t *) {
    launch_acq_win(ctx->stream, *cfg, d_if, g->n_search, g->search_stride_blocks, g->n_prn, g->prns, ctx->d_chips_all, ctx->if_hz, g->dopp_min_hz,
                   g->dopp_step_hz, g->n_dopp, g->weights == GPSX_WEIGHTS_SIGN_MAGNITUDE, d_pred, d_peaks, d_rep);
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
  if (int rc = check_ion(ctx, cfg->ion)) return rc;
  if (int rc = check_el_min(ctx, cfg->el_min_rad)) return rc;
  if (!(cfg->epoch_offset_s >= 0.0 && cfg->epoch_offset_s <= 4.096))
    return fail(ctx, GPSX_EINVAL, "epoch_offset_s must be finite and 0..4.096");
  if (!is_finite(cfg->max_resid_m) || !(cfg->max_resid_m > 0.0))
    return fail(ctx, GPSX_EINVAL, "max_resid_m must be finite and above 0");
  if (int rc = check_det_ratio(ctx, cfg->det_num, cfg->det_den)) return rc;
  if (int rc = check_min_sats(ctx, cfg->min_sats, 5)) return rc;
  for (int32_t v : cfg->reserved)
    if (v != 0)
      return fail(ctx, GPSX_EINVAL, "reserved must be 0");
  if (int rc = check_grid_shape(ctx, g)) return rc;
  if (int rc = check_prn_list(ctx, g->prns, g->n_prn)) return rc;
  if (int rc = check_doppler_bins(ctx, g)) return rc;
  if (bank_stride != 0 && bank_stride != g->n_prn)
    return fail(ctx, GPSX_EINVAL, "bank_stride must be 0 or n_prn");
  if (int rc = check_aligned(ctx, {d_bank}, 16, "d_bank must be 16-byte aligned")) return rc;
  if (!host) {
    if (int rc = check_aligned(ctx, {peaks}, 4, "d_peaks must be 4-byte and d_prior 8-byte aligned")) return rc;
    if (int rc = check_aligned(ctx, {prior}, 8, "d_peaks must be 4-byte and d_prior 8-byte aligned")) return rc;
    if (int rc = check_aligned(ctx, {snap, sv}, 16, "d_snap and d_sv must be 16-byte aligned")) return rc;
  }
  size_t peak_bytes = 0, bank_bytes = 0, prior_bytes = 0, snap_bytes = 0, sv_bytes = 0;
  if (records_overflow((size_t)g->n_search * (size_t)g->n_prn, g->n_dopp, sizeof(gpsx_peak_t), &peak_bytes) ||
      records_overflow((size_t)(bank_stride ? g->n_search : 1), g->n_prn, sizeof(gpsx_weph_t), &bank_bytes) ||
      records_overflow((size_t)g->n_search, 1, sizeof(gpsx_wsnap_prior_t), &prior_bytes) ||
      records_overflow((size_t)g->n_search, 1, sizeof(gpsx_wsnap_t), &snap_bytes) ||
      records_overflow((size_t)g->n_search, g->n_prn, sizeof(gpsx_wsnap_sv_t), &sv_bytes))
    return fail(ctx, GPSX_EINVAL, "n_search x n_prn x n_dopp records overflow a size");
  if (!host)   // (the two outputs against each other and against the three inputs)
    if (int rc = check_no_overlap(ctx, {{snap, snap_bytes}, {sv, sv_bytes}, {peaks, peak_bytes}, {d_bank, bank_bytes}, {prior, prior_bytes}}, 2,
                                  "d_snap or d_sv overlaps another array"))
      return rc;
  const gpsx_peak_t *d_peaks = peaks;
  const gpsx_wsnap_prior_t *d_prior = prior;
  gpsx_wsnap_t *d_snap = snap;
  gpsx_wsnap_sv_t *d_sv = sv;
  Staging s;
  s.add(&d_peaks, peaks, peak_bytes, COPY_IN);
  s.add(&d_prior, prior, prior_bytes, COPY_IN);
  s.add(&d_snap, snap, snap_bytes, COPY_OUT);
  s.add(&d_sv, sv, sv_bytes, COPY_OUT);
  if (host)
    if (int rc = stage(ctx, &s)) return rc;
  return launch_and_report(ctx, host, s, "k_wsnap", "k_wsnap raised the bad-state flag, which it never does", [&](uint32_t *) {
    launch_wsnap(ctx->stream, *cfg, g->n_search, g->n_prn, g->dopp_min_hz, g->dopp_step_hz, g->n_dopp, d_peaks, d_bank, bank_stride, d_prior, d_snap, d_sv);
  });
}

}  // namespace

// ---- the entry points, in include/gpsx.h's order -----------------------------------------------------------------------------------------
extern "C" {

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

int gpsx_wobs_pseudoranges(const gpsx_wobs_t *obs, int n, double offset_ms, double *pr_m, double *rx_tow_s)
{
  if (!obs || !pr_m || !rx_tow_s || n < 1 || !is_finite(offset_ms))
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
  if (!obs || !pr_m || !rx_tow_s || !n_valid || n_rx < 1 || ch_per_rx < 1 || __builtin_mul_overflow(n_rx, ch_per_rx, &n_ch) || !is_finite(offset_ms))
    return GPSX_EINVAL;
  for (int r = 0; r < n_rx; r++) {   // (the arguments are good: a slice's call returns its count)
    const size_t at = (size_t)r * (size_t)ch_per_rx;
    n_valid[r] = gpsx_wobs_pseudoranges(obs + at, ch_per_rx, offset_ms, pr_m + at, rx_tow_s + r);
    total += n_valid[r];
  }
  return total;
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

}  // extern "C"
