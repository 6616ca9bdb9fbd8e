/* include/gpsx.h -- C ABI of libgpsx.so, the MI355X (gfx950) GPS L1 C/A correlator engine.
 *
 * This is the "Tier 3" batched interface: plain pointers and sizes, no C++/torch types.  It
 * replaces, for many channels / hypotheses per call, what the reference firmware does one call at a time through
 * Firmware/project_main/GPS/gps_misc.h:195-216 (the per-call, symbol-compatible "Tier 1" mirror of that header is
 * include/gpsx_compat.h).  Everything below executes on the GPU; there is no CPU fallback -- without a usable HIP
 * device gpsx_create() fails with GPSX_ENODEV and nothing else can be called.
 *
 * Sample format (reference: PM/config.h:23-28, PM/signal_capture.c:9-11): 1 bit per sample (MAX2769 sign bit),
 * LSB first, fs = 16.368 MHz, IF = 4.092 MHz, one "block" = 1 ms = 16368 samples = 2046 bytes.
 *
 * Conventions: functions return 0 (GPSX_OK) or a negative errno-style code; *_dev variants take DEVICE pointers and
 * only enqueue work on the context's HIP stream (call gpsx_synchronize, or synchronize the stream you passed to
 * gpsx_create); the variants without _dev take HOST pointers and return when the results are in host memory.
 * A context is thread-compatible, not thread-safe (one stream, one set of scratch buffers).
 */
#ifndef GPSX_H
#define GPSX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPSX_VERSION            110        /* 0.1.1: gpsx_loop_state_t is 120 bytes (96 up to 0.1.0), flag bit 7 = "served" is new and
                                            * gps_tracking_words_batch skips flag bytes without it, the product library reads no
                                            * $GPSX_ACQ_* / $GPSX_TRACK_WAVE_FROM knobs (lib/libgpsx_lab.so does).  A host built against an
                                            * older header must not run on this library: call gpsx_abi_check once at start-up.
                                            * gpsx_acq_grid_weighted_ms(_dev) came later in 0.1.1: new entry points, no layout change;
                                            * so did gpsx_acq_grid_weighted_coh(_dev).
                                            * gpsx_track_epl_weighted(_dev) likewise: new entry points, no layout change;
                                            * gpsx_track_loop_weighted(_dev) and gpsx_track_loop_weighted_sync(_dev) too (new
                                            * structs of their own); gpsx_wnav_words(_dev) and gpsx_wnav_subframe_image likewise;
                                            * gpsx_wobs(_dev) and gpsx_wobs_pseudoranges too; gpsx_weph(_dev) and
                                            * gpsx_weph_to_eph (include/gpsx_compat.h) likewise; so are the four carrier-aided loop
                                            * calls gpsx_track_loop_weighted(_sync)_aided(_dev) with gpsx_waid_t; gpsx_wlock(_dev) and
                                            * gpsx_wlock_cn0_dbhz likewise; gpsx_track_loop_weighted_sync_multi(_dev) with
                                            * gpsx_wmulti_t and gpsx_wobs_pseudoranges_rx too; gpsx_wfix(_dev) with gpsx_wfix_cfg_t
                                            * and gpsx_wfix_t likewise; gpsx_wfde(_dev) with gpsx_wfde_cfg_t and gpsx_wfde_t too;
                                            * gpsx_wvel(_dev) with gpsx_wvel_cfg_t and gpsx_wvel_t likewise;
                                            * gpsx_wkf(_dev) with gpsx_wkf_cfg_t, gpsx_wkf_state_t and gpsx_wkf_t too. */
#define GPSX_BYTES_PER_MS       2046       /* PM/config.h:26-27: 16368 one-bit samples                    */
#define GPSX_PHASES_BYTE        2046       /* code-phase hypotheses at byte (0.5 chip) granularity         */
#define GPSX_PHASES_FINE        16368      /* byte offset x 8 replica bit shifts (PM/GPS/tracking.c:23)    */
#define GPSX_IF_HZ              4092000    /* PM/config.h:23                                               */
#define GPSX_MAX_PRN            210        /* PM/GPS/gps_misc.c:319-341                                    */

/* IF sample formats accepted wherever an entry point takes IF blocks (select with gpsx_set_if_format):
 *   GPSX_IF_1BIT    the reference's format: MAX2769 I1 (sign) only, 8 samples per byte LSB first, 2046 bytes per ms
 *   GPSX_IF_2BIT_SM MAX2769 I1/I0 sign + magnitude: 4 samples per byte LSB first, sample n in bits 2(n&3) (sign) and
 *                   2(n&3)+1 (magnitude), 4092 bytes per ms.  The kernels unpack the pairs in LDS and correlate on the
 *                   SIGN plane, i.e. exactly what the reference computes from the same front end (it wires I1 only,
 *                   PM/config.h:16); the magnitude plane is available through gpsx_if_unpack2. */
#define GPSX_IF_1BIT            0
#define GPSX_IF_2BIT_SM         1
#define GPSX_BYTES_PER_MS_2BIT  4092

#define GPSX_OK       0
#define GPSX_EIO     (-5)    /* a HIP runtime call failed (see gpsx_last_error)   */
#define GPSX_ENOMEM  (-12)
#define GPSX_ENODEV  (-19)   /* no usable gfx950 device                            */
#define GPSX_EINVAL  (-22)

typedef struct gpsx_ctx gpsx_ctx;

/* What correlation_search() (PM/GPS/gps_misc.c:155-191) returns, plus the un-divided sum. */
typedef struct {
  uint32_t max_val;  /* return value: largest correlation magnitude in the window                            */
  uint32_t phase;    /* *phase: first byte offset reaching it; 0 if nothing exceeded 0                       */
  uint32_t sum;      /* sum of magnitudes over the window                                                     */
  uint32_t avr;      /* *aver_val: sum / 2046 (the divisor is constant whatever the window)                   */
} gpsx_peak_t;

/* ---- context ------------------------------------------------------------------------------------------------ */

/* device: HIP device ordinal.  stream: a hipStream_t to enqueue on (e.g. torch's current stream), or NULL to let
 * the context create its own. */
int         gpsx_create(gpsx_ctx **ctx, int device, void *stream);
/* Receiver constants (the reference fixes them at compile time, PM/config.h:23-28).  sample_rate_hz is structural: the
 * 2046-byte millisecond and the 16368-phase grid are compiled into the kernels, any value but 16368000 is refused with
 * GPSX_EINVAL.  if_hz -- the centre of the acquisition grid's Doppler axis and the frequency a tracking channel's
 * if_freq_offset_hz is relative to -- is a run-time value of the context (front ends with another IF plan); entry points
 * that take absolute frequencies (gpsx_acq_jobs, gpsx_wipeoff) and the reference-named calls of gpsx_compat.h, whose
 * IF_FREQ_HZ is the reference's #define, do not look at it. */
typedef struct {
  uint32_t sample_rate_hz;   /* 16368000                                                                   */
  int32_t  if_hz;            /* GPSX_IF_HZ by default; 0 < if_hz < sample_rate_hz / 2                      */
} gpsx_config_t;
void        gpsx_config_default(gpsx_config_t *cfg);
int         gpsx_set_config(gpsx_ctx *ctx, const gpsx_config_t *cfg);
int         gpsx_get_config(const gpsx_ctx *ctx, gpsx_config_t *cfg);
void        gpsx_destroy(gpsx_ctx *ctx);
int         gpsx_synchronize(gpsx_ctx *ctx);
const char *gpsx_last_error(const gpsx_ctx *ctx);   /* text of the last failure on this context */
const char *gpsx_strerror(int code);
/* name of the dominant kernel the last gpsx_acq_grid* call launched (which form of the grid kernel the size picked) */
const char *gpsx_last_kernel(const gpsx_ctx *ctx);
int         gpsx_version(void);
/* The ABI handshake: pass the header's GPSX_VERSION and the sizes the host was COMPILED with,
 *   gpsx_abi_check(GPSX_VERSION, sizeof(gpsx_loop_state_t), sizeof(gpsx_acq_grid_t), sizeof(gpsx_peak_t))
 * GPSX_OK when the library was built from the same layout; GPSX_EINVAL when not (a host that strides d_state by another
 * sizeof(gpsx_loop_state_t) would corrupt device memory without any error).  Needs no context. */
int         gpsx_abi_check(int header_version, size_t sizeof_loop_state, size_t sizeof_acq_grid, size_t sizeof_peak);
/* name / CU count / clock of the device behind the context (for bench reports) */
int         gpsx_device_info(const gpsx_ctx *ctx, char *name, size_t name_len, int *compute_units, int *clock_khz);

/* Which hardware the fine acquisition grid (gpsx_acq_grid*, GPSX_PHASES_FINE) runs on.  Both give the same triplets and keys,
 * bit for bit (tests/test_gpu_parity.py; bench.py's letter_compliant leg compares the key tables of a whole 256-capture launch).
 *   GPSX_ACQ_PATH_MATRIX (default)  the exact MX-FP4 Toeplitz GEMM on the matrix cores (k_acq_mx)
 *   GPSX_ACQ_PATH_VECTOR            bit planes, v_and + v_bcnt polyphase recurrence, wave reductions on the vector ALU
 *                                   (k_acq_poly): no MFMA, about a sixth of the rate
 * The weighted two-bit extension (gpsx_acq_grid_weighted) follows the same switch: k_acq_mxw / k_acq_weighted. */
#define GPSX_ACQ_PATH_MATRIX 0
#define GPSX_ACQ_PATH_VECTOR 1
int gpsx_set_acq_path(gpsx_ctx *ctx, int path);
/* 0 for lib/libgpsx.so.  1 for lib/libgpsx_lab.so, the same sources built with -DGPSX_LAB: it additionally reads the
 * $GPSX_ACQ_* / $GPSX_TRACK_WAVE_FROM knobs that force kernel forms (tests of the alternative kernels, A/B timing). */
int gpsx_is_lab_build(void);

/* Sample format of the IF blocks passed to gpsx_acq_* and gpsx_track_* from now on (default GPSX_IF_1BIT). */
int gpsx_set_if_format(gpsx_ctx *ctx, int if_format);
/* Split n_blocks x 4092 bytes of GPSX_IF_2BIT_SM samples into the sign and magnitude bit planes, each n_blocks x 2046
 * bytes in the 1-bit layout (either output may be NULL).  Host buffers. */
int gpsx_if_unpack2(gpsx_ctx *ctx, const uint8_t *if_2bit, int n_blocks, uint8_t *sign_plane, uint8_t *magnitude_plane);

/* device memory + HIP-event timing on the context's stream (so a C caller needs no HIP headers) */
int gpsx_malloc(gpsx_ctx *ctx, void **dptr, size_t bytes);
/* page-locked host memory for the buffers a real-time host hands to the host-pointer entry points every millisecond
 * (capture blocks, channel states, accumulators): copies to and from it are plain DMA, without the runtime's staging of
 * pageable pages and its jitter */
int gpsx_host_alloc(gpsx_ctx *ctx, void **hptr, size_t bytes);
int gpsx_host_free(gpsx_ctx *ctx, void *hptr);
/* Pins the CALLING thread to the CPUs of the NUMA node the context's GPU hangs off (sysfs local_cpulist of its PCI
 * function), so that the per-millisecond buffers -- allocate them with gpsx_host_alloc afterwards: first touch -- and the
 * thread that fills them sit on the socket the DMA goes to.  On a two-socket host the far socket costs the E/P/L step of
 * 65536 channels 15-20 % and most of its jitter.  Returns GPSX_ENODEV (and changes nothing) when the topology is not
 * exposed; undo with sched_setaffinity. */
int gpsx_bind_thread_to_device(gpsx_ctx *ctx);
int gpsx_free(gpsx_ctx *ctx, void *dptr);
int gpsx_memcpy_h2d(gpsx_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
int gpsx_memcpy_d2h(gpsx_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);
int gpsx_event_create(gpsx_ctx *ctx, void **event);
int gpsx_event_record(gpsx_ctx *ctx, void *event);
int gpsx_event_elapsed_ms(gpsx_ctx *ctx, void *start, void *stop, float *ms);  /* synchronizes on `stop` */
int gpsx_event_destroy(gpsx_ctx *ctx, void *event);

/* ---- IF ingest: the capture ring  (replaces the circular DMA buffer and its half/full-transfer interrupt,
 *      PM/signal_capture.c:14-24,57-82, and the file replay of PC_SpiLight: raw stream, 2046 bytes per ms in the 1-bit
 *      format, 4092 in GPSX_IF_2BIT_SM) -------------------------------------------------------------------------------
 * A ring of n_slots 1 ms blocks in pinned host memory with a mirror in HBM.  The producer fills the write slot and
 * commits it -- what the DMA interrupt does: the ready pointer moves on, the packet counter counts, and the block goes
 * to the device by an asynchronous copy from pinned memory, enqueued on the context's stream (the call does not wait).
 * Host entry points of this library (gpsx_acq_grid, gpsx_acq_jobs, gpsx_track_epl_batch above 32768 channels, and the
 * reference-named step calls on top of them) recognise a pointer into a committed part of the ring and read the HBM
 * mirror instead of copying the block again.  (The per-millisecond tracking step of up to 32768 channels is one captured
 * graph that stages its own 2 KB block next to the channel states: one launch beats a saved 2 KB copy.)  The format is the context's if_format at creation time. */
typedef struct gpsx_capture gpsx_capture;
int            gpsx_capture_create(gpsx_ctx *ctx, int n_slots, gpsx_capture **cap);      /* 1 <= n_slots <= 4096 */
void           gpsx_capture_destroy(gpsx_capture *cap);
/* the slot the next block goes into (block_bytes of pinned memory); valid until the next commit */
uint8_t       *gpsx_capture_write_slot(gpsx_capture *cap);
int            gpsx_capture_commit(gpsx_capture *cap);
/* convenience: copy one block into the write slot and commit it */
int            gpsx_capture_push(gpsx_capture *cap, const uint8_t *block);
/* newest committed block, host view (NULL before the first commit) */
const uint8_t *gpsx_capture_ready_buf(const gpsx_capture *cap);
/* the last n_blocks committed blocks, oldest first, contiguous in HBM (n_blocks <= min(n_slots, blocks committed));
 * a window that wraps around the ring is gathered into a side buffer on the stream, valid until the next call.  Pass
 * the pointer to the *_dev entry points. */
int            gpsx_capture_window_dev(gpsx_capture *cap, int n_blocks, const void **d_blocks);
uint32_t       gpsx_capture_packet_cnt(const gpsx_capture *cap);                          /* blocks committed so far */
size_t         gpsx_capture_block_bytes(const gpsx_capture *cap);
/* Replay a recorded raw IF file through the ring: blocks first_block .. (at most max_blocks, < 0 = to the end) are read
 * into the write slot and committed one by one; after each commit on_block(user, cap, index) runs (may be NULL) and a
 * non-zero return stops the replay.  Returns the number of blocks committed, or a negative GPSX_E* code. */
typedef int (*gpsx_capture_block_fn)(void *user, gpsx_capture *cap, long block_index);
long           gpsx_capture_replay_file(gpsx_capture *cap, const char *path, long first_block, long max_blocks,
                                        gpsx_capture_block_fn on_block, void *user);

/* ---- K1: C/A Gold codes  (replaces gps_generate_prn / gps_channell_prepare, PM/GPS/gps_misc.c:306-372) -------- */

/* chips_out: n_prn x 1023 bytes of 0/1.  prn must be 1..210 (the reference silently ignores prn < 1; this
 * interface validates instead and returns GPSX_EINVAL). */
int gpsx_ca_codes(gpsx_ctx *ctx, const uint8_t *prns, int n_prn, uint8_t *chips_out);

/* ---- K2+K3+K4: acquisition grid  (replaces the data-parallel prefix of acquisition_freq_search /
 *      acquisition_code_phase_search, PM/GPS/acquisition.c:196-312: gps_generate_prn_data2 + gps_shift_to_zero_freq
 *      + correlation_search per (channel, Doppler bin, ms), here for every PRN x Doppler x phase in one launch) ---- */

typedef struct {
  int32_t        n_search;             /* independent searches (e.g. consecutive capture instants)              */
  int32_t        n_ms;                 /* blocks summed non-coherently per search; 1 = the reference            */
  int32_t        search_stride_blocks; /* search s starts at block s * stride                                   */
  int32_t        n_prn;
  const uint8_t *prns;                 /* HOST pointer, n_prn PRN numbers                                       */
  int32_t        dopp_min_hz;          /* Doppler bin d is dopp_min_hz + d * dopp_step_hz  (acquisition.c:285)  */
  int32_t        dopp_step_hz;
  int32_t        n_dopp;
  int32_t        phase_mode;           /* GPSX_PHASES_BYTE (replica shift 0 only) or GPSX_PHASES_FINE (0..7)   */
  int32_t        win_start, win_stop;  /* byte-offset window [start, stop); 0, 2046 for a full search           */
  int32_t        shard_index;          /* multi-GPU: of the U = n_search * n_dopp * ceil(n_prn / 8) work units      */
  int32_t        shard_count;          /*   u = (search * n_dopp + dopp) * ceil(n_prn / 8) + prn_idx / 8 this process  */
                                       /*   computes the run [index * U / count, (index + 1) * U / count); 0/1: all    */
} gpsx_acq_grid_t;

/* number of replica bit shifts a phase_mode implies (1 or 8) */
int gpsx_acq_bits(int phase_mode);

/* Sizes (in elements) of the result arrays for a descriptor: peaks[n_search][n_prn][n_dopp][n_bits],
 * keys[n_search][n_prn][n_dopp]. */
size_t gpsx_acq_peaks_count(const gpsx_acq_grid_t *g);
size_t gpsx_acq_keys_count(const gpsx_acq_grid_t *g);

/* Enqueue one grid.  d_if_blocks: n_blocks x 2046 bytes, blocks contiguous.  d_peaks: gpsx_acq_peaks_count()
 * entries; entries of (search, PRN, Doppler) units owned by other shards are written as zero.  d_keys (may be NULL):
 * one packed int64 per (search, PRN, Doppler): (max_val << 14) | (16383 - fine_phase), fine_phase = 8 * phase + bit
 * shift, maximised over the bit shifts -- zero for units of other shards, so that ONE all-reduce(MAX) over the ranks
 * yields every unit's peak, ties resolved to the lowest fine phase like correlation_search's strict '>'.
 * Optional debug/inspection outputs (NULL to skip), indexed like d_peaks with one more trailing axis:
 *   d_per_ms [..][n_ms]   the triplet the reference would have produced for each single block
 *   d_energy [..][2046]   accumulated magnitude per byte offset (0 outside the window)
 *   d_cnt    [..][2046][2] raw popcounts cnt_i, cnt_q of the LAST block (what gps_mult_and_summ returns) */
int gpsx_acq_grid_dev(gpsx_ctx *ctx, const gpsx_acq_grid_t *g, const void *d_if_blocks, int n_blocks,
                      gpsx_peak_t *d_peaks, int64_t *d_keys, gpsx_peak_t *d_per_ms, uint32_t *d_energy,
                      uint16_t *d_cnt);

/* Host-buffer convenience: copies the blocks in, runs, copies peaks (and keys if non-NULL) out. */
int gpsx_acq_grid(gpsx_ctx *ctx, const gpsx_acq_grid_t *g, const uint8_t *if_blocks, int n_blocks,
                  gpsx_peak_t *peaks, int64_t *keys);
/* The same, enqueued only: copy in, sweep and copies out are put on the context's stream and the call returns; the
 * host buffers (pinned memory, or the copies are not asynchronous) belong to the engine until gpsx_synchronize(ctx).
 * Two contexts used alternately overlap one call's PCIe transfers with the other's sweep -- how a host that streams
 * captures through the engine reaches the HBM-resident rate (bench.py `pcie_inclusive`). */
int gpsx_acq_grid_async(gpsx_ctx *ctx, const gpsx_acq_grid_t *g, const uint8_t *if_blocks, int n_blocks,
                        gpsx_peak_t *peaks, int64_t *keys);

/* Explicit job list: one search per job, each with its own PRN, carrier frequency, replica shift and window --
 * what acquisition_process() needs for the reference's 4-channel table with per-channel Doppler hints
 * (PM/GPS/acquisition.c:51-57,72-79) and what pre-tracking needs (PM/GPS/tracking.c:398-450). */
typedef struct {
  int32_t  block;        /* first block of the search                              */
  int32_t  n_ms;
  int32_t  prn;
  float    freq_hz;      /* IF + Doppler, as passed to gps_shift_to_zero_freq      */
  int32_t  offset_bits;  /* replica shift 0..15 (gps_generate_prn_data2)           */
  int32_t  win_start, win_stop;
} gpsx_acq_job_t;

int gpsx_acq_jobs(gpsx_ctx *ctx, const gpsx_acq_job_t *jobs, int n_jobs, const uint8_t *if_blocks, int n_blocks,
                  gpsx_peak_t *peaks /* n_jobs */, uint32_t *energy_opt /* n_jobs x 2046 or NULL */);

/* unpack a key produced by gpsx_acq_grid* */
static inline uint32_t gpsx_key_energy(int64_t key) { return (uint32_t)(key >> 14); }
static inline uint32_t gpsx_key_fine_phase(int64_t key) { return 16383u - (uint32_t)(key & 16383); }

/* ---- the sharded sweep inside ONE process (a C host has no torch.distributed): a group of contexts, one per GPU,
 *      joined by RCCL communicators (ncclCommInitAll; librccl is loaded when the first group is created).
 *      gpsx_acq_grid_sharded = what each rank of `bench.py --gpus N` does, for all the group's devices at once:
 *      context i sweeps the run of grid units [i * U / n, (i + 1) * U / n) (g's own shard fields are ignored) on its own copy of the
 *      captures, then ONE all-reduce(MAX) of the packed keys leaves the merged table in every d_keys[i].  Everything is
 *      enqueued on the contexts' streams; synchronize the contexts (or read through gpsx_memcpy_d2h) before using it. */
typedef struct gpsx_group gpsx_group;
int  gpsx_group_create(gpsx_ctx *const *ctxs, int n, gpsx_group **group);   /* n >= 1 contexts on n DIFFERENT devices */
void gpsx_group_destroy(gpsx_group *group);
int  gpsx_acq_grid_sharded(gpsx_group *group, const gpsx_acq_grid_t *g, const void *const *d_if_blocks, int n_blocks,
                           gpsx_peak_t *const *d_peaks, int64_t *const *d_keys);

/* ---- EXTENSION, not in the reference: the acquisition grid on WEIGHTED two-bit samples ---------------------------------
 * The reference wires the MAX2769's sign bit only (PM/config.h:16), and everything else in this header computes what the
 * reference computes -- from GPSX_IF_2BIT_SM captures too, whose magnitude bit it ignores.  This entry point is the one place
 * that uses both bits; it has its own CPU restatement to be tested against (tests/test_gpu_weighted.py) and cannot change a one-bit result.
 *   sample value   v[n] = (sign ? +1 : -1) * (magnitude ? 3 : 1)       GPSX_WEIGHTS_SIGN_MAGNITUDE
 *                  v[n] = (sign ? +1 : -1)                              GPSX_WEIGHTS_SIGN_ONLY (the same correlator on the sign
 *                                                                       plane: the point a processing gain is measured from)
 *   carrier        the reference's NCO (gps_shift_to_zero_freq, PM/GPS/gps_misc.c:211-240: the accumulator's quadrant picks the
 *                  Fs/4 pattern per 32-sample word, phase 0 at the block's start); the sixteen samples it never mixes: weight 0
 *   replica        the C/A code circularly at fine phase tau: chip ((n - tau) mod 16368) / 16
 *   result         per (search, PRN, Doppler bin): max over the 16368 phases of floor(sqrt(I^2 + Q^2)) (exact integers), the first
 *                  phase reaching it (0 .. 16367), the sum over the phases and sum / 16368 -- peaks[n_search][n_prn][n_dopp].
 * One 1 ms block per search (search s reads block s * search_stride_blocks), 4092-byte blocks whatever the context's format.
 * Runs on the matrix cores (k_acq_mxw: the Toeplitz GEMM of the sign-only grid on sums of sixteen weighted samples, MX-FP4 operands,
 * exact; about 9 x 10^11 hypotheses/s) or, under GPSX_ACQ_PATH_VECTOR, on the vector ALU (k_acq_weighted: v_dot4_i32_i8, about
 * 4 x 10^10): the same records, bit for bit. */
#define GPSX_WEIGHTS_SIGN_ONLY      0
#define GPSX_WEIGHTS_SIGN_MAGNITUDE 1
typedef struct {
  int32_t        n_search, search_stride_blocks;
  int32_t        n_prn;
  const uint8_t *prns;                 /* HOST pointer, n_prn PRN numbers 1 .. 210 */
  int32_t        dopp_min_hz, dopp_step_hz, n_dopp;
  int32_t        weights;              /* GPSX_WEIGHTS_* */
} gpsx_acq_weighted_t;
int gpsx_acq_grid_weighted_dev(gpsx_ctx *ctx, const gpsx_acq_weighted_t *g, const void *d_if_blocks_2bit, int n_blocks,
                               gpsx_peak_t *d_peaks);
int gpsx_acq_grid_weighted(gpsx_ctx *ctx, const gpsx_acq_weighted_t *g, const uint8_t *if_blocks_2bit, int n_blocks,
                           gpsx_peak_t *peaks);
/* The same grid over n_ms blocks per search, summed NON-coherently:
 *   search s reads blocks s * search_stride_blocks + b for b = 0 .. n_ms-1 (4092-byte blocks whatever the context's IF format;
 *                  stride 0 and overlapping searches are legal); the call needs (n_search-1)*stride + n_ms <= n_blocks
 *   m_b(tau)       = floor(sqrt(I_b(tau)^2 + Q_b(tau)^2)) for every fine phase tau in [0, 16368): the one-block definition above
 *                  applied to block b -- the reference's NCO on the sign plane with phase 0 at EACH block's start, the sixteen
 *                  unmixed samples at weight 0, the replica circular, both GPSX_WEIGHTS_* modes
 *   E(tau)         = sum_b m_b(tau), exact (at most 128 x 69375 < 2^24; one block's m is at most floor(sqrt(2) 49056) = 69375)
 *   record         max_val = max_tau E(tau); phase = the SMALLEST tau reaching max_val; sum = sum_tau E(tau) mod 2^32 (what u32
 *                  adds give in any order); avr = sum / 16368 -- peaks[n_search][n_prn][n_dopp], as the one-block call
 * n_ms runs from 1 to 128; n_ms out of range, too few blocks and whatever the one-block call refuses return GPSX_EINVAL (with a
 * gpsx_last_error text) and write nothing.  n_ms == 1 gives records byte-identical to gpsx_acq_grid_weighted (and runs its
 * kernels).  Matrix cores (k_acq_wmx_ms: k_acq_mxw's passes per block, running sums in a grow-only HBM scratch of the context,
 * 2 MB per cluster of 32 PRNs in flight, launched in chunks of clusters; GPSX_ENOMEM if not even one cluster's scratch can be
 * had) or, under GPSX_ACQ_PATH_VECTOR, the vector ALU (k_acq_weighted_ms: running sums in registers, no scratch): the same
 * records, bit for bit. */
int gpsx_acq_grid_weighted_ms_dev(gpsx_ctx *ctx, const gpsx_acq_weighted_t *g, int n_ms,
                                  const void *d_if_blocks_2bit, int n_blocks, gpsx_peak_t *d_peaks);
int gpsx_acq_grid_weighted_ms(gpsx_ctx *ctx, const gpsx_acq_weighted_t *g, int n_ms,
                              const uint8_t *if_blocks_2bit, int n_blocks, gpsx_peak_t *peaks);
/* The same grid over n_coh blocks per search integrated COHERENTLY (I and Q added over the blocks before the magnitude):
 *   blocks         search s reads blocks s * search_stride_blocks + b for b = 0 .. n_coh-1, as the _ms call (stride 0 and
 *                  overlapping searches are legal); the call needs (n_search-1)*stride + n_coh <= n_blocks
 *   carrier        f = (float)(if_hz + dopp_min_hz + d * dopp_step_hz), as the one-block call.  Block b is wiped by the reference's
 *                  NCO on its sign plane starting from acc_b, acc_0 = 0 and acc_{b+1} = the accumulator block b leaves (the
 *                  511-word loop: acc_b = b * 511 * step32 mod 2^32, step32 = (uint32)((uint64)nco_step(f) * 32)) -- what
 *                  consecutive gps_shift_to_zero_freq_track calls on one channel do (PM/GPS/gps_misc.c:244-274); the sixteen
 *                  unmixed samples of every block: weight 0
 *   samples        vI_b[n], vQ_b[n] in {0, +-1, +-3} ({0, +-1} under GPSX_WEIGHTS_SIGN_ONLY)
 *   correlation    I(tau) = sum_b sum_n vI_b[n] c[((n - tau) mod 16368) / 16], Q likewise, c the +-1 replica, tau in [0, 16368):
 *                  signed and exact, |I| <= 3 x 16352 x 20 = 981 120
 *   magnitude      m(tau) = floor(sqrt(I^2 + Q^2)), exact (I^2 + Q^2 < 2^41)
 *   record         the _ms call's: max_val = max m, phase = the smallest tau reaching it, sum = sum m mod 2^32, avr = sum / 16368
 * n_coh runs from 1 to 20: twenty blocks are one navigation-data bit.  n_coh out of range, too few blocks and whatever the
 * one-block call refuses return GPSX_EINVAL (with a gpsx_last_error text) and write nothing.  n_coh == 1 gives records
 * byte-identical to gpsx_acq_grid_weighted (and runs its kernels).
 * Caller guidance: a coherent window of n ms narrows a Doppler bin to about 1/n kHz -- step the grid by about 500/n Hz.  A window
 * that spans a data-bit edge loses signal; with n_coh <= 10, two consecutive searches (stride = n_coh) always include one window
 * without an edge: take the better record of the two.
 * The C/A code repeats every block, so the n_coh blocks' correlation is ONE correlation of their wiped sum: a workgroup adds the
 * blocks sample by sample in LDS and correlates once -- on the matrix cores (k_acq_coh_mx: v_mfma_i32_32x32x32_i8, a workgroup per
 * cluster of 32 PRNs) or, under GPSX_ACQ_PATH_VECTOR, the vector ALU (k_acq_coh_vec: v_dot2_i32_i16): the same records, bit for
 * bit.  No HBM scratch (no GPSX_ENOMEM). */
int gpsx_acq_grid_weighted_coh_dev(gpsx_ctx *ctx, const gpsx_acq_weighted_t *g, int n_coh,
                                   const void *d_if_blocks_2bit, int n_blocks, gpsx_peak_t *d_peaks);
int gpsx_acq_grid_weighted_coh(gpsx_ctx *ctx, const gpsx_acq_weighted_t *g, int n_coh,
                               const uint8_t *if_blocks_2bit, int n_blocks, gpsx_peak_t *peaks);
/* The product of the two multi-block calls: n_seg COHERENT windows ("segments") of n_coh blocks each per search, the windows'
 * magnitudes summed NON-COHERENTLY -- what a weak-signal search runs once one data bit is too short:
 *   blocks         search s, segment j, block b reads block s * search_stride_blocks + j * n_coh + b, j in [0, n_seg), b in
 *                  [0, n_coh) (stride 0 and overlapping searches are legal); the call needs
 *                  (n_search-1)*stride + n_coh*n_seg <= n_blocks
 *   a segment      exactly what gpsx_acq_grid_weighted_coh computes for a search starting at the segment's first block: the NCO
 *                  accumulator starts at 0 at the segment's first block and is chained through its n_coh blocks
 *                  (acc_b = b * 511 * step32 mod 2^32), the sixteen unmixed samples weigh 0, v in {0, +-1, +-3} (or {0, +-1}),
 *                  I_j(tau), Q_j(tau) signed and exact, m_j(tau) = floor(sqrt(I_j^2 + Q_j^2)) exact (< 2^21 at n_coh = 20)
 *   sum            E(tau) = sum_j m_j(tau)  (n_seg <= 128: E <= 128 x 1 387 513 < 2^28)
 *   record         the _ms call's: max_val = max E, phase = the smallest tau reaching it, sum = sum_tau E mod 2^32, avr = sum / 16368
 * n_coh runs from 1 to 20, n_seg from 1 to 128.  Checked in this order: n_coh, n_seg, n_blocks < n_coh * n_seg, then whatever the
 * one-block call refuses: each returns GPSX_EINVAL (with a gpsx_last_error text) and writes nothing.  n_seg == 1 gives records
 * byte-identical to gpsx_acq_grid_weighted_coh and n_coh == 1 to gpsx_acq_grid_weighted_ms with n_ms = n_seg (and runs their
 * kernels, with the latter's chunking and GPSX_ENOMEM): the call covers every legal argument of the two older ones.
 * Caller guidance: step the grid by about 500 / n_coh Hz.  With n_coh <= 10 no alignment to the data-bit edge is needed (at least
 * every second window is free of one).  Code Doppler slides the peak by about 3 samples per 100 ms at 5 kHz, so n_coh * n_seg much
 * beyond ~150 ms smears it unless the Doppler is small.  n_search = 20, stride = 1, n_coh = 20 scans the bit-edge alignment.
 * Matrix cores (k_acq_hyb_mx: per segment k_acq_coh_mx's pre-sum and passes, the roots added into u32 running sums in the
 * context's grow-only HBM scratch, 2 MB per cluster of 32 PRNs in flight, launched in chunks of clusters; GPSX_ENOMEM if not even
 * one cluster's scratch can be had) or, under GPSX_ACQ_PATH_VECTOR, the vector ALU (k_acq_hyb_vec: running sums in registers, no
 * scratch): the same records, bit for bit. */
int gpsx_acq_grid_weighted_hyb_dev(gpsx_ctx *ctx, const gpsx_acq_weighted_t *g, int n_coh, int n_seg,
                                   const void *d_if_blocks_2bit, int n_blocks, gpsx_peak_t *d_peaks);
int gpsx_acq_grid_weighted_hyb(gpsx_ctx *ctx, const gpsx_acq_weighted_t *g, int n_coh, int n_seg,
                               const uint8_t *if_blocks_2bit, int n_blocks, gpsx_peak_t *peaks);

/* ---- K2+K3+K5: Early/Prompt/Late tracking correlators  (replaces the correlator part of
 *      gps_tracking_data_process, PM/GPS/tracking.c:115-138, for n_ch channels at once) ------------------------- */

typedef struct {
  int32_t  prn;
  float    code_phase_fine;    /* gps_tracking_t.code_phase_fine, samples 0..16368       */
  float    if_freq_offset_hz;  /* gps_tracking_t.if_freq_offset_hz                       */
  uint32_t if_freq_accum;      /* gps_tracking_t.if_freq_accum: read, advanced, written  */
} gpsx_trk_state_t;

/* if_block: the current 1 ms block (2046 bytes, shared by all channels).  iq_out: n_ch x {IE,QE,IP,QP,IL,QL}.
 * PRNs are validated BY THE KERNELS, not before the launch (a host loop over the states costs a sixth of the millisecond at
 * 400 000 channels): a channel whose prn is outside 1..210 is correlated against the empty code, every channel's
 * if_freq_accum and accumulators ARE written, and the call then returns GPSX_EINVAL.  gpsx_track_epl_batch reports it
 * itself (it waits for its kernels); gpsx_track_epl_batch_dev only enqueues: its report comes from the next
 * gpsx_synchronize() on the context (a separate flag: step calls in between neither consume nor clear it). */
int gpsx_track_epl_batch(gpsx_ctx *ctx, const uint8_t *if_block, gpsx_trk_state_t *st, int n_ch, int16_t *iq_out);
int gpsx_track_epl_batch_dev(gpsx_ctx *ctx, const void *d_if_block, gpsx_trk_state_t *d_st, int n_ch,
                             int16_t *d_iq_out);
/* The same step for a host that has work of its own per channel (the reference's DLL / PLL / FLL after the correlators):
 * the channels go through in n_chunks (1..16) pieces on the copy / correlate / copy pipeline, and on_chunk(user, first, n) is
 * called ON THE CALLING THREAD as soon as st[first .. first + n) and iq_out of those channels are in the caller's arrays --
 * while the GPU works on the next pieces.  Page-locked arrays (gpsx_host_alloc) make the copies asynchronous.  Returns after
 * the last callback; the PRN verdict is the whole step's.  The callback must not call into the SAME context (its arena and
 * side streams are in use by the pieces still in flight): every gpsx_* entry point on it returns GPSX_EINVAL while a callback
 * runs; other contexts are free. */
typedef void (*gpsx_track_chunk_fn)(void *user, int first_channel, int n_channels);
int gpsx_track_epl_batch_chunked(gpsx_ctx *ctx, const uint8_t *if_block, gpsx_trk_state_t *st, int n_ch, int16_t *iq_out,
                                 int n_chunks, gpsx_track_chunk_fn on_chunk, void *user);

/* ---- EXTENSION, not in the reference: Early / Prompt / Late on WEIGHTED two-bit samples, K blocks per launch ---------------
 * The per-millisecond building block of a weak-signal receiver behind the weighted grids above: E/P/L I and Q on both bits, for
 * n_ch channels and n_blocks consecutive blocks in one launch, with the weighted grids' sample, carrier and replica definitions,
 * so that a grid record hands over to a channel state exactly (code_phase_fine = the record's phase, if_freq_offset_hz = its
 * Doppler bin, if_freq_accum = 0 at the window's first block: the sum of the prompts over the window's blocks is the record's I, Q).
 *   blocks         n_blocks consecutive 1 ms blocks of 4092 bytes each (GPSX_IF_2BIT_SM layout) whatever the context's IF format,
 *                  shared by all channels; 1 <= n_blocks <= 4096
 *   channel state  the gpsx_trk_state_t of gpsx_track_epl_batch (one state array serves the sign-only and the weighted step):
 *                  tau = (int)code_phase_fine (C truncation towards zero) reduced to [0, 16368) with a non-negative remainder,
 *                  constant over the call's blocks (code Doppler moves the peak about 3 samples per 100 ms at 5 kHz: the host
 *                  updates it between calls); f = (float)if_hz + if_freq_offset_hz, as gpsx_track_epl_batch forms it -- for
 *                  integer-valued offsets the weighted grids' (float)(if_hz + doppler)
 *   carrier        block b's sign plane is wiped by the reference's NCO starting from acc_b = if_freq_accum + b * 511 * step32
 *                  mod 2^32, step32 = (uint32)((uint64)nco_step(f) * 32): gpsx_acq_grid_weighted_coh's chaining, started from the
 *                  channel's accumulator instead of 0.  After the call if_freq_accum = acc_{n_blocks} is written back.  The
 *                  sixteen unmixed samples of every block: weight 0
 *   samples        vI_b[n], vQ_b[n] in {0, +-1, +-3} ({0, +-1} under GPSX_WEIGHTS_SIGN_ONLY): exactly the weighted grids' values
 *   correlators    for k = E, P, L with tau_E = tau - spacing, tau_P = tau, tau_L = tau + spacing (mod 16368):
 *                  I_k = sum_n vI_b[n] c[((n - tau_k) mod 16368) / 16], Q likewise, c the +-1 replica, circular;
 *                  |I|, |Q| <= 3 x 16352 = 49 056
 *   output         iq_out[n_blocks][n_ch][6] = IE, QE, IP, QP, IL, QL as int32, exact
 *   sign           (|E| - |L|) / (|E| + |L|) > 0 means tau is too large (magnitudes summed over 40 blocks of a satellite at
 *                  amplitude 0.1: a +3 sample error gives +0.36 at spacing 8, +0.14 at spacing 2, +0.40 at spacing 15; -3 gives
 *                  -0.32, -0.12, -0.45)
 * This is NOT gpsx_track_epl_batch on the sign plane: no reference quirks.  GPSX_WEIGHTS_SIGN_ONLY differs from that call by its
 * quirk terms (the replica's zeroed first samples, the words odd byte offsets skip, the half-chip tap spacing in bytes) and by
 * the int16 centring of its accumulators.
 * Errors: a NULL cfg, blocks, state or output pointer, weights or spacing out of range, n_blocks out of range, n_ch < 1 and a
 * size product that overflows return GPSX_EINVAL (with a gpsx_last_error text) and write nothing.  PRNs are validated BY THE
 * KERNEL, with gpsx_track_epl_batch(_dev)'s policy: a channel whose prn is outside 1..210 -- or whose code_phase_fine is not
 * finite or has magnitude >= 2^24 -- gets six zeros per block, its accumulator IS advanced, and the call then returns
 * GPSX_EINVAL: gpsx_track_epl_weighted after its wait, gpsx_track_epl_weighted_dev from the next gpsx_synchronize().
 * Vector ALU (k_track_epl_weighted: a wave per channel and block; three taps are no contraction, so there is no matrix-core form
 * and gpsx_set_acq_path does not apply).  The host variant copies blocks and states in, states and iq_out out, and does not
 * recognise capture-ring pointers. */
typedef struct {
  int32_t weights;   /* GPSX_WEIGHTS_SIGN_MAGNITUDE or GPSX_WEIGHTS_SIGN_ONLY                              */
  int32_t spacing;   /* Early and Late sit `spacing` samples before / after Prompt: 1 .. 15; 8 = half a chip */
} gpsx_trk_weighted_t;
int gpsx_track_epl_weighted_dev(gpsx_ctx *ctx, const gpsx_trk_weighted_t *cfg, const void *d_if_blocks_2bit, int n_blocks,
                                gpsx_trk_state_t *d_st, int n_ch, int32_t *d_iq_out);
int gpsx_track_epl_weighted(gpsx_ctx *ctx, const gpsx_trk_weighted_t *cfg, const uint8_t *if_blocks_2bit, int n_blocks,
                            gpsx_trk_state_t *st, int n_ch, int32_t *iq_out);

/* ---- EXTENSION, not in the reference: a closed DLL / Costas PLL / FLL on WEIGHTED two-bit samples, state resident in HBM -------
 * gpsx_track_epl_weighted with the loop behind it on the device: n_blocks consecutive 1 ms blocks per launch, the six correlator
 * sums of every coherent window of n_coh blocks (1 .. 20) fed to the discriminators, code phase and carrier updated once per
 * window, one 36-byte record per (window, channel) and nothing else back to the host.  cfg is per launch: a pull-in launch with
 * fll_c set and a small n_coh, then steady-state launches, on the same state array.  A grid record hands over by filling the
 * first four fields of a zeroed state (they ARE a gpsx_trk_state_t); the alignment of a 20 ms window with the data bit edge stays
 * the caller's business (the _hyb grid's guidance above).  No carrier aiding of the code loop in THIS call -- on real satellites
 * use gpsx_track_loop_weighted_aided / gpsx_track_loop_weighted_sync_aided below, which feed the slide forward; this definition
 * stays as it is for parity.  Unaided, a satellite's code slides by
 * fd x 0.01039 samples per second (fd / 1540 chips), the PI DLL follows that ramp with its integrator alone, and its discriminator
 * rests at d = fd x 0.01039 / dll_c2 -- with d(tau) = 16 tau / (64 + tau^2) at spacing 8, dll_c2 = 40 leaves the code 3.3 samples
 * behind at 2.7 kHz, d reaches 1 at |fd| = 3.85 kHz = dll_c2 x 96.25 Hz, and beyond that the code is lost.  On satellites on
 * orbits (tests/test_weighted_pvt_reference.py, |fd| up to 2.9 kHz) the steady gains dll = (0.5, 200) at n_coh = 20 hold the lag
 * to 0.6 samples and the fix of four channels to 35 m, where (0.5, 40) gives 125 m.
 *
 * Definition, for window u of a channel.  Every float operation is one IEEE single operation in the order written: no
 * contraction, correctly rounded division.
 *   correlators    for the window's blocks b = 0 .. n_coh - 1 the six int32 values gpsx_track_epl_weighted returns for the state at
 *                  the window's start: tau, f = (float)if_hz + if_freq_offset_hz and step32 constant over the window,
 *                  acc_b = if_freq_accum + b * 511 * step32; summed over b (|sum| <= 20 x 49 056).  if_freq_accum then advances by
 *                  n_coh * 511 * step32 (the step of the window just processed)
 *   DLL            e2 = IE^2 + QE^2, l2 = IL^2 + QL^2 in int64; d = (e2 + l2 == 0) ? 0 : (float)(e2 - l2) / (float)(e2 + l2)
 *                  (int64 -> float rounds to nearest even); d > 0: tau is too large.  T = (float)n_coh * 0.001f;
 *                  code_phase_fine = code_phase_fine - (dll_c1 * (d - dll_err) + (dll_c2 * T) * d); one wrap towards [0, 16368):
 *                  + 16368.0f if negative, - 16368.0f if >= 16368.0f; dll_err = d.  The wrap's own sum can round to 16368.0f (a
 *                  difference in about (-2^-11, 0)): that phase is used as tau = 0 by the next window, and gpsx_wobs treats a
 *                  record that carries it as one without a phase
 *   Costas PLL     IP == 0: p = QP > 0 ? 0.25f : QP < 0 ? -0.25f : 0; else p = atanf((float)QP / (float)IP) * 0.15915494f
 *                  (cycles; atanf is glibc <= 2.40's fdlibm one, operation by operation); insensitive to data bits
 *   FLL            only if fll_c != 0 and n_updates > 0: cross = prev_ip * QP - prev_qp * IP, dot = prev_ip * IP + prev_qp * QP in
 *                  int64; fe = (dot == 0) ? 0 : atanf((float)cross / (float)dot) * 0.15915494f / T (Hz); otherwise fe = 0
 *   carrier        if_freq_offset_hz = if_freq_offset_hz - ((pll_c1 * (p - pll_err) + (pll_c2 * T) * p) + fll_c * fe)
 *   end of window  pll_err = p; prev_ip = IP; prev_qp = QP; n_updates++; then the record is written
 * The int64 expressions above (e2, l2, cross, dot) are exact while the window sums, prev_ip and prev_qp have magnitudes <= 2^30;
 * sums the call forms itself stay below 2^20, so only a caller's state (gpsx_wsync_state_t's win_iq, prev_ip, prev_qp) can exceed that.
 * The loop rests at if_freq_offset_hz ~ fd (1 + 1/1022): the NCO mixes 16 352 of a block's 16 368 samples, so the accumulator loses
 * 16 samples of phase per block (as in the grids) and the loop makes that up in frequency.
 * Errors: NULL pointers, weights / spacing / n_coh out of range, n_blocks outside 1 .. 4096 or not a multiple of n_coh, n_ch < 1 and
 * a gain that is not finite return GPSX_EINVAL (with a gpsx_last_error text) and write nothing.  Channels are validated BY THE
 * KERNEL with gpsx_track_epl_weighted's policy, window by window: while a channel's prn is outside 1 .. 210 or its code_phase_fine is
 * not finite or has magnitude >= 2^24, its window's iq is zero, its floats and loop memory stay as they were, its accumulator IS
 * advanced, and GPSX_EINVAL comes from gpsx_track_loop_weighted after its wait / from the next gpsx_synchronize() after _dev.
 * The host variant takes blocks and records in host memory and the state on the device, as gpsx_track_loop does. */
typedef struct {                 /* 40 bytes, device resident */
  int32_t  prn;                  /* the first 16 bytes ARE a gpsx_trk_state_t: a grid record hands over by filling these four */
  float    code_phase_fine;
  float    if_freq_offset_hz;
  uint32_t if_freq_accum;
  float    dll_err, pll_err;     /* the previous window's discriminator outputs */
  int32_t  prev_ip, prev_qp;     /* the previous window's summed prompt (FLL) */
  uint32_t n_updates;            /* windows processed so far; 0 = no previous prompt */
  uint32_t reserved;             /* 0 */
} gpsx_wloop_state_t;

typedef struct {
  int32_t weights;               /* GPSX_WEIGHTS_SIGN_MAGNITUDE or GPSX_WEIGHTS_SIGN_ONLY */
  int32_t spacing;               /* 1 .. 15, as gpsx_trk_weighted_t */
  int32_t n_coh;                 /* blocks summed coherently before each loop update, 1 .. 20 */
  float   dll_c1, dll_c2;        /* the reference's PI form; its values are 1, 300 */
  float   pll_c1, pll_c2;        /* the reference's are 4, 3000 (8, 5000 after bit sync) */
  float   fll_c;                 /* 0 = no frequency loop */
} gpsx_wloop_cfg_t;

typedef struct {                 /* 36 bytes, one per (window, channel) */
  int32_t  iq[6];                /* IE, QE, IP, QP, IL, QL summed over the window's n_coh blocks, exact */
  float    code_phase_fine, if_freq_offset_hz;   /* AFTER this window's update */
  uint32_t if_freq_accum;        /* after the window's last block */
} gpsx_wloop_rec_t;

/* d_rec / rec: [n_blocks / n_coh][n_ch] */
int gpsx_track_loop_weighted_dev(gpsx_ctx *ctx, const gpsx_wloop_cfg_t *cfg, const void *d_if_blocks_2bit, int n_blocks,
                                 gpsx_wloop_state_t *d_state, int n_ch, gpsx_wloop_rec_t *d_rec);
int gpsx_track_loop_weighted(gpsx_ctx *ctx, const gpsx_wloop_cfg_t *cfg, const uint8_t *if_blocks_2bit, int n_blocks,
                             gpsx_wloop_state_t *d_state, int n_ch, gpsx_wloop_rec_t *rec);

/* ---- EXTENSION, not in the reference: the weighted loop with a per-channel 20 ms bit synchroniser and bit-aligned windows ------
 * gpsx_track_loop_weighted with what it leaves to the caller done on the device, channel by channel: every channel runs short
 * coherent windows (n_coh_search blocks, the `search` gains) while a bit synchroniser looks for the position of its data bit edge
 * in a 20 ms grid; once two consecutive rounds agree it waits for that edge and from then on runs windows of n_coh_lock blocks (the
 * `lock` gains) that never straddle a bit edge, and reports the sum of the prompts over every bit.  The open window lives in the
 * state, so a launch may be cut anywhere: n_blocks is 1 .. 4096 and no multiple of anything, and launches of any lengths give the
 * states and records of one launch over the same blocks.  gpsx_track_loop_weighted, its structs and its kernel are unchanged.
 *
 * Bit sync is NOT a presence detector: on noise alone two rounds agree with probability 1 / 20 and the energy ratio reaches what
 * weak signals give.  The caller decides whether a satellite is there (acquisition, the records' prompt energy) and re-arms a
 * search by writing mode = 0 into the state (search_n = 0 and prev_best_p1 = 0 with it for a fresh one).  gpsx_wlock below makes
 * that decision on the device from the records, and with its `rearm` does the writes.
 *
 * Definition, per channel and block b = 0 .. n_blocks - 1 of the launch, in this order.  Float operations as above: one IEEE
 * single operation each in the order written.  "The mode's" n_coh and gains: n_coh_search / `search` in SEARCH, n_coh_lock /
 * `lock` in LOCKED.
 *   1 validation   at the launch's start and after every window's end the channel is checked: prn in 1 .. 210, code_phase_fine
 *                  finite with magnitude < 2^24 (gpsx_track_loop_weighted's policy), and -- at the launch's start, where they
 *                  come from the caller -- mode in 0 .. 2, ms_count and edge in 0 .. 19, win_n in 0 .. 20, search_n in 0 .. 4020.
 *                  A channel that fails is BAD for the rest of the launch: per block only if_freq_accum += 511 * step32 happens;
 *                  it gets no window record (its slots are the empty pattern: zero sums), its floats, loop memory, window and
 *                  sync words stay as they were, and GPSX_EINVAL comes from gpsx_track_loop_weighted_sync after its wait / from
 *                  the next gpsx_synchronize() after _dev.  Steps 2 .. 7 are those of a good channel.  A prn of GPSX_PRN_NONE
 *                  (defined with gpsx_track_loop_weighted_sync_multi below) is a slot without a channel: treated like a BAD
 *                  channel in every byte, but never reported -- no GPSX_EINVAL.
 *   2 leaving WAIT if mode == WAIT and ms_count == edge: mode = LOCKED (this block is the first of a data bit)
 *   3 correlators  if mode != WAIT: the six int32 values of gpsx_track_epl_weighted for this block, with tau, f = (float)if_hz +
 *                  if_freq_offset_hz and step32 those of the state's floats -- which change at a window's end only, so a window
 *                  that continues over launches sees the same values -- and acc = if_freq_accum; they are added to win_iq and
 *                  win_n++.  In every mode if_freq_accum += 511 * step32
 *   4 counter      ms_count = (ms_count + 1) % 20
 *   5 search       in SEARCH only: p_i += IP_b, p_q += QP_b (this block's prompt; int32, wrapping); c = ms_count;
 *                  if search_n >= 20: e[c] += (int64)di * di + (int64)dq * dq with di = p_i - base[c][0], dq = p_q - base[c][1]
 *                  (int32, wrapping; the sum wraps modulo 2^64 -- neither happens from a zeroed search); base[c] = p; search_n++.
 *                  e[c] is the energy of the 20-block sums that START where ms_count == c
 *   6 window end   if mode != WAIT and (win_n >= the mode's n_coh, or mode == LOCKED and ms_count == edge -- which keeps bits
 *                  aligned whatever cfg did between launches): the DLL / Costas PLL / FLL / carrier / end-of-window arithmetic of
 *                  gpsx_track_loop_weighted above, verbatim, on win_iq with the mode's gains and T = (float)win_n * 0.001f.
 *                  In LOCKED bit_ip += IP (the window's), and if ms_count == edge the record gets GPSX_WSYNC_BIT and bit_ip, then
 *                  bit_ip = 0.  The record is written with GPSX_WSYNC_WINDOW (and GPSX_WSYNC_LOCKED in LOCKED), its first 36
 *                  bytes formed as gpsx_track_loop_weighted forms them; win_iq = 0, win_n = 0
 *   7 decision     in SEARCH when search_n >= 20 * (sync_bits + 1) (== in a run with one sync_bits): best = the lowest index of
 *                  the maximum of e[], opp = e[(best + 10) % 20]; accept iff best + 1 == prev_best_p1 and e[best] * sync_den >=
 *                  opp * sync_num (int64; from a zeroed search below 2^63 by the bounds on sync_bits and sync_num).  Always:
 *                  last_best_e = e[best], last_opp_e = opp, prev_best_p1 = best + 1, sync_rounds++, e[] = 0, p = 0, search_n = 0
 *                  (base[] is overwritten before it is read again).  On accept: edge = best, mode = WAIT, the open window is
 *                  discarded (win_iq = 0, win_n = 0, bit_ip = 0) and loop.n_updates = 0, so that the first locked window has no
 *                  FLL term from a window of another length; dll_err and pll_err stay.
 * prev_best_p1 holds the previous round's best + 1 and 0 for "none", so that a zeroed state has no predecessor and its first
 * decision is always a rejection: agreement of two consecutive rounds is the gate, the ratio only refuses flat rounds.
 * Records: rec[n_slots][n_ch] with span = min(n_coh_search, n_coh_lock) and n_slots = ceil(n_blocks / span); a window that ends at
 * block b goes to slot b / span.  Window ends of a channel are at least span blocks apart (from states this call wrote, under one
 * cfg; should a caller's state make two fall into one slot, the later one stays), a slot in which none ended is zero with
 * end_block = -1: every byte of rec is written.
 * Errors: NULL pointers, weights / spacing out of range, n_coh_search or n_coh_lock not in {1, 2, 4, 5, 10, 20}, sync_bits
 * outside 1 .. 200, sync_num or sync_den outside 1 .. 1024 or sync_num < sync_den, a gain that is not finite, n_blocks outside
 * 1 .. 4096, n_ch < 1 and a size that overflows return GPSX_EINVAL (with a gpsx_last_error text) and write nothing.
 * Vector ALU (k_track_wsync: k_track_wloop's shape with per-lane window ends).  The host variant takes blocks and records in host
 * memory and the state on the device, as gpsx_track_loop_weighted does. */
#define GPSX_WSYNC_SEARCH 0
#define GPSX_WSYNC_WAIT   1
#define GPSX_WSYNC_LOCKED 2
#define GPSX_WSYNC_WINDOW 1u     /* flags: the slot holds a window's record */
#define GPSX_WSYNC_LOCKED_FLAG 2u   /* the window ran in LOCKED */
#define GPSX_WSYNC_BIT    4u     /* the window's last block was a data bit's last: bit_ip is the bit's prompt sum */

typedef struct { float dll_c1, dll_c2, pll_c1, pll_c2, fll_c; } gpsx_wsync_gains_t;   /* as gpsx_wloop_cfg_t's */

typedef struct {                 /* 68 bytes */
  int32_t weights, spacing;      /* as gpsx_wloop_cfg_t */
  int32_t n_coh_search;          /* blocks per window in SEARCH: 1, 2, 4, 5, 10 or 20 */
  int32_t n_coh_lock;            /* blocks per window in LOCKED: 1, 2, 4, 5, 10 or 20 */
  gpsx_wsync_gains_t search, lock;
  int32_t sync_bits;             /* 20-block sums per candidate and round: 1 .. 200 */
  int32_t sync_num, sync_den;    /* accept needs e[best] / e[best + 10] >= sync_num / sync_den: 1 .. 1024, sync_num >= sync_den */
} gpsx_wsync_cfg_t;

typedef struct {                 /* 448 bytes, device resident; zeroed with loop's first four fields filled: a handover */
  gpsx_wloop_state_t loop;       /*   0  (reserved: 0) */
  int32_t  win_iq[6];            /*  40  the open window's sums IE, QE, IP, QP, IL, QL */
  int32_t  win_n;                /*  64  blocks in the open window */
  int32_t  ms_count;             /*  68  0 .. 19: the 20 ms grid the edge is counted in */
  int32_t  mode;                 /*  72  GPSX_WSYNC_SEARCH / _WAIT / _LOCKED */
  int32_t  edge;                 /*  76  0 .. 19: ms_count at a bit's first block; meaningful when mode != 0 */
  int32_t  bit_ip;               /*  80  the prompt sum of the open bit (LOCKED) */
  int32_t  search_n;             /*  84  blocks this search round has seen */
  int32_t  prev_best_p1;         /*  88  the previous round's best + 1; 0: none */
  int32_t  sync_rounds;          /*  92  decisions taken so far */
  int32_t  p_i, p_q;             /*  96  the round's running prompt sum */
  int64_t  last_best_e, last_opp_e;   /* 104  what the last decision compared */
  int32_t  zero[2];              /* 120  0 */
  int32_t  base[20][2];          /* 128  p when ms_count was c, 20 blocks ago */
  int64_t  e[20];                /* 288  per candidate: the energy of its 20-block sums this round */
} gpsx_wsync_state_t;

typedef struct {                 /* 48 bytes, one per (slot, channel) */
  gpsx_wloop_rec_t w;            /*  0  as gpsx_track_loop_weighted's record for this window */
  int32_t  end_block;            /* 36  the window's last block, counted from the launch's first; -1: no window ended in this slot */
  uint32_t flags;                /* 40  GPSX_WSYNC_WINDOW | GPSX_WSYNC_LOCKED_FLAG | GPSX_WSYNC_BIT */
  int32_t  bit_ip;               /* 44  with GPSX_WSYNC_BIT: the bit's prompt sum, its sign the data bit up to one polarity */
} gpsx_wsync_rec_t;

/* d_rec / rec: [ceil(n_blocks / min(n_coh_search, n_coh_lock))][n_ch] */
int gpsx_track_loop_weighted_sync_dev(gpsx_ctx *ctx, const gpsx_wsync_cfg_t *cfg, const void *d_if_blocks_2bit, int n_blocks,
                                      gpsx_wsync_state_t *d_state, int n_ch, gpsx_wsync_rec_t *d_rec);
int gpsx_track_loop_weighted_sync(gpsx_ctx *ctx, const gpsx_wsync_cfg_t *cfg, const uint8_t *if_blocks_2bit, int n_blocks,
                                  gpsx_wsync_state_t *d_state, int n_ch, gpsx_wsync_rec_t *rec);

/* ---- EXTENSION, not in the reference: carrier aiding of the weighted code loop ----------------------------------------------------
 * gpsx_track_loop_weighted and gpsx_track_loop_weighted_sync with ONE clause added to the DLL step of the window update: the code's
 * slide, which the carrier loop knows from its own offset, is fed forward, so that the PI DLL no longer has to follow the ramp with
 * its integrator.  An opt-in: the four unaided calls, their structs, their definitions and their kernels are unchanged, and cfg,
 * state, record, slot and launch-cut rules, channel validation and the errors of the aided calls are the unaided calls' to the letter.
 *
 * Definition.  In the DLL step (float operations as above: one IEEE single operation each in the order written, no contraction)
 *   phase = code_phase_fine - (dll_c1 * (d - dll_err) + (dll_c2 * T) * d)                     (as in the unaided call)
 *   if code_per_hz != 0.0f:  phase = phase - (code_per_hz * if_freq_offset_hz) * T
 *   one wrap towards [0, 16368) as in the unaided call, on that phase; code_phase_fine = phase; dll_err = d
 * if_freq_offset_hz is the value the window's correlators ran with: the state's BEFORE this window's carrier step.  T is the
 * window's own ((float)n_coh * 0.001f; in _sync (float)win_n * 0.001f), and in _sync the same factor serves SEARCH and LOCKED
 * windows.  With code_per_hz == 0.0f the term is not formed and the call returns the unaided call's bytes.  A bad channel takes no
 * step (its floats stay as they were).  For GPS L1 C/A at this sampling rate the factor is GPSX_WAID_L1CA: a Doppler of fd Hz
 * moves the code by fd x 16 / 1540 samples per second towards smaller code_phase_fine.
 * Rounding: the step is rounded into the phase, whose ulp is at most 2^-10 sample (phases of 8192 and above), so what a window's
 * step loses is at most 2^-11 sample; nothing accumulates the remainders, the DLL sees them as part of its error.
 * No step is taken while a _sync channel sits in WAIT (no window ends there): in up to 19 blocks the code slides by up to one
 * sample at 5 kHz, and the DLL takes that back in the first locked windows.
 * Which instant the recorded phase belongs to: the DLL zeroes the code error averaged over a window, and the step for window u is
 * taken at its end, so the recorded code_phase_fine is the phase for the MIDDLE of the window that follows, seen from the record's
 * instant (the window's end): against the true delay at that instant it is offset by about half a window's slide,
 * 0.5 x fd x 0.01039 x T samples (0.28 at 2.7 kHz and T = 20 ms, 0.47 at 4.5 kHz), towards smaller phases for positive fd.
 * Measured on the restatement, one satellite at +4500 / -4500 Hz, steady gains (0.5, 40), T = 20 ms: the recorded phase minus the true
 * delay at the record's instant is +0.40 / +1.50 samples in the mean, and +0.87 / +1.03 against the delay half a window later -- the
 * half-window term on either side of an offset of about 0.95 samples that all Dopplers share and a fix's clock term takes; the
 * largest error at the record's instant is 0.77 / 1.90 samples (tests/weighted_aided_cases.py MEASURED; EXPERIMENTS.md "Carrier
 * aiding of the weighted code loop").  gpsx_wobs is unchanged and does not take this term out.
 * Errors: the unaided call's, and with them: aid NULL ("null argument"), code_per_hz not finite or of magnitude above 1,
 * reserved != 0: GPSX_EINVAL with a gpsx_last_error text, nothing written.
 * Vector ALU (k_track_waid_loop, k_track_waid_sync: the bodies of k_track_wloop and k_track_wsync instantiated with the clause; the
 * same launch plan and resources). */
#define GPSX_WAID_L1CA 0.010389610f          /* 16 samples per chip / 1540 carrier cycles per chip */
typedef struct {
  float   code_per_hz;           /* samples of code phase per second and Hz of carrier offset; |.| <= 1; 0: no aiding */
  int32_t reserved;              /* 0 */
} gpsx_waid_t;

int gpsx_track_loop_weighted_aided_dev(gpsx_ctx *ctx, const gpsx_wloop_cfg_t *cfg, const gpsx_waid_t *aid, const void *d_if_blocks_2bit,
                                       int n_blocks, gpsx_wloop_state_t *d_state, int n_ch, gpsx_wloop_rec_t *d_rec);
int gpsx_track_loop_weighted_aided(gpsx_ctx *ctx, const gpsx_wloop_cfg_t *cfg, const gpsx_waid_t *aid, const uint8_t *if_blocks_2bit,
                                   int n_blocks, gpsx_wloop_state_t *d_state, int n_ch, gpsx_wloop_rec_t *rec);
int gpsx_track_loop_weighted_sync_aided_dev(gpsx_ctx *ctx, const gpsx_wsync_cfg_t *cfg, const gpsx_waid_t *aid, const void *d_if_blocks_2bit,
                                            int n_blocks, gpsx_wsync_state_t *d_state, int n_ch, gpsx_wsync_rec_t *d_rec);
int gpsx_track_loop_weighted_sync_aided(gpsx_ctx *ctx, const gpsx_wsync_cfg_t *cfg, const gpsx_waid_t *aid, const uint8_t *if_blocks_2bit,
                                        int n_blocks, gpsx_wsync_state_t *d_state, int n_ch, gpsx_wsync_rec_t *rec);

/* ---- EXTENSION, not in the reference: the sync loop for many receivers per launch, one IF stream each -------------------------------
 * gpsx_track_loop_weighted_sync(_aided) takes ONE stream, shared by all channels.  This call takes n_rx streams with ch_per_rx
 * channel slots on each, in one launch.  No arithmetic is new: receiver r's bytes ARE, by definition, the single-stream call's on
 * its stream.  The four single-stream calls, their structs, their kernels and GPSX_VERSION are unchanged.
 *
 * Definition.  Channel r * ch_per_rx + j is slot j of receiver r; n_ch = n_rx * ch_per_rx; d_state[n_ch] and d_rec[n_slots][n_ch]
 * (n_slots as above) are the single-stream call's arrays, so gpsx_wnav_words, gpsx_wobs, gpsx_weph and gpsx_wlock read them
 * unchanged with that n_ch.  Receiver r reads blocks b = 0 .. n_blocks - 1 at byte offset ((size_t)r * rx_stride_blocks + b) * 4092
 * of d_if_blocks_2bit and no byte outside them (of a block, bytes 0 .. 4087: the sixteen unmixed samples are not read).  After the
 * call the states [r * ch_per_rx, (r + 1) * ch_per_rx) and the matching record columns equal, byte for byte, what
 * gpsx_track_loop_weighted_sync_aided writes for that receiver's blocks, those ch_per_rx states and the same cfg and aid; with
 * aid == NULL, or a factor of 0, what gpsx_track_loop_weighted_sync writes.  The launch-cut rule carries over (launches of any
 * lengths give the bytes of one launch; a later launch starts from the pointer advanced by its predecessor's blocks, the stride
 * unchanged), and so do the empty-slot pattern and the BAD-channel policy: a bad channel of any receiver makes the call, or the
 * next gpsx_synchronize after _dev, return GPSX_EINVAL and changes nothing in any other channel or receiver.
 * A receiver with fewer than ch_per_rx satellites fills its spare slots with prn = GPSX_PRN_NONE (below).
 * Errors: the single-stream call's, in its order, with these in the place of its n_ch clause: rx NULL ("null argument", with the
 * other pointers), n_rx outside 1 .. 1 048 576, ch_per_rx outside 1 .. 64, rx_stride_blocks < n_blocks, reserved != 0,
 * n_rx * ch_per_rx above INT32_MAX; and behind the others a byte count (records, states, streams) that overflows size_t.  Each
 * returns GPSX_EINVAL with a gpsx_last_error text and writes nothing.
 * Vector ALU (k_track_wsync_multi: k_track_waid_sync's text with a workgroup of four waves per receiver, which stages only that
 * receiver's block; wave w serves slots w * cpw .. + cpw - 1, cpw = ceil(ch_per_rx / 4) -- hence 64 slots at most).  The host
 * variant takes the streams (the same stride) and the records in host memory and the state on the device; what the arena cannot
 * hold is refused with the arena's error.
 *
 * GPSX_PRN_NONE: a channel slot that holds no channel.  It names what every weighted tracking kernel already does with this prn
 * value (the padding channel of the validation rules above): the slot gets no correlators and no window record, its record slots
 * are the empty pattern, it is NOT reported as bad, and per block only its if_freq_accum moves (+= 511 * step32, as a bad
 * channel's). */
#define GPSX_PRN_NONE (-2147483647 - 1)   /* a channel slot that holds no channel */

typedef struct {                 /* 16 bytes */
  int32_t n_rx;                  /* receivers (IF streams): 1 .. 1 048 576 */
  int32_t ch_per_rx;             /* channel slots per receiver: 1 .. 64 */
  int32_t rx_stride_blocks;      /* 4092-byte blocks between two receivers' first blocks: >= n_blocks */
  int32_t reserved;              /* 0 */
} gpsx_wmulti_t;

/* aid NULL: unaided.  d_state [n_rx * ch_per_rx]; d_rec / rec: [ceil(n_blocks / min(n_coh_search, n_coh_lock))][n_rx * ch_per_rx] */
int gpsx_track_loop_weighted_sync_multi_dev(gpsx_ctx *ctx, const gpsx_wsync_cfg_t *cfg, const gpsx_waid_t *aid, const gpsx_wmulti_t *rx,
                                            const void *d_if_blocks_2bit, int n_blocks, gpsx_wsync_state_t *d_state, gpsx_wsync_rec_t *d_rec);
int gpsx_track_loop_weighted_sync_multi(gpsx_ctx *ctx, const gpsx_wsync_cfg_t *cfg, const gpsx_waid_t *aid, const gpsx_wmulti_t *rx,
                                        const uint8_t *if_blocks_2bit, int n_blocks, gpsx_wsync_state_t *d_state, gpsx_wsync_rec_t *rec);

/* ---- EXTENSION, not in the reference: LNAV frame sync and parity-checked words from the sync loop's bit records -----------------
 * What lies between a BIT record of gpsx_track_loop_weighted_sync and a navigation word, done on the device: a kernel reads the
 * loop's records where they are (d_rec, in HBM), keeps a 64-byte frame state per channel and returns parity-checked 30-bit words
 * only, 16 bytes each and at most n_blocks / 600 + 2 per channel and launch.  Unlike the reference's word layer it does not accept
 * a bare preamble: a channel synchronises on TLM + HOW as a whole (62 consecutive bits: two parity-checked words, the preamble,
 * the HOW's two zero bits and a subframe ID of 1 .. 5), in either polarity, and the polarity is what that test found.
 * gpsx_track_loop_weighted_sync, its structs and k_track_wsync are unchanged.
 *
 * Parity: the six equations of IS-GPS-200 table 20-XIV (kParityMask / kParityFromD30 of gpsx_steps.cpp).  For a received 30-bit
 * word W (its first bit in bit 29) and the two bits P29, P30 received before it: d = (W >> 6) ^ (P30 ? 0xFFFFFF : 0) are the source
 * bits d1 .. d24 (d1 in bit 23), and the word passes iff for k = 0 .. 5 bit 5 - k of W equals parity(d & mask_k) ^ (P29 for k = 0,
 * 2, 5; P30 for k = 1, 3, 4).  The test is invariant under inversion of the whole stream, and so is d.
 *
 * Definition, per channel: the slots of d_rec are read in order.  A record is a BIT if its flags have GPSX_WSYNC_WINDOW and
 * GPSX_WSYNC_BIT and 0 <= end_block < n_blocks; every other record is skipped.  For a bit, with E = blocks_seen + end_block:
 *   1 continuity   if last_bit_end_p1 != 0 and E + 1 != last_bit_end_p1 + 20 the stream broke (a re-armed search, another edge, a
 *                  gap): n_drop++ if mode == SYNCED; then mode = HUNT and fresh = word_idx = bit_idx = bad_run = ok_mask = 0.
 *                  In every case last_bit_end_p1 = E + 1
 *   2 shift        r = bit_ip < 0 (bit 0 is a positive prompt); hist = hist << 1 | r; fresh = min(fresh + 1, 62)
 *   3 HUNT         (mode == HUNT) only when fresh == 62: for inv' = 0, then 1, with x = hist ^ (inv' ? ~0 : 0), bits 61 and 60 of x
 *                  are D29*, D30*, bits 59 .. 30 word 1, bits 29 .. 0 word 2.  The first inv' is accepted for which word 1's first
 *                  eight bits are 10001011, word 1 passes parity against D29*, D30*, word 2 passes against word 1's last two
 *                  bits, word 2's last two bits are 0 and its source bits d20 .. d22 give an ID in 1 .. 5.  On accept: inv = inv',
 *                  mode = SYNCED, word_idx = 2, bit_idx = 0, bad_run = 0, ok_mask = 3 | ID << 16, n_sync++, and two records go out:
 *                  index 1 with end_block - 600 (which may be negative: the word ended before this launch; flags == 0 is what
 *                  marks an empty slot), then index 2 with end_block; both GPSX_WNAV_WORD | _OK | _SYNC (| _INVERTED if inv), both
 *                  with the ID, index 2 with the TOW count.  The bit is done
 *   4 SYNCED       (mode == SYNCED when the bit came, after step 1) bit_idx++; at 30 the word word_idx + 1 is complete: W = the
 *                  newest 30 bits of hist, P29 / P30 bits 31 / 30 of hist; passed = parity.  Word 1: with t = the first eight
 *                  bits of W ^ (inv ? ~0 : 0): t == 01110100 and passed: inv ^= 1 and the record gets _FLIPPED; t neither that nor
 *                  10001011: passed = 0 (an inverted preamble on a word that fails parity fails and flips nothing).  Word 2
 *                  passes only if it also ends in two zero bits and has an ID in 1 .. 5 (both after inv); the ID kept for the
 *                  subframe's records (ok_mask bits 16 .. 18) is that ID if word 2 passed, else 0.  The record: index, the word as
 *                  below with the inv that holds now, _WORD (| _OK if passed) (| _INVERTED if inv), the kept ID (0 for word 1: its
 *                  HOW is yet to come), aux = the TOW count (d1 .. d17 of word 2) for index 2 with _OK.  ok_mask |= passed << (index
 *                  - 1); bad_run = passed ? 0 : min(bad_run + 1, 10); bit_idx = 0; word_idx = (word_idx + 1) % 10.  After word 10:
 *                  _SUBFRAME and n_subframes++ if ok_mask's bits 0 .. 9 are all set, then ok_mask = 0.  Then, if bad_run >=
 *                  max_bad_words: _DROPPED, n_drop++, mode = HUNT, fresh = 0, word_idx = 0.
 * A record's word: x = W ^ (inv ? 0x3FFFFFFF : 0); bits 29 .. 6 = d1 .. d24 (the source bits: polarity and D30* removed -- the d of
 * the parity test), bits 5 .. 0 = x's D25 .. D30.  That is the word as gps_nav_data_decode_subframe's image holds it.
 * Output: a channel's records go to its slots 0, 1, .. of d_words[n_blocks / 600 + 2][n_ch] in order of completion; the remaining
 * slots get the empty pattern (end_block = -1, the rest 0): every byte of d_words is written.  The bound holds for any input: bits
 * count as consecutive only 20 blocks apart, a word needs 30 consecutive bits (600 blocks) and a sync, which yields two words,
 * 62 fresh ones (1220 blocks); the "+ 2" is a launch that begins one bit before a sync or a word's end.  At the launch's end
 * blocks_seen += n_blocks.
 * What can be trusted: parity is blind to the inversion of a whole word, and so are the source bits: d = D ^ D30* comes out the
 * same in either polarity.  After a half-cycle slip of the carrier loop the word the slip fell into fails (none, on a word boundary), the words up to the
 * next TLM pass with the right d1 .. d24 but under the OLD polarity: their six parity bits in `word` and their _INVERTED flag are
 * inverted until the TLM gets _FLIPPED.  Words 1 and 2 are the only ones whose test sees the polarity.  A consumer of whole
 * subframes takes the ten words that end with a word 10 flagged _SUBFRAME; a _FLIPPED TLM says that a slip lies in the subframe
 * before it.
 * Errors: NULL pointers, max_bad_words outside 1 .. 10, reserved != 0, n_blocks outside 1 .. 4096, n_slots outside 1 .. n_blocks,
 * n_ch < 1 and a size that overflows return GPSX_EINVAL (with a gpsx_last_error text) and write nothing.  A channel whose state is
 * out of range -- mode outside 0 .. 1, inv outside 0 .. 1, word_idx outside 0 .. 9, bit_idx outside 0 .. 29, fresh outside 0 .. 62,
 * bad_run outside 0 .. 10, blocks_seen or last_bit_end_p1 outside 0 .. 2^62 (E + 1 is then never 0, the value that means "no bit
 * yet", which the slot bound rests on) -- is BAD as gpsx_track_loop_weighted_sync's are: its state stays as it was, its slots are
 * empty, and GPSX_EINVAL comes from gpsx_wnav_words after its wait / from the next gpsx_synchronize() after _dev.
 * Vector ALU (k_wnav_words: one channel per lane, the records' three words loaded eight slots ahead of the recurrence).  On one
 * stream: gpsx_track_loop_weighted_sync_dev, then gpsx_wnav_words_dev on its d_rec with the same n_blocks and n_slots =
 * ceil(n_blocks / min(n_coh_search, n_coh_lock)). */
#define GPSX_WNAV_HUNT      0
#define GPSX_WNAV_SYNCED    1
#define GPSX_WNAV_WORD      1u   /* flags: the slot holds a word */
#define GPSX_WNAV_OK        2u   /* it passed parity (and, words 1 and 2, what is asked of a TLM / HOW) */
#define GPSX_WNAV_INVERTED  4u   /* the received polarity was inverted (removed in `word`) */
#define GPSX_WNAV_SYNC      8u   /* words 1 and 2 of the TLM + HOW test that took the channel from HUNT to SYNCED */
#define GPSX_WNAV_FLIPPED   16u  /* word 1 showed the inverted preamble and passed: the polarity changed with this word */
#define GPSX_WNAV_SUBFRAME  32u  /* word 10 of a subframe all of whose ten words passed */
#define GPSX_WNAV_DROPPED   64u  /* max_bad_words consecutive words failed: the channel is back in HUNT */

typedef struct {
  int32_t max_bad_words;         /* 1 .. 10: consecutive failed words that drop a channel back to HUNT */
  int32_t reserved;              /* 0 */
} gpsx_wnav_cfg_t;

typedef struct {                 /* 64 bytes, device resident; all zero = a fresh channel */
  uint64_t hist;                 /*  0  received hard bits, newest in bit 0, polarity as received */
  int64_t  blocks_seen;          /*  8  blocks of all earlier launches: the absolute time base */
  int64_t  last_bit_end_p1;      /* 16  absolute last block of the newest bit, + 1; 0: none yet */
  int32_t  fresh;                /* 24  consecutive bits in hist since the last reset, saturating at 62 */
  int32_t  mode;                 /* 28  GPSX_WNAV_HUNT / GPSX_WNAV_SYNCED */
  int32_t  inv;                  /* 32  0 / 1: received polarity is inverted */
  int32_t  word_idx;             /* 36  words of the current subframe completed, 0 .. 9 */
  int32_t  bit_idx;              /* 40  bits of the current word, 0 .. 29 */
  int32_t  bad_run;              /* 44  consecutive failed words */
  uint32_t ok_mask;              /* 48  bit w (0 .. 9): word w + 1 of the current subframe passed; bits 16 .. 18: its ID from the
                                  *     HOW if that passed, else 0 (what later words' records report) */
  uint32_t n_sync, n_drop, n_subframes;   /* 52  counters */
} gpsx_wnav_state_t;

typedef struct {                 /* 16 bytes, one per (word slot, channel) */
  int32_t  end_block;            /*  0  last block of the word's last bit, from the launch's first block; empty slot: -1 */
  uint32_t word;                 /*  4  bit 29 = d1 .. bit 6 = d24 (source bits), bits 5 .. 0 = D25 .. D30 (polarity removed) */
  uint8_t  index;                /*  8  1 .. 10 */
  uint8_t  flags;                /*  9  GPSX_WNAV_WORD | ...; empty slot: 0 */
  uint8_t  subframe_id;          /* 10  from the current subframe's HOW if it passed, else 0 */
  uint8_t  zero;                 /* 11 */
  uint32_t aux;                  /* 12  index 2 with GPSX_WNAV_OK: the 17-bit TOW count; else 0 */
} gpsx_wnav_word_t;

/* d_rec: what gpsx_track_loop_weighted_sync(_dev) wrote for n_blocks blocks, [n_slots][n_ch], on the device in both variants;
 * d_words / words: [n_blocks / 600 + 2][n_ch] */
int gpsx_wnav_words_dev(gpsx_ctx *ctx, const gpsx_wnav_cfg_t *cfg, const gpsx_wsync_rec_t *d_rec, int n_slots, int n_blocks,
                        gpsx_wnav_state_t *d_state, int n_ch, gpsx_wnav_word_t *d_words);
int gpsx_wnav_words(gpsx_ctx *ctx, const gpsx_wnav_cfg_t *cfg, const gpsx_wsync_rec_t *d_rec, int n_slots, int n_blocks,
                    gpsx_wnav_state_t *d_state, int n_ch, gpsx_wnav_word_t *words /* host */);
/* host only, no GPU: ten records of one subframe (index 1 .. 10 in this order, all GPSX_WNAV_OK; GPSX_EINVAL otherwise, and for
 * NULL) -> the 38-byte image gps_nav_data_decode_subframe reads (bit n of the subframe = bit n & 7 of byte n >> 3; the image's
 * last four bits are 0). */
int gpsx_wnav_subframe_image(const gpsx_wnav_word_t *ten, uint8_t image[38]);

/* ---- EXTENSION, not in the reference: weighted observables -- every channel's transmit time at the launch's end, on the device ----
 * What a receiver needs next on the weighted path: for every channel, the transmit time of the signal that arrives at one common
 * receiver instant -- here the first sample of the block that follows the launch.  Pseudoranges are differences of such times.
 * gpsx_wobs(_dev) is a fourth stage behind gpsx_track_loop_weighted_sync_dev and gpsx_wnav_words_dev: a kernel reads the two
 * arrays those left in HBM -- the window records d_rec[n_slots][n_ch] and the word records d_words[n_blocks / 600 + 2][n_ch] --
 * keeps an 80-byte state per channel and returns one 32-byte observable per channel and launch: a whole millisecond of the GPS
 * week, the code phase that goes with it, and flags that say what the number rests on.  Nothing existing changes.
 *
 * The time base: a channel's bit edges lie at absolute sample code_phase + 16368 (Z + 20 j) of the stream, Z = edge_block.  The
 * sync loop places a bit's end on a block; the true edge lies code_phase samples into the block after it (code phase below half
 * a block) or into that very block (at or above): "nearest block start".  A parity-checked HOW then says which millisecond of
 * the week the edge of block Z is: Tz.  Two things move afterwards and are followed from the window records alone:
 *   the seam       a channel whose code phase crosses the ends of the 16 368-sample circle moves its code-period boundary across a
 *                  block boundary: the phase jumps by nearly a block, and Z moves by one the other way.  k_track_wsync keeps its
 *                  ms_count through such a wrap, so the loop state's `edge` does not say which millisecond an edge is in; Z does.
 *   breaks         a SEARCH window or a bit that does not end 20 blocks after its predecessor ends the chain: EDGE and TOW go,
 *                  and the next bit starts another.
 *
 * Definition, per channel; every float operation is one IEEE single operation.
 * Pass 1: the slots of d_rec are read in order.  A record counts if its flags have GPSX_WSYNC_WINDOW, 0 <= end_block < n_blocks
 * and its p = w.code_phase_fine satisfies p >= 0.0f && p < 16368.0f (a NaN does not); every other record is skipped.  For a
 * record that counts, with W = blocks_seen + end_block, in this order:
 *   1 SEARCH       (no GPSX_WSYNC_LOCKED_FLAG) n_break++ if EDGE is set; EDGE, TOW, CONFIRMED and AMBIGUOUS are cleared;
 *                  last_bit_end_p1 = 0
 *   2 wrap         if EDGE and PHASE are set, with d = p - last_phase: d > 8184.0f: Z -= 1, n_wraps++; d < -8184.0f: Z += 1,
 *                  n_wraps++
 *   3 newest       last_phase = p, last_freq = w.if_freq_offset_hz, last_win_end_p1 = W + 1, PHASE is set
 *   4 bit          (GPSX_WSYNC_BIT and GPSX_WSYNC_LOCKED_FLAG) if last_bit_end_p1 != 0 and W + 1 != last_bit_end_p1 + 20 the chain
 *                  broke: n_break++ if EDGE is set, and EDGE, TOW, CONFIRMED, AMBIGUOUS are cleared.  If EDGE is not set (now):
 *                  Z = W + 1 - (p >= 8184.0f ? 1 : 0), chain_first_p1 = W + 1, EDGE is set, and AMBIGUOUS iff
 *                  fabsf(p - 8184.0f) < edge_guard.  Then last_bit_end_p1 = W + 1
 * Pass 2: the slots of d_words are read in order, on the state pass 1 left.  A record is used only if its flags have
 * GPSX_WNAV_WORD and GPSX_WNAV_OK, index == 2, aux < 100800, 0 <= end_block < n_blocks, EDGE is set, and with E = blocks_seen +
 * end_block: E + 1 >= chain_first_p1 + 1220, E + 1 <= last_bit_end_p1 and (last_bit_end_p1 - E - 1) % 20 == 0 (gpsx_wnav_words
 * needs 62 fresh bits for a HOW: one from before a break in the same launch cannot anchor the chain that came after it).  For a
 * used record: T = 6000 * ((aux + 100799) % 100800) + 1200 (the HOW's count is the next subframe's; word 2 ends 1.2 s into its
 * own), j = floor((E + 1 - Z + 10) / 20), r = E + 1 - Z - 20 j.  |r| > 5: n_mismatch++, the word is not used (the edge the words
 * stand on is not the chain's).  Otherwise Tc = (T - 20 j) mod 604 800 000, non-negative, and: no TOW yet: Tz = Tc, TOW is set,
 * n_anchor++; Tc == Tz: CONFIRMED is set; otherwise Tz = Tc, CONFIRMED is cleared, n_mismatch++.
 * Output: blocks_seen += n_blocks = B, and the observable as its struct says; every byte of d_obs is written.  The four
 * counters n_* wrap at 2^32.
 *
 * What the number is and is not.  tx_ms - code_phase_fine / 16368 ms is the transmit time of what arrives at sample 0 of block B,
 * but the code phase is that of the newest window's END, up to n_coh_lock blocks before B, and it is not extrapolated:
 * age_blocks says how old it is (the loop's drift over 20 ms is a few hundredths of a sample at 5 kHz of Doppler; a caller who
 * needs it extrapolates with if_freq_offset_hz / 1540 chips per second).  GPSX_WOBS_AMBIGUOUS says that the chain's edge was fixed with the
 * code phase within edge_guard samples of mid-block, where "nearest block start" is decided by the loop's noise: tx_ms may be
 * exactly 1 ms off, in either direction.  That is 300 km in a pseudorange -- try +-1 ms and let the solver's residuals decide.
 * It is reported, not resolved: resolving needs 1 ms prompts around the edge, which records of 20-block windows do not hold.
 * The call must be made on every launch of a stream, as gpsx_wnav_words must: blocks_seen is the time base, and a wrap between
 * two launches that were not both seen is a millisecond lost.
 * Where a stream is cut into launches does not matter to the observables, nor to the states but for this: pass 2 sees the state
 * as the launch left it.  A HOW that a break follows in its own launch anchors nothing, while with a cut between the two it
 * anchors the chain that then ends (n_anchor counts it, tx_ms_at_edge keeps it, no flag does); and r is taken against the Z of the
 * launch's end, which matters only to a channel that crosses the seam more than five times one way within one launch.
 * Errors: NULL pointers, an edge_guard that is not finite or outside 0 .. 8184, reserved != 0, n_blocks outside 1 .. 4096,
 * n_slots outside 1 .. n_blocks, n_ch < 1 and a size that overflows return GPSX_EINVAL (with a gpsx_last_error text) and write
 * nothing.  A channel is BAD if its state has flag bits other than GPSX_WOBS_PHASE .. _AMBIGUOUS or reserved != 0, if blocks_seen,
 * last_bit_end_p1, chain_first_p1 or last_win_end_p1 lies outside 0 .. 2^62, if |edge_block| > 2^62, if tx_ms_at_edge lies outside
 * 0 .. 604 799 999, or if last_phase is not in [0, 16368) while PHASE is set: its state stays as it was, its observable is all
 * zero with age_blocks = -1, and GPSX_EINVAL comes from gpsx_wobs after its wait / from the next gpsx_synchronize() after _dev.
 * Vector ALU (k_wobs: one channel per lane, a record's four words loaded eight slots ahead of the recurrence).  On one stream:
 * gpsx_track_loop_weighted_sync_dev, gpsx_wnav_words_dev, then gpsx_wobs_dev on their d_rec and d_words with the same n_blocks
 * and n_slots. */
#define GPSX_WOBS_PHASE      1u   /* a window record has been seen: code_phase_fine / if_freq_offset_hz are a record's */
#define GPSX_WOBS_EDGE       2u   /* an unbroken chain of bits is running and its edge block is known */
#define GPSX_WOBS_TOW        4u   /* a parity-checked HOW of this chain has anchored the time of week */
#define GPSX_WOBS_CONFIRMED  8u   /* a second HOW agreed with the anchor */
#define GPSX_WOBS_AMBIGUOUS 16u   /* the chain's edge was fixed with the code phase within edge_guard of mid-block: tx_ms may be 1 ms off */
#define GPSX_WOBS_VALID     32u   /* output only: PHASE, EDGE and TOW all hold */

typedef struct {
  float    edge_guard;           /* samples, 0 .. 8184, finite: |code phase - 8184| below it marks a new chain AMBIGUOUS (0: never) */
  int32_t  reserved;             /* 0 */
} gpsx_wobs_cfg_t;

typedef struct {                 /* 80 bytes, device resident; all zero = a fresh channel */
  int64_t  blocks_seen;          /*  0  blocks of all earlier launches */
  int64_t  last_bit_end_p1;      /*  8  absolute last block of the newest bit, + 1; 0: none */
  int64_t  chain_first_p1;       /* 16  the same for the first bit of the running chain */
  int64_t  edge_block;           /* 24  Z: the chain's bit edges are at absolute sample code_phase + 16368 (Z + 20 j) */
  int64_t  tx_ms_at_edge;        /* 32  Tz: transmit time, ms of week 0 .. 604 799 999, at the edge of block Z */
  int64_t  last_win_end_p1;      /* 40  absolute last block of the newest window record, + 1; 0: none */
  float    last_phase, last_freq;/* 48  that record's code_phase_fine, if_freq_offset_hz */
  uint32_t flags;                /* 56  GPSX_WOBS_PHASE .. _AMBIGUOUS */
  uint32_t n_wraps;              /* 60  seam crossings followed while a chain ran */
  uint32_t n_anchor, n_mismatch, n_break, reserved;   /* 64  HOWs that set Tz first; HOWs refused or contradicting; chains ended; 0 */
} gpsx_wobs_state_t;

typedef struct {                 /* 32 bytes, one per channel and launch */
  int64_t  tx_ms;                /*  0  with VALID: (Tz + B - Z) mod 604 800 000, B = blocks_seen + n_blocks after this launch; else 0 */
  float    code_phase_fine;      /*  8  transmit time at sample 0 of block B = tx_ms - code_phase_fine / 16368 ms (0 without PHASE) */
  float    if_freq_offset_hz;    /* 12  the newest window record's (0 without PHASE) */
  uint32_t flags;                /* 16  the state's flags | VALID */
  int32_t  age_blocks;           /* 20  B - last_win_end_p1, kept within 0 .. 2^31 - 1; -1 without PHASE */
  uint32_t n_wraps, reserved;    /* 24  the state's n_wraps; 0 */
} gpsx_wobs_t;

/* d_rec [n_slots][n_ch] and d_words [n_blocks / 600 + 2][n_ch]: what the two earlier stages wrote for these n_blocks blocks, on the
 * device in both variants, as d_state [n_ch] is; d_obs / obs: [n_ch] */
int gpsx_wobs_dev(gpsx_ctx *ctx, const gpsx_wobs_cfg_t *cfg, const gpsx_wsync_rec_t *d_rec, int n_slots, int n_blocks,
                  const gpsx_wnav_word_t *d_words, gpsx_wobs_state_t *d_state, int n_ch, gpsx_wobs_t *d_obs);
int gpsx_wobs(gpsx_ctx *ctx, const gpsx_wobs_cfg_t *cfg, const gpsx_wsync_rec_t *d_rec, int n_slots, int n_blocks,
              const gpsx_wnav_word_t *d_words, gpsx_wobs_state_t *d_state, int n_ch, gpsx_wobs_t *obs /* host */);
/* host only, no GPU: pseudoranges from the VALID observables of one launch.  The reference channel is the one with the latest
 * transmit time (the nearest satellite), found through differences of tx_ms folded into -302 400 000 .. 302 399 999 ms minus
 * the difference of the code phases / 16368, the first of equals; then for every VALID i
 *   pr_m[i] = 299792458e-3 * ((double)(folded tx_ms_ref - tx_ms_i) + ((double)phase_i - (double)phase_ref) / 16368.0 + offset_ms)
 * and pr_m[i] = 0 for the others.  *rx_tow_s = (tx_ms_ref - phase_ref / 16368 + offset_ms) / 1000, folded into 0 .. 604 800 s: the
 * receiver time that offset_ms stands for (0 without a VALID observable).  offset_ms is the reference channel's travel time as the
 * caller assumes it (the reference's own pseudorange step uses 68.802 ms: include/gpsx_compat.h); the solver's clock term takes
 * the rest.  Returns the number of VALID observables, or GPSX_EINVAL for NULL, n < 1 or an offset_ms that is not finite. */
int gpsx_wobs_pseudoranges(const gpsx_wobs_t *obs, int n, double offset_ms, double *pr_m, double *rx_tow_s);
/* host only, no GPU: gpsx_wobs_pseudoranges applied to each receiver's slice of the observables of a
 * gpsx_track_loop_weighted_sync_multi chain: obs [n_rx * ch_per_rx], receiver r's are [r * ch_per_rx, (r + 1) * ch_per_rx).  The
 * reference channel is chosen per receiver; pr_m [n_rx * ch_per_rx], rx_tow_s [n_rx] and n_valid [n_rx] (the per-slice return
 * values; 0 for a receiver without a VALID observable) are bitwise those of n_rx separate calls.  Returns the sum of n_valid, or
 * GPSX_EINVAL for NULL, n_rx < 1, ch_per_rx < 1, n_rx * ch_per_rx above INT32_MAX or an offset_ms that is not finite. */
int gpsx_wobs_pseudoranges_rx(const gpsx_wobs_t *obs, int n_rx, int ch_per_rx, double offset_ms, double *pr_m, double *rx_tow_s, int *n_valid);

/* ---- EXTENSION, not in the reference: weighted ephemerides -- every channel's broadcast ephemeris from the words, on the device ----
 * What a position needs beside the transmit times: the satellite's broadcast ephemeris.  gpsx_weph(_dev) is a fifth stage behind
 * gpsx_wnav_words_dev: a kernel reads the word records d_words[n_blocks / 600 + 2][n_ch] where the word layer left them, keeps a
 * 192-byte state per channel, assembles subframes across launches, keeps the newest complete subframes 1, 2 and 3 and returns one
 * 256-byte record per channel and launch.  When the three are of one issue of data the record holds the decoded ephemeris: what
 * gps_nav_data_decode_subframe (include/gpsx_compat.h) produces, field for field and bit for bit.  Nothing existing changes.
 *
 * Definition, per channel.  The slots of d_words are read in order.  A record counts only if its flags have GPSX_WNAV_WORD,
 * 1 <= index <= 10, -600 <= end_block < n_blocks (word 1 of a GPSX_WNAV_SYNC pair ends before its launch may) and, with
 * E1 = blocks_seen + end_block + 1, E1 >= 1; every other record is skipped.  `passed`: the record has GPSX_WNAV_OK -- and, for
 * index 2, subframe_id in 1 .. 5 and aux < 100800.  For a record that counts:
 *   1 word 1       cur_mask = passed, cur_next = 2, cur_id = cur_tow = 0, last_word_end_p1 = E1
 *   2 the expected word  (index == cur_next and E1 == last_word_end_p1 + 600)  if passed: cur_mask |= 1 << (index - 1); if passed
 *                  and index is 2: cur_id = subframe_id, cur_tow = aux; if passed and index >= 3: cur[index - 3] = (word >> 6) &
 *                  0xFFFFFF.  Then last_word_end_p1 = E1 and cur_next = index == 10 ? 0 : index + 1.  At index 10 with cur_mask ==
 *                  0x3FF: n_subframes++, and the subframe is committed if cur_id is 1 .. 3
 *   3 anything else  (a gap, a word out of order, a word while waiting for a word 1)  cur_next = 0, cur_mask = 0,
 *                  last_word_end_p1 = E1
 * Commit, with k = cur_id - 1: changed = !(have >> k & 1) || sf[k] != cur in any of the eight words; sf[k] = cur, sf_tow[k] =
 * cur_tow, have |= 1 << k; consistent = have == 7 && (sf[1][0] >> 16) == (sf[2][7] >> 16) && (sf[1][0] >> 16) == (sf[0][5] >> 16)
 * -- IODE of subframe 2 word 3, IODE of subframe 3 word 10, the low byte of IODC in subframe 1 word 8.  Consistent: VALID is set;
 * if it was not set before the commit, or `changed`, n_sets++ and the launch's record gets NEW.  Not consistent: VALID is cleared
 * (a data-set cutover is in progress: the caller keeps the set it has).  A break in the words never clears VALID, and a
 * reacquired satellite that sends the same set again is VALID without NEW.  (Word 10s lie 6000 blocks apart: at most one commit
 * per launch.)
 * Output: blocks_seen += n_blocks.  With VALID the record holds what gps_nav_data_decode_subframe leaves in eph_data.eph of a zeroed
 * channel after it has been given subframes 1, 2 and 3 in this order, with sf[0 .. 2] as the source bits and sf_tow[0] as the HOW
 * count of subframe 1: the same fields at the same bit positions (subframe bit n lies in word n / 30, and bits 0 .. 23 of a word are
 * d1 .. d24), the same decimal scale literals (three of which are not powers of two), the same order of double operations (one
 * IEEE multiply each: the scale, then 3.1415926535898 for semicircles; A = sqrtA * sqrtA), the week resolved around build week 2290,
 * and gps_time with its (int)sec split.  Without VALID every field but flags, n_sets and have is zero.  Every byte of d_eph is
 * written.  n_sets and n_subframes wrap at 2^32.  The call must be made on every launch of a stream, as gpsx_wnav_words must:
 * blocks_seen is the time base.  Where a stream is cut into launches matters to nothing but which launch's record gets NEW.
 * Errors: NULL pointers, a reserved field != 0, n_blocks outside 1 .. 4096, n_ch < 1 and a size that overflows return GPSX_EINVAL
 * (with a gpsx_last_error text) and write nothing.  A channel is BAD if blocks_seen or last_word_end_p1 lies outside 0 .. 2^62,
 * cur_next is not 0 or 2 .. 10, cur_mask > 0x3FF, cur_id > 5, cur_tow or a sf_tow >= 100800, a cur / sf word >= 2^24, have > 7, its
 * flags have bits other than VALID or VALID without have == 7, or reserved != 0: its state stays as it was, its record is all zero,
 * and GPSX_EINVAL comes from gpsx_weph after its wait / from the next gpsx_synchronize() after _dev.
 * Vector ALU (k_weph: one channel per lane, the word records' 16-byte loads all in flight before the first is looked at, the
 * records stored through LDS so that a wave writes consecutive lines).  On one
 * stream: gpsx_track_loop_weighted_sync_dev, gpsx_wnav_words_dev, then gpsx_wobs_dev and gpsx_weph_dev on their arrays with the
 * same n_blocks.  gpsx_weph_to_eph (include/gpsx_compat.h) turns a VALID record into the reference's eph_t. */
#define GPSX_WEPH_VALID 1u   /* subframes 1, 2, 3 are held and IODE(2) == IODE(3) == IODC(1) & 0xFF */
#define GPSX_WEPH_NEW   2u   /* output only: a commit in this launch made the set VALID with contents it did not have before */

typedef struct { int32_t reserved0, reserved1; } gpsx_weph_cfg_t;          /* both 0 */

typedef struct {                 /* 192 bytes, device resident; all zero = a fresh channel */
  int64_t  blocks_seen;          /*   0  blocks of all earlier launches */
  int64_t  last_word_end_p1;     /*   8  absolute last block of the newest word that counted, + 1; 0: none */
  uint32_t cur[8];               /*  16  d1 .. d24 (d1 in bit 23) of words 3 .. 10 of the subframe being assembled */
  uint32_t cur_mask;             /*  48  bit w (0 .. 9): word w + 1 of it counted and passed */
  uint32_t cur_next;             /*  52  index of the word expected next, 2 .. 10; 0: waiting for a word 1 */
  uint32_t cur_id, cur_tow;      /*  56  from its HOW if that passed: 1 .. 5 and the 17-bit count; else 0 */
  uint32_t sf[3][8];             /*  64  words 3 .. 10 of the newest complete subframes 1, 2, 3 */
  uint32_t sf_tow[3];            /* 160  their HOW counts */
  uint32_t have;                 /* 172  bit k: sf[k] holds a subframe */
  uint32_t flags;                /* 176  GPSX_WEPH_VALID */
  uint32_t n_sets, n_subframes, reserved;   /* 180  sets that became NEW; complete subframes of any ID; 0 */
} gpsx_weph_state_t;

typedef struct {                 /* 256 bytes, one per channel and launch */
  uint32_t flags;                /*   0  the state's flags | NEW */
  int32_t  iode, iodc, sva, svh, week, code, flag;            /*   4 */
  int64_t  toe_time, toc_time, ttr_time;                      /*  32  gtime_t.time of eph_t's toe / toc / ttr */
  double   toe_sec, toc_sec, ttr_sec;                         /*  56  gtime_t.sec */
  double   A, e, i0, OMG0, omg, M0, deln, OMGd, idot, crc, crs, cuc, cus, cic, cis, toes, fit, f0, f1, f2, tgd;   /* 80 */
  uint32_t n_sets, have;         /* 248  the state's */
} gpsx_weph_t;

/* d_words [n_blocks / 600 + 2][n_ch]: what gpsx_wnav_words(_dev) wrote for these n_blocks blocks, on the device in both variants, as
 * d_state [n_ch] is; d_eph / eph: [n_ch]; d_eph 16-byte aligned, as every gpsx_malloc pointer is (GPSX_EINVAL otherwise) */
int gpsx_weph_dev(gpsx_ctx *ctx, const gpsx_weph_cfg_t *cfg, const gpsx_wnav_word_t *d_words, int n_blocks,
                  gpsx_weph_state_t *d_state, int n_ch, gpsx_weph_t *d_eph);
int gpsx_weph(gpsx_ctx *ctx, const gpsx_weph_cfg_t *cfg, const gpsx_wnav_word_t *d_words, int n_blocks,
              gpsx_weph_state_t *d_state, int n_ch, gpsx_weph_t *eph /* host */);

/* ---- EXTENSION, not in the reference: weighted lock monitor -- is a channel tracking a satellite, and how strong, on the device ----
 * What no stage above says: whether a channel's records are a satellite's at all.  gpsx_wlock(_dev) is a fifth reader of the sync
 * loop's window records d_rec[n_slots][n_ch] (beside gpsx_wnav_words, gpsx_wobs and, through the words, gpsx_weph): a kernel reads
 * the six correlator sums and the flags of every record, keeps a 128-byte state per channel and returns one 64-byte record per
 * channel and launch: a code-lock (presence) and a carrier-lock indicator with hysteresis, the three ratios they rest on (one of
 * them the C/N0 estimator's), loss events, and -- an opt-in -- the re-arm of the bit search that gpsx_track_loop_weighted_sync
 * leaves to its caller.  Nothing existing changes.
 *
 * Definition, per channel.  Every float operation is one IEEE single operation in the order written: no contraction, int64 ->
 * float rounds to nearest even, correctly rounded division.  The slots of d_rec are read in order.  A record counts if its flags
 * have GPSX_WSYNC_WINDOW and 0 <= end_block < n_blocks (gpsx_wobs's rule, without the phase); every other record is skipped.
 * With IE, QE, IP, QP, IL, QL = w.iq[0 .. 5] and locked = the record has GPSX_WSYNC_LOCKED_FLAG, for a record that counts:
 *   1 range        if any |iq[k]| >= 2^20: n_range++, the launch's record gets GPSX_WLOCK_RANGE, and nothing else happens for this
 *                  record.  (The sync loop's own sums stay below 20 x 49 056 < 2^20; only a caller's state can exceed that.)
 *   2 SEARCH       if !locked: if CARRIER is set it is cleared, n_lost_carrier++ and the launch's record gets LOST_CARRIER;
 *                  car_good = car_bad = 0, false_run = 0
 *   3 kind         if epoch_n > 0 and the open epoch's kind (OPEN_LOCKED) differs from `locked`: the open epoch is discarded
 *                  (the five sums = 0, epoch_n = 0).  OPEN_LOCKED = locked
 *   4 sums         in int64, exactly: A += |IP|, P += IP^2 + QP^2, D += IP^2 - QP^2, E += IE^2 + QE^2, L += IL^2 + QL^2; epoch_n++
 *   5 epoch end    if epoch_n >= (locked ? epoch_lock : epoch_search), with K = epoch_n:
 *                    code_ratio = (E + L == 0) ? 0 : (float)(2 P) / (float)(E + L)
 *                    car_ratio  = (P == 0) ? 0 : (float)D / (float)P
 *                    snr        = (K P - A A == 0) ? 0 : (float)(A A) / (float)(K P - A A)
 *                  They, P, K and the kind become the newest epoch's (last_*; EPOCH_LOCKED = locked), last_epoch_end_p1 =
 *                  blocks_seen + end_block + 1, the launch's n_epochs++, then
 *                  5a code     good = code_ratio >= code_min.  good: code_bad = 0, code_good = min(code_good + 1, 255), and
 *                              code_good >= n_good sets CODE.  Not good: code_good = 0, code_bad = min(code_bad + 1, 255), and if
 *                              CODE is set and code_bad >= n_bad: CODE is cleared, n_lost_code++, the launch's record gets
 *                              LOST_CODE, and if rearm & 1 PENDING is set
 *                  5b carrier  only if locked: good = car_ratio >= car_min && snr >= snr_min; was = CARRIER before this step.  The
 *                              same rule on car_good, car_bad, CARRIER, n_lost_carrier and LOST_CARRIER (no PENDING from a loss).
 *                              Then false_run = good || was ? 0 : false_run + 1, and if !good && !was && (rearm & 2) && false_run >=
 *                              patience: PENDING is set and false_run = 0 -- a bit synchroniser that locked on noise or on a false
 *                              frequency (the 1-in-20 remark of gpsx_track_loop_weighted_sync) never gets a carrier verdict
 *                  then the five sums = 0 and epoch_n = 0.
 * The bound of step 1 is what keeps every integer exact: a square is below 2^40, a window's term below 2^41, an epoch has at most
 * 1024 windows (cfg's bound; a state's epoch_n is at most 1023 before step 4), so P, E, L, |D| <= 2^51 + 2^41, 2 P and E + L stay
 * below 2^53, A <= 2^30 + 2^20, A A < 2^61 and K P < 2^62.  K P - A A >= 0 from sums this call formed (Cauchy-Schwarz on |IP|).
 * What they are: code_ratio is the prompt's energy against the two half-chip taps' (about 1 on noise, 3 to 4 on a tracked
 * code at a spacing of half a chip); it needs no phase lock and no bit alignment, so it works in SEARCH.  car_ratio is the narrow-band
 * estimate of cos 2 phi, insensitive to data bits.  snr is the signal-to-noise-variance estimator on a window's prompt.
 * At the launch's end: blocks_seen += n_blocks.  Then, if PENDING is set: if rearm != 0 and d_sync_state[ch].mode ==
 * GPSX_WSYNC_LOCKED the channel's sync state gets what gpsx_track_loop_weighted_sync prescribes for a caller -- mode = 0,
 * search_n = 0, prev_best_p1 = 0, and the open window discarded as an accept discards it: win_iq = 0, win_n = 0, bit_ip = 0,
 * loop.n_updates = 0 -- the launch's record gets REARMED, n_rearm++, CODE and CARRIER, the four run counters, false_run and the
 * open epoch (its sums, epoch_n and OPEN_LOCKED) are cleared.  PENDING is cleared in every case: a channel that has left LOCKED by itself needs no write, and with
 * rearm == 0 nothing can act on it.  gpsx_wlock_dev is enqueued behind the sync launch on the context's stream; it reads the sync
 * state only here, the mode word of PENDING channels alone, and writes only the fields above, so no launch of the sync loop runs
 * beside it.  With rearm == 0 d_sync_state may be NULL and is never touched.
 * Where a stream is cut into launches matters to the states only through the re-arm (which acts at a launch's end) and to the
 * records only in their per-launch fields: n_epochs, the event flags and age_blocks.  The counters n_* wrap at 2^32, as false_run.
 * Errors: NULL pointers (d_sync_state only with rearm != 0), epoch_search or epoch_lock outside 1 .. 1024, n_good or n_bad outside
 * 1 .. 255, a threshold that is not finite, rearm outside 0 .. 3, patience < 0, reserved != 0, n_blocks outside 1 .. 4096, n_slots
 * outside 1 .. n_blocks, n_ch < 1 and a size that overflows return GPSX_EINVAL (with a gpsx_last_error text) and write nothing.
 * A channel is BAD if its state has flag bits other than CODE .. EPOCH_LOCKED or a reserved word != 0, if blocks_seen or
 * last_epoch_end_p1 lies outside 0 .. 2^62, if epoch_n > 1023 or last_k > 1024, if a run counter exceeds 255, if sum_a lies outside
 * 0 .. 2^30, sum_p, sum_e or sum_l outside 0 .. 2^51 or |sum_d| > 2^51: its state (and its sync state) stays as it was, its record
 * is all zero with age_blocks = -1, and GPSX_EINVAL comes from gpsx_wlock after its wait / from the next gpsx_synchronize() after
 * _dev.  Vector ALU (k_wlock: one channel per lane, 32 of a record's 48 bytes loaded four slots ahead of the recurrence). */
#define GPSX_WLOCK_CODE          1u    /* the code is there: n_good consecutive epochs with code_ratio >= code_min */
#define GPSX_WLOCK_CARRIER       2u    /* the carrier is locked: n_good consecutive LOCKED epochs with car_ratio and snr above theirs */
#define GPSX_WLOCK_PENDING       4u    /* state only: a re-arm is due at the launch's end */
#define GPSX_WLOCK_OPEN_LOCKED   8u    /* state only: the open epoch's windows are LOCKED ones */
#define GPSX_WLOCK_EPOCH_LOCKED  16u   /* the newest completed epoch was a LOCKED one */
#define GPSX_WLOCK_LOST_CODE     32u   /* output only, this launch: CODE was cleared */
#define GPSX_WLOCK_LOST_CARRIER  64u   /* output only, this launch: CARRIER was cleared */
#define GPSX_WLOCK_REARMED       128u  /* output only, this launch: the channel's bit search was re-armed */
#define GPSX_WLOCK_RANGE         256u  /* output only, this launch: a record with a sum of magnitude >= 2^20 was not accumulated */

typedef struct {                 /* 40 bytes */
  int32_t  epoch_search;         /* windows per epoch of SEARCH windows, 1 .. 1024 */
  int32_t  epoch_lock;           /* windows per epoch of LOCKED windows, 1 .. 1024 */
  float    code_min;             /* code verdict: code_ratio >= code_min (finite) */
  float    car_min, snr_min;     /* carrier verdict: car_ratio >= car_min && snr >= snr_min (finite) */
  int32_t  n_good, n_bad;        /* consecutive epochs that set / clear an indicator, 1 .. 255 */
  int32_t  rearm;                /* mask; 0: never.  1: on a code loss.  2: after `patience` bad carrier verdicts without CARRIER */
  int32_t  patience;             /* >= 0 */
  int32_t  reserved;             /* 0 */
} gpsx_wlock_cfg_t;

typedef struct {                 /* 128 bytes, device resident; all zero = a fresh channel */
  int64_t  blocks_seen;          /*   0  blocks of all earlier launches */
  int64_t  last_epoch_end_p1;    /*   8  absolute last block of the newest completed epoch, + 1; 0: none */
  int64_t  sum_a, sum_p, sum_d, sum_e, sum_l;   /*  16  the open epoch's A, P, D, E, L */
  int64_t  last_p;               /*  56  the newest completed epoch's P */
  float    last_code_ratio, last_car_ratio, last_snr;   /*  64  its three ratios */
  uint32_t epoch_n;              /*  76  windows in the open epoch, 0 .. 1023 */
  uint32_t flags;                /*  80  GPSX_WLOCK_CODE .. _EPOCH_LOCKED */
  uint32_t last_k;               /*  84  the newest completed epoch's K; 0: none yet */
  uint32_t code_good, code_bad, car_good, car_bad;   /*  88  runs of verdicts, 0 .. 255 */
  uint32_t false_run;            /* 104  consecutive bad carrier verdicts met without CARRIER */
  uint32_t n_lost_code, n_lost_carrier, n_rearm, n_range;   /* 108  losses of either indicator, re-arms, records refused by step 1 */
  uint32_t reserved;             /* 124  0 */
} gpsx_wlock_state_t;

typedef struct {                 /* 64 bytes, one per channel and launch */
  uint32_t flags;                /*  0  the state's CODE, CARRIER and EPOCH_LOCKED | this launch's LOST_CODE .. RANGE */
  uint32_t n_epochs;             /*  4  epochs completed in this launch */
  uint32_t last_k;               /*  8  the newest completed epoch's K (a launch without one repeats the state's); 0: none yet */
  int32_t  age_blocks;           /* 12  B - last_epoch_end_p1, B = blocks_seen after this launch, within 0 .. 2^31 - 1; -1: none yet */
  float    code_ratio, car_ratio, snr;   /* 16  that epoch's */
  uint32_t n_range;              /* 28  the state's */
  int64_t  p;                    /* 32  that epoch's P */
  uint32_t n_lost_code, n_lost_carrier, n_rearm;   /* 40  the state's */
  uint32_t reserved[3];          /* 52  0 */
} gpsx_wlock_t;

/* d_rec [n_slots][n_ch]: what gpsx_track_loop_weighted_sync(_dev) wrote for these n_blocks blocks, on the device in both variants,
 * as d_state [n_ch] and d_sync_state [n_ch] (that loop's own states; NULL unless cfg->rearm) are; d_lock / lock: [n_ch] */
int gpsx_wlock_dev(gpsx_ctx *ctx, const gpsx_wlock_cfg_t *cfg, const gpsx_wsync_rec_t *d_rec, int n_slots, int n_blocks,
                   gpsx_wlock_state_t *d_state, gpsx_wsync_state_t *d_sync_state, int n_ch, gpsx_wlock_t *d_lock);
int gpsx_wlock(gpsx_ctx *ctx, const gpsx_wlock_cfg_t *cfg, const gpsx_wsync_rec_t *d_rec, int n_slots, int n_blocks,
               gpsx_wlock_state_t *d_state, gpsx_wsync_state_t *d_sync_state, int n_ch, gpsx_wlock_t *lock /* host */);
/* host only, no GPU: C/N0 in dB-Hz from the records of one launch.  For a record whose newest epoch was a LOCKED one (EPOCH_LOCKED,
 * last_k > 0) with snr > 0: cn0_dbhz[i] = (float)(10 log10((double)snr / (n_coh_lock * 0.001))), n_coh_lock the sync loop's, the
 * logarithm in double; 0 for every other record.  (The logarithm stays on the host: what a device logarithm costs in parity is
 * told at snr_value below.)  Returns GPSX_OK, or GPSX_EINVAL for NULL, n < 1 or n_coh_lock outside 1 .. 20. */
int gpsx_wlock_cn0_dbhz(const gpsx_wlock_t *lock, int n, int n_coh_lock, float *cn0_dbhz);

/* ---- EXTENSION, not in the reference: weighted position fixes -- every receiver's single-point position, on the device -------------
 * The last step of the weighted chain: gpsx_wfix(_dev) is a stage behind gpsx_wobs_dev and gpsx_weph_dev (and gpsx_wlock_dev, when its
 * verdict is wanted).  It reads the observables d_obs[n_rx * ch_per_rx] and the ephemeris records d_eph[n_rx * ch_per_rx] where those
 * stages left them -- receiver r owns slots [r * ch_per_rx, (r + 1) * ch_per_rx), as in gpsx_track_loop_weighted_sync_multi -- and
 * returns one 128-byte record per receiver: what gpsx_wobs_pseudoranges_rx, gpsx_weph_to_eph per slot and pntpos per receiver
 * (include/gpsx_compat.h) give on the host, but with every usable satellite of up to 64 slots, not pntpos' four.  It keeps no state.
 * Nothing existing changes.
 *
 * Definition, per receiver; all arithmetic in IEEE double, uncontracted.
 *   1 usable       a slot is usable if its observable has GPSX_WOBS_VALID, its ephemeris record has GPSX_WEPH_VALID and, when d_lock is
 *                  given, its lock record has GPSX_WLOCK_CODE.  Fewer than min_sats usable slots: TOO_FEW, no iteration.
 *   2 ranges       gpsx_wobs_pseudoranges' definition applied to the usable slots alone (the others count as not VALID): ref_slot,
 *                  pr_m (0 for the others) and rx_tow_s.  Every operation there is an int64 or a single double operation, so the three
 *                  are the host helper's bit for bit.  (A pr_m or rx_tow_s that is not finite -- only an observable whose code phase
 *                  is not finite, which gpsx_wobs never writes, gives one -- is written as 0; such an rx_tow_s ends in NONFINITE.)
 *   3 time         the observation time is gtime_t{315964800 + 604800 week + (int)rx_tow_s, rx_tow_s - (int)rx_tow_s}, week the
 *                  reference slot's record's.  A week rollover (rx_tow_s within a travel time of the week's end) is NOT handled: the
 *                  same limit as the host glue's.  The same holds for records of another week than the receive time's -- the
 *                  previous week's broadcast (toes = 601200) at rx_tow_s = 1800, say: `week` is then that record's, the observation
 *                  time lies a week off, no slot passes step 4's |toe - time| rule and the receiver ends in TOO_FEW with n_used = 0
 *                  (pr_m, ref_slot and rx_tow_s are written as always).  gpsx_wvel folds its differences of times and gives
 *                  such slots rows.
 *   4 solver       then csrc/gpsx_pvt.cpp's solve(), branch for branch, on each usable slot's own record: |toe - time| <= 7201 s or the
 *                  slot has no satellite; the two time_adds (which never carry into the whole second) to the transmit time; the
 *                  broadcast clock's two fixed-point passes; the orbit (Kepler's equation to 1e-14 in fewer than 30 steps or no
 *                  satellite, A <= 0: a satellite at the centre, the URA table with sva outside 0 .. 14 read as 6144 m, the
 *                  relativistic clock term); per iteration ecef2pos of x (at the origin: latitude -pi / 2, height -Re, hence az = 0,
 *                  el = pi / 2 and no atmosphere; its fixed point is bounded at 30 steps here, which a finite x never needs), and per
 *                  slot: no row if the satellite's radius < Re, if rho = range + Sagnac <= 0, if el < 0 or if svh != 0; Klobuchar with
 *                  cfg's ion[] (all zero: the 2004 default set, as nav_t.ion_gps), Saastamoinen at humidity 0.7, the four variance
 *                  terms, the slot's own tgd; x += dx until |dx|^2 < 1e-8 over x, y, z, c dt, ten iterations at most.
 *   5 different from pntpos, on purpose: any number of rows up to 64; FOUR unknowns -- the reference's three tied-down bias unknowns
 *                  appear in no satellite row, so its 7 x 7 normal matrix is block diagonal and x, y, z, c dt and their covariance
 *                  are those of the 4 x 4 system, solved here by a Cholesky factorisation (pntpos: Gauss-Jordan with pivoting, so
 *                  the two agree to round-off, not to the bit); no duplicate-PRN rule (the stage sees no PRNs: the caller gives a
 *                  receiver distinct satellites); fewer than min_sats rows in an iteration: TOO_FEW; a pivot of the factorisation that
 *                  is not positive beyond the round-off of its own subtraction (p_k <= 1e-10 N_kk; p_0 <= 0): SINGULAR; a sum of
 *                  the normal system or a dx that is not finite: NONFINITE.
 *   6 start        x = d_prev[r].rr, c dt = 0 if that record has FIX, else the origin.  d_prev may be d_fix itself: a receiver reads
 *                  its own record before it writes it.
 *   7 output       with FIX: rr, dtr_s = x[3] / c, geo = ecef2pos(rr), qr as pntpos' sol_t.qr (xx, yy, zz, xy, yz, xz of the inverse
 *                  normal matrix, as floats), and resid_rms_m = sqrt(sum v^2 / n_used) over the unweighted residuals v recomputed at
 *                  the FINAL x for the slots of used_mask (that still give a row there).  n_iter counts the iterations whose rows
 *                  were formed, n_used and used_mask are the last one's.  Without FIX every numeric field but flags, n_used, n_iter,
 *                  ref_slot, used_mask, rx_tow_s and week is zero.  Exactly one of the five flags is set.  Every byte of d_fix (and
 *                  of d_pr_m if given) is written; no NaN or infinity is ever written (a result that has one: NONFINITE).
 * Errors: NULL ctx / cfg / d_obs / d_eph / d_fix, an offset_ms or ion[] that is not finite, ch_per_rx outside 1 .. 64, min_sats
 * outside 4 .. 64, reserved != 0, n_rx outside 1 .. 1 048 576, a d_fix that is not 16-byte aligned (_dev) and a byte count that
 * overflows return GPSX_EINVAL (with a gpsx_last_error text) and write nothing.  There is no per-channel BAD policy: a bad channel's
 * all-zero observable and record are simply not usable.
 * Vector ALU, FP64 (k_wfix: one slot per lane, a receiver a group of W lanes, W the smallest power of two >= ch_per_rx; the 10 + 4
 * sums of the normal system by xor-butterflies of width W; every loop bounded and every cross-lane operation under wave-uniform
 * control flow).  On one stream: ..., gpsx_wobs_dev, gpsx_weph_dev (, gpsx_wlock_dev), then gpsx_wfix_dev on their arrays. */
#define GPSX_WFIX_FIX        1u   /* rr, dtr_s, geo, qr, resid_rms_m hold a converged solution */
#define GPSX_WFIX_TOO_FEW    2u   /* fewer than min_sats usable slots (before or inside the iteration) */
#define GPSX_WFIX_SINGULAR   4u   /* the normal matrix had a pivot that was not positive (beyond round-off: 5 above) */
#define GPSX_WFIX_NO_CONV    8u   /* ten iterations without |dx|^2 < 1e-8 */
#define GPSX_WFIX_NONFINITE 16u   /* a non-finite number appeared; nothing non-finite is ever written */

typedef struct {                 /* 96 bytes */
  double   offset_ms;            /* gpsx_wobs_pseudoranges' offset_ms, finite */
  double   ion[8];               /* Klobuchar a0..a3, b0..b3, finite; all zero: the 2004 default set (nav_t.ion_gps) */
  int32_t  ch_per_rx;            /* 1 .. 64 */
  int32_t  min_sats;             /* 4 .. 64 */
  int32_t  reserved0, reserved1; /* 0 */
  int32_t  reserved2, reserved3; /* 0 */
} gpsx_wfix_cfg_t;

typedef struct {                 /* 128 bytes, one per receiver and launch */
  uint32_t flags;                /*   0 */
  int32_t  n_used;               /*   4  rows of the last iteration */
  int32_t  n_iter;               /*   8  iterations run, 0 .. 10 */
  int32_t  ref_slot;             /*  12  the reference slot within the receiver, -1: none */
  uint64_t used_mask;            /*  16  bit j: slot j gave a row in the last iteration */
  double   rr[3];                /*  24  ECEF, m */
  double   dtr_s;                /*  48  receiver clock term, x[3] / c */
  double   rx_tow_s;             /*  56  as gpsx_wobs_pseudoranges' *rx_tow_s over the usable slots */
  double   geo[3];               /*  64  latitude, longitude (rad), height (m) of rr */
  float    qr[6];                /*  88  pntpos' sol_t.qr */
  double   resid_rms_m;          /* 112  sqrt(sum v^2 / n_used), residuals recomputed at the FINAL x, unweighted */
  int32_t  week, reserved;       /* 120  the reference slot's eph week; 0 */
} gpsx_wfix_t;

/* d_obs, d_eph, d_lock (NULL: not consulted): [n_rx * ch_per_rx], d_prev (NULL: start at the origin) and d_fix: [n_rx], d_pr_m (NULL:
 * not written): [n_rx * ch_per_rx]; all on the device for _dev, all in host memory (staged through the arena; the call waits for its
 * kernel) for gpsx_wfix */
int gpsx_wfix_dev(gpsx_ctx *ctx, const gpsx_wfix_cfg_t *cfg, const gpsx_wobs_t *d_obs, const gpsx_weph_t *d_eph, const gpsx_wlock_t *d_lock,
                  const gpsx_wfix_t *d_prev, int n_rx, gpsx_wfix_t *d_fix, double *d_pr_m);
int gpsx_wfix(gpsx_ctx *ctx, const gpsx_wfix_cfg_t *cfg, const gpsx_wobs_t *obs, const gpsx_weph_t *eph, const gpsx_wlock_t *lock,
              const gpsx_wfix_t *prev, int n_rx, gpsx_wfix_t *fix, double *pr_m);

/* ---- EXTENSION, not in the reference: weighted fixes with millisecond repair and fault detection / exclusion, on the device --------
 * gpsx_wfix uses every usable slot as it stands: a slot whose tx_ms is the 1 ms off that GPSX_WOBS_AMBIGUOUS warns of (300 km of
 * range), or whose range is wrong by a few hundred metres, goes into the fix and moves it.  gpsx_wfde(_dev) is gpsx_wfix with both
 * looked after: it repairs the ambiguous millisecond from a fix over the unambiguous slots, then tests the residuals of the full fix
 * and excludes the worst slot until the test passes.  Same inputs, same gpsx_wfix_t per receiver, one 64-byte gpsx_wfde_t beside it.
 * It keeps no state.  gpsx_wfix and everything else stay as they are.
 *
 * Definition, per receiver.  A ROUND on an active set S is gpsx_wfix's definition above, steps 1 - 7, with "usable" replaced by S
 * and every slot's tx_ms replaced by tx_ms + k_j; the reference slot, rx_tow_s, the week and the satellites are those of the round.
 * The same arithmetic, IEEE double, uncontracted.
 *   1 sets         U: gpsx_wfix's usable set (d_lock included); A: the slots of U whose observable has GPSX_WOBS_AMBIGUOUS; C = U \ A.
 *                  k_j = 0 for every slot and excl_mask = 0 to begin with.
 *   2 repair       only if cfg.repair is set, A is not empty and |C| >= min_sats: one round on C, started from d_prev as in step 6.
 *                  If it ends in FIX at x_C, then for every j of A: pr_j by step 2's formula against C's reference slot, j's
 *                  satellite at its transmit time, v_j exactly the solver's row at x_C (clock term included).  No row: k_j = 0 and j
 *                  stays active.  Otherwise k_j = (int)rint(v_j / 299792.458); |k_j| <= 1 is kept (the plus or minus bit is set when it
 *                  is not zero); |k_j| > 1 or a v_j that is not finite puts j into excl_mask.  If the round does not end in FIX,
 *                  or the repair did not run while A is not empty: UNRESOLVED.
 *   3 detection    S = U minus excl_mask.  Every round starts as step 6 from the preceding round's record (its rr with FIX, else
 *     and          the origin); for the first round of all that is d_prev.  A round without FIX ends the receiver with NOFIX.  After
 *     exclusion    FIX, the residual pass at the final x: the rows counted are row AND used_mask, as resid_rms_m counts them;
 *                  dof = n_counted - 4, y_j = v_j / sig_j, T = sum y_j^2.  dof < 1: UNCHECKED, done.  Otherwise the limit is the
 *                  Wilson-Hilferty chi-square quantile, in doubles as written: t = 1 - 2 / (9 dof) + z_global sqrt(2 / (9 dof)),
 *                  limit = dof t t t.  T <= limit: PASSED.  Otherwise FAULT when the statistical exclusions so far equal max_excl,
 *                  when n_counted - 1 < min_sats, or when no slot can be named.  Naming: the counted rows' normal matrix is
 *                  factorised as in step 5 (a pivot fails: no name); h_jj = |M a_j|^2, w_j^2 = y_j^2 / (1 - h_jj), 0 where
 *                  1 - h_jj <= 1e-10; the named slot has the largest w_j^2 > 0, the lowest slot among equals.  It goes into
 *                  excl_mask and the next round runs: at most 1 + (max_excl + 1) rounds per receiver.  (The w-test, not the
 *                  largest |y_j|: a faulty row with leverage pulls the fix towards itself and hides its own residual.)
 *   4 output       d_fix[r] is the last round's gpsx_wfix_t, under the same byte rules (every byte written, nothing non-finite);
 *                  d_pr_m, if given, that round's pseudoranges, 0 for the slots not active in it; every byte of d_fde[r] is
 *                  written.  A T that is not finite (no finite record gives one) counts as a failed test and is written as 0.
 * Hence: with repair = 0 and max_excl = 0, d_fix and d_pr_m are gpsx_wfix_dev's on the same inputs, byte for byte; with four usable
 * slots the verdict is UNCHECKED and the record gpsx_wfix's.
 * Errors: all of gpsx_wfix's (on cfg.fix), and: d_fde NULL or not 16-byte aligned (_dev), z_global not finite or outside 0 .. 10,
 * max_excl outside 0 .. 8, repair outside 0 / 1, reserved != 0: GPSX_EINVAL with a gpsx_last_error text, nothing written.
 * Vector ALU, FP64 (k_wfde: k_wfix's lane layout with a loop over rounds around the pass loop; a group that is finished masks its
 * updates, the groups of one wave may sit in different rounds; the arg-max of w^2 is a butterfly on (value, slot)). */
#define GPSX_WFDE_PASSED      1u   /* the last round has FIX and its test passed */
#define GPSX_WFDE_UNCHECKED   2u   /* FIX with dof < 1: nothing to test with */
#define GPSX_WFDE_FAULT       4u   /* FIX, but the test failed and no further exclusion was possible or allowed */
#define GPSX_WFDE_NOFIX       8u   /* the last round has no FIX (d_fix tells why) */
#define GPSX_WFDE_EXCLUDED   16u   /* modifier: excl_mask is not zero */
#define GPSX_WFDE_REPAIRED   32u   /* modifier: a plus or minus bit is set */
#define GPSX_WFDE_UNRESOLVED 64u   /* modifier: AMBIGUOUS usable slots went in unrepaired */

typedef struct {                 /* 128 bytes */
  gpsx_wfix_cfg_t fix;           /*   0  as gpsx_wfix's, same rules */
  double   z_global;             /*  96  finite, 0 .. 10: the normal quantile of the global test (3.09: alpha = 1e-3) */
  int32_t  max_excl;             /* 104  0 .. 8: statistical exclusions allowed per receiver */
  int32_t  repair;               /* 108  0 / 1: run the millisecond repair */
  int32_t  reserved[4];          /* 112  0 */
} gpsx_wfde_cfg_t;

typedef struct {                 /* 64 bytes, one per receiver and launch */
  uint32_t flags;                /*  0  exactly one of PASSED / UNCHECKED / FAULT / NOFIX, and the modifiers */
  int32_t  n_rounds;             /*  4  solver rounds run, the repair round included */
  int32_t  n_excluded;           /*  8  popcount(excl_mask) */
  int32_t  dof;                  /* 12  rows counted in the last residual pass - 4 (0 without FIX) */
  uint64_t excl_mask;            /* 16  slots taken out, by the w-test or for |k| > 1 */
  uint64_t plus_mask, minus_mask;/* 24  slots whose tx_ms was corrected by +1 / -1 ms */
  double   t_stat, t_limit;      /* 40  the last round's T and its limit (0 where no test ran) */
  uint64_t reserved;             /* 56  0 */
} gpsx_wfde_t;

/* arrays as gpsx_wfix's; d_fde: [n_rx].  On one stream: ..., gpsx_wobs_dev, gpsx_weph_dev (, gpsx_wlock_dev), then gpsx_wfde_dev */
int gpsx_wfde_dev(gpsx_ctx *ctx, const gpsx_wfde_cfg_t *cfg, const gpsx_wobs_t *d_obs, const gpsx_weph_t *d_eph, const gpsx_wlock_t *d_lock,
                  const gpsx_wfix_t *d_prev, int n_rx, gpsx_wfix_t *d_fix, gpsx_wfde_t *d_fde, double *d_pr_m);
int gpsx_wfde(gpsx_ctx *ctx, const gpsx_wfde_cfg_t *cfg, const gpsx_wobs_t *obs, const gpsx_weph_t *eph, const gpsx_wlock_t *lock,
              const gpsx_wfix_t *prev, int n_rx, gpsx_wfix_t *fix, gpsx_wfde_t *fde, double *pr_m);

/* ---- EXTENSION, not in the reference: weighted velocity fixes -- every receiver's velocity and clock drift, on the device -----------
 * gpsx_wfix / gpsx_wfde give position and time.  gpsx_wvel(_dev) is a stateless stage behind either: from the carrier frequency that
 * every observable carries (gpsx_wobs_t.if_freq_offset_hz), the ephemeris records and the position records it solves, per receiver,
 * the ECEF velocity and the receiver clock's drift by one linear least-squares step, and returns one 112-byte gpsx_wvel_t.  Neither
 * the reference nor csrc/gpsx_pvt.cpp has a Doppler solver; this text is the definition.  Nothing existing changes.
 *
 * Definition, per receiver; all arithmetic in IEEE double, uncontracted.  c = 299792458, we = 7.2921151467e-5, mu = 3.9860050e14.
 *   1 rows         d_fix[r] has no GPSX_WFIX_FIX: NO_FIX.  Otherwise slot j is a candidate iff bit j of d_fix[r].used_mask is set (so
 *                  gpsx_wfde's repair and exclusion carry over: an excluded slot gives no Doppler row either), its observable has
 *                  GPSX_WOBS_VALID, its record has GPSX_WEPH_VALID and svh == 0, its if_freq_offset_hz is finite and, when d_lock is
 *                  given, its lock record has GPSX_WLOCK_CARRIER.  The records of other slots are not read.
 *   2 satellite    the satellite clock's reading of the transmit time comes straight from the observable:
 *                  t_sv = ((double)tx_ms - (double)code_phase_fine / 16368) / 1000, seconds of the week; no pseudorange and no reference
 *                  slot are needed.  With fold(d) = d > 302400 ? d - 604800 : d < -302400 ? d + 604800 : d (the week's end) and
 *                  toc = (double)((toc_time - 315964800) mod 604800) + toc_sec: tc = fold(t_sv - toc); tc -= poly(tc) twice (k_wfix's
 *                  two fixed-point passes, poly(t) = f0 + f1 t + f2 t t); t = t_sv - poly(tc); tk = fold(t - toes).  No row if
 *                  |tk| > 7201, if A <= 0, or if Kepler's iteration (gpsx_wfix's: to 1e-14) needs 30 steps.  n = sqrt(mu / A^3) + deln.
 *                  The position ps is gpsx_wfix's (IS-GPS-200 table 20-IV).  The velocity vs is its analytic derivative: with E, nu,
 *                  phi = nu + omg BEFORE the harmonic corrections and u, r, i after them,
 *                    E'  = n / (1 - e cos E)                     nu' = E' sqrt(1 - e^2) / (1 - e cos E)
 *                    u'  = nu' (1 + 2 (cus cos 2phi - cuc sin 2phi))
 *                    r'  = A e E' sin E + 2 nu' (crs cos 2phi - crc sin 2phi)
 *                    i'  = idot + 2 nu' (cis cos 2phi - cic sin 2phi)        W' = OMGd - we
 *                    xo' = r' cos u - r u' sin u                 yo' = r' sin u + r u' cos u
 *                    vx  = xo' cos W - yo' cos i sin W + yo i' sin i sin W - W' py
 *                    vy  = xo' sin W + yo' cos i cos W - yo i' sin i cos W + W' px
 *                    vz  = yo' sin i + yo i' cos i
 *                  and the satellite clock's rate d' = f1 + 2 f2 fold(t - toc) - 2 sqrt(mu A) e cos E E' / c^2.
 *                  A slot whose millisecond gpsx_wfde repaired (+- 1 ms) is evaluated at its UNREPAIRED tx_ms: the stage does not see
 *                  the repair, and 1 ms moves a satellite's velocity by about 6e-4 m/s.
 *   3 row          l = ps - rr, rr = d_fix[r].rr; s = l.l, rho = sqrt(s); no row if rho == 0; e = l / rho.  With k = we / c, the
 *                  derivative of gpsx_wfix's range model rho + k (ps_x rr_y - ps_y rr_x) + c dt - c d:
 *                    y_j = mps_per_hz f_j - (e . vs + k (vs_x rr_y - vs_y rr_x) - c d'_j)
 *                    a_j = (-e_x - k ps_y, -e_y + k ps_x, -e_z, 1)
 *                  The signs of the two k terms are the derivative's.  RTKLIB's resdop has both the other way round (+ k (vs_y rr_x -
 *                  vs_x rr_y) in the rate, + k ps_y and - k ps_x in the row); that is NOT a slip to be corrected here: on Dopplers formed
 *                  from the travel time's own derivative a receiver at rest comes out 3.6e-3 m/s off with these signs and 2.7e-2 m/s
 *                  off with resdop's (tests/test_weighted_vel_reference.py).
 *                  f_j = (double)if_freq_offset_hz.  mps_per_hz is the caller's statement of what a hertz of that field is worth, and
 *                  it must know the loop: this library's weighted loops rest at fd (1 + 1/1022), not at the Doppler fd (see
 *                  gpsx_track_loop_weighted above: the NCO mixes 16 352 of a block's 16 368 samples), so their frequencies take
 *                  GPSX_WVEL_L1CA_WLOOP = GPSX_WVEL_L1CA 1022 / 1023.  GPSX_WVEL_L1CA on them puts 0.1 % of every Doppler into its
 *                  row, up to 0.75 m/s at 4 kHz: a bias that no averaging removes.  (The tests' IF stream, a receiver at rest on
 *                  four satellites: 1.05 m/s with GPSX_WVEL_L1CA, 0.07 m/s with GPSX_WVEL_L1CA_WLOOP, the loops' frequencies then being
 *                  0.04 to 0.35 Hz off the truth.)  The model is linear in x = (v, c drift): one solve, no iteration.  Atmospheric
 *                  rates are neglected, and so are the terms of second order in 1 / c (the satellite moves on while the range
 *                  changes: e . vs times the range rate over c, up to 2e-3 m/s per row).  f_j is age_blocks old and is NOT
 *                  extrapolated to the launch's end: a line-of-sight acceleration stays below 1 Hz/s, times 20 ms.
 *   4 solve        fewer than min_sats rows: TOO_FEW.  N = sum a a^T, b = sum a y, unweighted.  A row's s counts among the sums: a sum
 *                  that is not finite: NONFINITE.  Cholesky as gpsx_wfix's with its pivot rule (p_0 <= 0, p_k <= 1e-10 N_kk:
 *                  SINGULAR), x = N^-1 b, v_j = y_j - a_j . x.  enu = (-sl x0 + cl x1, -sp cl x0 - sp sl x1 + cp x2,
 *                  cp cl x0 + cp sl x1 + sp x2) with the sines and cosines of d_fix[r].geo[0] (p) and geo[1] (l).  The checks run in
 *                  this order: NO_FIX, TOO_FEW, NONFINITE (sums), SINGULAR, NONFINITE (a result: x, drift, enu, qv, the rms).
 *   5 output       with VEL: vel = x[0..2], drift_s_s = x[3] / c, enu, qv = xx, yy, zz, xy, yz, xz of N^-1 as floats,
 *                  resid_rms_mps = sqrt(sum v^2 / n_used).  n_used and used_mask are the rows (0 with NO_FIX).  Without VEL every
 *                  numeric field but flags, n_used and used_mask is zero.  Exactly one of the five flags is set.  Every byte of
 *                  d_vel is written; no NaN or infinity is ever written.
 * Errors: NULL ctx / cfg / d_obs / d_eph / d_fix / d_vel, an mps_per_hz that is not finite or is 0, ch_per_rx outside 1 .. 64, min_sats
 * outside 4 .. 64, a reserved word != 0, n_rx outside 1 .. 1 048 576, a d_vel that is not 16-byte aligned (_dev) and a byte count that
 * overflows return GPSX_EINVAL (with a gpsx_last_error text) and write nothing.
 * Vector ALU, FP64 (k_wvel: gpsx_wfix's lane layout; the 10 + 4 sums and the sum of squared residuals by xor-butterflies of width W;
 * no loop but Kepler's).  On one stream: ..., gpsx_wfix_dev or gpsx_wfde_dev, then gpsx_wvel_dev on their arrays. */
#define GPSX_WVEL_L1CA (-0.19029367279836487)  /* -c / 1575.42e6: m/s of range rate per Hz of a frequency that IS the Doppler */
#define GPSX_WVEL_L1CA_WLOOP (GPSX_WVEL_L1CA * 1022.0 / 1023.0)   /* ... per Hz of this library's weighted loops' if_freq_offset_hz, which rest at fd (1 + 1/1022) */
#define GPSX_WVEL_VEL        1u   /* vel, drift_s_s, enu, qv, resid_rms_mps hold a solution */
#define GPSX_WVEL_NO_FIX     2u   /* d_fix[r] has no GPSX_WFIX_FIX: no position to stand on */
#define GPSX_WVEL_TOO_FEW    4u   /* fewer than min_sats rows */
#define GPSX_WVEL_SINGULAR   8u   /* a pivot failed gpsx_wfix's rule (p_0 <= 0, p_k <= 1e-10 N_kk) */
#define GPSX_WVEL_NONFINITE 16u   /* a sum or a result was not finite; nothing non-finite is ever written */

typedef struct {                 /* 32 bytes */
  double  mps_per_hz;            /* finite, not 0; negative where the frequency rises as a satellite approaches: GPSX_WVEL_L1CA_WLOOP for this library's weighted loops, GPSX_WVEL_L1CA for a true Doppler (step 3) */
  int32_t ch_per_rx;             /* 1 .. 64 */
  int32_t min_sats;              /* 4 .. 64 */
  int32_t reserved[4];           /* 0 */
} gpsx_wvel_cfg_t;

typedef struct {                 /* 112 bytes, one per receiver and launch */
  uint32_t flags;                /*   0  exactly one of the five */
  int32_t  n_used;               /*   4  rows */
  uint64_t used_mask;            /*   8  bit j: slot j gave a row */
  double   vel[3];               /*  16  ECEF, m/s */
  double   drift_s_s;            /*  40  receiver clock drift, x[3] / c */
  double   enu[3];               /*  48  vel in the east / north / up frame at d_fix[r].geo */
  float    qv[6];                /*  72  xx, yy, zz, xy, yz, xz of the inverse normal matrix (unweighted) */
  double   resid_rms_mps;        /*  96  sqrt(sum v^2 / n_used) */
  uint64_t reserved;             /* 104  0 */
} gpsx_wvel_t;

/* d_obs, d_eph, d_lock (NULL: not consulted): [n_rx * ch_per_rx], d_fix and d_vel: [n_rx]; all on the device for _dev, all in host
 * memory (staged through the arena; the call waits for its kernel) for gpsx_wvel */
int gpsx_wvel_dev(gpsx_ctx *ctx, const gpsx_wvel_cfg_t *cfg, const gpsx_wobs_t *d_obs, const gpsx_weph_t *d_eph, const gpsx_wlock_t *d_lock,
                  const gpsx_wfix_t *d_fix, int n_rx, gpsx_wvel_t *d_vel);
int gpsx_wvel(gpsx_ctx *ctx, const gpsx_wvel_cfg_t *cfg, const gpsx_wobs_t *obs, const gpsx_weph_t *eph, const gpsx_wlock_t *lock,
              const gpsx_wfix_t *fix, int n_rx, gpsx_wvel_t *vel);

/* ---- EXTENSION, not in the reference: weighted navigation filter -- every receiver's position, velocity and clock, carried from ------
 *      launch to launch in a resident state, on the device
 * gpsx_wfix / gpsx_wfde / gpsx_wvel keep no state: every launch's noise goes into that launch's fix, and a receiver with fewer than
 * four usable slots gets nothing.  gpsx_wkf(_dev) is a STATEFUL stage behind gpsx_wobs_dev and gpsx_weph_dev (and gpsx_wlock_dev,
 * gpsx_wfix_dev or gpsx_wfde_dev, gpsx_wvel_dev): an eight-state Kalman filter per receiver -- ECEF position, receiver clock term b (m),
 * velocity, clock drift d (m/s), in that order -- whose 384-byte gpsx_wkf_state_t lives in device memory (all zero: a fresh receiver)
 * and which returns one 240-byte gpsx_wkf_t per receiver and launch.  It is tightly coupled: its measurements are every slot's
 * pseudorange and carrier frequency, not the fix records, so it updates with one, two or three satellites too.  It must be called on
 * every launch of a stream, as gpsx_wobs.  Neither the reference nor csrc/gpsx_pvt.cpp has a filter; this text is the definition.
 * Nothing existing changes.
 *
 * Definition, per receiver; all arithmetic in IEEE double, uncontracted, sums in ascending index order unless a butterfly is named.
 * c = 299792458, ms = 299792.458 (c per millisecond), W = 604 800 000.  P is symmetric; P_ij below names its element, the state holds
 * the upper triangle row by row (P_00 .. P_07, P_11 .. P_17, ..., P_77: 36 doubles).
 *   0 state        BAD if the state has flag bits beyond GPSX_WKF_STATE_INIT, an rcv_ms outside 0 .. W - 1, an x or P element that
 *                  is not finite, or (with INIT) a P_ii <= 0.  A BAD state stays as it was, its record is all zero but for
 *                  flags = GPSX_WKF_BAD, and the call reports GPSX_EINVAL (gpsx_wkf after its wait, gpsx_wkf_dev at the next
 *                  gpsx_synchronize), as gpsx_wobs does.
 *   1 time base    the filter's clock is the sample count, not gpsx_wfix's reference slot (whose clock term jumps with the
 *                  reference): rcv_ms is the receiver clock's reading, in ms of the week, of sample 0 of the block that follows
 *                  the launch, and b = c (receiver clock - GPS time) moves with the oscillator alone.  An initialised receiver
 *                  first advances: rcv_ms += n_blocks; rcv_ms >= W: rcv_ms -= W, week += 1.  dt = (double)n_blocks * 1e-3.
 *   2 init         a state without INIT reads d_fix[r] (d_fix NULL: as a record without FIX).  Without GPSX_WFIX_FIX it stays as
 *                  it is: NOT_INIT, nothing counted, the state not written.  With it: u = 1000 (rx_tow_s - dtr_s), m = rint(u),
 *                  b = ms (m - u), rcv_ms = (int64)m, week = the record's; rcv_ms >= W: rcv_ms -= W, week += 1; rcv_ms < 0:
 *                  rcv_ms += W, week -= 1.  x = (rr, b, vel, c drift_s_s) with vel and drift_s_s from d_vel[r] if d_vel is given and
 *                  that record has GPSX_WVEL_VEL, else zeros.  P = diag(p0_pos^2 x 3, p0_clk^2, p0_vel^2 x 3, p0_drift^2).
 *                  n_starved = 0, n_init += 1.  No prediction and no update in this call: INIT (an |m| >= 2^53, an rcv_ms still
 *                  outside 0 .. W - 1, or anything of step 12's x, P or output that is not finite: NOT_INIT instead).  Initialised receivers never read d_fix or d_vel.
 *   3 prediction   constant velocity, F = [[I4, dt I4], [0, I4]]: x-_i = x_i + dt x_(4+i), x-_(4+i) = x_(4+i), i = 0 .. 3, and
 *                  P- = F P F^T + Q in three 4 x 4 blocks (i, j = 0 .. 3):
 *                    P-_(i,j)     = ((P_(i,j) + dt (P_(i,4+j) + P_(j,4+i))) + (dt dt) P_(4+i,4+j)) [+ qpp_i if i == j]
 *                    P-_(i,4+j)   = (P_(i,4+j) + dt P_(4+i,4+j)) [+ qpv_i if i == j]
 *                    P-_(4+i,4+j) = P_(4+i,4+j) [+ qvv_i if i == j]
 *                  with t3 = dt dt dt / 3, t2 = dt dt / 2; position axes i = 0 .. 2: qpp = q_acc t3, qpv = q_acc t2, qvv = q_acc dt;
 *                  clock i = 3: qpp = q_clk_f dt + q_clk_g t3, qpv = q_clk_g t2, qvv = q_clk_g dt.
 *   4 slots        slot j is usable as in gpsx_wfix's step 1 without the lock record (observable VALID, record VALID).  It may
 *                  give a pseudorange row if d_lock is NULL or its lock record has GPSX_WLOCK_CODE, and a Doppler row if d_lock is
 *                  NULL or that record has GPSX_WLOCK_CARRIER, and its if_freq_offset_hz is finite.  Both need svh == 0.
 *   5 satellite    one evaluation per slot at the transmit time its own clock reads, gpsx_wvel's step 2 with tx_ms + k_j in tx_ms'
 *                  place (k_j = 0 at first: step 7): t_sv, tc, t, tk, position ps, velocity vs and clock rate d', no satellite
 *                  if |tk| > 7201, A <= 0 or Kepler's iteration needs 30 steps.  The clock offset is gpsx_wfix's
 *                  dts = poly(fold(t - toc)) - 2 sqrt(mu A) e sin E / c^2 (without its "dts == 0" fallback), tgd = c * the record's,
 *                  the URA variance gpsx_wfix's table (sva outside 0 .. 14: 6144 m), squared.
 *   6 rows         the pseudorange, gpsx_wobs_pseudoranges' formula with rcv_ms in the reference's place, int64 and single double
 *                  operations, no reference slot and no offset_ms:
 *                    pr_j = 299792458e-3 * ((double)fold_ms(rcv_ms - (tx_ms_j + k_j)) + (double)code_phase_fine_j / 16368.0)
 *                  (fold_ms: gpsx_wobs_pseudoranges' fold into -W/2 .. W/2 - 1).  The pseudorange row is gpsx_wfix's row at x-
 *                  (step 4 there): no row if |ps| < Re, rho = range + Sagnac <= 0, el < 0; ecef2pos of x-_0..2 (30 steps at most),
 *                  Klobuchar with cfg.ion[] (all zero: the default set) at tow = (double)rcv_ms / 1000, Saastamoinen at humidity
 *                  0.7;  v = (pr - tgd) - (rho + dion + dtrp + x-_3 - c dts),  h = (-e, 1) on states 0 .. 3,
 *                  sig2 = gpsx_wfix's four variance terms (in its order) + sig_pr_m^2.
 *                  The Doppler row is gpsx_wvel's step 3 with rr = x-_0..2: no row if the range is 0; a_j on states 4 .. 7,
 *                  y = gpsx_wvel's y_j - (a_j . x-_4..7) (ascending), sig2 = sig_dop_mps^2; f_j and the code phase are age_blocks
 *                  old and are not extrapolated, as in the solvers.
 *   7 repair       a slot with GPSX_WOBS_AMBIGUOUS that gives a pseudorange row: k = (int)rint(v / ms).  |k| > 1: the row is
 *                  rejected (rej_pr_mask).  k = +-1: k_j = k, bit j of plus_mask / minus_mask (gpsx_wfde's convention: tx_ms is
 *                  corrected by k_j), and steps 5 and 6 are evaluated ONCE more for this slot at tx_ms + k_j -- both rows, without
 *                  a second repair -- so a repaired slot gives bit for bit what the unshifted observable would.
 *   8 gate         every row: s = h P- h^T + sig2 (over the row's 4 x 4 block, sum_i h_i (sum_j P-_ij h_j)), rejected if
 *                  v v > (gate gate) s or if v or s is not finite (rej_pr_mask / rej_dop_mask); the two rows of a slot are judged
 *                  apart.  n_pr, n_dop, pr_mask, dop_mask: the accepted rows.  nis_pr = sum v v / s over them, nis_dop likewise.
 *   9 update       information form, independent of the rows' order: with I = sum h^T h / sig2 (the upper-left 4 x 4 block from the
 *                  pseudorange rows, the lower-right from the Doppler rows: 10 + 10 sums, each term (h_i h_j) / sig2) and
 *                  g = sum h^T v / sig2 (4 + 4, each term (h_i v) / sig2):  L = (P-)^-1 + I,  P+ = L^-1,  x+ = x- + P+ g.
 *                  Both inverses by INV below.  No accepted row at all: x+ = x-, P+ = P-, COAST.  Otherwise UPDATED.
 *                  INV(N), 8 x 8: Cholesky N = L L^T column by column, p_j = N_jj - l_j0^2 - ... - l_j,j-1^2, gpsx_wfix's pivot rule
 *                  (p_0 <= 0 or p_j <= 1e-10 N_jj fails), l_jj = sqrt(p_j), l_ij = (N_ij - l_i0 l_j0 - ... ) / l_jj; M = L^-1 with
 *                  m_jj = 1 / l_jj, m_ij = -(l_ij m_jj + ... + l_i,i-1 m_i-1,j) / l_ii; N^-1_ij = the sum over
 *                  k = max(i, j) .. 7 of m_ki m_kj.  A failed pivot in either: LOST -- of an update, that is: without an accepted
 *                  row nothing is inverted that counts, and a P- that would fail coasts until a row arrives.
 *  10 starvation   no accepted pseudorange row: n_starved += 1, else n_starved = 0.  n_starved > max_coast: LOST.
 *  11 steering     x+_3 > ms / 2: x+_3 -= ms, rcv_ms -= 1 (rcv_ms < 0: += W, week -= 1); x+_3 < -ms / 2: x+_3 += ms, rcv_ms += 1
 *                  (rcv_ms >= W: -= W, week += 1); STEERED; once per call.  The pseudoranges of the next call follow rcv_ms.
 *  12 output       rr = x+_0..2, clk_m = x+_3, vel = x+_4..6, cdrift_mps = x+_7, geo = ecef2pos(rr), enu = vel in the east / north /
 *                  up frame at geo (gpsx_wvel's formula), sigma[i] = (float)sqrt(P+_ii), the counts, masks and sums of steps 7 - 9,
 *                  rcv_ms, week, n_starved.  flags: exactly one of INIT / NOT_INIT / UPDATED / COAST / LOST / BAD, and with UPDATED or
 *                  COAST the modifiers REPAIRED (a plus or minus bit), REJECTED (a reject bit), STEERED.  INIT fills rr .. sigma,
 *                  rcv_ms and week.  Anything in x+, P+, geo, enu, sigma, nis_pr or nis_dop that is not finite: LOST.  A LOST,
 *                  NOT_INIT or BAD record is zero but for its flag.  LOST clears the state to "not initialised": everything zero
 *                  but n_init and n_lost (+= 1); a later call re-initialises it from d_fix.  Every byte of d_kf is written, the
 *                  state of a receiver that is neither BAD nor NOT_INIT is written whole, nothing non-finite is written to either.
 * Errors (GPSX_EINVAL with a gpsx_last_error text, nothing written): NULL ctx / cfg / d_obs / d_eph / d_state / d_kf, ch_per_rx
 * outside 1 .. 64, n_rx outside 1 .. 1 048 576, n_blocks outside 1 .. 4096, max_coast outside 0 .. 1 000 000, gate not finite or outside
 * (0, 100], sig_dop_mps not finite or <= 0, sig_pr_m, a q_* or a p0_* not finite or negative, a p0_* of 0, mps_per_hz not finite or 0,
 * an ion[] not finite, a reserved word != 0, a d_state (both variants: it is device memory in both) or a d_kf (_dev) that is not
 * 16-byte aligned, a byte count that overflows.
 * Vector ALU, FP64 (k_wkf: gpsx_wfix's lane layout, a slot per lane; the 28 sums of I and g and the two of the NIS by
 * xor-butterflies of width W; P-, the two INVs and P+ in every lane of the group, in registers; every loop bounded, every cross-lane
 * operation under wave-uniform control flow).  On one stream: ..., gpsx_wfix_dev or gpsx_wfde_dev, gpsx_wvel_dev, then gpsx_wkf_dev. */
#define GPSX_WKF_INIT        1u   /* the state was initialised from d_fix (and d_vel) in this call; no update */
#define GPSX_WKF_NOT_INIT    2u   /* not initialised and no FIX record offered */
#define GPSX_WKF_UPDATED     4u   /* prediction and an update with n_pr + n_dop >= 1 rows */
#define GPSX_WKF_COAST       8u   /* prediction alone: no row was accepted */
#define GPSX_WKF_LOST       16u   /* a pivot failed, a result was not finite or n_starved > max_coast: the state is cleared */
#define GPSX_WKF_BAD        32u   /* the state was out of range: it is untouched, the record is otherwise zero */
#define GPSX_WKF_REPAIRED   64u   /* modifier: a plus or minus bit is set */
#define GPSX_WKF_REJECTED  128u   /* modifier: a bit of rej_pr_mask or rej_dop_mask is set */
#define GPSX_WKF_STEERED   256u   /* modifier: rcv_ms moved by a millisecond, clk_m by -+ 299 792.458 m */
#define GPSX_WKF_STATE_INIT  1u   /* gpsx_wkf_state_t.flags: x, P, rcv_ms and week hold a filter */

typedef struct {                 /* 176 bytes */
  double   ion[8];               /*   0  Klobuchar a0..a3, b0..b3, finite; all zero: the 2004 default set */
  double   mps_per_hz;           /*  64  as gpsx_wvel_cfg_t's: finite, not 0 */
  double   sig_pr_m;             /*  72  >= 0: receiver pseudorange noise, added to gpsx_wfix's variance terms */
  double   sig_dop_mps;          /*  80  > 0: range-rate noise of a Doppler row */
  double   gate;                 /*  88  (0, 100]: rows with |v| > gate sqrt(s) are rejected */
  double   q_acc;                /*  96  >= 0, m^2/s^3 per position axis */
  double   q_clk_f, q_clk_g;     /* 104  >= 0: clock phase (m^2/s) and frequency (m^2/s^3) noise */
  double   p0_pos, p0_clk, p0_vel, p0_drift;   /* 120  > 0: the initial standard deviations, m and m/s */
  int32_t  ch_per_rx;            /* 152  1 .. 64 */
  int32_t  max_coast;            /* 156  0 .. 1 000 000: launches without a pseudorange row before LOST */
  int32_t  reserved[4];          /* 160  0 */
} gpsx_wkf_cfg_t;

typedef struct {                 /* 384 bytes, one per receiver, resident in device memory; all zero: a fresh receiver */
  double   x[8];                 /*   0  x, y, z, b, vx, vy, vz, d */
  double   P[36];                /*  64  upper triangle, row by row */
  int64_t  rcv_ms;               /* 352  0 .. 604 799 999 */
  int32_t  week;                 /* 360 */
  uint32_t flags;                /* 364  GPSX_WKF_STATE_INIT */
  uint32_t n_starved;            /* 368  launches in a row without an accepted pseudorange row */
  uint32_t n_init, n_lost;       /* 372  counters (mod 2^32): initialisations, losses */
  uint32_t reserved;             /* 380  0 */
} gpsx_wkf_state_t;

typedef struct {                 /* 240 bytes, one per receiver and launch */
  uint32_t flags;                /*   0 */
  int32_t  n_pr, n_dop;          /*   4  accepted rows */
  uint32_t n_starved;            /*  12 */
  uint64_t pr_mask, dop_mask;    /*  16  bit j: slot j's row was accepted */
  uint64_t rej_pr_mask, rej_dop_mask;   /*  32  bit j: slot j's row was formed and rejected (|k| > 1 or the gate) */
  uint64_t plus_mask, minus_mask;/*  48  slots whose tx_ms was corrected by +1 / -1 ms */
  double   rr[3];                /*  64  ECEF, m */
  double   clk_m;                /*  88  b = c (receiver clock - GPS time), m */
  double   vel[3];               /*  96  ECEF, m/s */
  double   cdrift_mps;           /* 120  d, m/s */
  double   geo[3];               /* 128  latitude, longitude (rad), height (m) of rr */
  double   enu[3];               /* 152  vel in the east / north / up frame at geo */
  float    sigma[8];             /* 176  sqrt(P_ii) */
  double   nis_pr, nis_dop;      /* 208  sum v^2 / s over the accepted rows */
  int64_t  rcv_ms;               /* 224  the state's, after this call */
  int32_t  week, reserved;       /* 232  the state's; 0 */
} gpsx_wkf_t;

/* d_obs, d_eph, d_lock (NULL: not consulted): [n_rx * ch_per_rx]; d_fix, d_vel (NULL: none offered): [n_rx]; d_kf: [n_rx]; all on the
 * device for _dev, all in host memory (staged through the arena; the call waits for its kernel) for gpsx_wkf.  d_state [n_rx] is
 * device memory in both.  n_blocks: what this launch's gpsx_wobs_dev call got. */
int gpsx_wkf_dev(gpsx_ctx *ctx, const gpsx_wkf_cfg_t *cfg, const gpsx_wobs_t *d_obs, const gpsx_weph_t *d_eph, const gpsx_wlock_t *d_lock,
                 const gpsx_wfix_t *d_fix, const gpsx_wvel_t *d_vel, int n_rx, int n_blocks, gpsx_wkf_state_t *d_state, gpsx_wkf_t *d_kf);
int gpsx_wkf(gpsx_ctx *ctx, const gpsx_wkf_cfg_t *cfg, const gpsx_wobs_t *obs, const gpsx_weph_t *eph, const gpsx_wlock_t *lock,
             const gpsx_wfix_t *fix, const gpsx_wvel_t *vel, int n_rx, int n_blocks, gpsx_wkf_state_t *d_state, gpsx_wkf_t *kf);

/* ---- EXTENSION, not in the reference: acquisition decisions and slot hand-over -- a weighted grid's records to channel states ---------
 * The stage between the front and the middle of the weighted chain: gpsx_wacq(_dev) sits behind a launch of gpsx_acq_grid_weighted
 * {,_ms,_coh,_hyb}_dev and in front of gpsx_track_loop_weighted_sync_multi_dev (or, with one receiver, the single-stream sync loops).
 * It reads the grid's records peaks[n_search][n_prn][n_dopp] where they are, decides per receiver which PRNs are there, picks a slot
 * for each and writes the hand-over into that slot's states -- and it frees the slots whose code the lock monitor has not found, so
 * that a lost channel is re-acquired by the next grid launch.  No peak record and no channel state crosses to the host.  The stage is
 * stateless; it changes no existing struct, kernel or definition (GPSX_VERSION stays 110).  Every decision is in integers; its float
 * arithmetic is two single-precision operations on one value (step 5).
 *
 * g is the description the grid call was given: n_search is n_rx (search s IS receiver s: the grid's search_stride_blocks and the
 * multi loop's rx_stride_blocks describe the same buffer), prns a HOST pointer, the Doppler grid the grid call's.  The channel of
 * receiver r's slot j is r * ch_per_rx + j, as in gpsx_track_loop_weighted_sync_multi.
 *
 * Definition, per receiver r (everything is an integer but step 5):
 *   1 best record   per PRN index p: d* = the LOWEST bin whose max_val is the row's greatest; M = that max_val, S = that record's
 *                   sum, tau = that record's phase
 *   2 detection     a PRN is detected iff M >= max(min_peak, 1) and (uint64)M * 16368 * det_den >= (uint64)det_num * S: the
 *                   record's own peak over its mean across the 16 368 phases, at least det_num / det_den.  Exact for any uint32
 *                   pair (the left side stays below 2^56).  `sum` is the grids' sum mod 2^32, so the statistic needs a mean E(tau)
 *                   below 2^18 = 2^32 / 16 384: noise at n_coh = 20 x n_seg = 128 is about 1.6 x 10^5
 *   3 slots         slot j holds a channel iff d_sync_state[r * ch_per_rx + j].loop.prn != GPSX_PRN_NONE.  A slot that holds a
 *                   channel is EVICTED iff evict_after_blocks > 0, its lock state's flags lack GPSX_WLOCK_CODE and its lock
 *                   state's blocks_seen >= evict_after_blocks (blocks_seen counts since the hand-over, which zeroes it).  KEPT
 *                   slots hold a channel and are not evicted; FREE slots are empty or evicted
 *   4 candidates    the detected PRNs that no kept slot holds (the others are TRACKED), ranked by M, greater first; equal M: the
 *                   lower PRN index first.  The k-th candidate goes to the k-th free slot in ascending slot order; candidates
 *                   beyond the free slots are DROPPED
 *   5 hand-over     the whole 448-byte sync state of the slot becomes zero but for loop.prn = the PRN, loop.if_freq_offset_hz =
 *                   f = (float)(dopp_min_hz + d* x dopp_step_hz), loop.if_freq_accum = 0 and loop.code_phase_fine = p, where
 *                     p = (float)tau
 *                     if code_per_hz != 0.0f && lead_blocks != 0:
 *                       p = p - (code_per_hz * f) * ((float)lead_blocks * 0.001f)     one IEEE single operation each, in the order
 *                                                                                      written, no contraction
 *                       one wrap as the loops': + 16368.0f if p < 0, else - 16368.0f if p >= 16368.0f (a sum that rounds onto
 *                       16368.0f stays, as in the loops' own definition)
 *                   An evicted slot that receives no candidate becomes the same zeroed state with loop.prn = GPSX_PRN_NONE.  For
 *                   every slot handed over or evicted the lock, nav, obs and eph states are set to zero, in each of the four
 *                   arrays that is not NULL (all zero is "a fresh channel" in all four).  Kept slots and empty slots that stay
 *                   empty are not written at all
 *   6 records       d_acq[r] is written as the struct says, d_det[r][p] for every p unless d_det is NULL; every byte of both
 * What lead_blocks is for: a record's phase belongs to the search's first block, the loop starts lead_blocks later (a 10 x 8 hybrid
 * search handed to a loop that starts behind it: 80), and a Doppler of f Hz has moved the code by f x code_per_hz samples per second
 * meanwhile.  code_per_hz is gpsx_waid_t's factor (GPSX_WAID_L1CA).
 * Errors, each GPSX_EINVAL with a gpsx_last_error text and nothing written: cfg, g, g->prns, the peaks, d_sync_state or d_acq NULL;
 * ch_per_rx, det_num, det_den, lead_blocks, evict_after_blocks or reserved out of range; code_per_hz not finite or above 1 in
 * magnitude; d_lock_state NULL while evict_after_blocks != 0; n_search outside 1 .. 1 048 576; n_prn outside 1 .. 64; n_dopp outside 1 .. 1 048 576; a
 * PRN outside 1 .. 210 or listed twice; a Doppler bin outside int32; |code_per_hz| x max |bin's Hz| x lead_blocks x 0.001 >= 16368
 * (checked on the host in double: one wrap suffices); size products that overflow.
 * _dev only enqueues on the context's stream: behind the grid, before the next loop launch.  Vector ALU (k_wacq: a wave per
 * receiver, four receivers per workgroup; a row's bins strided over the lanes, a 64-bit key (max_val, bin) reduced by butterflies;
 * slots and PRNs one per lane, matched and ranked with ballots, popcounts and shuffles; states written 8 bytes per lane). */
#define GPSX_WACQ_DET_DETECTED 1u
#define GPSX_WACQ_DET_TRACKED  2u    /* detected, but a kept slot of this receiver already holds the PRN */
#define GPSX_WACQ_DET_ASSIGNED 4u
#define GPSX_WACQ_DET_DROPPED  8u    /* a candidate that found no free slot */
#define GPSX_WACQ_ASSIGNED 1u
#define GPSX_WACQ_EVICTED  2u
#define GPSX_WACQ_FULL     4u        /* n_dropped > 0 */

typedef struct {                 /* 32 bytes */
  int32_t  ch_per_rx;            /* 1 .. 64 */
  int32_t  det_num, det_den;     /* 1 .. 1024, det_num >= det_den */
  uint32_t min_peak;             /* a detection also needs max_val >= max(min_peak, 1) */
  int32_t  lead_blocks;          /* 0 .. 4096: blocks from the instant the record's phase belongs to, to the loop's first block */
  float    code_per_hz;          /* as gpsx_waid_t's; 0: the phase is not projected */
  int32_t  evict_after_blocks;   /* 0: never; 1 .. 2^30 */
  int32_t  reserved;             /* 0 */
} gpsx_wacq_cfg_t;

typedef struct {                 /* 16 bytes, one per (receiver, PRN index) */
  uint32_t max_val, phase;       /* the PRN's best record */
  int32_t  dopp_hz;              /* its bin */
  uint8_t  flags;  int8_t slot;  /* GPSX_WACQ_DET_*; the slot handed over to, else -1 */
  uint16_t zero;
} gpsx_wacq_det_t;

typedef struct {                 /* 64 bytes, one per receiver */
  uint32_t flags, n_detected, n_tracked, n_assigned, n_evicted, n_dropped;   /*  0 */
  uint64_t assigned_mask, evicted_mask, kept_mask, free_mask;                /* 24: bit j = slot j; free_mask: after the call */
  uint32_t reserved[2];                                                      /* 56: 0 */
} gpsx_wacq_t;

/* d_peaks [n_search][n_prn][n_dopp]; the five state arrays [n_search * ch_per_rx], device memory in both variants (d_lock_state NULL
 * only with evict_after_blocks == 0; d_nav_state, d_obs_state, d_eph_state NULL: not touched); d_acq [n_search], d_det (NULL: not
 * wanted) [n_search][n_prn].  gpsx_wacq takes peaks, acq and det in host memory (staged through the arena; it waits for its kernel). */
int gpsx_wacq_dev(gpsx_ctx *ctx, const gpsx_wacq_cfg_t *cfg, const gpsx_acq_weighted_t *g, const gpsx_peak_t *d_peaks,
                  gpsx_wsync_state_t *d_sync_state, gpsx_wlock_state_t *d_lock_state, gpsx_wnav_state_t *d_nav_state,
                  gpsx_wobs_state_t *d_obs_state, gpsx_weph_state_t *d_eph_state, gpsx_wacq_t *d_acq, gpsx_wacq_det_t *d_det);
int gpsx_wacq(gpsx_ctx *ctx, const gpsx_wacq_cfg_t *cfg, const gpsx_acq_weighted_t *g, const gpsx_peak_t *peaks,
              gpsx_wsync_state_t *d_sync_state, gpsx_wlock_state_t *d_lock_state, gpsx_wnav_state_t *d_nav_state,
              gpsx_wobs_state_t *d_obs_state, gpsx_weph_state_t *d_eph_state, gpsx_wacq_t *acq, gpsx_wacq_det_t *det);

/* ---- EXTENSION, not in the reference: the ephemeris bank -- a receiver's decoded orbits outlive the slots that decoded them ---------
 * gpsx_weph keeps a satellite's subframes in the state of the slot that tracks it, and gpsx_wacq zeroes that state on every hand-over
 * and eviction.  A satellite that is lost for ten seconds therefore comes back as a channel without an ephemeris for another 18 .. 30 s,
 * although its orbit was decoded minutes ago and holds for two hours.  gpsx_wbank(_dev) sits behind gpsx_weph_dev: it keeps, per
 * receiver and PRN of a list, the newest VALID record any slot has produced, in d_bank[n_rx][n_prn] (device resident, owned by the
 * caller; all zero = empty), and gives a slot that tracks a listed PRN without a VALID set of its own the bank's in a merged copy of
 * the launch's records.  The solvers and gpsx_wkf take that copy in d_eph's place.  It changes no existing struct, kernel or
 * definition (GPSX_VERSION stays 110).  Integers only: records are moved, never evaluated.
 *
 * prns is a HOST pointer to n_prn PRN numbers, as gpsx_acq_weighted_t's, passed to the kernel by value; PRN index p is its position
 * in the list.  The channel of receiver r's slot j is r * ch_per_rx + j.  d_sync_state is only read (for loop.prn).
 *
 * Definition, per receiver r:
 *   1 offer     slot j's PRN is d_sync_state[r * ch_per_rx + j].loop.prn; p_j is its index in prns (GPSX_PRN_NONE and a PRN that
 *               is not listed have none).  Slot j OFFERS iff it has an index and d_eph[r * ch_per_rx + j].flags has GPSX_WEPH_VALID
 *   2 store     among the offers for one index p the greatest toe_time wins, among equal toe_time the lowest slot.  d_bank[r][p] is
 *               replaced by the winner iff the bank's record lacks GPSX_WEPH_VALID or the winner's toe_time >= the bank's: an older
 *               set never pushes out a newer one; an equal one refreshes ttr (and is counted as stored).  What is stored is the
 *               slot's record byte for byte but for flags = GPSX_WEPH_VALID (NEW is cleared)
 *   3 merge     d_eph_out[r * ch_per_rx + j] is d_eph's record unchanged if that has VALID or the slot has no index; otherwise
 *               d_bank[r][p_j] as step 2 left it, byte for byte, if that has VALID (the slot is FROM THE BANK); otherwise d_eph's
 *               record unchanged
 *   4 report    d_rep[r] as the struct says, every byte written
 * d_eph_out NULL: no merged copy is wanted.  d_eph_out == d_eph: the merge happens in place (only FROM THE BANK records are written).
 * Errors, each GPSX_EINVAL with a gpsx_last_error text and nothing written: cfg, prns, d_sync_state, d_eph, d_bank or d_rep NULL;
 * ch_per_rx outside 1 .. 64; a reserved word != 0; n_rx outside 1 .. 1 048 576; n_prn outside 1 .. 64; a PRN outside 1 .. 210 or
 * listed twice; d_sync_state not 8-byte aligned, d_bank or (in _dev) d_eph, d_eph_out, d_rep not 16-byte aligned; two of the five
 * arrays overlapping other than d_eph_out == d_eph; size products that overflow.
 * _dev only enqueues on the context's stream: behind gpsx_weph_dev, before the solvers.  Vector ALU (k_wbank: a wave per receiver,
 * four receivers per workgroup, no LDS; slots and PRN indices one per lane, matched with shuffles and ballots; records moved by half
 * a wave each, 8 bytes per lane, two records a turn; no record is read back in the call that stored it). */
typedef struct {                 /* 16 bytes */
  int32_t ch_per_rx;             /* 1 .. 64 */
  int32_t reserved[3];           /* 0 */
} gpsx_wbank_cfg_t;

typedef struct {                 /* 32 bytes, one per receiver */
  uint64_t stored_mask;          /*  0  bit p: d_bank[r][p] was replaced in this call */
  uint64_t have_mask;            /*  8  bit p: d_bank[r][p] has GPSX_WEPH_VALID after it */
  uint64_t from_bank_mask;       /* 16  bit j: slot j's merged record is the bank's (also counted when d_eph_out is NULL) */
  uint16_t n_stored, n_have, n_from_bank, zero;   /* 24  the masks' bit counts; 0 */
} gpsx_wbank_t;

/* d_sync_state [n_rx * ch_per_rx] and d_bank [n_rx][n_prn]: device memory in both variants.  d_eph, d_eph_out (NULL: not wanted; may be
 * d_eph itself) [n_rx * ch_per_rx] and d_rep [n_rx]: device memory; gpsx_wbank takes eph, eph_out and rep in host memory (staged
 * through the arena; it waits for its kernel). */
int gpsx_wbank_dev(gpsx_ctx *ctx, const gpsx_wbank_cfg_t *cfg, int n_rx, int n_prn, const uint8_t *prns,
                   const gpsx_wsync_state_t *d_sync_state, const gpsx_weph_t *d_eph, gpsx_weph_t *d_bank, gpsx_weph_t *d_eph_out,
                   gpsx_wbank_t *d_rep);
int gpsx_wbank(gpsx_ctx *ctx, const gpsx_wbank_cfg_t *cfg, int n_rx, int n_prn, const uint8_t *prns,
               const gpsx_wsync_state_t *d_sync_state, const gpsx_weph_t *eph, gpsx_weph_t *d_bank, gpsx_weph_t *eph_out,
               gpsx_wbank_t *rep);

/* ---- EXTENSION, not in the reference: prediction and hot hand-over -- from the filter's state and the bank back to the slots ---------
 * gpsx_wkf holds every receiver's position, clock, velocity and drift; with an ephemeris that fixes the code phase of any satellite
 * to a fraction of a sample and its Doppler to a fraction of a hertz.  gpsx_wpred(_dev) sits behind gpsx_wkf_dev and in front of the
 * next loop launch: for every (receiver, PRN index) of the bank's list it computes elevation, azimuth, pseudorange, code phase and
 * Doppler at the loop's next block, and hands the satellites that are above el_min_rad, known well enough and tracked by no slot
 * straight to free slots, with no grid launch; no record and no state crosses to the host.  d_kf_state and d_bank are only read.
 * The slot bookkeeping (steps 5 - 7) is gpsx_wacq's, so the two stages can be called in either order on one stream.  Nothing existing
 * changes (GPSX_VERSION stays 110).
 *
 * Definition, per receiver r; all arithmetic in IEEE double, uncontracted, with gpsx_wkf's constants (c, ms = 299792.458, W =
 * 604 800 000, we, Re) and sum orders; P_ij names the state's element as there.
 *   0 state        without GPSX_WKF_STATE_INIT: NOT_INIT.  A state gpsx_wkf's step 0 would call BAD: BAD.  In either case d_rx[r] and
 *                  every d_pred[r][p] are zero but for that flag, no slot is read or written, and the call still returns 0: only the
 *                  filter reports a bad state as an error.
 *   1 epoch        T = rcv_ms + lead_blocks; T >= W: T -= W, week += 1.  dt = (double)lead_blocks * 1e-3; x^_i = x_i + dt x_(4+i),
 *                  i = 0 .. 3; x^_4..7 = x_4..7.  P^ is gpsx_wkf step 3's three blocks WITHOUT the q terms (what is known, not what
 *                  the filter fears): with lead_blocks == 0 it is P.  lat, lon, hgt = ecef2pos of x^_0..2 (30 steps at most).
 *   2 satellite    for every PRN index p whose bank record has GPSX_WEPH_VALID (HAVE_EPH) and svh == 0, exactly three passes, no
 *     and range    convergence test.  pr_0 = 72 ms (72 x 299792.458 m).  Pass k = 0, 1, 2:
 *                    t_sv = ((double)T - pr_k / ms) / 1000, seconds of the week
 *                    the satellite at its own clock's reading t_sv as in gpsx_wkf's step 5 (ps, vs, d', dts, tgd = c x the
 *                      record's); the pass fails if |tk| > 7201, A <= 0 or Kepler's iteration needs 30 steps
 *                    l = ps - x^_0..2, range = |l|; the pass fails if range == 0, |ps| < Re or rho = range + we (ps_x x^_1 - ps_y
 *                      x^_0) / c <= 0;  e = l / range;  az, el at (lat, lon, hgt) as gpsx_wfix
 *                    dion = Klobuchar(cfg.ion or the default set, tow = (double)T / 1000), dtrp = Saastamoinen(humidity 0.7); both
 *                      are 0 where el <= 0 (the models' own rule), so a satellite below the horizon is still predicted
 *                    pr_(k+1) = (rho + dion + dtrp + x^_3 - c dts) + tgd: the pseudorange for which gpsx_wkf's step 6 has v = 0
 *                  The last pass's ps, vs, d', e, el, az count.  Why three: pass k+1 is wrong by (range rate / c) <= 3e-6 of what
 *                  pass k was wrong by (the satellite moves at most 800 m/s along the line of sight during the error in time).  The
 *                  first guess is off by 20 ms = 6e6 m at most (ranges are 67 .. 86 ms); that leaves 18 m after the first pass,
 *                  5e-5 m after the second and below 1e-9 m after the third, under the round-off of a 2e7 m range in doubles (4e-9).
 *   3 observables  u = pr_3 / ms, q = floor(u), code_phase = (u - q) x 16368; tx_ms = (T - q) folded into 0 .. W - 1: gpsx_wobs_t's
 *                  convention (transmit time at sample 0 = tx_ms - code_phase / 16368 ms).  The Doppler in the loop's units is
 *                  gpsx_wvel's step 3 read backwards, with rr = x^_0..2, a = (-e_x - k ps_y, -e_y + k ps_x, -e_z, 1), k = we / c:
 *                    f_hz = ((a_0 x^_4 + a_1 x^_5 + a_2 x^_6 + x^_7) + (e . vs + k (vs_x rr_y - vs_y rr_x) - c d')) / mps_per_hz
 *                  s_pr = h P^ h^T over states 0 .. 3 with h = (-e, 1), in gpsx_wkf step 8's order (sum_i h_i (sum_j P^_ij h_j),
 *                  no sig2); s_f = (a P_vv a^T) / (mps_per_hz mps_per_hz) over states 4 .. 7 in the same order.
 *   4 flags        HAVE_EPH; PREDICTED: three passes that did not fail and pr_3, code_phase, f_hz, el, az, s_pr, s_f and both float
 *                  sigmas finite (a negative s gives none); VISIBLE: PREDICTED and el >= el_min_rad; CERTAIN: PREDICTED and
 *                  s_pr <= max_sigma_m^2 and s_f <= max_sigma_hz^2; TRACKED: a kept slot (step 5) holds the PRN, whatever is known
 *                  of it.  Nothing non-finite is ever written; a PRN without PREDICTED has zeros beside its flags and slot = -1.
 *   5 slots        gpsx_wacq's step 3, word for word: slot j holds a channel iff its loop.prn != GPSX_PRN_NONE; it is EVICTED iff
 *                  evict_after_blocks > 0, its lock state's flags lack GPSX_WLOCK_CODE and its blocks_seen >= evict_after_blocks;
 *                  KEPT slots hold a channel and are not evicted; FREE slots are empty or evicted.
 *   6 candidates   the PRNs that are VISIBLE and CERTAIN and not TRACKED, ranked by el, greater first; equal el: the lower index
 *                  first.  handover == 1: the k-th goes to the k-th free slot in ascending order (ASSIGNED, slot), those beyond the
 *                  free slots are DROPPED.  handover == 0: nothing is assigned, dropped or written; evicted slots stay as they are
 *                  (evicted_mask still names them, free_mask is the free slots).
 *   7 hand-over    gpsx_wacq's step 5 with loop.if_freq_offset_hz = (float)f_hz and loop.code_phase_fine = (float)code_phase (a cast
 *                  that lands on 16368.0f stays, as there) and no projection: step 1 already stands at the loop's first block.  The
 *                  slot's whole sync state is otherwise zero, its lock, nav, obs and eph states are zeroed where given; an evicted
 *                  slot without a candidate becomes GPSX_PRN_NONE; kept slots and empty slots that stay empty are not written.
 *   8 records      d_pred[r][p] (unless NULL) and d_rx[r] as the structs say, every byte of both written.
 * Errors, each GPSX_EINVAL with a gpsx_last_error text and nothing written: cfg, prns, d_kf_state, d_bank, d_sync_state or d_rx NULL;
 * an ion[] not finite; mps_per_hz not finite or 0; el_min_rad not finite or outside +-pi/2; max_sigma_m or max_sigma_hz not finite
 * or <= 0; ch_per_rx outside 1 .. 64; lead_blocks outside 0 .. 4096; evict_after_blocks outside 0 .. 2^30; handover not 0 or 1; a
 * reserved word != 0; d_lock_state NULL while evict_after_blocks != 0; n_rx outside 1 .. 1 048 576; n_prn outside 1 .. 64; a PRN
 * outside 1 .. 210 or listed twice; d_kf_state or d_bank not 16-byte aligned, d_rx or d_pred not 16-byte aligned (_dev); size
 * products that overflow.
 * _dev only enqueues.  Vector ALU, FP64 (k_wpred: a wave per receiver, four receivers per workgroup, no LDS; lane p is PRN index p
 * for steps 2 - 4 -- one satellite evaluation per lane and pass -- and lane j is slot j for steps 5 - 7, with gpsx_wacq's ballots,
 * shuffles and popcounts; states written 8 bytes per lane).  On one stream: ..., gpsx_weph_dev, gpsx_wbank_dev, the solvers on
 * d_eph_out, gpsx_wkf_dev, gpsx_wpred_dev, then the next loop launch lead_blocks after the filter's rcv_ms. */
#define GPSX_WPRED_HAVE_EPH    1u
#define GPSX_WPRED_PREDICTED   2u
#define GPSX_WPRED_VISIBLE     4u
#define GPSX_WPRED_CERTAIN     8u
#define GPSX_WPRED_TRACKED    16u
#define GPSX_WPRED_ASSIGNED   32u
#define GPSX_WPRED_DROPPED    64u
#define GPSX_WPRED_RX_PREDICTED 1u   /* the state is a filter's: the PRNs were looked at */
#define GPSX_WPRED_RX_NOT_INIT  2u
#define GPSX_WPRED_RX_BAD       4u
#define GPSX_WPRED_RX_ASSIGNED  8u
#define GPSX_WPRED_RX_EVICTED  16u
#define GPSX_WPRED_RX_FULL     32u   /* n_dropped > 0 */

typedef struct {                 /* 128 bytes */
  double  ion[8];                /*   0  as gpsx_wkf_cfg_t's */
  double  mps_per_hz;            /*  64  as gpsx_wkf_cfg_t's: finite, not 0 */
  double  el_min_rad;            /*  72  finite, -pi/2 .. pi/2 */
  double  max_sigma_m;           /*  80  > 0: CERTAIN needs sqrt(s_pr) <= this */
  double  max_sigma_hz;          /*  88  > 0: ... and sqrt(s_f) <= this */
  int32_t ch_per_rx;             /*  96  1 .. 64 */
  int32_t lead_blocks;           /* 100  0 .. 4096: blocks from the filter's rcv_ms to the loop's first block */
  int32_t evict_after_blocks;    /* 104  0: never; 1 .. 2^30 */
  int32_t handover;              /* 108  0: predict only; 1: write slots */
  int32_t reserved[4];           /* 112  0 */
} gpsx_wpred_cfg_t;

typedef struct {                 /* 64 bytes, one per (receiver, PRN index) */
  uint32_t flags;  int32_t slot; /*   0  GPSX_WPRED_*; the slot handed over to, else -1 */
  int64_t  tx_ms;                /*   8  0 .. W - 1 */
  double   pr_m, code_phase, f_hz, el, az;   /*  16  pr_3 (m), samples 0 .. 16368, the loop's Hz, rad */
  float    sigma_m, sigma_hz;    /*  56  (float)sqrt(s_pr), (float)sqrt(s_f) */
} gpsx_wpred_t;

typedef struct {                 /* 64 bytes, one per receiver */
  uint16_t flags;  int16_t week; /*   0  GPSX_WPRED_RX_*; the week of T */
  int32_t  t_ms;                 /*   4  T */
  uint8_t  n_have, n_visible, n_tracked, n_assigned, n_evicted, n_dropped;   /*  8 */
  uint16_t zero;                 /*  14 */
  uint64_t visible_mask, have_mask;   /*  16  bit p = PRN index p: VISIBLE; HAVE_EPH.  OR visible_mask over receivers: the next grid's PRNs */
  uint64_t assigned_mask, evicted_mask, kept_mask, free_mask;   /*  32  bit j = slot j, as gpsx_wacq_t's; free_mask: after the call */
} gpsx_wpred_rx_t;

/* d_kf_state [n_rx], d_bank [n_rx][n_prn] and the five state arrays [n_rx * ch_per_rx] (NULL rules as gpsx_wacq's): device memory in
 * both variants.  d_rx [n_rx], d_pred (NULL: not wanted) [n_rx][n_prn]: device memory; gpsx_wpred takes them in host memory. */
int gpsx_wpred_dev(gpsx_ctx *ctx, const gpsx_wpred_cfg_t *cfg, int n_rx, int n_prn, const uint8_t *prns, const gpsx_wkf_state_t *d_kf_state,
                   const gpsx_weph_t *d_bank, gpsx_wsync_state_t *d_sync_state, gpsx_wlock_state_t *d_lock_state, gpsx_wnav_state_t *d_nav_state,
                   gpsx_wobs_state_t *d_obs_state, gpsx_weph_state_t *d_eph_state, gpsx_wpred_rx_t *d_rx, gpsx_wpred_t *d_pred);
int gpsx_wpred(gpsx_ctx *ctx, const gpsx_wpred_cfg_t *cfg, int n_rx, int n_prn, const uint8_t *prns, const gpsx_wkf_state_t *d_kf_state,
               const gpsx_weph_t *d_bank, gpsx_wsync_state_t *d_sync_state, gpsx_wlock_state_t *d_lock_state, gpsx_wnav_state_t *d_nav_state,
               gpsx_wobs_state_t *d_obs_state, gpsx_weph_state_t *d_eph_state, gpsx_wpred_rx_t *rx, gpsx_wpred_t *pred);

/* ---- EXTENSION, not in the reference: time-of-week aiding of the observables -- the prediction names the millisecond a HOW has not yet ---
 * gpsx_wobs marks a slot VALID only once a parity-checked HOW of its chain has anchored the time of week: 1.2 .. 7.2 s after the bit
 * sync of every hand-over, eviction and chain break, and never for a satellite whose words fail parity.  gpsx_wpred's record for that
 * PRN already holds the transmit millisecond at the same block, good to a few samples, where the question is only "which millisecond"
 * and a millisecond is 16 368 samples wide.  gpsx_wtow(_dev) sits behind gpsx_wobs_dev and a gpsx_wpred_dev call and anchors, from
 * that record, the observable state of every slot whose bit chain runs (PHASE and EDGE) but has no TOW; it resolves
 * GPSX_WOBS_AMBIGUOUS on the way, where the prediction says that the edge block is the other "nearest block start".  A HOW stays the
 * authority: an anchor it set is never replaced here, and the next real HOW confirms an aided anchor or replaces it with
 * n_mismatch++, by gpsx_wobs' own rule.  No existing struct, kernel, definition or state rule changes; the aided state uses only flag
 * bits gpsx_wobs already knows (GPSX_VERSION stays 110).
 *
 * THE EPOCHS ARE THE CALLER'S DUTY.  The epoch T of the gpsx_wpred_dev call whose records are read (the filter's rcv_ms + its
 * lead_blocks) must be the clock's reading of sample 0 of block B, the block the observable states stand at (their blocks_seen).  The
 * stage cannot check it: a slot's blocks_seen restarts at every hand-over.  Two call orders are valid:
 *   after gpsx_wkf_dev    ..., gpsx_wobs_dev, ..., gpsx_wkf_dev, gpsx_wpred_dev with lead_blocks = 0, gpsx_wtow_dev: the aided slot counts
 *                         from the next launch on (d_obs may still be given: the records then say what the next launch will see).
 *   before gpsx_wkf_dev   ..., gpsx_wobs_dev, gpsx_wpred_dev with lead_blocks = n_blocks on the filter state of the launch before,
 *                         gpsx_wtow_dev with d_obs, the solvers, gpsx_wkf_dev: with d_obs rewritten the aided slot counts in this launch.
 *
 * Definition, per receiver r and slot j, ch = r * ch_per_rx + j, W = 604 800 000; all integers are int64, step 3 is three IEEE double
 * operations.  The first clause that holds ends the slot with that flag; a flag named in capitals is GPSX_WTOW_<name>.
 *   0 receiver     d_pred_rx[r].flags lacks GPSX_WPRED_RX_PREDICTED: NO_PRED.  d_tow_rx[r] and every d_tow[ch] are zero but for that
 *                  flag, no state is read or written.
 *   1 slot         d_sync_state[ch].loop.prn == GPSX_PRN_NONE: EMPTY.  The PRN is not in the list: UNLISTED; else p is its index.
 *                  The observable state is one gpsx_wobs calls BAD (its rule, its bounds): BAD, the state stays untouched and the
 *                  call still returns 0 -- only gpsx_wobs reports it as an error.  The state lacks PHASE or EDGE: WAITING.
 *                  blocks_seen - last_win_end_p1 > max_age_blocks: STALE (the code phase is older than the prediction may be held against).
 *   2 prediction   w = d_pred[r][p].  w.flags lacks GPSX_WPRED_PREDICTED, or (double)w.sigma_m > max_sigma_m: UNCERTAIN.
 *   3 millisecond  d = (double)last_phase - w.code_phase;  k = +1 if d > 8184, -1 if d < -8184, else 0;  rho = d - 16368 k (16368 k
 *                  is exact).  INCONSISTENT unless |rho| <= (double)max_resid_samples; a NaN fails this test (and is recorded as
 *                  the quiet NaN 0x7FC00000, whatever its sign and payload).  The loop's code phase and the predicted one are the
 *                  same edge seen across the ends of the 16 368-sample circle: k is the millisecond between them.
 *                  tx = (w.tx_ms + k) folded into 0 .. W - 1 (from a w.tx_ms in 0 .. W - 1, which gpsx_wpred writes; any other is
 *                  taken modulo W first);  Tz' = (tx - ((B mod W) - (Z mod W))) folded into 0 .. W - 1, B = blocks_seen, Z =
 *                  edge_block, both mods non-negative: the transmit millisecond at the edge of block Z;  m = Tz' mod 20.
 *   4 grid         a bit edge of this satellite is transmitted on a multiple of 20 ms.  m == 0: s = 0.  m == 1 or m == 19, and
 *                  AMBIGUOUS is set, and cfg.resolve: s = -1 for m == 1, s = +1 for m == 19, SHIFTED: Z* = Z + s, Tz* = (Tz' + s) mod
 *                  W, the other choice of "nearest block start".  (Without a shift Z* = Z, Tz* = Tz'.)  Anything else: OFF_GRID, the
 *                  bit synchroniser's edge is not a bit edge of this satellite, and nothing in the observable state changes; with
 *                  cfg.rearm and d_sync_state[ch].mode != 0 the sync state gets mode = 0, search_n = 0, prev_best_p1 = 0 (three
 *                  writes of gpsx_wlock's re-arm: the search starts again) and the record REARMED.
 *   5 anchor       on the grid.  No TOW: edge_block = Z*, tx_ms_at_edge = Tz*, TOW is set, AMBIGUOUS is cleared if cfg.resolve:
 *                  AIDED.  TOW and tx_ms_at_edge == Tz*: AGREES; with cfg.resolve edge_block = Z* and AMBIGUOUS is cleared (a
 *                  HOW-anchored chain whose edge block was chosen wrongly: Tz stays, Z moves).  TOW and they differ: DISAGREES,
 *                  nothing is written (SHIFTED then only says what step 4 found).  CONFIRMED, the four counters and every other
 *                  field stay as they are.
 *   6 observable   d_obs non-NULL and the state changed (AIDED, or AGREES with cfg.resolve from a state with AMBIGUOUS): d_obs[ch].tx_ms
 *                  = (Tz + B - Z) mod W and .flags = the state's flags | VALID, of the new state -- gpsx_wobs' output clause; PHASE,
 *                  EDGE and TOW all hold here.  The record's other fields and every other record are untouched.
 *   7 records      every byte of d_tow and d_tow_rx is written.  A slot's record: flags; prn_index = p, -1 for EMPTY and UNLISTED;
 *                  tx_ms = tx, resid = (float)rho, both 0 before step 3 (tx_ms also 0 for INCONSISTENT); m, -1 before step 3 and for
 *                  INCONSISTENT; shift = s.  A receiver's: the masks and their counts over its slots; valid_after: the slots that came
 *                  past EMPTY, UNLISTED and BAD whose state has PHASE, EDGE and TOW after the call.
 * A second call on the result finds AGREES where the first found AIDED, and changes nothing.
 * Errors, each GPSX_EINVAL with a gpsx_last_error text and nothing written: cfg, prns, d_pred_rx, d_pred, d_sync_state, d_obs_state,
 * d_tow or d_tow_rx NULL; max_sigma_m not finite or <= 0; max_resid_samples not finite, <= 0 or > 4092; max_age_blocks outside 0 ..
 * 4096; resolve or rearm not 0 or 1; reserved != 0; ch_per_rx outside 1 .. 64; n_rx outside 1 .. 1 048 576; n_prn outside 1 .. 64; a
 * PRN outside 1 .. 210 or listed twice; d_pred_rx, d_pred, d_obs_state or d_obs not 16-byte aligned, d_sync_state not 8-byte aligned,
 * d_tow or d_tow_rx not 16-byte aligned (_dev); size products that overflow; d_tow or d_tow_rx overlapping each other or an input.
 * _dev only enqueues.  Vector ALU (k_wtow: gpsx_wacq's geometry, a wave per receiver, four receivers per workgroup, lane j is slot j;
 * no LDS, no barrier; the 80-byte state is read as five 16-byte loads per lane and only the words that change are stored). */
#define GPSX_WTOW_NO_PRED         1u   /* the receiver has no prediction (step 0) */
#define GPSX_WTOW_EMPTY           2u
#define GPSX_WTOW_UNLISTED        4u
#define GPSX_WTOW_BAD             8u
#define GPSX_WTOW_WAITING        16u   /* no PHASE or no EDGE yet */
#define GPSX_WTOW_STALE          32u
#define GPSX_WTOW_UNCERTAIN      64u
#define GPSX_WTOW_INCONSISTENT  128u
#define GPSX_WTOW_OFF_GRID      256u
#define GPSX_WTOW_REARMED       512u   /* with OFF_GRID: the sync state was sent back to its search */
#define GPSX_WTOW_SHIFTED      1024u   /* the edge block is the other nearest block start: shift = +-1 */
#define GPSX_WTOW_AIDED        2048u   /* the anchor was written */
#define GPSX_WTOW_AGREES       4096u   /* a HOW's anchor says the same millisecond */
#define GPSX_WTOW_DISAGREES    8192u   /* ... another: the HOW stands */
#define GPSX_WTOW_RX_NO_PRED      1u
#define GPSX_WTOW_RX_AIDED        2u   /* n_aided > 0 */
#define GPSX_WTOW_RX_SHIFTED      4u   /* n_shifted > 0 */
#define GPSX_WTOW_RX_DISAGREES    8u   /* n_disagrees > 0 */
#define GPSX_WTOW_RX_OFF_GRID    16u   /* n_off_grid > 0 */
#define GPSX_WTOW_RX_REARMED     32u   /* a sync state was written */

typedef struct {                 /* 32 bytes */
  double  max_sigma_m;           /*  0  > 0, finite: a prediction with a greater sigma_m is UNCERTAIN */
  float   max_resid_samples;     /*  8  > 0 .. 4092: |rho| above it is INCONSISTENT */
  int32_t ch_per_rx;             /* 12  1 .. 64 */
  int32_t max_age_blocks;        /* 16  0 .. 4096: blocks_seen - last_win_end_p1 above it is STALE */
  int32_t resolve;               /* 20  0 / 1: move the edge block of an AMBIGUOUS chain where the prediction says so, clear AMBIGUOUS */
  int32_t rearm;                 /* 24  0 / 1: send the sync state of an OFF_GRID slot back to its search */
  int32_t reserved;              /* 28  0 */
} gpsx_wtow_cfg_t;

typedef struct {                 /* 32 bytes, one per slot */
  uint32_t flags;  int32_t prn_index;   /*  0  GPSX_WTOW_*; p, or -1 */
  int64_t  tx_ms;                /*  8  tx, or 0 */
  float    resid;                /* 16  (float)rho, samples */
  int32_t  m, shift;             /* 20  Tz' mod 20, or -1; s */
  uint32_t zero;                 /* 28 */
} gpsx_wtow_t;

typedef struct {                 /* 64 bytes, one per receiver */
  uint16_t flags;                /*  0  GPSX_WTOW_RX_* */
  uint8_t  n_aided, n_agrees, n_disagrees, n_off_grid, n_shifted, n_inconsistent;   /*  2  the popcounts of the first six masks */
  uint64_t aided_mask, agrees_mask, disagrees_mask, off_grid_mask, shifted_mask, inconsistent_mask;   /*  8  bit j = slot j */
  uint64_t valid_after_mask;     /* 56  step 7 */
} gpsx_wtow_rx_t;

/* d_pred_rx [n_rx] and d_pred [n_rx][n_prn]: what gpsx_wpred_dev wrote on the same list prns (n_prn PRN numbers, host memory in both
 * variants); d_sync_state (written only with cfg.rearm), d_obs_state and d_obs (NULL: no record is patched) [n_rx * ch_per_rx]: device
 * memory in both variants.  d_tow [n_rx * ch_per_rx], d_tow_rx [n_rx]: device memory; gpsx_wtow takes them in host memory. */
int gpsx_wtow_dev(gpsx_ctx *ctx, const gpsx_wtow_cfg_t *cfg, int n_rx, int n_prn, const uint8_t *prns, const gpsx_wpred_rx_t *d_pred_rx,
                  const gpsx_wpred_t *d_pred, gpsx_wsync_state_t *d_sync_state, gpsx_wobs_state_t *d_obs_state, gpsx_wobs_t *d_obs,
                  gpsx_wtow_t *d_tow, gpsx_wtow_rx_t *d_tow_rx);
int gpsx_wtow(gpsx_ctx *ctx, const gpsx_wtow_cfg_t *cfg, int n_rx, int n_prn, const uint8_t *prns, const gpsx_wpred_rx_t *d_pred_rx,
              const gpsx_wpred_t *d_pred, gpsx_wsync_state_t *d_sync_state, gpsx_wobs_state_t *d_obs_state, gpsx_wobs_t *d_obs,
              gpsx_wtow_t *tow, gpsx_wtow_rx_t *tow_rx);

/* ---- EXTENSION, not in the reference: almanac, ionosphere and UTC -- subframes 4 and 5 of the words, on the device ------------------
 * gpsx_weph counts subframes 4 and 5 and drops them; the reference's decoder keeps only their HOW time.  gpsx_walm(_dev) is a stage
 * behind gpsx_wnav_words_dev, beside gpsx_weph_dev, on the same d_words: it assembles every slot's subframes across launches, keeps
 * per RECEIVER the newest parity-clean copy of the 32 almanac pages, of subframe 4 page 18 (Klobuchar coefficients, UTC) and of
 * subframe 5 page 25 (almanac reference week, health summary) in a device-resident bank owned by the caller, and returns per launch the
 * decoded records: the ion[8] that gpsx_wfix_cfg_t, gpsx_wkf_cfg_t and gpsx_wpred_cfg_t take, GPS - UTC, and the constellation's
 * coarse orbits.  A slot's PRN plays no part: every satellite sends every page.  It changes no existing struct, kernel or definition
 * (GPSX_VERSION stays 110).  IS-GPS-200 20.3.3.5 is what the fields mean; the reference has no decoder for these pages, so THIS TEXT is
 * the definition.
 *
 * The channel of receiver r's slot j is r * ch_per_rx + j; d_words is [n_blocks / 600 + 2][n_rx * ch_per_rx].
 *
 * Assembly, per slot, on its 64-byte state.  The slots of d_words are read in order.  A record counts only if its flags have
 * GPSX_WNAV_WORD, 1 <= index <= 10, -600 <= end_block < n_blocks (word 1 of a GPSX_WNAV_SYNC pair ends before its launch may) and,
 * with E1 = blocks_seen + end_block + 1, E1 >= 1; every other record is skipped.  `passed`: the record has GPSX_WNAV_OK -- and, for
 * index 2, subframe_id in 1 .. 5 and aux < 100800.  For a record that counts:
 *   1 word 1       cur_mask = passed, cur_next = 2, cur_id = 0, last_word_end_p1 = E1
 *   2 the expected word  (index == cur_next and E1 == last_word_end_p1 + 600)  if passed: cur_mask |= 1 << (index - 1); if passed
 *                  and index is 2: cur_id = subframe_id; if passed and index >= 3: cur[index - 3] = (word >> 6) & 0xFFFFFF.  Then
 *                  last_word_end_p1 = E1 and cur_next = index == 10 ? 0 : index + 1.  At index 10 with cur_mask == 0x3FF and cur_id
 *                  4 or 5 the subframe is COMPLETE: it is offered to the bank with cur[] as it stands
 *   3 anything else  (a gap, a word out of order, a word while waiting for a word 1)  cur_next = 0, cur_mask = 0,
 *                  last_word_end_p1 = E1
 * Then blocks_seen += n_blocks.  (Word 10s lie 6000 blocks apart: a slot completes at most one subframe per launch.)  The call must
 * be made on every launch of a stream, as gpsx_wnav_words must: blocks_seen is the time base.
 *
 * Commit, per receiver.  Subframe bit n (0 = the first bit of word 1) lies in word n / 30, and bits 0 .. 23 of a word are d1 .. d24,
 * d1 first: u(p, l) is the l bits from bit p on, first bit most significant, s(p, l) the same as two's complement.  With data ID =
 * u(60, 2), s = u(62, 6) and toa = u(90, 8), a COMPLETE subframe goes to bank entry
 *     cur_id 5, data ID 1, s 1 .. 24,  toa <= 147     s - 1  (almanac of SV s)
 *     cur_id 4, data ID 1, s 25 .. 32, toa <= 147     s - 1  (almanac of SV s)
 *     cur_id 4, data ID 1, s 56                       32     (page 18)
 *     cur_id 5, data ID 1, s 51                       33     (page 25)
 * and anything else (another data ID, dummy SV 0, another page, an almanac toa beyond 147 * 4096 = 602 112 s) only counts in n_other.
 * A receiver's commits of one launch apply in ascending slot order: page[e] = cur[0 .. 7], have_mask |= 1 << e, n_stored++ -- the
 * highest slot's words stand, every commit counts.  Entry e is SEEN in a launch with a commit to it, and NEW if it is SEEN and was not
 * held before the launch or its eight words after the launch differ from those before it; n_changed += the number of NEW entries.
 * Nothing is ever cleared.  The counters wrap at 2^32.
 *
 * Output, per receiver, from the bank as the launch left it; every byte of d_rx and d_alm is written.  Doubles: the integer converted,
 * then one IEEE multiply by the scale (an exact power of two), then for semicircles one by 3.1415926535898, no contraction.
 * Eight-bit weeks (wna, wnt, wn_lsf) are resolved around build week 2290 as gpsx_weph resolves its ten bits:
 * W = w + (2290 - w + 128) / 256 * 256 in C's integers, 2163 .. 2418.
 *   d_alm[r][s - 1] from entry s - 1, all zero if it is not held:
 *     flags   HELD; NEW as above; HEALTHY iff svh == 0; WEEK iff entry 33 is held and its u(68, 8) equals this page's u(90, 8)
 *     svid u(62, 6) (= s), svh u(136, 8), week = page 25's resolved wna with WEEK, else 0
 *     e u(68,16) 2^-21;  toas u(90,8) * 4096;  i0 = (0.3 + s(98,16) 2^-19) * pi: the (exact) product, the sum, then the product;
 *     OMGd s(120,16) 2^-38 pi;  A = rootA * rootA with rootA = u(150,24) 2^-11;  OMG0 s(180,24) 2^-23 pi;  omg s(210,24) 2^-23 pi;
 *     M0 s(240,24) 2^-23 pi;  f0 = s11(u(270,8) << 3 | u(289,3)) 2^-20;  f1 s(278,11) 2^-38
 *   d_rx[r]:
 *     flags   GPSX_WALM_IONUTC iff entry 32 is held, GPSX_WALM_PAGE25 iff entry 33 is held;  n_stored: this launch's commits
 *     have_mask, new_mask, seen_mask: bit e;  healthy_mask / week_mask: bit s - 1 = the record's HEALTHY / WEEK
 *     from page 25 (zero without it): toa_s u(68,8) * 4096, wna u(76,8) resolved, p25_unhealthy_mask bit n - 1 iff the six-bit health
 *       word of SV n (1 .. 24), u(90 + 30 ((n - 1) / 4) + 6 ((n - 1) % 4), 6), is != 0
 *     from page 18 (zero without it): ion[0 .. 3] = alpha s(68,8) 2^-30, s(76,8) 2^-27, s(90,8) 2^-24, s(98,8) 2^-24; ion[4 .. 7] =
 *       beta s(106,8) 2^11, s(120,8) 2^14, s(128,8) 2^16, s(136,8) 2^16 (the layout of gpsx_wfix_cfg_t.ion); A1 s(150,24) 2^-50;
 *       A0 = (int32)(u(180,24) << 8 | u(210,8)) 2^-30; tot_s u(218,8) * 4096; wnt u(226,8) resolved; dt_ls s(240,8); wn_lsf u(248,8)
 *       resolved; dn u(256,8); dt_lsf s(270,8).  (A page 18 with all-zero alpha and beta gives an all-zero ion[]: the solvers then
 *       use their default set.)
 * d_alm NULL: the almanac records are not wanted.
 *
 * Errors, each GPSX_EINVAL with a gpsx_last_error text and nothing written: cfg, d_words, d_slot_state, d_bank or d_rx NULL;
 * ch_per_rx outside 1 .. 64; a reserved word != 0; n_blocks outside 1 .. 4096; n_rx outside 1 .. 1 048 576; d_words, d_slot_state,
 * d_bank or (in _dev) d_rx, d_alm not 16-byte aligned; two of the five arrays overlapping; size products that overflow.
 * A slot is BAD if blocks_seen or last_word_end_p1 lies outside 0 .. 2^62, cur_next is not 0 or 2 .. 10, cur_mask > 0x3FF, cur_id > 5,
 * a cur word >= 2^24 or reserved != 0: its state stays as it was and it commits nothing; the receiver's other slots are served.  A
 * bank is BAD if a page word is >= 2^24, have_mask has a bit from 34 on or a reserved word is != 0: the bank AND the receiver's slot
 * states stay as they were (nothing a slot completed is lost: the launch did not happen for this receiver) and its records are all
 * zero.  Either way GPSX_EINVAL comes from gpsx_walm after its wait / from the next gpsx_synchronize() after _dev; the other
 * receivers are served.
 * _dev only enqueues.  Vector ALU (k_walm: a wave per receiver, four receivers per workgroup, no LDS; lane j is slot j for the
 * assembly -- the word records' 16-byte loads and the state all in flight before the first is looked at --, lane e is bank entry e
 * for the commits, which a ballot finds and lane broadcasts apply in ascending slot order; an entry is written back only if it
 * changed, none is read back; lanes 0 .. 31 decode and store their almanac record).  On one stream: ..., gpsx_wnav_words_dev, then
 * gpsx_wobs_dev, gpsx_weph_dev and gpsx_walm_dev in any order on the same d_words and n_blocks; the host copies d_rx's ion[] into
 * the solvers' cfg (eight doubles). */
#define GPSX_WALM_IONUTC  1u   /* gpsx_walm_rx_t.flags: page 18 is held */
#define GPSX_WALM_PAGE25  2u   /* gpsx_walm_rx_t.flags: page 25 is held */
#define GPSX_WALM_HELD    1u   /* gpsx_walm_sv_t.flags: the SV's almanac page is held */
#define GPSX_WALM_WEEK    2u   /* ... and its toa is page 25's: `week` is its reference week */
#define GPSX_WALM_HEALTHY 4u   /* ... and its eight-bit health is 0 */
#define GPSX_WALM_NEW     8u   /* ... and a commit of this launch gave the entry contents it did not have before */
#define GPSX_WALM_ENTRIES 34   /* almanac pages of SV 1 .. 32, page 18, page 25 */

typedef struct {                 /* 16 bytes */
  int32_t ch_per_rx;             /* 1 .. 64 */
  int32_t reserved[3];           /* 0 */
} gpsx_walm_cfg_t;

typedef struct {                 /* 64 bytes per slot, device resident; all zero = a fresh slot */
  int64_t  blocks_seen;          /*  0  blocks of all earlier launches */
  int64_t  last_word_end_p1;     /*  8  absolute last block of the newest word that counted, + 1; 0: none */
  uint32_t cur[8];               /* 16  d1 .. d24 (d1 in bit 23) of words 3 .. 10 of the subframe being assembled */
  uint32_t cur_mask;             /* 48  bit w (0 .. 9): word w + 1 of it counted and passed */
  uint32_t cur_next;             /* 52  index of the word expected next, 2 .. 10; 0: waiting for a word 1 */
  uint32_t cur_id;               /* 56  from its HOW if that passed: 1 .. 5; else 0 */
  uint32_t reserved;             /* 60  0 */
} gpsx_walm_slot_t;

typedef struct {                 /* 1120 bytes per receiver, device resident; all zero = empty */
  uint32_t page[GPSX_WALM_ENTRIES][8];   /*    0  words 3 .. 10 of the newest copy of every entry */
  uint64_t have_mask;            /* 1088  bit e: page[e] holds a page */
  uint32_t n_stored, n_changed, n_other;   /* 1096  commits; entries that became NEW; complete subframes 4 / 5 that went nowhere */
  uint32_t reserved[3];          /* 1108  0 */
} gpsx_walm_bank_t;

typedef struct {                 /* 160 bytes, one per receiver and launch */
  uint32_t flags;                /*   0  GPSX_WALM_IONUTC | GPSX_WALM_PAGE25 */
  uint32_t n_stored;             /*   4  commits of this launch */
  uint64_t have_mask, new_mask, seen_mask;   /*   8  bit e = bank entry e */
  uint32_t healthy_mask, week_mask, p25_unhealthy_mask;   /*  32  bit s - 1 = SV s */
  int32_t  toa_s, wna;           /*  44  page 25 */
  int32_t  tot_s, wnt, dt_ls, wn_lsf, dn, dt_lsf;   /*  52  page 18 */
  uint32_t reserved;             /*  76  0 */
  double   A0, A1;               /*  80  page 18: UTC polynomial, s and s/s */
  double   ion[8];               /*  96  page 18: Klobuchar a0..a3, b0..b3, as gpsx_wfix_cfg_t.ion */
} gpsx_walm_rx_t;

typedef struct {                 /* 96 bytes, d_alm[r][s - 1] */
  uint32_t flags;                /*  0  GPSX_WALM_HELD | WEEK | HEALTHY | NEW */
  int32_t  svid, svh, week;      /*  4 */
  double   toas, e, A, i0, OMG0, omg, M0, OMGd, f0, f1;   /* 16  s, -, m, rad, rad, rad, rad, rad/s, s, s/s */
} gpsx_walm_sv_t;

/* d_words, d_slot_state [n_rx * ch_per_rx] and d_bank [n_rx]: device memory in both variants.  d_rx [n_rx] and d_alm (NULL: not
 * wanted) [n_rx][32]: device memory; gpsx_walm takes rx and alm in host memory (staged through the arena; it waits for its kernel). */
int gpsx_walm_dev(gpsx_ctx *ctx, const gpsx_walm_cfg_t *cfg, const gpsx_wnav_word_t *d_words, int n_blocks, int n_rx,
                  gpsx_walm_slot_t *d_slot_state, gpsx_walm_bank_t *d_bank, gpsx_walm_rx_t *d_rx, gpsx_walm_sv_t *d_alm);
int gpsx_walm(gpsx_ctx *ctx, const gpsx_walm_cfg_t *cfg, const gpsx_wnav_word_t *d_words, int n_blocks, int n_rx,
              gpsx_walm_slot_t *d_slot_state, gpsx_walm_bank_t *d_bank, gpsx_walm_rx_t *rx, gpsx_walm_sv_t *alm);

/* Host only, no GPU.  An almanac record with HELD and WEEK as a GPSX_WEPH_VALID ephemeris record, so that gpsx_weph_to_eph
 * (include/gpsx_compat.h) and the solvers' satellite position evaluate the almanac orbit unchanged: *out is zeroed, then flags =
 * GPSX_WEPH_VALID, A, e, i0, OMG0, omg, M0, OMGd, f0, f1, svh and week are the record's, toes = toas, and toe and toc are the
 * decoder's gps_time(week, toas) (time = 315964800 + 604800 week + (int)toas, sec = toas - (int)toas); every other field (the
 * harmonic terms, deln, idot, f2, tgd, iode, iodc, ttr, n_sets, have) stays zero.  GPSX_EINVAL for NULL and for a record without HELD
 * and WEEK (*out is then untouched). */
int gpsx_walm_to_eph(const gpsx_walm_sv_t *in, gpsx_weph_t *out);
/* Host only, no GPU.  GPS - UTC at GPS week `week` (full), second tow_s, from a receiver record with GPSX_WALM_IONUTC and dn in 1 .. 7
 * (IS-GPS-200 20.3.3.5.2.4; the leap second takes effect at the end of day dn of week wn_lsf), in this order of double operations:
 *   now = (double)week * 604800.0 + tow_s;   then = (double)wn_lsf * 604800.0 + (double)dn * 86400.0
 *   ls  = now >= then ? dt_lsf : dt_ls
 *   dt  = ((double)ls + A0) + A1 * ((tow_s - (double)tot_s) + 604800.0 * ((double)week - (double)wnt))
 * GPSX_EINVAL for NULL, a record without IONUTC, dn outside 1 .. 7 or a tow_s that is not finite (*dt_s is then untouched). */
int gpsx_walm_gps_minus_utc(const gpsx_walm_rx_t *rx, int week, double tow_s, double *dt_s);

/* ---- EXTENSION, not in the reference: the weighted grid in a WINDOW around each predicted satellite ---------------------------------
 * gpsx_wpred hands a satellite straight to a slot only when its prediction is CERTAIN (3 samples, 12.5 Hz); everything else used to go
 * through a full grid of n_prn x n_dopp x 16 368 hypotheses per receiver, although the chain often knows the answer to a few dozen
 * samples and a few hertz: a filter just after INIT, an outage of more than a few seconds, a bank entry that came from an almanac
 * (gpsx_walm_to_eph: the orbit is good to about a kilometre, some 70 samples).  gpsx_acq_window_weighted(_dev) takes gpsx_wpred's records
 * where they lie and searches, per (receiver, PRN index), the 2 W + 1 code phases and the at most 2 D + 1 Doppler bins around the
 * prediction only.  It answers in the grids' record format, so that gpsx_wacq decides and hands over unchanged.  No existing struct,
 * kernel or definition changes (GPSX_VERSION stays 110).
 *
 * g is the descriptor a gpsx_acq_grid_weighted_hyb call would be given: n_search = n_rx (search r is receiver r), search_stride_blocks
 * the multi loop's rx_stride_blocks, the Doppler lattice dopp_min_hz + d x dopp_step_hz for d in [0, n_dopp), weights either mode.
 * g->prns is a HOST pointer to THE SAME LIST gpsx_wpred was called with, index for index: d_pred[r][p] is read as the prediction for
 * PRN g->prns[p].  The device cannot check this; it is the caller's duty.
 *
 * Definition, per (receiver r, PRN index p), rec = d_pred[r][p]; W = half_width, D = half_bins:
 *   0 selection  SKIPPED unless (rec.flags & need_flags) == need_flags and (rec.flags & skip_flags) == 0.  BAD if selected but
 *                code_phase is not finite or lies outside [0, 16368], or f_hz is not finite.  In both cases every record of the row
 *                d_peaks[r][p][*] is zero and the report has zeros beside its flag.
 *   1 centre     c = (int)rint(code_phase) in double, ties to even; c == 16368 becomes 0.  The window is the 2 W + 1 phases
 *                (c + j) mod 16368, j = -W .. W.
 *   2 bins       x = (f_hz - (double)dopp_min_hz) / (double)dopp_step_hz: one subtraction, one division, uncontracted.  |x| > 2^30:
 *                OFF_LATTICE.  Otherwise dc = (int)rint(x), d0 = max(dc - D, 0), d1 = min(dc + D, n_dopp - 1); d0 > d1: OFF_LATTICE
 *                (zero row, the report has zeros beside that flag).  Otherwise SEARCHED, with CLIPPED if dc - D < 0 or dc + D >
 *                n_dopp - 1; the report has first_bin = d0, n_bins = d1 - d0 + 1, centre = c.
 *   3 energy     for each bin d in d0 .. d1, E_d(tau) is exactly gpsx_acq_grid_weighted_hyb's E(tau) for search r, PRN prns[p], bin
 *                d, n_coh, n_seg: segment j's blocks are r x stride + j x n_coh + b, the NCO runs from 0 at each segment's first
 *                block and is chained through its blocks, the sixteen unmixed samples weigh 0, the roots are exact.  It is
 *                evaluated at the window's phases only.
 *   4 record     d_peaks[r][p][d]: max_val = max E_d over the window; phase = the numerically smallest tau of the window that
 *                reaches it (the grids' rule and the grids' key: a window across the seam answers with its low taus), 0 when max_val
 *                is 0.  sum is the noise floor in the grids' units: F = the window's phases whose circular distance from `phase`
 *                exceeds guard (|F| >= 2 because guard < W), S_far = the sum of E_d over F, sum = the low 32 bits of
 *                floor(S_far x 16368 / |F|) in uint64 (S_far < 2^40: the product stays below 2^54); avr = sum / 16368.  With this
 *                sum gpsx_wacq's step 2 reads unchanged -- peak over the mean of the window's far phases >= det_num / det_den; the
 *                floor makes sum / 16368 SMALLER than the true mean by less than one part in 16 368 x mean, so it errs, if at all,
 *                towards a detection.  The grids' mod 2^32 condition carries over word for word: the mean must stay below 2^18.
 *   5 coverage   every other record of the row is all zero.  Every byte of d_peaks[n_rx][n_prn][n_dopp] is written by the call, and
 *                so is every byte of d_rep[n_rx][n_prn] unless it is NULL.
 * The call needs (n_search - 1) x search_stride_blocks + n_coh x n_seg <= n_blocks.
 *
 * The identity that ties it to the grids: for every searched (r, p, d), if the phase of gpsx_acq_grid_weighted_hyb's record for the
 * same (search, PRN, bin) lies in the window, then max_val and phase are that record's.
 *
 * Errors, each GPSX_EINVAL with a gpsx_last_error text and nothing written, checked in this order: g, cfg, g->prns, pred, blocks or
 * peaks NULL; n_coh outside 1 .. 20; n_seg outside 1 .. 128; half_width outside 1 .. 2047; half_bins outside 0 .. 32; guard outside
 * 0 .. half_width - 1; a bit outside the seven GPSX_WPRED_* in need_flags or skip_flags; need_flags without GPSX_WPRED_PREDICTED;
 * reserved != 0; unknown weights; dopp_step_hz < 1; n_search outside 1 .. 1 048 576; n_prn outside 1 .. 64; n_dopp outside
 * 1 .. 1 048 576; search_stride_blocks < 0; a PRN outside 1 .. 210 or listed twice; the lattice's last bin outside int32; too few
 * blocks; d_pred or d_rep not 16-byte aligned (_dev); size products that overflow.
 *
 * _dev only enqueues; gpsx_last_kernel says k_acq_win.  Vector ALU, exact in integers (k_acq_win: a workgroup of 256 threads per
 * (receiver, PRN index, bin of the 2 D + 1); the grids' pre-sum into LDS per segment, v_dot2_i32_i16 against the PRN's chip pairs at
 * the window's phases, E in LDS; no HBM scratch, no global atomics).
 *
 * For the caller.  On one stream: gpsx_wkf_dev; gpsx_wpred_dev (with handover = 1 the CERTAIN satellites go straight to slots and
 * carry ASSIGNED, which the intended skip_flags leave out); this call on the blocks that BEGIN AT THE PREDICTION'S EPOCH BLOCK;
 * gpsx_wacq_dev with the same g and lead_blocks = n_coh x n_seg; the next loop launch.  Matching the prediction's epoch (the filter's
 * rcv_ms + lead_blocks) to the first block is the caller's duty, as in gpsx_wtow.  The intended masks are need_flags = PREDICTED |
 * VISIBLE, skip_flags = TRACKED | ASSIGNED.  An almanac warm start fills bank entries with gpsx_walm_to_eph records on the host.
 * The same bank feeds gpsx_wsnap (below).
 * Step the lattice by about 500 / n_coh Hz.  The code slides about 3 samples per 100 ms at 5 kHz of Doppler: choose W over the
 * prediction's error plus that slide. */
#define GPSX_ACQ_WINDOW_SEARCHED     1u
#define GPSX_ACQ_WINDOW_SKIPPED      2u
#define GPSX_ACQ_WINDOW_BAD          4u
#define GPSX_ACQ_WINDOW_OFF_LATTICE  8u
#define GPSX_ACQ_WINDOW_CLIPPED     16u

typedef struct {                 /* 32 bytes */
  int32_t  n_coh;                /*  0  1 .. 20 blocks per coherent segment */
  int32_t  n_seg;                /*  4  1 .. 128 segments, their magnitudes summed */
  int32_t  half_width;           /*  8  W: 1 .. 2047 samples */
  int32_t  half_bins;            /* 12  D: 0 .. 32 bins */
  int32_t  guard;                /* 16  0 .. W - 1: phases within guard of the peak do not count as noise */
  uint32_t need_flags;           /* 20  GPSX_WPRED_* bits a record must have; must contain GPSX_WPRED_PREDICTED */
  uint32_t skip_flags;           /* 24  GPSX_WPRED_* bits a record must not have */
  int32_t  reserved;             /* 28  0 */
} gpsx_acq_window_t;

typedef struct {                 /* 16 bytes, one per (receiver, PRN index) */
  uint32_t flags;                /*  0  GPSX_ACQ_WINDOW_*: SEARCHED (with or without CLIPPED), or SKIPPED, BAD, OFF_LATTICE alone */
  int32_t  first_bin;            /*  4  d0 */
  int32_t  n_bins;               /*  8  d1 - d0 + 1 */
  int32_t  centre;               /* 12  c */
} gpsx_acq_window_rep_t;

/* d_pred [n_rx][n_prn], d_if_blocks_2bit (n_blocks 4092-byte blocks), d_peaks [n_rx][n_prn][n_dopp] and d_rep (NULL: not wanted)
 * [n_rx][n_prn]: device memory; gpsx_acq_window_weighted takes all four in host memory (staged through the arena; it waits for its
 * kernel). */
int gpsx_acq_window_weighted_dev(gpsx_ctx *ctx, const gpsx_acq_weighted_t *g, const gpsx_acq_window_t *cfg, const gpsx_wpred_t *d_pred,
                                 const void *d_if_blocks_2bit, int n_blocks, gpsx_peak_t *d_peaks, gpsx_acq_window_rep_t *d_rep);
int gpsx_acq_window_weighted(gpsx_ctx *ctx, const gpsx_acq_weighted_t *g, const gpsx_acq_window_t *cfg, const gpsx_wpred_t *pred,
                             const uint8_t *if_blocks_2bit, int n_blocks, gpsx_peak_t *peaks, gpsx_acq_window_rep_t *rep);

/* ---- EXTENSION, not in the reference: snapshot fixes -- a weighted grid's records, a bank and a coarse prior to a position -----------
 * A grid record becomes a position today only through a slot, bit sync, a HOW and 18 .. 30 s of subframes.  A capture of a few
 * milliseconds carries no navigation data; with the orbits from elsewhere (a gpsx_wbank bank, gpsx_walm_to_eph, another receiver of
 * the launch) and a prior that knows where and when to within a cell and a minute it can still be positioned: coarse-time navigation,
 * five unknowns (position, a common bias, the error of the time tag).  gpsx_wsnap(_dev) is a STATELESS stage behind any weighted grid
 * call (gpsx_acq_grid_weighted{,_ms,_coh,_hyb}, gpsx_acq_window_weighted): per receiver it reads the grid's records where they lie,
 * an ephemeris bank and a prior, and writes a position, the bias and a corrected time of week.  Nothing crosses to the host in
 * between.  No existing struct, kernel or definition changes (GPSX_VERSION stays 110).  The same bank that feeds gpsx_wpred and the
 * windowed grid feeds this stage.
 *
 * g is the description the grid call was given (gpsx_wacq's reading of it: search s IS receiver s, prns a HOST pointer, PRN index p
 * its position in the list).  THIS TEXT is the definition.  Decisions are integers where they can be; everything else is IEEE
 * double, uncontracted, with gpsx_wkf's constants (c, ms = 299792.458 m, we, Re) and the sum orders given here.
 *   0 prior        d_prior[r] = {flags, week, rr[3], tow_s, reserved}: where the receiver roughly is (ECEF, m) and the GPS week and
 *                  time of week of the search's first sample.  Without GPSX_WSNAP_PRIOR_HAVE, with a flag bit beyond it, with a
 *                  reserved word != 0, with an rr or tow_s that is not finite, a tow_s outside 0 <= tow_s < 604800 or a week outside
 *                  0 .. 32767: NO_PRIOR -- d_snap[r] and every d_sv[r][p] are zero but for that flag, and the call still returns 0.
 *   1 detection    gpsx_wacq's steps 1 and 2, word for word: per PRN index p the best record is the LOWEST bin of the row's
 *                  greatest max_val, M that max_val, S that record's sum, tau_p that record's phase, f_p = dopp_min_hz + bin x
 *                  dopp_step_hz; DETECTED iff M >= max(min_peak, 1) and (uint64)M x 16368 x det_den >= (uint64)det_num x S.
 *   2 satellites   the bank record of (r, p) is d_bank[r x bank_stride + p], bank_stride either n_prn (gpsx_wbank's layout) or 0 (one
 *                  row of n_prn records for every receiver).  A record with GPSX_WEPH_VALID has HAVE_EPH.  EVAL(x, t), for a record
 *                  with HAVE_EPH and svh == 0, is gpsx_wpred's step 2 at the point x with clock term 0 and receive time t in double
 *                  seconds, that step's T being the double 1000 t: pr_0 = 72 ms; pass k = 0, 1, 2: t_sv = (T - pr_k / ms) / 1000; the
 *                  satellite at its clock's reading t_sv (ps, vs,
 *                  d', dts, svar; the pass fails if |tk| > 7201, A <= 0 or Kepler's iteration needs 30 steps); l = ps - x, range =
 *                  |l|; the pass fails if range == 0, |ps| < Re or rho = range + we (ps_x x_1 - ps_y x_0) / c <= 0; e = l / range;
 *                  az, el at ecef2pos(x); dion = Klobuchar(cfg.ion or the default set where cfg's are all 0, tow = T / 1000), dtrp =
 *                  Saastamoinen(0.7), var = gpsx_wfix's variance of the row (measurement, svar, ionosphere, troposphere);
 *                  pr_(k+1) = (rho + dion + dtrp - c dts) + c tgd.  The last pass's values count: pr = pr_3, e, el, az, var and
 *                  rd = e . vs + k (vs_x x_1 - vs_y x_0) - c d', k = we / c, the pseudorange's rate (gpsx_wpred step 3's second
 *                  bracket).  EVAL is GOOD iff no pass failed and pr, el, az, rd and var are finite and |pr| < 1e12.
 *                  t0 = tow_s + epoch_offset_s (one addition; epoch_offset_s: half the search's span, because a non-coherent
 *                  sum's phase belongs to the middle of its blocks).  A CANDIDATE is DETECTED, has HAVE_EPH and svh == 0, EVAL(prior
 *                  rr, t0) is GOOD and its el >= el_min_rad.  Fewer than min_sats candidates: TOO_FEW (n_iter = 0).
 *   3 milliseconds the REFERENCE is the candidate of greatest el; at equal el the lower index.  With s_p = (double)tau_p / 16368 and
 *                  pr_p of step 2:  N_ref = rint(pr_ref / ms - s_ref);  b0 = (N_ref + s_ref) x ms - pr_ref;  for every candidate
 *                  (the reference too)  N_p = rint((pr_p + b0) / ms - s_p),  z_p = (N_p + s_p) x ms.  Every operation single, in the
 *                  order written, ties to even.  The N_p are fixed from here on (they resolve while the prior's combined error in
 *                  a range DIFFERENCE stays under half a millisecond, 150 km: position error x up to 2 plus 800 m/s x the time error).
 *   4 iteration    unknowns (x, y, z, b in metres, dt in seconds) from (prior rr, 0, 0).  Per pass every candidate runs
 *                  EVAL((x, y, z), t0 + dt) -- T = 1000 ((tow_s + epoch_offset_s) + dt).  It has a ROW iff that is GOOD and its el >= 0.  The row
 *                  is h = (-e_x, -e_y, -e_z, 1, rd), v = z_p - (pr + b), sig = sqrt(var), a = h / sig (a_3 = 1 / sig), y = v / sig.
 *                  The 15 + 5 sums N_ij = sum a_i a_j (i >= j), g_i = sum a_i y run over the 64 lanes of a wave (a lane without a
 *                  row adds zeros) as a butterfly: six rounds, in round m = 1, 2, 4, 8, 16, 32 lane l adds lane l ^ m's value.
 *                  Fewer than min_sats rows: TOO_FEW.  A sum not finite: NONFINITE.  Cholesky N = L L^T row by row as gpsx_wfix's:
 *                  p_j = N_jj - l_j0^2 - .. - l_j(j-1)^2, l_jj = sqrt(p_j), l_ij = (N_ij - l_i0 l_j0 - .. - l_i(j-1) l_j(j-1)) / l_jj;
 *                  p_0 <= 0 or p_k <= 1e-10 N_kk: SINGULAR.  M = L^-1: m_jj = 1 / l_jj, m_ij = -(l_ij m_jj + .. + l_i(i-1) m_(i-1)j)
 *                  / l_ii; w_i = m_i0 g_0 + .. + m_ii g_i; dx_j = m_jj w_j + .. + m_4j w_4 (sums left to right).  A dx not finite:
 *                  NONFINITE.  The unknowns += dx; converged when dx_0^2 + dx_1^2 + dx_2^2 + dx_3^2 + (1000 dx_4)^2 < 1e-8 (left
 *                  to right).  Ten passes at most, then NO_CONV.  n_iter counts the passes, n_used and used_mask are the last
 *                  pass's rows, qr the first three unknowns' block of M^T M of the converging pass in gpsx_wfix's order.
 *   5 check        one more EVAL at the final unknowns; over the rows of it that are in used_mask: resid_m_p = v_p,
 *                  resid_rms_m = sqrt(sum v^2 / n_used) (the butterfly's sum, unweighted); geo = ecef2pos of the final point.  A
 *                  wrong millisecond is 300 km: resid_rms_m > max_resid_m gives RESID, not FIX; the numbers stay in the record.
 *                  Anything of the record not finite (rr, b_m, dt_s, tow_s, geo, the float qr, the rms), or a tow_s that step 6's
 *                  single fold leaves outside 0 <= tow_s < 604800 (|dt_s| beyond a week: a solve that ran away): NONFINITE instead,
 *                  with zeros.
 *   6 records      d_snap[r]: flags is exactly one of FIX / RESID / TOO_FEW / SINGULAR / NO_CONV / NONFINITE / NO_PRIOR; the
 *                  counts, ref and used_mask as far as the receiver came (ref = -1 before step 3); rr .. resid_rms_m only with
 *                  FIX or RESID.  tow_s = the prior's tow_s + dt_s, week the prior's; tow_s >= 604800: tow_s -= 604800, week += 1;
 *                  tow_s < 0: tow_s += 604800, week -= 1 (with FIX or RESID; otherwise the prior's own).  d_sv[r][p] (unless NULL):
 *                  flags DETECTED, HAVE_EPH, CANDIDATE, USED (bit p of used_mask), REFERENCE; phase = tau_p and dopp_hz = f_p
 *                  always; n_ms = N_p of a candidate (once step 3 ran), el and az of step 2 for a candidate; resid_m with FIX or
 *                  RESID for a USED row of step 5.  Every byte of both is written; nothing non-finite is ever written.
 * Errors, each GPSX_EINVAL with a gpsx_last_error text and nothing written: cfg, g, g->prns, the peaks, d_bank, d_prior or d_snap
 * NULL; an ion[] not finite; el_min_rad not finite or outside +-pi/2; epoch_offset_s not finite or outside 0 .. 4.096; max_resid_m
 * not finite or <= 0; det_num, det_den outside 1 .. 1024 or det_num < det_den; min_sats outside 5 .. 64; a reserved word != 0; n_search
 * outside 1 .. 1 048 576; n_prn outside 1 .. 64; n_dopp outside 1 .. 1 048 576; a PRN outside 1 .. 210 or listed twice; a Doppler bin
 * outside int32; bank_stride neither 0 nor n_prn; d_bank not 16-byte aligned, (_dev) d_peaks not 4-byte, d_prior not 8-byte, d_snap or
 * d_sv not 16-byte aligned; (_dev) d_snap or d_sv overlapping each other or one of the three inputs; size products that overflow.
 * _dev only enqueues on the context's stream: the grid call, then gpsx_wsnap_dev on its d_peaks.  Vector ALU, FP64 (k_wsnap: a wave
 * per receiver, four receivers per workgroup, no LDS; step 1 is k_wacq's strided rows and 64-bit keys; from step 2 on lane p is PRN
 * index p, one satellite evaluation per lane and pass; the reference by ballots and shuffles; the twenty sums under wave-uniform
 * control flow, the 5 x 5 factorisation in every lane's registers). */
#define GPSX_WSNAP_FIX          1u
#define GPSX_WSNAP_RESID        2u   /* converged, but resid_rms_m > max_resid_m: a wrong millisecond, a wrong prior */
#define GPSX_WSNAP_TOO_FEW      4u
#define GPSX_WSNAP_SINGULAR     8u
#define GPSX_WSNAP_NO_CONV     16u
#define GPSX_WSNAP_NONFINITE   32u
#define GPSX_WSNAP_NO_PRIOR    64u
#define GPSX_WSNAP_PRIOR_HAVE   1u   /* gpsx_wsnap_prior_t.flags */
#define GPSX_WSNAP_SV_DETECTED  1u
#define GPSX_WSNAP_SV_HAVE_EPH  2u
#define GPSX_WSNAP_SV_CANDIDATE 4u
#define GPSX_WSNAP_SV_USED      8u
#define GPSX_WSNAP_SV_REFERENCE 16u

typedef struct {                 /* 128 bytes */
  double   ion[8];               /*   0  as gpsx_wfix_cfg_t's; all 0: the default set */
  double   el_min_rad;           /*  64  finite, -pi/2 .. pi/2 */
  double   epoch_offset_s;       /*  72  0 .. 4.096: from the search's first sample to the instant its phases belong to */
  double   max_resid_m;          /*  80  > 0 */
  int32_t  det_num, det_den;     /*  88  as gpsx_wacq_cfg_t's: 1 .. 1024, det_num >= det_den */
  uint32_t min_peak;             /*  96  as gpsx_wacq_cfg_t's */
  int32_t  min_sats;             /* 100  5 .. 64 */
  int32_t  reserved[6];          /* 104  0 */
} gpsx_wsnap_cfg_t;

typedef struct {                 /* 48 bytes, one per receiver */
  uint32_t flags;  int32_t week; /*   0  GPSX_WSNAP_PRIOR_HAVE; 0 .. 32767 */
  double   rr[3];                /*   8  ECEF, m */
  double   tow_s;                /*  32  of the search's first sample, 0 <= tow_s < 604800 */
  uint32_t reserved[2];          /*  40  0 */
} gpsx_wsnap_prior_t;

typedef struct {                 /* 128 bytes, one per receiver */
  uint32_t flags;  int32_t week; /*   0  GPSX_WSNAP_*; the week of tow_s */
  uint8_t  n_detected, n_candidates, n_used, n_iter;   /*   8 */
  int32_t  ref;                  /*  12  the reference's PRN index, -1: none */
  uint64_t used_mask;            /*  16  bit p = PRN index p */
  double   rr[3];                /*  24  ECEF, m */
  double   b_m;                  /*  48  the common bias */
  double   dt_s;                 /*  56  what the prior's tow_s was off by */
  double   tow_s;                /*  64  the prior's + dt_s, inside the week */
  double   geo[3];               /*  72  lat, lon (rad), height (m) */
  double   resid_rms_m;          /*  96 */
  float    qr[6];                /* 104  as gpsx_wfix_t's */
} gpsx_wsnap_t;

typedef struct {                 /* 48 bytes, one per (receiver, PRN index) */
  uint32_t flags;  int32_t n_ms; /*   0  GPSX_WSNAP_SV_*; N_p */
  uint32_t phase;  int32_t dopp_hz;   /*   8  tau_p, f_p */
  double   el, az, resid_m;      /*  16 */
  uint32_t reserved[2];          /*  40  0 */
} gpsx_wsnap_sv_t;

/* d_peaks [n_search][n_prn][n_dopp], d_bank [n_search][n_prn] or (bank_stride 0) [n_prn], d_prior [n_search], d_snap [n_search],
 * d_sv (NULL: not wanted) [n_search][n_prn]: device memory.  gpsx_wsnap takes peaks, prior, snap and sv in host memory (staged
 * through the arena; it waits for its kernel); the bank is device memory in both variants, as gpsx_wpred's. */
int gpsx_wsnap_dev(gpsx_ctx *ctx, const gpsx_wsnap_cfg_t *cfg, const gpsx_acq_weighted_t *g, const gpsx_peak_t *d_peaks,
                   const gpsx_weph_t *d_bank, int bank_stride, const gpsx_wsnap_prior_t *d_prior, gpsx_wsnap_t *d_snap,
                   gpsx_wsnap_sv_t *d_sv);
int gpsx_wsnap(gpsx_ctx *ctx, const gpsx_wsnap_cfg_t *cfg, const gpsx_acq_weighted_t *g, const gpsx_peak_t *peaks,
               const gpsx_weph_t *d_bank, int bank_stride, const gpsx_wsnap_prior_t *prior, gpsx_wsnap_t *snap, gpsx_wsnap_sv_t *sv);
/* Host only, no GPU.  A snapshot with FIX as the gpsx_wfix_t fields gpsx_wkf's INIT reads (flags = GPSX_WFIX_FIX, rr, dtr_s = b_m / c,
 * rx_tow_s = tow_s + dtr_s, week) and what else the two records share (n_used, n_iter, ref_slot = ref, used_mask, geo, qr,
 * resid_rms_m); so a snapshot can start the filter 30 s before the first subframe.  GPSX_EINVAL: a NULL, a record without FIX. */
int gpsx_wsnap_to_fix(const gpsx_wsnap_t *in, gpsx_wfix_t *out);

/* ---- the tracking LOOPS on the device: correlators + DLL / PLL / FLL + false-lock check + SNR + 20 ms bit synchroniser,
 *      K milliseconds per launch, channel state resident in HBM  (gps_tracking_data_process, PM/GPS/tracking.c:92-170,
 *      with gps_tracking_dll / _pll / _fll / _pll_check :175-393 and gps_nav_data_analyse_new_code, PM/GPS/nav_data.c:46-253)
 *
 * The bit-exact mode of this library runs those float loops on the host behind every correlator launch
 * (gps_tracking_process / gps_tracking_process_batch, include/gpsx_compat.h).  This is the other mode: a receiver that tracks
 * tens of thousands of channels keeps each channel's loop state in a gpsx_loop_state_t in device memory and hands the
 * engine K consecutive 1 ms blocks; one kernel runs, per channel and millisecond, the E/P/L correlators (bit-exact, as
 * above) and then the reference's loop arithmetic in its own order of float operations.  Nothing crosses the link per
 * millisecond but the IF block in and ONE byte per channel out:
 *     bit 0  prompt in-phase accumulator > 0          bit 1  a navigation bit was completed this millisecond ...
 *     bit 2  ... and this is its value                bit 3  20 ms bit period synchronised (after this millisecond)
 *     bit 4  the false-lock detector moved the carrier (tracking.c:309-326)
 *     bit 5  the bit edge inside the 20 ms grid was located (nav_data.c:145-218): accurate_swap_time =
 *            (tick - 3 + (bit 6 ? 2 : 1)) % 20 -- what the subframe time stamp is made of
 *     bit 7  the channel was served this millisecond (always set under GPSX_SCHED_EVERY_MS; under GPSX_SCHED_MUX17 the
 *            bytes of a channel's unserved milliseconds are 0)
 * -- what the word layer (gps_nav_data_words_detection, one call per completed bit; gps_tracking_words_batch in
 * include/gpsx_compat.h does it for a whole launch) needs.
 * Serving schedule (gpsx_loop_set_schedule), both the reference's own:
 *   GPSX_SCHED_EVERY_MS (default)  every channel every millisecond, index = tick & 3 (project_single_sat/main.c:96-109, as
 *       gps_tracking_process_batch).  The 4 ms groups then sit still on the 20 ms bit grid, and the reference's bit-edge
 *       locator -- it looks at groups with the sign change between index 1 and 2 only, nav_data.c:131-137 -- resolves the
 *       edge for the channels whose bit edges happen to fall there: one in four.
 *   GPSX_SCHED_MUX17  project_main's receiver: four channels share one correlator in a 17 ms cycle (PM/main.c:139-152).
 *       Channel c is slot (c & 3) of receiver (c >> 2); it is served on the ticks t with (t % 17) / 4 == slot, with
 *       index = (t % 17) % 4; t % 17 == 16 is the idle millisecond (the reference's navigation slot).  The milliseconds a
 *       channel was not served are made up in its carrier NCO when it is served again (gps_rewind_if_phase with the elapsed
 *       ticks - 1, PM/GPS/tracking.c:102-113, from prev_track_timestamp); code phase and loop filters stand still, as in the
 *       reference.  Every 17 ms the group start moves by 17 mod 20 over the bit grid, so every channel gets its bit edge
 *       located, hence accurate_swap_time, hence subframe time stamps and pseudoranges -- the complete receiver on the
 *       device loop (tests/test_gpu_track_mux.py: the reference's multiplexed traces, tests/test_gpu_pvt_chain.py: IF
 *       samples to position).  Hand channels over (gpsx_loop_state_from_channel) on a tick with t % 17 == 0.
 * Arithmetic against the host mode (= the reference's C on the host CPU): the float arctangents are the C library's own
 * algorithm restated operation by operation (csrc/gpsx_libm.hpp, compared with glibc bit for bit on the CPU), so the loops'
 * floats come out identical -- observed on every committed reference trace and on 26 000 channels from random states: every
 * byte of every record.  What remains different by construction: the double-precision atan2 of the PLL's IP <= 0 branch is the
 * device's (its result rounded to float differs from glibc's in about one argument pair in 2^29), and snr_value's logarithm
 * (a display value; the record gets the host's log10f of the sums the device latched, gpsx_loop_state_to_channel).  The stated
 * tolerance of SURVEY.md 8(c) -- |d code_phase_fine| <= 0.01 sample, |d if_freq_offset_hz| <= 0.5 Hz -- stays the tests'
 * fallback bar.  The false-lock jump draws by default from a per-channel xorshift32 (`rng`, never 0) instead of libc's
 * process-global rand(); gpsx_loop_set_draws(GPSX_DRAWS_LIBC) gives the reference's draws in the reference's order.
 * Data polarity (gpsx_loop_set_word_sync): the reference's word layer flips inv_polarity_flag when it has seen two inverted
 * preambles, and the very next millisecond's vote and sign-change detection use the new value (nav_data.c:60-66, 284-291).
 *   GPSX_WORDSYNC_DEVICE (default)  the kernel runs the polarity-deciding part of the word layer itself (preamble hunt, word
 *       collection, parity, the two-subframe timeout: 12 bytes of state) on every completed bit, so the flag changes on the
 *       millisecond the reference changes it on, whatever the launch length.  The host's word layer
 *       (gps_tracking_words_batch) sees the same bits at the same ticks and takes the same decisions; it still lists the
 *       channels whose flag changed, and handing them to gpsx_loop_set_polarity is harmless (the device already has the value).
 *   GPSX_WORDSYNC_HOST  the device never touches the flag: a host with its own word layer (one that overrides
 *       gps_nav_data_words_detection) writes it through gpsx_loop_set_polarity; it then takes effect at the next launch. */
typedef struct {
  int32_t  prn;                                /* 1 .. 210 */
  float    code_phase_fine;                    /* gps_tracking_t, same names, same meaning (include/gpsx_compat.h) */
  float    if_freq_offset_hz;
  uint32_t if_freq_accum;
  float    dll_code_err, pll_code_err, fll_err;
  int16_t  fll_old_i, fll_old_q;
  int16_t  pll_check_buf[4];
  uint16_t pll_bad_state_master_cnt;
  uint8_t  pll_bad_state_cnt;
  uint8_t  period_sync_ok_flag;                /* gps_nav_data_t: 20 ms bit period found (selects the PLL's gain set) */
  int16_t  found_freq_offset_hz;               /* gps_acq_t: centre of the false-lock jump */
  uint16_t reseed_count;                       /* false-lock jumps so far */
  uint32_t rng;                                /* xorshift32 state of those jumps; must not be 0 */
  uint32_t i_part_summ, q_part_summ;           /* SNR estimator */
  float    snr_value;
  uint16_t snr_summ_cnt;
  uint16_t code_filt_cnt;                      /* code-phase averaging window of the pseudorange step */
  float    code_phase_fine_filt;
  uint32_t old_swap_time;                      /* gps_nav_data_t: bit synchroniser */
  uint32_t slot_start_ticks;                   /* tick of index 0 of the current 4 ms group */
  int16_t  slot_ip[4];                         /* prompt I of the group so far */
  uint8_t  slot_bits;                          /* bit i = sign bit of index i of the group */
  uint8_t  right_period_cnt, old_reminder, accurate_swap_time, accurate_swap_ok;
  uint8_t  last_bit_pos_cnt, last_bit_neg_cnt;
  uint8_t  inv_polarity_flag;                  /* data polarity inverted: decided by the device's word sync (below), or written
                                                  through gpsx_loop_set_polarity under GPSX_WORDSYNC_HOST */
  uint32_t prev_track_timestamp;               /* gps_tracking_t: tick the channel was last served on */
  uint32_t snr_i_latch, snr_q_latch;           /* the sums snr_value was last made of (q = 0: snr_value stands as it is) */
  uint32_t word_buf;                           /* gps_nav_data_t.word_buf: bit i = word_buf[i]  (the device's word sync) */
  uint32_t word_detection_timestamp;
  uint8_t  word_cnt, word_bit_cnt, inv_preabmle_cnt;
  uint8_t  word_flags;                         /* bit 0 old_D29, bit 1 old_D30, bit 2 polarity_found */
} gpsx_loop_state_t;                           /* 120 bytes */

typedef struct {                               /* optional per-millisecond record, for tests and inspection */
  int16_t  iq[6];                              /* IE, QE, IP, QP, IL, QL of this millisecond */
  float    code_phase_fine, if_freq_offset_hz; /* AFTER this millisecond's loop updates */
  uint32_t if_freq_accum;
} gpsx_loop_trace_t;                           /* 24 bytes */

/* d_if_blocks: n_blocks consecutive 1 ms blocks in device memory (the context's IF format); d_state: n_ch states in device
 * memory, read, advanced by n_blocks milliseconds, written; first_tick_ms: the millisecond tick of the first block;
 * d_flags: [n_blocks][n_ch] bytes (above); d_trace_opt: NULL or [n_blocks][n_ch] records.  Enqueues and returns. */
int gpsx_track_loop_dev(gpsx_ctx *ctx, const void *d_if_blocks, int n_blocks, gpsx_loop_state_t *d_state, int n_ch,
                        uint32_t first_tick_ms, uint8_t *d_flags, gpsx_loop_trace_t *d_trace_opt);
/* The same with the blocks and the flag bytes in host memory (page-locked: gpsx_host_alloc): copies the blocks in,
 * runs, copies the flags (and trace records, if asked for) out, waits.  The states stay on the device. */
int gpsx_track_loop(gpsx_ctx *ctx, const uint8_t *if_blocks, int n_blocks, gpsx_loop_state_t *d_state, int n_ch,
                    uint32_t first_tick_ms, uint8_t *flags, gpsx_loop_trace_t *trace_opt);

/* Serving schedule of this context's gpsx_track_loop* launches from now on (above). */
#define GPSX_SCHED_EVERY_MS 0
#define GPSX_SCHED_MUX17    1
int gpsx_loop_set_schedule(gpsx_ctx *ctx, int schedule);

/* Where the false-lock detector's random carrier jump (PM/GPS/tracking.c:309-326) draws from.
 *   GPSX_DRAWS_XORSHIFT (default)  the channel's own xorshift32 (`rng`): any number of channels, nothing leaves the device.
 *   GPSX_DRAWS_LIBC  the reference's: libc's rand(), drawn on the host in the order a single-threaded loop over the
 *       milliseconds and channels makes the draws -- so a receiver that seeds as the reference does jumps where the reference
 *       jumps (tests/test_gpu_track_loop.py: the 64-channel trace with its 21 jumps).  A launch whose channels want to jump is
 *       run twice for those channels (they report, the host draws, they are replayed from the launch's input state); launches
 *       are limited to 320 ms and gpsx_track_loop_dev WAITS for its kernels in this mode.  rand() is process-global: the
 *       caller seeds it (and see INTEGRATION.md on the ROCm runtime's own draws when code objects load).
 *       A channel has ONE candidate slot per launch (its detector needs 324 ms to fill again, a launch is at most 320): should
 *       a replay not settle in four passes, or a channel report twice inside one launch, the call returns GPSX_EIO and
 *       d_state, flags and trace of that call are UNDEFINED -- restore the states from the caller's copy or drop the channels. */
#define GPSX_DRAWS_XORSHIFT 0
#define GPSX_DRAWS_LIBC     1
int gpsx_loop_set_draws(gpsx_ctx *ctx, int draws);

#define GPSX_WORDSYNC_DEVICE 0
#define GPSX_WORDSYNC_HOST   1
int gpsx_loop_set_word_sync(gpsx_ctx *ctx, int owner);

/* The host's word layer found (or gave up) inverted data polarity on n channels: d_state[channels[i]].inv_polarity_flag =
 * values[i] (host arrays; enqueued on the context's stream in front of the next launch). */
int gpsx_loop_set_polarity(gpsx_ctx *ctx, gpsx_loop_state_t *d_state, const int *channels, const uint8_t *values, int n);

/* The pseudorange step consumed the code-phase averaging window (gps_master_code_phase_filter_reset, gps_master.c:383-389):
 * code_phase_fine_filt = 0, code_filt_cnt = 0 for all n_ch device states (enqueued on the context's stream). */
int gpsx_loop_reset_code_filter(gpsx_ctx *ctx, gpsx_loop_state_t *d_state, int n_ch);

/* ---- per-call primitives on caller buffers (the device work behind include/gpsx_compat.h) --------------------- */

/* gps_shift_to_zero_freq(_track): *accum is the NCO accumulator in/out (0 for the stateless call).  Writes bytes
 * 0..2043 of data_i / data_q only (PM/GPS/gps_misc.c:229: the last 16 samples are never mixed). */
int gpsx_wipeoff(gpsx_ctx *ctx, const uint8_t *signal, float freq_hz, uint32_t *accum, uint8_t *data_i,
                 uint8_t *data_q);
/* gps_generate_prn_data2: chips = 1023 bytes 0/1; out = 1024 words, word 1023 is OR-ed with the spill. */
int gpsx_replica(gpsx_ctx *ctx, const uint8_t *chips, unsigned offset_bits, uint16_t *out);
/* gps_mult_and_summ + gps_correlation8 + gps_correlation_iq for a list of byte offsets (each 0..2046) on arbitrary
 * 2046-byte buffers.  Any of cnt_i/cnt_q (raw popcounts), corr8 may be NULL. */
int gpsx_corr_offsets(gpsx_ctx *ctx, const uint16_t *replica, const uint16_t *data_i, const uint16_t *data_q,
                      const uint16_t *offsets, int n, uint16_t *cnt_i, uint16_t *cnt_q, int16_t *corr8);
/* the magnitude stage of gps_correlation8 alone (PM/GPS/gps_misc.c:106-118) for n raw popcount pairs: centre by 8184,
 * clip negatives to zero, (int16) sqrtf((float)(I*I) + (float)(Q*Q)) */
int gpsx_mag8(gpsx_ctx *ctx, const uint16_t *cnt_i, const uint16_t *cnt_q, int n, int16_t *out);
/* correlation_search on arbitrary buffers */
int gpsx_corr_search(gpsx_ctx *ctx, const uint16_t *replica, const uint16_t *data_i, const uint16_t *data_q,
                     unsigned start_shift, unsigned stop_shift, gpsx_peak_t *peak);
/* gps_rewind_if_phase (PM/GPS/gps_misc.c:196-204) for n channel states (device arithmetic, same rounding) */
int gpsx_rewind(gpsx_ctx *ctx, gpsx_trk_state_t *st, int n_ch, const uint8_t *steps);

#ifdef __cplusplus
}
#endif
#endif /* GPSX_H */
