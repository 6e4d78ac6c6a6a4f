/* mi355fx.h — C ABI of the MI355X (gfx950) kernel library behind gst-plugins-rs' per-buffer
 * DSP elements (hsvfilter, hsvdetector, colorlut, rsaudioecho).
 *
 * This header is the drop-in boundary: each entry point replaces exactly one inner loop of the
 * reference (file:line cited per function, relative to the gst-plugins-rs tree) and takes what
 * that loop takes — plane pointer, stride, width/height, format, the settings snapshot.
 * The reference element keeps its GObject/BaseTransform surface and calls these through
 * `extern "C"` FFI (binding shown in INTEGRATION.md). Plain pointers and sizes only.
 *
 * Conventions
 *   - Every function returns MI355_OK (0) or a negative mi355_status; mi355_ctx_last_error()
 *     gives a human-readable message for the last failure on that context. The element maps any
 *     non-zero status to GST_FLOW_ERROR (transform vfuncs) or an ErrorMessage (start/setup).
 *   - One context = one element instance. A context is used by one thread at a time (the
 *     streaming thread, serialised by the pad stream lock); different contexts are independent.
 *   - "host" entry points borrow the caller's buffer for the duration of the call only
 *     (GstVideoFrame / GstBuffer map semantics): H2D copy, kernel, D2H copy, then return.
 *   - "_device" entry points take device pointers, enqueue on the context's stream and return
 *     without synchronising (adjacent mi355 elements, benchmarks).
 *   - There is no CPU fallback: without a usable gfx950 device every call fails loudly.
 */
#ifndef MI355FX_H
#define MI355FX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI355FX_ABI_VERSION 1

typedef enum mi355_status {
  MI355_OK = 0,
  MI355_ERR_INVALID_ARG = -1,   /* bad pointer / size / format            */
  MI355_ERR_NO_DEVICE = -2,     /* no gfx950 device, or HIP init failed   */
  MI355_ERR_HIP = -3,           /* a HIP runtime call or kernel failed    */
  MI355_ERR_NOT_CONFIGURED = -4,/* e.g. colorlut without a loaded LUT (colorlut/imp.rs:209-212),
                                   echo before setup (audioecho/imp.rs:210 NotNegotiated) */
  MI355_ERR_OUT_OF_MEMORY = -5,
  MI355_ERR_UNSUPPORTED = -6,
  MI355_ERR_TIMEOUT = -7        /* (reserved: mi355_agroup_wait of a lock-step group returned it; the members of every audio group are independent now) */
} mi355_status;

/* Packed-RGB formats of the hot path. Values are stable ABI.
 * hsvfilter caps: video/hsv/src/hsvfilter/imp.rs:274-312; colorlut caps: video/colorlut/src/colorlut/imp.rs:118-157. */
typedef enum mi355_video_format {
  MI355_FMT_RGBX = 0,
  MI355_FMT_XRGB = 1,
  MI355_FMT_BGRX = 2,
  MI355_FMT_XBGR = 3,
  MI355_FMT_RGBA = 4,
  MI355_FMT_ARGB = 5,
  MI355_FMT_BGRA = 6,
  MI355_FMT_ABGR = 7,
  MI355_FMT_RGB = 8,
  MI355_FMT_BGR = 9,
  MI355_FMT_RGBA64_LE = 10,
  MI355_FMT_RGBA64_BE = 11
} mi355_video_format;

typedef struct mi355_ctx mi355_ctx;

/* ---------------------------------------------------------------- context / plumbing */

int mi355_abi_version(void);
/* Number of visible HIP devices (0 if none or the runtime cannot initialise). */
int mi355_device_count(void);
/* Create a context on `device` (its own non-blocking stream). NULL on failure; *status set if non-NULL. */
mi355_ctx *mi355_ctx_create(int device, int *status);
void mi355_ctx_destroy(mi355_ctx *ctx);
const char *mi355_ctx_last_error(const mi355_ctx *ctx);
const char *mi355_status_string(int status);
/* hipStream_t of the context (as void*). */
void *mi355_ctx_stream(mi355_ctx *ctx);
/* Use an externally owned stream (e.g. the stream of the neighbouring element) instead. */
int mi355_ctx_set_stream(mi355_ctx *ctx, void *hip_stream);
int mi355_ctx_synchronize(mi355_ctx *ctx);

/* Diagnostic switches (tests, A/B measurements). MI355_FLAG_FORCE_GENERIC=1 makes every element use
 * its literal-arithmetic GENERIC kernel instead of the strength-reduced FAST one. */
typedef enum mi355_flag {
  MI355_FLAG_FORCE_GENERIC = 1,
  MI355_FLAG_HSV_BLOCKS_PER_CU = 2, /* grid cap (blocks per CU) of the streaming hsvfilter kernel; tuning knob */
  /* colorlut kernel choice for packed RGBA8 frames. 0 = auto (default): the interpolating kernel and the 2^24-entry
   * memoised-table kernel (built on the device from the interpolating kernel, so bit-identical) are both timed on the
   * first four launches after a LUT load; afterwards the kind in use is re-timed every 8th-32nd launch and the other
   * one every 64-1024 launches, and the faster one serves the launches in between. mi355_hsv_colorlut_* does the same
   * with a table of the composed function. 6 = interpolating kernels only: the brick-cache kernel (colorlut_brick.hip),
   * with noise-like streams handed to the three-pass whole-plane kernel by a miss-counter watch that never blocks;
   * 7 = brick-cache kernel only; 3 = three-pass kernel only; 1 / 2 = the three-pass kernel's late-prefetch / lean-state
   * forms (tuning experiments); 4 / 5 = table through the gather kernels only, linear / Morton table index; 8 = Morton table
   * read through a block-shared LDS cache of table bricks (colorlut_window.hip) where the launch is large enough; 9 =
   * Morton table, 5's or 8's kernel by measurement. Auto builds the Morton table and picks as 9 does. Auto records and queries events on
   * the context's stream: pin a variant (7, 3, 5 or 8) before capturing that stream into a hipGraph. */
  MI355_FLAG_LUT_VARIANT = 4,
  /* hsvfilter on packed colour-first 4-byte frames through a memoised table: 0 (default) = auto choice as for colorlut,
   * but only for settings that need the literal GENERIC arithmetic (|hue-shift| > 360 or non-finite); 1 = auto choice
   * for all settings; 2 = table only; 3 = arithmetic kernels only */
  MI355_FLAG_HSV_TABLE = 6,
  MI355_FLAG_LUT_STAGGER = 5,  /* colorlut 3D LDS kernel: spread of the per-block start delay in units of 256 clock ticks (0 = off) */
  MI355_FLAG_FUSED_VARIANT = 3, /* fused hsv+colorlut tiling: 0 = hsv inline after the load (default); 1 = software-pipelined kernel */
  MI355_FLAG_BRICK_TILES_PER_RUN = 7, /* brick-cache kernel: tiles (128 pixels x 4 or 8 rows) in a run, the part of a strip one wave owns (0 = default: one run per wave of the chip) */
  MI355_FLAG_DSSIM_TRANSLUCENT = 11, /* Dssim on RGBA pixels with alpha < 255: 0 (default) = composed over the crate's coloured, position-dependent pattern (mi355_dssim_create_image), 1 = over black (premultiplied values as they are) */
  MI355_FLAG_DSSIM_FAST = 19, /* Dssim on (reference, frame) PAIRS (mi355_dssim_compare_pairs*, mi355_dssim_pair_map_device, mi355_group_submit_compare), read when a pair is handed over: 0 (default) = the exact form, bit-identical to the restated algorithm; 1 = the fast form - the same algorithm with every 3x3 blur pass as a horizontal and a vertical 3-tap pass (taps [0.30876, 0.38248, 0.30876] * sqrt(1.000001)), one kernel per scale and pair, no image planes in memory; its value differs from the exact form's by f32 rounding noise (1e-5), identical frames still give exactly 0.0. Other values are refused. Image handles (mi355_dssim_create_image / _compare / _compare_frames*) are the exact form's objects and stay exact whatever this flag says */
  MI355_FLAG_BRICK_FOLD_AXIS = 10, /* accepted and ignored: the 32-set geometry of the brick-cache kernel is hashed over all three axes now (it used to give one axis 2 set residues instead of 4) */
  MI355_FLAG_BRICK_PRIO = 9, /* brick-cache kernel, how the waves of a block share work: bit 0 = waves lower their issue priority as they advance through their run, bit 1 = a wave that is done takes tiles from the run with most left (default 3) */
  MI355_FLAG_HRTF_METHOD = 12, /* hrtfrender convolution, read at mi355_hrtf_setup: 0 (default) = overlap-save FFT in LDS from 384-tap HRIRs on (the measured crossover), time-domain FIR below; 1 = FFT, 2 = FIR pinned (each only where it fits the LDS) */
  MI355_FLAG_BLOCKHASH_ANY_SIZE = 15, /* videocompare Blockhash on frames whose width or height is not a multiple of 8: 0 (default) = MI355_ERR_UNSUPPORTED, 1 = the crate's floating-point path (blockhash_slow: every pixel whole to block (floor(x / (w/8)), floor(y / (h/8))) in f32, block sums accumulated in pixel order - one lane per block, sequential by definition, 1-2 ms per 4K frame; restated from memory like the rest of the hash: parity unpinned) */
  MI355_FLAG_HSV_NT = 14, /* hsvfilter on packed 4-byte frames, how the flat kernels touch memory. 2 (default) = plain loads, write-through stores (system scope, no non-temporal bit): the kernel ends with no dirty L2 lines to drain and its output still allocates in the Infinity Cache, where the element behind it finds it; + 2.3 % on the hsvfilter ! colorlut chain against 0 = plain loads and stores (profiles/r07_store_policy_ab.txt). 1 = loads and stores carry the non-temporal hint: the kernel alone is 2-5 % faster than 0, but its output then bypasses the Infinity Cache and the element behind it reads from HBM (bench.py's `hsvfilter_nontemporal_ab` leg measures exactly that; lone entry only). The bytes are the same under all three */
  MI355_FLAG_WINDOW_ORDER = 17, /* LDS-cached table kernel: how its blocks share the picture: 1 (default) = aligned fronts (block b takes strip b % n_strips, layer b / n_strips; the blocks of a layer walk down side by side, so the chip streams a few bands of full rows), 0 = a contiguous share of the column-major step list each (round 4); A/B knob */
  MI355_FLAG_WINDOW_STATS = 18, /* 1 = the LDS-cached table kernels count pixels / pixels served past the cache / bricks installed for mi355_colorlut_window_stats (three atomics per wave; default 0) */
  MI355_FLAG_WINDOW_MIN_STEPS = 13, /* LDS-cached table kernel (LUT variants 0 / 8): smallest launch it serves, in 256 x 32 pixel steps per CU (default 3; 0 = any size - its first step per block runs on a cold cache, so small launches are faster through the gather kernels) */
  MI355_FLAG_BRICK_SETS = 8 /* brick-cache kernels: 0 (default) = chosen by the content watch; pinned: 32 (16 waves per CU) or 64 (8 waves per CU) sets per WAVE cache, 512 = the block-shared cache of colorlut3d_shared_kernel (512 sets per CU, RGBA8 plain colorlut, launches of at least 3 steps of 256 x 32 pixels per CU; smaller ones take the 32-set kernel); two ways each */
} mi355_flag;
int mi355_ctx_set_flag(mi355_ctx *ctx, int flag, int value);

void *mi355_device_alloc(mi355_ctx *ctx, size_t bytes);
int mi355_device_free(mi355_ctx *ctx, void *dptr);
int mi355_memcpy_h2d(mi355_ctx *ctx, void *dptr, const void *host, size_t bytes); /* synchronous */
int mi355_memcpy_d2h(mi355_ctx *ctx, void *host, const void *dptr, size_t bytes); /* synchronous */

/* ---------------------------------------------------------------- hsvfilter
 * Replaces HsvFilter::hsv_filter + the format match of transform_frame_ip
 * (video/hsv/src/hsvfilter/imp.rs:76-120, :323-376) and the hsvutils conversions it calls
 * (video/hsv/src/hsvutils.rs:44-198). Settings snapshot = `Settings` (hsvfilter/imp.rs:33-39). */
typedef struct mi355_hsv_settings {
  float hue_shift;      /* "hue-shift"      default 0.0 */
  float saturation_mul; /* "saturation-mul" default 1.0 */
  float saturation_off; /* "saturation-off" default 0.0 */
  float value_mul;      /* "value-mul"      default 1.0 */
  float value_off;      /* "value-off"      default 0.0 */
} mi355_hsv_settings;

/* In place on plane 0 of a mapped frame in host memory. `data_len` = plane_data_mut(0).len();
 * rows processed = data_len / stride (chunks_exact_mut drops a trailing partial row). */
int mi355_hsvfilter_frame_ip(mi355_ctx *ctx, uint8_t *data, size_t data_len, int width, int stride,
                             int format, const mi355_hsv_settings *settings);
/* Same on `n_frames` device-resident frames, frame f at d_data + f*frame_pitch. Asynchronous. */
int mi355_hsvfilter_frames_device(mi355_ctx *ctx, uint8_t *d_data, int n_frames, size_t frame_pitch,
                                  int width, int height, int stride, int format,
                                  const mi355_hsv_settings *settings);

/* ---------------------------------------------------------------- hsvdetector
 * Replaces HsvDetector::hsv_detect + transform_frame's 6x4 format match
 * (video/hsv/src/hsvdetector/imp.rs:100-160, :423-707). */
typedef struct mi355_hsvdetect_settings {
  float hue_ref, hue_var;               /* defaults 0.0, 10.0 */
  float saturation_ref, saturation_var; /* defaults 0.0, 0.15 */
  float value_ref, value_var;           /* defaults 0.0, 0.3  */
} mi355_hsvdetect_settings;

int mi355_hsvdetect_frame(mi355_ctx *ctx, const uint8_t *src, size_t src_len, int src_stride,
                          int src_format, uint8_t *dst, size_t dst_len, int dst_stride,
                          int dst_format, int width, const mi355_hsvdetect_settings *settings);
int mi355_hsvdetect_frames_device(mi355_ctx *ctx, const uint8_t *d_src, size_t src_pitch,
                                  int src_stride, int src_format, uint8_t *d_dst, size_t dst_pitch,
                                  int dst_stride, int dst_format, int n_frames, int width,
                                  int height, const mi355_hsvdetect_settings *settings);

/* ---------------------------------------------------------------- colorlut
 * mi355_colorlut_load replaces the `State { lut }` installed by ColorLut::start
 * (video/colorlut/src/colorlut/imp.rs:168-194): the element keeps parsing the .cube text
 * (video/colorlut/src/parser.rs:110-281) and hands over the parsed CubeLut:
 *   is3d=1: `table` = Lut3D::as_flat(), size^3 cells of [r,g,b,1.0], index x + y*size + z*size^2
 *           (parser.rs:19-53, :253-256);  is3d=0: r[size], g[size], b[size] back to back
 *           (CubeLutKind::Lut1D, parser.rs:57-66).
 *   domain_scale / domain_offset: CubeLut fields (parser.rs:69-75, :264-274). */
int mi355_colorlut_load(mi355_ctx *ctx, int is3d, size_t size, const float *table,
                        const float domain_scale[3], const float domain_offset[3]);
/* ColorLut::stop (colorlut/imp.rs:196-199). */
int mi355_colorlut_unload(mi355_ctx *ctx);
/* Diagnostics for MI355_FLAG_LUT_VARIANT 0 (auto): which kernel kind serves packed RGBA8 launches right now
 * (*table_in_use: 0 interpolating kernel, 1 memoised table) and the last measured time of each kind in ms per
 * megapixel (0 = not measured yet); fused = 0 for mi355_colorlut_*, 1 for mi355_hsv_colorlut_*, 2 for
 * mi355_hsvfilter_* (MI355_FLAG_HSV_TABLE; *table_in_use then tells what the last call ran); fused = 10 / 11: the choice
 * INSIDE the table path of mi355_colorlut_* / mi355_hsv_colorlut_* - *table_in_use: 1 = the LDS-cached kernel
 * (colorlut_window.hip), 0 = the gather kernel; "compute" = the gather kernel's time, "table" = the LDS-cached kernel's. No
 * reference counterpart. */
int mi355_colorlut_kernel_choice(mi355_ctx *ctx, int fused, int *table_in_use, double *ms_per_mpx_compute, double *ms_per_mpx_table);
/* Number of memoised 64 MiB tables alive in this process (tables are shared by all contexts that ask for the same
 * function on the same device: same LUT and layout, same hsv settings). Diagnostic; no reference counterpart. */
int mi355_shared_table_count(void);
/* Name of the kernel that served the last mi355_colorlut_* / mi355_hsv_colorlut_* launch of this context ("" before the
 * first one). Diagnostic; no reference counterpart. */
const char *mi355_colorlut_last_kernel(mi355_ctx *ctx);
/* Brick-cache kernel diagnostics (synchronous): counters[0] = 256-pixel steps that found a brick missing in the wave's
 * LDS cache since the last reset, counters[1] = steps that still missed after the fill rounds (slow path);
 * *last_miss_fraction = miss fraction of the content watch's last snapshot, *level = the level it has settled on (0 brick
 * kernel with 32 sets, 1 with 64 sets, 2 three-pass kernel). reset != 0 clears the device counters. No reference counterpart. */
int mi355_colorlut_brick_stats(mi355_ctx *ctx, uint64_t counters[2], double *last_miss_fraction, int *level, int reset);
/* Diagnostics of the LDS-cached memoised-table kernel (csrc/colorlut_window.hip; synchronous): counters[0] = pixels it
 * has looked up on this context since the last reset, counters[1] = pixels whose table brick was not in the block's
 * LDS cache (served from the table in global memory), counters[2] = bricks installed. No reference counterpart. */
int mi355_colorlut_window_stats(mi355_ctx *ctx, uint64_t counters[3], int reset);
/* Host-logic self test of the content-watch policy (csrc/brickwatch.hpp) against a scripted stream, no GPU needed: call i
 * would show miss / slow step fractions miss0[i], slow0[i] on the 32-set brick kernel and miss1[i], slow1[i] on the 64-set
 * one; snapshots become readable `lag` calls late. level_out[i] = 0 / 1 / 2 as above. */
int mi355_selftest_brickwatch(int n_calls, const double *miss0, const double *slow0, const double *miss1, const double *slow1, int lag,
                              int *level_out);
/* Host-logic self test of the auto-choice policy against a scripted device (no GPU needed): call i has n_vec[i] 16-byte
 * pixel groups and, if measured, takes ms_compute[i] or ms_table[i] depending on the kind it ran; a measurement becomes
 * readable `lag` calls later. kind_out[i] = 0 interpolating / 1 table, measured_out[i] (optional) = launch was bracketed. */
int mi355_selftest_autopick(int n_calls, const uint64_t *n_vec, const double *ms_compute, const double *ms_table, int lag,
                            int *kind_out, int *measured_out);
/* The same with the input's provenance scripted: settled[i] != 0 means call i reads what the launch before it wrote, still
 * on-die (hsvfilter ! colorlut); there the samples of the table kind in use thin out to one per 1024 launches while they
 * agree. settled == NULL is mi355_selftest_autopick. */
int mi355_selftest_autopick_settled(int n_calls, const uint64_t *n_vec, const double *ms_compute, const double *ms_table, const int *settled,
                                    int lag, int *kind_out, int *measured_out);
/* Replaces transform_frame's body: transform_rgba / transform_rgba64::<LE>
 * (colorlut/imp.rs:203-223 -> :226-397). format in {RGBA, RGBA64_LE, RGBA64_BE}; src and dst are
 * plane 0 of two different frames with independent strides; rows = chunks(stride).take(height). */
int mi355_colorlut_frame(mi355_ctx *ctx, const uint8_t *src, int src_stride, uint8_t *dst,
                         int dst_stride, int width, int height, int format);
int mi355_colorlut_frames_device(mi355_ctx *ctx, const uint8_t *d_src, size_t src_pitch,
                                 int src_stride, uint8_t *d_dst, size_t dst_pitch, int dst_stride,
                                 int n_frames, int width, int height, int format);

/* Measurement plumbing, no reference counterpart: one round of n independent streams issued from ONE native loop - for
 * stream i, hsvfilter in place on the frame at d_src[i] and colorlut from it into d_dst[i], each through its own context
 * ctxs[i] (own HIP stream, LUT loaded) exactly as mi355_hsvfilter_frames_device + mi355_colorlut_frames_device would be
 * called by that stream's thread. Lets a benchmark written in an interpreter measure the device instead of its own call
 * overhead. Returns the first error; asynchronous like the calls it makes. */
int mi355_issue_streams_round(mi355_ctx *const *ctxs, int n_streams, uint8_t *const *d_src, uint8_t *const *d_dst,
                              int width, int height, int stride, int format, const mi355_hsv_settings *settings);

/* ---------------------------------------------------------------- many streams, few launches (csrc/group.hip)
 * GstBaseTransform hands an element ONE buffer per call (hsvfilter/imp.rs:323-376, colorlut/imp.rs:203-223): N streams through
 * `hsvfilter ! colorlut` are 2 N short launches per frame period, each paying its own ramp and tail. A group collects what the
 * streams submit and issues the frames of up to max_batch streams that agree in size, format, hsv settings and LUT as ONE
 * hsvfilter launch and ONE colorlut launch (the frame's base pointer is looked up per block); everything else goes through
 * its context's own path, in order. Results are those of mi355_hsvfilter_frames_device + mi355_colorlut_frames_device on that
 * frame, bit for bit. No reference counterpart (the reference has no device to batch for).
 *   create : max_batch 0 = default (8 frames per launch), at most 16.
 *   submit_chain : hsvfilter in place on the packed RGBA frame at d_src (stride bytes per row; MI355_FMT_RGBA, the one format both
 *           elements accept - anything else is MI355_ERR_INVALID_ARG), then colorlut from it into d_dst,
 *           for stream `ctx` (its LUT, loaded with mi355_colorlut_load; the frame starts after what ctx's HIP stream held at
 *           this call). Never blocks; launches only when max_batch frames are pending. One frame per stream and launch:
 *           frames of one stream run in submission order. *ticket identifies the frame.
 *   flush  : launch what is pending now.
 *   order_after : makes ctx's HIP stream wait (on the device, no host wait) for the frame `ticket`: what ctx enqueues on its
 *           own stream afterwards - a download - sees the result. Not implied by submit.
 *   wait   : host wait until the frame `ticket` is in d_dst; flushes first if the frame has not been launched - an element
 *           that works one frame deep (submit n, wait n-1) thereby batches with whatever the other streams submitted in
 *           between. The group's lock is not held while waiting.
 *   stats  : {frames, batched launch pairs, frames that went through their context's own path}.
 * Threads: every entry point may be called from any thread (one lock per group, not held during host waits). A flush launches
 * on behalf of EVERY stream with a pending frame, from whichever thread caused it, and reads those streams' contexts (LUT
 * table, flags): between submit and the return of wait for that ticket a context is used only through the group - no LUT
 * reload / unload, no flag change, no other entry point, no destroy. A launch that fails is reported to the call that caused
 * it and, once, to wait / order_after for each frame it carried (never as a silent success). */
typedef struct mi355_group mi355_group;
mi355_group *mi355_group_create(int device, int max_batch, int *status);
void mi355_group_destroy(mi355_group *group);
const char *mi355_group_last_error(mi355_group *group);
int mi355_group_submit_chain(mi355_group *group, mi355_ctx *ctx, uint8_t *d_src, uint8_t *d_dst, int width, int height,
                             int stride, int format, const mi355_hsv_settings *settings, uint64_t *ticket);
/* The same for the FUSED pair (mi355_hsv_colorlut_frames_device's semantics: d_src is read and left untouched, d_src == d_dst
 * allowed): frames that agree in size, hsv settings and LUT share ONE launch through the composed table of those settings
 * (built - or found with another stream of the process - once a stream has submitted with them eight times in a row: a hue
 * shift animated frame by frame never builds one). 3D LUTs; everything else goes through its context's own fused path. Bit-identical to mi355_hsv_colorlut_frames_device on that frame. */
int mi355_group_submit_fused(mi355_group *group, mi355_ctx *ctx, uint8_t *d_src, uint8_t *d_dst, int width, int height,
                             int stride, int format, const mi355_hsv_settings *settings, uint64_t *ticket);
int mi355_group_flush(mi355_group *group);
int mi355_group_order_after(mi355_group *group, mi355_ctx *ctx, uint64_t ticket);
int mi355_group_wait(mi355_group *group, uint64_t ticket);
int mi355_group_wait_all(mi355_group *group);
int mi355_group_stats(mi355_group *group, uint64_t stats[3]);
/* Measurement plumbing like mi355_issue_streams_round: one frame of each of n streams submitted from one native loop, then
 * flushed - what n streaming threads that submit within one frame period amount to. */
int mi355_group_submit_round(mi355_group *group, mi355_ctx *const *ctxs, int n_streams, uint8_t *const *d_src,
                             uint8_t *const *d_dst, int width, int height, int stride, int format,
                             const mi355_hsv_settings *settings);
int mi355_group_submit_round_fused(mi355_group *group, mi355_ctx *const *ctxs, int n_streams, uint8_t *const *d_src,
                                   uint8_t *const *d_dst, int width, int height, int stride, int format,
                                   const mi355_hsv_settings *settings);

/* videocompare across independent element instances. The reference's aggregate() hashes the reference pad's frame, then hashes and
 * compares every other pad's frame (video/videofx/src/videocompare/imp.rs:316-350 -> hashed_image.rs:24-79) - per element, one
 * synchronous engine call per frame. N two-pad elements in one process are N such sequences on N streams, which on one device
 * run SLOWER side by side than one after the other (32 4K Dssim streams over 8 contexts: 1.8 k comparisons/s; one context in
 * sequence: 2.2 k). submit_compare queues one (reference frame, frame) pair of stream `ctx`; pairs of one geometry, format and
 * algorithm run as ONE launch sequence on the group's compare stream - every pair's reference image is created right before the
 * kernels that read it (one image pool for the whole batch), pairs with the same d_ref (videocompare with several pads) share
 * it, the reductions and the copy of the scores happen once per batch - and wait_compare returns what
 * mi355_dssim_create_image + mi355_dssim_compare_frames (algo MI355_HASH_DSSIM: *distance = the dssim value) or
 * mi355_videocompare_hash_frame x 2 + mi355_videocompare_distance (MI355_HASH_BLOCKHASH: hashes[0] the reference's, hashes[1] the
 * frame's) give for that pair, bit for bit. Other algorithms: MI355_ERR_UNSUPPORTED (they go through their context).
 *   set_rendezvous : an element needs its result before it can return from aggregate(), so every stream submits and waits at
 *           once. With expected_streams > 0 a launch goes out as soon as that many pairs are pending, and a waiter whose pair
 *           has not been launched lingers up to linger_us for the others before it launches what is there (0 / 0 = a wait
 *           launches at once, the behaviour of mi355_group_wait).
 *   Frames are read until wait_compare for their ticket has returned. A result is collected once. Threads as for the group.
 *   set_compare_lanes : the pairs of a launch sequence are dealt out to this many HIP streams (default 8, 1..16; before the first
 *           submit_compare): the Dssim kernels are VALU-bound and ~80 % busy when one runs alone - a neighbour stream's launches
 *           fill its tails (32 4K pairs: 1.48 k comparisons/s on one stream, 1.84 k+ over eight).
 */
int mi355_group_set_rendezvous(mi355_group *group, int expected_streams, unsigned linger_us);
int mi355_group_set_compare_lanes(mi355_group *group, int lanes);
int mi355_group_submit_compare(mi355_group *group, mi355_ctx *ctx, const uint8_t *d_ref, const uint8_t *d_frame, int stride, int width, int height,
                               int format, int algo, uint64_t *ticket);
int mi355_group_wait_compare(mi355_group *group, uint64_t ticket, double *distance, uint64_t hashes[2]);
/* {pairs launched, launch sequences, pairs in the largest one} */
int mi355_group_compare_stats(mi355_group *group, uint64_t stats[3]);

/* colordetect across independent element instances. The reference runs get_palette once per frame and element
 * (video/videofx/src/colordetect/imp.rs:57-84); N instances in one process are N times two short launches, an 800-byte copy and a
 * host synchronisation, and a lone frame's histogram launch cannot fill the device (one block per 16 Ki samples, 128 KiB of LDS
 * each). submit_colordetect queues one flat device plane of stream `ctx` - plane_data(0) as the lone entry points read it: strides
 * ignored, every quality-th pixel of floor(data_len / channels) - and whatever is pending goes out as ONE histogram launch over a
 * job table, ONE MMCQ launch and ONE copy of the palettes, on the queue's own HIP stream. Members are fully independent: each
 * frame has its own size, format, quality and max_colors. wait_colordetect returns what mi355_colordetect_frames_device(ctx,
 * d_data, data_len, data_len, 1, format, quality, max_colors, ...) returns for that plane, byte for byte (integer arithmetic
 * only): n_colors entries in palette order, the rest of the 765 bytes zero; a plane where no sample is kept gives 0 colours.
 *   submit : never blocks; the checks and status codes are those of mi355_colordetect_frames_device with n_frames = 1 (format,
 *           quality 1..10, max_colors 2..255, at most 2^32 - 1 samples; a null d_data with data_len > 0, a null ctx or a null
 *           ticket: MI355_ERR_INVALID_ARG). A refused submit queues nothing. The frame is read after what ctx's HIP stream held at
 *           the call, and until wait_colordetect for its ticket has returned.
 *   wait   : launches what is pending if the frame has not gone out (rendezvous first), then waits for its launch set; the
 *           group's lock is not held meanwhile. A result is collected once. Tickets are one sequence per group: a ticket that is
 *           unknown, already collected, a filter frame's, a compare pair's, a detector frame's or a decoder tensor's is
 *           MI355_ERR_INVALID_ARG here and stays collectable where it belongs; mi355_group_wait, _order_after and _wait_compare
 *           refuse a colordetect ticket likewise.
 *   set_colordetect_rendezvous : as set_rendezvous, counted over pending colordetect frames only. The compare queue's
 *           rendezvous, lanes and stats and this queue's do not touch each other.
 *   At most MI355_COLORDETECT_SET_MAX frames share a launch set; more go out as consecutive sets. flush, wait_all and destroy
 *   cover this queue as they cover pairs. A launch that fails is reported to the call that caused it and, once, to each frame's
 *   own wait. Scratch (the set's histograms and results on the device, pinned result blocks) belongs to the group and is
 *   allocated at the first submit.
 *   colordetect_stats : {frames launched, launch sets, frames in the largest set, kernel launches} - a set is two launches, one
 *           when none of its frames has a sample.
 *   mi355_selftest_colordetect_plan : host only, no device: the blocks of one launch set's histogram grid for n_jobs frames of
 *           n_samples[j] samples on n_cu CUs - one block per CU in all, shared out by sample count; every frame with samples
 *           gets at least one and at most ceil(n_samples / 16384), a frame without samples none; first_block is the running sum. */
#define MI355_COLORDETECT_SET_MAX 32 /* frames per launch set */
int mi355_group_set_colordetect_rendezvous(mi355_group *group, int expected_streams, unsigned linger_us);
int mi355_group_submit_colordetect(mi355_group *group, mi355_ctx *ctx, const uint8_t *d_data, size_t data_len, int format, int quality,
                                   int max_colors, uint64_t *ticket);
int mi355_group_wait_colordetect(mi355_group *group, uint64_t ticket, uint8_t palette_rgb[255 * 3], int *n_colors);
/* {frames launched, launch sets, frames in the largest set, kernel launches} */
int mi355_group_colordetect_stats(mi355_group *group, uint64_t stats[4]);
/* host only, no device: the block plan of one launch set */
int mi355_selftest_colordetect_plan(int n_cu, int n_jobs, const uint64_t *n_samples, uint32_t *first_block, uint32_t *blocks,
                                    uint64_t *samples_per_block, uint32_t *total_blocks);

/* hsvdetector across independent element instances. The reference hands each element one buffer per call
 * (video/hsv/src/hsvdetector/imp.rs:423-707); N detectors in one process are N short launches per frame period, each a few
 * microseconds of device work behind a launch that costs more. submit_hsvdetect queues one device frame of stream `ctx` and whatever
 * is pending goes out as at most TWO launches over a job table in the kernel arguments, on the queue's own HIP stream. Members are
 * fully independent: each frame has its own size, strides, input format (RGBx, xRGB, BGRx, xBGR, RGB, BGR), output format (RGBA,
 * ARGB, BGRA, ABGR) and six settings. After wait_hsvdetect, d_dst holds what mi355_hsvdetect_frames_device(ctx, d_src, 0,
 * src_stride, src_format, d_dst, 0, dst_stride, dst_format, 1, width, height, settings) would have written, byte for byte, and no
 * byte outside width * 4 bytes of each of height rows has been touched.
 *   submit : never blocks; the checks and status codes are those of mi355_hsvdetect_frames_device with n_frames = 1 (format pair,
 *           settings pointer, negative sizes, null data with a non-empty frame, line bytes against stride; a null ctx or a null
 *           ticket: MI355_ERR_INVALID_ARG). A refused submit queues nothing. A frame with width == 0 or height == 0 is accepted,
 *           gets a ticket and writes nothing. The settings are copied and the member's MI355_FLAG_FORCE_GENERIC is read at submit.
 *           The frame is read after what ctx's HIP stream held at the call; d_src is read and d_dst written until wait_hsvdetect
 *           for the ticket has returned.
 *   wait   : launches what is pending if the frame has not gone out (rendezvous first), then waits for its launch set; the
 *           group's lock is not held meanwhile. A result is collected once. Tickets are one sequence per group: a ticket that is
 *           unknown, already collected or another queue's (a decoder tensor's included) is MI355_ERR_INVALID_ARG here and stays
 *           collectable where it belongs; mi355_group_wait, _order_after, _wait_compare and _wait_colordetect refuse a detector
 *           ticket likewise.
 *   set_hsvdetect_rendezvous : as set_colordetect_rendezvous, counted over pending detector frames only. The other queues'
 *           rendezvous, streams and stats and this queue's do not touch each other.
 *   At most MI355_HSVDETECT_SET_MAX frames share a launch set; more go out as consecutive sets. flush, wait_all and destroy cover
 *   this queue as they cover the others. A launch that fails is reported to the call that caused it and, once, to each frame's
 *   own wait.
 *   The two launches: the vector launch (four pixels per lane) carries every frame the lone entry would give to its flat or its
 *   rgb24 kernel - packed rows on both sides, destination 16-byte aligned, source 16-byte (4-byte input) or 4-byte (3-byte input)
 *   aligned, pixel count a multiple of 4, 180 - hue_ref in [-360, 360], FORCE_GENERIC off; the literal launch (one pixel per lane,
 *   IEEE division and fmodf) carries every other frame.
 *   hsvdetect_stats : {frames launched, launch sets, frames in the largest set, kernel launches} - per set 0 launches when no frame
 *           has a pixel, 1 when all frames are of one class, 2 when both classes occur.
 *   mi355_selftest_hsvdetect_plan : host only, no device: the blocks of one launch over n_jobs jobs of units[j] work units.
 *           budget = n_cu * blocks_per_cu (at most 2^31 - 1); job j wants ceil(units[j] / units_per_block) blocks. If the wants fit
 *           the budget every job gets its want. Otherwise every job with units gets one block and the rest of the budget is shared
 *           in proportion to what the jobs still want (want - 1), rounded down: no job gets more than its want, a job without
 *           units gets none, and the total is at most max(budget, jobs with units). first_block is the running sum. The vector
 *           launch plans 16-byte pixel groups with units_per_block = 512 and blocks_per_cu = 64, the literal launch pixels with 256
 *           and 32. Refused (MI355_ERR_INVALID_ARG): n_cu < 1, blocks_per_cu < 1, units_per_block == 0, n_jobs outside
 *           0..MI355_HSVDETECT_SET_MAX, null arrays with n_jobs > 0, a null total_blocks. */
#define MI355_HSVDETECT_SET_MAX 32 /* frames per launch set */
int mi355_group_set_hsvdetect_rendezvous(mi355_group *group, int expected_streams, unsigned linger_us);
int mi355_group_submit_hsvdetect(mi355_group *group, mi355_ctx *ctx, const uint8_t *d_src, int src_stride, int src_format,
                                 uint8_t *d_dst, int dst_stride, int dst_format, int width, int height,
                                 const mi355_hsvdetect_settings *settings, uint64_t *ticket);
int mi355_group_wait_hsvdetect(mi355_group *group, uint64_t ticket);
/* {frames launched, launch sets, frames in the largest set, kernel launches} */
int mi355_group_hsvdetect_stats(mi355_group *group, uint64_t stats[4]);
/* host only, no device: the block plan of one launch of a set */
int mi355_selftest_hsvdetect_plan(int n_cu, int blocks_per_cu, unsigned units_per_block, int n_jobs, const uint64_t *units,
                                  uint32_t *first_block, uint32_t *blocks, uint32_t *total_blocks);

/* hsvfilter across independent element instances. The five properties of the element change while playing
 * (video/hsv/src/hsvfilter/imp.rs:127-156) and are snapshotted per buffer (:85): 32 cameras with a hue shift each, or one camera
 * whose shift is animated, are 32 lone launches per frame period. submit_hsvfilter queues one device frame of stream `ctx`, filtered
 * IN PLACE, and whatever is pending goes out as at most TWO launches over a job table in the kernel arguments, on the queue's own
 * HIP stream. Members are fully independent: each frame has its own size, stride, format (the ten 8-bit ones, MI355_FMT_RGBX ...
 * MI355_FMT_BGR) and five settings; no colorlut runs behind it. After wait_hsvfilter the frame's bytes are what
 * mi355_hsvfilter_frames_device(ctx, d_data, 1, 0, width, height, stride, format, settings) would have left, byte for byte (the x /
 * alpha byte of a 4-byte format unchanged), and no byte outside width * pixel_stride bytes of each of height rows has changed. The
 * frame is recorded as recently written, as the lone entry records it: a colorlut behind it sees an on-die source.
 *   submit : never blocks; the checks and status codes are those of mi355_hsvfilter_frames_device with n_frames = 1 (format -
 *           MI355_FMT_RGBA64_* included -, settings pointer, negative sizes, null data with a non-empty frame, stride against line
 *           bytes; a null ctx or a null ticket: MI355_ERR_INVALID_ARG). A refused submit queues nothing. A frame with width == 0 or
 *           height == 0 is accepted, gets a ticket and writes nothing. The settings are copied and the member's
 *           MI355_FLAG_FORCE_GENERIC is read at submit, and MI355_FLAG_HSV_NT for its value 2 (write-through stores for a packed,
 *           aligned 4-byte frame); its value 1 and the context's memoised hsv table play no part: the
 *           group's kernels otherwise use plain loads and stores and compute. The frame is processed after what ctx's HIP stream held at the
 *           call, and is read and written until wait_hsvfilter for the ticket has returned.
 *   order  : in place means order matters: two frames of one launch never touch the same bytes. Overlap is judged on the byte
 *           ranges [d_data, d_data + (height - 1) * stride + width * pixel_stride) - ranges only, conservative. A submit that
 *           overlaps a frame still pending first launches what is pending, then queues; sets run in order on the queue's one
 *           stream, so overlapping frames come out as if filtered one after the other in submission order. Frames that do not
 *           overlap share a set, wherever they were carved from.
 *   wait   : launches what is pending if the frame has not gone out (rendezvous first), then waits for its launch set; the
 *           group's lock is not held meanwhile. A result is collected once. Tickets are one sequence per group: a ticket that is
 *           unknown, already collected or another queue's is MI355_ERR_INVALID_ARG here and stays collectable where it belongs;
 *           mi355_group_wait, _order_after, _wait_compare, _wait_colordetect, _wait_hsvdetect, _wait_yolodec and _wait_handdec
 *           refuse an hsvfilter ticket likewise.
 *   set_hsvfilter_rendezvous : as set_hsvdetect_rendezvous, counted over pending hsvfilter frames only. The other queues'
 *           rendezvous, streams and stats and this queue's do not touch each other.
 *   At most MI355_HSVFILTER_SET_MAX frames share a launch set; more go out as consecutive sets. flush, wait_all and destroy cover
 *   this queue as they cover the others. A launch that fails is reported, once, to each frame's own wait.
 *   The two launches: the vector launch (four pixels per lane, one v_perm_b32 into a canonical byte order and one out of it) carries
 *   every frame whose settings give a FAST variant - hue_shift 0 or 1e-30 <= |hue_shift| <= 2^22, finite, FORCE_GENERIC off - and
 *   whose geometry is the lone entry's flat or rgb24 class: packed rows and, 4-byte formats, a 16-byte aligned base and a byte count
 *   that is a multiple of 16, or, 3-byte formats, a 4-byte aligned base and a byte count that is a multiple of 12 - or its rowpad
 *   class: a 4-byte format with padded rows whose base and stride are multiples of 16 (units: ceil(width / 4) groups per row). The
 *   literal launch (one pixel per lane, byte accesses; IEEE division and fmodf for the settings that need them) carries every other
 *   frame: GENERIC settings, FORCE_GENERIC, unaligned bases, pixel counts that do not fill whole groups, padded rows off the
 *   16-byte multiples and every padded row of a 3-byte format.
 *   hsvfilter_stats : {frames launched, launch sets, frames in the largest set, kernel launches} - per set 0 launches when no frame
 *           has a pixel, 1 when all frames are of one class, 2 when both classes occur.
 *   mi355_selftest_hsvfilter_set_plan : host only, no device: what the builder the queue launches from makes of n_frames frames in
 *           submission order. The addresses are numbers and are never dereferenced. Per frame: `set`, counted from 0 - a new set
 *           begins at MI355_HSVFILTER_SET_MAX frames and in front of a frame that overlaps one of the current set; `launch`, 0 no
 *           pixel, 1 vector, 2 literal; `variant`, vector: the FAST variant (bits 0-1 zero / positive / negative shift, bit 2
 *           identity saturation and value settings, bit 3 wide shift with its sign in bit 0), literal: >= 0 if the single-pixel FAST
 *           routine serves the settings (narrow shifts), -1 for the literal arithmetic, no pixel: -1; `units`, vector: groups of
 *           four pixels, literal: pixels; `first_block` and `blocks`, its share of its launch's grid by
 *           mi355_selftest_hsvdetect_plan's rule (vector: 512 units per block, 64 blocks per CU; literal: 256 and 32). *n_sets: the
 *           sets. Refused (MI355_ERR_INVALID_ARG): n_cu < 1, n_frames < 0, null arrays with n_frames > 0, a null n_sets, and a
 *           frame submit would refuse (format, negative sizes, stride below the line bytes of a frame with a pixel). */
#define MI355_HSVFILTER_SET_MAX 32 /* frames per launch set */
typedef struct mi355_hsvfilter_plan_frame {
  uint64_t address;            /* the frame's first byte, as a number */
  int32_t width, height, stride, format;
  mi355_hsv_settings settings;
  int32_t force_generic;       /* the member's MI355_FLAG_FORCE_GENERIC */
} mi355_hsvfilter_plan_frame;
typedef struct mi355_hsvfilter_plan_out {
  int32_t set, launch, variant;
  uint32_t first_block, blocks, reserved;
  uint64_t units;
} mi355_hsvfilter_plan_out;
int mi355_group_set_hsvfilter_rendezvous(mi355_group *group, int expected_streams, unsigned linger_us);
int mi355_group_submit_hsvfilter(mi355_group *group, mi355_ctx *ctx, uint8_t *d_data, int width, int height, int stride,
                                 int format, const mi355_hsv_settings *settings, uint64_t *ticket);
int mi355_group_wait_hsvfilter(mi355_group *group, uint64_t ticket);
/* {frames launched, launch sets, frames in the largest set, kernel launches} */
int mi355_group_hsvfilter_stats(mi355_group *group, uint64_t stats[4]);
/* host only, no device: the sets, launches and blocks of n_frames frames */
int mi355_selftest_hsvfilter_set_plan(int n_cu, const mi355_hsvfilter_plan_frame *frames, int n_frames,
                                      mi355_hsvfilter_plan_out *out, int *n_sets);

/* ---- colorlut frames of INDEPENDENT element instances (csrc/group.hip, csrc/colorlut_group.hip)
 * colorlut is one instance per stream and one buffer per call (video/colorlut/src/colorlut/imp.rs:203-223): a process that grades 32
 * cameras, each with its own .cube, makes 32 lone launches per frame period, and mi355_group_submit_chain / _fused batch only frames
 * behind an hsvfilter that agree in size, settings and LUT. submit_colorlut queues one device frame of stream `ctx`, source to
 * destination, and whatever is pending goes out as at most TWO launches over a job table in the kernel arguments, on the queue's
 * own HIP stream. Members are fully independent: each frame has its own size, strides and format (MI355_FMT_RGBA, MI355_FMT_RGBA64_LE,
 * MI355_FMT_RGBA64_BE) and the LUT that is loaded in `ctx` at the submit - 1D or 3D, any size and domain mi355_colorlut_load
 * accepts. After wait_colorlut d_dst holds what mi355_colorlut_frames_device(ctx, d_src, 0, src_stride, d_dst, 0, dst_stride, 1, width,
 * height, format) would have written, bit for bit (the alpha byte or word copied), and no byte of d_dst outside the width pixels of
 * each of height rows has changed. The destination is recorded as recently written, as the lone entry records it.
 *   submit : never blocks; the checks and status codes are those of mi355_colorlut_frames_device with n_frames = 1, in its order
 *           (format; MI355_ERR_NOT_CONFIGURED without a LUT; negative sizes; null data with a pixel; a stride below the row bytes; a
 *           null ctx or a null ticket: MI355_ERR_INVALID_ARG). One refusal is the queue's own: the element never works in place
 *           (the note at mi355_colorlut_frames_device speaks of two different frames), so a frame whose own source and destination
 *           byte ranges [p, p + (height - 1) * stride + width * bytes per pixel) meet is MI355_ERR_INVALID_ARG. A refused submit
 *           queues nothing. A frame with width == 0 or height == 0 is accepted, gets a ticket and touches nothing. The frame is
 *           processed after what ctx's HIP stream held at the call.
 *   borrowing : between the submit and the return of wait_colorlut for its ticket the frame's bytes AND the context's LUT are
 *           borrowed: no mi355_colorlut_load, no mi355_colorlut_unload and no mi355_ctx_destroy of `ctx` in between (the rule of
 *           mi355_group_submit_chain). Only the LUT's cells, kind, size and domain are read: the member's MI355_FLAG_FORCE_GENERIC
 *           is read at submit and sends its frame to the literal launch; MI355_FLAG_LUT_VARIANT, the compute / table choice, the
 *           memoised tables, the brick and window kernels and the content watch play no part, and the queue never builds, reads
 *           or measures a table.
 *   order  : a submit whose destination range meets the source or the destination range of a frame still pending, or whose source
 *           range meets a pending destination, first launches what is pending, then queues (ranges only: conservative - two
 *           sub-pictures side by side in one padded picture count as meeting); sets run in order on the queue's one stream, so the
 *           bytes are those of the lone calls in submission order. Frames that only share a SOURCE share a set.
 *   wait   : launches what is pending if the frame has not gone out (rendezvous first), then waits for its launch set; the
 *           group's lock is not held meanwhile. A result is collected once. Tickets are one sequence per group: a ticket that is
 *           unknown, already collected or another queue's is MI355_ERR_INVALID_ARG here and stays collectable where it belongs;
 *           mi355_group_wait, _order_after and the other queues' waits refuse a colorlut ticket likewise.
 *   set_colorlut_rendezvous : as set_hsvdetect_rendezvous, counted over pending colorlut frames only.
 *   At most MI355_COLORLUT_SET_MAX frames share a launch set; more go out as consecutive sets. flush, wait_all and destroy cover
 *   this queue as they cover the others. A launch that fails is reported, once, to each frame's own wait.
 *   The two launches: the vector launch (four pixels per lane, one 16-byte load and store; each block tables, for ITS job's domain
 *   and size, the cell index and weight of the 256 byte values per axis in 6 KiB of LDS with the reference's own operations, and
 *   gathers the eight cells of a pixel from the LUT in global memory) carries the MI355_FMT_RGBA frames of members without
 *   FORCE_GENERIC whose geometry is flat - both sides packed, both bases and the byte count multiples of 16 - or rowpad - both bases
 *   and both strides multiples of 16 (units: ceil(width / 4) groups per row). The literal launch (one pixel per lane, the arithmetic
 *   of the lone FORCE_GENERIC route) carries every other frame: both RGBA64 orders, RGBA frames off the 16-byte grid, FORCE_GENERIC.
 *   When it pays (measured, DESIGN 4.7.2: 32 members with 32 LUTs of 33^3, one thread, against 32 lone calls and their
 *   synchronisations): the queue removes launches and synchronisations, not device work, and its vector kernel gathers eight cells
 *   per pixel where the lone route reads a memoised table or LDS-cached bricks. It gains at 640x640 RGBA (3.3 x), at 1080p RGBA
 *   (1.19 x; nothing separable when all members hold one LUT) and at 1080p RGBA64 (1.47 x); at 4K RGBA it LOSES (0.56 x: 1.56 ms
 *   against 0.87 ms per interval). Leave 4K RGBA members on the lone entry.
 *   colorlut_stats : {frames launched, launch sets, frames in the largest set, kernel launches} - per set 0 launches when no frame
 *           has a pixel, 1 when all frames are of one class, 2 when both classes occur.
 *   mi355_selftest_colorlut_set_plan : host only, no device: what the builder the queue launches from makes of n_frames frames in
 *           submission order (no LUT is needed: the plan does not depend on it). The addresses are numbers and are never
 *           dereferenced. Per frame: `set`, counted from 0 - a new set begins at MI355_COLORLUT_SET_MAX frames and in front of a
 *           frame that meets one of the current set (the rule of `order`); `launch`, 0 no pixel, 1 vector, 2 literal; `geometry`,
 *           vector: 1 flat, 2 rowpad, else 0; `units`, vector: groups of four pixels, literal: pixels; `first_block` and `blocks`,
 *           its share of its launch's grid by mi355_selftest_hsvdetect_plan's rule (vector: 512 units per block, 16 blocks per CU;
 *           literal: 256 and 8). *n_sets: the sets. Refused (MI355_ERR_INVALID_ARG): n_cu < 1, n_frames < 0, null arrays with
 *           n_frames > 0, a null n_sets, and a frame submit would refuse (format, negative sizes, a null address with a pixel,
 *           strides below the row bytes, own source and destination meeting). */
#define MI355_COLORLUT_SET_MAX 32 /* frames per launch set */
typedef struct mi355_colorlut_plan_frame {
  uint64_t src_address, dst_address; /* the first bytes of source and destination, as numbers */
  int32_t src_stride, dst_stride, width, height, format;
  int32_t force_generic;             /* the member's MI355_FLAG_FORCE_GENERIC */
} mi355_colorlut_plan_frame;
typedef struct mi355_colorlut_plan_out {
  int32_t set, launch, geometry;
  uint32_t first_block, blocks, reserved;
  uint64_t units;
} mi355_colorlut_plan_out;
int mi355_group_set_colorlut_rendezvous(mi355_group *group, int expected_streams, unsigned linger_us);
int mi355_group_submit_colorlut(mi355_group *group, mi355_ctx *ctx, const uint8_t *d_src, int src_stride, uint8_t *d_dst,
                                int dst_stride, int width, int height, int format, uint64_t *ticket);
int mi355_group_wait_colorlut(mi355_group *group, uint64_t ticket);
/* {frames launched, launch sets, frames in the largest set, kernel launches} */
int mi355_group_colorlut_stats(mi355_group *group, uint64_t stats[4]);
/* host only, no device: the sets, launches and blocks of n_frames frames */
int mi355_selftest_colorlut_set_plan(int n_cu, const mi355_colorlut_plan_frame *frames, int n_frames,
                                     mi355_colorlut_plan_out *out, int *n_sets);

/* ---------------------------------------------------------------- many AUDIO element instances, few launches (csrc/agroup.hip)
 * rsaudioecho (audio/audiofx/src/audioecho/imp.rs:205-227), ebur128level (audio/audiofx/src/ebur128level/imp.rs:682-745) and
 * audioloudnorm (audio/audiofx/src/audioloudnorm/imp.rs:1545-1586) are one instance per stream and one buffer per call; the batch
 * entry points above need ONE caller that owns all streams. An agroup is that caller for a process full of independent
 * instances of one kind and configuration: `n_members` of them, each submitting its buffer of the interval from its own
 * streaming thread and waiting for its ticket; the batch runs - one launch set for all - when every attached member has
 * submitted (on the thread that completes the set). Per-member results are those of a single-instance context fed the same
 * buffers, bit for bit.
 *   create_echo     : members are fully independent (own ring of ring_len f64 and position; per submit its own buffer length,
 *                     sample type, delay, intensity, feedback). A waiter lingers linger_us for the missing members, then launches
 *                     whoever is there (linger 0 = at once).
 *   create_ebur128  : members are independent meters of one configuration: per submit its own buffer length, each with its own
 *                     100 ms phase, and ebur128_reset (the element's `reset` action, ebur128level/imp.rs:124-139) for one member
 *                     alone; one sample format per launch set. Linger as for create_echo: a member that is late, paused or
 *                     detached simply does not advance.
 *   create_loudnorm : members are independent too: each stands at its own frame type (its first 3 s frame, 100 ms frames, the final
 *                     rest) and hands over whole frames of mi355_agroup_loudnorm_frame_size(group, member), or the shorter rest with
 *                     final_frame = 1 - what drain_full_frames / drain hand to State::process. A launch set runs one launch
 *                     sequence per class of members that stand at the same frame type and size (streams that started together);
 *                     linger as for create_echo. (timeout_ms of set_linger is accepted and ignored; MI355_ERR_TIMEOUT is not
 *                     returned any more: nobody waits for a member that does not come.)
 *   submit_*        : device_data = 0: host buffers (copied through one pinned slab: one upload and one download per interval
 *                     for all members); 1: device pointers. Buffers are borrowed until wait(ticket) returns.
 *   wait            : *out_frames (optional) = frames produced (audioloudnorm), samples processed (echo), frames metered.
 *   ebur128_loudness / _peak : the member's meter readings (what: 0 momentary, 1 short-term, 2 global, 3 relative threshold,
 *                     4 loudness range), computed once per interval for all members.
 *   stats           : {buffers, launch sets, buffers in the largest set}.
 * A member's life cycle: a member has at most ONE buffer outstanding, from its submit_* until wait(ticket) has returned. Until then
 * another submit_* of that member and its setup / reset / load calls (agingradio_setup, ebur128_reset, hrtf_setup, hrtf_reset,
 * hrtf_load_sphere, sofa_setup, sofa_set_filter, sofa_set_drop, sofa_reset, mixer_setup, mixer_setup_minus1) are refused with MI355_ERR_INVALID_ARG - whether its launch set has run or not - and change nothing. A ticket is
 * collected once: wait takes only the member's outstanding ticket; a second wait for it, ticket 0, a ticket of a coming interval or
 * one the member was never given are refused with MI355_ERR_INVALID_ARG, run no launch set and write to no buffer. detach drops a
 * buffer whose launch set has not run (its wait answers "detached"); a result that has run can still be collected, once.
 * Threads: every entry point from any thread; one lock per group, held while a launch set runs. */
typedef struct mi355_agroup mi355_agroup;
mi355_agroup *mi355_agroup_create_echo(int device, int n_members, size_t ring_len, int *status);
mi355_agroup *mi355_agroup_create_ebur128(int device, int n_members, unsigned channels, unsigned rate, unsigned mode, const int *channel_class,
                                          int *status);
mi355_agroup *mi355_agroup_create_loudnorm(int device, int n_members, unsigned channels, double loudness_target, double loudness_range_target,
                                           double max_true_peak, double offset, int *status);
void mi355_agroup_destroy(mi355_agroup *group);
const char *mi355_agroup_last_error(mi355_agroup *group);
int mi355_agroup_set_linger(mi355_agroup *group, unsigned linger_us, unsigned timeout_ms);
int mi355_agroup_detach(mi355_agroup *group, int member);
int mi355_agroup_submit_echo(mi355_agroup *group, int member, void *data, size_t n, int is_f64, size_t delay_samples, double intensity,
                             double feedback, int device_data, uint64_t *ticket);
int mi355_agroup_submit_ebur128(mi355_agroup *group, int member, const void *data, size_t frames, int sample_format, int device_data,
                                uint64_t *ticket);
int mi355_agroup_ebur128_reset(mi355_agroup *group, int member);
int mi355_agroup_submit_loudnorm(mi355_agroup *group, int member, const double *data, size_t frames, double *out, size_t out_capacity_frames,
                                 int final_frame, int device_data, uint64_t *ticket);
size_t mi355_agroup_loudnorm_frame_size(mi355_agroup *group, int member);
/* audioloudnorm's sink_chain / drain for a member with the adapter on this side (what mi355_loudnorm_push / _drain are for a single
 * context; audioloudnorm/imp.rs:1545-1586, :226-310): push appends the buffer and hands every whole frame over together with
 * the other members (it blocks like wait); drain hands over the rest as the final frame. Host buffers. */
int mi355_agroup_loudnorm_push(mi355_agroup *group, int member, const double *data, size_t frames, double *out, size_t out_capacity_frames,
                               size_t *out_frames);
int mi355_agroup_loudnorm_drain(mi355_agroup *group, int member, double *out, size_t out_capacity_frames, size_t *out_frames, int *eos);
int mi355_agroup_wait(mi355_agroup *group, uint64_t ticket, size_t *out_frames);
int mi355_agroup_ebur128_loudness(mi355_agroup *group, int member, int what, double *out);
int mi355_agroup_ebur128_peak(mi355_agroup *group, int member, int true_peak, unsigned channel, double *out);
int mi355_agroup_echo_get_state(mi355_agroup *group, int member, double *ring_out, size_t ring_len, size_t *pos_out);
int mi355_agroup_stats(mi355_agroup *group, uint64_t stats[3]);
/* Process-wide groups. Elements of independent pipelines cannot hand a group to each other; what they share is the process
 * (gst/gstrsaudioecho.c, gstebur128level.c, gstaudioloudnorm.c, gstvideocompare.c, gstcolordetect.c, gsthsvdetector.c with MI355_GROUP_MEMBERS=n in the environment).
 *   mi355_agroup_shared_* : THE group of this configuration (kind, device, member count, parameters), created at first use, and
 *           the next free member index in *member; a group whose members have all been handed out is not offered again.
 *   mi355_agroup_release  : detach; the last member out destroys the group.
 *   mi355_group_shared / _release : THE dispatcher of `device` (mi355_group_create(device, 0)), reference-counted. */
mi355_agroup *mi355_agroup_shared_echo(int device, int n_members, size_t ring_len, int *member, int *status);
mi355_agroup *mi355_agroup_shared_ebur128(int device, int n_members, unsigned channels, unsigned rate, unsigned mode, const int *channel_class,
                                          int *member, int *status);
mi355_agroup *mi355_agroup_shared_loudnorm(int device, int n_members, unsigned channels, double loudness_target, double loudness_range_target,
                                           double max_true_peak, double offset, int *member, int *status);
void mi355_agroup_release(mi355_agroup *group, int member);
mi355_group *mi355_group_shared(int device, int *status);
void mi355_group_release(mi355_group *group);

/* ---------------------------------------------------------------- hsvfilter ! colorlut, fused
 * The chain `hsvfilter ! colorlut` on RGBA (the only format both elements accept, hsvfilter/imp.rs:252-266 and
 * colorlut/imp.rs:125-137) as ONE pass: every pixel goes through hsv_filter's body (hsvfilter/imp.rs:96-118) and
 * then transform_rgba's body (colorlut/imp.rs:226-294) in registers. Output is bit-identical to
 * mi355_hsvfilter_frames_device followed by mi355_colorlut_frames_device; src is left untouched (src == dst
 * allowed). Needs a loaded LUT; 1D LUTs and non-contiguous frames run as the two element kernels. */
int mi355_hsv_colorlut_frames_device(mi355_ctx *ctx, const uint8_t *d_src, size_t src_pitch,
                                     int src_stride, uint8_t *d_dst, size_t dst_pitch, int dst_stride,
                                     int n_frames, int width, int height,
                                     const mi355_hsv_settings *settings);

/* ---------------------------------------------------------------- rsaudioecho
 * mi355_echo_setup replaces AudioEcho::setup's RingBuffer::new(buffer_size)
 * (audio/audiofx/src/audioecho/imp.rs:248-259, ring_buffer.rs:15-24): ring of `ring_len` f64
 * zeros, position 0. mi355_echo_reset = stop() dropping the state (imp.rs:229-234). */
int mi355_echo_setup(mi355_ctx *ctx, size_t ring_len);
int mi355_echo_reset(mi355_ctx *ctx);
/* Replaces AudioEcho::process::<f32|f64> (imp.rs:69-85) + RingBufferIter (ring_buffer.rs:37-82).
 * `delay_samples` = delay_frames of imp.rs:74-77 (interleaved samples, after the max-delay
 * clamp of imp.rs:207). In place on `n` interleaved samples in host memory. */
int mi355_echo_process_f32(mi355_ctx *ctx, float *data, size_t n, size_t delay_samples,
                           double intensity, double feedback);
int mi355_echo_process_f64(mi355_ctx *ctx, double *data, size_t n, size_t delay_samples,
                           double intensity, double feedback);
int mi355_echo_process_device(mi355_ctx *ctx, void *d_data, size_t n, int is_f64,
                              size_t delay_samples, double intensity, double feedback);
/* Test/diagnostic access to the element state (ring contents + write position). */
int mi355_echo_get_state(mi355_ctx *ctx, double *ring_out, size_t ring_len, size_t *pos_out);
/* Batches: `n_streams` independent AudioEcho instances (own ring, own delay / intensity / feedback - the per-call arrays
 * have n_streams entries) advanced together by `n` interleaved samples per call, three launches for the whole batch
 * instead of three per stream (one rsaudioecho buffer is a few thousand samples: a single stream is launch-bound).
 * Stream s processes d_data + s * stream_stride elements (f32 or f64), in place, device memory. The single-stream
 * entry points above are the n_streams == 1 case of the same kernels. */
int mi355_echo_setup_batch(mi355_ctx *ctx, int n_streams, size_t ring_len);
int mi355_echo_process_batch_device(mi355_ctx *ctx, void *d_data, size_t stream_stride, size_t n, int is_f64,
                                    const size_t *delay_samples, const double *intensity, const double *feedback);
int mi355_echo_get_state_batch(mi355_ctx *ctx, int stream, double *ring_out, size_t ring_len, size_t *pos_out);

/* ---------------------------------------------------------------- ebur128 (loudness meter)
 * Replaces the `ebur128::EbuR128` object (third-party crate ebur128 0.1.10, Cargo.lock:3685-3686) that
 * `ebur128level` feeds and queries: EbuR128::new(channels, rate, mode) + set_channel_map
 * (audio/audiofx/src/ebur128level/imp.rs:518-595), reset() (:329), add_frames_{i16,i32,f32,f64}[_planar]
 * (:690-739), loudness_momentary / loudness_shortterm / loudness_global / relative_threshold /
 * loudness_range / sample_peak / true_peak (:378-452). The crate's source is not vendored: this is the
 * published BS.1770-4 / EBU R128 algorithm in libebur128's formulation (histogram mode, as the element
 * always requests, imp.rs:55-56); parity with the crate is unpinned.
 *   mode: bit 0 momentary, 1 short-term, 2 global (integrated + relative threshold), 3 loudness range,
 *         4 sample peak, 5 true peak  (== GstEbuR128LevelMode, imp.rs:34-51).
 *   channel_class[c]: 0 unused (LFE / unknown position), 1 weight 1.0 (L, R, C, ...), 2 weight 1.41
 *         (surround: +-110/+-90/+-60 degrees), 3 dual mono (weight 2.0); NULL = libebur128's default map.
 *   sample_format: 0 S16, 1 S32, 2 F32, 3 F64 (native endian), interleaved or planar.
 * Loudness values are LUFS / LU as f64; "no signal above the gate" is -inf (global) / -70 (threshold). */
typedef enum mi355_ebur128_mode {
  MI355_EBUR128_MOMENTARY = 1, MI355_EBUR128_SHORT_TERM = 2, MI355_EBUR128_GLOBAL = 4,
  MI355_EBUR128_LOUDNESS_RANGE = 8, MI355_EBUR128_SAMPLE_PEAK = 16, MI355_EBUR128_TRUE_PEAK = 32
} mi355_ebur128_mode;
int mi355_ebur128_setup(mi355_ctx *ctx, unsigned channels, unsigned rate, unsigned mode, const int *channel_class);
/* Batch form: `n_streams` independent meters of ONE configuration fed in lock step, every kernel launched once for all of
 * them (grid y = stream). One stream's K-weighting recurrence is serial; hundreds of streams are what fills the GPU
 * (ebur128level is one instance per stream in the reference: ebur128level/imp.rs:682-745 runs per element; a transcoding
 * farm runs hundreds of them). `data` of add_frames_batch: n_streams buffers of frames x channels interleaved samples,
 * back to back (host pointer; _device: device pointer, asynchronous up to the read-back of the gating energies).
 * loudness_batch: what = 0 momentary, 1 short-term, 2 global, 3 relative threshold, 4 loudness range -> out[n_streams];
 * peak_batch -> out[n_streams][channels]. mi355_ebur128_reset / _teardown apply to the batch as a whole. Per-stream results
 * are identical to n_streams separate single-stream meters (tests/test_gpu_ebur128.py). Meters that are fed independently - other
 * buffer sizes, late or paused members, a reset of one of them - are members of an audio group (mi355_agroup_create_ebur128 above):
 * the engine underneath keeps a 100 ms phase per stream. */
int mi355_ebur128_setup_batch(mi355_ctx *ctx, unsigned n_streams, unsigned channels, unsigned rate, unsigned mode, const int *channel_class);
int mi355_ebur128_add_frames_batch(mi355_ctx *ctx, const void *data, size_t frames, int sample_format);
int mi355_ebur128_add_frames_batch_device(mi355_ctx *ctx, const void *d_data, size_t frames, int sample_format);
int mi355_ebur128_loudness_batch(mi355_ctx *ctx, int what, double *out);
int mi355_ebur128_peak_batch(mi355_ctx *ctx, int true_peak, double *out);
int mi355_ebur128_reset(mi355_ctx *ctx);
int mi355_ebur128_teardown(mi355_ctx *ctx);
int mi355_ebur128_add_frames(mi355_ctx *ctx, const void *data, size_t frames, int sample_format);
int mi355_ebur128_add_frames_planar(mi355_ctx *ctx, const void *const *planes, size_t frames, int sample_format);
int mi355_ebur128_loudness_momentary(mi355_ctx *ctx, double *out);
int mi355_ebur128_loudness_shortterm(mi355_ctx *ctx, double *out);
int mi355_ebur128_loudness_global(mi355_ctx *ctx, double *out);
int mi355_ebur128_relative_threshold(mi355_ctx *ctx, double *out);
int mi355_ebur128_loudness_range(mi355_ctx *ctx, double *out);
int mi355_ebur128_sample_peak(mi355_ctx *ctx, unsigned channel, double *out);
int mi355_ebur128_true_peak(mi355_ctx *ctx, unsigned channel, double *out);

/* ---------------------------------------------------------------- audioloudnorm
 * Replaces audioloudnorm's State (audio/audiofx/src/audioloudnorm/imp.rs:83-127) and its methods: State::new (:130-205),
 * drain_full_frames / drain (:226-310), process and the frame handlers (:312-828), the true-peak limiter (:845-1430),
 * detect_peak (:1438-1524), gaussian_filter (:1526-1541). Audio is interleaved f64 at 192 kHz, the only caps the
 * element accepts (:1848-1851); the element keeps its pads, timestamps and events.
 *   setup : State::new(settings, info) with the four properties (loudness-target [LUFS], loudness-range-target [LU],
 *           max-true-peak [dbTP], offset [LU]; imp.rs:37-40).
 *   push  : sink_chain -> adapter.push + drain_full_frames: every complete frame (3 s first, then 100 ms) is processed;
 *           `out` receives *out_frames frames (0 while the first 3 s are still being collected). A frame that does not
 *           fit the rest of `out` is refused ("output buffer too small") before it changes anything - no meter has seen
 *           it -: it and what was pushed after it stay in the adapter, the frames delivered before it in the same call
 *           have left it and are counted in *out_frames. push again (0 frames will do) with room for the rest.
 *   drain : drain() at EOS / flush: the final frame (up to 3 s of latency comes out) or, with less than 3 s in total,
 *           the linear-gain path; *eos = 1 when there was nothing at all to drain (FlowError::Eos, :289-293).
 *           out_capacity_frames >= 30*19200 + pending frames covers every case. */
int mi355_loudnorm_setup(mi355_ctx *ctx, unsigned channels, double loudness_target,
                         double loudness_range_target, double max_true_peak, double offset);
int mi355_loudnorm_push(mi355_ctx *ctx, const double *data, size_t frames, double *out,
                        size_t out_capacity_frames, size_t *out_frames);
int mi355_loudnorm_drain(mi355_ctx *ctx, double *out, size_t out_capacity_frames, size_t *out_frames,
                         int *eos);
int mi355_loudnorm_teardown(mi355_ctx *ctx);
/* Batches (round 3): n_streams elements of one configuration in LOCK STEP - State::process (imp.rs:800-828) for all of them
 * per call, with the true-peak limiter's state machine (:845-1430) running on the device, one block per stream. The element
 * keeps its adapter: `process_batch` is called the way drain_full_frames (:226-268) calls State::process, with exactly
 * mi355_loudnorm_batch_frame_size() frames per stream (576,000 for the first call, then 19,200) - or, with final_frame = 1,
 * with the shorter rest at drain() (:270-310; 0 frames allowed). Stream s reads data + s * stream_stride and writes
 * out + s * out_stream_stride (interleaved f64, elements); every stream produces *out_frames frames. device_data = 1: both
 * are device pointers (no sample crosses PCIe); the call still waits for the device wherever State::process reads a meter
 * (the short-term / global loudness of every frame decides the gain on the host, as in the reference). The output capacity
 * is checked before anything changes: after "output buffer too small" the same call can be repeated with a larger buffer.
 * Per-stream samples are identical to n separate mi355_loudnorm_* contexts. mi355_loudnorm_teardown releases a batch as well. */
int mi355_loudnorm_setup_batch(mi355_ctx *ctx, unsigned n_streams, unsigned channels, double loudness_target,
                               double loudness_range_target, double max_true_peak, double offset);
size_t mi355_loudnorm_batch_frame_size(mi355_ctx *ctx);
int mi355_loudnorm_process_batch(mi355_ctx *ctx, const double *data, size_t stream_stride, size_t frames,
                                 double *out, size_t out_stream_stride, size_t out_capacity_frames,
                                 size_t *out_frames, int final_frame, int device_data);

/* ---------------------------------------------------------------- videocompare
 * Replaces HasherEngine::hash_image / compare (video/videofx/src/videocompare/hashed_image.rs:24-79) for
 * HashAlgorithm::Blockhash, the element default (videocompare/imp.rs:31): image_hasher 3.1.1 blockhash, 8x8 bits, on
 * the packed RGB / RGBA frame (rows addressed by `stride`, which covers tightly_packed_framebuffer :110-130).
 * `algo` takes GstVideoCompareHashAlgorithm values (videocompare/mod.rs:60-100). Blockhash on frame sizes that are not
 * divisible by 8 is MI355_ERR_UNSUPPORTED unless MI355_FLAG_BLOCKHASH_ANY_SIZE is set (the crate's floating-point path,
 * hashed_image.rs:37-44 -> image_hasher blockhash_slow); its hash is the 64 block bits, bit i = block i row-major. Mean / Gradient /
 * VertGradient / DoubleGradient (grayscale + Lanczos3 resize of the `image` crate + bit rule) give 64/64/64/40 bits in the
 * crate's iteration order. Dssim has no hash: see mi355_dssim_* below. */
typedef enum mi355_hash_algo {
  MI355_HASH_MEAN = 0, MI355_HASH_GRADIENT = 1, MI355_HASH_VERTGRADIENT = 2, MI355_HASH_DOUBLEGRADIENT = 3,
  MI355_HASH_BLOCKHASH = 4, MI355_HASH_DSSIM = 5
} mi355_hash_algo;
int mi355_videocompare_hash_frame(mi355_ctx *ctx, const uint8_t *data, int stride, int width, int height,
                                  int format, int algo, uint64_t *hash);
/* `n_frames` device-resident frames (frame f at d_frames + f*frame_pitch); `hashes` is a host array. Synchronous. */
int mi355_videocompare_hash_frames_device(mi355_ctx *ctx, const uint8_t *d_frames, size_t frame_pitch,
                                          int stride, int n_frames, int width, int height, int format,
                                          int algo, uint64_t *hashes);
/* ImageHash::dist as f64 (hashed_image.rs:64): Hamming distance. Negative for an unsupported `algo`. */
double mi355_videocompare_distance(int algo, uint64_t reference_hash, uint64_t frame_hash);
/* HashAlgorithm::Dssim (cargo feature `dssim`; hashed_image.rs:41-53,66-70): crate dssim-core 3.4.0.
 *   mi355_dssim_create_image  = Dssim::create_image_rgb / create_image_rgba on the packed frame (host pointer; the
 *                               _device variant takes a device-resident frame). The DssimImage<f32> stays on the device.
 *   mi355_dssim_compare       = Dssim::compare(original, modified).0 as f64 (0.0 for identical images).
 * format: MI355_FMT_RGB or MI355_FMT_RGBA. Translucent RGBA pixels (alpha < 255) are composed over dssim's coloured,
 * position-dependent background pattern (hashed_image.rs:54-55 -> create_image_rgba; written from memory of the crate:
 * parity unpinned like the rest of the engine; round 2 refused such frames); MI355_FLAG_DSSIM_TRANSLUCENT = 1 composes
 * them over black instead. create / free do not wait for the kernels (the host variant of create returns once `data` has
 * been uploaded and may be reused); mi355_dssim_compare does (it returns the value). An
 * image is created, compared and freed through ONE context. */
typedef struct mi355_dssim_image mi355_dssim_image;
int mi355_dssim_create_image(mi355_ctx *ctx, const uint8_t *data, int stride, int width, int height,
                             int format, mi355_dssim_image **out);
int mi355_dssim_create_image_device(mi355_ctx *ctx, const uint8_t *d_frame, int stride, int width,
                                    int height, int format, mi355_dssim_image **out);
void mi355_dssim_free_image(mi355_ctx *ctx, mi355_dssim_image *image);
int mi355_dssim_compare(mi355_ctx *ctx, const mi355_dssim_image *original,
                        const mi355_dssim_image *modified, double *dssim);
/* videocompare's loop over the non-reference pads of one aggregate (videocompare/imp.rs:316-345: each pad's frame goes
 * through HashedImage::new and HashedImage::compare against the reference pad's image, and its hash is dropped):
 * `n_frames` (<= 64) frames of the original's size are hashed AND compared against `original` in one pass per scale - their
 * DssimImages never reach memory - and dssim[i] receives what mi355_dssim_create_image + mi355_dssim_compare(original, .)
 * return for frames[i], bit for bit. One synchronisation per call. `frames` is a host array of host pointers (of device
 * pointers for the _device variant). */
int mi355_dssim_compare_frames(mi355_ctx *ctx, const mi355_dssim_image *original, const uint8_t *const *frames,
                               int n_frames, int stride, int width, int height, int format, double *dssim);
int mi355_dssim_compare_frames_device(mi355_ctx *ctx, const mi355_dssim_image *original,
                                      const uint8_t *const *d_frames, int n_frames, int stride, int width,
                                      int height, int format, double *dssim);
/* HashedImage::new + HashedImage::compare for n independent two-pad comparisons (hashed_image.rs:48-79: Dssim::create_image_rgb /
 * create_image_rgba on both frames, Dssim::compare): dssim[i] = the value of (refs[i], frames[i]), `n_pairs` <= 64 pairs of one
 * geometry, format MI355_FMT_RGB or MI355_FMT_RGBA, one synchronisation per call. `refs` / `frames` are host arrays of host
 * pointers (of device pointers for the _device variant). MI355_FLAG_DSSIM_FAST = 0: every pair is mi355_dssim_create_image(refs[i])
 * + mi355_dssim_compare_frames(frames[i]), bit for bit; 1: the fast form (see the flag). Nothing of a pair is kept. */
int mi355_dssim_compare_pairs(mi355_ctx *ctx, const uint8_t *const *refs, const uint8_t *const *frames, int n_pairs,
                              int stride, int width, int height, int format, double *dssim);
int mi355_dssim_compare_pairs_device(mi355_ctx *ctx, const uint8_t *const *d_refs, const uint8_t *const *d_frames,
                                     int n_pairs, int stride, int width, int height, int format, double *dssim);
/* Diagnostics (hashed_image.rs:48-79, the per-pixel SSIM map inside Dssim::compare): the f32 SSIM map of scale `scale` of ONE
 * pair of device-resident frames, in the form MI355_FLAG_DSSIM_FAST selects, copied to `out` (host; may be NULL to query the
 * scale's size only, as for mi355_dssim_image_plane). */
int mi355_dssim_pair_map_device(mi355_ctx *ctx, const uint8_t *d_ref, const uint8_t *d_frame, int stride, int width,
                                int height, int format, int scale, float *out, int *map_width, int *map_height);
/* Device self test of the LAB conversion's cube root: for every f32 whose bit pattern lies in [lo_bits, hi_bits], the
 * Halley iteration with the range-restricted division the kernels use against the same iteration with the compiler's IEEE
 * division; *mismatches = how many differ in any bit (0 over (216/24389, 2], the whole domain of the conversion). */
int mi355_selftest_dssim_cbrt(mi355_ctx *ctx, uint32_t lo_bits, uint32_t hi_bits, uint64_t *mismatches);
/* Test-only entries of the exact engine (tests/dssim_cases.py holds the model they are compared with).
 *   mi355_selftest_dssim_plan : host only, no device: what the engine's host code and kernels make of a width x height frame on a
 *           device of n_cu compute units, from the functions and constants the launches themselves use. tile_w x tile_h: the tile of
 *           the three tile kernels (tile_lanes lanes per block); scale_halo / compare_halo: the halo of the scale and hash-compare
 *           kernels / of the compare kernel. Scale k is w[k] x h[k] (halved while both sides are >= 8, at most 5 scales) in tiles[k]
 *           tiles, of which interior_scale[k] / interior_compare[k] take the kernels' INTERIOR path (the tile plus its halo lies
 *           inside the scale). Launch l of create_image / compare_frames serves launch_jobs[l] scales from launch_scale[l] on, job j
 *           in blocks [launch_first[l][j], launch_first[l][j + 1]). downsample_blocks[k] (k >= 1) and absdev_blocks[k]: the grids of
 *           the box chain and of the absolute-deviation reduction (capped at 8 n_cu); avg_blocks / sum_blocks: one block per scale.
 *           MI355_ERR_INVALID_ARG for a null plan, width / height <= 0 or n_cu <= 0.
 *   mi355_selftest_dssim_compare_detail : mi355_dssim_compare (same launches, same value in *dssim) that also copies out the f32
 *           SSIM map of scale `scale` (map, w[scale] * h[scale] floats; may be NULL) and that scale's three f64 reduction slots
 *           [sum of the map, avg = max(sum / len, 0) ^ (0.5 ^ scale), sum of |avg - map|] (slots; may be NULL). */
typedef struct mi355_dssim_plan {
  int32_t tile_w, tile_h, tile_lanes, scale_halo, compare_halo;
  int32_t n_scales;
  int32_t w[5], h[5];
  uint32_t tiles[5], interior_scale[5], interior_compare[5];
  int32_t n_launches;
  int32_t launch_scale[3], launch_jobs[3];
  uint32_t launch_first[3][4];
  uint32_t downsample_blocks[5], absdev_blocks[5];
  uint32_t avg_blocks, sum_blocks;
} mi355_dssim_plan;
int mi355_selftest_dssim_plan(int width, int height, int n_cu, mi355_dssim_plan *plan);
int mi355_selftest_dssim_compare_detail(mi355_ctx *ctx, const mi355_dssim_image *original, const mi355_dssim_image *modified,
                                        int scale, float *map, double *slots, double *dssim);
/* Diagnostics: one f32 plane of the image (kind 0 = LAB plane, 1 = mu, 2 = img_sq_blur) copied to `out` (may be NULL
 * to query the scale's size only). */
int mi355_dssim_image_plane(mi355_ctx *ctx, const mi355_dssim_image *image, int scale, int channel, int kind,
                            float *out, int *width, int *height);

/* ---------------------------------------------------------------- hrtfrender
 * Replaces the per-block body of HrtfRender::process (audio/hrtf/src/hrtf/imp.rs:164-278) including the calls
 * into the `hrtf` crate (HrirSphere::new, HrtfProcessor::new, process_samples).
 *   mi355_hrtf_load_sphere : Settings::sphere(rate) -> HrirSphere::new(bytes, rate) (imp.rs:84-94). `bytes` is the
 *       crate's file format ("HRIR", u32 rate, u32 len, u32 n_vertices, u32 n_indices, indices, vertices). A sphere
 *       whose rate differs from `device_rate` is converted at load time, every HRIR by band-limited (windowed-sinc)
 *       interpolation to round(len * device_rate / file_rate) taps - the crate does this with the `rubato` resampler, whose
 *       sources are not in the reference tree: same method, parity unpinned (csrc/hrtf_kernels.hip: resample_hrir).
 *   mi355_hrtf_setup       : the ChannelProcessor vector of set_caps (imp.rs:662-680): one HrtfProcessor per input
 *       channel, zeroed tails, no previous vector/gain.
 *   mi355_hrtf_reset       : State::reset_processors (imp.rs:124-129).
 *   mi355_hrtf_process_block : one block of block_length*interpolation_steps frames (imp.rs:196-271): `in` is
 *       interleaved f32 [frames][channels], `out` interleaved stereo f32 [frames][2], overwritten.
 *       positions[c] = Settings::position(c) (already `.to_right_handed()`, imp.rs:64-73), gains[c] =
 *       Settings::distance_gain(c). The adapter / drain logic around it (imp.rs:281-420) stays in the element. */
int mi355_hrtf_load_sphere(mi355_ctx *ctx, const void *bytes, size_t len, uint32_t device_rate);
int mi355_hrtf_setup(mi355_ctx *ctx, int channels, int block_length, int interpolation_steps);
int mi355_hrtf_reset(mi355_ctx *ctx);
int mi355_hrtf_teardown(mi355_ctx *ctx);
int mi355_hrtf_process_block(mi355_ctx *ctx, const float *in, float *out, const float *positions_xyz,
                             const float *distance_gains);
/* Same with device-resident input/output (asynchronous on the context stream). */
int mi355_hrtf_process_block_device(mi355_ctx *ctx, const float *d_in, float *d_out,
                                    const float *positions_xyz, const float *distance_gains);
/* Sphere geometry as loaded: HRIR length, vertices, faces. */
int mi355_hrtf_sphere_info(mi355_ctx *ctx, uint32_t *hrir_len, uint32_t *n_vertices, uint32_t *n_faces);
/* Which convolution form mi355_hrtf_setup chose: *fft_n = the overlap-save transform size (the next power of two holding
 * hrir_len - 1 + block_length, served for 512..4096), 0 when the time-domain FIR serves. Read-only. */
int mi355_hrtf_transform_size(mi355_ctx *ctx, int *fft_n);
/* Diagnostics: mesh face (or -1) and barycentric weights chosen per [channel][step] in the last block. */
int mi355_hrtf_last_lookup(mi355_ctx *ctx, int *faces, float *uvw);
/* hrtfrender through an audio group (csrc/agroup.hip; audio/hrtf/src/hrtf/imp.rs): members are fully independent instances, as echo
 * and agingradio members are - own sphere, channel count (1..64), block-length, interpolation-steps, HRIR length and convolution
 * form each - and whoever has submitted a block shares ONE launch set (prepare, at most one convolution launch per transform size
 * present plus one for the time-domain rows, mix), one upload and one download. A member's output is a lone context's, bit for bit.
 *   mi355_agroup_hrtf_load_sphere : Settings::sphere -> HrirSphere::new(bytes, rate) of one member (imp.rs:84-94). Members that
 *       load identical bytes at the same device rate share ONE device copy (parsed and resampled once, reference-counted).
 *   mi355_agroup_hrtf_setup : set_caps' ChannelProcessor vector of one member (imp.rs:648-707, :662-680). `method` is what
 *       MI355_FLAG_HRTF_METHOD is for a lone context (0 by HRIR length, 1 FFT, 2 FIR). Before a sphere: MI355_ERR_NOT_CONFIGURED;
 *       channels outside 1..64: MI355_ERR_INVALID_ARG (mi355_hrtf_setup answers the same above 64).
 *   mi355_agroup_hrtf_reset : State::reset_processors of one member (imp.rs:124-129): tails cleared, previous vectors and gains
 *       kept; ordered after the member's last launch set.
 *   mi355_agroup_submit_hrtf : one block (HrtfRender::process, imp.rs:164-278): `in` [S*B][C] f32, `out` [S*B][2] f32 (valid after
 *       mi355_agroup_wait, which answers the frames rendered), positions [C][3] (imp.rs:64-73) and gains [C], both copied at submit;
 *       device_data = 1: `in` / `out` are device pointers. Before setup: MI355_ERR_NOT_CONFIGURED.
 *   mi355_agroup_hrtf_info : the member's HRIR length (imp.rs:84-94, after the resampling), the transform size its setup chose
 *       (0: the time-domain FIR; -1 before setup) and the number of distinct spheres the group keeps on the device.
 *   mi355_agroup_hrtf_last_lookup : as mi355_hrtf_last_lookup, for one member (the crate's mesh search behind imp.rs:236-252).
 *   mi355_agroup_hrtf_launches : kernel launches of the group's launch sets so far (imp.rs:164-278 per member and block: three per
 *       set of uniform members instead of three per member). */
mi355_agroup *mi355_agroup_create_hrtf(int device, int n_members, int *status);
mi355_agroup *mi355_agroup_shared_hrtf(int device, int n_members, int *member, int *status);
int mi355_agroup_hrtf_load_sphere(mi355_agroup *group, int member, const void *bytes, size_t len, uint32_t device_rate);
int mi355_agroup_hrtf_setup(mi355_agroup *group, int member, int channels, int block_length, int interpolation_steps, int method);
int mi355_agroup_hrtf_reset(mi355_agroup *group, int member);
int mi355_agroup_submit_hrtf(mi355_agroup *group, int member, const float *in, float *out, const float *positions_xyz,
                             const float *distance_gains, int device_data, uint64_t *ticket);
int mi355_agroup_hrtf_info(mi355_agroup *group, int member, uint32_t *hrir_len, int *fft_n, int *spheres_held);
int mi355_agroup_hrtf_last_lookup(mi355_agroup *group, int member, int *faces, float *uvw);
uint64_t mi355_agroup_hrtf_launches(mi355_agroup *group);

/* ---------------------------------------------------------------- sofalizer
 * Replaces the per-block loop of Sofalizer::process (audio/hrtf/src/sofa/imp.rs:234-300): de-interleave each channel,
 * sofar's Renderer::process_block (uniformly partitioned convolution with `partition-length`, built in set_caps :793-798)
 * and the channel-ordered mix `out[2i] += l * gain, out[2i+1] += r * gain` (:282-297). The element keeps what is not
 * per-sample work: opening the SOFA file and looking up / interpolating the HRIR pair of a position (Sofar::filter in
 * State::update_filters, :129-160) - it hands each pair over with mi355_sofa_set_filter when a source has moved by more
 * than `update-threshold`, exactly where it calls Renderer::set_filter today - plus the adapter and drain logic.
 *   setup       block_length must be a multiple of partition_length (else INVALID_ARG with the reference's message,
 *               :775-781); partition_length a power of two in 8..2048 (UNSUPPORTED otherwise)
 *   set_filter  filter_len taps per ear + whole-sample onset delays (>= 0); effective from the next block
 *   set_drop    ChannelProcessor::Drop for LFE1 / LFE2 (:808-821). The element fixes it per channel when it negotiates and
 *               never toggles it: after the first block the call fails with INVALID_ARG until reset or setup (a channel
 *               returning in mid-run would have no defined history)
 *   reset       flush-stop (:840-848): input history cleared
 *   process_block  in: block_length x channels interleaved f32; out: block_length x 2 interleaved f32
 * The crate's arithmetic is not in the reference tree: parity is that of a streaming linear convolution, within 2e-6 of
 * full scale against the time-domain oracle. */
int mi355_sofa_setup(mi355_ctx *ctx, int channels, int filter_len, int partition_length, int block_length);
int mi355_sofa_set_filter(mi355_ctx *ctx, int channel, const float *left, const float *right, int delay_left, int delay_right);
int mi355_sofa_set_drop(mi355_ctx *ctx, int channel, int drop);
int mi355_sofa_reset(mi355_ctx *ctx);
int mi355_sofa_teardown(mi355_ctx *ctx);
int mi355_sofa_process_block(mi355_ctx *ctx, const float *in, float *out, const float *distance_gains);
int mi355_sofa_process_block_device(mi355_ctx *ctx, const float *d_in, float *d_out, const float *distance_gains);
/* sofalizer through an audio group (csrc/agroup.hip; audio/hrtf/src/sofa/imp.rs): members are fully independent instances, as
 * hrtfrender members are - own channel count (1..64), filter length, partition-length and block-length each - and whoever has
 * submitted shares ONE launch set: the filters set since the member's last buffer transformed (one launch per distinct partition
 * length among them, none if nothing is pending), one convolution launch per distinct partition length among the members with one
 * workgroup per (member, channel) that is not dropped, one mix; one upload and one download. A uniform group takes 2 launches per
 * set, 3 in the interval after a source moved. A member's output is a lone context's, bit for bit.
 *   mi355_agroup_create_sofa / _shared_sofa : a group of n_members sofalizer instances / THE group of the process (as _shared_hrtf).
 *   mi355_agroup_sofa_setup : set_caps of one member (sofa/imp.rs:747-838; Renderer::builder with partition-length, :794-798). The
 *       checks and messages of mi355_sofa_setup: "Block Length is not multiple of Partition Length" (:779-784) is
 *       MI355_ERR_INVALID_ARG, a partition that is not a power of two in 8..2048 MI355_ERR_UNSUPPORTED. The member's device memory
 *       and the group's tables are allocated here, never inside a launch set.
 *   mi355_agroup_sofa_set_filter : Renderer::set_filter of one channel where State::update_filters calls it (:129-160). QUEUED: the
 *       taps are copied at the call (onset delays folded in as mi355_sofa_set_filter folds them), nothing is launched or waited
 *       for; the transform runs with the member's next launch set, so the pair takes effect with its next block. A second call for
 *       the channel before that replaces the first. The pending filters of members that sit a launch set out stay pending.
 *   mi355_agroup_sofa_set_drop : ChannelProcessor::Drop for LFE1 / LFE2 (:812-818; :253-255 skips it). After the member's first block
 *       MI355_ERR_INVALID_ARG until reset or setup, as mi355_sofa_set_drop.
 *   mi355_agroup_sofa_reset : State::reset_processors of one member (:123-127, flush-stop :846-853): input history cleared, filters
 *       kept - transformed and pending alike; ordered after the member's last launch set.
 *   mi355_agroup_submit_sofa : n_blocks (1..8) whole blocks at once - Sofalizer::process takes every whole block its adapter holds
 *       (the `while state.adapter.available() >= inblksz` loop, :235-322): `in` [n_blocks * block_length][C] f32, `out`
 *       [n_blocks * block_length][2] f32 (valid after mi355_agroup_wait, which answers the frames rendered), gains [C] (:307) copied
 *       at submit and applied to all n_blocks; equal to n_blocks mi355_sofa_process_block calls in a row. device_data = 1: `in` /
 *       `out` are device pointers. An undropped channel with no filter, transformed or pending: MI355_ERR_NOT_CONFIGURED.
 *   mi355_agroup_sofa_info : the member's filter partitions K = ceil(filter_len / partition_length), its transform size 2 *
 *       partition_length, and how many of its filters are pending. Before setup: MI355_ERR_NOT_CONFIGURED.
 *   mi355_agroup_sofa_launches : kernel launches of the group's launch sets so far (:235-322 per member and block: two per member
 *       and block for lone contexts). */
mi355_agroup *mi355_agroup_create_sofa(int device, int n_members, int *status);
mi355_agroup *mi355_agroup_shared_sofa(int device, int n_members, int *member, int *status);
int mi355_agroup_sofa_setup(mi355_agroup *group, int member, int channels, int filter_len, int partition_length, int block_length);
int mi355_agroup_sofa_set_filter(mi355_agroup *group, int member, int channel, const float *left, const float *right, int delay_left,
                                 int delay_right);
int mi355_agroup_sofa_set_drop(mi355_agroup *group, int member, int channel, int drop);
int mi355_agroup_sofa_reset(mi355_agroup *group, int member);
int mi355_agroup_submit_sofa(mi355_agroup *group, int member, const float *in, float *out, int n_blocks, const float *distance_gains,
                             int device_data, uint64_t *ticket);
int mi355_agroup_sofa_info(mi355_agroup *group, int member, int *partitions_K, int *fft_n, int *pending_filters);
uint64_t mi355_agroup_sofa_launches(mi355_agroup *group);

/* ---------------------------------------------------------------- pinned memory + asynchronous host-buffer pipeline
 * For the GStreamer shim (precedent video/colorlut/src/d3d12colorlut/imp.rs:385-492 and
 * audio/audiofx/src/audiornnoise/imp.rs:323-348): mi355_host_alloc backs a GstAllocator / buffer pool offered in
 * propose_allocation so that mapped GstBuffer payloads are page-locked; mi355_pipe_* overlaps the upload of frame
 * n+1 and the download of frame n-1 with the kernels of frame n on side streams. The submit functions take the
 * arguments of the synchronous entry point they mirror (mi355_hsvfilter_frame_ip, mi355_colorlut_frame,
 * mi355_hsv_colorlut_frames_device on one frame), return at once with a ticket, and borrow the buffers until
 * mi355_pipe_wait(ticket) (or a later submit that reclaims the slot) returns. Results are identical. */
void *mi355_host_alloc(mi355_ctx *ctx, size_t bytes);
int mi355_host_free(mi355_ctx *ctx, void *ptr);
typedef struct mi355_pipe mi355_pipe;
mi355_pipe *mi355_pipe_create(mi355_ctx *ctx, int depth, size_t max_frame_bytes);
void mi355_pipe_destroy(mi355_pipe *pipe);
int mi355_pipe_submit_hsvfilter(mi355_pipe *pipe, uint8_t *data, size_t data_len, int width, int stride,
                                int format, const mi355_hsv_settings *settings, uint64_t *ticket);
int mi355_pipe_submit_colorlut(mi355_pipe *pipe, const uint8_t *src, int src_stride, uint8_t *dst,
                               int dst_stride, int width, int height, int format, uint64_t *ticket);
int mi355_pipe_submit_hsv_colorlut(mi355_pipe *pipe, const uint8_t *src, int src_stride, uint8_t *dst,
                                   int dst_stride, int width, int height,
                                   const mi355_hsv_settings *settings, uint64_t *ticket);
int mi355_pipe_wait(mi355_pipe *pipe, uint64_t ticket);
int mi355_pipe_wait_all(mi355_pipe *pipe);
/* Many pipelines in one process: with a group (mi355_group_*) set, mi355_pipe_submit_hsv_colorlut hands
 * its frame to the group's dispatcher instead of launching (the frame then shares a launch pair with the other streams'
 * frames) and the download is enqueued behind that batch when the frame is waited for. Same bytes. NULL = back to own launches.
 * The group is not owned. */
struct mi355_group;
int mi355_pipe_set_group(mi355_pipe *pipe, struct mi355_group *group);

/* ---------------------------------------------------------------- measurement helpers
 * Used by bench.py: run `iters` back-to-back launches of one kernel on the context's stream
 * bracketed by hipEvents on THAT stream and return the average milliseconds per launch. */
int mi355_time_hsvfilter_device(mi355_ctx *ctx, uint8_t *d_data, int n_frames, size_t frame_pitch,
                                int width, int height, int stride, int format,
                                const mi355_hsv_settings *settings, int iters, float *ms_per_launch);
int mi355_time_hsv_colorlut_device(mi355_ctx *ctx, const uint8_t *d_src, size_t src_pitch, int src_stride,
                                   uint8_t *d_dst, size_t dst_pitch, int dst_stride, int n_frames, int width,
                                   int height, const mi355_hsv_settings *settings, int iters, float *ms_per_launch);
int mi355_time_colorlut_device(mi355_ctx *ctx, const uint8_t *d_src, size_t src_pitch, int src_stride,
                               uint8_t *d_dst, size_t dst_pitch, int dst_stride, int n_frames,
                               int width, int height, int format, int iters, float *ms_per_launch);

/* hsvfilter (in place on d_src[k]) then colorlut (d_src[k] -> d_dst[k]) for n_batches independent batches of n_frames packed frames
 * each, issued from ONE native call - what n_batches pairs of mi355_hsvfilter_frames_device + mi355_colorlut_frames_device do
 * (video/hsv/src/hsvfilter/imp.rs:323-376 then video/colorlut/src/colorlut/imp.rs:203-223 per buffer), same kernels, same bytes.
 * lanes: 1 = all on the context's stream; 2 is accepted and runs as 1 (round 5's side stream for odd batches measured 12 % slower -
 * two memory-bound launches side by side evict each other's intermediate from the Infinity Cache - and did not order one-off
 * table builds across the lanes; removed in round 6). */
int mi355_hsv_colorlut_chain_batches_device(mi355_ctx *ctx, uint8_t *const *d_src, uint8_t *const *d_dst, int n_batches, int n_frames,
                                            size_t frame_pitch, int stride, int width, int height, int format,
                                            const mi355_hsv_settings *settings, int lanes);

/* ---------------------------------------------------------------- device buffers: what a device GstMemory wraps
 * Precedent: video/colorlut/src/d3d12colorlut/imp.rs:385-492 (propose_allocation / decide_allocation offer a pool of GPU
 * memory; an element whose input memory is "ours" works on the GPU resource, anything else maps it). A mi355_buf is `size`
 * bytes of HBM with a lazily created pinned host shadow and three-state dirty tracking (in sync / host newer / device newer):
 *   mi355_buf_device_ptr(buf, ctx, flags)  the pointer the *_device entry points take. MI355_MAP_READ uploads the shadow first
 *       if it is newer (on ctx's stream); MI355_MAP_WRITE marks the device side newer; ctx's stream is ordered behind the last
 *       commit of another context (hipStreamWaitEvent, no host wait). NULL on error (mi355_ctx_last_error(ctx)).
 *   mi355_buf_commit(buf, ctx)             call after enqueuing the kernels that use the pointer: "ctx's stream now holds the
 *       last use of this buffer".
 *   mi355_buf_map_host / unmap_host        GstMemory mem_map / mem_unmap: the pinned shadow; downloaded first (and the calling
 *       thread waits) only if the device side is newer; a WRITE map makes the host side newer at unmap.
 *   mi355_buf_ref / unref                  GstMemory copies share the buffer; the last unref waits for the device and frees.
 *   mi355_buf_state                        0 in sync, 1 host newer, 2 device newer (diagnostics).
 * mi355_ctx_transfer_counts: host->device / device->host copies enqueued so far by this context's buffers and by its
 * mi355_h2d / mi355_d2h / mask uploads (a chain of elements on device buffers costs ONE upload and ONE download:
 * tests/test_gpu_buf.py). */
enum { MI355_MAP_READ = 1, MI355_MAP_WRITE = 2 };
typedef struct mi355_buf mi355_buf;
mi355_buf *mi355_buf_alloc(mi355_ctx *ctx, size_t size);
mi355_buf *mi355_buf_ref(mi355_buf *buf);
void mi355_buf_unref(mi355_buf *buf);
size_t mi355_buf_size(const mi355_buf *buf);
void *mi355_buf_device_ptr(mi355_buf *buf, mi355_ctx *ctx, int flags);
int mi355_buf_commit(mi355_buf *buf, mi355_ctx *ctx);
void *mi355_buf_map_host(mi355_buf *buf, int flags);
int mi355_buf_unmap_host(mi355_buf *buf);
int mi355_buf_state(mi355_buf *buf);
int mi355_ctx_transfer_counts(mi355_ctx *ctx, uint64_t *h2d, uint64_t *d2h);

/* ---------------------------------------------------------------- roundedcorners on device-resident frames
 * video/videofx/src/border/imp.rs: generate_alpha_mask (:57-180) renders ONE A8 plane per caps / radius change and
 * prepare_output_buffer (:482-559) appends that one shared memory to every buffer as plane 3 of A420 (stride[3] x
 * round_up_2(height) bytes, :469-470). The bytes are cairo's and are rendered on the host (mi355host_rounded_corners_mask);
 *   mi355_roundedcorners_set_mask       keeps that plane in HBM (mask == NULL: passthrough, the plane is dropped);
 *   mi355_roundedcorners_mask_device    the shared device plane - what a device GstMemory appended to every buffer wraps
 *                                       (no bytes move per buffer, as in the reference);
 *   mi355_roundedcorners_append_device  writes the plane behind the I420 planes of n_frames frames (frame f's plane 3 at
 *                                       d_frames + f * frame_pitch + alpha_offset) for consumers that want A420 contiguous: one launch. */
int mi355_roundedcorners_set_mask(mi355_ctx *ctx, const uint8_t *mask, int width, int height, int stride);
int mi355_roundedcorners_mask_device(mi355_ctx *ctx, const uint8_t **d_mask, size_t *size, int *stride);
int mi355_roundedcorners_append_device(mi355_ctx *ctx, uint8_t *d_frames, size_t frame_pitch, size_t alpha_offset, int n_frames);

/* ---------------------------------------------------------------- colordetect
 * Replaces color_thief::get_palette(frame.plane_data(0), format, quality, max_colors) in ColorDetect::detect_color
 * (video/videofx/src/colordetect/imp.rs:57-84). The plane is read as one flat byte run of `data_len` bytes (row padding
 * included, strides ignored), every `quality`-th pixel of floor(data_len / ch) sampled. The MMCQ contract (color-thief 0.2.2,
 * not in the reference tree: parity unpinned) is DESIGN §4.8. Formats: MI355_FMT_RGB, _RGBA, _ARGB, _BGR, _BGRA; any other is
 * MI355_ERR_UNSUPPORTED. quality outside 1..10 or max_colors outside 2..255 is MI355_ERR_INVALID_ARG. A palette holds
 * *n_colors <= max_colors entries of r, g, b bytes in palette order (entry 0 is the dominant colour); 0 colours when no sample
 * is kept (the element turns that into GST_FLOW_ERROR). Scratch (histograms, results) belongs to the context.
 *   mi355_colordetect_frame            a host plane; synchronous.
 *   mi355_colordetect_frames_device    n_frames device planes at d_frames + f * frame_pitch; palette_rgb holds n_frames x 255 x 3
 *                                      bytes and n_colors n_frames ints; one synchronisation per call.
 *   mi355_colordetect_histogram_device diagnostics: the 32768 bins ((r>>3)<<10 | (g>>3)<<5 | (b>>3)) of one device plane and the
 *                                      first box {r1, r2, g1, g2, b1, b2} (all -1 when no sample is kept); synchronous.
 *   mi355_selftest_colordetect_mmcq    test only: the palette of a histogram the caller supplies. The 32768 bins are copied into
 *                                      the context's histogram scratch and colordetect_mmcq_kernel runs on them as it runs on a
 *                                      counted frame; palette, *n_colors and the first box come back and the scratch is zero
 *                                      again. Null pointers, max_colors outside 2..255 and bins that sum to more than 2^32 - 1
 *                                      (more than a frame can hold) are MI355_ERR_INVALID_ARG; synchronous. */
int mi355_colordetect_frame(mi355_ctx *ctx, const uint8_t *data, size_t data_len, int format, int quality, int max_colors,
                            uint8_t palette_rgb[255 * 3], int *n_colors);
int mi355_colordetect_frames_device(mi355_ctx *ctx, const uint8_t *d_frames, size_t frame_pitch, size_t data_len, int n_frames,
                                    int format, int quality, int max_colors, uint8_t *palette_rgb, int *n_colors);
int mi355_colordetect_histogram_device(mi355_ctx *ctx, const uint8_t *d_data, size_t data_len, int format, int quality,
                                       uint32_t hist[32768], int box[6]);
int mi355_selftest_colordetect_mmcq(mi355_ctx *ctx, const uint32_t bins[32768], int max_colors, uint8_t palette_rgb[255 * 3],
                                    int *n_colors, int box[6]);

/* ---------------------------------------------------------------- yolov8tensordec2 / yoloxtensordec (csrc/yolodec.hip)
 * Replaces the decode loops of YoloTensorDec::transform_ip (analytics/analytics/src/yolotensordec/imp.rs:234-422, iou :480-489):
 * per tensor the class argmax of every candidate under f32::total_cmp (the last of equal maxima), the thresholds, the sort by
 * class and descending confidence, the greedy per-class NMS and the casts handed to add_od_mtd. Bit-exact against the contract of
 * DESIGN 4.11. One stated deviation: the reference's sort_unstable_by leaves the order of entries of equal class and bit-equal
 * confidence open; here it is ascending candidate index. `max-detections` is never read by transform_ip and has no effect here
 * either; max_dets below is the caller's output capacity, not that property. Sign and payload of a NaN that arithmetic produces
 * (inf * 0, inf - inf) are the hardware's and outside the contract.
 *   layout        MI355_YOLO_V8: [1, F, N], field f of candidate c at data[c + f * N], classes are fields 4..F-1 (:297-327);
 *                 MI355_YOLO_X: [1, N, F], candidate c is the row data[c * F ..], b[4] is the box confidence, classes b[5..] (:328-356).
 *   record        the f32 box before the casts, the four ints add_od_mtd receives (:390-393), class index, confidence
 *                 (X: b[4] * class confidence) and the candidate's index in the tensor.
 *   _tensor          a host tensor; synchronous.
 *   _tensors_device  n_tensors device tensors of one shape at d_tensors + i * tensor_pitch_bytes, each with its OWN settings p[i]
 *                    (independent instances); dets holds n_tensors x max_dets records, n_dets n_tensors counts. Two launches,
 *                    one synchronisation and one download per call, whatever n_tensors is.
 *   n_dets[i] is the number of kept boxes even above max_dets; the first max_dets in output order are then written and the
 *   status stays MI355_OK. Limits: num_fields 6..1029 (below 6: MI355_ERR_INVALID_ARG, as find_yolo_tensor_meta refuses it,
 *   :459), num_candidates 0..65536 (0: no detections, no launch), n_tensors 1..1024, pitch >= F * N * 4 and a multiple of 4,
 *   device pointers 4-byte aligned; above the limits: MI355_ERR_UNSUPPORTED. Scratch belongs to the context and grows to the
 *   largest shape seen.
 *   mi355_selftest_yolodec_check : host only, no device: the status the shape checks of the two entry points give. */
typedef enum mi355_yolo_layout { MI355_YOLO_V8 = 0, MI355_YOLO_X = 1 } mi355_yolo_layout;
typedef struct mi355_yolo_params {
  float box_confidence_threshold;    /* "box-confidence-threshold" (X only, imp.rs:332) */
  float class_confidence_threshold;  /* "class-confidence-threshold" (imp.rs:314, :342) */
  float iou_threshold;               /* "iou-threshold" (imp.rs:376) */
} mi355_yolo_params;
typedef struct mi355_yolo_det {
  float xmin, ymin, xmax, ymax;      /* the f32 box, before the casts */
  int32_t x, y, width, height;       /* what add_od_mtd receives */
  uint32_t class_id;
  float confidence;
  uint32_t candidate;                /* index in the tensor */
  uint32_t reserved;                 /* 0 */
} mi355_yolo_det;
int mi355_yolodec_tensor(mi355_ctx *ctx, const float *data, int layout, uint32_t num_fields, uint32_t num_candidates,
                         const mi355_yolo_params *p, mi355_yolo_det *dets, uint32_t max_dets, uint32_t *n_dets);
int mi355_yolodec_tensors_device(mi355_ctx *ctx, const float *d_tensors, size_t tensor_pitch_bytes, int n_tensors, int layout,
                                 uint32_t num_fields, uint32_t num_candidates, const mi355_yolo_params *p, mi355_yolo_det *dets,
                                 uint32_t max_dets, uint32_t *n_dets);
int mi355_selftest_yolodec_check(size_t tensor_pitch_bytes, int n_tensors, int layout, uint32_t num_fields, uint32_t num_candidates);

/* ---------------------------------------------------------------- yoloxinference: head decode and input tensor (csrc/yolox_head.hip)
 * Replaces the two in-tree loops of `yoloxinference` around the network. The head decode is Head::forward / Head::decode
 * (analytics/burn/src/yoloxinference/yolox_burn/model/head.rs:23-34, :74-85, :89-122): from the per-level convolution outputs
 * reg_out, obj_out, cls_out - sigmoid, concatenation, flatten, transpose, then the grid / stride / exp decode - to the [1, A, 5 + C]
 * tensor that yoloxtensordec reads, or straight to its detections. The contract is DESIGN 4.13. Per tensor there are n_levels levels
 * in order (the reference fixes 3 with strides 8, 16, 32, head.rs:16); candidate a = (sum of the earlier levels' h * w) + y * w + x
 * (:84, :97-109: x is the fast index). Row a of the decoded tensor: (reg0 + x) * s, (reg1 + y) * s - an f32 add, then an f32
 * multiply, unfused (:114); exp(reg2) * s, exp(reg3) * s (:116); sigmoid(obj) (:75); sigmoid(cls[c]), c = 0..C-1. Detections are
 * DEFINED BY COMPOSITION: exactly what mi355_yolodec_tensors_device(..., MI355_YOLO_X, 5 + C, A, ...) returns for that tensor -
 * same records, same order, candidate = a; the class is the last of equal maxima of the SIGMOID values.
 * One stated deviation (as 4.12 a): exp and sigmoid come from burn's backend, whose source is not in the reference tree - RESTATED
 * WITHOUT SOURCE, PARITY UNPINNED. exp(x) is the f64 exponential of the f32 argument rounded once to f32 (overflow: inf);
 * sigmoid(x) is 1 / (1 + exp(-x)) evaluated in f64 from the f32 argument and rounded once (0 from about -104 down, exactly 1 from
 * about 17.4 up). A NaN in gives a NaN out; its sign and payload are the hardware's and outside the contract.
 *   level      device pointers to tensor 0's maps; tensor i's map is at (char *)p + i * pitch. reg [4][h][w], obj [1][h][w],
 *              cls [C][h][w], contiguous NCHW f32. The three maps of a level MAY LIE IN ONE ALLOCATION - obj = reg + 4 h w,
 *              cls = reg + 5 h w, equal pitches: the engine's fused [5 + C, h, w] output. Nothing is written to them.
 *   _head_decode_device  materialises [A, 5 + C] per tensor at d_out + i * out_pitch_bytes: one launch, asynchronous on the
 *                        context's stream. For callers who want the reference's tensor as it is.
 *   _head_dets_device    the fused form: p, dets, max_dets, n_dets exactly as in mi355_yolodec_tensors_device (own settings per
 *                        tensor, counts even above the capacity). Two launches, one synchronisation and one download per call,
 *                        whatever n_tensors is; no decoded tensor exists anywhere. A candidate is dropped on sigmoid(obj) <
 *                        box_confidence_threshold (yolotensordec/imp.rs:332) before any of its class values is read.
 *   _head_dets           the host form: the same struct with HOST pointers, one tensor, pitches ignored; synchronous.
 *   _input_frames_device the element's input (yoloxinference/imp.rs:439-447 packs the strided RGB frame, :533-539 converts and
 *                        permutes, no scaling): out[c][y][x] = (f32) in[y * stride + 3 x + c], [3][H][W] f32 per frame at
 *                        d_out + i * out_pitch_bytes, frame i at d_frames + i * frame_pitch (ignored for one frame). Exact. One
 *                        launch, asynchronous. n_frames 1..1024, width and height 1..65536 (above: MI355_ERR_UNSUPPORTED),
 *                        stride >= 3 * width, d_out 4-byte aligned, out pitch >= 3 H W 4 and a multiple of 4.
 *   MI355_ERR_INVALID_ARG: null pointers, n_levels < 1, n_tensors < 1, num_classes < 1, h, w or stride 0, reserved != 0, pointers
 *   not 4-byte aligned, a pitch below its map or no multiple of 4. MI355_ERR_UNSUPPORTED: n_levels > 8, 5 + C > 1029, A > 65536,
 *   stride > 65536, n_tensors > 1024. Scratch is the context's decoder scratch (yolodec) and grows to the largest shape seen.
 *   mi355_selftest_yolox_head_check : host only, no device: the status the shape checks of _head_decode_device give. The struct's
 *              pointers are checked for null and alignment only, never dereferenced. */
#define MI355_YOLOX_LEVELS_MAX 8
typedef struct mi355_yolox_level {
  const float *reg, *obj, *cls;      /* tensor i's map at (char *)p + i * pitch; reg [4][h][w], obj [1][h][w], cls [C][h][w] */
  size_t reg_pitch_bytes, obj_pitch_bytes, cls_pitch_bytes;
  uint32_t h, w, stride, reserved;   /* reserved 0 */
} mi355_yolox_level;
int mi355_yolox_head_decode_device(mi355_ctx *ctx, const mi355_yolox_level *levels, int n_levels, int n_tensors, uint32_t num_classes,
                                   float *d_out, size_t out_pitch_bytes);
int mi355_yolox_head_dets_device(mi355_ctx *ctx, const mi355_yolox_level *levels, int n_levels, int n_tensors, uint32_t num_classes,
                                 const mi355_yolo_params *p, mi355_yolo_det *dets, uint32_t max_dets, uint32_t *n_dets);
int mi355_yolox_head_dets(mi355_ctx *ctx, const mi355_yolox_level *levels, int n_levels, uint32_t num_classes,
                          const mi355_yolo_params *p, mi355_yolo_det *dets, uint32_t max_dets, uint32_t *n_dets);
int mi355_yolox_input_frames_device(mi355_ctx *ctx, const uint8_t *d_frames, size_t frame_pitch, size_t stride, int n_frames,
                                    uint32_t width, uint32_t height, float *d_out, size_t out_pitch_bytes);
int mi355_selftest_yolox_head_check(const mi355_yolox_level *levels, int n_levels, int n_tensors, uint32_t num_classes,
                                    size_t out_pitch_bytes);

/* ---------------------------------------------------------------- yoloxinference: the network (csrc/yolox_net.hip)
 * The f32 forward pass of Yolox::forward (analytics/burn/src/yoloxinference/yolox_burn/model/{blocks,bottleneck,darknet,pafpn,head,
 * yolox}.rs) up to, but not including, Head::decode and the two sigmoids of head.rs:75: for each of the three levels (strides 8, 16,
 * 32) the raw reg [4][h][w], obj [1][h][w] and cls [C][h][w] maps of reg_pred, obj_pred and cls_pred. The three maps of a level lie
 * in one allocation, the fused [5 + C, h, w] form of mi355_yolox_level, so the levels a forward fills go straight into
 * mi355_yolox_head_decode_device / _head_dets_device with n_tensors = n_frames. The contract is DESIGN 4.14.
 * Stated deviation (as 4.13's): burn's backends own the summation order of a convolution and their exp, and their source is not in the
 * reference tree - RESTATED WITHOUT SOURCE, PARITY UNPINNED. Ours is f32 throughout: f32 inputs, f32 fused multiply-add accumulation
 * in ascending (input channel, tap row, tap column) order - in steps of 16 terms whose sums are added in ascending order - and no
 * reduced-precision operand anywhere. BatchNorm (eps 1e-3, blocks.rs:114)
 * is a per-channel epilogue acc * scale + shift with scale = gamma / sqrt(var + eps), shift = beta - mean * scale computed in f64 and
 * rounded once to f32 at finalize; it is not folded into the weights. SiLU is x * (1 / (1 + exp(-x))) in f32. A Bottleneck's shortcut
 * is added after the activation (bottleneck.rs:20-30). Max-pool padding never wins (-inf). The net is deterministic: no atomics, no
 * split accumulation; the result of a frame does not depend on n_frames or on its position in the batch.
 *   config     depth in {0.33, 0.67, 1.0, 1.33} and width in {0.25, 0.375, 0.5, 0.75, 1.0, 1.25} (darknet.rs:51-59), depthwise 0 / 1,
 *              num_classes 1..1024, reserved 0; anything else MI355_ERR_INVALID_ARG (num_classes above 1024: MI355_ERR_UNSUPPORTED).
 *              Channel counts are floor(n * width) in f64 (blocks.rs:12), block counts max(round(3 * depth), 1) (darknet.rs:62), three
 *              times that in dark3 / dark4; shortcut is on in the backbone's C3 blocks but dark5's, off in the PAFPN's.
 *   parameters enumerated in ONE fixed order: the modules in the order their structs declare them (Yolox: backbone, head; Pafpn:
 *              backbone, lateral_conv0, c3_n3, c3_n4, c3_p3, c3_p4, reduce_conv1, bu_conv1, bu_conv2; CspDarknet: stem, dark2 .. dark5;
 *              CspBlock: conv, c3, spp; CspBottleneck: conv1, conv2, conv3, m.0 ..; Bottleneck and SppBottleneck: conv1, conv2;
 *              Head: stems.0 .. 2, cls_convs.0 .. 2 (conv0, conv1), reg_convs, cls_preds, reg_preds, obj_preds; a depthwise Conv:
 *              dconv, pconv), and per BaseConv conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var; per prediction
 *              layer weight, bias. Names are the state-dict names after the remapping of yolox.rs:255-272, e.g.
 *              backbone.backbone.dark3.c3.m.0.conv2.conv.weight, head.cls_convs.1.conv0.conv.weight. Weights are [out][in / groups][k][k].
 *   _set_param uploads parameter i from host memory (synchronous); n must be the parameter's element count. _finalize refuses
 *              (INVALID_ARG) while a parameter is unset; after it the net is immutable and _set_param fails (INVALID_ARG).
 *   _forward_device  d_in: [3][H][W] f32 per frame (what mi355_yolox_input_frames_device writes), frame i at (char *)d_in + i *
 *              in_pitch_bytes. Fills levels[3] with pointers into memory the net owns, valid until the next forward or destroy; level
 *              pitches are per frame. Asynchronous on the context's stream; no host synchronisation and no allocation once a shape
 *              has been seen: the activation arena is one allocation planned per (n_frames, H, W) that grows to the largest shape seen.
 *              H, W multiples of 32 (else INVALID_ARG; the pad template's rule, yoloxinference/imp.rs:239-247) and <= 2048, n_frames
 *              1..64 (above: MI355_ERR_UNSUPPORTED). Before _finalize: MI355_ERR_NOT_CONFIGURED.
 *   _launches  kernel launches of one forward (the length of the net's op list); _arena_info: the arena's bytes and how many device
 *              allocations the net has made for activations and the compositions' input tensor since create.
 *   _infer_frames_device / _infer_dets_device   DEFINED BY COMPOSITION: mi355_yolox_input_frames_device into a tensor the net owns,
 *              _forward_device, then mi355_yolox_head_decode_device / mi355_yolox_head_dets_device on the same stream - the same
 *              bytes as calling the three yourself. The second takes RGB frames and returns detections; nothing else crosses PCIe.
 *   mi355_selftest_yolox_net_plan / _param_info : host only, no device: every check's status, the parameter table and the plan.
 *   mi355_selftest_yolox_net_op_device : test only: ONE op of the list (kind 0 dense conv, 1 depthwise 3x3, 2 max-pool 5, 3 nearest
 *              2x upsample, 4 the stem's dense conv over the Focus gather of an [3][2 h_in][2 w_in] frame) on caller views: base
 *              pointer of channel 0 of the wider buffer, channel offset, channels of the wider buffer; frames are contiguous.
 *              The dense kernel has two tile shapes (64 channels x 64 or x 16 pixels; a forward takes the narrow one where the wide
 *              one would leave compute units without a block); every output is the same chain of 16-term steps under both, so the
 *              choice changes no byte.
 *   _set_precision   OPT-IN bf16 operands on the matrix cores. MI355_YOLOX_PRECISION_F32 (the default: everything above,
 *              byte for byte) or MI355_YOLOX_PRECISION_BF16; allowed between _create and _finalize, before or after the _set_param
 *              calls, any number of times - the last value holds. After _finalize, for an unknown value and for a null net:
 *              MI355_ERR_INVALID_ARG. _precision returns the value (null net: MI355_ERR_INVALID_ARG). A BF16 net:
 *                - every dense convolution (op kinds 0 and 4: the Focus stem and the nine prediction layers included) takes bf16
 *                  operands: a weight is rounded once at _finalize (on the device, into a second store beside the f32 one; an F32 net
 *                  allocates nothing new), an input activation as it is read; the pixel values 0 .. 255 are exact in bf16;
 *                - both roundings are round to nearest, ties to even; products are exact in f32 and accumulation is f32; the order
 *                  of accumulation inside a matrix instruction is the hardware's and is not pinned;
 *                - the epilogue is the f32 one unchanged: fmaf(acc, scale, shift), SiLU, residual, scale and shift as above;
 *                - activations stay f32 in the arena: views, arena plan, level buffers, depthwise, pool, upsample, head decode and
 *                  input conversion run the code they always ran; _launches and _arena_info are those of the F32 net;
 *                - deterministic: the same call twice gives the same bytes, a frame's maps depend neither on n_frames nor on its
 *                  position, the tile choice changes no byte (one instruction per output and 32-term step under either tile); no
 *                  atomics, no split accumulation;
 *                - operands of magnitude >= 2^127, NaN and f32 subnormals are outside the specification.
 *              The price, measured with the numpy restatement on the 40 seeded cases: the raw maps differ from the f64 maps by
 *              0.5 % to 5.8 % of a level's RMS. Group members of a BF16 net inherit the mode; a net has one precision for life.
 *   mi355_selftest_yolox_net_op_bf16_device : test only: op kinds 0 and 4 (others: MI355_ERR_INVALID_ARG) of the struct above under
 *              BF16: `weight` is f32 on the device and is packed by the routine _finalize uses, then the kernel a BF16 forward
 *              launches runs. tile: 0 as a forward chooses, 1 the 64 x 16 form, 4 the 64 x 64 form; anything else INVALID_ARG.
 *              Synchronises the context's stream (the packed copy is the call's own).
 * A net belongs to the context it was created on and is destroyed before it. */
typedef struct mi355_yolox_net mi355_yolox_net;
typedef struct mi355_yolox_net_config {
  double depth, width;
  int32_t depthwise;
  uint32_t num_classes;
  uint32_t reserved;   /* 0 */
} mi355_yolox_net_config;
/* the reference's six constructors (yolox.rs:40-222) */
#define MI355_YOLOX_NET_NANO(num_classes) {0.33, 0.25, 1, (num_classes), 0}
#define MI355_YOLOX_NET_TINY(num_classes) {0.33, 0.375, 0, (num_classes), 0}
#define MI355_YOLOX_NET_S(num_classes) {0.33, 0.50, 0, (num_classes), 0}
#define MI355_YOLOX_NET_M(num_classes) {0.67, 0.75, 0, (num_classes), 0}
#define MI355_YOLOX_NET_L(num_classes) {1.0, 1.0, 0, (num_classes), 0}
#define MI355_YOLOX_NET_X(num_classes) {1.33, 1.25, 0, (num_classes), 0}
#define MI355_YOLOX_NET_MAX_FRAMES 64
#define MI355_YOLOX_PRECISION_F32 0
#define MI355_YOLOX_PRECISION_BF16 1
#define MI355_YOLOX_NET_MAX_SIDE 2048
#define MI355_YOLOX_NET_NAME_MAX 96   /* a name_cap that holds every parameter name */
typedef struct mi355_yolox_net_plan {
  int32_t status;                                     /* the first refusal of: config, frames, size */
  int32_t config_status, frames_status, size_status;
  uint32_t param_count, launches;
  uint64_t param_floats, arena_bytes, macs;           /* macs: multiply-adds of one forward of n_frames frames */
  uint32_t level_h[3], level_w[3];
} mi355_yolox_net_plan;
typedef struct mi355_yolox_net_op {
  int32_t kind, k, stride, silu;                      /* k 1 / 3 (kind 0), stride 1 / 2 (kinds 0, 1) */
  uint32_t n_frames, h_in, w_in, tile;                /* tile (dense conv): 0 as a forward chooses, 1 the 64 x 16 form, 4 the 64 x 64 form */
  const float *in;
  uint32_t in_c, in_off, in_ctot, out_c;
  float *out;
  uint32_t out_off, out_ctot, res_off, res_ctot;
  const float *res;                                   /* null: no residual; out_c channels at the output's size */
  const float *weight, *scale, *shift;                /* kinds 0, 1, 4: [out_c][in_c / groups][k][k], [out_c], [out_c] */
} mi355_yolox_net_op;
int mi355_yolox_net_create(mi355_ctx *ctx, const mi355_yolox_net_config *config, mi355_yolox_net **net_out);
void mi355_yolox_net_destroy(mi355_yolox_net *net);
int mi355_yolox_net_param_count(const mi355_yolox_net *net);
int mi355_yolox_net_param_info(const mi355_yolox_net *net, int index, char *name, size_t name_cap, uint32_t dims[4], int *n_dims);
int mi355_yolox_net_set_param(mi355_yolox_net *net, int index, const float *host, size_t n);
int mi355_yolox_net_finalize(mi355_yolox_net *net);
int mi355_yolox_net_forward_device(mi355_yolox_net *net, const float *d_in, size_t in_pitch_bytes, int n_frames, uint32_t H, uint32_t W,
                                   mi355_yolox_level levels[3]);
int mi355_yolox_net_launches(const mi355_yolox_net *net);
int mi355_yolox_net_arena_info(const mi355_yolox_net *net, uint64_t *arena_bytes, uint64_t *allocations);
int mi355_yolox_infer_frames_device(mi355_yolox_net *net, const uint8_t *d_frames, size_t frame_pitch, size_t stride, int n_frames,
                                    uint32_t width, uint32_t height, float *d_out, size_t out_pitch_bytes);
int mi355_yolox_infer_dets_device(mi355_yolox_net *net, const uint8_t *d_frames, size_t frame_pitch, size_t stride, int n_frames,
                                  uint32_t width, uint32_t height, const mi355_yolo_params *p, mi355_yolo_det *dets, uint32_t max_dets,
                                  uint32_t *n_dets);
int mi355_selftest_yolox_net_plan(const mi355_yolox_net_config *config, int n_frames, uint32_t H, uint32_t W, mi355_yolox_net_plan *plan);
int mi355_selftest_yolox_net_param_info(const mi355_yolox_net_config *config, int index, char *name, size_t name_cap, uint32_t dims[4],
                                        int *n_dims);
int mi355_selftest_yolox_net_op_device(mi355_ctx *ctx, const mi355_yolox_net_op *op);
int mi355_yolox_net_set_precision(mi355_yolox_net *net, int precision);
int mi355_yolox_net_precision(const mi355_yolox_net *net);
int mi355_selftest_yolox_net_op_bf16_device(mi355_ctx *ctx, const mi355_yolox_net_op *op);

/* ---------------------------------------------------------------- handdetectiontensordec / handlandmarktensordec (csrc/handdec.hip)
 * Replaces the decode loops of the two hand decoders: extract_hands_from_palm_detection with is_valid_palm_candidate_normalized
 * and apply_nms_to_palm_candidates (analytics/analytics/src/hand/handdetectiontensordec/imp.rs:89-335), extract_hands with
 * compute_bbox_from_landmarks, compute_rotation_from_landmarks and the loops of attach_keypoint_metadata
 * (hand/handlandmarktensordec/imp.rs:101-391), and oriented_od_params_from_bbox_and_rotation (hand/helper.rs:69-114). The contract
 * is DESIGN 4.12; all arithmetic is f32 and unfused. Three stated deviations:
 *   a. atan2, sin, cos: the reference calls the platform's f32 libm, whose last bit differs between platforms. Here the value is
 *      the f64 function of the f32 arguments, rounded once to f32.
 *   b. iou: gst_analytics::image_util::iou_f32 is not in the reference tree. RESTATED WITHOUT SOURCE, PARITY UNPINNED: rects
 *      (x, y, w = max - min, h = max - min) as helpers.rs:22-37 builds them, right = x + w, bottom = y + h,
 *      iw = max(0, min(rights) - max(lefts)), ih likewise (f32::max / f32::min), inter = iw * ih,
 *      union = aw * ah + bw * bh - inter, iou = union > 0 ? inter / union : 0.
 *   c. sign and payload of a NaN that arithmetic produces are the hardware's and outside the contract.
 *   palm       [N, 8] row-major rows score, cx, cy, size, kp0x, kp0y, kp2x, kp2y (:133-153). Dropped iff score <
 *              confidence_threshold (IEEE: a NaN stays), iff size <= 0, iff the validity test fails (:231-296); a frame size scales
 *              the box (:177-183); descending score under f32::total_cmp, equal scores in ascending row index (sort_by is
 *              stable); greedy NMS as one class with the threshold clamped to [0, 1] (:315), stopping at max_hands.
 *   landmarks  [H, 21 * D] row-major, D >= 2, and an optional score vector: hand i has confidence scores[i] if i < num_scores, else
 *              1.0 (:274-277); the box is min / max over the finite points padded by 0.15 (:171-237), rotation from points 0 and
 *              9 unchecked (:148-169); sorted as palm; NMS with the threshold NOT clamped (:297-312). `attach-bounding-box` stays
 *              with the caller: the record always carries the box and has_od.
 *   record     the f32 box, rotation, rotation_od = rotation + (-FRAC_PI_2), confidence, the row / hand index, and what
 *              oriented_od_params_from_bbox_and_rotation returns: x, y, width, height with has_od = 1, or has_od = 0 and zeros
 *              when it returns None (the hand still counted toward max_hands and still suppressed others). mi355_hand_keypoints:
 *              the finite points of the hand in order, compacted (:337-373): count, positions (x as i32, y as i32), confidences
 *              (point[2] if D >= 3, else the hand's), visibilities (MI355_KP_*); entries from count on are zero.
 *   params     frame_width and frame_height both > 0: Some((w, h)); both 0: None; anything else MI355_ERR_INVALID_ARG. max_hands
 *              1..8 for palm, 1..10 for landmarks, otherwise MI355_ERR_INVALID_ARG.
 *   _tensor          host tensor(s); synchronous.
 *   _tensors_device  n_tensors device tensors of one shape at d + i * pitch, each with its OWN params p[i]; dets (and kps) hold
 *                    n_tensors x MI355_HAND_MAX records - tensor i's at [i * MI355_HAND_MAX ...), the first n_hands[i] written.
 *                    ONE launch (one block per tensor), one synchronisation and one download per call, whatever n_tensors is.
 *                    d_scores may be NULL (no scores: num_scores is then ignored); otherwise tensor i's num_scores scores are at
 *                    d_scores + i * score_pitch_bytes.
 *   Limits: palm num_rows 0..4096 and num_hands 0..1024 (0: counts 0, no launch), kps_dim 2..16 (below 2:
 *   MI355_ERR_INVALID_ARG, as decode_landmark_hands refuses it), num_scores 0..1024, n_tensors 1..1024 (below 1:
 *   MI355_ERR_INVALID_ARG); above the limits: MI355_ERR_UNSUPPORTED. Pitches at least the tensor (the scores) and a multiple of 4,
 *   pointers 4-byte aligned: otherwise MI355_ERR_INVALID_ARG. Scratch belongs to the context and grows to the largest call seen.
 *   mi355_selftest_handdec_check : host only, no device: the status the shape and params checks of the entry points give.
 *              decoder 0: palm (rows = num_rows; kps_dim, score_pitch_bytes, num_scores ignored), 1: landmarks (rows = num_hands;
 *              the score pitch is checked when num_scores > 0). */
#define MI355_HAND_MAX 10 /* records per tensor in the outputs */
typedef enum mi355_kp_visibility { MI355_KP_UNKNOWN = 0, MI355_KP_VISIBLE = 1, MI355_KP_OCCLUDED = 2 } mi355_kp_visibility;
typedef struct mi355_hand_params {
  float confidence_threshold;        /* "confidence-threshold" */
  float nms_iou_threshold;           /* "nms-iou-threshold" */
  uint32_t max_hands;                /* "max-hands" */
  int32_t frame_width, frame_height; /* the negotiated VideoInfo; 0, 0: none */
} mi355_hand_params;
typedef struct mi355_hand_det {
  float xmin, ymin, xmax, ymax;      /* the f32 box */
  float rotation, rotation_od;       /* the hand axis; what add_oriented_od_mtd receives (0 when has_od is 0) */
  float confidence;
  uint32_t index;                    /* row of the palm tensor / hand of the landmark tensor */
  int32_t x, y, width, height;       /* what add_oriented_od_mtd receives (0 when has_od is 0) */
  uint32_t has_od;                   /* 1: oriented_od_params_from_bbox_and_rotation returned Some */
  uint32_t reserved[3];              /* 0 */
} mi355_hand_det;
typedef struct mi355_hand_keypoints {
  uint32_t count;                    /* finite points */
  int32_t positions[42];             /* x0, y0, x1, y1, ... */
  float confidences[21];
  uint8_t visibilities[21];          /* mi355_kp_visibility */
  uint8_t reserved[11];              /* 0 */
} mi355_hand_keypoints;
int mi355_handdec_palm_tensor(mi355_ctx *ctx, const float *data, uint32_t num_rows, const mi355_hand_params *p, mi355_hand_det *dets,
                              uint32_t *n_hands);
int mi355_handdec_palm_tensors_device(mi355_ctx *ctx, const float *d_tensors, size_t tensor_pitch_bytes, int n_tensors,
                                      uint32_t num_rows, const mi355_hand_params *p, mi355_hand_det *dets, uint32_t *n_hands);
int mi355_handdec_landmarks_tensor(mi355_ctx *ctx, const float *landmarks, uint32_t num_hands, uint32_t kps_dim, const float *scores,
                                   uint32_t num_scores, const mi355_hand_params *p, mi355_hand_det *dets, mi355_hand_keypoints *kps,
                                   uint32_t *n_hands);
int mi355_handdec_landmarks_tensors_device(mi355_ctx *ctx, const float *d_landmarks, size_t tensor_pitch_bytes, int n_tensors,
                                           uint32_t num_hands, uint32_t kps_dim, const float *d_scores, size_t score_pitch_bytes,
                                           uint32_t num_scores, const mi355_hand_params *p, mi355_hand_det *dets,
                                           mi355_hand_keypoints *kps, uint32_t *n_hands);
int mi355_selftest_handdec_check(int decoder, size_t tensor_pitch_bytes, int n_tensors, uint32_t rows, uint32_t kps_dim,
                                 size_t score_pitch_bytes, uint32_t num_scores, uint32_t max_hands, int32_t frame_width,
                                 int32_t frame_height);

/* The tensor decoders across independent element instances. The reference element receives one tensor per buffer per instance
 * (analytics/analytics/src/yolotensordec/imp.rs:234-422); N decoders in one process are N lone calls per frame period, each almost
 * all launch, synchronisation and copy latency. submit_yolodec queues one device tensor of stream `ctx` and whatever is
 * pending goes out as at most THREE launches over job tables in the kernel arguments, on the queue's own HIP stream, with ONE
 * download of all counts and records. Members are fully independent: each tensor has its own shape (F, N), layout, three settings
 * and output capacity (raw yoloxinference head maps are members too: submit_yolox_head below). After wait_yolodec, dets and *n_dets hold exactly what mi355_yolodec_tensors_device(ctx, d_tensor,
 * F * N * 4, 1, layout, F, N, p, dets, max_dets, n_dets) would have returned, byte for byte: the tie rule (ascending candidate
 * index) makes the result independent of the order in which survivors were appended.
 *   submit : never blocks; the checks and status codes are those of mi355_yolodec_tensors_device with n_tensors = 1 and a pitch of
 *           F * N * 4 (layout, fields 6..1029, candidates 0..65536, a null or misaligned tensor with N > 0; a null group, ctx, p or
 *           ticket: MI355_ERR_INVALID_ARG). A refused submit queues nothing. N = 0 is accepted, gets a ticket and yields 0
 *           detections. The settings are copied at submit. The queue keeps room for min(max_dets, N) records for the tensor. The
 *           tensor is read after what ctx's HIP stream held at the call (an event recorded on that stream when it holds work);
 *           d_tensor is read until wait_yolodec for the ticket has returned.
 *   wait   : launches what is pending if the tensor has not gone out (rendezvous first), then waits for its launch set; the
 *           group's lock is not held meanwhile. Writes *n_dets (the kept count, even above max_dets) and the first
 *           min(*n_dets, max_dets) records into dets, which must hold the submit's max_dets records (null only when that was 0;
 *           a null n_dets or a null dets otherwise: MI355_ERR_INVALID_ARG, the result stays collectable). A result is collected
 *           once. Tickets are one sequence per group: a ticket that is unknown, already collected or another queue's is
 *           MI355_ERR_INVALID_ARG here and stays collectable where it belongs; mi355_group_wait, _order_after, _wait_compare,
 *           _wait_colordetect, _wait_hsvdetect and _wait_handdec refuse a decoder ticket - a tensor's or a head's - likewise.
 *   set_yolodec_rendezvous : as set_hsvdetect_rendezvous, counted over pending tensors only. The other queues' rendezvous, streams
 *           and stats and this queue's do not touch each other.
 *   At most MI355_YOLODEC_SET_MAX tensors share a launch set; more go out as consecutive sets. Per set: the V8 score launch if a V8
 *   tensor has a candidate, the X score launch likewise (kept apart: the X form's 33 KiB tile would halve the V8 form's occupancy),
 *   one NMS launch for all tensors with candidates, one device-to-host copy. A set whose tensors all have N = 0 launches and copies
 *   nothing. All scratch (counters, keys, kept boxes, result slabs) belongs to the queue and grows to the largest set seen; every set
 *   in flight has a pinned result block of its own, and results move out of it when the set is collected, so a later, larger set
 *   never overwrites what an earlier ticket still has to collect. flush, wait_all and destroy cover this queue as they cover the
 *   others. A launch that fails is reported to the call that caused it and, once, to each tensor's own wait; the survivor counters
 *   are cleared before the next set.
 *   yolodec_stats : {tensors launched, launch sets, tensors in the largest set, kernel launches}.
 *   mi355_selftest_yolodec_set_plan : host only, no device: the layout of one set, which the queue itself uses. Jobs keep submit
 *           order. blocks[j] = ceil(N_j / 256); first_block[j] = the running sum of blocks over the earlier jobs of j's own layout;
 *           key_offset = the running sum of the power of two at or above N_j (1 for N_j = 0) over all jobs; box_offset that of N_j;
 *           det_offset that of min(max_dets_j, N_j). totals = {V8 blocks, X blocks, NMS blocks (jobs with N > 0), keys, boxes,
 *           records}. Refused (MI355_ERR_INVALID_ARG): n_jobs outside 0..MI355_YOLODEC_SET_MAX, null arrays with n_jobs > 0, null
 *           totals; a job mi355_selftest_yolodec_check(F * N * 4, 1, layout, F, N) refuses returns that status. */
#define MI355_YOLODEC_SET_MAX 32 /* tensors per launch set */
int mi355_group_set_yolodec_rendezvous(mi355_group *group, int expected_streams, unsigned linger_us);
int mi355_group_submit_yolodec(mi355_group *group, mi355_ctx *ctx, const float *d_tensor, int layout, uint32_t num_fields,
                               uint32_t num_candidates, const mi355_yolo_params *p, uint32_t max_dets, uint64_t *ticket);
int mi355_group_wait_yolodec(mi355_group *group, uint64_t ticket, mi355_yolo_det *dets, uint32_t *n_dets);
/* {tensors launched, launch sets, tensors in the largest set, kernel launches} */
int mi355_group_yolodec_stats(mi355_group *group, uint64_t stats[4]);
/* host only, no device: the layout of one launch set */
int mi355_selftest_yolodec_set_plan(int n_jobs, const int *layout, const uint32_t *num_fields, const uint32_t *num_candidates,
                                    const uint32_t *max_dets, uint32_t *first_block, uint32_t *blocks, uint64_t *key_offset,
                                    uint64_t *box_offset, uint64_t *det_offset, uint64_t totals[6]);

/* yoloxinference's raw head maps as members of the decoder queue. A process with N `yoloxinference ! yoloxtensordec`
 * pipelines makes N lone mi355_yolox_head_dets_device calls per frame period; submit_yolox_head queues the head maps of ONE tensor of
 * stream `ctx` instead. A head is one more kind of member of the queue above, not a queue of its own: its ticket comes from the same
 * sequence and is collected with mi355_group_wait_yolodec into the same records; set_yolodec_rendezvous counts pending heads and
 * tensors together; MI355_YOLODEC_SET_MAX caps heads plus tensors per set; yolodec_stats counts a head as a tensor (its kernel
 * launches among the set's); flush, wait_all, destroy and the failure reporting cover it as they cover a tensor; the other queues'
 * wait functions refuse its ticket as they refuse a tensor's. After wait_yolodec, dets and *n_dets hold exactly what
 * mi355_yolox_head_dets_device(ctx, levels, n_levels, 1, C, p, dets, max_dets, n_dets) would have returned, byte for byte.
 *   submit : never blocks. Refused with the status of mi355_yolox_head_dets_device for one tensor: the shape checks of
 *           mi355_selftest_yolox_head_check(levels, n_levels, 1, C, ...) and its null or misaligned maps; the pitches are ignored
 *           (one tensor), there is no output pitch. A null group, ctx, p or ticket: MI355_ERR_INVALID_ARG. A refused submit queues
 *           nothing. The level structs and the settings are copied at submit. The maps are read after what ctx's HIP stream held at
 *           the call (the event of submit_yolodec) and until wait_yolodec for the ticket has returned; the three maps of a level may
 *           lie in one allocation. The queue keeps room for min(max_dets, A) records.
 *   Per set that holds a head: the tables of its heads and their levels (one level job per level of a head: the three planes, w,
 *   h w, first candidate, first tile, stride, head) are built in the set's pinned block, behind its results, and go to the device in
 *   ONE host-to-device copy; then TWO launches more than the set's tensors cost - the head score launch, one flat grid over the level
 *   jobs' tiles of 256 candidates of one level each, and the head NMS launch, one block per head - and the set's one download. A set
 *   of heads alone: one upload, two launches, one download. A set without a head uploads nothing and launches what it did before.
 *   yolox_head_stats : {heads launched, launch sets that held a head, level-table uploads, head kernel launches}.
 *   mi355_selftest_yolox_head_set_plan : host only, no device: the layout of one set that may hold heads, which the queue itself
 *           uses. kind[j]: MI355_YOLO_V8, MI355_YOLO_X or MI355_YOLO_X_HEAD (valid only here). A tensor job gets exactly what
 *           mi355_selftest_yolodec_set_plan gives it. A head job has num_fields = 5 + C, ignores num_candidates[j] and reads
 *           n_levels[j] and that many entries of level_h / level_w (the head jobs' levels one after the other; n_levels of a tensor
 *           job is not read): candidates[j] = A = the sum of h w (a tensor job's N), blocks[j] = the sum of ceil(h w / 256),
 *           first_block[j] = the running sum of blocks over the earlier head jobs, level_first_block (indexed as level_h) = the
 *           running sum of ceil(h w / 256) within the job. key_offset, box_offset and det_offset follow the old rules with N = A,
 *           over all jobs in submit order. totals = the old six (a head counts among the jobs with N > 0), head blocks, level jobs.
 *           Refused (MI355_ERR_INVALID_ARG): n_jobs outside 0..MI355_YOLODEC_SET_MAX, null arrays with n_jobs > 0 (the four level
 *           arrays only with a head job), null totals; a tensor job as in the old plan; a head job returns the status
 *           mi355_selftest_yolox_head_check gives its shape. */
#define MI355_YOLO_X_HEAD 2 /* a member kind of the queue's plan; no mi355_yolo_layout of the lone entry points or of submit_yolodec */
int mi355_group_submit_yolox_head(mi355_group *group, mi355_ctx *ctx, const mi355_yolox_level *levels, int n_levels,
                                  uint32_t num_classes, const mi355_yolo_params *p, uint32_t max_dets, uint64_t *ticket);
/* {heads launched, launch sets that held a head, level-table uploads, head kernel launches} */
int mi355_group_yolox_head_stats(mi355_group *group, uint64_t stats[4]);
/* host only, no device: the layout of one launch set that may hold heads */
int mi355_selftest_yolox_head_set_plan(int n_jobs, const int *kind, const uint32_t *num_fields, const uint32_t *num_candidates,
                                       const uint32_t *max_dets, const int *n_levels, const uint32_t *level_h,
                                       const uint32_t *level_w, uint32_t *candidates, uint32_t *first_block, uint32_t *blocks,
                                       uint64_t *key_offset, uint64_t *box_offset, uint64_t *det_offset,
                                       uint32_t *level_first_block, uint64_t totals[8]);

/* yoloxinference's network as a member of the decoder queue. A process with N `yoloxinference ! yoloxtensordec`
 * pipelines that share one finalized net makes N lone mi355_yolox_infer_dets_device calls of ONE frame per frame period, the worst
 * case of that call (88 - 160 dependent launches over grids that do not fill the device). submit_yolox_infer queues one RGB frame of
 * stream `ctx` for `net` instead, and a set runs ONE forward per (net, frame size) over all of its frames. An infer member is one
 * more kind of member of the queue above, not a queue of its own: its ticket comes from the group's one sequence and is collected
 * with mi355_group_wait_yolodec into mi355_yolo_det records; set_yolodec_rendezvous counts it with tensors and heads;
 * MI355_YOLODEC_SET_MAX caps the three kinds together (so a forward never exceeds 32 frames, within MI355_YOLOX_NET_MAX_FRAMES);
 * yolodec_stats counts it as a tensor, its launches among the set's; yolox_head_stats counts it as a head, which it is from the
 * score launch on; flush, wait_all, destroy, the failure reporting and the other queues' refusal of its ticket cover it as they
 * cover a head. After wait_yolodec, dets and *n_dets hold exactly what mi355_yolox_infer_dets_device(net, d_frame, 0, stride, 1,
 * width, height, p, dets, max_dets, n_dets) would have returned, byte for byte, the count above the capacity included: a frame's
 * maps depend neither on the frame count nor on its place in the batch, the tile choice changes no byte, the conversion is exact
 * and the head job kernels are byte-equal to the lone ones.
 *   submit : never blocks. Refused with the status the lone call gives one frame: H, W multiples of 32 (MI355_ERR_INVALID_ARG) and
 *           at most 2048 (MI355_ERR_UNSUPPORTED), MI355_ERR_NOT_CONFIGURED before _finalize, stride < 3 * width and a null frame
 *           (MI355_ERR_INVALID_ARG). MI355_ERR_INVALID_ARG also: a null group, ctx, net, p or ticket, and a net whose context is on
 *           another device than ctx. A refused submit queues nothing. The settings are copied at submit. The frame is read after
 *           what ctx's HIP stream held at the call (the event of submit_yolodec) and until wait_yolodec for the ticket has returned.
 *           The net must stay alive until every ticket that names it is collected. The queue keeps room for min(max_dets, A)
 *           records, A = the sum over l = 0..2 of (H >> (3 + l)) (W >> (3 + l)).
 *   A net shared by many threads: submit reads only what _finalize froze. The queue never touches the net's own arena, input tensor
 *           or plan: it runs forwards in activation LANES of its own, on the queue's stream, one per class key (net, H, W) - not per
 *           net: the head launches of a set run after all of its forwards, so two sizes of one net in a set need their own level
 *           buffers. The owner may go on making lone _forward_device / _infer_* calls between a submit and its wait. A lane grows to
 *           the largest frame count seen and is then reused without allocation; consecutive sets reuse it in stream order.
 *   Per set: the infer members fall into classes by (net, H, W), numbered by first appearance in submit order, their frames in submit
 *           order. The conversion jobs ride in the set's pinned block behind the head tables, in the same ONE host-to-device copy;
 *           then ONE conversion launch for all infer members of all classes (yolox_input_jobs_kernel: one flat grid over the jobs'
 *           blocks of 256 lanes of 4 pixels), then per class one forward of class_frames frames (mi355_yolox_net_launches(net)
 *           launches), then the set's launches as before - the head score and head NMS launches cover submitted heads and infer
 *           members together - and its one download. A set of k classes of infer members alone: one upload,
 *           1 + the sum of launches(net_c) + 2 launches, one download.
 *   release_yolox_net : waits for the queue's stream and frees the lanes of `net`. MI355_ERR_INVALID_ARG: null arguments, or a
 *           ticket that names the net is pending or uncollected (it stays collectable). mi355_group_destroy frees every lane. Lanes
 *           are keyed on a serial number a net gets at create, never on its address.
 *   yolox_infer_stats : {frames launched, forwards launched (classes), frames in the largest forward, kernel launches of conversions
 *           and forwards, lanes alive, device allocations made for lanes since create}.
 *   mi355_selftest_yolox_infer_set_plan : host only, no device: the infer side of one set's layout, which the queue itself uses.
 *           kind[j]: MI355_YOLO_V8, _X, _X_HEAD or MI355_YOLO_X_INFER. An infer job reads net_key[j] (any number that tells nets
 *           apart), height[j], width[j]: class_of[j] = its class, frame_in_class[j] = its position among the class's frames,
 *           conv_blocks[j] = ceil((W / 4) H / 256). Another job reads none of the three: class_of[j] = -1, conv_blocks[j] = 0.
 *           conv_first_block[j] = the running sum of conv_blocks over the earlier jobs, for every job. class_frames[c]: the frames
 *           of class c. totals = {classes, infer frames, conversion blocks}. The decode side of an infer job is what
 *           mi355_selftest_yolox_head_set_plan gives a head job of the levels (H/8, W/8), (H/16, W/16), (H/32, W/32) with 5 + C
 *           fields. Refused (MI355_ERR_INVALID_ARG): n_jobs outside 0..MI355_YOLODEC_SET_MAX, null arrays with n_jobs > 0, null
 *           totals, a kind outside 0..3; an infer job of a size the net refuses returns that status. */
#define MI355_YOLO_X_INFER 3 /* a member kind of the queue's plan only, as MI355_YOLO_X_HEAD is */
int mi355_group_submit_yolox_infer(mi355_group *group, mi355_ctx *ctx, mi355_yolox_net *net, const uint8_t *d_frame, size_t stride,
                                   uint32_t width, uint32_t height, const mi355_yolo_params *p, uint32_t max_dets, uint64_t *ticket);
int mi355_group_release_yolox_net(mi355_group *group, const mi355_yolox_net *net);
int mi355_group_yolox_infer_stats(mi355_group *group, uint64_t stats[6]);
int mi355_selftest_yolox_infer_set_plan(int n_jobs, const int *kind, const uint64_t *net_key, const uint32_t *height,
                                        const uint32_t *width, int32_t *class_of, uint32_t *frame_in_class,
                                        uint32_t *conv_first_block, uint32_t *conv_blocks, uint32_t *class_frames, uint64_t totals[3]);

/* The hand decoders across independent element instances. The reference elements receive one tensor per buffer per instance
 * (analytics/analytics/src/hand/handdetectiontensordec/imp.rs, hand/handlandmarktensordec/imp.rs: transform_ip); a process with N
 * camera pipelines, each with a palm decoder and a landmark decoder, makes 2 N lone calls per frame period, each a parameter
 * upload, a launch, a download and a synchronisation around a kernel of 5 - 15 us. submit_handdec_palm /
 * submit_handdec_landmarks queue one device tensor of stream `ctx` and whatever is pending goes out as at most TWO launches over job
 * tables in the kernel arguments (one block per tensor), on the queue's own HIP stream, with NO upload and ONE download of all counts
 * and records. Members are fully independent: each tensor has its own decoder, shape (N; H, D, scores) and settings. After
 * wait_handdec, dets, kps and *n_hands hold exactly what mi355_handdec_palm_tensors_device(ctx, d_tensor, N * 32, 1, N, p, dets,
 * n_hands) / mi355_handdec_landmarks_tensors_device(ctx, d_landmarks, H * 21 * D * 4, 1, H, D, d_scores, num_scores * 4, num_scores,
 * p, dets, kps, n_hands) would have returned, byte for byte: the job kernels run the lone kernels' own body (one device function,
 * one LDS layout).
 *   submit : never blocks; the checks and status codes are those of the lone entry points with n_tensors = 1 and a pitch equal to
 *           the tensor, i.e. what mi355_selftest_handdec_check(decoder, rows * row bytes, 1, rows, kps_dim, num_scores * 4,
 *           num_scores, max_hands, frame_width, frame_height) reports (palm rows 0..4096, hands 0..1024, kps_dim 2..16, scores
 *           0..1024, max_hands 1..8 / 1..10, the frame size both positive or both zero); a null group, ctx, p or ticket, or a null
 *           or misaligned tensor (or misaligned scores) with rows > 0: MI355_ERR_INVALID_ARG. d_scores == NULL: no scores, and
 *           num_scores is ignored. A refused submit queues nothing. Rows = 0 is accepted, gets a ticket and yields 0 hands. The
 *           settings are copied at submit. The tensor and the scores are read after what ctx's HIP stream held at the call (an
 *           event recorded on that stream when it holds work); they are read until wait_handdec for the ticket has returned.
 *   wait   : launches what is pending if the tensor has not gone out (rendezvous first), then waits for its launch set; the
 *           group's lock is not held meanwhile. Writes *n_hands (at most MI355_HAND_MAX) and the first *n_hands records of dets
 *           and, for a landmark ticket, of kps; records from *n_hands on are not touched, as in the lone form. dets and n_hands
 *           must not be null, kps must not be null for a landmark ticket (MI355_ERR_INVALID_ARG, the result stays collectable);
 *           kps is ignored for a palm ticket. A result is collected once. Tickets are one sequence per group: a ticket that is
 *           unknown, already collected or another queue's is MI355_ERR_INVALID_ARG here and stays collectable where it belongs;
 *           mi355_group_wait, _order_after, _wait_compare, _wait_colordetect, _wait_hsvdetect and _wait_yolodec refuse a hand
 *           ticket likewise.
 *   set_handdec_rendezvous : as set_hsvdetect_rendezvous, counted over pending hand tensors only. The other queues' rendezvous,
 *           streams and stats and this queue's do not touch each other.
 *   At most MI355_HANDDEC_SET_MAX tensors share a launch set; more go out as consecutive sets in submission order. Per set: the palm
 *   launch if a palm tensor has rows, the landmark launch likewise, one device-to-host copy of the set's result slab - 32 counts
 *   (128 bytes, by job), n_jobs x MI355_HAND_MAX mi355_hand_det (by job), n_landmark_jobs x MI355_HAND_MAX mi355_hand_keypoints (by
 *   the running index among landmark jobs). A set whose tensors all have 0 rows launches and copies nothing; a tensor without rows
 *   gets no block and its count is 0 on the host. Consecutive sets share the device slab (ordered on the queue's stream) and nothing
 *   in it is cleared between sets: every block writes its count on every path. Every set in flight has a pinned block of its own,
 *   and results move out of it when the set is collected. flush, wait_all and destroy cover this queue as they cover the others. A
 *   launch that fails is reported to the call that caused it and, once, to each tensor's own wait.
 *   handdec_stats : {tensors launched, launch sets, tensors in the largest set, kernel launches}.
 *   mi355_selftest_handdec_set_plan : host only, no device: the layout of one set, which the queue itself uses. Jobs keep submit
 *           order; decoder[j] is 0 (palm) or 1 (landmarks). block[j] = the running count of the earlier jobs of j's own decoder
 *           with rows > 0 - the block of j's launch that decodes it - or UINT32_MAX for a job without rows; kp_slot[j] = the
 *           running count of the earlier landmark jobs, or UINT32_MAX for a palm job. totals = {palm blocks, landmark blocks,
 *           landmark jobs, bytes copied = 128 + 640 n_jobs + 2880 landmark jobs, or 0 when no job has rows}. Refused
 *           (MI355_ERR_INVALID_ARG): n_jobs outside 0..MI355_HANDDEC_SET_MAX, null arrays with n_jobs > 0, null totals, a decoder
 *           that is neither 0 nor 1; rows above the decoder's limit (4096 / 1024): MI355_ERR_UNSUPPORTED. */
#define MI355_HANDDEC_SET_MAX 32 /* tensors per launch set */
int mi355_group_set_handdec_rendezvous(mi355_group *group, int expected_streams, unsigned linger_us);
int mi355_group_submit_handdec_palm(mi355_group *group, mi355_ctx *ctx, const float *d_tensor, uint32_t num_rows,
                                    const mi355_hand_params *p, uint64_t *ticket);
int mi355_group_submit_handdec_landmarks(mi355_group *group, mi355_ctx *ctx, const float *d_landmarks, uint32_t num_hands,
                                         uint32_t kps_dim, const float *d_scores, uint32_t num_scores, const mi355_hand_params *p,
                                         uint64_t *ticket);
int mi355_group_wait_handdec(mi355_group *group, uint64_t ticket, mi355_hand_det *dets, mi355_hand_keypoints *kps, uint32_t *n_hands);
/* {tensors launched, launch sets, tensors in the largest set, kernel launches} */
int mi355_group_handdec_stats(mi355_group *group, uint64_t stats[4]);
/* host only, no device: the layout of one launch set */
int mi355_selftest_handdec_set_plan(int n_jobs, const int *decoder, const uint32_t *rows, uint32_t *block, uint32_t *kp_slot,
                                    uint64_t totals[4]);

/* ---------------------------------------------------------------- agingradio
 * Replaces AgingRadio::process::<f32|f64> (audio/audiofx/src/agingradio/imp.rs:94-136): per pair of frames
 * (data.chunks_exact_mut(channels * 2), :101; an odd last frame is left untouched) either a click - every sample 1.0, filters
 * not run (:102-107) - or, per sample in f64: white noise (:108-112), the per-channel lowpass on the clamped sample (:113-116),
 * quantisation (:117-122), the cubic curve (:123-128), narrowed to the buffer's type (:130). The contract, the lowpass-filter
 * 0.4.1 restatement (parity unpinned) and the counter-based generator that replaces rand::rng() are DESIGN §4.9.
 *   settings         : Settings as transform_ip snapshots it once per buffer (imp.rs:284-305); lowpass-freq goes to setup.
 *   _setup           : AudioFilterImpl::setup (imp.rs:326-345): one filter per channel at y = 0 when lowpass_freq > 0, the pair
 *                      counter at 0, `seed` the instance's Philox key. channels or rate 0: MI355_ERR_INVALID_ARG; lowpass on
 *                      with more than 2048 channels: MI355_ERR_UNSUPPORTED.
 *   _process         : in place on `frames` interleaved frames in host memory (is_f64: F64, else F32); synchronous.
 *   _process_device  : the same on device memory; enqueued on the context's stream. Before setup both return
 *                      MI355_ERR_NOT_CONFIGURED (transform_ip's NotNegotiated, imp.rs:289).
 *   _get_state       : test access: the filters' outputs (min(channels, set-up channels) values; zeros without a lowpass) and
 *                      the frame pairs processed since setup.
 *   _reset           : BaseTransformImpl::stop (imp.rs:307-312): the state goes. */
typedef struct mi355_agingradio_settings {
  float white_noise_ampl;        /* "white-noise-ampl" 0..1 (imp.rs:108-112) */
  float clicks_prob;             /* "clicks-prob" 0..1 (imp.rs:102-103) */
  float bits_to_quantize;        /* "bits-to-quantize" 0..64 (imp.rs:117-122) */
  float cubic_curve_distortion;  /* "cubic-curve-distortion" 0..1 (imp.rs:123-128) */
  uint32_t cubic_curve_passes;   /* "cubic-curve-passes" (imp.rs:123-128) */
} mi355_agingradio_settings;
int mi355_agingradio_setup(mi355_ctx *ctx, unsigned channels, unsigned rate, unsigned lowpass_freq, uint64_t seed);
int mi355_agingradio_process(mi355_ctx *ctx, void *data, size_t frames, int is_f64, const mi355_agingradio_settings *settings);
int mi355_agingradio_process_device(mi355_ctx *ctx, void *d_data, size_t frames, int is_f64, const mi355_agingradio_settings *settings);
int mi355_agingradio_get_state(mi355_ctx *ctx, double *filter_state, unsigned channels, uint64_t *pairs_done);
int mi355_agingradio_reset(mi355_ctx *ctx);
/* agingradio through an audio group (csrc/agroup.hip): members are fully independent instances, as echo members are. Each has
 * its own setup (channels, rate, lowpass, seed: mi355_agroup_agingradio_setup, the element's AudioFilterImpl::setup), and each
 * submit carries its own buffer length, sample type and settings; one job table per launch set. A submit before the member's
 * setup returns MI355_ERR_NOT_CONFIGURED. get_state as mi355_agingradio_get_state, for one member. */
mi355_agroup *mi355_agroup_create_agingradio(int device, int n_members, int *status);
mi355_agroup *mi355_agroup_shared_agingradio(int device, int n_members, int *member, int *status);
int mi355_agroup_agingradio_setup(mi355_agroup *group, int member, unsigned channels, unsigned rate, unsigned lowpass_freq, uint64_t seed);
int mi355_agroup_submit_agingradio(mi355_agroup *group, int member, void *data, size_t frames, int is_f64,
                                   const mi355_agingradio_settings *settings, int device_data, uint64_t *ticket);
int mi355_agroup_agingradio_get_state(mi355_agroup *group, int member, double *filter_state, unsigned channels, uint64_t *pairs_done);

/* ---------------------------------------------------------------- minus1mixer / audiomultimixer (csrc/mixer.hip)
 * A conference bridge: every output hears the inputs its row of the contribution matrix names. Replaces the mixing loop of
 * MultiMixerElement::aggregate_one_buffer (audio/audiomultimixer/src/audiomultimixerelement.rs:606-753) and the splitter's
 * Splitter::sink_chain / split_output_buf (audio/audiomultimixer/src/splitter.rs:341-358, :433-467): the interleaved f32 buffer
 * n_out_channels wide that the one fills and the other slices never exists here. One interval of `frames` frames:
 *   - n_out_channels f32 accumulators per frame start at +0.0 (the aggregator's zero-filled buffer);
 *   - every segment - `num_frames` mono frames of input pad `input`, F32LE or S16LE, landing at output frame `out_offset` - adds
 *     in_sample = f32::from(x) / conv_scale (1.0 for F32, 32768.0 for S16, :707) to every channel c with contrib[input][c]
 *     (:711-715), IN ARRAY ORDER: f32 addition is not associative, the order is part of the result. A pad may send several
 *     segments per interval, or none;
 *   - every output owns the channels [channel_offset, channel_offset + n_channels) (create_output_buffer, :580-603) and gets
 *     T::from_f32(acc * conv_scale) (splitter.rs:460): F32 unchanged, S16 as Rust's `as i16` (toward zero, NaN 0, saturating).
 * Limits, beyond any of which the call returns MI355_ERR_UNSUPPORTED: n_inputs <= 256, n_out_channels <= 256, at most 1024
 * segments per interval, frames <= 2^20; and at most 1024 outputs per call. Inputs are mono, as the reference asserts (:624).
 *   _setup          : OutputConfiguration::get_output_contributions_for_input_channel (:191-214) as a row-major bool matrix
 *                     n_inputs x n_out_channels (non-zero = contributes). May be called again between intervals: pads come and go
 *                     (request_new_pad / release_pad). Zero inputs or channels, a null matrix: MI355_ERR_INVALID_ARG.
 *   _setup_minus1   : the matrix update_output_config builds (audio/audiomultimixer/src/minus1mixer.rs:500-537): n_streams inputs,
 *                     n_streams one-channel outputs, contrib[i][o] = (i != o). A lone participant hears silence.
 *   _process        : host buffers of any alignment, synchronous; the samples travel through one pinned slab: one upload and one
 *                     download per call, beside the small copy of the launch's job table that both forms make.
 *   _process_device : device buffers, enqueued on the context's stream (the segment and output arrays are copied in the call).
 *                     Every `data` pointer is aligned to its sample type - 4 bytes for F32, 2 for S16 - or the call returns
 *                     MI355_ERR_INVALID_ARG: apply in_offset in frames, not in bytes.
 *                     `data` of a segment points at its first frame to mix (the caller has applied in_offset); an output buffer is
 *                     frames x n_channels interleaved samples. Output ranges may overlap or leave channels unused. frames == 0,
 *                     a segment of no frames, no segment at all (silence) are fine. Nothing is written and nothing is launched when:
 *                     before setup MI355_ERR_NOT_CONFIGURED; input >= n_inputs, a format other than 0 / 1, out_offset + num_frames
 *                     > frames, channel_offset + n_channels > n_out_channels, n_channels == 0, null data of a non-empty segment
 *                     or output: MI355_ERR_INVALID_ARG.
 *   _reset          : the element's stop: the matrix goes (process answers MI355_ERR_NOT_CONFIGURED again).
 *   mi355_selftest_mixer_plan : host only, no device: the job table of one launch for n_members mixers. Member j gets
 *                     ceil(frames[j] / MI355_MIXER_FRAME_TILE) * ceil(n_out_channels[j] / 16) blocks from first_block[j] on and
 *                     its slices of the segment, output and contribution-word tables (seg_offset, out_offset, bits_offset; every
 *                     array is [n_members + 1], the total last). With the three block_* arrays (block_capacity entries each, at
 *                     least the total) it also answers, through the function the kernel uses, which member, frame tile and
 *                     channel group each block serves. A limit exceeded: MI355_ERR_UNSUPPORTED. */
#define MI355_MIXER_FRAME_TILE 64 /* frames per block of the mixer kernel */
typedef struct mi355_mixer_segment {
  const void *data;
  uint32_t input, format /* 0 F32LE, 1 S16LE */, out_offset, num_frames;
} mi355_mixer_segment;
typedef struct mi355_mixer_output {
  void *data;
  uint32_t format, channel_offset, n_channels;
} mi355_mixer_output;
int mi355_mixer_setup(mi355_ctx *ctx, unsigned n_inputs, unsigned n_out_channels, const uint8_t *contrib);
int mi355_mixer_setup_minus1(mi355_ctx *ctx, unsigned n_streams);
int mi355_mixer_process(mi355_ctx *ctx, const mi355_mixer_segment *segments, unsigned n_segments, const mi355_mixer_output *outputs,
                        unsigned n_outputs, size_t frames);
int mi355_mixer_process_device(mi355_ctx *ctx, const mi355_mixer_segment *segments, unsigned n_segments, const mi355_mixer_output *outputs,
                               unsigned n_outputs, size_t frames);
int mi355_mixer_reset(mi355_ctx *ctx);
int mi355_selftest_mixer_plan(int n_members, const uint32_t *n_inputs, const uint32_t *n_out_channels, const uint32_t *n_segments,
                              const uint32_t *n_outputs, const uint64_t *frames, uint32_t *first_block, uint32_t *seg_offset,
                              uint32_t *out_offset, uint32_t *bits_offset, uint32_t block_capacity, uint32_t *block_member,
                              uint32_t *block_tile, uint32_t *block_group);
/* mixers through an audio group (csrc/agroup.hip): a member is one mixer - one room of a bridge server - with its own matrix,
 * segment and output formats and `frames` per submit (aggregate_one_buffer, audiomultimixerelement.rs:606-753, and split_output_buf,
 * splitter.rs:433-467, for every member that has submitted in ONE kernel launch). Checks and statuses as mi355_mixer_process
 * (device_data = 0) / mi355_mixer_process_device (1); a
 * submit before the member's setup returns MI355_ERR_NOT_CONFIGURED. The segment and output arrays are copied at submit; the
 * buffers they name are borrowed until wait(ticket), which answers `frames`. mixer_launches: kernel launches of the group's launch
 * sets so far (one per set in which a member has a frame). */
mi355_agroup *mi355_agroup_create_mixer(int device, int n_members, int *status);
mi355_agroup *mi355_agroup_shared_mixer(int device, int n_members, int *member, int *status);
int mi355_agroup_mixer_setup(mi355_agroup *group, int member, unsigned n_inputs, unsigned n_out_channels, const uint8_t *contrib);
int mi355_agroup_mixer_setup_minus1(mi355_agroup *group, int member, unsigned n_streams);
int mi355_agroup_submit_mixer(mi355_agroup *group, int member, const mi355_mixer_segment *segments, unsigned n_segments,
                              const mi355_mixer_output *outputs, unsigned n_outputs, size_t frames, int device_data, uint64_t *ticket);
uint64_t mi355_agroup_mixer_launches(mi355_agroup *group);

#ifdef __cplusplus
}
#endif
#endif /* MI355FX_H */
