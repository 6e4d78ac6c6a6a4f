// internal.hpp — shared declarations between the C-ABI layer (ctx.hip) and the kernel files.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include "../../include/mi355fx.h"

#include "autopick.hpp"
#include "colorlut_brick.hpp"
#include "colorlut_window.hpp"

namespace mi355 {

// Device-side copy of a loaded CubeLut (video/colorlut/src/parser.rs:69-75).
// Choice between an interpolating ("compute") kernel and the memoised-table kernel for one entry point: the policy
// state (autopick.hpp) plus the two events that bracket a sampled launch (colorlut_kernels.hip: auto_launch).
struct AutoPick : AutoPolicy {
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
};

// "The settings (and, for hsvfilter alone, the byte order) have been the same for kStableCalls consecutive calls": what a memoised
// table is built for - an animated property would otherwise rebuild 64 MiB every buffer (colorlut_kernels.hip: table_front).
constexpr unsigned kStableCalls = 8;
struct Settled {
  mi355_hsv_settings hs{};  // settings of the previous call
  int bgr = 0;              // ... and its byte order
  unsigned stable = 0;      // for how many calls they have not changed
  bool note(const mi355_hsv_settings &h, int b = 0) {  // counts this call; true once the settings have stayed
    if (std::memcmp(&h, &hs, sizeof(h)) == 0 && b == bgr) { if (stable < kStableCalls) stable++; }
    else { hs = h; bgr = b; stable = 0; }
    return stable >= kStableCalls;
  }
};

struct LutDevice {
  int is3d = 0;
  int size = 0;
  float scale[3] = {1, 1, 1};
  float offset[3] = {0, 0, 0};
  float *d_cells = nullptr;   // 3D: [size^3][4] as the reference stores it; 1D: r|g|b planes
  float *d_planar = nullptr;  // 3D only: three channel planes in the LDS image layout (see colorlut_kernels.hip)
  uint32_t *d_axis = nullptr; // 3D only: per-axis {offset, t} tables, 3 x 256 x 2 dwords
  size_t planar_plane_floats = 0;  // floats per padded plane
  int lds_Sy = 0, lds_Sz = 0;      // LDS row / plane strides (floats)
  size_t lds_bytes = 0;            // dynamic LDS per block
  bool lds_all_resident = false;   // all three planes staged once (small LUTs)
  bool lds_ok = false;        // LDS fast path legal for this LUT (fits, finite, bounded)
  // 2^24-entry memoised tables (RGBA8): see colorlut_table_kernel. [0] = colorlut alone, [1] = hsvfilter -> colorlut
  // under the hsv settings in table_hs.
  uint32_t *d_table[2] = {nullptr, nullptr};   // = table_ref[i]'s device pointer (shared between contexts, see SharedTable)
  std::shared_ptr<void> table_ref[2];          // keeps the shared table alive while this context uses it
  std::string table_key[2];                    // what the table in use was built from
  std::string digest;                          // identifies the loaded LUT (contents, size, kind, domain) in table keys
  int table_morton[2] = {-1, -1};  // layout of the table: 0 linear, 1 Morton, -1 not built
  mi355_hsv_settings table_hs{};   // settings d_table[1] was built for
  Settled seen;                    // the fused entry point's settings, call by call
  AutoPick pick[2];                // compute-kernel / table-kernel choice for the two entry points
  int last_sub[2] = {0, 0};        // which kernel read the table last: 0 gather, 1 LDS-cached (colorlut_window.hip) - by provenance of the input
  BrickLut brick;                  // brick form of a 3D LUT for the brick-cache interpolating kernel (colorlut_brick.hip)
  bool building_table = false;     // launch_*_compute is being run over the all-colours frame by table_ensure
  const char *last_kernel = "";    // name of the kernel that served the last mi355_colorlut_* / mi355_hsv_colorlut_* launch
  bool loaded = false;
};

// hsvfilter through a memoised table (colorlut_kernels.hip: launch_hsvfilter): the table of the element's per-pixel
// function under `hs` for colour-first 4-byte formats (bgr selects the byte order the table was built for).
struct HsvTable {
  uint32_t *d_table = nullptr;         // = table_ref's device pointer
  std::shared_ptr<void> table_ref;
  bool valid = false;
  int bgr = 0;
  mi355_hsv_settings hs{};       // settings the table was built for
  Settled seen;                  // the settings and the byte order, call by call
  bool last_table = false;       // the last launch_hsvfilter call ran the table kernel
  AutoPick pick;
};

struct EchoDevice {
  double *d_ring = nullptr;   // n_streams rings of ring_len f64
  size_t ring_len = 0;
  size_t pos = 0;             // shared: every stream of a batch advances by the same number of samples per call
  int n_streams = 1;
  void *d_par = nullptr, *h_par = nullptr;  // per-stream {D, intensity, feedback}: device copy, pinned host copy
  hipEvent_t par_ev = nullptr;
  bool configured = false;
};

}  // namespace mi355

struct mi355_dssim_image;

struct mi355_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  int n_cu = 256;
  // staging for the host entry points
  void *d_stage[2] = {nullptr, nullptr};
  size_t d_stage_bytes[2] = {0, 0};
  mi355::LutDevice lut;
  mi355::EchoDevice echo;
  void *ebur128 = nullptr;     // mi355::Ebur128State (ebur128_kernels.hip)
  void *hrtf = nullptr;        // mi355::HrtfState (hrtf_kernels.hip)
  void *sofa = nullptr;        // mi355::SofaState (sofa_kernels.hip)
  void *loudnorm = nullptr;    // mi355::LoudNormLone (loudnorm.hip): a LoudNormBatch of one stream and the element's adapter
  void *loudnorm_batch = nullptr;  // mi355::LoudNormBatch (loudnorm.hip): n streams in lock step
  void *dssim_cache = nullptr; // mi355::DssimCache (dssim_kernels.hip)
  void *rounded = nullptr;     // mi355::RoundedMask (roundedcorners.hip): the element's alpha plane, device-resident
  void *colordetect = nullptr; // mi355::ColorDetectState (colordetect.hip): histograms and palette results
  void *agingradio = nullptr;  // mi355::AgingState (agingradio.hip): lowpass filter states, pair counter, seed
  void *mixer = nullptr;       // mi355::MixerState (mixer.hip): the contribution matrix, job tables and the host form's staging
  void *yolodec = nullptr;     // mi355::YoloDecState (yolodec.hip): survivor keys, kept boxes, results
  void *handdec = nullptr;     // mi355::HandDecState (handdec.hip): params, results, staging
  // host <-> device copies this context has enqueued through the library's own entry points and mi355_buf objects (tests assert
  // that a chain of elements on device buffers costs ONE upload and ONE download: mi355_ctx_transfer_counts)
  unsigned long long n_h2d = 0, n_d2h = 0;
  bool force_generic = false;
  int fused_variant = 0;  // MI355_FLAG_FUSED_VARIANT
  int lut_variant = 0;    // MI355_FLAG_LUT_VARIANT
  int hsv_table_mode = 0; // MI355_FLAG_HSV_TABLE: 0 auto for GENERIC settings only (default), 1 auto for all, 2 table only, 3 off
  mi355::HsvTable hsv_table;
  int lut_stagger = 0;    // MI355_FLAG_LUT_STAGGER (x256 clock ticks)
  int brick_tiles_per_run = 0;  // MI355_FLAG_BRICK_TILES_PER_RUN (tuning; 0 = default)
  int brick_fold_axis = 2;      // MI355_FLAG_BRICK_FOLD_AXIS (accepted, ignored)
  hipEvent_t host_copy_ev = nullptr;  // marks "the caller's host buffer has been read" for entry points that return before their kernels end
  int dssim_translucent = 0;    // MI355_FLAG_DSSIM_TRANSLUCENT: 1 = alpha < 255 composed over black instead of over the crate's pattern
  int dssim_fast = 0;           // MI355_FLAG_DSSIM_FAST: 1 = pairs go through the separable pair kernel (dssim_fast.hip), read when a pair is handed over
  int brick_prio = 3;           // MI355_FLAG_BRICK_PRIO: bit 0 progress-based wave priorities, bit 1 tile stealing within a block
  int brick_sets = 0;           // MI355_FLAG_BRICK_SETS: 0 = content watch decides (default); 32 (4x4x2 sets, 16 waves per CU) or 64 (4x4x4 sets, 8 waves per CU) pinned
  int hrtf_method = 0;         // MI355_FLAG_HRTF_METHOD: 0 = by HRIR length, 1 = overlap-save FFT, 2 = time-domain FIR (takes effect at mi355_hrtf_setup)
  int window_min_steps = mi355::kWindowMinStepsPerBlock;  // MI355_FLAG_WINDOW_MIN_STEPS
  int window_order = 1;         // MI355_FLAG_WINDOW_ORDER: how the blocks of colorlut_window_kernel share the steps (0 contiguous shares, 1 aligned fronts: default)
  bool window_stats_on = false; // MI355_FLAG_WINDOW_STATS: the LDS-cached kernels count {pixels, pixels past the cache, bricks installed} (three atomics per wave: off by default)
  unsigned long long *d_window_counters = nullptr;  // colorlut_window.hip: {pixels, pixels past the LDS cache, bricks installed} x 1024 slots
  int blockhash_any_size = 0;  // MI355_FLAG_BLOCKHASH_ANY_SIZE
  int hsv_nt = 2;              // MI355_FLAG_HSV_NT: 2 = plain loads, write-through stores that stay in the Infinity Cache (hsv_kernels.hip:
                               // hsv_store_through; the default by profiles/r07_store_policy_ab.txt), 0 = plain loads and stores, 1 = both
                               // with the non-temporal hint (measurement A/B)
  mi355_hsv_settings group_fused_hs{};  // mi355_group_submit_fused: the settings of this stream's last fused submit ...
  unsigned group_fused_stable = 0;      // ... and how many submits in a row have carried them (a composed table is built for settings that stay)
  int hsv_blocks_per_cu = 64;  // grid cap of the flat hsvfilter kernel (tunable: MI355_FLAG_HSV_BLOCKS_PER_CU)
  std::string last_error;
};

namespace mi355 {

// frames of several streams handed to ONE launch (group.hip): base pointers by value in the kernel arguments
constexpr int kMultiFrames = 16;
struct MultiFramePtrs { uint8_t *p[kMultiFrames]; };

// pixel layout of a packed-RGB format
struct PixFmt {
  int pixel_stride;  // bytes per pixel: 3, 4 (8 for RGBA64)
  int first;         // byte offset of the colour triple
  int bgr;           // triple stored B,G,R
  int has_alpha;     // 4th byte is alpha (vs padding) — informational
};
bool pixfmt_of(int format, PixFmt *out);

int set_error(mi355_ctx *ctx, int status, const std::string &msg);
// Where a launch's input comes from decides which of the two table kernels reads it (colorlut_kernels.hip: launch_table_raw):
// note_written: a launch of this library that WRITES [p, p + bytes) has just been enqueued on `device`; recently_written: is
// [p, p + bytes) inside what one of the last two such launches wrote, and small enough to still be on-die (Infinity Cache)?
void note_written(int device, const void *p, size_t bytes);
bool recently_written(int device, const void *p, size_t bytes);
void forget_written(int device, const void *p, size_t bytes);   // a host copy has replaced that range
int check_hip(mi355_ctx *ctx, hipError_t e, const char *what);

// An owning, grow-only buffer of n elements of T: in device memory, or (PINNED) in pinned host memory. Scratch that grows to the
// largest shape seen: the decoders' (yolodec.hip, handdec.hip) is made of these.
template <typename T, bool PINNED>
struct GrowBuf {
  T *p = nullptr;
  size_t n = 0;   // elements held; 0 when p is null
  GrowBuf() = default;
  GrowBuf(const GrowBuf &) = delete;
  GrowBuf &operator=(const GrowBuf &) = delete;
  ~GrowBuf() { release(); }
  void release() {
    if (p) (void)(PINNED ? hipHostFree(p) : hipFree(p));
    p = nullptr;
    n = 0;
  }
  // Nothing if the buffer already holds `want` elements. Otherwise the old allocation is freed and one of `want` elements made: the
  // contents are NOT kept, and *fresh (if given) is set - whatever the buffer held is gone, also when the allocation fails, which
  // leaves the buffer empty and the runtime's last error cleared.
  // (hipFree waits for the device: work still running on a stream has finished with the old allocation)
  hipError_t reserve(size_t want, bool *fresh = nullptr) {
    if (n >= want && p) return hipSuccess;
    release();
    if (fresh) *fresh = true;
    const hipError_t e = PINNED ? hipHostMalloc((void **)&p, want * sizeof(T), hipHostMallocDefault) : hipMalloc((void **)&p, want * sizeof(T));
    if (e != hipSuccess) {
      (void)hipGetLastError();
      p = nullptr;
      return e;
    }
    n = want;
    return hipSuccess;
  }
};
template <typename T> using DeviceBuf = GrowBuf<T, false>;
template <typename T> using PinnedBuf = GrowBuf<T, true>;

// kernel launchers (asynchronous on ctx->stream)
int launch_hsvfilter(mi355_ctx *ctx, uint8_t *d_data, int n_frames, size_t frame_pitch, int width,
                     int height, int stride, const PixFmt &fmt, const mi355_hsv_settings &s);
int launch_hsvfilter_compute(mi355_ctx *ctx, uint8_t *d_data, int n_frames, size_t frame_pitch, int width,
                     int height, int stride, const PixFmt &fmt, const mi355_hsv_settings &s);
void hsv_table_release(mi355_ctx *ctx);
bool hsvfilter_multi_applicable(const uint8_t *const *frames, int n_frames, int width, int height, int stride, const PixFmt &fmt);
int launch_hsvfilter_multi(mi355_ctx *ctx, hipStream_t stream, uint8_t *const *frames, int n_frames, int width, int height, const PixFmt &fmt,
                           const mi355_hsv_settings &s);
// colorlut of n separate packed RGBA frames of one size through ctx's memoised (Morton) table, ONE launch on `stream`; the table
// is built on ctx->stream first if need be (*table_out = what the launch reads). MI355_ERR_UNSUPPORTED: not this path's geometry.
int colorlut_multi_table(mi355_ctx *ctx, const uint32_t **table_out);
int colorlut_multi_fused_table(mi355_ctx *ctx, const mi355_hsv_settings *hs, const uint32_t **table_out);
int launch_colorlut_multi(mi355_ctx *ctx, hipStream_t stream, const uint32_t *table, uint8_t *const *srcs, uint8_t *const *dsts, int n_frames, int width,
                          int height, bool from_hbm = false);
int launch_hsvdetect(mi355_ctx *ctx, const uint8_t *d_src, size_t src_pitch, int src_stride,
                     const PixFmt &sfmt, uint8_t *d_dst, size_t dst_pitch, int dst_stride,
                     int dst_alpha_first, int dst_bgr, int n_frames, int width, int height,
                     const mi355_hsvdetect_settings &s);
int launch_colorlut(mi355_ctx *ctx, const uint8_t *d_src, size_t src_pitch, int src_stride,
                    uint8_t *d_dst, size_t dst_pitch, int dst_stride, int n_frames, int width,
                    int height, int format);
int launch_hsv_colorlut(mi355_ctx *ctx, const uint8_t *d_src, size_t src_pitch, int src_stride,
                        uint8_t *d_dst, size_t dst_pitch, int dst_stride, int n_frames, int width,
                        int height, const mi355_hsv_settings &hs);
bool table_variant(int lut_variant);  // the MI355_FLAG_LUT_VARIANT values that pin a memoised-table kernel
int lut_upload(mi355_ctx *ctx, int is3d, size_t size, const float *table, const float scale[3],
               const float offset[3]);
void lut_release(mi355_ctx *ctx);
int echo_setup(mi355_ctx *ctx, int n_streams, size_t ring_len);
void echo_release(mi355_ctx *ctx);
int launch_echo_batch(mi355_ctx *ctx, void *d_data, size_t stream_stride, size_t n, int is_f64, const size_t *delay, const double *intensity,
                      const double *feedback);
int launch_echo(mi355_ctx *ctx, void *d_data, size_t n, int is_f64, size_t delay, double intensity,
                double feedback);
int ebur128_setup(mi355_ctx *ctx, unsigned channels, unsigned rate, unsigned mode, const int *channel_class);
int ebur128_setup_batch(mi355_ctx *ctx, unsigned n_streams, unsigned channels, unsigned rate, unsigned mode, const int *channel_class);
int ebur128_add_frames_batch(mi355_ctx *ctx, const void *data, size_t frames, int fmt, int device_data);
int ebur128_query_batch(mi355_ctx *ctx, int what, double *out);
int ebur128_peak_batch(mi355_ctx *ctx, int true_peak, double *out);
int ebur128_reset(mi355_ctx *ctx);
int ebur128_reset_stream(mi355_ctx *ctx, unsigned stream);
int ebur128_add_frames_streams(mi355_ctx *ctx, const void *data, size_t slot_elems, const size_t *frames_per, int fmt, int device_data);
void ebur128_release(mi355_ctx *ctx);
int launch_blockhash(mi355_ctx *ctx, const uint8_t *d_frames, size_t frame_pitch, int stride, int n_frames, int width, int height,
                     int channels, unsigned long long *hashes);
int launch_imghash(mi355_ctx *ctx, const uint8_t *d_frames, size_t frame_pitch, int stride, int n_frames, int width, int height, int channels,
                   int algo, unsigned long long *hashes);
int loudnorm_setup(mi355_ctx *ctx, unsigned channels, double loudness_target, double loudness_range_target, double max_true_peak, double offset_db);
int loudnorm_push(mi355_ctx *ctx, const double *data, size_t frames, double *out, size_t out_cap_frames, size_t *out_frames);
int loudnorm_drain(mi355_ctx *ctx, double *out, size_t out_cap_frames, size_t *out_frames, int *eos);
void loudnorm_release(mi355_ctx *ctx);
int loudnorm_setup_batch(mi355_ctx *ctx, unsigned n_streams, unsigned channels, double loudness_target, double loudness_range_target, double max_true_peak, double offset_db);
size_t loudnorm_batch_frame_size(mi355_ctx *ctx);
size_t loudnorm_member_frame_size(mi355_ctx *ctx, unsigned stream);
int loudnorm_member_frame_type(mi355_ctx *ctx, unsigned stream);
int loudnorm_process_members(mi355_ctx *ctx, const unsigned char *members, const double *data, size_t stream_stride, size_t frames, double *out, size_t out_stride,
                             size_t out_cap_frames, size_t *out_frames, int device_data, int final_frame);
int loudnorm_process_batch(mi355_ctx *ctx, const double *data, size_t stream_stride, size_t frames, double *out, size_t out_stride, size_t out_cap_frames,
                           size_t *out_frames, int device_data, int final_frame);
void loudnorm_batch_release(mi355_ctx *ctx);
int dssim_create_image(mi355_ctx *ctx, const uint8_t *d_frame, int stride, int width, int height, int channels, mi355_dssim_image **out);
void dssim_free_image(mi355_ctx *ctx, mi355_dssim_image *img);
// map_scale >= 0 (mi355_selftest_dssim_compare_detail): the SSIM map of that scale goes to map_out and its [sum, avg, dev] slots to
// slots_out (host; either may be null) behind the value
int dssim_compare(mi355_ctx *ctx, const mi355_dssim_image *a, const mi355_dssim_image *b, double *out, int map_scale = -1, float *map_out = nullptr,
                  double *slots_out = nullptr);
int dssim_plan(int width, int height, int n_cu, mi355_dssim_plan *plan);   // host only (mi355_selftest_dssim_plan)
int dssim_compare_frames(mi355_ctx *ctx, const mi355_dssim_image *a, const uint8_t *const *d_frames, int n_frames, int stride, int width, int height,
                         int channels, double *out);
int dssim_compare_pairs_enqueue(mi355_ctx *ctx, const uint8_t *const *d_refs, const uint8_t *const *d_frames, int n_pairs, int stride, int width, int height,
                                int channels, double *h_slots);
void dssim_scores_from_slots(int width, int height, const double *h_slots, int n_pairs, double *out);
// pairs through the entry points of the C ABI: waited for; the form is ctx->dssim_fast's. map_scale >= 0: the SSIM map of that scale
// of pair 0 is copied to map_out (host) as well
int dssim_compare_pairs(mi355_ctx *ctx, const uint8_t *const *d_refs, const uint8_t *const *d_frames, int n_pairs, int stride, int width, int height,
                        int channels, double *out, int map_scale, float *map_out);
// the fast form's pair kernel (dssim_fast.hip): blocks [first[j], first[j+1]) take the 32 x 16 tiles of job j - one scale of one
// (reference, frame) pair, read from the packed bytes (scale 0) or from the two linear float4 chains - and write the scale's SSIM
// map and one f64 partial per tile
struct DssimFastJob { const uint8_t *u8[2]; const float4 *lin[2]; int stride, channels, pattern, w, h; float *map; double *partial; };
struct DssimFastJobs { DssimFastJob job[3]; unsigned first[4]; const float *lut; };
constexpr int kDssimFastTw = 32, kDssimFastTh = 16;
int dssim_fast_enqueue(mi355_ctx *ctx, const DssimFastJobs &J);
constexpr int kDssimSlotDoubles = 15;  // per comparison: 5 scales x [sum, avg, dev]
int blockhash_enqueue(mi355_ctx *ctx, const uint8_t *const *d_frames, int n, int stride, int width, int height, int channels, uint32_t *d_sums,
                      unsigned long long *d_hashes);
int dssim_cbrt_selftest(mi355_ctx *ctx, uint32_t lo_bits, uint32_t hi_bits, uint64_t *mismatches);
void dssim_release(mi355_ctx *ctx);
void roundedcorners_release(mi355_ctx *ctx);
void colordetect_release(mi355_ctx *ctx);
// launch sets of the video group's colordetect queue (colordetect.hip): frames of independent instances, one job table
constexpr int kCdSetMax = MI355_COLORDETECT_SET_MAX;
struct CdFrame { const uint8_t *data; size_t data_len; int format, quality, max_colors; };
struct CdSetScratch;  // kCdSetMax histograms (zero between sets) and results, on the device
// the checks of mi355_colordetect_frames_device for one frame; *why names the refusal
int colordetect_check_frame(size_t data_len, int format, int quality, int max_colors, const char **why);
int colordetect_plan(int n_cu, int n_jobs, const uint64_t *n_samples, uint32_t *first_block, uint32_t *blocks, uint64_t *samples_per_block, uint32_t *total_blocks);
CdSetScratch *colordetect_set_scratch_new(hipStream_t stream, int *status, std::string *err);
void colordetect_set_scratch_free(CdSetScratch *S);
size_t colordetect_set_block_bytes();  // the pinned block a set's results are copied to
// n <= kCdSetMax checked frames on `stream`: histogram launch (none if no frame has a sample), MMCQ launch, results into h_block
int colordetect_launch_set(CdSetScratch *S, hipStream_t stream, int n_cu, const CdFrame *frames, int n, void *h_block, int *kernel_launches, std::string *err);
void colordetect_set_result(const void *h_block, int i, uint8_t palette_rgb[255 * 3], int *n_colors);
// launch sets of the video group's hsvdetector queue (hsv_kernels.hip): frames of independent instances, one job table
constexpr int kHdSetMax = MI355_HSVDETECT_SET_MAX;
struct HdFrame {
  const uint8_t *src;
  uint8_t *dst;
  int src_stride, dst_stride, width, height;
  PixFmt sfmt;
  int dst_alpha_first, dst_bgr;
  mi355_hsvdetect_settings s;
  int force_generic;  // the member's MI355_FLAG_FORCE_GENERIC at submit
};
// the checks of mi355_hsvdetect_frames_device for n_frames frames (ctx.hip; both entries call it); *why names the refusal
int hsvdetect_check_frames(const uint8_t *d_src, int src_stride, int src_format, const uint8_t *d_dst, int dst_stride, int dst_format, int n_frames,
                           int width, int height, const mi355_hsvdetect_settings *settings, PixFmt *sfmt, int *alpha_first, int *bgr, const char **why);
int hsvdetect_plan(int n_cu, int blocks_per_cu, unsigned units_per_block, int n_jobs, const uint64_t *units, uint32_t *first_block, uint32_t *blocks,
                   uint32_t *total_blocks);
// n <= kHdSetMax checked frames on `stream`: the vector launch and / or the literal launch, whichever has a job with a pixel
int hsvdetect_launch_set(hipStream_t stream, int n_cu, const HdFrame *frames, int n, int *kernel_launches, std::string *err);
// launch sets of the video group's hsvfilter queue (hsv_kernels.hip): frames of independent instances filtered in place, one job table
constexpr int kHfSetMax = MI355_HSVFILTER_SET_MAX;
struct HfFrame {
  uint8_t *data;
  int width, height, stride;
  PixFmt fmt;
  mi355_hsv_settings s;
  int force_generic;  // the member's MI355_FLAG_FORCE_GENERIC at submit
  int hsv_nt;         // the member's MI355_FLAG_HSV_NT at submit: 2 = write-through stores for a flat 4-byte frame (1 is the lone entry's A/B only)
};
// the checks of mi355_hsvfilter_frames_device for n_frames frames (ctx.hip; both entries call it); *why names the refusal
int hsvfilter_check_frames(const uint8_t *d_data, int n_frames, size_t frame_pitch, int width, int height, int stride, int format,
                           const mi355_hsv_settings *settings, PixFmt *fmt, const char **why);
// do the byte ranges [data, data + (height - 1) stride + width pixel_stride) of two frames meet? (a frame without a pixel has no byte)
bool hsvfilter_frames_overlap(const HfFrame &a, const HfFrame &b);
// host only: the sets n frames go out in - a new one at kHfSetMax frames and in front of a frame that overlaps one of the set - and per
// frame its set, launch (0 no pixel, 1 vector, 2 literal), variant, units and blocks; the builder hsvfilter_launch_set launches from
int hsvfilter_set_plan(int n_cu, const HfFrame *frames, int n, mi355_hsvfilter_plan_out *out, int *n_sets);
// n <= kHfSetMax checked frames on `stream`: the vector launch and / or the literal launch, whichever has a job with a pixel
int hsvfilter_launch_set(hipStream_t stream, int n_cu, const HfFrame *frames, int n, int *kernel_launches, std::string *err);
// launch sets of the video group's colorlut queue (colorlut_group.hip): frames of independent instances, each with the LUT its context
// held at submit (borrowed: the cells stay the context's), source to destination, one job table
constexpr int kClSetMax = MI355_COLORLUT_SET_MAX;
struct ClFrame {
  const uint8_t *src;
  uint8_t *dst;
  int src_stride, dst_stride, width, height, format;
  const float *cells;  // the LUT as the reference stores it (LutDevice::d_cells)
  int is3d, size;
  float scale[3], offset[3];
  int force_generic;   // the member's MI355_FLAG_FORCE_GENERIC at submit
};
// the checks of mi355_colorlut_frames_device (ctx.hip; both entries call it), in its order; *bpp: bytes per pixel of the format; *why
// names the refusal. MI355_OK with n_frames, width or height 0 means "nothing to do"
int colorlut_check_frames(bool lut_loaded, const uint8_t *d_src, size_t src_pitch, int src_stride, const uint8_t *d_dst, size_t dst_pitch, int dst_stride,
                          int n_frames, int width, int height, int format, int *bpp, const char **why);
// do a frame's own source and destination byte ranges [p, p + (height - 1) stride + width bpp) meet? (no pixel: no byte)
bool colorlut_frame_in_place(const ClFrame &f);
// must `later` run after `earlier` has finished: its destination range meets earlier's source or destination, or its source meets
// earlier's destination (ranges only: conservative). The one test of the submit entry and of the set builder
bool colorlut_frames_meet(const ClFrame &earlier, const ClFrame &later);
// host only: the sets n frames go out in - a new one at kClSetMax frames and in front of a frame that meets one of the set - and per
// frame its set, launch (0 no pixel, 1 vector, 2 literal), geometry class, units and blocks; the builder colorlut_launch_set launches from
int colorlut_set_plan(int n_cu, const ClFrame *frames, int n, mi355_colorlut_plan_out *out, int *n_sets);
// n <= kClSetMax checked frames on `stream`: the vector launch and / or the literal launch, whichever has a job with a pixel
int colorlut_launch_set(hipStream_t stream, int n_cu, const ClFrame *frames, int n, int *kernel_launches, std::string *err);

// agingradio (agingradio.hip): one job = one element instance's buffer. The host fills the table (alpha and the quantise factor
// computed with its libm); the group (agroup.hip) submits one job per member, a context a table of one.
enum { kAgingClick = 1, kAgingNoise = 2, kAgingQuant = 4, kAgingCubic = 8 };
struct AgingJob {
  void *data;                        // interleaved F32 / F64 samples, processed in place
  double *state;                     // lowpass output y per channel; nullptr: no lowpass (lowpass-freq 0 at setup)
  unsigned long long frames, k0;     // frames of this buffer; frame pairs the instance has processed before it
  unsigned long long seed, p_int;    // Philox key; Bernoulli threshold (~0: always)
  double alpha, factor, ampl, dist;  // lowpass coefficient, 2^bits, white-noise amplitude, cubic distortion
  unsigned channels, passes;
  int is_f64, flags;                 // kAging*
};
int agingradio_setup_filter(unsigned rate, unsigned lowpass_freq, double *alpha);
void agingradio_settings_to_job(const mi355_agingradio_settings &s, AgingJob *J);
int launch_agingradio_jobs(hipStream_t stream, int n_cu, const AgingJob *h_jobs, const AgingJob *d_jobs, unsigned n_jobs, std::string *err);
void agingradio_release(mi355_ctx *ctx);
// minus1mixer / audiomultimixer (mixer.hip): one call = one mixer's interval, checked, its data pointers on the device. The group
// (agroup.hip) launches one call per member that has submitted, a context a set of one.
struct MixerCall {
  unsigned n_inputs, n_out_channels;
  const uint16_t *bits;   // host: mixer_pack_contrib's words
  const mi355_mixer_segment *segs;
  unsigned n_segs;
  const mi355_mixer_output *outs;
  unsigned n_outs;
  size_t frames;
};
struct MixerLayout {      // the host form's packing of a call's buffers into an input and an output slot
  std::vector<size_t> seg_off, seg_bytes, out_off, out_bytes;
  size_t in_bytes = 0, out_bytes_total = 0;
};
struct MixerTablesBuf;    // pinned + device image of a launch's job tables
MixerTablesBuf *mixer_tables_new(std::string *err, int *status);
void mixer_tables_free(MixerTablesBuf *B);
void mixer_pack_contrib(unsigned n_inputs, unsigned n_out, const uint8_t *contrib, std::vector<uint16_t> *bits);   // contrib nullptr: i != o
int mixer_check_setup(unsigned n_inputs, unsigned n_out, const char **why);
int mixer_check(unsigned n_inputs, unsigned n_out, const mi355_mixer_segment *segs, unsigned n_segs, const mi355_mixer_output *outs, unsigned n_outs,
                size_t frames, bool device, const char **why);
void mixer_layout(const mi355_mixer_segment *segs, unsigned n_segs, const mi355_mixer_output *outs, unsigned n_outs, size_t frames, MixerLayout *L);
int mixer_plan(int n_members, const uint32_t *n_inputs, const uint32_t *n_out_channels, const uint32_t *n_segments, const uint32_t *n_outputs,
               const uint64_t *frames, uint32_t *first_block, uint32_t *seg_off, uint32_t *out_off, uint32_t *bits_off);
int mixer_launch(MixerTablesBuf *B, hipStream_t stream, const MixerCall *calls, int n, int *kernel_launches, std::string *err);
void mixer_release(mi355_ctx *ctx);
void yolodec_release(mi355_ctx *ctx);
void handdec_release(mi355_ctx *ctx);
// yoloxinference's network as a member of the decoder queue (yolox_net.hip): what a submit reads of a net (frozen by _finalize, but
// for `finalized` itself), the plan of a set's infer members (mi355_selftest_yolox_infer_set_plan; yolodec_plan_set plans the queue's
// sets with it) and the queue's activation lanes, one per class key (net serial, H, W)
struct YxNetInfo { uint64_t serial; int device; bool finalized; uint32_t num_classes; int launches; };
void yolox_net_info(const mi355_yolox_net *net, YxNetInfo *out);
int yolox_net_check_size(uint32_t H, uint32_t W, const char **why);
int yolox_infer_set_plan(int n_jobs, const int *kind, const uint64_t *net_key, const uint32_t *height, const uint32_t *width, int32_t *class_of,
                         uint32_t *frame_in_class, uint32_t *conv_first_block, uint32_t *conv_blocks, uint32_t *class_frames, uint64_t totals[3]);
struct YxLanes;
YxLanes *yolox_lanes_new();
void yolox_lanes_free(YxLanes *S);   // frees every lane
void yolox_lanes_stats(const YxLanes *S, uint64_t *alive, uint64_t *allocations);
int yolox_lanes_release(YxLanes *S, uint64_t serial);   // frees the lanes of that net (hipFree waits for the device); how many
// the lane of (net, H, W) planned for n_frames and grown to hold them (no allocation once it has seen the largest count): its input
// tensor [n_frames][3][H][W] and frame 0's maps with the bytes from frame to frame
int yolox_lanes_prepare(YxLanes *S, const mi355_yolox_net *net, uint32_t n_frames, uint32_t H, uint32_t W, float **d_input, mi355_yolox_level levels[3],
                        std::string *err);
// one forward of the lane as prepared, from its input tensor, on `stream`
int yolox_lanes_forward(YxLanes *S, const mi355_yolox_net *net, uint32_t n_frames, uint32_t H, uint32_t W, hipStream_t stream, int n_cu, int *kernel_launches,
                        std::string *err);
// the checks of mi355_yolodec_tensors_device that need no device; *why names the refusal
int yolodec_check_args(size_t tensor_pitch_bytes, int n_tensors, int layout, uint32_t num_fields, uint32_t num_candidates, const char **why);
// launch sets of the video group's decoder queue (yolodec.hip): tensors of independent instances, job tables
constexpr int kYdSetMax = MI355_YOLODEC_SET_MAX;
constexpr size_t kYdCountsBytes = 128;  // a result block: kYdSetMax kept counts (by job), then the jobs' records at their det_offset
// A member is a decoded tensor (layout MI355_YOLO_V8 / MI355_YOLO_X: data) or the raw head maps of one yoloxinference tensor (layout
// MI355_YOLO_X_HEAD: head; data is null, num_fields = 5 + C, num_candidates = A, the sum of the levels' h * w).
struct YdHead { mi355_yolox_level lv[MI355_YOLOX_LEVELS_MAX]; int n_levels; };   // the submit's copy of the level structs
// (a tensor member carries no levels: its `head` is empty, and copying it through the queue costs what it did)
// An infer member (layout MI355_YOLO_X_INFER: infer; data and head are null, num_fields = 5 + C, num_candidates = A of the frame size)
// is one RGB frame for a finalized net: the set converts it, runs it through one forward of its class (net, H, W) in a lane of the
// queue's own, and from the score launch on it is a head of three levels in that lane's level buffers.
struct YdInfer { const mi355_yolox_net *net; uint64_t serial; const uint8_t *frame; size_t stride; uint32_t width, height; };
struct YdTensor {
  const float *data; int layout; uint32_t num_fields, num_candidates, max_dets; mi355_yolo_params p; std::shared_ptr<const YdHead> head;
  std::shared_ptr<const YdInfer> infer;
};
struct YdSetScratch;  // counters (zero between sets), keys, kept boxes and positions, results, the head members' tables, on the device
// the shape checks of the YOLOX head entry points (yolox_head.hip): everything but the map pointers and pitches; *A_out: the candidates
int yolox_head_check_shape(const mi355_yolox_level *lv, int n_levels, int n_tensors, uint32_t C, uint32_t *A_out, const char **why);
// the map pointers of checked levels (pitches are not looked at: one tensor)
int yolox_head_check_maps(const mi355_yolox_level *lv, int n_levels, const char **why);
// The layout of one set (mi355_selftest_yolox_head_set_plan and, without heads, mi355_selftest_yolodec_set_plan; yolodec_plan_set
// plans the queue's sets with it). kind: MI355_YOLO_V8 / _X / _X_HEAD per job. A head job reads its n_levels[j] and that many entries
// of level_h / level_w (the head jobs' levels one after the other) and ignores num_candidates[j]; candidates[j] is its A (a tensor
// job's N; may be num_candidates itself). level_first_block: per level, in the order of level_h, the running sum of ceil(h w / 256)
// within the job. The four level arrays may be null when no job is a head. totals: V8 score blocks, X score blocks, jobs with a
// candidate (a head counts as one), keys, boxes, records, then the head score blocks and the level jobs.
int yolodec_mixed_set_plan(int n_jobs, const int *kind, const uint32_t *num_fields, const uint32_t *num_candidates, const uint32_t *max_dets, const int *n_levels,
                           const uint32_t *level_h, const uint32_t *level_w, uint32_t *candidates, uint32_t *first_block, uint32_t *blocks, uint64_t *key_offset,
                           uint64_t *box_offset, uint64_t *det_offset, uint32_t *level_first_block, uint64_t totals[8]);
// the plan of one set of the queue: what yolodec_mixed_set_plan writes, by job (level_first_block: by level, the heads' levels one
// after the other). Made ONCE per set: it sizes the set's pinned block and yolodec_launch_set lays the set out with it.
struct YdSetPlan {
  uint32_t candidates[kYdSetMax], first_block[kYdSetMax], blocks[kYdSetMax];
  uint64_t key_off[kYdSetMax], box_off[kYdSetMax], det_off[kYdSetMax];
  uint32_t level_first_block[kYdSetMax * MI355_YOLOX_LEVELS_MAX];
  uint64_t totals[8];
  // the infer members' side (yolox_infer_set_plan): classes, frames of a class, conversion blocks; infer_totals = {classes, frames, blocks}
  int32_t class_of[kYdSetMax];
  uint32_t frame_in_class[kYdSetMax], conv_first_block[kYdSetMax], conv_blocks[kYdSetMax], class_frames[kYdSetMax];
  uint64_t infer_totals[3];
};
// the plan of n members (zeroed totals on a refusal): a head member without its levels, or with fewer than 0 or more than
// MI355_YOLOX_LEVELS_MAX of them, is MI355_ERR_INVALID_ARG; the rest are yolodec_mixed_set_plan's refusals
int yolodec_plan_set(const YdTensor *tensors, int n, YdSetPlan *out);
YdSetScratch *yolodec_set_scratch_new(int *status, std::string *err);
void yolodec_set_scratch_free(YdSetScratch *S);
size_t yolodec_set_result_bytes(uint64_t records);  // the counts and that many records (totals[5]): what a set's download writes
// the pinned block of a set: its results, and behind them the tables of its head members (level_jobs = totals[7]; 0: none)
// (infer_jobs = infer_totals[1]: the conversion jobs of the infer members ride behind the level jobs, in the same copy)
size_t yolodec_set_block_bytes(uint64_t records, uint64_t level_jobs, uint64_t infer_jobs = 0);
// n <= kYdSetMax members and their plan (yolodec_plan_set) on `stream`: the head tables' upload (only if the set holds a head), the
// V8 score launch, the X score launch (each only if it has a job with a candidate), the head score launch, the tensors' NMS launch,
// the heads' NMS launch, counts and records into h_block (nothing launched or copied if no member has a candidate). head_counts:
// {heads, table uploads, head kernel launches} of this set.
// A set with infer members takes the queue's lanes and the device's compute units: after the upload ONE conversion launch for all
// infer members, then one forward per class, then the launches above. infer_counts: {frames, classes, frames of the largest class,
// kernel launches of the conversion and the forwards} of this set.
int yolodec_launch_set(YdSetScratch *S, hipStream_t stream, const YdTensor *tensors, int n, const YdSetPlan &plan, void *h_block, size_t h_block_bytes,
                       int *kernel_launches, int head_counts[3], std::string *err, YxLanes *lanes = nullptr, int n_cu = 0, int infer_counts[4] = nullptr);
// launch sets of the video group's hand-decoder queue (handdec.hip): palm and landmark tensors of independent instances, job tables
constexpr int kHnSetMax = MI355_HANDDEC_SET_MAX;
constexpr size_t kHnCountsBytes = 128;  // a result block: kHnSetMax counts (by job), n x MI355_HAND_MAX box records (by job), then
                                        // MI355_HAND_MAX keypoint records per landmark job (by kp_slot)
struct HnTensor { int decoder; const float *data; uint32_t rows, D; const float *scores; uint32_t num_scores; mi355_hand_params p; };   // decoder 0: palm, 1: landmarks
struct HnSetScratch;  // the result slab of one set, on the device; nothing in it is cleared between sets
// the checks of the hand decoders' entry points that need no device; *why names the refusal
int handdec_check_args(int decoder, size_t tensor_pitch_bytes, int n_tensors, uint32_t rows, uint32_t kps_dim, size_t score_pitch_bytes, uint32_t num_scores,
                       const char **why);
int handdec_check_params(int decoder, uint32_t max_hands, int32_t frame_width, int32_t frame_height, const char **why);
// the layout of one set (mi355_selftest_handdec_set_plan; handdec_plan_set plans the queue's sets with it)
int handdec_set_plan(int n_jobs, const int *decoder, const uint32_t *rows, uint32_t *block, uint32_t *kp_slot, uint64_t totals[4]);
// the plan of one set of the queue: what handdec_set_plan writes, by job. Made ONCE per set: it says whether the set takes a pinned
// block, handdec_launch_set fills its tables with it, and the results are read by its kp_slot.
struct HnSetPlan {
  uint32_t block[kHnSetMax], kp_slot[kHnSetMax];
  uint64_t totals[4];
};
int handdec_plan_set(const HnTensor *tensors, int n, HnSetPlan *out);   // zeroed totals on a refusal
HnSetScratch *handdec_set_scratch_new(int *status, std::string *err);
void handdec_set_scratch_free(HnSetScratch *S);
size_t handdec_set_block_bytes();  // the pinned block a set's results are copied to: the slab's maximum, one size
// n <= kHnSetMax checked tensors and their plan (handdec_plan_set) on `stream`: the palm launch, the landmark launch (each only if it
// has a job with rows), then the slab's used prefix into h_block (nothing launched or copied if no tensor has rows)
int handdec_launch_set(HnSetScratch *S, hipStream_t stream, const HnTensor *tensors, int n, const HnSetPlan &plan, void *h_block, size_t h_block_bytes,
                       int *kernel_launches, std::string *err);
void handdec_set_result(const void *h_block, int n, int i, int decoder, uint32_t rows, uint32_t kp_slot, mi355_hand_det *dets, mi355_hand_keypoints *kps,
                        uint32_t *n_hands);
int dssim_image_plane(mi355_ctx *ctx, const mi355_dssim_image *img, int scale, int channel, int kind, float *out, int *w, int *h);
int hrtf_load_sphere(mi355_ctx *ctx, const unsigned char *bytes, size_t n, uint32_t device_rate);
int hrtf_setup(mi355_ctx *ctx, int channels, int block_len, int steps);
int hrtf_reset(mi355_ctx *ctx);
void hrtf_release(mi355_ctx *ctx);
int hrtf_process_block_device(mi355_ctx *ctx, const float *d_in, float *d_out, const float *positions, const float *gains);
int hrtf_process_block_host(mi355_ctx *ctx, const float *in, float *out, const float *positions, const float *gains);
int hrtf_last_lookup(mi355_ctx *ctx, int *faces, float *uvw);
int hrtf_info(mi355_ctx *ctx, uint32_t *len, uint32_t *vertices, uint32_t *faces);
int hrtf_transform_size(mi355_ctx *ctx, int *fft_n);
// the members of one hrtf agroup (hrtf_kernels.hip): spheres shared by content, one HrtfState per member, the job tables of a launch set
struct HrtfGroup;
struct HrtfSubmit { int member; const float *d_in; float *d_out; const float *positions, *gains; };   // positions [C][3], gains [C]: host
HrtfGroup *hrtf_group_new(int n_members, std::string *err, int *status);
void hrtf_group_free(HrtfGroup *G);
int hrtf_group_load_sphere(HrtfGroup *G, int m, const unsigned char *bytes, size_t n, uint32_t device_rate, std::string *err);
int hrtf_group_setup(HrtfGroup *G, int m, int channels, int block_len, int steps, int method, std::string *err);
int hrtf_group_reset(HrtfGroup *G, int m, hipStream_t stream, std::string *err);
bool hrtf_group_configured(const HrtfGroup *G, int m);
bool hrtf_group_has_sphere(const HrtfGroup *G, int m);
int hrtf_group_channels(const HrtfGroup *G, int m);
size_t hrtf_group_frames(const HrtfGroup *G, int m);
uint64_t hrtf_group_launches(const HrtfGroup *G);
int hrtf_group_info(HrtfGroup *G, int m, uint32_t *hrir_len, int *fft_n, int *spheres_held, std::string *err);
int hrtf_group_last_lookup(HrtfGroup *G, int m, hipStream_t stream, int *faces, float *uvw, std::string *err);
int hrtf_group_run(HrtfGroup *G, hipStream_t stream, const HrtfSubmit *subs, int n, std::string *err);
// the members of one sofa agroup (sofa_kernels.hip): one convolver set per member, the filter queue, the job tables of a launch set
struct SofaGroup;
constexpr int kSofaMaxBlocks = 8;   // whole blocks a member may hand over in one submit (Sofalizer::process takes every whole block its adapter holds)
struct SofaSubmit { int member; const float *d_in; float *d_out; const float *gains; int n_blocks; };   // gains [C]: host
SofaGroup *sofa_group_new(int n_members, std::string *err, int *status);
void sofa_group_free(SofaGroup *G);
int sofa_group_setup(SofaGroup *G, int m, hipStream_t stream, int channels, int filter_len, int partition_len, int block_len, std::string *err);
int sofa_group_set_filter(SofaGroup *G, int m, hipStream_t stream, int channel, const float *left, const float *right, int delay_left, int delay_right,
                          std::string *err);
int sofa_group_set_drop(SofaGroup *G, int m, hipStream_t stream, int channel, int drop, std::string *err);
int sofa_group_reset(SofaGroup *G, int m, hipStream_t stream, std::string *err);
bool sofa_group_configured(const SofaGroup *G, int m);
bool sofa_group_ready(const SofaGroup *G, int m);
int sofa_group_channels(const SofaGroup *G, int m);
int sofa_group_block(const SofaGroup *G, int m);
uint64_t sofa_group_launches(const SofaGroup *G);
int sofa_group_info(const SofaGroup *G, int m, int *partitions_K, int *fft_n, int *pending_filters, std::string *err);
int sofa_group_run(SofaGroup *G, hipStream_t stream, const SofaSubmit *subs, int n, std::string *err);
int sofa_setup(mi355_ctx *ctx, int channels, int filter_len, int partition_len, int block_len);
int sofa_set_filter(mi355_ctx *ctx, int channel, const float *left, const float *right, int delay_left, int delay_right);
int sofa_set_drop(mi355_ctx *ctx, int channel, int drop);
int sofa_reset(mi355_ctx *ctx);
int sofa_process_block_device(mi355_ctx *ctx, const float *d_in, float *d_out, const float *gains);
int sofa_process_block_host(mi355_ctx *ctx, const float *in, float *out, const float *gains);
void sofa_release(mi355_ctx *ctx);
int ebur128_add_frames(mi355_ctx *ctx, const void *data, const void *const *planes, size_t frames, int fmt);
int ebur128_query(mi355_ctx *ctx, int what, double *out);
int ebur128_peak(mi355_ctx *ctx, int true_peak, unsigned channel, double *out);

}  // namespace mi355
