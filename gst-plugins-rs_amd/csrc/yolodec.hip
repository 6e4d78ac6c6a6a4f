// yolodec.hip — the device side of `yolov8tensordec2` / `yoloxtensordec`: the tensor decoder of
// analytics/analytics/src/yolotensordec/imp.rs:234-422 (transform_ip) with `iou` of :480-489. In-tree Rust, pure f32 arithmetic:
// the results are bit-exact against the contract of DESIGN §4.11 (tests/yolodec_restate.py and tools/yolodec_cpu.cpp restate it
// independently). Per tensor of F fields x N candidates:
//   candidates  V8 (:297-327): field f of candidate c is data[c + f * N], classes are fields 4..F-1; X (:328-356): candidate c is
//               the row data[c * F ..], dropped iff b[4] < box_thr, classes are b[5..]. The class is the maximum under
//               f32::total_cmp, the LAST of equal maxima (Iterator::max_by); dropped iff conf < class_thr (IEEE: a NaN stays).
//               X: confidence = b[4] * conf.
//   boxes       xmin = x - w / 2, ymin = y - h / 2, xmax = x + w / 2, ymax = y + h / 2 (:318-323, :347-352), unfused.
//   order       class ascending, confidence descending under total_cmp (:360-364). The reference sorts with sort_unstable_by,
//               which leaves the order of entries of equal class and bit-equal confidence open; HERE IT IS DEFINED: ascending
//               candidate index (what a stable sort gives). This is the one stated deviation.
//   NMS         per class, in that order: a box is kept unless iou(kept_j, box) > iou_thr for an already kept box (:370-385);
//               the kept box is the first operand. A NaN IoU drops nothing.
//   output      kept boxes in class order, within a class in sorted order; x = xmin as i32, y = ymin as i32,
//               width = (xmax - xmin) as i32, height = (ymax - ymin) as i32 (:388-417; `as`: toward zero, saturating, NaN -> 0).
// `max-detections` is a property the reference never reads in transform_ip: it has no effect there and none here.
// Outside the bit-exact contract: sign and payload of a NaN that arithmetic PRODUCES (inf * 0, inf - inf) are the hardware's.
//
//   yolodec_score_kernel<LAYOUT>  grid (candidate tiles, tensors). V8: one lane per candidate walks the class planes (every plane
//                                 row is one coalesced wave load). X: the block's 256 rows go through an LDS tile of 32 fields
//                                 (row stride 33 dwords: lanes of a wave hit distinct banks), loaded by whole waves in 128-byte
//                                 row pieces; one lane per row folds each chunk into its running argmax. Survivors are appended
//                                 to the tensor's key list with one atomic per wave. Key: 11 bits class | 32 bits inverted
//                                 total_cmp key of the confidence | 16 bits candidate - ascending key order is the output order.
//   yolodec_nms_kernel            one block per tensor: bitonic sort of the keys (in LDS up to 4096 keys, in the tensor's global
//                                 scratch above; the same code), class runs found by their boundaries, greedy NMS per run by one
//                                 wave (chunks of 64 sorted boxes, one per lane: tested against all boxes kept before, then
//                                 resolved in order inside the chunk with ballots), prefix sum of the runs' kept counts, records.
//                                 The survivor counter is left at zero for the next call.
//   yolodec_score_jobs_kernel<LAYOUT>, yolodec_nms_jobs_kernel
//                                 the job-table forms for the video group's decoder queue (group.hip): tensors of independent
//                                 instances - own data pointer, F, N, layout, settings, scratch - in at most three launches per
//                                 set. Thin wrappers, as the lone kernels are, around the same device functions (score_tile here;
//                                 sort_keys, find_runs, greedy_nms, write_records in yolodec_device.hpp, which the YOLOX head
//                                 decoder of yolox_head.hip shares).
#include "yolodec_device.hpp"

#include <cstring>
#include <string>

namespace mi355 {

namespace {

constexpr int kXChunk = 32;             // fields of a row in the LDS tile
constexpr int kXStride = kXChunk + 1;   // odd row stride in dwords

// the score work of the 256-candidate tile that starts at candidate c0 (c0 < N), by the whole block: survivors are appended to
// keys[0 .. key_pitch) behind *count. LAYOUT 0: V8, 1: X. Shared by the lone kernel and the job-table kernel.
template <int LAYOUT>
__device__ __forceinline__ void score_tile(const uint32_t *__restrict__ data, uint32_t F, uint32_t N, const mi355_yolo_params &P, uint32_t c0,
                                           uint32_t *__restrict__ count, unsigned long long *__restrict__ keys, size_t key_pitch) {
  const int tid = threadIdx.x;
  const uint32_t c = c0 + (uint32_t)tid;
  const bool valid = c < N;
  int32_t best_key = INT_MIN;   // the smallest key there is: the first class always replaces it
  uint32_t best_bits = 0xffffffffu, best_cls = 0;
  bool keep = valid;
  uint32_t conf_bits = 0;
  if (LAYOUT == 0) {
    const uint32_t C = F - 4;
    if (valid) {
      const uint32_t *__restrict__ col = data + (size_t)4 * N + c;
      uint32_t i = 0;
      for (; i + 4 <= C; i += 4) {
        const uint32_t v0 = col[(size_t)(i + 0) * N], v1 = col[(size_t)(i + 1) * N], v2 = col[(size_t)(i + 2) * N], v3 = col[(size_t)(i + 3) * N];
        fold_class(v0, i + 0, best_key, best_bits, best_cls);
        fold_class(v1, i + 1, best_key, best_bits, best_cls);
        fold_class(v2, i + 2, best_key, best_bits, best_cls);
        fold_class(v3, i + 3, best_key, best_bits, best_cls);
      }
      for (; i < C; i++) fold_class(col[(size_t)i * N], i, best_key, best_bits, best_cls);
      if (__uint_as_float(best_bits) < P.class_confidence_threshold) keep = false;
      conf_bits = best_bits;
    }
  } else {
    __shared__ uint32_t tile[kScoreThreads * kXStride];
    const uint32_t rows = N - c0 < (uint32_t)kScoreThreads ? N - c0 : (uint32_t)kScoreThreads;   // rows of this block: c0 < N by the grid
    const uint32_t *__restrict__ blk = data + (size_t)c0 * F;
    uint32_t obj_bits = 0;
    for (uint32_t f0 = 0; f0 < F; f0 += kXChunk) {
      const uint32_t nf = F - f0 < (uint32_t)kXChunk ? F - f0 : (uint32_t)kXChunk;
      // element e of the chunk: row e / 32, field f0 + e % 32 - a wave loads two 128-byte row pieces per instruction
#pragma unroll 4
      for (uint32_t e = (uint32_t)tid; e < (uint32_t)kScoreThreads * kXChunk; e += kScoreThreads) {
        const uint32_t r = e / kXChunk, j = e % kXChunk;
        if (r < rows && j < nf) tile[r * kXStride + j] = blk[(size_t)r * F + f0 + j];
      }
      __syncthreads();
      if (valid) {
        const uint32_t *row = tile + (uint32_t)tid * kXStride;
        for (uint32_t j = 0; j < nf; j++) {
          const uint32_t f = f0 + j, v = row[j];
          if (f == 4) obj_bits = v;
          else if (f >= 5) fold_class(v, f - 5, best_key, best_bits, best_cls);
        }
      }
      __syncthreads();   // the tile is loaded again
    }
    if (valid) {
      const float obj = __uint_as_float(obj_bits), conf = __uint_as_float(best_bits);
      if (obj < P.box_confidence_threshold) keep = false;
      if (conf < P.class_confidence_threshold) keep = false;
      conf_bits = __float_as_uint(obj * conf);
    }
  }
  append_keys(keep, make_key(best_cls, conf_bits, c), count, keys, key_pitch);
}

// keys: [tensors][key_pitch], count: [tensors], zero on entry
template <int LAYOUT>
__global__ __launch_bounds__(kScoreThreads) void yolodec_score_kernel(const uint32_t *__restrict__ tensors, size_t pitch_dwords, uint32_t F, uint32_t N,
                                                                       const mi355_yolo_params *__restrict__ params, uint32_t *__restrict__ count,
                                                                       unsigned long long *__restrict__ keys, size_t key_pitch) {
  const uint32_t t = blockIdx.y;
  const mi355_yolo_params P = params[t];
  score_tile<LAYOUT>(tensors + (size_t)t * pitch_dwords, F, N, P, blockIdx.x * kScoreThreads, count + t, keys + (size_t)t * key_pitch, key_pitch);
}

template <int LAYOUT>
__device__ __forceinline__ Box load_box(const float *__restrict__ data, uint32_t F, uint32_t N, uint32_t c) {
  float x, y, w, h;
  if (LAYOUT == 0) {
    x = data[c];
    y = data[(size_t)N + c];
    w = data[(size_t)2 * N + c];
    h = data[(size_t)3 * N + c];
  } else {
    const float *b = data + (size_t)c * F;
    x = b[0];
    y = b[1];
    w = b[2];
    h = b[3];
  }
  return centre_box(x, y, w, h);
}

// LAYOUT 0: V8, 1: X, 2: `layout` decides (block-uniform: the job-table kernel)
template <int LAYOUT>
__device__ __forceinline__ Box load_box_of(int layout, const float *__restrict__ data, uint32_t F, uint32_t N, uint32_t c) {
  if (LAYOUT == 2) return layout == MI355_YOLO_V8 ? load_box<0>(data, F, N, c) : load_box<1>(data, F, N, c);
  return load_box<LAYOUT == 2 ? 0 : LAYOUT>(data, F, N, c);
}

// the box loader nms_block takes: the candidate's box from the tensor
template <int LAYOUT>
struct TensorBoxes {
  int layout;
  const float *__restrict__ data;
  uint32_t F, N;
  __device__ __forceinline__ Box operator()(uint32_t c) const { return load_box_of<LAYOUT>(layout, data, F, N, c); }
};

// kbox / ksrc: [tensors][N]
template <int LAYOUT>
__global__ __launch_bounds__(kNmsThreads) void yolodec_nms_kernel(const float *__restrict__ tensors, size_t pitch_dwords, uint32_t F, uint32_t N,
                                                                   const mi355_yolo_params *__restrict__ params, uint32_t *__restrict__ count,
                                                                   unsigned long long *__restrict__ keys, size_t key_pitch, float4 *__restrict__ kbox,
                                                                   uint32_t *__restrict__ ksrc, mi355_yolo_det *__restrict__ dets, uint32_t max_dets,
                                                                   uint32_t *__restrict__ n_dets) {
  __shared__ unsigned long long lds_keys[kLdsSortKeys];
  __shared__ NmsShared S;
  const uint32_t t = blockIdx.x;
  const TensorBoxes<LAYOUT> boxes = {LAYOUT, tensors + (size_t)t * pitch_dwords, F, N};
  nms_block(boxes, LAYOUT == 0 ? F - 4 : F - 5, N, params[t].iou_threshold, count + t, keys + (size_t)t * key_pitch, kbox + (size_t)t * N, ksrc + (size_t)t * N,
            dets + (size_t)t * max_dets, max_dets, n_dets + t, lds_keys, S);
}

// ---- job-table forms (the video group's decoder queue): tensors of independent instances - own data pointer, shape, layout, settings,
// scratch - in one launch. The table is passed in the kernel arguments; every field a block reads is block-uniform.
struct YdJob {
  const float *data;
  uint32_t *count;              // the job's survivor counter; zero on entry to the score launch, left at zero by the NMS launch
  unsigned long long *keys;     // key_cap entries
  float4 *kbox;                 // N entries
  uint32_t *ksrc;               // N entries
  mi355_yolo_det *dets;         // min(max_dets, N) records
  uint32_t *n_dets;
  uint32_t F, N, key_cap, max_dets;
  uint32_t first_block, blocks; // its tiles in the score launch of its layout (yolodec_mixed_set_plan)
  int32_t layout;
  mi355_yolo_params p;
};
struct YdJobTable {
  YdJob job[kYdSetMax];
  int32_t n_jobs, pad;
};
static_assert(sizeof(YdJob) == 96, "YdJob has no padding holes");
static_assert(sizeof(YdJobTable) <= 4096, "the job table is passed in the kernel arguments");

// one flat grid over the tiles of the jobs of one layout: jobs are in first_block order and every job of a table has a block
template <int LAYOUT>
__global__ __launch_bounds__(kScoreThreads) void yolodec_score_jobs_kernel(const YdJobTable T) {
  int j = 0;
  while (j + 1 < T.n_jobs && blockIdx.x >= T.job[j].first_block + T.job[j].blocks) j++;
  const uint32_t rel = blockIdx.x - T.job[j].first_block;
  if (blockIdx.x < T.job[j].first_block || rel >= T.job[j].blocks) return;   // a grid larger than the plan's total: the whole block leaves, before any barrier
  const mi355_yolo_params P = T.job[j].p;
  score_tile<LAYOUT>(reinterpret_cast<const uint32_t *>(T.job[j].data), T.job[j].F, T.job[j].N, P, rel * kScoreThreads, T.job[j].count, T.job[j].keys,
                     (size_t)T.job[j].key_cap);
}

// one block per job with candidates, whatever its layout
__global__ __launch_bounds__(kNmsThreads) void yolodec_nms_jobs_kernel(const YdJobTable T) {
  __shared__ unsigned long long lds_keys[kLdsSortKeys];
  __shared__ NmsShared S;
  const int j = (int)blockIdx.x;
  if (j >= T.n_jobs) return;
  const TensorBoxes<2> boxes = {T.job[j].layout, T.job[j].data, T.job[j].F, T.job[j].N};
  nms_block(boxes, T.job[j].layout == MI355_YOLO_V8 ? T.job[j].F - 4 : T.job[j].F - 5, T.job[j].N, T.job[j].p.iou_threshold, T.job[j].count, T.job[j].keys,
            T.job[j].kbox, T.job[j].ksrc, T.job[j].dets, T.job[j].max_dets, T.job[j].n_dets, lds_keys, S);
}

}  // namespace

void yolodec_release(mi355_ctx *ctx) {
  delete static_cast<YoloDecState *>(ctx->yolodec);
  ctx->yolodec = nullptr;
}

// the checks that need no device (both entry points; mi355_selftest_yolodec_check)
int yolodec_check_args(size_t tensor_pitch_bytes, int n_tensors, int layout, uint32_t num_fields, uint32_t num_candidates, const char **why) {
  *why = nullptr;
  if (layout != MI355_YOLO_V8 && layout != MI355_YOLO_X) *why = "yolodec: layout is neither MI355_YOLO_V8 nor MI355_YOLO_X";
  else if (num_fields < 6) *why = "yolodec: fewer than 6 fields (box, box confidence, one class)";
  else if (n_tensors < 1) *why = "yolodec: n_tensors must be at least 1";
  if (*why) return MI355_ERR_INVALID_ARG;
  if (num_fields > kMaxFields) *why = "yolodec: more than 1029 fields";
  else if (num_candidates > kMaxCandidates) *why = "yolodec: more than 65536 candidates";
  else if ((uint32_t)n_tensors > kMaxTensors) *why = "yolodec: more than 1024 tensors";
  if (*why) return MI355_ERR_UNSUPPORTED;
  if (tensor_pitch_bytes % 4 != 0 || tensor_pitch_bytes < (size_t)num_fields * num_candidates * 4) {
    *why = "yolodec: tensor pitch is smaller than the tensor or no multiple of 4";
    return MI355_ERR_INVALID_ARG;
  }
  return MI355_OK;
}

static size_t out_counts_bytes(uint32_t T) { return ((size_t)T * sizeof(uint32_t) + 63) / 64 * 64; }

int yolodec_scratch(mi355_ctx *ctx, uint32_t T, uint32_t N, uint32_t max_dets, YoloDecState **out) {
  auto *s = static_cast<YoloDecState *>(ctx->yolodec);
  if (!s) ctx->yolodec = s = new YoloDecState();
  bool fresh = false;
  int rc = check_hip(ctx, s->d_count.reserve(T, &fresh), "hipMalloc(yolodec counters)");
  if (fresh) s->count_zero = false;
  if (rc) return rc;
  // the settings are sized by the counters' T (>= this call's), whichever call set it: the three grow together
  if ((rc = check_hip(ctx, s->d_params.reserve(s->d_count.n), "hipMalloc(yolodec settings)"))) return rc;
  if ((rc = check_hip(ctx, s->h_params.reserve(s->d_count.n), "hipHostMalloc(yolodec settings)"))) return rc;
  const size_t key_pitch = pow2_at_least(N);
  if ((rc = check_hip(ctx, s->d_keys.reserve((size_t)T * key_pitch), "hipMalloc(yolodec keys)"))) return rc;
  if ((rc = check_hip(ctx, s->d_kbox.reserve((size_t)T * N), "hipMalloc(yolodec kept boxes)"))) return rc;
  if ((rc = check_hip(ctx, s->d_ksrc.reserve((size_t)T * N), "hipMalloc(yolodec kept positions)"))) return rc;
  const size_t out_bytes = out_counts_bytes(T) + (size_t)T * max_dets * sizeof(mi355_yolo_det);
  if ((rc = check_hip(ctx, s->d_out.reserve(out_bytes), "hipMalloc(yolodec results)"))) return rc;
  if ((rc = check_hip(ctx, s->h_out.reserve(out_bytes), "hipHostMalloc(yolodec results)"))) return rc;
  if (!s->count_zero) {
    if ((rc = check_hip(ctx, hipMemsetAsync(s->d_count.p, 0, s->d_count.n * sizeof(uint32_t), ctx->stream), "hipMemsetAsync(yolodec)"))) return rc;
    s->count_zero = true;
  }
  *out = s;
  return MI355_OK;
}

int yolodec_stage(mi355_ctx *ctx, YoloDecState *s, size_t floats) { return check_hip(ctx, s->d_stage.reserve(floats), "hipMalloc(yolodec staging)"); }

int yolodec_upload_params(mi355_ctx *ctx, YoloDecState *s, uint32_t T, const mi355_yolo_params *p) {
  std::memcpy(s->h_params.p, p, (size_t)T * sizeof(mi355_yolo_params));
  const int rc = check_hip(ctx, hipMemcpyAsync(s->d_params.p, s->h_params.p, (size_t)T * sizeof(mi355_yolo_params), hipMemcpyHostToDevice, ctx->stream), "yolodec settings H2D");
  if (rc) return rc;
  __atomic_fetch_add(&ctx->n_h2d, 1ull, __ATOMIC_RELAXED);
  return MI355_OK;
}

mi355_yolo_det *yolodec_d_dets(YoloDecState *s, uint32_t T) { return reinterpret_cast<mi355_yolo_det *>(s->d_out.p + out_counts_bytes(T)); }

int yolodec_download(mi355_ctx *ctx, YoloDecState *s, uint32_t T, mi355_yolo_det *dets, uint32_t max_dets, uint32_t *n_dets) {
  int rc = MI355_OK;
  const size_t bytes = out_counts_bytes(T) + (size_t)T * max_dets * sizeof(mi355_yolo_det);
  if ((rc = check_hip(ctx, hipMemcpyAsync(s->h_out.p, s->d_out.p, bytes, hipMemcpyDeviceToHost, ctx->stream), "yolodec D2H"))) return rc;
  __atomic_fetch_add(&ctx->n_d2h, 1ull, __ATOMIC_RELAXED);
  if ((rc = check_hip(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize"))) return rc;
  s->count_zero = true;
  const uint32_t *h_n = reinterpret_cast<const uint32_t *>(s->h_out.p);
  const mi355_yolo_det *h_dets = reinterpret_cast<const mi355_yolo_det *>(s->h_out.p + out_counts_bytes(T));
  for (uint32_t t = 0; t < T; t++) {
    n_dets[t] = h_n[t];
    const uint32_t w = h_n[t] < max_dets ? h_n[t] : max_dets;
    if (w) std::memcpy(dets + (size_t)t * max_dets, h_dets + (size_t)t * max_dets, (size_t)w * sizeof(mi355_yolo_det));
  }
  return MI355_OK;
}

// settings up, the two launches, results down, one synchronisation; d_tensors is checked
static int yolodec_run(mi355_ctx *ctx, YoloDecState *s, const float *d_tensors, size_t pitch_bytes, uint32_t T, int layout, uint32_t F, uint32_t N,
                       const mi355_yolo_params *p, mi355_yolo_det *dets, uint32_t max_dets, uint32_t *n_dets) {
  int rc = MI355_OK;
  if ((rc = yolodec_upload_params(ctx, s, T, p))) return rc;
  const size_t key_pitch = pow2_at_least(N), pitch_dwords = pitch_bytes / 4;
  uint32_t *d_n = yolodec_d_counts(s);
  mi355_yolo_det *d_dets = yolodec_d_dets(s, T);
  const dim3 grid((N + kScoreThreads - 1) / kScoreThreads, T);
  s->count_zero = false;   // true again only once the NMS kernel has been enqueued behind the score kernel
  if (layout == MI355_YOLO_V8)
    hipLaunchKernelGGL(yolodec_score_kernel<0>, grid, dim3(kScoreThreads), 0, ctx->stream, reinterpret_cast<const uint32_t *>(d_tensors), pitch_dwords, F, N,
                       s->d_params.p, s->d_count.p, s->d_keys.p, key_pitch);
  else
    hipLaunchKernelGGL(yolodec_score_kernel<1>, grid, dim3(kScoreThreads), 0, ctx->stream, reinterpret_cast<const uint32_t *>(d_tensors), pitch_dwords, F, N,
                       s->d_params.p, s->d_count.p, s->d_keys.p, key_pitch);
  if ((rc = check_hip(ctx, hipGetLastError(), "yolodec score launch"))) return rc;
  if (layout == MI355_YOLO_V8)
    hipLaunchKernelGGL(yolodec_nms_kernel<0>, dim3(T), dim3(kNmsThreads), 0, ctx->stream, d_tensors, pitch_dwords, F, N, s->d_params.p, s->d_count.p, s->d_keys.p, key_pitch,
                       s->d_kbox.p, s->d_ksrc.p, d_dets, max_dets, d_n);
  else
    hipLaunchKernelGGL(yolodec_nms_kernel<1>, dim3(T), dim3(kNmsThreads), 0, ctx->stream, d_tensors, pitch_dwords, F, N, s->d_params.p, s->d_count.p, s->d_keys.p, key_pitch,
                       s->d_kbox.p, s->d_ksrc.p, d_dets, max_dets, d_n);
  if ((rc = check_hip(ctx, hipGetLastError(), "yolodec nms launch"))) return rc;
  return yolodec_download(ctx, s, T, dets, max_dets, n_dets);
}

// ---- launch sets of the video group's decoder queue

// the layout of one set (the two selftest exports; yolodec_plan_set plans the queue's sets with it): a tensor job's tiles run in the
// score launch of its layout, a head job is a job of A candidates whose tiles run level by level in a launch of the heads' own
int yolodec_mixed_set_plan(int n_jobs, const int *kind, const uint32_t *num_fields, const uint32_t *num_candidates, const uint32_t *max_dets, const int *n_levels,
                           const uint32_t *level_h, const uint32_t *level_w, uint32_t *candidates, uint32_t *first_block, uint32_t *blocks, uint64_t *key_offset,
                           uint64_t *box_offset, uint64_t *det_offset, uint32_t *level_first_block, uint64_t totals[8]) {
  if (n_jobs < 0 || n_jobs > kYdSetMax || !totals) return MI355_ERR_INVALID_ARG;
  if (n_jobs > 0 && (!kind || !num_fields || !num_candidates || !max_dets || !candidates || !first_block || !blocks || !key_offset || !box_offset || !det_offset))
    return MI355_ERR_INVALID_ARG;
  size_t at = 0;   // levels read so far
  for (int j = 0; j < n_jobs; j++) {
    const char *why = nullptr;
    if (kind[j] != MI355_YOLO_X_HEAD) {
      if (const int rc = yolodec_check_args((size_t)num_fields[j] * num_candidates[j] * 4, 1, kind[j], num_fields[j], num_candidates[j], &why)) return rc;
      candidates[j] = num_candidates[j];
      continue;
    }
    if (!n_levels || !level_h || !level_w || !level_first_block) return MI355_ERR_INVALID_ARG;
    mi355_yolox_level lv[MI355_YOLOX_LEVELS_MAX] = {};
    for (int l = 0; l < n_levels[j] && l < MI355_YOLOX_LEVELS_MAX; l++) {
      lv[l].h = level_h[at + (size_t)l];
      lv[l].w = level_w[at + (size_t)l];
      lv[l].stride = 1;   // no part of the layout
    }
    if (const int rc = yolox_head_check_shape(lv, n_levels[j], 1, num_fields[j] < 5 ? 0 : num_fields[j] - 5, &candidates[j], &why)) return rc;
    at += (size_t)n_levels[j];
  }
  uint64_t t[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // V8 blocks, X blocks, jobs with a candidate, keys, boxes, records, head blocks, level jobs
  at = 0;
  for (int j = 0; j < n_jobs; j++) {
    const uint32_t N = candidates[j];
    if (kind[j] == MI355_YOLO_X_HEAD) {
      first_block[j] = (uint32_t)t[6];
      uint32_t b = 0;
      for (int l = 0; l < n_levels[j]; l++, at++) {
        level_first_block[at] = b;
        b += (level_h[at] * level_w[at] + kScoreThreads - 1) / kScoreThreads;
      }
      blocks[j] = b;
      t[6] += b;
      t[7] += (uint64_t)n_levels[j];
    } else {
      uint64_t &layout_blocks = t[kind[j] == MI355_YOLO_V8 ? 0 : 1];
      blocks[j] = (N + kScoreThreads - 1) / kScoreThreads;
      first_block[j] = (uint32_t)layout_blocks;   // at most 32 * 256 blocks
      layout_blocks += blocks[j];
    }
    if (N) t[2]++;
    key_offset[j] = t[3];
    t[3] += pow2_at_least(N);
    box_offset[j] = t[4];
    t[4] += N;
    det_offset[j] = t[5];
    t[5] += max_dets[j] < N ? max_dets[j] : N;
  }
  for (int k = 0; k < 8; k++) totals[k] = t[k];
  return MI355_OK;
}

// scratch of one queue; grows to the largest set seen
struct YdSetScratch {
  DeviceBuf<uint32_t> d_count;   // [kYdSetMax] survivors; zero between sets
  bool count_zero = false;       // false after the allocation or an interrupted set: cleared before the next launch
  DeviceBuf<unsigned long long> d_keys;
  DeviceBuf<float4> d_kbox;
  DeviceBuf<uint32_t> d_ksrc;
  DeviceBuf<uint8_t> d_out;      // [kYdSetMax] counts (kYdCountsBytes), then the jobs' records at their det_offset
  DeviceBuf<uint8_t> d_table;    // the head members' tables (a YhTable) of the set that runs and, behind its level jobs, the infer members'
                                 // conversion jobs: kYhUploadMax bytes, made with the first set that holds a head or an infer member
};

YdSetScratch *yolodec_set_scratch_new(int *status, std::string *err) {
  auto *S = new YdSetScratch();
  bool fresh = false;
  const hipError_t e = S->d_count.reserve((size_t)kYdSetMax, &fresh);
  if (fresh) S->count_zero = false;   // new counters hold anything
  if (e != hipSuccess) {
    delete S;
    *status = MI355_ERR_OUT_OF_MEMORY;
    *err = "hipMalloc(yolodec set counters)";
    return nullptr;
  }
  *status = MI355_OK;
  return S;
}

void yolodec_set_scratch_free(YdSetScratch *S) { delete S; }

size_t yolodec_set_result_bytes(uint64_t records) { return kYdCountsBytes + (size_t)records * sizeof(mi355_yolo_det); }

// where the head tables stand in a set's pinned block: behind its results, which the download writes
static size_t set_table_offset(uint64_t records) { return (yolodec_set_result_bytes(records) + 63) / 64 * 64; }

size_t yolodec_set_block_bytes(uint64_t records, uint64_t level_jobs, uint64_t infer_jobs) {
  return level_jobs ? set_table_offset(records) + yh_upload_bytes(level_jobs, infer_jobs) : yolodec_set_result_bytes(records);
}

// the one place a set's members become the plan's arrays
int yolodec_plan_set(const YdTensor *tensors, int n, YdSetPlan *out) {
  for (uint64_t &t : out->totals) t = 0;
  if (!tensors || n < 0 || n > kYdSetMax) return MI355_ERR_INVALID_ARG;
  for (uint64_t &t : out->infer_totals) t = 0;
  int member[kYdSetMax], kind[kYdSetMax], n_levels[kYdSetMax];
  uint32_t F[kYdSetMax], cap[kYdSetMax], lv_h[kYhLevelJobsMax], lv_w[kYhLevelJobsMax], in_h[kYdSetMax], in_w[kYdSetMax];
  uint64_t net_key[kYdSetMax];
  size_t n_lv = 0;
  for (int i = 0; i < n; i++) {
    const YdTensor &t = tensors[i];
    member[i] = t.layout; F[i] = t.num_fields; out->candidates[i] = t.num_candidates; cap[i] = t.max_dets;
    net_key[i] = 0; in_h[i] = in_w[i] = 0;
    if (member[i] == MI355_YOLO_X_HEAD && !t.head) return MI355_ERR_INVALID_ARG;
    if (member[i] == MI355_YOLO_X_INFER) {
      // the decode side of an infer member: a head of the three levels of its frame size
      if (!t.infer) return MI355_ERR_INVALID_ARG;
      net_key[i] = t.infer->serial; in_h[i] = t.infer->height; in_w[i] = t.infer->width;
      kind[i] = MI355_YOLO_X_HEAD;
      n_levels[i] = 3;
      for (int l = 0; l < 3; l++, n_lv++) { lv_h[n_lv] = in_h[i] >> (3 + l); lv_w[n_lv] = in_w[i] >> (3 + l); }
      continue;
    }
    kind[i] = member[i];
    n_levels[i] = kind[i] == MI355_YOLO_X_HEAD ? t.head->n_levels : 0;
    if (n_levels[i] < 0 || n_levels[i] > MI355_YOLOX_LEVELS_MAX) return MI355_ERR_INVALID_ARG;
    for (int l = 0; l < n_levels[i]; l++, n_lv++) { lv_h[n_lv] = t.head->lv[l].h; lv_w[n_lv] = t.head->lv[l].w; }
  }
  if (const int rc = yolox_infer_set_plan(n, member, net_key, in_h, in_w, out->class_of, out->frame_in_class, out->conv_first_block, out->conv_blocks, out->class_frames,
                                          out->infer_totals))
    return rc;
  return yolodec_mixed_set_plan(n, kind, F, out->candidates, cap, n_levels, lv_h, lv_w, out->candidates, out->first_block, out->blocks, out->key_off, out->box_off,
                                out->det_off, out->level_first_block, out->totals);
}

int yolodec_launch_set(YdSetScratch *S, hipStream_t stream, const YdTensor *tensors, int n, const YdSetPlan &P, void *h_block, size_t h_block_bytes,
                       int *kernel_launches, int head_counts[3], std::string *err, YxLanes *lanes, int n_cu, int infer_counts[4]) {
  *kernel_launches = 0;
  head_counts[0] = head_counts[1] = head_counts[2] = 0;
  if (infer_counts) infer_counts[0] = infer_counts[1] = infer_counts[2] = infer_counts[3] = 0;
  if (!S || !tensors || n < 1 || n > kYdSetMax) { *err = "yolodec: bad launch set"; return MI355_ERR_INVALID_ARG; }
  const uint64_t *totals = P.totals;
  if (totals[2] == 0) return MI355_OK;   // no job has a candidate: nothing to launch, nothing to copy
  const uint32_t n_classes = (uint32_t)P.infer_totals[0], n_infer = (uint32_t)P.infer_totals[1];
  if (n_infer && (!lanes || !infer_counts)) { *err = "yolodec: a set with infer members and no lanes"; return MI355_ERR_INVALID_ARG; }
  const size_t bytes = yolodec_set_result_bytes(totals[5]), table_bytes = yh_upload_bytes(totals[7], n_infer);
  if (!h_block || h_block_bytes < yolodec_set_block_bytes(totals[5], totals[7], n_infer)) { *err = "yolodec: the pinned block is too small for the set"; return MI355_ERR_INVALID_ARG; }
  // (growing frees first, which waits for the device: a set still running on the queue's stream has finished with the old allocation)
  if (S->d_keys.reserve((size_t)totals[3]) != hipSuccess || S->d_kbox.reserve((size_t)totals[4]) != hipSuccess ||
      S->d_ksrc.reserve((size_t)totals[4]) != hipSuccess || S->d_out.reserve(bytes) != hipSuccess ||
      (table_bytes && S->d_table.reserve(kYhUploadMax) != hipSuccess)) {
    *err = "hipMalloc(yolodec set scratch)";
    return MI355_ERR_OUT_OF_MEMORY;
  }
  if (!S->count_zero) {
    if (hipMemsetAsync(S->d_count.p, 0, (size_t)kYdSetMax * sizeof(uint32_t), stream) != hipSuccess) { *err = "hipMemsetAsync(yolodec set counters)"; return MI355_ERR_HIP; }
    S->count_zero = true;
  }
  YdJobTable score[2] = {}, nms = {};
  YhTable *heads = table_bytes ? reinterpret_cast<YhTable *>(static_cast<uint8_t *>(h_block) + set_table_offset(totals[5])) : nullptr;
  const YhTable *d_heads = reinterpret_cast<const YhTable *>(S->d_table.p);
  YxConvJob *conv = n_infer ? reinterpret_cast<YxConvJob *>(reinterpret_cast<uint8_t *>(heads) + yx_conv_offset(totals[7])) : nullptr;
  const YxConvJob *d_conv = n_infer ? reinterpret_cast<const YxConvJob *>(S->d_table.p + yx_conv_offset(totals[7])) : nullptr;
  // the lanes of the set's classes, before anything is enqueued: a lane that grows frees first, which waits for the device
  const YdInfer *class_first[kYdSetMax] = {};
  float *class_input[kYdSetMax] = {};
  mi355_yolox_level class_lv[kYdSetMax][3];
  for (int i = 0; i < n && n_infer; i++) {
    const int c = P.class_of[i];
    if (c < 0 || class_first[c]) continue;
    class_first[c] = tensors[i].infer.get();
    if (const int lrc = yolox_lanes_prepare(lanes, class_first[c]->net, P.class_frames[c], class_first[c]->height, class_first[c]->width, &class_input[c], class_lv[c], err))
      return lrc;
  }
  uint32_t n_heads = 0, n_level_jobs = 0, n_conv = 0;
  uint32_t *d_n = reinterpret_cast<uint32_t *>(S->d_out.p);
  mi355_yolo_det *d_dets = reinterpret_cast<mi355_yolo_det *>(S->d_out.p + kYdCountsBytes);
  for (int i = 0; i < n; i++) {
    const YdTensor &t = tensors[i];
    const uint32_t N = P.candidates[i];
    if (!N) continue;   // no candidate: no job
    if (t.layout == MI355_YOLO_X_HEAD || t.layout == MI355_YOLO_X_INFER) {
      mi355_yolox_level own[3];
      if (t.layout == MI355_YOLO_X_INFER) {
        // its frame of its class's lane: the conversion writes the input tensor there, the forward the level buffers
        const int c = P.class_of[i];
        const uint32_t f = P.frame_in_class[i];
        const YdInfer &I = *t.infer;
        YxConvJob &K = conv[n_conv++];
        K.src = I.frame;
        K.dst = class_input[c] + (size_t)f * 3 * I.height * I.width;
        K.stride = I.stride;
        K.W = I.width;
        K.H = I.height;
        K.first_block = P.conv_first_block[i];
        K.pad = 0;
        for (int l = 0; l < 3; l++) {
          own[l] = class_lv[c][l];
          const size_t at = (size_t)f * (own[l].reg_pitch_bytes / 4);
          own[l].reg += at, own[l].obj += at, own[l].cls += at;
        }
      }
      const mi355_yolox_level *lv = t.layout == MI355_YOLO_X_INFER ? own : t.head->lv;
      const int n_levels = t.layout == MI355_YOLO_X_INFER ? 3 : t.head->n_levels;   // the plan stands: the head has its levels
      YhHeadJob &H = heads->head[n_heads];
      H.count = S->d_count.p + i;
      H.keys = S->d_keys.p + P.key_off[i];
      H.kbox = S->d_kbox.p + P.box_off[i];
      H.ksrc = S->d_ksrc.p + P.box_off[i];
      H.dets = d_dets + P.det_off[i];
      H.n_dets = d_n + i;
      H.A = N;
      H.C = t.num_fields - 5;
      H.key_cap = pow2_at_least(N);
      H.max_dets = t.max_dets;
      H.first_level = n_level_jobs;
      H.n_levels = (uint32_t)n_levels;
      H.p = t.p;
      H.pad = 0;
      uint32_t a = 0;
      for (int l = 0; l < MI355_YOLOX_LEVELS_MAX; l++) {
        H.start[l] = a;   // A from n_levels on
        if (l >= n_levels) continue;
        const mi355_yolox_level &v = lv[l];
        YhLevelJob &L = heads->level[n_level_jobs];
        L.reg = v.reg;
        L.obj = v.obj;
        L.cls = v.cls;
        L.w = v.w;
        L.hw = v.h * v.w;
        L.first_cand = a;
        L.first_block = P.first_block[i] + P.level_first_block[n_level_jobs];   // the level jobs of a set are in the order of the plan's levels
        L.head = n_heads;
        L.stride = (float)v.stride;   // <= 65536: exact
        a += L.hw;
        n_level_jobs++;
      }
      n_heads++;
      continue;
    }
    YdJob J;
    J.data = t.data;
    J.count = S->d_count.p + i;
    J.keys = S->d_keys.p + P.key_off[i];
    J.kbox = S->d_kbox.p + P.box_off[i];
    J.ksrc = S->d_ksrc.p + P.box_off[i];
    J.dets = d_dets + P.det_off[i];
    J.n_dets = d_n + i;
    J.F = t.num_fields;
    J.N = N;
    J.key_cap = pow2_at_least(N);
    J.max_dets = t.max_dets;
    J.first_block = P.first_block[i];
    J.blocks = P.blocks[i];
    J.layout = t.layout;
    J.p = t.p;
    YdJobTable &T = score[t.layout == MI355_YOLO_V8 ? 0 : 1];
    T.job[T.n_jobs++] = J;
    nms.job[nms.n_jobs++] = J;
  }
  hipError_t e = hipSuccess;
  if (n_heads) {
    // the tables of all heads of the set, one copy: what the launches below read stands in device memory behind it
    e = hipMemcpyAsync(S->d_table.p, heads, table_bytes, hipMemcpyHostToDevice, stream);
    if (e != hipSuccess) { *err = std::string("yolodec set head tables H2D: ") + hipGetErrorString(e); return MI355_ERR_HIP; }
    head_counts[1] = 1;
  }
  if (n_infer) {
    // every infer member's frame in one launch, then one forward per class: the level buffers the head launches below read
    int made = 0;
    if (const int crc = yolox_input_launch_jobs(stream, d_conv, n_conv, (uint32_t)P.infer_totals[2], &made, err)) return crc;
    for (uint32_t c = 0; c < n_classes; c++) {
      if (const int frc = yolox_lanes_forward(lanes, class_first[c]->net, P.class_frames[c], class_first[c]->height, class_first[c]->width, stream, n_cu, &made, err))
        return frc;
      if ((int)P.class_frames[c] > infer_counts[2]) infer_counts[2] = (int)P.class_frames[c];
    }
    infer_counts[0] = (int)n_infer;
    infer_counts[1] = (int)n_classes;
    infer_counts[3] = made;
    *kernel_launches += made;
  }
  S->count_zero = false;   // true again only once the NMS launches have been enqueued behind the score launches
  for (int l = 0; l < 2; l++) {
    if (!score[l].n_jobs) continue;
    const dim3 grid((uint32_t)totals[l]);
    if (l == 0) hipLaunchKernelGGL(yolodec_score_jobs_kernel<0>, grid, dim3(kScoreThreads), 0, stream, score[l]);
    else hipLaunchKernelGGL(yolodec_score_jobs_kernel<1>, grid, dim3(kScoreThreads), 0, stream, score[l]);
    e = hipGetLastError();
    if (e != hipSuccess) { *err = std::string("yolodec score jobs kernel launch: ") + hipGetErrorString(e); return MI355_ERR_HIP; }
    (*kernel_launches)++;
  }
  if (nms.n_jobs) {
    hipLaunchKernelGGL(yolodec_nms_jobs_kernel, dim3((uint32_t)nms.n_jobs), dim3(kNmsThreads), 0, stream, nms);
    e = hipGetLastError();
    if (e != hipSuccess) { *err = std::string("yolodec nms jobs kernel launch: ") + hipGetErrorString(e); return MI355_ERR_HIP; }
    (*kernel_launches)++;
  }
  if (n_heads) {
    // (a launch of their own: merged into the tensors' NMS kernel, the head loader's registers would be every tensor job's)
    if (const int hrc = yolox_head_launch_jobs(stream, d_heads, n_heads, n_level_jobs, (uint32_t)totals[6], &head_counts[2], err)) return hrc;
    *kernel_launches += head_counts[2];
    head_counts[0] = (int)n_heads;
  }
  S->count_zero = true;
  e = hipMemcpyAsync(h_block, S->d_out.p, bytes, hipMemcpyDeviceToHost, stream);
  if (e != hipSuccess) { *err = std::string("yolodec set D2H: ") + hipGetErrorString(e); return MI355_ERR_HIP; }
  return MI355_OK;
}

}  // namespace mi355

using namespace mi355;

extern "C" {

int mi355_yolodec_tensors_device(mi355_ctx *ctx, const float *d_tensors, size_t tensor_pitch_bytes, int n_tensors, int layout, uint32_t num_fields,
                                 uint32_t num_candidates, const mi355_yolo_params *p, mi355_yolo_det *dets, uint32_t max_dets, uint32_t *n_dets) {
  if (!ctx) return MI355_ERR_INVALID_ARG;
  const char *why = nullptr;
  int rc = yolodec_check_args(tensor_pitch_bytes, n_tensors, layout, num_fields, num_candidates, &why);
  if (rc) return set_error(ctx, rc, why);
  if (!p || !n_dets || (max_dets && !dets)) return set_error(ctx, MI355_ERR_INVALID_ARG, "yolodec: null settings or result arrays");
  if (num_candidates == 0) {
    for (int t = 0; t < n_tensors; t++) n_dets[t] = 0;
    return MI355_OK;
  }
  if (!d_tensors || (uintptr_t)d_tensors % 4 != 0) return set_error(ctx, MI355_ERR_INVALID_ARG, "yolodec: null or misaligned tensors");
  if ((rc = check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice"))) return rc;
  YoloDecState *s = nullptr;
  if ((rc = yolodec_scratch(ctx, (uint32_t)n_tensors, num_candidates, max_dets, &s))) return rc;
  return yolodec_run(ctx, s, d_tensors, tensor_pitch_bytes, (uint32_t)n_tensors, layout, num_fields, num_candidates, p, dets, max_dets, n_dets);
}

int mi355_yolodec_tensor(mi355_ctx *ctx, const float *data, int layout, uint32_t num_fields, uint32_t num_candidates, const mi355_yolo_params *p,
                         mi355_yolo_det *dets, uint32_t max_dets, uint32_t *n_dets) {
  if (!ctx) return MI355_ERR_INVALID_ARG;
  const char *why = nullptr;
  const size_t bytes = (size_t)num_fields * num_candidates * 4;
  int rc = yolodec_check_args(bytes, 1, layout, num_fields, num_candidates, &why);
  if (rc) return set_error(ctx, rc, why);
  if (!p || !n_dets || (max_dets && !dets)) return set_error(ctx, MI355_ERR_INVALID_ARG, "yolodec: null settings or result arrays");
  if (num_candidates == 0) {
    *n_dets = 0;
    return MI355_OK;
  }
  if (!data) return set_error(ctx, MI355_ERR_INVALID_ARG, "yolodec: null tensor");
  if ((rc = check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice"))) return rc;
  YoloDecState *s = nullptr;
  if ((rc = yolodec_scratch(ctx, 1, num_candidates, max_dets, &s))) return rc;
  if ((rc = yolodec_stage(ctx, s, bytes / 4))) return rc;
  if ((rc = check_hip(ctx, hipMemcpyAsync(s->d_stage.p, data, bytes, hipMemcpyHostToDevice, ctx->stream), "yolodec H2D"))) return rc;
  __atomic_fetch_add(&ctx->n_h2d, 1ull, __ATOMIC_RELAXED);
  return yolodec_run(ctx, s, s->d_stage.p, bytes, 1, layout, num_fields, num_candidates, p, dets, max_dets, n_dets);
}

int mi355_selftest_yolodec_check(size_t tensor_pitch_bytes, int n_tensors, int layout, uint32_t num_fields, uint32_t num_candidates) {
  const char *why = nullptr;
  return yolodec_check_args(tensor_pitch_bytes, n_tensors, layout, num_fields, num_candidates, &why);
}

int mi355_selftest_yolodec_set_plan(int n_jobs, const int *layout, const uint32_t *num_fields, const uint32_t *num_candidates, const uint32_t *max_dets,
                                    uint32_t *first_block, uint32_t *blocks, uint64_t *key_offset, uint64_t *box_offset, uint64_t *det_offset, uint64_t totals[6]) {
  if (!totals) return MI355_ERR_INVALID_ARG;
  // the mixed plan without level arrays: it refuses a head job with MI355_ERR_INVALID_ARG, in job order with the other refusals
  uint32_t candidates[kYdSetMax];
  uint64_t t[8];
  const int rc = yolodec_mixed_set_plan(n_jobs, layout, num_fields, num_candidates, max_dets, nullptr, nullptr, nullptr, candidates, first_block, blocks, key_offset,
                                        box_offset, det_offset, nullptr, t);
  if (rc) return rc;
  for (int k = 0; k < 6; k++) totals[k] = t[k];
  return MI355_OK;
}

int mi355_selftest_yolox_head_set_plan(int n_jobs, const int *kind, const uint32_t *num_fields, const uint32_t *num_candidates, const uint32_t *max_dets,
                                       const int *n_levels, const uint32_t *level_h, const uint32_t *level_w, uint32_t *candidates, uint32_t *first_block,
                                       uint32_t *blocks, uint64_t *key_offset, uint64_t *box_offset, uint64_t *det_offset, uint32_t *level_first_block,
                                       uint64_t totals[8]) {
  return yolodec_mixed_set_plan(n_jobs, kind, num_fields, num_candidates, max_dets, n_levels, level_h, level_w, candidates, first_block, blocks, key_offset, box_offset,
                                det_offset, level_first_block, totals);
}

}  // extern "C"
