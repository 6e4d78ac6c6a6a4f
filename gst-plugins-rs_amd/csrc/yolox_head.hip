// yolox_head.hip — the two in-tree loops of `yoloxinference` around the network: the head decode (Head::forward / Head::decode,
// analytics/burn/src/yoloxinference/yolox_burn/model/head.rs:23-34, :74-85, :89-122) and the frame -> input tensor conversion
// (yoloxinference/imp.rs:439-447, :533-539). The contract is DESIGN §4.13 (tests/yolox_head_restate.py and tools/yolox_head_cpu.cpp
// restate it independently). Per tensor there are L levels; level l has the NCHW f32 maps reg[4][h][w], obj[1][h][w], cls[C][h][w]
// and an integer stride s. Candidate a = (sum of the earlier levels' h * w) + i, i = y * w + x (head.rs:84: cat after flatten; :97-
// 109: x is the fast index of the grid). Row a of the decoded tensor [A, 5 + C]:
//   0, 1    (reg0[i] + x) * s, (reg1[i] + y) * s: an f32 add, then an f32 multiply (:114)
//   2, 3    exp(reg2[i]) * s, exp(reg3[i]) * s (:116)
//   4       sigmoid(obj[i]) (:75)
//   5 + c   sigmoid(cls[c][i])
// Detections are what the X decoder (yolodec.hip) makes of that tensor, record for record; `candidate` is the row a.
// The stated deviation (the one handdec.hip makes for atan2): exp and sigmoid come from burn's backend, whose source is not in the
// reference tree - RESTATED WITHOUT SOURCE, PARITY UNPINNED. exp(x) is the f64 exponential of the f32 argument rounded once to f32
// (an overflow gives inf), sigmoid(x) is 1 / (1 + exp(-x)) evaluated in f64 from the f32 argument and rounded once. A NaN in
// gives a NaN out, sign and payload the hardware's.
//
//   yolox_head_score_kernel   grid (candidate tiles, tensors), one lane per candidate; every plane read is a coalesced wave load,
//                             as in the V8 form of the tensor decoder. The level comes from a scan of the (at most 8) prefix sums
//                             in the kernel arguments. obj is read first and its sigmoid tested against box_thr (a NaN stays);
//                             only the lanes that stay walk the class planes. The class is the LAST of equal maxima of the
//                             SIGMOID values under total_cmp; the walk finds it on the raw logits with two or three f64
//                             exponentials per candidate instead of C (best_class below says why that is the same index). Key
//                             and append as score_tile does; confidence = sigmoid(obj) * sigmoid(best class).
//   yolox_head_nms_kernel     nms_block of yolodec_device.hpp with a loader that decodes a survivor's box from the four reg planes
//                             (two exponentials per survivor).
//   yolox_head_decode_kernel  the materialised tensor: 64 candidates x 32 fields per step through an LDS tile (row stride 33), plane
//                             reads by whole waves, row pieces of 128 bytes out.
//   yolox_input_kernel        RGB u8 -> [3][H][W] f32: one lane takes 4 pixels of a row (12 bytes as three dwords where the row
//                             piece is aligned, as the 3-byte hsvfilter kernel does) and stores one float4 per plane.
//   yolox_input_jobs_kernel   the job-table form of yolox_input_kernel for the decoder queue's infer members: one flat grid over the
//                             frames of independent instances, each with its own pointer, stride, size and destination.
//   yolox_head_score_jobs_kernel, yolox_head_nms_jobs_kernel
//                             the job-table forms for the video group's decoder queue (group.hip; the set is laid out and launched
//                             by yolodec_launch_set): heads of independent instances in two launches per set. A tile is 256
//                             candidates of one level and its block reads that level's job, so there is no scan of the levels and
//                             no per-lane level table; the candidate's work is score_cand / best_class / reg_box, as above.
#include "yolodec_device.hpp"

#include <cstring>
#include <string>

namespace mi355 {

namespace {

constexpr int kLv = MI355_YOLOX_LEVELS_MAX;
constexpr uint32_t kMaxStride = 65536, kMaxInputSide = 65536;
constexpr int kDecRows = 64, kDecChunk = 32, kDecStride = kDecChunk + 1;

static_assert(sizeof(mi355_yolox_level) == 64, "mi355_yolox_level is 64 bytes");

// the levels of a call, passed in the kernel arguments; pitches in dwords; entries from n_levels on are zero
struct HeadMaps {
  const float *reg[kLv], *obj[kLv], *cls[kLv];
  unsigned long long reg_pitch[kLv], obj_pitch[kLv], cls_pitch[kLv];
  uint32_t start[kLv + 1];   // first candidate of the level; A from n_levels on: level l has start[l + 1] - start[l] elements
  uint32_t w[kLv];
  float stride[kLv];
  uint32_t n_levels, C;
};
static_assert(sizeof(HeadMaps) <= 1024, "the levels are passed in the kernel arguments");

// the stated deviation: f64 functions of the f32 argument, rounded once
__device__ __forceinline__ float exp_c(float v) { return (float)exp((double)v); }
__device__ __forceinline__ float sigmoid_c(float v) { return (float)(1.0 / (1.0 + exp(-(double)v))); }

// candidate a of tensor t: its level's maps, its element, its grid position
struct Cand {
  const float *reg, *obj, *cls;
  uint32_t hw, i;
  float gx, gy, s;
};

// a scan of the prefix sums: every index is a constant, so the levels stay in scalar registers (a < A by the caller)
__device__ __forceinline__ Cand locate(const HeadMaps &H, uint32_t t, uint32_t a) {
  const float *reg = H.reg[0] + (size_t)t * H.reg_pitch[0], *obj = H.obj[0] + (size_t)t * H.obj_pitch[0], *cls = H.cls[0] + (size_t)t * H.cls_pitch[0];
  uint32_t first = 0, w = H.w[0], hw = H.start[1];
  float s = H.stride[0];
#define MI355_YH_LEVEL(l)                              \
  if (a >= H.start[l]) { /* start[l] = A from n_levels on */ \
    reg = H.reg[l] + (size_t)t * H.reg_pitch[l];         \
    obj = H.obj[l] + (size_t)t * H.obj_pitch[l];         \
    cls = H.cls[l] + (size_t)t * H.cls_pitch[l];         \
    first = H.start[l];                                  \
    w = H.w[l];                                          \
    hw = H.start[l + 1] - H.start[l];                    \
    s = H.stride[l];                                     \
  }
  MI355_YH_LEVEL(1) MI355_YH_LEVEL(2) MI355_YH_LEVEL(3) MI355_YH_LEVEL(4) MI355_YH_LEVEL(5) MI355_YH_LEVEL(6) MI355_YH_LEVEL(7)
#undef MI355_YH_LEVEL
  Cand k;
  k.reg = reg;
  k.obj = obj;
  k.cls = cls;
  k.hw = hw;
  k.i = a - first;   // < hw
  const uint32_t y = k.i / w;
  k.gx = (float)(k.i - y * w);
  k.gy = (float)y;
  k.s = s;
  return k;
}

// The class of one candidate: the LAST of equal maxima of sigmoid_c(col[c * hw]) under total_cmp, and that maximum's bits.
// The contract's sigmoid is non-decreasing in its argument (exp, 1 + e, 1 / d and the two roundings all are) and maps numbers to
// numbers in [0, 1], where total_cmp is the numeric order and equality is bit equality. So over the classes that are numbers:
//   - the largest sigmoid is sigmoid(m), m the largest logit (-0 and +0 compare equal here and share the sigmoid 0.5);
//   - with im the last index whose logit equals m, an index after im wins iff its sigmoid equals sigmoid(m). `after`, the largest
//     logit behind im, decides whether there is one; if so a second walk behind im finds the last, evaluating the sigmoid only
//     for logits between the largest known not to tie and the smallest known to tie (a logit between two that tie ties).
// A NaN logit gives a NaN sigmoid with the hardware's sign: a positive NaN is above every number, a negative one below. They are
// folded on their sigmoid bits as the tensor decoder folds; the best of them wins iff it is positive or no class is a number.
__device__ __forceinline__ void best_class(const float *__restrict__ col, size_t hw, uint32_t C, uint32_t &cls_out, uint32_t &bits_out) {
  bool have = false, have_after = false, have_nan = false;
  float m = 0.0f, after = 0.0f;
  uint32_t im = 0;
  int32_t nan_key = INT_MIN;
  uint32_t nan_bits = 0, nan_cls = 0;
  auto fold = [&](float x, uint32_t c) {
    if (x != x) {
      fold_class(__float_as_uint(sigmoid_c(x)), c, nan_key, nan_bits, nan_cls);
      have_nan = true;
    } else if (!have || x >= m) {
      m = x;
      im = c;
      have = true;
      have_after = false;
    } else if (!have_after || x > after) {
      after = x;
      have_after = true;
    }
  };
  uint32_t c = 0;
  for (; c + 4 <= C; c += 4) {
    const float v0 = col[(size_t)(c + 0) * hw], v1 = col[(size_t)(c + 1) * hw], v2 = col[(size_t)(c + 2) * hw], v3 = col[(size_t)(c + 3) * hw];
    fold(v0, c + 0);
    fold(v1, c + 1);
    fold(v2, c + 2);
    fold(v3, c + 3);
  }
  for (; c < C; c++) fold(col[(size_t)c * hw], c);
  if (have_nan && (nan_key > 0 || !have)) {
    cls_out = nan_cls;
    bits_out = nan_bits;
    return;
  }
  const float sm = sigmoid_c(m);
  uint32_t last = im;
  if (have_after && sigmoid_c(after) == sm) {
    float lo = after, fail = 0.0f;   // lo: the smallest logit known to tie; fail: the largest known not to
    bool have_fail = false;
    for (c = im + 1; c < C; c++) {
      const float x = col[(size_t)c * hw];
      if (x != x) continue;
      bool tie;
      if (x >= lo) tie = true;
      else if (have_fail && x <= fail) tie = false;
      else {
        tie = sigmoid_c(x) == sm;
        if (tie) lo = x;
        else {
          fail = x;
          have_fail = true;
        }
      }
      if (tie) last = c;
    }
  }
  cls_out = last;
  bits_out = __float_as_uint(sm);
}

// element i of a level with the planes obj[hw], cls[C][hw]: does the candidate stay, and if so its class and confidence. Shared by
// the lone kernel and the job-table kernel.
__device__ __forceinline__ bool score_cand(const float *__restrict__ obj, const float *__restrict__ cls, uint32_t hw, uint32_t i, uint32_t C,
                                           const mi355_yolo_params &P, uint32_t &best_cls, uint32_t &conf_bits) {
  const float so = sigmoid_c(obj[i]);
  if (so < P.box_confidence_threshold) return false;   // yolotensordec/imp.rs:332, before any class plane is touched
  uint32_t sc_bits = 0;
  best_class(cls + i, (size_t)hw, C, best_cls, sc_bits);
  const float sc = __uint_as_float(sc_bits);
  conf_bits = __float_as_uint(so * sc);
  return !(sc < P.class_confidence_threshold);
}

// element i of a level with the planes reg[4][hw] at grid position (gx, gy) and stride s: its box
__device__ __forceinline__ Box reg_box(const float *__restrict__ reg, uint32_t hw, uint32_t i, float gx, float gy, float s) {
  const float *__restrict__ r = reg + i;
  const float r0 = r[0], r1 = r[(size_t)hw], r2 = r[(size_t)2 * hw], r3 = r[(size_t)3 * hw];
  return centre_box((r0 + gx) * s, (r1 + gy) * s, exp_c(r2) * s, exp_c(r3) * s);
}

// the score work of the 256-candidate tile of tensor t that starts at candidate c0, by the whole block: survivors are appended to
// keys[0 .. key_pitch) behind *count
__device__ __forceinline__ void head_score_tile(const HeadMaps &H, uint32_t t, uint32_t A, const mi355_yolo_params &P, uint32_t c0, uint32_t *__restrict__ count,
                                                unsigned long long *__restrict__ keys, size_t key_pitch) {
  const uint32_t a = c0 + (uint32_t)threadIdx.x;
  bool keep = a < A;
  uint32_t best_cls = 0, conf_bits = 0;
  if (keep) {
    const Cand k = locate(H, t, a);
    keep = score_cand(k.obj, k.cls, k.hw, k.i, H.C, P, best_cls, conf_bits);
  }
  append_keys(keep, make_key(best_cls, conf_bits, a), count, keys, key_pitch);
}

// keys: [tensors][key_pitch], count: [tensors], zero on entry
__global__ __launch_bounds__(kScoreThreads) void yolox_head_score_kernel(const HeadMaps H, uint32_t A, const mi355_yolo_params *__restrict__ params,
                                                                          uint32_t *__restrict__ count, unsigned long long *__restrict__ keys, size_t key_pitch) {
  const uint32_t t = blockIdx.y;
  const mi355_yolo_params P = params[t];
  head_score_tile(H, t, A, P, blockIdx.x * kScoreThreads, count + t, keys + (size_t)t * key_pitch, key_pitch);
}

// the box loader nms_block takes: the candidate's box decoded from the four reg planes
struct HeadBoxes {
  const HeadMaps &H;
  uint32_t t;
  __device__ __forceinline__ Box operator()(uint32_t a) const {
    const Cand k = locate(H, t, a);
    return reg_box(k.reg, k.hw, k.i, k.gx, k.gy, k.s);
  }
};

// kbox / ksrc: [tensors][A]
__global__ __launch_bounds__(kNmsThreads) void yolox_head_nms_kernel(const HeadMaps H, uint32_t A, const mi355_yolo_params *__restrict__ params,
                                                                      uint32_t *__restrict__ count, unsigned long long *__restrict__ keys, size_t key_pitch,
                                                                      float4 *__restrict__ kbox, uint32_t *__restrict__ ksrc, mi355_yolo_det *__restrict__ dets,
                                                                      uint32_t max_dets, uint32_t *__restrict__ n_dets) {
  __shared__ unsigned long long lds_keys[kLdsSortKeys];
  __shared__ NmsShared S;
  const uint32_t t = blockIdx.x;
  const HeadBoxes boxes = {H, t};
  nms_block(boxes, H.C, A, params[t].iou_threshold, count + t, keys + (size_t)t * key_pitch, kbox + (size_t)t * A, ksrc + (size_t)t * A,
            dets + (size_t)t * max_dets, max_dets, n_dets + t, lds_keys, S);
}

// ---- job-table forms (the video group's decoder queue): the heads of independent instances - own levels, C, settings, scratch - in
// one launch set. The tables (YhTable, yolodec_device.hpp) are in device memory; a level's fields come with its job, so nothing
// scans the levels per lane as locate does.

// One flat grid over the tiles of the level jobs; a tile is 256 candidates of ONE level. The level job is the last one whose first
// tile is at or before this block: a binary search on blockIdx.x alone, block-uniform, before anything else. (A two-step form - the
// head among 32 first blocks in one load, then the level among the head's 8: three dependent loads for up to ten - measured the same
// and was dropped)
__global__ __launch_bounds__(kScoreThreads) void yolox_head_score_jobs_kernel(const YhTable *__restrict__ T, uint32_t n_level_jobs) {
  uint32_t lo = 0, hi = n_level_jobs;   // level[lo].first_block <= blockIdx.x throughout: level[0].first_block is 0
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (T->level[mid].first_block <= blockIdx.x) lo = mid;
    else hi = mid;
  }
  const YhLevelJob *__restrict__ L = T->level + lo;
  const YhHeadJob *__restrict__ J = T->head + L->head;
  const uint32_t hw = L->hw, i = (blockIdx.x - L->first_block) * kScoreThreads + (uint32_t)threadIdx.x;
  const mi355_yolo_params P = J->p;
  bool keep = i < hw;   // (a grid larger than the plan's total: no lane of the last level's surplus tiles stays)
  uint32_t best_cls = 0, conf_bits = 0;
  if (keep) keep = score_cand(L->obj, L->cls, hw, i, J->C, P, best_cls, conf_bits);
  append_keys(keep, make_key(best_cls, conf_bits, L->first_cand + i), J->count, J->keys, (size_t)J->key_cap);
}

// the box loader nms_block takes: the survivor's level from the head's prefix sums (held in registers: every index is a constant),
// then that level job's fields
struct HeadJobBoxes {
  const YhLevelJob *__restrict__ level;   // the head's first level job
  uint32_t start[kLv];
  __device__ __forceinline__ Box operator()(uint32_t a) const {
    uint32_t l = 0;
#pragma unroll
    for (int k = 1; k < kLv; k++) l += a >= start[k] ? 1u : 0u;   // start[k] = A > a from n_levels on
    const YhLevelJob *__restrict__ L = level + l;
    const uint32_t w = L->w, i = a - L->first_cand, y = i / w;
    return reg_box(L->reg, L->hw, i, (float)(i - y * w), (float)y, L->stride);
  }
};

// one block per head
__global__ __launch_bounds__(kNmsThreads) void yolox_head_nms_jobs_kernel(const YhTable *__restrict__ T, uint32_t n_heads) {
  __shared__ unsigned long long lds_keys[kLdsSortKeys];
  __shared__ NmsShared S;
  if (blockIdx.x >= n_heads) return;
  const YhHeadJob *__restrict__ J = T->head + blockIdx.x;
  HeadJobBoxes boxes;
  boxes.level = T->level + J->first_level;
#pragma unroll
  for (int k = 0; k < kLv; k++) boxes.start[k] = J->start[k];
  nms_block(boxes, J->C, J->A, J->p.iou_threshold, J->count, J->keys, J->kbox, J->ksrc, J->dets, J->max_dets, J->n_dets, lds_keys, S);
}

// field f of the decoded row (f is wave-uniform in the kernel below)
__device__ __forceinline__ float head_field(const Cand &k, uint32_t f) {
  if (f < 4) {
    const float v = k.reg[(size_t)f * k.hw + k.i];
    if (f == 0) return (v + k.gx) * k.s;
    if (f == 1) return (v + k.gy) * k.s;
    return exp_c(v) * k.s;
  }
  if (f == 4) return sigmoid_c(k.obj[k.i]);
  return sigmoid_c(k.cls[(size_t)(f - 5) * k.hw + k.i]);
}

// grid (tiles of 64 candidates, tensors): lane = candidate for the plane reads, 32 fields of 64 rows per step through the tile
__global__ __launch_bounds__(256) void yolox_head_decode_kernel(const HeadMaps H, uint32_t A, float *__restrict__ out, size_t out_pitch_dwords) {
  __shared__ float tile[kDecRows * kDecStride];
  const uint32_t t = blockIdx.y, a0 = blockIdx.x * kDecRows, F = 5 + H.C;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t a = a0 + (uint32_t)lane;
  const bool valid = a < A;
  Cand k = {nullptr, nullptr, nullptr, 0, 0, 0.0f, 0.0f, 0.0f};
  if (valid) k = locate(H, t, a);
  const uint32_t rows = A - a0 < (uint32_t)kDecRows ? A - a0 : (uint32_t)kDecRows;   // a0 < A by the grid
  float *__restrict__ o = out + (size_t)t * out_pitch_dwords + (size_t)a0 * F;
  for (uint32_t f0 = 0; f0 < F; f0 += kDecChunk) {
    const uint32_t nf = F - f0 < (uint32_t)kDecChunk ? F - f0 : (uint32_t)kDecChunk;
    for (uint32_t j = (uint32_t)wave; j < nf; j += 4)
      if (valid) tile[lane * kDecStride + j] = head_field(k, f0 + j);
    __syncthreads();
    for (uint32_t e = (uint32_t)tid; e < (uint32_t)kDecRows * kDecChunk; e += 256) {
      const uint32_t r = e / kDecChunk, j = e % kDecChunk;
      if (r < rows && j < nf) o[(size_t)r * F + f0 + j] = tile[r * kDecStride + j];
    }
    __syncthreads();   // the tile is written again
  }
}

// grid (groups of 4 pixels, frames): out[c][y][x] = (f32) in[y * stride + 3 x + c]
__global__ __launch_bounds__(256) void yolox_input_kernel(const uint8_t *__restrict__ frames, size_t frame_pitch, size_t stride, uint32_t W, uint32_t Hh,
                                                           float *__restrict__ out, size_t out_pitch_dwords, uint32_t groups_per_row) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= (size_t)groups_per_row * Hh) return;
  const uint32_t y = (uint32_t)(g / groups_per_row), x0 = (uint32_t)(g % groups_per_row) * 4;
  const uint32_t n = W - x0 < 4u ? W - x0 : 4u;
  const uint8_t *__restrict__ src = frames + (size_t)blockIdx.y * frame_pitch + (size_t)y * stride + (size_t)3 * x0;
  uint32_t d0 = 0, d1 = 0, d2 = 0;   // the 12 bytes of the group, little-endian
  if (n == 4 && ((uintptr_t)src & 3) == 0) {
    const uint32_t *__restrict__ s4 = reinterpret_cast<const uint32_t *>(src);
    d0 = s4[0];
    d1 = s4[1];
    d2 = s4[2];
  } else {
    for (uint32_t b = 0; b < 3 * n; b++) {
      const uint32_t v = (uint32_t)src[b] << (8 * (b & 3));
      if (b < 4) d0 |= v;
      else if (b < 8) d1 |= v;
      else d2 |= v;
    }
  }
  const uint32_t p[4] = {d0, (d0 >> 24) | (d1 << 8), (d1 >> 16) | (d2 << 16), d2 >> 8};   // pixel j: c0 | c1 << 8 | c2 << 16
  const size_t plane = (size_t)W * Hh;
  float *__restrict__ dst = out + (size_t)blockIdx.y * out_pitch_dwords + (size_t)y * W + x0;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    float *__restrict__ q = dst + (size_t)c * plane;
    const float v0 = (float)((p[0] >> (8 * c)) & 0xffu), v1 = (float)((p[1] >> (8 * c)) & 0xffu), v2 = (float)((p[2] >> (8 * c)) & 0xffu),
                v3 = (float)((p[3] >> (8 * c)) & 0xffu);
    if (n == 4 && ((uintptr_t)q & 15) == 0) {
      *reinterpret_cast<float4 *>(q) = make_float4(v0, v1, v2, v3);
    } else {
      q[0] = v0;
      if (n > 1) q[1] = v1;
      if (n > 2) q[2] = v2;
      if (n > 3) q[3] = v3;
    }
  }
}

// The job-table form of yolox_input_kernel for the decoder queue's infer members: one flat grid over the conversion blocks of all
// jobs, a block 256 lanes of 4 pixels of ONE job. The job is the last one whose first block is at or before this block: a binary
// search on blockIdx.x alone, block-uniform, as yolox_head_score_jobs_kernel finds its level job. W is a multiple of 32, so a group
// of 4 pixels never meets a row's end and every store is one aligned float4 (the lane's input tensor is an allocation's start plus
// whole frames); the byte path stays: a member's base pointer and stride are its own.
__global__ __launch_bounds__(256) void yolox_input_jobs_kernel(const YxConvJob *__restrict__ jobs, uint32_t n_jobs, uint32_t total_blocks) {
  if (blockIdx.x >= total_blocks) return;   // a grid larger than the plan's total
  uint32_t lo = 0, hi = n_jobs;   // jobs[lo].first_block <= blockIdx.x throughout: jobs[0].first_block is 0
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (jobs[mid].first_block <= blockIdx.x) lo = mid;
    else hi = mid;
  }
  const YxConvJob *__restrict__ J = jobs + lo;
  const uint32_t W = J->W, Hh = J->H, groups_per_row = W >> 2;
  const uint32_t g = (blockIdx.x - J->first_block) * 256 + (uint32_t)threadIdx.x;
  if (g >= groups_per_row * Hh) return;   // <= 2048 * 512 groups; the last block's tail, and the blocks of a job with more blocks than its frame has
  const uint32_t y = g / groups_per_row, x0 = (g - y * groups_per_row) * 4;
  const uint8_t *__restrict__ src = J->src + (size_t)y * J->stride + (size_t)3 * x0;
  uint32_t d0 = 0, d1 = 0, d2 = 0;   // the 12 bytes of the group, little-endian
  if (((uintptr_t)src & 3) == 0) {
    const uint32_t *__restrict__ s4 = reinterpret_cast<const uint32_t *>(src);
    d0 = s4[0];
    d1 = s4[1];
    d2 = s4[2];
  } else {
#pragma unroll
    for (uint32_t b = 0; b < 12; b++) {
      const uint32_t v = (uint32_t)src[b] << (8 * (b & 3));
      if (b < 4) d0 |= v;
      else if (b < 8) d1 |= v;
      else d2 |= v;
    }
  }
  const uint32_t p[4] = {d0, (d0 >> 24) | (d1 << 8), (d1 >> 16) | (d2 << 16), d2 >> 8};   // pixel j: c0 | c1 << 8 | c2 << 16
  const size_t plane = (size_t)W * Hh;
  float *__restrict__ dst = J->dst + (size_t)y * W + x0;
#pragma unroll
  for (int c = 0; c < 3; c++)
    *reinterpret_cast<float4 *>(dst + (size_t)c * plane) = make_float4((float)((p[0] >> (8 * c)) & 0xffu), (float)((p[1] >> (8 * c)) & 0xffu),
                                                                        (float)((p[2] >> (8 * c)) & 0xffu), (float)((p[3] >> (8 * c)) & 0xffu));
}

}  // namespace

// the checks of the level shapes (every entry point, the group's submit and its set plan): everything but the map pointers and
// pitches. *A_out: the candidates of one tensor.
int yolox_head_check_shape(const mi355_yolox_level *lv, int n_levels, int n_tensors, uint32_t C, uint32_t *A_out, const char **why) {
  *why = nullptr;
  if (!lv) *why = "yolox_head: null levels";
  else if (n_levels < 1) *why = "yolox_head: n_levels must be at least 1";
  else if (n_tensors < 1) *why = "yolox_head: n_tensors must be at least 1";
  else if (C < 1) *why = "yolox_head: num_classes must be at least 1";
  if (*why) return MI355_ERR_INVALID_ARG;
  if (n_levels > kLv) *why = "yolox_head: more than 8 levels";
  else if (C > kMaxFields - 5) *why = "yolox_head: more than 1029 fields (5 + num_classes)";
  else if ((uint32_t)n_tensors > kMaxTensors) *why = "yolox_head: more than 1024 tensors";
  if (*why) return MI355_ERR_UNSUPPORTED;
  for (int l = 0; l < n_levels; l++) {
    if (lv[l].h == 0 || lv[l].w == 0 || lv[l].stride == 0) *why = "yolox_head: a level's h, w or stride is 0";
    else if (lv[l].reserved != 0) *why = "yolox_head: a level's reserved field is not 0";
    if (*why) return MI355_ERR_INVALID_ARG;
  }
  uint64_t A = 0;
  for (int l = 0; l < n_levels; l++) {
    const uint64_t hw = (uint64_t)lv[l].h * lv[l].w;
    if (lv[l].stride > kMaxStride) *why = "yolox_head: a stride above 65536";
    else if (hw > kMaxCandidates || (A += hw) > kMaxCandidates) *why = "yolox_head: more than 65536 candidates";
    if (*why) return MI355_ERR_UNSUPPORTED;
  }
  if (A_out) *A_out = (uint32_t)A;
  return MI355_OK;
}

// the maps of one level of a checked shape; device: the pitches count
static int check_level_maps(const mi355_yolox_level &lv, bool device, uint32_t C, const char **why) {
  const uint64_t hw = (uint64_t)lv.h * lv.w;
  if (!lv.reg || !lv.obj || !lv.cls) *why = "yolox_head: a null map";
  else if ((uintptr_t)lv.reg % 4 != 0 || (uintptr_t)lv.obj % 4 != 0 || (uintptr_t)lv.cls % 4 != 0) *why = "yolox_head: a map is not 4-byte aligned";
  else if (device && (lv.reg_pitch_bytes % 4 != 0 || lv.obj_pitch_bytes % 4 != 0 || lv.cls_pitch_bytes % 4 != 0 || lv.reg_pitch_bytes < 4 * hw * 4 ||
                      lv.obj_pitch_bytes < hw * 4 || lv.cls_pitch_bytes < (uint64_t)C * hw * 4))
    *why = "yolox_head: a map pitch is smaller than the map or no multiple of 4";
  return *why ? MI355_ERR_INVALID_ARG : MI355_OK;
}

int yolox_head_check_maps(const mi355_yolox_level *lv, int n_levels, const char **why) {
  *why = nullptr;
  for (int l = 0; l < n_levels; l++)
    if (const int rc = check_level_maps(lv[l], false, 0, why)) return rc;
  return MI355_OK;
}

// the checks that need no device (every entry point; mi355_selftest_yolox_head_check). device: the pitches count and n_tensors may
// exceed 1; with_out: out_pitch_bytes is the pitch of the materialised tensor. *A_out: the candidates of one tensor.
static int yolox_head_check_args(const mi355_yolox_level *lv, int n_levels, int n_tensors, uint32_t C, bool device, bool with_out, size_t out_pitch_bytes,
                                 uint32_t *A_out, const char **why) {
  uint32_t A = 0;
  if (const int rc = yolox_head_check_shape(lv, n_levels, n_tensors, C, &A, why)) return rc;
  for (int l = 0; l < n_levels; l++)
    if (const int rc = check_level_maps(lv[l], device, C, why)) return rc;
  if (with_out && (out_pitch_bytes % 4 != 0 || out_pitch_bytes < (uint64_t)A * (5 + (uint64_t)C) * 4)) {
    *why = "yolox_head: output pitch is smaller than the tensor or no multiple of 4";
    return MI355_ERR_INVALID_ARG;
  }
  if (A_out) *A_out = A;
  return MI355_OK;
}

// checked levels -> the kernels' argument
static void head_maps(const mi355_yolox_level *lv, int n_levels, uint32_t C, HeadMaps *H) {
  std::memset(H, 0, sizeof(*H));
  uint32_t a = 0;
  for (int l = 0; l < n_levels; l++) {
    H->reg[l] = lv[l].reg;
    H->obj[l] = lv[l].obj;
    H->cls[l] = lv[l].cls;
    H->reg_pitch[l] = lv[l].reg_pitch_bytes / 4;
    H->obj_pitch[l] = lv[l].obj_pitch_bytes / 4;
    H->cls_pitch[l] = lv[l].cls_pitch_bytes / 4;
    H->start[l] = a;
    H->w[l] = lv[l].w;
    H->stride[l] = (float)lv[l].stride;   // <= 65536: exact
    a += lv[l].h * lv[l].w;
  }
  for (int l = n_levels; l <= kLv; l++) H->start[l] = a;
  H->n_levels = (uint32_t)n_levels;
  H->C = C;
}

// settings up, the two launches, results down, one synchronisation
static int head_dets_run(mi355_ctx *ctx, YoloDecState *s, const HeadMaps &H, uint32_t A, uint32_t T, const mi355_yolo_params *p, mi355_yolo_det *dets,
                         uint32_t max_dets, uint32_t *n_dets) {
  int rc = MI355_OK;
  if ((rc = yolodec_upload_params(ctx, s, T, p))) return rc;
  const size_t key_pitch = pow2_at_least(A);
  s->count_zero = false;   // true again only once the NMS kernel has been enqueued behind the score kernel
  hipLaunchKernelGGL(yolox_head_score_kernel, dim3((A + kScoreThreads - 1) / kScoreThreads, T), dim3(kScoreThreads), 0, ctx->stream, H, A, s->d_params.p, s->d_count.p,
                     s->d_keys.p, key_pitch);
  if ((rc = check_hip(ctx, hipGetLastError(), "yolox_head score launch"))) return rc;
  hipLaunchKernelGGL(yolox_head_nms_kernel, dim3(T), dim3(kNmsThreads), 0, ctx->stream, H, A, s->d_params.p, s->d_count.p, s->d_keys.p, key_pitch, s->d_kbox.p, s->d_ksrc.p,
                     yolodec_d_dets(s, T), max_dets, yolodec_d_counts(s));
  if ((rc = check_hip(ctx, hipGetLastError(), "yolox_head nms launch"))) return rc;
  return yolodec_download(ctx, s, T, dets, max_dets, n_dets);
}

// the head members of a decoder launch set (yolodec_launch_set): the tables are on the device behind what `stream` holds
int yolox_head_launch_jobs(hipStream_t stream, const YhTable *d_table, uint32_t n_heads, uint32_t n_level_jobs, uint32_t score_blocks, int *kernel_launches,
                           std::string *err) {
  if (!d_table || n_heads < 1 || n_heads > (uint32_t)kYdSetMax || n_level_jobs < n_heads || n_level_jobs > (uint32_t)kYhLevelJobsMax || score_blocks < n_level_jobs) {
    *err = "yolox_head: bad job tables";
    return MI355_ERR_INVALID_ARG;
  }
  hipLaunchKernelGGL(yolox_head_score_jobs_kernel, dim3(score_blocks), dim3(kScoreThreads), 0, stream, d_table, n_level_jobs);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { *err = std::string("yolox_head score jobs kernel launch: ") + hipGetErrorString(e); return MI355_ERR_HIP; }
  (*kernel_launches)++;
  hipLaunchKernelGGL(yolox_head_nms_jobs_kernel, dim3(n_heads), dim3(kNmsThreads), 0, stream, d_table, n_heads);
  e = hipGetLastError();
  if (e != hipSuccess) { *err = std::string("yolox_head nms jobs kernel launch: ") + hipGetErrorString(e); return MI355_ERR_HIP; }
  (*kernel_launches)++;
  return MI355_OK;
}

// the infer members of a decoder launch set (yolodec_launch_set): the jobs are on the device behind what `stream` holds
int yolox_input_launch_jobs(hipStream_t stream, const YxConvJob *d_jobs, uint32_t n_jobs, uint32_t total_blocks, int *kernel_launches, std::string *err) {
  if (!d_jobs || n_jobs < 1 || n_jobs > (uint32_t)kYdSetMax || total_blocks < n_jobs || (uintptr_t)d_jobs % 8 != 0) {
    *err = "yolox_input: bad conversion jobs";
    return MI355_ERR_INVALID_ARG;
  }
  hipLaunchKernelGGL(yolox_input_jobs_kernel, dim3(total_blocks), dim3(256), 0, stream, d_jobs, n_jobs, total_blocks);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { *err = std::string("yolox_input jobs kernel launch: ") + hipGetErrorString(e); return MI355_ERR_HIP; }
  (*kernel_launches)++;
  return MI355_OK;
}

}  // namespace mi355

using namespace mi355;

extern "C" {

int mi355_yolox_head_decode_device(mi355_ctx *ctx, const mi355_yolox_level *levels, int n_levels, int n_tensors, uint32_t num_classes, float *d_out,
                                   size_t out_pitch_bytes) {
  if (!ctx) return MI355_ERR_INVALID_ARG;
  const char *why = nullptr;
  uint32_t A = 0;
  int rc = yolox_head_check_args(levels, n_levels, n_tensors, num_classes, true, true, out_pitch_bytes, &A, &why);
  if (rc) return set_error(ctx, rc, why);
  if (!d_out || (uintptr_t)d_out % 4 != 0) return set_error(ctx, MI355_ERR_INVALID_ARG, "yolox_head: null or misaligned output");
  if ((rc = check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice"))) return rc;
  HeadMaps H;
  head_maps(levels, n_levels, num_classes, &H);
  hipLaunchKernelGGL(yolox_head_decode_kernel, dim3((A + kDecRows - 1) / kDecRows, (uint32_t)n_tensors), dim3(256), 0, ctx->stream, H, A, d_out, out_pitch_bytes / 4);
  return check_hip(ctx, hipGetLastError(), "yolox_head decode launch");
}

int mi355_yolox_head_dets_device(mi355_ctx *ctx, const mi355_yolox_level *levels, int n_levels, int n_tensors, uint32_t num_classes, const mi355_yolo_params *p,
                                 mi355_yolo_det *dets, uint32_t max_dets, uint32_t *n_dets) {
  if (!ctx) return MI355_ERR_INVALID_ARG;
  const char *why = nullptr;
  uint32_t A = 0;
  int rc = yolox_head_check_args(levels, n_levels, n_tensors, num_classes, true, false, 0, &A, &why);
  if (rc) return set_error(ctx, rc, why);
  if (!p || !n_dets || (max_dets && !dets)) return set_error(ctx, MI355_ERR_INVALID_ARG, "yolox_head: null settings or result arrays");
  if ((rc = check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice"))) return rc;
  YoloDecState *s = nullptr;
  if ((rc = yolodec_scratch(ctx, (uint32_t)n_tensors, A, max_dets, &s))) return rc;
  HeadMaps H;
  head_maps(levels, n_levels, num_classes, &H);
  return head_dets_run(ctx, s, H, A, (uint32_t)n_tensors, p, dets, max_dets, n_dets);
}

int mi355_yolox_head_dets(mi355_ctx *ctx, const mi355_yolox_level *levels, int n_levels, uint32_t num_classes, const mi355_yolo_params *p, mi355_yolo_det *dets,
                          uint32_t max_dets, uint32_t *n_dets) {
  if (!ctx) return MI355_ERR_INVALID_ARG;
  const char *why = nullptr;
  uint32_t A = 0;
  int rc = yolox_head_check_args(levels, n_levels, 1, num_classes, false, false, 0, &A, &why);
  if (rc) return set_error(ctx, rc, why);
  if (!p || !n_dets || (max_dets && !dets)) return set_error(ctx, MI355_ERR_INVALID_ARG, "yolox_head: null settings or result arrays");
  if ((rc = check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice"))) return rc;
  YoloDecState *s = nullptr;
  if ((rc = yolodec_scratch(ctx, 1, A, max_dets, &s))) return rc;
  // the maps side by side in the staging buffer: per level reg, obj, cls - the engine's fused [5 + C, h, w] form
  if ((rc = yolodec_stage(ctx, s, (size_t)A * (5 + (size_t)num_classes)))) return rc;
  mi355_yolox_level dl[kLv];
  float *at = s->d_stage.p;
  for (int l = 0; l < n_levels; l++) {
    const size_t hw = (size_t)levels[l].h * levels[l].w;
    const float *src[3] = {levels[l].reg, levels[l].obj, levels[l].cls};
    const size_t floats[3] = {4 * hw, hw, (size_t)num_classes * hw};
    dl[l] = levels[l];
    for (int k = 0; k < 3; k++) {
      if ((rc = check_hip(ctx, hipMemcpyAsync(at, src[k], floats[k] * 4, hipMemcpyHostToDevice, ctx->stream), "yolox_head H2D"))) return rc;
      __atomic_fetch_add(&ctx->n_h2d, 1ull, __ATOMIC_RELAXED);
      (k == 0 ? dl[l].reg : k == 1 ? dl[l].obj : dl[l].cls) = at;
      at += floats[k];
    }
    dl[l].reg_pitch_bytes = dl[l].obj_pitch_bytes = dl[l].cls_pitch_bytes = 0;   // one tensor
  }
  HeadMaps H;
  head_maps(dl, n_levels, num_classes, &H);
  return head_dets_run(ctx, s, H, A, 1, p, dets, max_dets, n_dets);
}

int mi355_yolox_input_frames_device(mi355_ctx *ctx, const uint8_t *d_frames, size_t frame_pitch, size_t stride, int n_frames, uint32_t width, uint32_t height,
                                    float *d_out, size_t out_pitch_bytes) {
  if (!ctx) return MI355_ERR_INVALID_ARG;
  if (n_frames < 1 || width < 1 || height < 1) return set_error(ctx, MI355_ERR_INVALID_ARG, "yolox_input: n_frames, width and height must be at least 1");
  if ((uint32_t)n_frames > kMaxTensors || width > kMaxInputSide || height > kMaxInputSide)
    return set_error(ctx, MI355_ERR_UNSUPPORTED, "yolox_input: more than 1024 frames or a side above 65536");
  const size_t row = (size_t)3 * width, frame = (size_t)(height - 1) * stride + row, plane3 = (size_t)3 * width * height * 4;
  if (stride < row || (n_frames > 1 && frame_pitch < frame)) return set_error(ctx, MI355_ERR_INVALID_ARG, "yolox_input: stride below the row or frame pitch below the frame");
  if (out_pitch_bytes % 4 != 0 || out_pitch_bytes < plane3) return set_error(ctx, MI355_ERR_INVALID_ARG, "yolox_input: output pitch is smaller than the tensor or no multiple of 4");
  if (!d_frames || !d_out || (uintptr_t)d_out % 4 != 0) return set_error(ctx, MI355_ERR_INVALID_ARG, "yolox_input: null frames, or null or misaligned output");
  int rc = MI355_OK;
  if ((rc = check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice"))) return rc;
  const uint32_t groups_per_row = (width + 3) / 4;
  const size_t groups = (size_t)groups_per_row * height;
  hipLaunchKernelGGL(yolox_input_kernel, dim3((uint32_t)((groups + 255) / 256), (uint32_t)n_frames), dim3(256), 0, ctx->stream, d_frames, frame_pitch, stride, width, height,
                     d_out, out_pitch_bytes / 4, groups_per_row);
  return check_hip(ctx, hipGetLastError(), "yolox_input launch");
}

int mi355_selftest_yolox_head_check(const mi355_yolox_level *levels, int n_levels, int n_tensors, uint32_t num_classes, size_t out_pitch_bytes) {
  const char *why = nullptr;
  return yolox_head_check_args(levels, n_levels, n_tensors, num_classes, true, true, out_pitch_bytes, nullptr, &why);
}

}  // extern "C"
