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
//                                 set. Thin wrappers, as the lone kernels are, around the same device functions (score_tile,
//                                 sort_keys, find_runs, greedy_nms, write_records).
#include "internal.hpp"

#include <climits>
#include <cstring>
#include <string>

namespace mi355 {

namespace {

constexpr int kScoreThreads = 256;
constexpr int kNmsThreads = 512;
constexpr int kNmsWaves = kNmsThreads / 64;
constexpr int kLdsSortKeys = 4096;
constexpr int kXChunk = 32;             // fields of a row in the LDS tile
constexpr int kXStride = kXChunk + 1;   // odd row stride in dwords
constexpr uint32_t kMaxFields = 1029, kMaxCandidates = 65536, kMaxTensors = 1024;
constexpr int kMaxClasses = 1025;       // V8 at F = 1029
constexpr unsigned long long kPadKey = ~0ull;   // class 2047: above every real key

static_assert(sizeof(mi355_yolo_det) == 48, "mi355_yolo_det is 48 bytes");
static_assert(sizeof(mi355_yolo_params) == 12, "mi355_yolo_params is three floats");

// f32::total_cmp's key: the order of the result as i32 is the total order
__device__ __forceinline__ int32_t total_key(uint32_t bits) {
  const int32_t s = (int32_t)bits;
  return s ^ (int32_t)((uint32_t)(s >> 31) >> 1);
}

__device__ __forceinline__ unsigned long long make_key(uint32_t cls, uint32_t conf_bits, uint32_t cand) {
  const uint32_t asc = (uint32_t)total_key(conf_bits) ^ 0x80000000u;   // unsigned, ascending with the confidence
  return ((unsigned long long)cls << 48) | ((unsigned long long)(~asc) << 16) | (unsigned long long)cand;
}
__device__ __forceinline__ uint32_t key_class(unsigned long long k) { return (uint32_t)(k >> 48); }
__device__ __forceinline__ uint32_t key_cand(unsigned long long k) { return (uint32_t)(k & 0xffffu); }
__device__ __forceinline__ uint32_t key_conf_bits(unsigned long long k) {
  const uint32_t t = (~(uint32_t)(k >> 16)) ^ 0x80000000u;   // total_key as u32
  const int32_t s = (int32_t)t;
  return (uint32_t)(s ^ (int32_t)((uint32_t)(s >> 31) >> 1));   // the key map is its own inverse
}

// max_by's fold: a later element replaces the best unless it is smaller
__device__ __forceinline__ void fold_class(uint32_t bits, uint32_t cls, int32_t &best_key, uint32_t &best_bits, uint32_t &best_cls) {
  const int32_t k = total_key(bits);
  if (k >= best_key) {
    best_key = k;
    best_bits = bits;
    best_cls = cls;
  }
}

// called by every lane of the wave: the survivors' keys go to keys[old count ...), one atomic for the wave
__device__ __forceinline__ void append_keys(bool keep, unsigned long long key, uint32_t *count, unsigned long long *keys, size_t key_pitch) {
  const unsigned long long m = __ballot(keep);
  if (m == 0) return;   // wave-uniform
  const int lane = (int)__lane_id();
  const int leader = __ffsll((long long)m) - 1;
  uint32_t base = 0;
  if (lane == leader) base = atomicAdd(count, (uint32_t)__popcll(m));
  base = (uint32_t)__shfl((int)base, leader);
  const size_t at = (size_t)base + (size_t)__popcll(m & ((1ull << lane) - 1ull));
  if (keep && at < key_pitch) keys[at] = key;   // always inside: the counter starts at zero and a candidate is appended once
}

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

// ascending bitonic sort of n2 keys (a power of two) by the whole block
__device__ __forceinline__ void bitonic_sort(unsigned long long *K, uint32_t n2) {
  for (uint32_t k = 2; k <= n2; k <<= 1) {
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t i = threadIdx.x; i < n2; i += kNmsThreads) {
        const uint32_t l = i ^ j;
        if (l > i) {
          const unsigned long long a = K[i], b = K[l];
          const bool up = (i & k) == 0;
          if (up ? a > b : a < b) {
            K[i] = b;
            K[l] = a;
          }
        }
      }
      __syncthreads();
    }
  }
}

struct Box { float xmin, ymin, xmax, ymax; };

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
  Box r;
  r.xmin = x - w / 2.0f;
  r.ymin = y - h / 2.0f;
  r.xmax = x + w / 2.0f;
  r.ymax = y + h / 2.0f;
  return r;
}

// imp.rs:480-489, literally; fmaxf / fminf are maxNum / minNum as f32::max / f32::min
__device__ __forceinline__ float iou(const Box &b1, const Box &b2) {
  const float b1_area = (b1.xmax - b1.xmin + 1.0f) * (b1.ymax - b1.ymin + 1.0f);
  const float b2_area = (b2.xmax - b2.xmin + 1.0f) * (b2.ymax - b2.ymin + 1.0f);
  const float i_xmin = fmaxf(b1.xmin, b2.xmin);
  const float i_xmax = fminf(b1.xmax, b2.xmax);
  const float i_ymin = fmaxf(b1.ymin, b2.ymin);
  const float i_ymax = fminf(b1.ymax, b2.ymax);
  const float i_area = fmaxf(i_xmax - i_xmin + 1.0f, 0.0f) * fmaxf(i_ymax - i_ymin + 1.0f, 0.0f);
  return i_area / (b1_area + b2_area - i_area);
}

// Rust's `as i32`: toward zero, saturating, NaN -> 0
__device__ __forceinline__ int32_t cast_i32(float f) {
  if (f != f) return 0;
  if (f >= 2147483648.0f) return INT_MAX;
  if (f <= -2147483648.0f) return INT_MIN;
  return (int32_t)f;
}

struct NmsShared {
  uint32_t run_lo[kMaxClasses], run_hi[kMaxClasses];   // the class's run in the sorted keys: [lo, hi), both 0 when it has none
  uint32_t kept[2][kMaxClasses + 1];                   // kept boxes per class, then their exclusive prefix sums (ping-pong)
  uint32_t n;
};

// LAYOUT 0: V8, 1: X, 2: `layout` decides (block-uniform: the job-table kernel)
template <int LAYOUT>
__device__ __forceinline__ Box load_box_of(int layout, const float *__restrict__ data, uint32_t F, uint32_t N, uint32_t c) {
  if (LAYOUT == 2) return layout == MI355_YOLO_V8 ? load_box<0>(data, F, N, c) : load_box<1>(data, F, N, c);
  return load_box<LAYOUT == 2 ? 0 : LAYOUT>(data, F, N, c);
}

// the n survivors' keys sorted ascending by the whole block: in LDS up to kLdsSortKeys keys, in the key list itself above (gk holds
// at least the power of two above n). Returns where the sorted keys are.
__device__ __forceinline__ const unsigned long long *sort_keys(unsigned long long *lds_keys, unsigned long long *gk, uint32_t n) {
  const int tid = threadIdx.x;
  uint32_t n2 = 1;
  while (n2 < n) n2 <<= 1;
  const bool in_lds = n2 <= (uint32_t)kLdsSortKeys;
  if (in_lds) {
    for (uint32_t i = tid; i < n2; i += kNmsThreads) lds_keys[i] = i < n ? gk[i] : kPadKey;
    __syncthreads();
    bitonic_sort(lds_keys, n2);
  } else {
    for (uint32_t i = n + tid; i < n2; i += kNmsThreads) gk[i] = kPadKey;
    __syncthreads();
    bitonic_sort(gk, n2);
  }
  return in_lds ? lds_keys : gk;
}

// class runs by their boundaries (S.run_lo / S.run_hi are zero on entry); ends in a barrier
__device__ __forceinline__ void find_runs(const unsigned long long *K, uint32_t n, uint32_t n_classes, NmsShared &S) {
  for (uint32_t i = threadIdx.x; i < n; i += kNmsThreads) {
    const uint32_t c = key_class(K[i]);
    if (c < n_classes) {   // always: classes come from the score kernel
      if (i == 0 || key_class(K[i - 1]) != c) S.run_lo[c] = i;
      if (i + 1 == n || key_class(K[i + 1]) != c) S.run_hi[c] = i + 1;
    }
  }
  __syncthreads();
}

// greedy NMS: the runs shared out over the waves. kb / ks: the kept boxes of a run compacted at the run's start (and the sorted
// position each came from); S.kept[0][c]: how many. Ends in a barrier.
template <int LAYOUT>
__device__ __forceinline__ void greedy_nms(int layout, const float *__restrict__ data, uint32_t F, uint32_t N, const unsigned long long *K, float iou_thr,
                                           uint32_t n_classes, float4 *kb, uint32_t *ks, NmsShared &S) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (uint32_t c = wave; c < n_classes; c += kNmsWaves) {
    const uint32_t lo = S.run_lo[c], hi = S.run_hi[c];
    uint32_t m = 0;   // boxes kept so far in this run (wave-uniform)
    for (uint32_t base = lo; base < hi; base += 64) {
      const uint32_t i = base + (uint32_t)lane;
      bool alive = i < hi;
      Box b = {0.0f, 0.0f, 0.0f, 0.0f};
      if (alive) b = load_box_of<LAYOUT>(layout, data, F, N, key_cand(K[i]));
      // against everything kept in earlier chunks
      for (uint32_t j = 0; j < m; j++) {
        const float4 q = kb[lo + j];
        const Box kj = {q.x, q.y, q.z, q.w};
        if (alive && iou(kj, b) > iou_thr) alive = false;
      }
      // inside the chunk, in order: the lowest undecided live lane is kept and tests the lanes above it
      unsigned long long todo = __ballot(alive);
      while (todo) {
        const int l = __ffsll((long long)todo) - 1;
        Box bl;
        bl.xmin = __shfl(b.xmin, l);
        bl.ymin = __shfl(b.ymin, l);
        bl.xmax = __shfl(b.xmax, l);
        bl.ymax = __shfl(b.ymax, l);
        if (alive && lane > l && iou(bl, b) > iou_thr) alive = false;
        const unsigned long long above = l == 63 ? 0ull : ~((2ull << l) - 1ull);
        todo = __ballot(alive) & above;
      }
      const unsigned long long keptm = __ballot(alive);
      if (alive) {
        const uint32_t r = lo + m + (uint32_t)__popcll(keptm & ((1ull << lane) - 1ull));   // <= i: inside the run
        kb[r] = make_float4(b.xmin, b.ymin, b.xmax, b.ymax);
        ks[r] = i;
      }
      m += (uint32_t)__popcll(keptm);
      __threadfence_block();   // the next chunk of this wave reads kb
    }
    if (lane == 0) S.kept[0][c] = m;
  }
  __syncthreads();
}

// prefix sum of the runs' kept counts, the total into *n_out, the first max_dets records into out
__device__ __forceinline__ void write_records(const unsigned long long *K, uint32_t n_classes, const float4 *kb, const uint32_t *ks, NmsShared &S,
                                              mi355_yolo_det *__restrict__ out, uint32_t max_dets, uint32_t *__restrict__ n_out) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // exclusive prefix sums of the kept counts over n_classes + 1 entries (Hillis-Steele on the shifted array)
  const uint32_t L = n_classes + 1;
  for (uint32_t c = tid; c < L; c += kNmsThreads) S.kept[1][c] = c == 0 ? 0 : S.kept[0][c - 1];
  __syncthreads();
  int cur = 1;
  for (uint32_t d = 1; d < L; d <<= 1) {
    for (uint32_t c = tid; c < L; c += kNmsThreads) S.kept[cur ^ 1][c] = S.kept[cur][c] + (c >= d ? S.kept[cur][c - d] : 0);
    __syncthreads();
    cur ^= 1;
  }
  const uint32_t *first = S.kept[cur];   // first[c]: output index of class c's first box; first[n_classes]: the total
  if (tid == 0) *n_out = first[n_classes];
  for (uint32_t c = wave; c < n_classes; c += kNmsWaves) {
    const uint32_t lo = S.run_lo[c], m = first[c + 1] - first[c], o0 = first[c];
    for (uint32_t j = lane; j < m; j += 64) {
      const uint32_t o = o0 + j;
      if (o >= max_dets) break;
      const float4 q = kb[lo + j];
      const unsigned long long key = K[ks[lo + j]];
      mi355_yolo_det d;
      d.xmin = q.x;
      d.ymin = q.y;
      d.xmax = q.z;
      d.ymax = q.w;
      d.x = cast_i32(q.x);
      d.y = cast_i32(q.y);
      d.width = cast_i32(q.z - q.x);
      d.height = cast_i32(q.w - q.y);
      d.class_id = c;
      d.confidence = __uint_as_float(key_conf_bits(key));
      d.candidate = key_cand(key);
      d.reserved = 0;
      out[o] = d;
    }
  }
}

// one tensor by one block: sort, runs, NMS, records. *count (the survivors behind gk) is left at zero. kb / ks: N entries each;
// gk: at least the power of two above N keys. Shared by the lone kernel and the job-table kernel.
template <int LAYOUT>
__device__ __forceinline__ void nms_block(int layout, const float *__restrict__ data, uint32_t F, uint32_t N, float iou_thr, uint32_t *__restrict__ count,
                                          unsigned long long *__restrict__ gk, float4 *__restrict__ kb, uint32_t *__restrict__ ks,
                                          mi355_yolo_det *__restrict__ out, uint32_t max_dets, uint32_t *__restrict__ n_out,
                                          unsigned long long *lds_keys, NmsShared &S) {
  const int tid = threadIdx.x;
  const bool v8 = LAYOUT == 2 ? layout == MI355_YOLO_V8 : LAYOUT == 0;
  const uint32_t n_classes = v8 ? F - 4 : F - 5;
  if (tid == 0) {
    S.n = *count;
    *count = 0;   // zero again for the next call
  }
  for (uint32_t c = tid; c < n_classes; c += kNmsThreads) {
    S.run_lo[c] = 0;
    S.run_hi[c] = 0;
    S.kept[0][c] = 0;
  }
  __syncthreads();
  const uint32_t n = S.n < N ? S.n : N;   // S.n <= N: every candidate is appended at most once
  if (n == 0) {
    if (tid == 0) *n_out = 0;
    return;
  }
  const unsigned long long *K = sort_keys(lds_keys, gk, n);
  find_runs(K, n, n_classes, S);
  greedy_nms<LAYOUT>(layout, data, F, N, K, iou_thr, n_classes, kb, ks, S);
  write_records(K, n_classes, kb, ks, S, out, max_dets, n_out);
}

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
  nms_block<LAYOUT>(LAYOUT, tensors + (size_t)t * pitch_dwords, F, N, params[t].iou_threshold, count + t, keys + (size_t)t * key_pitch, kbox + (size_t)t * N,
                    ksrc + (size_t)t * N, dets + (size_t)t * max_dets, max_dets, n_dets + t, lds_keys, S);
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
  uint32_t first_block, blocks; // its tiles in the score launch of its layout (yolodec_set_plan)
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
  nms_block<2>(T.job[j].layout, T.job[j].data, T.job[j].F, T.job[j].N, T.job[j].p.iou_threshold, T.job[j].count, T.job[j].keys, T.job[j].kbox, T.job[j].ksrc,
               T.job[j].dets, T.job[j].max_dets, T.job[j].n_dets, lds_keys, S);
}

uint32_t pow2_at_least(uint32_t n) {
  uint32_t p = 1;
  while (p < n) p <<= 1;
  return p;
}

}  // namespace

// scratch of one context; grows to the largest shape seen
struct YoloDecState {
  uint32_t *d_count = nullptr;   // [tensors] survivors; zero between calls
  mi355_yolo_params *d_params = nullptr, *h_params = nullptr;
  uint32_t tensors = 0;
  bool count_zero = false;       // false after an allocation or an interrupted call: cleared before the next launch
  unsigned long long *d_keys = nullptr;
  float4 *d_kbox = nullptr;
  uint32_t *d_ksrc = nullptr;
  size_t key_elems = 0, kbox_elems = 0, ksrc_elems = 0;
  uint8_t *d_out = nullptr, *h_out = nullptr;   // [tensors] counts (padded to 64 bytes), then [tensors][max_dets] records
  size_t d_out_bytes = 0, h_out_bytes = 0;
  float *d_stage = nullptr;      // the host form's tensor
  size_t stage_floats = 0;
};

void yolodec_release(mi355_ctx *ctx) {
  auto *s = static_cast<YoloDecState *>(ctx->yolodec);
  if (!s) return;
  if (s->d_count) (void)hipFree(s->d_count);
  if (s->d_params) (void)hipFree(s->d_params);
  if (s->h_params) (void)hipHostFree(s->h_params);
  if (s->d_keys) (void)hipFree(s->d_keys);
  if (s->d_kbox) (void)hipFree(s->d_kbox);
  if (s->d_ksrc) (void)hipFree(s->d_ksrc);
  if (s->d_out) (void)hipFree(s->d_out);
  if (s->h_out) (void)hipHostFree(s->h_out);
  if (s->d_stage) (void)hipFree(s->d_stage);
  delete s;
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

template <typename T>
static int grow(mi355_ctx *ctx, T **p, size_t *have, size_t want, const char *what, bool host = false) {
  if (*have >= want && *p) return MI355_OK;
  if (*p) (void)(host ? hipHostFree(*p) : hipFree(*p));
  *p = nullptr;
  *have = 0;
  const hipError_t e = host ? hipHostMalloc((void **)p, want * sizeof(T), hipHostMallocDefault) : hipMalloc((void **)p, want * sizeof(T));
  const int rc = check_hip(ctx, e, what);
  if (rc) { *p = nullptr; return rc; }
  *have = want;
  return MI355_OK;
}

static size_t out_counts_bytes(uint32_t T) { return ((size_t)T * sizeof(uint32_t) + 63) / 64 * 64; }

static int yolodec_scratch(mi355_ctx *ctx, uint32_t T, uint32_t N, uint32_t max_dets, YoloDecState **out) {
  auto *s = static_cast<YoloDecState *>(ctx->yolodec);
  if (!s) ctx->yolodec = s = new YoloDecState();
  int rc = MI355_OK;
  if (s->tensors < T) {
    if (s->d_count) (void)hipFree(s->d_count);
    if (s->d_params) (void)hipFree(s->d_params);
    if (s->h_params) (void)hipHostFree(s->h_params);
    s->d_count = nullptr;
    s->d_params = s->h_params = nullptr;
    s->tensors = 0;
    s->count_zero = false;
    if ((rc = check_hip(ctx, hipMalloc((void **)&s->d_count, (size_t)T * sizeof(uint32_t)), "hipMalloc(yolodec counters)"))) return rc;
    if ((rc = check_hip(ctx, hipMalloc((void **)&s->d_params, (size_t)T * sizeof(mi355_yolo_params)), "hipMalloc(yolodec settings)"))) return rc;
    if ((rc = check_hip(ctx, hipHostMalloc((void **)&s->h_params, (size_t)T * sizeof(mi355_yolo_params), hipHostMallocDefault), "hipHostMalloc(yolodec settings)")))
      return rc;
    s->tensors = T;
  }
  const size_t key_pitch = pow2_at_least(N);
  if ((rc = grow(ctx, &s->d_keys, &s->key_elems, (size_t)T * key_pitch, "hipMalloc(yolodec keys)"))) return rc;
  if ((rc = grow(ctx, &s->d_kbox, &s->kbox_elems, (size_t)T * N, "hipMalloc(yolodec kept boxes)"))) return rc;
  if ((rc = grow(ctx, &s->d_ksrc, &s->ksrc_elems, (size_t)T * N, "hipMalloc(yolodec kept positions)"))) return rc;
  const size_t out_bytes = out_counts_bytes(T) + (size_t)T * max_dets * sizeof(mi355_yolo_det);
  if ((rc = grow(ctx, &s->d_out, &s->d_out_bytes, out_bytes, "hipMalloc(yolodec results)"))) return rc;
  if ((rc = grow(ctx, &s->h_out, &s->h_out_bytes, out_bytes, "hipHostMalloc(yolodec results)", true))) return rc;
  if (!s->count_zero) {
    if ((rc = check_hip(ctx, hipMemsetAsync(s->d_count, 0, (size_t)s->tensors * sizeof(uint32_t), ctx->stream), "hipMemsetAsync(yolodec)"))) return rc;
    s->count_zero = true;
  }
  *out = s;
  return MI355_OK;
}

// settings up, the two launches, results down, one synchronisation; d_tensors is checked
static int yolodec_run(mi355_ctx *ctx, YoloDecState *s, const float *d_tensors, size_t pitch_bytes, uint32_t T, int layout, uint32_t F, uint32_t N,
                       const mi355_yolo_params *p, mi355_yolo_det *dets, uint32_t max_dets, uint32_t *n_dets) {
  int rc = MI355_OK;
  std::memcpy(s->h_params, p, (size_t)T * sizeof(mi355_yolo_params));
  if ((rc = check_hip(ctx, hipMemcpyAsync(s->d_params, s->h_params, (size_t)T * sizeof(mi355_yolo_params), hipMemcpyHostToDevice, ctx->stream), "yolodec settings H2D")))
    return rc;
  __atomic_fetch_add(&ctx->n_h2d, 1ull, __ATOMIC_RELAXED);
  const size_t key_pitch = pow2_at_least(N), pitch_dwords = pitch_bytes / 4;
  uint32_t *d_n = reinterpret_cast<uint32_t *>(s->d_out);
  mi355_yolo_det *d_dets = reinterpret_cast<mi355_yolo_det *>(s->d_out + out_counts_bytes(T));
  const dim3 grid((N + kScoreThreads - 1) / kScoreThreads, T);
  s->count_zero = false;   // true again only once the NMS kernel has been enqueued behind the score kernel
  if (layout == MI355_YOLO_V8)
    hipLaunchKernelGGL(yolodec_score_kernel<0>, grid, dim3(kScoreThreads), 0, ctx->stream, reinterpret_cast<const uint32_t *>(d_tensors), pitch_dwords, F, N,
                       s->d_params, s->d_count, s->d_keys, key_pitch);
  else
    hipLaunchKernelGGL(yolodec_score_kernel<1>, grid, dim3(kScoreThreads), 0, ctx->stream, reinterpret_cast<const uint32_t *>(d_tensors), pitch_dwords, F, N,
                       s->d_params, s->d_count, s->d_keys, key_pitch);
  if ((rc = check_hip(ctx, hipGetLastError(), "yolodec score launch"))) return rc;
  if (layout == MI355_YOLO_V8)
    hipLaunchKernelGGL(yolodec_nms_kernel<0>, dim3(T), dim3(kNmsThreads), 0, ctx->stream, d_tensors, pitch_dwords, F, N, s->d_params, s->d_count, s->d_keys, key_pitch,
                       s->d_kbox, s->d_ksrc, d_dets, max_dets, d_n);
  else
    hipLaunchKernelGGL(yolodec_nms_kernel<1>, dim3(T), dim3(kNmsThreads), 0, ctx->stream, d_tensors, pitch_dwords, F, N, s->d_params, s->d_count, s->d_keys, key_pitch,
                       s->d_kbox, s->d_ksrc, d_dets, max_dets, d_n);
  if ((rc = check_hip(ctx, hipGetLastError(), "yolodec nms launch"))) return rc;
  const size_t bytes = out_counts_bytes(T) + (size_t)T * max_dets * sizeof(mi355_yolo_det);
  if ((rc = check_hip(ctx, hipMemcpyAsync(s->h_out, s->d_out, bytes, hipMemcpyDeviceToHost, ctx->stream), "yolodec D2H"))) return rc;
  __atomic_fetch_add(&ctx->n_d2h, 1ull, __ATOMIC_RELAXED);
  if ((rc = check_hip(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize"))) return rc;
  s->count_zero = true;
  const uint32_t *h_n = reinterpret_cast<const uint32_t *>(s->h_out);
  const mi355_yolo_det *h_dets = reinterpret_cast<const mi355_yolo_det *>(s->h_out + out_counts_bytes(T));
  for (uint32_t t = 0; t < T; t++) {
    n_dets[t] = h_n[t];
    const uint32_t w = h_n[t] < max_dets ? h_n[t] : max_dets;
    if (w) std::memcpy(dets + (size_t)t * max_dets, h_dets + (size_t)t * max_dets, (size_t)w * sizeof(mi355_yolo_det));
  }
  return MI355_OK;
}

// ---- launch sets of the video group's decoder queue

// the layout of one set (mi355_selftest_yolodec_set_plan; yolodec_launch_set lays its scratch out with it)
int yolodec_set_plan(int n_jobs, const int *layout, const uint32_t *num_fields, const uint32_t *num_candidates, const uint32_t *max_dets, uint32_t *first_block,
                     uint32_t *blocks, uint64_t *key_offset, uint64_t *box_offset, uint64_t *det_offset, uint64_t totals[6]) {
  if (n_jobs < 0 || n_jobs > kYdSetMax || !totals) return MI355_ERR_INVALID_ARG;
  if (n_jobs > 0 && (!layout || !num_fields || !num_candidates || !max_dets || !first_block || !blocks || !key_offset || !box_offset || !det_offset))
    return MI355_ERR_INVALID_ARG;
  for (int j = 0; j < n_jobs; j++) {
    const char *why = nullptr;
    const int rc = yolodec_check_args((size_t)num_fields[j] * num_candidates[j] * 4, 1, layout[j], num_fields[j], num_candidates[j], &why);
    if (rc) return rc;
  }
  uint64_t t[6] = {0, 0, 0, 0, 0, 0};   // V8 blocks, X blocks, NMS blocks, keys, boxes, records
  for (int j = 0; j < n_jobs; j++) {
    const uint32_t N = num_candidates[j];
    uint64_t &layout_blocks = t[layout[j] == MI355_YOLO_V8 ? 0 : 1];
    blocks[j] = (N + kScoreThreads - 1) / kScoreThreads;
    first_block[j] = (uint32_t)layout_blocks;   // at most 32 * 256 blocks
    layout_blocks += blocks[j];
    if (N) t[2]++;
    key_offset[j] = t[3];
    t[3] += pow2_at_least(N);
    box_offset[j] = t[4];
    t[4] += N;
    det_offset[j] = t[5];
    t[5] += max_dets[j] < N ? max_dets[j] : N;
  }
  for (int k = 0; k < 6; k++) totals[k] = t[k];
  return MI355_OK;
}

// scratch of one queue; grows to the largest set seen
struct YdSetScratch {
  uint32_t *d_count = nullptr;   // [kYdSetMax] survivors; zero between sets
  bool count_zero = false;       // false after the allocation or an interrupted set: cleared before the next launch
  unsigned long long *d_keys = nullptr;
  float4 *d_kbox = nullptr;
  uint32_t *d_ksrc = nullptr;
  uint8_t *d_out = nullptr;      // [kYdSetMax] counts (kYdCountsBytes), then the jobs' records at their det_offset
  size_t key_elems = 0, kbox_elems = 0, ksrc_elems = 0, out_bytes = 0;
};

YdSetScratch *yolodec_set_scratch_new(int *status, std::string *err) {
  auto *S = new YdSetScratch();
  if (hipMalloc((void **)&S->d_count, (size_t)kYdSetMax * sizeof(uint32_t)) != hipSuccess) {
    (void)hipGetLastError();
    delete S;
    *status = MI355_ERR_OUT_OF_MEMORY;
    *err = "hipMalloc(yolodec set counters)";
    return nullptr;
  }
  *status = MI355_OK;
  return S;
}

void yolodec_set_scratch_free(YdSetScratch *S) {
  if (!S) return;
  if (S->d_count) (void)hipFree(S->d_count);
  if (S->d_keys) (void)hipFree(S->d_keys);
  if (S->d_kbox) (void)hipFree(S->d_kbox);
  if (S->d_ksrc) (void)hipFree(S->d_ksrc);
  if (S->d_out) (void)hipFree(S->d_out);
  delete S;
}

// (hipFree waits for the device: a set still running on the queue's stream has finished with the old allocation)
template <typename T>
static bool set_grow(T **p, size_t *have, size_t want) {
  if (*have >= want && *p) return true;
  if (*p) (void)hipFree(*p);
  *p = nullptr;
  *have = 0;
  if (hipMalloc((void **)p, want * sizeof(T)) != hipSuccess) { (void)hipGetLastError(); *p = nullptr; return false; }
  *have = want;
  return true;
}

size_t yolodec_set_result_bytes(uint64_t records) { return kYdCountsBytes + (size_t)records * sizeof(mi355_yolo_det); }

int yolodec_launch_set(YdSetScratch *S, hipStream_t stream, const YdTensor *tensors, int n, void *h_block, size_t h_block_bytes, int *kernel_launches,
                       std::string *err) {
  *kernel_launches = 0;
  if (!S || !tensors || n < 1 || n > kYdSetMax) { *err = "yolodec: bad launch set"; return MI355_ERR_INVALID_ARG; }
  int layout[kYdSetMax];
  uint32_t F[kYdSetMax], N[kYdSetMax], cap[kYdSetMax], first[kYdSetMax], blocks[kYdSetMax];
  uint64_t key_off[kYdSetMax], box_off[kYdSetMax], det_off[kYdSetMax], totals[6];
  for (int i = 0; i < n; i++) { layout[i] = tensors[i].layout; F[i] = tensors[i].num_fields; N[i] = tensors[i].num_candidates; cap[i] = tensors[i].max_dets; }
  const int rc = yolodec_set_plan(n, layout, F, N, cap, first, blocks, key_off, box_off, det_off, totals);
  if (rc) { *err = "yolodec: bad launch set"; return rc; }
  if (totals[2] == 0) return MI355_OK;   // no job has a candidate: nothing to launch, nothing to copy
  const size_t bytes = yolodec_set_result_bytes(totals[5]);
  if (!h_block || h_block_bytes < bytes) { *err = "yolodec: the pinned result block is too small for the set"; return MI355_ERR_INVALID_ARG; }
  if (!set_grow(&S->d_keys, &S->key_elems, (size_t)totals[3]) || !set_grow(&S->d_kbox, &S->kbox_elems, (size_t)totals[4]) ||
      !set_grow(&S->d_ksrc, &S->ksrc_elems, (size_t)totals[4]) || !set_grow(&S->d_out, &S->out_bytes, bytes)) {
    *err = "hipMalloc(yolodec set scratch)";
    return MI355_ERR_OUT_OF_MEMORY;
  }
  if (!S->count_zero) {
    if (hipMemsetAsync(S->d_count, 0, (size_t)kYdSetMax * sizeof(uint32_t), stream) != hipSuccess) { *err = "hipMemsetAsync(yolodec set counters)"; return MI355_ERR_HIP; }
    S->count_zero = true;
  }
  YdJobTable score[2] = {}, nms = {};
  uint32_t *d_n = reinterpret_cast<uint32_t *>(S->d_out);
  mi355_yolo_det *d_dets = reinterpret_cast<mi355_yolo_det *>(S->d_out + kYdCountsBytes);
  for (int i = 0; i < n; i++) {
    if (!N[i]) continue;   // no candidate: no job
    YdJob J;
    J.data = tensors[i].data;
    J.count = S->d_count + i;
    J.keys = S->d_keys + key_off[i];
    J.kbox = S->d_kbox + box_off[i];
    J.ksrc = S->d_ksrc + box_off[i];
    J.dets = d_dets + det_off[i];
    J.n_dets = d_n + i;
    J.F = F[i];
    J.N = N[i];
    J.key_cap = pow2_at_least(N[i]);
    J.max_dets = cap[i];
    J.first_block = first[i];
    J.blocks = blocks[i];
    J.layout = layout[i];
    J.p = tensors[i].p;
    YdJobTable &T = score[layout[i] == MI355_YOLO_V8 ? 0 : 1];
    T.job[T.n_jobs++] = J;
    nms.job[nms.n_jobs++] = J;
  }
  S->count_zero = false;   // true again only once the NMS launch has been enqueued behind the score launches
  for (int l = 0; l < 2; l++) {
    if (!score[l].n_jobs) continue;
    const dim3 grid((uint32_t)totals[l]);
    if (l == 0) hipLaunchKernelGGL(yolodec_score_jobs_kernel<0>, grid, dim3(kScoreThreads), 0, stream, score[l]);
    else hipLaunchKernelGGL(yolodec_score_jobs_kernel<1>, grid, dim3(kScoreThreads), 0, stream, score[l]);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { *err = std::string("yolodec score jobs kernel launch: ") + hipGetErrorString(e); return MI355_ERR_HIP; }
    (*kernel_launches)++;
  }
  hipLaunchKernelGGL(yolodec_nms_jobs_kernel, dim3((uint32_t)nms.n_jobs), dim3(kNmsThreads), 0, stream, nms);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { *err = std::string("yolodec nms jobs kernel launch: ") + hipGetErrorString(e); return MI355_ERR_HIP; }
  (*kernel_launches)++;
  S->count_zero = true;
  e = hipMemcpyAsync(h_block, S->d_out, bytes, hipMemcpyDeviceToHost, stream);
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
  if ((rc = grow(ctx, &s->d_stage, &s->stage_floats, bytes / 4, "hipMalloc(yolodec staging)"))) return rc;
  if ((rc = check_hip(ctx, hipMemcpyAsync(s->d_stage, data, bytes, hipMemcpyHostToDevice, ctx->stream), "yolodec H2D"))) return rc;
  __atomic_fetch_add(&ctx->n_h2d, 1ull, __ATOMIC_RELAXED);
  return yolodec_run(ctx, s, s->d_stage, bytes, 1, layout, num_fields, num_candidates, p, dets, max_dets, n_dets);
}

int mi355_selftest_yolodec_check(size_t tensor_pitch_bytes, int n_tensors, int layout, uint32_t num_fields, uint32_t num_candidates) {
  const char *why = nullptr;
  return yolodec_check_args(tensor_pitch_bytes, n_tensors, layout, num_fields, num_candidates, &why);
}

int mi355_selftest_yolodec_set_plan(int n_jobs, const int *layout, const uint32_t *num_fields, const uint32_t *num_candidates, const uint32_t *max_dets,
                                    uint32_t *first_block, uint32_t *blocks, uint64_t *key_offset, uint64_t *box_offset, uint64_t *det_offset, uint64_t totals[6]) {
  return yolodec_set_plan(n_jobs, layout, num_fields, num_candidates, max_dets, first_block, blocks, key_offset, box_offset, det_offset, totals);
}

}  // extern "C"
