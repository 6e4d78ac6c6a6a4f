// yolodec_device.hpp - the device functions and the per-context scratch that the tensor decoders (yolodec.hip) and the YOLOX head
// decoder (yolox_head.hip) share: the survivor key (11 bits class | 32 bits inverted total_cmp key of the confidence | 16 bits
// candidate - ascending key order is the output order) and the NMS block - bitonic sort of the keys, class runs, greedy NMS per run,
// records. What differs between the callers is where a candidate's box comes from: nms_block takes a loader,
// `Box load(uint32_t candidate)`. The primitives the hand decoders use as well (total_key and its inverse, cast_i32, Box, kPadKey,
// pow2_at_least, the wave-aggregated append_keys) are in decode_device.hpp.
#pragma once
#include "decode_device.hpp"
#include "internal.hpp"

namespace mi355 {

namespace {

constexpr int kScoreThreads = 256;
constexpr int kNmsThreads = 512;
constexpr int kNmsWaves = kNmsThreads / 64;
constexpr int kLdsSortKeys = 4096;
constexpr uint32_t kMaxFields = 1029, kMaxCandidates = 65536, kMaxTensors = 1024;
constexpr int kMaxClasses = 1025;       // V8 at F = 1029

static_assert(sizeof(mi355_yolo_det) == 48, "mi355_yolo_det is 48 bytes");
static_assert(sizeof(mi355_yolo_params) == 12, "mi355_yolo_params is three floats");

__device__ __forceinline__ unsigned long long make_key(uint32_t cls, uint32_t conf_bits, uint32_t cand) {
  const uint32_t asc = (uint32_t)total_key(conf_bits) ^ 0x80000000u;   // unsigned, ascending with the confidence
  return ((unsigned long long)cls << 48) | ((unsigned long long)(~asc) << 16) | (unsigned long long)cand;
}
__device__ __forceinline__ uint32_t key_class(unsigned long long k) { return (uint32_t)(k >> 48); }
__device__ __forceinline__ uint32_t key_cand(unsigned long long k) { return (uint32_t)(k & 0xffffu); }
__device__ __forceinline__ uint32_t key_conf_bits(unsigned long long k) { return total_key_bits((~(uint32_t)(k >> 16)) ^ 0x80000000u); }

// max_by's fold: a later element replaces the best unless it is smaller
__device__ __forceinline__ void fold_class(uint32_t bits, uint32_t cls, int32_t &best_key, uint32_t &best_bits, uint32_t &best_cls) {
  const int32_t k = total_key(bits);
  if (k >= best_key) {
    best_key = k;
    best_bits = bits;
    best_cls = cls;
  }
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

// imp.rs:318-323, :347-352: the corners of a centre / size box, unfused
__device__ __forceinline__ Box centre_box(float x, float y, float w, float h) {
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

struct NmsShared {
  uint32_t run_lo[kMaxClasses], run_hi[kMaxClasses];   // the class's run in the sorted keys: [lo, hi), both 0 when it has none
  uint32_t kept[2][kMaxClasses + 1];                   // kept boxes per class, then their exclusive prefix sums (ping-pong)
  uint32_t n;
};

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
template <class LoadBox>
__device__ __forceinline__ void greedy_nms(const LoadBox &load, const unsigned long long *K, float iou_thr, uint32_t n_classes, float4 *kb, uint32_t *ks,
                                           NmsShared &S) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (uint32_t c = wave; c < n_classes; c += kNmsWaves) {
    const uint32_t lo = S.run_lo[c], hi = S.run_hi[c];
    uint32_t m = 0;   // boxes kept so far in this run (wave-uniform)
    for (uint32_t base = lo; base < hi; base += 64) {
      const uint32_t i = base + (uint32_t)lane;
      bool alive = i < hi;
      Box b = {0.0f, 0.0f, 0.0f, 0.0f};
      if (alive) b = load(key_cand(K[i]));
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
// gk: at least the power of two above N keys; load(c): the box of candidate c. Shared by the lone kernels and the job-table kernel.
template <class LoadBox>
__device__ __forceinline__ void nms_block(const LoadBox &load, uint32_t n_classes, uint32_t N, float iou_thr, uint32_t *__restrict__ count,
                                          unsigned long long *__restrict__ gk, float4 *__restrict__ kb, uint32_t *__restrict__ ks,
                                          mi355_yolo_det *__restrict__ out, uint32_t max_dets, uint32_t *__restrict__ n_out,
                                          unsigned long long *lds_keys, NmsShared &S) {
  const int tid = threadIdx.x;
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
  greedy_nms(load, K, iou_thr, n_classes, kb, ks, S);
  write_records(K, n_classes, kb, ks, S, out, max_dets, n_out);
}

}  // namespace

// scratch of one context; grows to the largest shape seen. Both decoders' calls use it: they run one after the other on the
// context's stream and each leaves the counters at zero.
struct YoloDecState {
  DeviceBuf<uint32_t> d_count;   // [tensors] survivors; zero between calls
  DeviceBuf<mi355_yolo_params> d_params;   // as many as d_count holds, and as many in h_params
  PinnedBuf<mi355_yolo_params> h_params;
  bool count_zero = false;       // false after an allocation or an interrupted call: cleared before the next launch
  DeviceBuf<unsigned long long> d_keys;
  DeviceBuf<float4> d_kbox;
  DeviceBuf<uint32_t> d_ksrc;
  DeviceBuf<uint8_t> d_out;      // [tensors] counts (padded to 64 bytes), then [tensors][max_dets] records
  PinnedBuf<uint8_t> h_out;
  DeviceBuf<float> d_stage;      // the host form's tensor
};

// counters (zero on return, or cleared on the stream), settings, keys, kept boxes and positions, results for T tensors of N candidates
int yolodec_scratch(mi355_ctx *ctx, uint32_t T, uint32_t N, uint32_t max_dets, YoloDecState **out);
// grows the host forms' staging to at least `floats`
int yolodec_stage(mi355_ctx *ctx, YoloDecState *s, size_t floats);
// the T settings to s->d_params on the context's stream
int yolodec_upload_params(mi355_ctx *ctx, YoloDecState *s, uint32_t T, const mi355_yolo_params *p);
// where the NMS launch writes: T counts, then T x max_dets records
inline uint32_t *yolodec_d_counts(YoloDecState *s) { return reinterpret_cast<uint32_t *>(s->d_out.p); }
mi355_yolo_det *yolodec_d_dets(YoloDecState *s, uint32_t T);
// results down, one synchronisation, the caller's arrays filled
int yolodec_download(mi355_ctx *ctx, YoloDecState *s, uint32_t T, mi355_yolo_det *dets, uint32_t max_dets, uint32_t *n_dets);

// ---- the head members of a decoder launch set (the video group's decoder queue): yolodec_launch_set builds the two tables in the
// set's pinned block and uploads them in one copy; the job kernels of yolox_head.hip read them from device memory (32 heads x 8
// levels do not fit the kernel arguments). A level job is one level of one head; every field a block reads is block-uniform.
struct YhHeadJob {
  uint32_t *count;              // the head's survivor counter; zero on entry to the score launch, left at zero by the NMS launch
  unsigned long long *keys;     // key_cap entries
  float4 *kbox;                 // A entries
  uint32_t *ksrc;               // A entries
  mi355_yolo_det *dets;         // min(max_dets, A) records
  uint32_t *n_dets;
  uint32_t A, C, key_cap, max_dets;
  uint32_t first_level, n_levels;   // its level jobs: level[first_level .. first_level + n_levels)
  mi355_yolo_params p;
  uint32_t pad;
  uint32_t start[MI355_YOLOX_LEVELS_MAX];   // first candidate of level l; A from n_levels on
};
struct YhLevelJob {
  const float *reg, *obj, *cls;
  uint32_t w, hw;               // hw = h * w
  uint32_t first_cand;          // candidate index of the level's element 0
  uint32_t first_block;         // its first tile in the head score launch; tiles are 256 candidates of this level
  uint32_t head;                // index into YhTable::head
  float stride;
};
constexpr int kYhLevelJobsMax = kYdSetMax * MI355_YOLOX_LEVELS_MAX;
struct YhTable {
  YhHeadJob head[kYdSetMax];
  YhLevelJob level[kYhLevelJobsMax];   // in first_block order; the upload ends behind the last one used
};
static_assert(sizeof(YhHeadJob) == 120 && sizeof(YhLevelJob) == 48, "the head tables have no padding holes");
inline size_t yh_table_bytes(uint64_t level_jobs) { return level_jobs ? offsetof(YhTable, level) + (size_t)level_jobs * sizeof(YhLevelJob) : 0; }
// A conversion job of the decoder queue's infer members (yolox_input_jobs_kernel): one RGB frame of a member - its own base pointer
// and stride - into frame `frame_in_class` of its class's lane input tensor, [3][H][W] f32. The jobs of a set stand behind its level
// jobs, in the same upload, in first_block order.
struct YxConvJob {
  const uint8_t *src;
  float *dst;
  unsigned long long stride;   // bytes from row to row of src
  uint32_t W, H;               // multiples of 32
  uint32_t first_block;        // its first block in the conversion launch; a block is 256 lanes of 4 pixels
  uint32_t pad;
};
static_assert(sizeof(YxConvJob) == 40, "the conversion jobs have no padding holes");
// where the conversion jobs stand in the uploaded bytes, and the bytes of the upload (0: the set has neither a head nor an infer member)
inline size_t yx_conv_offset(uint64_t level_jobs) { return (yh_table_bytes(level_jobs ? level_jobs : 1) + 15) / 16 * 16; }
inline size_t yh_upload_bytes(uint64_t level_jobs, uint64_t conv_jobs) {
  return conv_jobs ? yx_conv_offset(level_jobs) + (size_t)conv_jobs * sizeof(YxConvJob) : yh_table_bytes(level_jobs);
}
constexpr size_t kYhUploadMax = (sizeof(YhTable) + 15) / 16 * 16 + (size_t)kYdSetMax * sizeof(YxConvJob);
// the conversion launch over uploaded jobs: one flat grid of total_blocks
int yolox_input_launch_jobs(hipStream_t stream, const YxConvJob *d_jobs, uint32_t n_jobs, uint32_t total_blocks, int *kernel_launches, std::string *err);
// the two launches over uploaded tables: the score launch (grid = score_blocks, the level jobs' tiles), the NMS launch (a block per head)
int yolox_head_launch_jobs(hipStream_t stream, const YhTable *d_table, uint32_t n_heads, uint32_t n_level_jobs, uint32_t score_blocks, int *kernel_launches,
                           std::string *err);

}  // namespace mi355
