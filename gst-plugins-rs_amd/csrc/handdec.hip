// handdec.hip — the device side of `handdetectiontensordec` / `handlandmarktensordec`: the decode loops of
// analytics/analytics/src/hand/handdetectiontensordec/imp.rs:89-335, hand/handlandmarktensordec/imp.rs:101-391 and
// hand/helper.rs:69-114. Bit-exact against the contract of DESIGN §4.12 (tests/handdec_restate.py and tools/handdec_cpu.cpp restate
// it independently). All arithmetic is f32 and unfused.
//   palm       row = score, cx, cy, size, kp0x, kp0y, kp2x, kp2y. Dropped iff score < confidence_threshold (IEEE: a NaN stays), then
//              iff size <= 0 (:143-157). rotation = FRAC_PI_2 + atan2(kp2y - kp0y, kp2x - kp0x) (:214-218), rr = 2.9 * size,
//              center_x = cx + (0.5 * size) * sin(rotation), center_y = cy - (0.5 * size) * cos(rotation) (:160-162), the validity
//              test literally (:231-296), the frame scaling (:177-183), the box center -+ rr / 2 (:185-189).
//   landmarks  hand i: confidence scores[i] if i < num_scores else 1.0, dropped iff confidence < threshold (:274-280); the box is
//              min / max over the finite (x, y) pairs, dropped when there is none or width or height <= 0, padded by 0.15 * width and
//              0.15 * height (:171-237). The sign of a zero min or max reaches no output: width and height are > 0, so min - pad is
//              negative and max + pad positive, whichever zero it was. rotation from points 0 and 9 unchecked (:148-169).
//   order      descending score under f32::total_cmp; sort_by is stable, so equal keys stay in ascending row index (:316, :297).
//   NMS        greedy over the whole list as one class: skipped iff iou(candidate, kept) > thr for some kept box; thr is
//              clamp(nms_iou_threshold, 0, 1) for palm (:315) and the plain setting for landmarks (:303). Stops at max_hands.
//   record     oriented_od_params_from_bbox_and_rotation (helper.rs:69-114): floor / ceil, only boxes fully outside the frame are
//              dropped, `as i32` (toward zero, saturating), rotation + (-FRAC_PI_2). None: has_od = 0; the hand still counted and
//              still suppressed. Keypoints (:337-373): the finite points in order, compacted.
// Three stated deviations:
//   a. atan2 / sin / cos are the f64 functions of the f32 arguments, rounded once to f32 (the reference's f32 libm differs in the
//      last bit between platforms). Computed only for candidates that passed the score and size tests.
//   b. iou is RESTATED WITHOUT SOURCE, PARITY UNPINNED (gst_analytics::image_util::iou_f32 is not in the reference tree): rects
//      (x, y, w = max - min, h = max - min), right = x + w, bottom = y + h, iw = max(0, min(rights) - max(lefts)), ih likewise,
//      inter = iw * ih, union = aw * ah + bw * bh - inter, union > 0 ? inter / union : 0; max / min are maxNum / minNum.
//   c. sign and payload of a NaN that arithmetic PRODUCES are the hardware's.
//
//   handdec_palm_kernel      one block of 1024 threads per tensor. The score and size tests run on every row and the rows that pass are
//                            compacted in LDS (one LDS atomic per wave), so the f64 functions run in full waves over those rows alone;
//                            lanes then load whole 32-byte rows as two 16-byte loads and apply the candidate rules; survivors' keys
//                            (32 bits inverted total_cmp key of the score | row) go to an LDS list, again one atomic per wave; bitonic
//                            sort of the list padded to a power of two (in-wave steps in registers); one wave walks the sorted list in
//                            chunks of 64 against the kept boxes (at most 8, in LDS), resolves each chunk in order with ballots and stops at
//                            max_hands; the selected lanes write the records. A candidate's box is computed again from its row in
//                            the walk (the same device function, so the same bits): no per-candidate storage.
//   handdec_landmark_kernel  one block per tensor, one wave per hand in turn: lanes 0-20 load a point each, wave min / max over the
//                            finite points, box and rotation into LDS by hand index; then the same key list, sort and selection.
//                            Selected hands write their box record and their compacted keypoint record (assembled in LDS).
//   handdec_palm_jobs_kernel / handdec_landmark_jobs_kernel  the same two bodies (palm_decode, landmark_decode) over a job table in the
//                            kernel arguments: block b decodes job b - its own tensor, shape and settings - into the result slab of a
//                            launch set of the video group's hand-decoder queue (handdec_launch_set, group.hip). No upload per set.
// total_key and its inverse, cast_i32, Box, kPadKey and the wave-aggregated append_keys are decode_device.hpp's, shared with the YOLO
// decoders; the key layout (score | index), the IoU, the in-wave register sort and select_hands are this file's own.
#include "decode_device.hpp"
#include "internal.hpp"

#include <cstddef>
#include <cstring>

namespace mi355 {

namespace {

constexpr int kPalmThreads = 1024;   // 4096 rows in four steps; 16 waves share the sort
constexpr int kThreads = 256;        // landmarks: a wave per hand, few hands
constexpr int kWaves = kThreads / 64;
constexpr uint32_t kMaxRows = 4096, kMaxHands = 1024, kMaxDim = 16, kMaxTensors = 1024, kMaxScores = 1024;
constexpr uint32_t kPalmMaxHands = 8, kLandmarkMaxHands = MI355_HAND_MAX;

constexpr float kFracPi2 = 1.57079632679489661923f;   // f32::consts::FRAC_PI_2
constexpr float kPalmMinRr = 0.06f, kPalmMaxRr = 1.40f, kPalmMinVisible = 0.5f, kPalmMinSpan = 0.15f, kPalmMaxSpan = 1.60f;
constexpr float kHandPad = 0.15f;

static_assert(sizeof(mi355_hand_params) == 20, "mi355_hand_params is five words");
static_assert(sizeof(mi355_hand_det) == 64, "mi355_hand_det is 64 bytes");
static_assert(sizeof(mi355_hand_keypoints) == 288, "mi355_hand_keypoints is 288 bytes");
static_assert(offsetof(mi355_hand_keypoints, confidences) == 172 && offsetof(mi355_hand_keypoints, visibilities) == 256, "mi355_hand_keypoints layout");

typedef float float4u __attribute__((ext_vector_type(4), aligned(4)));   // a 16-byte load from a 4-byte aligned address

// ascending key order is the output order: score descending, then index ascending
__device__ __forceinline__ unsigned long long make_key(uint32_t score_bits, uint32_t index) {
  const uint32_t asc = (uint32_t)total_key(score_bits) ^ 0x80000000u;
  return ((unsigned long long)(~asc) << 32) | (unsigned long long)index;
}
__device__ __forceinline__ uint32_t key_index(unsigned long long k) { return (uint32_t)k; }
__device__ __forceinline__ uint32_t key_score_bits(unsigned long long k) { return total_key_bits((~(uint32_t)(k >> 32)) ^ 0x80000000u); }

__device__ __forceinline__ bool finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// deviation a: the f64 function of the f32 arguments, rounded once
__device__ __forceinline__ float atan2_c(float y, float x) { return (float)atan2((double)y, (double)x); }
__device__ __forceinline__ float sin_c(float v) { return (float)sin((double)v); }
__device__ __forceinline__ float cos_c(float v) { return (float)cos((double)v); }

// deviation b
__device__ __forceinline__ float iou(const Box &a, const Box &b) {
  const float aw = a.xmax - a.xmin, ah = a.ymax - a.ymin, bw = b.xmax - b.xmin, bh = b.ymax - b.ymin;
  const float iw = fmaxf(0.0f, fminf(a.xmin + aw, b.xmin + bw) - fmaxf(a.xmin, b.xmin));
  const float ih = fmaxf(0.0f, fminf(a.ymin + ah, b.ymin + bh) - fmaxf(a.ymin, b.ymin));
  const float inter = iw * ih;
  const float uni = aw * ah + bw * bh - inter;
  return uni > 0.0f ? inter / uni : 0.0f;
}

// a palm row that passed the score test -> its box and rotation, or false (imp.rs:147-189, :231-296)
__device__ __forceinline__ bool palm_candidate(const float4u r0, const float4u r1, const mi355_hand_params &P, Box &box, float &rotation) {
  const float cx = r0.y, cy = r0.z, size = r0.w, kp0x = r1.x, kp0y = r1.y, kp2x = r1.z, kp2y = r1.w;
  if (size <= 0.0f) return false;
  const float kdx = kp2x - kp0x, kdy = kp2y - kp0y;
  rotation = kFracPi2 + atan2_c(kdy, kdx);
  float rr = 2.9f * size;
  float center_x = cx + (0.5f * size) * sin_c(rotation);
  float center_y = cy - (0.5f * size) * cos_c(rotation);
  if (!finite(center_x) || !finite(center_y) || !finite(rr) || !finite(size) || !finite(kp0x) || !finite(kp0y) || !finite(kp2x) || !finite(kp2y)) return false;
  if (!(kPalmMinRr <= rr && rr <= kPalmMaxRr)) return false;
  if (!(0.0f <= center_x && center_x <= 1.0f) || !(0.0f <= center_y && center_y <= 1.0f)) return false;
  const float span = __fsqrt_rn(kdx * kdx + kdy * kdy);
  const float ratio = span / size;
  if (!(kPalmMinSpan <= ratio && ratio <= kPalmMaxSpan)) return false;
  const float hs = rr * 0.5f;
  const float x0 = center_x - hs, y0 = center_y - hs, x1 = center_x + hs, y1 = center_y + hs;
  const float area = fmaxf(x1 - x0, 0.0f) * fmaxf(y1 - y0, 0.0f);
  if (area <= 0.0f) return false;
  const float ix0 = fmaxf(x0, 0.0f), iy0 = fmaxf(y0, 0.0f), ix1 = fminf(x1, 1.0f), iy1 = fminf(y1, 1.0f);
  const float inter = fmaxf(ix1 - ix0, 0.0f) * fmaxf(iy1 - iy0, 0.0f);
  if (!(inter / area >= kPalmMinVisible)) return false;
  if (P.frame_width > 0) {   // both or neither: checked by the host
    const float w = (float)P.frame_width, h = (float)P.frame_height;
    center_x = center_x * w;
    center_y = center_y * h;
    rr = rr * fmaxf(w, h);
  }
  const float half = rr / 2.0f;
  box.xmin = center_x - half;
  box.ymin = center_y - half;
  box.xmax = center_x + half;
  box.ymax = center_y + half;
  return true;
}

// helper.rs:69-114 into the record's x, y, width, height, rotation_od, has_od
__device__ __forceinline__ void oriented_od(const Box &b, float rotation, const mi355_hand_params &P, mi355_hand_det &d) {
  d.x = d.y = d.width = d.height = 0;
  d.rotation_od = 0.0f;
  d.has_od = 0;
  if (!finite(b.xmin) || !finite(b.ymin) || !finite(b.xmax) || !finite(b.ymax)) return;
  const float x0 = floorf(b.xmin), y0 = floorf(b.ymin), x1 = ceilf(b.xmax), y1 = ceilf(b.ymax);
  if (x1 <= x0 || y1 <= y0) return;
  if (P.frame_width > 0 && P.frame_height > 0) {
    const float fw = (float)P.frame_width, fh = (float)P.frame_height;
    if (x1 <= 0.0f || y1 <= 0.0f || x0 >= fw || y0 >= fh) return;
  }
  const int32_t x = cast_i32(x0), y = cast_i32(y0), w = cast_i32(x1 - x0), h = cast_i32(y1 - y0);
  if (w <= 0 || h <= 0) return;
  d.x = x;
  d.y = y;
  d.width = w;
  d.height = h;
  d.rotation_od = rotation + (-kFracPi2);
  d.has_od = 1;
}

// the bitonic steps j = j0, j0 / 2, ... 1 (j0 <= 32) of stage k for element i, whose partners i ^ j all lie in the wave: in registers
__device__ __forceinline__ unsigned long long wave_steps(unsigned long long a, uint32_t i, uint32_t k, uint32_t j0) {
  const bool up = (i & k) == 0;
  for (uint32_t j = j0; j > 0; j >>= 1) {
    const unsigned long long b = __shfl_xor(a, (int)j);
    const bool keep_min = ((i & j) == 0) == up;
    a = keep_min ? (a < b ? a : b) : (a > b ? a : b);
  }
  return a;
}

// the n keys padded to a power of two and sorted ascending (bitonic) by the whole block of THREADS; ends in a barrier. A wave holds 64
// consecutive keys, so the steps with j <= 32 run in registers through shuffles and only the steps with j >= 64 cross waves through LDS
// and a barrier: 256 keys take 6 barriers, not 36.
template <int THREADS>
__device__ __forceinline__ void sort_keys(unsigned long long *K, uint32_t n) {
  uint32_t n2 = 1;
  while (n2 < n) n2 <<= 1;
  for (uint32_t i = n + threadIdx.x; i < n2; i += THREADS) K[i] = kPadKey;
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u, first = threadIdx.x - lane;
  // stages k = 2 .. 64 (every step inside the wave)
  for (uint32_t i0 = first; i0 < n2; i0 += THREADS) {   // wave-uniform: every lane takes part in the shuffles
    const uint32_t i = i0 + lane;
    unsigned long long a = i < n2 ? K[i] : kPadKey;   // (n2 < 64: the lanes from n2 on only accompany)
    for (uint32_t k = 2; k <= 64 && k <= n2; k <<= 1) a = wave_steps(a, i, k, k >> 1);
    if (i < n2) K[i] = a;
  }
  __syncthreads();
  for (uint32_t k = 128; k <= n2; k <<= 1) {
    for (uint32_t j = k >> 1; j >= 64; j >>= 1) {
      for (uint32_t i = threadIdx.x; i < n2; i += THREADS) {
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
    for (uint32_t i0 = first; i0 < n2; i0 += THREADS) K[i0 + lane] = wave_steps(K[i0 + lane], i0 + lane, k, 32);   // n2 >= 128: whole waves
    __syncthreads();
  }
}

struct Selected {
  Box box[MI355_HAND_MAX];
  float rotation[MI355_HAND_MAX];
  unsigned long long key[MI355_HAND_MAX];
  uint32_t m;
};

// Greedy selection by ONE wave (all 64 lanes call it): the sorted keys K[0 .. n) in chunks of 64, one per lane. A lane is first tested
// against the boxes kept in earlier chunks, then the chunk is resolved in order: the lowest undecided live lane is kept and tests the
// lanes above it. Stops at max_hands. load(index, box, rotation) gives a candidate's box and rotation.
template <typename Load>
__device__ __forceinline__ void select_hands(const unsigned long long *K, uint32_t n, float thr, uint32_t max_hands, Selected &S, Load load) {
  const int lane = (int)__lane_id();
  uint32_t m = 0;   // wave-uniform
  for (uint32_t base = 0; base < n && m < max_hands; base += 64) {
    const uint32_t i = base + (uint32_t)lane;
    bool alive = i < n;
    Box b = {0.0f, 0.0f, 0.0f, 0.0f};
    float rot = 0.0f;
    unsigned long long key = 0;
    if (alive) {
      key = K[i];
      load(key_index(key), b, rot);
    }
    for (uint32_t j = 0; j < m; j++) {
      const Box kj = S.box[j];
      if (alive && iou(b, kj) > thr) alive = false;
    }
    unsigned long long todo = __ballot(alive);
    while (todo && m < max_hands) {
      const int l = __ffsll((long long)todo) - 1;
      Box bl;
      bl.xmin = __shfl(b.xmin, l);
      bl.ymin = __shfl(b.ymin, l);
      bl.xmax = __shfl(b.xmax, l);
      bl.ymax = __shfl(b.ymax, l);
      if (lane == l) {   // m < max_hands <= MI355_HAND_MAX
        S.box[m] = b;
        S.rotation[m] = rot;
        S.key[m] = key;
      }
      m++;
      if (alive && lane > l && iou(b, bl) > thr) alive = false;
      const unsigned long long above = l == 63 ? 0ull : ~((2ull << l) - 1ull);
      todo = __ballot(alive) & above;
    }
    __threadfence_block();   // the next chunk of this wave reads S.box
  }
  if (lane == 0) S.m = m;
  __threadfence_block();
}

__device__ __forceinline__ void write_det(const Selected &S, uint32_t j, const mi355_hand_params &P, mi355_hand_det *out) {
  mi355_hand_det d;
  const Box b = S.box[j];
  d.xmin = b.xmin;
  d.ymin = b.ymin;
  d.xmax = b.xmax;
  d.ymax = b.ymax;
  d.rotation = S.rotation[j];
  d.confidence = __uint_as_float(key_score_bits(S.key[j]));
  d.index = key_index(S.key[j]);
  oriented_od(b, d.rotation, P, d);
  d.reserved[0] = d.reserved[1] = d.reserved[2] = 0;
  out[j] = d;
}

// One palm tensor by one block of kPalmThreads: data [N][8], its MI355_HAND_MAX records and its count. The body of the lone kernel and
// of its job form: both run these instructions on this LDS layout, so a tensor's bytes do not depend on which of the two carried it.
// *n_hands is written on every path.
__device__ __forceinline__ void palm_decode(const float *__restrict__ data, uint32_t N, const mi355_hand_params &P, mi355_hand_det *__restrict__ dets,
                                            uint32_t *__restrict__ n_hands) {
  __shared__ unsigned long long K[kMaxRows];
  __shared__ uint32_t passed[kMaxRows];
  __shared__ Selected S;
  __shared__ uint32_t n_passed, count;
  const int tid = threadIdx.x;
  if (tid == 0) n_passed = count = 0;
  __syncthreads();
  // rule 1 on every row (the row's first 16 bytes): the rows that pass are compacted, so that the f64 functions of rules 2 and 4 run in
  // full waves over those rows alone and not in every wave that holds one of them
  for (uint32_t base = 0; base < N; base += kPalmThreads) {   // block-uniform bound: whole waves reach append_keys
    const uint32_t r = base + (uint32_t)tid;
    bool pass = false;
    if (r < N) {
      const float4u r0 = *reinterpret_cast<const float4u *>(data + (size_t)r * 8);
      pass = !(r0.x < P.confidence_threshold) && !(r0.w <= 0.0f);
    }
    append_keys(pass, r, &n_passed, passed, kMaxRows);
  }
  __syncthreads();
  const uint32_t n1 = n_passed < N ? n_passed : N;
  // rules 2 - 6 on the compacted rows (whole 32-byte rows, two 16-byte loads): the valid ones' keys
  for (uint32_t base = 0; base < n1; base += kPalmThreads) {
    const uint32_t i = base + (uint32_t)tid;
    bool keep = false;
    uint32_t score_bits = 0, r = 0;
    if (i < n1) {
      r = passed[i];   // < N
      const float4u *row = reinterpret_cast<const float4u *>(data + (size_t)r * 8);
      const float4u r0 = row[0], r1 = row[1];
      score_bits = __float_as_uint(r0.x);
      Box b;
      float rot;
      keep = palm_candidate(r0, r1, P, b, rot);
    }
    append_keys(keep, make_key(score_bits, r), &count, K, kMaxRows);
  }
  __syncthreads();
  const uint32_t n = count < N ? count : N;
  if (n == 0) {
    if (tid == 0) *n_hands = 0;
    return;
  }
  sort_keys<kPalmThreads>(K, n);
  if (tid < 64) {
    const float lo = P.nms_iou_threshold < 0.0f ? 0.0f : P.nms_iou_threshold;   // f32::clamp(0, 1): a NaN stays
    const float thr = lo > 1.0f ? 1.0f : lo;
    const uint32_t max_hands = P.max_hands < kPalmMaxHands ? P.max_hands : kPalmMaxHands;
    select_hands(K, n, thr, max_hands, S, [&](uint32_t r, Box &b, float &rot) {
      const float4u *row = reinterpret_cast<const float4u *>(data + (size_t)r * 8);
      (void)palm_candidate(row[0], row[1], P, b, rot);   // true: the row passed it above
    });
    const uint32_t m = S.m;
    if ((uint32_t)tid < m) write_det(S, (uint32_t)tid, P, dets);
    if (tid == 0) *n_hands = m;
  }
}

// tensors: [T] at a pitch; dets: [T][MI355_HAND_MAX]; n_hands: [T]
__global__ __launch_bounds__(kPalmThreads) void handdec_palm_kernel(const float *__restrict__ tensors, size_t pitch_floats, uint32_t N,
                                                                 const mi355_hand_params *__restrict__ params, mi355_hand_det *__restrict__ dets,
                                                                 uint32_t *__restrict__ n_hands) {
  const uint32_t t = blockIdx.x;
  const mi355_hand_params P = params[t];
  palm_decode(tensors + (size_t)t * pitch_floats, N, P, dets + (size_t)t * MI355_HAND_MAX, n_hands + t);
}

// ---- the job forms (launch sets of the video group's hand-decoder queue): block b decodes job b of a table passed by value in the
// kernel arguments - the tensor, its shape and its settings - into the set's result slab: counts[slot], dets[slot][MI355_HAND_MAX],
// kps[kp_slot][MI355_HAND_MAX]. Only jobs with rows are in a table.
struct HnPalmJob {
  const float *data;
  uint32_t N, slot;   // slot: the job's index in its set
  mi355_hand_params p;
  uint32_t pad;
};
struct HnPalmTable { HnPalmJob job[MI355_HANDDEC_SET_MAX]; };
struct HnLandmarkJob {
  const float *data, *scores;   // scores: null or num_scores floats
  uint32_t H, slot, D, num_scores, kp_slot;   // kp_slot: the job's index among the landmark jobs of its set
  mi355_hand_params p;
};
struct HnLandmarkTable { HnLandmarkJob job[MI355_HANDDEC_SET_MAX]; };
static_assert(sizeof(HnPalmJob) == 40 && sizeof(HnLandmarkJob) == 56, "the jobs have no padding holes");
static_assert(sizeof(HnPalmTable) + 64 <= 4096 && sizeof(HnLandmarkTable) + 64 <= 4096, "a job table and the slab pointers are passed in the kernel arguments");

__global__ __launch_bounds__(kPalmThreads) void handdec_palm_jobs_kernel(const HnPalmTable T, mi355_hand_det *__restrict__ dets, uint32_t *__restrict__ n_hands) {
  const HnPalmJob &J = T.job[blockIdx.x];
  const mi355_hand_params P = J.p;
  palm_decode(J.data, J.N, P, dets + (size_t)J.slot * MI355_HAND_MAX, n_hands + J.slot);
}

struct KpScratch { uint32_t w[sizeof(mi355_hand_keypoints) / 4]; };

// One landmark tensor by one block of kThreads: data [H][21 * D], sc null or num_scores scores, its MI355_HAND_MAX box and keypoint
// records and its count. The body of the lone kernel and of its job form, as palm_decode is. *n_hands is written on every path.
__device__ __forceinline__ void landmark_decode(const float *__restrict__ data, uint32_t H, uint32_t D, const float *__restrict__ sc, uint32_t num_scores,
                                                const mi355_hand_params &P, mi355_hand_det *__restrict__ dets, mi355_hand_keypoints *__restrict__ kps,
                                                uint32_t *__restrict__ n_hands) {
  __shared__ unsigned long long K[kMaxHands];
  __shared__ float4 hbox[kMaxHands];
  __shared__ float hrot[kMaxHands];
  __shared__ Selected S;
  __shared__ KpScratch kp[kWaves];
  __shared__ uint32_t count;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t hand_floats = (size_t)21 * D;
  if (tid == 0) count = 0;
  __syncthreads();
  for (uint32_t h = (uint32_t)wave; h < H; h += kWaves) {   // wave-uniform
    const float conf = (sc && h < num_scores) ? sc[h] : 1.0f;
    if (conf < P.confidence_threshold) continue;
    const float *hand = data + (size_t)h * hand_floats;
    float x = 0.0f, y = 0.0f;
    bool fin = false;
    if (lane < 21) {
      x = hand[(size_t)lane * D];
      y = hand[(size_t)lane * D + 1];
      fin = finite(x) && finite(y);
    }
    if (__ballot(fin) == 0) continue;   // no finite point
    float mnx = fin ? x : INFINITY, mxx = fin ? x : -INFINITY, mny = fin ? y : INFINITY, mxy = fin ? y : -INFINITY;
    for (int o = 32; o > 0; o >>= 1) {
      mnx = fminf(mnx, __shfl_xor(mnx, o));
      mxx = fmaxf(mxx, __shfl_xor(mxx, o));
      mny = fminf(mny, __shfl_xor(mny, o));
      mxy = fmaxf(mxy, __shfl_xor(mxy, o));
    }
    const float width = mxx - mnx, height = mxy - mny;
    if (width <= 0.0f || height <= 0.0f) continue;
    if (lane == 0) {
      hbox[h] = make_float4(mnx - width * kHandPad, mny - height * kHandPad, mxx + width * kHandPad, mxy + height * kHandPad);
      const float wx = hand[0], wy = hand[1], bx = hand[(size_t)9 * D], by = hand[(size_t)9 * D + 1];
      hrot[h] = kFracPi2 + atan2_c(by - wy, bx - wx);
      const uint32_t at = atomicAdd(&count, 1u);
      if (at < kMaxHands) K[at] = make_key(__float_as_uint(conf), h);   // always inside: a hand is appended once
    }
  }
  __syncthreads();
  const uint32_t n = count < H ? count : H;
  if (n == 0) {
    if (tid == 0) *n_hands = 0;
    return;
  }
  sort_keys<kThreads>(K, n);
  if (tid < 64) {
    const uint32_t max_hands = P.max_hands < kLandmarkMaxHands ? P.max_hands : kLandmarkMaxHands;
    select_hands(K, n, P.nms_iou_threshold, max_hands, S, [&](uint32_t h, Box &b, float &rot) {
      const float4 q = hbox[h];
      b.xmin = q.x;
      b.ymin = q.y;
      b.xmax = q.z;
      b.ymax = q.w;
      rot = hrot[h];
    });
    const uint32_t m = S.m;
    if ((uint32_t)tid < m) write_det(S, (uint32_t)tid, P, dets);
    if (tid == 0) *n_hands = m;
  }
  __syncthreads();
  // the keypoint records: a wave per selected hand in turn, assembled in the wave's LDS record, then copied out whole
  const uint32_t m = S.m;
  constexpr uint32_t kWords = sizeof(mi355_hand_keypoints) / 4;
  for (uint32_t j = (uint32_t)wave; j < m; j += kWaves) {
    uint32_t *w = kp[wave].w;
    uint8_t *bytes = reinterpret_cast<uint8_t *>(w);
    for (uint32_t e = (uint32_t)lane; e < kWords; e += 64) w[e] = 0;
    __threadfence_block();
    const uint32_t h = key_index(S.key[j]);
    const float hconf = __uint_as_float(key_score_bits(S.key[j]));
    const float *hand = data + (size_t)h * hand_floats;
    float x = 0.0f, y = 0.0f, c = hconf;
    uint8_t vis = MI355_KP_UNKNOWN;
    bool fin = false;
    if (lane < 21) {
      x = hand[(size_t)lane * D];
      y = hand[(size_t)lane * D + 1];
      fin = finite(x) && finite(y);
      if (D >= 3) {
        c = hand[(size_t)lane * D + 2];
        vis = c > 0.5f ? MI355_KP_VISIBLE : MI355_KP_OCCLUDED;
      }
    }
    const unsigned long long mask = __ballot(fin);
    if (fin) {
      const uint32_t at = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));   // < 21
      w[1 + 2 * at] = (uint32_t)cast_i32(x);
      w[2 + 2 * at] = (uint32_t)cast_i32(y);
      w[43 + at] = __float_as_uint(c);
      bytes[256 + at] = vis;
    }
    if (lane == 0) w[0] = (uint32_t)__popcll(mask);
    __threadfence_block();
    uint32_t *out = reinterpret_cast<uint32_t *>(kps + j);
    for (uint32_t e = (uint32_t)lane; e < kWords; e += 64) out[e] = w[e];
    __threadfence_block();   // the wave's record is assembled again for its next hand
  }
}

// landmarks: [T][H][21 * D] at a pitch; scores: null or [T][num_scores] at a pitch; dets, kps: [T][MI355_HAND_MAX]
__global__ __launch_bounds__(kThreads) void handdec_landmark_kernel(const float *__restrict__ tensors, size_t pitch_floats, uint32_t H, uint32_t D,
                                                                     const float *__restrict__ scores, size_t score_pitch_floats, uint32_t num_scores,
                                                                     const mi355_hand_params *__restrict__ params, mi355_hand_det *__restrict__ dets,
                                                                     mi355_hand_keypoints *__restrict__ kps, uint32_t *__restrict__ n_hands) {
  const uint32_t t = blockIdx.x;
  const mi355_hand_params P = params[t];
  landmark_decode(tensors + (size_t)t * pitch_floats, H, D, scores ? scores + (size_t)t * score_pitch_floats : nullptr, num_scores, P,
                  dets + (size_t)t * MI355_HAND_MAX, kps + (size_t)t * MI355_HAND_MAX, n_hands + t);
}

__global__ __launch_bounds__(kThreads) void handdec_landmark_jobs_kernel(const HnLandmarkTable T, mi355_hand_det *__restrict__ dets,
                                                                          mi355_hand_keypoints *__restrict__ kps, uint32_t *__restrict__ n_hands) {
  const HnLandmarkJob &J = T.job[blockIdx.x];
  const mi355_hand_params P = J.p;
  landmark_decode(J.data, J.H, J.D, J.scores, J.num_scores, P, dets + (size_t)J.slot * MI355_HAND_MAX, kps + (size_t)J.kp_slot * MI355_HAND_MAX, n_hands + J.slot);
}

}  // namespace

// scratch of one context; grows to the largest call seen
struct HandDecState {
  DeviceBuf<mi355_hand_params> d_params;
  PinnedBuf<mi355_hand_params> h_params;
  DeviceBuf<uint8_t> d_out;      // [tensors] counts (padded to 64 bytes), [tensors][MI355_HAND_MAX] dets, then keypoint records
  PinnedBuf<uint8_t> h_out;
  DeviceBuf<float> d_stage, d_stage_scores;   // the host forms' tensor and scores
};

void handdec_release(mi355_ctx *ctx) {
  delete static_cast<HandDecState *>(ctx->handdec);
  ctx->handdec = nullptr;
}

// the checks that need no device (every entry point; mi355_selftest_handdec_check)
int handdec_check_args(int decoder, size_t tensor_pitch_bytes, int n_tensors, uint32_t rows, uint32_t kps_dim, size_t score_pitch_bytes, uint32_t num_scores,
                       const char **why) {
  *why = nullptr;
  const bool palm = decoder == 0;
  if (decoder != 0 && decoder != 1) *why = "handdec: decoder is neither 0 (palm) nor 1 (landmarks)";
  else if (!palm && kps_dim < 2) *why = "handdec: fewer than 2 values per keypoint";
  else if (n_tensors < 1) *why = "handdec: n_tensors must be at least 1";
  if (*why) return MI355_ERR_INVALID_ARG;
  if (palm && rows > kMaxRows) *why = "handdec: more than 4096 palm rows";
  else if (!palm && rows > kMaxHands) *why = "handdec: more than 1024 hands";
  else if (!palm && kps_dim > kMaxDim) *why = "handdec: more than 16 values per keypoint";
  else if (!palm && num_scores > kMaxScores) *why = "handdec: more than 1024 scores";
  else if ((uint32_t)n_tensors > kMaxTensors) *why = "handdec: more than 1024 tensors";
  if (*why) return MI355_ERR_UNSUPPORTED;
  const size_t tensor_bytes = palm ? (size_t)rows * 32 : (size_t)rows * 21 * kps_dim * 4;
  if (tensor_pitch_bytes % 4 != 0 || tensor_pitch_bytes < tensor_bytes) {
    *why = "handdec: tensor pitch is smaller than the tensor or no multiple of 4";
    return MI355_ERR_INVALID_ARG;
  }
  if (!palm && num_scores > 0 && (score_pitch_bytes % 4 != 0 || score_pitch_bytes < (size_t)num_scores * 4)) {
    *why = "handdec: score pitch is smaller than the scores or no multiple of 4";
    return MI355_ERR_INVALID_ARG;
  }
  return MI355_OK;
}

int handdec_check_params(int decoder, uint32_t max_hands, int32_t frame_width, int32_t frame_height, const char **why) {
  *why = nullptr;
  const uint32_t cap = decoder == 0 ? kPalmMaxHands : kLandmarkMaxHands;
  if (max_hands < 1 || max_hands > cap) *why = "handdec: max_hands outside 1..8 (palm) or 1..10 (landmarks)";
  else if (!((frame_width > 0 && frame_height > 0) || (frame_width == 0 && frame_height == 0))) *why = "handdec: frame size is neither both positive nor both zero";
  return *why ? MI355_ERR_INVALID_ARG : MI355_OK;
}

static size_t counts_bytes(uint32_t T) { return ((size_t)T * sizeof(uint32_t) + 63) / 64 * 64; }
static size_t dets_bytes(uint32_t T) { return (size_t)T * MI355_HAND_MAX * sizeof(mi355_hand_det); }
static size_t kps_bytes(uint32_t T) { return (size_t)T * MI355_HAND_MAX * sizeof(mi355_hand_keypoints); }

static int handdec_scratch(mi355_ctx *ctx, uint32_t T, bool landmarks, HandDecState **out) {
  auto *s = static_cast<HandDecState *>(ctx->handdec);
  if (!s) ctx->handdec = s = new HandDecState();
  int rc = MI355_OK;
  if ((rc = check_hip(ctx, s->d_params.reserve((size_t)T), "hipMalloc(handdec params)"))) return rc;
  if ((rc = check_hip(ctx, s->h_params.reserve((size_t)T), "hipHostMalloc(handdec params)"))) return rc;
  const size_t bytes = counts_bytes(T) + dets_bytes(T) + (landmarks ? kps_bytes(T) : 0);
  if ((rc = check_hip(ctx, s->d_out.reserve(bytes), "hipMalloc(handdec results)"))) return rc;
  if ((rc = check_hip(ctx, s->h_out.reserve(bytes), "hipHostMalloc(handdec results)"))) return rc;
  *out = s;
  return MI355_OK;
}

// params up, the one launch, results down, one synchronisation; every argument is checked
static int handdec_run(mi355_ctx *ctx, HandDecState *s, bool landmarks, const float *d_tensors, size_t pitch_bytes, uint32_t T, uint32_t rows, uint32_t D,
                       const float *d_scores, size_t score_pitch_bytes, uint32_t num_scores, const mi355_hand_params *p, mi355_hand_det *dets,
                       mi355_hand_keypoints *kps, uint32_t *n_hands) {
  int rc = MI355_OK;
  std::memcpy(s->h_params.p, p, (size_t)T * sizeof(mi355_hand_params));
  if ((rc = check_hip(ctx, hipMemcpyAsync(s->d_params.p, s->h_params.p, (size_t)T * sizeof(mi355_hand_params), hipMemcpyHostToDevice, ctx->stream), "handdec params H2D")))
    return rc;
  __atomic_fetch_add(&ctx->n_h2d, 1ull, __ATOMIC_RELAXED);
  uint32_t *d_n = reinterpret_cast<uint32_t *>(s->d_out.p);
  mi355_hand_det *d_dets = reinterpret_cast<mi355_hand_det *>(s->d_out.p + counts_bytes(T));
  mi355_hand_keypoints *d_kps = reinterpret_cast<mi355_hand_keypoints *>(s->d_out.p + counts_bytes(T) + dets_bytes(T));
  if (landmarks)
    hipLaunchKernelGGL(handdec_landmark_kernel, dim3(T), dim3(kThreads), 0, ctx->stream, d_tensors, pitch_bytes / 4, rows, D, d_scores, score_pitch_bytes / 4,
                       d_scores ? num_scores : 0u, s->d_params.p, d_dets, d_kps, d_n);
  else
    hipLaunchKernelGGL(handdec_palm_kernel, dim3(T), dim3(kPalmThreads), 0, ctx->stream, d_tensors, pitch_bytes / 4, rows, s->d_params.p, d_dets, d_n);
  if ((rc = check_hip(ctx, hipGetLastError(), "handdec launch"))) return rc;
  const size_t bytes = counts_bytes(T) + dets_bytes(T) + (landmarks ? kps_bytes(T) : 0);
  if ((rc = check_hip(ctx, hipMemcpyAsync(s->h_out.p, s->d_out.p, bytes, hipMemcpyDeviceToHost, ctx->stream), "handdec D2H"))) return rc;
  __atomic_fetch_add(&ctx->n_d2h, 1ull, __ATOMIC_RELAXED);
  if ((rc = check_hip(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize"))) return rc;
  const uint32_t *h_n = reinterpret_cast<const uint32_t *>(s->h_out.p);
  const mi355_hand_det *h_dets = reinterpret_cast<const mi355_hand_det *>(s->h_out.p + counts_bytes(T));
  const mi355_hand_keypoints *h_kps = reinterpret_cast<const mi355_hand_keypoints *>(s->h_out.p + counts_bytes(T) + dets_bytes(T));
  for (uint32_t t = 0; t < T; t++) {
    const uint32_t n = h_n[t] < MI355_HAND_MAX ? h_n[t] : MI355_HAND_MAX;
    n_hands[t] = n;
    if (n) std::memcpy(dets + (size_t)t * MI355_HAND_MAX, h_dets + (size_t)t * MI355_HAND_MAX, (size_t)n * sizeof(mi355_hand_det));
    if (n && landmarks) std::memcpy(kps + (size_t)t * MI355_HAND_MAX, h_kps + (size_t)t * MI355_HAND_MAX, (size_t)n * sizeof(mi355_hand_keypoints));
  }
  return MI355_OK;
}

// the checks every entry point makes before it touches the device; *launch is false when there are no rows (counts are then zero)
static int handdec_enter(mi355_ctx *ctx, int decoder, size_t pitch_bytes, int n_tensors, uint32_t rows, uint32_t D, bool have_scores, size_t score_pitch_bytes,
                         uint32_t num_scores, const mi355_hand_params *p, const void *dets, const void *kps, uint32_t *n_hands, bool *launch) {
  *launch = false;
  const char *why = nullptr;
  int rc = handdec_check_args(decoder, pitch_bytes, n_tensors, rows, D, score_pitch_bytes, have_scores ? num_scores : 0, &why);
  if (rc) return set_error(ctx, rc, why);
  if (!p || !n_hands || !dets || (decoder == 1 && !kps)) return set_error(ctx, MI355_ERR_INVALID_ARG, "handdec: null params or result arrays");
  for (int t = 0; t < n_tensors; t++)
    if ((rc = handdec_check_params(decoder, p[t].max_hands, p[t].frame_width, p[t].frame_height, &why))) return set_error(ctx, rc, why);
  if (rows == 0) {
    for (int t = 0; t < n_tensors; t++) n_hands[t] = 0;
    return MI355_OK;
  }
  *launch = true;
  return MI355_OK;
}

// ---- launch sets of the video group's hand-decoder queue

static size_t set_bytes(uint64_t n_jobs, uint64_t n_landmark_jobs) { return kHnCountsBytes + dets_bytes((uint32_t)n_jobs) + kps_bytes((uint32_t)n_landmark_jobs); }
constexpr size_t kHnSlabBytes = kHnCountsBytes + (size_t)kHnSetMax * MI355_HAND_MAX * (sizeof(mi355_hand_det) + sizeof(mi355_hand_keypoints));
static_assert(kHnCountsBytes >= kHnSetMax * sizeof(uint32_t) && kHnCountsBytes % 8 == 0, "the counts come first and the records behind them stay aligned");
static_assert(kHnSlabBytes == 128 + 32 * 640 + 32 * 2880, "the slab's maximum: pinned blocks are of one size");

// the layout of one set (mi355_selftest_handdec_set_plan; handdec_plan_set plans the queue's sets with it)
int handdec_set_plan(int n_jobs, const int *decoder, const uint32_t *rows, uint32_t *block, uint32_t *kp_slot, uint64_t totals[4]) {
  if (n_jobs < 0 || n_jobs > kHnSetMax || !totals) return MI355_ERR_INVALID_ARG;
  if (n_jobs > 0 && (!decoder || !rows || !block || !kp_slot)) return MI355_ERR_INVALID_ARG;
  for (int j = 0; j < n_jobs; j++)
    if (decoder[j] != 0 && decoder[j] != 1) return MI355_ERR_INVALID_ARG;
  for (int j = 0; j < n_jobs; j++)
    if (rows[j] > (decoder[j] == 0 ? kMaxRows : kMaxHands)) return MI355_ERR_UNSUPPORTED;
  uint64_t t[4] = {0, 0, 0, 0};   // palm blocks, landmark blocks, landmark jobs, bytes copied
  for (int j = 0; j < n_jobs; j++) {
    block[j] = rows[j] ? (uint32_t)t[decoder[j]]++ : UINT32_MAX;
    kp_slot[j] = decoder[j] == 1 ? (uint32_t)t[2]++ : UINT32_MAX;
  }
  if (t[0] + t[1]) t[3] = set_bytes((uint64_t)n_jobs, t[2]);
  for (int k = 0; k < 4; k++) totals[k] = t[k];
  return MI355_OK;
}

// The queue's device scratch is the result slab of ONE set, at its maximum (kHnSlabBytes): consecutive sets share it, ordered on the
// queue's stream - a set's copy precedes the next set's kernels. NOTHING in it is cleared between sets: it holds no counter that a
// kernel adds to. A job with rows has a block, and every block writes its count on every path (palm_decode, landmark_decode: 0 on the
// early return, the selected hands otherwise) and exactly that many records; a job without rows has no block and its count is 0 on
// the host (the queue never reads its slot). What an earlier set left in a slot is therefore never read.
struct HnSetScratch {
  DeviceBuf<uint8_t> d_out;
};

HnSetScratch *handdec_set_scratch_new(int *status, std::string *err) {
  auto *S = new HnSetScratch();
  if (S->d_out.reserve(kHnSlabBytes) != hipSuccess) {
    delete S;
    *status = MI355_ERR_OUT_OF_MEMORY;
    *err = "hipMalloc(handdec set results)";
    return nullptr;
  }
  *status = MI355_OK;
  return S;
}

void handdec_set_scratch_free(HnSetScratch *S) { delete S; }

size_t handdec_set_block_bytes() { return kHnSlabBytes; }

// the one place a set's members become the plan's arrays
int handdec_plan_set(const HnTensor *tensors, int n, HnSetPlan *out) {
  for (uint64_t &t : out->totals) t = 0;
  if (!tensors || n < 0 || n > kHnSetMax) return MI355_ERR_INVALID_ARG;
  int decoder[kHnSetMax];
  uint32_t rows[kHnSetMax];
  for (int i = 0; i < n; i++) { decoder[i] = tensors[i].decoder; rows[i] = tensors[i].rows; }
  return handdec_set_plan(n, decoder, rows, out->block, out->kp_slot, out->totals);
}

int handdec_launch_set(HnSetScratch *S, hipStream_t stream, const HnTensor *tensors, int n, const HnSetPlan &P, void *h_block, size_t h_block_bytes,
                       int *kernel_launches, std::string *err) {
  *kernel_launches = 0;
  if (!S || !tensors || n < 1 || n > kHnSetMax) { *err = "handdec: bad launch set"; return MI355_ERR_INVALID_ARG; }
  const uint64_t *totals = P.totals;
  if (totals[3] == 0) return MI355_OK;   // no job has rows: nothing to launch, nothing to copy
  const size_t bytes = (size_t)totals[3];   // <= kHnSlabBytes: n <= kHnSetMax
  if (!h_block || h_block_bytes < bytes) { *err = "handdec: the pinned result block is too small for the set"; return MI355_ERR_INVALID_ARG; }
  HnPalmTable palm = {};
  HnLandmarkTable lm = {};
  for (int i = 0; i < n; i++) {
    const HnTensor &t = tensors[i];
    if (!t.rows) continue;   // no rows: no block
    if (t.decoder == 0) {
      HnPalmJob &J = palm.job[P.block[i]];   // block[i] < palm blocks <= kHnSetMax
      J.data = t.data;
      J.N = t.rows;
      J.slot = (uint32_t)i;
      J.p = t.p;
    } else {
      HnLandmarkJob &J = lm.job[P.block[i]];
      J.data = t.data;
      J.scores = t.scores;
      J.H = t.rows;
      J.slot = (uint32_t)i;
      J.D = t.D;
      J.num_scores = t.scores ? t.num_scores : 0u;
      J.kp_slot = P.kp_slot[i];
      J.p = t.p;
    }
  }
  uint32_t *d_n = reinterpret_cast<uint32_t *>(S->d_out.p);
  mi355_hand_det *d_dets = reinterpret_cast<mi355_hand_det *>(S->d_out.p + kHnCountsBytes);
  mi355_hand_keypoints *d_kps = reinterpret_cast<mi355_hand_keypoints *>(S->d_out.p + kHnCountsBytes + dets_bytes((uint32_t)n));
  if (totals[0]) {
    hipLaunchKernelGGL(handdec_palm_jobs_kernel, dim3((uint32_t)totals[0]), dim3(kPalmThreads), 0, stream, palm, d_dets, d_n);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { *err = std::string("handdec palm jobs kernel launch: ") + hipGetErrorString(e); return MI355_ERR_HIP; }
    (*kernel_launches)++;
  }
  if (totals[1]) {
    hipLaunchKernelGGL(handdec_landmark_jobs_kernel, dim3((uint32_t)totals[1]), dim3(kThreads), 0, stream, lm, d_dets, d_kps, d_n);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { *err = std::string("handdec landmark jobs kernel launch: ") + hipGetErrorString(e); return MI355_ERR_HIP; }
    (*kernel_launches)++;
  }
  const hipError_t e = hipMemcpyAsync(h_block, S->d_out.p, bytes, hipMemcpyDeviceToHost, stream);
  if (e != hipSuccess) { *err = std::string("handdec set D2H: ") + hipGetErrorString(e); return MI355_ERR_HIP; }
  return MI355_OK;
}

// tensor i of a set of n (its decoder, rows and kp_slot as the plan gave them) out of the set's pinned block; h_block may be null
// when no job of the set had rows
void handdec_set_result(const void *h_block, int n, int i, int decoder, uint32_t rows, uint32_t kp_slot, mi355_hand_det *dets, mi355_hand_keypoints *kps,
                        uint32_t *n_hands) {
  *n_hands = 0;
  if (!h_block || !rows) return;   // a job without rows had no block: its slot holds nothing of this set
  const uint8_t *h = static_cast<const uint8_t *>(h_block);
  const uint32_t c = reinterpret_cast<const uint32_t *>(h)[i];
  const uint32_t m = c < MI355_HAND_MAX ? c : MI355_HAND_MAX;
  *n_hands = m;
  if (!m) return;
  std::memcpy(dets, h + kHnCountsBytes + dets_bytes((uint32_t)i), (size_t)m * sizeof(mi355_hand_det));
  if (decoder == 1) std::memcpy(kps, h + kHnCountsBytes + dets_bytes((uint32_t)n) + kps_bytes(kp_slot), (size_t)m * sizeof(mi355_hand_keypoints));
}

}  // namespace mi355

using namespace mi355;

extern "C" {

int mi355_handdec_palm_tensors_device(mi355_ctx *ctx, const float *d_tensors, size_t tensor_pitch_bytes, int n_tensors, uint32_t num_rows,
                                      const mi355_hand_params *p, mi355_hand_det *dets, uint32_t *n_hands) {
  if (!ctx) return MI355_ERR_INVALID_ARG;
  bool launch = false;
  int rc = handdec_enter(ctx, 0, tensor_pitch_bytes, n_tensors, num_rows, 0, false, 0, 0, p, dets, nullptr, n_hands, &launch);
  if (rc || !launch) return rc;
  if (!d_tensors || (uintptr_t)d_tensors % 4 != 0) return set_error(ctx, MI355_ERR_INVALID_ARG, "handdec: null or misaligned tensors");
  if ((rc = check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice"))) return rc;
  HandDecState *s = nullptr;
  if ((rc = handdec_scratch(ctx, (uint32_t)n_tensors, false, &s))) return rc;
  return handdec_run(ctx, s, false, d_tensors, tensor_pitch_bytes, (uint32_t)n_tensors, num_rows, 0, nullptr, 0, 0, p, dets, nullptr, n_hands);
}

int mi355_handdec_palm_tensor(mi355_ctx *ctx, const float *data, uint32_t num_rows, const mi355_hand_params *p, mi355_hand_det *dets, uint32_t *n_hands) {
  if (!ctx) return MI355_ERR_INVALID_ARG;
  const size_t bytes = (size_t)num_rows * 32;
  bool launch = false;
  int rc = handdec_enter(ctx, 0, bytes, 1, num_rows, 0, false, 0, 0, p, dets, nullptr, n_hands, &launch);
  if (rc || !launch) return rc;
  if (!data) return set_error(ctx, MI355_ERR_INVALID_ARG, "handdec: null tensor");
  if ((rc = check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice"))) return rc;
  HandDecState *s = nullptr;
  if ((rc = handdec_scratch(ctx, 1, false, &s))) return rc;
  if ((rc = check_hip(ctx, s->d_stage.reserve(bytes / 4), "hipMalloc(handdec staging)"))) return rc;
  if ((rc = check_hip(ctx, hipMemcpyAsync(s->d_stage.p, data, bytes, hipMemcpyHostToDevice, ctx->stream), "handdec H2D"))) return rc;
  __atomic_fetch_add(&ctx->n_h2d, 1ull, __ATOMIC_RELAXED);
  return handdec_run(ctx, s, false, s->d_stage.p, bytes, 1, num_rows, 0, nullptr, 0, 0, p, dets, nullptr, n_hands);
}

int mi355_handdec_landmarks_tensors_device(mi355_ctx *ctx, const float *d_landmarks, size_t tensor_pitch_bytes, int n_tensors, uint32_t num_hands, uint32_t kps_dim,
                                           const float *d_scores, size_t score_pitch_bytes, uint32_t num_scores, const mi355_hand_params *p, mi355_hand_det *dets,
                                           mi355_hand_keypoints *kps, uint32_t *n_hands) {
  if (!ctx) return MI355_ERR_INVALID_ARG;
  bool launch = false;
  int rc = handdec_enter(ctx, 1, tensor_pitch_bytes, n_tensors, num_hands, kps_dim, d_scores != nullptr, score_pitch_bytes, num_scores, p, dets, kps, n_hands, &launch);
  if (rc || !launch) return rc;
  if (!d_landmarks || (uintptr_t)d_landmarks % 4 != 0 || (uintptr_t)d_scores % 4 != 0) return set_error(ctx, MI355_ERR_INVALID_ARG, "handdec: null or misaligned tensors");
  if ((rc = check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice"))) return rc;
  HandDecState *s = nullptr;
  if ((rc = handdec_scratch(ctx, (uint32_t)n_tensors, true, &s))) return rc;
  return handdec_run(ctx, s, true, d_landmarks, tensor_pitch_bytes, (uint32_t)n_tensors, num_hands, kps_dim, d_scores, score_pitch_bytes, num_scores, p, dets, kps,
                     n_hands);
}

int mi355_handdec_landmarks_tensor(mi355_ctx *ctx, const float *landmarks, uint32_t num_hands, uint32_t kps_dim, const float *scores, uint32_t num_scores,
                                   const mi355_hand_params *p, mi355_hand_det *dets, mi355_hand_keypoints *kps, uint32_t *n_hands) {
  if (!ctx) return MI355_ERR_INVALID_ARG;
  const size_t bytes = (size_t)num_hands * 21 * kps_dim * 4, score_bytes = (size_t)num_scores * 4;
  const bool have_scores = scores != nullptr && num_scores > 0;
  bool launch = false;
  int rc = handdec_enter(ctx, 1, bytes, 1, num_hands, kps_dim, have_scores, score_bytes, num_scores, p, dets, kps, n_hands, &launch);
  if (rc || !launch) return rc;
  if (!landmarks) return set_error(ctx, MI355_ERR_INVALID_ARG, "handdec: null tensor");
  if ((rc = check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice"))) return rc;
  HandDecState *s = nullptr;
  if ((rc = handdec_scratch(ctx, 1, true, &s))) return rc;
  if ((rc = check_hip(ctx, s->d_stage.reserve(bytes / 4), "hipMalloc(handdec staging)"))) return rc;
  if ((rc = check_hip(ctx, hipMemcpyAsync(s->d_stage.p, landmarks, bytes, hipMemcpyHostToDevice, ctx->stream), "handdec H2D"))) return rc;
  __atomic_fetch_add(&ctx->n_h2d, 1ull, __ATOMIC_RELAXED);
  if (have_scores) {
    if ((rc = check_hip(ctx, s->d_stage_scores.reserve((size_t)num_scores), "hipMalloc(handdec score staging)"))) return rc;
    if ((rc = check_hip(ctx, hipMemcpyAsync(s->d_stage_scores.p, scores, score_bytes, hipMemcpyHostToDevice, ctx->stream), "handdec scores H2D"))) return rc;
    __atomic_fetch_add(&ctx->n_h2d, 1ull, __ATOMIC_RELAXED);
  }
  return handdec_run(ctx, s, true, s->d_stage.p, bytes, 1, num_hands, kps_dim, have_scores ? s->d_stage_scores.p : nullptr, score_bytes, num_scores, p, dets, kps, n_hands);
}

int mi355_selftest_handdec_check(int decoder, size_t tensor_pitch_bytes, int n_tensors, uint32_t rows, uint32_t kps_dim, size_t score_pitch_bytes, uint32_t num_scores,
                                 uint32_t max_hands, int32_t frame_width, int32_t frame_height) {
  const char *why = nullptr;
  const int rc = handdec_check_args(decoder, tensor_pitch_bytes, n_tensors, rows, kps_dim, score_pitch_bytes, num_scores, &why);
  if (rc) return rc;
  return handdec_check_params(decoder, max_hands, frame_width, frame_height, &why);
}

int mi355_selftest_handdec_set_plan(int n_jobs, const int *decoder, const uint32_t *rows, uint32_t *block, uint32_t *kp_slot, uint64_t totals[4]) {
  return handdec_set_plan(n_jobs, decoder, rows, block, kp_slot, totals);
}

}  // extern "C"
