// handdec_cpu.cpp — a plain single-thread C++ restatement of the handdetectiontensordec / handlandmarktensordec decode contract
// (DESIGN §4.12), written from the contract's rules. The second independent restatement beside tests/handdec_restate.py and the
// one-core baseline of tools/bench_handdec.py. Not part of libmi355fx.so or of the host library: the product computes nothing on the CPU.
//   g++ -O3 -ffp-contract=off -fno-fast-math -shared -fPIC tools/handdec_cpu.cpp -o libhanddec_cpu.so
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

struct Det {   // mi355_hand_det
  float xmin, ymin, xmax, ymax;
  float rotation, rotation_od, confidence;
  uint32_t index;
  int32_t x, y, width, height;
  uint32_t has_od, reserved[3];
};
struct Kp {   // mi355_hand_keypoints
  uint32_t count;
  int32_t positions[42];
  float confidences[21];
  uint8_t visibilities[21], reserved[11];
};
static_assert(sizeof(Det) == 64 && sizeof(Kp) == 288, "record layouts");

const float kFracPi2 = 1.57079632679489661923f;

// rule 7: the order of f32::total_cmp as an i32
inline int32_t total_key(float v) {
  uint32_t bits;
  std::memcpy(&bits, &v, 4);
  const int32_t s = (int32_t)bits;
  return s ^ (int32_t)((uint32_t)(s >> 31) >> 1);
}

// toward zero, saturating, NaN -> 0
inline int32_t cast_i32(float f) {
  if (std::isnan(f)) return 0;
  if (f >= 2147483648.0f) return INT_MAX;
  if (f <= -2147483648.0f) return INT_MIN;
  return (int32_t)f;
}

// deviation a: libm's double functions of the f32 arguments, rounded once
inline float atan2_c(float y, float x) { return (float)std::atan2((double)y, (double)x); }
inline float sin_c(float v) { return (float)std::sin((double)v); }
inline float cos_c(float v) { return (float)std::cos((double)v); }

// deviation b: restated without source
inline float iou(const Det &a, const Det &b) {
  const float aw = a.xmax - a.xmin, ah = a.ymax - a.ymin, bw = b.xmax - b.xmin, bh = b.ymax - b.ymin;
  const float left = std::fmax(a.xmin, b.xmin), right = std::fmin(a.xmin + aw, b.xmin + bw);
  const float top = std::fmax(a.ymin, b.ymin), bottom = std::fmin(a.ymin + ah, b.ymin + bh);
  const float inter = std::fmax(0.0f, right - left) * std::fmax(0.0f, bottom - top);
  const float uni = aw * ah + bw * bh - inter;
  return uni > 0.0f ? inter / uni : 0.0f;
}

// rule 9: the oriented-OD values of one hand; has_od = 0 and zeros when there are none
void oriented_od(Det &d, int32_t fw_i, int32_t fh_i) {
  d.x = d.y = d.width = d.height = 0;
  d.rotation_od = 0.0f;
  d.has_od = 0;
  if (!std::isfinite(d.xmin) || !std::isfinite(d.ymin) || !std::isfinite(d.xmax) || !std::isfinite(d.ymax)) return;
  const float x0 = std::floor(d.xmin), y0 = std::floor(d.ymin), x1 = std::ceil(d.xmax), y1 = std::ceil(d.ymax);
  if (x1 <= x0 || y1 <= y0) return;
  if (fw_i > 0 && fh_i > 0 && (x1 <= 0.0f || y1 <= 0.0f || x0 >= (float)fw_i || y0 >= (float)fh_i)) return;
  const int32_t w = cast_i32(x1 - x0), h = cast_i32(y1 - y0);
  if (w <= 0 || h <= 0) return;
  d.x = cast_i32(x0);
  d.y = cast_i32(y0);
  d.width = w;
  d.height = h;
  d.rotation_od = d.rotation + (-kFracPi2);
  d.has_od = 1;
}

// rules 7 and 8: stable sort by descending confidence, greedy selection up to max_hands
std::vector<Det> sort_and_select(std::vector<Det> &cand, float thr, uint32_t max_hands) {
  std::stable_sort(cand.begin(), cand.end(), [](const Det &a, const Det &b) { return total_key(a.confidence) > total_key(b.confidence); });
  std::vector<Det> kept;
  for (const Det &c : cand) {
    bool drop = false;
    for (const Det &k : kept)
      if (iou(c, k) > thr) {
        drop = true;
        break;
      }
    if (drop) continue;
    kept.push_back(c);
    if (kept.size() >= max_hands) break;
  }
  return kept;
}

inline bool in_range(float lo, float v, float hi) { return lo <= v && v <= hi; }

}  // namespace

// rows: [N][8]. frame_w, frame_h: both > 0 or both 0. Writes at most max_hands (<= 8) records; returns 0, or -1 outside the contract.
extern "C" int handdec_palm_cpu(const float *rows, uint32_t N, float conf_thr, float iou_thr, uint32_t max_hands, int32_t frame_w, int32_t frame_h, void *dets_out,
                                uint32_t *n_hands) {
  if (!n_hands || !dets_out || (N && !rows) || max_hands < 1 || max_hands > 8) return -1;
  std::vector<Det> cand;
  for (uint32_t r = 0; r < N; r++) {
    const float *v = rows + (size_t)r * 8;
    const float score = v[0], cx = v[1], cy = v[2], size = v[3], k0x = v[4], k0y = v[5], k2x = v[6], k2y = v[7];
    if (score < conf_thr) continue;                                                  // rule 1
    if (size <= 0.0f) continue;
    const float dx = k2x - k0x, dy = k2y - k0y;
    const float rotation = kFracPi2 + atan2_c(dy, dx);                               // rule 2
    float rr = 2.9f * size;                                                          // rule 3
    float center_x = cx + (0.5f * size) * sin_c(rotation);                           // rule 4
    float center_y = cy - (0.5f * size) * cos_c(rotation);
    const float all8[8] = {center_x, center_y, rr, size, k0x, k0y, k2x, k2y};        // rule 5
    bool fin = true;
    for (float f : all8) fin = fin && std::isfinite(f);
    if (!fin) continue;
    if (!in_range(0.06f, rr, 1.40f)) continue;
    if (!in_range(0.0f, center_x, 1.0f) || !in_range(0.0f, center_y, 1.0f)) continue;
    const float ratio = std::sqrt(dx * dx + dy * dy) / size;
    if (!in_range(0.15f, ratio, 1.60f)) continue;
    const float hs = rr * 0.5f;
    const float x0 = center_x - hs, y0 = center_y - hs, x1 = center_x + hs, y1 = center_y + hs;
    const float area = std::fmax(x1 - x0, 0.0f) * std::fmax(y1 - y0, 0.0f);
    if (area <= 0.0f) continue;
    const float vis_w = std::fmax(std::fmin(x1, 1.0f) - std::fmax(x0, 0.0f), 0.0f), vis_h = std::fmax(std::fmin(y1, 1.0f) - std::fmax(y0, 0.0f), 0.0f);
    if (!(vis_w * vis_h / area >= 0.5f)) continue;
    if (frame_w > 0 && frame_h > 0) {                                                // rule 6
      const float w = (float)frame_w, h = (float)frame_h;
      center_x *= w;
      center_y *= h;
      rr *= std::fmax(w, h);
    }
    const float half = rr / 2.0f;
    Det d;
    std::memset(&d, 0, sizeof d);
    d.xmin = center_x - half;
    d.ymin = center_y - half;
    d.xmax = center_x + half;
    d.ymax = center_y + half;
    d.rotation = rotation;
    d.confidence = score;
    d.index = r;
    cand.push_back(d);
  }
  const float thr = iou_thr < 0.0f ? 0.0f : iou_thr > 1.0f ? 1.0f : iou_thr;         // f32::clamp: a NaN stays
  std::vector<Det> kept = sort_and_select(cand, thr, max_hands);
  Det *out = static_cast<Det *>(dets_out);
  for (size_t j = 0; j < kept.size(); j++) {
    oriented_od(kept[j], frame_w, frame_h);
    out[j] = kept[j];
  }
  *n_hands = (uint32_t)kept.size();
  return 0;
}

// landmarks: [H][21 * D]; scores: null or num_scores values. Writes at most max_hands (<= 10) records of each kind.
extern "C" int handdec_landmarks_cpu(const float *landmarks, uint32_t H, uint32_t D, const float *scores, uint32_t num_scores, float conf_thr, float iou_thr,
                                     uint32_t max_hands, int32_t frame_w, int32_t frame_h, void *dets_out, void *kps_out, uint32_t *n_hands) {
  if (!n_hands || !dets_out || !kps_out || (H && !landmarks) || D < 2 || max_hands < 1 || max_hands > 10) return -1;
  std::vector<Det> cand;
  for (uint32_t h = 0; h < H; h++) {
    const float conf = (scores && h < num_scores) ? scores[h] : 1.0f;                // rule 1
    if (conf < conf_thr) continue;
    const float *p = landmarks + (size_t)h * 21 * D;
    float mnx = INFINITY, mxx = -INFINITY, mny = INFINITY, mxy = -INFINITY;          // rule 2
    int finite_points = 0;
    for (int j = 0; j < 21; j++) {
      const float x = p[(size_t)j * D], y = p[(size_t)j * D + 1];
      if (!std::isfinite(x) || !std::isfinite(y)) continue;
      finite_points++;
      mnx = std::fmin(mnx, x);
      mxx = std::fmax(mxx, x);
      mny = std::fmin(mny, y);
      mxy = std::fmax(mxy, y);
    }
    if (!finite_points) continue;
    const float width = mxx - mnx, height = mxy - mny;
    if (width <= 0.0f || height <= 0.0f) continue;
    Det d;
    std::memset(&d, 0, sizeof d);
    d.xmin = mnx - width * 0.15f;
    d.ymin = mny - height * 0.15f;
    d.xmax = mxx + width * 0.15f;
    d.ymax = mxy + height * 0.15f;
    d.rotation = kFracPi2 + atan2_c(p[(size_t)9 * D + 1] - p[1], p[(size_t)9 * D] - p[0]);   // rule 3: unchecked
    d.confidence = conf;
    d.index = h;
    cand.push_back(d);
  }
  std::vector<Det> kept = sort_and_select(cand, iou_thr, max_hands);                 // rule 4: not clamped
  Det *out = static_cast<Det *>(dets_out);
  Kp *kout = static_cast<Kp *>(kps_out);
  for (size_t j = 0; j < kept.size(); j++) {
    oriented_od(kept[j], frame_w, frame_h);
    out[j] = kept[j];
    Kp k;                                                                            // rule 5
    std::memset(&k, 0, sizeof k);
    const float *p = landmarks + (size_t)kept[j].index * 21 * D;
    for (int q = 0; q < 21; q++) {
      const float x = p[(size_t)q * D], y = p[(size_t)q * D + 1];
      if (!std::isfinite(x) || !std::isfinite(y)) continue;
      const uint32_t n = k.count++;
      k.positions[2 * n] = cast_i32(x);
      k.positions[2 * n + 1] = cast_i32(y);
      if (D >= 3) {
        k.confidences[n] = p[(size_t)q * D + 2];
        k.visibilities[n] = p[(size_t)q * D + 2] > 0.5f ? 1 : 2;
      } else {
        k.confidences[n] = kept[j].confidence;
        k.visibilities[n] = 0;
      }
    }
    kout[j] = k;
  }
  *n_hands = (uint32_t)kept.size();
  return 0;
}
