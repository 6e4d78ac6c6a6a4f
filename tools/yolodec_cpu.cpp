// yolodec_cpu.cpp — a plain single-thread C++ restatement of the yolov8tensordec2 / yoloxtensordec decode contract,
// written from the contract's rules. The second independent restatement beside tests/yolodec_restate.py and the one-core baseline of
// tools/bench_yolodec.py. Not part of libmi355fx.so or of the host library: the product computes nothing on the CPU.
//   g++ -O3 -ffp-contract=off -fno-fast-math -shared -fPIC tools/yolodec_cpu.cpp -o libyolodec_cpu.so
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

struct Det {   // mi355_yolo_det
  float xmin, ymin, xmax, ymax;
  int32_t x, y, width, height;
  uint32_t class_id;
  float confidence;
  uint32_t candidate, reserved;
};
static_assert(sizeof(Det) == 48, "record layout");

// rule 1: the order of f32::total_cmp as an i32
inline int32_t total_key(float v) {
  uint32_t bits;
  std::memcpy(&bits, &v, 4);
  const int32_t s = (int32_t)bits;
  return s ^ (int32_t)((uint32_t)(s >> 31) >> 1);
}

// rule 6: toward zero, saturating, NaN -> 0
inline int32_t cast_i32(float f) {
  if (std::isnan(f)) return 0;
  if (f >= 2147483648.0f) return INT_MAX;
  if (f <= -2147483648.0f) return INT_MIN;
  return (int32_t)f;
}

// rule 5: the kept box first
inline float iou(const Det &k, const Det &b) {
  const float ka = (k.xmax - k.xmin + 1.0f) * (k.ymax - k.ymin + 1.0f);
  const float ba = (b.xmax - b.xmin + 1.0f) * (b.ymax - b.ymin + 1.0f);
  const float x0 = std::fmax(k.xmin, b.xmin), x1 = std::fmin(k.xmax, b.xmax);
  const float y0 = std::fmax(k.ymin, b.ymin), y1 = std::fmin(k.ymax, b.ymax);
  const float ia = std::fmax(x1 - x0 + 1.0f, 0.0f) * std::fmax(y1 - y0 + 1.0f, 0.0f);
  return ia / (ka + ba - ia);
}

}  // namespace

// layout 0: V8 [F][N], 1: X [N][F]. Returns 0, or -1 for arguments outside the contract. *n_dets is the kept count; the first
// min(*n_dets, max_dets) records in output order are written.
extern "C" int yolodec_cpu(const float *data, int layout, uint32_t F, uint32_t N, float box_thr, float class_thr, float iou_thr, void *dets_out,
                           uint32_t max_dets, uint32_t *n_dets) {
  if (!n_dets || F < 6 || (layout != 0 && layout != 1) || (N && !data) || (max_dets && !dets_out)) return -1;
  Det *out = static_cast<Det *>(dets_out);
  std::vector<Det> cand;
  const uint32_t first_class = layout == 0 ? 4 : 5;
  for (uint32_t c = 0; c < N; c++) {
    auto field = [&](uint32_t f) { return layout == 0 ? data[(size_t)f * N + c] : data[(size_t)c * F + f]; };
    if (layout == 1 && field(4) < box_thr) continue;              // rule 2
    uint32_t cls = 0;
    float conf = field(first_class);
    for (uint32_t f = first_class + 1; f < F; f++) {               // rule 1: the last of equal maxima
      const float v = field(f);
      if (total_key(v) >= total_key(conf)) {
        conf = v;
        cls = f - first_class;
      }
    }
    if (conf < class_thr) continue;                                // a NaN stays
    const float x = field(0), y = field(1), w = field(2), h = field(3);
    Det d;
    d.xmin = x - w / 2.0f;                                         // rule 3
    d.ymin = y - h / 2.0f;
    d.xmax = x + w / 2.0f;
    d.ymax = y + h / 2.0f;
    d.x = d.y = d.width = d.height = 0;
    d.class_id = cls;
    d.confidence = layout == 1 ? field(4) * conf : conf;
    d.candidate = c;
    d.reserved = 0;
    cand.push_back(d);
  }
  // rule 4: stable, so equal entries stay in candidate order
  std::stable_sort(cand.begin(), cand.end(), [](const Det &a, const Det &b) {
    if (a.class_id != b.class_id) return a.class_id < b.class_id;
    return total_key(a.confidence) > total_key(b.confidence);
  });
  uint32_t total = 0;
  std::vector<Det> kept;
  for (size_t lo = 0; lo < cand.size();) {
    size_t hi = lo;
    while (hi < cand.size() && cand[hi].class_id == cand[lo].class_id) hi++;
    kept.clear();
    for (size_t i = lo; i < hi; i++) {                             // rule 5
      bool drop = false;
      for (const Det &k : kept)
        if (iou(k, cand[i]) > iou_thr) {
          drop = true;
          break;
        }
      if (!drop) kept.push_back(cand[i]);
    }
    for (Det d : kept) {                                           // rule 6
      d.x = cast_i32(d.xmin);
      d.y = cast_i32(d.ymin);
      d.width = cast_i32(d.xmax - d.xmin);
      d.height = cast_i32(d.ymax - d.ymin);
      if (total < max_dets) out[total] = d;
      total++;
    }
    lo = hi;
  }
  *n_dets = total;
  return 0;
}
