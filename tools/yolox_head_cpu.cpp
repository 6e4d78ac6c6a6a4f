// yolox_head_cpu.cpp — a plain single-thread C++ restatement of the yoloxinference head decode contract, written
// from the contract's rules: the decoded [A, 5 + C] tensor, and its detections by composition with the tensor decoder's
// restatement (tools/yolodec_cpu.cpp, included here). The second independent restatement beside tests/yolox_head_restate.py and
// the one-core baseline of tools/bench_yolox_head.py. Not part of libmi355fx.so or of the host library: the product computes
// nothing on the CPU.
//   g++ -O3 -ffp-contract=off -fno-fast-math -shared -fPIC tools/yolox_head_cpu.cpp -o libyolox_head_cpu.so
#include "yolodec_cpu.cpp"

namespace {

// the stated deviation: the f64 function of the f32 argument, rounded once
inline float exp_c(float v) { return (float)std::exp((double)v); }
inline float sigmoid_c(float v) { return (float)(1.0 / (1.0 + std::exp(-(double)v))); }

}  // namespace

// level l: reg[l] [4][h][w], obj[l] [1][h][w], cls[l] [C][h][w]; out: [A][5 + C], A = the sum of h * w. Returns 0, or -1 for
// arguments outside the contract.
extern "C" int yolox_head_tensor_cpu(const float *const *reg, const float *const *obj, const float *const *cls, const uint32_t *h, const uint32_t *w,
                                     const uint32_t *stride, int n_levels, uint32_t C, float *out) {
  if (!reg || !obj || !cls || !h || !w || !stride || !out || n_levels < 1 || n_levels > 8 || C < 1) return -1;
  const size_t F = 5 + (size_t)C;
  float *row = out;
  for (int l = 0; l < n_levels; l++) {
    if (!reg[l] || !obj[l] || !cls[l] || !h[l] || !w[l] || !stride[l] || stride[l] > 65536) return -1;
    const size_t hw = (size_t)h[l] * w[l];
    const float s = (float)stride[l];
    for (uint32_t y = 0; y < h[l]; y++)
      for (uint32_t x = 0; x < w[l]; x++, row += F) {              // x is the fast index; levels one after the other
        const size_t i = (size_t)y * w[l] + x;
        const float cx = reg[l][i] + (float)x, cy = reg[l][hw + i] + (float)y;   // rounded to f32 before the multiply
        row[0] = cx * s;
        row[1] = cy * s;
        row[2] = exp_c(reg[l][2 * hw + i]) * s;
        row[3] = exp_c(reg[l][3 * hw + i]) * s;
        row[4] = sigmoid_c(obj[l][i]);
        for (uint32_t c = 0; c < C; c++) row[5 + c] = sigmoid_c(cls[l][(size_t)c * hw + i]);
      }
  }
  return 0;
}

// the detections of one head: the tensor above through yolodec_cpu, layout X. scratch: A * (5 + C) floats.
extern "C" int yolox_head_dets_cpu(const float *const *reg, const float *const *obj, const float *const *cls, const uint32_t *h, const uint32_t *w,
                                   const uint32_t *stride, int n_levels, uint32_t C, float box_thr, float class_thr, float iou_thr, float *scratch, void *dets_out,
                                   uint32_t max_dets, uint32_t *n_dets) {
  if (!scratch) return -1;
  const int rc = yolox_head_tensor_cpu(reg, obj, cls, h, w, stride, n_levels, C, scratch);
  if (rc) return rc;
  uint64_t A = 0;
  for (int l = 0; l < n_levels; l++) A += (uint64_t)h[l] * w[l];
  return yolodec_cpu(scratch, 1, 5 + C, (uint32_t)A, box_thr, class_thr, iou_thr, dets_out, max_dets, n_dets);
}
