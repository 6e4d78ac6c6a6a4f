// dssim_fast.hip — the opt-in fast form of videocompare's Dssim engine for (reference, frame) pairs (MI355_FLAG_DSSIM_FAST = 1).
//
// Reference path replaced: the same as dssim_kernels.hip's - HashedImage::new + HashedImage::compare with HashAlgorithm::Dssim
// (video/videofx/src/videocompare/hashed_image.rs:48-79 -> crate dssim-core, sources not in the reference tree; the reference
// test pins identical frames -> 0.0). The exact kernels follow oracle/dssim_restate.py bit for bit; this form follows the same
// algorithm with ONE substitution: every 3 x 3 blur pass is a horizontal then a vertical 3-tap pass with the taps
// [a, b, a] = [0.30876, 0.38248, 0.30876] * sqrt(1.000001) (the published 3 x 3 weights are their outer product to six digits, and
// sum to 1.000001: the gain is matched because it feeds the cancelling sq - mu^2 terms), each pass replicating its own edges. It
// is held to the f64 evaluation of the restatement within the exact form's own f32 rounding noise (tests/test_gpu_dssim_fast.py).
//
// What the kernel evaluates: horizontal and vertical passes commute, so a blur (two 3 x 3 passes) is one 5-tap pass per axis,
// [a^2, 2ab, 2a^2 + b^2, 2ab, a^2]. Two 3-tap passes that each replicate the edge are that 5-tap pass over a SYMMETRICALLY
// padded line (p[-1] = p[0], p[-2] = p[1]; NOT p[-2] = p[0]): tile borders that touch an image edge map their tap coordinates
// that way, in image coordinates, and nothing else distinguishes them.
//
// dssim_pair_kernel: one block = one 32 x 16 tile of one scale of one pair. Both frames' tile plus a halo of 4 is converted to LAB
// into LDS as {reference, frame} pairs of f32 - every later operation is a packed-f32 operation on such a pair (v_pk_fma_f32:
// two IEEE operations), so both frames go through the same instructions and identical frames give identical bits. Chroma
// pre-blur (5-tap x, 5-tap y, in place), then per channel the 5-tap x pass of {p1, p2}, {p1^2, p2^2} and p1 * p2 into LDS and the
// 5-tap y pass per tile pixel into the running sums of the SSIM formula. Only the SSIM map tile and the tile's f64 partial
// reach memory: no img / mu / sq plane does. Fusion is written out (the library is built with -ffp-contract=off).
// Identical frames -> exactly 0.0: i12 comes from the code that gives sq, 2 x stands against x + x, and the quotient of two
// bit-equal numbers is exactly 1 (dssim_fast_div).
#include "internal.hpp"

namespace mi355 {

namespace {

typedef float f2 __attribute__((ext_vector_type(2)));

constexpr int kTw = kDssimFastTw, kTh = kDssimFastTh, kNt = 256, kHalo = 4;
constexpr int kRw = kTw + 2 * kHalo, kRh = kTh + 2 * kHalo, kCells = kRw * kRh;   // 40 x 24 region
constexpr int kPw = kRw - 4, kPh = kRh - 4;                                        // 36 x 20: the tile plus a halo of 2
constexpr int kHcells = kTw * kPh;                                                 // x-pass planes: tile columns x (tile rows + 2 + 2)
constexpr int kPpl = kTw * kTh / kNt;                                              // tile pixels per lane
static_assert(kTw * kTh % kNt == 0 && 5 * kHcells >= 2 * kCells && 5 * kHcells >= 512, "tile geometry; the x-pass planes hold the pre-blur's plane and the tables");

constexpr double kTa = 0.30876, kTb = 0.38248, kGain = 1.000001;   // 1-D taps [a, b, a] * sqrt(gain)
constexpr float kK0 = (float)(kTa * kTa * kGain), kK1 = (float)(2.0 * kTa * kTb * kGain), kK2 = (float)((2.0 * kTa * kTa + kTb * kTb) * kGain);

__device__ __forceinline__ f2 splat(float v) { return f2{v, v}; }
__device__ __forceinline__ f2 fma2(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }

// one blur of one axis from its five (symmetrically padded) samples
__device__ __forceinline__ f2 tap5(f2 v0, f2 v1, f2 v2, f2 v3, f2 v4) { return fma2(splat(kK2), v2, fma2(splat(kK1), v1 + v3, splat(kK0) * (v0 + v4))); }
__device__ __forceinline__ float tap5(float v0, float v1, float v2, float v3, float v4) {
  return __builtin_fmaf(kK2, v2, __builtin_fmaf(kK1, v1 + v3, kK0 * (v0 + v4)));
}

// n / d within an ulp for positive normal operands: reciprocal, one Newton step, quotient, one fused residual correction. For
// n == d: r = (1 + e) / d with |e| < 2^-22, q = n r rounds to 1 + k 2^-24 with |k| <= 4, the residual d - d q = -d k 2^-24 is exact,
// and q + residual * r = 1 - k 2^-24 e exactly, which rounds to 1.0f.
__device__ __forceinline__ float dssim_fast_div(float n, float d) {
  float r = __builtin_amdgcn_rcpf(d);
  r = __builtin_fmaf(__builtin_fmaf(-d, r, 1.0f), r, r);
  const float q = n * r;
  return __builtin_fmaf(__builtin_fmaf(-d, q, n), r, q);
}
__device__ __forceinline__ f2 dssim_fast_div2(f2 n, f2 d) {
  f2 r = {__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y)};
  r = fma2(fma2(-d, r, splat(1.0f)), r, r);
  const f2 q = n * r;
  return fma2(fma2(-d, q, n), r, q);
}

// the crate's LAB variant for a {reference, frame} pair of one cell: polynomial start + two Halley steps for the cube root
__device__ __forceinline__ f2 lab_f(f2 t) {
  const float eps = (float)(216.0 / 24389.0), kk = (float)(24389.0 / (27.0 * 116.0));
  f2 y = fma2(fma2(splat(-0.5f), t, splat(1.51f)), t, splat(0.2f));
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const f2 y3 = y * y * y;
    y = dssim_fast_div2(y * fma2(splat(2.0f), t, y3), fma2(splat(2.0f), y3, t));   // finite for every t >= 0
  }
  const f2 cb = y - splat((float)(16.0 / 116.0)), lin = splat(kk) * t;
  return f2{t.x > eps ? cb.x : lin.x, t.y > eps ? cb.y : lin.y};
}
__device__ __forceinline__ void lab_pair(f2 r, f2 g, f2 b, f2 &L, f2 &A, f2 &B) {
  const double dx = 0.9505, dz = 1.089;
  const f2 fx = fma2(b, splat((float)(0.1805 / dx)), fma2(g, splat((float)(0.3576 / dx)), r * splat((float)(0.4124 / dx))));
  const f2 fy = fma2(b, splat(0.0722f), fma2(g, splat(0.7152f), r * splat(0.2126f)));
  const f2 fz = fma2(b, splat((float)(0.9505 / dz)), fma2(g, splat((float)(0.1192 / dz)), r * splat((float)(0.0193 / dz))));
  const f2 X = lab_f(fx), Y = lab_f(fy), Z = lab_f(fz);
  L = Y * splat(1.05f);
  A = fma2(splat((float)(500.0 / 220.0)), X - Y, splat((float)(86.2 / 220.0)));
  B = fma2(splat((float)(200.0 / 220.0)), Y - Z, splat((float)(107.9 / 220.0)));
}

// premultiplied linear r, g, b of one in-image cell of one frame: gamma table and alpha / 255 (scale 0) or the box chain's
// float4; translucent pixels over the crate's pattern (J.pattern) or over black
__device__ __forceinline__ void linear_px(const DssimFastJob &J, int f, const float *s_lut, int gx, int gy, float &r, float &g, float &b) {
  float a;
  if (J.u8[f]) {
    const uint8_t *p = J.u8[f] + (size_t)gy * J.stride + (size_t)gx * J.channels;
    r = s_lut[p[0]]; g = s_lut[p[1]]; b = s_lut[p[2]];
    if (J.channels != 4) return;
    a = s_lut[256 + p[3]];
    r = r * a; g = g * a; b = b * a;
  } else {
    const float4 v = J.lin[f][(size_t)gy * J.w + gx];
    r = v.x; g = v.y; b = v.z; a = v.w;
  }
  if (J.pattern && a != 1.0f) {
    const int n = (gx + 11) ^ (gy + 11);
    const float t = 1.0f - a;
    if (n & 16) r = r + t;
    if (n & 8) g = g + t;
    if (n & 32) b = b + t;
  }
}

// tap coordinate j of a line of n samples under two replicated 3-tap passes = one 5-tap pass with symmetric padding
template <bool INTERIOR>
__device__ __forceinline__ int sym(int j, int n) {
  if (INTERIOR) return j;
  j = j < 0 ? -1 - j : (j >= n ? 2 * n - 1 - j : j);
  return j < 0 ? 0 : (j >= n ? n - 1 : j);   // lines shorter than 3
}

template <bool INTERIOR>
__device__ __forceinline__ double pair_body(const DssimFastJob &J, f2 (*s_lab)[kCells], float *s_h, int x0, int y0) {
  const int w = J.w, h = J.h, tid = (int)threadIdx.x;
  // 1. LAB of both frames on the region (cells outside the image are never read: every tap coordinate is mapped into it)
  for (int e = tid; e < kCells; e += kNt) {
    const int ly = e / kRw, lx = e - ly * kRw, gx = x0 + lx, gy = y0 + ly;
    f2 L = splat(0.0f), A = L, B = L;
    if (INTERIOR || (gx >= 0 && gx < w && gy >= 0 && gy < h)) {
      float r0, g0, b0, r1, g1, b1;
      linear_px(J, 0, s_h, gx, gy, r0, g0, b0);
      linear_px(J, 1, s_h, gx, gy, r1, g1, b1);
      lab_pair(f2{r0, r1}, f2{g0, g1}, f2{b0, b1}, L, A, B);
    }
    s_lab[0][e] = L; s_lab[1][e] = A; s_lab[2][e] = B;
  }
  __syncthreads();
  // 2. chroma pre-blur, in place: x pass on the region minus 2 columns each side, y pass on the region minus 2 each side
  f2 *const s_t = (f2 *)s_h;
  for (int c = 1; c < 3; c++) {
    f2 *const P = s_lab[c];
    for (int e = tid; e < kPw * kRh; e += kNt) {
      const int ly = e / kPw, lx = 2 + e - ly * kPw, gx = x0 + lx, gy = y0 + ly;
      if (INTERIOR || (gx >= 0 && gx < w && gy >= 0 && gy < h)) {
        const f2 *row = P + ly * kRw;
        s_t[ly * kRw + lx] = tap5(row[sym<INTERIOR>(gx - 2, w) - x0], row[sym<INTERIOR>(gx - 1, w) - x0], row[lx], row[sym<INTERIOR>(gx + 1, w) - x0],
                                  row[sym<INTERIOR>(gx + 2, w) - x0]);
      }
    }
    __syncthreads();
    for (int e = tid; e < kPw * kPh; e += kNt) {
      const int ly = 2 + e / kPw, lx = 2 + e - (e / kPw) * kPw, gx = x0 + lx, gy = y0 + ly;
      if (INTERIOR || (gx >= 0 && gx < w && gy >= 0 && gy < h)) {
        const f2 *col = s_t + lx;
        P[ly * kRw + lx] = tap5(col[(sym<INTERIOR>(gy - 2, h) - y0) * kRw], col[(sym<INTERIOR>(gy - 1, h) - y0) * kRw], col[ly * kRw],
                                col[(sym<INTERIOR>(gy + 1, h) - y0) * kRw], col[(sym<INTERIOR>(gy + 2, h) - y0) * kRw]);
      }
    }
    __syncthreads();
  }
  // 3. per channel: x pass of {p1, p2}, {p1^2, p2^2}, p1 p2 on tile columns x (tile rows +- 2), y pass per tile pixel into the sums
  f2 *const s_hm = (f2 *)s_h, *const s_hs = s_hm + kHcells;
  float *const s_hx = s_h + 4 * kHcells;
  f2 smm[kPpl], svv[kPpl];        // {sum mu1^2, sum mu2^2}, {sum sq1 - mu1^2, sum sq2 - mu2^2} over the channels
  float sm12[kPpl], sv12[kPpl];   // sum mu1 mu2, sum i12 - mu1 mu2
#pragma unroll
  for (int k = 0; k < kPpl; k++) { smm[k] = svv[k] = splat(0.0f); sm12[k] = sv12[k] = 0.0f; }
#pragma unroll
  for (int c = 0; c < 3; c++) {
    for (int e = tid; e < kHcells; e += kNt) {
      const int ry = e / kTw, tx = e - ry * kTw, gx = x0 + kHalo + tx, gy = y0 + 2 + ry;
      if (INTERIOR || (gx < w && gy >= 0 && gy < h)) {
        const f2 *row = s_lab[c] + (ry + 2) * kRw;
        const f2 v0 = row[sym<INTERIOR>(gx - 2, w) - x0], v1 = row[sym<INTERIOR>(gx - 1, w) - x0], v2 = row[kHalo + tx], v3 = row[sym<INTERIOR>(gx + 1, w) - x0],
                 v4 = row[sym<INTERIOR>(gx + 2, w) - x0];
        s_hm[e] = tap5(v0, v1, v2, v3, v4);
        s_hs[e] = tap5(v0 * v0, v1 * v1, v2 * v2, v3 * v3, v4 * v4);
        s_hx[e] = tap5(v0.x * v0.y, v1.x * v1.y, v2.x * v2.y, v3.x * v3.y, v4.x * v4.y);
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kPpl; k++) {
      const int e = tid + k * kNt, ty = e / kTw, tx = e - ty * kTw, gx = x0 + kHalo + tx, gy = y0 + kHalo + ty;
      if (INTERIOR || (gx < w && gy < h)) {
        const int yb = y0 + 2;   // image row of x-pass row 0
        const int r0 = (sym<INTERIOR>(gy - 2, h) - yb) * kTw + tx, r1 = (sym<INTERIOR>(gy - 1, h) - yb) * kTw + tx, r2 = (gy - yb) * kTw + tx,
                  r3 = (sym<INTERIOR>(gy + 1, h) - yb) * kTw + tx, r4 = (sym<INTERIOR>(gy + 2, h) - yb) * kTw + tx;
        const f2 m = tap5(s_hm[r0], s_hm[r1], s_hm[r2], s_hm[r3], s_hm[r4]);
        const f2 q = tap5(s_hs[r0], s_hs[r1], s_hs[r2], s_hs[r3], s_hs[r4]);
        const float x = tap5(s_hx[r0], s_hx[r1], s_hx[r2], s_hx[r3], s_hx[r4]);
        smm[k] = fma2(m, m, smm[k]);
        sm12[k] = __builtin_fmaf(m.x, m.y, sm12[k]);
        svv[k] = svv[k] + fma2(-m, m, q);
        sv12[k] = sv12[k] + __builtin_fmaf(-m.x, m.y, x);
      }
    }
    __syncthreads();
  }
  // 4. the SSIM map and the lane's share of the tile's sum
  const float c1 = (float)(0.01 * 0.01), c2 = (float)(0.03 * 0.03), third = 1.0f / 3.0f;
  double dsum = 0.0;
#pragma unroll
  for (int k = 0; k < kPpl; k++) {
    const int e = tid + k * kNt, ty = e / kTw, tx = e - ty * kTw, gx = x0 + kHalo + tx, gy = y0 + kHalo + ty;
    if (INTERIOR || (gx < w && gy < h)) {
      const f2 mm = smm[k] * splat(third), vv = svv[k] * splat(third);
      const float m12 = sm12[k] * third, v12 = sv12[k] * third;
      const float num = (2.0f * m12 + c1) * (2.0f * v12 + c2), den = ((mm.x + mm.y) + c1) * ((vv.x + vv.y) + c2);
      const float ssim = dssim_fast_div(num, den);
      J.map[(size_t)gy * w + gx] = ssim;
      dsum += (double)ssim;
    }
  }
  return dsum;
}

}  // namespace

// 3 LAB planes of pairs (23,040 B) + the x-pass planes (12,800 B; the pre-blur's plane and the gamma / alpha tables live there
// before them) + the block-sum words: four blocks per CU by LDS
__global__ __launch_bounds__(kNt) void dssim_pair_kernel(DssimFastJobs JJ) {
  __shared__ __attribute__((aligned(16))) f2 s_lab[3][kCells];
  __shared__ __attribute__((aligned(16))) float s_h[5 * kHcells];
  __shared__ double s_w[kNt / 64];
  const int j = blockIdx.x >= JJ.first[2] ? 2 : (blockIdx.x >= JJ.first[1] ? 1 : 0);
  const DssimFastJob &J = JJ.job[j];
  const unsigned tile = blockIdx.x - JJ.first[j];
  if (J.u8[0]) { s_h[threadIdx.x] = JJ.lut[threadIdx.x]; s_h[256 + threadIdx.x] = (float)threadIdx.x / 255.0f; }   // kNt == 256
  const int tiles_x = (J.w + kTw - 1) / kTw;
  const int tx = (int)(tile % (unsigned)tiles_x), ty = (int)(tile / (unsigned)tiles_x);
  const int x0 = tx * kTw - kHalo, y0 = ty * kTh - kHalo;   // image coordinates of region cell (0, 0)
  __syncthreads();
  double v = (x0 >= 0 && y0 >= 0 && x0 + kRw <= J.w && y0 + kRh <= J.h) ? pair_body<true>(J, s_lab, s_h, x0, y0) : pair_body<false>(J, s_lab, s_h, x0, y0);
  // the tile's partial: lanes, then waves, in a fixed order
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) J.partial[tile] = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}
static_assert(kNt == 256, "table load and block sum are written for four waves");

int dssim_fast_enqueue(mi355_ctx *ctx, const DssimFastJobs &J) {
  if (J.first[3] == 0) return MI355_OK;
  hipLaunchKernelGGL(dssim_pair_kernel, dim3(J.first[3]), dim3(kNt), 0, ctx->stream, J);
  return check_hip(ctx, hipGetLastError(), "dssim pair kernel launch");
}

}  // namespace mi355
