// yolox_net.hip — the network of `yoloxinference` (analytics/burn/src/yoloxinference/yolox_burn/model/{blocks,bottleneck,darknet,
// pafpn,head,yolox}.rs): the f32 forward pass of Yolox::forward up to the raw reg / obj / cls maps of the three levels, which
// yolox_head.hip decodes. The contract is DESIGN §4.14 (tests/yolox_net_restate.py restates the model files independently).
//
// The config is walked ONCE into a NetDef: the parameter table (struct declaration order, state-dict names), the convolutions, the
// activation buffers and a flat list of ops in forward order. Every Tensor::cat of the model is PLACEMENT: a producer writes at its
// channel offset into the wider buffer (C3's [x1, x2], SPP's four parts, the PAFPN's [upsampled, feature] and [p_out, fpn_out], the
// head's [reg, obj, cls]), so an op reads and writes VIEWS (buffer, channel offset, channels). A forward is a loop over the list.
// Buffers are placed in one arena per (n_frames, H, W) by liveness: a buffer lives from the first to the last op that touches it
// (features.0/1, fpn_out0/1 and C3's x2 sit in concat buffers whose last reader comes late, so nothing overwrites them).
//
//   yolox_conv_kernel<K, MODE, TPX>  dense k x k conv (k 1 / 3, stride 1 / 2, zero pad (k - 1) / 2) as an implicit GEMM: a block takes 64
//                               output channels x 64 output pixels of one frame, a thread 4 x 4 of them in registers (TPX 4; TPX 1:
//                               64 x 16 and 4 x 1, for grids that would leave compute units idle - the same bytes); the reduction
//                               (input channel, tap) goes through LDS in steps of 16: 16 x 64 weights and 16 x 64 gathered input
//                               values per step, each fetched from memory once per block and used 64 times; the next step's values
//                               are loaded into registers while the current step is summed. Accumulation is fmaf in
//                               ascending (channel, tap) order within a step and one f32 add per step in ascending order (blocked
//                               summation: the error grows with 16 + K / 16, not K), so a result depends on nothing but its own inputs. Both tails (Cout,
//                               Cin k k, pixels) are guarded. MODE 1 folds the Focus gather (blocks.rs:176-211: top-left,
//                               bottom-left, top-right, bottom-right, 3 channels each) into the input addressing of the stem.
//   yolox_conv_mfma_kernel<K, MODE, TN>  the same convolution for a net of MI355_YOLOX_PRECISION_BF16: an implicit
//                               GEMM on v_mfma_f32_16x16x32_bf16. A block takes 64 output channels x TN output pixels of one frame
//                               (TN 64: four waves of 32 x 32; TN 16: four waves of 16 x 16 - the same bytes); the reduction goes
//                               through LDS in steps of 32: a 64 x 32 tile of the weights packed to bf16 at _finalize
//                               (yolox_pack_bf16_kernel: rows padded to 64, the reduction to 32, with zeros) and TN x 32 input
//                               values gathered with the addressing above and rounded to bf16 (nearest, ties to even) on the way
//                               into LDS, both laid out so that a lane's 8 consecutive k are one 16-byte read. Products are exact in
//                               f32, accumulation is f32 in the accumulator registers, one instruction per output and step in
//                               ascending order; the epilogue is conv_store, unchanged.
//   yolox_dw_kernel             depthwise 3 x 3 (groups = C), one lane per output value.
//   yolox_pool5_kernel          max-pool 5 x 5, stride 1, pad 2 with -inf; SPP's 9 and 13 are the cascade 5∘5 and 5∘5∘5 (max is exact).
//   yolox_up2_kernel            nearest 2x: out[y][x] = in[y / 2][x / 2], written into the concat destination.
// A forward is split from the state it plans into (YxLane: arena, input tensor, cached plan, allocation count): the entry points run
// the net's own lane on its context's stream; the video group's decoder queue runs lanes of its own, one per (net serial, H, W), on
// its stream (YxLanes; mi355_group_submit_yolox_infer), reading nothing of the net but what _finalize froze.
// Epilogue of the convolutions: acc * scale + shift per channel (BatchNorm; a prediction layer has scale 1, shift bias), optional SiLU
// x * (1 / (1 + exp(-x))), optional residual added AFTER the activation (bottleneck.rs:20-30).
#include "internal.hpp"

#include <algorithm>
#include <atomic>
#include <climits>
#include <cmath>
#include <map>

namespace mi355 {

namespace {

constexpr int kTM = 64, kTN = 64, kTK = 16, kPad = 4;
constexpr uint32_t kMaxClasses = 1024;

enum OpKind { kOpConv = 0, kOpDw = 1, kOpPool = 2, kOpUp = 3, kOpFocus = 4 };

// one launch: views are (pointer to the view's first channel in frame 0, floats from frame to frame)
struct ConvArgs {
  const float *in;
  unsigned long long in_pitch;
  float *out;
  unsigned long long out_pitch;
  const float *res;   // null: none
  unsigned long long res_pitch;
  const float *w, *scale, *shift;
  uint32_t cin, cout, hi, wi, ho, wo, stride, silu;
  const unsigned short *wp;   // a BF16 net: the packed weights [cout padded to 64][kpad] bf16; null otherwise
  uint32_t kpad;              // cin k k padded to 32
};

__device__ __forceinline__ float silu_f(float v) { return v * (1.0f / (1.0f + expf(-v))); }

__device__ __forceinline__ void conv_store(const ConvArgs &A, uint32_t f, uint32_t oc, uint32_t P, uint32_t p, float acc, float sc, float sh) {
  float v = fmaf(acc, sc, sh);
  if (A.silu) v = silu_f(v);
  const size_t at = (size_t)oc * P + p;
  if (A.res) v = v + A.res[(size_t)f * A.res_pitch + at];
  A.out[(size_t)f * A.out_pitch + at] = v;
}

// grid (pixel tiles, channel tiles, frames); a thread takes 4 channels x TPX pixels, a block 64 channels x 16 TPX pixels
template <int K, int MODE, int TPX>
__global__ __launch_bounds__(256) void yolox_conv_kernel(const ConvArgs A) {
  __shared__ float As[kTK][kTM + kPad];
  constexpr int TN = 16 * TPX;
  __shared__ float Bs[kTK][TN + kPad];
  constexpr uint32_t KK = K * K;
  constexpr int pad = (K - 1) / 2;
  const uint32_t tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const uint32_t P = A.ho * A.wo, p0 = blockIdx.x * TN, oc0 = blockIdx.y * kTM, f = blockIdx.z;
  const uint32_t Ktot = A.cin * KK;
  const float *__restrict__ in = A.in + (size_t)f * A.in_pitch;
  const float *__restrict__ w = A.w;
  // the TPX pixels of this thread: the same in its gather role (row ty of the step) and in its compute role
  int iy0[TPX], ix0[TPX];
  bool pv[TPX];
#pragma unroll
  for (int j = 0; j < TPX; j++) {
    const uint32_t p = p0 + tx * TPX + j;
    pv[j] = p < P;
    const uint32_t oy = pv[j] ? p / A.wo : 0, ox = pv[j] ? p - oy * A.wo : 0;
    iy0[j] = (int)(oy * A.stride) - pad;
    ix0[j] = (int)(ox * A.stride) - pad;
  }
  const uint32_t a_oc = oc0 + (tid >> 2), a_k = (tid & 3) * 4;   // weight role: 4 consecutive reduction indices of one channel
  float acc[4][TPX];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < TPX; j++) acc[i][j] = 0.0f;
  // the values of one step for this thread's two roles: 4 weights, TPX gathered input values
  auto fetch = [&](uint32_t k0, float (&ar)[4], float (&br)[TPX]) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint32_t kk = k0 + a_k + j;
      ar[j] = (a_oc < A.cout && kk < Ktot) ? w[(size_t)a_oc * Ktot + kk] : 0.0f;
    }
    const uint32_t kk = k0 + ty;
    const bool kv = kk < Ktot;
    const uint32_t ci = kk / KK, tap = kk - ci * KK;
    const int dy = (int)(tap / K), dx = (int)(tap - (tap / K) * K);
#pragma unroll
    for (int j = 0; j < TPX; j++) {
      const int iy = iy0[j] + dy, ix = ix0[j] + dx;
      float v = 0.0f;
      if (kv && pv[j] && (unsigned)iy < A.hi && (unsigned)ix < A.wi) {
        if (MODE == 0) {
          v = in[((size_t)ci * A.hi + (uint32_t)iy) * A.wi + (uint32_t)ix];
        } else {   // Focus: channel ci = 3 * patch + c; patch 0 .. 3 = top-left, bottom-left, top-right, bottom-right
          const uint32_t patch = ci / 3, c = ci - 3 * patch;
          const uint32_t fy = 2 * (uint32_t)iy + (patch & 1), fx = 2 * (uint32_t)ix + (patch >> 1);
          v = in[((size_t)c * (2 * A.hi) + fy) * (2 * A.wi) + fx];
        }
      }
      br[j] = v;
    }
  };
  float ar[4], br[TPX];
  fetch(0, ar, br);
  for (uint32_t k0 = 0; k0 < Ktot; k0 += kTK) {
#pragma unroll
    for (int j = 0; j < 4; j++) As[a_k + j][tid >> 2] = ar[j];
#pragma unroll
    for (int j = 0; j < TPX; j++) Bs[ty][tx * TPX + j] = br[j];
    __syncthreads();
    if (k0 + kTK < Ktot) fetch(k0 + kTK, ar, br);   // the next step's loads are in flight while this one is summed
    float part[4][TPX];   // the step's 16 terms on their own, then one add: the rounding error of a long reduction grows with the
#pragma unroll          // number of steps, not of terms
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int j = 0; j < TPX; j++) part[i][j] = 0.0f;
#pragma unroll
    for (int kk = 0; kk < kTK; kk++) {
      const float4 a = *reinterpret_cast<const float4 *>(&As[kk][ty * 4]);
      const float av[4] = {a.x, a.y, a.z, a.w};
      float bv[TPX];
      if (TPX == 4) {
        const float4 b = *reinterpret_cast<const float4 *>(&Bs[kk][tx * TPX]);
        bv[0] = b.x, bv[TPX > 1 ? 1 : 0] = b.y, bv[TPX > 2 ? 2 : 0] = b.z, bv[TPX > 3 ? 3 : 0] = b.w;
      } else {
#pragma unroll
        for (int j = 0; j < TPX; j++) bv[j] = Bs[kk][tx * TPX + j];
      }
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < TPX; j++) part[i][j] = fmaf(av[i], bv[j], part[i][j]);
    }
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int j = 0; j < TPX; j++) acc[i][j] = acc[i][j] + part[i][j];
    __syncthreads();   // the tiles are written again
  }
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const uint32_t oc = oc0 + ty * 4 + i;
    if (oc >= A.cout) continue;
    const float sc = A.scale[oc], sh = A.shift[oc];
#pragma unroll
    for (int j = 0; j < TPX; j++) {
      const uint32_t p = p0 + tx * TPX + j;
      if (p < P) conv_store(A, f, oc, P, p, acc[i][j], sc, sh);
    }
  }
}

// grid (pixel groups of 256, channels, frames); weights [C][1][3][3]
__global__ __launch_bounds__(256) void yolox_dw_kernel(const ConvArgs A) {
  const uint32_t P = A.ho * A.wo, p = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y, f = blockIdx.z;
  if (p >= P) return;
  const uint32_t oy = p / A.wo, ox = p - oy * A.wo;
  const float *__restrict__ in = A.in + (size_t)f * A.in_pitch + (size_t)c * A.hi * A.wi;
  const float *__restrict__ w = A.w + (size_t)c * 9;
  float acc = 0.0f;
#pragma unroll
  for (int dy = 0; dy < 3; dy++)
#pragma unroll
    for (int dx = 0; dx < 3; dx++) {
      const int iy = (int)(oy * A.stride) - 1 + dy, ix = (int)(ox * A.stride) - 1 + dx;
      if ((unsigned)iy < A.hi && (unsigned)ix < A.wi) acc = fmaf(w[dy * 3 + dx], in[(size_t)(uint32_t)iy * A.wi + (uint32_t)ix], acc);
    }
  conv_store(A, f, c, P, p, acc, A.scale[c], A.shift[c]);
}

// grid (groups of 256 values of a frame's C planes, 1, frames)
__global__ __launch_bounds__(256) void yolox_pool5_kernel(const float *__restrict__ in, unsigned long long in_pitch, float *__restrict__ out,
                                                           unsigned long long out_pitch, uint32_t C, uint32_t h, uint32_t w) {
  const size_t P = (size_t)h * w, e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= P * C) return;
  const uint32_t c = (uint32_t)(e / P), p = (uint32_t)(e - (size_t)c * P), y = p / w, x = p - y * w;
  const float *__restrict__ src = in + (size_t)blockIdx.z * in_pitch + (size_t)c * P;
  const uint32_t y_lo = y >= 2 ? y - 2 : 0, y_hi = y + 2 < h ? y + 2 : h - 1, x_lo = x >= 2 ? x - 2 : 0, x_hi = x + 2 < w ? x + 2 : w - 1;
  float m = -INFINITY;   // the padding never wins
  for (uint32_t yy = y_lo; yy <= y_hi; yy++)
    for (uint32_t xx = x_lo; xx <= x_hi; xx++) m = fmaxf(m, src[(size_t)yy * w + xx]);
  out[(size_t)blockIdx.z * out_pitch + e] = m;
}

// grid (groups of 256 output values of a frame's C planes, 1, frames); h, w: the input's
__global__ __launch_bounds__(256) void yolox_up2_kernel(const float *__restrict__ in, unsigned long long in_pitch, float *__restrict__ out,
                                                         unsigned long long out_pitch, uint32_t C, uint32_t h, uint32_t w) {
  const size_t Po = (size_t)4 * h * w, e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= Po * C) return;
  const uint32_t c = (uint32_t)(e / Po), p = (uint32_t)(e - (size_t)c * Po), y = p / (2 * w), x = p - y * (2 * w);
  out[(size_t)blockIdx.z * out_pitch + e] = in[(size_t)blockIdx.z * in_pitch + ((size_t)c * h + (y >> 1)) * w + (x >> 1)];
}

// ---- bf16 operands on the matrix cores (MI355_YOLOX_PRECISION_BF16)

constexpr int kMK = 32, kMPitch = 40;   // the reduction step; bf16 values from row to row of a tile in LDS (80 B: 16-byte reads stay aligned)

// f32 -> bf16, round to nearest, ties to even, on the bit pattern: finite values below 2^127 (the contract excludes the rest)
__host__ __device__ __forceinline__ uint32_t bf16_rne(uint32_t bits) { return (bits + 0x7FFFu + ((bits >> 16) & 1u)) >> 16; }

// one dense conv's weights [cout][ktot] f32 -> [rows][kpad] bf16, zeros in the padding; grid: groups of 256 values
__global__ __launch_bounds__(256) void yolox_pack_bf16_kernel(const float *__restrict__ w, unsigned short *__restrict__ out, uint32_t cout, uint32_t ktot, uint32_t rows,
                                                                 uint32_t kpad) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)rows * kpad) return;
  const uint32_t r = (uint32_t)(e / kpad), c = (uint32_t)(e - (size_t)r * kpad);
  out[e] = (r < cout && c < ktot) ? (unsigned short)bf16_rne(__float_as_uint(w[(size_t)r * ktot + c])) : (unsigned short)0;
}

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(4))) float f32x4;

// two activations -> two bf16 in one dword, the first in the low half: the hardware's conversion (v_cvt_pk_bf16_f32: round to nearest,
// ties to even - for the values of the contract the bits of bf16_rne, which tests/test_gpu_yolox_net_bf16.py pins with planted ties)
__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
  const bf16x2 r = __builtin_convertvector(f32x2{lo, hi}, bf16x2);
  return __builtin_bit_cast(uint32_t, r);
}

// grid (pixel tiles, channel tiles, frames); 4 waves: TN 64 as 2 x 2 of 32 channels x 32 pixels, TN 16 as 4 x 1 of 16 x 16
template <int K, int MODE, int TN>
__global__ __launch_bounds__(256) void yolox_conv_mfma_kernel(const ConvArgs A) {
  static_assert(TN == 64 || TN == 16, "tile");
  constexpr int KPT = kMK * TN / 256;           // gathered values of a step per thread: 8 consecutive k of one pixel, or 2
  constexpr int MI = TN == 64 ? 2 : 1, NI = MI;  // 16 x 16 tiles of a wave
  __shared__ __attribute__((aligned(16))) unsigned short As[kTM][kMPitch];
  __shared__ __attribute__((aligned(16))) unsigned short Bs[TN][kMPitch];
  constexpr uint32_t KK = K * K;
  constexpr int pad = (K - 1) / 2;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t P = A.ho * A.wo, p0 = blockIdx.x * TN, oc0 = blockIdx.y * kTM, f = blockIdx.z;
  const uint32_t Ktot = A.cin * KK;
  const float *__restrict__ in = A.in + (size_t)f * A.in_pitch;
  // gather role: one pixel, KPT consecutive reduction indices
  const uint32_t g_px = tid % TN, g_k = (tid / TN) * KPT;
  const uint32_t gp = p0 + g_px;
  const bool pv = gp < P;
  const uint32_t oy = pv ? gp / A.wo : 0, ox = pv ? gp - oy * A.wo : 0;
  const int iy0 = (int)(oy * A.stride) - pad, ix0 = (int)(ox * A.stride) - pad;
  const uint32_t plane = A.hi * A.wi;
  // weight role: 8 consecutive reduction indices of one channel, 16 bytes of the packed store (padded: no guard)
  const unsigned short *__restrict__ wrow = A.wp + (size_t)(oc0 + (tid >> 2)) * A.kpad + (tid & 3) * 8;
  auto fetch = [&](uint32_t k0, uint4 &ar, float (&br)[KPT]) {
    ar = *reinterpret_cast<const uint4 *>(wrow + k0);
    uint32_t kk = k0 + g_k;
    uint32_t ci = kk / KK, tap = kk - ci * KK;
#pragma unroll
    for (int j = 0; j < KPT; j++) {
      const int dy = (int)(tap / K), dx = (int)(tap - (tap / K) * K);
      const int iy = iy0 + dy, ix = ix0 + dx;
      // every load is issued, at the view's first value where the term is padding, and then zeroed: no branch around a load,
      // so the step's loads are in flight together
      const bool ok = kk < Ktot && pv && (unsigned)iy < A.hi && (unsigned)ix < A.wi;
      size_t at;   // one 32-bit offset inside a plane (a side is at most 2048), one 64-bit multiply-add for the plane
      if (MODE == 0) {
        at = (size_t)ci * plane + ((uint32_t)iy * A.wi + (uint32_t)ix);
      } else {   // Focus, as in yolox_conv_kernel
        const uint32_t patch = ci / 3, c = ci - 3 * patch;
        const uint32_t fy = 2 * (uint32_t)iy + (patch & 1), fx = 2 * (uint32_t)ix + (patch >> 1);
        at = (size_t)c * (4 * plane) + (fy * (2 * A.wi) + fx);
      }
      float v = in[ok ? at : 0];
      v = ok ? v : 0.0f;
      br[j] = v;
      kk++;
      if (++tap == KK) tap = 0, ci++;
    }
  };
  const uint32_t wm = TN == 64 ? wave >> 1 : wave, wn = TN == 64 ? wave & 1 : 0;   // the wave's place in the block's tile
  const uint32_t fr = lane & 15, fk = (lane >> 4) * 8;                              // fragment row (A) or column (B); first k
  f32x4 acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; i++)
#pragma unroll
    for (int j = 0; j < NI; j++) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  uint4 ar;
  float br[KPT];
  fetch(0, ar, br);
  for (uint32_t k0 = 0; k0 < Ktot; k0 += kMK) {
    *reinterpret_cast<uint4 *>(&As[tid >> 2][(tid & 3) * 8]) = ar;
    uint32_t pk[KPT / 2];
#pragma unroll
    for (int j = 0; j < KPT / 2; j++) pk[j] = pack_bf16x2(br[2 * j], br[2 * j + 1]);
    if (KPT == 8) *reinterpret_cast<uint4 *>(&Bs[g_px][g_k]) = uint4{pk[0], pk[KPT > 2 ? 1 : 0], pk[KPT > 4 ? 2 : 0], pk[KPT > 6 ? 3 : 0]};
    else *reinterpret_cast<uint32_t *>(&Bs[g_px][g_k]) = pk[0];
    __syncthreads();
    if (k0 + kMK < Ktot) fetch(k0 + kMK, ar, br);   // the next step's loads are in flight while this one is summed
    bf16x8 af[MI], bf[NI];
#pragma unroll
    for (int i = 0; i < MI; i++) af[i] = *reinterpret_cast<const bf16x8 *>(&As[(wm * MI + i) * 16 + fr][fk]);
#pragma unroll
    for (int j = 0; j < NI; j++) bf[j] = *reinterpret_cast<const bf16x8 *>(&Bs[(wn * NI + j) * 16 + fr][fk]);
#pragma unroll
    for (int i = 0; i < MI; i++)
#pragma unroll
      for (int j = 0; j < NI; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bf[j], acc[i][j], 0, 0, 0);
    __syncthreads();   // the tiles are written again
  }
  // accumulator register r of a lane: channel 4 (lane / 16) + r, pixel lane % 16 of the 16 x 16 tile
#pragma unroll
  for (int i = 0; i < MI; i++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const uint32_t oc = oc0 + (wm * MI + i) * 16 + (lane >> 4) * 4 + r;
      if (oc >= A.cout) continue;
      const float sc = A.scale[oc], sh = A.shift[oc];
#pragma unroll
      for (int j = 0; j < NI; j++) {
        const uint32_t p = p0 + (wn * NI + j) * 16 + fr;
        if (p < P) conv_store(A, f, oc, P, p, acc[i][j][r], sc, sh);
      }
    }
}

// ---- the definition of a net: what the config alone decides

struct ParamDef {
  std::string name;
  int nd;
  uint32_t dims[4];
  size_t n, off;   // elements; first float in the parameter store
};
struct ConvDef {
  int w = -1, g = -1, b = -1, m = -1, v = -1, bias = -1;   // parameter indices; a BaseConv has w + the four bn, a prediction layer w + bias
  uint32_t cin = 0, cout = 0, k = 1, stride = 1;
  bool dw = false;
  size_t ss = 0;   // first channel in the scale / shift arrays
};
struct BufDef {
  uint32_t C, ds;   // channels; the buffer's maps are (H / ds) x (W / ds)
  int first, last;  // the ops that touch it first and last
  bool keep;        // a level's output: lives until the next forward
};
struct View { int buf; uint32_t off, C; };   // buf 0: the caller's input frames
struct OpDef {
  int kind;
  View in, out, res;
  bool has_res, silu;
  int conv;
};
struct NetDef {
  mi355_yolox_net_config cfg{};
  std::vector<ParamDef> params;
  std::vector<ConvDef> convs;
  std::map<std::string, int> conv_by_name;
  std::vector<BufDef> bufs;
  std::vector<OpDef> ops;
  size_t param_floats = 0, ss_channels = 0;
  int level_buf[3] = {-1, -1, -1};
  bool bad = false;   // a lookup or a channel count that does not fit: the walk is wrong
};

uint32_t expand(uint32_t n, double factor) { return (uint32_t)std::floor((double)n * factor); }   // blocks.rs:12

struct Builder {
  NetDef &N;
  bool depthwise;

  int add_param(const std::string &name, int nd, uint32_t d0, uint32_t d1 = 1, uint32_t d2 = 1, uint32_t d3 = 1) {
    ParamDef p;
    p.name = name;
    p.nd = nd;
    p.dims[0] = d0, p.dims[1] = d1, p.dims[2] = d2, p.dims[3] = d3;
    p.n = (size_t)d0 * d1 * d2 * d3;
    p.off = N.param_floats;
    N.param_floats += p.n;
    N.params.push_back(p);
    return (int)N.params.size() - 1;
  }
  int add_conv(const std::string &name, ConvDef c) {
    c.ss = N.ss_channels;
    N.ss_channels += c.cout;
    N.convs.push_back(c);
    N.conv_by_name[name] = (int)N.convs.size() - 1;
    return (int)N.convs.size() - 1;
  }
  // ---- declarations, in the order the structs declare their fields
  void decl_base(const std::string &name, uint32_t cin, uint32_t cout, uint32_t k, uint32_t stride, bool dw = false) {   // BaseConv
    ConvDef c;
    c.cin = cin, c.cout = cout, c.k = k, c.stride = stride, c.dw = dw;
    c.w = add_param(name + ".conv.weight", 4, cout, dw ? 1 : cin, k, k);
    c.g = add_param(name + ".bn.weight", 1, cout);
    c.b = add_param(name + ".bn.bias", 1, cout);
    c.m = add_param(name + ".bn.running_mean", 1, cout);
    c.v = add_param(name + ".bn.running_var", 1, cout);
    add_conv(name, c);
  }
  void decl_conv(const std::string &name, uint32_t cin, uint32_t cout, uint32_t k, uint32_t stride) {   // Conv: BaseConv or DwsConv
    if (depthwise) {
      decl_base(name + ".dconv", cin, cin, k, stride, true);
      decl_base(name + ".pconv", cin, cout, 1, 1);
    } else {
      decl_base(name, cin, cout, k, stride);
    }
  }
  void decl_c3(const std::string &name, uint32_t cin, uint32_t cout, uint32_t n) {   // CspBottleneck, expansion 0.5
    const uint32_t hid = expand(cout, 0.5);
    decl_base(name + ".conv1", cin, hid, 1, 1);
    decl_base(name + ".conv2", cin, hid, 1, 1);
    decl_base(name + ".conv3", 2 * hid, cout, 1, 1);
    for (uint32_t i = 0; i < n; i++) {
      const std::string b = name + ".m." + std::to_string(i);
      decl_base(b + ".conv1", hid, hid, 1, 1);
      decl_conv(b + ".conv2", hid, hid, 3, 1);
    }
  }
  void decl_block(const std::string &name, uint32_t cin, uint32_t cout, uint32_t depth, bool spp) {   // CspBlock: conv, c3, spp
    decl_conv(name + ".conv", cin, cout, 3, 2);
    decl_c3(name + ".c3", cout, cout, depth);
    if (spp) {
      decl_base(name + ".spp.conv1", cout, cout / 2, 1, 1);
      decl_base(name + ".spp.conv2", (cout / 2) * 4, cout, 1, 1);
    }
  }
  void decl_pred(const std::string &name, uint32_t cin, uint32_t cout) {
    ConvDef c;
    c.cin = cin, c.cout = cout;
    c.w = add_param(name + ".weight", 4, cout, cin, 1, 1);
    c.bias = add_param(name + ".bias", 1, cout);
    add_conv(name, c);
  }

  // ---- the forward walk
  int new_buf(uint32_t C, uint32_t ds, bool keep = false) {
    N.bufs.push_back({C, ds, INT_MAX, -1, keep});
    return (int)N.bufs.size() - 1;
  }
  void touch(const View &v) {
    BufDef &b = N.bufs[v.buf];
    const int at = (int)N.ops.size();
    b.first = std::min(b.first, at);
    b.last = std::max(b.last, at);
    if (v.off + v.C > b.C) N.bad = true;
  }
  void push(const OpDef &op) {
    touch(op.in);
    touch(op.out);
    if (op.has_res) touch(op.res);
    N.ops.push_back(op);
  }
  // a BaseConv or prediction layer by name: into dst (channels dst.C = cout) or a new buffer
  View base(const std::string &name, View in, const View *dst = nullptr, const View *res = nullptr, bool focus = false) {
    auto it = N.conv_by_name.find(name);
    if (it == N.conv_by_name.end()) {
      N.bad = true;
      return in;
    }
    const ConvDef &c = N.convs[it->second];
    const uint32_t ds = N.bufs[in.buf].ds * (focus ? 2 : c.stride);
    if ((focus ? in.C * 4 : in.C) != c.cin) N.bad = true;
    View out = dst ? *dst : View{new_buf(c.cout, ds), 0, c.cout};
    if (out.C != c.cout || N.bufs[out.buf].ds != ds) N.bad = true;
    OpDef op{};
    op.kind = focus ? kOpFocus : c.dw ? kOpDw : kOpConv;
    op.in = in, op.out = out;
    op.has_res = res != nullptr;
    if (res) op.res = *res;
    op.silu = c.bias < 0;   // every BaseConv; not the prediction layers
    op.conv = it->second;
    push(op);
    return out;
  }
  View conv(const std::string &name, View in, const View *dst = nullptr, const View *res = nullptr) {   // Conv
    if (!depthwise) return base(name, in, dst, res);
    const View t = base(name + ".dconv", in);
    return base(name + ".pconv", t, dst, res);
  }
  View c3(const std::string &name, View in, uint32_t cout, uint32_t n, bool shortcut, const View *dst = nullptr) {
    const uint32_t hid = expand(cout, 0.5), ds = N.bufs[in.buf].ds;
    const int cat = new_buf(2 * hid, ds);
    const View x1_dst{cat, 0, hid}, x2_dst{cat, hid, hid};
    View x = base(name + ".conv1", in);
    base(name + ".conv2", in, &x2_dst);
    for (uint32_t i = 0; i < n; i++) {
      const std::string b = name + ".m." + std::to_string(i);
      const View u = base(b + ".conv1", x);
      x = conv(b + ".conv2", u, i + 1 == n ? &x1_dst : nullptr, shortcut ? &x : nullptr);
    }
    const View all{cat, 0, 2 * hid};
    return base(name + ".conv3", all, dst);
  }
  View spp(const std::string &name, View in, uint32_t cout) {
    const uint32_t hid = in.C / 2, ds = N.bufs[in.buf].ds;
    const int cat = new_buf(4 * hid, ds);
    const View part0{cat, 0, hid};
    base(name + ".conv1", in, &part0);
    for (uint32_t i = 1; i < 4; i++) {   // 5, 9 = 5∘5, 13 = 5∘5∘5
      OpDef op{};
      op.kind = kOpPool;
      op.in = View{cat, (i - 1) * hid, hid};
      op.out = View{cat, i * hid, hid};
      op.conv = -1;
      push(op);
    }
    (void)cout;
    return base(name + ".conv2", View{cat, 0, 4 * hid});
  }
  View block(const std::string &name, View in, uint32_t cout, uint32_t depth, bool with_spp, const View *dst = nullptr) {   // CspBlock::forward
    View x = conv(name + ".conv", in);
    if (with_spp) x = spp(name + ".spp", x, cout);
    return c3(name + ".c3", x, cout, depth, !with_spp, dst);
  }
  void up2(View in, View out) {
    OpDef op{};
    op.kind = kOpUp;
    op.in = in, op.out = out;
    op.conv = -1;
    if (N.bufs[in.buf].ds != 2 * N.bufs[out.buf].ds || in.C != out.C) N.bad = true;
    push(op);
  }
};

bool in_set(double v, const double *set, int n) {
  for (int i = 0; i < n; i++)
    if (v == set[i]) return true;
  return false;
}

int check_config(const mi355_yolox_net_config *cfg, const char **why) {
  static const double depths[4] = {0.33, 0.67, 1.0, 1.33}, widths[6] = {0.25, 0.375, 0.5, 0.75, 1.0, 1.25};
  *why = nullptr;
  if (!cfg) *why = "yolox_net: null config";
  else if (cfg->reserved != 0) *why = "yolox_net: the config's reserved field is not 0";
  else if (!in_set(cfg->depth, depths, 4)) *why = "yolox_net: depth is not one of 0.33, 0.67, 1.0, 1.33";
  else if (!in_set(cfg->width, widths, 6)) *why = "yolox_net: width is not one of 0.25, 0.375, 0.5, 0.75, 1.0, 1.25";
  else if (cfg->depthwise != 0 && cfg->depthwise != 1) *why = "yolox_net: depthwise is neither 0 nor 1";
  else if (cfg->num_classes < 1) *why = "yolox_net: num_classes must be at least 1";
  if (*why) return MI355_ERR_INVALID_ARG;
  if (cfg->num_classes > kMaxClasses) {
    *why = "yolox_net: more than 1024 classes";
    return MI355_ERR_UNSUPPORTED;
  }
  return MI355_OK;
}
int check_frames(int n_frames, const char **why) {
  *why = nullptr;
  if (n_frames < 1) {
    *why = "yolox_net: n_frames must be at least 1";
    return MI355_ERR_INVALID_ARG;
  }
  if (n_frames > MI355_YOLOX_NET_MAX_FRAMES) {
    *why = "yolox_net: more than 64 frames";
    return MI355_ERR_UNSUPPORTED;
  }
  return MI355_OK;
}
int check_size(uint32_t H, uint32_t W, const char **why) {
  *why = nullptr;
  if (H == 0 || W == 0 || H % 32 != 0 || W % 32 != 0) {
    *why = "yolox_net: H and W must be positive multiples of 32";
    return MI355_ERR_INVALID_ARG;
  }
  if (H > MI355_YOLOX_NET_MAX_SIDE || W > MI355_YOLOX_NET_MAX_SIDE) {
    *why = "yolox_net: a side above 2048";
    return MI355_ERR_UNSUPPORTED;
  }
  return MI355_OK;
}

// a checked config -> its definition
bool build_def(const mi355_yolox_net_config &cfg, NetDef *out) {
  NetDef &N = *out;
  N.cfg = cfg;
  Builder B{N, cfg.depthwise != 0};
  const double wd = cfg.width;
  const uint32_t base = expand(64, wd);
  const uint32_t base_depth = std::max((uint32_t)std::llround(cfg.depth * 3.0), 1u);   // darknet.rs:62
  const uint32_t n_blocks = (uint32_t)std::llround(3.0 * cfg.depth);                   // pafpn.rs:106
  const uint32_t in0 = expand(256, wd), in1 = expand(512, wd), in2 = expand(1024, wd);
  const uint32_t hid0 = expand(512, wd), hid1 = expand(1024, wd), hc = expand(256, wd), C = cfg.num_classes;
  const std::string bb = "backbone.backbone.", pf = "backbone.", hd = "head.";
  // ---- parameters
  B.decl_base(bb + "stem.conv", 12, base, 3, 1);
  B.decl_block(bb + "dark2", base, base * 2, base_depth, false);
  B.decl_block(bb + "dark3", base * 2, base * 4, base_depth * 3, false);
  B.decl_block(bb + "dark4", base * 4, base * 8, base_depth * 3, false);
  B.decl_block(bb + "dark5", base * 8, base * 16, base_depth, true);
  B.decl_base(pf + "lateral_conv0", in2, in1, 1, 1);
  B.decl_c3(pf + "c3_n3", hid0, in1, n_blocks);
  B.decl_c3(pf + "c3_n4", hid1, in2, n_blocks);
  B.decl_c3(pf + "c3_p3", hid0, in0, n_blocks);
  B.decl_c3(pf + "c3_p4", hid1, in1, n_blocks);
  B.decl_base(pf + "reduce_conv1", in1, in0, 1, 1);
  B.decl_conv(pf + "bu_conv1", in1, in1, 3, 2);
  B.decl_conv(pf + "bu_conv2", in0, in0, 3, 2);
  const uint32_t feat_c[3] = {in0, in1, in2};
  for (int l = 0; l < 3; l++) B.decl_base(hd + "stems." + std::to_string(l), feat_c[l], hc, 1, 1);
  for (const char *branch : {"cls_convs.", "reg_convs."})
    for (int l = 0; l < 3; l++) {
      B.decl_conv(hd + branch + std::to_string(l) + ".conv0", hc, hc, 3, 1);
      B.decl_conv(hd + branch + std::to_string(l) + ".conv1", hc, hc, 3, 1);
    }
  for (int l = 0; l < 3; l++) B.decl_pred(hd + "cls_preds." + std::to_string(l), hc, C);
  for (int l = 0; l < 3; l++) B.decl_pred(hd + "reg_preds." + std::to_string(l), hc, 4);
  for (int l = 0; l < 3; l++) B.decl_pred(hd + "obj_preds." + std::to_string(l), hc, 1);
  // ---- ops
  N.bufs.push_back({3, 1, INT_MAX, -1, false});   // buffer 0: the caller's frames
  const View frames{0, 0, 3};
  // the four concat buffers of the PAFPN (pafpn.rs:49-65): [upsampled, features.1], [upsampled, features.0], [bu_conv2, fpn_out1], [bu_conv1, fpn_out0]
  const int catA = B.new_buf(in1 + base * 8, 16), catB = B.new_buf(in0 + base * 4, 8), catC = B.new_buf(2 * in0, 16), catD = B.new_buf(2 * in1, 32);
  const View feat0{catB, in0, base * 4}, feat1{catA, in1, base * 8}, fpn1{catC, in0, in0}, fpn0{catD, in1, in1};
  View x = B.base(bb + "stem.conv", frames, nullptr, nullptr, true);
  x = B.block(bb + "dark2", x, base * 2, base_depth, false);
  B.block(bb + "dark3", x, base * 4, base_depth * 3, false, &feat0);
  B.block(bb + "dark4", feat0, base * 8, base_depth * 3, false, &feat1);
  const View feat2 = B.block(bb + "dark5", feat1, base * 16, base_depth, true);
  B.base(pf + "lateral_conv0", feat2, &fpn0);
  B.up2(fpn0, View{catA, 0, in1});
  const View f_out0 = B.c3(pf + "c3_p4", View{catA, 0, in1 + base * 8}, in1, n_blocks, false);
  B.base(pf + "reduce_conv1", f_out0, &fpn1);
  B.up2(fpn1, View{catB, 0, in0});
  const View pan2 = B.c3(pf + "c3_p3", View{catB, 0, in0 + base * 4}, in0, n_blocks, false);
  const View p_out1{catC, 0, in0};
  B.conv(pf + "bu_conv2", pan2, &p_out1);
  const View pan1 = B.c3(pf + "c3_n3", View{catC, 0, 2 * in0}, in1, n_blocks, false);
  const View p_out0{catD, 0, in1};
  B.conv(pf + "bu_conv1", pan1, &p_out0);
  const View pan0 = B.c3(pf + "c3_n4", View{catD, 0, 2 * in1}, in2, n_blocks, false);
  const View feats[3] = {pan2, pan1, pan0};
  for (int l = 0; l < 3; l++) {   // head.rs:63-75: [reg 4][obj 1][cls C] in the level's buffer
    const std::string s = std::to_string(l);
    const int lv = N.level_buf[l] = B.new_buf(5 + C, 8u << l, true);
    const View reg{lv, 0, 4}, obj{lv, 4, 1}, cls{lv, 5, C};
    const View feat = B.base(hd + "stems." + s, feats[l]);
    View t = B.conv(hd + "cls_convs." + s + ".conv0", feat);
    t = B.conv(hd + "cls_convs." + s + ".conv1", t);
    B.base(hd + "cls_preds." + s, t, &cls);
    t = B.conv(hd + "reg_convs." + s + ".conv0", feat);
    t = B.conv(hd + "reg_convs." + s + ".conv1", t);
    B.base(hd + "reg_preds." + s, t, &reg);
    B.base(hd + "obj_preds." + s, t, &obj);
  }
  return !N.bad;
}

// the arena of a shape: every buffer's first float (64-float granules) and the arena's floats. A buffer may share memory with
// another only if their [first, last] op ranges do not meet; a level's buffer is never shared.
void plan_arena(const NetDef &N, uint32_t n_frames, uint32_t H, uint32_t W, std::vector<size_t> *offset, size_t *arena_floats) {
  const size_t nb = N.bufs.size();
  offset->assign(nb, 0);
  std::vector<size_t> size(nb, 0);
  std::vector<int> order;
  for (size_t b = 1; b < nb; b++) {
    const BufDef &d = N.bufs[b];
    size[b] = (((size_t)n_frames * d.C * (H / d.ds) * (W / d.ds)) + 63) / 64 * 64;
    order.push_back((int)b);
  }
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return N.bufs[a].first < N.bufs[b].first; });
  std::vector<int> placed;
  size_t top = 0;
  for (int b : order) {
    const int first = N.bufs[b].first, last = N.bufs[b].keep ? INT_MAX : N.bufs[b].last;
    std::vector<std::pair<size_t, size_t>> busy;   // the ranges of the placed buffers alive with this one
    for (int q : placed) {
      const int qf = N.bufs[q].first, ql = N.bufs[q].keep ? INT_MAX : N.bufs[q].last;
      if (qf <= last && first <= ql) busy.push_back({(*offset)[q], (*offset)[q] + size[q]});
    }
    std::sort(busy.begin(), busy.end());
    size_t at = 0;
    for (const auto &r : busy)
      if (at + size[b] > r.first && at < r.second) at = r.second;   // sorted by start: the first gap that holds the buffer
    (*offset)[b] = at;
    top = std::max(top, at + size[b]);
    placed.push_back(b);
  }
  *arena_floats = top;
}

uint64_t count_macs(const NetDef &N, uint32_t n_frames, uint32_t H, uint32_t W) {
  uint64_t macs = 0;
  for (const OpDef &op : N.ops) {
    if (op.conv < 0) continue;
    const ConvDef &c = N.convs[op.conv];
    const uint32_t ds = N.bufs[op.out.buf].ds;
    macs += (uint64_t)n_frames * c.cout * (H / ds) * (W / ds) * (c.dw ? 1 : c.cin) * c.k * c.k;
  }
  return macs;
}

template <int TPX>
void launch_conv(hipStream_t stream, int kind, const ConvArgs &A, uint32_t k, uint32_t n_frames) {
  const uint32_t P = A.ho * A.wo, tn = 16 * TPX;
  const dim3 grid((P + tn - 1) / tn, (A.cout + kTM - 1) / kTM, n_frames);
  if (kind == kOpFocus) hipLaunchKernelGGL((yolox_conv_kernel<3, 1, TPX>), grid, dim3(256), 0, stream, A);
  else if (k == 3) hipLaunchKernelGGL((yolox_conv_kernel<3, 0, TPX>), grid, dim3(256), 0, stream, A);
  else hipLaunchKernelGGL((yolox_conv_kernel<1, 0, TPX>), grid, dim3(256), 0, stream, A);
}

template <int TN>
void launch_conv_mfma(hipStream_t stream, int kind, const ConvArgs &A, uint32_t k, uint32_t n_frames) {
  const uint32_t P = A.ho * A.wo;
  const dim3 grid((P + TN - 1) / TN, (A.cout + kTM - 1) / kTM, n_frames);
  if (kind == kOpFocus) hipLaunchKernelGGL((yolox_conv_mfma_kernel<3, 1, TN>), grid, dim3(256), 0, stream, A);
  else if (k == 3) hipLaunchKernelGGL((yolox_conv_mfma_kernel<3, 0, TN>), grid, dim3(256), 0, stream, A);
  else hipLaunchKernelGGL((yolox_conv_mfma_kernel<1, 0, TN>), grid, dim3(256), 0, stream, A);
}

// the bf16 store of one dense conv: rows and reduction length as packed
uint32_t pack_rows(uint32_t cout) { return (cout + kTM - 1) / kTM * kTM; }
uint32_t pack_kpad(uint32_t ktot) { return (ktot + kMK - 1) / kMK * kMK; }
hipError_t launch_pack(hipStream_t stream, const float *w, unsigned short *out, uint32_t cout, uint32_t ktot) {
  const uint32_t rows = pack_rows(cout), kpad = pack_kpad(ktot);
  const size_t total = (size_t)rows * kpad;
  hipLaunchKernelGGL(yolox_pack_bf16_kernel, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, stream, w, out, cout, ktot, rows, kpad);
  return hipGetLastError();
}

// n_cu: the device's compute units. A convolution with fewer than three 64 x 64 tiles for four CUs takes 64 x 16 tiles instead
// (measured, DESIGN 4.14: one frame of YOLOX-s 3.85 -> 2.80 ms; at one or two tiles per CU the batches of 8 lose 5 % and 34 %).
// Every output is the same chain of 16-term steps under either tile, so the choice changes no byte of the result.
// precision BF16 (A.wp set): the dense convolutions take the matrix-core kernel, under the same rule and with the same property (one
// instruction per output and 32-term step under either tile); every other op runs the code it always ran.
hipError_t launch_op(hipStream_t stream, int kind, const ConvArgs &A, uint32_t k, uint32_t n_frames, uint32_t n_cu, int precision) {
  const uint32_t P = A.ho * A.wo;
  if (kind == kOpConv || kind == kOpFocus) {
    const uint64_t wide_blocks = (uint64_t)((P + kTN - 1) / kTN) * ((A.cout + kTM - 1) / kTM) * n_frames;
    const bool narrow = wide_blocks * 4 < 3ull * n_cu;
    if (precision == MI355_YOLOX_PRECISION_BF16) {
      if (!A.wp) return hipErrorInvalidValue;   // no packed weights: never the f32 kernel in their place
      if (narrow) launch_conv_mfma<16>(stream, kind, A, k, n_frames);
      else launch_conv_mfma<64>(stream, kind, A, k, n_frames);
    } else if (narrow) launch_conv<1>(stream, kind, A, k, n_frames);
    else launch_conv<4>(stream, kind, A, k, n_frames);
  } else if (kind == kOpDw) {
    hipLaunchKernelGGL(yolox_dw_kernel, dim3((P + 255) / 256, A.cout, n_frames), dim3(256), 0, stream, A);
  } else if (kind == kOpPool) {
    const size_t total = (size_t)A.cin * A.hi * A.wi;
    hipLaunchKernelGGL(yolox_pool5_kernel, dim3((uint32_t)((total + 255) / 256), 1, n_frames), dim3(256), 0, stream, A.in, A.in_pitch, A.out, A.out_pitch, A.cin, A.hi,
                       A.wi);
  } else {
    const size_t total = (size_t)4 * A.cin * A.hi * A.wi;
    hipLaunchKernelGGL(yolox_up2_kernel, dim3((uint32_t)((total + 255) / 256), 1, n_frames), dim3(256), 0, stream, A.in, A.in_pitch, A.out, A.out_pitch, A.cin, A.hi,
                       A.wi);
  }
  return hipGetLastError();
}

}  // namespace

}  // namespace mi355

using namespace mi355;

// What a forward plans into and writes: the arena of the activations, the input tensor of the compositions, the plan of the last
// shape. A net has one of its own (the lone entry points, on its context's stream); the video group's decoder queue keeps its own,
// one per (net, H, W), and runs them on the queue's stream (YxLanes below) - a forward touches nothing of the net but what
// _finalize froze.
struct YxLane {
  float *d_arena = nullptr, *d_input = nullptr;
  size_t arena_floats = 0, input_floats = 0;
  uint64_t allocations = 0;
  // the plan of the last shape
  uint32_t plan_n = 0, plan_h = 0, plan_w = 0;
  std::vector<size_t> offset;
  size_t plan_floats = 0;
  void release() {
    for (float *p : {d_arena, d_input})
      if (p) (void)hipFree(p);   // waits for the device: a forward still running has finished with them
    d_arena = d_input = nullptr;
    arena_floats = input_floats = 0;
  }
};

struct mi355_yolox_net {
  mi355_ctx *ctx = nullptr;
  uint64_t serial = 0;                    // given at create, never again: what the queue's lanes are keyed on (an address comes back)
  NetDef def;
  std::vector<char> is_set;
  std::vector<float> host_small;          // the host copy of every 1-d parameter (BatchNorm, biases), at host_off
  std::vector<size_t> host_off;
  bool finalized = false;
  float *d_params = nullptr, *d_ss = nullptr;   // the parameter store; scale [channels] then shift [channels]
  int precision = MI355_YOLOX_PRECISION_F32;    // of the dense convolutions' operands; frozen by _finalize
  unsigned short *d_wp = nullptr;               // a BF16 net: every dense conv's packed bf16 weights, conv c at wp_off[c]
  std::vector<size_t> wp_off;
  YxLane lane;                            // the lone entry points'
};

static int param_info_of(const NetDef &N, int index, char *name, size_t name_cap, uint32_t dims[4], int *n_dims) {
  if (index < 0 || (size_t)index >= N.params.size() || !dims || !n_dims) return MI355_ERR_INVALID_ARG;
  const ParamDef &p = N.params[index];
  if (name) {
    if (name_cap < p.name.size() + 1) return MI355_ERR_INVALID_ARG;
    std::memcpy(name, p.name.c_str(), p.name.size() + 1);
  }
  for (int d = 0; d < 4; d++) dims[d] = d < p.nd ? p.dims[d] : 1;
  *n_dims = p.nd;
  return MI355_OK;
}

// the view's first channel in frame 0 and the floats from frame to frame
static float *view_ptr(const NetDef &N, const YxLane &lane, const View &v, uint32_t H, uint32_t W, unsigned long long *pitch) {
  const BufDef &b = N.bufs[v.buf];
  const size_t hw = (size_t)(H / b.ds) * (W / b.ds);
  *pitch = (unsigned long long)b.C * hw;
  return lane.d_arena + lane.offset[v.buf] + (size_t)v.off * hw;
}

// ---- a forward, split from the state it plans into: (net, lane, stream, n_cu). Shapes are checked by the callers.

// the lane's plan for (n, H, W), and an arena that holds it: grows to the largest shape seen (hipFree waits for the device)
static hipError_t lane_plan(const NetDef &N, YxLane *lane, uint32_t n, uint32_t H, uint32_t W) {
  if (lane->plan_n != n || lane->plan_h != H || lane->plan_w != W) {
    plan_arena(N, n, H, W, &lane->offset, &lane->plan_floats);
    lane->plan_n = n, lane->plan_h = H, lane->plan_w = W;
  }
  if (lane->plan_floats > lane->arena_floats) {
    if (lane->d_arena) (void)hipFree(lane->d_arena);
    lane->d_arena = nullptr;
    lane->arena_floats = 0;
    if (const hipError_t e = hipMalloc((void **)&lane->d_arena, lane->plan_floats * 4)) return e;
    lane->arena_floats = lane->plan_floats;
    lane->allocations++;
  }
  return hipSuccess;
}

// the lane's input tensor, for `want` floats
static hipError_t lane_input(YxLane *lane, size_t want) {
  if (want <= lane->input_floats) return hipSuccess;
  if (lane->d_input) (void)hipFree(lane->d_input);
  lane->d_input = nullptr;
  lane->input_floats = 0;
  if (const hipError_t e = hipMalloc((void **)&lane->d_input, want * 4)) return e;
  lane->input_floats = want;
  lane->allocations++;
  return hipSuccess;
}

// the launches of one forward of the planned lane: d_in [n][3][H][W] at in_pitch floats from frame to frame
static hipError_t lane_run(const mi355_yolox_net *net, const YxLane &lane, hipStream_t stream, uint32_t n_cu, const float *d_in, unsigned long long in_pitch, uint32_t n,
                           uint32_t H, uint32_t W) {
  const NetDef &N = net->def;
  for (const OpDef &op : N.ops) {
    ConvArgs A{};
    const BufDef &bi = N.bufs[op.in.buf], &bo = N.bufs[op.out.buf];
    A.hi = H / bi.ds, A.wi = W / bi.ds, A.ho = H / bo.ds, A.wo = W / bo.ds;
    if (op.in.buf == 0) {
      A.in = d_in;
      A.in_pitch = in_pitch;
    } else {
      A.in = view_ptr(N, lane, op.in, H, W, &A.in_pitch);
    }
    A.out = view_ptr(N, lane, op.out, H, W, &A.out_pitch);
    if (op.has_res) A.res = view_ptr(N, lane, op.res, H, W, &A.res_pitch);
    A.cin = op.in.C, A.cout = op.out.C;
    uint32_t k = 0;
    if (op.conv >= 0) {
      const ConvDef &c = N.convs[op.conv];
      A.w = net->d_params + N.params[c.w].off;
      A.scale = net->d_ss + c.ss;
      A.shift = net->d_ss + N.ss_channels + c.ss;
      A.stride = c.stride, A.silu = op.silu ? 1 : 0;
      A.cin = c.cin;
      k = c.k;
      if (net->d_wp && !c.dw) A.wp = net->d_wp + net->wp_off[op.conv], A.kpad = pack_kpad(c.cin * c.k * c.k);
    }
    if (op.kind == kOpFocus) A.hi = A.ho, A.wi = A.wo;   // the gathered [12][H / 2][W / 2] input
    if (const hipError_t e = launch_op(stream, op.kind, A, k, n, n_cu, net->precision)) return e;
  }
  return hipSuccess;
}

// frame 0's maps of the planned lane, and the bytes from frame to frame
static void lane_levels(const NetDef &N, const YxLane &lane, uint32_t H, uint32_t W, mi355_yolox_level levels[3]) {
  for (int l = 0; l < 3; l++) {
    unsigned long long pitch = 0;
    const View all{N.level_buf[l], 0, 5 + N.cfg.num_classes};
    float *p = view_ptr(N, lane, all, H, W, &pitch);
    const size_t hw = (size_t)(H >> (3 + l)) * (W >> (3 + l));
    mi355_yolox_level &lv = levels[l];
    lv.reg = p, lv.obj = p + 4 * hw, lv.cls = p + 5 * hw;
    lv.reg_pitch_bytes = lv.obj_pitch_bytes = lv.cls_pitch_bytes = (size_t)pitch * 4;
    lv.h = H >> (3 + l), lv.w = W >> (3 + l), lv.stride = 8u << l, lv.reserved = 0;
  }
}

// ---- the net as a member of the video group's decoder queue (group.hip, yolodec.hip): what the queue reads of a net,
// the plan of a set's infer members, and the queue's own lanes
namespace mi355 {

void yolox_net_info(const mi355_yolox_net *net, YxNetInfo *out) {
  out->serial = net->serial;
  out->device = net->ctx->device;
  out->finalized = net->finalized;
  out->num_classes = net->def.cfg.num_classes;
  out->launches = (int)net->def.ops.size();
}

int yolox_net_check_size(uint32_t H, uint32_t W, const char **why) { return check_size(H, W, why); }

// the one place a set's infer members become classes, frames of a class and conversion blocks
int yolox_infer_set_plan(int n_jobs, const int *kind, const uint64_t *net_key, const uint32_t *height, const uint32_t *width, int32_t *class_of,
                         uint32_t *frame_in_class, uint32_t *conv_first_block, uint32_t *conv_blocks, uint32_t *class_frames, uint64_t totals[3]) {
  if (n_jobs < 0 || n_jobs > kYdSetMax || !totals) return MI355_ERR_INVALID_ARG;
  if (n_jobs > 0 && (!kind || !net_key || !height || !width || !class_of || !frame_in_class || !conv_first_block || !conv_blocks || !class_frames))
    return MI355_ERR_INVALID_ARG;
  for (int j = 0; j < n_jobs; j++) {
    if (kind[j] < MI355_YOLO_V8 || kind[j] > MI355_YOLO_X_INFER) return MI355_ERR_INVALID_ARG;
    const char *why = nullptr;
    if (kind[j] == MI355_YOLO_X_INFER)
      if (const int rc = check_size(height[j], width[j], &why)) return rc;
  }
  int first_of[kYdSetMax];   // the first job of each class
  uint32_t classes = 0, frames = 0, blocks = 0;
  for (int j = 0; j < n_jobs; j++) {
    conv_first_block[j] = blocks;
    if (kind[j] != MI355_YOLO_X_INFER) {
      class_of[j] = -1;
      frame_in_class[j] = 0;
      conv_blocks[j] = 0;
      continue;
    }
    uint32_t c = 0;
    while (c < classes && !(net_key[first_of[c]] == net_key[j] && height[first_of[c]] == height[j] && width[first_of[c]] == width[j])) c++;
    if (c == classes) {
      first_of[classes++] = j;
      class_frames[c] = 0;
    }
    class_of[j] = (int32_t)c;
    frame_in_class[j] = class_frames[c]++;
    conv_blocks[j] = (uint32_t)(((uint64_t)(width[j] / 4) * height[j] + 255) / 256);   // one lane takes 4 pixels; <= 4096 blocks a frame
    blocks += conv_blocks[j];
    frames++;
  }
  totals[0] = classes, totals[1] = frames, totals[2] = blocks;
  return MI355_OK;
}

// The queue's lanes: one per class key (net serial, H, W), never per net - the head launches of a set run after ALL of its forwards,
// so two classes of one net in a set would overwrite each other's level buffers in a shared lane.
struct YxLaneKey {
  uint64_t serial;
  uint32_t H, W;
  bool operator<(const YxLaneKey &o) const { return serial != o.serial ? serial < o.serial : H != o.H ? H < o.H : W < o.W; }
};
struct YxLanes {
  std::map<YxLaneKey, YxLane> lanes;
  uint64_t allocations = 0;   // made for lanes since the store exists, released lanes' included
};

YxLanes *yolox_lanes_new() { return new YxLanes(); }

void yolox_lanes_free(YxLanes *S) {
  if (!S) return;
  for (auto &kv : S->lanes) kv.second.release();
  delete S;
}

void yolox_lanes_stats(const YxLanes *S, uint64_t *alive, uint64_t *allocations) {
  *alive = S ? (uint64_t)S->lanes.size() : 0;
  *allocations = S ? S->allocations : 0;
}

int yolox_lanes_release(YxLanes *S, uint64_t serial) {
  int n = 0;
  for (auto it = S->lanes.begin(); it != S->lanes.end();) {
    if (it->first.serial != serial) { ++it; continue; }
    it->second.release();
    it = S->lanes.erase(it);
    n++;
  }
  return n;
}

int yolox_lanes_prepare(YxLanes *S, const mi355_yolox_net *net, uint32_t n_frames, uint32_t H, uint32_t W, float **d_input, mi355_yolox_level levels[3],
                        std::string *err) {
  const char *why = nullptr;
  int rc = MI355_OK;
  if (!S || !net || !net->finalized) { *err = "yolox_net: no lanes, or a net that is not finalized"; return MI355_ERR_INVALID_ARG; }
  if ((rc = check_frames((int)n_frames, &why)) || (rc = check_size(H, W, &why))) { *err = why; return rc; }
  YxLane &lane = S->lanes[YxLaneKey{net->serial, H, W}];
  const uint64_t before = lane.allocations;
  hipError_t e = lane_input(&lane, (size_t)3 * H * W * n_frames);
  if (e == hipSuccess) e = lane_plan(net->def, &lane, n_frames, H, W);
  S->allocations += lane.allocations - before;
  if (e != hipSuccess) {
    (void)hipGetLastError();
    *err = "hipMalloc(yolox_net lane)";
    return MI355_ERR_OUT_OF_MEMORY;
  }
  *d_input = lane.d_input;
  lane_levels(net->def, lane, H, W, levels);
  return MI355_OK;
}

int yolox_lanes_forward(YxLanes *S, const mi355_yolox_net *net, uint32_t n_frames, uint32_t H, uint32_t W, hipStream_t stream, int n_cu, int *kernel_launches,
                        std::string *err) {
  auto it = S->lanes.find(YxLaneKey{net->serial, H, W});
  if (it == S->lanes.end() || it->second.plan_n != n_frames || it->second.plan_h != H || it->second.plan_w != W) {
    *err = "yolox_net: a forward of a lane that is not prepared for it";
    return MI355_ERR_INVALID_ARG;
  }
  const YxLane &lane = it->second;
  const hipError_t e = lane_run(net, lane, stream, (uint32_t)n_cu, lane.d_input, (unsigned long long)3 * H * W, n_frames, H, W);
  if (e != hipSuccess) { *err = std::string("yolox_net lane launch: ") + hipGetErrorString(e); return MI355_ERR_HIP; }
  *kernel_launches += (int)net->def.ops.size();
  return MI355_OK;
}

}  // namespace mi355

extern "C" {

int mi355_selftest_yolox_infer_set_plan(int n_jobs, const int *kind, const uint64_t *net_key, const uint32_t *height, const uint32_t *width, int32_t *class_of,
                                        uint32_t *frame_in_class, uint32_t *conv_first_block, uint32_t *conv_blocks, uint32_t *class_frames, uint64_t totals[3]) {
  return yolox_infer_set_plan(n_jobs, kind, net_key, height, width, class_of, frame_in_class, conv_first_block, conv_blocks, class_frames, totals);
}

int mi355_yolox_net_create(mi355_ctx *ctx, const mi355_yolox_net_config *config, mi355_yolox_net **net_out) {
  if (!ctx) return MI355_ERR_INVALID_ARG;
  if (!net_out) return set_error(ctx, MI355_ERR_INVALID_ARG, "yolox_net: null result pointer");
  *net_out = nullptr;
  const char *why = nullptr;
  int rc = check_config(config, &why);
  if (rc) return set_error(ctx, rc, why);
  std::unique_ptr<mi355_yolox_net> net(new mi355_yolox_net);
  net->ctx = ctx;
  static std::atomic<uint64_t> next_serial{1};
  net->serial = next_serial.fetch_add(1);
  if (!build_def(*config, &net->def)) return set_error(ctx, MI355_ERR_UNSUPPORTED, "yolox_net: the config's channel counts do not fit the model");
  const NetDef &N = net->def;
  net->is_set.assign(N.params.size(), 0);
  net->host_off.assign(N.params.size(), 0);
  size_t small = 0;
  for (size_t i = 0; i < N.params.size(); i++)
    if (N.params[i].nd == 1) {
      net->host_off[i] = small;
      small += N.params[i].n;
    }
  net->host_small.assign(small, 0.0f);
  if ((rc = check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice"))) return rc;
  if ((rc = check_hip(ctx, hipMalloc((void **)&net->d_params, N.param_floats * 4), "hipMalloc(yolox_net parameters)"))) return rc;
  if ((rc = check_hip(ctx, hipMalloc((void **)&net->d_ss, N.ss_channels * 2 * 4), "hipMalloc(yolox_net epilogue)"))) {
    (void)hipFree(net->d_params);
    return rc;
  }
  *net_out = net.release();
  return MI355_OK;
}

void mi355_yolox_net_destroy(mi355_yolox_net *net) {
  if (!net) return;
  if (net->ctx) (void)hipSetDevice(net->ctx->device);
  for (void *p : {(void *)net->d_params, (void *)net->d_ss, (void *)net->d_wp})
    if (p) (void)hipFree(p);   // waits for the device: a forward still running has finished with them
  net->lane.release();
  delete net;
}

int mi355_yolox_net_param_count(const mi355_yolox_net *net) { return net ? (int)net->def.params.size() : MI355_ERR_INVALID_ARG; }

int mi355_yolox_net_param_info(const mi355_yolox_net *net, int index, char *name, size_t name_cap, uint32_t dims[4], int *n_dims) {
  if (!net) return MI355_ERR_INVALID_ARG;
  const int rc = param_info_of(net->def, index, name, name_cap, dims, n_dims);
  return rc ? set_error(net->ctx, rc, "yolox_net: bad parameter index, null result or name buffer too small") : rc;
}

int mi355_yolox_net_set_param(mi355_yolox_net *net, int index, const float *host, size_t n) {
  if (!net) return MI355_ERR_INVALID_ARG;
  mi355_ctx *ctx = net->ctx;
  if (net->finalized) return set_error(ctx, MI355_ERR_INVALID_ARG, "yolox_net: the net is finalized and immutable");
  if (index < 0 || (size_t)index >= net->def.params.size() || !host) return set_error(ctx, MI355_ERR_INVALID_ARG, "yolox_net: bad parameter index or null data");
  const ParamDef &p = net->def.params[index];
  if (n != p.n) return set_error(ctx, MI355_ERR_INVALID_ARG, "yolox_net: wrong element count for " + p.name);
  int rc = MI355_OK;
  if ((rc = check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice"))) return rc;
  if ((rc = check_hip(ctx, hipMemcpy(net->d_params + p.off, host, n * 4, hipMemcpyHostToDevice), "yolox_net parameter H2D"))) return rc;
  __atomic_fetch_add(&ctx->n_h2d, 1ull, __ATOMIC_RELAXED);
  if (p.nd == 1) std::memcpy(net->host_small.data() + net->host_off[index], host, n * 4);
  net->is_set[index] = 1;
  return MI355_OK;
}

int mi355_yolox_net_finalize(mi355_yolox_net *net) {
  if (!net) return MI355_ERR_INVALID_ARG;
  mi355_ctx *ctx = net->ctx;
  if (net->finalized) return MI355_OK;
  const NetDef &N = net->def;
  for (size_t i = 0; i < N.params.size(); i++)
    if (!net->is_set[i]) return set_error(ctx, MI355_ERR_INVALID_ARG, "yolox_net: parameter not set: " + N.params[i].name);
  std::vector<float> ss(N.ss_channels * 2);
  float *scale = ss.data(), *shift = ss.data() + N.ss_channels;
  auto small = [&](int param) { return net->host_small.data() + net->host_off[param]; };
  for (const ConvDef &c : N.convs)
    for (uint32_t ch = 0; ch < c.cout; ch++) {
      if (c.bias >= 0) {
        scale[c.ss + ch] = 1.0f;
        shift[c.ss + ch] = small(c.bias)[ch];
      } else {   // BatchNorm, eps 1e-3 (blocks.rs:114): f64, rounded once
        const double s = (double)small(c.g)[ch] / std::sqrt((double)small(c.v)[ch] + 1e-3);
        scale[c.ss + ch] = (float)s;
        shift[c.ss + ch] = (float)((double)small(c.b)[ch] - (double)small(c.m)[ch] * s);
      }
    }
  int rc = MI355_OK;
  if ((rc = check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice"))) return rc;
  if ((rc = check_hip(ctx, hipMemcpy(net->d_ss, ss.data(), ss.size() * 4, hipMemcpyHostToDevice), "yolox_net epilogue H2D"))) return rc;
  __atomic_fetch_add(&ctx->n_h2d, 1ull, __ATOMIC_RELAXED);
  if (net->precision == MI355_YOLOX_PRECISION_BF16) {   // the dense convolutions' weights, rounded once, on the device (the host keeps none)
    net->wp_off.assign(N.convs.size(), 0);
    size_t total = 0;
    for (size_t c = 0; c < N.convs.size(); c++) {
      if (N.convs[c].dw) continue;
      net->wp_off[c] = total;
      total += (size_t)pack_rows(N.convs[c].cout) * pack_kpad(N.convs[c].cin * N.convs[c].k * N.convs[c].k);
    }
    if ((rc = check_hip(ctx, hipMalloc((void **)&net->d_wp, total * 2), "hipMalloc(yolox_net bf16 weights)"))) return rc;
    hipError_t e = hipSuccess;
    for (size_t c = 0; c < N.convs.size() && e == hipSuccess; c++) {
      const ConvDef &cd = N.convs[c];
      if (!cd.dw) e = launch_pack(ctx->stream, net->d_params + N.params[cd.w].off, net->d_wp + net->wp_off[c], cd.cout, cd.cin * cd.k * cd.k);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
      (void)hipFree(net->d_wp);
      net->d_wp = nullptr;
      return check_hip(ctx, e, "yolox_net bf16 weight packing");
    }
  }
  net->finalized = true;
  return MI355_OK;
}

int mi355_yolox_net_set_precision(mi355_yolox_net *net, int precision) {
  if (!net) return MI355_ERR_INVALID_ARG;
  if (net->finalized) return set_error(net->ctx, MI355_ERR_INVALID_ARG, "yolox_net: the net is finalized and immutable");
  if (precision != MI355_YOLOX_PRECISION_F32 && precision != MI355_YOLOX_PRECISION_BF16)
    return set_error(net->ctx, MI355_ERR_INVALID_ARG, "yolox_net: precision is neither MI355_YOLOX_PRECISION_F32 nor _BF16");
  net->precision = precision;
  return MI355_OK;
}

int mi355_yolox_net_precision(const mi355_yolox_net *net) { return net ? net->precision : MI355_ERR_INVALID_ARG; }

int mi355_yolox_net_forward_device(mi355_yolox_net *net, const float *d_in, size_t in_pitch_bytes, int n_frames, uint32_t H, uint32_t W,
                                   mi355_yolox_level levels[3]) {
  if (!net) return MI355_ERR_INVALID_ARG;
  mi355_ctx *ctx = net->ctx;
  const char *why = nullptr;
  int rc = MI355_OK;
  if ((rc = check_frames(n_frames, &why)) || (rc = check_size(H, W, &why))) return set_error(ctx, rc, why);
  if (!net->finalized) return set_error(ctx, MI355_ERR_NOT_CONFIGURED, "yolox_net: forward before finalize");
  if (!d_in || (uintptr_t)d_in % 4 != 0 || !levels) return set_error(ctx, MI355_ERR_INVALID_ARG, "yolox_net: null or misaligned input, or null levels");
  if (in_pitch_bytes % 4 != 0 || (n_frames > 1 && in_pitch_bytes < (size_t)3 * H * W * 4))
    return set_error(ctx, MI355_ERR_INVALID_ARG, "yolox_net: input pitch is smaller than the tensor or no multiple of 4");
  if ((rc = check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice"))) return rc;
  const uint32_t n = (uint32_t)n_frames;
  if ((rc = check_hip(ctx, lane_plan(net->def, &net->lane, n, H, W), "hipMalloc(yolox_net arena)"))) return rc;
  if ((rc = check_hip(ctx, lane_run(net, net->lane, ctx->stream, (uint32_t)ctx->n_cu, d_in, in_pitch_bytes / 4, n, H, W), "yolox_net launch"))) return rc;
  lane_levels(net->def, net->lane, H, W, levels);
  return MI355_OK;
}

int mi355_yolox_net_launches(const mi355_yolox_net *net) { return net ? (int)net->def.ops.size() : MI355_ERR_INVALID_ARG; }

int mi355_yolox_net_arena_info(const mi355_yolox_net *net, uint64_t *arena_bytes, uint64_t *allocations) {
  if (!net) return MI355_ERR_INVALID_ARG;
  if (arena_bytes) *arena_bytes = (uint64_t)net->lane.arena_floats * 4;
  if (allocations) *allocations = net->lane.allocations;
  return MI355_OK;
}

// the compositions' first two steps: frames -> the net's input tensor -> levels
static int infer_levels(mi355_yolox_net *net, const uint8_t *d_frames, size_t frame_pitch, size_t stride, int n_frames, uint32_t width, uint32_t height,
                        mi355_yolox_level levels[3]) {
  mi355_ctx *ctx = net->ctx;
  const char *why = nullptr;
  int rc = MI355_OK;
  if ((rc = check_frames(n_frames, &why)) || (rc = check_size(height, width, &why))) return set_error(ctx, rc, why);
  if (!net->finalized) return set_error(ctx, MI355_ERR_NOT_CONFIGURED, "yolox_net: inference before finalize");
  if ((rc = check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice"))) return rc;
  const size_t frame_floats = (size_t)3 * width * height, want = frame_floats * (size_t)n_frames;
  if ((rc = check_hip(ctx, lane_input(&net->lane, want), "hipMalloc(yolox_net input)"))) return rc;
  if ((rc = mi355_yolox_input_frames_device(ctx, d_frames, frame_pitch, stride, n_frames, width, height, net->lane.d_input, frame_floats * 4))) return rc;
  return mi355_yolox_net_forward_device(net, net->lane.d_input, frame_floats * 4, n_frames, height, width, levels);
}

int mi355_yolox_infer_frames_device(mi355_yolox_net *net, const uint8_t *d_frames, size_t frame_pitch, size_t stride, int n_frames, uint32_t width,
                                    uint32_t height, float *d_out, size_t out_pitch_bytes) {
  if (!net) return MI355_ERR_INVALID_ARG;
  mi355_yolox_level levels[3];
  if (const int rc = infer_levels(net, d_frames, frame_pitch, stride, n_frames, width, height, levels)) return rc;
  return mi355_yolox_head_decode_device(net->ctx, levels, 3, n_frames, net->def.cfg.num_classes, d_out, out_pitch_bytes);
}

int mi355_yolox_infer_dets_device(mi355_yolox_net *net, const uint8_t *d_frames, size_t frame_pitch, size_t stride, int n_frames, uint32_t width,
                                  uint32_t height, const mi355_yolo_params *p, mi355_yolo_det *dets, uint32_t max_dets, uint32_t *n_dets) {
  if (!net) return MI355_ERR_INVALID_ARG;
  mi355_yolox_level levels[3];
  if (const int rc = infer_levels(net, d_frames, frame_pitch, stride, n_frames, width, height, levels)) return rc;
  return mi355_yolox_head_dets_device(net->ctx, levels, 3, n_frames, net->def.cfg.num_classes, p, dets, max_dets, n_dets);
}

int mi355_selftest_yolox_net_plan(const mi355_yolox_net_config *config, int n_frames, uint32_t H, uint32_t W, mi355_yolox_net_plan *plan) {
  if (!plan) return MI355_ERR_INVALID_ARG;
  std::memset(plan, 0, sizeof(*plan));
  const char *why = nullptr;
  plan->config_status = check_config(config, &why);
  plan->frames_status = check_frames(n_frames, &why);
  plan->size_status = check_size(H, W, &why);
  plan->status = plan->config_status ? plan->config_status : plan->frames_status ? plan->frames_status : plan->size_status;
  if (plan->config_status) return plan->status;
  NetDef N;
  if (!build_def(*config, &N)) return plan->status = plan->config_status = MI355_ERR_UNSUPPORTED;
  plan->param_count = (uint32_t)N.params.size();
  plan->param_floats = N.param_floats;
  plan->launches = (uint32_t)N.ops.size();
  if (plan->status) return plan->status;
  std::vector<size_t> offset;
  size_t floats = 0;
  plan_arena(N, (uint32_t)n_frames, H, W, &offset, &floats);
  plan->arena_bytes = (uint64_t)floats * 4;
  plan->macs = count_macs(N, (uint32_t)n_frames, H, W);
  for (int l = 0; l < 3; l++) plan->level_h[l] = H >> (3 + l), plan->level_w[l] = W >> (3 + l);
  return MI355_OK;
}

int mi355_selftest_yolox_net_param_info(const mi355_yolox_net_config *config, int index, char *name, size_t name_cap, uint32_t dims[4], int *n_dims) {
  const char *why = nullptr;
  if (const int rc = check_config(config, &why)) return rc;
  // the table of the last config asked about: an enumeration walks one config from 0 up
  static thread_local NetDef cached;
  static thread_local bool have = false;
  const mi355_yolox_net_config &cc = cached.cfg;
  if (!have || cc.depth != config->depth || cc.width != config->width || cc.depthwise != config->depthwise || cc.num_classes != config->num_classes) {
    cached = NetDef();
    have = build_def(*config, &cached);
    if (!have) return MI355_ERR_UNSUPPORTED;
  }
  return param_info_of(cached, index, name, name_cap, dims, n_dims);
}

// the checks of the one-op entries and the launch arguments of a checked op
static int selftest_op_args(mi355_ctx *ctx, const mi355_yolox_net_op *op, ConvArgs *args, uint32_t *k_out) {
  if (!ctx) return MI355_ERR_INVALID_ARG;
  if (!op || !op->in || !op->out || (op->tile != 0 && op->tile != 1 && op->tile != 4)) return set_error(ctx, MI355_ERR_INVALID_ARG, "yolox_net op: null op or views, or a tile that is not 0, 1 or 4");
  const int kind = op->kind;
  const bool is_conv = kind == kOpConv || kind == kOpDw || kind == kOpFocus;
  if (kind < kOpConv || kind > kOpFocus || op->n_frames < 1 || op->n_frames > MI355_YOLOX_NET_MAX_FRAMES || op->h_in < 1 || op->w_in < 1 ||
      op->h_in > MI355_YOLOX_NET_MAX_SIDE || op->w_in > MI355_YOLOX_NET_MAX_SIDE || op->in_c < 1 || op->out_c < 1 || op->in_off + op->in_c > op->in_ctot ||
      op->out_off + op->out_c > op->out_ctot || (op->res && op->res_off + op->out_c > op->res_ctot))
    return set_error(ctx, MI355_ERR_INVALID_ARG, "yolox_net op: bad kind, shape or view");
  if (is_conv && (!op->weight || !op->scale || !op->shift || (op->stride != 1 && op->stride != 2))) return set_error(ctx, MI355_ERR_INVALID_ARG, "yolox_net op: bad conv");
  if (kind == kOpConv && op->k != 1 && op->k != 3) return set_error(ctx, MI355_ERR_INVALID_ARG, "yolox_net op: k is 1 or 3");
  if ((kind == kOpDw || kind == kOpPool || kind == kOpUp) && op->in_c != op->out_c) return set_error(ctx, MI355_ERR_INVALID_ARG, "yolox_net op: channel counts differ");
  if (kind == kOpFocus && (op->in_c != 3 || op->stride != 1 || op->in_off != 0 || op->in_ctot != 3)) return set_error(ctx, MI355_ERR_INVALID_ARG, "yolox_net op: bad focus");
  if (!is_conv && op->res) return set_error(ctx, MI355_ERR_INVALID_ARG, "yolox_net op: a residual needs a convolution");
  int rc = MI355_OK;
  if ((rc = check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice"))) return rc;
  ConvArgs &A = *args;
  A = ConvArgs{};
  const uint32_t k = kind == kOpConv ? (uint32_t)op->k : 3, stride = is_conv ? (uint32_t)op->stride : 1, padk = (k - 1) / 2;
  A.hi = op->h_in, A.wi = op->w_in;
  if (kind == kOpUp) A.ho = 2 * A.hi, A.wo = 2 * A.wi;
  else if (kind == kOpPool) A.ho = A.hi, A.wo = A.wi;
  else A.ho = (A.hi + 2 * padk - k) / stride + 1, A.wo = (A.wi + 2 * padk - k) / stride + 1;
  const size_t in_hw = kind == kOpFocus ? (size_t)4 * A.hi * A.wi : (size_t)A.hi * A.wi, out_hw = (size_t)A.ho * A.wo;
  A.in = op->in + (size_t)op->in_off * in_hw;
  A.in_pitch = (unsigned long long)op->in_ctot * in_hw;
  A.out = op->out + (size_t)op->out_off * out_hw;
  A.out_pitch = (unsigned long long)op->out_ctot * out_hw;
  if (op->res) {
    A.res = op->res + (size_t)op->res_off * out_hw;
    A.res_pitch = (unsigned long long)op->res_ctot * out_hw;
  }
  A.w = op->weight, A.scale = op->scale, A.shift = op->shift;
  A.cin = kind == kOpFocus ? 12 : op->in_c, A.cout = op->out_c, A.stride = stride, A.silu = op->silu ? 1 : 0;
  *k_out = k;
  return MI355_OK;
}

// the n_cu that makes launch_op take the tile an op names
static uint32_t selftest_op_cu(const mi355_ctx *ctx, const mi355_yolox_net_op *op) { return op->tile == 4 ? 0u : op->tile == 1 ? UINT32_MAX / 2 : (uint32_t)ctx->n_cu; }

int mi355_selftest_yolox_net_op_device(mi355_ctx *ctx, const mi355_yolox_net_op *op) {
  ConvArgs A{};
  uint32_t k = 0;
  if (const int rc = selftest_op_args(ctx, op, &A, &k)) return rc;
  return check_hip(ctx, launch_op(ctx->stream, op->kind, A, k, op->n_frames, selftest_op_cu(ctx, op), MI355_YOLOX_PRECISION_F32), "yolox_net op launch");
}

int mi355_selftest_yolox_net_op_bf16_device(mi355_ctx *ctx, const mi355_yolox_net_op *op) {
  ConvArgs A{};
  uint32_t k = 0;
  if (const int rc = selftest_op_args(ctx, op, &A, &k)) return rc;
  if (op->kind != kOpConv && op->kind != kOpFocus) return set_error(ctx, MI355_ERR_INVALID_ARG, "yolox_net bf16 op: the kind is neither a dense conv nor the Focus stem");
  const uint32_t ktot = A.cin * k * k;
  unsigned short *d_wp = nullptr;
  int rc = MI355_OK;
  if ((rc = check_hip(ctx, hipMalloc((void **)&d_wp, (size_t)pack_rows(A.cout) * pack_kpad(ktot) * 2), "hipMalloc(yolox_net op bf16 weights)"))) return rc;
  hipError_t e = launch_pack(ctx->stream, A.w, d_wp, A.cout, ktot);   // what _finalize runs per conv
  A.wp = d_wp, A.kpad = pack_kpad(ktot);
  if (e == hipSuccess) e = launch_op(ctx->stream, op->kind, A, k, op->n_frames, selftest_op_cu(ctx, op), MI355_YOLOX_PRECISION_BF16);
  const hipError_t es = hipStreamSynchronize(ctx->stream);   // the packed copy is this call's
  (void)hipFree(d_wp);
  return check_hip(ctx, e != hipSuccess ? e : es, "yolox_net bf16 op");
}

}  // extern "C"
