// hrtf_kernels.hip — gfx950 kernels for hrtfrender (BASELINE config 4).
//
// Reference path replaced: HrtfRender::process (audio/hrtf/src/hrtf/imp.rs:164-278), which per block of
// block_length*interpolation_steps frames and per input channel calls the third-party crate
// hrtf 0.8.1 `HrtfProcessor::process_samples` (sources not in the reference tree; algorithm restated in
// oracle/hrtf_oracle.c) and sums every channel's (left, right) into the stereo output (imp.rs:256-268).
//
// What the crate computes per channel and interpolation step is a streaming linear convolution of the source
// with a barycentric blend of three HRIRs of the sphere-mesh face the (interpolated) source direction points at,
// scaled by the interpolated distance gain. The crate evaluates it with an FFT overlap-save of size
// block_length + hrir_len - 1; by linearity of the DFT the blend of spectra is the spectrum of the blended
// HRIRs, so the same value is produced here in the time domain (tolerance parity):
//   hrtf_prepare_kernel : per channel — direction/gain interpolation, ray/mesh search (first face in file order,
//                         same f32 operation order as the crate), tap blend per step, input de-interleave with
//                         the previous block's tail in front (the crate's prev_left/right_samples are both the
//                         raw input tail)
//   hrtf_fir_kernel     : per (step, tile, channel) — direct-form FIR from LDS tiles of the input and both ears' taps
//   hrtf_fft_kernel     : the same convolution as ONE overlap-save FFT per (step, channel) in LDS, the form BASELINE config 4
//                         names and the crate uses (round 3): window [L-1 history | B samples] zero-padded to N = 2^k,
//                         X = FFT(x), Z = FFT(h_left + i h_right), y = IFFT(X Z): x is real, so Re y is the left ear and
//                         Im y the right one - three radix-2 transforms in LDS per step and channel instead of 2 B L MACs.
//                         Serves whenever N <= 4096 fits the LDS (HRIRs up to ~3.5 k taps at the default block of 512);
//                         the FIR stays for what does not (and can be pinned with MI355_FLAG_HRTF_METHOD).
//   hrtf_mix_kernel     : channel-ordered sum into the interleaved stereo output (imp.rs:256-268 order)
// HBM traffic per block is ~C*(frames+taps)*4 B in and frames*8 B out; the FIR is LDS-bound (1 LDS read per MAC).
#include "internal.hpp"

#include <cmath>
#include <cstring>
#include <vector>

namespace mi355 {

struct HrtfState {
  // sphere (HrirSphere, crate file format)
  uint32_t rate = 0, len = 0, n_vertices = 0, n_faces = 0;
  float *d_pos = nullptr;      // [V][3]
  uint32_t *d_idx = nullptr;   // [F][3]
  float *d_hrir = nullptr;     // [V][2][len]
  bool sphere_loaded = false;
  // processors (HrtfProcessor::new per channel, imp.rs:662-680)
  int channels = 0, steps = 0, block_len = 0;
  bool configured = false;
  float *d_x[2] = {nullptr, nullptr};  // ping-pong [C][pad + frames]: history + de-interleaved block
  int cur = 0;
  int fft_n = 0, fft_log = 0;    // overlap-save transform size (0: the time-domain FIR serves)
  float *d_taps = nullptr;       // [C][S][2][len]
  float *d_last_taps = nullptr;  // [C][2][len] taps of the last successful mesh lookup
  float *d_gain = nullptr;       // [C][S]
  int *d_face = nullptr;         // [C][S] face index or -1 (diagnostics/tests)
  float *d_uvw = nullptr;        // [C][S][3]
  float *d_partial = nullptr;    // [C][frames][2]
  float *d_in = nullptr, *d_out = nullptr;  // staging for the host entry point
  std::vector<float> prev_vec, prev_gain;
  std::vector<unsigned char> have_prev;
};

static HrtfState *hrtf_of(mi355_ctx *ctx) { return (HrtfState *)ctx->hrtf; }

struct V3 { float x, y, z; };
__device__ __forceinline__ V3 v_sub(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 v_scale(V3 a, float s) { return V3{a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ float v_dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 v_cross(V3 a, V3 b) { return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ float lerpf(float a, float b, float t) { return a + (b - a) * t; }

// ray origin -> dir against one face; same operation order as the crate's ray_triangle_intersection +
// get_barycentric_coords (IEEE sqrt/div, no contraction)
__device__ __forceinline__ bool ray_face(V3 dir, V3 a, V3 b, V3 c, float &u, float &v, float &w) {
  const V3 ba = v_sub(b, a), ca = v_sub(c, a);
  V3 n = v_cross(ba, ca);
  const float l = sqrtf(v_dot(n, n));
  n = V3{n.x / l, n.y / l, n.z / l};
  const float d = -v_dot(a, n);
  const float num = -(0.0f + d);  // origin . normal == 0
  const float den = v_dot(dir, n);
  const float t = num / den;
  if (!(t > 0.0f && t < 1.0f)) return false;
  const V3 p = V3{0.0f + dir.x * t, 0.0f + dir.y * t, 0.0f + dir.z * t};
  const V3 v2 = v_sub(p, a);
  const float d00 = v_dot(ba, ba), d01 = v_dot(ba, ca), d11 = v_dot(ca, ca), d20 = v_dot(v2, ba), d21 = v_dot(v2, ca);
  const float denom = d00 * d11 - d01 * d01;
  const float bv = (d11 * d20 - d01 * d21) / denom;
  const float bw = (d00 * d21 - d01 * d20) / denom;
  const float bu = 1.0f - bv - bw;
  const float eps = 1.1920929e-7f;
  if (!(bu >= -eps && bv >= -eps && bu + bv <= 1.0f + eps)) return false;
  u = bu; v = bv; w = bw;
  return true;
}

// previous / new direction and gain of every channel, passed by value in the kernel arguments (<= 64 channels: 2 KiB)
struct HrtfVecGain { float v[8 * 64]; };  // prev_vec[C][3], new_vec[C][3], prev_gain[C], new_gain[C] with C = channels

// One block per channel.
__global__ __launch_bounds__(256) void hrtf_prepare_kernel(const float *__restrict__ in, int C, int S, int B, int L,
                                                           const float *__restrict__ pos, const uint32_t *__restrict__ idx, int F,
                                                           const float *__restrict__ hrir, HrtfVecGain VG,
                                                           const float *__restrict__ x_old, float *__restrict__ x_new,
                                                           float *__restrict__ taps, float *__restrict__ last_taps,
                                                           float *__restrict__ gain, int *__restrict__ face_out, float *__restrict__ uvw_out) {
  const int c = blockIdx.x;
  const int frames = S * B, pad = L - 1;
  const float pv[3] = {VG.v[3 * c], VG.v[3 * c + 1], VG.v[3 * c + 2]};
  const float nv[3] = {VG.v[3 * C + 3 * c], VG.v[3 * C + 3 * c + 1], VG.v[3 * C + 3 * c + 2]};
  const float pg = VG.v[6 * C + c], ng = VG.v[7 * C + c];
  __shared__ int s_face[64];
  __shared__ float s_uvw[64][3];
  // ---- mesh lookup: one wave-sized group of lanes per step scans the faces in file order; the FIRST hit wins
  for (int s = threadIdx.x / 64; s < S; s += blockDim.x / 64) {
    const int lane = threadIdx.x & 63;
    const float t = (float)(s + 1) / (float)S;
    const V3 dir = v_scale(V3{lerpf(pv[0], nv[0], t), lerpf(pv[1], nv[1], t), lerpf(pv[2], nv[2], t)}, 10.0f);
    int best = 0x7fffffff;
    float bu = 0, bv = 0, bw = 0;
    for (int f0 = 0; f0 < F && best == 0x7fffffff; f0 += 64) {
      const int f = f0 + lane;
      bool hit = false;
      float u = 0, v = 0, w = 0;
      if (f < F) {
        const uint32_t i0 = idx[3 * f], i1 = idx[3 * f + 1], i2 = idx[3 * f + 2];
        hit = ray_face(dir, V3{pos[3 * i0], pos[3 * i0 + 1], pos[3 * i0 + 2]}, V3{pos[3 * i1], pos[3 * i1 + 1], pos[3 * i1 + 2]},
                       V3{pos[3 * i2], pos[3 * i2 + 1], pos[3 * i2 + 2]}, u, v, w);
      }
      const unsigned long long m = __ballot(hit);
      if (m) {
        const int first = __ffsll((long long)m) - 1;
        best = f0 + first;
        bu = __shfl(u, first); bv = __shfl(v, first); bw = __shfl(w, first);
      }
    }
    if (lane == 0) {
      const int fidx = best == 0x7fffffff ? -1 : best;
      if (s < 64) { s_face[s] = fidx; s_uvw[s][0] = bu; s_uvw[s][1] = bv; s_uvw[s][2] = bw; }
      face_out[c * S + s] = fidx;
      uvw_out[(c * S + s) * 3 + 0] = bu; uvw_out[(c * S + s) * 3 + 1] = bv; uvw_out[(c * S + s) * 3 + 2] = bw;
      gain[c * S + s] = lerpf(pg, ng, t);
    }
  }
  __syncthreads();
  // ---- taps per step; a step without a hit keeps the previous taps (crate: left_hrtf/right_hrtf untouched)
  for (int e_k = threadIdx.x; e_k < 2 * L; e_k += blockDim.x) {
    const int e = e_k / L, k = e_k - e * L;
    float prev = last_taps[((size_t)c * 2 + e) * L + k];
    for (int s = 0; s < S; s++) {
      const int f = s_face[s];
      if (f >= 0) {
        const float a = hrir[((size_t)idx[3 * f] * 2 + e) * L + k];
        const float b = hrir[((size_t)idx[3 * f + 1] * 2 + e) * L + k];
        const float cc = hrir[((size_t)idx[3 * f + 2] * 2 + e) * L + k];
        prev = a * s_uvw[s][0] + b * s_uvw[s][1] + cc * s_uvw[s][2];
      }
      taps[(((size_t)c * S + s) * 2 + e) * L + k] = prev;
    }
    last_taps[((size_t)c * 2 + e) * L + k] = prev;
  }
  // ---- input row: previous tail, then this block's samples of channel c
  const size_t row = (size_t)pad + frames;
  for (int k = threadIdx.x; k < pad; k += blockDim.x) x_new[c * row + k] = x_old[c * row + frames + k];
  for (int i = threadIdx.x; i < frames; i += blockDim.x) x_new[c * row + pad + i] = in[(size_t)i * C + c];
}

// grid (S * tiles, C); block 256; dynamic LDS: [T + pad] input + [2][L] taps
__global__ __launch_bounds__(256) void hrtf_fir_kernel(const float *__restrict__ x, const float *__restrict__ taps,
                                                       const float *__restrict__ gain, float *__restrict__ partial, int S, int B,
                                                       int L, int T, int tiles) {
  extern __shared__ float sm[];
  const int c = blockIdx.y;
  const int s = blockIdx.x / tiles, tile = blockIdx.x - s * tiles;
  const int pad = L - 1, frames = S * B;
  const int n0 = s * B + tile * T;                 // first output frame of this tile
  const int n1 = min(n0 + T, (s + 1) * B);         // end (exclusive)
  float *sx = sm;                                  // x[n0 - pad .. n1) -> sx[0 .. pad + (n1-n0))
  float *st = sm + (T + pad);                      // taps [2][L]
  const float *xrow = x + (size_t)c * (pad + frames);
  for (int i = threadIdx.x; i < pad + (n1 - n0); i += 256) sx[i] = xrow[n0 + i];  // row index of frame n is pad + n
  const float *tp = taps + ((size_t)c * S + s) * 2 * L;
  for (int i = threadIdx.x; i < 2 * L; i += 256) st[i] = tp[i];
  __syncthreads();
  const float g = gain[c * S + s];
  for (int i = threadIdx.x; i < n1 - n0; i += 256) {
    float accl = 0.0f, accr = 0.0f;
    const float *xp = sx + pad + i;  // x[n], then x[n-1], ...
    for (int k = 0; k < L; k++) {
      const float xv = xp[-k];
      accl += st[k] * xv;
      accr += st[L + k] * xv;
    }
    float *o = partial + ((size_t)c * frames + n0 + i) * 2;
    o[0] = accl * g;
    o[1] = accr * g;
  }
}

// ---- overlap-save FFT form. grid (S, C); block 256; dynamic LDS: X[N], Z[N], twiddles[N/2] (float2)
__device__ __forceinline__ float2 hrtf_cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ int hrtf_bitrev(int v, int bits) { return (int)(__brev((unsigned)v) >> (32 - bits)); }
// in-place radix-2 decimation-in-time transform of buf[0..N) (input stored bit-reversed), all lanes of the block
template <bool INVERSE>
__device__ __forceinline__ void hrtf_fft_lds(float2 *buf, const float2 *tw, int N, int logN) {
  for (int st = 1; st <= logN; st++) {
    const int half = 1 << (st - 1);
    __syncthreads();
    for (int t = threadIdx.x; t < N / 2; t += 256) {
      const int j = t & (half - 1), base = (t >> (st - 1)) << st;
      float2 w = tw[j << (logN - st)];
      if (INVERSE) w.y = -w.y;
      const float2 a = buf[base + j], b = hrtf_cmul(buf[base + j + half], w);
      buf[base + j] = make_float2(a.x + b.x, a.y + b.y);
      buf[base + j + half] = make_float2(a.x - b.x, a.y - b.y);
    }
  }
  __syncthreads();
}

__global__ __launch_bounds__(256) void hrtf_fft_kernel(const float *__restrict__ x, const float *__restrict__ taps, const float *__restrict__ gain,
                                                       float *__restrict__ partial, int S, int B, int L, int N, int logN) {
  extern __shared__ float2 hsm[];
  float2 *X = hsm, *Z = hsm + N, *tw = hsm + 2 * N;
  const int s = blockIdx.x, c = blockIdx.y;
  const int pad = L - 1, frames = S * B, W = pad + B;  // window: x[n0 - pad .. n0 + B), n0 = s * B; row index of frame n is pad + n
  const float *xrow = x + (size_t)c * (pad + frames) + (size_t)s * B;
  const float *tp = taps + ((size_t)c * S + s) * 2 * L;
  for (int i = threadIdx.x; i < N / 2; i += 256) {
    float sn, cs;
    sincospif(-2.0f * (float)i / (float)N, &sn, &cs);
    tw[i] = make_float2(cs, sn);
  }
  for (int i = threadIdx.x; i < N; i += 256) {
    const int r = hrtf_bitrev(i, logN);
    X[r] = make_float2(i < W ? xrow[i] : 0.0f, 0.0f);
    Z[r] = i < L ? make_float2(tp[i], tp[L + i]) : make_float2(0.0f, 0.0f);  // left ear in the real part, right ear in the imaginary
  }
  hrtf_fft_lds<false>(X, tw, N, logN);
  hrtf_fft_lds<false>(Z, tw, N, logN);
  // Y = X Z back into X in bit-reversed order (every lane first reads its products, then all write)
  float2 y[16];
#pragma unroll
  for (int k = 0; k < 16; k++) {
    const int i = threadIdx.x + 256 * k;
    if (i < N) y[k] = hrtf_cmul(X[i], Z[i]);
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 16; k++) {
    const int i = threadIdx.x + 256 * k;
    if (i < N) X[hrtf_bitrev(i, logN)] = y[k];
  }
  hrtf_fft_lds<true>(X, tw, N, logN);
  const float g = gain[c * S + s] / (float)N;
  for (int i = threadIdx.x; i < B; i += 256) {  // overlap-save: window position pad + i holds output frame n0 + i
    const float2 v = X[pad + i];
    float *o = partial + ((size_t)c * frames + (size_t)s * B + i) * 2;
    o[0] = v.x * g;
    o[1] = v.y * g;
  }
}

// out[n] = ((0 + ch0) + ch1) + ...   (imp.rs:186 zero fill, :256-268 accumulation order)
__global__ __launch_bounds__(256) void hrtf_mix_kernel(const float *__restrict__ partial, float *__restrict__ out, int C, int frames) {
  const int i = blockIdx.x * 256 + threadIdx.x;  // index into [frames][2]
  if (i >= 2 * frames) return;
  float acc = 0.0f;
  int c = 0;
  for (; c + 8 <= C; c += 8) {  // eight independent loads in flight, added in channel order
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; u++) v[u] = partial[(size_t)(c + u) * frames * 2 + i];
#pragma unroll
    for (int u = 0; u < 8; u++) acc += v[u];
  }
  for (; c < C; c++) acc += partial[(size_t)c * frames * 2 + i];
  out[i] = acc;
}

// ------------------------------------------------------------------ host side

static void hrtf_free_processors(HrtfState *H) {
  for (int i = 0; i < 2; i++) { if (H->d_x[i]) (void)hipFree(H->d_x[i]); H->d_x[i] = nullptr; }
  float **fp[] = {&H->d_taps, &H->d_last_taps, &H->d_gain, &H->d_uvw, &H->d_partial, &H->d_in, &H->d_out};
  for (auto p : fp) { if (*p) (void)hipFree(*p); *p = nullptr; }
  if (H->d_face) (void)hipFree(H->d_face);
  H->d_face = nullptr;
  H->configured = false;
}

void hrtf_release(mi355_ctx *ctx) {
  HrtfState *H = hrtf_of(ctx);
  if (!H) return;
  hrtf_free_processors(H);
  if (H->d_pos) (void)hipFree(H->d_pos);
  if (H->d_idx) (void)hipFree(H->d_idx);
  if (H->d_hrir) (void)hipFree(H->d_hrir);
  delete H;
  ctx->hrtf = nullptr;
}

static uint32_t rd_u32(const unsigned char *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// HrirSphere::new(bytes, device_rate) (imp.rs:84-94)
// Sample-rate conversion of one HRIR when the sphere file was measured at another rate than the stream runs at
// (HrirSphere::new(bytes, rate), audio/hrtf/src/hrtf/imp.rs:83-93; the crate hands every HRIR to the `rubato` sinc
// resampler, whose sources are not in the reference tree: PARITY UNPINNED, this is the published method, not its bits).
// Band-limited interpolation: y[m] = sum_n h[n] * fc * sinc(fc * (t - n)) * w((t - n) / half), t = m / ratio,
// fc = 0.95 * min(1, ratio) (cut-off relative to the input Nyquist rate, 5 % guard band), half = 128 / min(1, ratio)
// input samples on either side (rubato's customary sinc_len = 256), w = squared 4-term Blackman-Harris window,
// f64 accumulation, no added delay; out_len = round(len * ratio). Runs once per sphere load on the host.
static std::vector<float> resample_hrir(const float *h, uint32_t len, double ratio, uint32_t out_len) {
  const double pi = 3.14159265358979323846;
  const double lo = ratio < 1.0 ? ratio : 1.0, fc = 0.95 * lo, half = 128.0 / lo;
  std::vector<float> y(out_len);
  for (uint32_t m = 0; m < out_len; m++) {
    const double t = (double)m / ratio;
    long n0 = (long)std::ceil(t - half), n1 = (long)std::floor(t + half);
    if (n0 < 0) n0 = 0;
    if (n1 > (long)len - 1) n1 = (long)len - 1;
    double acc = 0.0;
    for (long n = n0; n <= n1; n++) {
      const double d = t - (double)n, x = pi * fc * d;
      const double sinc = std::fabs(x) < 1e-12 ? 1.0 : std::sin(x) / x;
      const double u = 0.5 * (d / half + 1.0);  // 0..1 across the window
      const double bh = 0.35875 - 0.48829 * std::cos(2.0 * pi * u) + 0.14128 * std::cos(4.0 * pi * u) - 0.01168 * std::cos(6.0 * pi * u);
      acc += (double)h[n] * fc * sinc * bh * bh;
    }
    y[m] = (float)acc;
  }
  return y;
}

int hrtf_load_sphere(mi355_ctx *ctx, const unsigned char *bytes, size_t n, uint32_t device_rate) {
  if (!bytes || n < 20 || std::memcmp(bytes, "HRIR", 4) != 0) return set_error(ctx, MI355_ERR_INVALID_ARG, "hrtfrender: not an HRIR sphere (bad magic)");
  const uint32_t rate = rd_u32(bytes + 4), file_len = rd_u32(bytes + 8), nv = rd_u32(bytes + 12), ni = rd_u32(bytes + 16);
  if (file_len == 0) return set_error(ctx, MI355_ERR_INVALID_ARG, "hrtfrender: HRIR length is zero");
  const size_t need = 20 + 4 * (size_t)ni + (size_t)nv * (12 + 8 * (size_t)file_len);
  if (n < need) return set_error(ctx, MI355_ERR_INVALID_ARG, "hrtfrender: truncated HRIR sphere");
  if (rate == 0 || device_rate == 0) return set_error(ctx, MI355_ERR_INVALID_ARG, "hrtfrender: zero sample rate");
  const bool resample = rate != device_rate;
  const double ratio = (double)device_rate / (double)rate;
  uint32_t len = file_len;
  if (resample) {
    const double l = std::floor((double)file_len * ratio + 0.5);
    len = l < 1.0 ? 1u : (uint32_t)l;
  }
  std::vector<uint32_t> idx(ni);
  for (uint32_t i = 0; i < ni; i++) {
    idx[i] = rd_u32(bytes + 20 + 4 * (size_t)i);
    if (idx[i] >= nv) return set_error(ctx, MI355_ERR_INVALID_ARG, "hrtfrender: face index out of range");
  }
  std::vector<float> pos((size_t)nv * 3), hr((size_t)nv * 2 * len);
  size_t off = 20 + 4 * (size_t)ni;
  for (uint32_t v = 0; v < nv; v++) {
    std::memcpy(&pos[(size_t)v * 3], bytes + off, 12);  // little-endian host
    off += 12;
    if (!resample) {
      std::memcpy(&hr[(size_t)v * 2 * len], bytes + off, 8 * (size_t)len);
    } else {
      std::vector<float> raw(2 * (size_t)file_len);
      std::memcpy(raw.data(), bytes + off, 8 * (size_t)file_len);
      for (int ear = 0; ear < 2; ear++) {
        const std::vector<float> y = resample_hrir(raw.data() + (size_t)ear * file_len, file_len, ratio, len);
        std::memcpy(&hr[((size_t)v * 2 + ear) * len], y.data(), 4 * (size_t)len);
      }
    }
    off += 8 * (size_t)file_len;
  }
  HrtfState *H = hrtf_of(ctx);
  if (!H) { H = new HrtfState(); ctx->hrtf = H; }
  hrtf_free_processors(H);
  if (H->d_pos) (void)hipFree(H->d_pos);
  if (H->d_idx) (void)hipFree(H->d_idx);
  if (H->d_hrir) (void)hipFree(H->d_hrir);
  H->d_pos = nullptr; H->d_idx = nullptr; H->d_hrir = nullptr; H->sphere_loaded = false;
  int rc;
  if ((rc = check_hip(ctx, hipMalloc(&H->d_pos, pos.size() * 4 + 4), "hipMalloc(hrir positions)"))) return rc;
  if ((rc = check_hip(ctx, hipMalloc(&H->d_idx, idx.size() * 4 + 4), "hipMalloc(hrir indices)"))) return rc;
  if ((rc = check_hip(ctx, hipMalloc(&H->d_hrir, hr.size() * 4 + 4), "hipMalloc(hrir data)"))) return rc;
  if ((rc = check_hip(ctx, hipMemcpy(H->d_pos, pos.data(), pos.size() * 4, hipMemcpyHostToDevice), "upload hrir positions"))) return rc;
  if (!idx.empty() && (rc = check_hip(ctx, hipMemcpy(H->d_idx, idx.data(), idx.size() * 4, hipMemcpyHostToDevice), "upload hrir indices"))) return rc;
  if ((rc = check_hip(ctx, hipMemcpy(H->d_hrir, hr.data(), hr.size() * 4, hipMemcpyHostToDevice), "upload hrir data"))) return rc;
  H->rate = device_rate; H->len = len; H->n_vertices = nv; H->n_faces = ni / 3;
  H->sphere_loaded = true;
  return MI355_OK;
}

int hrtf_setup(mi355_ctx *ctx, int channels, int block_len, int steps) {
  HrtfState *H = hrtf_of(ctx);
  if (!H || !H->sphere_loaded) return set_error(ctx, MI355_ERR_NOT_CONFIGURED, "hrtfrender: impulse response not set");
  if (channels < 1 || block_len < 1 || steps < 1 || steps > 64) return set_error(ctx, MI355_ERR_INVALID_ARG, "hrtfrender: bad channels/block-length/interpolation-steps");
  if ((size_t)block_len * (size_t)steps > (1u << 24)) return set_error(ctx, MI355_ERR_INVALID_ARG, "hrtfrender: block too large");
  hrtf_free_processors(H);
  const size_t L = H->len, pad = L - 1, frames = (size_t)block_len * steps, C = (size_t)channels, S = (size_t)steps;
  const size_t T = block_len < 1024 ? (size_t)block_len : 1024;
  // overlap-save transform size: the next power of two that holds the window [L-1 | block]; X, Z and the twiddles fit the LDS up to 4096
  int fft_n = 1, fft_log = 0;
  while ((size_t)fft_n < (size_t)block_len + pad) { fft_n <<= 1; fft_log++; }
  const bool fft_fits = fft_n <= 4096 && fft_n >= 512;
  const bool fir_fits = (T + pad + 2 * L) * 4 <= 160 * 1024;
  if (!fft_fits && !fir_fits) return set_error(ctx, MI355_ERR_UNSUPPORTED, "hrtfrender: HRIR too long for the LDS (block + HRIR length above 4096 and FIR tile above 160 KB)");
  // method: 1 = FFT, 2 = FIR pinned; 0 = FFT from kHrtfFftMinTaps taps on, FIR below
  // measured, 64 sources, block 512 x 8 (ms per block, FFT / FIR): 64 taps 0.040 / 0.030, 256: 0.042 / 0.040, 512: 0.047 / 0.056,
  // 1024: 0.072 / 0.087, 2048: 0.128 / 0.156 (tools/bench_hrtf.py --method 1 / 2, r03)
  constexpr size_t kHrtfFftMinTaps = 384;
  const bool use_fft = fft_fits && (ctx->hrtf_method == 1 || !fir_fits || (ctx->hrtf_method == 0 && L >= kHrtfFftMinTaps));
  int rc;
  for (int i = 0; i < 2; i++) {
    if ((rc = check_hip(ctx, hipMalloc(&H->d_x[i], C * (pad + frames) * 4 + 4), "hipMalloc(hrtf input rows)"))) return rc;
    if ((rc = check_hip(ctx, hipMemset(H->d_x[i], 0, C * (pad + frames) * 4), "hipMemset(hrtf input rows)"))) return rc;
  }
  struct { float **p; size_t n; } bufs[] = {{&H->d_taps, C * S * 2 * L}, {&H->d_last_taps, C * 2 * L}, {&H->d_gain, C * S}, {&H->d_uvw, C * S * 3},
                                            {&H->d_partial, C * frames * 2}, {&H->d_in, frames * C}, {&H->d_out, frames * 2}};
  for (auto &b : bufs) {
    if ((rc = check_hip(ctx, hipMalloc(b.p, b.n * 4 + 4), "hipMalloc(hrtf state)"))) return rc;
    if ((rc = check_hip(ctx, hipMemset(*b.p, 0, b.n * 4), "hipMemset(hrtf state)"))) return rc;
  }
  if ((rc = check_hip(ctx, hipMalloc(&H->d_face, C * S * 4 + 4), "hipMalloc(hrtf faces)"))) return rc;
  H->channels = channels; H->steps = steps; H->block_len = block_len; H->cur = 0;
  H->fft_n = use_fft ? fft_n : 0; H->fft_log = use_fft ? fft_log : 0;
  H->prev_vec.assign(C * 3, 0.0f); H->prev_gain.assign(C, 0.0f); H->have_prev.assign(C, 0);
  H->configured = true;
  return MI355_OK;
}

// State::reset_processors (imp.rs:124-129): tails cleared, previous vectors/gains kept
int hrtf_reset(mi355_ctx *ctx) {
  HrtfState *H = hrtf_of(ctx);
  if (!H || !H->configured) return MI355_OK;
  const size_t row = (size_t)H->len - 1 + (size_t)H->block_len * H->steps;
  for (int i = 0; i < 2; i++) {
    int rc = check_hip(ctx, hipMemsetAsync(H->d_x[i], 0, (size_t)H->channels * row * 4, ctx->stream), "hipMemset(hrtf tails)");
    if (rc) return rc;
  }
  return MI355_OK;
}

// One block; d_in [frames][C] and d_out [frames][2] are device pointers. positions [C][3] right-handed (what the
// element hands the crate, imp.rs:64-73), gains [C]; both host arrays.
int hrtf_process_block_device(mi355_ctx *ctx, const float *d_in, float *d_out, const float *positions, const float *gains) {
  HrtfState *H = hrtf_of(ctx);
  if (!H || !H->configured) return set_error(ctx, MI355_ERR_NOT_CONFIGURED, "hrtfrender: not negotiated (setup not called)");
  const int C = H->channels, S = H->steps, B = H->block_len, L = (int)H->len, frames = S * B;
  HrtfVecGain vg;
  for (int c = 0; c < C; c++) {
    const float *nv = positions + 3 * c;
    const float *pv = H->have_prev[c] ? &H->prev_vec[3 * c] : nv;  // prev_sample_vector.unwrap_or(new) (imp.rs:236)
    for (int j = 0; j < 3; j++) { vg.v[3 * c + j] = pv[j]; vg.v[3 * C + 3 * c + j] = nv[j]; }
    vg.v[6 * C + c] = H->have_prev[c] ? H->prev_gain[c] : gains[c];
    vg.v[7 * C + c] = gains[c];
  }
  float *x_old = H->d_x[H->cur], *x_new = H->d_x[H->cur ^ 1];
  hipLaunchKernelGGL(hrtf_prepare_kernel, dim3(C), dim3(256), 0, ctx->stream, d_in, C, S, B, L, (const float *)H->d_pos, (const uint32_t *)H->d_idx,
                     (int)H->n_faces, (const float *)H->d_hrir, vg, (const float *)x_old, x_new, H->d_taps, H->d_last_taps,
                     H->d_gain, H->d_face, H->d_uvw);
  int rc;
  if (H->fft_n) {
    const size_t lds = (size_t)(2 * H->fft_n + H->fft_n / 2) * sizeof(float2);
    if ((rc = check_hip(ctx, hipFuncSetAttribute((const void *)hrtf_fft_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds), "hipFuncSetAttribute(hrtf fft LDS)"))) return rc;
    hipLaunchKernelGGL(hrtf_fft_kernel, dim3(S, C), dim3(256), lds, ctx->stream, (const float *)x_new, (const float *)H->d_taps, (const float *)H->d_gain, H->d_partial,
                       S, B, L, H->fft_n, H->fft_log);
  } else {
    const int T = B < 1024 ? B : 1024, tiles = (B + T - 1) / T;
    const size_t lds = (size_t)(T + (L - 1) + 2 * L) * 4;
    if ((rc = check_hip(ctx, hipFuncSetAttribute((const void *)hrtf_fir_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds), "hipFuncSetAttribute(hrtf fir LDS)"))) return rc;
    hipLaunchKernelGGL(hrtf_fir_kernel, dim3(S * tiles, C), dim3(256), lds, ctx->stream, (const float *)x_new, (const float *)H->d_taps,
                       (const float *)H->d_gain, H->d_partial, S, B, L, T, tiles);
  }
  hipLaunchKernelGGL(hrtf_mix_kernel, dim3((2 * frames + 255) / 256), dim3(256), 0, ctx->stream, (const float *)H->d_partial, d_out, C, frames);
  rc = check_hip(ctx, hipGetLastError(), "hrtf kernel launch");
  if (rc) return rc;
  H->cur ^= 1;
  for (int c = 0; c < C; c++) {
    for (int j = 0; j < 3; j++) H->prev_vec[3 * c + j] = positions[3 * c + j];
    H->prev_gain[c] = gains[c];
    H->have_prev[c] = 1;
  }
  return MI355_OK;
}

int hrtf_process_block_host(mi355_ctx *ctx, const float *in, float *out, const float *positions, const float *gains) {
  HrtfState *H = hrtf_of(ctx);
  if (!H || !H->configured) return set_error(ctx, MI355_ERR_NOT_CONFIGURED, "hrtfrender: not negotiated (setup not called)");
  const size_t frames = (size_t)H->steps * H->block_len;
  int rc = check_hip(ctx, hipMemcpyAsync(H->d_in, in, frames * H->channels * 4, hipMemcpyHostToDevice, ctx->stream), "hrtf H2D");
  if (rc) return rc;
  rc = hrtf_process_block_device(ctx, H->d_in, H->d_out, positions, gains);
  if (rc) return rc;
  rc = check_hip(ctx, hipMemcpyAsync(out, H->d_out, frames * 2 * 4, hipMemcpyDeviceToHost, ctx->stream), "hrtf D2H");
  if (rc) return rc;
  return check_hip(ctx, hipStreamSynchronize(ctx->stream), "hrtf sync");
}

// diagnostics: faces / weights chosen for the last block (tests compare the mesh search with the oracle's)
int hrtf_last_lookup(mi355_ctx *ctx, int *faces, float *uvw) {
  HrtfState *H = hrtf_of(ctx);
  if (!H || !H->configured) return set_error(ctx, MI355_ERR_NOT_CONFIGURED, "hrtfrender: not negotiated (setup not called)");
  const size_t n = (size_t)H->channels * H->steps;
  int rc = check_hip(ctx, hipStreamSynchronize(ctx->stream), "hrtf sync");
  if (rc) return rc;
  if (faces && (rc = check_hip(ctx, hipMemcpy(faces, H->d_face, n * 4, hipMemcpyDeviceToHost), "hrtf faces D2H"))) return rc;
  if (uvw && (rc = check_hip(ctx, hipMemcpy(uvw, H->d_uvw, n * 12, hipMemcpyDeviceToHost), "hrtf uvw D2H"))) return rc;
  return MI355_OK;
}

int hrtf_info(mi355_ctx *ctx, uint32_t *len, uint32_t *vertices, uint32_t *faces) {
  HrtfState *H = hrtf_of(ctx);
  if (!H || !H->sphere_loaded) return set_error(ctx, MI355_ERR_NOT_CONFIGURED, "hrtfrender: impulse response not set");
  if (len) *len = H->len;
  if (vertices) *vertices = H->n_vertices;
  if (faces) *faces = H->n_faces;
  return MI355_OK;
}

// which convolution form setup chose: the overlap-save transform size, 0 for the time-domain FIR
int hrtf_transform_size(mi355_ctx *ctx, int *fft_n) {
  HrtfState *H = hrtf_of(ctx);
  if (!H || !H->configured) return set_error(ctx, MI355_ERR_NOT_CONFIGURED, "hrtfrender: not negotiated (setup not called)");
  if (!fft_n) return set_error(ctx, MI355_ERR_INVALID_ARG, "hrtfrender: null output");
  *fft_n = H->fft_n;
  return MI355_OK;
}

}  // namespace mi355
