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
#include "audio_fft.hpp"
#include "internal.hpp"

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace mi355 {

// one HrirSphere on the device (crate file format, resampled to the device rate at load). A lone context owns its sphere; the
// members of an hrtf agroup that load the same bytes at the same rate share one (refs counts them).
struct HrtfSphere {
  uint32_t rate = 0, len = 0, n_vertices = 0, n_faces = 0;
  float *d_pos = nullptr;      // [V][3]
  uint32_t *d_idx = nullptr;   // [F][3]
  float *d_hrir = nullptr;     // [V][2][len]
  int refs = 1;
  std::vector<unsigned char> bytes;   // what it was made from (groups only: the key of the sharing)
};

struct HrtfState {
  HrtfSphere *sphere = nullptr;
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
  float *d_in = nullptr, *d_out = nullptr;  // staging for the host entry point (a lone context's; group members use the group's slabs)
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

// The three steps as __device__ bodies: the lone kernels below and the job-table kernels of an hrtf agroup (further down) call the
// SAME code with the same per-sample operation order, so a member's bits are a lone context's (tests/golden/hrtf_lone_crc.json pins
// the lone path's at the commit before the bodies were shared).
//
// One block per channel c of one instance.
__device__ __forceinline__ void hrtf_prepare_body(const float *__restrict__ in, int C, int S, int B, int L, const float *__restrict__ pos,
                                                  const uint32_t *__restrict__ idx, int F, const float *__restrict__ hrir, const float pv[3],
                                                  const float nv[3], float pg, float ng, const float *__restrict__ x_old, float *__restrict__ x_new,
                                                  float *__restrict__ taps, float *__restrict__ last_taps, float *__restrict__ gain,
                                                  int *__restrict__ face_out, float *__restrict__ uvw_out, int c) {
  const int frames = S * B, pad = L - 1;
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

// One block per channel.
__global__ __launch_bounds__(256) void hrtf_prepare_kernel(const float *__restrict__ in, int C, int S, int B, int L,
                                                           const float *__restrict__ pos, const uint32_t *__restrict__ idx, int F,
                                                           const float *__restrict__ hrir, HrtfVecGain VG,
                                                           const float *__restrict__ x_old, float *__restrict__ x_new,
                                                           float *__restrict__ taps, float *__restrict__ last_taps,
                                                           float *__restrict__ gain, int *__restrict__ face_out, float *__restrict__ uvw_out) {
  const int c = blockIdx.x;
  const float pv[3] = {VG.v[3 * c], VG.v[3 * c + 1], VG.v[3 * c + 2]};
  const float nv[3] = {VG.v[3 * C + 3 * c], VG.v[3 * C + 3 * c + 1], VG.v[3 * C + 3 * c + 2]};
  const float pg = VG.v[6 * C + c], ng = VG.v[7 * C + c];
  hrtf_prepare_body(in, C, S, B, L, pos, idx, F, hrir, pv, nv, pg, ng, x_old, x_new, taps, last_taps, gain, face_out, uvw_out, c);
}

// grid (S * tiles, C); block 256; dynamic LDS: [T + pad] input + [2][L] taps
__device__ __forceinline__ void hrtf_fir_body(float *sm, const float *__restrict__ x, const float *__restrict__ taps, const float *__restrict__ gain,
                                              float *__restrict__ partial, int S, int B, int L, int T, int c, int s, int tile) {
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

__global__ __launch_bounds__(256) void hrtf_fir_kernel(const float *__restrict__ x, const float *__restrict__ taps,
                                                       const float *__restrict__ gain, float *__restrict__ partial, int S, int B,
                                                       int L, int T, int tiles) {
  extern __shared__ float sm[];
  const int s = blockIdx.x / tiles;
  hrtf_fir_body(sm, x, taps, gain, partial, S, B, L, T, blockIdx.y, s, blockIdx.x - s * tiles);
}

// ---- overlap-save FFT form. grid (S, C); block 256; dynamic LDS: X[N], Z[N], twiddles[N/2] (float2)
// (cmul, bitrev and the transform in LDS are audio_fft.hpp's; its lanes stride by the block's 256 here)
__device__ __forceinline__ void hrtf_fft_body(float2 *hsm, const float *__restrict__ x, const float *__restrict__ taps, const float *__restrict__ gain,
                                              float *__restrict__ partial, int S, int B, int L, int N, int logN, int s, int c) {
  float2 *X = hsm, *Z = hsm + N, *tw = hsm + 2 * N;
  const int pad = L - 1, frames = S * B, W = pad + B;  // window: x[n0 - pad .. n0 + B), n0 = s * B; row index of frame n is pad + n
  const float *xrow = x + (size_t)c * (pad + frames) + (size_t)s * B;
  const float *tp = taps + ((size_t)c * S + s) * 2 * L;
  for (int i = threadIdx.x; i < N / 2; i += 256) {
    float sn, cs;
    sincospif(-2.0f * (float)i / (float)N, &sn, &cs);
    tw[i] = make_float2(cs, sn);
  }
  for (int i = threadIdx.x; i < N; i += 256) {
    const int r = bitrev(i, logN);
    X[r] = make_float2(i < W ? xrow[i] : 0.0f, 0.0f);
    Z[r] = i < L ? make_float2(tp[i], tp[L + i]) : make_float2(0.0f, 0.0f);  // left ear in the real part, right ear in the imaginary
  }
  fft_lds<false, 256>(X, tw, N, logN);
  fft_lds<false, 256>(Z, tw, N, logN);
  // Y = X Z back into X in bit-reversed order (every lane first reads its products, then all write)
  float2 y[16];
#pragma unroll
  for (int k = 0; k < 16; k++) {
    const int i = threadIdx.x + 256 * k;
    if (i < N) y[k] = cmul(X[i], Z[i]);
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 16; k++) {
    const int i = threadIdx.x + 256 * k;
    if (i < N) X[bitrev(i, logN)] = y[k];
  }
  fft_lds<true, 256>(X, tw, N, logN);
  const float g = gain[c * S + s] / (float)N;
  for (int i = threadIdx.x; i < B; i += 256) {  // overlap-save: window position pad + i holds output frame n0 + i
    const float2 v = X[pad + i];
    float *o = partial + ((size_t)c * frames + (size_t)s * B + i) * 2;
    o[0] = v.x * g;
    o[1] = v.y * g;
  }
}

__global__ __launch_bounds__(256) void hrtf_fft_kernel(const float *__restrict__ x, const float *__restrict__ taps, const float *__restrict__ gain,
                                                       float *__restrict__ partial, int S, int B, int L, int N, int logN) {
  extern __shared__ float2 hsm[];
  hrtf_fft_body(hsm, x, taps, gain, partial, S, B, L, N, logN, blockIdx.x, blockIdx.y);
}

// out[n] = ((0 + ch0) + ch1) + ...   (imp.rs:186 zero fill, :256-268 accumulation order)
__device__ __forceinline__ void hrtf_mix_body(const float *__restrict__ partial, float *__restrict__ out, int C, int frames, int i) {
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

__global__ __launch_bounds__(256) void hrtf_mix_kernel(const float *__restrict__ partial, float *__restrict__ out, int C, int frames) {
  hrtf_mix_body(partial, out, C, frames, blockIdx.x * 256 + threadIdx.x);  // index into [frames][2]
}

// ------------------------------------------------------------------ the job-table form (hrtf agroups, agroup.hip)
// Independent hrtfrender instances - own sphere, channel count, block-length, interpolation-steps, HRIR length and convolution
// form each - in ONE launch set. Two tables travel per set: one entry per member that has submitted (geometry, sphere, state,
// in / out) and one row per (member, channel) with the row's previous / new direction and gain (what HrtfVecGain carries by value
// for a lone context: 8 x 64 floats of kernel arguments cannot hold a set).
struct HrtfJobMember {
  const float *in; float *out;
  const float *pos; const uint32_t *idx; const float *hrir;
  const float *x_old; float *x_new;
  float *taps, *last_taps, *gain, *uvw, *partial;
  int *face;
  int C, S, B, L, F, N, logN, T, tiles, pad_;
};
struct HrtfJobRow { int member, c; float pv[3], nv[3], pg, ng; };

// grid (rows)
__global__ __launch_bounds__(256) void hrtf_prepare_jobs_kernel(const HrtfJobMember *__restrict__ members, const HrtfJobRow *__restrict__ rows) {
  const HrtfJobRow R = rows[blockIdx.x];
  const HrtfJobMember M = members[R.member];
  hrtf_prepare_body(M.in, M.C, M.S, M.B, M.L, M.pos, M.idx, M.F, M.hrir, R.pv, R.nv, R.pg, R.ng, M.x_old, M.x_new, M.taps, M.last_taps, M.gain, M.face,
                    M.uvw, R.c);
}

// grid (rows * ny), ny = max S * tiles of the FIR members; a block whose row is served by a transform, or that lies beyond its member's
// steps x tiles, leaves at once (as a whole: nobody is left at a barrier). Dynamic LDS: the largest [T + pad] + [2][L] of the set.
__global__ __launch_bounds__(256) void hrtf_fir_jobs_kernel(const HrtfJobMember *__restrict__ members, const HrtfJobRow *__restrict__ rows, int ny) {
  extern __shared__ float sm[];
  const int row = blockIdx.x / ny, y = blockIdx.x - row * ny;
  const HrtfJobRow R = rows[row];
  const HrtfJobMember M = members[R.member];
  if (M.N != 0 || y >= M.S * M.tiles) return;
  const int s = y / M.tiles;
  hrtf_fir_body(sm, M.x_new, M.taps, M.gain, M.partial, M.S, M.B, M.L, M.T, R.c, s, y - s * M.tiles);
}

// grid (rows * ny), ny = max S of the members on transform size N; one launch per distinct N in the set. Dynamic LDS: X[N], Z[N], twiddles[N/2].
__global__ __launch_bounds__(256) void hrtf_fft_jobs_kernel(const HrtfJobMember *__restrict__ members, const HrtfJobRow *__restrict__ rows, int N, int ny) {
  extern __shared__ float2 hsm[];
  const int row = blockIdx.x / ny, y = blockIdx.x - row * ny;
  const HrtfJobRow R = rows[row];
  const HrtfJobMember M = members[R.member];
  if (M.N != N || y >= M.S) return;
  hrtf_fft_body(hsm, M.x_new, M.taps, M.gain, M.partial, M.S, M.B, M.L, M.N, M.logN, y, R.c);
}

// grid (blocks of the longest output, members)
__global__ __launch_bounds__(256) void hrtf_mix_jobs_kernel(const HrtfJobMember *__restrict__ members) {
  const HrtfJobMember M = members[blockIdx.y];
  hrtf_mix_body(M.partial, M.out, M.C, M.S * M.B, blockIdx.x * 256 + threadIdx.x);
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

static void hrtf_sphere_unref(HrtfSphere *S) {
  if (!S || --S->refs > 0) return;
  if (S->d_pos) (void)hipFree(S->d_pos);
  if (S->d_idx) (void)hipFree(S->d_idx);
  if (S->d_hrir) (void)hipFree(S->d_hrir);
  delete S;
}

void hrtf_release(mi355_ctx *ctx) {
  HrtfState *H = hrtf_of(ctx);
  if (!H) return;
  hrtf_free_processors(H);
  hrtf_sphere_unref(H->sphere);
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

// HrirSphere::new(bytes, device_rate) (imp.rs:84-94): parsed, resampled where the rates differ, uploaded. *out is a new sphere with one reference.
static int hrtf_sphere_create(const unsigned char *bytes, size_t n, uint32_t device_rate, HrtfSphere **out, std::string *err) {
  if (!bytes || n < 20 || std::memcmp(bytes, "HRIR", 4) != 0) return audio_fail(MI355_ERR_INVALID_ARG, "hrtfrender: not an HRIR sphere (bad magic)", err);
  const uint32_t rate = rd_u32(bytes + 4), file_len = rd_u32(bytes + 8), nv = rd_u32(bytes + 12), ni = rd_u32(bytes + 16);
  if (file_len == 0) return audio_fail(MI355_ERR_INVALID_ARG, "hrtfrender: HRIR length is zero", err);
  const size_t need = 20 + 4 * (size_t)ni + (size_t)nv * (12 + 8 * (size_t)file_len);
  if (n < need) return audio_fail(MI355_ERR_INVALID_ARG, "hrtfrender: truncated HRIR sphere", err);
  if (rate == 0 || device_rate == 0) return audio_fail(MI355_ERR_INVALID_ARG, "hrtfrender: zero sample rate", err);
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
    if (idx[i] >= nv) return audio_fail(MI355_ERR_INVALID_ARG, "hrtfrender: face index out of range", err);
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
  HrtfSphere *S = new HrtfSphere();
  int rc;
  if ((rc = audio_hip(hipMalloc(&S->d_pos, pos.size() * 4 + 4), "hipMalloc(hrir positions)", err)) ||
      (rc = audio_hip(hipMalloc(&S->d_idx, idx.size() * 4 + 4), "hipMalloc(hrir indices)", err)) ||
      (rc = audio_hip(hipMalloc(&S->d_hrir, hr.size() * 4 + 4), "hipMalloc(hrir data)", err)) ||
      (rc = audio_hip(hipMemcpy(S->d_pos, pos.data(), pos.size() * 4, hipMemcpyHostToDevice), "upload hrir positions", err)) ||
      (!idx.empty() && (rc = audio_hip(hipMemcpy(S->d_idx, idx.data(), idx.size() * 4, hipMemcpyHostToDevice), "upload hrir indices", err))) ||
      (rc = audio_hip(hipMemcpy(S->d_hrir, hr.data(), hr.size() * 4, hipMemcpyHostToDevice), "upload hrir data", err))) {
    hrtf_sphere_unref(S);
    return rc;
  }
  S->rate = device_rate; S->len = len; S->n_vertices = nv; S->n_faces = ni / 3;
  *out = S;
  return MI355_OK;
}

int hrtf_load_sphere(mi355_ctx *ctx, const unsigned char *bytes, size_t n, uint32_t device_rate) {
  std::string err;
  HrtfSphere *S = nullptr;
  // (a load that fails in its checks leaves what was loaded before untouched; one that fails on the device leaves no sphere)
  int rc = hrtf_sphere_create(bytes, n, device_rate, &S, &err);
  if (rc == MI355_ERR_INVALID_ARG) return set_error(ctx, rc, err);
  HrtfState *H = hrtf_of(ctx);
  if (!H) { H = new HrtfState(); ctx->hrtf = H; }
  hrtf_free_processors(H);
  hrtf_sphere_unref(H->sphere);
  H->sphere = S;
  if (rc) return set_error(ctx, rc, err);
  return MI355_OK;
}

// HrtfProcessor::new per channel (imp.rs:662-680) for one instance: `method` is MI355_FLAG_HRTF_METHOD's value
static int hrtf_state_setup(HrtfState *H, int method, int channels, int block_len, int steps, bool own_staging, std::string *err) {
  if (!H || !H->sphere) return audio_fail(MI355_ERR_NOT_CONFIGURED, "hrtfrender: impulse response not set", err);
  // (channels above 64: the element's caps stop there, and HrtfVecGain holds 64 channels' directions and gains)
  if (channels < 1 || channels > 64 || block_len < 1 || steps < 1 || steps > 64) return audio_fail(MI355_ERR_INVALID_ARG, "hrtfrender: bad channels/block-length/interpolation-steps", err);
  if ((size_t)block_len * (size_t)steps > (1u << 24)) return audio_fail(MI355_ERR_INVALID_ARG, "hrtfrender: block too large", err);
  hrtf_free_processors(H);
  const size_t L = H->sphere->len, pad = L - 1, frames = (size_t)block_len * steps, C = (size_t)channels, S = (size_t)steps;
  const size_t T = block_len < 1024 ? (size_t)block_len : 1024;
  // overlap-save transform size: the next power of two that holds the window [L-1 | block]; X, Z and the twiddles fit the LDS up to 4096
  int fft_n = 1, fft_log = 0;
  while ((size_t)fft_n < (size_t)block_len + pad) { fft_n <<= 1; fft_log++; }
  const bool fft_fits = fft_n <= 4096 && fft_n >= 512;
  const bool fir_fits = (T + pad + 2 * L) * 4 <= 160 * 1024;
  if (!fft_fits && !fir_fits) return audio_fail(MI355_ERR_UNSUPPORTED, "hrtfrender: HRIR too long for the LDS (block + HRIR length above 4096 and FIR tile above 160 KB)", err);
  // method: 1 = FFT, 2 = FIR pinned; 0 = FFT from kHrtfFftMinTaps taps on, FIR below
  // measured, 64 sources, block 512 x 8 (ms per block, FFT / FIR): 64 taps 0.040 / 0.030, 256: 0.042 / 0.040, 512: 0.047 / 0.056,
  // 1024: 0.072 / 0.087, 2048: 0.128 / 0.156 (tools/bench_hrtf.py --method 1 / 2, r03)
  constexpr size_t kHrtfFftMinTaps = 384;
  const bool use_fft = fft_fits && (method == 1 || !fir_fits || (method == 0 && L >= kHrtfFftMinTaps));
  int rc;
  for (int i = 0; i < 2; i++) {
    if ((rc = audio_hip(hipMalloc(&H->d_x[i], C * (pad + frames) * 4 + 4), "hipMalloc(hrtf input rows)", err))) return rc;
    if ((rc = audio_hip(hipMemset(H->d_x[i], 0, C * (pad + frames) * 4), "hipMemset(hrtf input rows)", err))) return rc;
  }
  struct { float **p; size_t n; } bufs[] = {{&H->d_taps, C * S * 2 * L}, {&H->d_last_taps, C * 2 * L}, {&H->d_gain, C * S}, {&H->d_uvw, C * S * 3},
                                            {&H->d_partial, C * frames * 2}, {&H->d_in, frames * C}, {&H->d_out, frames * 2}};
  for (auto &b : bufs) {
    if (!own_staging && (b.p == &H->d_in || b.p == &H->d_out)) continue;
    if ((rc = audio_hip(hipMalloc(b.p, b.n * 4 + 4), "hipMalloc(hrtf state)", err))) return rc;
    if ((rc = audio_hip(hipMemset(*b.p, 0, b.n * 4), "hipMemset(hrtf state)", err))) return rc;
  }
  if ((rc = audio_hip(hipMalloc(&H->d_face, C * S * 4 + 4), "hipMalloc(hrtf faces)", err))) return rc;
  H->channels = channels; H->steps = steps; H->block_len = block_len; H->cur = 0;
  H->fft_n = use_fft ? fft_n : 0; H->fft_log = use_fft ? fft_log : 0;
  H->prev_vec.assign(C * 3, 0.0f); H->prev_gain.assign(C, 0.0f); H->have_prev.assign(C, 0);
  H->configured = true;
  return MI355_OK;
}

int hrtf_setup(mi355_ctx *ctx, int channels, int block_len, int steps) {
  std::string err;
  const int rc = hrtf_state_setup(hrtf_of(ctx), ctx->hrtf_method, channels, block_len, steps, true, &err);
  return rc ? set_error(ctx, rc, err) : MI355_OK;
}

// State::reset_processors (imp.rs:124-129): tails cleared, previous vectors/gains kept
static int hrtf_state_reset(HrtfState *H, hipStream_t stream, std::string *err) {
  if (!H || !H->configured) return MI355_OK;
  const size_t row = (size_t)H->sphere->len - 1 + (size_t)H->block_len * H->steps;
  for (int i = 0; i < 2; i++) {
    int rc = audio_hip(hipMemsetAsync(H->d_x[i], 0, (size_t)H->channels * row * 4, stream), "hipMemset(hrtf tails)", err);
    if (rc) return rc;
  }
  return MI355_OK;
}

int hrtf_reset(mi355_ctx *ctx) {
  std::string err;
  const int rc = hrtf_state_reset(hrtf_of(ctx), ctx->stream, &err);
  return rc ? set_error(ctx, rc, err) : MI355_OK;
}

// prev_sample_vector.unwrap_or(new) (imp.rs:236): the row's previous / new direction and gain for this block
static void hrtf_prev_new(const HrtfState *H, int c, const float *positions, const float *gains, float pv[3], float nv[3], float *pg, float *ng) {
  const float *n = positions + 3 * c;
  const float *p = H->have_prev[c] ? &H->prev_vec[3 * c] : n;
  for (int j = 0; j < 3; j++) { pv[j] = p[j]; nv[j] = n[j]; }
  *pg = H->have_prev[c] ? H->prev_gain[c] : gains[c];
  *ng = gains[c];
}

static void hrtf_advance(HrtfState *H, const float *positions, const float *gains) {
  H->cur ^= 1;
  for (int c = 0; c < H->channels; c++) {
    for (int j = 0; j < 3; j++) H->prev_vec[3 * c + j] = positions[3 * c + j];
    H->prev_gain[c] = gains[c];
    H->have_prev[c] = 1;
  }
}

// One block; d_in [frames][C] and d_out [frames][2] are device pointers. positions [C][3] right-handed (what the
// element hands the crate, imp.rs:64-73), gains [C]; both host arrays.
int hrtf_process_block_device(mi355_ctx *ctx, const float *d_in, float *d_out, const float *positions, const float *gains) {
  HrtfState *H = hrtf_of(ctx);
  if (!H || !H->configured) return set_error(ctx, MI355_ERR_NOT_CONFIGURED, "hrtfrender: not negotiated (setup not called)");
  const HrtfSphere *Sp = H->sphere;
  const int C = H->channels, S = H->steps, B = H->block_len, L = (int)Sp->len, frames = S * B;
  HrtfVecGain vg;
  for (int c = 0; c < C; c++) {
    float pv[3], nv[3];
    hrtf_prev_new(H, c, positions, gains, pv, nv, &vg.v[6 * C + c], &vg.v[7 * C + c]);
    for (int j = 0; j < 3; j++) { vg.v[3 * c + j] = pv[j]; vg.v[3 * C + 3 * c + j] = nv[j]; }
  }
  float *x_old = H->d_x[H->cur], *x_new = H->d_x[H->cur ^ 1];
  hipLaunchKernelGGL(hrtf_prepare_kernel, dim3(C), dim3(256), 0, ctx->stream, d_in, C, S, B, L, (const float *)Sp->d_pos, (const uint32_t *)Sp->d_idx,
                     (int)Sp->n_faces, (const float *)Sp->d_hrir, vg, (const float *)x_old, x_new, H->d_taps, H->d_last_taps,
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
  hrtf_advance(H, positions, gains);
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

static int hrtf_state_last_lookup(HrtfState *H, hipStream_t stream, int *faces, float *uvw, std::string *err) {
  if (!H || !H->configured) return audio_fail(MI355_ERR_NOT_CONFIGURED, "hrtfrender: not negotiated (setup not called)", err);
  const size_t n = (size_t)H->channels * H->steps;
  int rc = audio_hip(hipStreamSynchronize(stream), "hrtf sync", err);
  if (rc) return rc;
  if (faces && (rc = audio_hip(hipMemcpy(faces, H->d_face, n * 4, hipMemcpyDeviceToHost), "hrtf faces D2H", err))) return rc;
  if (uvw && (rc = audio_hip(hipMemcpy(uvw, H->d_uvw, n * 12, hipMemcpyDeviceToHost), "hrtf uvw D2H", err))) return rc;
  return MI355_OK;
}

// diagnostics: faces / weights chosen for the last block (tests compare the mesh search with the oracle's)
int hrtf_last_lookup(mi355_ctx *ctx, int *faces, float *uvw) {
  std::string err;
  const int rc = hrtf_state_last_lookup(hrtf_of(ctx), ctx->stream, faces, uvw, &err);
  return rc ? set_error(ctx, rc, err) : MI355_OK;
}

int hrtf_info(mi355_ctx *ctx, uint32_t *len, uint32_t *vertices, uint32_t *faces) {
  HrtfState *H = hrtf_of(ctx);
  if (!H || !H->sphere) return set_error(ctx, MI355_ERR_NOT_CONFIGURED, "hrtfrender: impulse response not set");
  if (len) *len = H->sphere->len;
  if (vertices) *vertices = H->sphere->n_vertices;
  if (faces) *faces = H->sphere->n_faces;
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

// ------------------------------------------------------------------ the members of one hrtf agroup
// The dispatcher (agroup.hip) collects the submissions and owns the stream and the staging slabs; what an hrtfrender instance IS -
// its sphere, its processors, its previous directions - lives here, next to the lone context's.
struct HrtfGroup {
  std::vector<HrtfState> members;
  std::vector<HrtfSphere *> spheres;      // the distinct spheres the group keeps on the device
  // the tables of the launch set: pinned block + device block ([members of the set][rows of the set]); ev: the previous set's
  // tables have left the pinned block
  char *h_tab = nullptr, *d_tab = nullptr;
  size_t row_cap = 0;
  hipEvent_t ev = nullptr;
  uint64_t n_launches = 0;
};

static size_t hrtf_rows_offset(const HrtfGroup *G) { return (G->members.size() * sizeof(HrtfJobMember) + 15) & ~(size_t)15; }

HrtfGroup *hrtf_group_new(int n_members, std::string *err, int *status) {
  HrtfGroup *G = new HrtfGroup();
  G->members.resize((size_t)n_members);
  *status = audio_hip(hipEventCreateWithFlags(&G->ev, hipEventDisableTiming), "hipEventCreate(hrtf group)", err);
  if (*status) { delete G; return nullptr; }
  return G;
}

void hrtf_group_free(HrtfGroup *G) {
  if (!G) return;
  for (HrtfState &H : G->members) { hrtf_free_processors(&H); hrtf_sphere_unref(H.sphere); H.sphere = nullptr; }
  if (G->h_tab) (void)hipHostFree(G->h_tab);
  if (G->d_tab) (void)hipFree(G->d_tab);
  if (G->ev) (void)hipEventDestroy(G->ev);
  delete G;
}

static void hrtf_group_drop_sphere(HrtfGroup *G, HrtfState *H) {
  HrtfSphere *S = H->sphere;
  H->sphere = nullptr;
  if (!S) return;
  if (S->refs == 1)
    for (size_t i = 0; i < G->spheres.size(); i++)
      if (G->spheres[i] == S) { G->spheres.erase(G->spheres.begin() + (std::ptrdiff_t)i); break; }
  hrtf_sphere_unref(S);
}

// Members that load identical bytes at the same device rate share ONE device copy; the parse and the windowed-sinc resampling
// run once per distinct (bytes, rate). (The caller has ordered this after the member's last launch set.)
int hrtf_group_load_sphere(HrtfGroup *G, int m, const unsigned char *bytes, size_t n, uint32_t device_rate, std::string *err) {
  HrtfState *H = &G->members[(size_t)m];
  HrtfSphere *S = nullptr;
  if (bytes)
    for (HrtfSphere *s : G->spheres)
      if (s->rate == device_rate && s->bytes.size() == n && std::memcmp(s->bytes.data(), bytes, n) == 0) { S = s; break; }
  if (S) {
    S->refs++;
  } else {
    const int rc = hrtf_sphere_create(bytes, n, device_rate, &S, err);
    if (rc == MI355_ERR_INVALID_ARG) return rc;   // (what was loaded before stays, as for a lone context)
    if (rc) { hrtf_free_processors(H); hrtf_group_drop_sphere(G, H); return rc; }
    S->bytes.assign(bytes, bytes + n);
    G->spheres.push_back(S);
  }
  hrtf_free_processors(H);
  hrtf_group_drop_sphere(G, H);
  H->sphere = S;
  return MI355_OK;
}

int hrtf_group_setup(HrtfGroup *G, int m, int channels, int block_len, int steps, int method, std::string *err) {
  if (method < 0 || method > 2) return audio_fail(MI355_ERR_INVALID_ARG, "hrtfrender: method is 0 (by HRIR length), 1 (FFT) or 2 (FIR)", err);
  return hrtf_state_setup(&G->members[(size_t)m], method, channels, block_len, steps, false, err);
}

int hrtf_group_reset(HrtfGroup *G, int m, hipStream_t stream, std::string *err) { return hrtf_state_reset(&G->members[(size_t)m], stream, err); }

bool hrtf_group_configured(const HrtfGroup *G, int m) { return G->members[(size_t)m].configured; }
bool hrtf_group_has_sphere(const HrtfGroup *G, int m) { return G->members[(size_t)m].sphere != nullptr; }
int hrtf_group_channels(const HrtfGroup *G, int m) { return G->members[(size_t)m].channels; }
size_t hrtf_group_frames(const HrtfGroup *G, int m) { const HrtfState &H = G->members[(size_t)m]; return (size_t)H.steps * H.block_len; }
uint64_t hrtf_group_launches(const HrtfGroup *G) { return G->n_launches; }

int hrtf_group_info(HrtfGroup *G, int m, uint32_t *hrir_len, int *fft_n, int *spheres_held, std::string *err) {
  const HrtfState &H = G->members[(size_t)m];
  if (!H.sphere) return audio_fail(MI355_ERR_NOT_CONFIGURED, "hrtfrender: impulse response not set", err);
  if (hrir_len) *hrir_len = H.sphere->len;
  if (fft_n) *fft_n = H.configured ? H.fft_n : -1;
  if (spheres_held) *spheres_held = (int)G->spheres.size();
  return MI355_OK;
}

int hrtf_group_last_lookup(HrtfGroup *G, int m, hipStream_t stream, int *faces, float *uvw, std::string *err) {
  return hrtf_state_last_lookup(&G->members[(size_t)m], stream, faces, uvw, err);
}

// the largest dynamic LDS a job kernel has been allowed so far (the attribute belongs to the function, not to a group)
static size_t g_hrtf_fir_lds = 0, g_hrtf_fft_lds = 0;

// ONE launch set for the members in subs[0..n): tables up, prepare, at most one convolution launch per distinct transform size plus
// one for the FIR rows, mix. Enqueued on `stream`; nothing is waited for but the pinned table block of the previous set.
int hrtf_group_run(HrtfGroup *G, hipStream_t stream, const HrtfSubmit *subs, int n, std::string *err) {
  if (n <= 0) return MI355_OK;
  size_t n_rows = 0;
  for (int j = 0; j < n; j++) n_rows += (size_t)G->members[(size_t)subs[j].member].channels;
  const size_t rows_off = hrtf_rows_offset(G);
  int rc;
  if (n_rows > G->row_cap) {
    if ((rc = audio_hip(hipStreamSynchronize(stream), "hrtf group: sync", err))) return rc;
    if (G->h_tab) (void)hipHostFree(G->h_tab);
    if (G->d_tab) (void)hipFree(G->d_tab);
    G->h_tab = G->d_tab = nullptr; G->row_cap = 0;
    size_t cap = 64;
    while (cap < n_rows) cap *= 2;
    const size_t bytes = rows_off + cap * sizeof(HrtfJobRow);
    if ((rc = audio_hip(hipHostMalloc((void **)&G->h_tab, bytes, hipHostMallocDefault), "hipHostMalloc(hrtf group tables)", err))) return rc;
    if ((rc = audio_hip(hipMalloc((void **)&G->d_tab, bytes), "hipMalloc(hrtf group tables)", err))) return rc;
    G->row_cap = cap;
  }
  if ((rc = audio_hip(hipEventSynchronize(G->ev), "hipEventSynchronize(hrtf group tables)", err))) return rc;
  HrtfJobMember *hm = (HrtfJobMember *)G->h_tab;
  HrtfJobRow *hr = (HrtfJobRow *)(G->h_tab + rows_off);
  size_t r = 0, fir_lds = 0;
  int fir_y = 0, mix_x = 0;
  int fft_sizes[4] = {0, 0, 0, 0}, fft_y[4] = {0, 0, 0, 0}, n_fft = 0;   // 512, 1024, 2048, 4096 at the most
  for (int j = 0; j < n; j++) {
    HrtfState &H = G->members[(size_t)subs[j].member];
    const HrtfSphere *Sp = H.sphere;
    HrtfJobMember &M = hm[j];
    M.in = subs[j].d_in; M.out = subs[j].d_out;
    M.pos = Sp->d_pos; M.idx = Sp->d_idx; M.hrir = Sp->d_hrir;
    M.x_old = H.d_x[H.cur]; M.x_new = H.d_x[H.cur ^ 1];
    M.taps = H.d_taps; M.last_taps = H.d_last_taps; M.gain = H.d_gain; M.uvw = H.d_uvw; M.partial = H.d_partial; M.face = H.d_face;
    M.C = H.channels; M.S = H.steps; M.B = H.block_len; M.L = (int)Sp->len; M.F = (int)Sp->n_faces; M.N = H.fft_n; M.logN = H.fft_log;
    M.T = H.block_len < 1024 ? H.block_len : 1024; M.tiles = (H.block_len + M.T - 1) / M.T; M.pad_ = 0;
    for (int c = 0; c < H.channels; c++, r++) {
      HrtfJobRow &R = hr[r];
      R.member = j; R.c = c;
      hrtf_prev_new(&H, c, subs[j].positions, subs[j].gains, R.pv, R.nv, &R.pg, &R.ng);
    }
    if (H.fft_n) {
      int k = 0;
      while (k < n_fft && fft_sizes[k] != H.fft_n) k++;
      if (k == n_fft) fft_sizes[n_fft++] = H.fft_n;
      if (H.steps > fft_y[k]) fft_y[k] = H.steps;
    } else {
      const size_t lds = (size_t)(M.T + (M.L - 1) + 2 * M.L) * 4;
      if (lds > fir_lds) fir_lds = lds;
      if (M.S * M.tiles > fir_y) fir_y = M.S * M.tiles;
    }
    const int mx = (2 * M.S * M.B + 255) / 256;
    if (mx > mix_x) mix_x = mx;
  }
  const HrtfJobMember *dm = (const HrtfJobMember *)G->d_tab;
  const HrtfJobRow *dr = (const HrtfJobRow *)(G->d_tab + rows_off);
  // (two copies, each of what this set fills: the member entries end where the rows' fixed offset begins only in a full group)
  if ((rc = audio_hip(hipMemcpyAsync(G->d_tab, G->h_tab, (size_t)n * sizeof(HrtfJobMember), hipMemcpyHostToDevice, stream), "hrtf group: member table", err))) return rc;
  if ((rc = audio_hip(hipMemcpyAsync(G->d_tab + rows_off, G->h_tab + rows_off, n_rows * sizeof(HrtfJobRow), hipMemcpyHostToDevice, stream), "hrtf group: row table", err))) return rc;
  if ((rc = audio_hip(hipEventRecord(G->ev, stream), "hipEventRecord(hrtf group tables)", err))) return rc;
  hipLaunchKernelGGL(hrtf_prepare_jobs_kernel, dim3((unsigned)n_rows), dim3(256), 0, stream, dm, dr);
  G->n_launches++;
  for (int k = 0; k < n_fft; k++) {
    const size_t lds = (size_t)(2 * fft_sizes[k] + fft_sizes[k] / 2) * sizeof(float2);
    if ((rc = audio_allow_lds((const void *)hrtf_fft_jobs_kernel, &g_hrtf_fft_lds, lds, "hipFuncSetAttribute(hrtf group fft LDS)", err))) return rc;
    hipLaunchKernelGGL(hrtf_fft_jobs_kernel, dim3((unsigned)(n_rows * (size_t)fft_y[k])), dim3(256), lds, stream, dm, dr, fft_sizes[k], fft_y[k]);
    G->n_launches++;
  }
  if (fir_y) {
    if ((rc = audio_allow_lds((const void *)hrtf_fir_jobs_kernel, &g_hrtf_fir_lds, fir_lds, "hipFuncSetAttribute(hrtf group fir LDS)", err))) return rc;
    hipLaunchKernelGGL(hrtf_fir_jobs_kernel, dim3((unsigned)(n_rows * (size_t)fir_y)), dim3(256), fir_lds, stream, dm, dr, fir_y);
    G->n_launches++;
  }
  hipLaunchKernelGGL(hrtf_mix_jobs_kernel, dim3((unsigned)mix_x, (unsigned)n), dim3(256), 0, stream, dm);
  G->n_launches++;
  if ((rc = audio_hip(hipGetLastError(), "hrtf group kernel launch", err))) return rc;
  for (int j = 0; j < n; j++) hrtf_advance(&G->members[(size_t)subs[j].member], subs[j].positions, subs[j].gains);
  return MI355_OK;
}

}  // namespace mi355
