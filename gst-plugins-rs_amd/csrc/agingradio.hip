// agingradio.hip — gfx950 kernels for agingradio.
//
// Reference loop replaced: AgingRadio::process (audio/audiofx/src/agingradio/imp.rs:94-136). Per pair of frames k (a buffer
// walked in chunks_exact_mut(channels * 2), :101) either a click - every sample 1.0, no filter step (:102-107) - or, per sample
// in f64: + uniform noise (:108-112); lowpass y += alpha * (clamp(x) - y) on filter c % channels (:113-116); round(x * f) / f
// (:117-122); `passes` times x - d * x^3 (:123-128); narrowed to the buffer's type (:130). The random draws come from
// Philox4x32-10 keyed by the instance's seed and counted by (pair, draw slot), so any lane can compute any draw.
//
// Two kernels over one job table (internal.hpp: AgingJob):
//   agingradio_stream_kernel : jobs without a lowpass. Every sample is independent: one streaming pass, no LDS.
//   agingradio_tiled_kernel  : jobs with a lowpass, one workgroup each. The filter is a serial recurrence per channel, so a tile
//                              of frame pairs goes (a) all lanes: load, draw, click / noise / clamp, stage f64 and the click flags
//                              in LDS; (b) one lane per channel: the recurrence over the tile's non-click samples in order;
//                              (c) all lanes: quantise, cubic curve, narrow, store in place.
// Arithmetic is plain f64 (-ffp-contract=off): nothing is fused, as in the reference.
#include "internal.hpp"

#include <cmath>
#include <cstring>

namespace mi355 {

// ---------------------------------------------------------------- device side

// Philox4x32-10 (Salmon et al., SC'11; Random123's constants)
__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; r++) {
    const uint32_t lo0 = 0xD2511F53u * c.x, hi0 = __umulhi(0xD2511F53u, c.x);
    const uint32_t lo1 = 0xCD9E8D57u * c.z, hi1 = __umulhi(0xCD9E8D57u, c.z);
    c = make_uint4(hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c;
}

// draw j of frame pair `pair`: 64-bit word j & 1 of Philox(counter = (pair_lo, pair_hi, j >> 1, 0), key = seed)
__device__ __forceinline__ unsigned long long aging_draw(const AgingJob &J, unsigned long long pair, unsigned long long j) {
  const uint4 r = philox4x32_10(make_uint4((uint32_t)pair, (uint32_t)(pair >> 32), (uint32_t)(j >> 1), 0u), (uint32_t)J.seed, (uint32_t)(J.seed >> 32));
  return (j & 1) ? ((unsigned long long)r.w << 32 | r.z) : ((unsigned long long)r.y << 32 | r.x);
}

// rng.random_bool(p) = Bernoulli::new(p).sample: always when p == 1, else u64 < (p * 2^64) as u64 (draw 0)
__device__ __forceinline__ bool aging_click(const AgingJob &J, unsigned long long pair) {
  if (!(J.flags & kAgingClick)) return false;
  if (J.p_int == ~0ull) return true;
  return aging_draw(J, pair, 0) < J.p_int;
}

// x + rng.random_range(-a..a) (draw 1 + c): a value in [1, 2) from the top 52 bits, minus 1, times the range, plus the low end
__device__ __forceinline__ double aging_noise(const AgingJob &J, double x, unsigned long long pair, unsigned long long c) {
  if (!(J.flags & kAgingNoise)) return x;
  const unsigned long long u = aging_draw(J, pair, 1 + c);
  const double v = __longlong_as_double((long long)((u >> 12) | 0x3FF0000000000000ull)) - 1.0;
  const double scale = J.ampl + J.ampl;
  const double noise = v * scale + (-J.ampl);
  return x + noise;
}

// f64::clamp(-1.0, 1.0): compare-based, so NaN stays NaN
__device__ __forceinline__ double aging_clamp(double x) { return x < -1.0 ? -1.0 : (x > 1.0 ? 1.0 : x); }

// quantise and the cubic curve (imp.rs:117-128): round() rounds half away from zero; the quotient is a division
__device__ __forceinline__ double aging_shape(const AgingJob &J, double x) {
  if (J.flags & kAgingQuant) {
    x = x * J.factor;
    x = round(x);
    x = x / J.factor;
  }
  if (J.flags & kAgingCubic)
    for (unsigned p = 0; p < J.passes; p++) x = x - J.dist * (x * (x * x));
  return x;
}

template <typename T>
__device__ __forceinline__ void aging_stream(const AgingJob &J) {
  T *data = (T *)J.data;
  const unsigned long long span = 2ull * J.channels, n = (J.frames / 2) * span;
  const size_t gs = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gs) {
    const unsigned long long pl = i / span, c = i - pl * span, pair = J.k0 + pl;
    double x = (double)data[i];
    if (aging_click(J, pair)) x = 1.0;
    else x = aging_shape(J, aging_noise(J, x, pair, c));
    data[i] = (T)x;
  }
}

// Where a launch finds its jobs: a context's single job travels in the kernel arguments (no copy, no event), a group's table
// through device memory.
struct AgingJobSrc {
  const AgingJob *dev;
  AgingJob inl;
  __device__ __forceinline__ AgingJob at(unsigned j) const { return dev ? dev[j] : inl; }
};

__global__ __launch_bounds__(256) void agingradio_stream_kernel(AgingJobSrc src) {
  const AgingJob J = src.at(blockIdx.y);
  if (J.state) return;   // the tiled kernel's job
  if (J.is_f64) aging_stream<double>(J); else aging_stream<float>(J);
}

constexpr unsigned kAgingTileSamples = 4096;   // f64 staged per tile: 32 KiB of LDS (2 * channels <= this: channels <= 2048)
constexpr unsigned kAgingBatch = 8;            // pairs whose samples phase (b) loads before it runs their recurrence steps

template <typename T>
__device__ __forceinline__ void aging_tiled(const AgingJob &J, double *v, unsigned char *clk) {
  T *data = (T *)J.data;
  const unsigned ch = J.channels, span = 2 * ch;
  const unsigned long long pairs = J.frames / 2;
  const unsigned tile_pairs = kAgingTileSamples / span;
  const double alpha = J.alpha;
  for (unsigned long long p0 = 0; p0 < pairs; p0 += tile_pairs) {
    const unsigned tp = (unsigned)(pairs - p0 < tile_pairs ? pairs - p0 : tile_pairs), ns = tp * span;
    T *tile = data + p0 * span;
    // (a) draws, noise and clamp for every sample; the click flag per pair (its sample 0 writes it)
    for (unsigned s = threadIdx.x; s < ns; s += blockDim.x) {
      const unsigned pl = s / span, c = s - pl * span;
      const unsigned long long pair = J.k0 + p0 + pl;
      const bool k = aging_click(J, pair);
      if (c == 0) clk[pl] = k ? 1 : 0;
      v[s] = k ? 1.0 : aging_clamp(aging_noise(J, (double)tile[s], pair, c));
    }
    __syncthreads();
    // (b) the recurrence y = y + alpha * (x - y), one lane per channel, samples of the tile in order; clicks leave y alone
    for (unsigned c = threadIdx.x; c < ch; c += blockDim.x) {
      double y = J.state[c];
      unsigned pl = 0;
      for (; pl + kAgingBatch <= tp; pl += kAgingBatch) {
        double x[2 * kAgingBatch];
        bool k[kAgingBatch];
#pragma unroll
        for (unsigned q = 0; q < kAgingBatch; q++) {
          k[q] = clk[pl + q] != 0;
          x[2 * q] = v[(pl + q) * span + c];
          x[2 * q + 1] = v[(pl + q) * span + ch + c];
        }
#pragma unroll
        for (unsigned q = 0; q < kAgingBatch; q++) {
          if (k[q]) continue;
          y = y + alpha * (x[2 * q] - y);
          x[2 * q] = y;
          y = y + alpha * (x[2 * q + 1] - y);
          x[2 * q + 1] = y;
        }
#pragma unroll
        for (unsigned q = 0; q < kAgingBatch; q++) {
          v[(pl + q) * span + c] = x[2 * q];
          v[(pl + q) * span + ch + c] = x[2 * q + 1];
        }
      }
      for (; pl < tp; pl++) {
        if (clk[pl]) continue;
        const unsigned i0 = pl * span + c, i1 = i0 + ch;
        y = y + alpha * (v[i0] - y);
        v[i0] = y;
        y = y + alpha * (v[i1] - y);
        v[i1] = y;
      }
      J.state[c] = y;
    }
    __syncthreads();
    // (c) quantise, cubic curve, narrow, store in place
    for (unsigned s = threadIdx.x; s < ns; s += blockDim.x) {
      const unsigned pl = s / span;
      tile[s] = (T)(clk[pl] ? 1.0 : aging_shape(J, v[s]));
    }
    __syncthreads();   // the next tile's phase (a) overwrites v and clk
  }
}

__global__ __launch_bounds__(256) void agingradio_tiled_kernel(AgingJobSrc src) {
  __shared__ double v[kAgingTileSamples];
  __shared__ unsigned char clk[kAgingTileSamples / 2];
  const AgingJob J = src.at(blockIdx.y);
  if (!J.state) return;   // the streaming kernel's job
  if (J.is_f64) aging_tiled<double>(J, v, clk); else aging_tiled<float>(J, v, clk);
}

// ---------------------------------------------------------------- host side

// LowpassFilter::<f64>::new(rate, cutoff) (lowpass-filter 0.4.1): rc = 1 / (cutoff * 2 * pi), dt = 1 / rate, alpha = dt / (rc + dt)
int agingradio_setup_filter(unsigned rate, unsigned lowpass_freq, double *alpha) {
  const double rc = 1.0 / ((double)lowpass_freq * 2.0 * 3.141592653589793);
  const double dt = 1.0 / (double)rate;
  *alpha = dt / (rc + dt);
  return MI355_OK;
}

// Settings as transform_ip snapshots them (imp.rs:284-305); 2^bits through the host's libm pow, as f64::powf does
void agingradio_settings_to_job(const mi355_agingradio_settings &s, AgingJob *J) {
  J->flags = 0;
  J->p_int = 0;
  if (s.clicks_prob > 0.0f) {
    const double p = (double)s.clicks_prob;
    J->flags |= kAgingClick;
    J->p_int = p >= 1.0 ? ~0ull : (unsigned long long)(p * 18446744073709551616.0);
  }
  J->ampl = (double)s.white_noise_ampl;
  if (J->ampl > 0.0) J->flags |= kAgingNoise;
  J->factor = 1.0;
  if (s.bits_to_quantize > 0.0f) {
    J->flags |= kAgingQuant;
    J->factor = std::pow(2.0, (double)s.bits_to_quantize);
  }
  J->dist = (double)s.cubic_curve_distortion;
  J->passes = s.cubic_curve_passes;
  if (s.cubic_curve_distortion > 0.0f && s.cubic_curve_passes > 0) J->flags |= kAgingCubic;
}

static unsigned aging_blocks(unsigned long long n, int n_cu, unsigned jobs) {
  unsigned long long b = (n + 255) / 256;
  unsigned long long cap = (unsigned long long)n_cu * 8 / (jobs ? jobs : 1);
  if (cap < 1) cap = 1;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return (unsigned)b;
}

// h_jobs: the table on the host (what decides the grids); d_jobs: the same table in device memory, or nullptr for a table of
// one that travels in the kernel arguments.
int launch_agingradio_jobs(hipStream_t stream, int n_cu, const AgingJob *h_jobs, const AgingJob *d_jobs, unsigned n_jobs, std::string *err) {
  if (n_jobs == 0) return MI355_OK;
  unsigned long long widest = 0;
  bool any_tiled = false, any_stream = false;
  for (unsigned j = 0; j < n_jobs; j++) {
    if (h_jobs[j].frames < 2) continue;
    if (h_jobs[j].state) any_tiled = true;
    else {
      any_stream = true;
      const unsigned long long n = (h_jobs[j].frames / 2) * 2ull * h_jobs[j].channels;
      if (n > widest) widest = n;
    }
  }
  AgingJobSrc src;
  src.dev = d_jobs;
  src.inl = h_jobs[0];
  if (any_stream)
    hipLaunchKernelGGL(agingradio_stream_kernel, dim3(aging_blocks(widest, n_cu, n_jobs), n_jobs), dim3(256), 0, stream, src);
  if (any_tiled) hipLaunchKernelGGL(agingradio_tiled_kernel, dim3(1, n_jobs), dim3(256), 0, stream, src);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    if (err) *err = std::string("agingradio kernel launch: ") + hipGetErrorString(e);
    return MI355_ERR_HIP;
  }
  return MI355_OK;
}

struct AgingState {
  unsigned channels = 0;
  double alpha = 0;
  double *d_state = nullptr;       // channels f64 when the lowpass is on
  unsigned long long k = 0, seed = 0;
  void *d_stage = nullptr;         // host entry point's staging
  size_t stage_bytes = 0;
};

void agingradio_release(mi355_ctx *ctx) {
  auto *s = static_cast<AgingState *>(ctx->agingradio);
  if (!s) return;
  if (s->d_state) (void)hipFree(s->d_state);
  if (s->d_stage) (void)hipFree(s->d_stage);
  delete s;
  ctx->agingradio = nullptr;
}

static int aging_enqueue(mi355_ctx *ctx, AgingState *s, void *d_data, size_t frames, int is_f64, const mi355_agingradio_settings &set) {
  AgingJob J{};
  agingradio_settings_to_job(set, &J);
  J.data = d_data;
  J.state = s->d_state;
  J.frames = frames;
  J.k0 = s->k;
  J.seed = s->seed;
  J.alpha = s->alpha;
  J.channels = s->channels;
  J.is_f64 = is_f64 ? 1 : 0;
  std::string err;
  const int rc = launch_agingradio_jobs(ctx->stream, ctx->n_cu, &J, nullptr, 1, &err);
  if (rc) return set_error(ctx, rc, err);
  s->k += frames / 2;   // chunks_exact_mut: an odd last frame is not a pair and draws nothing
  return MI355_OK;
}

static int aging_check(mi355_ctx *ctx, const void *data, size_t frames, const mi355_agingradio_settings *set, AgingState **out) {
  if (!ctx) return MI355_ERR_INVALID_ARG;
  auto *s = static_cast<AgingState *>(ctx->agingradio);
  if (!s) return set_error(ctx, MI355_ERR_NOT_CONFIGURED, "agingradio: not negotiated (setup not called)");
  if (!set) return set_error(ctx, MI355_ERR_INVALID_ARG, "agingradio: null settings");
  if (frames && !data) return set_error(ctx, MI355_ERR_INVALID_ARG, "agingradio: null data");
  *out = s;
  return check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice");
}

}  // namespace mi355

using namespace mi355;

extern "C" {

int mi355_agingradio_setup(mi355_ctx *ctx, unsigned channels, unsigned rate, unsigned lowpass_freq, uint64_t seed) {
  if (!ctx) return MI355_ERR_INVALID_ARG;
  if (channels == 0 || rate == 0) return set_error(ctx, MI355_ERR_INVALID_ARG, "agingradio: 0 channels or rate 0");
  if (lowpass_freq > 0 && channels > kAgingTileSamples / 2)
    return set_error(ctx, MI355_ERR_UNSUPPORTED, "agingradio: the lowpass runs on at most 2048 channels");
  int rc = check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice");
  if (rc) return rc;
  (void)hipStreamSynchronize(ctx->stream);
  agingradio_release(ctx);
  auto *s = new AgingState();
  s->channels = channels;
  s->seed = seed;
  if (lowpass_freq > 0) {
    agingradio_setup_filter(rate, lowpass_freq, &s->alpha);
    if ((rc = check_hip(ctx, hipMalloc((void **)&s->d_state, (size_t)channels * sizeof(double)), "hipMalloc(agingradio filters)")) ||
        (rc = check_hip(ctx, hipMemsetAsync(s->d_state, 0, (size_t)channels * sizeof(double), ctx->stream), "hipMemset(agingradio filters)"))) {
      if (s->d_state) (void)hipFree(s->d_state);
      delete s;
      return rc;
    }
  }
  ctx->agingradio = s;
  return MI355_OK;
}

int mi355_agingradio_reset(mi355_ctx *ctx) {
  if (!ctx) return MI355_ERR_INVALID_ARG;
  int rc = check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice");
  if (rc) return rc;
  (void)hipStreamSynchronize(ctx->stream);
  agingradio_release(ctx);
  return MI355_OK;
}

int mi355_agingradio_process_device(mi355_ctx *ctx, void *d_data, size_t frames, int is_f64, const mi355_agingradio_settings *settings) {
  AgingState *s = nullptr;
  const int rc = aging_check(ctx, d_data, frames, settings, &s);
  if (rc) return rc;
  return aging_enqueue(ctx, s, d_data, frames, is_f64, *settings);
}

int mi355_agingradio_process(mi355_ctx *ctx, void *data, size_t frames, int is_f64, const mi355_agingradio_settings *settings) {
  AgingState *s = nullptr;
  int rc = aging_check(ctx, data, frames, settings, &s);
  if (rc) return rc;
  // only whole pairs are touched: the odd last frame stays in the caller's buffer
  const size_t bytes = (frames / 2) * 2 * (size_t)s->channels * (is_f64 ? 8 : 4);
  if (bytes == 0) return MI355_OK;
  if (s->stage_bytes < bytes) {
    if (s->d_stage) (void)hipFree(s->d_stage);
    s->d_stage = nullptr;
    s->stage_bytes = 0;
    if ((rc = check_hip(ctx, hipMalloc(&s->d_stage, bytes), "hipMalloc(agingradio staging)"))) return rc;
    s->stage_bytes = bytes;
  }
  if ((rc = check_hip(ctx, hipMemcpyAsync(s->d_stage, data, bytes, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync(H2D audio)"))) return rc;
  ctx->n_h2d++;
  if ((rc = aging_enqueue(ctx, s, s->d_stage, frames, is_f64, *settings))) return rc;
  if ((rc = check_hip(ctx, hipMemcpyAsync(data, s->d_stage, bytes, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync(D2H audio)"))) return rc;
  ctx->n_d2h++;
  return check_hip(ctx, hipStreamSynchronize(ctx->stream), "agingradio: stream synchronize");
}

int mi355_agingradio_get_state(mi355_ctx *ctx, double *filter_state, unsigned channels, uint64_t *pairs_done) {
  if (!ctx) return MI355_ERR_INVALID_ARG;
  auto *s = static_cast<AgingState *>(ctx->agingradio);
  if (!s) return set_error(ctx, MI355_ERR_NOT_CONFIGURED, "agingradio: not negotiated (setup not called)");
  int rc = check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice");
  if (rc) return rc;
  if ((rc = check_hip(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize"))) return rc;
  if (pairs_done) *pairs_done = s->k;
  if (filter_state && channels) {
    const unsigned n = channels < s->channels ? channels : s->channels;
    if (!s->d_state) std::memset(filter_state, 0, (size_t)n * sizeof(double));
    else if ((rc = check_hip(ctx, hipMemcpy(filter_state, s->d_state, (size_t)n * sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy(agingradio filters)")))
      return rc;
  }
  return MI355_OK;
}

}  // extern "C"
