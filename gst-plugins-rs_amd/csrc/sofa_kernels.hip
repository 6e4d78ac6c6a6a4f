// sofa_kernels.hip — gfx950 kernels for `sofalizer`: uniformly partitioned FFT convolution of every input channel with
// its head-related impulse-response pair, mixed to stereo.
//
// Reference path replaced: the per-block loop of Sofalizer::process (audio/hrtf/src/sofa/imp.rs:234-300): per input block
// of `block-length` frames and per channel that is not dropped (LFE1 / LFE2 are ChannelProcessor::Drop, :808-821) the
// channel is de-interleaved (:250-256), run through the third-party crate sofar's `Renderer::process_block` (built with
// `partition-length`, :793-798; the block length must be a multiple of it, :775-781) and mixed
// `out[2i] += l * gain; out[2i+1] += r * gain` in channel order (:282-297). Which HRIR pair a channel uses is decided on
// the host (Sofar::filter lookup in the SOFA file, State::update_filters :129-160) and handed over with
// mi355_sofa_set_filter: reading SOFA/HDF5 files is not part of the per-buffer path.
// sofar's sources are not in the reference tree (Cargo dependency `sofar`, features "dsp"): PARITY UNPINNED. What a
// uniformly partitioned convolver computes is a streaming linear convolution, y = x * h per ear, with h changing at block
// boundaries; that is the contract here, checked against a time-domain oracle (oracle/oracle.py: SofaRenderer) within 2e-6 of
// full scale (f32 FFT round-off), not bit for bit.
//
// Algorithm (uniformly partitioned overlap-save, partition P, FFT size N = 2P, K = ceil(L / P) filter partitions):
//   per sub-block j of P input samples:  X_j = FFT([x_{j-1} | x_j]);  Y = sum_k X_{j-k} . H_k;  y_j = IFFT(Y)[P .. 2P)
// One workgroup per channel walks the B / P sub-blocks of a block: the 2P-point transforms run in LDS (radix-2, all lanes
// of the workgroup on N/2 butterflies per stage, twiddles from an LDS table), the frequency-domain delay line (K spectra
// per channel) lives in global memory (L2-resident: K * N * 8 B per channel), the two ears share X.
#include "audio_fft.hpp"
#include "internal.hpp"

#include <cmath>
#include <cstring>
#include <vector>

namespace mi355 {

struct SofaState {
  int channels = 0, filter_len = 0, P = 0, B = 0, K = 0, N = 0, logN = 0;
  float2 *d_H = nullptr;     // [C][2][K][N] filter partition spectra
  float2 *d_fdl = nullptr;   // [C][K][N] spectra of the last K input windows (ring, slot = sub-block counter mod K)
  float *d_prev = nullptr;   // [C][P] previous sub-block of every channel
  float *d_partial = nullptr;  // [C][B][2]
  float *d_in = nullptr, *d_out = nullptr;  // staging for the host entry point
  float *d_gain = nullptr;   // [C]
  float *d_taps = nullptr;   // [2][K*P] staging for set_filter
  int *d_drop = nullptr;     // [C]
  std::vector<int> drop;
  std::vector<unsigned char> have_filter;
  unsigned long long counter = 0;  // sub-blocks processed (FDL write slot = counter mod K)
};
static SofaState *sofa_of(mi355_ctx *ctx) { return (SofaState *)ctx->sofa; }

// cmul, bitrev and the transform in LDS (fft_lds, its lanes striding by blockDim.x here) are audio_fft.hpp's.
// The bodies below are shared by the lone kernels (one context, one instance) and the job-table kernels of a sofa agroup further
// down: a member of a group computes what a lone context computes, bit for bit, because it runs the same statements.

// spectrum of partition k of one ear of one filter: taps[2][K*P] zero padded -> H[2][K][N]. sm: [N] buffer + [N/2] twiddles
__device__ __forceinline__ void sofa_filter_fft_body(float2 *sm, const float *__restrict__ taps, float2 *__restrict__ H, int P, int K, int N, int logN, int k,
                                                     int ear) {
  float2 *buf = sm, *tw = sm + N;
  for (int i = threadIdx.x; i < N / 2; i += blockDim.x) {
    float s, c;
    sincospif(-2.0f * (float)i / (float)N, &s, &c);
    tw[i] = make_float2(c, s);
  }
  for (int i = threadIdx.x; i < N; i += blockDim.x) buf[bitrev(i, logN)] = make_float2(i < P ? taps[(size_t)ear * K * P + (size_t)k * P + i] : 0.0f, 0.0f);
  fft_lds<false, kLanesBlockDim>(buf, tw, N, logN);
  for (int i = threadIdx.x; i < N; i += blockDim.x) H[((size_t)ear * K + k) * N + i] = buf[i];
}

// `nsub` consecutive sub-blocks of P samples of ONE channel: in[i * in_stride] is its sample i, H [2][K][N], F [K][N] and pv [P] are the
// channel's own, out [nsub * P][2] its partial output. Between sub-blocks - and between blocks - the convolver carries F, pv and the slot
// counter only, so nsub = n * B / P is n blocks of B in a row. sm: [N] X, [N] Yl, [N] Yr, [N/2] twiddles
__device__ __forceinline__ void sofa_convolve_body(float2 *sm, const float *__restrict__ in, size_t in_stride, const float2 *__restrict__ H,
                                                   float2 *__restrict__ F, float *__restrict__ pv, float *__restrict__ out, int P, int nsub, int K, int N,
                                                   int logN, unsigned slot0) {
  float2 *X = sm, *Yl = sm + N, *Yr = sm + 2 * N, *tw = sm + 3 * N;
  for (int i = threadIdx.x; i < N / 2; i += blockDim.x) {
    float s, co;
    sincospif(-2.0f * (float)i / (float)N, &s, &co);
    tw[i] = make_float2(co, s);
  }
  const float2 *Hl = H, *Hr = Hl + (size_t)K * N;
  const float inv_n = 1.0f / (float)N;
  for (int j = 0; j < nsub; j++) {
    const unsigned slot = (slot0 + (unsigned)j) % (unsigned)K;
    __syncthreads();
    // window [previous sub-block | this sub-block], stored bit-reversed for the in-place transform
    for (int i = threadIdx.x; i < N; i += blockDim.x) {
      const float v = i < P ? pv[i] : in[(size_t)(j * P + i - P) * in_stride];  // de-interleave (sofa/imp.rs:257-263)
      X[bitrev(i, logN)] = make_float2(v, 0.0f);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < P; i += blockDim.x) pv[i] = in[(size_t)(j * P + i) * in_stride];
    fft_lds<false, kLanesBlockDim>(X, tw, N, logN);
    for (int i = threadIdx.x; i < N; i += blockDim.x) F[(size_t)slot * N + i] = X[i];
    __syncthreads();
    // Y = sum_k X_{j-k} . H_k, partitions in ascending k (fixed order: deterministic)
    for (int i = threadIdx.x; i < N; i += blockDim.x) {
      float2 al = make_float2(0.0f, 0.0f), ar = al;
      for (int k = 0; k < K; k++) {
        const unsigned s = (slot + (unsigned)K - (unsigned)k) % (unsigned)K;
        const float2 x = k == 0 ? X[i] : F[(size_t)s * N + i];
        const float2 pl = cmul(x, Hl[(size_t)k * N + i]), pr = cmul(x, Hr[(size_t)k * N + i]);
        al.x += pl.x; al.y += pl.y; ar.x += pr.x; ar.y += pr.y;
      }
      Yl[bitrev(i, logN)] = al;
      Yr[bitrev(i, logN)] = ar;
    }
    fft_lds<true, kLanesBlockDim>(Yl, tw, N, logN);
    fft_lds<true, kLanesBlockDim>(Yr, tw, N, logN);
    for (int i = threadIdx.x; i < P; i += blockDim.x) {  // overlap-save: the last P samples are the valid ones
      out[(size_t)(j * P + i) * 2 + 0] = Yl[P + i].x * inv_n;
      out[(size_t)(j * P + i) * 2 + 1] = Yr[P + i].x * inv_n;
    }
  }
}

// out[i] = ((0 + l_0 * g_0) + l_1 * g_1) + ... over the channels that are not dropped, in channel order: the accumulation order of
// Sofalizer::process (sofa/imp.rs:215 zero fill, :302-319 `y[0] += l * gain; y[1] += r * gain` per Render processor in vector order).
// partial [C][row] with row = 2 * frames interleaved samples, i < row
__device__ __forceinline__ void sofa_mix_body(const float *__restrict__ partial, const float *__restrict__ gain, const int *__restrict__ drop,
                                              float *__restrict__ out, int C, size_t row, size_t i) {
  float acc = 0.0f;
  for (int c = 0; c < C; c++) {
    if (drop[c]) continue;
    acc += partial[(size_t)c * row + i] * gain[c];
  }
  out[i] = acc;
}

// spectra of one channel's filter partitions: grid (K, 2 ears), taps[ear][K*P] zero padded
__global__ __launch_bounds__(256) void sofa_filter_fft_kernel(const float *__restrict__ taps, float2 *__restrict__ H, int P, int K, int N, int logN) {
  extern __shared__ float2 sm[];  // [N] buffer + [N/2] twiddles
  sofa_filter_fft_body(sm, taps, H, P, K, N, logN, blockIdx.x, blockIdx.y);
}

// one workgroup per channel: the B / P sub-blocks of one input block
__global__ __launch_bounds__(256) void sofa_convolve_kernel(const float *__restrict__ in, int C, const float2 *__restrict__ H, float2 *__restrict__ fdl,
                                                            float *__restrict__ prev, float *__restrict__ partial, const int *__restrict__ drop,
                                                            int P, int B, int K, int N, int logN, unsigned slot0) {
  extern __shared__ float2 sm[];  // [N] X, [N] Yl, [N] Yr, [N/2] twiddles
  const int c = blockIdx.x;
  float *out = partial + (size_t)c * B * 2;
  if (drop[c]) {  // ChannelProcessor::Drop contributes nothing (sofa/imp.rs:253-255)
    for (int i = threadIdx.x; i < 2 * B; i += blockDim.x) out[i] = 0.0f;
    return;
  }
  sofa_convolve_body(sm, in + c, (size_t)C, H + (size_t)c * 2 * K * N, fdl + (size_t)c * K * N, prev + (size_t)c * P, out, P, B / P, K, N, logN, slot0);
}

// the channel-ordered mix of one block (sofa_mix_body)
__global__ __launch_bounds__(256) void sofa_mix_kernel(const float *__restrict__ partial, const float *__restrict__ gain, const int *__restrict__ drop,
                                                       float *__restrict__ out, int C, int B) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 2 * B) return;
  sofa_mix_body(partial, gain, drop, out, C, (size_t)2 * B, (size_t)i);
}

// ------------------------------------------------------------------ the job-table form (sofa agroups, agroup.hip)
// Independent sofalizer instances - own channel count, filter length, partition-length and block-length each - in ONE launch set.
// One table travels per set: an entry per member that has submitted (its mix), a row per (member, channel) that is not dropped (its
// convolution; a dropped channel has no row: nothing runs for it and the mix skips it) and a row per filter that is pending among
// those members. Rows of one partition length lie together: a launch serves ONE partition length, so that its dynamic LDS,
// (3N + N/2) * sizeof(float2), fits every block in it and a P = 8 member does not inherit the 112 KiB of a P = 2048 neighbour.
struct SofaJobMember {
  const float *partial; float *out;
  const int *drop;       // [C], the member's own (fixed before its first block)
  int C, pad_;
  unsigned long long row;  // 2 * frames of this submit
  float gain[64];        // copied at submit
};
struct SofaJobConv {
  const float *in; const float2 *H; float2 *fdl; float *prev; float *partial;
  unsigned long long in_stride;
  int P, nsub, K, N, logN;
  unsigned slot0;
};
struct SofaJobFilter { const float *taps; float2 *H; int P, K, N, logN; };

// grid (rows of one partition length); rows = the first of them
__global__ __launch_bounds__(256) void sofa_convolve_jobs_kernel(const SofaJobConv *__restrict__ rows) {
  extern __shared__ float2 sm[];
  const SofaJobConv J = rows[blockIdx.x];
  sofa_convolve_body(sm, J.in, (size_t)J.in_stride, J.H, J.fdl, J.prev, J.partial, J.P, J.nsub, J.K, J.N, J.logN, J.slot0);
}

// grid (filters of one partition length * ky, 2 ears), ky = the most partitions among them; a block beyond its filter's K leaves at
// once (as a whole: nobody is left at a barrier)
__global__ __launch_bounds__(256) void sofa_filter_fft_jobs_kernel(const SofaJobFilter *__restrict__ rows, int ky) {
  extern __shared__ float2 sm[];
  const int f = blockIdx.x / ky, k = blockIdx.x - f * ky;
  const SofaJobFilter J = rows[f];
  if (k >= J.K) return;
  sofa_filter_fft_body(sm, J.taps, J.H, J.P, J.K, J.N, J.logN, k, blockIdx.y);
}

// grid (blocks of the longest output, members)
__global__ __launch_bounds__(256) void sofa_mix_jobs_kernel(const SofaJobMember *__restrict__ members) {
  const SofaJobMember *M = members + blockIdx.y;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= M->row) return;
  sofa_mix_body(M->partial, M->gain, M->drop, M->out, M->C, (size_t)M->row, i);
}

// ------------------------------------------------------------------ host side

void sofa_release(mi355_ctx *ctx) {
  SofaState *S = sofa_of(ctx);
  if (!S) return;
  void *ptrs[] = {S->d_H, S->d_fdl, S->d_prev, S->d_partial, S->d_in, S->d_out, S->d_gain, S->d_taps, S->d_drop};
  for (void *p : ptrs) if (p) (void)hipFree(p);
  delete S;
  ctx->sofa = nullptr;
}

int sofa_setup(mi355_ctx *ctx, int channels, int filter_len, int partition_len, int block_len) {
  sofa_release(ctx);
  if (channels < 1 || channels > 64) return set_error(ctx, MI355_ERR_INVALID_ARG, "sofalizer: bad channel count");
  if (filter_len < 1 || filter_len > (1 << 20)) return set_error(ctx, MI355_ERR_INVALID_ARG, "sofalizer: bad filter length");
  if (partition_len < 1 || partition_len > 65535 || block_len < 1 || block_len > 65535)  // property ranges, sofa/imp.rs:384-397
    return set_error(ctx, MI355_ERR_INVALID_ARG, "sofalizer: partition / block length out of range");
  if (block_len % partition_len != 0) return set_error(ctx, MI355_ERR_INVALID_ARG, "Block Length is not multiple of Partition Length");  // :775-781
  if ((partition_len & (partition_len - 1)) != 0 || partition_len < 8 || partition_len > 2048)
    return set_error(ctx, MI355_ERR_UNSUPPORTED, "sofalizer: partition length must be a power of two in 8..2048 (radix-2 transforms in LDS)");
  SofaState *S = new SofaState();
  ctx->sofa = S;
  S->channels = channels; S->filter_len = filter_len; S->P = partition_len; S->B = block_len;
  S->K = (filter_len + partition_len - 1) / partition_len;
  S->N = 2 * partition_len;
  S->logN = 0;
  while ((1 << S->logN) < S->N) S->logN++;
  S->drop.assign(channels, 0);
  S->have_filter.assign(channels, 0);
  const size_t C = channels, K = S->K, N = S->N;
  int rc;
#define MI355_SOFA_ALLOC(p, bytes, what) if ((rc = check_hip(ctx, hipMalloc((void **)&(p), (bytes)), what))) return rc; \
  if ((rc = check_hip(ctx, hipMemsetAsync((p), 0, (bytes), ctx->stream), what))) return rc;
  MI355_SOFA_ALLOC(S->d_H, C * 2 * K * N * sizeof(float2), "hipMalloc(sofalizer filter spectra)")
  MI355_SOFA_ALLOC(S->d_fdl, C * K * N * sizeof(float2), "hipMalloc(sofalizer delay line)")
  MI355_SOFA_ALLOC(S->d_prev, C * S->P * sizeof(float), "hipMalloc(sofalizer history)")
  MI355_SOFA_ALLOC(S->d_partial, C * S->B * 2 * sizeof(float), "hipMalloc(sofalizer partial outputs)")
  MI355_SOFA_ALLOC(S->d_in, C * S->B * sizeof(float), "hipMalloc(sofalizer input)")
  MI355_SOFA_ALLOC(S->d_out, (size_t)S->B * 2 * sizeof(float), "hipMalloc(sofalizer output)")
  MI355_SOFA_ALLOC(S->d_gain, C * sizeof(float), "hipMalloc(sofalizer gains)")
  MI355_SOFA_ALLOC(S->d_taps, 2 * K * S->P * sizeof(float), "hipMalloc(sofalizer taps)")
  MI355_SOFA_ALLOC(S->d_drop, C * sizeof(int), "hipMalloc(sofalizer drop flags)")
#undef MI355_SOFA_ALLOC
  return check_hip(ctx, hipStreamSynchronize(ctx->stream), "sofalizer: stream synchronize");
}

// Renderer::set_filter for one channel: FIR pair of filter_len taps and whole-sample onset delays (>= 0) that are folded
// into the taps; the pair takes effect with the next block. Taps beyond filter_len after the delay are cut.
int sofa_set_filter(mi355_ctx *ctx, int channel, const float *left, const float *right, int delay_left, int delay_right) {
  SofaState *S = sofa_of(ctx);
  if (!S) return set_error(ctx, MI355_ERR_NOT_CONFIGURED, "sofalizer: not configured");
  if (channel < 0 || channel >= S->channels || !left || !right || delay_left < 0 || delay_right < 0)
    return set_error(ctx, MI355_ERR_INVALID_ARG, "sofalizer: bad filter argument");
  const size_t KP = (size_t)S->K * S->P;
  std::vector<float> taps(2 * KP, 0.0f);
  for (int e = 0; e < 2; e++) {
    const float *h = e ? right : left;
    const int d = e ? delay_right : delay_left;
    for (int i = 0; i + d < S->filter_len; i++) taps[e * KP + (size_t)(i + d)] = h[i];
  }
  int rc = check_hip(ctx, hipMemcpyAsync(S->d_taps, taps.data(), taps.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync(sofalizer taps)");
  if (rc) return rc;
  const size_t lds = ((size_t)S->N + S->N / 2) * sizeof(float2);
  hipLaunchKernelGGL(sofa_filter_fft_kernel, dim3(S->K, 2), dim3(256), lds, ctx->stream, (const float *)S->d_taps,
                     S->d_H + (size_t)channel * 2 * S->K * S->N, S->P, S->K, S->N, S->logN);
  if ((rc = check_hip(ctx, hipGetLastError(), "sofalizer filter kernel launch"))) return rc;
  S->have_filter[channel] = 1;
  return check_hip(ctx, hipStreamSynchronize(ctx->stream), "sofalizer: stream synchronize");  // `taps` is host memory of this call
}

int sofa_set_drop(mi355_ctx *ctx, int channel, int drop) {
  SofaState *S = sofa_of(ctx);
  if (!S) return set_error(ctx, MI355_ERR_NOT_CONFIGURED, "sofalizer: not configured");
  if (channel < 0 || channel >= S->channels) return set_error(ctx, MI355_ERR_INVALID_ARG, "sofalizer: bad channel");
  // the element fixes Drop per channel when it negotiates and never toggles it; a channel that came back in mid-run would find
  // a delay line that stopped at some earlier sub-block, so the flags are fixed once a block has run (until reset or setup)
  if (S->counter != 0) return set_error(ctx, MI355_ERR_INVALID_ARG, "sofalizer: drop flags are fixed once a block has been processed (reset first)");
  S->drop[channel] = drop ? 1 : 0;
  return check_hip(ctx, hipMemcpy(S->d_drop, S->drop.data(), S->drop.size() * sizeof(int), hipMemcpyHostToDevice), "hipMemcpy(sofalizer drop flags)");
}

// ChannelProcessor::reset (flush-stop, sofa/imp.rs:840-848): the input history goes, the filters stay until the element sets new ones
int sofa_reset(mi355_ctx *ctx) {
  SofaState *S = sofa_of(ctx);
  if (!S) return set_error(ctx, MI355_ERR_NOT_CONFIGURED, "sofalizer: not configured");
  int rc = check_hip(ctx, hipMemsetAsync(S->d_fdl, 0, (size_t)S->channels * S->K * S->N * sizeof(float2), ctx->stream), "hipMemset(sofalizer delay line)");
  if (rc) return rc;
  rc = check_hip(ctx, hipMemsetAsync(S->d_prev, 0, (size_t)S->channels * S->P * sizeof(float), ctx->stream), "hipMemset(sofalizer history)");
  S->counter = 0;
  return rc;
}

int sofa_process_block_device(mi355_ctx *ctx, const float *d_in, float *d_out, const float *gains) {
  SofaState *S = sofa_of(ctx);
  if (!S) return set_error(ctx, MI355_ERR_NOT_CONFIGURED, "sofalizer: not configured");
  for (int c = 0; c < S->channels; c++)
    if (!S->drop[c] && !S->have_filter[c]) return set_error(ctx, MI355_ERR_NOT_CONFIGURED, "sofalizer: a channel has no filter yet");
  int rc = check_hip(ctx, hipMemcpyAsync(S->d_gain, gains, (size_t)S->channels * sizeof(float), hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync(sofalizer gains)");
  if (rc) return rc;
  const size_t lds = (3 * (size_t)S->N + S->N / 2) * sizeof(float2);
  // partition 2048 needs 112 KiB, above the default limit: a refused request must not reach the launch
  if ((rc = check_hip(ctx, hipFuncSetAttribute((const void *)sofa_convolve_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds), "hipFuncSetAttribute(sofalizer convolve LDS)"))) return rc;
  hipLaunchKernelGGL(sofa_convolve_kernel, dim3(S->channels), dim3(256), lds, ctx->stream, d_in, S->channels, (const float2 *)S->d_H, S->d_fdl, S->d_prev,
                     S->d_partial, (const int *)S->d_drop, S->P, S->B, S->K, S->N, S->logN, (unsigned)(S->counter % (unsigned long long)S->K));
  hipLaunchKernelGGL(sofa_mix_kernel, dim3((2 * S->B + 255) / 256), dim3(256), 0, ctx->stream, (const float *)S->d_partial, (const float *)S->d_gain,
                     (const int *)S->d_drop, d_out, S->channels, S->B);
  S->counter += (unsigned long long)(S->B / S->P);
  if ((rc = check_hip(ctx, hipGetLastError(), "sofalizer kernel launch"))) return rc;
  return check_hip(ctx, hipStreamSynchronize(ctx->stream), "sofalizer: stream synchronize");  // `gains` is host memory of this call
}

int sofa_process_block_host(mi355_ctx *ctx, const float *in, float *out, const float *gains) {
  SofaState *S = sofa_of(ctx);
  if (!S) return set_error(ctx, MI355_ERR_NOT_CONFIGURED, "sofalizer: not configured");
  int rc = check_hip(ctx, hipMemcpyAsync(S->d_in, in, (size_t)S->channels * S->B * sizeof(float), hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync(sofalizer input)");
  if (rc) return rc;
  if ((rc = sofa_process_block_device(ctx, S->d_in, S->d_out, gains))) return rc;
  if ((rc = check_hip(ctx, hipMemcpyAsync(out, S->d_out, (size_t)S->B * 2 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync(sofalizer output)"))) return rc;
  return check_hip(ctx, hipStreamSynchronize(ctx->stream), "sofalizer: stream synchronize");
}

// ------------------------------------------------------------------ the members of one sofa agroup
// The dispatcher (agroup.hip) collects the submissions and owns the stream and the staging slabs; what a sofalizer instance IS - its
// filter spectra, delay lines, drop flags and sub-block counter - lives here, next to the lone context's. Every function below is
// called with the group's lock held.
struct SofaMember {
  bool configured = false;
  int channels = 0, filter_len = 0, P = 0, B = 0, K = 0, N = 0, logN = 0;
  float2 *d_H = nullptr;      // [C][2][K][N]
  float2 *d_fdl = nullptr;    // [C][K][N]
  float *d_prev = nullptr;    // [C][P]
  float *d_partial = nullptr; // [C][kSofaMaxBlocks * B][2]: a submit of n blocks uses rows of n * B frames
  int *d_drop = nullptr;      // [C]
  std::vector<int> drop;
  std::vector<unsigned char> have_filter;      // [C]: d_H holds a transformed filter
  std::vector<std::vector<float>> pending;     // [C]: taps [2][K*P] (onset delays folded in) set and not transformed yet; empty = none
  int n_pending = 0;
  unsigned long long counter = 0;              // sub-blocks processed
};

struct SofaGroup {
  std::vector<SofaMember> members;
  // the table of the launch set: pinned block + device block, [member entries][convolution rows][filter rows], sized at setup for
  // every configured member at once; the taps slab: pinned + device, sized at set_filter for everything pending at once. ev: the
  // previous set's table and taps have left the pinned blocks
  char *h_tab = nullptr, *d_tab = nullptr;
  size_t tab_rows = 0;        // channels of all configured members the blocks are sized for
  float *h_slab = nullptr, *d_slab = nullptr;
  size_t slab_floats = 0;
  hipEvent_t ev = nullptr;
  uint64_t n_launches = 0;
};

static size_t sofa_align16(size_t v) { return (v + 15) & ~(size_t)15; }
static size_t sofa_conv_offset(const SofaGroup *G) { return sofa_align16(G->members.size() * sizeof(SofaJobMember)); }
static size_t sofa_filter_offset(const SofaGroup *G, size_t rows) { return sofa_conv_offset(G) + sofa_align16(rows * sizeof(SofaJobConv)); }
static size_t sofa_tab_bytes(const SofaGroup *G, size_t rows) { return sofa_filter_offset(G, rows) + sofa_align16(rows * sizeof(SofaJobFilter)); }

SofaGroup *sofa_group_new(int n_members, std::string *err, int *status) {
  SofaGroup *G = new SofaGroup();
  G->members.resize((size_t)n_members);
  *status = audio_hip(hipEventCreateWithFlags(&G->ev, hipEventDisableTiming), "hipEventCreate(sofa group)", err);
  if (*status) { delete G; return nullptr; }
  return G;
}

static void sofa_member_free(SofaMember *M) {
  void *ptrs[] = {M->d_H, M->d_fdl, M->d_prev, M->d_partial, M->d_drop};
  for (void *p : ptrs) if (p) (void)hipFree(p);
  *M = SofaMember{};
}

void sofa_group_free(SofaGroup *G) {
  if (!G) return;
  for (SofaMember &M : G->members) sofa_member_free(&M);
  if (G->h_tab) (void)hipHostFree(G->h_tab);
  if (G->d_tab) (void)hipFree(G->d_tab);
  if (G->h_slab) (void)hipHostFree(G->h_slab);
  if (G->d_slab) (void)hipFree(G->d_slab);
  if (G->ev) (void)hipEventDestroy(G->ev);
  delete G;
}

// set_caps of one member (sofa/imp.rs:747-838): the checks and messages of sofa_setup. Everything the member and the launch sets it
// will take part in need is allocated HERE, after the stream has drained (nothing in flight reads what is replaced): a launch set
// allocates nothing.
int sofa_group_setup(SofaGroup *G, int m, hipStream_t stream, int channels, int filter_len, int partition_len, int block_len, std::string *err) {
  if (channels < 1 || channels > 64) return audio_fail(MI355_ERR_INVALID_ARG, "sofalizer: bad channel count", err);
  if (filter_len < 1 || filter_len > (1 << 20)) return audio_fail(MI355_ERR_INVALID_ARG, "sofalizer: bad filter length", err);
  if (partition_len < 1 || partition_len > 65535 || block_len < 1 || block_len > 65535)  // property ranges
    return audio_fail(MI355_ERR_INVALID_ARG, "sofalizer: partition / block length out of range", err);
  if (block_len % partition_len != 0) return audio_fail(MI355_ERR_INVALID_ARG, "Block Length is not multiple of Partition Length", err);  // :779-784
  if ((partition_len & (partition_len - 1)) != 0 || partition_len < 8 || partition_len > 2048)
    return audio_fail(MI355_ERR_UNSUPPORTED, "sofalizer: partition length must be a power of two in 8..2048 (radix-2 transforms in LDS)", err);
  int rc;
  if ((rc = audio_hip(hipStreamSynchronize(stream), "sofa group: stream synchronize", err))) return rc;
  SofaMember *M = &G->members[(size_t)m];
  sofa_member_free(M);
  M->channels = channels; M->filter_len = filter_len; M->P = partition_len; M->B = block_len;
  M->K = (filter_len + partition_len - 1) / partition_len;
  M->N = 2 * partition_len;
  while ((1 << M->logN) < M->N) M->logN++;
  M->drop.assign((size_t)channels, 0);
  M->have_filter.assign((size_t)channels, 0);
  M->pending.assign((size_t)channels, std::vector<float>());
  const size_t C = (size_t)channels, K = (size_t)M->K, N = (size_t)M->N;
#define MI355_SOFA_GALLOC(p, bytes, what) if ((rc = audio_hip(hipMalloc((void **)&(p), (bytes)), what, err)) || \
                                              (rc = audio_hip(hipMemsetAsync((p), 0, (bytes), stream), what, err))) { sofa_member_free(M); return rc; }
  MI355_SOFA_GALLOC(M->d_H, C * 2 * K * N * sizeof(float2), "hipMalloc(sofa group filter spectra)")
  MI355_SOFA_GALLOC(M->d_fdl, C * K * N * sizeof(float2), "hipMalloc(sofa group delay line)")
  MI355_SOFA_GALLOC(M->d_prev, C * (size_t)M->P * sizeof(float), "hipMalloc(sofa group history)")
  MI355_SOFA_GALLOC(M->d_partial, C * (size_t)kSofaMaxBlocks * (size_t)M->B * 2 * sizeof(float), "hipMalloc(sofa group partial outputs)")
  MI355_SOFA_GALLOC(M->d_drop, C * sizeof(int), "hipMalloc(sofa group drop flags)")
#undef MI355_SOFA_GALLOC
  // the table blocks hold a row per channel of every configured member, this one included
  size_t rows = C;
  for (const SofaMember &o : G->members) if (o.configured) rows += (size_t)o.channels;
  if (rows > G->tab_rows) {
    if (G->h_tab) (void)hipHostFree(G->h_tab);
    if (G->d_tab) (void)hipFree(G->d_tab);
    G->h_tab = G->d_tab = nullptr; G->tab_rows = 0;
    size_t cap = 64;
    while (cap < rows) cap *= 2;
    const size_t bytes = sofa_tab_bytes(G, cap);
    if ((rc = audio_hip(hipHostMalloc((void **)&G->h_tab, bytes, hipHostMallocDefault), "hipHostMalloc(sofa group tables)", err)) ||
        (rc = audio_hip(hipMalloc((void **)&G->d_tab, bytes), "hipMalloc(sofa group tables)", err))) { sofa_member_free(M); return rc; }
    G->tab_rows = cap;
  }
  if ((rc = audio_hip(hipStreamSynchronize(stream), "sofa group: stream synchronize", err))) { sofa_member_free(M); return rc; }
  M->configured = true;
  return MI355_OK;
}

// Renderer::set_filter of one channel (State::update_filters, sofa/imp.rs:129-160), queued: the taps are copied now, the onset delays
// folded in as sofa_set_filter folds them; the transform runs with the member's next launch set. A filter still pending for the
// channel is replaced. Nothing is launched and nothing is waited for, unless the taps slab has to grow to hold everything that is
// pending in the group (then the stream drains first, as for the staging slabs: it is never replaced under a launch).
int sofa_group_set_filter(SofaGroup *G, int m, hipStream_t stream, int channel, const float *left, const float *right, int delay_left, int delay_right,
                          std::string *err) {
  SofaMember *M = &G->members[(size_t)m];
  if (!M->configured) return audio_fail(MI355_ERR_NOT_CONFIGURED, "sofalizer: not configured", err);
  if (channel < 0 || channel >= M->channels || !left || !right || delay_left < 0 || delay_right < 0)
    return audio_fail(MI355_ERR_INVALID_ARG, "sofalizer: bad filter argument", err);
  const size_t KP = (size_t)M->K * M->P;
  size_t need = 0;
  for (const SofaMember &o : G->members) need += (size_t)o.n_pending * 2 * (size_t)o.K * (size_t)o.P;
  if (M->pending[(size_t)channel].empty()) need += 2 * KP;
  if (need > G->slab_floats) {
    int rc;
    if ((rc = audio_hip(hipStreamSynchronize(stream), "sofa group: stream synchronize", err))) return rc;
    size_t cap = 4096;
    while (cap < need && cap < ((size_t)1 << 20)) cap *= 2;
    if (cap < need) cap = (need + 4095) & ~(size_t)4095;
    float *h = nullptr, *d = nullptr;
    if ((rc = audio_hip(hipHostMalloc((void **)&h, cap * sizeof(float), hipHostMallocDefault), "hipHostMalloc(sofa group taps)", err))) return rc;
    if ((rc = audio_hip(hipMalloc((void **)&d, cap * sizeof(float)), "hipMalloc(sofa group taps)", err))) { (void)hipHostFree(h); return rc; }
    if (G->h_slab) (void)hipHostFree(G->h_slab);
    if (G->d_slab) (void)hipFree(G->d_slab);
    G->h_slab = h; G->d_slab = d; G->slab_floats = cap;
  }
  std::vector<float> &taps = M->pending[(size_t)channel];
  if (taps.empty()) M->n_pending++;
  taps.assign(2 * KP, 0.0f);
  for (int e = 0; e < 2; e++) {
    const float *h = e ? right : left;
    const int d = e ? delay_right : delay_left;
    for (int i = 0; i + d < M->filter_len; i++) taps[(size_t)e * KP + (size_t)(i + d)] = h[i];
  }
  return MI355_OK;
}

int sofa_group_set_drop(SofaGroup *G, int m, hipStream_t stream, int channel, int drop, std::string *err) {
  SofaMember *M = &G->members[(size_t)m];
  if (!M->configured) return audio_fail(MI355_ERR_NOT_CONFIGURED, "sofalizer: not configured", err);
  if (channel < 0 || channel >= M->channels) return audio_fail(MI355_ERR_INVALID_ARG, "sofalizer: bad channel", err);
  if (M->counter != 0) return audio_fail(MI355_ERR_INVALID_ARG, "sofalizer: drop flags are fixed once a block has been processed (reset first)", err);
  M->drop[(size_t)channel] = drop ? 1 : 0;
  int rc = audio_hip(hipMemcpyAsync(M->d_drop, M->drop.data(), M->drop.size() * sizeof(int), hipMemcpyHostToDevice, stream), "hipMemcpyAsync(sofa group drop flags)", err);
  if (rc) return rc;
  return audio_hip(hipStreamSynchronize(stream), "sofa group: stream synchronize", err);   // (M->drop may change again at once)
}

// ChannelProcessor::reset of every channel (sofa/imp.rs:84-90, :123-127; flush-stop :846-853): the input history goes, the filters -
// transformed and pending alike - stay. On the group's stream: after the member's last launch set, before its next.
int sofa_group_reset(SofaGroup *G, int m, hipStream_t stream, std::string *err) {
  SofaMember *M = &G->members[(size_t)m];
  if (!M->configured) return audio_fail(MI355_ERR_NOT_CONFIGURED, "sofalizer: not configured", err);
  int rc = audio_hip(hipMemsetAsync(M->d_fdl, 0, (size_t)M->channels * M->K * M->N * sizeof(float2), stream), "hipMemset(sofa group delay line)", err);
  if (rc) return rc;
  rc = audio_hip(hipMemsetAsync(M->d_prev, 0, (size_t)M->channels * M->P * sizeof(float), stream), "hipMemset(sofa group history)", err);
  M->counter = 0;
  return rc;
}

bool sofa_group_configured(const SofaGroup *G, int m) { return G->members[(size_t)m].configured; }
int sofa_group_channels(const SofaGroup *G, int m) { return G->members[(size_t)m].channels; }
int sofa_group_block(const SofaGroup *G, int m) { return G->members[(size_t)m].B; }
uint64_t sofa_group_launches(const SofaGroup *G) { return G->n_launches; }

// every channel that is not dropped has a filter, transformed or pending (what sofa_process_block_device asks of a lone context)
bool sofa_group_ready(const SofaGroup *G, int m) {
  const SofaMember &M = G->members[(size_t)m];
  for (int c = 0; c < M.channels; c++)
    if (!M.drop[(size_t)c] && !M.have_filter[(size_t)c] && M.pending[(size_t)c].empty()) return false;
  return true;
}

int sofa_group_info(const SofaGroup *G, int m, int *partitions_K, int *fft_n, int *pending_filters, std::string *err) {
  const SofaMember &M = G->members[(size_t)m];
  if (!M.configured) return audio_fail(MI355_ERR_NOT_CONFIGURED, "sofalizer: not configured", err);
  if (partitions_K) *partitions_K = M.K;
  if (fft_n) *fft_n = M.N;
  if (pending_filters) *pending_filters = M.n_pending;
  return MI355_OK;
}

// the largest dynamic LDS the job kernels have been allowed so far (the attribute belongs to the function, not to a group)
static size_t g_sofa_conv_lds = 0, g_sofa_filter_lds = 0;   // (partition 2048 needs 112 KiB, above the default limit)

// ONE launch set for the members in subs[0..n): the pending filters of THESE members packed into the taps slab and uploaded once, the
// table uploaded once, one filter-transform launch per distinct partition length among those filters, one convolution launch per
// distinct partition length among the members, one mix. Enqueued on `stream`; nothing is waited for but the pinned blocks of the
// previous set, nothing is allocated.
int sofa_group_run(SofaGroup *G, hipStream_t stream, const SofaSubmit *subs, int n, std::string *err) {
  if (n <= 0) return MI355_OK;
  constexpr int kClasses = 9;   // partition lengths 8 .. 2048
  size_t n_rows = 0, n_filters = 0, n_taps = 0;
  for (int j = 0; j < n; j++) {
    const SofaMember &M = G->members[(size_t)subs[j].member];
    for (int c = 0; c < M.channels; c++) if (!M.drop[(size_t)c]) n_rows++;
    n_filters += (size_t)M.n_pending;
    n_taps += (size_t)M.n_pending * 2 * (size_t)M.K * (size_t)M.P;
  }
  if (n_rows > G->tab_rows || n_filters > G->tab_rows || n_taps > G->slab_floats || (size_t)n > G->members.size())
    return audio_fail(MI355_ERR_INVALID_ARG, "sofa group: tables smaller than the launch set (internal)", err);
  int rc;
  if ((rc = audio_hip(hipEventSynchronize(G->ev), "hipEventSynchronize(sofa group tables)", err))) return rc;
  const size_t conv_off = sofa_conv_offset(G), filt_off = sofa_filter_offset(G, G->tab_rows);
  SofaJobMember *hm = (SofaJobMember *)G->h_tab;
  SofaJobConv *hc = (SofaJobConv *)(G->h_tab + conv_off);
  SofaJobFilter *hf = (SofaJobFilter *)(G->h_tab + filt_off);
  const SofaJobMember *dm = (const SofaJobMember *)G->d_tab;
  const SofaJobConv *dc = (const SofaJobConv *)(G->d_tab + conv_off);
  const SofaJobFilter *df = (const SofaJobFilter *)(G->d_tab + filt_off);
  size_t mix_x = 1;
  for (int j = 0; j < n; j++) {
    const SofaMember &M = G->members[(size_t)subs[j].member];
    SofaJobMember &E = hm[j];
    E.partial = M.d_partial; E.out = subs[j].d_out; E.drop = M.d_drop; E.C = M.channels; E.pad_ = 0;
    E.row = 2ull * (unsigned long long)subs[j].n_blocks * (unsigned long long)M.B;
    for (int c = 0; c < 64; c++) E.gain[c] = c < M.channels ? subs[j].gains[c] : 0.0f;
    const size_t mx = ((size_t)E.row + 255) / 256;
    if (mx > mix_x) mix_x = mx;
  }
  // rows by partition length, classes in ascending order
  size_t conv_first[kClasses + 1] = {0}, filt_first[kClasses + 1] = {0};
  int filt_ky[kClasses] = {0};
  size_t r = 0, f = 0, t = 0;
  for (int k = 0; k < kClasses; k++) {
    const int P = 8 << k;
    conv_first[k] = r; filt_first[k] = f;
    for (int j = 0; j < n; j++) {
      SofaMember &M = G->members[(size_t)subs[j].member];
      if (M.P != P) continue;
      const size_t KN = (size_t)M.K * M.N, row = 2 * (size_t)subs[j].n_blocks * (size_t)M.B;
      for (int c = 0; c < M.channels; c++) {
        if (!M.pending[(size_t)c].empty()) {
          const std::vector<float> &taps = M.pending[(size_t)c];
          std::memcpy(G->h_slab + t, taps.data(), taps.size() * sizeof(float));
          SofaJobFilter &F = hf[f++];
          F.taps = G->d_slab + t; F.H = M.d_H + (size_t)c * 2 * KN; F.P = M.P; F.K = M.K; F.N = M.N; F.logN = M.logN;
          t += taps.size();
          if (M.K > filt_ky[k]) filt_ky[k] = M.K;
        }
        if (M.drop[(size_t)c]) continue;
        SofaJobConv &J = hc[r++];
        J.in = subs[j].d_in + c; J.in_stride = (unsigned long long)M.channels;
        J.H = M.d_H + (size_t)c * 2 * KN; J.fdl = M.d_fdl + (size_t)c * KN; J.prev = M.d_prev + (size_t)c * M.P;
        J.partial = M.d_partial + (size_t)c * row;
        J.P = M.P; J.nsub = subs[j].n_blocks * (M.B / M.P); J.K = M.K; J.N = M.N; J.logN = M.logN;
        J.slot0 = (unsigned)(M.counter % (unsigned long long)M.K);
      }
    }
  }
  conv_first[kClasses] = r; filt_first[kClasses] = f;
  if (t && (rc = audio_hip(hipMemcpyAsync(G->d_slab, G->h_slab, t * sizeof(float), hipMemcpyHostToDevice, stream), "sofa group: taps", err))) return rc;
  // (three copies at the most, each of what this set fills: the sections lie at fixed offsets)
  if ((rc = audio_hip(hipMemcpyAsync(G->d_tab, G->h_tab, (size_t)n * sizeof(SofaJobMember), hipMemcpyHostToDevice, stream), "sofa group: member table", err))) return rc;
  if (r && (rc = audio_hip(hipMemcpyAsync(G->d_tab + conv_off, G->h_tab + conv_off, r * sizeof(SofaJobConv), hipMemcpyHostToDevice, stream), "sofa group: row table", err))) return rc;
  if (f && (rc = audio_hip(hipMemcpyAsync(G->d_tab + filt_off, G->h_tab + filt_off, f * sizeof(SofaJobFilter), hipMemcpyHostToDevice, stream), "sofa group: filter table", err))) return rc;
  if ((rc = audio_hip(hipEventRecord(G->ev, stream), "hipEventRecord(sofa group tables)", err))) return rc;
  for (int k = 0; k < kClasses; k++) {
    const size_t cnt = filt_first[k + 1] - filt_first[k];
    if (!cnt) continue;
    const size_t N = (size_t)(16 << k), lds = (N + N / 2) * sizeof(float2);
    if ((rc = audio_allow_lds((const void *)sofa_filter_fft_jobs_kernel, &g_sofa_filter_lds, lds, "hipFuncSetAttribute(sofa group filter LDS)", err))) return rc;
    hipLaunchKernelGGL(sofa_filter_fft_jobs_kernel, dim3((unsigned)(cnt * (size_t)filt_ky[k]), 2), dim3(256), lds, stream, df + filt_first[k], filt_ky[k]);
    G->n_launches++;
  }
  for (int k = 0; k < kClasses; k++) {
    const size_t cnt = conv_first[k + 1] - conv_first[k];
    if (!cnt) continue;
    const size_t N = (size_t)(16 << k), lds = (3 * N + N / 2) * sizeof(float2);
    if ((rc = audio_allow_lds((const void *)sofa_convolve_jobs_kernel, &g_sofa_conv_lds, lds, "hipFuncSetAttribute(sofa group convolve LDS)", err))) return rc;
    hipLaunchKernelGGL(sofa_convolve_jobs_kernel, dim3((unsigned)cnt), dim3(256), lds, stream, dc + conv_first[k]);
    G->n_launches++;
  }
  hipLaunchKernelGGL(sofa_mix_jobs_kernel, dim3((unsigned)mix_x, (unsigned)n), dim3(256), 0, stream, dm);
  G->n_launches++;
  if ((rc = audio_hip(hipGetLastError(), "sofa group kernel launch", err))) return rc;
  for (int j = 0; j < n; j++) {
    SofaMember &M = G->members[(size_t)subs[j].member];
    for (int c = 0; c < M.channels; c++)
      if (!M.pending[(size_t)c].empty()) { M.pending[(size_t)c] = std::vector<float>(); M.have_filter[(size_t)c] = 1; }
    M.n_pending = 0;
    M.counter += (unsigned long long)subs[j].n_blocks * (unsigned long long)(M.B / M.P);
  }
  return MI355_OK;
}

}  // namespace mi355
