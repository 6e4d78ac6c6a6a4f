// audio_fft.hpp - what the two partitioned-convolution elements (sofa_kernels.hip, hrtf_kernels.hip) share: the complex product, the
// bit reversal, the radix-2 transform in LDS, and the host helpers that turn a HIP error or a refusal into a status and a message.
// One copy: a correction to one of them is a correction to both elements.
#pragma once
#include "internal.hpp"

#include <mutex>
#include <string>

namespace mi355 {

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ int bitrev(int v, int bits) { return (int)(__brev((unsigned)v) >> (32 - bits)); }

// In-place radix-2 decimation-in-time FFT of buf[0..N) in LDS by all lanes of the workgroup. tw[k] = exp(-2 pi i k / N),
// k < N/2. INVERSE: conjugated twiddles, no scaling. The caller has stored the input in bit-reversed order.
// LANES: the stride of the lanes over the N/2 butterflies of a stage. hrtfrender passes the 256 of its launch bounds, sofalizer
// kLanesBlockDim for blockDim.x, read in the loop: the two conventions each file had when it kept its own copy, and a template
// argument so that either caller's kernels compile to the instructions they had then (a run-time argument does not: the compiler
// schedules the sofalizer kernels differently around a stride it holds in a register).
constexpr int kLanesBlockDim = 0;
template <bool INVERSE, int LANES>
__device__ __forceinline__ void fft_lds(float2 *buf, const float2 *tw, int N, int logN) {
  for (int s = 1; s <= logN; s++) {
    const int half = 1 << (s - 1);
    __syncthreads();
    for (int t = threadIdx.x; t < N / 2; t += LANES == kLanesBlockDim ? (int)blockDim.x : LANES) {
      const int j = t & (half - 1), base = (t >> (s - 1)) << s;
      float2 w = tw[j << (logN - s)];
      if (INVERSE) w.y = -w.y;
      const float2 a = buf[base + j], b = cmul(buf[base + j + half], w);
      buf[base + j] = make_float2(a.x + b.x, a.y + b.y);
      buf[base + j + half] = make_float2(a.x - b.x, a.y - b.y);
    }
  }
  __syncthreads();
}

// a HIP result as a status of the C ABI, the message in *err
inline int audio_hip(hipError_t e, const char *what, std::string *err) {
  if (e == hipSuccess) return MI355_OK;
  (void)hipGetLastError();
  *err = std::string(what) + ": " + hipGetErrorString(e);
  return e == hipErrorOutOfMemory ? MI355_ERR_OUT_OF_MEMORY : MI355_ERR_HIP;
}
inline int audio_fail(int status, const char *msg, std::string *err) { *err = msg; return status; }

// Raise the dynamic LDS a kernel may be launched with to `lds`; *allowed is the largest granted so far (the attribute belongs to the
// function, not to a group or a context). A transform of 4096 points needs 112 KiB, above the default limit: a refused request
// must not reach the launch.
inline int audio_allow_lds(const void *fn, size_t *allowed, size_t lds, const char *what, std::string *err) {
  static std::mutex mu;
  std::lock_guard<std::mutex> lk(mu);
  if (lds <= *allowed) return MI355_OK;
  const int rc = audio_hip(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds), what, err);
  if (!rc) *allowed = lds;
  return rc;
}

}  // namespace mi355
