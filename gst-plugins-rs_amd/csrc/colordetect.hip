// colordetect.hip — the device side of `colordetect` (video/videofx/src/colordetect/imp.rs:57-84): per frame,
// color_thief::get_palette(plane_data(0), format, quality, max_colors) and nothing else. The crate (color-thief 0.2.2) is not
// in the reference tree; DESIGN §4.8 states the contract these kernels implement (parity unpinned) and
// tests/colordetect_restate.py restates it independently. Integer arithmetic only: results are bit-exact by construction.
//
//   colordetect_hist_kernel  every quality-th pixel of n_frames flat planes (strides ignored, as plane_data(0) is read), kept
//                            samples binned 5:5:5 into a 32768-bin LDS histogram per block; the non-zero bins are added to the
//                            frame's global histogram. Grid (blocks per frame, n_frames), one 1024-thread block per CU (128 KiB
//                            of LDS). A wave adds the bin of its first lane once with the count of all lanes that share it, so
//                            solid content costs one LDS atomic per wave instead of 64 serialised ones.
//   colordetect_mmcq_kernel  one block per frame: the histogram into LDS (and zeroed in HBM for the next call), the first box,
//                            the two MMCQ phases with workgroup-uniform control flow, the palette. Only palettes leave the device.
// A launch set of the video group's colordetect queue (group.hip: frames of INDEPENDENT element instances - each with its own plane
// size, format, quality and max_colors) runs the same two steps over a job table instead of one pitch and one setting:
//   colordetect_hist_jobs_kernel  1-D grid; a block finds its job (CdJob, up to 32 in the kernel arguments) from blockIdx and
//                                 accumulates its share of that frame's samples exactly as above - dword or byte loads per job;
//   colordetect_mmcq_jobs_kernel  one block per job, max_colors per job.
//   colordetect_plan              the blocks of a set: one per CU in all, shared out by sample count (host; mi355_selftest_colordetect_plan).
#include "internal.hpp"

#include <cstring>

namespace mi355 {

namespace {

constexpr int kBins = 32768;
constexpr int kHistThreads = 1024;
constexpr int kMmcqThreads = 512;
constexpr int kMmcqWaves = kMmcqThreads / 64;
constexpr int kQueueCap = 256;
constexpr int kMaxIterations = 1000;  // color-thief's MAX_ITERATIONS
constexpr uint32_t kNoBin = 0xffffffffu;

// what one frame's MMCQ leaves for the host (one D2H copy per call for the whole batch)
struct CdResult {
  uint8_t rgb[255 * 3];
  uint8_t pad0[3];
  int32_t n_colors;
  int32_t box[6];  // first box r1, r2, g1, g2, b1, b2; -1 when no sample was kept
  int32_t pad1;
};
static_assert(sizeof(CdResult) % 16 == 0, "CdResult keeps 16-byte alignment in arrays");

struct CdBox {
  int lo[3], hi[3];
  uint32_t count, volume, avg;  // avg: r | g << 8 | b << 16
  uint32_t pad;
};

struct Layout { int ri, gi, bi, ai; };  // byte offsets inside a pixel; ai < 0: opaque

__device__ __forceinline__ uint32_t sample_bin(uint32_t r, uint32_t g, uint32_t b, uint32_t a) {
  const bool keep = a >= 125 && !(r > 250 && g > 250 && b > 250);
  return keep ? ((r >> 3) << 10) | ((g >> 3) << 5) | (b >> 3) : kNoBin;
}

// called by every lane of the wave: the first lane's bin is added once for all lanes that hold it
__device__ __forceinline__ void add_bin(uint32_t *h, uint32_t bin) {
  const uint32_t lead = __builtin_amdgcn_readfirstlane(bin);
  const bool same = bin == lead;
  const unsigned long long m = __ballot(same);
  if (same) {
    if (lead != kNoBin && (int)__lane_id() == __ffsll((long long)m) - 1) atomicAdd(&h[lead], (uint32_t)__popcll(m));
  } else if (bin != kNoBin) {
    atomicAdd(&h[bin], 1u);
  }
}

// samples [s0, s1) of the flat plane at `base` into the block's LDS histogram. WORD: 4-byte pixels at 4-byte aligned addresses,
// one dword load per sample; otherwise byte loads. Called by every thread of the block with the same range.
template <bool WORD>
__device__ __forceinline__ void hist_accumulate(uint32_t *h, const uint8_t *__restrict__ base, size_t s0, size_t s1, size_t step, const Layout &L) {
  const int tid = threadIdx.x;
  constexpr int U = 4;
  // the trip count is the same for every lane (ballots in add_bin need the whole wave)
  for (size_t s = s0; s < s1; s += (size_t)U * kHistThreads) {
    uint32_t px[U][4];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const size_t k = s + (size_t)u * kHistThreads + tid;
      px[u][0] = px[u][1] = px[u][2] = 0;
      px[u][3] = kNoBin;  // marks a lane past the end
      if (k < s1) {
        const uint8_t *p = base + k * step;
        if (WORD) {
          const uint32_t v = *reinterpret_cast<const uint32_t *>(p);
          px[u][0] = (v >> (8 * L.ri)) & 255u;
          px[u][1] = (v >> (8 * L.gi)) & 255u;
          px[u][2] = (v >> (8 * L.bi)) & 255u;
          px[u][3] = L.ai < 0 ? 255u : (v >> (8 * L.ai)) & 255u;
        } else {
          px[u][0] = p[L.ri];
          px[u][1] = p[L.gi];
          px[u][2] = p[L.bi];
          px[u][3] = L.ai < 0 ? 255u : p[L.ai];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; u++) add_bin(h, px[u][3] == kNoBin ? kNoBin : sample_bin(px[u][0], px[u][1], px[u][2], px[u][3]));
  }
}

__device__ __forceinline__ void hist_clear(uint4 *lds_hist4) {
  for (int i = threadIdx.x; i < kBins / 4; i += kHistThreads) lds_hist4[i] = make_uint4(0, 0, 0, 0);
  __syncthreads();
}

// the block's non-zero bins into the frame's histogram `g`
__device__ __forceinline__ void hist_flush(const uint4 *lds_hist4, uint32_t *__restrict__ g) {
  __syncthreads();
  for (int i = threadIdx.x; i < kBins / 4; i += kHistThreads) {
    const uint4 v = lds_hist4[i];
    if (v.x) atomicAdd(&g[4 * i + 0], v.x);
    if (v.y) atomicAdd(&g[4 * i + 1], v.y);
    if (v.z) atomicAdd(&g[4 * i + 2], v.z);
    if (v.w) atomicAdd(&g[4 * i + 3], v.w);
  }
}

template <bool WORD>
__global__ __launch_bounds__(kHistThreads) void colordetect_hist_kernel(const uint8_t *__restrict__ frames, size_t frame_pitch, size_t n_samples,
                                                                         size_t step, size_t samples_per_block, Layout L, uint32_t *__restrict__ hist) {
  extern __shared__ uint4 lds_hist4[];
  hist_clear(lds_hist4);
  const uint8_t *base = frames + (size_t)blockIdx.y * frame_pitch;
  const size_t s0 = (size_t)blockIdx.x * samples_per_block;
  const size_t s1 = s0 + samples_per_block < n_samples ? s0 + samples_per_block : n_samples;
  hist_accumulate<WORD>(reinterpret_cast<uint32_t *>(lds_hist4), base, s0, s1, step, L);
  hist_flush(lds_hist4, hist + (size_t)blockIdx.y * kBins);
}

// one frame of a launch set: what its blocks need. The table travels in the kernel arguments (no upload, no lifetime); a block's
// job index comes from blockIdx, so the fields are scalar loads and stay in SGPRs.
struct CdJob {
  const uint8_t *base;         // the flat plane (nullptr only with blocks == 0)
  uint64_t samples_per_block;  // block b of the job takes samples [b * samples_per_block, ...) up to n_samples
  uint32_t n_samples, step;    // every quality-th pixel: byte step = quality * channels
  uint32_t first_block, blocks;  // its blocks in the 1-D grid (colordetect_plan)
  Layout L;
  int32_t word;                // 1: 4-byte pixels at a 4-byte aligned address (dword loads); 0: byte loads
  int32_t pad;
};
struct CdJobTable {
  CdJob job[kCdSetMax];
  int32_t n_jobs, pad;
};
static_assert(sizeof(CdJobTable) <= 2048, "the job table is passed in the kernel arguments");
struct CdSetColors { uint8_t max_colors[kCdSetMax]; };

__global__ __launch_bounds__(kHistThreads) void colordetect_hist_jobs_kernel(const CdJobTable T, uint32_t *__restrict__ hist) {
  extern __shared__ uint4 lds_hist4[];
  const uint32_t b = blockIdx.x;
  int j = 0;
  while (j + 1 < T.n_jobs && b >= T.job[j].first_block + T.job[j].blocks) j++;
  const uint32_t rel = b - T.job[j].first_block;
  if (b < T.job[j].first_block || rel >= T.job[j].blocks) return;  // not reached: the grid is the plan's total (uniform per block)
  hist_clear(lds_hist4);
  const size_t n_samples = T.job[j].n_samples, per_block = T.job[j].samples_per_block;
  const size_t s0 = (size_t)rel * per_block;
  const size_t s1 = s0 + per_block < n_samples ? s0 + per_block : n_samples;
  uint32_t *h = reinterpret_cast<uint32_t *>(lds_hist4);
  const Layout L = T.job[j].L;
  // the path is the job's, the same for every wave of the block
  if (T.job[j].word) hist_accumulate<true>(h, T.job[j].base, s0, s1, T.job[j].step, L);
  else hist_accumulate<false>(h, T.job[j].base, s0, s1, T.job[j].step, L);
  hist_flush(lds_hist4, hist + (size_t)j * kBins);
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}
__device__ __forceinline__ int wave_min(int x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = min(x, __shfl_xor(x, o));
  return x;
}
__device__ __forceinline__ int wave_max(int x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = max(x, __shfl_xor(x, o));
  return x;
}

__device__ __forceinline__ CdBox make_box(const int lo[3], const int hi[3], unsigned long long count, const unsigned long long sum[3]) {
  CdBox v;
  uint32_t vol = 1, avg = 0;
  for (int c = 0; c < 3; c++) {
    v.lo[c] = lo[c];
    v.hi[c] = hi[c];
    const int w = hi[c] - lo[c] + 1;
    vol *= w > 0 ? (uint32_t)w : 0u;
    const uint32_t a = count ? (uint32_t)(sum[c] / count) : (uint32_t)(4 * (lo[c] + hi[c] + 1)) & 255u;
    avg |= a << (8 * c);
  }
  v.count = (uint32_t)count;
  v.volume = vol;
  v.avg = avg;
  v.pad = 0;
  return v;
}

__device__ __forceinline__ unsigned long long box_key(const CdBox &v, bool by_volume) {
  return by_volume ? (unsigned long long)v.count * v.volume : (unsigned long long)v.count;
}

struct MmcqShared {
  CdBox q[kQueueCap], tmp[kQueueCap];
  unsigned long long slice[4][32];  // per slice of the cut axis: count, sum r, sum g, sum b
  unsigned long long red[4][kMmcqWaves];
  int ired[6][kMmcqWaves];
};

// pop's stable ascending sort, done only when a push may have broken the order: rank = smaller keys + equal keys standing before
__device__ void sort_queue(MmcqShared &S, int n, bool by_volume) {
  const int tid = threadIdx.x;
  const bool unsorted = tid < n - 1 && box_key(S.q[tid], by_volume) > box_key(S.q[tid + 1], by_volume);
  if (!__syncthreads_or(unsorted)) return;
  if (tid < n) {
    const unsigned long long k = box_key(S.q[tid], by_volume);
    int r = 0;
    for (int j = 0; j < n; j++) {
      const unsigned long long kj = box_key(S.q[j], by_volume);
      r += kj < k || (kj == k && j < tid);
    }
    S.tmp[r] = S.q[tid];
  }
  __syncthreads();
  if (tid < n) S.q[tid] = S.tmp[tid];
  __syncthreads();
}

// cut of a box with count >= 2 (DESIGN §4.8 "Cut" steps 2-8): the slices of the widest axis are summed by the waves, the split
// is then chosen by every thread from the same LDS values
__device__ void cut_box(MmcqShared &S, const uint32_t *H, const CdBox &v, CdBox *v1, CdBox *v2) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int width[3];
  for (int c = 0; c < 3; c++) width[c] = v.hi[c] - v.lo[c] + 1;
  const int axis = (width[0] >= width[1] && width[0] >= width[2]) ? 0 : (width[1] >= width[2] ? 1 : 2);
  const int a1 = axis == 0 ? 1 : 0, a2 = axis == 2 ? 1 : 2;
  auto sel = [](const int *a, int k) { return k == 0 ? a[0] : (k == 1 ? a[1] : a[2]); };  // no dynamic register indexing
  const int lo = sel(v.lo, axis), hi = sel(v.hi, axis), w = sel(width, axis);
  if (tid < 128) S.slice[tid >> 5][tid & 31] = 0;
  __syncthreads();
  const int parts = w >= kMmcqWaves ? 1 : kMmcqWaves / w;
  const int n1 = sel(width, a1), n2 = sel(width, a2), lo_1 = sel(v.lo, a1), lo_2 = sel(v.lo, a2);
  for (int item = wave; item < w * parts; item += kMmcqWaves) {
    const int s = lo + item / parts, part = item % parts;
    const int r_beg = part * n1 / parts, r_end = (part + 1) * n1 / parts;
    const int n_bins = (r_end - r_beg) * n2;
    unsigned long long acc[4] = {0, 0, 0, 0};
    for (int k = lane; k < n_bins; k += 64) {
      const int x1 = lo_1 + r_beg + k / n2, x2 = lo_2 + k % n2;
      const int cr = axis == 0 ? s : x1, cg = axis == 1 ? s : (axis == 0 ? x1 : x2), cb = axis == 2 ? s : x2;
      const uint32_t hv = H[(cr << 10) | (cg << 5) | cb];
      if (hv) {
        acc[0] += hv;
        acc[1] += (unsigned long long)hv * (unsigned)(8 * cr + 4);
        acc[2] += (unsigned long long)hv * (unsigned)(8 * cg + 4);
        acc[3] += (unsigned long long)hv * (unsigned)(8 * cb + 4);
      }
    }
    for (int c = 0; c < 4; c++) acc[c] = wave_sum(acc[c]);
    if (lane == 0 && acc[0])
      for (int c = 0; c < 4; c++) atomicAdd(&S.slice[c][s - lo], acc[c]);
  }
  __syncthreads();
  // partial[s] = count of slices lo..s
  unsigned long long total = 0;
  for (int s = 0; s < w; s++) total += S.slice[0][s];
  int i = lo;
  {
    unsigned long long p = 0;
    for (int s = lo; s <= hi; s++) {
      p += S.slice[0][s - lo];
      if (2 * p > total) { i = s; break; }
    }
  }
  auto partial = [&](int d) {
    unsigned long long p = 0;
    for (int s = lo; s <= d; s++) p += S.slice[0][s - lo];
    return p;
  };
  const int left = i - lo, right = hi - i;
  int d = left <= right ? min(hi - 1, i + right / 2) : max(lo, i - 1 - (left + 1) / 2);
  while (d < lo || partial(d) == 0) d++;
  unsigned long long c2 = total - partial(d);
  while (c2 == 0 && d - 1 >= lo && partial(d - 1) != 0) {
    d--;
    c2 = total - partial(d);
  }
  unsigned long long cnt1 = 0, sum1[3] = {0, 0, 0}, cnt2 = 0, sum2[3] = {0, 0, 0};
  for (int s = lo; s <= hi; s++) {
    unsigned long long *cnt = s <= d ? &cnt1 : &cnt2, *sum = s <= d ? sum1 : sum2;
    *cnt += S.slice[0][s - lo];
    for (int c = 0; c < 3; c++) sum[c] += S.slice[1 + c][s - lo];
  }
  int lo1[3], hi1[3], lo2[3], hi2[3];
  for (int c = 0; c < 3; c++) {
    lo1[c] = v.lo[c];
    hi2[c] = v.hi[c];
    hi1[c] = c == axis ? d : v.hi[c];
    lo2[c] = c == axis ? d + 1 : v.lo[c];
  }
  *v1 = make_box(lo1, hi1, cnt1, sum1);
  *v2 = make_box(lo2, hi2, cnt2, sum2);
  __syncthreads();  // S.slice is reused by the next cut
}

// iter(Q, target) of DESIGN §4.8; `n` is the queue size, the same value in every thread
__device__ void mmcq_iter(MmcqShared &S, const uint32_t *H, int &n, bool &dirty, bool by_volume, int max_colors) {
  const int tid = threadIdx.x;
  for (int it = 0; it < kMaxIterations;) {
    if (by_volume ? n >= max_colors : 4 * n >= 3 * max_colors) return;
    it++;
    if (dirty) sort_queue(S, n, by_volume);
    dirty = false;
    const CdBox v = S.q[n - 1];
    if (v.count == 0) {  // popped and pushed back: the queue is unchanged
      it++;
      continue;
    }
    if (v.count == 1) continue;  // cut returns a copy and no second box: the same
    CdBox v1, v2;
    cut_box(S, H, v, &v1, &v2);
    if (n + 1 > kQueueCap) return;  // not reached: n stops at max_colors <= 255
    if (tid == 0) {
      S.q[n - 1] = v1;
      S.q[n] = v2;
    }
    n++;
    dirty = true;
    __syncthreads();
  }
}

// one frame, by the whole block: its histogram `hist` into LDS (and zeroed in HBM), the first box, the two phases, the palette
__device__ __forceinline__ void mmcq_frame(uint32_t *__restrict__ hist, int max_colors, CdResult *__restrict__ res) {
  extern __shared__ uint4 lds_hist4[];
  __shared__ MmcqShared S;
  uint32_t *H = reinterpret_cast<uint32_t *>(lds_hist4);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint4 *g4 = reinterpret_cast<uint4 *>(hist);
  unsigned long long cnt = 0, sum[3] = {0, 0, 0};
  int mn[3] = {32, 32, 32}, mx[3] = {-1, -1, -1};
  for (int i = tid; i < kBins / 4; i += kMmcqThreads) {
    const uint4 v = g4[i];
    lds_hist4[i] = v;
    g4[i] = make_uint4(0, 0, 0, 0);  // the histogram is zero again for the next call
    const uint32_t hv[4] = {v.x, v.y, v.z, v.w};
    for (int c = 0; c < 4; c++) {
      if (!hv[c]) continue;
      const int idx = 4 * i + c, co[3] = {idx >> 10, (idx >> 5) & 31, idx & 31};
      cnt += hv[c];
      for (int k = 0; k < 3; k++) {
        sum[k] += (unsigned long long)hv[c] * (unsigned)(8 * co[k] + 4);
        mn[k] = min(mn[k], co[k]);
        mx[k] = max(mx[k], co[k]);
      }
    }
  }
  cnt = wave_sum(cnt);
  for (int k = 0; k < 3; k++) {
    sum[k] = wave_sum(sum[k]);
    mn[k] = wave_min(mn[k]);
    mx[k] = wave_max(mx[k]);
  }
  if (lane == 0) {
    S.red[0][wave] = cnt;
    for (int k = 0; k < 3; k++) {
      S.red[1 + k][wave] = sum[k];
      S.ired[k][wave] = mn[k];
      S.ired[3 + k][wave] = mx[k];
    }
  }
  __syncthreads();
  cnt = 0;
  for (int k = 0; k < 3; k++) { sum[k] = 0; mn[k] = 32; mx[k] = -1; }
  for (int wv = 0; wv < kMmcqWaves; wv++) {
    cnt += S.red[0][wv];
    for (int k = 0; k < 3; k++) {
      sum[k] += S.red[1 + k][wv];
      mn[k] = min(mn[k], S.ired[k][wv]);
      mx[k] = max(mx[k], S.ired[3 + k][wv]);
    }
  }
  if (cnt == 0) {  // nothing kept: no colours
    if (tid < 6) res->box[tid] = -1;
    if (tid == 0) res->n_colors = 0;
    return;
  }
  if (tid < 6) res->box[tid] = (tid & 1) ? mx[tid >> 1] : mn[tid >> 1];
  if (tid == 0) S.q[0] = make_box(mn, mx, cnt, sum);
  __syncthreads();
  int n = 1;
  bool dirty = false;
  mmcq_iter(S, H, n, dirty, false, max_colors);  // queue A, key count, target 0.75 * max_colors
  // pop A until it is empty, pushing onto B: B is A sorted by count, reversed
  if (dirty) sort_queue(S, n, false);
  if (tid < n) S.tmp[n - 1 - tid] = S.q[tid];
  __syncthreads();
  if (tid < n) S.q[tid] = S.tmp[tid];
  __syncthreads();
  dirty = true;
  mmcq_iter(S, H, n, dirty, true, max_colors);  // queue B, key count * volume, target max_colors
  if (dirty) sort_queue(S, n, true);
  // pop B until it is empty: palette order
  if (tid < n) {
    const uint32_t a = S.q[n - 1 - tid].avg;
    res->rgb[3 * tid + 0] = (uint8_t)(a & 255u);
    res->rgb[3 * tid + 1] = (uint8_t)((a >> 8) & 255u);
    res->rgb[3 * tid + 2] = (uint8_t)((a >> 16) & 255u);
  }
  if (tid == 0) res->n_colors = n;
}

__global__ __launch_bounds__(kMmcqThreads) void colordetect_mmcq_kernel(uint32_t *__restrict__ hist, int max_colors, CdResult *__restrict__ out) {
  mmcq_frame(hist + (size_t)blockIdx.x * kBins, max_colors, out + blockIdx.x);
}

// a launch set: block = job, max_colors per job (a job without samples finds its histogram empty: 0 colours, box -1)
__global__ __launch_bounds__(kMmcqThreads) void colordetect_mmcq_jobs_kernel(uint32_t *__restrict__ hist, const CdSetColors C, CdResult *__restrict__ out) {
  mmcq_frame(hist + (size_t)blockIdx.x * kBins, (int)C.max_colors[blockIdx.x], out + blockIdx.x);
}

bool layout_of(int format, int *ch, Layout *L) {
  switch (format) {
    case MI355_FMT_RGB: *ch = 3; *L = {0, 1, 2, -1}; return true;
    case MI355_FMT_RGBA: *ch = 4; *L = {0, 1, 2, 3}; return true;
    case MI355_FMT_ARGB: *ch = 4; *L = {1, 2, 3, 0}; return true;
    case MI355_FMT_BGR: *ch = 3; *L = {2, 1, 0, -1}; return true;
    case MI355_FMT_BGRA: *ch = 4; *L = {2, 1, 0, 3}; return true;
    default: return false;
  }
}

}  // namespace

// scratch of one context: the frames' histograms (all zero between calls), the results on both sides, the host frame's staging
struct ColorDetectState {
  uint32_t *d_hist = nullptr;
  int hist_frames = 0;
  bool hist_zero = false;  // false after an allocation or an interrupted call: cleared before the next launch
  CdResult *d_res = nullptr, *h_res = nullptr;
  int res_frames = 0;
  uint8_t *d_stage = nullptr;
  size_t stage_bytes = 0;
};

void colordetect_release(mi355_ctx *ctx) {
  auto *s = static_cast<ColorDetectState *>(ctx->colordetect);
  if (!s) return;
  if (s->d_hist) (void)hipFree(s->d_hist);
  if (s->d_res) (void)hipFree(s->d_res);
  if (s->h_res) (void)hipHostFree(s->h_res);
  if (s->d_stage) (void)hipFree(s->d_stage);
  delete s;
  ctx->colordetect = nullptr;
}

static int colordetect_scratch(mi355_ctx *ctx, int n_frames, ColorDetectState **out) {
  auto *s = static_cast<ColorDetectState *>(ctx->colordetect);
  if (!s) ctx->colordetect = s = new ColorDetectState();
  int rc = MI355_OK;
  if (s->hist_frames < n_frames) {
    if (s->d_hist) (void)hipFree(s->d_hist);
    s->d_hist = nullptr;
    s->hist_frames = 0;
    if ((rc = check_hip(ctx, hipMalloc((void **)&s->d_hist, (size_t)n_frames * kBins * sizeof(uint32_t)), "hipMalloc(colordetect histograms)"))) return rc;
    s->hist_frames = n_frames;
    s->hist_zero = false;
  }
  if (!s->hist_zero) {
    if ((rc = check_hip(ctx, hipMemsetAsync(s->d_hist, 0, (size_t)s->hist_frames * kBins * sizeof(uint32_t), ctx->stream), "hipMemsetAsync(colordetect)"))) return rc;
    s->hist_zero = true;
  }
  if (s->res_frames < n_frames) {
    if (s->d_res) (void)hipFree(s->d_res);
    if (s->h_res) (void)hipHostFree(s->h_res);
    s->d_res = nullptr;
    s->h_res = nullptr;
    s->res_frames = 0;
    if ((rc = check_hip(ctx, hipMalloc((void **)&s->d_res, (size_t)n_frames * sizeof(CdResult)), "hipMalloc(colordetect results)"))) return rc;
    if ((rc = check_hip(ctx, hipHostMalloc((void **)&s->h_res, (size_t)n_frames * sizeof(CdResult), hipHostMallocDefault), "hipHostMalloc(colordetect results)")))
      return rc;
    s->res_frames = n_frames;
  }
  *out = s;
  return MI355_OK;
}

static size_t samples_of(size_t data_len, int ch, int quality) { return (data_len / (size_t)ch + (size_t)quality - 1) / (size_t)quality; }

static int colordetect_check_args(size_t data_len, int n_frames, int format, int quality, int max_colors, int *ch, Layout *L, const char **why) {
  if (!layout_of(format, ch, L)) { *why = "colordetect: format is not RGB, RGBA, ARGB, BGR or BGRA"; return MI355_ERR_UNSUPPORTED; }
  *why = nullptr;
  if (quality < 1 || quality > 10) *why = "colordetect: quality must be 1..10";
  else if (max_colors < 2 || max_colors > 255) *why = "colordetect: max_colors must be 2..255";
  else if (n_frames < 0 || n_frames > 65535) *why = "colordetect: n_frames must be 0..65535";
  // bins are 32-bit: at most 2^32 - 1 samples per frame
  else if (samples_of(data_len, *ch, quality) > 0xffffffffull) *why = "colordetect: more than 2^32 - 1 samples in a frame";
  return *why ? MI355_ERR_INVALID_ARG : MI355_OK;
}

static int colordetect_check(mi355_ctx *ctx, size_t data_len, int n_frames, int format, int quality, int max_colors, int *ch, Layout *L) {
  const char *why = nullptr;
  const int rc = colordetect_check_args(data_len, n_frames, format, quality, max_colors, ch, L, &why);
  return rc ? set_error(ctx, rc, why) : MI355_OK;
}

// both kernels on ctx->stream; the histograms are zero again once the MMCQ kernel has run
static int colordetect_enqueue(mi355_ctx *ctx, ColorDetectState *s, const uint8_t *d_frames, size_t frame_pitch, size_t data_len, int n_frames, int ch,
                               const Layout &L, int quality, int max_colors, bool mmcq) {
  const size_t n_samples = (data_len / (size_t)ch + (size_t)quality - 1) / (size_t)quality;
  const size_t step = (size_t)quality * (size_t)ch;
  int rc = MI355_OK;
  if (n_samples > 0) {
    // one block per CU in all (the LDS histogram takes 128 KiB), at least 16 samples per thread
    size_t blocks = ((size_t)ctx->n_cu + (size_t)n_frames - 1) / (size_t)n_frames;
    const size_t by_work = (n_samples + 16 * kHistThreads - 1) / (16 * kHistThreads);
    if (blocks > by_work) blocks = by_work;
    if (blocks < 1) blocks = 1;
    const size_t per_block = (n_samples + blocks - 1) / blocks;
    const bool word = ch == 4 && ((uintptr_t)d_frames % 4 == 0) && (frame_pitch % 4 == 0 || n_frames == 1);
    const size_t lds = kBins * sizeof(uint32_t);
    auto kern = word ? colordetect_hist_kernel<true> : colordetect_hist_kernel<false>;
    if ((rc = check_hip(ctx, hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds), "hipFuncSetAttribute(max dynamic LDS)")))
      return rc;
    s->hist_zero = false;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks, (unsigned)n_frames), dim3(kHistThreads), lds, ctx->stream, d_frames, frame_pitch, n_samples, step, per_block, L,
                       s->d_hist);
    if ((rc = check_hip(ctx, hipGetLastError(), "colordetect histogram launch"))) return rc;
  }
  if (!mmcq) return MI355_OK;
  const size_t lds = kBins * sizeof(uint32_t);
  if ((rc = check_hip(ctx, hipFuncSetAttribute((const void *)colordetect_mmcq_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds),
                      "hipFuncSetAttribute(max dynamic LDS)")))
    return rc;
  s->hist_zero = false;
  hipLaunchKernelGGL(colordetect_mmcq_kernel, dim3((unsigned)n_frames), dim3(kMmcqThreads), lds, ctx->stream, s->d_hist, max_colors, s->d_res);
  if ((rc = check_hip(ctx, hipGetLastError(), "colordetect mmcq launch"))) return rc;
  s->hist_zero = true;
  return MI355_OK;
}

static int colordetect_collect(mi355_ctx *ctx, ColorDetectState *s, int n_frames, uint8_t *palette_rgb, int *n_colors) {
  int rc = check_hip(ctx, hipMemcpyAsync(s->h_res, s->d_res, (size_t)n_frames * sizeof(CdResult), hipMemcpyDeviceToHost, ctx->stream), "colordetect D2H");
  if (rc) { s->hist_zero = false; return rc; }
  __atomic_fetch_add(&ctx->n_d2h, 1ull, __ATOMIC_RELAXED);
  if ((rc = check_hip(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize"))) { s->hist_zero = false; return rc; }
  for (int f = 0; f < n_frames; f++) {
    const CdResult &r = s->h_res[f];
    n_colors[f] = r.n_colors;
    std::memset(palette_rgb + (size_t)f * 255 * 3, 0, 255 * 3);
    std::memcpy(palette_rgb + (size_t)f * 255 * 3, r.rgb, (size_t)r.n_colors * 3);
  }
  return MI355_OK;
}

// ---------------------------------------------------------------- launch sets (the video group's colordetect queue, group.hip)

int colordetect_check_frame(size_t data_len, int format, int quality, int max_colors, const char **why) {
  int ch = 0;
  Layout L{};
  return colordetect_check_args(data_len, 1, format, quality, max_colors, &ch, &L, why);
}

// The blocks of one launch set. A histogram block holds 128 KiB of LDS, so a CU runs one: n_cu blocks in all. Every job with
// samples gets one; what is left of n_cu is shared out by sample count (rounded down), up to the lone launch's limit of one block
// per 16 Ki samples. The job's samples are then cut into equal shares and the block count is what those shares need, so no block
// is empty: blocks * samples_per_block >= n_samples > (blocks - 1) * samples_per_block.
int colordetect_plan(int n_cu, int n_jobs, const uint64_t *n_samples, uint32_t *first_block, uint32_t *blocks, uint64_t *samples_per_block, uint32_t *total_blocks) {
  if (n_cu < 1 || n_jobs < 0 || n_jobs > kCdSetMax || !total_blocks || (n_jobs && (!n_samples || !first_block || !blocks || !samples_per_block)))
    return MI355_ERR_INVALID_ARG;
  uint64_t all = 0, with_samples = 0;
  for (int j = 0; j < n_jobs; j++) {
    if (n_samples[j] > 0xffffffffull) return MI355_ERR_INVALID_ARG;
    all += n_samples[j];
    with_samples += n_samples[j] > 0;
  }
  const uint64_t spare = (uint64_t)n_cu > with_samples ? (uint64_t)n_cu - with_samples : 0;
  uint32_t next = 0;
  for (int j = 0; j < n_jobs; j++) {
    const uint64_t n = n_samples[j];
    uint64_t b = 0, per = 0;
    if (n) {
      b = 1 + n * spare / all;  // n < 2^32, spare < 2^31: no overflow
      const uint64_t by_work = (n + 16 * kHistThreads - 1) / (16 * kHistThreads);
      if (b > by_work) b = by_work;
      per = (n + b - 1) / b;
      b = (n + per - 1) / per;
    }
    first_block[j] = next;
    blocks[j] = (uint32_t)b;
    samples_per_block[j] = per;
    next += (uint32_t)b;
  }
  *total_blocks = next;
  return MI355_OK;
}

struct CdSetScratch {
  uint32_t *d_hist = nullptr;  // [kCdSetMax][kBins]
  CdResult *d_res = nullptr;   // [kCdSetMax]
  bool hist_zero = false;      // false after the allocation or an interrupted set: cleared before the next launch
};

void colordetect_set_scratch_free(CdSetScratch *S) {
  if (!S) return;
  if (S->d_hist) (void)hipFree(S->d_hist);
  if (S->d_res) (void)hipFree(S->d_res);
  delete S;
}

CdSetScratch *colordetect_set_scratch_new(hipStream_t stream, int *status, std::string *err) {
  CdSetScratch *S = new CdSetScratch();
  const size_t lds = kBins * sizeof(uint32_t), hist_bytes = (size_t)kCdSetMax * kBins * sizeof(uint32_t);
  const char *what = nullptr;
  int st = MI355_ERR_HIP;
  if (hipMalloc((void **)&S->d_hist, hist_bytes) != hipSuccess) { what = "hipMalloc(colordetect set histograms)"; st = MI355_ERR_OUT_OF_MEMORY; }
  else if (hipMalloc((void **)&S->d_res, (size_t)kCdSetMax * sizeof(CdResult)) != hipSuccess) { what = "hipMalloc(colordetect set results)"; st = MI355_ERR_OUT_OF_MEMORY; }
  else if (hipMemsetAsync(S->d_hist, 0, hist_bytes, stream) != hipSuccess) what = "hipMemsetAsync(colordetect set histograms)";
  else if (hipFuncSetAttribute((const void *)colordetect_hist_jobs_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess ||
           hipFuncSetAttribute((const void *)colordetect_mmcq_jobs_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    what = "hipFuncSetAttribute(max dynamic LDS)";
  if (what) {
    (void)hipGetLastError();
    colordetect_set_scratch_free(S);
    *status = st;
    *err = what;
    return nullptr;
  }
  S->hist_zero = true;
  *status = MI355_OK;
  return S;
}

size_t colordetect_set_block_bytes() { return (size_t)kCdSetMax * sizeof(CdResult); }

int colordetect_launch_set(CdSetScratch *S, hipStream_t stream, int n_cu, const CdFrame *frames, int n, void *h_block, int *kernel_launches, std::string *err) {
  *kernel_launches = 0;
  if (!S || !frames || !h_block || n < 1 || n > kCdSetMax) { *err = "colordetect: bad launch set"; return MI355_ERR_INVALID_ARG; }
  CdJobTable T{};
  CdSetColors C{};
  uint64_t n_samples[kCdSetMax], per_block[kCdSetMax];
  uint32_t first[kCdSetMax], blocks[kCdSetMax], total = 0;
  int ch[kCdSetMax];
  for (int i = 0; i < n; i++) {
    if (!layout_of(frames[i].format, &ch[i], &T.job[i].L)) { *err = "colordetect: bad launch set"; return MI355_ERR_INVALID_ARG; }
    n_samples[i] = samples_of(frames[i].data_len, ch[i], frames[i].quality);
  }
  int rc = colordetect_plan(n_cu, n, n_samples, first, blocks, per_block, &total);
  if (rc) { *err = "colordetect: bad launch set"; return rc; }
  for (int i = 0; i < n; i++) {
    CdJob &J = T.job[i];
    J.base = frames[i].data;
    J.samples_per_block = per_block[i];
    J.n_samples = (uint32_t)n_samples[i];
    J.step = (uint32_t)(frames[i].quality * ch[i]);
    J.first_block = first[i];
    J.blocks = blocks[i];
    J.word = ch[i] == 4 && (uintptr_t)frames[i].data % 4 == 0;
    C.max_colors[i] = (uint8_t)frames[i].max_colors;
  }
  T.n_jobs = n;
  auto hip_failed = [&](hipError_t e, const char *what) {
    if (e == hipSuccess) return false;
    (void)hipGetLastError();
    *err = std::string(what) + ": " + hipGetErrorString(e);
    return true;
  };
  const size_t lds = kBins * sizeof(uint32_t);
  if (!S->hist_zero) {
    if (hip_failed(hipMemsetAsync(S->d_hist, 0, (size_t)kCdSetMax * kBins * sizeof(uint32_t), stream), "hipMemsetAsync(colordetect set)")) return MI355_ERR_HIP;
    S->hist_zero = true;
  }
  if (total > 0) {
    S->hist_zero = false;
    hipLaunchKernelGGL(colordetect_hist_jobs_kernel, dim3(total), dim3(kHistThreads), lds, stream, T, S->d_hist);
    if (hip_failed(hipGetLastError(), "colordetect set histogram launch")) return MI355_ERR_HIP;
    ++*kernel_launches;
  }
  S->hist_zero = false;
  hipLaunchKernelGGL(colordetect_mmcq_jobs_kernel, dim3((unsigned)n), dim3(kMmcqThreads), lds, stream, S->d_hist, C, S->d_res);
  if (hip_failed(hipGetLastError(), "colordetect set mmcq launch")) return MI355_ERR_HIP;
  ++*kernel_launches;
  S->hist_zero = true;  // the MMCQ kernel leaves every histogram it read zeroed
  if (hip_failed(hipMemcpyAsync(h_block, S->d_res, (size_t)n * sizeof(CdResult), hipMemcpyDeviceToHost, stream), "colordetect set D2H")) return MI355_ERR_HIP;
  return MI355_OK;
}

void colordetect_set_result(const void *h_block, int i, uint8_t palette_rgb[255 * 3], int *n_colors) {
  const CdResult &r = static_cast<const CdResult *>(h_block)[i];
  *n_colors = r.n_colors;
  std::memset(palette_rgb, 0, 255 * 3);
  std::memcpy(palette_rgb, r.rgb, (size_t)r.n_colors * 3);
}

}  // namespace mi355

using namespace mi355;

extern "C" {

int mi355_colordetect_frames_device(mi355_ctx *ctx, const uint8_t *d_frames, size_t frame_pitch, size_t data_len, int n_frames, int format, int quality,
                                    int max_colors, uint8_t *palette_rgb, int *n_colors) {
  if (!ctx) return MI355_ERR_INVALID_ARG;
  int ch = 0;
  Layout L{};
  int rc = colordetect_check(ctx, data_len, n_frames, format, quality, max_colors, &ch, &L);
  if (rc) return rc;
  if (n_frames == 0) return MI355_OK;
  if (!palette_rgb || !n_colors || (data_len && !d_frames)) return set_error(ctx, MI355_ERR_INVALID_ARG, "colordetect: null frames or result arrays");
  if (n_frames > 1 && frame_pitch < data_len) return set_error(ctx, MI355_ERR_INVALID_ARG, "colordetect: frame_pitch smaller than data_len");
  if ((rc = check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice"))) return rc;
  ColorDetectState *s = nullptr;
  if ((rc = colordetect_scratch(ctx, n_frames, &s))) return rc;
  if ((rc = colordetect_enqueue(ctx, s, d_frames, frame_pitch, data_len, n_frames, ch, L, quality, max_colors, true))) return rc;
  return colordetect_collect(ctx, s, n_frames, palette_rgb, n_colors);
}

int mi355_colordetect_frame(mi355_ctx *ctx, const uint8_t *data, size_t data_len, int format, int quality, int max_colors, uint8_t *palette_rgb, int *n_colors) {
  if (!ctx) return MI355_ERR_INVALID_ARG;
  int ch = 0;
  Layout L{};
  int rc = colordetect_check(ctx, data_len, 1, format, quality, max_colors, &ch, &L);
  if (rc) return rc;
  if (!palette_rgb || !n_colors || (data_len && !data)) return set_error(ctx, MI355_ERR_INVALID_ARG, "colordetect: null frame or result arrays");
  if ((rc = check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice"))) return rc;
  ColorDetectState *s = nullptr;
  if ((rc = colordetect_scratch(ctx, 1, &s))) return rc;
  if (s->stage_bytes < data_len) {
    if (s->d_stage) (void)hipFree(s->d_stage);
    s->d_stage = nullptr;
    s->stage_bytes = 0;
    if ((rc = check_hip(ctx, hipMalloc((void **)&s->d_stage, data_len), "hipMalloc(colordetect staging)"))) return rc;
    s->stage_bytes = data_len;
  }
  if (data_len) {
    if ((rc = check_hip(ctx, hipMemcpyAsync(s->d_stage, data, data_len, hipMemcpyHostToDevice, ctx->stream), "colordetect H2D"))) return rc;
    __atomic_fetch_add(&ctx->n_h2d, 1ull, __ATOMIC_RELAXED);
  }
  if ((rc = colordetect_enqueue(ctx, s, s->d_stage, data_len, data_len, 1, ch, L, quality, max_colors, true))) return rc;
  return colordetect_collect(ctx, s, 1, palette_rgb, n_colors);
}

int mi355_colordetect_histogram_device(mi355_ctx *ctx, const uint8_t *d_data, size_t data_len, int format, int quality, uint32_t *hist, int *box) {
  if (!ctx) return MI355_ERR_INVALID_ARG;
  int ch = 0;
  Layout L{};
  int rc = colordetect_check(ctx, data_len, 1, format, quality, 2, &ch, &L);
  if (rc) return rc;
  if (!hist || !box || (data_len && !d_data)) return set_error(ctx, MI355_ERR_INVALID_ARG, "colordetect: null frame or result arrays");
  if ((rc = check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice"))) return rc;
  ColorDetectState *s = nullptr;
  if ((rc = colordetect_scratch(ctx, 1, &s))) return rc;
  if ((rc = colordetect_enqueue(ctx, s, d_data, data_len, data_len, 1, ch, L, quality, 2, false))) return rc;
  if ((rc = check_hip(ctx, hipMemcpyAsync(hist, s->d_hist, kBins * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream), "colordetect histogram D2H"))) {
    s->hist_zero = false;
    return rc;
  }
  // the MMCQ kernel finds the first box (and zeroes the histogram)
  if ((rc = colordetect_enqueue(ctx, s, d_data, data_len, 0, 1, ch, L, quality, 2, true))) return rc;
  uint8_t pal[255 * 3];
  int n = 0;
  if ((rc = colordetect_collect(ctx, s, 1, pal, &n))) return rc;
  std::memcpy(box, s->h_res[0].box, sizeof(s->h_res[0].box));
  return MI355_OK;
}

int mi355_selftest_colordetect_plan(int n_cu, int n_jobs, const uint64_t *n_samples, uint32_t *first_block, uint32_t *blocks, uint64_t *samples_per_block,
                                    uint32_t *total_blocks) {
  return colordetect_plan(n_cu, n_jobs, n_samples, first_block, blocks, samples_per_block, total_blocks);
}

// test only: the MMCQ kernel on a histogram given by the caller instead of one counted from a frame, launched as
// mi355_colordetect_histogram_device launches its second step
int mi355_selftest_colordetect_mmcq(mi355_ctx *ctx, const uint32_t *bins, int max_colors, uint8_t *palette_rgb, int *n_colors, int *box) {
  if (!ctx) return MI355_ERR_INVALID_ARG;
  if (!bins || !palette_rgb || !n_colors || !box) return set_error(ctx, MI355_ERR_INVALID_ARG, "colordetect: null bins or result arrays");
  if (max_colors < 2 || max_colors > 255) return set_error(ctx, MI355_ERR_INVALID_ARG, "colordetect: max_colors must be 2..255");
  uint64_t all = 0;
  for (int i = 0; i < kBins; i++) all += bins[i];
  if (all > 0xffffffffull) return set_error(ctx, MI355_ERR_INVALID_ARG, "colordetect: more than 2^32 - 1 samples in the bins");
  int ch = 0;
  Layout L{};
  (void)layout_of(MI355_FMT_RGBA, &ch, &L);
  int rc = check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice");
  if (rc) return rc;
  ColorDetectState *s = nullptr;
  if ((rc = colordetect_scratch(ctx, 1, &s))) return rc;
  s->hist_zero = false;
  if ((rc = check_hip(ctx, hipMemcpyAsync(s->d_hist, bins, kBins * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream), "colordetect bins H2D"))) return rc;
  __atomic_fetch_add(&ctx->n_h2d, 1ull, __ATOMIC_RELAXED);
  if ((rc = colordetect_enqueue(ctx, s, nullptr, 0, 0, 1, ch, L, 1, max_colors, true))) return rc;
  if ((rc = colordetect_collect(ctx, s, 1, palette_rgb, n_colors))) return rc;
  std::memcpy(box, s->h_res[0].box, sizeof(s->h_res[0].box));
  return MI355_OK;
}

}  // extern "C"
