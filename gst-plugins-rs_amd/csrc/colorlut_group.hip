// colorlut_group.hip — launch sets of the video group's colorlut queue (group.hip: ClKind, mi355_group_submit_colorlut).
//
// Frames of independent colorlut instances (one buffer per call and element: video/colorlut/src/colorlut/imp.rs:203-223) - each with
// its own size, strides, format and its own LUT, 1D or 3D, of any size and domain - in at most two launches over a job table. The
// form is the hsvfilter queue's (hsv_kernels.hip, job_set.hpp): the table travels in the kernel arguments, a block finds its one job
// from blockIdx alone (hsvdetect_job_of), so every job field is scalar and every path choice the same for all waves of a block; the
// blocks are planned by hsvdetect_plan from the jobs' own units.
//   colorlut_jobs_kernel       the vector launch: RGBA8 frames of the flat class (both sides packed, both bases and the byte count
//                              multiples of 16) or the rowpad class (both bases and both strides multiples of 16; ceil(width / 4)
//                              groups per row, the 1-3 pixel group at a row's end read and written dword by dword), FORCE_GENERIC off.
//                              Four pixels per lane, one 16-byte load and one 16-byte store. A byte has 256 values, so per axis the
//                              reference's norm_comp, `* (size - 1)`, floor index and weight (imp.rs:471-479, :496-503) have 256
//                              possible results: each block computes them once for ITS job - the operations of norm_comp_generic<false>,
//                              floor_idx and `x - x0`, one thread per byte value - into 6 KiB of LDS as {x0, t} pairs, which takes the
//                              three IEEE divisions out of the pixel. The corners, the eight float4 cell reads from the job's cells in
//                              global memory and the seven lerps per channel are sample_3d_at, the same function colorlut_rows_kernel
//                              runs behind its own index arithmetic; a 1D LUT is sample_1d_at per channel. The alpha byte is kept.
//   colorlut_rows_jobs_kernel  the literal launch, one pixel per lane through colorlut_px_literal, the body of colorlut_rows_kernel:
//                              both RGBA64 byte orders (alpha word copied raw), RGBA8 frames off the 16-byte grid, FORCE_GENERIC.
// Neither kernel stages LUT cells in LDS, neither reads a memoised table: the cells come from global memory (L2) as they are gathered.
//
// The block plan - (units per block, blocks per CU), stated here once:
//   vector   512 groups of four pixels per block (two per lane), 16 blocks per CU: the budget of a squeezed plan is four rounds of the
//            four blocks a CU can hold (107 VGPRs: 4 waves per SIMD), so that unequal jobs still balance while the 768-entry LDS
//            fill is paid by few blocks
//   literal  256 pixels per block, 8 blocks per CU: the lone launch_rows' grid (colorlut_kernels.hip)
// Source to destination means order matters across frames, not inside one: colorlut_set_build closes a set in front of a frame that
// meets one already in it (colorlut_frames_meet), and sets run one after the other on the queue's stream.
#include "internal.hpp"
#include "exact_math.hpp"
#include "colorlut_device.hpp"
#include "job_set.hpp"

#include <cstring>
#include <vector>

namespace mi355 {

constexpr JobGrid kClJobGrid = {{512, 256}, {16, 8}};

enum : uint32_t { CL_3D = 1u, CL_ROWPAD = 2u, CL_B16 = 4u, CL_BE = 8u };
struct ClJob {
  const uint8_t *src;
  uint8_t *dst;
  const float *cells;                             // 3D: [size^3][4] as the reference stores it; 1D: r|g|b planes
  uint64_t units;                                 // vector launch: groups of four pixels; literal launch: pixels
  LutK k;                                         // the LUT's domain scale, offset and size
  int32_t width, height, src_stride, dst_stride;
  int32_t format;                                 // MI355_FMT_RGBA / RGBA64_LE / RGBA64_BE
  uint32_t flags;                                 // CL_*: LUT kind, geometry class (vector), sample width and byte order (literal)
  uint32_t first_block, blocks;                   // its blocks in the 1-D grid (hsvdetect_plan)
  uint32_t pad;
};
struct ClJobTable {
  ClJob job[kClSetMax];
  int32_t n_jobs, pad;
};
static_assert(sizeof(LutK) == 28 && sizeof(ClJob) == 96, "ClJob has no padding holes");
static_assert(sizeof(ClJobTable) == kClSetMax * 96 + 8 && sizeof(ClJobTable) <= 4096, "the job table is passed in the kernel arguments");

// per axis and byte value: the cell index floor_idx(x, size - 1) and the weight x - x0 of x = norm_comp(value) * (size - 1)
struct ClAxis {
  uint32_t x0;
  float t;
};
struct ClLds {
  ClAxis axis[3][256];
};
static_assert(sizeof(ClLds) == 6144, "three axes of 256 pairs");

// Filled by a block of 256 threads, one byte value each; the caller synchronises.
__device__ __forceinline__ void colorlut_lds_fill(ClLds *lds, const LutK &k) {
  const float sm1 = (float)k.size - 1.0f;
  const uint32_t max_idx = (uint32_t)k.size - 1;
  const uint32_t v = threadIdx.x;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const float x = norm_comp_generic<false>(k, c, (float)v) * sm1;
    const uint32_t x0 = floor_idx(x, max_idx);
    lds->axis[c][v] = ClAxis{x0, x - (float)x0};
  }
}

template <bool IS3D>
__device__ __forceinline__ uint32_t colorlut_px_lds(uint32_t p, const ClLds *lds, const float *__restrict__ cells, uint32_t size) {
  const ClAxis r = lds->axis[0][p & 0xffu], g = lds->axis[1][(p >> 8) & 0xffu], b = lds->axis[2][(p >> 16) & 0xffu];
  float o[3];
  if constexpr (IS3D) {
    sample_3d_at((const float4 *)cells, size, r.x0, g.x0, b.x0, r.t, g.t, b.t, o);
  } else {
    o[0] = sample_1d_at(cells, size, r.x0, r.t);
    o[1] = sample_1d_at(cells + (size_t)size, size, g.x0, g.t);
    o[2] = sample_1d_at(cells + 2 * (size_t)size, size, b.x0, b.t);
  }
  return (p & 0xff000000u) | rs_as_u8(float_to_u8f(o[0])) | (rs_as_u8(float_to_u8f(o[1])) << 8) | (rs_as_u8(float_to_u8f(o[2])) << 16);
}

// the groups of one job's share
template <bool IS3D>
__device__ __forceinline__ void colorlut_job_groups(const ClJob &J, uint32_t rel, const ClLds *lds) {
  const float *__restrict__ cells = J.cells;
  const uint32_t size = (uint32_t)J.k.size;
  const size_t n = J.units, stride = (size_t)J.blocks * 256;
  if (J.flags & CL_ROWPAD) {
    // padded rows, bases and strides on 16-byte multiples: (row, group of four pixels); the last group of a row may hold 1-3 pixels
    // and only those are read and written
    const uint32_t groups = ((uint32_t)J.width + 3u) >> 2;
    for (size_t i = (size_t)rel * 256 + threadIdx.x; i < n; i += stride) {
      const size_t row = i / groups;
      const uint32_t g = (uint32_t)(i - row * groups);
      const uint8_t *from = J.src + row * (size_t)J.src_stride + (size_t)g * 16;
      uint8_t *to = J.dst + row * (size_t)J.dst_stride + (size_t)g * 16;
      const int left = J.width - (int)(g * 4);
      if (left >= 4) {
        uint4 p = *(const uint4 *)from;
        p.x = colorlut_px_lds<IS3D>(p.x, lds, cells, size); p.y = colorlut_px_lds<IS3D>(p.y, lds, cells, size);
        p.z = colorlut_px_lds<IS3D>(p.z, lds, cells, size); p.w = colorlut_px_lds<IS3D>(p.w, lds, cells, size);
        *(uint4 *)to = p;
      } else {
        for (int q = 0; q < left; q++) ((uint32_t *)to)[q] = colorlut_px_lds<IS3D>(((const uint32_t *)from)[q], lds, cells, size);
      }
    }
  } else {
    const uint4 *__restrict__ src = (const uint4 *)J.src;
    uint4 *__restrict__ dst = (uint4 *)J.dst;
    for (size_t i = (size_t)rel * 256 + threadIdx.x; i < n; i += stride) {
      uint4 p = src[i];
      p.x = colorlut_px_lds<IS3D>(p.x, lds, cells, size); p.y = colorlut_px_lds<IS3D>(p.y, lds, cells, size);
      p.z = colorlut_px_lds<IS3D>(p.z, lds, cells, size); p.w = colorlut_px_lds<IS3D>(p.w, lds, cells, size);
      dst[i] = p;
    }
  }
}

__global__ __launch_bounds__(256) void colorlut_jobs_kernel(const ClJobTable T) {
  const int j = hsvdetect_job_of(T, blockIdx.x);
  const uint32_t rel = blockIdx.x - T.job[j].first_block;
  if (blockIdx.x < T.job[j].first_block || rel >= T.job[j].blocks) return;  // a grid larger than the plan's total: the whole block leaves, before the barrier
  __shared__ ClLds lds;
  colorlut_lds_fill(&lds, T.job[j].k);
  __syncthreads();
  // the job, and with it the LUT's kind, is the block's: every wave takes the same arm
  if (T.job[j].flags & CL_3D) colorlut_job_groups<true>(T.job[j], rel, &lds);
  else colorlut_job_groups<false>(T.job[j], rel, &lds);
}

template <bool IS3D, bool BITS16, bool LE>
__device__ __forceinline__ void colorlut_job_pixels(const ClJob &J, uint32_t rel) {
  const LutK k = J.k;
  const float sm1 = (float)k.size - 1.0f;
  const size_t total = J.units, width = (size_t)J.width, stride = (size_t)J.blocks * 256;
  for (size_t i = (size_t)rel * 256 + threadIdx.x; i < total; i += stride) {
    const size_t row = i / width;
    const size_t col = i - row * width;
    colorlut_px_literal<IS3D, BITS16, LE>(J.src, J.src_stride, J.dst, J.dst_stride, row, col, J.cells, k, sm1);
  }
}

__global__ __launch_bounds__(256) void colorlut_rows_jobs_kernel(const ClJobTable T) {
  const int j = hsvdetect_job_of(T, blockIdx.x);
  const uint32_t rel = blockIdx.x - T.job[j].first_block;
  if (blockIdx.x < T.job[j].first_block || rel >= T.job[j].blocks) return;  // a grid larger than the plan's total
  // (the instance the lone launch_rows picks for the job's LUT kind and format)
  switch (T.job[j].flags & (CL_3D | CL_B16 | CL_BE)) {
    case CL_3D: colorlut_job_pixels<true, false, true>(T.job[j], rel); break;
    case 0: colorlut_job_pixels<false, false, true>(T.job[j], rel); break;
    case CL_3D | CL_B16: colorlut_job_pixels<true, true, true>(T.job[j], rel); break;
    case CL_B16: colorlut_job_pixels<false, true, true>(T.job[j], rel); break;
    case CL_3D | CL_B16 | CL_BE: colorlut_job_pixels<true, true, false>(T.job[j], rel); break;
    case CL_B16 | CL_BE: colorlut_job_pixels<false, true, false>(T.job[j], rel); break;
    default: break;  // (RGBA8 has no byte order: CL_BE is never set without CL_B16)
  }
}

// ---------------------------------------------------------------- host side

namespace {
int cl_bpp(const ClFrame &f) { return f.format == MI355_FMT_RGBA ? 4 : 8; }
bool cl_has_pixel(const ClFrame &f) { return f.width > 0 && f.height > 0; }
size_t cl_span(const ClFrame &f, int stride) { return (size_t)(f.height - 1) * (size_t)stride + (size_t)f.width * (size_t)cl_bpp(f); }
bool cl_ranges_meet(const uint8_t *a, size_t a_bytes, const uint8_t *b, size_t b_bytes) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}
}  // namespace

bool colorlut_frame_in_place(const ClFrame &f) {
  return cl_has_pixel(f) && cl_ranges_meet(f.src, cl_span(f, f.src_stride), f.dst, cl_span(f, f.dst_stride));
}

bool colorlut_frames_meet(const ClFrame &a, const ClFrame &b) {
  if (!cl_has_pixel(a) || !cl_has_pixel(b)) return false;  // no pixel, no byte
  const size_t a_src = cl_span(a, a.src_stride), a_dst = cl_span(a, a.dst_stride), b_src = cl_span(b, b.src_stride), b_dst = cl_span(b, b.dst_stride);
  return cl_ranges_meet(b.dst, b_dst, a.src, a_src) || cl_ranges_meet(b.dst, b_dst, a.dst, a_dst) || cl_ranges_meet(b.src, b_src, a.dst, a_dst);
}

// The ONE builder of launch sets, for colorlut_launch_set and mi355_selftest_colorlut_set_plan alike: closes a set at kClSetMax frames
// and in front of a frame that meets one already in it, classifies each set's frames into its two tables and has JobSet plan the
// blocks. The frames' addresses are numbers here: nothing is dereferenced. `out` (per frame) may be null.
typedef JobSet<ClJobTable> ClSet;
static int colorlut_set_build(int n_cu, const ClFrame *frames, int n, std::vector<ClSet> *sets, mi355_colorlut_plan_out *out) {
  sets->clear();
  if (n_cu < 1 || n < 0 || (n && !frames)) return MI355_ERR_INVALID_ARG;
  for (int begin = 0; begin < n;) {
    int end = begin;
    for (; end < n && end - begin < kClSetMax; end++) {
      bool meets = false;
      for (int e = begin; e < end && !meets; e++) meets = colorlut_frames_meet(frames[e], frames[end]);
      if (meets) break;
    }
    sets->emplace_back();
    ClSet &S = sets->back();
    std::memset(&S, 0, sizeof(S));
    for (int i = begin; i < end; i++) {
      const ClFrame &f = frames[i];
      if (out) out[i] = mi355_colorlut_plan_out{(int32_t)sets->size() - 1, 0, 0, 0, 0, 0, 0};
      if (!cl_has_pixel(f)) continue;  // no pixel: no job
      const bool rgba8 = f.format == MI355_FMT_RGBA;
      const size_t row_bytes = (size_t)f.width * 4, total_bytes = row_bytes * (size_t)f.height;
      const uintptr_t from = (uintptr_t)f.src, to = (uintptr_t)f.dst;
      const bool based = from % 16 == 0 && to % 16 == 0;
      const bool flat = based && (size_t)f.src_stride == row_bytes && (size_t)f.dst_stride == row_bytes && total_bytes % 16 == 0;
      const bool rowpad = !flat && based && f.src_stride % 16 == 0 && f.dst_stride % 16 == 0;
      const bool vector = rgba8 && !f.force_generic && (flat || rowpad);
      ClJobTable &T = S.table[vector ? kVec : kLit];
      ClJob &J = T.job[T.n_jobs++];
      J.src = f.src;
      J.dst = f.dst;
      J.cells = f.cells;
      for (int c = 0; c < 3; c++) { J.k.scale[c] = f.scale[c]; J.k.offset[c] = f.offset[c]; }
      J.k.size = f.size;
      J.width = f.width;
      J.height = f.height;
      J.src_stride = f.src_stride;
      J.dst_stride = f.dst_stride;
      J.format = f.format;
      J.flags = (f.is3d ? CL_3D : 0u) | (rgba8 ? 0u : CL_B16) | (f.format == MI355_FMT_RGBA64_BE ? CL_BE : 0u);
      if (vector) {
        if (rowpad) J.flags |= CL_ROWPAD;
        J.units = rowpad ? (uint64_t)(((uint32_t)f.width + 3u) / 4u) * (uint64_t)f.height : total_bytes / 16;
      } else {
        J.units = (uint64_t)f.width * (uint64_t)f.height;
      }
      if (out) { out[i].launch = 1 + (vector ? kVec : kLit); out[i].geometry = vector ? (rowpad ? 2 : 1) : 0; out[i].units = J.units; }
    }
    if (const int rc = S.plan(n_cu, kClJobGrid)) return rc;
    int next[2] = {0, 0};   // a table's jobs are in the order of their frames
    for (int i = begin; out && i < end; i++) {
      if (!out[i].launch) continue;
      const ClJob &J = S.table[out[i].launch - 1].job[next[out[i].launch - 1]++];
      out[i].first_block = J.first_block;
      out[i].blocks = J.blocks;
    }
    begin = end;
  }
  return MI355_OK;
}

int colorlut_set_plan(int n_cu, const ClFrame *frames, int n, mi355_colorlut_plan_out *out, int *n_sets) {
  std::vector<ClSet> sets;
  const int rc = colorlut_set_build(n_cu, frames, n, &sets, out);
  if (!rc) *n_sets = (int)sets.size();
  return rc;
}

int colorlut_launch_set(hipStream_t stream, int n_cu, const ClFrame *frames, int n, int *kernel_launches, std::string *err) {
  *kernel_launches = 0;
  if (!frames || n < 1 || n > kClSetMax) { *err = "colorlut: bad launch set"; return MI355_ERR_INVALID_ARG; }
  std::vector<ClSet> sets;
  if (const int rc = colorlut_set_build(n_cu, frames, n, &sets, nullptr)) { *err = "colorlut: bad launch set"; return rc; }
  // (one set, unless the caller handed over frames that meet: then their sets, in order on the one stream)
  for (const ClSet &S : sets)
    if (const int rc = S.launch(stream, {colorlut_jobs_kernel, colorlut_rows_jobs_kernel}, {"colorlut jobs kernel launch: ", "colorlut rows jobs kernel launch: "}, kernel_launches, err)) return rc;
  return MI355_OK;
}

}  // namespace mi355
