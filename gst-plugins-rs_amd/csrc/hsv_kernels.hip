// hsv_kernels.hip — gfx950 kernels for hsvfilter / hsvdetector.
//
// Reference loops replaced (gst-plugins-rs tree):
//   video/hsv/src/hsvutils.rs:44-128    from_rgb / from_bgr
//   video/hsv/src/hsvutils.rs:132-198   to_rgb / to_bgr
//   video/hsv/src/hsvfilter/imp.rs:96-118     per-pixel filter body
//   video/hsv/src/hsvdetector/imp.rs:126-156  per-pixel detector body
//
// Two arithmetic variants per kernel:
//   GENERIC — literal transliteration (IEEE `/`, fmodf, every branch incl. NaN/inf settings).
//   FAST    — strength-reduced but bit-identical for `hue_shift == 0 || 1e-30 <= |hue_shift| <= 360`
//             (finite): exact constant divisions (exact_math.hpp), rcp+residual quotients,
//             bounded-range fmod, sextant select as one LDS lookup + v_perm_b32.
//             Facts it relies on, all checked exhaustively over the 2^24 colours by the tests:
//             hue in [0,360) before the shift (so `hue % 360` is the identity), saturation and
//             value already inside [0,1], results of to_rgb inside [0,255.0001].
// The pixel filters are pure streaming kernels: 4 B read + 4 B written per pixel, HBM-bound
// once the VALU work per pixel is below ~80 instructions.
#include "internal.hpp"
#include "exact_math.hpp"
#include "hsv_device.hpp"
#include "job_set.hpp"

namespace mi355 {

// ---------------------------------------------------------------- hsvfilter kernels

// Four pixels of one lane through the filter. FAST variants: two calls of the pair routine with the block's HsvLds;
// GENERIC: the pair routine's settings-independent from_rgb (exact for every colour, all-colours tests) followed by the
// literal fmodf / `/ 60` / sextant chain, which is what non-finite and out-of-range hue shifts need.
template <int VARIANT, int RPOS, int GPOS, int BPOS, int NPOS>
__device__ __forceinline__ void hsvfilter_quad(uint32_t &a, uint32_t &b, uint32_t &c, uint32_t &d, const HsvK &k, const HsvLds *lds) {
  if constexpr (VARIANT >= 0) {
    hsvfilter_px2_lds<RPOS, GPOS, BPOS, NPOS, hsv_shift_of(VARIANT), hsv_sv_ident_of(VARIANT)>(a, b, k, lds);
    hsvfilter_px2_lds<RPOS, GPOS, BPOS, NPOS, hsv_shift_of(VARIANT), hsv_sv_ident_of(VARIANT)>(c, d, k, lds);
  } else {
    hsvfilter_px2_generic<RPOS, GPOS, BPOS, NPOS>(a, b, k, lds);
    hsvfilter_px2_generic<RPOS, GPOS, BPOS, NPOS>(c, d, k, lds);
  }
}

// MI355_FLAG_HSV_NT = 2: a lane's 16 bytes as ONE global_store_dwordx4 that carries the system scope (sc0 sc1) and no nt bit. The L2
// writes the line through as it takes it, so the kernel ends with no dirty backlog for its release to drain, and the line still
// allocates in the memory-side Infinity Cache, where the launch behind finds it. The compiler has no spelling for this store: a
// relaxed system-scope atomic gives the bits but is four dword stores, volatile gives them with a wait for every store. The
// s_nop is the wait state a store of more than 8 bytes needs before a VALU instruction may overwrite its data registers - the
// compiler inserts it behind its own stores and cannot see into this one. Ordered like any store: the kernel's end releases it.
__device__ __forceinline__ void hsv_store_through(uint4 *at, const uint4 &p) {
  typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
  const u32x4_t o = {p.x, p.y, p.z, p.w};
  asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 0" : : "v"(at), "v"(o) : "memory");
}

// Flat streaming kernel for 4-byte formats on contiguous storage (stride == width*4 and frames
// back to back): each lane owns 16 B (4 pixels) per iteration -> global_load/store_dwordx4.
// VARIANT: -1 = GENERIC arithmetic; otherwise FAST, see hsv_shift_of / hsv_sv_ident_of.
// nt (MI355_FLAG_HSV_NT): 2, the default, plain loads and write-through stores (hsv_store_through): 0.0823 against 0.0858 ms with
// plain stores (0), the chain 44.9-45.7 k against 44.0-44.6 k frames/s, in turn on one box (profiles/r07_store_policy_ab.txt).
// No non-temporal hint on purpose: with it on loads and stores (1) this kernel alone is 2-5 % faster than with plain ones (0.086
// against 0.091 ms for the bare read-modify-write of 8 x 4K frames, tools/hsv_mem_probe.hip), but its output then bypasses the
// Infinity Cache and the element behind it reads from HBM: colorlut 0.115 instead of 0.087 ms, the chain 38.5 k instead of
// 44.4 k frames/s (r03, bench.py). One load in flight per lane: two measured the same or slower once the arithmetic had
// shrunk (63 VGPRs, 8 waves per SIMD cover the latency).
template <int VARIANT, int FIRST, bool BGR>
__global__ __launch_bounds__(256) void hsvfilter_flat_kernel(uint4 *__restrict__ data, size_t n_vec,
                                                             HsvK k, int nt) {
  constexpr int RPOS = FIRST + (BGR ? 2 : 0), GPOS = FIRST + 1, BPOS = FIRST + (BGR ? 0 : 2);
  constexpr int NPOS = FIRST == 0 ? 3 : 0;
  __shared__ HsvLds lds;
  hsv_lds_fill<RPOS, GPOS, BPOS, NPOS>(&lds);
  __syncthreads();
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  if (nt == 2) {  // MI355_FLAG_HSV_NT = 2: plain loads, write-through stores that stay in the Infinity Cache (hsv_store_through)
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_vec; i += stride) {
      uint4 p = data[i];
      hsvfilter_quad<VARIANT, RPOS, GPOS, BPOS, NPOS>(p.x, p.y, p.z, p.w, k, &lds);
      hsv_store_through(data + i, p);
    }
    return;
  }
  if (nt) {  // MI355_FLAG_HSV_NT = 1 (the A/B of bench.py: what the chain costs when this launch's output bypasses the Infinity Cache)
    typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
    u32x4_t *d4 = (u32x4_t *)data;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_vec; i += stride) {
      const u32x4_t v = __builtin_nontemporal_load(d4 + i);
      uint4 p = {v.x, v.y, v.z, v.w};
      hsvfilter_quad<VARIANT, RPOS, GPOS, BPOS, NPOS>(p.x, p.y, p.z, p.w, k, &lds);
      const u32x4_t o = {p.x, p.y, p.z, p.w};
      __builtin_nontemporal_store(o, d4 + i);
    }
    return;
  }
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_vec; i += stride) {
    uint4 p = data[i];
    hsvfilter_quad<VARIANT, RPOS, GPOS, BPOS, NPOS>(p.x, p.y, p.z, p.w, k, &lds);
    data[i] = p;
  }
}

// The flat kernel over up to kMultiFrames SEPARATE frames of one size (blockIdx.y = frame): the frames of different streams
// batched into one launch by the group dispatcher (group.hip), so that a frame does not pay the ramp and the tail of a launch
// of its own. Same arithmetic, same per-lane work; through != 0: the stores of MI355_FLAG_HSV_NT = 2, as the lone kernel's.
template <int VARIANT, int FIRST, bool BGR>
__global__ __launch_bounds__(256) void hsvfilter_flat_multi_kernel(MultiFramePtrs frames, size_t n_vec, HsvK k, int through) {
  constexpr int RPOS = FIRST + (BGR ? 2 : 0), GPOS = FIRST + 1, BPOS = FIRST + (BGR ? 0 : 2);
  constexpr int NPOS = FIRST == 0 ? 3 : 0;
  __shared__ HsvLds lds;
  hsv_lds_fill<RPOS, GPOS, BPOS, NPOS>(&lds);
  __syncthreads();
  uint4 *__restrict__ data = (uint4 *)frames.p[blockIdx.y];
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_vec; i += stride) {
    uint4 p = data[i];
    hsvfilter_quad<VARIANT, RPOS, GPOS, BPOS, NPOS>(p.x, p.y, p.z, p.w, k, &lds);
    if (through) hsv_store_through(data + i, p);  // (the launch's: every wave takes the same side)
    else data[i] = p;
  }
}

// 4-byte formats with padded rows and / or frame pitches (what real caps negotiate when upstream aligns strides):
// the same 16 B per lane, addressed as (frame, row, 4-pixel group). Needs base, stride and pitch to be multiples of 16;
// the last group of a row may hold 1-3 pixels: its padding bytes are read, filtered as pixels and NOT written back
// (only `line[..width*4]` of a row is touched, hsvfilter/imp.rs:94-97).
template <int VARIANT, int FIRST, bool BGR>
__global__ __launch_bounds__(256) void hsvfilter_strided_kernel(uint8_t *__restrict__ data, int n_frames, size_t frame_pitch, int width,
                                                                int height, int stride, HsvK k) {
  constexpr int RPOS = FIRST + (BGR ? 2 : 0), GPOS = FIRST + 1, BPOS = FIRST + (BGR ? 0 : 2);
  constexpr int NPOS = FIRST == 0 ? 3 : 0;
  __shared__ HsvLds lds;
  hsv_lds_fill<RPOS, GPOS, BPOS, NPOS>(&lds);
  __syncthreads();
  const uint32_t groups = ((uint32_t)width + 3u) >> 2;  // per row
  const size_t rows = (size_t)height * (size_t)n_frames;
  const size_t total = rows * groups;
  const size_t gstride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gstride) {
    const size_t rowi = i / groups;
    const uint32_t g = (uint32_t)(i - rowi * groups);
    const size_t f = rowi / (size_t)height;
    const size_t row = rowi - f * (size_t)height;
    uint8_t *at = data + f * frame_pitch + row * (size_t)stride + (size_t)g * 16;
    const int left = width - (int)(g * 4);  // pixels of this group inside the row
    if (left >= 4) {
      uint4 p = *(const uint4 *)at;
      hsvfilter_quad<VARIANT, RPOS, GPOS, BPOS, NPOS>(p.x, p.y, p.z, p.w, k, &lds);
      *(uint4 *)at = p;
    } else {
      // the row's bytes end inside this group: read only what belongs to the row
      uint32_t px[4] = {0, 0, 0, 0};
      for (int j = 0; j < left; j++) px[j] = ((const uint32_t *)at)[j];
      hsvfilter_quad<VARIANT, RPOS, GPOS, BPOS, NPOS>(px[0], px[1], px[2], px[3], k, &lds);
      for (int j = 0; j < left; j++) ((uint32_t *)at)[j] = px[j];
    }
  }
}

// The same for the common case of padded ROWS only (frame_pitch == stride * height: one tall picture of rows_total rows), without
// the two 64-bit divisions per lane and iteration of the kernel above (~200 instructions next to the 146 of the four pixels): a
// block is 64 lanes x 4 rows, blockIdx.x picks 64 groups of the row (1 KB contiguous per wave), blockIdx.y strides over the rows.
// Round 5: 65 % -> see profiles/r05_configs_elements.txt.
template <int VARIANT, int FIRST, bool BGR>
__global__ __launch_bounds__(256) void hsvfilter_rowpad_kernel(uint8_t *__restrict__ data, unsigned rows_total, int width, int stride, HsvK k) {
  constexpr int RPOS = FIRST + (BGR ? 2 : 0), GPOS = FIRST + 1, BPOS = FIRST + (BGR ? 0 : 2);
  constexpr int NPOS = FIRST == 0 ? 3 : 0;
  __shared__ HsvLds lds;
  hsv_lds_fill<RPOS, GPOS, BPOS, NPOS>(&lds);
  __syncthreads();
  const uint32_t groups = ((uint32_t)width + 3u) >> 2;
  const uint32_t g = blockIdx.x * 64u + (threadIdx.x & 63u);
  if (g >= groups) return;
  const int left = width - (int)(g * 4);  // pixels of this group inside the row
  for (uint32_t r = blockIdx.y * 4u + (threadIdx.x >> 6); r < rows_total; r += gridDim.y * 4u) {
    uint8_t *at = data + (size_t)r * (size_t)stride + (size_t)g * 16;
    if (left >= 4) {
      uint4 p = *(const uint4 *)at;
      hsvfilter_quad<VARIANT, RPOS, GPOS, BPOS, NPOS>(p.x, p.y, p.z, p.w, k, &lds);
      *(uint4 *)at = p;
    } else {
      uint32_t px[4] = {0, 0, 0, 0};
      for (int j = 0; j < left; j++) px[j] = ((const uint32_t *)at)[j];
      hsvfilter_quad<VARIANT, RPOS, GPOS, BPOS, NPOS>(px[0], px[1], px[2], px[3], k, &lds);
      for (int j = 0; j < left; j++) ((uint32_t *)at)[j] = px[j];
    }
  }
}

// 3-byte formats (RGB / BGR) on contiguous storage: one lane = 12 B = 4 pixels. The three dwords are
// split into four pixel words with v_alignbit-style shifts, filtered by the same pair routine as the
// 4-byte formats (byte 3 of each word is scratch) and re-packed.
struct Rgb24x4 { uint32_t d0, d1, d2; };
template <int VARIANT, bool BGR>
__global__ __launch_bounds__(256) void hsvfilter_rgb24_kernel(Rgb24x4 *__restrict__ data, size_t n_grp, HsvK k) {
  constexpr int RPOS = BGR ? 2 : 0, GPOS = 1, BPOS = BGR ? 0 : 2, NPOS = 3;
  __shared__ HsvLds lds;
  hsv_lds_fill<RPOS, GPOS, BPOS, NPOS>(&lds);
  __syncthreads();
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_grp; i += stride) {
    const Rgb24x4 v = data[i];
    uint32_t p0 = v.d0, p1 = (v.d0 >> 24) | (v.d1 << 8), p2 = (v.d1 >> 16) | (v.d2 << 16), p3 = v.d2 >> 8;
    hsvfilter_quad<VARIANT, RPOS, GPOS, BPOS, NPOS>(p0, p1, p2, p3, k, &lds);
    Rgb24x4 o;
    o.d0 = (p0 & 0x00ffffffu) | (p1 << 24);
    o.d1 = ((p1 >> 8) & 0x0000ffffu) | (p2 << 16);
    o.d2 = ((p2 >> 16) & 0x000000ffu) | (p3 << 8);
    data[i] = o;
  }
}

// The same formats with fully coalesced memory accesses (round 3; the 12-byte-per-lane form above moves 42-57 % of the
// HBM peak, its dwordx3 accesses leave every fourth dword slot of the memory pipeline empty): a wave takes 3 KB = 1024 pixels
// per iteration as three 16-byte loads per lane (lane l: bytes [16 l, 16 l + 16) of each 1 KB third), passes them through
// a wave-private 3 KB LDS strip so that lane l owns the 48 contiguous bytes of pixels 16 l .. 16 l + 15 (ds_read_b128 at a
// 48-byte lane stride: the 16 lanes of a pass start on 16 different 4-bank groups), filters them with the pair routine
// and sends them back the same way. The caller gives whole 3 KB chunks; the remainder goes to the kernel above.
template <int VARIANT, bool BGR>
__global__ __launch_bounds__(256) void hsvfilter_rgb24x16_kernel(uint4 *__restrict__ data, size_t n_chunks, HsvK k) {
  constexpr int RPOS = BGR ? 2 : 0, GPOS = 1, BPOS = BGR ? 0 : 2, NPOS = 3;
  __shared__ HsvLds lds;
  __shared__ uint4 strip[4][192];
  hsv_lds_fill<RPOS, GPOS, BPOS, NPOS>(&lds);
  __syncthreads();
  const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  uint4 *x = strip[wave];
  auto wave_sync = [] {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  };
  const size_t n_waves = (size_t)gridDim.x * 4;
  size_t c = (size_t)blockIdx.x * 4 + wave;
  if (c >= n_chunks) return;
  uint4 a0 = data[c * 192 + lane], a1 = data[c * 192 + 64 + lane], a2 = data[c * 192 + 128 + lane];
  for (; c < n_chunks; c += n_waves) {
    uint4 *base = data + c * 192;
    // the next chunk's loads are in flight while this one is worked on (16 pixels per lane are ~600 VALU instructions:
    // without the prefetch a wave has nothing outstanding for four fifths of its time)
    const size_t cn = c + n_waves < n_chunks ? c + n_waves : c;
    const uint4 n0 = data[cn * 192 + lane], n1 = data[cn * 192 + 64 + lane], n2 = data[cn * 192 + 128 + lane];
    x[lane] = a0;
    x[64 + lane] = a1;
    x[128 + lane] = a2;
    wave_sync();
    uint4 v[3] = {x[3 * lane], x[3 * lane + 1], x[3 * lane + 2]};  // 12 dwords = 16 pixels
    wave_sync();
    uint32_t *d = (uint32_t *)v;
#pragma unroll
    for (int q = 0; q < 4; q++) {  // four pixels = three dwords at a time
      const uint32_t d0 = d[3 * q], d1 = d[3 * q + 1], d2 = d[3 * q + 2];
      uint32_t p0 = d0, p1 = (d0 >> 24) | (d1 << 8), p2 = (d1 >> 16) | (d2 << 16), p3 = d2 >> 8;
      hsvfilter_quad<VARIANT, RPOS, GPOS, BPOS, NPOS>(p0, p1, p2, p3, k, &lds);
      d[3 * q] = (p0 & 0x00ffffffu) | (p1 << 24);
      d[3 * q + 1] = ((p1 >> 8) & 0x0000ffffu) | (p2 << 16);
      d[3 * q + 2] = ((p2 >> 16) & 0x000000ffu) | (p3 << 8);
    }
    x[3 * lane] = v[0];
    x[3 * lane + 1] = v[1];
    x[3 * lane + 2] = v[2];
    wave_sync();
    base[lane] = x[lane];
    base[64 + lane] = x[64 + lane];
    base[128 + lane] = x[128 + lane];
    wave_sync();
    a0 = n0; a1 = n1; a2 = n2;
  }
}

// General kernel: any stride / pixel stride (3 or 4) / triple offset / alignment, one pixel per lane, byte
// accesses. Only `line[..width*pixel_stride]` of each row is touched (hsvfilter/imp.rs:94-97).
template <bool FAST>
__global__ __launch_bounds__(256) void hsvfilter_rows_kernel(uint8_t *__restrict__ data, int n_frames,
                                                             size_t frame_pitch, int width, int height,
                                                             int stride, int pixel_stride, int first,
                                                             int bgr, HsvK k) {
  __shared__ uint32_t sel_tab[8];
  if (threadIdx.x < 7) sel_tab[threadIdx.x] = hsv_sel_entry(threadIdx.x, 0, 1, 2, 3);
  __syncthreads();
  const size_t per_frame = (size_t)width * (size_t)height;
  const size_t total = per_frame * (size_t)n_frames;
  const size_t gstride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gstride) {
    const size_t f = i / per_frame;
    const size_t r = i - f * per_frame;
    const size_t row = r / (size_t)width;
    const size_t col = r - row * (size_t)width;
    uint8_t *px = data + f * frame_pitch + row * (size_t)stride + col * (size_t)pixel_stride + first;
    const uint32_t c0 = px[0], c1 = px[1], c2 = px[2];
    const uint32_t p = bgr ? (c2 | (c1 << 8) | (c0 << 16)) : (c0 | (c1 << 8) | (c2 << 16));
    const uint32_t o = hsvfilter_px<FAST, 0, 1, 2, 3>(p, k, sel_tab);
    const uint8_t orr = (uint8_t)(o & 0xff), og = (uint8_t)((o >> 8) & 0xff), ob = (uint8_t)((o >> 16) & 0xff);
    px[0] = bgr ? ob : orr;
    px[1] = og;
    px[2] = bgr ? orr : ob;
  }
}

static int grid_for(mi355_ctx *ctx, size_t work_items, int block, int blocks_per_cu) {
  size_t blocks = (work_items + (size_t)block - 1) / (size_t)block;
  size_t cap = (size_t)ctx->n_cu * (size_t)blocks_per_cu;
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  return (int)blocks;
}

// ---- run-time value -> template argument, each conversion written once. A launcher nests the helpers it needs around its ONE
// hipLaunchKernelGGL line; f is a generic lambda and gets std::integral_constant / std::bool_constant values.

// the variant number of hsv_variant_for: -1 = GENERIC, the nine narrow FAST classes by number, every other number is 13
template <class F>
static void with_variant(int variant, F &&f) {
  switch (variant) {
    case -1: f(std::integral_constant<int, -1>{}); break;
    case 0: f(std::integral_constant<int, 0>{}); break;
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 5: f(std::integral_constant<int, 5>{}); break;
    case 6: f(std::integral_constant<int, 6>{}); break;
    case 8: f(std::integral_constant<int, 8>{}); break;
    case 9: f(std::integral_constant<int, 9>{}); break;
    case 12: f(std::integral_constant<int, 12>{}); break;
    default: f(std::integral_constant<int, 13>{}); break;
  }
}

// a two-way choice: the 3-byte formats' byte order, the detector's offset class, the rows kernels' FAST
template <class F>
static void with_flag(bool on, F &&f) {
  if (on) f(std::true_type{});
  else f(std::false_type{});
}

// the byte order of a 4-byte format: f(FIRST, BGR), FIRST = 0 (RGBx, BGRx) or 1 (xRGB, xBGR)
template <class F>
static void with_byte_order(int first, int bgr, F &&f) {
  if (first == 0 && !bgr) f(std::integral_constant<int, 0>{}, std::false_type{});
  else if (first == 0 && bgr) f(std::integral_constant<int, 0>{}, std::true_type{});
  else if (first == 1 && !bgr) f(std::integral_constant<int, 1>{}, std::false_type{});
  else f(std::integral_constant<int, 1>{}, std::true_type{});
}

static void launch_flat(mi355_ctx *ctx, int variant, uint4 *d, size_t n_vec, const HsvK &k, int first, int bgr, int grid) {
  const int nt = ctx->hsv_nt;
  with_variant(variant, [&](auto V) { with_byte_order(first, bgr, [&](auto FIRST, auto BGR) {
    hipLaunchKernelGGL((hsvfilter_flat_kernel<V, FIRST, BGR>), dim3(grid), dim3(256), 0, ctx->stream, d, n_vec, k, nt);
  }); });
}

static void launch_strided(mi355_ctx *ctx, int variant, uint8_t *d, int n_frames, size_t frame_pitch, int width, int height, int stride, const HsvK &k,
                           int first, int bgr, int grid) {
  // padded rows only: the batch is one tall picture, for the rowpad kernel and its (gx, gy) grid; else the strided kernel on `grid`
  const bool tall = (n_frames == 1 || frame_pitch == (size_t)stride * (size_t)height) && (size_t)n_frames * (size_t)height < (1u << 31);
  const unsigned rows_total = (unsigned)n_frames * (unsigned)height, gx = ((unsigned)(width + 3) / 4 + 63) / 64;
  unsigned gy = (rows_total + 3) / 4;
  const unsigned cap = (unsigned)ctx->n_cu * (unsigned)ctx->hsv_blocks_per_cu / (gx ? gx : 1) + 1;
  if (gy > cap) gy = cap;
  if (gy > 65535) gy = 65535;
  with_variant(variant, [&](auto V) {
    if (tall) {
      with_byte_order(first, bgr, [&](auto FIRST, auto BGR) {
        hipLaunchKernelGGL((hsvfilter_rowpad_kernel<V, FIRST, BGR>), dim3(gx, gy), dim3(256), 0, ctx->stream, d, rows_total, width, stride, k);
      });
    } else {
      with_byte_order(first, bgr, [&](auto FIRST, auto BGR) {
        hipLaunchKernelGGL((hsvfilter_strided_kernel<V, FIRST, BGR>), dim3(grid), dim3(256), 0, ctx->stream, d, n_frames, frame_pitch, width, height, stride, k);
      });
    }
  });
}

static void launch_rgb24x16(mi355_ctx *ctx, int variant, uint4 *d, size_t n_chunks, const HsvK &k, int bgr, int grid) {
  with_variant(variant, [&](auto V) { with_flag(bgr != 0, [&](auto BGR) {
    hipLaunchKernelGGL((hsvfilter_rgb24x16_kernel<V, BGR>), dim3(grid), dim3(256), 0, ctx->stream, d, n_chunks, k);
  }); });
}

static void launch_rgb24(mi355_ctx *ctx, int variant, Rgb24x4 *d, size_t n_grp, const HsvK &k, int bgr, int grid) {
  with_variant(variant, [&](auto V) { with_flag(bgr != 0, [&](auto BGR) {
    hipLaunchKernelGGL((hsvfilter_rgb24_kernel<V, BGR>), dim3(grid), dim3(256), 0, ctx->stream, d, n_grp, k);
  }); });
}

int launch_hsvfilter_compute(mi355_ctx *ctx, uint8_t *d_data, int n_frames, size_t frame_pitch, int width,
                     int height, int stride, const PixFmt &fmt, const mi355_hsv_settings &s) {
  if (n_frames <= 0 || width <= 0 || height <= 0) return MI355_OK;  // nothing to do
  const HsvK k{s.hue_shift, s.saturation_mul, s.saturation_off, s.value_mul, s.value_off};
  const int variant = hsv_variant_for(s, ctx->force_generic, true);
  const size_t row_bytes = (size_t)width * (size_t)fmt.pixel_stride;
  const bool packed_rows = (size_t)stride == row_bytes && (n_frames == 1 || frame_pitch == row_bytes * (size_t)height);
  const size_t total_bytes = row_bytes * (size_t)height * (size_t)n_frames;
  if (fmt.pixel_stride == 4 && packed_rows && ((uintptr_t)d_data % 16 == 0) && (total_bytes % 16 == 0)) {
    const size_t n_vec = total_bytes / 16;
    // at least two 16-byte groups per lane: a block pays its LDS tables and its ramp once, and launches of one or two frames
    // (one stream's buffer) are 10-15 % faster than with one group per lane (tools/r03_single_frame_launch.py)
    const int grid = grid_for(ctx, (n_vec + 1) / 2, 256, ctx->hsv_blocks_per_cu);
    uint4 *d = (uint4 *)d_data;
    launch_flat(ctx, variant, d, n_vec, k, fmt.first, fmt.bgr, grid);
  } else if (fmt.pixel_stride == 4 && ((uintptr_t)d_data % 16 == 0) && stride % 16 == 0 && (n_frames == 1 || frame_pitch % 16 == 0)) {
    const size_t n_grp = (size_t)((width + 3) / 4) * (size_t)height * (size_t)n_frames;
    const int grid = grid_for(ctx, (n_grp + 1) / 2, 256, ctx->hsv_blocks_per_cu);
    launch_strided(ctx, variant, d_data, n_frames, frame_pitch, width, height, stride, k, fmt.first, fmt.bgr, grid);
  } else if (fmt.pixel_stride == 3 && fmt.first == 0 && packed_rows && ((uintptr_t)d_data % 4 == 0) && (total_bytes % 12 == 0)) {
    // whole 3 KB chunks (1024 pixels) through the coalescing kernel when the base is 16-byte aligned, the rest 12 bytes per lane
    const size_t n_chunks = ((uintptr_t)d_data % 16 == 0) ? total_bytes / 3072 : 0;
    if (n_chunks) {
      const int grid = grid_for(ctx, n_chunks * 64, 256, ctx->hsv_blocks_per_cu / 2);
      launch_rgb24x16(ctx, variant, (uint4 *)d_data, n_chunks, k, fmt.bgr, grid);
    }
    const size_t n_grp = (total_bytes - n_chunks * 3072) / 12;
    if (n_grp) {
      const int grid = grid_for(ctx, n_grp, 256, ctx->hsv_blocks_per_cu);
      Rgb24x4 *d = (Rgb24x4 *)(d_data + n_chunks * 3072);
      launch_rgb24(ctx, variant, d, n_grp, k, fmt.bgr, grid);
    }
  } else {
    const size_t total = (size_t)width * (size_t)height * (size_t)n_frames;
    const int grid = grid_for(ctx, total, 256, 32);
    // one pixel per lane: the single-pixel FAST routine knows the narrow shift classes only
    with_flag(hsv_variant_for(s, ctx->force_generic, false) >= 0, [&](auto FAST) {
      hipLaunchKernelGGL((hsvfilter_rows_kernel<FAST>), dim3(grid), dim3(256), 0, ctx->stream, d_data, n_frames,
                         frame_pitch, width, height, stride, fmt.pixel_stride, fmt.first, fmt.bgr, k);
    });
  }
  return check_hip(ctx, hipGetLastError(), "hsvfilter kernel launch");
}

// hsvfilter in place on n separate packed frames of one size and format with one set of settings, ONE launch on `stream`
// (group.hip). false if the geometry is not the flat kernel's (the caller then goes frame by frame through launch_hsvfilter).
bool hsvfilter_multi_applicable(const uint8_t *const *frames, int n_frames, int width, int height, int stride, const PixFmt &fmt) {
  if (n_frames < 1 || n_frames > kMultiFrames || width <= 0 || height <= 0 || fmt.pixel_stride != 4 || (size_t)stride != (size_t)width * 4) return false;
  if (((size_t)width * 4 * (size_t)height) % 16 != 0) return false;
  for (int f = 0; f < n_frames; f++)
    if (!frames[f] || (uintptr_t)frames[f] % 16 != 0) return false;
  return true;
}
static void launch_flat_multi(hipStream_t stream, int variant, const MultiFramePtrs &frames, int n_frames, size_t n_vec, const HsvK &k, int first, int bgr, int grid_x,
                              int through) {
  with_variant(variant, [&](auto V) { with_byte_order(first, bgr, [&](auto FIRST, auto BGR) {
    hipLaunchKernelGGL((hsvfilter_flat_multi_kernel<V, FIRST, BGR>), dim3(grid_x, n_frames), dim3(256), 0, stream, frames, n_vec, k, through);
  }); });
}
int launch_hsvfilter_multi(mi355_ctx *ctx, hipStream_t stream, uint8_t *const *frames, int n_frames, int width, int height, const PixFmt &fmt,
                           const mi355_hsv_settings &s) {
  const HsvK k{s.hue_shift, s.saturation_mul, s.saturation_off, s.value_mul, s.value_off};
  const int variant = hsv_variant_for(s, ctx->force_generic, true);
  const size_t n_vec = (size_t)width * 4 * (size_t)height / 16;
  MultiFramePtrs ptrs{};
  for (int f = 0; f < n_frames; f++) ptrs.p[f] = frames[f];
  // the same total grid as one launch over n contiguous frames would get, split evenly over the frames
  int gx = grid_for(ctx, ((size_t)n_frames * n_vec + 1) / 2, 256, ctx->hsv_blocks_per_cu) / n_frames;
  if (gx < 1) gx = 1;
  launch_flat_multi(stream, variant, ptrs, n_frames, n_vec, k, fmt.first, fmt.bgr, gx, ctx->hsv_nt == 2);
  return check_hip(ctx, hipGetLastError(), "hsvfilter multi-frame kernel launch");
}

// ---------------------------------------------------------------- hsvdetector

struct HsvDetK {
  float hue_ref, hue_var, sat_ref, sat_var, val_ref, val_var;
};

// One pixel, literally: input 3 or 4 bytes/pixel at ip, output always 4 at op (hsvdetector/imp.rs:118-156).
// Arithmetic is the GENERIC conversion (IEEE ops) — the detector is a "next" row.
__device__ __forceinline__ void hsvdetect_px_literal(const uint8_t *ip, uint8_t *op, int in_bgr, int out_alpha_first, int out_bgr, const HsvDetK &k) {
  const uint32_t c0 = ip[0], c1 = ip[1], c2 = ip[2];
  const uint32_t r8 = in_bgr ? c2 : c0, g8 = c1, b8 = in_bgr ? c0 : c2;
  float h, s, v;
  hsv_from_rgb<false>((float)r8, (float)g8, (float)b8, h, s, v);
  const float ref_hue_offset = 180.0f - k.hue_ref;
  float sh = h + ref_hue_offset;
  if (sh < 0.0f) sh += 360.0f;
  sh = fmodf(sh, 360.0f);
  const bool hit = fabsf(sh - 180.0f) <= k.hue_var && fabsf(s - k.sat_ref) <= k.sat_var &&
                   fabsf(v - k.val_ref) <= k.val_var;
  const uint8_t alpha = hit ? 255 : 0;
  uint8_t *c = op + (out_alpha_first ? 1 : 0);
  if (out_bgr) { c[0] = (uint8_t)b8; c[1] = (uint8_t)g8; c[2] = (uint8_t)r8; }
  else { c[0] = (uint8_t)r8; c[1] = (uint8_t)g8; c[2] = (uint8_t)b8; }
  op[out_alpha_first ? 0 : 3] = alpha;
}

// One pixel per lane over n_frames frames of one geometry.
__global__ __launch_bounds__(256) void hsvdetect_rows_kernel(const uint8_t *__restrict__ src, size_t src_pitch,
                                                             int src_stride, int in_pixel_stride, int in_first,
                                                             int in_bgr, uint8_t *__restrict__ dst, size_t dst_pitch,
                                                             int dst_stride, int out_alpha_first, int out_bgr,
                                                             int n_frames, int width, int height, HsvDetK k) {
  const size_t per_frame = (size_t)width * (size_t)height;
  const size_t total = per_frame * (size_t)n_frames;
  const size_t gstride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gstride) {
    const size_t f = i / per_frame;
    const size_t r = i - f * per_frame;
    const size_t row = r / (size_t)width;
    const size_t col = r - row * (size_t)width;
    const uint8_t *ip = src + f * src_pitch + row * (size_t)src_stride + col * (size_t)in_pixel_stride + in_first;
    uint8_t *op = dst + f * dst_pitch + row * (size_t)dst_stride + col * 4;
    hsvdetect_px_literal(ip, op, in_bgr, out_alpha_first, out_bgr, k);
  }
}

// FAST detector kernel: 4-byte input formats on contiguous storage, 4 pixels per lane. Two classes of the offset
// off = 180 - hue_ref (hsvdetector/imp.rs:140-144: shifted = hue + off; if shifted < 0 { shifted += 360 }; shifted %= 360):
//   NEG = false, off in [0, 360] (hue_ref in [-180, 180]): shifted lies in [0, 720), the `< 0` test never fires and `% 360`
//         is one conditional exact subtraction;
//   NEG = true, off in [-360, 0) (hue_ref in (180, 540], i.e. every hue on the usual 0..360 dial): shifted lies in
//         [-360, 360); negative values get + 360 (one rounding, as in the reference) and land in [0, 360], where `% 360` only
//         turns an exact 360 into 0; non-negative values are below 360 and `% 360` keeps them.
__device__ __forceinline__ f2 hsvdetect_shifted(f2 h, float off, bool neg) {
  const f2 t = h + splat2(off);
  return sub360_if_reached2(neg ? add360_if_negative2(t) : t);
}

// Four pixel words of one lane through the FAST detector: colour channels at bytes RPOS / GPOS / BPOS of each word; out_sel
// picks the colour bytes from the input word (selector 4..7) and the alpha byte from the second operand (selector 0).
template <int RPOS, int GPOS, int BPOS>
__device__ __forceinline__ void hsvdetect_quad(const uint32_t (&in)[4], uint32_t (&out)[4], const HsvDetK &k, float off, bool neg, uint32_t out_sel,
                                               const HsvLds *lds) {
#pragma unroll
  for (int j = 0; j < 4; j += 2) {
    f2 h, s, v;
    hsv_from_rgb_pair_fast<RPOS, GPOS, BPOS, 1>(in[j], in[j + 1], h, s, v, lds);
    const f2 sh = hsvdetect_shifted(h, off, neg);
    const f2 dh = sh - splat2(180.0f), dsat = s - splat2(k.sat_ref), dv = v - splat2(k.val_ref);
    const bool hit0 = fabsf(dh.x) <= k.hue_var && fabsf(dsat.x) <= k.sat_var && fabsf(dv.x) <= k.val_var;
    const bool hit1 = fabsf(dh.y) <= k.hue_var && fabsf(dsat.y) <= k.sat_var && fabsf(dv.y) <= k.val_var;
    out[j] = __builtin_amdgcn_perm(in[j], hit0 ? 255u : 0u, out_sel);
    out[j + 1] = __builtin_amdgcn_perm(in[j + 1], hit1 ? 255u : 0u, out_sel);
  }
}

template <int IN_FIRST, bool IN_BGR, bool NEG = false>
__global__ __launch_bounds__(256) void hsvdetect_flat_kernel(const uint4 *__restrict__ src, uint4 *__restrict__ dst, size_t n_vec,
                                                             HsvDetK k, uint32_t out_sel) {
  constexpr int RPOS = IN_FIRST + (IN_BGR ? 2 : 0), GPOS = IN_FIRST + 1, BPOS = IN_FIRST + (IN_BGR ? 0 : 2);
  const float off = 180.0f - k.hue_ref;  // ref_hue_offset (hsvdetector/imp.rs:140)
  __shared__ HsvLds lds;  // value / reciprocal tables of the pair routine (the sextant entries are not used here)
  hsv_lds_fill<0, 1, 2, 3>(&lds);
  __syncthreads();
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_vec; i += stride) {
    const uint4 p = src[i];
    const uint32_t in[4] = {p.x, p.y, p.z, p.w};
    uint32_t out[4];
    hsvdetect_quad<RPOS, GPOS, BPOS>(in, out, k, off, NEG, out_sel, &lds);
    dst[i] = make_uint4(out[0], out[1], out[2], out[3]);
  }
}

// Same for the 3-byte input formats (RGB / BGR): one lane reads 12 B = 4 pixels as three dwords, splits them into four
// pixel words (byte 3 = scratch) and writes 16 B.
template <bool IN_BGR, bool NEG = false>
__global__ __launch_bounds__(256) void hsvdetect_rgb24_kernel(const Rgb24x4 *__restrict__ src, uint4 *__restrict__ dst, size_t n_grp, HsvDetK k,
                                                              uint32_t out_sel) {
  constexpr int RPOS = IN_BGR ? 2 : 0, GPOS = 1, BPOS = IN_BGR ? 0 : 2;
  const float off = 180.0f - k.hue_ref;
  __shared__ HsvLds lds;
  hsv_lds_fill<0, 1, 2, 3>(&lds);
  __syncthreads();
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_grp; i += stride) {
    const Rgb24x4 v = src[i];
    const uint32_t in[4] = {v.d0, (v.d0 >> 24) | (v.d1 << 8), (v.d1 >> 16) | (v.d2 << 16), v.d2 >> 8};
    uint32_t out[4];
    hsvdetect_quad<RPOS, GPOS, BPOS>(in, out, k, off, NEG, out_sel, &lds);
    dst[i] = make_uint4(out[0], out[1], out[2], out[3]);
  }
}

// Which kernel a batch of frames goes to: the one predicate of the lone entry (launch_hsvdetect) and of the group's launch sets
// (hsvdetect_launch_set), so that a frame is in the same class wherever it runs.
//   FLAT  : 4-byte input, packed rows on both sides (and packed frames), both pointers 16-byte aligned, pixel count % 4 == 0
//   RGB24 : 3-byte input, packed rows (and frames), source 4-byte and destination 16-byte aligned, pixel count % 4 == 0
//   both need off = 180 - hue_ref in [-360, 360] (hsvdetect_shifted) and the context's force-generic flag off
//   ROWS  : everything else, literally
enum HsvDetPath { HSVDET_FLAT, HSVDET_RGB24, HSVDET_ROWS };
static HsvDetPath hsvdetect_path(int force_generic, const uint8_t *d_src, size_t src_pitch, int src_stride, const PixFmt &sfmt, const uint8_t *d_dst,
                                 size_t dst_pitch, int dst_stride, int n_frames, int width, int height, const mi355_hsvdetect_settings &s) {
  const size_t total = (size_t)width * (size_t)height * (size_t)n_frames;
  const size_t row_bytes = (size_t)width * 4;
  const bool contiguous = sfmt.pixel_stride == 4 && (size_t)src_stride == row_bytes && (size_t)dst_stride == row_bytes &&
                          (n_frames == 1 || (src_pitch == row_bytes * (size_t)height && dst_pitch == row_bytes * (size_t)height));
  const float off = 180.0f - s.hue_ref;   // as the kernels (and the reference) compute it
  const bool fast = !force_generic && off >= -360.0f && off <= 360.0f;
  if (fast && contiguous && ((uintptr_t)d_src % 16 == 0) && ((uintptr_t)d_dst % 16 == 0) && ((total * 4) % 16 == 0)) return HSVDET_FLAT;
  const size_t row3 = (size_t)width * 3;
  const bool contiguous3 = sfmt.pixel_stride == 3 && sfmt.first == 0 && (size_t)src_stride == row3 && (size_t)dst_stride == row_bytes &&
                           (n_frames == 1 || (src_pitch == row3 * (size_t)height && dst_pitch == row_bytes * (size_t)height));
  if (fast && contiguous3 && ((uintptr_t)d_src % 4 == 0) && ((uintptr_t)d_dst % 16 == 0) && (total % 4 == 0)) return HSVDET_RGB24;
  return HSVDET_ROWS;
}

// v_perm selector of the FAST kernels' output word: colour channel c (R, G, B) sits at input byte in_pos[c]; the alpha byte
// selector stays 0 (= byte 0 of the 0/255 operand)
static uint32_t hsvdetect_out_sel(const int in_pos[3], int dst_alpha_first, int dst_bgr) {
  const int cbase = dst_alpha_first ? 1 : 0;
  uint32_t sel = 0;
  for (int c = 0; c < 3; c++) {
    const int out_byte = cbase + (dst_bgr ? 2 - c : c);
    sel |= (uint32_t)(4 + in_pos[c]) << (8 * out_byte);
  }
  return sel;
}

int launch_hsvdetect(mi355_ctx *ctx, const uint8_t *d_src, size_t src_pitch, int src_stride,
                     const PixFmt &sfmt, uint8_t *d_dst, size_t dst_pitch, int dst_stride,
                     int dst_alpha_first, int dst_bgr, int n_frames, int width, int height,
                     const mi355_hsvdetect_settings &s) {
  if (n_frames <= 0 || width <= 0 || height <= 0) return MI355_OK;
  const HsvDetK k{s.hue_ref, s.hue_var, s.saturation_ref, s.saturation_var, s.value_ref, s.value_var};
  const size_t total = (size_t)width * (size_t)height * (size_t)n_frames;
  const bool neg = 180.0f - s.hue_ref < 0.0f;
  const HsvDetPath path = hsvdetect_path(ctx->force_generic, d_src, src_pitch, src_stride, sfmt, d_dst, dst_pitch, dst_stride, n_frames, width, height, s);
  if (path == HSVDET_FLAT) {
    const int in_pos[3] = {sfmt.first + (sfmt.bgr ? 2 : 0), sfmt.first + 1, sfmt.first + (sfmt.bgr ? 0 : 2)};  // R,G,B
    const uint32_t sel = hsvdetect_out_sel(in_pos, dst_alpha_first, dst_bgr);
    const size_t n_vec = total / 4;
    const int fgrid = grid_for(ctx, (n_vec + 1) / 2, 256, 64);   // two groups per lane, as the hsvfilter kernels (one-frame launches)
    with_byte_order(sfmt.first, sfmt.bgr, [&](auto FIRST, auto BGR) { with_flag(neg, [&](auto NEG) {
      hipLaunchKernelGGL((hsvdetect_flat_kernel<FIRST, BGR, NEG>), dim3(fgrid), dim3(256), 0, ctx->stream, (const uint4 *)d_src, (uint4 *)d_dst, n_vec, k, sel);
    }); });
    return check_hip(ctx, hipGetLastError(), "hsvdetect flat kernel launch");
  }
  if (path == HSVDET_RGB24) {
    const int in_pos[3] = {sfmt.bgr ? 2 : 0, 1, sfmt.bgr ? 0 : 2};
    const uint32_t sel = hsvdetect_out_sel(in_pos, dst_alpha_first, dst_bgr);
    const size_t n_grp = total / 4;
    const int fgrid = grid_for(ctx, n_grp, 256, 64);
    with_flag(sfmt.bgr != 0, [&](auto BGR) { with_flag(neg, [&](auto NEG) {
      hipLaunchKernelGGL((hsvdetect_rgb24_kernel<BGR, NEG>), dim3(fgrid), dim3(256), 0, ctx->stream, (const Rgb24x4 *)d_src, (uint4 *)d_dst, n_grp, k, sel);
    }); });
    return check_hip(ctx, hipGetLastError(), "hsvdetect rgb24 kernel launch");
  }
  const int grid = grid_for(ctx, total, 256, 32);
  hipLaunchKernelGGL(hsvdetect_rows_kernel, dim3(grid), dim3(256), 0, ctx->stream, d_src, src_pitch, src_stride,
                     sfmt.pixel_stride, sfmt.first, sfmt.bgr, d_dst, dst_pitch, dst_stride, dst_alpha_first, dst_bgr,
                     n_frames, width, height, k);
  return check_hip(ctx, hipGetLastError(), "hsvdetect kernel launch");
}

// ---------------------------------------------------------------- hsvdetector launch sets (the video group's detector queue)
//
// Frames of independent element instances - each with its own geometry, formats and settings - in at most two launches over a
// job table. The table travels in the kernel arguments (no upload, no lifetime); a block's job index comes from blockIdx alone,
// so the search and every job field are scalar and the path choices below are the same for all waves of a block. The host side is
// hsvdetect_launch_set: it sorts the frames into the two tables of a JobSet, which plans and launches them (hsvfilter's sets too).
//   hsvdetect_jobs_kernel       the jobs the lone entry gives to hsvdetect_flat_kernel or hsvdetect_rgb24_kernel: four pixels per
//                               lane through hsvdetect_quad. One v_perm_b32 brings a job's byte order to R,G,B,0; the arithmetic
//                               reads byte values only, so it is that of the <RPOS, GPOS, BPOS> instance the lone entry picks.
//   hsvdetect_rows_jobs_kernel  every other job, through hsvdetect_px_literal, one pixel per lane. Kept apart because its IEEE
//                               division and fmodf would set the register budget of the kernel all aligned frames run.
enum : uint32_t { HD_IN3 = 1u, HD_NEG = 2u, HD_IN_BGR = 4u, HD_OUT_ALPHA_FIRST = 8u, HD_OUT_BGR = 16u, HD_IN_FIRST = 32u };
struct HdJob {
  const uint8_t *src;
  uint8_t *dst;
  uint64_t units;                        // vector launch: 16-byte output groups (4 pixels); literal launch: pixels
  int32_t width, src_stride, dst_stride; // literal launch
  uint32_t in_sel, out_sel;              // vector launch: v_perm selectors into and out of the canonical word
  HsvDetK k;
  uint32_t flags;                        // HD_*: 12- or 16-byte loads and the offset class (vector), byte positions (literal)
  uint32_t first_block, blocks;          // its blocks in the 1-D grid (hsvdetect_plan)
};
struct HdJobTable {
  HdJob job[kHdSetMax];
  int32_t n_jobs, pad;
};
static_assert(sizeof(HdJob) == 80, "HdJob has no padding holes");
static_assert(sizeof(HdJobTable) <= 4096, "the job table is passed in the kernel arguments");

__global__ __launch_bounds__(256) void hsvdetect_jobs_kernel(const HdJobTable T) {
  const int j = hsvdetect_job_of(T, blockIdx.x);
  const uint32_t rel = blockIdx.x - T.job[j].first_block;
  if (blockIdx.x < T.job[j].first_block || rel >= T.job[j].blocks) return;  // a grid larger than the plan's total: the whole block leaves, before the barrier
  __shared__ HsvLds lds;
  hsv_lds_fill<0, 1, 2, 3>(&lds);
  __syncthreads();
  const HsvDetK k = T.job[j].k;
  const float off = 180.0f - k.hue_ref;  // ref_hue_offset (hsvdetector/imp.rs:140)
  const uint32_t flags = T.job[j].flags, in_sel = T.job[j].in_sel, out_sel = T.job[j].out_sel;
  const bool neg = (flags & HD_NEG) != 0;
  const size_t n = T.job[j].units, stride = (size_t)T.job[j].blocks * 256;
  uint4 *__restrict__ dst = (uint4 *)T.job[j].dst;
  if (flags & HD_IN3) {
    const Rgb24x4 *__restrict__ src = (const Rgb24x4 *)T.job[j].src;
    for (size_t i = (size_t)rel * 256 + threadIdx.x; i < n; i += stride) {
      const Rgb24x4 v = src[i];
      const uint32_t raw[4] = {v.d0, (v.d0 >> 24) | (v.d1 << 8), (v.d1 >> 16) | (v.d2 << 16), v.d2 >> 8};
      uint32_t in[4], out[4];
#pragma unroll
      for (int q = 0; q < 4; q++) in[q] = __builtin_amdgcn_perm(raw[q], 0u, in_sel);
      hsvdetect_quad<0, 1, 2>(in, out, k, off, neg, out_sel, &lds);
      dst[i] = make_uint4(out[0], out[1], out[2], out[3]);
    }
  } else {
    const uint4 *__restrict__ src = (const uint4 *)T.job[j].src;
    for (size_t i = (size_t)rel * 256 + threadIdx.x; i < n; i += stride) {
      const uint4 p = src[i];
      const uint32_t raw[4] = {p.x, p.y, p.z, p.w};
      uint32_t in[4], out[4];
#pragma unroll
      for (int q = 0; q < 4; q++) in[q] = __builtin_amdgcn_perm(raw[q], 0u, in_sel);
      hsvdetect_quad<0, 1, 2>(in, out, k, off, neg, out_sel, &lds);
      dst[i] = make_uint4(out[0], out[1], out[2], out[3]);
    }
  }
}

__global__ __launch_bounds__(256) void hsvdetect_rows_jobs_kernel(const HdJobTable T) {
  const int j = hsvdetect_job_of(T, blockIdx.x);
  const uint32_t rel = blockIdx.x - T.job[j].first_block;
  if (blockIdx.x < T.job[j].first_block || rel >= T.job[j].blocks) return;  // a grid larger than the plan's total
  const HsvDetK k = T.job[j].k;
  const uint32_t flags = T.job[j].flags;
  const int in_bgr = (flags & HD_IN_BGR) != 0, out_alpha_first = (flags & HD_OUT_ALPHA_FIRST) != 0, out_bgr = (flags & HD_OUT_BGR) != 0;
  const size_t in_pixel_stride = (flags & HD_IN3) ? 3 : 4, in_first = (flags & HD_IN_FIRST) ? 1 : 0;
  const size_t total = T.job[j].units, width = (size_t)T.job[j].width, stride = (size_t)T.job[j].blocks * 256;
  const size_t src_stride = (size_t)T.job[j].src_stride, dst_stride = (size_t)T.job[j].dst_stride;
  const uint8_t *__restrict__ src = T.job[j].src;
  uint8_t *__restrict__ dst = T.job[j].dst;
  for (size_t i = (size_t)rel * 256 + threadIdx.x; i < total; i += stride) {
    const size_t row = i / width;
    const size_t col = i - row * width;
    hsvdetect_px_literal(src + row * src_stride + col * in_pixel_stride + in_first, dst + row * dst_stride + col * 4, in_bgr, out_alpha_first, out_bgr, k);
  }
}

// The blocks of one launch of a set (mi355_selftest_hsvdetect_plan). Job j wants ceil(units / units_per_block) blocks; if the
// wants fit the budget of n_cu * blocks_per_cu every job gets its want - the grid the lone launch would give it. Otherwise every job
// with units gets one block and the rest of the budget is shared in proportion to what the jobs still want, rounded down: a big
// frame among small ones takes what they leave, equal frames get equal shares, and the total stays within max(budget, jobs).
int hsvdetect_plan(int n_cu, int blocks_per_cu, unsigned units_per_block, int n_jobs, const uint64_t *units, uint32_t *first_block, uint32_t *blocks,
                   uint32_t *total_blocks) {
  if (n_cu < 1 || blocks_per_cu < 1 || units_per_block == 0 || n_jobs < 0 || n_jobs > kHdSetMax || !total_blocks ||
      (n_jobs && (!units || !first_block || !blocks)))
    return MI355_ERR_INVALID_ARG;
  uint64_t budget = (uint64_t)n_cu * (uint64_t)blocks_per_cu;
  if (budget > 0x7fffffffull) budget = 0x7fffffffull;  // (a grid's x dimension)
  uint64_t want[kHdSetMax];
  unsigned __int128 all = 0, still = 0;
  uint64_t with_units = 0;
  for (int j = 0; j < n_jobs; j++) {
    want[j] = units[j] / units_per_block + (units[j] % units_per_block != 0);
    all += want[j];
    if (want[j]) { with_units++; still += want[j] - 1; }
  }
  const bool fits = all <= budget;
  const uint64_t spare = budget > with_units ? budget - with_units : 0;   // (!fits: spare < still)
  uint32_t next = 0;
  for (int j = 0; j < n_jobs; j++) {
    uint64_t b = want[j];
    if (!fits && b) b = 1 + (uint64_t)((unsigned __int128)(want[j] - 1) * spare / (still ? still : 1));
    first_block[j] = next;
    blocks[j] = (uint32_t)b;
    next += (uint32_t)b;
  }
  *total_blocks = next;
  return MI355_OK;
}

// A launch set is a JobSet (job_set.hpp) over HdJobTable or HfJobTable: hsvdetect_launch_set and hsvfilter_set_build classify frames
// into its two tables and fill them; it plans and launches them, for both elements, on the grid of kHsvJobGrid.
int hsvdetect_launch_set(hipStream_t stream, int n_cu, const HdFrame *frames, int n, int *kernel_launches, std::string *err) {
  *kernel_launches = 0;
  if (!frames || n < 1 || n > kHdSetMax) { *err = "hsvdetector: bad launch set"; return MI355_ERR_INVALID_ARG; }
  JobSet<HdJobTable> S{};
  for (int i = 0; i < n; i++) {
    const HdFrame &f = frames[i];
    if (f.width <= 0 || f.height <= 0) continue;  // no pixel: no job
    const size_t total = (size_t)f.width * (size_t)f.height;
    const HsvDetPath path = hsvdetect_path(f.force_generic, f.src, 0, f.src_stride, f.sfmt, f.dst, 0, f.dst_stride, 1, f.width, f.height, f.s);
    HdJobTable &T = S.table[path == HSVDET_ROWS ? kLit : kVec];
    HdJob &J = T.job[T.n_jobs++];
    J.src = f.src;
    J.dst = f.dst;
    J.width = f.width;
    J.src_stride = f.src_stride;
    J.dst_stride = f.dst_stride;
    J.k = HsvDetK{f.s.hue_ref, f.s.hue_var, f.s.saturation_ref, f.s.saturation_var, f.s.value_ref, f.s.value_var};
    J.flags = (f.sfmt.pixel_stride == 3 ? HD_IN3 : 0u) | (180.0f - f.s.hue_ref < 0.0f ? HD_NEG : 0u) | (f.sfmt.bgr ? HD_IN_BGR : 0u) |
              (f.dst_alpha_first ? HD_OUT_ALPHA_FIRST : 0u) | (f.dst_bgr ? HD_OUT_BGR : 0u) | (f.sfmt.first ? HD_IN_FIRST : 0u);
    if (path == HSVDET_ROWS) {
      J.units = total;
    } else {
      // canonical word: R, G, B at bytes 0, 1, 2 and a zero (selector 0x0c) - the lone kernels' selector with in_pos = {0, 1, 2}
      const int rpos = f.sfmt.first + (f.sfmt.bgr ? 2 : 0), gpos = f.sfmt.first + 1, bpos = f.sfmt.first + (f.sfmt.bgr ? 0 : 2);
      const int canon[3] = {0, 1, 2};
      J.in_sel = (uint32_t)(4 + rpos) | ((uint32_t)(4 + gpos) << 8) | ((uint32_t)(4 + bpos) << 16) | (0x0cu << 24);
      J.out_sel = hsvdetect_out_sel(canon, f.dst_alpha_first, f.dst_bgr);
      J.units = total / 4;
    }
  }
  if (const int rc = S.plan(n_cu)) { *err = "hsvdetector: bad launch set"; return rc; }
  return S.launch(stream, {hsvdetect_jobs_kernel, hsvdetect_rows_jobs_kernel}, {"hsvdetect jobs kernel launch: ", "hsvdetect rows jobs kernel launch: "}, kernel_launches, err);
}

// ---------------------------------------------------------------- hsvfilter launch sets (the video group's filter queue)
//
// The same form for hsvfilter: frames of independent element instances - own size, stride, format (the ten 8-bit ones) and five
// settings, which the reference lets change while playing (hsvfilter/imp.rs:127-156, snapshot per buffer :85) - filtered IN PLACE
// in at most two launches over a job table in the kernel arguments.
//   hsvfilter_jobs_kernel       the vector launch, four pixels per lane through hsvfilter_quad in its canonical instance <0, 1, 2, 3>:
//                               one v_perm_b32 (in_sel) brings R, G, B to bytes 0-2 and the x / alpha byte to byte 3 (a 3-byte
//                               format's byte 3 is the neighbour's byte: carried along, dropped by the re-pack), a second one
//                               (out_sel) restores the order; the arithmetic reads byte values only, so it is that of the
//                               <RPOS, GPOS, BPOS, NPOS> instance the lone entry picks. It carries every frame with a pixel whose
//                               settings give a FAST variant (hsv_variant_for(s, force_generic, true) >= 0, wide shifts included) and
//                               whose geometry is the lone entry's flat or rgb24 class: packed rows and, 4-byte formats, a 16-byte
//                               aligned base and a byte count % 16 == 0, or, 3-byte formats, a 4-byte aligned base and a byte count
//                               % 12 == 0. 4-byte frames with padded rows whose base and stride are multiples of 16 (the lone
//                               rowpad class) are here too, addressed as (row, group) with the 1-3 pixel group at a row's end read
//                               and written dword by dword: by the compiler's resource report that branch costs the kernel no
//                               vector register and no scratch (49 VGPRs with and without it). The variant is a per-job
//                               value: a block-uniform switch over the ten FAST instantiations (same report: no scratch, 8 waves
//                               per SIMD as the lone flat kernel).
//   hsvfilter_rows_jobs_kernel  the literal launch, one pixel per lane through hsvfilter_px<FAST / generic> with byte accesses, as
//                               hsvfilter_rows_kernel: GENERIC settings, FORCE_GENERIC, unaligned bases, padded rows off the 16-byte
//                               multiples (and all padded rows of 3-byte formats), pixel counts that do not fill whole groups. Kept
//                               apart because IEEE division and fmodf would set the register budget of the kernel all aligned
//                               frames run.
// In place means order matters: two jobs of one launch never touch the same bytes. hsvfilter_set_build closes a set in front of a
// frame whose byte range [data, data + (height - 1) stride + width pixel_stride) meets that of a frame already in it (ranges only:
// conservative), and sets run one after the other on the queue's stream - overlapping frames come out as if filtered in order.
// The host side is that builder and the detector's JobSet: hsvfilter_launch_set builds, then launches each set.
enum : uint32_t { HF_PX3 = 1u, HF_BGR = 2u, HF_FIRST = 4u, HF_ROWPAD = 8u };
struct HfJob {
  uint8_t *data;
  uint64_t units;                // vector launch: groups of four pixels (16 or 12 bytes); literal launch: pixels
  HsvK k;
  uint32_t in_sel, out_sel;      // vector launch: v_perm selectors into and out of the canonical word
  int32_t width, stride;         // literal launch
  int32_t variant;               // vector launch: the FAST variant (hsv_shift_of / hsv_sv_ident_of); literal launch: >= 0 FAST, -1 generic
  uint32_t flags;                // HF_*: 12- or 16-byte groups (vector), pixel stride and byte positions (literal)
  uint32_t first_block, blocks;  // its blocks in the 1-D grid (hsvdetect_plan)
  uint32_t through;              // vector launch, flat 4-byte frames: the member's MI355_FLAG_HSV_NT was 2 at submit (hsv_store_through)
};
struct HfJobTable {
  HfJob job[kHfSetMax];
  int32_t n_jobs, pad;
};
static_assert(sizeof(HfJob) == 72, "HfJob has no padding holes");
static_assert(sizeof(HfJobTable) == kHfSetMax * 72 + 8 && sizeof(HfJobTable) <= 4096, "the job table is passed in the kernel arguments");

// the groups of one job's share through the FAST variant VARIANT
template <int VARIANT>
__device__ __forceinline__ void hsvfilter_job_groups(const HfJob &J, uint32_t rel, const HsvLds *lds) {
  const HsvK k = J.k;
  const uint32_t in_sel = J.in_sel, out_sel = J.out_sel;
  const size_t n = J.units, stride = (size_t)J.blocks * 256;
  if (J.flags & HF_PX3) {
    Rgb24x4 *__restrict__ data = (Rgb24x4 *)J.data;
    for (size_t i = (size_t)rel * 256 + threadIdx.x; i < n; i += stride) {
      const Rgb24x4 v = data[i];
      uint32_t p0 = __builtin_amdgcn_perm(v.d0, 0u, in_sel), p1 = __builtin_amdgcn_perm((v.d0 >> 24) | (v.d1 << 8), 0u, in_sel);
      uint32_t p2 = __builtin_amdgcn_perm((v.d1 >> 16) | (v.d2 << 16), 0u, in_sel), p3 = __builtin_amdgcn_perm(v.d2 >> 8, 0u, in_sel);
      hsvfilter_quad<VARIANT, 0, 1, 2, 3>(p0, p1, p2, p3, k, lds);
      p0 = __builtin_amdgcn_perm(p0, 0u, out_sel); p1 = __builtin_amdgcn_perm(p1, 0u, out_sel);
      p2 = __builtin_amdgcn_perm(p2, 0u, out_sel); p3 = __builtin_amdgcn_perm(p3, 0u, out_sel);
      Rgb24x4 o;
      o.d0 = (p0 & 0x00ffffffu) | (p1 << 24);
      o.d1 = ((p1 >> 8) & 0x0000ffffu) | (p2 << 16);
      o.d2 = ((p2 >> 16) & 0x000000ffu) | (p3 << 8);
      data[i] = o;
    }
  } else if (J.flags & HF_ROWPAD) {
    // padded rows, base and stride on 16-byte multiples: (row, group of four pixels); the last group of a row may hold 1-3 pixels
    // and only those are read and written (hsvfilter_rowpad_kernel)
    const uint32_t groups = ((uint32_t)J.width + 3u) >> 2;
    for (size_t i = (size_t)rel * 256 + threadIdx.x; i < n; i += stride) {
      const size_t row = i / groups;
      const uint32_t g = (uint32_t)(i - row * groups);
      uint8_t *at = J.data + row * (size_t)J.stride + (size_t)g * 16;
      const int left = J.width - (int)(g * 4);
      uint32_t px[4] = {0, 0, 0, 0};
      if (left >= 4) {
        const uint4 p = *(const uint4 *)at;
        px[0] = p.x; px[1] = p.y; px[2] = p.z; px[3] = p.w;
      } else {
        for (int q = 0; q < left; q++) px[q] = ((const uint32_t *)at)[q];
      }
#pragma unroll
      for (int q = 0; q < 4; q++) px[q] = __builtin_amdgcn_perm(px[q], 0u, in_sel);
      hsvfilter_quad<VARIANT, 0, 1, 2, 3>(px[0], px[1], px[2], px[3], k, lds);
#pragma unroll
      for (int q = 0; q < 4; q++) px[q] = __builtin_amdgcn_perm(px[q], 0u, out_sel);
      if (left >= 4) *(uint4 *)at = make_uint4(px[0], px[1], px[2], px[3]);
      else
        for (int q = 0; q < left; q++) ((uint32_t *)at)[q] = px[q];
    }
  } else {
    uint4 *__restrict__ data = (uint4 *)J.data;
    const uint32_t through = J.through;
    for (size_t i = (size_t)rel * 256 + threadIdx.x; i < n; i += stride) {
      uint4 p = data[i];
      p.x = __builtin_amdgcn_perm(p.x, 0u, in_sel); p.y = __builtin_amdgcn_perm(p.y, 0u, in_sel);
      p.z = __builtin_amdgcn_perm(p.z, 0u, in_sel); p.w = __builtin_amdgcn_perm(p.w, 0u, in_sel);
      hsvfilter_quad<VARIANT, 0, 1, 2, 3>(p.x, p.y, p.z, p.w, k, lds);
      p.x = __builtin_amdgcn_perm(p.x, 0u, out_sel); p.y = __builtin_amdgcn_perm(p.y, 0u, out_sel);
      p.z = __builtin_amdgcn_perm(p.z, 0u, out_sel); p.w = __builtin_amdgcn_perm(p.w, 0u, out_sel);
      if (through) hsv_store_through(data + i, p);  // (the job's, so the block's)
      else data[i] = p;
    }
  }
}

__global__ __launch_bounds__(256) void hsvfilter_jobs_kernel(const HfJobTable T) {
  const int j = hsvdetect_job_of(T, blockIdx.x);
  const uint32_t rel = blockIdx.x - T.job[j].first_block;
  if (blockIdx.x < T.job[j].first_block || rel >= T.job[j].blocks) return;  // a grid larger than the plan's total: the whole block leaves, before the barrier
  __shared__ HsvLds lds;
  hsv_lds_fill<0, 1, 2, 3>(&lds);
  __syncthreads();
  // the job, and with it the variant, is the block's: every wave takes the same case
  switch (T.job[j].variant) {
    case 0: hsvfilter_job_groups<0>(T.job[j], rel, &lds); break;
    case 1: hsvfilter_job_groups<1>(T.job[j], rel, &lds); break;
    case 2: hsvfilter_job_groups<2>(T.job[j], rel, &lds); break;
    case 4: hsvfilter_job_groups<4>(T.job[j], rel, &lds); break;
    case 5: hsvfilter_job_groups<5>(T.job[j], rel, &lds); break;
    case 6: hsvfilter_job_groups<6>(T.job[j], rel, &lds); break;
    case 8: hsvfilter_job_groups<8>(T.job[j], rel, &lds); break;
    case 9: hsvfilter_job_groups<9>(T.job[j], rel, &lds); break;
    case 12: hsvfilter_job_groups<12>(T.job[j], rel, &lds); break;
    case 13: hsvfilter_job_groups<13>(T.job[j], rel, &lds); break;
    default: break;  // (no other variant is ever put into a vector table)
  }
}

template <bool FAST>
__device__ __forceinline__ void hsvfilter_job_pixels(const HfJob &J, uint32_t rel, const uint32_t *sel_tab) {
  const HsvK k = J.k;
  const bool bgr = (J.flags & HF_BGR) != 0;
  const size_t pixel_stride = (J.flags & HF_PX3) ? 3 : 4, first = (J.flags & HF_FIRST) ? 1 : 0;
  const size_t total = J.units, width = (size_t)J.width, row_stride = (size_t)J.stride, stride = (size_t)J.blocks * 256;
  uint8_t *__restrict__ data = J.data;
  for (size_t i = (size_t)rel * 256 + threadIdx.x; i < total; i += stride) {
    const size_t row = i / width;
    const size_t col = i - row * width;
    uint8_t *px = data + row * row_stride + col * pixel_stride + first;
    const uint32_t c0 = px[0], c1 = px[1], c2 = px[2];
    const uint32_t p = bgr ? (c2 | (c1 << 8) | (c0 << 16)) : (c0 | (c1 << 8) | (c2 << 16));
    const uint32_t o = hsvfilter_px<FAST, 0, 1, 2, 3>(p, k, sel_tab);
    const uint8_t orr = (uint8_t)(o & 0xff), og = (uint8_t)((o >> 8) & 0xff), ob = (uint8_t)((o >> 16) & 0xff);
    px[0] = bgr ? ob : orr;
    px[1] = og;
    px[2] = bgr ? orr : ob;
  }
}

__global__ __launch_bounds__(256) void hsvfilter_rows_jobs_kernel(const HfJobTable T) {
  const int j = hsvdetect_job_of(T, blockIdx.x);
  const uint32_t rel = blockIdx.x - T.job[j].first_block;
  if (blockIdx.x < T.job[j].first_block || rel >= T.job[j].blocks) return;  // a grid larger than the plan's total
  __shared__ uint32_t sel_tab[8];
  if (threadIdx.x < 7) sel_tab[threadIdx.x] = hsv_sel_entry(threadIdx.x, 0, 1, 2, 3);
  __syncthreads();
  if (T.job[j].variant >= 0) hsvfilter_job_pixels<true>(T.job[j], rel, sel_tab);
  else hsvfilter_job_pixels<false>(T.job[j], rel, sel_tab);
}

bool hsvfilter_frames_overlap(const HfFrame &a, const HfFrame &b) {
  if (a.width <= 0 || a.height <= 0 || b.width <= 0 || b.height <= 0) return false;  // no pixel, no byte
  const uintptr_t a0 = (uintptr_t)a.data, b0 = (uintptr_t)b.data;
  const uintptr_t a1 = a0 + (size_t)(a.height - 1) * (size_t)a.stride + (size_t)a.width * (size_t)a.fmt.pixel_stride;
  const uintptr_t b1 = b0 + (size_t)(b.height - 1) * (size_t)b.stride + (size_t)b.width * (size_t)b.fmt.pixel_stride;
  return a0 < b1 && b0 < a1;
}

// The ONE builder of launch sets, for hsvfilter_launch_set and mi355_selftest_hsvfilter_set_plan alike: closes a set at kHfSetMax
// frames and in front of a frame that overlaps one already in it, classifies each set's frames into its two tables with their
// variants and selectors, and has JobSet plan the blocks. The frames' addresses are numbers here: nothing is dereferenced. `out` (per
// frame) may be null.
typedef JobSet<HfJobTable> HfSet;
static int hsvfilter_set_build(int n_cu, const HfFrame *frames, int n, std::vector<HfSet> *sets, mi355_hsvfilter_plan_out *out) {
  sets->clear();
  if (n_cu < 1 || n < 0 || (n && !frames)) return MI355_ERR_INVALID_ARG;
  for (int begin = 0; begin < n;) {
    int end = begin;
    for (; end < n && end - begin < kHfSetMax; end++) {
      bool meets = false;
      for (int e = begin; e < end && !meets; e++) meets = hsvfilter_frames_overlap(frames[e], frames[end]);
      if (meets) break;
    }
    sets->emplace_back();
    HfSet &S = sets->back();
    std::memset(&S, 0, sizeof(S));
    for (int i = begin; i < end; i++) {
      const HfFrame &f = frames[i];
      if (out) out[i] = mi355_hsvfilter_plan_out{(int32_t)sets->size() - 1, 0, -1, 0, 0, 0, 0};
      if (f.width <= 0 || f.height <= 0) continue;  // no pixel: no job
      const size_t row_bytes = (size_t)f.width * (size_t)f.fmt.pixel_stride, total_bytes = row_bytes * (size_t)f.height;
      const bool packed = (size_t)f.stride == row_bytes;
      const uintptr_t at = (uintptr_t)f.data;
      const int wide_variant = hsv_variant_for(f.s, f.force_generic != 0, true);
      const bool flat = f.fmt.pixel_stride == 4 ? packed && at % 16 == 0 && total_bytes % 16 == 0
                                                : f.fmt.first == 0 && packed && at % 4 == 0 && total_bytes % 12 == 0;
      const bool rowpad = !flat && f.fmt.pixel_stride == 4 && at % 16 == 0 && f.stride % 16 == 0;
      const bool vector = wide_variant >= 0 && (flat || rowpad);
      HfJobTable &T = S.table[vector ? kVec : kLit];
      HfJob &J = T.job[T.n_jobs++];
      J.data = f.data;
      J.k = HsvK{f.s.hue_shift, f.s.saturation_mul, f.s.saturation_off, f.s.value_mul, f.s.value_off};
      J.width = f.width;
      J.stride = f.stride;
      J.flags = (f.fmt.pixel_stride == 3 ? HF_PX3 : 0u) | (f.fmt.bgr ? HF_BGR : 0u) | (f.fmt.first ? HF_FIRST : 0u);
      if (vector) {
        // canonical word: R, G, B at bytes 0, 1, 2, the x / alpha byte (3-byte formats: the word's spare byte) at byte 3. Selector
        // bytes 4..7 pick from the first operand of v_perm_b32
        const uint32_t rpos = (uint32_t)(f.fmt.first + (f.fmt.bgr ? 2 : 0)), gpos = (uint32_t)f.fmt.first + 1, bpos = (uint32_t)(f.fmt.first + (f.fmt.bgr ? 0 : 2));
        const uint32_t npos = f.fmt.pixel_stride == 4 && f.fmt.first ? 0 : 3;
        J.in_sel = (4 + rpos) | ((4 + gpos) << 8) | ((4 + bpos) << 16) | ((4 + npos) << 24);
        J.out_sel = (4u << (8 * rpos)) | (5u << (8 * gpos)) | (6u << (8 * bpos)) | (7u << (8 * npos));
        J.variant = wide_variant;
        J.through = f.hsv_nt == 2;
        if (rowpad) J.flags |= HF_ROWPAD;
        J.units = rowpad ? (uint64_t)(((uint32_t)f.width + 3u) / 4u) * (uint64_t)f.height : total_bytes / (f.fmt.pixel_stride == 4 ? 16 : 12);
      } else {
        // one pixel per lane: the single-pixel FAST routine knows the narrow shift classes only (as the lone rows kernel's choice)
        J.variant = hsv_variant_for(f.s, f.force_generic != 0, false);
        J.units = (uint64_t)f.width * (uint64_t)f.height;
      }
      if (out) { out[i].launch = 1 + (vector ? kVec : kLit); out[i].variant = J.variant; out[i].units = J.units; }
    }
    if (const int rc = S.plan(n_cu)) return rc;
    int next[2] = {0, 0};   // a table's jobs are in the order of their frames
    for (int i = begin; out && i < end; i++) {
      if (!out[i].launch) continue;
      const HfJob &J = S.table[out[i].launch - 1].job[next[out[i].launch - 1]++];
      out[i].first_block = J.first_block;
      out[i].blocks = J.blocks;
    }
    begin = end;
  }
  return MI355_OK;
}

int hsvfilter_set_plan(int n_cu, const HfFrame *frames, int n, mi355_hsvfilter_plan_out *out, int *n_sets) {
  std::vector<HfSet> sets;
  const int rc = hsvfilter_set_build(n_cu, frames, n, &sets, out);
  if (!rc) *n_sets = (int)sets.size();
  return rc;
}

int hsvfilter_launch_set(hipStream_t stream, int n_cu, const HfFrame *frames, int n, int *kernel_launches, std::string *err) {
  *kernel_launches = 0;
  if (!frames || n < 1 || n > kHfSetMax) { *err = "hsvfilter: bad launch set"; return MI355_ERR_INVALID_ARG; }
  std::vector<HfSet> sets;
  if (const int rc = hsvfilter_set_build(n_cu, frames, n, &sets, nullptr)) { *err = "hsvfilter: bad launch set"; return rc; }
  // (one set, unless the caller handed over frames that overlap: then their sets, in order on the one stream)
  for (const HfSet &S : sets)
    if (const int rc = S.launch(stream, {hsvfilter_jobs_kernel, hsvfilter_rows_jobs_kernel}, {"hsvfilter jobs kernel launch: ", "hsvfilter rows jobs kernel launch: "}, kernel_launches, err)) return rc;
  return MI355_OK;
}

}  // namespace mi355
