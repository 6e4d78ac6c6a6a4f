// colorlut_device.hpp — the colorlut element's arithmetic as the reference writes it (video/colorlut/src/colorlut/imp.rs:471-543,
// parser.rs:43-53), operation by operation: shared by colorlut_kernels.hip (colorlut_rows_kernel, the route every other kernel is
// held to) and colorlut_group.hip (the video group's colorlut queue). Compile without contraction.
#pragma once
#include "internal.hpp"
#include "exact_math.hpp"

namespace mi355 {

struct LutK {
  float scale[3];
  float offset[3];
  int size;
};

// ---------------------------------------------------------------- generic arithmetic

// `x.floor() as usize` then `.min(max_idx)` (imp.rs:485,496-498)
__device__ __forceinline__ uint32_t floor_idx(float x, uint32_t max_idx) {
  const float f = floorf(x);
  // as usize: NaN -> 0, negative -> 0, huge -> saturate (then min)
  uint32_t i = (f > 0.0f) ? ((f >= 4294967040.0f) ? 0xffffffffu : (uint32_t)f) : 0u;
  return i < max_idx ? i : max_idx;
}

__device__ __forceinline__ float float_to_u8f(float v) { return roundf(rs_clamp(v, 0.0f, 1.0f) * 255.0f); }
__device__ __forceinline__ float float_to_u16f(float v) { return roundf(rs_clamp(v, 0.0f, 1.0f) * 65535.0f); }

template <bool BITS16>
__device__ __forceinline__ float norm_comp_generic(const LutK &k, int c, float value) {
  const float v = BITS16 ? value / 65535.0f : value / 255.0f;
  return rs_clamp(v * k.scale[c] + k.offset[c], 0.0f, 1.0f);
}

// a 1D LUT between x0 = floor_idx(x, len - 1) and its clamped neighbour, t = x - x0 (imp.rs:482-493)
__device__ __forceinline__ float sample_1d_at(const float *__restrict__ lut, uint32_t len, uint32_t x0, float t) {
  const uint32_t max_idx = len - 1;
  const uint32_t x1 = (x0 + 1 < max_idx) ? x0 + 1 : max_idx;
  const float a = lut[x0], b = lut[x1];
  return a + (b - a) * t;
}

__device__ __forceinline__ float sample_1d_generic(const float *__restrict__ lut, uint32_t len, float x) {
  const uint32_t x0 = floor_idx(x, len - 1);
  return sample_1d_at(lut, len, x0, x - (float)x0);
}

__device__ __forceinline__ float lerp1(float a, float b, float t) { return a + (b - a) * t; }

// trilinear on the [r,g,b,1] cells from the cell (x0, y0, z0) = floor_idx of the coordinates and the weights t = coordinate - floor;
// alpha lane is never consumed by the reference callers. No corner lies past the table: every index is at most size - 1.
__device__ __forceinline__ void sample_3d_at(const float4 *__restrict__ cells, uint32_t size, uint32_t x0, uint32_t y0, uint32_t z0,
                                             float tx, float ty, float tz, float out[3]) {
  const uint32_t max_idx = size - 1;
  const uint32_t x1 = (x0 + 1 < max_idx) ? x0 + 1 : max_idx;
  const uint32_t y1 = (y0 + 1 < max_idx) ? y0 + 1 : max_idx;
  const uint32_t z1 = (z0 + 1 < max_idx) ? z0 + 1 : max_idx;
  const uint32_t s2 = size * size;
  const float4 c000 = cells[x0 + y0 * size + z0 * s2], c100 = cells[x1 + y0 * size + z0 * s2];
  const float4 c010 = cells[x0 + y1 * size + z0 * s2], c110 = cells[x1 + y1 * size + z0 * s2];
  const float4 c001 = cells[x0 + y0 * size + z1 * s2], c101 = cells[x1 + y0 * size + z1 * s2];
  const float4 c011 = cells[x0 + y1 * size + z1 * s2], c111 = cells[x1 + y1 * size + z1 * s2];
#define MI355_TRI(ch)                                                              \
  lerp1(lerp1(lerp1(c000.ch, c100.ch, tx), lerp1(c010.ch, c110.ch, tx), ty),       \
        lerp1(lerp1(c001.ch, c101.ch, tx), lerp1(c011.ch, c111.ch, tx), ty), tz)
  out[0] = MI355_TRI(x);
  out[1] = MI355_TRI(y);
  out[2] = MI355_TRI(z);
#undef MI355_TRI
}

__device__ __forceinline__ void sample_3d_generic(const float4 *__restrict__ cells, uint32_t size, float x,
                                                  float y, float z, float out[3]) {
  const uint32_t max_idx = size - 1;
  const uint32_t x0 = floor_idx(x, max_idx), y0 = floor_idx(y, max_idx), z0 = floor_idx(z, max_idx);
  sample_3d_at(cells, size, x0, y0, z0, x - (float)x0, y - (float)y0, z - (float)z0, out);
}

__device__ __forceinline__ uint16_t bswap16(uint16_t v) { return (uint16_t)((v >> 8) | (v << 8)); }

// The pixel at (row, col) of one frame, literally: what one lane of colorlut_rows_kernel does, and one lane of the group's
// colorlut_rows_jobs_kernel. BITS16: RGBA64 (u16 samples, LE selects byte order); else RGBA8. `table`: the cells as the reference
// stores them (3D: [size^3][4]; 1D: r|g|b planes); sm1 = (float)k.size - 1.
template <bool IS3D, bool BITS16, bool LE>
__device__ __forceinline__ void colorlut_px_literal(const uint8_t *__restrict__ src, int src_stride, uint8_t *__restrict__ dst, int dst_stride,
                                                    size_t row, size_t col, const float *__restrict__ table, const LutK &k, float sm1) {
  float in[3];
  if constexpr (BITS16) {
    // stride is taken in u16 units: plane_stride / 2 (imp.rs:358-359)
    const uint16_t *s = (const uint16_t *)src + row * (size_t)(src_stride / 2) + col * 4;
    uint16_t *d = (uint16_t *)dst + row * (size_t)(dst_stride / 2) + col * 4;
    uint16_t raw[4] = {s[0], s[1], s[2], s[3]};
    for (int c = 0; c < 3; c++) in[c] = (float)(LE ? raw[c] : bswap16(raw[c]));
    float o[3];
    if constexpr (IS3D) {
      sample_3d_generic((const float4 *)table, (uint32_t)k.size, norm_comp_generic<true>(k, 0, in[0]) * sm1,
                        norm_comp_generic<true>(k, 1, in[1]) * sm1, norm_comp_generic<true>(k, 2, in[2]) * sm1, o);
    } else {
      for (int c = 0; c < 3; c++)
        o[c] = sample_1d_generic(table + (size_t)c * k.size, (uint32_t)k.size, norm_comp_generic<true>(k, c, in[c]) * sm1);
    }
    for (int c = 0; c < 3; c++) {
      const uint16_t v = (uint16_t)rs_as_u16(float_to_u16f(o[c]));
      d[c] = LE ? v : bswap16(v);
    }
    d[3] = raw[3];  // alpha word copied raw (imp.rs:344,394)
  } else {
    const uint8_t *s = src + row * (size_t)src_stride + col * 4;
    uint8_t *d = dst + row * (size_t)dst_stride + col * 4;
    const uint8_t raw[4] = {s[0], s[1], s[2], s[3]};
    for (int c = 0; c < 3; c++) in[c] = (float)raw[c];
    float o[3];
    if constexpr (IS3D) {
      sample_3d_generic((const float4 *)table, (uint32_t)k.size, norm_comp_generic<false>(k, 0, in[0]) * sm1,
                        norm_comp_generic<false>(k, 1, in[1]) * sm1, norm_comp_generic<false>(k, 2, in[2]) * sm1, o);
    } else {
      for (int c = 0; c < 3; c++)
        o[c] = sample_1d_generic(table + (size_t)c * k.size, (uint32_t)k.size, norm_comp_generic<false>(k, c, in[c]) * sm1);
    }
    d[0] = (uint8_t)rs_as_u8(float_to_u8f(o[0]));
    d[1] = (uint8_t)rs_as_u8(float_to_u8f(o[1]));
    d[2] = (uint8_t)rs_as_u8(float_to_u8f(o[2]));
    d[3] = raw[3];
  }
}

}  // namespace mi355
