// decode_device.hpp - the bit-exactness primitives every tensor decoder shares (yolodec_device.hpp for yolodec.hip and yolox_head.hip,
// handdec.hip): Rust's f32::total_cmp as an integer key and its inverse, Rust's `as i32`, the corner box, the pad key of the sorts,
// the power of two a key list is padded to, and the wave-aggregated append to a key list. One copy: a correction to one of them is
// a correction to every decoder. What differs between the decoders stays with them: the key layouts, the IoU formulas, the sorts.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstddef>
#include <cstdint>

namespace mi355 {

namespace {

constexpr unsigned long long kPadKey = ~0ull;   // above every real key of either layout

// f32::total_cmp's key: the order of the result as i32 is the total order
__device__ __forceinline__ int32_t total_key(uint32_t bits) {
  const int32_t s = (int32_t)bits;
  return s ^ (int32_t)((uint32_t)(s >> 31) >> 1);
}

// the f32 bits a total_key (as u32) came from: the key map is its own inverse
__device__ __forceinline__ uint32_t total_key_bits(uint32_t key) {
  const int32_t s = (int32_t)key;
  return (uint32_t)(s ^ (int32_t)((uint32_t)(s >> 31) >> 1));
}

// Rust's `as i32`: toward zero, saturating, NaN -> 0
__device__ __forceinline__ int32_t cast_i32(float f) {
  if (f != f) return 0;
  if (f >= 2147483648.0f) return INT_MAX;
  if (f <= -2147483648.0f) return INT_MIN;
  return (int32_t)f;
}

struct Box { float xmin, ymin, xmax, ymax; };

// called by every lane of the wave: the survivors' keys go to keys[old count ...), one atomic for the wave (on a global or an LDS
// counter). Cap is the integer type the caller holds the list's capacity in: the position is computed in it.
template <typename Key, typename Cap>
__device__ __forceinline__ void append_keys(bool keep, Key key, uint32_t *count, Key *keys, Cap cap) {
  const unsigned long long m = __ballot(keep);
  if (m == 0) return;   // wave-uniform
  const int lane = (int)__lane_id();
  const int leader = __ffsll((long long)m) - 1;
  uint32_t base = 0;
  if (lane == leader) base = atomicAdd(count, (uint32_t)__popcll(m));
  base = (uint32_t)__shfl((int)base, leader);
  const Cap at = (Cap)base + (Cap)__popcll(m & ((1ull << lane) - 1ull));
  if (keep && at < cap) keys[at] = key;   // always inside: the counter starts at zero and a candidate is appended once
}

inline uint32_t pow2_at_least(uint32_t n) {
  uint32_t p = 1;
  while (p < n) p <<= 1;
  return p;
}

}  // namespace

}  // namespace mi355
