// The attention-dropout mask of the self-attention training kernels (csrc/mha.hip): stateless and counter-based, a function of
// (seed, batch element, head, query index, key index) and of nothing else -- not of the tiling, the launch geometry, the batch
// size or the kernel that asks.  Every kernel that needs a decision calls drop_keep or composes the same three steps.
//
// 8 bits per decision: p is quantised to threshold / 256 (drop_threshold), an element is kept iff its byte >= threshold, and
// the kept elements are scaled by 256 / (256 - threshold) = 1 / (1 - p_q): the expectation is exact for the quantised p_q.
// One 32-bit word serves the four keys 4 c .. 4 c + 3 of one query: byte j & 3 of drop_word(row key of the query, j >> 2).
#pragma once
#include <stdint.h>

namespace mha {

constexpr uint32_t DROP_GOLD = 0x9E3779B9u;

static inline int drop_threshold(float p) {
  const int t = (int)(p * 256.f + 0.5f);
  return t > 255 ? 255 : t;
}

// 32-bit finaliser (two multiplies, three xor-shifts): a bijection with full avalanche
__device__ __forceinline__ uint32_t drop_mix(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

// wave-uniform: once per workgroup
__device__ __forceinline__ uint32_t drop_head_key(uint64_t seed, int b, int head) {
  const uint32_t s = drop_mix((uint32_t)seed) ^ drop_mix((uint32_t)(seed >> 32) + DROP_GOLD);
  return drop_mix(s + (uint32_t)(b * 8 + head) * 0x85ebca6bu);
}

// once per query row
__device__ __forceinline__ uint32_t drop_row_key(uint32_t head_key, int query) { return drop_mix(head_key ^ (uint32_t)query); }

// the four decisions of keys 4 chunk .. 4 chunk + 3 of the row
__device__ __forceinline__ uint32_t drop_word(uint32_t row_key, uint32_t chunk) { return drop_mix(row_key + chunk * DROP_GOLD); }

__device__ __forceinline__ bool drop_keep(uint64_t seed, int b, int head, int query, int key, int threshold) {
  const uint32_t w = drop_word(drop_row_key(drop_head_key(seed, b, head), query), (uint32_t)key >> 2);
  return (int)((w >> (8 * (key & 3))) & 255u) >= threshold;
}

}  // namespace mha
