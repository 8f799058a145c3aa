// The 61-bit polynomial hash of a label string: the identity of a beam's string and of a partial word in ds2_beam.hip and lm.py's
// word table, and of a word in ds2_errors.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr uint64_t kM61 = (1ull << 61) - 1;          // prime modulus of the string hash
constexpr uint64_t kHashBase = 0x0b7e151628aed2a7ull;  // fixed base < kM61
constexpr uint64_t kHashEmpty = 0x1f3d5b79a2c4e6f8ull % kM61;

// hash(s + c) = (hash(s) * base + c + 1) mod (2^61 - 1)
__device__ __forceinline__ uint64_t hash_ext(uint64_t h, int c) {
  const uint64_t lo = h * kHashBase, hi = __umul64hi(h, kHashBase);
  uint64_t r = (lo & kM61) + ((lo >> 61) | (hi << 3));
  r = (r & kM61) + (r >> 61);
  r += (uint64_t)(c + 1);
  r = (r & kM61) + (r >> 61);
  return r >= kM61 ? r - kM61 : r;
}

}  // namespace
