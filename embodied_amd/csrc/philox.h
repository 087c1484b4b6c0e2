// Philox4x32-10 (Salmon et al., SC'11), the whole block at counter (g, offset)
// under key seed -- the keying onehot_sample.h documents:
//   key     = (seed & 0xffffffff, seed >> 32)
//   counter = (g & 0xffffffff, g >> 32, offset & 0xffffffff, offset >> 32)
// Device code only; included by onehot_sample.hip (word 0: the uniform of a
// group) and normal_policy.hip (words 0 and 1: the Box-Muller pair of an element).
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace emb {
namespace philox {

struct Block {
  uint32_t word[4];
};

__device__ __forceinline__ Block block(uint64_t seed, uint64_t offset, uint64_t g) {
  constexpr uint32_t kM0 = 0xD2511F53u, kM1 = 0xCD9E8D57u, kW0 = 0x9E3779B9u, kW1 = 0xBB67AE85u;
  uint32_t k0 = static_cast<uint32_t>(seed), k1 = static_cast<uint32_t>(seed >> 32);
  uint32_t c0 = static_cast<uint32_t>(g), c1 = static_cast<uint32_t>(g >> 32);
  uint32_t c2 = static_cast<uint32_t>(offset), c3 = static_cast<uint32_t>(offset >> 32);
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint32_t hi0 = __umulhi(kM0, c0), lo0 = kM0 * c0;
    const uint32_t hi1 = __umulhi(kM1, c2), lo1 = kM1 * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += kW0;
    k1 += kW1;
  }
  return Block{{c0, c1, c2, c3}};
}

}  // namespace philox
}  // namespace emb
