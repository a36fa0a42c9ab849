// qmpc_philox.h -- Random123's Philox4x32 with ten rounds, the tree's one counter-based generator, in plain C++,
// __host__ and __device__: qmpc_sense.hip draws its noise from it and qmpc_episode_rule.h its spawn and command rows.
// Multipliers 0xD2511F53 (on counter word 0) and 0xCD9E8D57 (on word 2), key increments 0x9E3779B9 / 0xBB67AE85 between
// the rounds; a round maps (c0, c1, c2, c3) to (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)).  The
// 32 x 32 -> 64 bit products are written as such: a multiply-high and a multiply-low on the device.
#ifndef QMPC_PHILOX_H
#define QMPC_PHILOX_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#include <hip/hip_runtime.h>
#define QMPC_PHILOX_HD __host__ __device__ __forceinline__
#else
#define QMPC_PHILOX_HD inline
#endif

QMPC_PHILOX_HD void qmpc_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                       uint32_t* w) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * (uint64_t)c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * (uint64_t)c2;
    c0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    c1 = (uint32_t)p1;
    c2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c3 = (uint32_t)p0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  w[0] = c0;
  w[1] = c1;
  w[2] = c2;
  w[3] = c3;
}

#endif
