// The LDS bitonic network of the ranking kernels (csrc/rank.hip, csrc/match.hip): 64-bit keys with a 16-bit payload.
#pragma once
#include "sgg_common.h"

#define SGG_SORT_MAX_P 4096                     // entries of one sort (the payload is an index below it)
#define SGG_SORT_MAX_V (1 << 21)                // three tokens pack into 63 bits: a packed triple never equals SGG_SORT_PAD
#define SGG_SORT_PAD 0xffffffffffffffffull      // sorts behind every real entry

#ifdef __HIPCC__
// ascending bitonic sort of the P (a power of two) pairs (key[i], pay[i]), compared as (key, pay); blockDim.x threads
__device__ __forceinline__ void sgg_bitonic_pairs(unsigned long long* key, unsigned short* pay, int P) {
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      __syncthreads();
      for (int t = threadIdx.x; t < (P >> 1); t += blockDim.x) {
        const int i = 2 * t - (t & (j - 1)), l = i + j;      // bit j of i is clear
        const unsigned long long a = key[i], b = key[l];
        const unsigned short pa = pay[i], pb = pay[l];
        const bool gt = a > b || (a == b && pa > pb);
        if (gt == ((i & k) == 0)) {
          key[i] = b; key[l] = a;
          pay[i] = pb; pay[l] = pa;
        }
      }
    }
  }
  __syncthreads();
}

// (s, p, o) with every token in [0, SGG_SORT_MAX_V) -> one key whose order is the lexicographic order of the triple
__device__ __forceinline__ unsigned long long sgg_pack_triple(long long s, long long p, long long o) {
  return ((unsigned long long)(s & (SGG_SORT_MAX_V - 1)) << 42) | ((unsigned long long)(p & (SGG_SORT_MAX_V - 1)) << 21) |
         (unsigned long long)(o & (SGG_SORT_MAX_V - 1));
}
#endif
