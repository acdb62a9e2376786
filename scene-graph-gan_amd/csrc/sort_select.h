// Sorting and selecting in LDS: what the evaluation kernels share (csrc/rank.hip, match.hip, kbest.hip, ground.hip, retrieve.hip).
// Everything is one workgroup of blockDim.x threads (a multiple of 64, at most 1024) over 64-bit keys; the formats are decided here:
//   packed triple   s << 42 | p << 21 | o, every token in [0, SGG_SORT_MAX_V): its order is the lexicographic order of the triple
//                   (rank step 3, match, kbest_merge, ground_assign); 63 bits, so it never equals SGG_SORT_PAD;
//   value key       ~orderable(value) << 21 | index, index in [0, SGG_KEY_MAX_INDEX): ascending key order = (value descending,
//                   index ascending), SGG_KEY_BITS = 53 bits wide (kbest_triples: logit and token; retrieve: score and image).  The
//                   radix selection takes its digit plan from that width;
//   orderable       the unsigned image of a float whose order is the float order, +-0 one value.  The kernels that sort whole
//                   64-bit words (rank step 2, the candidate and merge sorts of kbest) put it, or its complement, in the high word.
// A kernel that selects or scans hands in the LDS scratch (sgg_select_lds, 16 ints of wave totals): no helper owns storage.
#pragma once
#include "sgg_common.h"

#define SGG_SORT_MAX_P 4096                     // entries of one sort (the payload is an index below it)
#define SGG_SORT_FIELD_BITS 21                  // a token of a packed triple; the index of a value key
#define SGG_SORT_MAX_V (1 << SGG_SORT_FIELD_BITS)
#define SGG_KEY_MAX_INDEX (1 << SGG_SORT_FIELD_BITS)
#define SGG_KEY_BITS (32 + SGG_SORT_FIELD_BITS)
#define SGG_SORT_PAD 0xffffffffffffffffull      // sorts behind every real entry

// Launch geometry of a sort of n entries: P = the power of two >= max(n, min_p), T = P / 2 threads up to 1024 (64 .. 1024 from
// min_p = 128: at least two entries per thread, T divides P, P / T <= 4 at SGG_SORT_MAX_P)
#ifdef __HIPCC__
#define SGG_HOST_DEVICE __host__ __device__     // (retrieve_ranks sizes its sort on the device)
#else
#define SGG_HOST_DEVICE
#endif
struct sgg_sort_geometry {
  int P, T;
  SGG_HOST_DEVICE sgg_sort_geometry(int n, int min_p) {
    for (P = min_p; P < n; P <<= 1) {}
    T = P / 2 > 1024 ? 1024 : P / 2;
  }
};

#ifdef __HIPCC__
#define SGG_QNAN __uint_as_float(0x7fc00000u)   // what a slot without a result holds

// ascending bitonic sort of the P (a power of two) pairs (key[i], pay[i]), compared as (key, pay)
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

// ---- formats ---------------------------------------------------------------------------------------------------------------------
// float -> unsigned whose order is the float order (-inf lowest, +inf = 0xff800000 highest); +-0 are one value
__device__ __forceinline__ unsigned sgg_orderable(float s) {
  const unsigned b = (s == 0.f) ? 0u : __float_as_uint(s);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float sgg_from_orderable(unsigned o) {
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

__device__ __forceinline__ unsigned long long sgg_value_key(float v, int index) {
  return ((unsigned long long)(unsigned)~sgg_orderable(v) << SGG_SORT_FIELD_BITS) | (unsigned long long)index;
}
__device__ __forceinline__ int sgg_value_key_index(unsigned long long k) { return (int)(k & (unsigned long long)(SGG_KEY_MAX_INDEX - 1)); }

__device__ __forceinline__ bool sgg_in_vocab3(const long long* t, int V) {
  return t[0] >= 0 && t[0] < V && t[1] >= 0 && t[1] < V && t[2] >= 0 && t[2] < V;
}
__device__ __forceinline__ unsigned long long sgg_pack_triple(long long s, long long p, long long o) {
  return ((unsigned long long)(s & (SGG_SORT_MAX_V - 1)) << 42) | ((unsigned long long)(p & (SGG_SORT_MAX_V - 1)) << 21) |
         (unsigned long long)(o & (SGG_SORT_MAX_V - 1));
}
__device__ __forceinline__ void sgg_unpack_triple(unsigned long long c, int& s, int& p, int& o) {
  s = (int)(c >> 42);
  p = (int)(c >> 21) & (SGG_SORT_MAX_V - 1);
  o = (int)c & (SGG_SORT_MAX_V - 1);
}

// ---- searches over ascending keys ------------------------------------------------------------------------------------------------
// first position in [lo, hi) whose key is >= c (hi where there is none)
__device__ __forceinline__ int sgg_lower_bound(const unsigned long long* key, int lo, int hi, unsigned long long c) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (key[mid] < c) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// first position in [lo, hi) whose key is > c: from q + 1, the end of the run of c = key[q]
__device__ __forceinline__ int sgg_upper_bound(const unsigned long long* key, int lo, int hi, unsigned long long c) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (key[mid] <= c) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// ---- prefix sums -----------------------------------------------------------------------------------------------------------------
// inclusive prefix sum over the 64 lanes of a wave
__device__ __forceinline__ int sgg_wave_scan(int v) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(v, o, 64);
    if ((threadIdx.x & 63) >= o) v += u;
  }
  return v;
}
// exclusive prefix sum of `mine` over the threads of the workgroup -> the thread's base and, where asked for (total != nullptr: a
// caller without use for it reads only the waves before its own), the sum over all of them.
// wave_tot: 16 ints of LDS that no thread still reads; one barrier, which every thread of the workgroup must reach
__device__ __forceinline__ int sgg_block_scan(int mine, int* wave_tot, int* total = nullptr) {
  const int incl = sgg_wave_scan(mine), wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 63) wave_tot[wave] = incl;
  __syncthreads();
  int base = incl - mine, sum = 0;
  for (int w = 0; w < (total ? (int)(blockDim.x >> 6) : wave); ++w) {
    if (w < wave) base += wave_tot[w];
    sum += wave_tot[w];
  }
  if (total) *total = sum;
  return base;
}

// ---- selection -------------------------------------------------------------------------------------------------------------------
struct alignas(16) sgg_select_lds {              // scratch of a selecting kernel, in its __shared__ storage (1040 bytes)
  int hist[256];                                 // (16-byte aligned: the scan reads four bins at a time)
  unsigned long long prefix;
  int rem, cnt;
};

// The key of rank `rem` (0-based) among the n DISTINCT value keys key_of(0 .. n - 1): radix selection, most significant digit
// first, one histogram pass over the keys per digit (ceil(SGG_KEY_BITS / 8) = 7 passes: six digits of 8 bits and one of 5; the
// first shift is 45).  Every thread gets the key; the first wave finds the digit's bucket, four buckets per lane.
template <class KeyOf>
__device__ __forceinline__ unsigned long long sgg_radix_select(KeyOf key_of, int n, int rem, sgg_select_lds& s) {
  const int T = blockDim.x, tid = threadIdx.x;
  constexpr int passes = (SGG_KEY_BITS + 7) / 8, last_width = SGG_KEY_BITS - 8 * (passes - 1);
  unsigned long long prefix = 0;
  for (int pass = 0; pass < passes; ++pass) {
    const int width = pass < passes - 1 ? 8 : last_width, shift = pass < passes - 1 ? SGG_KEY_BITS - 8 - 8 * pass : 0;
    for (int b = tid; b < 256; b += T) s.hist[b] = 0;
    __syncthreads();
    for (int t = tid; t < n; t += T) {
      const unsigned long long k = key_of(t);
      if ((k >> (shift + width)) == prefix) atomicAdd(&s.hist[(int)(k >> shift) & ((1 << width) - 1)], 1);
    }
    __syncthreads();
    if (tid < 64) {
      const int c0 = s.hist[4 * tid], c1 = s.hist[4 * tid + 1], c2 = s.hist[4 * tid + 2], c3 = s.hist[4 * tid + 3];
      const int tot = c0 + c1 + c2 + c3, incl = sgg_wave_scan(tot);
      const unsigned long long ahead = __ballot(incl > rem);      // (never empty: rem < the keys under this prefix)
      if (ahead != 0 && tid == __ffsll((long long)ahead) - 1) {
        int r = rem - (incl - tot), d = 0;
        if (r >= c0) { r -= c0; d = 1; if (r >= c1) { r -= c1; d = 2; if (r >= c2) { r -= c2; d = 3; } } }
        s.prefix = (prefix << width) | (unsigned long long)(4 * tid + d);
        s.rem = r;
      }
    }
    __syncthreads();
    prefix = s.prefix;
    rem = s.rem;
  }
  return prefix;
}

// The M smallest of those keys, ascending, in sel[0 .. M); SGG_SORT_PAD behind them up to sel[P) (P a power of two >= M; pay[P]
// is the sort's payload and ends as zeros).  The keys up to the M-th are collected in any order - they are unique, so exactly M
// - and sorted once.
template <class KeyOf>
__device__ __forceinline__ void sgg_select_sorted(KeyOf key_of, int n, int M, unsigned long long* sel, unsigned short* pay, int P,
                                                  sgg_select_lds& s) {
  const int T = blockDim.x, tid = threadIdx.x;
  const unsigned long long kth = sgg_radix_select(key_of, n, M - 1, s);
  for (int r = tid; r < P; r += T) { sel[r] = SGG_SORT_PAD; pay[r] = 0; }
  if (tid == 0) s.cnt = 0;
  __syncthreads();
  for (int t = tid; t < n; t += T) {
    const unsigned long long k = key_of(t);
    if (k <= kth) {
      const int pos = atomicAdd(&s.cnt, 1);
      if (pos < P) sel[pos] = k;
    }
  }
  sgg_bitonic_pairs(sel, pay, P);
}
#endif
