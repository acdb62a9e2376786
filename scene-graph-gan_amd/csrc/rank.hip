// Scene-graph prediction: from the N scored generator samples of an image to its ranked list of DISTINCT triples (gfx950).
//   rank_triples   the host loop of the evaluation (reference train.py:314-327: accumulate, argsort, top-k; SceneGraphGAN._rank /
//                  recalls) as one workgroup per image, everything in LDS:
//                    1. score[k] = ((d0 + d1) + d2) / 3 in fp32 (what numpy's float32 mean over the three steps gives, bit for bit);
//                    2. bitonic sort of (orderable score bits, sample index): the stable argsort, NaN last in either direction;
//                    3. bitonic sort of (packed triple, rank): equal triples become one run whose head is the best-ranked sample;
//                       the run length (binary search for its end) is the triple's count;
//                    4. prefix sum of the run heads in rank order = the slot of every distinct triple.
// Not on the training path.
#include "bitonic.h"

#define RANK_MAX_N SGG_SORT_MAX_P
#define RANK_MAX_V SGG_SORT_MAX_V       // three tokens pack into 63 bits
#define RANK_PAD SGG_SORT_PAD           // sorts behind every sample in both sorts

// float -> unsigned whose order is the float order (-inf lowest, +inf = 0xff800000 highest); +-0 are one value
__device__ __forceinline__ unsigned rank_orderable(float s) {
  const unsigned b = (s == 0.f) ? 0u : __float_as_uint(s);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ float rank_score(const float* __restrict__ d, int k, int nb, int j) {
  const float* p = d + ((size_t)k * nb + j) * 3;
  return ((p[0] + p[1]) + p[2]) / 3.0f;       // correctly rounded division (no reciprocal: x * (1/3) differs in a third of the rows)
}

// LDS: key[P] (8 B), order[P], pay[P], cnt[P] (2 B each) = 14 * P bytes (56 KB at P = 4096)
__global__ __launch_bounds__(1024) void rank_triples_kernel(const long long* __restrict__ tokens, const float* __restrict__ d, int N,
                                                            int nb, int K, int P, int descending, long long* __restrict__ triples,
                                                            float* __restrict__ scores, int* __restrict__ first_rank,
                                                            int* __restrict__ first_sample, int* __restrict__ counts,
                                                            int* __restrict__ n_distinct, float* __restrict__ sample_scores) {
  extern __shared__ unsigned long long rank_lds[];
  __shared__ int wave_tot[16];
  unsigned long long* key = rank_lds;
  unsigned short* order = reinterpret_cast<unsigned short*>(key + P);
  unsigned short* pay = order + P;
  unsigned short* cnt = pay + P;
  const int j = blockIdx.x, T = blockDim.x, tid = threadIdx.x;

  // 1. scores -> (orderable key, sample index)
  for (int k = tid; k < P; k += T) {
    unsigned long long kk = RANK_PAD;
    if (k < N) {
      const float s = rank_score(d, k, nb, j);
      if (sample_scores) sample_scores[(size_t)j * N + k] = s;
      unsigned o = 0xffffffffu;                                 // NaN: behind every number, in sample order
      if (s == s) o = descending ? ~rank_orderable(s) : rank_orderable(s);
      kk = ((unsigned long long)o << 32) | (unsigned)k;
    }
    key[k] = kk;
    order[k] = (unsigned short)k;
    cnt[k] = 0;
  }
  // 2. the stable order: order[r] = sample at rank r
  sgg_bitonic_pairs(key, order, P);
  // 3. (packed triple, rank)
  for (int r = tid; r < P; r += T) {
    unsigned long long c = RANK_PAD;
    if (r < N) {
      const long long* t = tokens + ((size_t)order[r] * nb + j) * 3;
      c = sgg_pack_triple(t[0], t[1], t[2]);
    }
    key[r] = c;
    pay[r] = (unsigned short)r;
  }
  sgg_bitonic_pairs(key, pay, P);
  for (int q = tid; q < N; q += T) {             // (the first N sorted entries are the samples: the padding sorts last)
    const unsigned long long c = key[q];
    if (q > 0 && key[q - 1] == c) continue;
    int lo = q + 1, hi = N;                      // first position in (q, N] whose triple differs
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (key[mid] == c) lo = mid + 1; else hi = mid;
    }
    cnt[pay[q]] = (unsigned short)(lo - q);      // head of the run = its smallest rank
  }
  __syncthreads();
  // 4. slot of every first occurrence: exclusive prefix sum of (cnt > 0) over the ranks, C consecutive ranks per thread
  const int C = P / T;
  int mine = 0;
  for (int e = 0; e < C; ++e) mine += cnt[tid * C + e] > 0;
  int incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(incl, o, 64);
    if ((tid & 63) >= o) incl += v;
  }
  if ((tid & 63) == 63) wave_tot[tid >> 6] = incl;
  __syncthreads();
  int base = incl - mine, total = 0;
  for (int w = 0; w < (T >> 6); ++w) {
    if (w < (tid >> 6)) base += wave_tot[w];
    total += wave_tot[w];
  }
  for (int e = 0; e < C; ++e) {
    const int r = tid * C + e, c = cnt[r];
    if (c == 0) continue;
    const int u = base++;
    if (u >= K) continue;
    const int k = order[r];
    const size_t o = (size_t)j * K + u;
    const long long* t = tokens + ((size_t)k * nb + j) * 3;
    triples[o * 3 + 0] = t[0];
    triples[o * 3 + 1] = t[1];
    triples[o * 3 + 2] = t[2];
    scores[o] = rank_score(d, k, nb, j);
    first_rank[o] = r;
    first_sample[o] = k;
    counts[o] = c;
  }
  for (int u = total + tid; u < K; u += T) {
    const size_t o = (size_t)j * K + u;
    triples[o * 3 + 0] = -1; triples[o * 3 + 1] = -1; triples[o * 3 + 2] = -1;
    scores[o] = __uint_as_float(0x7fc00000u);
    first_rank[o] = -1;
    first_sample[o] = -1;
    counts[o] = 0;
  }
  if (tid == 0) n_distinct[j] = total;
}

extern "C" int sgg_rank_triples(const long long* tokens, const float* d, int N, int nb, int V, int K, int descending,
                                long long* triples, float* scores, int* first_rank, int* first_sample, int* counts, int* n_distinct,
                                float* sample_scores, void* stream) {
  SGG_CHECK_ARG(N >= 1 && N <= RANK_MAX_N, "sgg_rank_triples: 1 <= N <= %d samples per image (got %d)", RANK_MAX_N, N);
  SGG_CHECK_ARG(K >= 1 && K <= N, "sgg_rank_triples: 1 <= K <= N (got K = %d, N = %d)", K, N);
  SGG_CHECK_ARG(nb >= 1 && V >= 1 && V <= RANK_MAX_V, "sgg_rank_triples: nb >= 1 and 1 <= V <= 2^21 (got nb = %d, V = %d)", nb, V);
  SGG_CHECK_ARG(descending == 0 || descending == 1, "sgg_rank_triples: descending is 0 or 1 (got %d)", descending);
  SGG_CHECK_ARG(tokens && d && triples && scores && first_rank && first_sample && counts && n_distinct,
                "sgg_rank_triples: null pointer");
  int P = 128;                                   // power of two >= N; at least two entries per thread
  while (P < N) P <<= 1;
  const int T = P / 2 > 1024 ? 1024 : P / 2;     // 64 .. 1024, divides P
  hipLaunchKernelGGL(rank_triples_kernel, dim3(nb), dim3(T), (size_t)P * 14, (hipStream_t)stream, tokens, d, N, nb, K, P,
                     descending, triples, scores, first_rank, first_sample, counts, n_distinct, sample_scores);
  SGG_LAUNCH_CHECK("sgg_rank_triples");
  return SGG_OK;
}
