// Scene-graph prediction: from the N scored generator samples of an image to its ranked list of DISTINCT triples (gfx950).
//   rank_triples   the host loop of the evaluation (reference train.py:314-327: accumulate, argsort, top-k; SceneGraphGAN._rank /
//                  recalls) as one workgroup per image, everything in LDS:
//                    1. score[k] = ((d0 + d1) + d2) / 3 in fp32 (what numpy's float32 mean over the three steps gives, bit for bit);
//                    2. bitonic sort of (orderable score bits, sample index): the stable argsort, NaN last in either direction;
//                    3. bitonic sort of (packed triple, rank): equal triples become one run whose head is the best-ranked sample;
//                       the run length (binary search for its end) is the triple's count;
//                    4. prefix sum of the run heads in rank order = the slot of every distinct triple.
// Not on the training path.
#include "sort_select.h"

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
    unsigned long long kk = SGG_SORT_PAD;                         // behind every sample in both sorts
    if (k < N) {
      const float s = rank_score(d, k, nb, j);
      if (sample_scores) sample_scores[(size_t)j * N + k] = s;
      unsigned o = 0xffffffffu;                                 // NaN: behind every number, in sample order
      if (s == s) o = descending ? ~sgg_orderable(s) : sgg_orderable(s);
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
    unsigned long long c = SGG_SORT_PAD;
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
    cnt[pay[q]] = (unsigned short)(sgg_upper_bound(key, q + 1, N, c) - q);      // head of the run = its smallest rank
  }
  __syncthreads();
  // 4. slot of every first occurrence: exclusive prefix sum of (cnt > 0) over the ranks, C consecutive ranks per thread
  const int C = P / T;
  int mine = 0;
  for (int e = 0; e < C; ++e) mine += cnt[tid * C + e] > 0;
  int total, base = sgg_block_scan(mine, wave_tot, &total);
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
    scores[o] = SGG_QNAN;
    first_rank[o] = -1;
    first_sample[o] = -1;
    counts[o] = 0;
  }
  if (tid == 0) n_distinct[j] = total;
}

extern "C" int sgg_rank_triples(const long long* tokens, const float* d, int N, int nb, int V, int K, int descending,
                                long long* triples, float* scores, int* first_rank, int* first_sample, int* counts, int* n_distinct,
                                float* sample_scores, void* stream) {
  SGG_CHECK_ARG(N >= 1 && N <= SGG_SORT_MAX_P, "sgg_rank_triples: 1 <= N <= %d samples per image (got %d)", SGG_SORT_MAX_P, N);
  SGG_CHECK_ARG(K >= 1 && K <= N, "sgg_rank_triples: 1 <= K <= N (got K = %d, N = %d)", K, N);
  SGG_CHECK_ARG(nb >= 1 && V >= 1 && V <= SGG_SORT_MAX_V, "sgg_rank_triples: nb >= 1 and 1 <= V <= 2^21 (got nb = %d, V = %d)", nb, V);
  SGG_CHECK_ARG(descending == 0 || descending == 1, "sgg_rank_triples: descending is 0 or 1 (got %d)", descending);
  SGG_CHECK_ARG(tokens && d && triples && scores && first_rank && first_sample && counts && n_distinct,
                "sgg_rank_triples: null pointer");
  const sgg_sort_geometry g(N, 128);
  hipLaunchKernelGGL(rank_triples_kernel, dim3(nb), dim3(g.T), (size_t)g.P * 14, (hipStream_t)stream, tokens, d, N, nb, K, g.P,
                     descending, triples, scores, first_rank, first_sample, counts, n_distinct, sample_scores);
  SGG_LAUNCH_CHECK("sgg_rank_triples");
  return SGG_OK;
}
