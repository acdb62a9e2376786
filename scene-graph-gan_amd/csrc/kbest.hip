// K-best decoding: ranked distinct triples from the generator's softmax, without sampling tokens and without the critic (gfx950).
// The three decoder outputs of a head row (reference generator_with_attention.py:85-90) are conditioned on the noise and the LSTM
// state, never on the token chosen at the step before, so given one noise vector the distribution over triples factorises:
//     lp(s, p, o) = (a_0(s) + a_1(p)) + a_2(o),   a_t(x) = logits[t][x] - lse[t]      (fp32, in exactly that association)
//   kbest_triples  one workgroup per head row: per slot the log-sum-exp and the top M = min(K, V) tokens under (logit descending,
//                  token ascending) - an exact radix selection of the M-th smallest 53-bit key (~orderable logit, token), seven
//                  histogram passes over the row - then every rank tuple (i, j, l) with (i+1)(j+1)(l+1) <= K (a triple is preceded
//                  by all triples at componentwise smaller-or-equal ranks, fp32 addition is monotone: at most 2045 tuples at K = 128)
//                  through ONE bitonic sort of (descending-orderable lp, i, j, l).
//   kbest_merge    one workgroup per image: the lists of its N samples sorted as packed triples (equal triples form one run), every
//                  distinct triple scored by its log-probability under the mixture of ALL N samples, a second sort by (score
//                  descending, packed triple ascending).
// Finite logits are a precondition of both.  Every result is a pure function of the inputs: the LDS atomics only count (integers)
// or hand out slots of arrays that are sorted by unique keys afterwards, so two calls give the same bits.
// Not on the training path.
#include "sort_select.h"

#define KBEST_MAX_K 128                         // 5136 rank tuples at K = 256 would not fit one 4096-entry sort
#define KBEST_T 512                             // threads of a kbest_triples workgroup

// block-wide max / sum in a fixed order (blockDim.x a multiple of 64, at most 1024); `red` holds 16 floats; every thread gets the result
__device__ __forceinline__ float kbest_block_max(float v, float* red) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = red[0];
  for (int w = 1; w < (int)(blockDim.x >> 6); ++w) r = fmaxf(r, red[w]);
  return r;
}
__device__ __forceinline__ float kbest_block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = red[0];
  for (int w = 1; w < (int)(blockDim.x >> 6); ++w) r += red[w];
  return r;
}

// LDS: key[P] (8 B) + pay[P] (2 B) of the candidate sort (40 KB at P = 4096) + 5.4 KB static (sel 1 KB, sel_pay 256 B,
//      tok_s and a_s 1.5 KB each, the selection's scratch 1 KB, the rest under 100 B)
__global__ __launch_bounds__(KBEST_T) void kbest_triples_kernel(const float* __restrict__ logits, long long ld, int V, int K, int M,
                                                                int P, long long* __restrict__ triples, float* __restrict__ logp,
                                                                float* __restrict__ lse_out) {
  extern __shared__ unsigned long long kbest_lds[];
  __shared__ unsigned long long sel[KBEST_MAX_K];
  __shared__ unsigned short sel_pay[KBEST_MAX_K];
  __shared__ int tok_s[3][KBEST_MAX_K];
  __shared__ float a_s[3][KBEST_MAX_K];
  __shared__ sgg_select_lds sl;
  __shared__ float red[16];
  unsigned long long* key = kbest_lds;
  unsigned short* pay = reinterpret_cast<unsigned short*>(key + P);
  const int T = blockDim.x, tid = threadIdx.x;
  const size_t row = blockIdx.x;
  const float* x = logits + row * (size_t)ld;

  for (int s = 0; s < 3; ++s) {
    const float* xs = x + (size_t)s * V;
    // log-sum-exp, stabilised by the maximum; fixed summation order
    float m = -INFINITY;
    for (int t = tid; t < V; t += T) m = fmaxf(m, xs[t]);
    m = kbest_block_max(m, red);
    float sum = 0.f;
    for (int t = tid; t < V; t += T) sum += expf(xs[t] - m);
    sum = kbest_block_sum(sum, red);
    const float lse = m + logf(sum);
    if (tid == 0) lse_out[row * 3 + s] = lse;
    // the M best tokens under (logit descending, token ascending): rank r -> token
    sgg_select_sorted([xs](int t) { return sgg_value_key(xs[t], t); }, V, M, sel, sel_pay, KBEST_MAX_K, sl);
    for (int r = tid; r < M; r += T) {
      const int t = sgg_value_key_index(sel[r]);
      tok_s[s][r] = t;
      a_s[s][r] = xs[t < V ? t : 0] - lse;
    }
    __syncthreads();
  }

  // every rank tuple that can be among the K best -> (descending-orderable lp, i, j, l)
  for (int q = tid; q < P; q += T) { key[q] = SGG_SORT_PAD; pay[q] = 0; }
  if (tid == 0) sl.cnt = 0;                       // (the selections are over: their slot counter hands out the candidates' slots)
  __syncthreads();
  for (int ij = tid; ij < M * M; ij += T) {
    const int i = ij / M, j = ij - i * M, prod = (i + 1) * (j + 1);
    if (prod > K) continue;
    const int L = min(M, K / prod);
    const int base = atomicAdd(&sl.cnt, L);
    const float a01 = a_s[0][i] + a_s[1][j];
    for (int l = 0; l < L && base + l < P; ++l) {
      const float lp = a01 + a_s[2][l];
      key[base + l] = ((unsigned long long)(unsigned)~sgg_orderable(lp) << 32) | (unsigned long long)((i << 14) | (j << 7) | l);
    }
  }
  sgg_bitonic_pairs(key, pay, P);
  for (int u = tid; u < K; u += T) {
    const unsigned c = (unsigned)key[u];
    const int i = (c >> 14) & 127, j = (c >> 7) & 127, l = c & 127;
    const size_t o = row * (size_t)K + u;
    triples[o * 3 + 0] = tok_s[0][i];
    triples[o * 3 + 1] = tok_s[1][j];
    triples[o * 3 + 2] = tok_s[2][l];
    logp[o] = (a_s[0][i] + a_s[1][j]) + a_s[2][l];
  }
}

// lp of the triple (t0, t1, t2) under head row `r`
__device__ __forceinline__ float kbest_row_lp(const float* __restrict__ logits, long long ld, int V, const float* __restrict__ lse,
                                              size_t r, int t0, int t1, int t2) {
  const float* x = logits + r * (size_t)ld;
  const float* z = lse + r * 3;
  return ((x[t0] - z[0]) + (x[(size_t)V + t1] - z[1])) + (x[2 * (size_t)V + t2] - z[2]);
}

// LDS: key[P] (8 B), pay[P], cnt[P], best[P] (2 B each) = 14 * P bytes (56 KB at P = 4096)
__global__ __launch_bounds__(1024) void kbest_merge_kernel(const long long* __restrict__ lists, const float* __restrict__ logits,
                                                           long long ld, const float* __restrict__ lse, int N, int nb, int Kc, int V,
                                                           int K, int P, long long* __restrict__ triples, float* __restrict__ scores,
                                                           int* __restrict__ best_sample, float* __restrict__ best_logp,
                                                           int* __restrict__ counts, int* __restrict__ n_distinct) {
  extern __shared__ unsigned long long kbest_lds[];
  __shared__ int total_s;
  unsigned long long* key = kbest_lds;
  unsigned short* pay = reinterpret_cast<unsigned short*>(key + P);
  unsigned short* cnt = pay + P;
  unsigned short* best = cnt + P;
  const int j = blockIdx.x, T = blockDim.x, tid = threadIdx.x, n = N * Kc;
  const float log_n = logf((float)N);

  // 1. (packed triple, pool index q = k * Kc + u); an entry with a token outside [0, V) is dropped (it would index outside the logits)
  for (int q = tid; q < P; q += T) {
    unsigned long long c = SGG_SORT_PAD;
    if (q < n) {
      const int k = q / Kc, u = q - k * Kc;
      const long long* t = lists + (((size_t)k * nb + j) * Kc + u) * 3;
      // (sgg_in_vocab3 spelled out on values loaded first: on the global pointer it reads a token only once the one before has
      //  passed, three dependent round trips per entry - measured 0.5 % of this kernel)
      const long long t0 = t[0], t1 = t[1], t2 = t[2];
      if (t0 >= 0 && t0 < V && t1 >= 0 && t1 < V && t2 >= 0 && t2 < V) c = sgg_pack_triple(t0, t1, t2);
    }
    key[q] = c;
    pay[q] = (unsigned short)q;
  }
  if (tid == 0) total_s = 0;
  sgg_bitonic_pairs(key, pay, P);
  // 2. every run head: its length, and the triple's log-probability under the mixture of all N samples (registers; the keys are
  //    replaced only after every thread has read its neighbours)
  unsigned long long next[4];                       // P / T <= 4
  const int C = P / T;
  for (int e = 0; e < C; ++e) {
    const int q = tid + e * T;
    const unsigned long long c = key[q];
    next[e] = SGG_SORT_PAD;
    cnt[q] = 0;
    best[q] = 0;
    if (c == SGG_SORT_PAD || (q > 0 && key[q - 1] == c)) continue;
    const int end = sgg_upper_bound(key, q + 1, P, c);      // (the padding is above every triple)
    int t0, t1, t2;
    sgg_unpack_triple(c, t0, t1, t2);
    float m = -INFINITY;
    int bk = 0;
    for (int k = 0; k < N; ++k) {
      const float lp = kbest_row_lp(logits, ld, V, lse, (size_t)k * nb + j, t0, t1, t2);
      if (lp > m) { m = lp; bk = k; }
    }
    float sum = 0.f;
    for (int k = 0; k < N; ++k) sum += expf(kbest_row_lp(logits, ld, V, lse, (size_t)k * nb + j, t0, t1, t2) - m);
    const float score = m + (logf(sum) - log_n);
    cnt[q] = (unsigned short)(end - q);
    best[q] = (unsigned short)bk;
    // (q, the position among the sorted packed triples, breaks ties of the score in packed-triple order)
    next[e] = ((unsigned long long)(unsigned)~sgg_orderable(score) << 32) | (unsigned long long)q;
    atomicAdd(&total_s, 1);
  }
  __syncthreads();
  for (int e = 0; e < C; ++e) key[tid + e * T] = next[e];
  // 3. (score descending, packed triple ascending); pay keeps the pool index of the run's first entry
  sgg_bitonic_pairs(key, pay, P);
  const int total = total_s;
  // 4. the first K
  for (int u = tid; u < K; u += T) {
    const size_t o = (size_t)j * K + u;
    if (u < total) {
      const unsigned long long kk = key[u];
      const int q = (int)(kk & 0xffffffffull), src = pay[u];
      const int k = src / Kc, uu = src - k * Kc;
      const long long* t = lists + (((size_t)k * nb + j) * Kc + uu) * 3;
      const long long t0 = t[0], t1 = t[1], t2 = t[2];
      triples[o * 3 + 0] = t0; triples[o * 3 + 1] = t1; triples[o * 3 + 2] = t2;
      scores[o] = sgg_from_orderable(~(unsigned)(kk >> 32));
      best_sample[o] = best[q];
      best_logp[o] = kbest_row_lp(logits, ld, V, lse, (size_t)best[q] * nb + j, (int)t0, (int)t1, (int)t2);
      counts[o] = cnt[q];
    } else {
      triples[o * 3 + 0] = -1; triples[o * 3 + 1] = -1; triples[o * 3 + 2] = -1;
      scores[o] = SGG_QNAN;
      best_sample[o] = -1;
      best_logp[o] = SGG_QNAN;
      counts[o] = 0;
    }
  }
  if (tid == 0) n_distinct[j] = total;
}

// rank tuples (i, j, l) below M with (i+1)(j+1)(l+1) <= K
static int kbest_candidates(int K, int M) {
  int n = 0;
  for (int i = 1; i <= M && i <= K; ++i)
    for (int j = 1; j <= M && i * j <= K; ++j) n += K / (i * j) < M ? K / (i * j) : M;
  return n;
}

extern "C" int sgg_kbest_triples(const float* logits, long long ld, int R, int V, int K, long long* triples, float* logp, float* lse,
                                 void* stream) {
  SGG_CHECK_ARG(R >= 1 && V >= 1 && V <= SGG_SORT_MAX_V, "sgg_kbest_triples: R >= 1 and 1 <= V <= 2^21 (got R = %d, V = %d)", R, V);
  const long long v3 = V >= KBEST_MAX_K ? (long long)KBEST_MAX_K : (long long)V * V * V;
  SGG_CHECK_ARG(K >= 1 && K <= KBEST_MAX_K && K <= v3, "sgg_kbest_triples: 1 <= K <= min(%d, V^3) (got K = %d, V = %d)", KBEST_MAX_K, K,
                V);
  SGG_CHECK_ARG(ld >= 3LL * V, "sgg_kbest_triples: row stride ld >= 3 V (got ld = %lld, V = %d)", ld, V);
  SGG_CHECK_ARG(logits && triples && logp && lse, "sgg_kbest_triples: null pointer");
  const int M = K < V ? K : V;
  const int P = sgg_sort_geometry(kbest_candidates(K, M), 128).P;
  SGG_CHECK_ARG(P <= SGG_SORT_MAX_P, "sgg_kbest_triples: %d candidates exceed one sort", kbest_candidates(K, M));
  hipLaunchKernelGGL(kbest_triples_kernel, dim3(R), dim3(KBEST_T), (size_t)P * 10, (hipStream_t)stream, logits, ld, V, K, M, P, triples,
                     logp, lse);
  SGG_LAUNCH_CHECK("sgg_kbest_triples");
  return SGG_OK;
}

extern "C" int sgg_kbest_merge(const long long* lists, const float* logits, long long ld, const float* lse, int N, int nb, int Kc, int V,
                               int K, long long* triples, float* scores, int* best_sample, float* best_logp, int* counts,
                               int* n_distinct, void* stream) {
  SGG_CHECK_ARG(N >= 1 && Kc >= 1 && (long long)N * Kc <= SGG_SORT_MAX_P,
                "sgg_kbest_merge: N >= 1, Kc >= 1 and N * Kc <= %d list entries per image (got N = %d, Kc = %d)", SGG_SORT_MAX_P, N, Kc);
  SGG_CHECK_ARG(K >= 1 && K <= N * Kc, "sgg_kbest_merge: 1 <= K <= N * Kc (got K = %d, N = %d, Kc = %d)", K, N, Kc);
  SGG_CHECK_ARG(nb >= 1 && V >= 1 && V <= SGG_SORT_MAX_V, "sgg_kbest_merge: nb >= 1 and 1 <= V <= 2^21 (got nb = %d, V = %d)", nb, V);
  SGG_CHECK_ARG(ld >= 3LL * V, "sgg_kbest_merge: row stride ld >= 3 V (got ld = %lld, V = %d)", ld, V);
  SGG_CHECK_ARG(lists && logits && lse && triples && scores && best_sample && best_logp && counts && n_distinct,
                "sgg_kbest_merge: null pointer");
  const sgg_sort_geometry g(N * Kc, 128);        // P / T <= 4
  hipLaunchKernelGGL(kbest_merge_kernel, dim3(nb), dim3(g.T), (size_t)g.P * 14, (hipStream_t)stream, lists, logits, ld, lse, N, nb, Kc, V, K,
                     g.P, triples, scores, best_sample, best_logp, counts, n_distinct);
  SGG_LAUNCH_CHECK("sgg_kbest_merge");
  return SGG_OK;
}
