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
#include "bitonic.h"

#define KBEST_MAX_K 128                         // 5136 rank tuples at K = 256 would not fit one 4096-entry sort
#define KBEST_MAX_POOL SGG_SORT_MAX_P
#define KBEST_MAX_V SGG_SORT_MAX_V
#define KBEST_PAD SGG_SORT_PAD
#define KBEST_T 512                             // threads of a kbest_triples workgroup

// float -> unsigned whose order is the float order; +-0 are one value (rank.hip's rank_orderable)
__device__ __forceinline__ unsigned kbest_orderable(float s) {
  const unsigned b = (s == 0.f) ? 0u : __float_as_uint(s);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float kbest_from_orderable(unsigned o) {
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

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

// ascending key order = (logit descending, token ascending); 32 + 21 bits
__device__ __forceinline__ unsigned long long kbest_token_key(float x, int t) {
  return ((unsigned long long)(unsigned)~kbest_orderable(x) << 21) | (unsigned long long)t;
}

// LDS: key[P] (8 B) + pay[P] (2 B) of the candidate sort (40 KB at P = 4096) + 5.4 KB static (sel 1 KB, sel_pay 256 B,
//      tok_s and a_s 1.5 KB each, hist 1 KB, the rest under 100 B)
__global__ __launch_bounds__(KBEST_T) void kbest_triples_kernel(const float* __restrict__ logits, long long ld, int V, int K, int M,
                                                                int P, long long* __restrict__ triples, float* __restrict__ logp,
                                                                float* __restrict__ lse_out) {
  extern __shared__ unsigned long long kbest_lds[];
  __shared__ unsigned long long sel[KBEST_MAX_K];
  __shared__ unsigned short sel_pay[KBEST_MAX_K];
  __shared__ int tok_s[3][KBEST_MAX_K];
  __shared__ float a_s[3][KBEST_MAX_K];
  __shared__ int hist[256];
  __shared__ float red[16];
  __shared__ unsigned long long prefix_s;
  __shared__ int rem_s, cnt_s;
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
    // the key of rank M - 1 among the V distinct keys: radix selection, most significant digit first
    unsigned long long prefix = 0;
    int rem = M - 1;
    for (int pass = 0; pass < 7; ++pass) {
      const int width = pass < 6 ? 8 : 5, shift = pass < 6 ? 45 - 8 * pass : 0;
      for (int b = tid; b < 256; b += T) hist[b] = 0;
      __syncthreads();
      for (int t = tid; t < V; t += T) {
        const unsigned long long k = kbest_token_key(xs[t], t);
        if ((k >> (shift + width)) == prefix) atomicAdd(&hist[(int)(k >> shift) & ((1 << width) - 1)], 1);
      }
      __syncthreads();
      if (tid < 64) {
        const int c0 = hist[4 * tid], c1 = hist[4 * tid + 1], c2 = hist[4 * tid + 2], c3 = hist[4 * tid + 3];
        const int tot = c0 + c1 + c2 + c3;
        int incl = tot;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const int v = __shfl_up(incl, o, 64);
          if (tid >= o) incl += v;
        }
        const unsigned long long ahead = __ballot(incl > rem);      // (never empty: rem < the keys under this prefix)
        if (ahead != 0 && tid == __ffsll((long long)ahead) - 1) {
          int r = rem - (incl - tot), d = 0;
          if (r >= c0) { r -= c0; d = 1; if (r >= c1) { r -= c1; d = 2; if (r >= c2) { r -= c2; d = 3; } } }
          prefix_s = (prefix << width) | (unsigned long long)(4 * tid + d);
          rem_s = r;
        }
      }
      __syncthreads();
      prefix = prefix_s;
      rem = rem_s;
    }
    // the M keys up to it, in any order, then sorted: rank r -> token
    for (int r = tid; r < KBEST_MAX_K; r += T) { sel[r] = KBEST_PAD; sel_pay[r] = 0; }
    if (tid == 0) cnt_s = 0;
    __syncthreads();
    for (int t = tid; t < V; t += T) {
      const unsigned long long k = kbest_token_key(xs[t], t);
      if (k <= prefix) {
        const int pos = atomicAdd(&cnt_s, 1);
        if (pos < KBEST_MAX_K) sel[pos] = k;
      }
    }
    sgg_bitonic_pairs(sel, sel_pay, KBEST_MAX_K);
    for (int r = tid; r < M; r += T) {
      const int t = (int)(sel[r] & (unsigned long long)(KBEST_MAX_V - 1));
      tok_s[s][r] = t;
      a_s[s][r] = xs[t < V ? t : 0] - lse;
    }
    __syncthreads();
  }

  // every rank tuple that can be among the K best -> (descending-orderable lp, i, j, l)
  for (int q = tid; q < P; q += T) { key[q] = KBEST_PAD; pay[q] = 0; }
  if (tid == 0) cnt_s = 0;
  __syncthreads();
  for (int ij = tid; ij < M * M; ij += T) {
    const int i = ij / M, j = ij - i * M, prod = (i + 1) * (j + 1);
    if (prod > K) continue;
    const int L = min(M, K / prod);
    const int base = atomicAdd(&cnt_s, L);
    const float a01 = a_s[0][i] + a_s[1][j];
    for (int l = 0; l < L && base + l < P; ++l) {
      const float lp = a01 + a_s[2][l];
      key[base + l] = ((unsigned long long)(unsigned)~kbest_orderable(lp) << 32) | (unsigned long long)((i << 14) | (j << 7) | l);
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
    unsigned long long c = KBEST_PAD;
    if (q < n) {
      const int k = q / Kc, u = q - k * Kc;
      const long long* t = lists + (((size_t)k * nb + j) * Kc + u) * 3;
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
    next[e] = KBEST_PAD;
    cnt[q] = 0;
    best[q] = 0;
    if (c == KBEST_PAD || (q > 0 && key[q - 1] == c)) continue;
    int lo = q + 1, hi = P;                         // first position behind q whose triple differs (the padding differs from all)
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (key[mid] == c) lo = mid + 1; else hi = mid;
    }
    const int t0 = (int)(c >> 42), t1 = (int)(c >> 21) & (KBEST_MAX_V - 1), t2 = (int)c & (KBEST_MAX_V - 1);
    float m = -INFINITY;
    int bk = 0;
    for (int k = 0; k < N; ++k) {
      const float lp = kbest_row_lp(logits, ld, V, lse, (size_t)k * nb + j, t0, t1, t2);
      if (lp > m) { m = lp; bk = k; }
    }
    float sum = 0.f;
    for (int k = 0; k < N; ++k) sum += expf(kbest_row_lp(logits, ld, V, lse, (size_t)k * nb + j, t0, t1, t2) - m);
    const float score = m + (logf(sum) - log_n);
    cnt[q] = (unsigned short)(lo - q);
    best[q] = (unsigned short)bk;
    // (q, the position among the sorted packed triples, breaks ties of the score in packed-triple order)
    next[e] = ((unsigned long long)(unsigned)~kbest_orderable(score) << 32) | (unsigned long long)q;
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
      scores[o] = kbest_from_orderable(~(unsigned)(kk >> 32));
      best_sample[o] = best[q];
      best_logp[o] = kbest_row_lp(logits, ld, V, lse, (size_t)best[q] * nb + j, (int)t0, (int)t1, (int)t2);
      counts[o] = cnt[q];
    } else {
      triples[o * 3 + 0] = -1; triples[o * 3 + 1] = -1; triples[o * 3 + 2] = -1;
      scores[o] = __uint_as_float(0x7fc00000u);
      best_sample[o] = -1;
      best_logp[o] = __uint_as_float(0x7fc00000u);
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
  SGG_CHECK_ARG(R >= 1 && V >= 1 && V <= KBEST_MAX_V, "sgg_kbest_triples: R >= 1 and 1 <= V <= 2^21 (got R = %d, V = %d)", R, V);
  const long long v3 = V >= KBEST_MAX_K ? (long long)KBEST_MAX_K : (long long)V * V * V;
  SGG_CHECK_ARG(K >= 1 && K <= KBEST_MAX_K && K <= v3, "sgg_kbest_triples: 1 <= K <= min(%d, V^3) (got K = %d, V = %d)", KBEST_MAX_K, K,
                V);
  SGG_CHECK_ARG(ld >= 3LL * V, "sgg_kbest_triples: row stride ld >= 3 V (got ld = %lld, V = %d)", ld, V);
  SGG_CHECK_ARG(logits && triples && logp && lse, "sgg_kbest_triples: null pointer");
  const int M = K < V ? K : V;
  int P = 128;
  while (P < kbest_candidates(K, M)) P <<= 1;
  SGG_CHECK_ARG(P <= KBEST_MAX_POOL, "sgg_kbest_triples: %d candidates exceed one sort", kbest_candidates(K, M));
  hipLaunchKernelGGL(kbest_triples_kernel, dim3(R), dim3(KBEST_T), (size_t)P * 10, (hipStream_t)stream, logits, ld, V, K, M, P, triples,
                     logp, lse);
  SGG_LAUNCH_CHECK("sgg_kbest_triples");
  return SGG_OK;
}

extern "C" int sgg_kbest_merge(const long long* lists, const float* logits, long long ld, const float* lse, int N, int nb, int Kc, int V,
                               int K, long long* triples, float* scores, int* best_sample, float* best_logp, int* counts,
                               int* n_distinct, void* stream) {
  SGG_CHECK_ARG(N >= 1 && Kc >= 1 && (long long)N * Kc <= KBEST_MAX_POOL,
                "sgg_kbest_merge: N >= 1, Kc >= 1 and N * Kc <= %d list entries per image (got N = %d, Kc = %d)", KBEST_MAX_POOL, N, Kc);
  SGG_CHECK_ARG(K >= 1 && K <= N * Kc, "sgg_kbest_merge: 1 <= K <= N * Kc (got K = %d, N = %d, Kc = %d)", K, N, Kc);
  SGG_CHECK_ARG(nb >= 1 && V >= 1 && V <= KBEST_MAX_V, "sgg_kbest_merge: nb >= 1 and 1 <= V <= 2^21 (got nb = %d, V = %d)", nb, V);
  SGG_CHECK_ARG(ld >= 3LL * V, "sgg_kbest_merge: row stride ld >= 3 V (got ld = %lld, V = %d)", ld, V);
  SGG_CHECK_ARG(lists && logits && lse && triples && scores && best_sample && best_logp && counts && n_distinct,
                "sgg_kbest_merge: null pointer");
  int P = 128;                                   // power of two >= N * Kc; at least two entries per thread
  while (P < N * Kc) P <<= 1;
  const int T = P / 2 > 1024 ? 1024 : P / 2;     // 64 .. 1024, divides P; P / T <= 4
  hipLaunchKernelGGL(kbest_merge_kernel, dim3(nb), dim3(T), (size_t)P * 14, (hipStream_t)stream, lists, logits, ld, lse, N, nb, Kc, V, K,
                     P, triples, scores, best_sample, best_logp, counts, n_distinct);
  SGG_LAUNCH_CHECK("sgg_kbest_merge");
  return SGG_OK;
}
