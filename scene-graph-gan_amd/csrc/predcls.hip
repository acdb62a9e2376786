// Predicate classification: for given (subject, object) pairs of an image, the generator's mixture log-probability of EVERY predicate
// token, the predicates ranked per pair and the (pair, predicate) candidates ranked across the pairs of the image (gfx950).
// The arithmetic of a term is that of csrc/xent.hip's triple_logp, bit for bit:
//     a_t(x) = logits[t][x] - lse[t],   lp_k(v) = (a_0(s) + a_1(v)) + a_2(o),   m = max_k lp_k
//     joint(v) = m + (log(sum_k exp(lp_k - m)) - log N)     summed in sample order in fp32
//     marg     = the same with a_1 = 0.f: the pair's log-probability with the predicate marginalised (its softmax sums to 1)
//   pair_predicate_logp  grid (column tile, pair tile, image), one thread per predicate column v, PCLS_TP pairs per workgroup.  The
//                        draws are walked PCLS_DK at a time: the chunk's a_0(s_p), a_2(o_p) of the tile's pairs (2 x 16 x 64 floats,
//                        8 KB) and its predicate lse are gathered into LDS, then every thread reads its column of the chunk's
//                        predicate rows ONCE (coalesced) and updates all PCLS_TP pairs from LDS broadcasts.  Two walks: the
//                        maxima, then the sums against them - the two loops of triple_logp, so the bits are its bits.  The threads
//                        tid < PCLS_TP of column tile 0 carry marg of pair tid beside it.
//   predcls_pair_topk    one workgroup per (pair, image): the first Kc tokens of the pair's joint row under (joint descending, token
//                        ascending) by sgg_select_sorted (value keys), and for every true triple of the pair the 1-based rank of
//                        its predicate in that order (a count of smaller keys: integers).
//   predcls_merge        one workgroup per image: the candidates (pair i, slot r < per_pair) under (score descending, i ascending,
//                        r ascending) - one value key per candidate, its index i * per_pair + r - the first K of them.
// Finite logits are a precondition.  No workspace, no float atomics: the LDS atomics count integers or hand out slots of an array
// that is sorted by unique keys afterwards, so two calls give the same bits.  Not on the training path.
#include "sort_select.h"

#define PCLS_T 256                               // threads = predicate columns of a pair_predicate_logp workgroup
#define PCLS_TP 16                               // pairs of a workgroup: 2 x 16 accumulators per thread
#define PCLS_DK 64                               // draws per LDS chunk: 64 x 16 x (a_0, a_2) = 8 KB
#define PCLS_MAX_N 4096
#define PCLS_MAX_P 4096
#define PCLS_MAX_KC 128
#define PCLS_MAX_M 4096
#define PCLS_MAX_K 1024
#define PCLS_PADDING (-3)
#define PCLS_INVALID (-4)

// ---- pair_predicate_logp ---------------------------------------------------------------------------------------------------------
// LDS: ab 8 KB + z1 256 B + the tile's tokens 192 B
__global__ __launch_bounds__(PCLS_T) void pair_predicate_logp_kernel(const float* __restrict__ logits, long long ld,
                                                                     const float* __restrict__ lse, int N, int nb, int V,
                                                                     const int* __restrict__ pairs, const int* __restrict__ pair_count,
                                                                     int P, float* __restrict__ joint, long long ldj,
                                                                     float* __restrict__ marg, int* __restrict__ status) {
  __shared__ float2 ab[PCLS_DK][PCLS_TP];        // (a_0(s_p), a_2(o_p)) of draw k0 + k; zeros for a pair that is not valid
  __shared__ float z1[PCLS_DK];                  // the predicate row's lse of draw k0 + k
  __shared__ int tok_s[PCLS_TP], tok_o[PCLS_TP], st_s[PCLS_TP];
  const int tid = threadIdx.x, j = blockIdx.z, p0 = blockIdx.y * PCLS_TP;
  const int v = blockIdx.x * PCLS_T + tid;
  const int vr = v < V ? v : V - 1;              // the column this thread reads (the last tile's spare threads re-read V - 1)
  if (tid < PCLS_TP) {
    const int p = p0 + tid;
    int cnt = pair_count[j];
    cnt = cnt < 0 ? 0 : (cnt > P ? P : cnt);
    int st = PCLS_PADDING, s = 0, o = 0;
    if (p < cnt) {
      s = pairs[((size_t)j * P + p) * 2];
      o = pairs[((size_t)j * P + p) * 2 + 1];
      st = (s >= 0 && s < V && o >= 0 && o < V) ? 0 : PCLS_INVALID;
    }
    tok_s[tid] = st == 0 ? s : 0;
    tok_o[tid] = st == 0 ? o : 0;
    st_s[tid] = st;
  }
  float m[PCLS_TP], sum[PCLS_TP];
#pragma unroll
  for (int p = 0; p < PCLS_TP; ++p) { m[p] = -INFINITY; sum[p] = 0.f; }
  const bool margin = blockIdx.x == 0 && tid < PCLS_TP;      // this thread also carries marg of pair p0 + tid
  __syncthreads();
  bool any = false;
#pragma unroll
  for (int p = 0; p < PCLS_TP; ++p) any |= st_s[p] == 0;
  if (!any) {                                    // a tile of padding (uniform over the workgroup): NaN rows, no walk
    if (v < V)
      for (int p = 0; p < PCLS_TP && p0 + p < P; ++p) joint[((size_t)j * P + p0 + p) * (size_t)ldj + v] = SGG_QNAN;
    if (margin && p0 + tid < P) {
      marg[(size_t)j * P + p0 + tid] = SGG_QNAN;
      status[(size_t)j * P + p0 + tid] = st_s[tid];
    }
    return;
  }
  float mm = -INFINITY, msum = 0.f;
  const float* xv = logits + (size_t)j * (size_t)ld + (size_t)V + vr;       // column vr of the predicate row of (draw 0, image j)
  const size_t draw = (size_t)nb * (size_t)ld;

  for (int pass = 0; pass < 2; ++pass) {
    for (int k0 = 0; k0 < N; k0 += PCLS_DK) {
      const int nk = min(PCLS_DK, N - k0);
      __syncthreads();                           // the chunk before has been read (and, first, the tile's tokens are written)
      for (int i = tid; i < nk * PCLS_TP; i += PCLS_T) {
        const int k = i / PCLS_TP, p = i - k * PCLS_TP;
        float2 a = make_float2(0.f, 0.f);
        if (st_s[p] == 0) {
          const size_t r = (size_t)(k0 + k) * nb + j;
          const float* x = logits + r * (size_t)ld;
          a.x = x[tok_s[p]] - lse[r * 3];
          a.y = x[2 * (size_t)V + tok_o[p]] - lse[r * 3 + 2];
        }
        ab[k][p] = a;
      }
      if (tid < nk) z1[tid] = lse[((size_t)(k0 + tid) * nb + j) * 3 + 1];
      __syncthreads();
      const float* xk = xv + (size_t)k0 * draw;
      if (pass == 0) {
#pragma unroll 4
        for (int k = 0; k < nk; ++k) {
          const float a1 = xk[(size_t)k * draw] - z1[k];
#pragma unroll
          for (int p = 0; p < PCLS_TP; ++p) {
            const float lp = (ab[k][p].x + a1) + ab[k][p].y;
            if (lp > m[p]) m[p] = lp;
          }
        }
        if (margin)
          for (int k = 0; k < nk; ++k) {
            const float lp = (ab[k][tid].x + 0.f) + ab[k][tid].y;
            if (lp > mm) mm = lp;
          }
      } else {
#pragma unroll 4
        for (int k = 0; k < nk; ++k) {
          const float a1 = xk[(size_t)k * draw] - z1[k];
#pragma unroll
          for (int p = 0; p < PCLS_TP; ++p) {
            const float lp = (ab[k][p].x + a1) + ab[k][p].y;
            sum[p] += expf(lp - m[p]);
          }
        }
        if (margin)
          for (int k = 0; k < nk; ++k) {
            const float lp = (ab[k][tid].x + 0.f) + ab[k][tid].y;
            msum += expf(lp - mm);
          }
      }
    }
  }
  const float log_n = logf((float)N);
  if (v < V) {
#pragma unroll
    for (int p = 0; p < PCLS_TP; ++p)
      if (p0 + p < P) joint[((size_t)j * P + p0 + p) * (size_t)ldj + v] = st_s[p] == 0 ? m[p] + (logf(sum[p]) - log_n) : SGG_QNAN;
  }
  if (margin && p0 + tid < P) {
    const size_t o = (size_t)j * P + p0 + tid;
    marg[o] = st_s[tid] == 0 ? mm + (logf(msum) - log_n) : SGG_QNAN;
    status[o] = st_s[tid];
  }
}

// the number of threads of the workgroup whose `flag` is set, summed over `mine`; red: 16 ints nobody still reads; two barriers
__device__ __forceinline__ int pcls_block_count(int mine, int* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mine;
  __syncthreads();
  int tot = 0;
  for (int w = 0; w < (int)(blockDim.x >> 6); ++w) tot += red[w];
  return tot;
}

// ---- predcls_pair_topk -----------------------------------------------------------------------------------------------------------
// LDS: sel 1 KB + pay 256 B + the selection's scratch 1 KB + hits 16 KB
__global__ __launch_bounds__(1024) void predcls_pair_topk_kernel(const float* __restrict__ joint, long long ldj,
                                                                 const int* __restrict__ status, int P, int V, int Kc, int Msel, int Psel,
                                                                 const int* __restrict__ gt_pair, const int* __restrict__ gt_pred, int M,
                                                                 int* __restrict__ top_tok, float* __restrict__ top_score,
                                                                 int* __restrict__ gt_rank) {
  __shared__ unsigned long long sel[PCLS_MAX_KC];
  __shared__ unsigned short sel_pay[PCLS_MAX_KC];
  __shared__ sgg_select_lds sl;
  __shared__ int hits[PCLS_MAX_M];               // the true triples of this pair (rows of gt_pair), in any order
  __shared__ int n_hits, red[16];
  const int T = blockDim.x, tid = threadIdx.x, i = blockIdx.x, j = blockIdx.y;
  const size_t pr = (size_t)j * P + i;
  const float* x = joint + pr * (size_t)ldj;
  const bool valid = status[pr] == 0;            // (uniform over the workgroup)
  const int* gp = gt_pair + (size_t)j * M;
  const int* gv = gt_pred + (size_t)j * M;
  int* gr = gt_rank + (size_t)j * M;
  if (tid == 0) n_hits = 0;
  __syncthreads();
  for (int mrow = tid; mrow < M; mrow += T) {
    const int q = gp[mrow];
    if (q == i) {
      const int t = gv[mrow];
      if (valid && t >= 0 && t < V) hits[atomicAdd(&n_hits, 1)] = mrow;
      else gr[mrow] = 0;
    } else if (i == 0 && (q < 0 || q >= P))
      gr[mrow] = 0;                              // a true triple without a candidate pair: the first workgroup of the image says so
  }
  if (!valid) {
    for (int u = tid; u < Kc; u += T) {
      top_tok[pr * Kc + u] = -1;
      top_score[pr * Kc + u] = SGG_QNAN;
    }
    return;
  }
  sgg_select_sorted([x](int t) { return sgg_value_key(x[t], t); }, V, Msel, sel, sel_pay, Psel, sl);
  for (int u = tid; u < Kc; u += T) {
    const int t = u < Msel ? sgg_value_key_index(sel[u]) : -1;
    const bool in = t >= 0 && t < V;             // (always below Msel: the Msel smallest keys are real ones)
    top_tok[pr * Kc + u] = in ? t : -1;
    top_score[pr * Kc + u] = in ? x[t] : SGG_QNAN;      // the input's own bits (the key has folded -0 into +0)
  }
  const int nh = n_hits;                         // (written before the barriers of the selection)
  for (int h = 0; h < nh; ++h) {
    const int mrow = hits[h], t = gv[mrow];
    const unsigned long long own = sgg_value_key(x[t], t);
    int ahead = 0;
    for (int c = tid; c < V; c += T) ahead += sgg_value_key(x[c], c) < own;
    ahead = pcls_block_count(ahead, red);
    if (tid == 0) gr[mrow] = 1 + ahead;
  }
}

// ---- predcls_merge ---------------------------------------------------------------------------------------------------------------
// LDS: sel 8 KB + pay 2 KB + the selection's scratch 1 KB
__global__ __launch_bounds__(1024) void predcls_merge_kernel(const int* __restrict__ pairs, const int* __restrict__ top_tok,
                                                             const float* __restrict__ top_score, const float* __restrict__ marg, int P,
                                                             int Kc, int per_pair, int conditional, int K, int Msel, int Psel,
                                                             long long* __restrict__ triples, float* __restrict__ scores,
                                                             int* __restrict__ src, int* __restrict__ n_distinct) {
  __shared__ unsigned long long sel[PCLS_MAX_K];
  __shared__ unsigned short sel_pay[PCLS_MAX_K];
  __shared__ sgg_select_lds sl;
  __shared__ int red[16];
  const int T = blockDim.x, tid = threadIdx.x, j = blockIdx.x, n = P * per_pair;
  const int* tt = top_tok + (size_t)j * P * Kc;
  const float* ts = top_score + (size_t)j * P * Kc;
  const float* mg = marg + (size_t)j * P;
  const int* pj = pairs + (size_t)j * P * 2;
  // candidate c = i * per_pair + r: its score, or -inf behind every real one (finite) where the slot is empty
  auto score_of = [=](int c) {
    const int i = c / per_pair, r = c - i * per_pair;
    const size_t e = (size_t)i * Kc + r;
    if (tt[e] < 0) return -INFINITY;
    return conditional ? ts[e] - mg[i] : ts[e];
  };
  int mine = 0;
  for (int c = tid; c < n; c += T) {
    const int i = c / per_pair, r = c - i * per_pair;
    mine += tt[(size_t)i * Kc + r] >= 0;
  }
  const int total = pcls_block_count(mine, red);
  sgg_select_sorted([=](int c) { return sgg_value_key(score_of(c), c); }, n, Msel, sel, sel_pay, Psel, sl);
  for (int u = tid; u < K; u += T) {
    const size_t o = (size_t)j * K + u;
    if (u < total && u < Msel) {
      const int c = sgg_value_key_index(sel[u]);
      const int i = c / per_pair, r = c - i * per_pair;
      triples[o * 3 + 0] = pj[2 * i];
      triples[o * 3 + 1] = tt[(size_t)i * Kc + r];
      triples[o * 3 + 2] = pj[2 * i + 1];
      scores[o] = score_of(c);
      src[o] = c;
    } else {
      triples[o * 3 + 0] = -1; triples[o * 3 + 1] = -1; triples[o * 3 + 2] = -1;
      scores[o] = SGG_QNAN;
      src[o] = -1;
    }
  }
  if (tid == 0) n_distinct[j] = total;
}

extern "C" int sgg_pair_predicate_logp(const float* logits, long long ld, const float* lse, int N, int nb, int V, const int* pairs,
                                       const int* pair_count, int P, float* joint, long long ldj, float* marg, int* status,
                                       void* stream) {
  SGG_CHECK_ARG(N >= 1 && N <= PCLS_MAX_N && P >= 1 && P <= PCLS_MAX_P,
                "sgg_pair_predicate_logp: 1 <= N <= 4096 and 1 <= P <= 4096 (got N = %d, P = %d)", N, P);
  SGG_CHECK_ARG(nb >= 1 && nb <= 65535 && V >= 1 && V <= SGG_SORT_MAX_V,
                "sgg_pair_predicate_logp: 1 <= nb <= 65535 and 1 <= V <= 2^21 (got nb = %d, V = %d)", nb, V);
  SGG_CHECK_ARG(ld >= 3LL * V, "sgg_pair_predicate_logp: row stride ld >= 3 V (got ld = %lld, V = %d)", ld, V);
  SGG_CHECK_ARG(ldj >= V, "sgg_pair_predicate_logp: joint row stride ldj >= V (got ldj = %lld, V = %d)", ldj, V);
  SGG_CHECK_ARG(logits && lse && pairs && pair_count && joint && marg && status, "sgg_pair_predicate_logp: null pointer");
  hipLaunchKernelGGL(pair_predicate_logp_kernel, dim3(sgg_cdiv(V, PCLS_T), sgg_cdiv(P, PCLS_TP), nb), dim3(PCLS_T), 0, (hipStream_t)stream,
                     logits, ld, lse, N, nb, V, pairs, pair_count, P, joint, ldj, marg, status);
  SGG_LAUNCH_CHECK("sgg_pair_predicate_logp");
  return SGG_OK;
}

extern "C" int sgg_predcls_pair_topk(const float* joint, long long ldj, const int* status, int nb, int P, int V, int Kc,
                                     const int* gt_pair, const int* gt_pred, int M, int* top_tok, float* top_score, int* gt_rank,
                                     void* stream) {
  SGG_CHECK_ARG(nb >= 1 && nb <= 65535 && P >= 1 && P <= PCLS_MAX_P && V >= 1 && V <= SGG_KEY_MAX_INDEX,
                "sgg_predcls_pair_topk: 1 <= nb <= 65535, 1 <= P <= 4096 and 1 <= V <= 2^21 (got nb = %d, P = %d, V = %d)", nb, P, V);
  SGG_CHECK_ARG(Kc >= 1 && Kc <= PCLS_MAX_KC, "sgg_predcls_pair_topk: 1 <= Kc <= %d (got Kc = %d)", PCLS_MAX_KC, Kc);
  SGG_CHECK_ARG(M >= 1 && M <= PCLS_MAX_M, "sgg_predcls_pair_topk: 1 <= M <= %d true triples per image (got M = %d)", PCLS_MAX_M, M);
  SGG_CHECK_ARG(ldj >= V, "sgg_predcls_pair_topk: joint row stride ldj >= V (got ldj = %lld, V = %d)", ldj, V);
  SGG_CHECK_ARG(joint && status && gt_pair && gt_pred && top_tok && top_score && gt_rank, "sgg_predcls_pair_topk: null pointer");
  const int Msel = Kc < V ? Kc : V;
  const int T = V >= 1024 ? 1024 : 256;          // threads for the passes over the row, not for the sort of the Msel survivors
  hipLaunchKernelGGL(predcls_pair_topk_kernel, dim3(P, nb), dim3(T), 0, (hipStream_t)stream, joint, ldj, status, P, V, Kc, Msel,
                     sgg_sort_geometry(Msel, 64).P, gt_pair, gt_pred, M, top_tok, top_score, gt_rank);
  SGG_LAUNCH_CHECK("sgg_predcls_pair_topk");
  return SGG_OK;
}

extern "C" int sgg_predcls_merge(const int* pairs, const int* top_tok, const float* top_score, const float* marg, int nb, int P, int Kc,
                                 int per_pair, int conditional, int K, long long* triples, float* scores, int* src, int* n_distinct,
                                 void* stream) {
  SGG_CHECK_ARG(nb >= 1 && P >= 1 && Kc >= 1 && Kc <= PCLS_MAX_KC, "sgg_predcls_merge: nb >= 1, P >= 1 and 1 <= Kc <= %d (got nb = %d, P = %d, Kc = %d)",
                PCLS_MAX_KC, nb, P, Kc);
  SGG_CHECK_ARG(per_pair >= 1 && per_pair <= Kc && (long long)P * per_pair <= SGG_KEY_MAX_INDEX,
                "sgg_predcls_merge: 1 <= per_pair <= Kc and P * per_pair <= 2^21 (got per_pair = %d, Kc = %d, P = %d)", per_pair, Kc, P);
  SGG_CHECK_ARG(K >= 1 && K <= PCLS_MAX_K, "sgg_predcls_merge: 1 <= K <= %d (got K = %d)", PCLS_MAX_K, K);
  SGG_CHECK_ARG(conditional == 0 || conditional == 1, "sgg_predcls_merge: conditional is 0 or 1 (got %d)", conditional);
  SGG_CHECK_ARG(pairs && top_tok && top_score && marg && triples && scores && src && n_distinct, "sgg_predcls_merge: null pointer");
  const int n = P * per_pair, Msel = K < n ? K : n;
  const int T = n >= 1024 ? 1024 : 256;
  hipLaunchKernelGGL(predcls_merge_kernel, dim3(nb), dim3(T), 0, (hipStream_t)stream, pairs, top_tok, top_score, marg, P, Kc, per_pair,
                     conditional, K, Msel, sgg_sort_geometry(Msel, 64).P, triples, scores, src, n_distinct);
  SGG_LAUNCH_CHECK("sgg_predcls_merge");
  return SGG_OK;
}
