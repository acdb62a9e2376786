// Image retrieval by triple query: the generator's likelihood of a shared query list for every image of a collection, ranked across
// images on the device (gfx950).  The arithmetic of a term is that of csrc/kbest.hip and csrc/xent.hip:
//     a_t(x) = logits[t][x] - lse[t],   lp_k = (a_0 + a_1) + a_2   (fp32, in that association; an unspecified slot contributes 0.f)
//     score = logsumexp_k(lp_k) - log N: the log-probability of the (partial) triple under the mixture of the image's N noise draws
//   query_logp      grid (image, query tile).  The workgroup walks the N samples once, S samples per round: per round it gathers the
//                   a_t of the LISTED tokens only (W = u0 + u1 + u2 <= 3 U floats per sample, independent of V) into LDS, then every
//                   thread updates the online (max, sum) pair of its query from three LDS operands.  One array of LDS, 49 KB;
//                   the next round's loads are in flight in registers while the current one is consumed.
//   retrieve_topk   one workgroup per query: exact radix selection of the K-th smallest 53-bit key (~orderable score, image) - seven
//                   histogram passes over the row - then ONE bitonic sort of the survivors (sgg_select_sorted, csrc/sort_select.h).
//   retrieve_ranks  one workgroup per query: the keys of its relevant images sorted, every image of the row placed among them by a
//                   binary search (integer LDS counters), a prefix sum -> 1-based ranks; average precision in fp64 in a fixed order.
// Finite logits are a precondition of query_logp.  No float atomics: the LDS atomics count integers or hand out slots of an array
// that is sorted by unique keys afterwards, so two calls give the same bits.  Not on the training path.
#include "sort_select.h"

#define RETR_LDS_FLOATS 12288                    // 48 KB: one sample's logits of three full token lists of 4096
#define RETR_MAX_Q 4096
#define RETR_MAX_N 4096
#define RETR_MAX_K 1024
#define RETR_MAX_REL 4096
#define RETR_MAX_IMAGES SGG_KEY_MAX_INDEX        // the image is the index of a value key
#define RETR_MAX_ROUND 64                        // samples per gather round at most (3 * 64 lse values: the first 192 threads load them)

// ---- query_logp ----------------------------------------------------------------------------------------------------------------
// One query per thread: thread `tid` of tile blockIdx.y owns query blockIdx.y * blockDim.x + tid.
// A round is S samples: S * W logits in LDS in the order (sample of the round, element of the three lists), then their 3 S lse.
// Element f of a round is gathered by thread f % blockDim.x in its slot f / blockDim.x, and since the layout of every round is the
// same, where a slot reads - its offset from the round's first head row - is found ONCE and kept in registers; the token lists are
// never read again, and a round's loads are independent of each other and of any other load.  They are issued into registers BEFORE
// the round in LDS is consumed, so they are in flight under the exp chain of the current round (a software pipeline one round deep,
// no second buffer).  a_t = x - lse is formed when a query reads its operand (the lse read is a broadcast).
#define RETR_T 512                               // threads of a query_logp workgroup at most
#define RETR_SLOTS 24                            // gather slots of a thread: 24 * 512 threads = the 12288 logits of a round at most
#define RETR_BAD 0xffffffffffffffffull           // slot: nothing to gather (behind the round, or a token outside [0, V))

__global__ __launch_bounds__(RETR_T) void query_logp_kernel(const float* __restrict__ logits, long long ld, const float* __restrict__ lse,
                                                            int N, int nb, int V, const int* __restrict__ tok, int U, int u0, int u1,
                                                            int u2, const int* __restrict__ qidx, int Q, int S, float* __restrict__ scores,
                                                            long long lds, long long col0) {
  extern __shared__ float retr_a[];              // [S][W] logits of sample (k0 + s), slot segments at 0, u0, u0 + u1; then [S][3] lse
  const int T = blockDim.x, tid = threadIdx.x, j = blockIdx.x;
  const int W = u0 + u1 + u2, off1 = u0, off2 = u0 + u1;
  float* z = retr_a + S * W;
  const int q = blockIdx.y * T + tid;
  int o0 = -2, o1 = -2, o2 = -2;                 // LDS offsets of the query's operands inside a sample's segment; -1 wildcard, -2 invalid
  if (q < Q) {
    const int i0 = qidx[(size_t)q * 3], i1 = qidx[(size_t)q * 3 + 1], i2 = qidx[(size_t)q * 3 + 2];
    o0 = i0 == -1 ? -1 : (i0 >= 0 && i0 < u0 ? i0 : -2);
    o1 = i1 == -1 ? -1 : (i1 >= 0 && i1 < u1 ? off1 + i1 : -2);
    o2 = i2 == -1 ? -1 : (i2 >= 0 && i2 < u2 ? off2 + i2 : -2);
  }
  const bool live = o0 != -2 && o1 != -2 && o2 != -2;
  float m = -INFINITY, s = 0.f;
  // where slot i reads, in floats behind the round's first head row
  const int full = S * W;                        // <= RETR_SLOTS * T (the host chose S)
  unsigned long long goff[RETR_SLOTS];
#pragma unroll
  for (int i = 0; i < RETR_SLOTS; ++i) {
    const int f = tid + i * T;
    goff[i] = RETR_BAD;
    if (f < full) {
      const int sl = f / W, e = f - sl * W;
      const int slot = e < off1 ? 0 : (e < off2 ? 1 : 2);
      const int t = tok[slot * U + (e - (slot == 0 ? 0 : (slot == 1 ? off1 : off2)))];
      if (t >= 0 && t < V) goff[i] = ((unsigned long long)sl * nb + j) * (unsigned long long)ld + (unsigned long long)(slot * V + t);
    }
  }
  float v[RETR_SLOTS], zv = 0.f;
  // the loads of the round that starts at sample k0 (ns samples of it exist); NaN where there is no token
  auto gather = [&](int k0, int ns) {
    const float* x = logits + (size_t)k0 * nb * (size_t)ld;
#pragma unroll
    for (int i = 0; i < RETR_SLOTS; ++i) {
      v[i] = SGG_QNAN;
      if (goff[i] != RETR_BAD && tid + i * T < ns * W) v[i] = x[goff[i]];
    }
    if (tid < 3 * ns) zv = lse[((size_t)(k0 + tid / 3) * nb + j) * 3 + tid % 3];
  };
  gather(0, min(S, N));
  for (int k0 = 0; k0 < N; k0 += S) {
    const int ns = min(S, N - k0);
    __syncthreads();                             // the round before has been read
#pragma unroll
    for (int i = 0; i < RETR_SLOTS; ++i) {
      const int f = tid + i * T;
      if (f < ns * W) retr_a[f] = v[i];
    }
    if (tid < 3 * ns) z[tid] = zv;
    __syncthreads();
    if (k0 + S < N) gather(k0 + S, min(S, N - k0 - S));
    if (!live) continue;
    for (int sl = 0; sl < ns; ++sl) {
      const float* a = retr_a + sl * W;
      const float a0 = o0 >= 0 ? a[o0] - z[sl * 3] : 0.f, a1 = o1 >= 0 ? a[o1] - z[sl * 3 + 1] : 0.f,
                  a2 = o2 >= 0 ? a[o2] - z[sl * 3 + 2] : 0.f;
      const float lp = (a0 + a1) + a2;
      if (lp > m) {                              // online (max, sum): the sum rescaled to the new maximum
        s = s * expf(m - lp) + 1.f;
        m = lp;
      } else
        s += expf(lp - m);
    }
  }
  if (q < Q) scores[(size_t)q * (size_t)lds + (size_t)col0 + j] = live ? m + (logf(s) - logf((float)N)) : SGG_QNAN;
}

// ---- retrieve_topk ---------------------------------------------------------------------------------------------------------------
// LDS: sel 8 KB + pay 2 KB + the selection's scratch 1 KB
__global__ __launch_bounds__(1024) void retrieve_topk_kernel(const float* __restrict__ scores, long long lds, int n, int K, int M, int P,
                                                             int* __restrict__ idx, float* __restrict__ top) {
  __shared__ unsigned long long sel[RETR_MAX_K];
  __shared__ unsigned short sel_pay[RETR_MAX_K];
  __shared__ sgg_select_lds sl;
  const int T = blockDim.x, tid = threadIdx.x;
  const size_t q = blockIdx.x;
  const float* x = scores + q * (size_t)lds;
  // the M best images under (score descending, image ascending)
  sgg_select_sorted([x](int t) { return sgg_value_key(x[t], t); }, n, M, sel, sel_pay, P, sl);
  for (int u = tid; u < K; u += T) {
    const size_t o = q * (size_t)K + u;
    if (u < M) {
      const int image = sgg_value_key_index(sel[u]);
      const bool in = image < n;                 // (always: the M smallest keys are real ones)
      idx[o] = in ? image : -1;
      top[o] = in ? x[image] : SGG_QNAN;         // the input's own bits (the key has folded -0 into +0)
    } else {
      idx[o] = -1;
      top[o] = SGG_QNAN;
    }
  }
}

// ---- retrieve_ranks --------------------------------------------------------------------------------------------------------------
// LDS: key 32 KB + pay 8 KB + ahead 16 KB + under 1 KB
__global__ __launch_bounds__(1024) void retrieve_ranks_kernel(const float* __restrict__ scores, long long lds, int n,
                                                              const int* __restrict__ rel_ptr, const int* __restrict__ rel_idx,
                                                              int* __restrict__ ranks, int* __restrict__ first_rank,
                                                              double* __restrict__ ap, int* __restrict__ status) {
  __shared__ unsigned long long key[RETR_MAX_REL];
  __shared__ unsigned short pay[RETR_MAX_REL];
  __shared__ int ahead[RETR_MAX_REL];            // ahead[p]: images whose key lies between the sorted relevant keys p - 1 and p
  __shared__ int wave_tot[16];
  __shared__ double wave_ap[16];
  __shared__ int bad_s;
  const int T = blockDim.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t q = blockIdx.x;
  const float* x = scores + q * (size_t)lds;
  const long long p0 = rel_ptr[q], p1 = rel_ptr[q + 1];
  const long long R64 = p1 - p0;
  if (R64 <= 0 || R64 > RETR_MAX_REL || p0 < 0) {          // (uniform over the workgroup)
    if (tid == 0) {
      status[q] = R64 == 0 ? -3 : -4;
      first_rank[q] = 0;
      ap[q] = __longlong_as_double(0x7ff8000000000000ll);
    }
    return;
  }
  const int R = (int)R64;
  const int P = sgg_sort_geometry(R, 64).P;
  if (tid == 0) bad_s = 0;
  __syncthreads();
  for (int i = tid; i < P; i += T) {
    unsigned long long k = SGG_SORT_PAD;
    if (i < R) {
      const int image = rel_idx[p0 + i];
      if (image >= 0 && image < n) k = sgg_value_key(x[image], image);
      else bad_s = 1;
    }
    key[i] = k;
    pay[i] = (unsigned short)i;
    ahead[i] = 0;
  }
  sgg_bitonic_pairs(key, pay, P);
  if (bad_s) {                                   // an index outside [0, n_images): nothing of the query is reported
    if (tid == 0) {
      status[q] = -4;
      first_rank[q] = 0;
      ap[q] = __longlong_as_double(0x7ff8000000000000ll);
    }
    return;
  }
  // image t precedes every relevant key above its own: count it at the first such position
  for (int t = tid; t < n; t += T) {
    const int lo = sgg_upper_bound(key, 0, R, sgg_value_key(x[t], t));
    if (lo < R) atomicAdd(&ahead[lo], 1);
  }
  __syncthreads();
  // inclusive prefix sum over ahead[0 .. P): thread `tid` owns the C consecutive entries from tid * C
  const int C = (P + T - 1) / T;                 // <= 4
  int loc[4], run = 0;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int i = tid * C + c;
    loc[c] = (c < C && i < P) ? ahead[i] : 0;
    run += loc[c];
  }
  int before = sgg_block_scan(run, wave_tot);
  // rank of the i-th sorted relevant image = 1 + images ahead of it; AP = mean_i (i + 1) / rank_i, fp64, fixed order
  double part = 0.0;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int i = tid * C + c;
    before += loc[c];
    if (c < C && i < R) {
      const int rank = 1 + before;
      ranks[p0 + pay[i]] = rank;
      if (i == 0) first_rank[q] = rank;
      part += (double)(i + 1) / (double)rank;
    }
  }
  part = wave_sum(part);
  if (lane == 0) wave_ap[wave] = part;
  __syncthreads();
  if (tid == 0) {
    double sum = 0.0;
    for (int w = 0; w < (T >> 6); ++w) sum += wave_ap[w];
    ap[q] = sum / (double)R;
    status[q] = 0;
  }
}

extern "C" int sgg_query_logp(const float* logits, long long ld, const float* lse, int N, int nb, int V, const int* tok, int U, int u0,
                              int u1, int u2, const int* qidx, int Q, float* scores, long long lds, long long col0, void* stream) {
  SGG_CHECK_ARG(N >= 1 && N <= RETR_MAX_N && Q >= 1 && Q <= RETR_MAX_Q, "sgg_query_logp: 1 <= N <= 4096 and 1 <= Q <= 4096 (got N = %d, Q = %d)",
                N, Q);
  SGG_CHECK_ARG(nb >= 1 && nb <= 65535 && V >= 1 && V <= SGG_SORT_MAX_V, "sgg_query_logp: 1 <= nb <= 65535 and 1 <= V <= 2^21 (got nb = %d, V = %d)",
                nb, V);
  SGG_CHECK_ARG(U >= 1 && U <= Q, "sgg_query_logp: 1 <= U <= Q token-list entries per slot (got U = %d, Q = %d)", U, Q);
  SGG_CHECK_ARG(u0 >= 0 && u0 <= U && u1 >= 0 && u1 <= U && u2 >= 0 && u2 <= U,
                "sgg_query_logp: 0 <= ucount <= U (got %d, %d, %d with U = %d)", u0, u1, u2, U);
  SGG_CHECK_ARG(ld >= 3LL * V, "sgg_query_logp: row stride ld >= 3 V (got ld = %lld, V = %d)", ld, V);
  SGG_CHECK_ARG(col0 >= 0 && lds >= col0 + nb, "sgg_query_logp: 0 <= col0 and col0 + nb <= lds (got col0 = %lld, nb = %d, lds = %lld)", col0,
                nb, lds);
  SGG_CHECK_ARG(logits && lse && tok && qidx && scores, "sgg_query_logp: null pointer");
  const int W = u0 + u1 + u2;                    // <= 12288 = RETR_LDS_FLOATS
  int T = ((Q < RETR_T ? Q : RETR_T) + 63) / 64 * 64;        // one query per thread in tiles of T; at least four waves gather
  T = T < 256 ? 256 : T;
  // samples per round: what the threads' gather slots and the LDS hold.  W <= 3 U <= 3 Q, so W <= 3 T below a full tile and
  // W <= 12288 = RETR_SLOTS * RETR_T at one: a sample always fits
  const int cap = RETR_SLOTS * T < RETR_LDS_FLOATS ? RETR_SLOTS * T : RETR_LDS_FLOATS;
  int S = W > 0 ? cap / W : RETR_MAX_ROUND;
  S = S > RETR_MAX_ROUND ? RETR_MAX_ROUND : S;
  S = S > N ? N : S;
  const size_t bytes = (size_t)(S * W + 3 * S) * sizeof(float);
  hipLaunchKernelGGL(query_logp_kernel, dim3(nb, sgg_cdiv(Q, T)), dim3(T), bytes, (hipStream_t)stream, logits, ld, lse, N, nb, V, tok, U, u0,
                     u1, u2, qidx, Q, S, scores, lds, col0);
  SGG_LAUNCH_CHECK("sgg_query_logp");
  return SGG_OK;
}

extern "C" int sgg_retrieve_topk(const float* scores, long long lds, int Q, int n_images, int K, int* idx, float* top, void* stream) {
  SGG_CHECK_ARG(Q >= 1 && n_images >= 1 && n_images <= RETR_MAX_IMAGES, "sgg_retrieve_topk: Q >= 1 and 1 <= n_images <= 2^21 (got Q = %d, n_images = %d)",
                Q, n_images);
  SGG_CHECK_ARG(K >= 1 && K <= RETR_MAX_K, "sgg_retrieve_topk: 1 <= K <= %d (got K = %d)", RETR_MAX_K, K);
  SGG_CHECK_ARG(lds >= n_images, "sgg_retrieve_topk: row stride lds >= n_images (got lds = %lld, n_images = %d)", lds, n_images);
  SGG_CHECK_ARG(scores && idx && top, "sgg_retrieve_topk: null pointer");
  const int M = K < n_images ? K : n_images;
  const int T = n_images >= 1024 ? 1024 : 256;   // threads for the passes over the row, not for the sort of the M survivors
  hipLaunchKernelGGL(retrieve_topk_kernel, dim3(Q), dim3(T), 0, (hipStream_t)stream, scores, lds, n_images, K, M,
                     sgg_sort_geometry(M, 64).P, idx, top);
  SGG_LAUNCH_CHECK("sgg_retrieve_topk");
  return SGG_OK;
}

extern "C" int sgg_retrieve_ranks(const float* scores, long long lds, int Q, int n_images, const int* rel_ptr, const int* rel_idx,
                                  int* ranks, int* first_rank, double* ap, int* status, void* stream) {
  SGG_CHECK_ARG(Q >= 1 && n_images >= 1 && n_images <= RETR_MAX_IMAGES, "sgg_retrieve_ranks: Q >= 1 and 1 <= n_images <= 2^21 (got Q = %d, n_images = %d)",
                Q, n_images);
  SGG_CHECK_ARG(lds >= n_images, "sgg_retrieve_ranks: row stride lds >= n_images (got lds = %lld, n_images = %d)", lds, n_images);
  SGG_CHECK_ARG(scores && rel_ptr && rel_idx && ranks && first_rank && ap && status, "sgg_retrieve_ranks: null pointer");      // (an empty CSR list still has one allocated entry)
  hipLaunchKernelGGL(retrieve_ranks_kernel, dim3(Q), dim3(1024), 0, (hipStream_t)stream, scores, lds, n_images, rel_ptr, rel_idx, ranks,
                     first_rank, ap, status);
  SGG_LAUNCH_CHECK("sgg_retrieve_ranks");
  return SGG_OK;
}
