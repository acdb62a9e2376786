// Scene-graph metrics: where in an image's ranked list of DISTINCT predicted triples (csrc/rank.hip) each of its ground-truth
// triples stands (gfx950).
//   match_triples   one workgroup per image, the ground truth in LDS:
//                     1. every ground-truth row m becomes (packed triple, m); padding rows and rows with a token outside [0, V)
//                        get their codes (-3, -4) at once and the pad key, which sorts behind every valid row;
//                     2. bitonic sort of (packed triple, m): equal triples become one run whose head is the smallest row; the
//                        other rows of a run are duplicates (-2), and the heads are the distinct valid triples (n_gt);
//                     3. every prediction slot u < min(n_distinct, K) binary-searches the sorted keys and writes u into pos of
//                        the head of the run it finds.  The list is distinct, so at most one slot writes a row.
// Integers only: two launches give the same bits.  Not on the training path.
#include "sort_select.h"

#define MATCH_ABSENT (-1)
#define MATCH_DUPLICATE (-2)
#define MATCH_PADDING (-3)
#define MATCH_INVALID (-4)

// LDS: key[P] (8 B), pay[P] (2 B) = 10 * P bytes (40 KB at P = 4096)
__global__ __launch_bounds__(1024) void match_triples_kernel(const long long* __restrict__ ranked, const int* __restrict__ n_distinct,
                                                             int K, const long long* __restrict__ gt, const int* __restrict__ gt_count,
                                                             int M, int V, int P, int* __restrict__ pos, int* __restrict__ n_gt) {
  extern __shared__ unsigned long long match_lds[];
  __shared__ int heads;
  unsigned long long* key = match_lds;
  unsigned short* pay = reinterpret_cast<unsigned short*>(key + P);
  const int j = blockIdx.x, T = blockDim.x, tid = threadIdx.x;
  const int count = min(max(gt_count[j], 0), M);       // (a count outside [0, M] must not take the kernel out of its rows)
  const int U = min(max(n_distinct[j], 0), K);
  const long long* g = gt + (size_t)j * M * 3;
  int* pj = pos + (size_t)j * M;

  // 1. (packed triple, row); every row of pos gets a value here, and only valid rows are written again
  if (tid == 0) heads = 0;
  for (int m = tid; m < P; m += T) {
    unsigned long long c = SGG_SORT_PAD;
    if (m < M) {
      int code = MATCH_PADDING;
      if (m < count) {
        const bool ok = sgg_in_vocab3(g + (size_t)m * 3, V);
        code = ok ? MATCH_ABSENT : MATCH_INVALID;
        if (ok) c = sgg_pack_triple(g[(size_t)m * 3], g[(size_t)m * 3 + 1], g[(size_t)m * 3 + 2]);
      }
      pj[m] = code;
    }
    key[m] = c;
    pay[m] = (unsigned short)m;
  }
  // 2. runs of equal triples: the head of a run is its smallest row (the sort compares (key, row))
  sgg_bitonic_pairs(key, pay, P);
  int mine = 0;
  for (int q = tid; q < P; q += T) {
    const unsigned long long c = key[q];
    if (c == SGG_SORT_PAD) continue;
    if (q > 0 && key[q - 1] == c) pj[pay[q]] = MATCH_DUPLICATE;
    else ++mine;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
  if ((tid & 63) == 0 && mine) atomicAdd(&heads, mine);
  // 3. the predictions look themselves up (rows written here are run heads: disjoint from the duplicates above, and their
  //    first value was stored before the barriers of the sort)
  const long long* rj = ranked + (size_t)j * K * 3;
  for (int u = tid; u < U; u += T) {
    const long long* t = rj + (size_t)u * 3;
    if (!sgg_in_vocab3(t, V)) continue;
    const unsigned long long c = sgg_pack_triple(t[0], t[1], t[2]);
    const int lo = sgg_lower_bound(key, 0, P, c);
    if (lo < P && key[lo] == c) pj[pay[lo]] = u;
  }
  __syncthreads();
  if (tid == 0) n_gt[j] = heads;
}

extern "C" int sgg_match_triples(const long long* ranked, const int* n_distinct, int nb, int K, const long long* gt,
                                 const int* gt_count, int M, int V, int* pos, int* n_gt, void* stream) {
  SGG_CHECK_ARG(K >= 1 && K <= SGG_SORT_MAX_P, "sgg_match_triples: 1 <= K <= %d list slots per image (got %d)", SGG_SORT_MAX_P, K);
  SGG_CHECK_ARG(M >= 1 && M <= SGG_SORT_MAX_P, "sgg_match_triples: 1 <= M <= %d ground-truth rows per image (got %d)",
                SGG_SORT_MAX_P, M);
  SGG_CHECK_ARG(nb >= 1 && V >= 1 && V <= SGG_SORT_MAX_V, "sgg_match_triples: nb >= 1 and 1 <= V <= 2^21 (got nb = %d, V = %d)", nb, V);
  SGG_CHECK_ARG(ranked && n_distinct && gt && gt_count && pos && n_gt, "sgg_match_triples: null pointer");
  const sgg_sort_geometry g(M, 128);
  hipLaunchKernelGGL(match_triples_kernel, dim3(nb), dim3(g.T), (size_t)g.P * 10, (hipStream_t)stream, ranked, n_distinct, K, gt, gt_count,
                     M, V, g.P, pos, n_gt);
  SGG_LAUNCH_CHECK("sgg_match_triples");
  return SGG_OK;
}
