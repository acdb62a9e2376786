// Grounded scene graphs: from an image's ranked distinct triples (csrc/rank.hip, csrc/kbest.hip) and the generator's attention
// rows of its N samples to entity INSTANCES (gfx950).  The definitions are those of sgg_amd/ground.py (ground_reference).
//   ground_assign    one workgroup per image: bitonic sort of (packed triple, slot); every sample binary-searches its packed
//                    triple (slot_of_sample); a second sort of (slot, sample) groups the samples (members, start).
//   ground_pool      one workgroup per (slot, image), lanes over the 3 * L cells of the slot's three maps: the mean of the member
//                    rows of alpha_t in member order, fp32, one division.  Every attention row is read once: an HBM stream.
//   ground_resolve   one 1024-thread workgroup per image: the 2U mentions sorted by (token, mention) in LDS; waves take the pairs
//                    inside a same-token group (min-sum over the cells, wave reduction); a pair at or above the threshold is united
//                    in an LDS parent array by compare-and-swap hooking of the larger root under the smaller, so that the final
//                    root is the component's smallest mention whatever the order in which the pairs were found; roots are
//                    prefix-counted into node ids; a sort of (root, mention) makes every node's mentions contiguous for the pass
//                    that accumulates node maps, boxes and centres.
// No float atomics anywhere: two launches give the same bits.  No host read-back between the three.  Not on the training path.
#include "sort_select.h"

#define GROUND_MAX_K 1024                       // resolve: 2 K mentions per image, compared pairwise within a token
#define GROUND_UNASSIGNED 0x7fffffffffffffffull // second sort of assign: behind every slot, in front of the padding

// LDS: key[P] (8 B), pay[P] (2 B) = 10 * P bytes (40 KB at P = 4096); P >= max(N, K), at most 4 samples per thread
__global__ __launch_bounds__(1024) void ground_assign_kernel(const long long* __restrict__ tokens, const long long* __restrict__ triples,
                                                             const int* __restrict__ n_distinct, int N, int nb, int K, int V, int P,
                                                             int* __restrict__ slot_of_sample, int* __restrict__ members,
                                                             int* __restrict__ start) {
  extern __shared__ unsigned long long ground_lds[];
  unsigned long long* key = ground_lds;
  unsigned short* pay = reinterpret_cast<unsigned short*>(key + P);
  const int j = blockIdx.x, T = blockDim.x, tid = threadIdx.x;
  const int U = min(max(n_distinct[j], 0), K);
  const long long* tj = triples + (size_t)j * K * 3;

  // 1. (packed triple, slot); a slot with a token outside [0, V) can equal no sample
  for (int u = tid; u < P; u += T) {
    unsigned long long c = SGG_SORT_PAD;
    if (u < U && sgg_in_vocab3(tj + (size_t)u * 3, V)) c = sgg_pack_triple(tj[(size_t)u * 3], tj[(size_t)u * 3 + 1], tj[(size_t)u * 3 + 2]);
    key[u] = c;
    pay[u] = (unsigned short)u;
  }
  sgg_bitonic_pairs(key, pay, P);
  // 2. every sample looks itself up (the first position of a run = its smallest slot)
  int slot[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int k = tid + e * T;
    slot[e] = -1;
    if (k < N) {
      const long long* t = tokens + ((size_t)k * nb + j) * 3;
      if (sgg_in_vocab3(t, V)) {
        const unsigned long long c = sgg_pack_triple(t[0], t[1], t[2]);
        const int lo = sgg_lower_bound(key, 0, P, c);
        if (lo < P && key[lo] == c) slot[e] = pay[lo];
      }
      slot_of_sample[(size_t)j * N + k] = slot[e];
    }
  }
  __syncthreads();
  // 3. (slot, sample): the samples of a slot become one run, ascending sample inside it
  for (int k = tid; k < P; k += T) key[k] = SGG_SORT_PAD;
  __syncthreads();
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int k = tid + e * T;
    if (k < N) key[k] = slot[e] >= 0 ? (unsigned long long)slot[e] : GROUND_UNASSIGNED;
  }
  for (int k = tid; k < P; k += T) pay[k] = (unsigned short)k;
  sgg_bitonic_pairs(key, pay, P);
  for (int q = tid; q < N; q += T) members[(size_t)j * N + q] = key[q] < (unsigned long long)K ? (int)pay[q] : -1;
  // first position whose slot is >= u (slots >= U have no sample: start[U])
  for (int u = tid; u <= K; u += T) start[(size_t)j * (K + 1) + u] = sgg_lower_bound(key, 0, N, (unsigned long long)u);
}

// grid (K, nb), 256 threads over the 3 * L cells of the slot
__global__ __launch_bounds__(256) void ground_pool_kernel(const float* __restrict__ a0, const float* __restrict__ a1,
                                                          const float* __restrict__ a2, long long lda, const int* __restrict__ members,
                                                          const int* __restrict__ start, const int* __restrict__ fallback_sample,
                                                          const int* __restrict__ n_distinct, int N, int nb, int K, int L,
                                                          float* __restrict__ maps, int* __restrict__ n_pooled) {
  const int u = blockIdx.x, j = blockIdx.y, tid = threadIdx.x;
  const int U = min(max(n_distinct[j], 0), K);
  float* out = maps + ((size_t)j * K + u) * 3 * L;
  int lo = 0, n = 0, fb = -1;
  if (u < U) {
    lo = min(max(start[(size_t)j * (K + 1) + u], 0), N);
    n = min(max(start[(size_t)j * (K + 1) + u + 1], lo), N) - lo;        // (device arrays are clamped, never trusted)
    if (n == 0) fb = fallback_sample[(size_t)j * K + u];
  }
  if (tid == 0) n_pooled[(size_t)j * K + u] = n;
  const int* mem = members + (size_t)j * N + lo;
  for (int e = tid; e < 3 * L; e += 256) {
    const int t = e / L, l = e - t * L;
    const float* a = (t == 0 ? a0 : (t == 1 ? a1 : a2)) + l;
    float acc = 0.f;
    if (n > 0) {
      int i = 0;
      for (; i + 4 <= n; i += 4) {                  // four rows in flight; added in member order
        const int k0 = min(max(mem[i], 0), N - 1), k1 = min(max(mem[i + 1], 0), N - 1);
        const int k2 = min(max(mem[i + 2], 0), N - 1), k3 = min(max(mem[i + 3], 0), N - 1);
        const float v0 = a[((size_t)k0 * nb + j) * lda], v1 = a[((size_t)k1 * nb + j) * lda];
        const float v2 = a[((size_t)k2 * nb + j) * lda], v3 = a[((size_t)k3 * nb + j) * lda];
        acc = (((acc + v0) + v1) + v2) + v3;
      }
      for (; i < n; ++i) {
        const int k = min(max(mem[i], 0), N - 1);
        acc += a[((size_t)k * nb + j) * lda];
      }
      acc = acc / (float)n;
    } else if (fb >= 0 && fb < N) {
      acc = a[((size_t)fb * nb + j) * lda];
    }
    out[e] = acc;
  }
}

__device__ __forceinline__ int ground_load(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// root of x in the parent array (parents only ever decrease, and every parent is a member of the same set)
__device__ __forceinline__ int ground_find(int* parent, int x) {
  int r = x, p = ground_load(parent + r);
  while (p != r) {
    r = p;
    p = ground_load(parent + r);
  }
  // path compression: r is an ancestor of every mention on the path (it may have ceased to be a root meanwhile: still one), and
  // only roots are hooked, so lowering the parent of a non-root to r keeps the sets as they are
  while (x > r) {
    p = ground_load(parent + x);
    if (p > r) atomicMin(parent + x, r);
    x = p;
  }
  return r;
}
// unite the sets of a and b: the larger root goes under the smaller (retry when another wave moved it first)
__device__ __forceinline__ void ground_unite(int* parent, int a, int b) {
  for (;;) {
    int ra = ground_find(parent, a), rb = ground_find(parent, b);
    if (ra == rb) return;
    if (ra > rb) { const int s = ra; ra = rb; rb = s; }
    if (atomicCAS(parent + rb, rb, ra) == rb) return;
  }
}
__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}

// LDS: key[P] (8 B), pay[P] (2 B), parent[P], node[P], head[P] (4 B each) = 22 * P bytes (44 KB at P = 2048); P >= 2 K
__global__ __launch_bounds__(1024) void ground_resolve_kernel(const float* __restrict__ maps, const long long* __restrict__ triples,
                                                              const int* __restrict__ n_distinct, const int* __restrict__ n_pooled,
                                                              int K, int Hf, int Wf, float overlap, float box_frac, int P,
                                                              int* __restrict__ mention_node, int* __restrict__ n_nodes,
                                                              long long* __restrict__ node_word, int* __restrict__ node_first,
                                                              int* __restrict__ node_weight, int* __restrict__ node_mentions,
                                                              float* __restrict__ node_map, int* __restrict__ node_box,
                                                              float* __restrict__ node_center) {
  extern __shared__ unsigned long long ground_lds[];
  __shared__ int wave_tot[16];
  unsigned long long* key = ground_lds;
  int* parent = reinterpret_cast<int*>(key + P);
  int* node = parent + P;                         // node id of a ROOT mention
  int* head = node + P;                           // sorted position of the first mention of node n
  unsigned short* pay = reinterpret_cast<unsigned short*>(head + P);
  const int j = blockIdx.x, T = blockDim.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, waves = T >> 6;
  const int L = Hf * Wf;
  const int U = min(max(n_distinct[j], 0), K), M = 2 * U;
  const long long* tj = triples + (size_t)j * K * 3;
  const float* mj = maps + (size_t)j * K * 3 * L;
  const int* wj = n_pooled + (size_t)j * K;
  // map of mention m = 2u + r: maps[j][u][2r]
#define GROUND_MAP(m) (mj + ((size_t)((m) >> 1) * 3 + (((m) & 1) << 1)) * L)
#define GROUND_TOKEN(m) (tj[(size_t)((m) >> 1) * 3 + (((m) & 1) << 1)])

  // 1. (token, mention): same-token groups become contiguous.  The padding sorts behind every mention (key and payload)
  for (int m = tid; m < P; m += T) {
    key[m] = m < M ? (unsigned long long)GROUND_TOKEN(m) : SGG_SORT_PAD;
    pay[m] = (unsigned short)m;
    parent[m] = m;
  }
  sgg_bitonic_pairs(key, pay, P);
  // 2. the pairs inside a group: wave w takes the positions q = w, w + waves, ... and pairs each with the rest of its group
  for (int q = wave; q < M; q += waves) {
    const unsigned long long c = key[q];
    const int m = pay[q];
    const float* a = GROUND_MAP(m);
    for (int q2 = q + 1; q2 < M && key[q2] == c; ++q2) {
      const int m2 = pay[q2];
      int same = 0;
      if (lane == 0) same = ground_find(parent, m) == ground_find(parent, m2);
      if (__shfl(same, 0, 64)) continue;          // already in one set: the pair can change nothing
      const float* b = GROUND_MAP(m2);
      float s = 0.f;
      for (int l = lane; l < L; l += 64) s += fminf(a[l], b[l]);
      s = wave_sum(s);
      if (lane == 0 && s >= overlap) ground_unite(parent, min(m, m2), max(m, m2));
    }
  }
  __syncthreads();
  // 3. roots -> node ids in mention order: exclusive prefix sum of (root == m), C consecutive mentions per thread
  const int C = P / T;                            // P >= 2 T or T == P / 2: C >= 2
  int mine = 0;
  for (int e = 0; e < C; ++e) {
    const int m = tid * C + e;
    mine += m < M && parent[m] == m;
  }
  int total, base = sgg_block_scan(mine, wave_tot, &total);
  for (int e = 0; e < C; ++e) {
    const int m = tid * C + e;
    if (m < M && parent[m] == m) node[m] = base++;
  }
  __syncthreads();
  // (root, mention): the mentions of a node become one run in ascending mention order
  for (int m = tid; m < P; m += T) {
    key[m] = m < M ? (unsigned long long)ground_find(parent, m) : SGG_SORT_PAD;
    pay[m] = (unsigned short)m;
  }
  sgg_bitonic_pairs(key, pay, P);
  for (int q = tid; q < M; q += T) {
    const int r = (int)key[q], n = node[r];
    mention_node[(size_t)j * K * 2 + pay[q]] = n;
    if (q == 0 || key[q - 1] != key[q]) head[n] = q;
  }
  for (int m = M + tid; m < 2 * K; m += T) mention_node[(size_t)j * K * 2 + m] = -1;
  if (tid == 0) n_nodes[j] = total;
  __syncthreads();
  // 4. one wave per node: weights, map (mentions in ascending order), box and centre
  const size_t nj = (size_t)j * 2 * K;
  for (int n = wave; n < total; n += waves) {
    const int q0 = head[n];
    const unsigned long long c = key[q0];
    int q1 = q0, wsum = 0;
    for (; q1 < M && key[q1] == c; ++q1) wsum += max(wj[pay[q1] >> 1], 1);
    float* out = node_map + (nj + n) * L;
    const float fw = (float)wsum;
    float mx = 0.f, sa = 0.f, sy = 0.f, sx = 0.f;
    for (int l = lane; l < L; l += 64) {
      float acc = 0.f;
      for (int q = q0; q < q1; ++q) {
        const int m = pay[q];
        acc += (float)max(wj[m >> 1], 1) * GROUND_MAP(m)[l];
      }
      const float v = acc / fw;
      out[l] = v;
      const int y = l / Wf, x = l - y * Wf;
      mx = fmaxf(mx, v);
      sa += v;
      sy += v * ((float)y + 0.5f);
      sx += v * ((float)x + 0.5f);
    }
    mx = wave_max(mx);
    sa = wave_sum(sa);
    sy = wave_sum(sy);
    sx = wave_sum(sx);
    const float thr = box_frac * mx;
    int y0 = Hf, x0 = Wf, y1 = -1, x1 = -1;
    for (int l = lane; l < L; l += 64) {
      if (out[l] >= thr) {                        // (this lane's own store)
        const int y = l / Wf, x = l - y * Wf;
        y0 = min(y0, y); x0 = min(x0, x); y1 = max(y1, y); x1 = max(x1, x);
      }
    }
    y0 = wave_min_i(y0); x0 = wave_min_i(x0); y1 = wave_max_i(y1); x1 = wave_max_i(x1);
    if (lane == 0) {
      const int m0 = pay[q0];
      node_word[nj + n] = GROUND_TOKEN(m0);
      node_first[nj + n] = m0;
      node_weight[nj + n] = wsum;
      node_mentions[nj + n] = q1 - q0;
      int* bx = node_box + (nj + n) * 4;
      bx[0] = y0; bx[1] = x0; bx[2] = y1; bx[3] = x1;
      node_center[(nj + n) * 2] = sy / sa;
      node_center[(nj + n) * 2 + 1] = sx / sa;
    }
  }
  // padding behind the nodes
  for (int n = total + tid; n < 2 * K; n += T) {
    node_word[nj + n] = -1;
    node_first[nj + n] = -1;
    node_weight[nj + n] = -1;
    node_mentions[nj + n] = -1;
    int* bx = node_box + (nj + n) * 4;
    bx[0] = -1; bx[1] = -1; bx[2] = -1; bx[3] = -1;
    node_center[(nj + n) * 2] = SGG_QNAN;
    node_center[(nj + n) * 2 + 1] = SGG_QNAN;
  }
  const size_t pad0 = (size_t)total * L, pad1 = (size_t)2 * K * L;
  for (size_t e = pad0 + tid; e < pad1; e += T) node_map[nj * L + e] = 0.f;
#undef GROUND_MAP
#undef GROUND_TOKEN
}

extern "C" int sgg_ground_assign(const long long* tokens, const long long* triples, const int* n_distinct, int N, int nb, int K, int V,
                                 int* slot_of_sample, int* members, int* start, void* stream) {
  SGG_CHECK_ARG(N >= 1 && N <= SGG_SORT_MAX_P, "sgg_ground_assign: 1 <= N <= %d samples per image (got %d)", SGG_SORT_MAX_P, N);
  SGG_CHECK_ARG(K >= 1 && K <= SGG_SORT_MAX_P, "sgg_ground_assign: 1 <= K <= %d list slots per image (got %d)", SGG_SORT_MAX_P, K);
  SGG_CHECK_ARG(nb >= 1 && V >= 1 && V <= SGG_SORT_MAX_V, "sgg_ground_assign: nb >= 1 and 1 <= V <= 2^21 (got nb = %d, V = %d)", nb, V);
  SGG_CHECK_ARG(tokens && triples && n_distinct && slot_of_sample && members && start, "sgg_ground_assign: null pointer");
  const sgg_sort_geometry g(N > K ? N : K, 128);  // at most 4 entries per thread
  hipLaunchKernelGGL(ground_assign_kernel, dim3(nb), dim3(g.T), (size_t)g.P * 10, (hipStream_t)stream, tokens, triples, n_distinct, N, nb,
                     K, V, g.P, slot_of_sample, members, start);
  SGG_LAUNCH_CHECK("sgg_ground_assign");
  return SGG_OK;
}

extern "C" int sgg_ground_pool(const float* alpha0, const float* alpha1, const float* alpha2, long long lda, const int* members,
                               const int* start, const int* fallback_sample, const int* n_distinct, int N, int nb, int K, int L,
                               float* maps, int* n_pooled, void* stream) {
  SGG_CHECK_ARG(N >= 1 && N <= SGG_SORT_MAX_P, "sgg_ground_pool: 1 <= N <= %d samples per image (got %d)", SGG_SORT_MAX_P, N);
  SGG_CHECK_ARG(K >= 1 && K <= SGG_SORT_MAX_P, "sgg_ground_pool: 1 <= K <= %d list slots per image (got %d)", SGG_SORT_MAX_P, K);
  SGG_CHECK_ARG(nb >= 1 && nb <= 65535, "sgg_ground_pool: 1 <= nb <= 65535 images (got %d)", nb);
  SGG_CHECK_ARG(L >= 1 && L <= (1 << 20) && lda >= L, "sgg_ground_pool: 1 <= L <= 2^20 cells and lda >= L (got L = %d, lda = %lld)", L, lda);
  SGG_CHECK_ARG(alpha0 && alpha1 && alpha2 && members && start && fallback_sample && n_distinct && maps && n_pooled,
                "sgg_ground_pool: null pointer");
  hipLaunchKernelGGL(ground_pool_kernel, dim3(K, nb), dim3(256), 0, (hipStream_t)stream, alpha0, alpha1, alpha2, lda, members, start,
                     fallback_sample, n_distinct, N, nb, K, L, maps, n_pooled);
  SGG_LAUNCH_CHECK("sgg_ground_pool");
  return SGG_OK;
}

extern "C" int sgg_ground_resolve(const float* maps, const long long* triples, const int* n_distinct, const int* n_pooled, int nb, int K,
                                  int Hf, int Wf, float overlap, float box_frac, int* mention_node, int* n_nodes, long long* node_word,
                                  int* node_first, int* node_weight, int* node_mentions, float* node_map, int* node_box,
                                  float* node_center, void* stream) {
  SGG_CHECK_ARG(K >= 1 && K <= GROUND_MAX_K, "sgg_ground_resolve: 1 <= K <= %d list slots per image (got %d): the 2 K mentions of an "
                "image are compared pairwise", GROUND_MAX_K, K);
  SGG_CHECK_ARG(nb >= 1 && Hf >= 1 && Wf >= 1 && (long long)Hf * Wf <= (1 << 20),
                "sgg_ground_resolve: nb >= 1 and 1 <= Hf * Wf <= 2^20 cells (got nb = %d, Hf = %d, Wf = %d)", nb, Hf, Wf);
  SGG_CHECK_ARG(overlap > 0.f && overlap <= 1.f, "sgg_ground_resolve: overlap must be in (0, 1] (got %g)", (double)overlap);
  SGG_CHECK_ARG(box_frac > 0.f && box_frac <= 1.f, "sgg_ground_resolve: box_frac must be in (0, 1] (got %g)", (double)box_frac);
  SGG_CHECK_ARG(maps && triples && n_distinct && n_pooled && mention_node && n_nodes && node_word && node_first && node_weight &&
                node_mentions && node_map && node_box && node_center, "sgg_ground_resolve: null pointer");
  const sgg_sort_geometry g(2 * K, 128);
  hipLaunchKernelGGL(ground_resolve_kernel, dim3(nb), dim3(g.T), (size_t)g.P * 22, (hipStream_t)stream, maps, triples, n_distinct, n_pooled,
                     K, Hf, Wf, overlap, box_frac, g.P, mention_node, n_nodes, node_word, node_first, node_weight, node_mentions,
                     node_map, node_box, node_center);
  SGG_LAUNCH_CHECK("sgg_ground_resolve");
  return SGG_OK;
}
