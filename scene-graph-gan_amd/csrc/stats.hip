// Training diagnostics: per-tensor statistics of a network's four arenas in one streaming pass (gfx950).
//   arena_stats_chunk_kernel   workgroups walk a host-built chunk table grid-stride; a chunk is at most SGG_STATS_CHUNK elements of
//                              ONE tensor.  Per element (16-byte loads of params, grads, m, v; the tail of a chunk masked):
//                                g = grads * grad_scale                  (fp32, as adam_kernel forms it)
//                                u = lr_t * m / (sqrtf(v) + eps)         (fp32, as adam_kernel forms it: the step's applied delta)
//                              and of g, the parameter and u: sum of squares (squares formed and summed in fp64), max |.| and the
//                              count of non-finite elements; sums and maxima run over the FINITE elements only.  Each chunk's row
//                              of SGG_STATS_NSTAT doubles goes to the workspace with plain stores.
//   arena_stats_tensor_kernel  one wave per tensor: finds the tensor's chunk rows (the table is sorted by tensor), lane l sums rows
//                              l, l + 64, ... in that order, then a fixed shuffle tree.
// No atomics: a chunk's row depends on its elements and the block size only, a tensor's row on its chunk rows in a fixed order - the
// output is bit-identical from call to call and for every grid size.  Not on the training path (read-only on all four arenas).
//   vector_stats_kernel        min, max, sum, count above a threshold (finite elements) and the non-finite count of a short vector,
//                              one workgroup, fp64.
#include "sgg_common.h"

#define SGG_STATS_CHUNK 16384      // elements per chunk: a multiple of 4 (chunks start 16-byte aligned), 16 float4 per thread and arena
#define SGG_STATS_NSTAT 9          // (sum of squares, max |.|, non-finite count) of g, of the parameter, of u
#define SGG_STATS_THREADS 256
#define SGG_VSTATS_N 5             // min, max, sum, count above the threshold, non-finite count

struct StatAcc {
  double ss;
  float mx;
  int bad;
  __device__ __forceinline__ void add(float x) {
    if (sgg_finite(x)) {
      ss += (double)x * (double)x;
      mx = fmaxf(mx, fabsf(x));
    } else {
      ++bad;
    }
  }
};

// table: n_chunks x (tensor, first arena element, count) as int64
__global__ __launch_bounds__(SGG_STATS_THREADS) void arena_stats_chunk_kernel(
    const float* __restrict__ p, const float* __restrict__ g, const float* __restrict__ m, const float* __restrict__ v,
    const long long* __restrict__ table, int n_chunks, float lr_t, float eps, float gscale, double* __restrict__ ws) {
  __shared__ double red[SGG_STATS_THREADS / 64][SGG_STATS_NSTAT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const long long first = table[(size_t)c * 3 + 1];
    const int count = (int)min(max(table[(size_t)c * 3 + 2], 0ll), (long long)SGG_STATS_CHUNK);   // (never past the chunk the host sized)
    StatAcc ag = {0.0, 0.f, 0}, ap = {0.0, 0.f, 0}, au = {0.0, 0.f, 0};
    const int n4 = (count + 3) >> 2;
    for (int i = tid; i < n4; i += SGG_STATS_THREADS) {
      const long long e = first + 4ll * i;
      const f32x4 gv = *reinterpret_cast<const f32x4*>(g + e) * gscale;
      const f32x4 pv = *reinterpret_cast<const f32x4*>(p + e);
      const f32x4 mv = *reinterpret_cast<const f32x4*>(m + e);
      const f32x4 vv = *reinterpret_cast<const f32x4*>(v + e);
      const int live = min(4, count - 4 * i);        // the last float4 of a tensor may hold padding: never read into a statistic
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (q < live) {
          ag.add(gv[q]);
          ap.add(pv[q]);
          au.add(lr_t * mv[q] / (sqrtf(vv[q]) + eps));
        }
      }
    }
    double row[SGG_STATS_NSTAT] = {ag.ss, (double)ag.mx, (double)ag.bad, ap.ss, (double)ap.mx, (double)ap.bad,
                                   au.ss, (double)au.mx, (double)au.bad};
#pragma unroll
    for (int s = 0; s < SGG_STATS_NSTAT; ++s) row[s] = (s % 3 == 1) ? wave_max(row[s]) : wave_sum(row[s]);
    __syncthreads();                                  // (the previous chunk's readers of `red` are done)
    if (lane == 0) {
#pragma unroll
      for (int s = 0; s < SGG_STATS_NSTAT; ++s) red[wave][s] = row[s];
    }
    __syncthreads();
    if (tid < SGG_STATS_NSTAT) {
      double r = red[0][tid];
#pragma unroll
      for (int w = 1; w < SGG_STATS_THREADS / 64; ++w) r = (tid % 3 == 1) ? fmax(r, red[w][tid]) : r + red[w][tid];
      ws[(size_t)c * SGG_STATS_NSTAT + tid] = r;
    }
  }
}

// first chunk whose tensor column is >= t (the table is sorted by tensor)
__device__ __forceinline__ int stats_lower_bound(const long long* __restrict__ table, int n_chunks, long long t) {
  int lo = 0, hi = n_chunks;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (table[(size_t)mid * 3] < t) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(64) void arena_stats_tensor_kernel(const long long* __restrict__ table, int n_chunks,
                                                                const double* __restrict__ ws, int n_tensors,
                                                                double* __restrict__ out) {
  const int t = blockIdx.x, lane = threadIdx.x;
  if (t >= n_tensors) return;
  const int c0 = stats_lower_bound(table, n_chunks, t), c1 = stats_lower_bound(table, n_chunks, (long long)t + 1);
  double row[SGG_STATS_NSTAT];
#pragma unroll
  for (int s = 0; s < SGG_STATS_NSTAT; ++s) row[s] = 0.0;
  for (int c = c0 + lane; c < c1; c += 64) {
#pragma unroll
    for (int s = 0; s < SGG_STATS_NSTAT; ++s) {
      const double x = ws[(size_t)c * SGG_STATS_NSTAT + s];
      row[s] = (s % 3 == 1) ? fmax(row[s], x) : row[s] + x;
    }
  }
#pragma unroll
  for (int s = 0; s < SGG_STATS_NSTAT; ++s) row[s] = (s % 3 == 1) ? wave_max(row[s]) : wave_sum(row[s]);
  if (lane == 0) {
#pragma unroll
    for (int s = 0; s < SGG_STATS_NSTAT; ++s) out[(size_t)t * SGG_STATS_NSTAT + s] = row[s];
  }
}

__global__ __launch_bounds__(SGG_STATS_THREADS) void vector_stats_kernel(const float* __restrict__ x, int n, float threshold,
                                                                         double* __restrict__ out) {
  __shared__ double red[SGG_STATS_THREADS / 64][SGG_VSTATS_N];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double mn = INFINITY, mx = -INFINITY, sum = 0.0, above = 0.0, bad = 0.0;
  for (int i = tid; i < n; i += SGG_STATS_THREADS) {
    const float a = x[i];
    if (sgg_finite(a)) {
      mn = fmin(mn, (double)a);
      mx = fmax(mx, (double)a);
      sum += (double)a;
      if (a > threshold) above += 1.0;
    } else {
      bad += 1.0;
    }
  }
  mn = wave_min(mn);
  mx = wave_max(mx);
  sum = wave_sum(sum);
  above = wave_sum(above);
  bad = wave_sum(bad);
  if (lane == 0) {
    red[wave][0] = mn; red[wave][1] = mx; red[wave][2] = sum; red[wave][3] = above; red[wave][4] = bad;
  }
  __syncthreads();
  if (tid < SGG_VSTATS_N) {
    double r = red[0][tid];
#pragma unroll
    for (int w = 1; w < SGG_STATS_THREADS / 64; ++w)
      r = tid == 0 ? fmin(r, red[w][tid]) : (tid == 1 ? fmax(r, red[w][tid]) : r + red[w][tid]);
    out[tid] = r;
  }
}

extern "C" int sgg_arena_stats_chunk(void) { return SGG_STATS_CHUNK; }
extern "C" int sgg_arena_stats_nstat(void) { return SGG_STATS_NSTAT; }

extern "C" size_t sgg_arena_stats_workspace_bytes(int n_chunks) {
  return n_chunks > 0 ? (size_t)n_chunks * SGG_STATS_NSTAT * sizeof(double) : 0;
}

extern "C" int sgg_arena_stats(const float* params, const float* grads, const float* m, const float* v, const long long* chunk_table,
                               int n_chunks, int n_tensors, float lr_t, float eps, float grad_scale, int grid, void* workspace,
                               size_t workspace_bytes, double* out, void* stream) {
  SGG_CHECK_ARG(params && grads && m && v && chunk_table && workspace && out, "sgg_arena_stats: null pointer");
  SGG_CHECK_ARG(n_chunks >= 1 && n_tensors >= 1 && n_tensors <= n_chunks,
                "sgg_arena_stats: 1 <= n_tensors <= n_chunks (got n_tensors = %d, n_chunks = %d)", n_tensors, n_chunks);
  SGG_CHECK_ARG((((uintptr_t)params | (uintptr_t)grads | (uintptr_t)m | (uintptr_t)v) & 15) == 0,
                "sgg_arena_stats: arena pointers must be 16-byte aligned");
  SGG_CHECK_ARG((((uintptr_t)chunk_table | (uintptr_t)workspace | (uintptr_t)out) & 7) == 0,
                "sgg_arena_stats: chunk table, workspace and output must be 8-byte aligned");
  SGG_CHECK_ARG(grid >= 0 && grid <= 65535, "sgg_arena_stats: 0 <= grid <= 65535 (0 = default; got %d)", grid);
  if (workspace_bytes < sgg_arena_stats_workspace_bytes(n_chunks)) {
    sgg_set_error("sgg_arena_stats: workspace of %zu bytes, need %zu", workspace_bytes, sgg_arena_stats_workspace_bytes(n_chunks));
    return SGG_ERR_WORKSPACE;
  }
  const int blocks = grid > 0 ? grid : (n_chunks < 4096 ? n_chunks : 4096);
  hipLaunchKernelGGL(arena_stats_chunk_kernel, dim3(blocks), dim3(SGG_STATS_THREADS), 0, (hipStream_t)stream, params, grads, m, v,
                     chunk_table, n_chunks, lr_t, eps, grad_scale, (double*)workspace);
  SGG_LAUNCH_CHECK("sgg_arena_stats (chunks)");
  hipLaunchKernelGGL(arena_stats_tensor_kernel, dim3(n_tensors), dim3(64), 0, (hipStream_t)stream, chunk_table, n_chunks,
                     (const double*)workspace, n_tensors, out);
  SGG_LAUNCH_CHECK("sgg_arena_stats (tensors)");
  return SGG_OK;
}

extern "C" int sgg_vector_stats(const float* x, int n, float threshold, double* out, void* stream) {
  SGG_CHECK_ARG(x && out, "sgg_vector_stats: null pointer");
  SGG_CHECK_ARG(n >= 1 && n <= (1 << 20), "sgg_vector_stats: 1 <= n <= 2^20 (one workgroup; got %d)", n);
  SGG_CHECK_ARG(((uintptr_t)out & 7) == 0, "sgg_vector_stats: output must be 8-byte aligned");
  hipLaunchKernelGGL(vector_stats_kernel, dim3(1), dim3(SGG_STATS_THREADS), 0, (hipStream_t)stream, x, n, threshold, out);
  SGG_LAUNCH_CHECK("sgg_vector_stats");
  return SGG_OK;
}
