// Guarded optimiser updates: global-norm clipping and the non-finite skip, decided on the device (gfx950).  Plain HIP C++, 16-byte
// loads, wave shuffles for the fp64 sums, no atomics, no LDS beyond the cross-wave hand-over.
//   grad_guard_chunk_kernel   workgroups walk the flat gradient range grid-stride in chunks of sgg_arena_stats_chunk() elements.  Per
//                             element x = g * grad_scale (fp32, as adam_kernel forms it): a finite x adds (double)x * (double)x to the
//                             chunk's sum of squares, a non-finite one is only counted (sgg_finite, as csrc/stats.hip tests it).
//                             Each chunk's row (ss, count) goes to the workspace with plain stores.
//   grad_guard_final_kernel   ONE workgroup: thread t sums rows t, t + 256, ... in that order, a fixed shuffle tree, the four waves in
//                             order; thread 0 then forms the record of eight doubles (include/sgg_hip.h) and read-modify-writes its
//                             two cumulative counters.
//                             A chunk's row depends on its elements only, the record on the rows in a fixed order: bit-identical from
//                             call to call and for every grid.
// The record's readers are adam_guarded_kernel and adam_ema_guarded_kernel (csrc/optim.hip): (float)record[4] is their gradient
// scale, record[5] == 0 drops the update.
// coef is EXACTLY 1 while the norm does not exceed the threshold (TF's clip_norm * min(1 / norm, 1 / clip_norm) is within an ulp of
// it): a run whose threshold is never reached is bit-identical to an unguarded one.
#include "sgg_common.h"

#define SGG_GUARD_THREADS 256
#define SGG_GUARD_NROW 2           // per-chunk row: sum of squares of the finite elements, non-finite count
#define SGG_GUARD_NREC 8           // the record (include/sgg_hip.h)

extern "C" int sgg_arena_stats_chunk(void);

// the four waves' (ss, count) summed in wave order by thread 0; every thread must call it (barriers)
__device__ __forceinline__ void guard_block_sum(double& ss, double& bad, double (*red)[SGG_GUARD_NROW]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  ss = wave_sum(ss);
  bad = wave_sum(bad);
  __syncthreads();                                    // (the previous round's reader of `red` is done)
  if (lane == 0) {
    red[wave][0] = ss;
    red[wave][1] = bad;
  }
  __syncthreads();
  if (tid == 0) {
    ss = red[0][0];
    bad = red[0][1];
#pragma unroll
    for (int w = 1; w < SGG_GUARD_THREADS / 64; ++w) {
      ss += red[w][0];
      bad += red[w][1];
    }
  }
}

__global__ __launch_bounds__(SGG_GUARD_THREADS) void grad_guard_chunk_kernel(const float* __restrict__ g, long long n, int chunk,
                                                                             long long n_chunks, float gscale,
                                                                             double* __restrict__ ws) {
  __shared__ double red[SGG_GUARD_THREADS / 64][SGG_GUARD_NROW];
  const int tid = threadIdx.x;
  for (long long c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const long long first = c * chunk;
    const int count = (int)min((long long)chunk, n - first);
    double ss = 0.0, bad = 0.0;
    const int n4 = (count + 3) >> 2;
    for (int i = tid; i < n4; i += SGG_GUARD_THREADS) {
      const long long e = first + 4ll * i;            // (chunk % 4 == 0 and g is 16-byte aligned: so is g + e)
      const int live = min(4, count - 4 * i);
      f32x4 gv = {0.f, 0.f, 0.f, 0.f};
      if (live == 4) {
        gv = *reinterpret_cast<const f32x4*>(g + e);
      } else {                                        // the last 1 .. 3 elements of the range: nothing behind g[n - 1] is read
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          if (q < live) gv[q] = g[e + q];
        }
      }
      gv = gv * gscale;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (q < live) {
          const float x = gv[q];
          if (sgg_finite(x)) ss += (double)x * (double)x; else bad += 1.0;
        }
      }
    }
    guard_block_sum(ss, bad, red);
    if (tid == 0) {
      ws[(size_t)c * SGG_GUARD_NROW + 0] = ss;
      ws[(size_t)c * SGG_GUARD_NROW + 1] = bad;
    }
  }
}

__global__ __launch_bounds__(SGG_GUARD_THREADS) void grad_guard_final_kernel(const double* __restrict__ ws, long long n_chunks,
                                                                             float gscale, float max_norm, int skip_nonfinite,
                                                                             double* __restrict__ rec) {
  __shared__ double red[SGG_GUARD_THREADS / 64][SGG_GUARD_NROW];
  const int tid = threadIdx.x;
  double ss = 0.0, bad = 0.0;
  for (long long c = tid; c < n_chunks; c += SGG_GUARD_THREADS) {
    ss += ws[(size_t)c * SGG_GUARD_NROW + 0];
    bad += ws[(size_t)c * SGG_GUARD_NROW + 1];
  }
  guard_block_sum(ss, bad, red);
  if (tid == 0) {
    const double norm = sqrt(ss);
    const double coef = (max_norm > 0.f && norm > (double)max_norm) ? (double)max_norm / norm : 1.0;
    const double s_eff = (double)(float)((double)gscale * coef);
    const double apply = (skip_nonfinite && bad > 0.0) ? 0.0 : 1.0;
    rec[0] = ss;
    rec[1] = bad;
    rec[2] = norm;
    rec[3] = coef;
    rec[4] = s_eff;
    rec[5] = apply;
    if (coef < 1.0 && apply != 0.0) rec[6] = rec[6] + 1.0;       // updates clipped so far
    if (apply == 0.0) rec[7] = rec[7] + 1.0;                    // updates skipped so far
  }
}

// ---- C ABI ------------------------------------------------------------------------------------------
static inline long long guard_chunks(long long n) {
  const long long chunk = sgg_arena_stats_chunk();
  return n > 0 ? (n + chunk - 1) / chunk : 0;
}

extern "C" size_t sgg_grad_guard_workspace_bytes(long long n) {
  return (size_t)guard_chunks(n) * SGG_GUARD_NROW * sizeof(double);
}

extern "C" int sgg_grad_guard(const float* grads, long long n, float grad_scale, float max_norm, int skip_nonfinite, int grid,
                              void* workspace, size_t workspace_bytes, double* record, void* stream) {
  SGG_CHECK_ARG(grads && workspace && record, "sgg_grad_guard: null pointer");
  SGG_CHECK_ARG(n > 0, "sgg_grad_guard: n must be positive (got %lld)", n);
  SGG_CHECK_ARG(((uintptr_t)grads & 15) == 0, "sgg_grad_guard: grads must be 16-byte aligned");
  SGG_CHECK_ARG((((uintptr_t)workspace | (uintptr_t)record) & 7) == 0, "sgg_grad_guard: workspace and record must be 8-byte aligned");
  SGG_CHECK_ARG(std::isfinite(max_norm) && max_norm >= 0.f, "sgg_grad_guard: max_norm %g must be finite and >= 0 (0 = no clipping)",
                (double)max_norm);
  SGG_CHECK_ARG(std::isfinite(grad_scale), "sgg_grad_guard: grad_scale %g must be finite", (double)grad_scale);
  SGG_CHECK_ARG(grid >= 0 && grid <= 65535, "sgg_grad_guard: 0 <= grid <= 65535 (0 = default; got %d)", grid);
  const int chunk = sgg_arena_stats_chunk();
  const long long n_chunks = guard_chunks(n);
  SGG_CHECK_ARG(chunk > 0 && chunk % 4 == 0 && n_chunks <= 0x7fffffffll, "sgg_grad_guard: n %lld is too long", n);
  if (workspace_bytes < sgg_grad_guard_workspace_bytes(n)) {
    sgg_set_error("sgg_grad_guard: workspace of %zu bytes, need %zu", workspace_bytes, sgg_grad_guard_workspace_bytes(n));
    return SGG_ERR_WORKSPACE;
  }
  const int blocks = grid > 0 ? grid : (int)(n_chunks < 4096 ? n_chunks : 4096);
  hipLaunchKernelGGL(grad_guard_chunk_kernel, dim3(blocks), dim3(SGG_GUARD_THREADS), 0, (hipStream_t)stream, grads, n, chunk, n_chunks,
                     grad_scale, (double*)workspace);
  SGG_LAUNCH_CHECK("sgg_grad_guard (chunks)");
  hipLaunchKernelGGL(grad_guard_final_kernel, dim3(1), dim3(SGG_GUARD_THREADS), 0, (hipStream_t)stream, (const double*)workspace,
                     n_chunks, grad_scale, max_norm, skip_nonfinite, record);
  SGG_LAUNCH_CHECK("sgg_grad_guard (record)");
  return SGG_OK;
}
