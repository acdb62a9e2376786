// Weight averaging of a network's parameter arena (gfx950): plain HIP C++, 16-byte loads and stores, grid-stride loops, no LDS.
//   adam_ema_kernel   the Adam step of adam_kernel (csrc/misc.hip), expression for expression, and in the same pass TF's shadow
//                     update of tf.train.ExponentialMovingAverage on the new parameter value the thread still holds in registers:
//                     e -= (e - p_new) * one_minus_decay.  Nine streams (7 of Adam + read and write of the average) instead of the
//                     ten a separate averaging pass behind adam_kernel moves.
//   swap_kernel       exchanges two ranges bit for bit (Network.averaged(): the average takes the place of the live parameters, so
//                     every view, descriptor and pre-split copy that points into the arena stays valid).
//   grad_accumulate_kernel   gradient accumulation over micro-batches (Network.end_micro_batch): acc = g (first) or acc = acc + g, one
//                     fp32 addition per element, no atomics - a pure function of the inputs for any grid.  Three streams (two when
//                     first) against the seven of adam_kernel.
#include "sgg_common.h"

__global__ void adam_ema_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                float* __restrict__ e, long long n, float lr_t, float b1, float b2, float eps, float gscale, float omd) {
  const long long n4 = n >> 2;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i] * gscale;
    f32x4 mv = reinterpret_cast<f32x4*>(m)[i], vv = reinterpret_cast<f32x4*>(v)[i], pv = reinterpret_cast<f32x4*>(p)[i];
    f32x4 ev = reinterpret_cast<f32x4*>(e)[i];
    mv = mv * b1 + gv * (1.f - b1);
    vv = vv * b2 + gv * gv * (1.f - b2);
#pragma unroll
    for (int q = 0; q < 4; ++q) pv[q] -= lr_t * mv[q] / (sqrtf(vv[q]) + eps);
#pragma unroll
    for (int q = 0; q < 4; ++q) ev[q] -= (ev[q] - pv[q]) * omd;
    reinterpret_cast<f32x4*>(m)[i] = mv;
    reinterpret_cast<f32x4*>(v)[i] = vv;
    reinterpret_cast<f32x4*>(p)[i] = pv;
    reinterpret_cast<f32x4*>(e)[i] = ev;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const long long i = (n4 << 2) + threadIdx.x;
    const float gv = g[i] * gscale;
    const float mv = m[i] * b1 + gv * (1.f - b1);
    const float vv = v[i] * b2 + gv * gv * (1.f - b2);
    m[i] = mv; v[i] = vv;
    float pv = p[i];
    pv -= lr_t * mv / (sqrtf(vv) + eps);
    p[i] = pv;
    const float ev = e[i];
    e[i] = ev - (ev - pv) * omd;
  }
}

// (values are only moved, never computed with: NaN payloads and the sign of zero survive)
__global__ void swap_kernel(float* __restrict__ a, float* __restrict__ b, long long n) {
  const long long n4 = n >> 2;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    const f32x4 av = reinterpret_cast<f32x4*>(a)[i], bv = reinterpret_cast<f32x4*>(b)[i];
    reinterpret_cast<f32x4*>(a)[i] = bv;
    reinterpret_cast<f32x4*>(b)[i] = av;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const long long i = (n4 << 2) + threadIdx.x;
    const float av = a[i], bv = b[i];
    a[i] = bv;
    b[i] = av;
  }
}

template <bool FIRST>
__global__ void grad_accumulate_kernel(float* __restrict__ acc, const float* __restrict__ g, long long n) {
  const long long n4 = n >> 2;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
    if (FIRST) {
      reinterpret_cast<f32x4*>(acc)[i] = gv;
    } else {
      const f32x4 av = reinterpret_cast<f32x4*>(acc)[i];
      reinterpret_cast<f32x4*>(acc)[i] = av + gv;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const long long i = (n4 << 2) + threadIdx.x;
    acc[i] = FIRST ? g[i] : acc[i] + g[i];
  }
}

// ---- C ABI ------------------------------------------------------------------------------------------
static inline int grid_for(long long n, int block) {
  long long g = (n + block - 1) / block;
  if (g > 4096) g = 4096;
  if (g < 1) g = 1;
  return (int)g;
}

// [a, a + n) and [b, b + n) floats share a byte
static inline bool ranges_overlap(const float* a, const float* b, long long n) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b, len = (uintptr_t)n * sizeof(float);
  return x < y + len && y < x + len;
}

extern "C" int sgg_adam_tf_multi_ema(float* params, const float* grads, float* m, float* v, float* ema, long long n, float lr_t,
                                     float beta1, float beta2, float eps, float grad_scale, float one_minus_decay, void* stream) {
  SGG_CHECK_ARG(params && grads && m && v && ema && n > 0, "sgg_adam_tf_multi_ema: bad argument");
  SGG_CHECK_ARG((((uintptr_t)params | (uintptr_t)grads | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema) & 15) == 0,
                "sgg_adam_tf_multi_ema: pointers must be 16-byte aligned");
  SGG_CHECK_ARG(!ranges_overlap(ema, params, n) && !ranges_overlap(ema, grads, n) && !ranges_overlap(ema, m, n) &&
                    !ranges_overlap(ema, v, n),
                "sgg_adam_tf_multi_ema: ema overlaps another operand");
  SGG_CHECK_ARG(one_minus_decay >= 0.f && one_minus_decay <= 1.f, "sgg_adam_tf_multi_ema: one_minus_decay %g is outside [0, 1]",
                (double)one_minus_decay);
  hipLaunchKernelGGL(adam_ema_kernel, dim3(grid_for(n / 4 + 1, 256)), dim3(256), 0, (hipStream_t)stream, params, grads, m, v, ema, n,
                     lr_t, beta1, beta2, eps, grad_scale, one_minus_decay);
  SGG_LAUNCH_CHECK("sgg_adam_tf_multi_ema");
  return SGG_OK;
}

extern "C" int sgg_swap_f32(float* a, float* b, long long n, void* stream) {
  SGG_CHECK_ARG(a && b && n > 0, "sgg_swap_f32: bad argument");
  SGG_CHECK_ARG((((uintptr_t)a | (uintptr_t)b) & 15) == 0, "sgg_swap_f32: pointers must be 16-byte aligned");
  SGG_CHECK_ARG(!ranges_overlap(a, b, n), "sgg_swap_f32: the ranges overlap");
  hipLaunchKernelGGL(swap_kernel, dim3(grid_for(n / 4 + 1, 256)), dim3(256), 0, (hipStream_t)stream, a, b, n);
  SGG_LAUNCH_CHECK("sgg_swap_f32");
  return SGG_OK;
}

extern "C" int sgg_grad_accumulate(float* acc, const float* g, long long n, int first, void* stream) {
  SGG_CHECK_ARG(acc && g && n > 0, "sgg_grad_accumulate: bad argument");
  SGG_CHECK_ARG((((uintptr_t)acc | (uintptr_t)g) & 15) == 0, "sgg_grad_accumulate: pointers must be 16-byte aligned");
  SGG_CHECK_ARG(!ranges_overlap(acc, g, n), "sgg_grad_accumulate: the ranges overlap");
  const dim3 grid(grid_for(n / 4 + 1, 256)), block(256);
  if (first)
    hipLaunchKernelGGL(grad_accumulate_kernel<true>, grid, block, 0, (hipStream_t)stream, acc, g, n);
  else
    hipLaunchKernelGGL(grad_accumulate_kernel<false>, grid, block, 0, (hipStream_t)stream, acc, g, n);
  SGG_LAUNCH_CHECK("sgg_grad_accumulate");
  return SGG_OK;
}
