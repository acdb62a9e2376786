// The whole-arena passes of the optimiser step (gfx950): plain HIP C++, 16-byte loads and stores, grid-stride loops, no LDS, no
// atomics - each a pure function of its inputs for any grid.
//   adam_body<EMA, GUARDED>   tf.train.AdamOptimizer(1e-4, beta1=0.5, beta2=0.9), train.py:258-259 (Appendix A.8):
//                             theta -= lr_t * m / (sqrt(v) + eps), eps OUTSIDE the bias correction.  The ONE statement of the update
//                             (vector loop and scalar tail); the four kernels below are its instances:
//     adam_kernel               <false, false>  seven streams
//     adam_ema_kernel           <true, false>   and in the same pass TF's shadow update of tf.train.ExponentialMovingAverage on the new
//                                               parameter value the thread still holds in registers: e -= (e - p_new) * one_minus_decay.
//                                               Nine streams instead of the ten a separate averaging pass behind adam_kernel moves.
//     adam_guarded_kernel       <false, true>   the gradient scale read from the record of sgg_grad_guard ((float)record[4],
//     adam_ema_guarded_kernel   <true, true>    csrc/guard.hip) instead of a kernel argument; record[5] == 0 (the update is dropped):
//                                               the kernel returns before its first load, nothing is written.
//   swap_kernel               exchanges two ranges bit for bit (Network.averaged(): the average takes the place of the live parameters,
//                             so every view, descriptor and pre-split copy that points into the arena stays valid).
//   grad_accumulate_kernel    gradient accumulation over micro-batches (Network.end_micro_batch): acc = g (first) or acc = acc + g, one
//                             fp32 addition per element.  Three streams (two when first) against the seven of adam_kernel.
#include "sgg_common.h"

// i0 / stride: the thread's first float4 and the grid's stride, formed by the __global__ function.  (The compiler lowers a kernel's
// own blockDim.x read through the uniform-work-group-size rule before it inlines; the same read in here takes the general, longer
// form: DESIGN.md, "One Adam body".)  e, omd: unused unless EMA; gscale: unused if GUARDED; rec: unused unless GUARDED.
// -ffp-contract=fast: regrouping a product and a sum below can change which ones fuse, and with that the bits of every network.
template <bool EMA, bool GUARDED>
__device__ __forceinline__ void adam_body(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                          float* __restrict__ v, float* __restrict__ e, long long n, float lr_t, float b1, float b2,
                                          float eps, float gscale, const double* __restrict__ rec, float omd, long long i0,
                                          long long stride) {
  if (GUARDED) {
    if (rec[5] == 0.0) return;
    gscale = (float)rec[4];
  }
  const long long n4 = n >> 2;
  for (long long i = i0; i < n4; i += stride) {
    const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i] * gscale;
    f32x4 mv = reinterpret_cast<f32x4*>(m)[i], vv = reinterpret_cast<f32x4*>(v)[i], pv = reinterpret_cast<f32x4*>(p)[i];
    f32x4 ev;
    if (EMA) ev = reinterpret_cast<f32x4*>(e)[i];
    mv = mv * b1 + gv * (1.f - b1);
    vv = vv * b2 + gv * gv * (1.f - b2);
#pragma unroll
    for (int q = 0; q < 4; ++q) pv[q] -= lr_t * mv[q] / (sqrtf(vv[q]) + eps);
    if (EMA) {
#pragma unroll
      for (int q = 0; q < 4; ++q) ev[q] -= (ev[q] - pv[q]) * omd;
    }
    reinterpret_cast<f32x4*>(m)[i] = mv;
    reinterpret_cast<f32x4*>(v)[i] = vv;
    reinterpret_cast<f32x4*>(p)[i] = pv;
    if (EMA) reinterpret_cast<f32x4*>(e)[i] = ev;
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
    if (EMA) {
      const float ev = e[i];
      e[i] = ev - (ev - pv) * omd;
    }
  }
}

#define SGG_GRID_I0 ((long long)blockIdx.x * blockDim.x + threadIdx.x)
#define SGG_GRID_STRIDE ((long long)gridDim.x * blockDim.x)

__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                            long long n, float lr_t, float b1, float b2, float eps, float gscale) {
  adam_body<false, false>(p, g, m, v, nullptr, n, lr_t, b1, b2, eps, gscale, nullptr, 0.f, SGG_GRID_I0, SGG_GRID_STRIDE);
}

__global__ void adam_ema_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                float* __restrict__ e, long long n, float lr_t, float b1, float b2, float eps, float gscale, float omd) {
  adam_body<true, false>(p, g, m, v, e, n, lr_t, b1, b2, eps, gscale, nullptr, omd, SGG_GRID_I0, SGG_GRID_STRIDE);
}

__global__ void adam_guarded_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                    long long n, float lr_t, float b1, float b2, float eps, const double* __restrict__ rec) {
  adam_body<false, true>(p, g, m, v, nullptr, n, lr_t, b1, b2, eps, 0.f, rec, 0.f, SGG_GRID_I0, SGG_GRID_STRIDE);
}

__global__ void adam_ema_guarded_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                        float* __restrict__ v, float* __restrict__ e, long long n, float lr_t, float b1, float b2,
                                        float eps, const double* __restrict__ rec, float omd) {
  adam_body<true, true>(p, g, m, v, e, n, lr_t, b1, b2, eps, 0.f, rec, omd, SGG_GRID_I0, SGG_GRID_STRIDE);
}

// (values are only moved, never computed with: NaN payloads and the sign of zero survive)
__global__ void swap_kernel(float* __restrict__ a, float* __restrict__ b, long long n) {
  const long long n4 = n >> 2;
  for (long long i = SGG_GRID_I0; i < n4; i += SGG_GRID_STRIDE) {
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
  for (long long i = SGG_GRID_I0; i < n4; i += SGG_GRID_STRIDE) {
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
// The four Adam entry points (include/sgg_hip.h) differ in two optional operands: ema (with one_minus_decay) and record (in place of
// grad_scale).  "multi-tensor": every trainable tensor of a network lives in one arena, so one flat range covers them all.
static int adam_launch(const char* name, float* params, const float* grads, float* m, float* v, float* ema, long long n, float lr_t,
                       float beta1, float beta2, float eps, float grad_scale, const double* record, float one_minus_decay, bool has_ema,
                       bool guarded, void* stream) {
  SGG_CHECK_ARG(params && grads && m && v && (ema || !has_ema) && (record || !guarded) && n > 0, "%s: bad argument", name);
  SGG_CHECK_ARG((((uintptr_t)params | (uintptr_t)grads | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema) & 15) == 0,
                "%s: pointers must be 16-byte aligned", name);
  SGG_CHECK_ARG(((uintptr_t)record & 7) == 0, "%s: record must be 8-byte aligned", name);
  if (has_ema) {
    SGG_CHECK_ARG(!ranges_overlap(ema, params, n) && !ranges_overlap(ema, grads, n) && !ranges_overlap(ema, m, n) &&
                      !ranges_overlap(ema, v, n),
                  "%s: ema overlaps another operand", name);
    SGG_CHECK_ARG(one_minus_decay >= 0.f && one_minus_decay <= 1.f, "%s: one_minus_decay %g is outside [0, 1]", name,
                  (double)one_minus_decay);
  }
  const dim3 grid(grid_for(n / 4 + 1, 256)), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (has_ema && guarded)
    hipLaunchKernelGGL(adam_ema_guarded_kernel, grid, block, 0, s, params, grads, m, v, ema, n, lr_t, beta1, beta2, eps, record,
                       one_minus_decay);
  else if (has_ema)
    hipLaunchKernelGGL(adam_ema_kernel, grid, block, 0, s, params, grads, m, v, ema, n, lr_t, beta1, beta2, eps, grad_scale,
                       one_minus_decay);
  else if (guarded)
    hipLaunchKernelGGL(adam_guarded_kernel, grid, block, 0, s, params, grads, m, v, n, lr_t, beta1, beta2, eps, record);
  else
    hipLaunchKernelGGL(adam_kernel, grid, block, 0, s, params, grads, m, v, n, lr_t, beta1, beta2, eps, grad_scale);
  SGG_LAUNCH_CHECK(name);
  return SGG_OK;
}

// grad_scale multiplies the gradient first (1/world_size after a sum all-reduce)
extern "C" int sgg_adam_tf_multi(float* params, const float* grads, float* m, float* v, long long n, float lr_t, float beta1,
                                 float beta2, float eps, float grad_scale, void* stream) {
  return adam_launch("sgg_adam_tf_multi", params, grads, m, v, nullptr, n, lr_t, beta1, beta2, eps, grad_scale, nullptr, 0.f, false,
                     false, stream);
}

extern "C" int sgg_adam_tf_multi_ema(float* params, const float* grads, float* m, float* v, float* ema, long long n, float lr_t,
                                     float beta1, float beta2, float eps, float grad_scale, float one_minus_decay, void* stream) {
  return adam_launch("sgg_adam_tf_multi_ema", params, grads, m, v, ema, n, lr_t, beta1, beta2, eps, grad_scale, nullptr,
                     one_minus_decay, true, false, stream);
}

extern "C" int sgg_adam_tf_multi_guarded(float* params, const float* grads, float* m, float* v, long long n, float lr_t, float beta1,
                                         float beta2, float eps, const double* record, void* stream) {
  return adam_launch("sgg_adam_tf_multi_guarded", params, grads, m, v, nullptr, n, lr_t, beta1, beta2, eps, 0.f, record, 0.f, false,
                     true, stream);
}

extern "C" int sgg_adam_tf_multi_ema_guarded(float* params, const float* grads, float* m, float* v, float* ema, long long n,
                                             float lr_t, float beta1, float beta2, float eps, const double* record,
                                             float one_minus_decay, void* stream) {
  return adam_launch("sgg_adam_tf_multi_ema_guarded", params, grads, m, v, ema, n, lr_t, beta1, beta2, eps, 0.f, record,
                     one_minus_decay, true, true, stream);
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
