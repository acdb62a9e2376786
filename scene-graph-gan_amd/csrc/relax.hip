// Relaxed generator output: the critic's fake rows as points of the probability simplex (gfx950).
//     forward    y_j  = exp(z_j - max z) / sum_k exp(z_k - max z),   z = (x + g) / tau,   g = 0 or Gumbel noise drawn in the kernel
//     backward   dx_j = (scale / tau) * y_j * (dy_j - sum_k y_k dy_k)          (needs neither x nor the noise)
// Nothing is drawn on the host, and a row may be recomputed at any time: the streaming forward draws it twice.  The decomposition
// (resident rows of V <= 1024, streamed rows above), the noise and the pieces of every kernel here are those of csrc/softmax_rows.h;
// a resident row holds 16 registers per lane (two rows, y / x and dy: 32).
// Aliasing (y on x, dx on dy, same stride): a resident row is read whole before it is written; a streaming row is written in pass 2
// only, behind the barrier that ends pass 1, and there every element is read and written by the same thread.
// The straight-through (hard) pair sits behind the soft entry points: one-hot rows of argmax(x + g) forward, the soft row's gradient
// rebuilt from x and the noise backward, in the same two decompositions.
#include "softmax_rows.h"

#include <cmath>
#include <type_traits>

// ---- forward -----------------------------------------------------------------------------------------------------------------------
template <bool GUMBEL>
__global__ __launch_bounds__(256) void relax_rows_resident_kernel(const float* x, long long ldx, int R, int V, float inv_tau, relax_rng rng,
                                                                  float* y, long long ldy, float* u_out, long long ldu) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= R) return;
  const float* xr = x + (size_t)row * (size_t)ldx;
  const rows_noise<GUMBEL> noise = {rng, (unsigned)row, u_out ? u_out + (size_t)row * (size_t)ldu : nullptr};
  float v[ROWS_NPER];
  rows_resident_softmax(v, lane, V, [=](int, int idx) {
    float xv = xr[idx];
    noise.add(xv, idx);
    return xv * inv_tau;
  });
  float* yr = y + (size_t)row * (size_t)ldy;
#pragma unroll
  for (int i = 0; i < ROWS_NPER; ++i) {
    const int idx = lane + 64 * i;
    if (idx < V) yr[idx] = v[i];
  }
}

template <bool GUMBEL>
__global__ __launch_bounds__(ROWS_T) void relax_rows_stream_kernel(const float* x, long long ldx, int V, float inv_tau, relax_rng rng, float* y,
                                                                   long long ldy, float* u_out, long long ldu) {
  const int tid = threadIdx.x;
  const size_t row = blockIdx.x;
  const float* xr = x + row * (size_t)ldx;
  // ---- pass 1: one read of the row; u_out is written here only ------------------------------------------------------------------
  const rows_noise<GUMBEL> draw1 = {rng, (unsigned)row, u_out ? u_out + row * (size_t)ldu : nullptr}, draw2 = {rng, (unsigned)row, nullptr};
  rows_online<false, false> acc;
  rows_walk<1, true>(tid, V, xr, nullptr, nullptr, draw1, [&acc, inv_tau](int, float s, float) {
    acc.take(s * inv_tau);
    return 0.f;
  });
  acc.merge();                                              // every read of pass 1 is behind its barrier (y may be x)
  const float bm = acc.m, inv = 1.f / acc.s;
  // ---- pass 2: y; the row is read (and its noise drawn) a second time -----------------------------------------------------------------
  rows_walk<2>(tid, V, xr, nullptr, y + row * (size_t)ldy, draw2, [=](int, float s, float) { return expf(s * inv_tau - bm) * inv; });
}

// ---- backward ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void relax_bwd_resident_kernel(const float* __restrict__ y, long long ldy, const float* dy, long long lddy,
                                                                 int R, int V, float coef, float* dx, long long lddx) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= R) return;
  const float* yr = y + (size_t)row * (size_t)ldy;
  const float* gr = dy + (size_t)row * (size_t)lddy;
  float yv[ROWS_NPER], gv[ROWS_NPER];
  float dot = 0.f;
#pragma unroll
  for (int i = 0; i < ROWS_NPER; ++i) {
    const int idx = lane + 64 * i;
    yv[i] = idx < V ? yr[idx] : 0.f;
    gv[i] = idx < V ? gr[idx] : 0.f;
    dot += yv[i] * gv[i];
  }
  dot = wave_sum(dot);
  float* dr = dx + (size_t)row * (size_t)lddx;
#pragma unroll
  for (int i = 0; i < ROWS_NPER; ++i) {
    const int idx = lane + 64 * i;
    if (idx < V) dr[idx] = coef * yv[i] * (gv[i] - dot);
  }
}

__global__ __launch_bounds__(ROWS_T) void relax_bwd_stream_kernel(const float* __restrict__ y, long long ldy, const float* dy, long long lddy,
                                                                  int V, float coef, float* dx, long long lddx) {
  __shared__ float red[ROWS_T / 64];
  const int tid = threadIdx.x;
  const size_t row = blockIdx.x;
  const float* yr = y + row * (size_t)ldy;
  const float* gr = dy + row * (size_t)lddy;
  // ---- pass 1: the dot product ---------------------------------------------------------------------------------------------------
  float dot = 0.f;
  rows_walk<4>(tid, V, yr, gr, nullptr, [&dot](int, float yv, float g) {
    dot += yv * g;
    return 0.f;
  });
  dot = wave_sum(dot);
  if ((tid & 63) == 0) red[tid >> 6] = dot;
  __syncthreads();                                          // every read of pass 1 is behind this barrier (dx may be dy)
  dot = 0.f;
  for (int w = 0; w < ROWS_T / 64; ++w) dot += red[w];
  // ---- pass 2: dx ----------------------------------------------------------------------------------------------------------------
  rows_walk<4>(tid, V, yr, gr, dx + row * (size_t)lddx, [=](int, float yv, float g) { return coef * yv * (g - dot); });
}

// ---- host: what the entry points share ------------------------------------------------------------------------------------------------
static relax_rng relax_pack_rng(unsigned long long seed, unsigned long long draw) {
  return {(unsigned)(seed & 0xffffffffu), (unsigned)(seed >> 32), (unsigned)(draw & 0xffffffffu), (unsigned)(draw >> 32)};
}

// launch(resident, gumbel, grid, block) with the first two as std::bool_constant: the <resident | stream> x <gumbel> instance of a kernel
template <class LAUNCH>
static void relax_launch(int R, int V, int gumbel, LAUNCH launch) {
  const rows_resident_geometry geo(R);
  if (V <= ROWS_SMALL_V) {
    if (gumbel) launch(std::true_type(), std::true_type(), geo.grid, geo.block);
    else launch(std::true_type(), std::false_type(), geo.grid, geo.block);
  } else if (gumbel) {
    launch(std::false_type(), std::true_type(), dim3(R), dim3(ROWS_T));
  } else {
    launch(std::false_type(), std::false_type(), dim3(R), dim3(ROWS_T));
  }
}

static int relax_check_tau(const char* fn, float tau) {
  SGG_CHECK_ARG(std::isfinite(tau) && tau > 0.f, "%s: tau must be finite and > 0 (got %g)", fn, (double)tau);
  return SGG_OK;
}
static int relax_check_shape(const char* fn, int R, int V) {
  SGG_CHECK_ARG(R >= 1 && V >= 1 && V <= ROWS_MAX_V, "%s: R >= 1 and 1 <= V <= 2^21 (got R = %d, V = %d)", fn, R, V);
  return SGG_OK;
}
// the two forwards: x -> y (y absent: ldy is not looked at)
static int relax_check_fwd(const char* fn, const float* x, long long ldx, int V, const float* y, long long ldy, int gumbel) {
  SGG_CHECK_ARG(ldx >= V && (!y || ldy >= V), "%s: row strides ldx, ldy >= V (got ldx = %lld, ldy = %lld, V = %d)", fn, ldx, ldy, V);
  SGG_CHECK_ARG(y != x || ldy == ldx, "%s: y aliasing x needs the same row stride (got ldx = %lld, ldy = %lld)", fn, ldx, ldy);
  SGG_CHECK_ARG(gumbel == 0 || gumbel == 1, "%s: gumbel is 0 or 1 (got %d)", fn, gumbel);
  return SGG_OK;
}
// the two backwards: (a, dy) -> dx, a = the row named `an` ("y": the soft row, "x": the logits)
static int relax_check_bwd(const char* fn, const char* an, const float* a, long long lda, const float* dy, long long lddy, int R, int V,
                           float tau, float scale, const float* dx, long long lddx) {
  if (const int rc = relax_check_tau(fn, tau)) return rc;
  SGG_CHECK_ARG(std::isfinite(scale), "%s: scale must be finite (got %g)", fn, (double)scale);
  if (const int rc = relax_check_shape(fn, R, V)) return rc;
  SGG_CHECK_ARG(a && dy && dx, "%s: null pointer", fn);
  SGG_CHECK_ARG(lda >= V && lddy >= V && lddx >= V, "%s: row strides ld%s, lddy, lddx >= V (got ld%s = %lld, lddy = %lld, lddx = %lld, V = %d)",
                fn, an, an, lda, lddy, lddx, V);
  SGG_CHECK_ARG(dx != dy || lddx == lddy, "%s: dx aliasing dy needs the same row stride (got lddy = %lld, lddx = %lld)", fn, lddy, lddx);
  SGG_CHECK_ARG(dx != a, "%s: dx must not alias %s", fn, an);
  return SGG_OK;
}

// ---- entry points --------------------------------------------------------------------------------------------------------------------
extern "C" int sgg_relax_rows(const float* x, long long ldx, int R, int V, float tau, int gumbel, unsigned long long seed,
                              unsigned long long draw, float* y, long long ldy, float* u_out, long long ldu, void* stream) {
  const char* fn = "sgg_relax_rows";
  if (const int rc = relax_check_tau(fn, tau)) return rc;
  if (const int rc = relax_check_shape(fn, R, V)) return rc;
  SGG_CHECK_ARG(x && y, "sgg_relax_rows: null pointer");
  if (const int rc = relax_check_fwd(fn, x, ldx, V, y, ldy, gumbel)) return rc;
  SGG_CHECK_ARG(!u_out || (gumbel && ldu >= V && u_out != y && (const float*)u_out != x),
                "sgg_relax_rows: u_out needs gumbel = 1, a row stride ldu >= V and a buffer of its own (got gumbel = %d, ldu = %lld)", gumbel,
                ldu);
  const float inv_tau = 1.f / tau;
  const relax_rng rng = relax_pack_rng(seed, draw);
  hipStream_t st = (hipStream_t)stream;
  relax_launch(R, V, gumbel, [&](auto resident, auto g, dim3 grid, dim3 block) {
    if constexpr (resident)
      hipLaunchKernelGGL(relax_rows_resident_kernel<g>, grid, block, 0, st, x, ldx, R, V, inv_tau, rng, y, ldy, u_out, ldu);
    else
      hipLaunchKernelGGL(relax_rows_stream_kernel<g>, grid, block, 0, st, x, ldx, V, inv_tau, rng, y, ldy, u_out, ldu);
  });
  SGG_LAUNCH_CHECK(fn);
  return SGG_OK;
}

extern "C" int sgg_relax_rows_bwd(const float* y, long long ldy, const float* dy, long long lddy, int R, int V, float tau, float scale,
                                  float* dx, long long lddx, void* stream) {
  const char* fn = "sgg_relax_rows_bwd";
  if (const int rc = relax_check_bwd(fn, "y", y, ldy, dy, lddy, R, V, tau, scale, dx, lddx)) return rc;
  const float coef = scale / tau;
  hipStream_t st = (hipStream_t)stream;
  if (V <= ROWS_SMALL_V) {
    const rows_resident_geometry geo(R);
    hipLaunchKernelGGL(relax_bwd_resident_kernel, geo.grid, geo.block, 0, st, y, ldy, dy, lddy, R, V, coef, dx, lddx);
  } else {
    hipLaunchKernelGGL(relax_bwd_stream_kernel, dim3(R), dim3(ROWS_T), 0, st, y, ldy, dy, lddy, V, coef, dx, lddx);
  }
  SGG_LAUNCH_CHECK(fn);
  return SGG_OK;
}

// ---- straight-through (hard) rows ----------------------------------------------------------------------------------------------------
//     forward    k = first argmax_j (x_j + g_j), g as above;   y_j = 1.0f at j = k, +0.0f elsewhere;   tok = k
//     backward   dx_j = (scale / tau) * y_j * (dy_j - sum_k y_k dy_k) with the SOFT row y = softmax((x + g) / tau) rebuilt from x and
//                the noise: the critic's input buffer holds the one-hot row, not y
// The argmax is taken on the fp32 x + g, before any scaling: there is no tau in the forward.  (value, index) pairs by wave_argmax's
// rule - that of argmax_rows (csrc/misc.hip).  A row without a comparable maximum (NaN everywhere: outside the precondition) gives
// 0; no store is addressed by k, every thread compares its own indices with it.
template <bool GUMBEL>
__global__ __launch_bounds__(256) void relax_hard_resident_kernel(const float* x, long long ldx, int R, int V, relax_rng rng, float* y,
                                                                  long long ldy, long long* tok) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= R) return;
  const float* xr = x + (size_t)row * (size_t)ldx;
  const rows_noise<GUMBEL> noise = {rng, (unsigned)row, nullptr};
  float v[ROWS_NPER];
#pragma unroll
  for (int i = 0; i < ROWS_NPER; ++i) {
    const int idx = lane + 64 * i;
    v[i] = idx < V ? xr[idx] : -INFINITY;
  }
  float bv = -INFINITY;
  int bi = 0x7fffffff;
#pragma unroll
  for (int i = 0; i < ROWS_NPER; ++i) {
    const int idx = lane + 64 * i;
    if (idx < V) {
      float s = v[i];
      noise.add(s, idx);
      if (s > bv) { bv = s; bi = idx; }                   // a lane's indices ascend: a strict >
    }
  }
  wave_argmax(bv, bi);                                    // every load of the row is in front of this exchange (y may be x)
  const int k = bi < V ? bi : 0;
  if (tok && lane == 0) tok[row] = (long long)k;
  if (!y) return;
  float* yr = y + (size_t)row * (size_t)ldy;
#pragma unroll
  for (int i = 0; i < ROWS_NPER; ++i) {
    const int idx = lane + 64 * i;
    if (idx < V) yr[idx] = idx == k ? 1.f : 0.f;
  }
}

template <bool GUMBEL>
__global__ __launch_bounds__(ROWS_T) void relax_hard_stream_kernel(const float* x, long long ldx, int V, relax_rng rng, float* y, long long ldy,
                                                                   long long* tok) {
  __shared__ float red_v[ROWS_T / 64];
  __shared__ int red_i[ROWS_T / 64];
  const int tid = threadIdx.x;
  const size_t row = blockIdx.x;
  const rows_noise<GUMBEL> noise = {rng, (unsigned)row, nullptr};
  // ---- pass 1: one read of the row, one draw; a thread's indices ascend (head < body < tail): a strict > ------------------------------
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  rows_walk<1, true>(tid, V, x + row * (size_t)ldx, nullptr, nullptr, noise, [&bv, &bi](int i, float s, float) {
    if (s > bv) { bv = s; bi = i; }
    return 0.f;
  });
  wave_argmax(bv, bi);
  if ((tid & 63) == 0) { red_v[tid >> 6] = bv; red_i[tid >> 6] = bi; }
  __syncthreads();                                          // every read of the row is behind this barrier (y may be x)
  lds_argmax(red_v, red_i, ROWS_T / 64, bv, bi);
  const int k = bi < V ? bi : 0;
  if (tok && tid == 0) tok[row] = (long long)k;
  if (!y) return;
  // ---- pass 2: nothing is read or drawn; 16-byte stores on y's own aligned body, the 1 by the thread that owns k ---------------------
  rows_walk<1>(tid, V, nullptr, nullptr, y + row * (size_t)ldy, [=](int i, float, float) { return i == k ? 1.f : 0.f; });
}

// resident backward: x and dy in registers (32 per lane); y is relax_rows_resident_kernel's, dx relax_bwd_resident_kernel's
template <bool GUMBEL>
__global__ __launch_bounds__(256) void relax_hard_bwd_resident_kernel(const float* __restrict__ x, long long ldx, const float* dy, long long lddy,
                                                                      int R, int V, float inv_tau, float coef, relax_rng rng, float* dx,
                                                                      long long lddx) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= R) return;
  const float* xr = x + (size_t)row * (size_t)ldx;
  const float* gr = dy + (size_t)row * (size_t)lddy;
  const rows_noise<GUMBEL> noise = {rng, (unsigned)row, nullptr};
  float v[ROWS_NPER], gv[ROWS_NPER];
#pragma unroll
  for (int i = 0; i < ROWS_NPER; ++i) gv[i] = 0.f;
  rows_resident_softmax(v, lane, V, [=, &gv](int i, int idx) {
    gv[i] = gr[idx];
    float s = xr[idx];
    noise.add(s, idx);
    return s * inv_tau;
  });
  float dot = 0.f;
#pragma unroll
  for (int i = 0; i < ROWS_NPER; ++i) dot += v[i] * gv[i];
  dot = wave_sum(dot);
  float* dr = dx + (size_t)row * (size_t)lddx;
#pragma unroll
  for (int i = 0; i < ROWS_NPER; ++i) {
    const int idx = lane + 64 * i;
    if (idx < V) dr[idx] = coef * v[i] * (gv[i] - dot);
  }
}

template <bool GUMBEL>
__global__ __launch_bounds__(ROWS_T) void relax_hard_bwd_stream_kernel(const float* __restrict__ x, long long ldx, const float* dy,
                                                                       long long lddy, int V, float inv_tau, float coef, relax_rng rng,
                                                                       float* dx, long long lddx) {
  const int tid = threadIdx.x;
  const size_t row = blockIdx.x;
  const float* xr = x + row * (size_t)ldx;
  const float* gr = dy + row * (size_t)lddy;
  const rows_noise<GUMBEL> noise = {rng, (unsigned)row, nullptr};
  // ---- pass 1: one read of x and dy, the online triple -------------------------------------------------------------------------------
  rows_online<false, true> acc;
  rows_walk<2>(tid, V, xr, gr, nullptr, noise, [&acc, inv_tau](int, float s, float g) {
    acc.take(s * inv_tau, 0, g);
    return 0.f;
  });
  acc.merge();                                              // every read of pass 1 is behind its barrier (dx may be dy)
  const float bm = acc.m, inv = 1.f / acc.s;
  const float dot = acc.d * inv;
  // ---- pass 2: both rows are read and the noise drawn a second time: the soft y of the streaming forward, then its gradient ------------
  rows_walk<2>(tid, V, xr, gr, dx + row * (size_t)lddx, noise, [=](int, float s, float g) {
    const float yv = expf(s * inv_tau - bm) * inv;
    return coef * yv * (g - dot);
  });
}

extern "C" int sgg_relax_rows_hard(const float* x, long long ldx, int R, int V, int gumbel, unsigned long long seed, unsigned long long draw,
                                   float* y, long long ldy, long long* tok, void* stream) {
  const char* fn = "sgg_relax_rows_hard";
  if (const int rc = relax_check_shape(fn, R, V)) return rc;
  SGG_CHECK_ARG(x && (y || tok), "sgg_relax_rows_hard: null pointer (x, and at least one of y and tok)");
  if (const int rc = relax_check_fwd(fn, x, ldx, V, y, ldy, gumbel)) return rc;
  const relax_rng rng = relax_pack_rng(seed, draw);
  hipStream_t st = (hipStream_t)stream;
  relax_launch(R, V, gumbel, [&](auto resident, auto g, dim3 grid, dim3 block) {
    if constexpr (resident)
      hipLaunchKernelGGL(relax_hard_resident_kernel<g>, grid, block, 0, st, x, ldx, R, V, rng, y, ldy, tok);
    else
      hipLaunchKernelGGL(relax_hard_stream_kernel<g>, grid, block, 0, st, x, ldx, V, rng, y, ldy, tok);
  });
  SGG_LAUNCH_CHECK(fn);
  return SGG_OK;
}

extern "C" int sgg_relax_rows_hard_bwd(const float* x, long long ldx, const float* dy, long long lddy, int R, int V, float tau, float scale,
                                       int gumbel, unsigned long long seed, unsigned long long draw, float* dx, long long lddx, void* stream) {
  const char* fn = "sgg_relax_rows_hard_bwd";
  if (const int rc = relax_check_bwd(fn, "x", x, ldx, dy, lddy, R, V, tau, scale, dx, lddx)) return rc;
  SGG_CHECK_ARG(gumbel == 0 || gumbel == 1, "sgg_relax_rows_hard_bwd: gumbel is 0 or 1 (got %d)", gumbel);
  const float inv_tau = 1.f / tau, coef = scale / tau;
  const relax_rng rng = relax_pack_rng(seed, draw);
  hipStream_t st = (hipStream_t)stream;
  relax_launch(R, V, gumbel, [&](auto resident, auto g, dim3 grid, dim3 block) {
    if constexpr (resident)
      hipLaunchKernelGGL(relax_hard_bwd_resident_kernel<g>, grid, block, 0, st, x, ldx, dy, lddy, R, V, inv_tau, coef, rng, dx, lddx);
    else
      hipLaunchKernelGGL(relax_hard_bwd_stream_kernel<g>, grid, block, 0, st, x, ldx, dy, lddy, V, inv_tau, coef, rng, dx, lddx);
  });
  SGG_LAUNCH_CHECK(fn);
  return SGG_OK;
}
