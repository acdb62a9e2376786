// Relaxed generator output: the critic's fake rows as points of the probability simplex (gfx950).
//     forward    y_j  = exp(z_j - max z) / sum_k exp(z_k - max z),   z = (x + g) / tau,   g = 0 or Gumbel noise drawn in the kernel
//     backward   dx_j = (scale / tau) * y_j * (dy_j - sum_k y_k dy_k)          (needs neither x nor the noise)
// The noise is a pure function of (seed, draw, r, j): Philox4x32-10 with key (seed lo, seed hi) and counter (j >> 2, r, draw lo,
// draw hi); element j takes output word j & 3; u = ((w >> 9) + 0.5) * 2^-23 (exact in fp32, strictly inside (0, 1): no clamp);
// g = -log(-log u).  Nothing is drawn on the host, and a row may be recomputed at any time: the streaming forward draws it twice.
// Both kernels have the two decompositions of csrc/xent.hip (rows need not be 16-byte aligned):
//     V <= 1024   one wave per row, the row RESIDENT in 16 registers per lane (y and dy: 32), wave-shuffle reductions; one row per
//                 workgroup up to 1024 rows, four above.
//     V >  1024   one 1024-thread workgroup per row.  Pass 1: online maximum / sum (forward), dot product (backward); pass 2 re-reads
//                 the row and rewrites it.  16-byte accesses on the aligned body of the row, scalar peels in front and behind; where
//                 the rows of a pass are misaligned differently that pass is scalar.
// Aliasing (y on x, dx on dy, same stride): a resident row is read whole before it is written; a streaming row is written in pass 2
// only, behind the barrier that ends pass 1, and there every element is read and written by the same thread.
// No float atomics, no workspace; every sum has a fixed order for given pointers and shapes: two calls give the same bits.
// The straight-through (hard) pair sits behind the soft entry points: one-hot rows of argmax(x + g) forward, the soft row's gradient
// rebuilt from x and the noise backward, in the same two decompositions.
#include "sgg_common.h"

#include <cmath>

#define RELAX_MAX_V (1 << 21)                    // csrc/xent.hip's XENT_MAX_V
#define RELAX_SMALL_V 1024                       // rows up to here are register-resident
#define RELAX_NPER (RELAX_SMALL_V / 64)
#define RELAX_SPREAD_R 1024                      // resident rows: up to this many, one row per workgroup; above, four
#define RELAX_T 1024                             // threads of a streaming workgroup

struct relax_rng {                               // seed and draw as the 32-bit words Philox takes
  unsigned k0, k1, d0, d1;
};

// Philox4x32-10 (Salmon et al., SC'11): the block function
__device__ __forceinline__ void relax_philox(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned w[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const unsigned h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0;
    c1 = l1;
    c2 = h0 ^ c3 ^ k1;
    c3 = l0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

__device__ __forceinline__ float relax_u(unsigned w) { return ((float)(w >> 9) + 0.5f) * 0x1p-23f; }
__device__ __forceinline__ float relax_gumbel(float u) { return -logf(-logf(u)); }

// u of element j of row r (one block per call: the scalar paths)
__device__ __forceinline__ float relax_u_at(const relax_rng& g, unsigned r, int j) {
  unsigned w[4];
  relax_philox((unsigned)j >> 2, r, g.d0, g.d1, g.k0, g.k1, w);
  const int c = j & 3;
  return relax_u(c == 0 ? w[0] : c == 1 ? w[1] : c == 2 ? w[2] : w[3]);
}

// u of the four elements i0 .. i0 + 3: one block where i0 is a multiple of four, else the two blocks they straddle
__device__ __forceinline__ void relax_u4(const relax_rng& g, unsigned r, int i0, float u[4]) {
  unsigned a[4], b[4];
  relax_philox((unsigned)i0 >> 2, r, g.d0, g.d1, g.k0, g.k1, a);
  const int s = i0 & 3;                          // (the same for every 16-byte word of a row: a uniform branch)
  if (s == 0) {
#pragma unroll
    for (int c = 0; c < 4; ++c) u[c] = relax_u(a[c]);
    return;
  }
  relax_philox(((unsigned)i0 >> 2) + 1u, r, g.d0, g.d1, g.k0, g.k1, b);
  unsigned w[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
#pragma unroll
  for (int c = 0; c < 4; ++c) u[c] = relax_u(s == 1 ? w[c + 1] : s == 2 ? w[c + 2] : w[c + 3]);
}

// elements in front of the first 16-byte boundary of a row
__device__ __forceinline__ int relax_head(const float* p, int V) {
  const int h = (int)((4u - (unsigned)((reinterpret_cast<uintptr_t>(p) >> 2) & 3u)) & 3u);
  return h < V ? h : V;
}

// ---- forward -----------------------------------------------------------------------------------------------------------------------
template <bool GUMBEL>
__global__ __launch_bounds__(256) void relax_rows_resident_kernel(const float* x, long long ldx, int R, int V, float inv_tau, relax_rng rng,
                                                                  float* y, long long ldy, float* u_out, long long ldu) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= R) return;                                   // (no barrier in this kernel: waves are independent)
  const float* xr = x + (size_t)row * (size_t)ldx;
  float v[RELAX_NPER];
  float m = -INFINITY;
#pragma unroll
  for (int i = 0; i < RELAX_NPER; ++i) {
    const int idx = lane + 64 * i;
    v[i] = -INFINITY;
    if (idx < V) {
      float xv = xr[idx];
      if (GUMBEL) {
        const float u = relax_u_at(rng, (unsigned)row, idx);
        if (u_out) u_out[(size_t)row * (size_t)ldu + idx] = u;
        xv += relax_gumbel(u);
      }
      v[i] = xv * inv_tau;
    }
    m = fmaxf(m, v[i]);
  }
  m = wave_max(m);
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < RELAX_NPER; ++i) {
    v[i] = lane + 64 * i < V ? expf(v[i] - m) : 0.f;
    s += v[i];
  }
  s = wave_sum(s);
  const float inv = 1.f / s;
  float* yr = y + (size_t)row * (size_t)ldy;
#pragma unroll
  for (int i = 0; i < RELAX_NPER; ++i) {
    const int idx = lane + 64 * i;
    if (idx < V) yr[idx] = v[i] * inv;
  }
}

// online maximum / sum of one thread: s = sum exp(z - m) over the elements seen so far
__device__ __forceinline__ void relax_online(float z, float& m, float& s) {
  if (z > m) {
    s = s * expf(m - z) + 1.f;                            // (first element: 0 * exp(-inf) + 1)
    m = z;
  } else {
    s += expf(z - m);
  }
}

template <bool GUMBEL>
__device__ __forceinline__ float relax_z(float xv, const relax_rng& rng, unsigned row, int idx, float inv_tau, float* ur) {
  if (GUMBEL) {
    const float u = relax_u_at(rng, row, idx);
    if (ur) ur[idx] = u;
    xv += relax_gumbel(u);
  }
  return xv * inv_tau;
}

template <bool GUMBEL>
__device__ __forceinline__ void relax_z4(f32x4& v4, const relax_rng& rng, unsigned row, int i0, float inv_tau, float* ur) {
  if (GUMBEL) {
    float u[4];
    relax_u4(rng, row, i0, u);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (ur) ur[i0 + c] = u[c];
      v4[c] += relax_gumbel(u[c]);
    }
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) v4[c] *= inv_tau;
}

template <bool GUMBEL>
__global__ __launch_bounds__(RELAX_T) void relax_rows_stream_kernel(const float* x, long long ldx, int V, float inv_tau, relax_rng rng, float* y,
                                                                    long long ldy, float* u_out, long long ldu) {
  __shared__ float red_m[RELAX_T / 64], red_s[RELAX_T / 64];
  const int tid = threadIdx.x;
  const size_t row = blockIdx.x;
  const unsigned r32 = (unsigned)row;
  const float* xr = x + row * (size_t)ldx;
  float* yr = y + row * (size_t)ldy;
  float* ur = u_out ? u_out + row * (size_t)ldu : nullptr;          // (written in pass 1 only, 4 bytes at a time: any alignment)
  const int head = relax_head(xr, V), nvec = (V - head) >> 2, tail0 = head + 4 * nvec;
  // ---- pass 1: one read of the row ---------------------------------------------------------------------------------------------
  float m = -INFINITY, s = 0.f;
  if (tid < head) relax_online(relax_z<GUMBEL>(xr[tid], rng, r32, tid, inv_tau, ur), m, s);
  const f32x4* xb = reinterpret_cast<const f32x4*>(xr + head);
  int q = tid;
  // four 16-byte loads in flight per thread (csrc/xent.hip); the elements are consumed in ascending order either way
  for (; q + 3 * RELAX_T < nvec; q += 4 * RELAX_T) {
    f32x4 v4[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v4[k] = xb[q + k * RELAX_T];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      relax_z4<GUMBEL>(v4[k], rng, r32, head + 4 * (q + k * RELAX_T), inv_tau, ur);
#pragma unroll
      for (int c = 0; c < 4; ++c) relax_online(v4[k][c], m, s);
    }
  }
  for (; q < nvec; q += RELAX_T) {
    f32x4 v4 = xb[q];
    relax_z4<GUMBEL>(v4, rng, r32, head + 4 * q, inv_tau, ur);
#pragma unroll
    for (int c = 0; c < 4; ++c) relax_online(v4[c], m, s);
  }
  if (tail0 + tid < V) relax_online(relax_z<GUMBEL>(xr[tail0 + tid], rng, r32, tail0 + tid, inv_tau, ur), m, s);
  // wave, then workgroup, in a fixed order; a thread or wave without elements holds (m, s) = (-inf, 0) and adds nothing
  const float wm = wave_max(m);
  const float ws = wave_sum(m == -INFINITY ? 0.f : s * expf(m - wm));
  if ((tid & 63) == 0) { red_m[tid >> 6] = wm; red_s[tid >> 6] = ws; }
  __syncthreads();                                          // every read of pass 1 is behind this barrier (y may be x)
  float bm = red_m[0];
  for (int w = 1; w < RELAX_T / 64; ++w) bm = fmaxf(bm, red_m[w]);
  float bs = 0.f;
  for (int w = 0; w < RELAX_T / 64; ++w)
    if (red_m[w] != -INFINITY) bs += red_s[w] * expf(red_m[w] - bm);
  const float inv = 1.f / bs;
  // ---- pass 2: y; the row is read (and its noise drawn) a second time -----------------------------------------------------------------
  if (relax_head(yr, V) != head) {                          // the two rows sit differently against 16 bytes: 4-byte accesses
    for (int i = tid; i < V; i += RELAX_T) yr[i] = expf(relax_z<GUMBEL>(xr[i], rng, r32, i, inv_tau, nullptr) - bm) * inv;
    return;
  }
  if (tid < head) yr[tid] = expf(relax_z<GUMBEL>(xr[tid], rng, r32, tid, inv_tau, nullptr) - bm) * inv;
#pragma unroll 2
  for (int p = tid; p < nvec; p += RELAX_T) {
    const int i0 = head + 4 * p;
    f32x4 v4 = *reinterpret_cast<const f32x4*>(xr + i0);
    relax_z4<GUMBEL>(v4, rng, r32, i0, inv_tau, nullptr);
#pragma unroll
    for (int c = 0; c < 4; ++c) v4[c] = expf(v4[c] - bm) * inv;
    *reinterpret_cast<f32x4*>(yr + i0) = v4;
  }
  if (tail0 + tid < V) {
    const int i = tail0 + tid;
    yr[i] = expf(relax_z<GUMBEL>(xr[i], rng, r32, i, inv_tau, nullptr) - bm) * inv;
  }
}

// ---- backward ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void relax_bwd_resident_kernel(const float* __restrict__ y, long long ldy, const float* dy, long long lddy,
                                                                 int R, int V, float coef, float* dx, long long lddx) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= R) return;
  const float* yr = y + (size_t)row * (size_t)ldy;
  const float* gr = dy + (size_t)row * (size_t)lddy;
  float yv[RELAX_NPER], gv[RELAX_NPER];
  float dot = 0.f;
#pragma unroll
  for (int i = 0; i < RELAX_NPER; ++i) {
    const int idx = lane + 64 * i;
    yv[i] = idx < V ? yr[idx] : 0.f;
    gv[i] = idx < V ? gr[idx] : 0.f;
    dot += yv[i] * gv[i];
  }
  dot = wave_sum(dot);
  float* dr = dx + (size_t)row * (size_t)lddx;
#pragma unroll
  for (int i = 0; i < RELAX_NPER; ++i) {
    const int idx = lane + 64 * i;
    if (idx < V) dr[idx] = coef * yv[i] * (gv[i] - dot);
  }
}

__global__ __launch_bounds__(RELAX_T) void relax_bwd_stream_kernel(const float* __restrict__ y, long long ldy, const float* dy, long long lddy,
                                                                   int V, float coef, float* dx, long long lddx) {
  __shared__ float red[RELAX_T / 64];
  const int tid = threadIdx.x;
  const size_t row = blockIdx.x;
  const float* yr = y + row * (size_t)ldy;
  const float* gr = dy + row * (size_t)lddy;
  float* dr = dx + row * (size_t)lddx;
  const int head = relax_head(yr, V), nvec = (V - head) >> 2, tail0 = head + 4 * nvec;
  const bool vec1 = relax_head(gr, V) == head;             // y and dy sit alike against 16 bytes
  // ---- pass 1: the dot product ---------------------------------------------------------------------------------------------------
  float dot = 0.f;
  if (!vec1) {
    for (int i = tid; i < V; i += RELAX_T) dot += yr[i] * gr[i];
  } else {
    if (tid < head) dot += yr[tid] * gr[tid];
#pragma unroll 4
    for (int p = tid; p < nvec; p += RELAX_T) {
      const int i0 = head + 4 * p;
      const f32x4 a = *reinterpret_cast<const f32x4*>(yr + i0);
      const f32x4 b = *reinterpret_cast<const f32x4*>(gr + i0);
#pragma unroll
      for (int c = 0; c < 4; ++c) dot += a[c] * b[c];
    }
    if (tail0 + tid < V) dot += yr[tail0 + tid] * gr[tail0 + tid];
  }
  dot = wave_sum(dot);
  if ((tid & 63) == 0) red[tid >> 6] = dot;
  __syncthreads();                                          // every read of pass 1 is behind this barrier (dx may be dy)
  dot = 0.f;
  for (int w = 0; w < RELAX_T / 64; ++w) dot += red[w];
  // ---- pass 2: dx ----------------------------------------------------------------------------------------------------------------
  if (!vec1 || relax_head(dr, V) != head) {
    for (int i = tid; i < V; i += RELAX_T) dr[i] = coef * yr[i] * (gr[i] - dot);
    return;
  }
  if (tid < head) dr[tid] = coef * yr[tid] * (gr[tid] - dot);
#pragma unroll 4
  for (int p = tid; p < nvec; p += RELAX_T) {
    const int i0 = head + 4 * p;
    const f32x4 a = *reinterpret_cast<const f32x4*>(yr + i0);
    const f32x4 b = *reinterpret_cast<const f32x4*>(gr + i0);
    f32x4 o;
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] = coef * a[c] * (b[c] - dot);
    *reinterpret_cast<f32x4*>(dr + i0) = o;
  }
  if (tail0 + tid < V) {
    const int i = tail0 + tid;
    dr[i] = coef * yr[i] * (gr[i] - dot);
  }
}

// ---- entry points --------------------------------------------------------------------------------------------------------------------
extern "C" int sgg_relax_rows(const float* x, long long ldx, int R, int V, float tau, int gumbel, unsigned long long seed,
                              unsigned long long draw, float* y, long long ldy, float* u_out, long long ldu, void* stream) {
  SGG_CHECK_ARG(std::isfinite(tau) && tau > 0.f, "sgg_relax_rows: tau must be finite and > 0 (got %g)", (double)tau);
  SGG_CHECK_ARG(R >= 1 && V >= 1 && V <= RELAX_MAX_V, "sgg_relax_rows: R >= 1 and 1 <= V <= 2^21 (got R = %d, V = %d)", R, V);
  SGG_CHECK_ARG(x && y, "sgg_relax_rows: null pointer");
  SGG_CHECK_ARG(ldx >= V && ldy >= V, "sgg_relax_rows: row strides ldx, ldy >= V (got ldx = %lld, ldy = %lld, V = %d)", ldx, ldy, V);
  SGG_CHECK_ARG((const float*)y != x || ldy == ldx, "sgg_relax_rows: y aliasing x needs the same row stride (got ldx = %lld, ldy = %lld)", ldx,
                ldy);
  SGG_CHECK_ARG(gumbel == 0 || gumbel == 1, "sgg_relax_rows: gumbel is 0 or 1 (got %d)", gumbel);
  SGG_CHECK_ARG(!u_out || (gumbel && ldu >= V && u_out != y && (const float*)u_out != x),
                "sgg_relax_rows: u_out needs gumbel = 1, a row stride ldu >= V and a buffer of its own (got gumbel = %d, ldu = %lld)", gumbel,
                ldu);
  const float inv_tau = 1.f / tau;
  const relax_rng rng = {(unsigned)(seed & 0xffffffffu), (unsigned)(seed >> 32), (unsigned)(draw & 0xffffffffu), (unsigned)(draw >> 32)};
  hipStream_t st = (hipStream_t)stream;
  if (V <= RELAX_SMALL_V) {
    const int wg_rows = R <= RELAX_SPREAD_R ? 1 : 4;
    const dim3 grid(sgg_cdiv(R, wg_rows)), block(64 * wg_rows);
    if (gumbel)
      hipLaunchKernelGGL(relax_rows_resident_kernel<true>, grid, block, 0, st, x, ldx, R, V, inv_tau, rng, y, ldy, u_out, ldu);
    else
      hipLaunchKernelGGL(relax_rows_resident_kernel<false>, grid, block, 0, st, x, ldx, R, V, inv_tau, rng, y, ldy, u_out, ldu);
  } else if (gumbel) {
    hipLaunchKernelGGL(relax_rows_stream_kernel<true>, dim3(R), dim3(RELAX_T), 0, st, x, ldx, V, inv_tau, rng, y, ldy, u_out, ldu);
  } else {
    hipLaunchKernelGGL(relax_rows_stream_kernel<false>, dim3(R), dim3(RELAX_T), 0, st, x, ldx, V, inv_tau, rng, y, ldy, u_out, ldu);
  }
  SGG_LAUNCH_CHECK("sgg_relax_rows");
  return SGG_OK;
}

extern "C" int sgg_relax_rows_bwd(const float* y, long long ldy, const float* dy, long long lddy, int R, int V, float tau, float scale,
                                  float* dx, long long lddx, void* stream) {
  SGG_CHECK_ARG(std::isfinite(tau) && tau > 0.f, "sgg_relax_rows_bwd: tau must be finite and > 0 (got %g)", (double)tau);
  SGG_CHECK_ARG(std::isfinite(scale), "sgg_relax_rows_bwd: scale must be finite (got %g)", (double)scale);
  SGG_CHECK_ARG(R >= 1 && V >= 1 && V <= RELAX_MAX_V, "sgg_relax_rows_bwd: R >= 1 and 1 <= V <= 2^21 (got R = %d, V = %d)", R, V);
  SGG_CHECK_ARG(y && dy && dx, "sgg_relax_rows_bwd: null pointer");
  SGG_CHECK_ARG(ldy >= V && lddy >= V && lddx >= V,
                "sgg_relax_rows_bwd: row strides ldy, lddy, lddx >= V (got ldy = %lld, lddy = %lld, lddx = %lld, V = %d)", ldy, lddy, lddx, V);
  SGG_CHECK_ARG((const float*)dx != dy || lddx == lddy,
                "sgg_relax_rows_bwd: dx aliasing dy needs the same row stride (got lddy = %lld, lddx = %lld)", lddy, lddx);
  SGG_CHECK_ARG((const float*)dx != y, "sgg_relax_rows_bwd: dx must not alias y");
  const float coef = scale / tau;
  hipStream_t st = (hipStream_t)stream;
  if (V <= RELAX_SMALL_V) {
    const int wg_rows = R <= RELAX_SPREAD_R ? 1 : 4;
    hipLaunchKernelGGL(relax_bwd_resident_kernel, dim3(sgg_cdiv(R, wg_rows)), dim3(64 * wg_rows), 0, st, y, ldy, dy, lddy, R, V, coef, dx, lddx);
  } else {
    hipLaunchKernelGGL(relax_bwd_stream_kernel, dim3(R), dim3(RELAX_T), 0, st, y, ldy, dy, lddy, V, coef, dx, lddx);
  }
  SGG_LAUNCH_CHECK("sgg_relax_rows_bwd");
  return SGG_OK;
}

// ---- straight-through (hard) rows ----------------------------------------------------------------------------------------------------
//     forward    k = first argmax_j (x_j + g_j), g as above;   y_j = 1.0f at j = k, +0.0f elsewhere;   tok = k
//     backward   dx_j = (scale / tau) * y_j * (dy_j - sum_k y_k dy_k) with the SOFT row y = softmax((x + g) / tau) rebuilt from x and
//                the noise: the critic's input buffer holds the one-hot row, not y
// The argmax is taken on the fp32 x + g, before any scaling: there is no tau in the forward.  (value, index) pairs: the larger value
// wins, on equal values the smaller index - the tie rule of argmax_rows (csrc/misc.hip).  A row without a comparable maximum (NaN
// everywhere: outside the precondition) gives 0; no store is addressed by k, every thread compares its own indices with it.
struct relax_best {
  float v;
  int i;
};

__device__ __forceinline__ void relax_take(relax_best& b, float v, int i) {      // indices arrive in ascending order: a strict >
  if (v > b.v) { b.v = v; b.i = i; }
}
__device__ __forceinline__ void relax_merge(relax_best& b, float ov, int oi) {
  if (ov > b.v || (ov == b.v && oi < b.i)) { b.v = ov; b.i = oi; }
}
__device__ __forceinline__ relax_best wave_best(relax_best b) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(b.v, o, 64);
    const int oi = __shfl_xor(b.i, o, 64);
    relax_merge(b, ov, oi);
  }
  return b;
}

template <bool GUMBEL>
__global__ __launch_bounds__(256) void relax_hard_resident_kernel(const float* x, long long ldx, int R, int V, relax_rng rng, float* y,
                                                                  long long ldy, long long* tok) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= R) return;                                   // (no barrier in this kernel: waves are independent)
  const float* xr = x + (size_t)row * (size_t)ldx;
  float v[RELAX_NPER];
#pragma unroll
  for (int i = 0; i < RELAX_NPER; ++i) {
    const int idx = lane + 64 * i;
    v[i] = idx < V ? xr[idx] : -INFINITY;
  }
  relax_best b = {-INFINITY, 0x7fffffff};
#pragma unroll
  for (int i = 0; i < RELAX_NPER; ++i) {
    const int idx = lane + 64 * i;
    if (idx < V) {
      float s = v[i];
      if (GUMBEL) s += relax_gumbel(relax_u_at(rng, (unsigned)row, idx));
      relax_take(b, s, idx);
    }
  }
  b = wave_best(b);                                       // every load of the row is in front of this exchange (y may be x)
  const int k = b.i < V ? b.i : 0;
  if (tok && lane == 0) tok[row] = (long long)k;
  if (!y) return;
  float* yr = y + (size_t)row * (size_t)ldy;
#pragma unroll
  for (int i = 0; i < RELAX_NPER; ++i) {
    const int idx = lane + 64 * i;
    if (idx < V) yr[idx] = idx == k ? 1.f : 0.f;
  }
}

template <bool GUMBEL>
__device__ __forceinline__ float relax_s(float xv, const relax_rng& rng, unsigned row, int idx) {
  if (GUMBEL) xv += relax_gumbel(relax_u_at(rng, row, idx));
  return xv;
}

template <bool GUMBEL>
__device__ __forceinline__ void relax_s4(f32x4& v4, const relax_rng& rng, unsigned row, int i0) {
  if (GUMBEL) {
    float u[4];
    relax_u4(rng, row, i0, u);
#pragma unroll
    for (int c = 0; c < 4; ++c) v4[c] += relax_gumbel(u[c]);
  }
}

template <bool GUMBEL>
__global__ __launch_bounds__(RELAX_T) void relax_hard_stream_kernel(const float* x, long long ldx, int V, relax_rng rng, float* y, long long ldy,
                                                                    long long* tok) {
  __shared__ float red_v[RELAX_T / 64];
  __shared__ int red_i[RELAX_T / 64];
  const int tid = threadIdx.x;
  const size_t row = blockIdx.x;
  const unsigned r32 = (unsigned)row;
  const float* xr = x + row * (size_t)ldx;
  const int head = relax_head(xr, V), nvec = (V - head) >> 2, tail0 = head + 4 * nvec;
  // ---- pass 1: one read of the row, one draw; a thread's indices ascend (head < body < tail) ------------------------------------------
  relax_best b = {-INFINITY, 0x7fffffff};
  if (tid < head) relax_take(b, relax_s<GUMBEL>(xr[tid], rng, r32, tid), tid);
  const f32x4* xb = reinterpret_cast<const f32x4*>(xr + head);
  int q = tid;
  for (; q + 3 * RELAX_T < nvec; q += 4 * RELAX_T) {      // four 16-byte loads in flight per thread, consumed in ascending order
    f32x4 v4[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v4[k] = xb[q + k * RELAX_T];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i0 = head + 4 * (q + k * RELAX_T);
      relax_s4<GUMBEL>(v4[k], rng, r32, i0);
#pragma unroll
      for (int c = 0; c < 4; ++c) relax_take(b, v4[k][c], i0 + c);
    }
  }
  for (; q < nvec; q += RELAX_T) {
    f32x4 v4 = xb[q];
    const int i0 = head + 4 * q;
    relax_s4<GUMBEL>(v4, rng, r32, i0);
#pragma unroll
    for (int c = 0; c < 4; ++c) relax_take(b, v4[c], i0 + c);
  }
  if (tail0 + tid < V) relax_take(b, relax_s<GUMBEL>(xr[tail0 + tid], rng, r32, tail0 + tid), tail0 + tid);
  b = wave_best(b);
  if ((tid & 63) == 0) { red_v[tid >> 6] = b.v; red_i[tid >> 6] = b.i; }
  __syncthreads();                                          // every read of the row is behind this barrier (y may be x)
  relax_best w = {red_v[0], red_i[0]};
  for (int j = 1; j < RELAX_T / 64; ++j) relax_merge(w, red_v[j], red_i[j]);
  const int k = w.i < V ? w.i : 0;
  if (tok && tid == 0) tok[row] = (long long)k;
  if (!y) return;
  // ---- pass 2: nothing is read or drawn; zeros in 16-byte stores on y's own aligned body, the 1 by the thread that owns k -----------
  float* yr = y + row * (size_t)ldy;
  const int yhead = relax_head(yr, V), ynvec = (V - yhead) >> 2, ytail0 = yhead + 4 * ynvec;
  if (tid < yhead) yr[tid] = tid == k ? 1.f : 0.f;
  for (int p = tid; p < ynvec; p += RELAX_T) {
    const int i0 = yhead + 4 * p;
    f32x4 o;
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] = i0 + c == k ? 1.f : 0.f;
    *reinterpret_cast<f32x4*>(yr + i0) = o;
  }
  if (ytail0 + tid < V) yr[ytail0 + tid] = ytail0 + tid == k ? 1.f : 0.f;
}

// resident backward: x and dy in registers (32 per lane); y as relax_rows_resident_kernel forms it, dx as relax_bwd_resident_kernel
template <bool GUMBEL>
__global__ __launch_bounds__(256) void relax_hard_bwd_resident_kernel(const float* __restrict__ x, long long ldx, const float* dy, long long lddy,
                                                                      int R, int V, float inv_tau, float coef, relax_rng rng, float* dx,
                                                                      long long lddx) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= R) return;
  const float* xr = x + (size_t)row * (size_t)ldx;
  const float* gr = dy + (size_t)row * (size_t)lddy;
  float v[RELAX_NPER], gv[RELAX_NPER];
  float m = -INFINITY;
#pragma unroll
  for (int i = 0; i < RELAX_NPER; ++i) {
    const int idx = lane + 64 * i;
    v[i] = -INFINITY;
    gv[i] = idx < V ? gr[idx] : 0.f;
    if (idx < V) v[i] = relax_s<GUMBEL>(xr[idx], rng, (unsigned)row, idx) * inv_tau;
    m = fmaxf(m, v[i]);
  }
  m = wave_max(m);
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < RELAX_NPER; ++i) {
    v[i] = lane + 64 * i < V ? expf(v[i] - m) : 0.f;
    s += v[i];
  }
  s = wave_sum(s);
  const float inv = 1.f / s;
  float dot = 0.f;
#pragma unroll
  for (int i = 0; i < RELAX_NPER; ++i) {
    v[i] *= inv;
    dot += v[i] * gv[i];
  }
  dot = wave_sum(dot);
  float* dr = dx + (size_t)row * (size_t)lddx;
#pragma unroll
  for (int i = 0; i < RELAX_NPER; ++i) {
    const int idx = lane + 64 * i;
    if (idx < V) dr[idx] = coef * v[i] * (gv[i] - dot);
  }
}

// online maximum / sum / weighted sum of one thread: s = sum exp(z - m), d = sum exp(z - m) * dy over the elements seen so far
__device__ __forceinline__ void relax_online3(float z, float g, float& m, float& s, float& d) {
  if (z > m) {
    const float c = expf(m - z);                            // (first element: exp(-inf) = 0)
    s = s * c + 1.f;
    d = d * c + g;
    m = z;
  } else {
    const float e = expf(z - m);
    s += e;
    d += e * g;
  }
}

// one element of pass 2 (s = x + g): the soft y of the streaming forward, then the gradient - one expression for every path of the pass
__device__ __forceinline__ float relax_dx(float s, float g, float inv_tau, float bm, float inv, float coef, float dot) {
  const float yv = expf(s * inv_tau - bm) * inv;
  return coef * yv * (g - dot);
}

template <bool GUMBEL>
__global__ __launch_bounds__(RELAX_T) void relax_hard_bwd_stream_kernel(const float* __restrict__ x, long long ldx, const float* dy,
                                                                        long long lddy, int V, float inv_tau, float coef, relax_rng rng,
                                                                        float* dx, long long lddx) {
  __shared__ float red_m[RELAX_T / 64], red_s[RELAX_T / 64], red_d[RELAX_T / 64];
  const int tid = threadIdx.x;
  const size_t row = blockIdx.x;
  const unsigned r32 = (unsigned)row;
  const float* xr = x + row * (size_t)ldx;
  const float* gr = dy + row * (size_t)lddy;
  float* dr = dx + row * (size_t)lddx;
  const int head = relax_head(xr, V), nvec = (V - head) >> 2, tail0 = head + 4 * nvec;
  const bool vec1 = relax_head(gr, V) == head;             // x and dy sit alike against 16 bytes
  // ---- pass 1: one read of x and dy, the online triple -------------------------------------------------------------------------------
  float m = -INFINITY, s = 0.f, d = 0.f;
  if (!vec1) {
    for (int i = tid; i < V; i += RELAX_T) relax_online3(relax_s<GUMBEL>(xr[i], rng, r32, i) * inv_tau, gr[i], m, s, d);
  } else {
    if (tid < head) relax_online3(relax_s<GUMBEL>(xr[tid], rng, r32, tid) * inv_tau, gr[tid], m, s, d);
#pragma unroll 2
    for (int p = tid; p < nvec; p += RELAX_T) {
      const int i0 = head + 4 * p;
      f32x4 a = *reinterpret_cast<const f32x4*>(xr + i0);
      const f32x4 g4 = *reinterpret_cast<const f32x4*>(gr + i0);
      relax_s4<GUMBEL>(a, rng, r32, i0);
#pragma unroll
      for (int c = 0; c < 4; ++c) relax_online3(a[c] * inv_tau, g4[c], m, s, d);
    }
    if (tail0 + tid < V) relax_online3(relax_s<GUMBEL>(xr[tail0 + tid], rng, r32, tail0 + tid) * inv_tau, gr[tail0 + tid], m, s, d);
  }
  // wave, then workgroup, in a fixed order; a thread or wave without elements holds (m, s, d) = (-inf, 0, 0) and adds nothing
  const float wm = wave_max(m);
  const float f = m == -INFINITY ? 0.f : expf(m - wm);
  const float ws = wave_sum(s * f), wd = wave_sum(d * f);
  if ((tid & 63) == 0) { red_m[tid >> 6] = wm; red_s[tid >> 6] = ws; red_d[tid >> 6] = wd; }
  __syncthreads();                                          // every read of pass 1 is behind this barrier (dx may be dy)
  float bm = red_m[0];
  for (int w = 1; w < RELAX_T / 64; ++w) bm = fmaxf(bm, red_m[w]);
  float bs = 0.f, bd = 0.f;
  for (int w = 0; w < RELAX_T / 64; ++w)
    if (red_m[w] != -INFINITY) {
      const float c = expf(red_m[w] - bm);
      bs += red_s[w] * c;
      bd += red_d[w] * c;
    }
  const float inv = 1.f / bs;
  const float dot = bd * inv;
  // ---- pass 2: both rows are read and the noise drawn a second time; every element is read and written by the same thread ------------
  if (!vec1 || relax_head(dr, V) != head) {
    for (int i = tid; i < V; i += RELAX_T) {
      dr[i] = relax_dx(relax_s<GUMBEL>(xr[i], rng, r32, i), gr[i], inv_tau, bm, inv, coef, dot);
    }
    return;
  }
  if (tid < head) dr[tid] = relax_dx(relax_s<GUMBEL>(xr[tid], rng, r32, tid), gr[tid], inv_tau, bm, inv, coef, dot);
#pragma unroll 2
  for (int p = tid; p < nvec; p += RELAX_T) {
    const int i0 = head + 4 * p;
    f32x4 a = *reinterpret_cast<const f32x4*>(xr + i0);
    const f32x4 g4 = *reinterpret_cast<const f32x4*>(gr + i0);
    relax_s4<GUMBEL>(a, rng, r32, i0);
    f32x4 o;
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] = relax_dx(a[c], g4[c], inv_tau, bm, inv, coef, dot);
    *reinterpret_cast<f32x4*>(dr + i0) = o;
  }
  if (tail0 + tid < V) {
    const int i = tail0 + tid;
    dr[i] = relax_dx(relax_s<GUMBEL>(xr[i], rng, r32, i), gr[i], inv_tau, bm, inv, coef, dot);
  }
}

extern "C" int sgg_relax_rows_hard(const float* x, long long ldx, int R, int V, int gumbel, unsigned long long seed, unsigned long long draw,
                                   float* y, long long ldy, long long* tok, void* stream) {
  SGG_CHECK_ARG(R >= 1 && V >= 1 && V <= RELAX_MAX_V, "sgg_relax_rows_hard: R >= 1 and 1 <= V <= 2^21 (got R = %d, V = %d)", R, V);
  SGG_CHECK_ARG(x && (y || tok), "sgg_relax_rows_hard: null pointer (x, and at least one of y and tok)");
  SGG_CHECK_ARG(ldx >= V && (!y || ldy >= V), "sgg_relax_rows_hard: row strides ldx, ldy >= V (got ldx = %lld, ldy = %lld, V = %d)", ldx, ldy,
                V);
  SGG_CHECK_ARG((const float*)y != x || ldy == ldx, "sgg_relax_rows_hard: y aliasing x needs the same row stride (got ldx = %lld, ldy = %lld)",
                ldx, ldy);
  SGG_CHECK_ARG(gumbel == 0 || gumbel == 1, "sgg_relax_rows_hard: gumbel is 0 or 1 (got %d)", gumbel);
  const relax_rng rng = {(unsigned)(seed & 0xffffffffu), (unsigned)(seed >> 32), (unsigned)(draw & 0xffffffffu), (unsigned)(draw >> 32)};
  hipStream_t st = (hipStream_t)stream;
  if (V <= RELAX_SMALL_V) {
    const int wg_rows = R <= RELAX_SPREAD_R ? 1 : 4;
    const dim3 grid(sgg_cdiv(R, wg_rows)), block(64 * wg_rows);
    if (gumbel)
      hipLaunchKernelGGL(relax_hard_resident_kernel<true>, grid, block, 0, st, x, ldx, R, V, rng, y, ldy, tok);
    else
      hipLaunchKernelGGL(relax_hard_resident_kernel<false>, grid, block, 0, st, x, ldx, R, V, rng, y, ldy, tok);
  } else if (gumbel) {
    hipLaunchKernelGGL(relax_hard_stream_kernel<true>, dim3(R), dim3(RELAX_T), 0, st, x, ldx, V, rng, y, ldy, tok);
  } else {
    hipLaunchKernelGGL(relax_hard_stream_kernel<false>, dim3(R), dim3(RELAX_T), 0, st, x, ldx, V, rng, y, ldy, tok);
  }
  SGG_LAUNCH_CHECK("sgg_relax_rows_hard");
  return SGG_OK;
}

extern "C" int sgg_relax_rows_hard_bwd(const float* x, long long ldx, const float* dy, long long lddy, int R, int V, float tau, float scale,
                                       int gumbel, unsigned long long seed, unsigned long long draw, float* dx, long long lddx, void* stream) {
  SGG_CHECK_ARG(std::isfinite(tau) && tau > 0.f, "sgg_relax_rows_hard_bwd: tau must be finite and > 0 (got %g)", (double)tau);
  SGG_CHECK_ARG(std::isfinite(scale), "sgg_relax_rows_hard_bwd: scale must be finite (got %g)", (double)scale);
  SGG_CHECK_ARG(R >= 1 && V >= 1 && V <= RELAX_MAX_V, "sgg_relax_rows_hard_bwd: R >= 1 and 1 <= V <= 2^21 (got R = %d, V = %d)", R, V);
  SGG_CHECK_ARG(x && dy && dx, "sgg_relax_rows_hard_bwd: null pointer");
  SGG_CHECK_ARG(ldx >= V && lddy >= V && lddx >= V,
                "sgg_relax_rows_hard_bwd: row strides ldx, lddy, lddx >= V (got ldx = %lld, lddy = %lld, lddx = %lld, V = %d)", ldx, lddy, lddx,
                V);
  SGG_CHECK_ARG((const float*)dx != dy || lddx == lddy,
                "sgg_relax_rows_hard_bwd: dx aliasing dy needs the same row stride (got lddy = %lld, lddx = %lld)", lddy, lddx);
  SGG_CHECK_ARG((const float*)dx != x, "sgg_relax_rows_hard_bwd: dx must not alias x");
  SGG_CHECK_ARG(gumbel == 0 || gumbel == 1, "sgg_relax_rows_hard_bwd: gumbel is 0 or 1 (got %d)", gumbel);
  const float inv_tau = 1.f / tau, coef = scale / tau;
  const relax_rng rng = {(unsigned)(seed & 0xffffffffu), (unsigned)(seed >> 32), (unsigned)(draw & 0xffffffffu), (unsigned)(draw >> 32)};
  hipStream_t st = (hipStream_t)stream;
  if (V <= RELAX_SMALL_V) {
    const int wg_rows = R <= RELAX_SPREAD_R ? 1 : 4;
    const dim3 grid(sgg_cdiv(R, wg_rows)), block(64 * wg_rows);
    if (gumbel)
      hipLaunchKernelGGL(relax_hard_bwd_resident_kernel<true>, grid, block, 0, st, x, ldx, dy, lddy, R, V, inv_tau, coef, rng, dx, lddx);
    else
      hipLaunchKernelGGL(relax_hard_bwd_resident_kernel<false>, grid, block, 0, st, x, ldx, dy, lddy, R, V, inv_tau, coef, rng, dx, lddx);
  } else if (gumbel) {
    hipLaunchKernelGGL(relax_hard_bwd_stream_kernel<true>, dim3(R), dim3(RELAX_T), 0, st, x, ldx, dy, lddy, V, inv_tau, coef, rng, dx, lddx);
  } else {
    hipLaunchKernelGGL(relax_hard_bwd_stream_kernel<false>, dim3(R), dim3(RELAX_T), 0, st, x, ldx, dy, lddy, V, inv_tau, coef, rng, dx, lddx);
  }
  SGG_LAUNCH_CHECK("sgg_relax_rows_hard_bwd");
  return SGG_OK;
}
