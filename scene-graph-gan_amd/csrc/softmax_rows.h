// Row kernels over [R, V] fp32 logits - the likelihood (csrc/xent.hip), the relaxed and straight-through generator output
// (csrc/relax.hip): their one decomposition and its device pieces (gfx950).  Rows need not be 16-byte aligned.
//     V <= 1024   one wave per row, the row RESIDENT in 16 registers per lane: one read (4-byte coalesced loads: any alignment),
//                 reductions by wave shuffles, the outputs from the registers.  One row per workgroup up to 1024 rows (a step's 192
//                 rows then spread over 192 CUs instead of sharing 48 of the 256), four rows per workgroup above (evaluation passes);
//                 the arithmetic of a row does not depend on it.  No barrier: waves are independent.
//     V >  1024   one 1024-thread workgroup per row, the row STREAMED twice.  Pass 1 reduces it ONLINE (a thread rescales its sum
//                 when its maximum grows), pass 2 re-reads it and writes.  Where that second read is served from has not been
//                 measured: one 280 KB row (V = 70 000) fits an XCD's 4 MiB L2, the ~24 rows an XCD works on at once at batch 64
//                 (6.7 MB) do not.  16-byte accesses on the aligned body of the row, a scalar peel in front and behind; where the
//                 rows of a pass sit differently against 16 bytes that pass is scalar.  A row is written in pass 2 only, behind
//                 the barrier that ends pass 1, and there every element is read and written by the same thread (in-place calls).
// No float atomics, no workspace; every sum has a fixed order for given pointers and shapes: two calls give the same bits.
#pragma once
#include "sgg_common.h"

#include <cstddef>

#define ROWS_MAX_V (1 << 21)
#define ROWS_SMALL_V 1024                       // rows up to here are register-resident
#define ROWS_NPER (ROWS_SMALL_V / 64)           // elements per lane of a resident row
#define ROWS_SPREAD_R 1024                      // resident rows: up to this many, one row per workgroup; above, four
#define ROWS_T 1024                             // threads of a streaming workgroup

// launch geometry of a resident kernel: a wave per row, blockDim.x / 64 rows per workgroup
struct rows_resident_geometry {
  dim3 grid, block;
  explicit rows_resident_geometry(int R) : grid(sgg_cdiv(R, R <= ROWS_SPREAD_R ? 1 : 4)), block(64 * (R <= ROWS_SPREAD_R ? 1 : 4)) {}
};

// elements in front of the first 16-byte boundary of a row
__device__ __forceinline__ int rows_head(const float* p, int V) {
  const int h = (int)((4u - (unsigned)((reinterpret_cast<uintptr_t>(p) >> 2) & 3u)) & 3u);
  return h < V ? h : V;
}

// ---- the noise: x + g --------------------------------------------------------------------------------------------------------------
// A pure function of (seed, draw, r, j): Philox4x32-10 with key (seed lo, seed hi) and counter (j >> 2, r, draw lo, draw hi); element
// j takes output word j & 3; u = ((w >> 9) + 0.5) * 2^-23 (exact in fp32, strictly inside (0, 1): no clamp); g = -log(-log u).
struct relax_rng {                                // seed and draw as the 32-bit words Philox takes
  unsigned k0, k1, d0, d1;
};

// Philox4x32-10 (Salmon et al., SC'11): the block function
__device__ __forceinline__ void rows_philox(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned w[4]) {
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

__device__ __forceinline__ float rows_u(unsigned w) { return ((float)(w >> 9) + 0.5f) * 0x1p-23f; }
__device__ __forceinline__ float rows_gumbel(float u) { return -logf(-logf(u)); }

// The draw of one row.  GUMBEL false: nothing is drawn, x stays.  ur: where the row's u go (4 bytes at a time: any alignment), or null.
template <bool GUMBEL>
struct rows_noise {
  relax_rng rng;
  unsigned row;
  float* ur;
  // x_idx + g: one Philox block per call (the scalar paths)
  __device__ __forceinline__ void add(float& xv, int idx) const {
    if (!GUMBEL) return;
    unsigned w[4];
    rows_philox((unsigned)idx >> 2, row, rng.d0, rng.d1, rng.k0, rng.k1, w);
    const int c = idx & 3;
    const float u = rows_u(c == 0 ? w[0] : c == 1 ? w[1] : c == 2 ? w[2] : w[3]);
    if (ur) ur[idx] = u;
    xv += rows_gumbel(u);
  }
  // the four elements i0 .. i0 + 3: one block where i0 is a multiple of four, else the two blocks they straddle
  __device__ __forceinline__ void add(f32x4& v4, int i0) const {
    if (!GUMBEL) return;
    unsigned a[4], b[4];
    float u[4];
    rows_philox((unsigned)i0 >> 2, row, rng.d0, rng.d1, rng.k0, rng.k1, a);
    const int s = i0 & 3;                        // (the same for every 16-byte word of a row: a uniform branch)
    if (s == 0) {
#pragma unroll
      for (int c = 0; c < 4; ++c) u[c] = rows_u(a[c]);
    } else {
      rows_philox(((unsigned)i0 >> 2) + 1u, row, rng.d0, rng.d1, rng.k0, rng.k1, b);
      const unsigned w[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
#pragma unroll
      for (int c = 0; c < 4; ++c) u[c] = rows_u(s == 1 ? w[c + 1] : s == 2 ? w[c + 2] : w[c + 3]);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (ur) ur[i0 + c] = u[c];
      v4[c] += rows_gumbel(u[c]);
    }
  }
};

// ---- one traversal of a streamed row -------------------------------------------------------------------------------------------------
// A row that a pass does not have is passed as nullptr - a fact of the call's types: its elements read as 0 and nothing is stored.
__device__ __forceinline__ float rows_get(std::nullptr_t, int) { return 0.f; }
__device__ __forceinline__ float rows_get(const float* p, int i) { return p[i]; }
__device__ __forceinline__ f32x4 rows_get4(std::nullptr_t, int) { return f32x4{0.f, 0.f, 0.f, 0.f}; }
__device__ __forceinline__ f32x4 rows_get4(const float* p, int i0) { return *reinterpret_cast<const f32x4*>(p + i0); }     // 16-byte aligned
__device__ __forceinline__ void rows_put(std::nullptr_t, int, float) {}
__device__ __forceinline__ void rows_put(float* p, int i, float v) { p[i] = v; }
__device__ __forceinline__ void rows_put4(std::nullptr_t, int, const f32x4&) {}
__device__ __forceinline__ void rows_put4(float* p, int i0, const f32x4& v) { *reinterpret_cast<f32x4*>(p + i0) = v; }
__device__ __forceinline__ int rows_head(std::nullptr_t, int) { return -1; }                                                // (sits like any row)
// an output row that is stored (add == 0) or added to
struct rows_accumulate {
  float* p;
  int add;
};
__device__ __forceinline__ void rows_put(rows_accumulate o, int i, float v) { o.p[i] = o.add ? o.p[i] + v : v; }
__device__ __forceinline__ void rows_put4(rows_accumulate o, int i0, f32x4 v) {
  if (o.add) {
    const f32x4 o4 = rows_get4(o.p, i0);
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = o4[c] + v[c];
  }
  rows_put4(o.p, i0, v);
}
__device__ __forceinline__ int rows_head(rows_accumulate o, int V) { return rows_head(o.p, V); }

// Thread tid of ROWS_T visits its elements of up to three rows of V floats in ascending order: a and b are read (a with its noise),
// f(i, a_i, b_i) is stored to out; out may be a or b.  Rows that sit alike against 16 bytes: scalar head, 16-byte body (UNROLL
// iterations unrolled), scalar tail; else 4-byte accesses over the whole row.  DEEP (a alone is read): four 16-byte loads in flight
// per thread - for an f that is a dependent chain (the online update), where the plain loop waits for every load; the elements are
// consumed in ascending order either way, so a thread's sums do not depend on it.
template <int UNROLL, bool DEEP = false, class A, class B, class O, class NOISE, class F>
__device__ __forceinline__ void rows_walk(int tid, int V, A a, B b, O out, const NOISE& noise, F f) {
  const auto one = [=](int i) {
    float av = rows_get(a, i);
    const float bv = rows_get(b, i);                       // (both loads in front of the draw: its arithmetic hides them)
    noise.add(av, i);
    rows_put(out, i, f(i, av, bv));
  };
  const int ha = rows_head(a, V), hb = rows_head(b, V), ho = rows_head(out, V);
  const int head = ha >= 0 ? ha : ho, nvec = (V - head) >> 2, tail0 = head + 4 * nvec;
  if ((hb >= 0 && hb != head) || (ho >= 0 && ho != head)) {
    for (int i = tid; i < V; i += ROWS_T) one(i);
    return;
  }
  const auto four = [=](int q, f32x4 a4) {
    const int i0 = head + 4 * q;
    const f32x4 b4 = rows_get4(b, i0);
    noise.add(a4, i0);
    f32x4 r4;
#pragma unroll
    for (int c = 0; c < 4; ++c) r4[c] = f(i0 + c, a4[c], b4[c]);
    rows_put4(out, i0, r4);
  };
  if (tid < head) one(tid);
  int q = tid;
  if (DEEP) {
    for (; q + 3 * ROWS_T < nvec; q += 4 * ROWS_T) {
      f32x4 a4[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) a4[u] = rows_get4(a, head + 4 * (q + u * ROWS_T));
#pragma unroll
      for (int u = 0; u < 4; ++u) four(q + u * ROWS_T, a4[u]);
    }
  }
#pragma unroll UNROLL
  for (; q < nvec; q += ROWS_T) four(q, rows_get4(a, head + 4 * q));
  if (tail0 + tid < V) one(tail0 + tid);
}

template <int UNROLL, bool DEEP = false, class A, class B, class O, class F>
__device__ __forceinline__ void rows_walk(int tid, int V, A a, B b, O out, F f) {
  rows_walk<UNROLL, DEEP>(tid, V, a, b, out, rows_noise<false>{}, f);
}

// ---- one online accumulator ------------------------------------------------------------------------------------------------------------
// Of the elements z a thread has taken: m = their maximum, s = sum exp(z - m); INDEX: mi = the first index of the maximum (a thread's
// indices ascend); WSUM: d = sum exp(z - m) * g.  merge() leaves the workgroup's (m, s[, mi][, d]) in every thread.
template <bool INDEX, bool WSUM>
struct rows_online {
  float m = -INFINITY, s = 0.f, d = 0.f;
  int mi = 0x7fffffff;

  __device__ __forceinline__ void take(float z, int idx = 0, float g = 0.f) {
    if (z > m) {
      const float c = expf(m - z);                          // (first element: exp(-inf) = 0, s = 0 * 0 + 1)
      s = s * c + 1.f;
      if (WSUM) d = d * c + g;
      m = z;
      if (INDEX) mi = idx;
    } else {
      const float e = expf(z - m);
      s += e;
      if (WSUM) d += e * g;
    }
  }

  // Wave, then the ROWS_T / 64 waves through LDS, in a fixed order.  A thread or wave without elements (short rows: V < 4 * ROWS_T)
  // holds (m, s, d) = (-inf, 0, 0) and adds nothing - tested (the short streaming rows of tests/test_xent_gpu.py and
  // tests/test_relax_gpu.py), since -inf - -inf is NaN where a whole wave is empty.  Holds the workgroup's one barrier.
  __device__ __forceinline__ void merge() {
    constexpr int NW = ROWS_T / 64;
    __shared__ float red_m[NW], red_s[NW], red_d[WSUM ? NW : 1];
    __shared__ int red_i[INDEX ? NW : 1];
    const int tid = threadIdx.x;
    float wm = m;
    int wi = mi;
    if (INDEX) wave_argmax(wm, wi);
    else wm = wave_max(m);
    // (the guard sits on the product, or - WSUM - on the factor: s * f contracts with the first addition of wave_sum, the guarded
    //  product does not, and every kernel keeps the bits it had)
    const float f = m == -INFINITY ? 0.f : expf(m - wm);
    const float ws = wave_sum(WSUM ? s * f : (m == -INFINITY ? 0.f : s * expf(m - wm)));
    const float wd = WSUM ? wave_sum(d * f) : 0.f;
    if ((tid & 63) == 0) {
      red_m[tid >> 6] = wm;
      red_s[tid >> 6] = ws;
      if (WSUM) red_d[tid >> 6] = wd;
      if (INDEX) red_i[tid >> 6] = wi;
    }
    __syncthreads();
    if (INDEX) {
      lds_argmax(red_m, red_i, NW, m, mi);
    } else {
      m = red_m[0];
      for (int w = 1; w < NW; ++w) m = fmaxf(m, red_m[w]);
    }
    s = 0.f;
    d = 0.f;
    for (int w = 0; w < NW; ++w)
      if (red_m[w] != -INFINITY) {
        const float c = expf(red_m[w] - m);
        s += red_s[w] * c;
        if (WSUM) d += red_d[w] * c;
      }
  }
};

// ---- one resident softmax ----------------------------------------------------------------------------------------------------------------
// v[i] = softmax(z)[lane + 64 i] of the wave's row, z_idx = load(i, idx) called for idx < V; 0 behind the row
template <class LOAD>
__device__ __forceinline__ void rows_resident_softmax(float (&v)[ROWS_NPER], int lane, int V, LOAD load) {
  float m = -INFINITY;
#pragma unroll
  for (int i = 0; i < ROWS_NPER; ++i) {
    const int idx = lane + 64 * i;
    v[i] = -INFINITY;
    if (idx < V) v[i] = load(i, idx);
    m = fmaxf(m, v[i]);
  }
  m = wave_max(m);
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < ROWS_NPER; ++i) {
    v[i] = lane + 64 * i < V ? expf(v[i] - m) : 0.f;
    s += v[i];
  }
  s = wave_sum(s);
  const float inv = 1.f / s;
#pragma unroll
  for (int i = 0; i < ROWS_NPER; ++i) v[i] *= inv;
}
