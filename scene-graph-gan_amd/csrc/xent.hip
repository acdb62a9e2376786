// Generator likelihood: softmax cross-entropy of the decoder rows, forward and gradient, its summary, and the log-probability of given
// triples under the mixture of an image's noise samples (gfx950).  The arithmetic of a row is that of csrc/kbest.hip:
//     lse = max + log(sum exp(x - max)),   a(x_j) = x_j - lse,   lp(s, p, o) = (a_0(s) + a_1(p)) + a_2(o)
//   softmax_xent  two decompositions by the row length (both bandwidth-bound; rows need not be 16-byte aligned):
//       V <= 1024   one wave per row, the row RESIDENT in 16 registers per lane: one read of the logits (4-byte coalesced loads: any
//                   alignment), maximum / argmax and the sum by wave shuffles, the gradient from the registers.  The workload's
//                   V = 1000 rows (4 KB) are here.  One row per workgroup up to 1024 rows (a step's 192 rows then spread over 192
//                   CUs), four rows per workgroup above (evaluation passes); the arithmetic of a row does not depend on it.
//       V >  1024   one 1024-thread workgroup per row.  Pass 1 is an ONLINE maximum / sum (a thread rescales its sum when its maximum
//                   grows), so the row is read once for lse, nll and hit; pass 2 re-reads the row for the gradient.  Where that read is
//                   served from has not been measured: one 280 KB row (V = 70 000) fits an XCD's 4 MiB L2, the ~24 rows an XCD
//                   works on at once at batch 64 (6.7 MB) do not, so part of it comes from the Infinity Cache or HBM.  16-byte loads and stores on the aligned body of the row, a scalar peel
//                   in front and behind; where the logits row and the gradient row are misaligned differently, pass 2 is scalar.
//   xent_summary  one workgroup: mean nll per valid row (fp64 sum), token and triple accuracy, number of valid rows.
//   triple_logp   one workgroup per image, one thread per ground-truth row, two loops over the N samples (kbest_merge's score).
// No float atomics, no workspace; every sum has a fixed order for given pointers and shapes: two calls give the same bits.
#include "sgg_common.h"

#define XENT_MAX_V (1 << 21)
#define XENT_SMALL_V 1024                       // rows up to here are register-resident
#define XENT_NPER (XENT_SMALL_V / 64)           // elements per lane of a resident row
#define XENT_SPREAD_R 1024                      // resident rows: up to this many, one row per workgroup; above, four
#define XENT_T 1024                             // threads of a streaming workgroup
#define XENT_NAN __uint_as_float(0x7fc00000u)

// (value, index) maximum over a wave; on equal values the smaller index wins (tf.argmax, sgg_argmax_rows)
__device__ __forceinline__ void xent_wave_argmax(float& m, int& mi) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o, 64);
    const int oi = __shfl_xor(mi, o, 64);
    if (om > m || (om == m && oi < mi)) { m = om; mi = oi; }
  }
}

__global__ __launch_bounds__(256) void xent_rows_resident_kernel(const float* __restrict__ logits, long long ld, int R, int V,
                                                                 const long long* __restrict__ labels, float scale, int accumulate,
                                                                 float* __restrict__ dlogits, long long ldd, float* __restrict__ nll,
                                                                 float* __restrict__ lse_out, int* __restrict__ hit) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);     // blockDim.x / 64 rows per workgroup
  if (row >= R) return;                                   // (no barrier in this kernel: waves are independent)
  const float* x = logits + (size_t)row * (size_t)ld;
  float v[XENT_NPER];
  float m = -INFINITY;
  int mi = 0x7fffffff;
#pragma unroll
  for (int i = 0; i < XENT_NPER; ++i) {
    const int idx = lane + 64 * i;
    v[i] = idx < V ? x[idx] : -INFINITY;
    if (v[i] > m) { m = v[i]; mi = idx; }                 // a lane's indices ascend: the first of equal values stays
  }
  xent_wave_argmax(m, mi);
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < XENT_NPER; ++i)
    if (lane + 64 * i < V) s += expf(v[i] - m);
  s = wave_sum(s);
  const float lse = m + logf(s);
  const long long lab = labels ? labels[row] : -1;
  const bool valid = labels && lab >= 0 && lab < V;
  if (lane == 0) {
    if (lse_out) lse_out[row] = lse;
    if (nll) nll[row] = valid ? lse - x[lab] : 0.f;
    if (hit) hit[row] = valid ? (int)(lab == (long long)mi) : -1;
  }
  if (!dlogits || (!valid && accumulate)) return;
  float* d = dlogits + (size_t)row * (size_t)ldd;
#pragma unroll
  for (int i = 0; i < XENT_NPER; ++i) {
    const int idx = lane + 64 * i;
    if (idx >= V) continue;
    const float g = valid ? scale * (expf(v[i] - lse) - (idx == (int)lab ? 1.f : 0.f)) : 0.f;
    d[idx] = accumulate ? d[idx] + g : g;
  }
}

// online maximum / sum of one thread: s = sum exp(x - m) over the elements seen so far, mi = the first index of the maximum
__device__ __forceinline__ void xent_online(float xv, int idx, float& m, float& s, int& mi) {
  if (xv > m) {
    s = s * expf(m - xv) + 1.f;                           // (first element: 0 * exp(-inf) + 1)
    m = xv;
    mi = idx;
  } else {
    s += expf(xv - m);
  }
}

// elements in front of the first 16-byte boundary of a row
__device__ __forceinline__ int xent_head(const float* p, int V) {
  const int h = (int)((4u - (unsigned)((reinterpret_cast<uintptr_t>(p) >> 2) & 3u)) & 3u);
  return h < V ? h : V;
}

__global__ __launch_bounds__(XENT_T) void xent_rows_stream_kernel(const float* __restrict__ logits, long long ld, int V,
                                                                  const long long* __restrict__ labels, float scale, int accumulate,
                                                                  float* __restrict__ dlogits, long long ldd, float* __restrict__ nll,
                                                                  float* __restrict__ lse_out, int* __restrict__ hit) {
  __shared__ float red_m[XENT_T / 64], red_s[XENT_T / 64];
  __shared__ int red_i[XENT_T / 64];
  const int tid = threadIdx.x;
  const size_t row = blockIdx.x;
  const float* x = logits + row * (size_t)ld;
  const int head = xent_head(x, V), nvec = (V - head) >> 2, tail0 = head + 4 * nvec;
  // ---- pass 1: one read of the row -----------------------------------------------------------------------------------------
  float m = -INFINITY, s = 0.f;
  int mi = 0x7fffffff;
  if (tid < head) xent_online(x[tid], tid, m, s, mi);
  // four 16-byte loads in flight per thread (the online update is a dependent chain: without them the loop waits for every load);
  // the elements are consumed in ascending order either way, so the sums do not depend on the unrolling
  const f32x4* xb = reinterpret_cast<const f32x4*>(x + head);
  int q = tid;
  for (; q + 3 * XENT_T < nvec; q += 4 * XENT_T) {
    f32x4 v4[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v4[u] = xb[q + u * XENT_T];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i0 = head + 4 * (q + u * XENT_T);
#pragma unroll
      for (int c = 0; c < 4; ++c) xent_online(v4[u][c], i0 + c, m, s, mi);
    }
  }
  for (; q < nvec; q += XENT_T) {
    const f32x4 v4 = xb[q];
    const int i0 = head + 4 * q;
#pragma unroll
    for (int c = 0; c < 4; ++c) xent_online(v4[c], i0 + c, m, s, mi);
  }
  if (tail0 + tid < V) xent_online(x[tail0 + tid], tail0 + tid, m, s, mi);
  // wave, then workgroup, in a fixed order; a thread or wave without elements (short rows: V < 4 * XENT_T) holds (m, s) = (-inf, 0)
  // and adds nothing - tested, since -inf - -inf is NaN where a whole wave is empty
  float wm = m;
  int wi = mi;
  xent_wave_argmax(wm, wi);
  const float ws = wave_sum(m == -INFINITY ? 0.f : s * expf(m - wm));
  if ((tid & 63) == 0) { red_m[tid >> 6] = wm; red_s[tid >> 6] = ws; red_i[tid >> 6] = wi; }
  __syncthreads();
  float bm = red_m[0];
  int bi = red_i[0];
  for (int w = 1; w < XENT_T / 64; ++w)
    if (red_m[w] > bm || (red_m[w] == bm && red_i[w] < bi)) { bm = red_m[w]; bi = red_i[w]; }
  float bs = 0.f;
  for (int w = 0; w < XENT_T / 64; ++w)
    if (red_m[w] != -INFINITY) bs += red_s[w] * expf(red_m[w] - bm);
  const float lse = bm + logf(bs);
  const long long lab = labels ? labels[row] : -1;
  const bool valid = labels && lab >= 0 && lab < V;
  if (tid == 0) {
    if (lse_out) lse_out[row] = lse;
    if (nll) nll[row] = valid ? lse - x[lab] : 0.f;
    if (hit) hit[row] = valid ? (int)(lab == (long long)bi) : -1;
  }
  if (!dlogits || (!valid && accumulate)) return;
  // ---- pass 2: the gradient; the row is read a second time (from whichever cache still holds it) -----------------------------------
  float* d = dlogits + row * (size_t)ldd;
  if (!valid) {                                            // skipped row, stored: zeros
    for (int i = tid; i < V; i += XENT_T) d[i] = 0.f;
    return;
  }
  const int il = (int)lab;
  if (xent_head(d, V) != head) {                           // the two rows sit differently against 16 bytes: 4-byte accesses
    for (int i = tid; i < V; i += XENT_T) {
      const float g = scale * (expf(x[i] - lse) - (i == il ? 1.f : 0.f));
      d[i] = accumulate ? d[i] + g : g;
    }
    return;
  }
  if (tid < head) {
    const float g = scale * (expf(x[tid] - lse) - (tid == il ? 1.f : 0.f));
    d[tid] = accumulate ? d[tid] + g : g;
  }
#pragma unroll 4
  for (int q = tid; q < nvec; q += XENT_T) {          // (independent iterations: the unrolled loads overlap)
    const int i0 = head + 4 * q;
    const f32x4 v4 = *reinterpret_cast<const f32x4*>(x + i0);
    f32x4 g4;
#pragma unroll
    for (int c = 0; c < 4; ++c) g4[c] = scale * (expf(v4[c] - lse) - (i0 + c == il ? 1.f : 0.f));
    if (accumulate) {
      const f32x4 o4 = *reinterpret_cast<const f32x4*>(d + i0);
#pragma unroll
      for (int c = 0; c < 4; ++c) g4[c] = o4[c] + g4[c];
    }
    *reinterpret_cast<f32x4*>(d + i0) = g4;
  }
  if (tail0 + tid < V) {
    const int i = tail0 + tid;
    const float g = scale * (expf(x[i] - lse) - (i == il ? 1.f : 0.f));
    d[i] = accumulate ? d[i] + g : g;
  }
}

// ---- the numbers of a log line ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void xent_summary_kernel(const float* __restrict__ nll, const int* __restrict__ hit, int R,
                                                           float* __restrict__ out4) {
  __shared__ double s_sum[256];
  __shared__ int s_cnt[4][256];                            // valid rows, hit rows, all-valid triples, all-hit triples
  const int tid = threadIdx.x;
  double sum = 0.0;
  int c[4] = {0, 0, 0, 0};
  for (int g = tid; g < R / 3; g += 256) {
    int nv = 0, nh = 0;
    for (int t = 0; t < 3; ++t) {
      const int h = hit[3 * (size_t)g + t];
      if (h >= 0) {
        ++nv;
        nh += (h == 1);
        sum += (double)nll[3 * (size_t)g + t];
      }
    }
    c[0] += nv;
    c[1] += nh;
    c[2] += (nv == 3);
    c[3] += (nv == 3 && nh == 3);
  }
  s_sum[tid] = sum;
  for (int k = 0; k < 4; ++k) s_cnt[k][tid] = c[k];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {                      // fixed tree
    if (tid < o) {
      s_sum[tid] += s_sum[tid + o];
      for (int k = 0; k < 4; ++k) s_cnt[k][tid] += s_cnt[k][tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const int valid = s_cnt[0][0], triples = s_cnt[2][0];
    out4[0] = valid ? (float)(s_sum[0] / (double)valid) : 0.f;
    out4[1] = valid ? (float)((double)s_cnt[1][0] / (double)valid) : 0.f;
    out4[2] = triples ? (float)((double)s_cnt[3][0] / (double)triples) : 0.f;
    out4[3] = (float)valid;
  }
}

// ---- log-probability of given triples under the mixture of the N samples ------------------------------------------------------------
__global__ __launch_bounds__(256) void triple_logp_kernel(const float* __restrict__ logits, long long ld, const float* __restrict__ lse,
                                                          int N, int nb, int V, const long long* __restrict__ gt,
                                                          const int* __restrict__ gt_count, int M, float* __restrict__ mix,
                                                          float* __restrict__ mean, float* __restrict__ slot, int* __restrict__ status) {
  const int j = blockIdx.x;
  int cnt = gt_count[j];
  cnt = cnt < 0 ? 0 : (cnt > M ? M : cnt);
  const float log_n = logf((float)N), inv_n = 1.f / (float)N;
  for (int mrow = threadIdx.x; mrow < M; mrow += 256) {
    const size_t o = (size_t)j * M + mrow;
    int st = 0;
    long long t0 = 0, t1 = 0, t2 = 0;
    if (mrow >= cnt) {
      st = -3;
    } else {
      t0 = gt[o * 3]; t1 = gt[o * 3 + 1]; t2 = gt[o * 3 + 2];
      if (!(t0 >= 0 && t0 < V && t1 >= 0 && t1 < V && t2 >= 0 && t2 < V)) st = -4;
    }
    status[o] = st;
    if (st != 0) {
      mix[o] = XENT_NAN; mean[o] = XENT_NAN;
      slot[o * 3] = XENT_NAN; slot[o * 3 + 1] = XENT_NAN; slot[o * 3 + 2] = XENT_NAN;
      continue;
    }
    float mx = -INFINITY, sum_lp = 0.f, sa0 = 0.f, sa1 = 0.f, sa2 = 0.f;
    for (int k = 0; k < N; ++k) {
      const size_t r = (size_t)k * nb + j;
      const float* x = logits + r * (size_t)ld;
      const float* z = lse + r * 3;
      const float a0 = x[t0] - z[0], a1 = x[(size_t)V + t1] - z[1], a2 = x[2 * (size_t)V + t2] - z[2];
      const float lp = (a0 + a1) + a2;
      if (lp > mx) mx = lp;
      sum_lp += lp;
      sa0 += a0; sa1 += a1; sa2 += a2;
    }
    float sum = 0.f;
    for (int k = 0; k < N; ++k) {
      const size_t r = (size_t)k * nb + j;
      const float* x = logits + r * (size_t)ld;
      const float* z = lse + r * 3;
      const float lp = ((x[t0] - z[0]) + (x[(size_t)V + t1] - z[1])) + (x[2 * (size_t)V + t2] - z[2]);
      sum += expf(lp - mx);
    }
    mix[o] = mx + (logf(sum) - log_n);
    mean[o] = sum_lp * inv_n;
    slot[o * 3] = sa0 * inv_n; slot[o * 3 + 1] = sa1 * inv_n; slot[o * 3 + 2] = sa2 * inv_n;
  }
}

extern "C" int sgg_softmax_xent(const float* logits, long long ld, int R, int V, const long long* labels, float scale, int accumulate,
                                float* dlogits, long long ldd, float* nll, float* lse, int* hit, void* stream) {
  SGG_CHECK_ARG(R >= 1 && V >= 1 && V <= XENT_MAX_V, "sgg_softmax_xent: R >= 1 and 1 <= V <= 2^21 (got R = %d, V = %d)", R, V);
  SGG_CHECK_ARG(logits && ld >= V, "sgg_softmax_xent: logits with a row stride ld >= V (got ld = %lld, V = %d)", ld, V);
  SGG_CHECK_ARG(labels || (!dlogits && !nll && !hit), "sgg_softmax_xent: labels = NULL is the lse-only mode: dlogits, nll and hit must be NULL");
  SGG_CHECK_ARG(!dlogits || ldd >= V, "sgg_softmax_xent: dlogits needs a row stride ldd >= V (got ldd = %lld, V = %d)", ldd, V);
  SGG_CHECK_ARG(dlogits || nll || lse || hit, "sgg_softmax_xent: no output");
  SGG_CHECK_ARG(accumulate == 0 || accumulate == 1, "sgg_softmax_xent: accumulate is 0 or 1 (got %d)", accumulate);
  if (V <= XENT_SMALL_V) {
    // a wave per row either way; up to XENT_SPREAD_R rows (the 192 of a batch-64 step) every row gets a workgroup of its own, so that the
    // rows spread over the CUs instead of sharing 48 of the 256; above, four rows per workgroup
    const int wg_rows = R <= XENT_SPREAD_R ? 1 : 4;
    hipLaunchKernelGGL(xent_rows_resident_kernel, dim3(sgg_cdiv(R, wg_rows)), dim3(64 * wg_rows), 0, (hipStream_t)stream, logits, ld, R, V,
                       labels, scale, accumulate, dlogits, ldd, nll, lse, hit);
  } else
    hipLaunchKernelGGL(xent_rows_stream_kernel, dim3(R), dim3(XENT_T), 0, (hipStream_t)stream, logits, ld, V, labels, scale, accumulate,
                       dlogits, ldd, nll, lse, hit);
  SGG_LAUNCH_CHECK("sgg_softmax_xent");
  return SGG_OK;
}

extern "C" int sgg_xent_summary(const float* nll, const int* hit, int R, float* out4, void* stream) {
  SGG_CHECK_ARG(R >= 3 && R % 3 == 0, "sgg_xent_summary: R = 3 B rows, one group of three per triple (got R = %d)", R);
  SGG_CHECK_ARG(nll && hit && out4, "sgg_xent_summary: null pointer");
  hipLaunchKernelGGL(xent_summary_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, nll, hit, R, out4);
  SGG_LAUNCH_CHECK("sgg_xent_summary");
  return SGG_OK;
}

extern "C" int sgg_triple_logp(const float* logits, long long ld, const float* lse, int N, int nb, int V, const long long* gt,
                               const int* gt_count, int M, float* mix, float* mean, float* slot, int* status, void* stream) {
  SGG_CHECK_ARG(N >= 1 && N <= 4096 && M >= 1 && M <= 4096, "sgg_triple_logp: 1 <= N <= 4096 and 1 <= M <= 4096 (got N = %d, M = %d)", N, M);
  SGG_CHECK_ARG(nb >= 1 && V >= 1 && V <= XENT_MAX_V, "sgg_triple_logp: nb >= 1 and 1 <= V <= 2^21 (got nb = %d, V = %d)", nb, V);
  SGG_CHECK_ARG(ld >= 3LL * V, "sgg_triple_logp: row stride ld >= 3 V (got ld = %lld, V = %d)", ld, V);
  SGG_CHECK_ARG(logits && lse && gt && gt_count && mix && mean && slot && status, "sgg_triple_logp: null pointer");
  hipLaunchKernelGGL(triple_logp_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, logits, ld, lse, N, nb, V, gt, gt_count, M, mix,
                     mean, slot, status);
  SGG_LAUNCH_CHECK("sgg_triple_logp");
  return SGG_OK;
}
