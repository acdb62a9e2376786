// Generator likelihood: softmax cross-entropy of the decoder rows, forward and gradient, its summary, and the log-probability of given
// triples under the mixture of an image's noise samples (gfx950).  The arithmetic of a row is that of csrc/kbest.hip:
//     lse = max + log(sum exp(x - max)),   a(x_j) = x_j - lse,   lp(s, p, o) = (a_0(s) + a_1(p)) + a_2(o)
//   softmax_xent  the two decompositions of csrc/softmax_rows.h (both bandwidth-bound): resident rows give maximum / argmax and the sum by
//                 wave shuffles and the gradient from the registers (the workload's V = 1000 rows, 4 KB, are here); streamed rows are
//                 read once for lse, nll and hit (pass 1) and a second time for the gradient (pass 2).
//   xent_summary  one workgroup: mean nll per valid row (fp64 sum), token and triple accuracy, number of valid rows.
//   triple_logp   one workgroup per image, one thread per ground-truth row, two loops over the N samples (kbest_merge's score).
// No float atomics, no workspace; every sum has a fixed order for given pointers and shapes: two calls give the same bits.
#include "softmax_rows.h"

#define XENT_NAN __uint_as_float(0x7fc00000u)

__global__ __launch_bounds__(256) void xent_rows_resident_kernel(const float* __restrict__ logits, long long ld, int R, int V,
                                                                 const long long* __restrict__ labels, float scale, int accumulate,
                                                                 float* __restrict__ dlogits, long long ldd, float* __restrict__ nll,
                                                                 float* __restrict__ lse_out, int* __restrict__ hit) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= R) return;
  const float* x = logits + (size_t)row * (size_t)ld;
  float v[ROWS_NPER];
  float m = -INFINITY;
  int mi = 0x7fffffff;
#pragma unroll
  for (int i = 0; i < ROWS_NPER; ++i) {
    const int idx = lane + 64 * i;
    v[i] = idx < V ? x[idx] : -INFINITY;
    if (v[i] > m) { m = v[i]; mi = idx; }                 // a lane's indices ascend: the first of equal values stays
  }
  wave_argmax(m, mi);
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < ROWS_NPER; ++i)
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
  for (int i = 0; i < ROWS_NPER; ++i) {
    const int idx = lane + 64 * i;
    if (idx >= V) continue;
    const float g = valid ? scale * (expf(v[i] - lse) - (idx == (int)lab ? 1.f : 0.f)) : 0.f;
    d[idx] = accumulate ? d[idx] + g : g;
  }
}

__global__ __launch_bounds__(ROWS_T) void xent_rows_stream_kernel(const float* __restrict__ logits, long long ld, int V,
                                                                  const long long* __restrict__ labels, float scale, int accumulate,
                                                                  float* __restrict__ dlogits, long long ldd, float* __restrict__ nll,
                                                                  float* __restrict__ lse_out, int* __restrict__ hit) {
  const int tid = threadIdx.x;
  const size_t row = blockIdx.x;
  const float* x = logits + row * (size_t)ld;
  // ---- pass 1: one read of the row -----------------------------------------------------------------------------------------
  rows_online<true, false> acc;
  rows_walk<1, true>(tid, V, x, nullptr, nullptr, [&acc](int i, float xv, float) {
    acc.take(xv, i);
    return 0.f;
  });
  acc.merge();
  const float lse = acc.m + logf(acc.s);
  const long long lab = labels ? labels[row] : -1;
  const bool valid = labels && lab >= 0 && lab < V;
  if (tid == 0) {
    if (lse_out) lse_out[row] = lse;
    if (nll) nll[row] = valid ? lse - x[lab] : 0.f;
    if (hit) hit[row] = valid ? (int)(lab == (long long)acc.mi) : -1;
  }
  if (!dlogits || (!valid && accumulate)) return;
  // ---- pass 2: the gradient ------------------------------------------------------------------------------------------------
  float* d = dlogits + row * (size_t)ldd;
  if (!valid) {                                            // skipped row, stored: zeros
    for (int i = tid; i < V; i += ROWS_T) d[i] = 0.f;
    return;
  }
  const int il = (int)lab;
  rows_walk<4>(tid, V, x, nullptr, rows_accumulate{d, accumulate}, [=](int i, float xv, float) {        // (independent iterations: the loads overlap)
    return scale * (expf(xv - lse) - (i == il ? 1.f : 0.f));
  });
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
  SGG_CHECK_ARG(R >= 1 && V >= 1 && V <= ROWS_MAX_V, "sgg_softmax_xent: R >= 1 and 1 <= V <= 2^21 (got R = %d, V = %d)", R, V);
  SGG_CHECK_ARG(logits && ld >= V, "sgg_softmax_xent: logits with a row stride ld >= V (got ld = %lld, V = %d)", ld, V);
  SGG_CHECK_ARG(labels || (!dlogits && !nll && !hit), "sgg_softmax_xent: labels = NULL is the lse-only mode: dlogits, nll and hit must be NULL");
  SGG_CHECK_ARG(!dlogits || ldd >= V, "sgg_softmax_xent: dlogits needs a row stride ldd >= V (got ldd = %lld, V = %d)", ldd, V);
  SGG_CHECK_ARG(dlogits || nll || lse || hit, "sgg_softmax_xent: no output");
  SGG_CHECK_ARG(accumulate == 0 || accumulate == 1, "sgg_softmax_xent: accumulate is 0 or 1 (got %d)", accumulate);
  if (V <= ROWS_SMALL_V) {
    const rows_resident_geometry geo(R);
    hipLaunchKernelGGL(xent_rows_resident_kernel, geo.grid, geo.block, 0, (hipStream_t)stream, logits, ld, R, V, labels, scale, accumulate,
                       dlogits, ldd, nll, lse, hit);
  } else
    hipLaunchKernelGGL(xent_rows_stream_kernel, dim3(R), dim3(ROWS_T), 0, (hipStream_t)stream, logits, ld, V, labels, scale, accumulate,
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
  SGG_CHECK_ARG(nb >= 1 && V >= 1 && V <= ROWS_MAX_V, "sgg_triple_logp: nb >= 1 and 1 <= V <= 2^21 (got nb = %d, V = %d)", nb, V);
  SGG_CHECK_ARG(ld >= 3LL * V, "sgg_triple_logp: row stride ld >= 3 V (got ld = %lld, V = %d)", ld, V);
  SGG_CHECK_ARG(logits && lse && gt && gt_count && mix && mean && slot && status, "sgg_triple_logp: null pointer");
  hipLaunchKernelGGL(triple_logp_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, logits, ld, lse, N, nb, V, gt, gt_count, M, mix,
                     mean, slot, status);
  SGG_LAUNCH_CHECK("sgg_triple_logp");
  return SGG_OK;
}
