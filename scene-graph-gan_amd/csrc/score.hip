// Score-function (REINFORCE) generator update: the policy gradient of sampled triples (gfx950).  The generator's decoder rows x are a
// policy p = softmax(x); a token a was sampled from it (sgg_relax_rows_hard with tok and Gumbel noise), the critic scored the sample,
// and the update needs no gradient through the critic:
//     score_advantage  one workgroup: reward r_b = mean_t D(sample b), advantage A_b = r_b or r_b - mean of the OTHER rewards
//     score_rows       dx_j = w (p_j - [j == a]) + ent_coef p_j ((x_j - lse) + H),  w = coef * A,  H = lse - sum_j p_j x_j:
//                      the gradient of -w log p_a - ent_coef H by x; logp = x_a - lse and H beside it
//     score_summary    one workgroup: mean logp, mean H
// score_rows takes the two decompositions of csrc/softmax_rows.h with the arithmetic of csrc/xent.hip (p_j = exp(x_j - lse)): resident
// rows reduce (max, sum exp, sum exp * (x - max)) by wave shuffles; streamed rows take ONE online pass for (m, s, sum exp(x - m) x) and a
// second pass that re-reads x and writes dx (no second pass without dx).  The token is read once per row and range-checked; no load or
// store is addressed by it: x_a is kept by the thread that meets index a in its traversal, which also writes logp.
// No float atomics, no workspace; every sum has a fixed order for given pointers and shapes: two calls give the same bits.
#include "softmax_rows.h"

#include <cmath>

#define SCORE_MAX_B (1 << 20)
#define SCORE_MAX_T 64
#define SCORE_MAX_R (1 << 24)
#define SCORE_RT 256                            // threads of the one-workgroup kernels

// ---- one-workgroup fp64 sums in index order -----------------------------------------------------------------------------------------
// Thread t of SCORE_RT owns the contiguous indices [t * chunk, (t + 1) * chunk) and sums them ascending; thread 0 then adds the
// SCORE_RT partial sums ascending: the sum runs in index order (n <= SCORE_RT: one index per thread, the plain sequential sum).
__device__ __forceinline__ double score_ordered_sum(double part, double* red) {
  const int tid = threadIdx.x;
  __syncthreads();                                          // (red may still be read from the sum before)
  red[tid] = part;
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int t = 0; t < SCORE_RT; ++t) s += red[t];
    red[SCORE_RT] = s;
  }
  __syncthreads();
  return red[SCORE_RT];
}

__device__ __forceinline__ float score_reward(const float* __restrict__ d_out, long long ldd, int b, int T) {
  const float* row = d_out + (size_t)b * (size_t)ldd;
  float r = 0.f;
  for (int t = 0; t < T; ++t) r += row[t];
  return r / (float)T;
}

__global__ __launch_bounds__(SCORE_RT) void score_advantage_kernel(const float* __restrict__ d_out, long long ldd, int B, int T, int baseline,
                                                                   float* __restrict__ adv, float* __restrict__ out2) {
  __shared__ double red[SCORE_RT + 1];
  const int tid = threadIdx.x;
  const int chunk = (B + SCORE_RT - 1) / SCORE_RT;
  const int b0 = tid * chunk < B ? tid * chunk : B, b1 = b0 + chunk < B ? b0 + chunk : B;
  double part = 0.0;
  for (int b = b0; b < b1; ++b) part += (double)score_reward(d_out, ldd, b, T);
  const double S = score_ordered_sum(part, red);
  part = 0.0;
  for (int b = b0; b < b1; ++b) {
    const double r = (double)score_reward(d_out, ldd, b, T);        // (the same fp32 sum: the same bits)
    const float a = baseline ? (float)(r - (S - r) / (double)(B - 1)) : (float)r;
    adv[b] = a;
    part += (double)a * (double)a;
  }
  if (!out2) return;                                        // (uniform)
  const double Q = score_ordered_sum(part, red);
  if (tid == 0) {
    out2[0] = (float)(S / (double)B);
    out2[1] = (float)(Q / (double)B);
  }
}

__global__ __launch_bounds__(SCORE_RT) void score_summary_kernel(const float* __restrict__ logp, const float* __restrict__ ent, int R,
                                                                 float* __restrict__ out2) {
  __shared__ double red[SCORE_RT + 1];
  const int tid = threadIdx.x;
  const int chunk = (R + SCORE_RT - 1) / SCORE_RT;
  const int r0 = tid * chunk < R ? tid * chunk : R, r1 = r0 + chunk < R ? r0 + chunk : R;
  double pl = 0.0, pe = 0.0;
  for (int r = r0; r < r1; ++r) {
    pl += (double)logp[r];
    pe += (double)ent[r];
  }
  const double L = score_ordered_sum(pl, red);
  const double E = score_ordered_sum(pe, red);
  if (tid == 0) {
    out2[0] = (float)(L / (double)R);
    out2[1] = (float)(E / (double)R);
  }
}

// ---- the rows ------------------------------------------------------------------------------------------------------------------------
// what a row's threads need once (lse, H) are known: dx_j from x_j
struct score_row {
  float w, ent_coef, lse, H;
  int a;                                                    // the sampled token (valid rows only)
  __device__ __forceinline__ float dx(int j, float xv) const {
    const float t = xv - lse, p = expf(t);
    return w * (p - (j == a ? 1.f : 0.f)) + ent_coef * p * (t + H);
  }
};

__global__ __launch_bounds__(256) void score_rows_resident_kernel(const float* __restrict__ x, long long ldx, int R, int V,
                                                                  const long long* __restrict__ tok, const float* __restrict__ adv, int group,
                                                                  float coef, float ent_coef, int accumulate, float* __restrict__ dx,
                                                                  long long lddx, float* __restrict__ logp, float* __restrict__ ent) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= R) return;
  const float* xr = x + (size_t)row * (size_t)ldx;
  const long long t = tok[row];
  const bool valid = t >= 0 && t < V;
  const int a = valid ? (int)t : -1;
  float v[ROWS_NPER];
  float m = -INFINITY, xa = 0.f;
  bool mine = false;
#pragma unroll
  for (int i = 0; i < ROWS_NPER; ++i) {
    const int idx = lane + 64 * i;
    v[i] = idx < V ? xr[idx] : -INFINITY;
    m = fmaxf(m, v[i]);
    if (idx == a) { xa = v[i]; mine = true; }
  }
  m = wave_max(m);
  float s = 0.f, d = 0.f;
#pragma unroll
  for (int i = 0; i < ROWS_NPER; ++i)
    if (lane + 64 * i < V) {
      const float c = v[i] - m, e = expf(c);
      s += e;
      d += e * c;
    }
  s = wave_sum(s);
  d = wave_sum(d);
  const float ls = logf(s), lse = m + ls;
  const float H = ls - d / s;                               // lse - sum p x with the maximum taken out of both terms
  if (ent && lane == 0) ent[row] = H;
  if (logp) {
    if (mine) logp[row] = xa - lse;
    if (!valid && lane == 0) logp[row] = 0.f;
  }
  if (!dx || (!valid && accumulate)) return;
  float* dr = dx + (size_t)row * (size_t)lddx;
  const score_row sr = {coef * (adv ? adv[row / group] : 1.f), ent_coef, lse, H, a};
#pragma unroll
  for (int i = 0; i < ROWS_NPER; ++i) {
    const int idx = lane + 64 * i;
    if (idx >= V) continue;
    const float g = valid ? sr.dx(idx, v[i]) : 0.f;
    dr[idx] = accumulate ? dr[idx] + g : g;
  }
}

__global__ __launch_bounds__(ROWS_T) void score_rows_stream_kernel(const float* __restrict__ x, long long ldx, int V,
                                                                   const long long* __restrict__ tok, const float* __restrict__ adv, int group,
                                                                   float coef, float ent_coef, int accumulate, float* __restrict__ dx,
                                                                   long long lddx, float* __restrict__ logp, float* __restrict__ ent) {
  const int tid = threadIdx.x;
  const size_t row = blockIdx.x;
  const float* xr = x + row * (size_t)ldx;
  const long long t = tok[row];
  const bool valid = t >= 0 && t < V;
  const int a = valid ? (int)t : -1;
  // ---- pass 1: one read of the row: the online triple (m, s, sum exp(x - m) x), and x_a in the thread that meets a --------------------
  rows_online<false, true> acc;
  float xa = 0.f;
  bool mine = false;
  rows_walk<1, true>(tid, V, xr, nullptr, nullptr, [&acc, &xa, &mine, a](int i, float xv, float) {
    acc.take(xv, 0, xv);
    if (i == a) { xa = xv; mine = true; }
    return 0.f;
  });
  acc.merge();
  const float lse = acc.m + logf(acc.s);
  const float H = lse - acc.d / acc.s;
  if (ent && tid == 0) ent[row] = H;
  if (logp) {
    if (mine) logp[row] = xa - lse;
    if (!valid && tid == 0) logp[row] = 0.f;
  }
  if (!dx || (!valid && accumulate)) return;
  // ---- pass 2: the gradient --------------------------------------------------------------------------------------------------------
  float* dr = dx + row * (size_t)lddx;
  if (!valid) {                                             // skipped row, stored: zeros
    for (int i = tid; i < V; i += ROWS_T) dr[i] = 0.f;
    return;
  }
  const score_row sr = {coef * (adv ? adv[row / (size_t)group] : 1.f), ent_coef, lse, H, a};
  rows_walk<4>(tid, V, xr, nullptr, rows_accumulate{dr, accumulate}, [=](int i, float xv, float) { return sr.dx(i, xv); });
}

// ---- entry points --------------------------------------------------------------------------------------------------------------------
extern "C" int sgg_score_advantage(const float* d_out, long long ldd, int B, int T, int baseline, float* adv, float* out2, void* stream) {
  SGG_CHECK_ARG(B >= 1 && B <= SCORE_MAX_B && T >= 1 && T <= SCORE_MAX_T, "sgg_score_advantage: 1 <= B <= 2^20 and 1 <= T <= 64 (got B = %d, T = %d)",
                B, T);
  SGG_CHECK_ARG(baseline == 0 || baseline == 1, "sgg_score_advantage: baseline is 0 (none) or 1 (leave-one-out) (got %d)", baseline);
  SGG_CHECK_ARG(baseline == 0 || B >= 2, "sgg_score_advantage: the leave-one-out baseline needs B >= 2 (got B = %d)", B);
  SGG_CHECK_ARG(d_out && adv, "sgg_score_advantage: null pointer");
  SGG_CHECK_ARG(ldd >= T, "sgg_score_advantage: row stride ldd >= T (got ldd = %lld, T = %d)", ldd, T);
  hipLaunchKernelGGL(score_advantage_kernel, dim3(1), dim3(SCORE_RT), 0, (hipStream_t)stream, d_out, ldd, B, T, baseline, adv, out2);
  SGG_LAUNCH_CHECK("sgg_score_advantage");
  return SGG_OK;
}

extern "C" int sgg_score_rows(const float* x, long long ldx, int R, int V, const long long* tok, const float* adv, int group, float coef,
                              float ent_coef, int accumulate, float* dx, long long lddx, float* logp, float* ent, void* stream) {
  SGG_CHECK_ARG(R >= 1 && V >= 1 && V <= ROWS_MAX_V, "sgg_score_rows: R >= 1 and 1 <= V <= 2^21 (got R = %d, V = %d)", R, V);
  SGG_CHECK_ARG(x && tok, "sgg_score_rows: null pointer (x, tok)");
  SGG_CHECK_ARG(ldx >= V && (!dx || lddx >= V), "sgg_score_rows: row strides ldx, lddx >= V (got ldx = %lld, lddx = %lld, V = %d)", ldx, lddx, V);
  SGG_CHECK_ARG(group >= 1, "sgg_score_rows: group >= 1 (got %d)", group);
  SGG_CHECK_ARG(std::isfinite(coef) && std::isfinite(ent_coef), "sgg_score_rows: coef and ent_coef must be finite (got %g, %g)", (double)coef,
                (double)ent_coef);
  SGG_CHECK_ARG(accumulate == 0 || accumulate == 1, "sgg_score_rows: accumulate is 0 or 1 (got %d)", accumulate);
  SGG_CHECK_ARG(dx || logp || ent, "sgg_score_rows: no output");
  SGG_CHECK_ARG((const float*)dx != x, "sgg_score_rows: dx must not alias x");
  hipStream_t st = (hipStream_t)stream;
  if (V <= ROWS_SMALL_V) {
    const rows_resident_geometry geo(R);
    hipLaunchKernelGGL(score_rows_resident_kernel, geo.grid, geo.block, 0, st, x, ldx, R, V, tok, adv, group, coef, ent_coef, accumulate, dx,
                       lddx, logp, ent);
  } else {
    hipLaunchKernelGGL(score_rows_stream_kernel, dim3(R), dim3(ROWS_T), 0, st, x, ldx, V, tok, adv, group, coef, ent_coef, accumulate, dx, lddx,
                       logp, ent);
  }
  SGG_LAUNCH_CHECK("sgg_score_rows");
  return SGG_OK;
}

extern "C" int sgg_score_summary(const float* logp, const float* ent, int R, float* out2, void* stream) {
  SGG_CHECK_ARG(R >= 1 && R <= SCORE_MAX_R, "sgg_score_summary: 1 <= R <= 2^24 (got R = %d)", R);
  SGG_CHECK_ARG(logp && ent && out2, "sgg_score_summary: null pointer");
  hipLaunchKernelGGL(score_summary_kernel, dim3(1), dim3(SCORE_RT), 0, (hipStream_t)stream, logp, ent, R, out2);
  SGG_LAUNCH_CHECK("sgg_score_summary");
  return SGG_OK;
}
