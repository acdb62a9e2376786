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

// ======================================================================================================================================
// S samples per row (sgg_*_multi): S Gumbel-max samples of every row in one launch, advantages against the other samples of the SAME
// image, and one gradient launch for all of them.  Layout: sample s of logits row r sits at index s * R + r.
//     sample_rows_multi      sample s = the first argmax of x + g, g drawn at draw number draw | (s << 56): bit for bit the tok of
//                            sgg_relax_rows_hard(gumbel = 1) at that draw number.  Resident rows stay in registers for all S draws;
//                            a streamed row is read once per chunk of up to SCORE_CH samples, every thread holding one (best value,
//                            best index) pair per sample of the chunk (S <= 8: one read, S <= 16: two).  No one-hot row is written.
//     score_advantage_multi  one workgroup: r[s][b] = mean_t d_out[s * B + b][t]; none | leave-one-out over all S * B | over the other
//                            samples of image b
//     score_rows_multi       dx_j = (sum_s w_s) p_j - sum_s w_s [j == a_s] + ent_coef p_j ((x_j - lse) + H): the S tokens of a row are
//                            read once and held (uniform per row), the one-hot terms come from comparing j with them - a token sampled
//                            twice counts twice; a token outside [0, V) drops its own term only
//     score_summary_multi    one workgroup: mean logp over S * R, mean H over R
#define SCORE_MAX_S 16
#define SCORE_CH 8                              // samples of a streamed row drawn per read of the row

__host__ __device__ __forceinline__ relax_rng score_sample_rng(relax_rng rng, int s) {      // draw | (s << 56): bits 24 .. 31 of the high word
  rng.d1 |= (unsigned)s << 24;
  return rng;
}

__global__ __launch_bounds__(256) void sample_rows_multi_resident_kernel(const float* __restrict__ x, long long ldx, int R, int V, int S,
                                                                         relax_rng rng, long long* __restrict__ tok) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= R) return;
  const float* xr = x + (size_t)row * (size_t)ldx;
  float v[ROWS_NPER];
#pragma unroll
  for (int i = 0; i < ROWS_NPER; ++i) {
    const int idx = lane + 64 * i;
    v[i] = idx < V ? xr[idx] : -INFINITY;
  }
  for (int s = 0; s < S; ++s) {                             // the row stays in its registers: relax_hard_resident_kernel's draw, S times
    const rows_noise<true> noise = {score_sample_rng(rng, s), (unsigned)row, nullptr};
    float bv = -INFINITY;
    int bi = 0x7fffffff;
#pragma unroll
    for (int i = 0; i < ROWS_NPER; ++i) {
      const int idx = lane + 64 * i;
      if (idx < V) {
        float z = v[i];
        noise.add(z, idx);
        if (z > bv) { bv = z; bi = idx; }
      }
    }
    wave_argmax(bv, bi);
    if (lane == 0) tok[(size_t)s * (size_t)R + (size_t)row] = (long long)(bi < V ? bi : 0);
  }
}

// what rows_walk calls as the "noise" of an element: the CH draws of it, each into its sample's running (best value, best index).
// x itself is left alone.  bv / bi are the thread's own fully unrolled arrays (compile-time indices only: registers).
template <int CH>
struct score_draws {
  relax_rng rng;                                            // of sample s0
  unsigned row;
  int s0, S;
  float* bv;
  int* bi;
  __device__ __forceinline__ void add(float& xv, int idx) const {
#pragma unroll
    for (int c = 0; c < CH; ++c)
      if (s0 + c < S) {                                     // (uniform)
        float z = xv;
        rows_noise<true>{score_sample_rng(rng, c), row, nullptr}.add(z, idx);
        if (z > bv[c]) { bv[c] = z; bi[c] = idx; }
      }
  }
  __device__ __forceinline__ void add(f32x4& v4, int i0) const {
#pragma unroll
    for (int c = 0; c < CH; ++c)
      if (s0 + c < S) {
        f32x4 z4 = v4;
        rows_noise<true>{score_sample_rng(rng, c), row, nullptr}.add(z4, i0);
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (z4[e] > bv[c]) { bv[c] = z4[e]; bi[c] = i0 + e; }      // a thread's indices ascend: a strict >
      }
  }
};

template <int CH>
__global__ __launch_bounds__(ROWS_T) void sample_rows_multi_stream_kernel(const float* __restrict__ x, long long ldx, int R, int V, int S,
                                                                          relax_rng rng, long long* __restrict__ tok) {
  __shared__ float red_v[CH][ROWS_T / 64];
  __shared__ int red_i[CH][ROWS_T / 64];
  const int tid = threadIdx.x;
  const size_t row = blockIdx.x;
  for (int s0 = 0; s0 < S; s0 += CH) {                      // one read of the row per chunk of CH samples
    float bv[CH];
    int bi[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) { bv[c] = -INFINITY; bi[c] = 0x7fffffff; }
    // (s0 is a multiple of CH <= 8 and below 16: or-ing it in front of c gives s0 + c)
    const score_draws<CH> draws = {score_sample_rng(rng, s0), (unsigned)row, s0, S, bv, bi};
    rows_walk<1, true>(tid, V, x + row * (size_t)ldx, nullptr, nullptr, draws, [](int, float, float) { return 0.f; });
    if (s0) __syncthreads();                                // (the chunk before has read red_*)
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      wave_argmax(bv[c], bi[c]);
      if ((tid & 63) == 0) { red_v[c][tid >> 6] = bv[c]; red_i[c][tid >> 6] = bi[c]; }
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < CH; ++c)
      if (s0 + c < S) {
        lds_argmax(red_v[c], red_i[c], ROWS_T / 64, bv[c], bi[c]);
        if (tid == 0) tok[(size_t)(s0 + c) * (size_t)R + row] = (long long)(bi[c] < V ? bi[c] : 0);
      }
  }
}

// ---- advantages ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SCORE_RT) void score_advantage_multi_kernel(const float* __restrict__ d_out, long long ldd, int B, int S, int T,
                                                                         int baseline, float* __restrict__ adv, float* __restrict__ out2) {
  __shared__ double red[SCORE_RT + 1];
  const int tid = threadIdx.x;
  const int N = S * B;
  const int chunk = (N + SCORE_RT - 1) / SCORE_RT;
  const int n0 = tid * chunk < N ? tid * chunk : N, n1 = n0 + chunk < N ? n0 + chunk : N;
  double part = 0.0;
  for (int n = n0; n < n1; ++n) part += (double)score_reward(d_out, ldd, n, T);
  const double sum = score_ordered_sum(part, red);
  part = 0.0;
  for (int n = n0; n < n1; ++n) {
    const double r = (double)score_reward(d_out, ldd, n, T);        // (the same fp32 sum: the same bits)
    double a = r;
    if (baseline == 1) {
      a = r - (sum - r) / (double)(N - 1);
    } else if (baseline == 2) {
      const int b = n % B;
      double col = 0.0;                                     // the S rewards of image b, in order of s
      for (int s = 0; s < S; ++s) col += (double)score_reward(d_out, ldd, s * B + b, T);
      a = r - (col - r) / (double)(S - 1);
    }
    const float af = (float)a;
    adv[n] = af;
    part += (double)af * (double)af;
  }
  if (!out2) return;                                        // (uniform)
  const double Q = score_ordered_sum(part, red);
  if (tid == 0) {
    out2[0] = (float)(sum / (double)N);
    out2[1] = (float)(Q / (double)N);
  }
}

__global__ __launch_bounds__(SCORE_RT) void score_summary_multi_kernel(const float* __restrict__ logp, int n_logp, const float* __restrict__ ent,
                                                                       int n_ent, float* __restrict__ out2) {
  __shared__ double red[SCORE_RT + 1];
  const int tid = threadIdx.x;
  const int cl = (n_logp + SCORE_RT - 1) / SCORE_RT, ce = (n_ent + SCORE_RT - 1) / SCORE_RT;
  const int l0 = tid * cl < n_logp ? tid * cl : n_logp, l1 = l0 + cl < n_logp ? l0 + cl : n_logp;
  const int e0 = tid * ce < n_ent ? tid * ce : n_ent, e1 = e0 + ce < n_ent ? e0 + ce : n_ent;
  double pl = 0.0, pe = 0.0;
  for (int i = l0; i < l1; ++i) pl += (double)logp[i];
  for (int i = e0; i < e1; ++i) pe += (double)ent[i];
  const double L = score_ordered_sum(pl, red);
  const double E = score_ordered_sum(pe, red);
  if (tid == 0) {
    out2[0] = (float)(L / (double)n_logp);
    out2[1] = (float)(E / (double)n_ent);
  }
}

// ---- the rows ------------------------------------------------------------------------------------------------------------------------
// The NS (compile-time, >= S) samples of one row: token (-1: outside [0, V) or c >= S - it meets no index) and weight (0 then), and
// what a row's threads need once (lse, H) are known.  Uniform over the row's threads; compile-time indices only.
template <int NS>
struct score_row_multi {
  int a[NS];
  float w[NS];
  float W, ent_coef, lse, H;                                // W = sum of the valid samples' weights, in order of s

  // The loads of a row's S tokens, and of its S advantages, are issued side by side and their values used only behind all of them: a
  // load whose value is used inside the branch that guards it is waited for there, one memory latency per sample.
  __device__ __forceinline__ void load_tokens(const long long* __restrict__ tok, size_t row, int R, int V, int S) {
    long long t[NS];
#pragma unroll
    for (int c = 0; c < NS; ++c) {
      t[c] = -1;
      if (c < S) t[c] = tok[(size_t)c * (size_t)R + row];   // (uniform; nothing inside the branch waits for the load)
    }
#pragma unroll
    for (int c = 0; c < NS; ++c) a[c] = (c < S && t[c] >= 0 && t[c] < V) ? (int)t[c] : -1;
  }
  // ... behind load_tokens (adv null: every weight is coef)
  __device__ __forceinline__ void load_weights(const float* __restrict__ adv, size_t row, int R, int S, int group, float coef) {
    float r[NS];
    const size_t per = (size_t)(R / group), g0 = row / (size_t)group;
#pragma unroll
    for (int c = 0; c < NS; ++c) {
      r[c] = 1.f;
      if (adv && c < S) r[c] = adv[(size_t)c * per + g0];
    }
    W = 0.f;
#pragma unroll
    for (int c = 0; c < NS; ++c) {
      w[c] = a[c] >= 0 ? coef * r[c] : 0.f;
      W += w[c];
    }
  }
  __device__ __forceinline__ float dx(int j, float xv) const {
    const float t = xv - lse, p = expf(t);
    float hit = 0.f;
#pragma unroll
    for (int c = 0; c < NS; ++c) hit += j == a[c] ? w[c] : 0.f;
    return (W * p - hit) + ent_coef * p * (t + H);
  }
};

template <int NS>
__global__ __launch_bounds__(256) void score_rows_multi_resident_kernel(const float* __restrict__ x, long long ldx, int R, int V, int S,
                                                                        const long long* __restrict__ tok, const float* __restrict__ adv,
                                                                        int group, float coef, float ent_coef, int accumulate,
                                                                        float* __restrict__ dx, long long lddx, float* __restrict__ logp,
                                                                        float* __restrict__ ent) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= R) return;
  const float* xr = x + (size_t)row * (size_t)ldx;
  score_row_multi<NS> sr;
  sr.load_tokens(tok, (size_t)row, R, V, S);
  if (dx) sr.load_weights(adv, (size_t)row, R, S, group, coef);    // (uniform; the advantages' loads fly with the row's)
  float v[ROWS_NPER];
  float m = -INFINITY;
#pragma unroll
  for (int i = 0; i < ROWS_NPER; ++i) {
    const int idx = lane + 64 * i;
    v[i] = idx < V ? xr[idx] : -INFINITY;
    m = fmaxf(m, v[i]);
  }
  // x_a of each sample, in the lane that holds index a.  The wave's row, and so its tokens, are uniform: WHICH register holds a is a
  // scalar branch around one move, not a compare per element and sample.
  float xa[NS];
  bool me[NS];
#pragma unroll
  for (int c = 0; c < NS; ++c) {
    sr.a[c] = __builtin_amdgcn_readfirstlane(sr.a[c]);
    me[c] = (sr.a[c] & 63) == lane;
    xa[c] = 0.f;
#pragma unroll
    for (int i = 0; i < ROWS_NPER; ++i)
      if ((sr.a[c] >> 6) == i) xa[c] = v[i];                // (a = -1: no register)
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
#pragma unroll
    for (int c = 0; c < NS; ++c)
      if (c < S) {
        float* lp = logp + (size_t)c * (size_t)R + (size_t)row;
        if (sr.a[c] < 0) { if (lane == 0) *lp = 0.f; }
        else if (me[c]) *lp = xa[c] - lse;                  // the lane that holds a_c
      }
  }
  if (!dx) return;
  float* dr = dx + (size_t)row * (size_t)lddx;
  // the one-hot terms of a lane's elements, added in order of s as score_row_multi::dx adds them
  float hit[ROWS_NPER];
#pragma unroll
  for (int i = 0; i < ROWS_NPER; ++i) hit[i] = 0.f;
#pragma unroll
  for (int c = 0; c < NS; ++c) {
#pragma unroll
    for (int i = 0; i < ROWS_NPER; ++i)
      if ((sr.a[c] >> 6) == i) hit[i] += me[c] ? sr.w[c] : 0.f;
  }
#pragma unroll
  for (int i = 0; i < ROWS_NPER; ++i) {
    const int idx = lane + 64 * i;
    if (idx >= V) continue;
    const float t = v[i] - lse, p = expf(t);
    const float g = (sr.W * p - hit[i]) + ent_coef * p * (t + H);
    dr[idx] = accumulate ? dr[idx] + g : g;
  }
}

template <int NS>
__global__ __launch_bounds__(ROWS_T) void score_rows_multi_stream_kernel(const float* __restrict__ x, long long ldx, int R, int V, int S,
                                                                         const long long* __restrict__ tok, const float* __restrict__ adv,
                                                                         int group, float coef, float ent_coef, int accumulate,
                                                                         float* __restrict__ dx, long long lddx, float* __restrict__ logp,
                                                                         float* __restrict__ ent) {
  const int tid = threadIdx.x;
  const size_t row = blockIdx.x;
  const float* xr = x + row * (size_t)ldx;
  score_row_multi<NS> sr;
  sr.load_tokens(tok, row, R, V, S);
  // ---- pass 1: one read of the row: the online triple (m, s, sum exp(x - m) x), and x_a of each sample in the thread that meets it ----
  rows_online<false, true> acc;
  float xa[NS];
  bool mine[NS];
#pragma unroll
  for (int c = 0; c < NS; ++c) { xa[c] = 0.f; mine[c] = false; }
  rows_walk<1, true>(tid, V, xr, nullptr, nullptr, [&acc, &xa, &mine, &sr](int i, float xv, float) {
    acc.take(xv, 0, xv);
#pragma unroll
    for (int c = 0; c < NS; ++c)
      if (i == sr.a[c]) { xa[c] = xv; mine[c] = true; }
    return 0.f;
  });
  acc.merge();
  const float lse = acc.m + logf(acc.s);
  const float H = lse - acc.d / acc.s;
  if (ent && tid == 0) ent[row] = H;
  if (logp) {
#pragma unroll
    for (int c = 0; c < NS; ++c)
      if (c < S) {
        float* lp = logp + (size_t)c * (size_t)R + row;
        if (sr.a[c] < 0) { if (tid == 0) *lp = 0.f; }
        else if (mine[c]) *lp = xa[c] - lse;
      }
  }
  if (!dx) return;
  // ---- pass 2: the gradient --------------------------------------------------------------------------------------------------------
  sr.load_weights(adv, row, R, S, group, coef);
  sr.ent_coef = ent_coef;
  sr.lse = lse;
  sr.H = H;
  rows_walk<4>(tid, V, xr, nullptr, rows_accumulate{dx + row * (size_t)lddx, accumulate}, [=](int i, float xv, float) { return sr.dx(i, xv); });
}

// ---- entry points --------------------------------------------------------------------------------------------------------------------
static int score_check_samples(const char* fn, int S) {
  SGG_CHECK_ARG(S >= 1 && S <= SCORE_MAX_S, "%s: 1 <= S <= 16 samples per row (got S = %d)", fn, S);
  return SGG_OK;
}

extern "C" int sgg_sample_rows_multi(const float* x, long long ldx, int R, int V, int S, unsigned long long seed, unsigned long long draw,
                                     long long* tok, void* stream) {
  const char* fn = "sgg_sample_rows_multi";
  SGG_CHECK_ARG(R >= 1 && R <= SCORE_MAX_R && V >= 1 && V <= ROWS_MAX_V, "%s: 1 <= R <= 2^24 and 1 <= V <= 2^21 (got R = %d, V = %d)", fn, R, V);
  if (const int rc = score_check_samples(fn, S)) return rc;
  SGG_CHECK_ARG(draw < (1ull << 56), "%s: draw < 2^56 - the sample's number takes the bits above (got %llu)", fn, draw);
  SGG_CHECK_ARG(x && tok, "%s: null pointer", fn);
  SGG_CHECK_ARG(ldx >= V, "%s: row stride ldx >= V (got ldx = %lld, V = %d)", fn, ldx, V);
  const relax_rng rng = {(unsigned)(seed & 0xffffffffu), (unsigned)(seed >> 32), (unsigned)(draw & 0xffffffffu), (unsigned)(draw >> 32)};
  hipStream_t st = (hipStream_t)stream;
  if (V <= ROWS_SMALL_V) {
    const rows_resident_geometry geo(R);
    hipLaunchKernelGGL(sample_rows_multi_resident_kernel, geo.grid, geo.block, 0, st, x, ldx, R, V, S, rng, tok);
  } else if (S == 1) {
    hipLaunchKernelGGL(sample_rows_multi_stream_kernel<1>, dim3(R), dim3(ROWS_T), 0, st, x, ldx, R, V, S, rng, tok);
  } else if (S == 2) {
    hipLaunchKernelGGL(sample_rows_multi_stream_kernel<2>, dim3(R), dim3(ROWS_T), 0, st, x, ldx, R, V, S, rng, tok);
  } else if (S <= 4) {
    hipLaunchKernelGGL(sample_rows_multi_stream_kernel<4>, dim3(R), dim3(ROWS_T), 0, st, x, ldx, R, V, S, rng, tok);
  } else {
    hipLaunchKernelGGL(sample_rows_multi_stream_kernel<SCORE_CH>, dim3(R), dim3(ROWS_T), 0, st, x, ldx, R, V, S, rng, tok);
  }
  SGG_LAUNCH_CHECK(fn);
  return SGG_OK;
}

extern "C" int sgg_score_advantage_multi(const float* d_out, long long ldd, int B, int S, int T, int baseline, float* adv, float* out2,
                                         void* stream) {
  const char* fn = "sgg_score_advantage_multi";
  SGG_CHECK_ARG(B >= 1 && B <= SCORE_MAX_B && T >= 1 && T <= SCORE_MAX_T, "%s: 1 <= B <= 2^20 and 1 <= T <= 64 (got B = %d, T = %d)", fn, B, T);
  if (const int rc = score_check_samples(fn, S)) return rc;
  SGG_CHECK_ARG(baseline >= 0 && baseline <= 2, "%s: baseline is 0 (none), 1 (leave-one-out over all S * B) or 2 (over the image's other samples) (got %d)",
                fn, baseline);
  SGG_CHECK_ARG(baseline != 1 || (long long)S * B >= 2, "%s: the leave-one-out baseline needs S * B >= 2 (got S = %d, B = %d)", fn, S, B);
  SGG_CHECK_ARG(baseline != 2 || S >= 2, "%s: the per-image baseline needs S >= 2 samples (got S = %d)", fn, S);
  SGG_CHECK_ARG(d_out && adv, "%s: null pointer", fn);
  SGG_CHECK_ARG(ldd >= T, "%s: row stride ldd >= T (got ldd = %lld, T = %d)", fn, ldd, T);
  hipLaunchKernelGGL(score_advantage_multi_kernel, dim3(1), dim3(SCORE_RT), 0, (hipStream_t)stream, d_out, ldd, B, S, T, baseline, adv, out2);
  SGG_LAUNCH_CHECK(fn);
  return SGG_OK;
}

template <int NS>
static void score_rows_multi_launch(hipStream_t st, const float* x, long long ldx, int R, int V, int S, const long long* tok, const float* adv,
                                    int group, float coef, float ent_coef, int accumulate, float* dx, long long lddx, float* logp, float* ent) {
  if (V <= ROWS_SMALL_V) {
    const rows_resident_geometry geo(R);
    hipLaunchKernelGGL(score_rows_multi_resident_kernel<NS>, geo.grid, geo.block, 0, st, x, ldx, R, V, S, tok, adv, group, coef, ent_coef,
                       accumulate, dx, lddx, logp, ent);
  } else {
    hipLaunchKernelGGL(score_rows_multi_stream_kernel<NS>, dim3(R), dim3(ROWS_T), 0, st, x, ldx, R, V, S, tok, adv, group, coef, ent_coef,
                       accumulate, dx, lddx, logp, ent);
  }
}

extern "C" int sgg_score_rows_multi(const float* x, long long ldx, int R, int V, int S, const long long* tok, const float* adv, int group,
                                    float coef, float ent_coef, int accumulate, float* dx, long long lddx, float* logp, float* ent,
                                    void* stream) {
  const char* fn = "sgg_score_rows_multi";
  SGG_CHECK_ARG(R >= 1 && R <= SCORE_MAX_R && V >= 1 && V <= ROWS_MAX_V, "%s: 1 <= R <= 2^24 and 1 <= V <= 2^21 (got R = %d, V = %d)", fn, R, V);
  if (const int rc = score_check_samples(fn, S)) return rc;
  SGG_CHECK_ARG(x && tok, "%s: null pointer (x, tok)", fn);
  SGG_CHECK_ARG(ldx >= V && (!dx || lddx >= V), "%s: row strides ldx, lddx >= V (got ldx = %lld, lddx = %lld, V = %d)", fn, ldx, lddx, V);
  SGG_CHECK_ARG(group >= 1 && R % group == 0, "%s: group >= 1 and a divisor of R - a sample's advantages are R / group apart (got group = %d, R = %d)",
                fn, group, R);
  SGG_CHECK_ARG(std::isfinite(coef) && std::isfinite(ent_coef), "%s: coef and ent_coef must be finite (got %g, %g)", fn, (double)coef,
                (double)ent_coef);
  SGG_CHECK_ARG(accumulate == 0 || accumulate == 1, "%s: accumulate is 0 or 1 (got %d)", fn, accumulate);
  SGG_CHECK_ARG(dx || logp || ent, "%s: no output", fn);
  SGG_CHECK_ARG((const float*)dx != x, "%s: dx must not alias x", fn);
  hipStream_t st = (hipStream_t)stream;
#define SCORE_ROWS_MULTI(NS) score_rows_multi_launch<NS>(st, x, ldx, R, V, S, tok, adv, group, coef, ent_coef, accumulate, dx, lddx, logp, ent)
  if (S == 1) SCORE_ROWS_MULTI(1);
  else if (S == 2) SCORE_ROWS_MULTI(2);
  else if (S <= 4) SCORE_ROWS_MULTI(4);
  else if (S <= 8) SCORE_ROWS_MULTI(8);
  else SCORE_ROWS_MULTI(16);
#undef SCORE_ROWS_MULTI
  SGG_LAUNCH_CHECK(fn);
  return SGG_OK;
}

extern "C" int sgg_score_summary_multi(const float* logp, int n_logp, const float* ent, int n_ent, float* out2, void* stream) {
  const char* fn = "sgg_score_summary_multi";
  SGG_CHECK_ARG(n_logp >= 1 && n_logp <= SCORE_MAX_S * SCORE_MAX_R && n_ent >= 1 && n_ent <= SCORE_MAX_R,
                "%s: 1 <= n_logp <= 2^28 and 1 <= n_ent <= 2^24 (got %d, %d)", fn, n_logp, n_ent);
  SGG_CHECK_ARG(logp && ent && out2, "%s: null pointer", fn);
  hipLaunchKernelGGL(score_summary_multi_kernel, dim3(1), dim3(SCORE_RT), 0, (hipStream_t)stream, logp, n_logp, ent, n_ent, out2);
  SGG_LAUNCH_CHECK(fn);
  return SGG_OK;
}
