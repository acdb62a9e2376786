// The per-element arithmetic of LayerNorm + ELU and of its backward, written once: the streaming kernels of layernorm.hip and the
// two kernels that compute dy while staging it (conv_c3_dgrad_kernel<true>, conv_c3_wgrad_kernel<true>) call these, so their values
// are the same bits by construction.  The build contracts a * b + c into an fma (-ffp-contract=fast): the grouping of every
// expression below is part of its result.
// (Not the LN prologue of split16.h, ln_elu4 / ln_elu8: its ELU is __expf(z) - 1.f, other arithmetic; it stays where it is.)
#pragma once
#include "sgg_common.h"

// forward, the four channels of a lane: ELU(v * inv + shift), inv = gamma_c * rstd, shift = beta_c - inv * mean; ELU through expm1f.
// (The four arguments first, then the four activations: with the activation inside the per-channel expression the compiler
// flattens expm1f's branches, which measured 0.6 % slower in the pre-split forward kernel.)
__device__ __forceinline__ float ln_elu1(float z) { return z > 0.f ? z : expm1f(z); }
__device__ __forceinline__ f32x4 ln_elu(const f32x4& v, const f32x4& inv, const f32x4& shift) {
  f32x4 o = v * inv + shift;
  o[0] = ln_elu1(o[0]); o[1] = ln_elu1(o[1]); o[2] = ln_elu1(o[2]); o[3] = ln_elu1(o[3]);
  return o;
}

// backward, one element: xhat = (y - mean) * rstd, n = xhat * gamma_c + beta_c (the ELU's argument), dn = da * ELU'(n)
struct LnBwdTerms {
  float xhat, n, dn;
};
__device__ __forceinline__ LnBwdTerms ln_bwd_terms(float y, float da, float mean, float rstd, float gamma, float beta) {
  LnBwdTerms t;
  t.xhat = (y - mean) * rstd;
  t.n = t.xhat * gamma + beta;
  t.dn = da * (t.n > 0.f ? 1.f : __expf(t.n));
  return t;
}
// dy = rstd * (dxhat - mean dxhat - xhat * mean(dxhat * xhat)), dxhat = dn * gamma_c; m1, m2: the two means of the sample
__device__ __forceinline__ float ln_bwd_dy(const LnBwdTerms& t, float rstd, float gamma, float m1, float m2) {
  return rstd * (t.dn * gamma - m1 - t.xhat * m2);
}
__device__ __forceinline__ float ln_bwd_dy(float y, float da, float mean, float rstd, float gamma, float beta, float m1, float m2) {
  return ln_bwd_dy(ln_bwd_terms(y, da, mean, rstd, gamma, beta), rstd, gamma, m1, m2);
}
