// conv1_1's input gradient (Conv2DBackpropInput of architectures/generator_with_attention.py:29, the same layer in the critic):
//   dx[b,y,x,ci] = sum_{kh,kw,co} dy[b, y+1-kh, x+1-kw, co] * W[kh,kw,ci,co]      3x3, stride 1, SAME, 32 -> 3 channels, NHWC f32
// The training step never needs it (the encoder backward ends with conv1_1's filter gradient); image gradients do: saliency maps,
// input perturbations, image-space penalties (sgg_amd/grad.py).
//
// HBM-bound (batch 64 at 224^2: 411 MB of dy read, 38.5 MB of dx written; 5.5 GFLOP).  Three output channels would fill 3 of 32
// columns of a 32x32 f32 MFMA tile (59 GFLOP of issued work), so the contraction is plain VALU fmaf chains (~70 us at the VALU
// rate; packed f32 is off in this build):
//   * a workgroup owns a tile of 16 rows x 32 columns of dx; the dy it reads - the tile plus a one-pixel halo, 18 x 34 pixels, all
//     32 channels - is staged once in LDS (78 KB: two workgroups per CU) as [channel quad][row][column] 16-byte items;
//   * lane (column c, row pair r) computes the two pixels (2r, c), (2r+1, c): per tap column kw and channel quad it reads the four
//     dy rows 2r .. 2r+3 at column c+2-kw (ds_read_b128; the 32 lanes of a row read 512 contiguous bytes) and uses each for both
//     pixels' taps - 72 FMAs per four reads;
//   * the filter (864 floats, HWIO) is wave-uniform: scalar loads.
// Fixed summation order (channel quad, kw, kh, channel in program order; no atomics): two calls are bit-equal.
//
// LNB: dy is not read - it is COMPUTED while staging, from the operands of the LayerNorm backward of conv1_1's output, by the
// function ln_bwd_apply_kernel (csrc/layernorm.hip) and conv_c3_wgrad_kernel<true> (csrc/conv_wgrad.hip) call (ln_math.h: ln_bwd_dy):
//   dy = rstd * (da * ELU'(n) * gamma - m1 - xhat * m2),  xhat = (y - mean) * rstd,  n = xhat * gamma + beta
// with m1, m2 from sgg_layernorm_hwc_elu_bwd_sums.  One read of y and da replaces the apply pass (read y, da; write dy) and the
// plain kernel's read of dy.
#include "ln_math.h"

namespace {

constexpr int C3D_TH = 16, C3D_TW = 32;                    // output tile
constexpr int C3D_HR = C3D_TH + 2, C3D_HC = C3D_TW + 2;    // staged dy: tile + one-pixel halo
constexpr int C3D_CO = 32, C3D_NQ = C3D_CO / 4;

struct C3DgradLn {
  const float* y;
  const float* da;
  const float* gamma;
  const float* beta;
  const float* stats;      // [B][2] (mean, rstd)
  const float* means;      // [B][2] (m1, m2)
};

template <bool LNB>
__global__ __launch_bounds__(256, 2) void conv_c3_dgrad_kernel(const float* __restrict__ dy, const float* __restrict__ w,
                                                               float* __restrict__ dx, int H, int W, int tiles_x, int tiles_y,
                                                               C3DgradLn ln) {
  __shared__ f32x4 sdy[C3D_NQ][C3D_HR][C3D_HC];
  const int tid = threadIdx.x;
  const int tx = blockIdx.x % tiles_x, t2 = blockIdx.x / tiles_x;
  const int ty = t2 % tiles_y, b = t2 / tiles_y;
  const int y0 = ty * C3D_TH, x0 = tx * C3D_TW;
  float mean = 0.f, rstd = 0.f, m1 = 0.f, m2 = 0.f;
  f32x4 gm = {0.f, 0.f, 0.f, 0.f}, bt = gm;
  if constexpr (LNB) {
    mean = ln.stats[2 * b]; rstd = ln.stats[2 * b + 1]; m1 = ln.means[2 * b]; m2 = ln.means[2 * b + 1];
    gm = *reinterpret_cast<const f32x4*>(ln.gamma + 4 * (tid & (C3D_NQ - 1)));     // (the lane's channel quad qs below)
    bt = *reinterpret_cast<const f32x4*>(ln.beta + 4 * (tid & (C3D_NQ - 1)));
  }
  // ---- stage dy rows y0-1 .. y0+16, columns x0-1 .. x0+32 (zeros outside the image: no pixel, no contribution) ------------------
  // item e = tid + 256 k: pixel e / 8 of the halo patch, channel quad e % 8 - eight consecutive lanes read one pixel's 128 contiguous
  // bytes.  Every load of a lane is issued before the first LDS write (C3D_NI 16-byte loads in flight per lane, twice that with LNB):
  // one load at a time would keep ~8 KB per CU in flight, ~1 TB/s over the chip.
  constexpr int C3D_NE = C3D_HR * C3D_HC * C3D_NQ, C3D_NI = (C3D_NE + 255) / 256;
  const int qs = tid & (C3D_NQ - 1);     // (the same channel quad for every item of the lane)
  f32x4 v[C3D_NI], v2[LNB ? C3D_NI : 1];
#pragma unroll
  for (int k = 0; k < C3D_NI; ++k) {
    const int e = tid + 256 * k;
    const int p = e / C3D_NQ;
    const int r = p / C3D_HC, c = p - r * C3D_HC;
    const int yy = y0 - 1 + r, xx = x0 - 1 + c;
    v[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (LNB) v2[k] = v[k];
    if (e < C3D_NE && (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W) {
      const size_t off = ((size_t)(b * H + yy) * W + xx) * C3D_CO + 4 * qs;
      if constexpr (LNB) {
        v[k] = *reinterpret_cast<const f32x4*>(ln.y + off);
        v2[k] = *reinterpret_cast<const f32x4*>(ln.da + off);
      } else {
        v[k] = *reinterpret_cast<const f32x4*>(dy + off);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < C3D_NI; ++k) {
    const int e = tid + 256 * k;
    if (e >= C3D_NE) break;
    const int p = e / C3D_NQ;
    const int r = p / C3D_HC, c = p - r * C3D_HC;
    f32x4 o = v[k];
    if constexpr (LNB) {
      const int yy = y0 - 1 + r, xx = x0 - 1 + c;
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] = ln_bwd_dy(v[k][i], v2[k][i], mean, rstd, gm[i], bt[i], m1, m2);
      if (!((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W)) o = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    sdy[qs][r][c] = o;
  }
  __syncthreads();
  // ---- contraction: lane (c, rp) -> output pixels (y0 + 2 rp + p, x0 + c), p = 0, 1 ---------------------------------------------
  const int c = tid & 31, rp = tid >> 5;
  float acc[2][3];
#pragma unroll
  for (int p = 0; p < 2; ++p) acc[p][0] = acc[p][1] = acc[p][2] = 0.f;
  for (int q = 0; q < C3D_NQ; ++q) {
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      f32x4 d[4];     // dy rows y0 - 1 + 2 rp + j, j = 0 .. 3, at column x0 + c + 1 - kw
#pragma unroll
      for (int j = 0; j < 4; ++j) d[j] = sdy[q][2 * rp + j][c + 2 - kw];
#pragma unroll
      for (int kh = 0; kh < 3; ++kh) {
        const float* wt = w + (kh * 3 + kw) * 3 * C3D_CO + 4 * q;     // W[kh][kw][ci][4q ..]
#pragma unroll
        for (int ci = 0; ci < 3; ++ci) {
          const f32x4 wv = *reinterpret_cast<const f32x4*>(wt + ci * C3D_CO);
#pragma unroll
          for (int p = 0; p < 2; ++p) {
            const f32x4 dv = d[p + 2 - kh];      // dy row y + 1 - kh of output row y = y0 + 2 rp + p
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[p][ci] = fmaf(dv[k], wv[k], acc[p][ci]);
          }
        }
      }
    }
  }
  const int xx = x0 + c;
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int yy = y0 + 2 * rp + p;
    if (yy < H && xx < W) {
      float* o = dx + ((size_t)(b * H + yy) * W + xx) * 3;
      o[0] = acc[p][0]; o[1] = acc[p][1]; o[2] = acc[p][2];
    }
  }
}

int c3_dgrad_launch(const float* dy, const float* w, float* dx, int B, int H, int W, const C3DgradLn& ln, bool lnb, hipStream_t st) {
  const int tiles_x = sgg_cdiv(W, C3D_TW), tiles_y = sgg_cdiv(H, C3D_TH);
  const long long ntiles = (long long)B * tiles_x * tiles_y;
  SGG_CHECK_ARG(ntiles < (1LL << 31), "sgg_conv2d_nhwc_dgrad_c3: grid too large");
  if (lnb)
    hipLaunchKernelGGL(conv_c3_dgrad_kernel<true>, dim3((unsigned)ntiles), dim3(256), 0, st, dy, w, dx, H, W, tiles_x, tiles_y, ln);
  else
    hipLaunchKernelGGL(conv_c3_dgrad_kernel<false>, dim3((unsigned)ntiles), dim3(256), 0, st, dy, w, dx, H, W, tiles_x, tiles_y, ln);
  return SGG_OK;
}

}  // namespace

extern "C" int sgg_conv2d_nhwc_dgrad_c3(const float* dy, const float* w_hwio, float* dx, int B, int H, int W, int pad_t, int pad_l,
                                        void* stream) {
  SGG_CHECK_ARG(dy && w_hwio && dx, "sgg_conv2d_nhwc_dgrad_c3: null pointer");
  SGG_CHECK_ARG(B > 0 && H > 0 && W > 0 && pad_t == 1 && pad_l == 1, "sgg_conv2d_nhwc_dgrad_c3: bad dims (3x3 stride 1, SAME padding)");
  SGG_CHECK_ARG((long long)B * H * W * C3D_CO < (1LL << 31), "sgg_conv2d_nhwc_dgrad_c3: tensor exceeds 2^31 elements");
  SGG_CHECK_ARG(((uintptr_t)dy & 15) == 0 && ((uintptr_t)w_hwio & 15) == 0, "sgg_conv2d_nhwc_dgrad_c3: dy and w must be 16-byte aligned");
  const int rc = c3_dgrad_launch(dy, w_hwio, dx, B, H, W, C3DgradLn{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}, false,
                                 (hipStream_t)stream);
  if (rc != SGG_OK) return rc;
  SGG_LAUNCH_CHECK("sgg_conv2d_nhwc_dgrad_c3");
  return SGG_OK;
}

extern "C" int sgg_conv2d_nhwc_dgrad_c3_ln(const float* y, const float* da, const float* gamma, const float* beta, const float* stats,
                                           const float* means, const float* w_hwio, float* dx, int B, int H, int W, int pad_t, int pad_l,
                                           void* stream) {
  SGG_CHECK_ARG(y && da && gamma && beta && stats && means && w_hwio && dx, "sgg_conv2d_nhwc_dgrad_c3_ln: null pointer");
  SGG_CHECK_ARG(B > 0 && H > 0 && W > 0 && pad_t == 1 && pad_l == 1, "sgg_conv2d_nhwc_dgrad_c3_ln: bad dims (3x3 stride 1, SAME padding)");
  SGG_CHECK_ARG((long long)B * H * W * C3D_CO < (1LL << 31), "sgg_conv2d_nhwc_dgrad_c3_ln: tensor exceeds 2^31 elements");
  SGG_CHECK_ARG((((uintptr_t)y | (uintptr_t)da | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)w_hwio) & 15) == 0,
                "sgg_conv2d_nhwc_dgrad_c3_ln: y, da, gamma, beta and w must be 16-byte aligned");
  const int rc = c3_dgrad_launch(nullptr, w_hwio, dx, B, H, W, C3DgradLn{y, da, gamma, beta, stats, means}, true, (hipStream_t)stream);
  if (rc != SGG_OK) return rc;
  SGG_LAUNCH_CHECK("sgg_conv2d_nhwc_dgrad_c3_ln");
  return SGG_OK;
}
