// Halo-resident 3x3 stride-1 convolution (split 16-bit modes): internal interface between conv_halo.hip (kernel, launch)
// and conv_gather.hip (the sgg_conv2d_nhwc_fwd / _dgrad entry points that dispatch to it).
#pragma once
#include "sgg_common.h"

struct HaloParams {
  const float* src;       // [B, H, W, C] f32 NHWC (forward: x; dgrad: dy)
  const void* wfrag;      // weights as MFMA B fragments (sgg_conv_split_weights_frag)
  const float* bias;      // may be null
  float* out;             // [B, H, W, N]
  const float* amax_src;  // precision 2: device words with max|src| and max|w|
  const float* amax_w;
  float* tile_stats;      // optional: per (8x8 block, wave column range) (count, mean, M2, max dev) for the following LayerNorm
  // LN prologue (forward only, optional): src holds the PRE-LayerNorm convolution output y of the producing layer; the patch staging
  // applies a = ELU((y - mean_b) * rstd_b * gamma_c + beta_c) on the fly (ln_stats [B][2] from sgg_layernorm_hwc_finalize), so the
  // LayerNorm apply pass and the materialised activation are not needed (generator_with_attention.py:30..56)
  const float* ln_stats;
  const float* ln_gamma;
  const float* ln_beta;
  int B, H, W, C, N;
  int bh, bw, nblk;       // 8x8 blocks per image (rows, cols) and in total
  int flip;               // 0: forward (correlation); 1: dgrad (taps mirrored)
  unsigned src_bytes, w_bytes;
  int gx;                 // workgroups per XCD (set by the launchers from the route)
  // Addressing in floats (sgg_halo_dense_strides fills the NHWC defaults).  Source: grid row / pixel strides and the offset of
  // 32-channel chunk cc = (cc >> 1) * in_cA + (cc & 1) * in_cB; output: the same for 32-column group g.  A 5x5 stride-2
  // convolution over 32 channels runs here as a 3x3 stride-1 convolution over the SPACE-TO-DEPTH view of x (chunk = pixel parity
  // (qy, qx): row stride 2*Wx*32, pixel stride 64, cA = Wx*32, cB = 32), its dgrad writes dx through the same view.
  int in_rs, in_ps, in_cA, in_cB;
  int out_rs, out_ps, out_nA, out_nB;
  int ln_nc;              // LN prologue: real channels of the source (a power of two: C, or 32 for the space-to-depth view)
  int frag16;             // 1: wfrag holds the fragments of the K = 32 MFMA shape (w_split_layout 4): the producer / consumer kernel
  int src_s16;            // 1: src is a pre-split ("S16") tensor of the LayerNorm kernels (split16.h): staged without arithmetic
  int cu_cap;             // > 0: the persistent workgroups occupy at most this many of an XCD's 32 CUs (launch hint of the forward entry point)
};
// CUs of an XCD a persistent launch may occupy
inline int sgg_persist_cus(int cu_cap) { return (cu_cap > 0 && cu_cap < SGG_PERSIST_CUS_PER_XCD) ? cu_cap : SGG_PERSIST_CUS_PER_XCD; }
inline void sgg_halo_dense_strides(HaloParams& h) {
  h.in_rs = h.W * h.C; h.in_ps = h.C; h.in_cA = 64; h.in_cB = 32;
  h.out_rs = h.W * h.N; h.out_ps = h.N; h.out_nA = 64; h.out_nB = 32;
  h.ln_nc = h.C;
  h.frag16 = 0;
  h.src_s16 = 0;
  h.cu_cap = 0;
}

// Workgroups per XCD of a persistent launch: XCD k of the 8 owns an eighth of the `units` (M-tiles, bands), each with `ntn` (n-tile
// [, channel half]) items; at most `slots` workgroups are resident on its CUs; a whole number of units per trip.
inline int sgg_persist_gx(int units, int ntn, int slots) {
  const int per_xcd = sgg_cdiv(units, 8) * ntn;
  return sgg_cdiv(per_xcd < slots ? per_xcd : slots, ntn) * ntn;
}

// ---- routes ------------------------------------------------------------------------------------------------------------------
// Which kernel a launch runs is decided ONCE per family, by a pure host function (no HIP call, no pointer dereferenced: it sees only
// which optional operands are present) that fills a route: exactly the template arguments of the instantiation plus the launch
// geometry derived with them.  The launcher switches on the route; sgg_*_symbol prints the same route as the kernel's symbol
// (rocprofv3's spelling with spaces removed, defaulted template arguments written out) for sgg_conv2d_nhwc_fwd_symbol / _dgrad_symbol.
// one arm of a launcher's instantiation list: the route's values that select it, then the launch
#define SGG_LAUNCH_ARM(selected, ...)  \
  if (selected) {                      \
    hipLaunchKernelGGL(__VA_ARGS__);   \
    return SGG_OK;                     \
  }
inline const char* sgg_tf(bool b) { return b ? "true" : "false"; }
struct HaloRoute {      // conv_halo3_kernel<NB, BN, WGM, WGN, HALF, true, ONECH, LNP, ONE, 1>
  int NB, BN, WGM, WGN;
  bool HALF, ONECH, LNP, ONE;
  int gx;
};
struct HaloPcRoute {    // conv_halo3_pc_kernel<HALF, LNP, DMAP, NB>
  bool HALF, LNP, DMAP;
  int NB;
  int gx;
};
struct S2Route {        // conv_s2_kernel<DGRAD, HALF, MT, ONE, LNP, DMAP, NW>
  bool DGRAD, HALF;
  int MT;
  bool ONE, LNP, DMAP;
  int NW;
  int ksplit, gx;
  bool wide;
};

// 1 if the halo kernel serves a 3x3 / stride-1 convolution over an H x W grid in this precision
int sgg_halo_applicable(int KH, int KW, int stride, int H, int W, int C, int N, int precision);
int sgg_s2d_applicable(int KH, int KW, int stride, int Hi, int Wi, int Cin, int Cout, int precision);
// columns covered by one (count, mean, M2) partial of the halo kernel for N output channels
int sgg_halo_stats_cols(int N);
HaloRoute sgg_halo_route(const HaloParams& p, int precision);
int sgg_halo_launch(const HaloRoute& r, const HaloParams& p, hipStream_t st);     // SGG_OK, or SGG_ERR_ARG: no such instantiation
void sgg_halo_symbol(const HaloRoute& r, char* buf, size_t len);
// producer / consumer form for 128-column tiles in the two-piece modes (conv_halo_pc.hip; weights in w_split_layout 4: the entry
// points take this family when HaloParams::frag16 is set)
int sgg_halo_pc_applicable(int C, int N, int precision);
// its four-block form for 64-column tiles (pre-split sources only)
int sgg_halo_pc64_applicable(int C, int N, int precision);
HaloPcRoute sgg_halo_pc_route(const HaloParams& p, int precision);
int sgg_halo_pc_launch(const HaloPcRoute& r, const HaloParams& p, hipStream_t st);
void sgg_halo_pc_symbol(const HaloPcRoute& r, char* buf, size_t len);

// ---- filter gradient (conv_wgrad.hip; resident kernels: conv_wgrad_halo.hip, conv_wgrad_dma.hip) ------------------------------------
// One route per launch, as above: wgrad_route (conv_wgrad.hip) validates the launch's scalars and fills it, sgg_conv2d_nhwc_wgrad
// switches on the family, sgg_conv2d_nhwc_wgrad_symbol prints it, sgg_conv2d_nhwc_wgrad_resident reads its family.
enum { WGRAD_C3, WGRAD_TAP, WGRAD_TAP_TR, WGRAD_HALO, WGRAD_HALO_RB, WGRAD_DMA, WGRAD_DMA_RB };
// The taps of one launch of the resident kernels.  Stride 1: one class, all 3x3 taps.  5x5 stride 2: the four parity classes (cy, cx)
// of the x pixels, each a stride-1 problem on the sub-sampled x grid: taps kh with (kh - pad_t) mod 2 == cy, kh = kh0 + 2 ia, which
// read sub-grid pixel (oy + a0y + ia, ox + a0x + ib).
struct WgradTapClass {
  int cy, cx, a0y, a0x, kh0, kw0;
  int nkh, nkw;           // taps of the class: the kernels' NKH x NKW
};
struct WgradRoute {
  int family;
  // template arguments.  WGRAD_C3: conv_c3_wgrad_kernel<false>; _TAP: conv_wgrad_kernel<BMC, BNC, WM, WN, P, HALF>; _TAP_TR:
  // conv_wgrad_tr_kernel<P, HALF>; _HALO / _HALO_RB: conv_wgrad_halo3_kernel<CT, NT, HALF, CT == NT, NKH, NKW, LNP, GEO = 0 / 1, ONE>;
  // _DMA: conv_wgrad_dma_kernel<NT, NKH, NKW>; _DMA_RB: conv_wgrad_dma_rb_kernel<NKH, NKW>  (NKH, NKW: of each tap class)
  int BMC, BNC, WM, WN, P;
  int CT, NT;             // channel chunk of a resident workgroup: 32*CT input x 32*NT output channels
  bool HALF, LNP, ONE;
  dim3 grid;
  int nslabs;             // partial dW slabs [slab][taps][Cin][Cout] the launch writes; the slab reduce sums them into dw
  size_t ws_bytes;        // of those slabs; 0: a single slab, written straight into dw (per-tap kernels only)
  int ncls;
  WgradTapClass cls[4];   // resident families: one launch per class, in this order
  // launch geometry that goes into the kernels' params
  int tiles, chunk;       // _C3: 8 x 32 pixel tiles, tiles per workgroup;  _TAP*: channel tiles, pixels per split
  int stages;             // resident: stages per workgroup
  int R, pc, xslots;      // row bands (_RB): rows per band (R * W <= 112 pixels), patch pitch (W + 1: one shared zero column), patch slots
};
// (cy, cx, ...) of a tap class, the tap step and the slab layout into either resident kernel's params
template <class Params>
inline void sgg_wgrad_set_class(Params& p, const WgradTapClass& c, int stride) {
  p.cy = c.cy; p.cx = c.cx; p.a0y = c.a0y; p.a0x = c.a0x; p.kh0 = c.kh0; p.kw0 = c.kw0;
  p.kstep = stride; p.KWt = stride == 1 ? 3 : 5; p.taps_total = p.KWt * p.KWt;
}
// H, W: the dy grid.  One launch per tap class of the route, each writing r.nslabs partial slabs (unscaled f32) into `slabs`.
// SGG_OK, or SGG_ERR_ARG: no such instantiation.
// halo: operand_format bit 0 = x, bit 1 = dy is a pre-split ("S16") tensor (split16.h); dma: both are
int sgg_wgrad_halo_launch(const WgradRoute& r, const float* x, const float* dy, float* slabs, int B, int H, int W, int Cin, int Cout,
                          int stride, const float* amax_x, const float* amax_dy, const float* ln_stats, const float* ln_gamma,
                          const float* ln_beta, int operand_format, hipStream_t st);
int sgg_wgrad_dma_launch(const WgradRoute& r, const void* x, const void* dy, float* slabs, int B, int H, int W, int Cin, int Cout, int stride,
                         const float* amax_x, const float* amax_dy, hipStream_t st);

// ---- band-resident 5x5 stride-2 convolution, forward and dgrad (conv_s2.hip) -----------------------------------------
struct S2Params {
  const float* src;       // forward: x [B, 2*Ho, 2*Wo, C];  dgrad: dy [B, Ho, Wo, C]
  const void* wfrag;      // 25 taps as MFMA B fragments (sgg_conv_split_weights_frag with taps = 25)
  const float* bias;      // forward only, may be null
  float* out;             // forward: y [B, Ho, Wo, N];  dgrad: dx [B, 2*Ho, 2*Wo, N]
  const float* amax_src;
  const float* amax_w;
  float* tile_stats;      // forward, optional: (count, mean, M2) per (band, 32 output channels)
  // LN prologue (forward, two-piece modes, optional): src is the producing layer's PRE-LayerNorm output; the patch staging applies
  // ELU((y - mean_b) * rstd_b * gamma_c + beta_c) (see HaloParams)
  const float* ln_stats;
  const float* ln_gamma;
  const float* ln_beta;
  int B, Ho, Wo;          // the half-resolution grid (forward: output positions; dgrad: dy positions)
  int C, N;               // contraction channels, output channels
  int M;                  // B * Ho * Wo
  int nbands;             // ceil(M / 224)
  int pitch;              // Wo: slots per patch row (no halo columns: edge lanes read a zero slot)
  unsigned src_bytes, w_bytes;
  int gx;                 // workgroups per XCD (set by sgg_s2_launch from the route)
  int src_s16;            // 1: src is a pre-split ("S16") tensor (split16.h)
  int ksplit;             // 1, or 2: two workgroups per (band, n-tile), each contracting half of the channel chunks and ADDING its
                          // partial into the zeroed output (a + b = b + a: still deterministic); set by sgg_s2_launch
  int cu_cap;             // as HaloParams::cu_cap
};
// 1 if the band-resident kernel serves this 5x5 / stride-2 / SAME convolution (Hi, Wi = the full-resolution grid, both even;
// C = contraction channels, N = output channels of the direction asked for)
int sgg_s2_applicable(int KH, int KW, int stride, int B, int Hi, int Wi, int C, int N, int precision);
// (count, mean, M2) partials per sample the forward emits, 0 if bands do not align with samples
int sgg_s2_stats_per_sample(int Ho, int Wo, int N);
S2Route sgg_s2_route(const S2Params& p, int dgrad, int precision);
int sgg_s2_launch(const S2Route& r, const S2Params& p, hipStream_t st);
void sgg_s2_symbol(const S2Route& r, char* buf, size_t len);
