/* libsgg_hip.so — C ABI of the MI355X-native (gfx950) Scene-Graph-GAN training hot path.
 *
 * The reference (mklawonn/Scene-Graph-GAN, Python 2 + TensorFlow 1.x) has NO FFI / plugin boundary: every
 * arithmetic op is a stock TensorFlow kernel composed by architectures/*.py and train.py.  This header is the
 * boundary a maintainer would bind instead of those TF kernels; each entry point cites the reference call
 * site (file:line, relative to the reference root) whose TF op (and its autodiff gradient under
 * optimizer.minimize, train.py:265-266) it replaces.  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error (sgg_last_error() gives the text); nothing throws,
 *     allocates, or synchronises; work is enqueued on `stream` (a hipStream_t passed as void*).
 *   - all pointers are DEVICE pointers to fp32 unless stated; tensors are dense row-major; activations are
 *     NHWC, conv kernels HWIO [kh][kw][cin][cout] (TF layouts), dense kernels [in][out].
 *   - `*_workspace_bytes` functions size the scratch buffer the caller must pass.
 *   - "dual" pointer pairs: the second-order path of the gradient penalty runs the same kernels on dual
 *     numbers (real plane, dual plane).  Passing NULL for the *_dual inputs selects plain fp32.
 */
#ifndef SGG_HIP_H
#define SGG_HIP_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

int sgg_version(void);
const char* sgg_last_error(void);
int sgg_device_info(int* cu_count, size_t* lds_bytes_per_cu, size_t* hbm_bytes, char* arch, int arch_len);

/* ---- convolutional encoder: tf.layers.conv2d(padding="same") --------------------------------------------
 * generator_with_attention.py:29-68, discriminator_with_attention.py:29-68 (12 live layers each).
 * pad_t / pad_l are the TF SAME "before" pads (pad_total // 2); the "after" pad is implied by Ho/Wo. */
int sgg_hwio_to_hwoi(const float* w_hwio, float* w_hwoi, int taps, int cin, int cout, void* stream);
/* forward: `w` = HWIO kernel when Cin == 3, else its HWOI transpose (sgg_hwio_to_hwoi). y = conv(x) + bias */
/* precision: 0 = native f32 MFMA (v_mfma_f32_32x32x2_f32, exact f32);
 *            2 = f32 operands scaled by a per-tensor power of two (from amax_* = device words holding max|tensor|, see
 *                sgg_absmax / the amax_out of the LayerNorm kernels) and split into two fp16 pieces, 3 fp16 MFMAs, f32
 *                accumulate: the two pieces are taken with round-to-nearest-even (v_cvt_pk_f16_f32; csrc/sgg_common.h f16_split2),
 *                i.e. 23 significant bits per operand for elements within 2^-16 of the tensor maximum, min(23, 39 - d) bits for an
 *                element 2^-d below it (DESIGN.md "Error model and its floor"); error vs fp64 within 2x native f32 + 3e-7 on every
 *                configs[1] layer (tests/test_fullsize_conv_gpu.py);
 *            3 / 6 = split into 2 / 3 bf16 pieces, 3 / 6 bf16 MFMAs (6: f32-equivalent, 3: 2^-17 cross terms dropped);
 *            1 / 4 = MIXED PRECISION (not the reference's arithmetic): operands rounded to ONE fp16 (scaled
 *                like precision 2) / ONE bf16 piece, one MFMA per product, f32 accumulate - error vs fp64 2e-3 / 1.5e-2 of the
 *                output's maximum.  Served by the resident kernels (w_split_layout 1 / 2 / 3, the halo-resident wgrad); other
 *                shapes run these codes in the two-piece arithmetic (2 / 3).  The pre-split weights are the ones of precision 2 / 3.
 * amax pointers are only read for precision 1 / 2 (may be NULL otherwise). */
/* w_split (optional, may be NULL): the same weights pre-split by sgg_split_bf16 into precision/2 bf16 planes [P][n];
 * saves the per-workgroup split of the weight operand in the split-bf16 modes. */
int sgg_conv_split_weights(const float* in, void* out, long long n, int precision, const float* amax, void* stream);
int sgg_absmax(const float* x, long long n, float* amax /* atomically max-ed; zero it first */, void* stream);
/* Halo-resident kernel for the 3x3 stride-1 layers (generator_with_attention.py:31-57: conv1_2, conv2_1..2_4, conv3_1,
 * conv3_2) in precision 2 / 3: sgg_conv_wsplit_layout returns 1 where it applies (H % 8 == W % 8 == 0); the pre-split weights
 * must then be in MFMA fragment order (sgg_conv_split_weights_frag over the [taps][N][C] tensor: the HWOI transpose for the
 * forward, the HWIO kernel for dgrad) and w_split_layout = 1 is passed to sgg_conv2d_nhwc_fwd / _dgrad.  Layout 0 = planes.
 * Band-resident kernel for the 5x5 stride-2 layers (generator_with_attention.py:35,50,65,68: conv2_5, conv3_5, `downsampled`;
 * conv1_3 has too few channels for its 128-column tile) on even grids: sgg_conv_wsplit_layout returns 2 (H, W = the full-resolution
 * grid; ask with (Cin, Cout) swapped for the dgrad direction); weights in the same fragment order with taps = 25.
 * conv1_3 (generator_with_attention.py:35: 5x5 stride 2 over 32 -> 32 channels, H % 16 == W % 16 == 0): sgg_conv_wsplit_layout
 * returns 3 - the convolution runs on the halo-resident kernel as a 3x3 stride-1 convolution over the space-to-depth view of x
 * (x[2a + qy][2c + qx][ci] = channel (qy, qx, ci) of pixel (a, c); no copy, strides only) with the 9-tap kernel
 * [3][3][4 * Cin][Cout] of sgg_conv_s2d_weights (11 of its 36 (tap, parity) slots are zero); weights in fragment order with
 * taps = 9 (forward: the HWOI transpose of that kernel, N = Cout, C = 4 * Cin; dgrad: the kernel itself, N = 4 * Cin, C = Cout).
 * Producer / consumer kernel for the 3x3 stride-1 layers with 128-column tiles (generator_with_attention.py:44-57: conv2_3,
 * conv2_4, conv3_1, conv3_2 forward; conv2_4, conv3_1, conv3_2 dgrad): where a layout-1 layer also has Cout % 128 == 0 and
 * Cin % 64 == 0 in precision 2 / 3, sgg_conv_wsplit_layout returns 4 instead - one 8-wave workgroup per CU (4 MFMA waves on
 * v_mfma_f32_16x16x32_*, 4 producer waves that each DMA a quarter of every tap's weight fragments and stage a quarter of the patch; csrc/conv_halo_pc.hip); the pre-split weights are then the
 * fragments of THAT MFMA shape (sgg_conv_split_weights_frag16) and w_split_layout = 4 is passed to sgg_conv2d_nhwc_fwd / _dgrad.
 * Same arithmetic as layout 1 (same pieces, same three products per f32 product, f32 accumulation; the order of the sum over the
 * 32 channels of a chunk differs). */
int sgg_conv_s2d_weights(const float* w5 /* [5][5][Cin][Cout] */, float* w3 /* [3][3][4*Cin][Cout] */, int Cin, int Cout, void* stream);
/* All of the above for every layer of one encoder after an optimiser step, in three launches (the per-layer entry points are
 * ~45 five-microsecond launches per network): w_hwoi = the HWOI transpose; *amax = max|w| (precision 1 / 2; may be NULL
 * otherwise); layout 3 (in either direction): w3 / w3_hwoi = the 9-tap space-to-depth kernel and its transpose; ws_fwd / ws_bwd
 * (optional) = the pre-split operands of the forward / dgrad direction in layout_fwd / layout_bwd (sgg_conv_wsplit_layout; 0 =
 * planes of sgg_conv_split_weights).  At most 16 layers per call; Cin == 3 layers need no preparation. */
typedef struct {
  const float* w;        /* HWIO [taps][Cin][Cout] */
  float* w_hwoi;         /* [taps][Cout][Cin] */
  float* w3;             /* layout 3 only, else NULL: [9][4*Cin][Cout] */
  float* w3_hwoi;        /* layout 3 only, else NULL: [9][Cout][4*Cin] */
  void* ws_fwd;          /* may be NULL */
  void* ws_bwd;          /* may be NULL */
  float* amax;
  int taps, cin, cout, layout_fwd, layout_bwd;
} sgg_conv_weight_desc;
int sgg_conv_prepare_weights(const sgg_conv_weight_desc* layers, int n_layers, int precision, void* stream);
/* The library reads no environment variables and keeps no mutable global state: every kernel choice is a function of the
 * arguments (w_split_layout here, `algo` of sgg_conv2d_nhwc_wgrad). */
int sgg_conv_wsplit_layout(int KH, int KW, int stride, int H, int W, int Cin, int Cout, int precision);
/* The same question for a launch whose source operand (x of the forward, dy of the dgrad) WILL arrive pre-split (operand_format 1):
 * 3x3 stride-1 layers with Cout % 64 == 0 (not 128) and Cin % 64 == 0 in precision 2 then also run on the producer / consumer kernel,
 * in its four-block form (4 blocks x 64 columns per workgroup; the patch by LDS-DMA only): 4 is returned for them as well, and such a
 * launch MUST pass operand_format 1 (an f32 source with this layout is refused).  generator_with_attention.py:41,44: the
 * Conv2DBackpropInput of conv2_2 and conv2_3. */
int sgg_conv_wsplit_layout_presplit(int KH, int KW, int stride, int H, int W, int Cin, int Cout, int precision);
int sgg_conv_split_weights_frag(const float* in, void* out, int taps, int N, int C, int precision, const float* amax, void* stream);
int sgg_conv_split_weights_frag16(const float* in, void* out, int taps, int N, int C, int precision, const float* amax, void* stream);
int sgg_conv2d_nhwc_fwd(const float* x, const float* w, const void* w_split, const float* bias, float* y, int B, int Hi, int Wi, int Cin,
                        int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad_t, int pad_l, int precision, int w_split_layout,
                        const float* amax_x, const float* amax_w, float* tile_stats, const float* ln_stats, const float* ln_gamma,
                        const float* ln_beta, int operand_format, void* stream);
/* operand_format of sgg_conv2d_nhwc_fwd, bits 8 .. 13 (launch hint, 0 = none): the persistent resident kernels (w_split_layout
 * 1 .. 4) occupy at most that many of an XCD's 32 CUs instead of all of them - for a forward pass that runs on its own HIP stream
 * beside another stream's chain of short, latency-critical launches (the recurrent heads), which then find free CUs at once.  The
 * work decomposition (tiles, products, summation orders) does not depend on it: results are bit-identical
 * (tests/test_persistent_tiles_gpu.py: every resident kernel form under caps that give a workgroup several tiles, against no cap).
 * operand_format bit 0 (sgg_conv2d_nhwc_fwd / _dgrad: 0 or 1; _wgrad: bit 0 = x, bit 1 = dy): 1 = the operand is a PRE-SPLIT tensor as
 * sgg_layernorm_hwc_elu_fwd / _bwd write it with out_format 1 - same shape and bytes as the f32 tensor, every aligned group of 32
 * channels (128 B) holding the 32 leading fp16 pieces (64 B) then the 32 residual pieces of x * 2^e, e from the tensor's amax word
 * (which must be the word the producer used).  The kernel then stages the operand without splitting it again (bit-identical
 * products).  Precision 1 / 2 and the resident kernels only (w_split_layout 1 .. 4; wgrad: where sgg_conv2d_nhwc_wgrad_resident
 * says 1); not together with an LN prologue on that operand.
 * tile_stats (optional): the epilogue also writes (count, mean, M2, max |y - mean|) of every output tile, [B][n][4] with
 * n = sgg_conv2d_nhwc_fwd_tile_stats(...) > 0; pass them to sgg_layernorm_hwc_elu_fwd to skip its statistics pass, or to
 * sgg_layernorm_hwc_finalize when the consumer applies the LayerNorm itself:
 * LN prologue (ln_stats / ln_gamma / ln_beta, optional, w_split_layout 1 only; also on sgg_conv2d_nhwc_wgrad where its halo-resident
 * kernel applies): x is the PRE-LayerNorm output y of the producing convolution and the kernel computes
 * ELU((y - mean_b) * rstd_b * gamma_c + beta_c) while it stages its input patch (tf.contrib.layers.layer_norm(activation_fn=elu),
 * generator_with_attention.py:30..56), so the LayerNorm apply pass and the activation tensor are never written.  ln_stats [B][2] =
 * (mean, rstd) from sgg_layernorm_hwc_finalize; amax_x must then be the word that call published (an upper bound of max|a|). */
int sgg_conv2d_nhwc_fwd_tile_stats(int Ho, int Wo, int Cin, int Cout, int KH, int KW, int stride, int precision, int w_split_layout);
/* Conv2DBackpropInput: dx from dy and the HWIO kernel */
int sgg_conv2d_nhwc_dgrad(const float* dy, const float* w_hwio, const void* w_split, float* dx, int B, int Hi, int Wi, int Cin, int Ho,
                          int Wo, int Cout, int KH, int KW, int stride, int pad_t, int pad_l, int precision, int w_split_layout,
                          const float* amax_dy, const float* amax_w, int operand_format, void* stream);
/* Which kernel the launch with these arguments runs: its symbol as rocprofv3 prints it with the spaces removed, every defaulted
 * template argument written out (e.g. conv_halo3_pc_kernel<true,false,true,2>), into buf (buf_len >= 96).  Same scalar arguments as
 * sgg_conv2d_nhwc_fwd / _dgrad; the optional operands only as flags (has_w_split, has_tile_stats, has_ln: that pointer would not be
 * NULL; the required ones and the amax words count as given).  Both run the launch's own validation and read the symbol off the very
 * route the launch switches on, so an argument set the launch refuses is refused here in the same way (sgg_last_error), and what
 * they report is what runs.  Pure host functions: no GPU needed, nothing launched. */
int sgg_conv2d_nhwc_fwd_symbol(int B, int Hi, int Wi, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad_t, int pad_l,
                               int precision, int w_split_layout, int has_w_split, int has_tile_stats, int has_ln, int operand_format,
                               char* buf, int buf_len);
int sgg_conv2d_nhwc_dgrad_symbol(int B, int Hi, int Wi, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad_t, int pad_l,
                                 int precision, int w_split_layout, int has_w_split, int operand_format, char* buf, int buf_len);
/* Conv2DBackpropFilter: dw (HWIO) from x and dy.  algo: 0 = automatic (the resident kernels where they apply), 1 = per-tap
 * kernels only (A/B measurements).  One routing decision per launch: which kernel runs, with which template arguments and grid, into
 * how many partial slabs of the workspace (summed by one deterministic reduce launch) follows from the scalar arguments alone -
 * sgg_conv2d_nhwc_wgrad_symbol reports it.  The launch needs exactly the workspace the query reports (none where a per-tap kernel
 * writes dw directly); sgg_conv2d_nhwc_wgrad_workspace_bytes, which knows neither precision nor stride, is an upper bound of it. */
size_t sgg_conv2d_nhwc_wgrad_workspace_bytes(int B, int Hi, int Wi, int Cin, int Ho, int Wo, int Cout, int KH, int KW);
int sgg_conv2d_nhwc_wgrad(const float* x, const float* dy, float* dw_hwio, int B, int Hi, int Wi, int Cin, int Ho,
                          int Wo, int Cout, int KH, int KW, int stride, int pad_t, int pad_l, int precision, int algo,
                          const float* amax_x, const float* amax_dy, const float* ln_stats, const float* ln_gamma, const float* ln_beta,
                          int operand_format, void* workspace, size_t workspace_bytes, void* stream);
/* The convolution kernels the launch with these arguments starts, as sgg_conv2d_nhwc_fwd_symbol spells them, in launch order and
 * separated by ';' into buf (buf_len >= 256): one for stride 1, the four tap-parity classes for a 5x5 stride-2 layer on the resident
 * kernels (e.g. conv_wgrad_dma_kernel<4,3,2>;...); the slab reduce is not listed.  has_ln: ln_stats would not be NULL (gamma, beta,
 * the required operands and the amax words count as given).  *workspace_bytes (may be NULL) receives the launch's exact need.  The
 * launch's own validation and route: what it refuses is refused here in the same way (sgg_last_error).  No GPU needed. */
int sgg_conv2d_nhwc_wgrad_symbol(int B, int Hi, int Wi, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad_t, int pad_l,
                                 int precision, int algo, int has_ln, int operand_format, size_t* workspace_bytes, char* buf, int buf_len);
/* 0: the per-tap kernels serve this shape; 1: the halo-resident kernel does with algo 0 (it takes pre-split operands and stages them
 * through registers, without arithmetic); 2: as 1, and when BOTH operands are pre-split (operand_format 3, precision 2, no LN prologue)
 * the LDS-DMA kernel runs instead: 64 x 128 / 64 x 64 channel tiles, both operands copied HBM -> LDS by `buffer_load ... lds`, no
 * staging registers or arithmetic (csrc/conv_wgrad_dma.hip; channels % 64 == 0, 8-divisible grids or row bands of <= 112 pixels).
 * Read off the route of the SAME-padded launch (x grid = stride x the Ho x Wo grid); where that launch would be refused the answer
 * is 0 and sgg_last_error holds the reason. */
int sgg_conv2d_nhwc_wgrad_resident(int B, int Ho, int Wo, int Cin, int Cout, int KH, int KW, int stride, int precision);

/* ---- tf.contrib.layers.layer_norm(activation_fn=tf.nn.elu) over (H,W,C) per sample ------------------------
 * generator_with_attention.py:30..66 / discriminator_with_attention.py:30..66.  C: power of two in [4,1024].
 * fwd writes a = ELU(LN(y)) and stats[b] = (mean, rstd).  bwd writes dy, dgamma, dbeta and (optional, may be
 * NULL) dbias_prev = sum_{b,h,w} dy = the BiasAddGrad of the convolution that produced y. */
size_t sgg_layernorm_hwc_elu_workspace_bytes(int B, int HW, int C);
/* amax_out (optional): device word atomically max-ed with max|output| (the consumer convolution's f16 scaling).
 * Valid region (fwd and bwd): W == 0 -> the whole HW plane is normalised.  W > 0 -> the plane is an (HW / W) x W canvas that
 * holds the layer's true (Hv x Wv) map at rows [y0, y0 + Hv), columns [x0, x0 + Wv) (odd image sizes such as the reference's
 * 221 x 221, train.py:171, run on even canvases so that the tiled convolution kernels apply): statistics, gradients and
 * parameter gradients cover the region only; a / dy are written as ZEROS outside it (the next convolution's zero padding).
 * tile_stats must be NULL with W > 0. */
int sgg_layernorm_hwc_elu_fwd(const float* y, const float* gamma, const float* beta, float* a, float* stats,
                              float* amax_out, const float* tile_stats, int n_tile_stats, int B, int HW, int C,
                              int W, int y0, int x0, int Hv, int Wv, int out_format, void* workspace, size_t workspace_bytes, void* stream);
/* out_format 1 (both directions): the output tensor (a / dy) is written PRE-SPLIT for the convolutions that consume it (see
 * operand_format of sgg_conv2d_nhwc_fwd): every aligned 32-channel group as 32 leading + 32 residual fp16 pieces of x * 2^e.  The
 * scale must be fixed before the tensor is written, so *amax_out (required, C % 32 == 0) then receives an upper BOUND of max|x|
 * instead of the maximum: forward - the caller zeroes the word, the call merges the statistics, publishes max over the samples of
 * max|gamma| * max|y - mean| * rstd + max|beta| and applies (three launches; two with tile_stats); backward - max(rstd * max|dxhat|) *
 * (2 + max|xhat|), the two maxima published atomically by the reduction pass into the caller-zeroed words pq. */
/* An f32 NHWC tensor (n elements, channel count a multiple of 32) -> the PRE-SPLIT format under the scale of *amax (its maximum from
 * sgg_absmax, or any upper bound): for operands that no LayerNorm kernel produces - the gradient the attention head hands to
 * `downsampled` (generator_with_attention.py:68,74), whose Conv2DBackpropInput / Conv2DBackpropFilter then stage it by LDS-DMA like
 * every other layer's.  out may be x (in place). */
int sgg_presplit16(const float* x, float* out, long long n, const float* amax, void* stream);
/* statistics only: stats[b] = (mean, rstd) merged from the convolution's tile partials; amax_out max-ed with an upper bound of
 * max|ELU(LN(y))| (for the fp16 scaling of a consumer with an LN prologue) */
int sgg_layernorm_hwc_finalize(const float* tile_stats, int n_tile_stats, const float* gamma, const float* beta, float* stats,
                               float* amax_out, int B, int HW, int C, void* stream);
int sgg_layernorm_hwc_elu_bwd(const float* y, const float* da, const float* gamma, const float* beta,
                              const float* stats, float* dy, float* dgamma, float* dbeta, float* dbias_prev,
                              float* amax_out, int B, int HW, int C, int W, int y0, int x0, int Hv, int Wv, int out_format,
                              float* pq /* out_format 1: two words, zeroed by the caller, for the maxima the bound is made of */,
                              void* workspace, size_t workspace_bytes, void* stream);

/* The REDUCTION half of sgg_layernorm_hwc_elu_bwd without its apply pass, for a consumer that computes dy itself
 * (sgg_conv2d_nhwc_wgrad_c3_ln below): the partial sums go to `workspace` exactly as sgg_layernorm_hwc_elu_bwd leaves them (dgamma /
 * dbeta / dbias_prev: all NULL and sgg_layernorm_hwc_bwd_finalize later, or all given), and means [B][2] receives the two per-sample
 * means of the backward, (mean dxhat, mean dxhat * xhat), bit-identical to the values the apply pass derives.  Whole planes only. */
int sgg_layernorm_hwc_elu_bwd_sums(const float* y, const float* da, const float* gamma, const float* beta, const float* stats,
                                   float* means, float* dgamma, float* dbeta, float* dbias_prev, int B, int HW, int C, void* workspace,
                                   size_t workspace_bytes, void* stream);
/* conv1_1's filter gradient FUSED with the apply half of the LayerNorm backward of its output (generator_with_attention.py:29-30
 * under optimizer.minimize, train.py:265-266): dW [3][3][3][32] = Conv2DBackpropFilter(x, dy) with
 *   dy = rstd * (da * ELU'(n) * gamma - m1 - xhat * m2),  xhat = (y - mean) * rstd,  n = xhat * gamma + beta
 * computed from (y, da) [B][H][W][32] inside the kernel - in the training step conv1_1's filter gradient is the only consumer of
 * that dy (the step takes no image gradient, the bias gradient comes from the LayerNorm reductions; an image gradient reads it
 * through sgg_conv2d_nhwc_dgrad_c3_ln), so it is never written: one read of y and da replaces the apply pass (read y, read da,
 * write dy) and the filter gradient's read of dy.  stats [B][2] = (mean, rstd) of the forward,
 * means [B][2] from sgg_layernorm_hwc_elu_bwd_sums; exact f32 MFMA arithmetic as sgg_conv2d_nhwc_wgrad with Cin == 3; workspace as
 * sgg_conv2d_nhwc_wgrad_workspace_bytes(B, H, W, 3, H, W, 32, 3, 3). */
int sgg_conv2d_nhwc_wgrad_c3_ln(const float* x, const float* y, const float* da, const float* gamma, const float* beta,
                                const float* stats, const float* means, float* dw, int B, int H, int W, int pad_t, int pad_l,
                                void* workspace, size_t workspace_bytes, void* stream);
/* conv1_1's INPUT gradient: Conv2DBackpropInput of the first convolution (architectures/generator_with_attention.py:29, the same
 * layer in the critic), the last link of an image gradient (saliency maps, input perturbations; sgg_amd/grad.py):
 *   dx [B][H][W][3] = sum_{kh,kw,co} dy[b, y+1-kh, x+1-kw, co] * w_hwio[kh][kw][ci][co]      3x3, stride 1, SAME (pad_t = pad_l = 1)
 * from dy [B][H][W][32].  Exact f32 (fmaf chains) in every precision mode, fixed summation order (two calls are bit-equal); any
 * B, H, W.  sgg_conv2d_nhwc_dgrad rejects Cin == 3. */
int sgg_conv2d_nhwc_dgrad_c3(const float* dy, const float* w_hwio, float* dx, int B, int H, int W, int pad_t, int pad_l, void* stream);
/* The same with dy COMPUTED inside the kernel from the LayerNorm backward's operands, as sgg_conv2d_nhwc_wgrad_c3_ln does:
 *   dy = rstd * (da * ELU'(n) * gamma - m1 - xhat * m2),  xhat = (y - mean) * rstd,  n = xhat * gamma + beta
 * y, da [B][H][W][32]; stats [B][2] = (mean, rstd) of the forward; means [B][2] from sgg_layernorm_hwc_elu_bwd_sums.  dy is never
 * written: one read of y and da replaces the apply pass and the plain kernel's read of dy.  Whole planes only. */
int sgg_conv2d_nhwc_dgrad_c3_ln(const float* y, const float* da, const float* gamma, const float* beta, const float* stats,
                                const float* means, const float* w_hwio, float* dx, int B, int H, int W, int pad_t, int pad_l,
                                void* stream);

/* dgamma == dbeta == NULL in sgg_layernorm_hwc_elu_bwd DEFERS the parameter-gradient reductions (dgamma, dbeta, dbias_prev): the
 * partial sums stay in `workspace` (give every layer its own), and one launch of sgg_layernorm_hwc_bwd_finalize reduces up to 16
 * layers at once (an encoder backward: eleven 20-microsecond launches off its critical path). */
typedef struct {
  const void* workspace;   /* as left by sgg_layernorm_hwc_elu_bwd(…, dgamma = NULL, …) with the same B, HW, C */
  const float* gamma;
  const float* stats;
  float* dgamma;
  float* dbeta;
  float* dbias_prev;       /* may be NULL */
  int B, HW, C, HW_valid;  /* HW_valid: pixels of the valid window (= HW without one) */
} sgg_ln_finalize_desc;
int sgg_layernorm_hwc_bwd_finalize(const sgg_ln_finalize_desc* layers, int n_layers, void* stream);

/* ---- initial LSTM state: tf.reduce_mean(downsampled, axis=(1,2)) -------------------------------------------
 * generator_with_attention.py:76-77.  Rows r in [0,R) use image r % B (R/B passes share one feature map). */
int sgg_spatial_mean_fwd(const float* ctx, float* out_c, int ldc, float* out_h, int ldh, int R, int B, int L, int C,
                         void* stream);
int sgg_spatial_mean_bwd(const float* dc0, int ldc, const float* dh0, int ldh, float* dctx, int R, int B, int L, int C,
                         int accumulate, void* stream);

/* ---- dense contractions on f32 MFMA: tf.layers.dense / LSTM kernel matmul / tf.matmul(indices, W) ----------
 * generator_with_attention.py:15,87,88; discriminator_with_attention.py:15,87,89,90.
 *   fwd   C[M,N] (+)= A[M,K] B[K,N] (+ bias[N])
 *   dgrad C[M,N] (+)= A[M,K] B[N,K]^T
 *   wgrad C[M,N] (+)= A[K,M]^T B[K,N]
 * Split-K partial slabs go to `workspace` (sgg_gemm_workspace_bytes). */
size_t sgg_gemm_workspace_bytes(int M, int N, int K);
int sgg_gemm_skinny_fwd(int M, int N, int K, const float* A, int lda, const float* B, int ldb, float* C, int ldc,
                        const float* bias, int accumulate, void* workspace, size_t workspace_bytes, void* stream);
int sgg_gemm_skinny_dgrad(int M, int N, int K, const float* A, int lda, const float* B, int ldb, float* C, int ldc,
                          int accumulate, void* workspace, size_t workspace_bytes, void* stream);
int sgg_gemm_skinny_wgrad(int M, int N, int K, const float* A, int lda, const float* B, int ldb, float* C, int ldc,
                          int accumulate, void* workspace, size_t workspace_bytes, void* stream);
/* The kernels the launch with these scalars starts (mode 0 = fwd, 1 = dgrad, 2 = wgrad), in launch order and separated by ';',
 * spelled as rocprofv3 prints them with spaces removed and every template argument written out, for instance
 * "gemm_wk_kernel<2,false,4>" or "gemm_kernel<false,true>;gemm_slab_reduce_wide_kernel".  *nsplit (may be NULL) = the K ranges
 * the slab kernels split into (1: no slabs).  A pure host function: the launch's own validation and route, no GPU.  The route
 * does not depend on pointers or leading dimensions (those only choose between vector and scalar loads inside a kernel).
 * buf_len >= 96. */
int sgg_gemm_skinny_symbol(int mode, int M, int N, int K, int* nsplit, char* buf, int buf_len);
/* the step-invariant part of the attention perceptron, ctx_flat[B, L*C] x W_ctx[L*C, L] (same kernels, named
 * for the call site generator_with_attention.py:15) */
int sgg_attn_ctx_gemm_fwd(int B, int L, int LC, const float* ctx_flat, const float* w_ctx, const float* bias, float* P,
                          void* workspace, size_t workspace_bytes, void* stream);
int sgg_attn_ctx_gemm_dgrad(int B, int L, int LC, const float* dP, const float* w_ctx, float* dctx_flat, int accumulate,
                            void* workspace, size_t workspace_bytes, void* stream);
int sgg_attn_ctx_gemm_wgrad(int B, int L, int LC, const float* ctx_flat, const float* dP, float* dw_ctx, int accumulate,
                            void* workspace, size_t workspace_bytes, void* stream);

/* ---- tf.matmul(indices, W) with one-hot indices = embedding row gather ----------------------------------------
 * discriminator_with_attention.py:86-87 on the real triples (float one-hots, train.py:173).
 *   fwd  out[r, 0:E] = W[labels[r * label_stride], :]   (zero row for a label outside [0, V), as tf.one_hot)
 *   bwd  dW[labels[r * label_stride], :] += dY[r, 0:E]  (rows sharing a label summed in row order: deterministic) */
int sgg_embed_gather_fwd(const long long* labels, int label_stride, const float* W, int V, int E, float* out, int ldo, int R,
                         void* stream);
int sgg_embed_gather_bwd(const long long* labels, int label_stride, const float* dY, int lddy, float* dW, int V, int E, int R,
                         void* stream);

/* ---- attentionMechanism: score add -> softmax over L -> weighted sum of feature rows ------------------------
 * generator_with_attention.py:13-18 / discriminator_with_attention.py:13-18.
 *   e[r,:] = P[r % B,:] + ec[r,:]   (ec = c @ W_c, by sgg_gemm_skinny_fwd)
 *   alpha = softmax(e);  z[r,:] = sum_l alpha[r,l] * ctx[r % B, l, :]
 * bwd: de (cotangent of ec), dP[b,:] (+)= sum over its rows, dctx[b] (+)= alpha (x) dz.  With the *_dual
 * pointers it is the dual-number evaluation used for the gradient-penalty term ("bwd2"). */
int sgg_attn_step_fwd(const float* P, const float* ec, const float* ec_dual, int ldec, const float* ctx, float* alpha,
                      float* alpha_dual, float* z, float* z_dual, int ldz, int R, int B, int L, int C, void* stream);
int sgg_attn_step_bwd(const float* ctx, const float* alpha, const float* alpha_dual, const float* dz,
                      const float* dz_dual, int lddz, float* de, float* de_dual, float* dP, float* dctx, int R, int B,
                      int L, int C, int accumulate, void* stream);
/* The kernels those two launches start for these scalars (dual != 0: the *_dual pointers are given), in the spelling of
 * sgg_gemm_skinny_symbol, for instance "attn_step_bwd_ctx_kernel<Dual>;attn_step_bwd_softmax_kernel<Dual>".  Pure host
 * functions; they refuse what the launches refuse, with the same sgg_last_error text.  buf_len >= 96. */
int sgg_attn_step_fwd_symbol(int R, int B, int L, int C, int dual, char* buf, int buf_len);
int sgg_attn_step_bwd_symbol(int R, int B, int L, int C, int dual, char* buf, int buf_len);

/* ---- tf.contrib.rnn.LayerNormBasicLSTMCell(512) pointwise part ---------------------------------------------
 * generator_with_attention.py:79,87 / discriminator_with_attention.py:81,89.  gates = [x,h] @ kernel, [R,2048] in
 * the order i, j, f, o.  ln_params = [10][512]: gamma,beta of scopes input, transform, forget, output, state.
 * One wave per row; wave-level reductions for the five LayerNorms. pgrad: [R][10][512] per-row LN-parameter
 * gradients (sum the rows with sgg_colsum). */
int sgg_lnlstm_gates_fwd(const float* gates, const float* gates_dual, const float* c_prev, const float* c_prev_dual,
                         const float* ln_params, float* c_new, float* c_new_dual, float* h_new, float* h_new_dual,
                         int ldh, int R, void* stream);
int sgg_lnlstm_gates_bwd(const float* gates, const float* gates_dual, const float* c_prev, const float* c_prev_dual,
                         const float* ln_params, const float* dh, const float* dh_dual, int lddh, const float* dc_new,
                         const float* dc_new_dual, float* dgates, float* dgates_dual, float* dc_prev,
                         float* dc_prev_dual, float* pgrad, int R, void* stream);
size_t sgg_colsum_workspace_bytes(int rows, int cols);
int sgg_colsum(const float* X, int rows, int cols, int ld, float* out, int accumulate, void* workspace,
               size_t workspace_bytes, void* stream);

/* ---- WGAN-GP loss: tf.contrib.gan.gan_loss(wasserstein_*, gradient_penalty_weight, one_sided) ---------------
 * train.py:245-250 */
int sgg_onehot(const long long* labels, float* out, int rows, int V, void* stream);            /* train.py:173 */
int sgg_interpolate(const float* real, const float* fake, const float* alpha, float* out, int B, int n, void* stream);
int sgg_wgan_gp_loss_fwd(const float* g, float* slopes, float* pen, int B, int n, void* stream);
int sgg_wgan_gp_loss_bwd(const float* g, const float* slopes, const float* pen, float* v, int B, int n, float scale,
                         void* stream);
/* out4 = { disc_cost, wasserstein distance term, gradient penalty, mean D(fake) }  (gen_cost = -out4[3]) */
int sgg_wgan_losses(const float* d_out, const float* pen, float lam, int B, int T, int has_real, float* out4, void* stream);

/* ---- input pipeline: tf.image.resize_images(decoded, [221, 221]) + standardisation: train.py:171-172 ---------------------
 * TF 1.x bilinear resize with its defaults (align_corners=False: legacy grid src = dst * in/out, no antialiasing) of B RGB
 * uint8 images of different sizes ([H_b][W_b][3] at src + offsets[b], device memory) into dst [B][out_h][out_w][3] fp32,
 * then (x - means[c]) / stds[c]. */
int sgg_resize_bilinear_tf1(const unsigned char* src, const long long* offsets, const int* heights, const int* widths, float* dst,
                            int B, int out_h, int out_w, const float* means, const float* stds, void* stream);

/* ---- tf.train.AdamOptimizer(1e-4, beta1=0.5, beta2=0.9).minimize: train.py:258-266 ---------------------------
 * lr_t = lr*sqrt(1-beta2^t)/(1-beta1^t) is computed by the caller; theta -= lr_t*m/(sqrt(v)+eps). */
int sgg_adam_tf_multi(float* params, const float* grads, float* m, float* v, long long n, float lr_t, float beta1,
                      float beta2, float eps, float grad_scale, void* stream);

/* ---- tf.train.ExponentialMovingAverage of the trained variables (csrc/optim.hip) ------------------------------------------
 * The reference never averages its weights; its framework ships the op, and evaluating a WGAN-GP generator on the average of its
 * iterates is the usual remedy for the noise of the last one.
 * sgg_adam_tf_multi_ema: sgg_adam_tf_multi and, in the same pass, the shadow update of the average on the new parameter value:
 *   ema -= (ema - params_new) * one_minus_decay    in fp32 (one_minus_decay = 1 - min(decay, (1 + k) / (10 + k)) for the k-th
 *   update, formed by the caller in double: sgg_amd/ema.py).  params, m and v come out bit-identical to sgg_adam_tf_multi on the
 *   same inputs.  Nine streams of n words instead of seven.  All five pointers 16-byte aligned; `ema` must not overlap any other
 *   operand (argument error); 0 <= one_minus_decay <= 1.
 * sgg_swap_f32: exchanges a[0 .. n) and b[0 .. n) bit for bit (values are moved, never computed with: NaN payloads and -0.0
 *   survive).  Both 16-byte aligned, the ranges must not overlap (argument error). */
int sgg_adam_tf_multi_ema(float* params, const float* grads, float* m, float* v, float* ema, long long n, float lr_t, float beta1,
                          float beta2, float eps, float grad_scale, float one_minus_decay, void* stream);
int sgg_swap_f32(float* a, float* b, long long n, void* stream);

/* ---- gradient accumulation over micro-batches (csrc/optim.hip) ---------------------------------------------------------------
 * The reference takes every update from one minibatch; every loss term is a mean over rows and no op couples samples, so the mean
 * of the gradients of N equal micro-batches is the gradient of their union (sgg_amd/step.py: Network.end_micro_batch).
 * acc[i] = g[i] (first != 0; a bit copy) or acc[i] = acc[i] + g[i] (one fp32 addition per element; no atomics: the result is a pure
 * function of the inputs).  Both 16-byte aligned, n > 0, the ranges must not overlap (argument error, nothing is launched). */
int sgg_grad_accumulate(float* acc, const float* g, long long n, int first, void* stream);

/* ---- guarded updates: global-norm clipping and the non-finite skip, decided on the device (csrc/guard.hip, csrc/optim.hip) -----
 * The reference clips nothing and checks nothing; a trainer of its kind is expected to bound an outlier update by the gradient's
 * global norm and to drop an update whose gradient is not finite.  Both decisions need a reduction over the whole gradient arena;
 * it is taken on the device and consumed by the Adam pass from device memory - no host read-back.
 * sgg_grad_guard: reads grads[0 .. n) and writes `record`, eight fp64 values that persist from call to call:
 *   per element x = grads[i] * grad_scale in fp32, as sgg_adam_tf_multi forms it; a finite x adds (double)x * (double)x to ss, a
 *   non-finite one (Inf, NaN: the test of sgg_arena_stats) is only counted.
 *     [0] ss     sum of squares of the finite elements          [1] the non-finite count
 *     [2] norm   sqrt(ss) in fp64
 *     [3] coef   (max_norm > 0 && norm > max_norm) ? (double)max_norm / norm : 1.0
 *     [4] s_eff  (double)(float)((double)grad_scale * coef): the gradient scale the guarded Adam pass applies
 *     [5] apply  (skip_nonfinite && [1] > 0) ? 0.0 : 1.0
 *     [6] += 1 if coef < 1 and apply (updates clipped so far)   [7] += 1 if apply == 0 (updates skipped so far)
 *   [6] and [7] are read-modify-written by one thread: the caller zero-fills the record once.  coef is EXACTLY 1 while the
 *   threshold is not exceeded - on purpose not TF's clip_norm * min(1 / norm, 1 / clip_norm), from which it differs by at most an
 *   ulp: a run whose threshold is never reached stays bit-identical to an unguarded one.  With skip_nonfinite = 0 and non-finite
 *   elements present, norm is that of the finite elements and the step is applied as without a guard.
 *   Two launches on `stream`: per-chunk rows (chunks of sgg_arena_stats_chunk() elements of the flat range) into `workspace`
 *   (sgg_grad_guard_workspace_bytes(n), plain stores), then one workgroup sums the rows in a fixed order and writes the record.  No
 *   atomics: bit-identical from call to call and for every `grid` (workgroups of the first launch; 0 = the default,
 *   min(chunks, 4096)).  grads 16-byte aligned, record and workspace 8-byte aligned, n > 0, max_norm finite and >= 0 (0 = no
 *   clipping), grad_scale finite (argument errors, nothing is launched); a workspace too small: SGG_ERR_WORKSPACE.
 * sgg_adam_tf_multi_guarded / sgg_adam_tf_multi_ema_guarded: sgg_adam_tf_multi / sgg_adam_tf_multi_ema with `record` (device, as
 *   sgg_grad_guard left it on the same stream) in place of grad_scale.  record[5] == 0: the kernel writes nothing - params, m, v
 *   and ema keep every bit, NaN payloads included.  Otherwise the results are bit-identical to the unguarded entry point called
 *   with grad_scale = (float)record[4].  Pointer rules of the unguarded entry points; record 8-byte aligned. */
size_t sgg_grad_guard_workspace_bytes(long long n);
int sgg_grad_guard(const float* grads, long long n, float grad_scale, float max_norm, int skip_nonfinite, int grid, void* workspace,
                   size_t workspace_bytes, double* record, void* stream);
int sgg_adam_tf_multi_guarded(float* params, const float* grads, float* m, float* v, long long n, float lr_t, float beta1,
                              float beta2, float eps, const double* record, void* stream);
int sgg_adam_tf_multi_ema_guarded(float* params, const float* grads, float* m, float* v, float* ema, long long n, float lr_t,
                                  float beta1, float beta2, float eps, const double* record, float one_minus_decay, void* stream);

/* ---- tf.argmax(x, axis=-1): train.py:270-271 ----------------------------------------------------------------
 * out[r] = the first index of the maximum over the non-NaN entries of row r (x + r * ld, V entries, ld >= V).  A NaN entry is never
 * selected; a row without a non-NaN entry gives 0: every token is in [0, V). */
int sgg_argmax_rows(const float* x, long long* out, int rows, int V, int ld, void* stream);

/* ---- scene-graph prediction: score_accumulator.argsort() and the top-k selection, train.py:314-327 -----------
 * The host side of the reference's evaluation (accumulate the N sampled triples of an image and their critic scores, argsort,
 * take the first k) as one workgroup per image, extended to what a prediction needs: the DISTINCT triples in ranked order.
 *   tokens int64 [N][nb][3] (sample k of image j at [k][j]; every token in [0, V)), d fp32 [N][nb][3] (the critic's three outputs).
 *   score[k] = ((d0 + d1) + d2) / 3 in fp32 with a correctly rounded division (= numpy's float32 mean over the three steps).
 *   Order: ascending score (descending = 1: descending), ties by the smaller sample index, NaN scores last in sample order in
 *   both directions (ascending: np.argsort(score, kind="stable")).  A sample whose three tokens equal those of an earlier one in
 *   that order is a duplicate of it.  For image j and u < min(n_distinct[j], K), slot [j][u] holds the u-th distinct triple:
 *   triples int64 [nb][K][3], scores fp32 [nb][K] (of its first = best-ranked occurrence), first_rank int32 [nb][K] (position of
 *   that occurrence among the N ordered samples), first_sample int32 [nb][K] (its sample index k), counts int32 [nb][K] (how many
 *   of the N samples are this triple).  Slots u >= n_distinct[j] hold -1, NaN, -1, -1, 0.  sample_scores (optional, may be NULL):
 *   fp32 [nb][N], the per-sample scores.  1 <= K <= N <= 4096, 1 <= V <= 2^21. */
int sgg_rank_triples(const long long* tokens, const float* d, int N, int nb, int V, int K, int descending, long long* triples,
                     float* scores, int* first_rank, int* first_sample, int* counts, int* n_distinct, float* sample_scores,
                     void* stream);

/* ---- scene-graph metrics: the ground truth matched against the ranked distinct list --------------------------------------
 * Where each ground-truth triple of an image stands in that image's ranked list of distinct predictions (sgg_rank_triples), one
 * workgroup per image.
 *   ranked int64 [nb][K][3], n_distinct int32 [nb]: outputs of sgg_rank_triples; image j's list is its first
 *   U_j = min(n_distinct[j], K) rows, the rows behind U_j are never read.  gt int64 [nb][M][3], gt_count int32 [nb]: image j has
 *   gt_count[j] ground-truth rows, the rows m >= gt_count[j] are padding with arbitrary content.
 *   pos int32 [nb][M]:  u >= 0  row m equals ranked[j][u] (at most one u: the list is distinct);
 *                       -1      valid row, absent from the list;
 *                       -2      valid row equal to an earlier row m' < m of the image (the smallest row carries the result);
 *                       -3      padding row;
 *                       -4      valid row with a token outside [0, V): never matches, never merges with another row, not counted.
 *   n_gt int32 [nb]: rows with pos >= -1, the distinct valid ground-truth triples of the image.
 *   1 <= K <= 4096, 1 <= M <= 4096, 1 <= V <= 2^21.  gt_count and n_distinct are device arrays and are NOT checked on the host:
 *   the kernel clamps them to [0, M] and [0, K].  All results are integers: two launches give the same bits. */
int sgg_match_triples(const long long* ranked, const int* n_distinct, int nb, int K, const long long* gt, const int* gt_count, int M,
                      int V, int* pos, int* n_gt, void* stream);

/* ---- K-best decoding: ranked distinct triples from the generator's softmax (csrc/kbest.hip) --------------------------------
 * The three decoder outputs of a head row (generator_with_attention.py:88, the tf.layers.dense of each step) depend on the noise and
 * the LSTM state, never on the token of the step before: given one noise vector the distribution over triples is the product of
 * the three softmaxes.  Finite logits are a precondition of both entry points.
 * sgg_kbest_triples: the K most probable triples of every head row, one workgroup per row.
 *   logits fp32 [R][3][V], rows `ld` >= 3 V floats apart.  lse fp32 [R][3]: the log-sum-exp of each slot, stabilised by its maximum,
 *   fixed summation order.  a_t(x) = logits[t][x] - lse[t] and lp(s, p, o) = (a_0(s) + a_1(p)) + a_2(o), fp32 in that association.
 *   Tokens of a slot rank by (logit descending, token ascending); triples rank by (lp descending, then the tuple of slot ranks
 *   (i, j, l) ascending lexicographically).  triples int64 [R][K][3] and logp fp32 [R][K]: the first K triples in that order and
 *   their lp.  Exact: only the top min(K, V) tokens of a slot and the rank tuples with (i+1)(j+1)(l+1) <= K can take part (at most
 *   2045 at K = 128).  R >= 1, 1 <= V <= 2^21, 1 <= K <= min(128, V^3).  Two calls give the same bits.
 * sgg_kbest_merge: the lists of an image's N samples merged into one ranked distinct list, one workgroup per image.
 *   lists int64 [N][nb][Kc][3] (sample k of image j is row k * nb + j, as everywhere; the triples of one list are distinct - the
 *   output of sgg_kbest_triples on the same logits), logits and ld as above with R = N * nb, lse fp32 [N][nb][3].  An entry with a
 *   token outside [0, V) is ignored.  For every distinct triple c of the image's N * Kc entries and EVERY sample k (whether or not
 *   its own list held c): lp_k(c) from logits and lse as above; m = max_k lp_k(c);
 *   score(c) = m + (log(sum_k exp(lp_k(c) - m)) - log N), summed in sample order in fp32: the log-probability of c under the
 *   mixture of the N noise draws.  Order: score descending, ties by the packed triple (s, p, o) ascending.  For image j and
 *   u < min(n_distinct[j], K): triples int64 [nb][K][3], scores fp32 [nb][K], best_sample int32 [nb][K] (the smallest k with
 *   lp_k = m), best_logp fp32 [nb][K] (m), counts int32 [nb][K] (the lists that hold c); n_distinct int32 [nb].  Slots behind
 *   n_distinct[j] hold -1, NaN, -1, NaN, 0.  triples / n_distinct have the layout of sgg_rank_triples (sgg_match_triples takes
 *   them).  N = 1: the list itself.  N > 1: the candidates are the union of the N lists, which approximates the mixture's own K
 *   best (a triple that is in no sample's list cannot appear).  N * Kc <= 4096, 1 <= K <= N * Kc, 1 <= V <= 2^21. */
int sgg_kbest_triples(const float* logits, long long ld, int R, int V, int K, long long* triples, float* logp, float* lse,
                      void* stream);
int sgg_kbest_merge(const long long* lists, const float* logits, long long ld, const float* lse, int N, int nb, int Kc, int V, int K,
                    long long* triples, float* scores, int* best_sample, float* best_logp, int* counts, int* n_distinct,
                    void* stream);

/* ---- grounded scene graphs: entity instances from the pooled attention of an image's samples (csrc/ground.hip) ---------------
 * From the ranked distinct triples of an image (sgg_rank_triples / sgg_kbest_merge) and the generator's attention rows of its N
 * samples to the nodes of a scene graph of entity INSTANCES.  The definitions are stated in fp64 by sgg_amd/ground.py
 * (ground_reference).  Three launches, no host read-back between them, no float atomics: two calls give the same bits.
 * n_distinct is a device array and is clamped to [0, K]: U_j = min(n_distinct[j], K).
 * sgg_ground_assign: which samples are which slot; one workgroup per image.
 *   tokens int64 [N][nb][3], triples int64 [nb][K][3].  slot_of_sample int32 [nb][N]: the slot u < U_j whose triple equals the
 *   sample's three tokens (the smallest such slot, should the list not be distinct), -1 when there is none or a token lies outside
 *   [0, V).  members int32 [nb][N]: the assigned samples grouped by slot, ascending sample inside a slot, -1 in the tail of
 *   unassigned samples.  start int32 [nb][K + 1]: the members of slot u are members[j][start[u] .. start[u + 1]); start[u] =
 *   start[U_j] for u >= U_j.  1 <= N <= 4096, 1 <= K <= 4096, 1 <= V <= 2^21.
 * sgg_ground_pool: the mean attention of every slot's members; one workgroup per (slot, image).
 *   alpha0 / alpha1 / alpha2 fp32: the attention of decoding step t (subject, predicate, object), row k * nb + j of sample k of
 *   image j, rows lda >= L floats apart (plane 0 of the head's attention buffers: not copied).  members, start: as above.
 *   maps fp32 [nb][K][3][L]: the mean of the member rows in member order, fp32, one division.  A slot without a member takes the
 *   single row fallback_sample[j][u] (int32 [nb][K]: first_sample / best_sample of the ranking), or zeros when that lies outside
 *   [0, N).  n_pooled int32 [nb][K]: the number of members (0 when the fallback was used).  Slots u >= U_j: zeros and 0.
 *   1 <= N <= 4096, 1 <= K <= 4096, 1 <= nb <= 65535, 1 <= L <= 2^20.
 * sgg_ground_resolve: mentions joined into nodes; one workgroup per image.
 *   Mention m = 2u + r of slot u < U_j (r = 0 subject, 1 object) has token triples[j][u][2r], map maps[j][u][2r] and weight
 *   max(n_pooled[j][u], 1).  ov(m, m') = sum_l min(a_l, b_l).  Two mentions are joined when their tokens are equal and
 *   ov >= overlap; the nodes are the connected components, numbered in the order of their smallest mention.
 *   mention_node int32 [nb][K][2] (-1 behind U_j), n_nodes int32 [nb]; per node n < n_nodes[j], in arrays of 2 K rows per image:
 *   node_word int64 (its token), node_first int32 (its smallest mention), node_weight int32 (sum of its mentions' weights),
 *   node_mentions int32, node_map fp32 [L] (sum_m w_m map_m / sum_m w_m over its mentions in ascending order, fp32), node_box
 *   int32 [4] = { y0, x0, y1, x1 } (inclusive: the smallest cell rectangle with every cell a >= box_frac * max a), node_center
 *   fp32 [2] = (sum a (y + 0.5), sum a (x + 0.5)) / sum a in cell units (NaN for an all-zero map).  Rows behind n_nodes[j] hold
 *   -1 (integers), 0 (node_map), NaN (node_center).  overlap and box_frac in (0, 1].  1 <= K <= 1024 (the pair work of an image
 *   whose mentions all share one word is quadratic in 2 K), Hf * Wf <= 2^20. */
int sgg_ground_assign(const long long* tokens, const long long* triples, const int* n_distinct, int N, int nb, int K, int V,
                      int* slot_of_sample, int* members, int* start, void* stream);
int sgg_ground_pool(const float* alpha0, const float* alpha1, const float* alpha2, long long lda, const int* members, const int* start,
                    const int* fallback_sample, const int* n_distinct, int N, int nb, int K, int L, float* maps, int* n_pooled,
                    void* stream);
int sgg_ground_resolve(const float* maps, const long long* triples, const int* n_distinct, const int* n_pooled, int nb, int K, int Hf,
                       int Wf, float overlap, float box_frac, int* mention_node, int* n_nodes, long long* node_word, int* node_first,
                       int* node_weight, int* node_mentions, float* node_map, int* node_box, float* node_center, void* stream);

/* ---- generator likelihood: softmax cross-entropy and the log-probability of given triples (csrc/xent.hip) -------------------
 * The likelihood K-best decoding ranks by (above), as a training objective and as a held-out measurement.  Finite logits are a
 * precondition of all three entry points; none uses a workspace or a float atomic, and two calls give the same bits.
 * sgg_softmax_xent: row-wise log-softmax cross-entropy, forward and gradient in one launch.
 *   Row r is logits[r * ld .. r * ld + V), ld >= V, any 4-byte alignment.  lse[r] = max + log(sum_j exp(x_j - max)), fixed summation
 *   order.  labels int64 [R].  For a label in [0, V): nll[r] = lse[r] - x[label]; hit[r] = 1 if label is the row's tf.argmax (the
 *   first index of the maximum, as sgg_argmax_rows), else 0; dlogits[r][j] = scale * (exp(x_j - lse[r]) - [j == label]), rows ldd >= V
 *   apart, stored (accumulate = 0) or added to what is there (accumulate = 1).  A label outside [0, V) SKIPS the row: nll = 0,
 *   hit = -1, its dlogits row zero-filled (accumulate = 0) or untouched (accumulate = 1); lse is written all the same.
 *   dlogits, nll, lse and hit may each be NULL (not all).  labels = NULL: the lse-only mode, dlogits = nll = hit = NULL.
 *   R >= 1, 1 <= V <= 2^21; element offsets are 64-bit.  V <= 1024: one wave per row, the row in registers; above: one workgroup
 *   per row, an online max / sum pass and a gradient pass that re-reads the row.
 * sgg_xent_summary: the numbers of a log line from nll / hit of R = 3 B rows, three consecutive rows per triple; one workgroup.
 *   Valid rows: hit >= 0.  out4 fp32 = { mean nll per valid row (nats per token; summed in fp64), share of valid rows with hit = 1,
 *   share of the all-valid triples whose three rows all hit, number of valid rows }; a share over nothing is 0.
 * sgg_triple_logp: the log-probability of given triples under the mixture of an image's N noise samples; one workgroup per image.
 *   logits fp32 [N * nb][3][V], rows ld >= 3 V apart, sample k of image j is row k * nb + j; lse fp32 [N][nb][3] (sgg_softmax_xent's
 *   lse-only mode on the R = N * nb * 3 slot rows, or sgg_kbest_triples').  gt int64 [nb][M][3], gt_count int32 [nb] as
 *   sgg_match_triples takes them (gt_count clamped to [0, M] on the device).  For a valid row (s, p, o): a_t(x) = logits[t][x] - lse[t],
 *   lp_k = (a_0(s) + a_1(p)) + a_2(o), m = max_k lp_k, mix = m + (log(sum_k exp(lp_k - m)) - log N), summed in sample order in fp32 -
 *   the arithmetic of sgg_kbest_merge's score, bit for bit.  mean fp32 [nb][M] = mean_k lp_k; slot fp32 [nb][M][3] = mean_k a_t.
 *   status int32 [nb][M]: 0 valid, -3 padding (m >= gt_count[j]), -4 a token outside [0, V); the float outputs of a row that is
 *   not valid hold NaN.  Duplicated rows are each scored.  1 <= N <= 4096, 1 <= M <= 4096, nb >= 1, 1 <= V <= 2^21. */
int sgg_softmax_xent(const float* logits, long long ld, int R, int V, const long long* labels, float scale, int accumulate,
                     float* dlogits, long long ldd, float* nll, float* lse, int* hit, void* stream);
int sgg_xent_summary(const float* nll, const int* hit, int R, float* out4, void* stream);
int sgg_triple_logp(const float* logits, long long ld, const float* lse, int N, int nb, int V, const long long* gt,
                    const int* gt_count, int M, float* mix, float* mean, float* slot, int* status, void* stream);

/* ---- image retrieval by triple query: the generator's likelihood ranked across images (csrc/retrieve.hip) -------------------
 * The other direction of the likelihood above: ONE list of Q (partial) triples scored against every image of a collection, and the
 * images ranked per query.  No entry point uses a workspace or a float atomic, and two calls give the same bits.
 * sgg_query_logp: the mixture log-probability of Q shared queries for the nb images of one batch; grid (image, query tile).
 *   logits, ld, lse, N, nb, V: as sgg_triple_logp takes them (finite logits are a precondition).  tok int32 [3][U]: per slot the
 *   distinct tokens the queries use, u0 / u1 / u2 <= U of them valid (built on the host; every token in [0, V) - one outside
 *   makes the scores of the queries that name it NaN, nothing is read out of bounds).  qidx int32 [Q][3]: per slot an index into
 *   that slot's list, or -1 for an unspecified slot (a wildcard); any other value makes the query's score NaN.
 *   a_t = logits[t][tok] - lse[t], or exactly 0.f for a wildcard (the slot is marginalised: its softmax sums to 1);
 *   lp_k = (a_0 + a_1) + a_2; score = m + (log(sum_k exp(lp_k - m)) - log N) with (m, sum) kept ONLINE over the samples in sample
 *   order (the sum rescaled by exp(m_old - m_new) when the maximum rises): the arithmetic of sgg_triple_logp's mix up to that
 *   summation.  A query of three wildcards scores 0.  scores[q * lds + col0 + j] for j < nb; nothing else is written.
 *   1 <= N <= 4096, 1 <= Q <= 4096, 1 <= U <= Q, 1 <= nb <= 65535, 1 <= V <= 2^21, 0 <= col0, col0 + nb <= lds.
 * sgg_retrieve_topk: per query the first K images of the row scores[q * lds .. + n_images) under the total order (score
 *   descending, image index ascending; +0 and -0 are equal); one workgroup per query.  idx int32 [Q][K], top fp32 [Q][K] (the
 *   scores' own bits); slots behind min(K, n_images) hold -1 and NaN.  Exact: a radix selection of the K-th key (seven passes over
 *   the row) and one sort of the K survivors.  1 <= K <= 1024, 1 <= n_images <= 2^21 <= lds.  Columns >= n_images are not read.
 * sgg_retrieve_ranks: where a query's relevant images stand in that order; one workgroup per query.
 *   rel_ptr int32 [Q + 1], rel_idx int32 [rel_ptr[Q]] (CSR; at least one entry allocated): the relevant images of query q are
 *   rel_idx[rel_ptr[q] .. rel_ptr[q + 1]), ascending, at most 4096, all in [0, n_images).  ranks int32, parallel to rel_idx: 1 + the
 *   number of images that precede the image in the total order (integers).  first_rank int32 [Q]: the smallest of them.
 *   ap fp64 [Q]: average precision = mean_i (i + 1) / rank_(i) over the ascending ranks, in fp64, fixed order.  status int32 [Q]:
 *   0 valid; -3 no relevant image (first_rank 0, ap NaN); -4 a list longer than 4096 or an index outside [0, n_images) (first_rank
 *   0, ap NaN, its ranks not written). */
int sgg_query_logp(const float* logits, long long ld, const float* lse, int N, int nb, int V, const int* tok, int U, int u0, int u1,
                   int u2, const int* qidx, int Q, float* scores, long long lds, long long col0, void* stream);
int sgg_retrieve_topk(const float* scores, long long lds, int Q, int n_images, int K, int* idx, float* top, void* stream);
int sgg_retrieve_ranks(const float* scores, long long lds, int Q, int n_images, const int* rel_ptr, const int* rel_idx, int* ranks,
                       int* first_rank, double* ap, int* status, void* stream);

/* ---- predicate classification: predicates ranked per entity pair, candidates ranked per image (csrc/predcls.hip) -------------
 * Given the (subject, object) pairs of an image, the likelihood above for EVERY predicate token of every pair, and the two rankings
 * the PredCls protocol needs.  No entry point uses a workspace, a float atomic or a host read-back, and two calls give the same bits.
 * sgg_pair_predicate_logp: grid (tile of 256 predicate columns, tile of 16 pairs, image), one thread per column.
 *   logits, ld, lse, N, nb, V: as sgg_triple_logp takes them (finite logits are a precondition).  pairs int32 [nb][P][2] = (s, o);
 *   pair_count int32 [nb], clamped to [0, P] on the device.  For a valid pair and a token v: lp_k(v) = (a_0(s) + a_1(v)) + a_2(o),
 *   m = max_k lp_k, joint(v) = m + (log(sum_k exp(lp_k - m)) - log N), summed in sample order in fp32 - bit for bit sgg_triple_logp's
 *   mix of (s, v, o).  marg = the same with a_1 = 0.f: the pair's log-probability with the predicate marginalised; joint(v) - marg is
 *   log p(v | s, o, image).  joint fp32: row j * P + p holds V floats, rows ldj >= V apart (columns >= V are never written);
 *   marg fp32 [nb][P]; status int32 [nb][P]: 0 valid, -3 padding (p >= pair_count[j]), -4 a token outside [0, V) - the float
 *   outputs of such a pair hold NaN, nothing is read out of bounds.  The draws are walked twice (maxima, then sums), 64 at a time:
 *   each predicate row is read once per walk and pair tile.  1 <= N <= 4096, 1 <= P <= 4096, 1 <= nb <= 65535, 1 <= V <= 2^21.
 * sgg_predcls_pair_topk: one workgroup per (pair, image).  top_tok int32 [nb][P][Kc], top_score fp32 [nb][P][Kc]: the first Kc
 *   tokens of the pair's joint row under (joint descending, token ascending; +0 and -0 equal) and their scores' own bits; slots
 *   behind min(Kc, V), and every slot of a pair with status != 0, hold -1 and NaN.  gt_pair int32 [nb][M] (the pair index of true
 *   triple m, or -1), gt_pred int32 [nb][M] -> gt_rank int32 [nb][M] = 1 + the number of tokens that precede gt_pred in its pair's
 *   order; 0 where gt_pair is outside [0, P), the pair is not valid or the token lies outside [0, V).  1 <= Kc <= 128,
 *   1 <= M <= 4096.
 * sgg_predcls_merge: one workgroup per image.  The candidates are (pair i, slot r < per_pair <= Kc) with top_tok >= 0, scored
 *   top_score - marg[i] (conditional = 1) or top_score (conditional = 0), ordered by (score descending, i ascending, r ascending);
 *   the first K: triples int64 [nb][K][3] = (pairs[i][0], token, pairs[i][1]), scores fp32 [nb][K], src int32 [nb][K] =
 *   i * per_pair + r, n_distinct int32 [nb] = the number of candidates (it may exceed K); slots behind it hold -1 / NaN / -1: the
 *   layout of sgg_rank_triples, which sgg_match_triples takes.  per_pair = 1 lists one predicate per pair (the graph constraint).
 *   The pairs of an image must be distinct.  P * per_pair <= 2^21, 1 <= K <= 1024. */
int sgg_pair_predicate_logp(const float* logits, long long ld, const float* lse, int N, int nb, int V, const int* pairs,
                            const int* pair_count, int P, float* joint, long long ldj, float* marg, int* status, void* stream);
int sgg_predcls_pair_topk(const float* joint, long long ldj, const int* status, int nb, int P, int V, int Kc, const int* gt_pair,
                          const int* gt_pred, int M, int* top_tok, float* top_score, int* gt_rank, void* stream);
int sgg_predcls_merge(const int* pairs, const int* top_tok, const float* top_score, const float* marg, int nb, int P, int Kc,
                      int per_pair, int conditional, int K, long long* triples, float* scores, int* src, int* n_distinct, void* stream);

/* ---- relaxed generator output: softmax / Gumbel-softmax rows for the critic, and their gradient (csrc/relax.hip) ---------------
 * The critic's fake rows as points of the probability simplex instead of raw decoder logits.  Neither entry point uses a workspace
 * or a float atomic, and two calls give the same bits.  Rows are any 4-byte alignment; element offsets are 64-bit.  R >= 1,
 * 1 <= V <= 2^21, tau finite and > 0; anything else is refused without a launch.
 * sgg_relax_rows: y[r][j] = exp(z_j - max z) / sum_k exp(z_k - max z) with z = (x[r] + g) / tau; x rows ldx >= V apart, y rows
 *   ldy >= V apart.  y may BE x (same pointer, then ldy == ldx): the row is relaxed in place.  gumbel = 0: g = 0.  gumbel = 1: g is
 *   drawn in the kernel, a pure function of (seed, draw, r, j): Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter
 *   (j >> 2, r, draw & 0xffffffff, draw >> 32); element j takes output word w = out[j & 3]; u = ((w >> 9) + 0.5) * 2^-23, exact in
 *   fp32 and strictly inside (0, 1); g = -log(-log u).  u_out (optional, gumbel = 1 only, rows ldu >= V apart, a buffer of its own)
 *   receives u.  Finite x is a precondition.
 * sgg_relax_rows_bwd: dx[r][j] = (scale / tau) * y_j * (dy_j - sum_k y_k dy_k) - the gradient of scale * <dy, y> by x for y of
 *   sgg_relax_rows, with either value of gumbel; it needs neither x nor the noise.  dx may BE dy (then lddx == lddy), not y.
 * V <= 1024: one wave per row, the row in registers; above: one workgroup per row, a reduction pass and a pass that re-reads the
 * row and writes it. */
int sgg_relax_rows(const float* x, long long ldx, int R, int V, float tau, int gumbel, unsigned long long seed, unsigned long long draw,
                   float* y, long long ldy, float* u_out, long long ldu, void* stream);
int sgg_relax_rows_bwd(const float* y, long long ldy, const float* dy, long long lddy, int R, int V, float tau, float scale, float* dx,
                       long long lddx, void* stream);
/* The straight-through (hard) pair: the critic sees one-hot rows, the generator's update takes the soft row's gradient.
 * sgg_relax_rows_hard: k_r = the FIRST index that maximises the fp32 s_j = x[r][j] (gumbel = 0) or x[r][j] + g_j (gumbel = 1, g formed
 *   exactly as sgg_relax_rows forms it: one fp32 add).  No tau: the argmax is taken before any scaling.  y[r][j] = 1.0f at j = k_r,
 *   +0.0f elsewhere; tok[r] = k_r (int64).  Either output may be null, not both; tok alone with gumbel = 1 is a Gumbel-max sample
 *   from softmax(x[r]).  y may BE x (then ldy == ldx).  Finite x is a precondition (a row of NaN gives k_r = 0).
 * sgg_relax_rows_hard_bwd: dx[r][j] = (scale / tau) * y_j * (dy_j - sum_k y_k dy_k) with y = softmax((x + g) / tau) recomputed from x
 *   and the noise of (seed, draw) as sgg_relax_rows computes it - the input buffer of the critic holds the one-hot row, not y.
 *   dx may BE dy (then lddx == lddy), not x.
 * V <= 1024: one wave per row (the backward: x and dy in registers); above: one workgroup per row - the forward reads and draws
 * the row once and writes it behind the barrier without reading; the backward reads x and dy and draws the noise in both passes. */
int sgg_relax_rows_hard(const float* x, long long ldx, int R, int V, int gumbel, unsigned long long seed, unsigned long long draw,
                        float* y, long long ldy, long long* tok, void* stream);
int sgg_relax_rows_hard_bwd(const float* x, long long ldx, const float* dy, long long lddy, int R, int V, float tau, float scale,
                            int gumbel, unsigned long long seed, unsigned long long draw, float* dx, long long lddx, void* stream);

/* ---- score-function (REINFORCE) generator update: the policy gradient of sampled triples (csrc/score.hip) ----------------------
 * The decoder rows x are a policy p = softmax(x); tokens sampled from it (sgg_relax_rows_hard with tok and gumbel = 1) were scored by
 * the critic, and the generator's gradient needs nothing of the critic but those scores.  None of the three uses a workspace or a
 * float atomic, and two calls give the same bits; element offsets are 64-bit; anything outside the stated ranges is refused without
 * a launch.
 * sgg_score_advantage: one workgroup.  d_out fp32 [B][T], rows ldd >= T apart: the critic's outputs of sample b.
 *   r_b = (sum_t d_out[b][t]) / T, summed in fp32 in order of t; S = sum_b r_b in fp64 in order of b.  baseline = 0 (none):
 *   adv[b] = r_b.  baseline = 1 (leave-one-out): adv[b] = (float)(r_b - (S - r_b) / (B - 1)) in fp64, the reward against the mean of
 *   the OTHER rewards; it needs B >= 2.  out2 (optional) fp32 = { mean_b r_b, mean_b adv[b]^2 }, summed in fp64 in order of b.
 *   1 <= B <= 2^20, 1 <= T <= 64.
 * sgg_score_rows: row r is x[r * ldx .. r * ldx + V), ldx >= V, any 4-byte alignment.  lse = max + log(sum_j exp(x_j - max)),
 *   p_j = exp(x_j - lse), H_r = lse - sum_j p_j x_j (the row's entropy), w_r = coef * adv[r / group] (adv = NULL: w_r = coef; adv has
 *   ceil(R / group) entries).  tok int64 [R].  For a token a = tok[r] in [0, V):
 *   dx[r][j] = w_r (p_j - [j == a]) + ent_coef * p_j ((x_j - lse) + H_r) - the gradient of -w_r log p_a - ent_coef H_r by x - rows
 *   lddx >= V apart, stored (accumulate = 0) or added to what is there (accumulate = 1); logp[r] = x_a - lse; ent[r] = H_r.  A token
 *   outside [0, V) SKIPS the row as sgg_softmax_xent does: logp = 0, its dx row zero-filled (accumulate = 0) or untouched
 *   (accumulate = 1); ent is written all the same.  The token is read once per row and addresses no load or store.  dx, logp and ent
 *   may each be NULL (not all; without dx the row is read once).  dx must not BE x.  R >= 1, 1 <= V <= 2^21, group >= 1, coef and
 *   ent_coef finite; finite x is a precondition.  V <= 1024: one wave per row, the row in registers; above: one workgroup per row,
 *   an online pass for (max, sum exp, sum exp * x) and a gradient pass that re-reads the row.
 * sgg_score_summary: one workgroup.  out2 fp32 = { mean logp, mean ent } over the R rows, summed in fp64 in row order.
 *   1 <= R <= 2^24. */
int sgg_score_advantage(const float* d_out, long long ldd, int B, int T, int baseline, float* adv, float* out2, void* stream);
int sgg_score_rows(const float* x, long long ldx, int R, int V, const long long* tok, const float* adv, int group, float coef,
                   float ent_coef, int accumulate, float* dx, long long lddx, float* logp, float* ent, void* stream);
int sgg_score_summary(const float* logp, const float* ent, int R, float* out2, void* stream);

/* ---- score-function update with S samples per row (csrc/score.hip) -------------------------------------------------------------
 * S Gumbel-max samples of every decoder row in one launch, advantages against the other samples of the same image, one gradient
 * launch for all of them.  Layout everywhere: sample s of logits row r sits at index s * R + r (with R = B * T rows a sample's
 * tokens are a contiguous [B][T] block, and critic row s * B + b scores sample s of image b).  1 <= S <= 16.  No workspace, no
 * float atomic, fixed summation orders: two calls give the same bits; anything outside the stated ranges is refused without a launch.
 * sgg_sample_rows_multi: tok int64 [S][R]; tok[s][r] = the first argmax_j of x[r][j] + g_j with g drawn as sgg_relax_rows draws it at
 *   draw number draw | (s << 56) - bit for bit the tok of sgg_relax_rows_hard(gumbel = 1, seed, draw | (s << 56)); draw < 2^56.  A row
 *   of V <= 1024 stays in registers for all S draws; a longer row is read once for S <= 8 and twice for S <= 16.  No one-hot row is
 *   written and no load or store is addressed by a token.  1 <= R <= 2^24, 1 <= V <= 2^21, ldx >= V.
 * sgg_score_advantage_multi: one workgroup.  d_out fp32 [S * B][T], rows ldd >= T apart; r[s][b] = (sum_t d_out[s * B + b][t]) / T in
 *   fp32 in order of t.  baseline = 0 (none): adv = r.  1 (leave-one-out over all): adv[n] = r_n - (sum_all - r_n) / (S * B - 1), it
 *   needs S * B >= 2.  2 (image): adv[s][b] = r[s][b] - (sum_s' r[s'][b] - r[s][b]) / (S - 1), the reward against the mean of the
 *   OTHER samples of the same image; it needs S >= 2, B = 1 is allowed.  Sums in fp64 in index order.  adv fp32 [S * B]; out2
 *   (optional) fp32 = { mean r, mean adv^2 } over S * B.  1 <= B <= 2^20, 1 <= T <= 64.
 * sgg_score_rows_multi: x, lse, p, H_r, dx, accumulate, ent as sgg_score_rows.  tok int64 [S][R]; w_s = coef * adv[s * (R / group) +
 *   r / group] (adv = NULL: coef); R % group == 0.  With the sum over the samples s whose token a_s lies in [0, V):
 *   dx[r][j] = (sum_s w_s) p_j - sum_s w_s [j == a_s] + ent_coef * p_j ((x_j - lse) + H_r); logp fp32 [S][R]: logp[s][r] = x_{a_s} - lse.
 *   A token sampled twice counts twice.  A token outside [0, V) drops that sample's term alone (its logp = 0): the other samples'
 *   terms, the entropy term and the row's store stay.  The S tokens of a row are read once and address no load or store.
 * sgg_score_summary_multi: one workgroup.  out2 fp32 = { mean of logp[0 .. n_logp), mean of ent[0 .. n_ent) }, fp64 sums in index
 *   order.  1 <= n_logp <= 2^28, 1 <= n_ent <= 2^24. */
int sgg_sample_rows_multi(const float* x, long long ldx, int R, int V, int S, unsigned long long seed, unsigned long long draw,
                          long long* tok, void* stream);
int sgg_score_advantage_multi(const float* d_out, long long ldd, int B, int S, int T, int baseline, float* adv, float* out2, void* stream);
int sgg_score_rows_multi(const float* x, long long ldx, int R, int V, int S, const long long* tok, const float* adv, int group, float coef,
                         float ent_coef, int accumulate, float* dx, long long lddx, float* logp, float* ent, void* stream);
int sgg_score_summary_multi(const float* logp, int n_logp, const float* ent, int n_ent, float* out2, void* stream);

/* ---- training diagnostics: per-tensor norms and non-finite counts of a network's arenas (csrc/stats.hip) ----------------------
 * One read-only streaming pass over params, grads, m and v: fp32 arenas of ONE layout, every tensor 16-byte aligned and rounded up
 * to 4 elements (the arena ends on such a boundary), as sgg_adam_tf_multi takes them.
 *   chunk_table int64 [n_chunks][3] (device): (tensor, first arena element, count) per chunk, built by the host: a chunk lies inside
 *   ONE tensor, `first` is a multiple of 4, 1 <= count <= sgg_arena_stats_chunk(), the rows are sorted by tensor, tensors are
 *   numbered 0 .. n_tensors - 1.  The table is device data and is NOT checked here: the caller guarantees first + count rounded up
 *   to 4 <= the arenas' length.  Padding elements (behind a tensor's count) enter no statistic.
 *   Per element: g = grads * grad_scale and u = lr_t * m / (sqrtf(v) + eps), both in fp32 exactly as sgg_adam_tf_multi forms them
 *   (called right behind it with the same lr_t and eps, u is the delta that step applied, up to its sign).
 *   out fp64 [n_tensors][sgg_arena_stats_nstat() = 9]: (sum of squares, max |.|, non-finite count) of g, of the parameter, of u.
 *   Sums of squares (squares formed and summed in fp64) and maxima run over the FINITE elements; Inf and NaN are counted only.
 *   Two launches on `stream`: per-chunk rows into `workspace` (sgg_arena_stats_workspace_bytes(n_chunks), plain stores), then one
 *   wave per tensor sums its chunk rows in a fixed order.  No atomics: bit-identical from call to call and for every `grid`
 *   (workgroups of the first launch; 0 = the default, min(n_chunks, 4096)). */
int sgg_arena_stats_chunk(void);
int sgg_arena_stats_nstat(void);
size_t sgg_arena_stats_workspace_bytes(int n_chunks);
int sgg_arena_stats(const float* params, const float* grads, const float* m, const float* v, const long long* chunk_table,
                    int n_chunks, int n_tensors, float lr_t, float eps, float grad_scale, int grid, void* workspace,
                    size_t workspace_bytes, double* out, void* stream);
/* out fp64 [5] = { min, max, sum, count of x > threshold } over the finite elements of x [n] and the non-finite count; min = +Inf,
 * max = -Inf, sum = 0 when no element is finite.  One workgroup, fixed summation order; 1 <= n <= 2^20. */
int sgg_vector_stats(const float* x, int n, float threshold, double* out, void* stream);

int sgg_fill(float* p, long long n, float value, void* stream);

/* ---- training-time augmentation in the input kernel (csrc/augment.hip) ----------------------------------------------------------
 * Random crop, mirror and colour jitter of the loader's packed uint8 batch, drawn on the device and applied by the launch that resizes
 * and standardises it.  The reference has none (train.py:167-172 feeds every image pixel-identical every epoch).  numpy restatement:
 * tests/augment_ref.py; host path of the CPU loader: sgg_amd/augment.py.
 *
 * Amplitudes arrive as 16-bit fixed point, q = round(a * 65536):
 *   crop_q in [1, 65536]        the smallest side fraction of the crop box; 65536 = off: the box is the image
 *   flip_q in [0, 65536]        probability of mirroring the output; 0 = off
 *   brightness_q, contrast_q, saturation_q in [0, 65535]   factor in [1 - a, 1 + a]; 0 = off: factor exactly 1.0f, stage not executed
 *
 * The table, one row per example b, a pure function of (seed, draw = draw0 + b as a 64-bit sum, H_b, W_b, amplitudes, labels):
 *   box int32 [B][6] = y0, x0, ch, cw, flip, 0 (reserved)        factors fp32 [B][4] = brightness, contrast, saturation, grey mean
 * Philox4x32-10, key (seed & 0xffffffff, (seed >> 32) ^ 0x41554731) - seed is --seed, never the rank; the relaxation kernels key on
 * (rank, --seed) - counters (0, 0, draw lo, draw hi) -> words w0..w3 and (1, 0, draw lo, draw hi) -> w4..w7.  With r(w) = w >> 8:
 *   hmin = max(1, (H * crop_q + 65535) >> 16)     ch = hmin + (((H - hmin + 1) * r(w0)) >> 24)     y0 = ((H - ch + 1) * r(w1)) >> 24
 *   wmin, cw, x0 the same from W, w2, w3 (64-bit products)          flip = (w4 >> 16) < flip_q
 *   factor(a_q, w) = (float)(2^39 + a_q * (2 * (w >> 9) + 1 - 2^23)) * 2^-39: brightness from w5, contrast from w6, saturation w7
 * - integers throughout and ONE int64 -> fp32 conversion (round to nearest even) per factor, no transcendental function: 0 <= y0,
 * y0 + ch <= H always, crop_q = 65536 gives (0, 0, H, W), and numpy reproduces every row bit for bit.
 * Grey mean (contrast_q > 0 only, else 0.0f): the integer sum of 77 R + 150 G + 29 B over the SOURCE pixels of the box, 64 bits,
 * divided by 256 * ch * cw in fp64 and rounded once to fp32.  32 workgroups per image, one 64-bit integer atomic each into
 * `workspace` (sgg_augment_plan_workspace_bytes(B), 8-byte aligned, needed with contrast_q > 0 only): integer sums commute, the
 * result does not depend on the order.  No float atomics.
 * Labels: swap int32 [V] maps a word to the word with the tokens `left` and `right` exchanged (itself without them, -1 where the
 * vocabulary lacks the counterpart: sgg_amd/augment.py flip_swap_table).  An example whose triple holds a word with swap < 0 (or a
 * label outside [0, V)) is not mirrored: its flip is cleared.  labels_out int64 [B][3] = the remapped triple of a mirrored example,
 * labels_in's row otherwise.  B <= 65535.
 *
 * sgg_augment_resize: dst [B][out_h][out_w][3] fp32 from src and the table alone (`stages`: bit 0 saturation, bit 1 contrast, bit 2
 * brightness).  Every table row is clamped into its image first (ch to [1, H], y0 to [0, H - ch], ...; flip = box[4] != 0): no row
 * is followed out of the image.  Output pixel (y, x), with xs = flip ? out_w - 1 - x : x (the mirror of the unflipped output):
 *   the legacy TF-1.x grid of sgg_resize_bilinear_tf1 laid over the BOX: sy = (float)ch / out_h, fy = fl(y * sy), row y0 + floor(fy),
 *   upper neighbour min(floor(fy) + 1, ch - 1) - clamped to the box, not the image - and the same in x; every product rounded
 *   before it is added.  With stages = 0 the output equals sgg_resize_bilinear_tf1 on a copy of the box's pixels bit for bit.
 *   Then on the interpolated 0..255 values v_c:  saturation v = g + s (v - g), g = 0.299 v_r + 0.587 v_g + 0.114 v_b of that pixel;
 *   contrast v = m + c (v - m), m the grey mean;  brightness v = b v;  clamp to [0, 255] (only where a stage ran);
 *   (v - means[c]) / stds[c].  The colour stages are plain fp32 and may be fused: they are compared with fp64 (tests/augment_ref.py). */
size_t sgg_augment_plan_workspace_bytes(int B);
int sgg_augment_plan(const unsigned char* src, const long long* offsets, const int* heights, const int* widths, const long long* labels_in,
                     const int* swap, int V, int B, int crop_q, int flip_q, int brightness_q, int contrast_q, int saturation_q,
                     unsigned long long seed, unsigned long long draw0, int* box, float* factors, long long* labels_out, void* workspace,
                     size_t workspace_bytes, void* stream);
int sgg_augment_resize(const unsigned char* src, const long long* offsets, const int* heights, const int* widths, const int* box,
                       const float* factors, int stages, float* dst, int B, int out_h, int out_w, const float* means, const float* stds,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SGG_HIP_H */
