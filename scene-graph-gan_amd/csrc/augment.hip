// Training-time image augmentation inside the input kernel (include/sgg_hip.h, "training-time augmentation"): random crop, mirror,
// saturation / contrast / brightness jitter, drawn on the device from Philox4x32-10 and applied in the loader's one resize launch.
//     sgg_augment_plan     the per-example parameter table - three launches at most:
//       augment_plan_kernel      one thread per example: two Philox blocks -> box, flip, factors (integer arithmetic, one int64 -> fp32
//                                conversion per factor), the labels of a mirrored example remapped;
//       augment_grey_sum_kernel  (contrast on) the integer sum of 77 R + 150 G + 29 B over the crop box: AUG_SUM_CHUNKS workgroups per
//                                image, each a band of the box's rows; 64-bit sums through the wave, LDS, then ONE 64-bit integer atomic
//                                per workgroup - integer sums commute, so the bits do not depend on the arrival order;
//       augment_grey_mean_kernel (contrast on) sum / (256 ch cw) in fp64, rounded once to fp32.
//     sgg_augment_resize   a pure function of the source and the table: one thread per OUTPUT PIXEL (saturation needs the three
//                          channels), the legacy TF-1.x grid of resize_bilinear_tf1_kernel (csrc/misc.hip) laid over the crop box with
//                          the same rounding discipline, then the colour stages and (v - mean) / std.  HBM-bound: 12 source bytes
//                          gathered and 12 bytes stored per pixel, the stores of a wave contiguous.
#include "softmax_rows.h"

#define AUG_SUM_CHUNKS 32                        // workgroups per image of the grey sum (a 640x480 box: 15 rows each)
#define AUG_KEY1 0x41554731u                     // "AUG1": xor-ed into the key's high word (include/sgg_hip.h)

__device__ __forceinline__ int aug_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The crop interval on one axis of n pixels: length hmin + floor((n - hmin + 1) r_len / 2^24), start floor((n - len + 1) r_pos / 2^24).
__device__ __forceinline__ void aug_interval(int n, int lo_q, unsigned w_len, unsigned w_pos, int& start, int& len) {
  long long mn = ((long long)n * lo_q + 65535) >> 16;
  if (mn < 1) mn = 1;
  len = (int)(mn + ((((long long)n - mn + 1) * (long long)(w_len >> 8)) >> 24));
  start = (int)((((long long)n - len + 1) * (long long)(w_pos >> 8)) >> 24);
}

// 1 + a (2 u - 1) with u = ((w >> 9) + 0.5) 2^-23, as one integer: 2^39 + a_q (2 (w >> 9) + 1 - 2^23), converted once, scaled by 2^-39
__device__ __forceinline__ float aug_factor(int a_q, unsigned w) {
  if (a_q == 0) return 1.0f;
  const long long t = 2ll * (long long)(w >> 9) + 1ll - (1ll << 23);
  return (float)((1ll << 39) + (long long)a_q * t) * 0x1p-39f;
}

__global__ void augment_plan_kernel(const int* __restrict__ heights, const int* __restrict__ widths, const long long* __restrict__ labels_in,
                                    const int* __restrict__ swap, int V, int B, int crop_q, int flip_q, int bright_q, int contrast_q,
                                    int sat_q, unsigned k0, unsigned k1, unsigned long long draw0, int* __restrict__ box,
                                    float* __restrict__ factors, long long* __restrict__ labels_out, unsigned long long* __restrict__ sums) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const unsigned long long draw = draw0 + (unsigned long long)b;
  unsigned a[4], c[4];
  rows_philox(0u, 0u, (unsigned)draw, (unsigned)(draw >> 32), k0, k1, a);
  rows_philox(1u, 0u, (unsigned)draw, (unsigned)(draw >> 32), k0, k1, c);
  const int H = heights[b], W = widths[b];
  int y0, x0, ch, cw;
  aug_interval(H, crop_q, a[0], a[1], y0, ch);
  aug_interval(W, crop_q, a[2], a[3], x0, cw);
  int flip = (int)(c[0] >> 16) < flip_q;
  long long l[3], m[3];
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    l[i] = labels_in[(size_t)b * 3 + i];
    const int s = (l[i] >= 0 && l[i] < V) ? swap[l[i]] : -1;
    ok = ok && s >= 0 && s < V;
    m[i] = s;
  }
  flip = flip && ok;                                       // a word without a mirrored counterpart: the example is not mirrored
#pragma unroll
  for (int i = 0; i < 3; ++i) labels_out[(size_t)b * 3 + i] = flip ? m[i] : l[i];
  int* bx = box + (size_t)b * 6;
  bx[0] = y0; bx[1] = x0; bx[2] = ch; bx[3] = cw; bx[4] = flip; bx[5] = 0;
  float* f = factors + (size_t)b * 4;
  f[0] = aug_factor(bright_q, c[1]);
  f[1] = aug_factor(contrast_q, c[2]);
  f[2] = aug_factor(sat_q, c[3]);
  f[3] = 0.f;
  if (sums) sums[b] = 0ull;
}

__device__ __forceinline__ unsigned long long aug_wave_sum(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)v, o, 64), hi = __shfl_xor((unsigned)(v >> 32), o, 64);
    v += ((unsigned long long)hi << 32) | lo;
  }
  return v;
}

// grid (AUG_SUM_CHUNKS, B), 256 threads: workgroup (k, b) sums rows [ch k / CHUNKS, ch (k + 1) / CHUNKS) of example b's box.  The box
// is the plan kernel's (inside the image by construction); it is clamped all the same, as every reader of the table does.
__global__ void augment_grey_sum_kernel(const unsigned char* __restrict__ src, const long long* __restrict__ offsets,
                                        const int* __restrict__ heights, const int* __restrict__ widths, const int* __restrict__ box,
                                        unsigned long long* __restrict__ sums) {
  __shared__ unsigned long long red[4];
  const int b = blockIdx.y, k = blockIdx.x;
  const int H = heights[b], W = widths[b];
  if (H < 1 || W < 1) return;
  const int* bx = box + (size_t)b * 6;
  const int ch = aug_clampi(bx[2], 1, H), cw = aug_clampi(bx[3], 1, W);
  const int y0 = aug_clampi(bx[0], 0, H - ch), x0 = aug_clampi(bx[1], 0, W - cw);
  const int r0 = (int)(((long long)ch * k) / AUG_SUM_CHUNKS), r1 = (int)(((long long)ch * (k + 1)) / AUG_SUM_CHUNKS);
  const unsigned char* im = src + offsets[b];
  unsigned long long acc = 0ull;
  for (int r = r0 + (int)(threadIdx.x >> 6); r < r1; r += 4) {          // a wave per row, its lanes along the row: no division
    const unsigned char* row = im + ((size_t)(y0 + r) * W + x0) * 3;
    for (int x = threadIdx.x & 63; x < cw; x += 64) acc += 77u * row[3 * x] + 150u * row[3 * x + 1] + 29u * row[3 * x + 2];
  }
  acc = aug_wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long s = red[0] + red[1] + red[2] + red[3];
    if (s) atomicAdd(sums + b, s);
  }
}

__global__ void augment_grey_mean_kernel(const int* __restrict__ heights, const int* __restrict__ widths, const int* __restrict__ box,
                                         const unsigned long long* __restrict__ sums, float* __restrict__ factors, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int H = heights[b], W = widths[b];
  if (H < 1 || W < 1) return;
  const int ch = aug_clampi(box[(size_t)b * 6 + 2], 1, H), cw = aug_clampi(box[(size_t)b * 6 + 3], 1, W);
  const double mean = (double)(long long)sums[b] / (double)(256ll * ch * cw);
  factors[(size_t)b * 4 + 3] = (float)mean;
}

struct aug_rgb {
  float r, g, b;
};

// grid (ceil(oh ow / 256), B), 256 threads, one output pixel per thread.  SAT / CON / BRI: the stage mask (uniform branches).
__global__ void augment_resize_kernel(const unsigned char* __restrict__ src, const long long* __restrict__ offsets,
                                      const int* __restrict__ heights, const int* __restrict__ widths, const int* __restrict__ box,
                                      const float* __restrict__ factors, int stages, float* __restrict__ dst, int oh, int ow,
                                      const float* __restrict__ means, const float* __restrict__ stds) {
  // every product through an opaque register copy: the library is built with -ffp-contract=fast (resize_bilinear_tf1_kernel)
#define R(x) ({ float r__ = (x); asm volatile("" : "+v"(r__)); r__; })
  const int b = blockIdx.y;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= oh * ow) return;
  const int H = heights[b], W = widths[b];
  if (H < 1 || W < 1) return;
  // the table row, clamped into its image: a bad row is never followed out of the packed buffer
  const int* bx = box + (size_t)b * 6;
  const int ch = aug_clampi(bx[2], 1, H), cw = aug_clampi(bx[3], 1, W);
  const int by = aug_clampi(bx[0], 0, H - ch), bxx = aug_clampi(bx[1], 0, W - cw);
  const bool flip = bx[4] != 0;
  const unsigned char* im = src + offsets[b];
  const int y = p / ow, xo = p - y * ow;
  const int x = flip ? ow - 1 - xo : xo;
  const float sy = (float)ch / (float)oh, sx = (float)cw / (float)ow;
  const float fy = R((float)y * sy), fx = R((float)x * sx);
  // (floor(fy) <= ch - 1 for every output size the call accepts but the very largest, where fl((oh - 1) * fl(ch / oh)) can reach ch:
  //  the lower neighbour is clamped as well - nothing is ever read outside the box)
  const int y0 = min((int)floorf(fy), ch - 1), y1 = min(y0 + 1, ch - 1);
  const int x0 = min((int)floorf(fx), cw - 1), x1 = min(x0 + 1, cw - 1);
  const float wy = fy - (float)y0, wx = fx - (float)x0;
  const unsigned char* ptl = im + ((size_t)(by + y0) * W + (bxx + x0)) * 3;
  const unsigned char* ptr = im + ((size_t)(by + y0) * W + (bxx + x1)) * 3;
  const unsigned char* pbl = im + ((size_t)(by + y1) * W + (bxx + x0)) * 3;
  const unsigned char* pbr = im + ((size_t)(by + y1) * W + (bxx + x1)) * 3;
  float v[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float tl = (float)ptl[c], tr = (float)ptr[c], bl = (float)pbl[c], br = (float)pbr[c];
    const float dt = tr - tl, db = br - bl;
    const float pt = R(dt * wx), pb = R(db * wx);
    const float top = tl + pt, bot = bl + pb;
    const float dv = bot - top;
    const float pv = R(dv * wy);
    v[c] = top + pv;
  }
  if (stages) {
    const float* f = factors + (size_t)b * 4;
    if (stages & 1) {                                      // saturation, about the pixel's own grey value
      const float s = f[2], g = 0.299f * v[0] + 0.587f * v[1] + 0.114f * v[2];
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = g + s * (v[c] - g);
    }
    if (stages & 2) {                                      // contrast, about the box's grey mean
      const float k = f[1], m = f[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = m + k * (v[c] - m);
    }
    if (stages & 4) {                                      // brightness
      const float k = f[0];
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = k * v[c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = fminf(fmaxf(v[c], 0.f), 255.f);
  }
  aug_rgb o;
  o.r = (v[0] - means[0]) / stds[0];
  o.g = (v[1] - means[1]) / stds[1];
  o.b = (v[2] - means[2]) / stds[2];
  *reinterpret_cast<aug_rgb*>(dst + (((size_t)b * oh + y) * ow + xo) * 3) = o;
#undef R
}

extern "C" size_t sgg_augment_plan_workspace_bytes(int B) { return B > 0 ? (size_t)B * sizeof(unsigned long long) : 0; }

extern "C" int sgg_augment_plan(const unsigned char* src, const long long* offsets, const int* heights, const int* widths,
                                const long long* labels_in, const int* swap, int V, int B, int crop_q, int flip_q, int brightness_q,
                                int contrast_q, int saturation_q, unsigned long long seed, unsigned long long draw0, int* box,
                                float* factors, long long* labels_out, void* workspace, size_t workspace_bytes, void* stream) {
  SGG_CHECK_ARG(src && offsets && heights && widths && labels_in && swap && box && factors && labels_out && B > 0 && B <= 65535 &&
                V > 0, "sgg_augment_plan: bad argument");
  SGG_CHECK_ARG(crop_q >= 1 && crop_q <= 65536 && flip_q >= 0 && flip_q <= 65536, "sgg_augment_plan: crop must lie in (0, 1] and flip "
                "in [0, 1] as 16-bit fixed point (got %d, %d)", crop_q, flip_q);
  SGG_CHECK_ARG(brightness_q >= 0 && brightness_q < 65536 && contrast_q >= 0 && contrast_q < 65536 && saturation_q >= 0 &&
                saturation_q < 65536, "sgg_augment_plan: a jitter amplitude must lie in [0, 1) as 16-bit fixed point (got %d, %d, %d)",
                brightness_q, contrast_q, saturation_q);
  unsigned long long* sums = nullptr;
  if (contrast_q > 0) {
    SGG_CHECK_ARG(workspace && workspace_bytes >= sgg_augment_plan_workspace_bytes(B) && (((uintptr_t)workspace) & 7) == 0,
                  "sgg_augment_plan: contrast needs an 8-byte aligned workspace of sgg_augment_plan_workspace_bytes(B) bytes");
    sums = static_cast<unsigned long long*>(workspace);
  }
  const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32) ^ AUG_KEY1;
  hipLaunchKernelGGL(augment_plan_kernel, dim3(sgg_cdiv(B, 64)), dim3(64), 0, (hipStream_t)stream, heights, widths, labels_in, swap, V, B,
                     crop_q, flip_q, brightness_q, contrast_q, saturation_q, k0, k1, draw0, box, factors, labels_out, sums);
  if (sums) {
    hipLaunchKernelGGL(augment_grey_sum_kernel, dim3(AUG_SUM_CHUNKS, B), dim3(256), 0, (hipStream_t)stream, src, offsets, heights, widths,
                       box, sums);
    hipLaunchKernelGGL(augment_grey_mean_kernel, dim3(sgg_cdiv(B, 64)), dim3(64), 0, (hipStream_t)stream, heights, widths, box, sums,
                       factors, B);
  }
  SGG_LAUNCH_CHECK("sgg_augment_plan");
  return SGG_OK;
}

extern "C" int sgg_augment_resize(const unsigned char* src, const long long* offsets, const int* heights, const int* widths, const int* box,
                                  const float* factors, int stages, float* dst, int B, int out_h, int out_w, const float* means,
                                  const float* stds, void* stream) {
  SGG_CHECK_ARG(src && offsets && heights && widths && box && factors && dst && means && stds && B > 0 && out_h > 0 && out_w > 0 &&
                B <= 65535 && (long long)out_h * out_w <= (1ll << 30) && stages >= 0 && stages <= 7, "sgg_augment_resize: bad argument");
  hipLaunchKernelGGL(augment_resize_kernel, dim3(sgg_cdiv((long long)out_h * out_w, 256), B), dim3(256), 0, (hipStream_t)stream, src,
                     offsets, heights, widths, box, factors, stages, dst, out_h, out_w, means, stds);
  SGG_LAUNCH_CHECK("sgg_augment_resize");
  return SGG_OK;
}
