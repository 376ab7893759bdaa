// PIL-to-tensor preprocessing on the device (gfx950): Pillow's 8-bit bicubic resize, .convert("RGB") and the image processor's normalisation.
//
// Reference op replaced: FeatureExtractor.preprocess_image of feature/diffusion_feature.py:118-140 for one PIL image,
//   pipe.image_processor.preprocess(x.resize((S, S)).convert("RGB")),
// restated from the published algorithm of Pillow's ImagingResample (8 bits per channel, filter BICUBIC, whole-image box):
// per axis a table of fixed-point coefficients made in IEEE double WITHOUT fused multiply-add, a horizontal pass into a uint8 intermediate,
// a vertical pass over it, each pass acc = 2^21 + sum src * kk in int32 and one clamp(acc >> 22, 0, 255) per byte.  The result is compared
// with Pillow's for equality, so nothing here may round differently: the whole file is compiled with contraction off.
//
// Launches per image (no device -> host read anywhere; a pass whose axis already has the target size is skipped with its table):
//   pil_coeffs_kernel     (in, out) -> bounds int32 [out][2] = (xmin, xmax), kk int32 [out][ksize]           one lane per output sample
//   pil_horizontal_kernel uint8 [H][W][C] -> uint8 [H][OW][C]                                                 one lane per output byte
//   pil_final_kernel      uint8 [H][OW][C] -> uint8 [OH][OW][3] and / or fp32 [3][OH][OW] = (u / 255) * 2 - 1  one lane per (c, oy, ox): the vertical
//                         pass, or (RESAMPLE = false) the bytes as they are: the normalise-only form
// C = 1 (mode L) is replicated to the three output channels by the final kernel.
#include <cmath>

#include "kernels.h"

#pragma clang fp contract(off)

namespace gdf {

namespace {

enum { PIL_PRECISION_BITS = 32 - 8 - 2 };

__device__ __forceinline__ double pil_bicubic(double x) {
  x = fabs(x);
  if (x < 1.0) return ((1.5 * x - 2.5) * x) * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * -0.5;
  return 0.0;
}

__device__ __forceinline__ uint8_t pil_clip8(int acc) {
  const int v = acc >> PIL_PRECISION_BITS;                                  // arithmetic shift
  return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// (fp32(u) / 255.0f) * 2.0f - 1.0f with a correctly rounded division: the double quotient rounded to fp32 equals the fp32 quotient for
// every u in 0 .. 255 (tests/test_pil_resample_cpu.py checks all of them); 2 x is exact, the subtraction rounds once
__device__ __forceinline__ float pil_normalise(uint8_t u) {
  const float x = (float)((double)u / 255.0);
  return x * 2.0f - 1.0f;
}

}  // namespace

// The filter is evaluated twice per tap (once for the sum, once for the tap): the same operations on the same operands, hence the same doubles
// as the stored k[x] of the C code.
__global__ __launch_bounds__(64) void pil_coeffs_kernel(int in, int out, int ksize, int* __restrict__ bounds, int* __restrict__ kk) {
  const int xx = blockIdx.x * 64 + threadIdx.x;
  if (xx >= out) return;
  const double scale = (double)in / (double)out;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = 2.0 * fs;
  const double ss = 1.0 / fs;
  const double center = (xx + 0.5) * scale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > in) xmax = in;
  xmax -= xmin;
  if (xmax > ksize) xmax = ksize;                                            // (never: xmax <= 2 ceil(support) + 1; keeps the writes inside the row)
  double ww = 0.0;
  for (int x = 0; x < xmax; ++x) ww += pil_bicubic((x + xmin - center + 0.5) * ss);
  int* k = kk + (size_t)xx * ksize;
  for (int x = 0; x < xmax; ++x) {
    double w = pil_bicubic((x + xmin - center + 0.5) * ss);
    if (ww != 0.0) w /= ww;
    k[x] = w < 0 ? (int)(-0.5 + w * 4194304.0) : (int)(0.5 + w * 4194304.0);
  }
  for (int x = xmax; x < ksize; ++x) k[x] = 0;
  bounds[2 * xx] = xmin;
  bounds[2 * xx + 1] = xmax;
}

// lane i = (y * OW + ox) * C + c, the index of the byte it writes
__global__ __launch_bounds__(256) void pil_horizontal_kernel(const uint8_t* __restrict__ src, int H, int W, int C, int OW, int ksize,
                                                             const int* __restrict__ bounds, const int* __restrict__ kk,
                                                             uint8_t* __restrict__ mid) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;                         // (H OW C < 2^31: no wrap)
  if (i >= (unsigned)H * OW * C) return;
  const int c = i % C, ox = (i / C) % OW, y = i / ((unsigned)C * OW);
  const int xmin = bounds[2 * ox], xmax = bounds[2 * ox + 1];
  const int* k = kk + (size_t)ox * ksize;
  const uint8_t* s = src + ((size_t)y * W + xmin) * C + c;
  int acc = 1 << (PIL_PRECISION_BITS - 1);
  for (int x = 0; x < xmax; ++x) acc += (int)s[(size_t)x * C] * k[x];
  mid[i] = pil_clip8(acc);
}

// lane i = (c * OH + oy) * OW + ox over the C channels of `mid` ([H][OW][C]); with RESAMPLE = false H == OH and the byte passes through
template <bool RESAMPLE>
__global__ __launch_bounds__(256) void pil_final_kernel(const uint8_t* __restrict__ mid, int C, int OH, int OW, int ksize,
                                                        const int* __restrict__ bounds, const int* __restrict__ kk,
                                                        uint8_t* __restrict__ dst_u8, float* __restrict__ dst_f32) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;                         // (3 OH OW < 2^31: no wrap)
  if (i >= (unsigned)C * OH * OW) return;
  const int ox = i % OW, oy = (i / OW) % OH, c = i / ((unsigned)OW * OH);
  uint8_t u;
  if constexpr (RESAMPLE) {
    const int ymin = bounds[2 * oy], ymax = bounds[2 * oy + 1];
    const int* k = kk + (size_t)oy * ksize;
    const size_t row = (size_t)OW * C;
    const uint8_t* s = mid + (size_t)ymin * row + (size_t)ox * C + c;
    int acc = 1 << (PIL_PRECISION_BITS - 1);
    for (int y = 0; y < ymax; ++y) acc += (int)s[y * row] * k[y];
    u = pil_clip8(acc);
  } else {
    u = mid[((size_t)oy * OW + ox) * C + c];
  }
  const size_t p = (size_t)oy * OW + ox, plane = (size_t)OH * OW;
  if (C == 3) {
    if (dst_u8) dst_u8[p * 3 + c] = u;
    if (dst_f32) dst_f32[c * plane + p] = pil_normalise(u);
  } else {                                                                    // .convert("RGB") of an L image: the channel three times
    if (dst_u8) { dst_u8[p * 3] = u; dst_u8[p * 3 + 1] = u; dst_u8[p * 3 + 2] = u; }
    if (dst_f32) { const float v = pil_normalise(u); dst_f32[p] = v; dst_f32[plane + p] = v; dst_f32[2 * plane + p] = v; }
  }
}

int pil_ksize(int in, int out) {
  const double scale = (double)in / (double)out;
  const double fs = scale < 1.0 ? 1.0 : scale;
  return (int)std::ceil(2.0 * fs) * 2 + 1;
}

namespace {
size_t r16(size_t v) { return (v + 15) / 16 * 16; }
size_t table_bytes(int in, int out) { return in == out ? 0 : r16((size_t)out * 2 * 4) + r16((size_t)out * pil_ksize(in, out) * 4); }
}  // namespace

// workspace: [horizontal bounds | horizontal kk | vertical bounds | vertical kk | intermediate uint8 [src_h][out_w][C]], every part rounded up to 16
// bytes; a skipped pass has no table, and the intermediate exists only when the horizontal pass runs
size_t pil_resize_workspace_bytes(int src_h, int src_w, int channels, int out_h, int out_w) {
  const size_t mid = src_w != out_w ? r16((size_t)src_h * out_w * channels) : 0;
  return table_bytes(src_w, out_w) + table_bytes(src_h, out_h) + mid + 16;   // (+ 16: never zero, so that a caller's allocation has an address)
}

hipError_t launch_pil_coeffs(int in, int out, int* bounds, int* kk, hipStream_t s) {
  hipLaunchKernelGGL(pil_coeffs_kernel, dim3((unsigned)((out + 63) / 64)), dim3(64), 0, s, in, out, pil_ksize(in, out), bounds, kk);
  return hipGetLastError();
}

hipError_t launch_pil_resize_u8(const uint8_t* src, int src_h, int src_w, int C, int out_h, int out_w, uint8_t* dst_u8, float* dst_f32,
                                void* workspace, hipStream_t s) {
  uint8_t* ws = (uint8_t*)workspace;
  const bool horiz = src_w != out_w, vert = src_h != out_h;
  int *hb = nullptr, *hk = nullptr, *vb = nullptr, *vk = nullptr;
  int hks = 0, vks = 0;
  if (horiz) {
    hks = pil_ksize(src_w, out_w);
    hb = (int*)ws; ws += r16((size_t)out_w * 8);
    hk = (int*)ws; ws += r16((size_t)out_w * hks * 4);
    if (hipError_t e = launch_pil_coeffs(src_w, out_w, hb, hk, s)) return e;
  }
  if (vert) {
    vks = pil_ksize(src_h, out_h);
    vb = (int*)ws; ws += r16((size_t)out_h * 8);
    vk = (int*)ws; ws += r16((size_t)out_h * vks * 4);
    if (hipError_t e = launch_pil_coeffs(src_h, out_h, vb, vk, s)) return e;
  }
  const unsigned n_final = (unsigned)(((size_t)C * out_h * out_w + 255) / 256);
  const uint8_t* in = src;
  if (horiz) {
    uint8_t* mid = ws;
    hipLaunchKernelGGL(pil_horizontal_kernel, dim3((unsigned)(((size_t)src_h * out_w * C + 255) / 256)), dim3(256), 0, s, src, src_h, src_w, C,
                       out_w, hks, (const int*)hb, (const int*)hk, mid);
    if (hipError_t e = hipGetLastError()) return e;
    in = mid;
  }
  if (vert)
    hipLaunchKernelGGL(pil_final_kernel<true>, dim3(n_final), dim3(256), 0, s, in, C, out_h, out_w, vks, (const int*)vb, (const int*)vk, dst_u8, dst_f32);
  else
    hipLaunchKernelGGL(pil_final_kernel<false>, dim3(n_final), dim3(256), 0, s, in, C, out_h, out_w, 0, (const int*)nullptr, (const int*)nullptr,
                       dst_u8, dst_f32);
  return hipGetLastError();
}

}  // namespace gdf
