// ControlNet conditioning embedding (`controlnet_cond_embedding` of diffusers' ControlNetModel), gfx950.
//
// Reference op replaced: the chain  conv_in 3->16, SiLU; six 3x3 convs 16->16 s1, 16->32 s2, 32->32 s1, 32->96 s2, 96->96 s1, 96->256 s2, each + SiLU;
// conv_out 256->block_out_channels[0]  on the control image (B, 3, 8 H_lat, 8 W_lat) — the model the reference drives from
// feature/components/controlnet.py:95-130.
//
// The GEMM family's conv (gemm.hip, A_CONV3) wants Cin % 64 == 0 and its conv_in form Cin <= 8 at stride 1; these layers have Cin in
// {8 (the image packed to 8 channels), 16, 32, 96, 256} at strides 1 and 2 on images 64 x the pixel count of the latents.  So: one direct 3x3
// conv, NHWC fp16 in and out, straight from global memory into MFMA fragments (no LDS stage: a pixel's 8 consecutive channels are one 16-byte
// load, and the 3x3 halo re-reads hit the cache), fp32 accumulation, bias (+ SiLU) (+ the destination's old value) and ONE fp16 rounding at
// the store.
//
// Contraction index k = tap * Cin + c, padded with zero weights to a multiple of 32 (v_mfma_f32_16x16x32_f16: a lane holds 8 consecutive k).
// Cin % 8 == 0, so a lane's 8 k never straddle a tap.  Weights are packed at load time as [k / 8][Cout][8] (launch_cond_pack_weights): the
// 16 lanes of a fragment row group read 256 contiguous bytes.  The MFMA runs "transposed" — weights as the A operand (rows = output
// channels), pixels as B (columns) — so a lane ends up with 4 CONSECUTIVE output channels of one pixel: 8-byte stores.
//
// Work split: a wave owns 64 consecutive output pixels (4 column tiles) x NT * 16 output channels; 4 waves per workgroup; blockIdx.y walks the
// channel chunks (only the 256 -> C0 layer and 96 -> 256 have more than one).  HBM traffic per layer = input once + output once.
#include <algorithm>

#include "kernels.h"

namespace gdf {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int NT>
__global__ __launch_bounds__(256) void cond_conv3x3_kernel(CondConvParams p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int fr = lane & 15, g = lane >> 4;
  const unsigned p0 = (blockIdx.x * 4u + wave) * 64u;
  if (p0 >= p.M) return;
  const int n0 = blockIdx.y * (NT * 16);
  // the lane's pixel of each of the 4 column tiles: sample, top-left input coordinate of its 3x3 window
  int pb[4], iy0[4], ix0[4];
  bool pv[4];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    const unsigned pm = p0 + mt * 16 + fr;
    pv[mt] = pm < p.M;
    const unsigned q = pv[mt] ? pm : 0u;
    const unsigned b = q / (unsigned)(p.OH * p.OW), r = q - b * (unsigned)(p.OH * p.OW);
    const unsigned oy = r / (unsigned)p.OW, ox = r - oy * (unsigned)p.OW;
    pb[mt] = (int)b; iy0[mt] = (int)oy * p.stride - 1; ix0[mt] = (int)ox * p.stride - 1;
  }
  f32x4 acc[4][NT];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  int tap = (8 * g) / p.Cin, c = (8 * g) - tap * p.Cin;
  const half_t* wp = p.w + ((size_t)g * p.Cout + n0 + fr) * 8;
  for (int kk = 0; kk < p.Kpad; kk += 32) {
    f16x8 wf[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) wf[nt] = *(const f16x8*)(wp + (size_t)nt * 128);
    wp += (size_t)4 * p.Cout * 8;
    const int dy = tap / 3, dx = tap - 3 * dy;
    f16x8 xf[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      const int iy = iy0[mt] + dy, ix = ix0[mt] + dx;
      const bool ok = pv[mt] && tap < 9 && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
      xf[mt] = f16x8{0, 0, 0, 0, 0, 0, 0, 0};
      if (ok) xf[mt] = *(const f16x8*)(p.x + (((size_t)pb[mt] * p.H + iy) * p.W + ix) * p.ldx + c);
    }
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[nt], xf[mt], acc[mt][nt], 0, 0, 0);
    c += 32;
    while (c >= p.Cin) { c -= p.Cin; ++tap; }
  }
  // D[row = 4 g + r][col = fr]: output channels n0 + nt * 16 + 4 g + (0..3) of pixel p0 + mt * 16 + fr
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int co = n0 + nt * 16 + 4 * g;
    const f32x4 bv = p.bias ? *(const f32x4*)(p.bias + co) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      if (!pv[mt]) continue;
      half_t* op = p.out + (size_t)(p0 + mt * 16 + fr) * p.ldo + co;
      f32x4 v = acc[mt][nt] + bv;
      if (p.silu) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] / (1.0f + expf(-v[e]));      // (expf, not the fast form: the error budget beside the fp16 rounding is ~2^-22)
      }
      if (p.add) {
        const f16x4 old = *(const f16x4*)op;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] += (float)old[e];
      }
      f16x4 h;
#pragma unroll
      for (int e = 0; e < 4; ++e) h[e] = (_Float16)v[e];
      *(f16x4*)op = h;
    }
  }
}

// tiles of 16 output channels per wave: the whole width of the narrow layers, chunks of 64 from 256 channels up
static int cond_conv_nt(int Cout) { return Cout == 16 ? 1 : Cout == 32 ? 2 : Cout == 96 ? 6 : (Cout >= 64 && Cout % 64 == 0) ? 4 : 0; }

bool cond_conv_ok(int Cin, int Cout) {
  switch (Cin) {
    case 8: return Cout == 16;
    case 16: return Cout == 16 || Cout == 32;
    case 32: return Cout == 32 || Cout == 96;
    case 96: return Cout == 96 || Cout == 256;
    case 256: return Cout >= 64 && Cout % 64 == 0;         // conv_out: 256 -> block_out_channels[0]
    default: return false;
  }
}
int cond_conv_kpad(int Cin) { return (9 * Cin + 31) / 32 * 32; }
size_t cond_conv_weight_bytes(int Cin, int Cout) { return (size_t)cond_conv_kpad(Cin) * Cout * 2; }

hipError_t launch_cond_conv3x3(const CondConvParams& q, hipStream_t s) {
  CondConvParams p = q;
  if (!cond_conv_ok(p.Cin, p.Cout) || p.B < 1 || p.H < 1 || p.W < 1) return hipErrorInvalidValue;
  if (p.stride != 1 && p.stride != 2) return hipErrorInvalidValue;
  if (p.stride == 2 && ((p.H | p.W) & 1)) return hipErrorInvalidValue;
  if (p.ldx < p.Cin || p.ldo < p.Cout || (p.ldx & 7) || (p.ldo & 7)) return hipErrorInvalidValue;
  if (!p.x || !p.w || !p.out || (((uintptr_t)p.x | (uintptr_t)p.w | (uintptr_t)p.out | (uintptr_t)p.bias) & 15)) return hipErrorInvalidValue;
  p.OH = (p.H - 1) / p.stride + 1; p.OW = (p.W - 1) / p.stride + 1;
  const size_t M = (size_t)p.B * p.OH * p.OW;
  if (M >= (1ull << 31)) return hipErrorInvalidValue;
  p.M = (unsigned)M; p.Kpad = cond_conv_kpad(p.Cin);
  const int nt = cond_conv_nt(p.Cout);
  const dim3 grid((unsigned)((M + 255) / 256), (unsigned)(p.Cout / (nt * 16)));
  switch (nt) {
    case 1: hipLaunchKernelGGL(cond_conv3x3_kernel<1>, grid, dim3(256), 0, s, p); break;
    case 2: hipLaunchKernelGGL(cond_conv3x3_kernel<2>, grid, dim3(256), 0, s, p); break;
    case 4: hipLaunchKernelGGL(cond_conv3x3_kernel<4>, grid, dim3(256), 0, s, p); break;
    case 6: hipLaunchKernelGGL(cond_conv3x3_kernel<6>, grid, dim3(256), 0, s, p); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

__device__ __forceinline__ float cond_ld(const void* src, int dtype, size_t i) {
  if (dtype == 1) return ((const float*)src)[i];
  if (dtype == 2) return __uint_as_float((uint32_t)((const unsigned short*)src)[i] << 16);
  return (float)((const half_t*)src)[i];
}

// OIHW src[O][I][9] -> dst[k / 8][O][8] fp16, k = tap * cin_pad + c; channels from I up and k from 9 * cin_pad up are zero
__global__ void cond_pack_weights_kernel(const void* src, int dtype, half_t* dst, int O, int I, int cin_pad, long total) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int e = (int)(i & 7), o = (int)((i >> 3) % O);
    const int k = (int)((i >> 3) / O) * 8 + e, tap = k / cin_pad, c = k - tap * cin_pad;
    float v = 0.f;
    if (tap < 9 && c < I) v = cond_ld(src, dtype, ((size_t)o * I + c) * 9 + tap);
    dst[i] = (_Float16)v;
  }
}
hipError_t launch_cond_pack_weights(const void* src, int dtype, half_t* dst, int O, int I, int cin_pad, hipStream_t s) {
  if (O < 1 || I < 1 || I > cin_pad || (cin_pad & 7)) return hipErrorInvalidValue;
  const long total = (long)cond_conv_kpad(cin_pad) * O;
  hipLaunchKernelGGL(cond_pack_weights_kernel, dim3((unsigned)std::min<long>((total + 255) / 256, 8192)), dim3(256), 0, s, src, dtype, dst, O, I,
                     cin_pad, total);
  return hipGetLastError();
}

// control image NCHW (B, C <= 8, H, W), fp16 or fp32 (dtype 1) -> NHWC pixels of 8 fp16 channels, channels from C up zero
__global__ __launch_bounds__(256) void cond_pack_image_kernel(const void* x, int dtype, int C, long HW, long total, half_t* nhwc8) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long b = i / HW, pix = i - b * HW;
    f16x8 o = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int c = 0; c < C; ++c) o[c] = (_Float16)cond_ld(x, dtype, ((size_t)b * C + c) * HW + pix);
    *(f16x8*)(nhwc8 + (size_t)i * 8) = o;
  }
}
hipError_t launch_cond_pack_image(const void* x, int dtype, int B, int C, int H, int W, half_t* nhwc8, hipStream_t s) {
  if (C < 1 || C > 8 || (dtype != 0 && dtype != 1) || !x || !nhwc8 || ((uintptr_t)nhwc8 & 15)) return hipErrorInvalidValue;
  const long total = (long)B * H * W;
  if (total < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(cond_pack_image_kernel, dim3((unsigned)std::min<long>((total + 255) / 256, 8192)), dim3(256), 0, s, x, dtype, C, (long)H * W, total,
                     nhwc8);
  return hipGetLastError();
}

}  // namespace gdf
