// HBM-bound kernels of the MMDiT (Flux) path for gfx950.
//
// Reference ops replaced (paths under /root/reference/feature/diffusers/models; the normalisation / embedding classes
// are un-vendored diffusers==0.32.2, imported at transformers/transformer_flux.py:34-38 and attention_processor.py:141,2331):
//   AdaLayerNormZero / AdaLayerNormZeroSingle / AdaLayerNormContinuous `norm(x) * (1 + scale[:, None]) + shift[:, None]`
//   and the norm2 modulate of FluxTransformerBlock (transformer_flux.py:194-195, 214-215)      -> layernorm_mod_kernel
//   Attention.norm_q / norm_k / norm_added_q / norm_added_k (RMSNorm per head, attention_processor.py:2300-2303,
//   2321-2324) + apply_rotary_emb (attention_processor.py:2331-2335)                           -> qk_norm_rope_kernel
//   FluxPosEmbed (transformer_flux.py:498-499)                                                 -> rope_table_kernel
// All are streaming kernels: 16 bytes per lane, one pass over the data.
#include <algorithm>

#include "kernels.h"

namespace gdf {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// one wave per row, the row lives in registers (C <= 64 * 8 * MAXC), exact two-pass statistics
// ---- fp8 (OCP e4m3) row quantisation: q = fp8(v / s), s = the smallest power of two with |v| / s <= 448 (the e4m3 maximum) ----
__device__ __forceinline__ float fp8_row_scale(float amax) {
  if (!(amax > 0.f) || !(amax < 3.0e38f)) return 1.0f;
  int e; (void)frexpf(amax * (1.0f / 448.0f), &e);        // amax / 448 = m 2^e, m in [0.5, 1)  ->  2^e >= amax / 448
  return ldexpf(1.0f, e);
}
__device__ __forceinline__ uint2 pack_fp8x8(const float v[8], float inv) {
  int lo = 0, hi = 0;
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(v[0] * inv, v[1] * inv, lo, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(v[2] * inv, v[3] * inv, lo, true);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(v[4] * inv, v[5] * inv, hi, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(v[6] * inv, v[7] * inv, hi, true);
  return uint2{(unsigned)lo, (unsigned)hi};
}
// 16-bit rows [R][ld] (K columns used) -> fp8 [R][ldq] + scale[R]; one workgroup per row, two passes (the second read hits L2)
__global__ __launch_bounds__(256) void quant_rows_fp8_kernel(const half_t* x, int ld, int K, int bf, unsigned char* q, int ldq, float* scale) {
  const size_t row = blockIdx.x;
  const half_t* xr = x + row * (size_t)ld;
  __shared__ float red[4];
  float amax = 0.f;
  for (int c = threadIdx.x * 8; c < K; c += 256 * 8) {
    const f16x8 a = *(const f16x8*)(xr + c);
#pragma unroll
    for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(e16_to_f32(a[e], bf)));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) amax = fmaxf(amax, __shfl_xor(amax, off));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = amax;
  __syncthreads();
  amax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  const float sc = fp8_row_scale(amax), inv = 1.0f / sc;
  if (threadIdx.x == 0) scale[row] = sc;
  for (int c = threadIdx.x * 8; c < K; c += 256 * 8) {
    const f16x8 a = *(const f16x8*)(xr + c);
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = e16_to_f32(a[e], bf);
    *(uint2*)(q + row * (size_t)ldq + c) = pack_fp8x8(v, inv);
  }
}
hipError_t launch_quant_rows_fp8(const half_t* x, int ld, int R, int K, int bf16, unsigned char* q, int ldq, float* scale, hipStream_t s) {
  if (R <= 0) return hipSuccess;
  if ((K & 7) || (ld & 7) || (ldq & 7)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(quant_rows_fp8_kernel, dim3((unsigned)R), dim3(256), 0, s, x, ld, K, bf16, q, ldq, scale);
  return hipGetLastError();
}

template <int MAXC>
__global__ __launch_bounds__(256) void layernorm_mod_kernel(const half_t* x16, const float* x32, int ld, int R, int C,
                                                            float eps, const float* scale, const float* shift, int ldm,
                                                            int rps, int seg_rows, int rps2, half_t* y, int bf, int ldy, int y_lo,
                                                            unsigned char* q8, int ldq8, float* q8_scale) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  const int CH = C / 8;
  float v[MAXC][8];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    const int c = lane + 64 * i;
    if (c < CH) {
      if (x32) {
        const f32x4 a = *(const f32x4*)(x32 + (size_t)row * ld + c * 8), b = *(const f32x4*)(x32 + (size_t)row * ld + c * 8 + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { v[i][e] = a[e]; v[i][4 + e] = b[e]; }
      } else {
        const f16x8 a = *(const f16x8*)(x16 + (size_t)row * ld + c * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[i][e] = (float)a[e];
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) s += v[i][e];
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  const float mean = s / (float)C;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    const int c = lane + 64 * i;
    if (c < CH) {
#pragma unroll
      for (int e = 0; e < 8; ++e) { const float d = v[i][e] - mean; q += d * d; }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) q += __shfl_xor(q, off);
  const float rstd = rsqrtf(q / (float)C + eps);
  const int smp = (seg_rows > 0 && row >= seg_rows) ? (row - seg_rows) / rps2 : row / rps;
  const float* sc = scale + (size_t)smp * ldm;
  const float* sh = shift + (size_t)smp * ldm;
  float amax = 0.f;                                     // fp8 output ('fp8-mx' plans): |max| of the modulated row
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    const int c = lane + 64 * i;
    if (c < CH) {
      const f32x4 g0 = *(const f32x4*)(sc + c * 8), g1 = *(const f32x4*)(sc + c * 8 + 4);
      const f32x4 b0 = *(const f32x4*)(sh + c * 8), b1 = *(const f32x4*)(sh + c * 8 + 4);
      f16x8 o;
      float t[8];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        t[e] = (v[i][e] - mean) * rstd * (1.0f + g0[e]) + b0[e];
        t[4 + e] = (v[i][4 + e] - mean) * rstd * (1.0f + g1[e]) + b1[e];
      }
      if (q8) {
#pragma unroll
        for (int e = 0; e < 8; ++e) { v[i][e] = t[e]; amax = fmaxf(amax, fabsf(t[e])); }   // keep the modulated values for the fp8 pass
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = f32_to_e16(t[e], bf);
      *(f16x8*)(y + (size_t)row * ldy + c * 8) = o;
      if (y_lo > 0) {                                    // split operand of the consumer GEMM ('bfloat16x2' plans): lo = e16(v - hi)
        f16x8 l;
#pragma unroll
        for (int e = 0; e < 8; ++e) l[e] = f32_to_e16(t[e] - e16_to_f32(o[e], bf), bf);
        *(f16x8*)(y + (size_t)row * ldy + c * 8 + y_lo) = l;
      }
    }
  }
  if (q8) {                                              // the same row as fp8 (e4m3) with one power-of-two scale (operand of an 'fp8-mx' GEMM)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) amax = fmaxf(amax, __shfl_xor(amax, off));
    const float sc8 = fp8_row_scale(amax), inv = 1.0f / sc8;
    if (lane == 0) q8_scale[row] = sc8;
#pragma unroll
    for (int i = 0; i < MAXC; ++i) {
      const int c = lane + 64 * i;
      if (c < CH) *(uint2*)(q8 + (size_t)row * ldq8 + c * 8) = pack_fp8x8(v[i], inv);
    }
  }
}

// registers chunks (8 columns per lane each) of the instantiation that holds a row of C columns; 0: no instantiation (C % 8, C > 4096)
int layernorm_mod_maxc(int C) {
  if (C <= 0 || C % 8 || C > 64 * 8 * 8) return 0;
  const int CH = C / 8;
  return CH <= 64 ? 1 : CH <= 128 ? 2 : CH <= 256 ? 4 : CH <= 384 ? 6 : 8;
}

hipError_t launch_layernorm_mod(const half_t* x16, const float* x32, int ld, int R, int C, float eps, const float* scale,
                                const float* shift, int ldm, int rps, int seg_rows, int rps2, half_t* y, hipStream_t s,
                                int bf16, int ldy, int y_lo, unsigned char* q8, int ldq8, float* q8_scale) {
  const int maxc = layernorm_mod_maxc(C);
  if (!maxc || (ldm & 3) || rps <= 0 || (y_lo & 7) || (ldy & 7) || (q8 && ((ldq8 & 7) || !q8_scale))) return hipErrorInvalidValue;
  if (!x16 == !x32 || (x32 ? (ld & 3) : (ld & 7))) return hipErrorInvalidValue;   // one source; its rows stay aligned for the 16-byte loads
  if (ldy <= 0) ldy = C;
  if (R <= 0) return hipSuccess;
  dim3 grid((R + 3) / 4), blk(256);
#define GDF_LNM(N) hipLaunchKernelGGL(layernorm_mod_kernel<N>, grid, blk, 0, s, x16, x32, ld, R, C, eps, scale, shift, ldm, rps, seg_rows, rps2, y, bf16, ldy, y_lo, q8, ldq8, q8_scale)
  switch (maxc) {
    case 1: GDF_LNM(1); break;
    case 2: GDF_LNM(2); break;
    case 4: GDF_LNM(4); break;
    case 6: GDF_LNM(6); break;
    default: GDF_LNM(8); break;
  }
#undef GDF_LNM
  return hipGetLastError();
}

// 16 lanes per (row, head): 8 halves (= 4 rotary pairs) per lane, D = 128.  q then k of the same (row, head).
// BF (bf16 container) is a COMPILE-TIME parameter of the body (round 6): with the runtime flag every input element went through
// `bf ? shift : cvt` — sixteen v_cndmask on a lane mask the wave held in VCC from its first instruction to its last — and with a second
// HSA queue active on the device (another host thread's stream) single elements of 16-lane groups came out as if the mask had been wrong
// for one instruction (tools/micro/op_race.py: this kernel beside a 128-row ring GEMM, 150-270 of 600 launches; 0 of 1000 without the
// per-element select; not a cvt -> select forwarding hazard: wait states between them change nothing).  The cause is below this library
// (wave state across queue switches is the suspect); the kernel no longer keeps anything in a mask register across its body.
template <bool BF>
__device__ __forceinline__ void qk_norm_rope_body(half_t* x, int ld, long R, int heads, int q_col, int k_col, const float* wq, const float* wk, float eps,
                                                  const float* cos_t, const float* sin_t, int pos0, int rps) {
  constexpr int D = 128;
  const long g = (long)blockIdx.x * 16 + (threadIdx.x >> 4);     // (row, head) pair
  if (g >= R * heads) return;
  const int sub = threadIdx.x & 15;
  const long row = g / heads;
  const int head = (int)(g - row * heads);
  const int pos = pos0 + (int)(row % rps);
  const f32x4 c0 = *(const f32x4*)(cos_t + (size_t)pos * D + sub * 8), c1 = *(const f32x4*)(cos_t + (size_t)pos * D + sub * 8 + 4);
  const f32x4 s0 = *(const f32x4*)(sin_t + (size_t)pos * D + sub * 8), s1 = *(const f32x4*)(sin_t + (size_t)pos * D + sub * 8 + 4);
  float cs[8], sn[8];
#pragma unroll
  for (int e = 0; e < 4; ++e) { cs[e] = c0[e]; cs[4 + e] = c1[e]; sn[e] = s0[e]; sn[4 + e] = s1[e]; }
#pragma unroll
  for (int which = 0; which < 2; ++which) {
    half_t* px = x + (size_t)row * ld + (which ? k_col : q_col) + head * D + sub * 8;
    const float* w = (which ? wk : wq) + sub * 8;
    const f16x8 hv = *(const f16x8*)px;
    float v[8];
    float ss = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) { v[e] = e16_to_f32(hv[e], BF ? 1 : 0); ss += v[e] * v[e]; }
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) ss += __shfl_xor(ss, off);   // the 16 lanes of this (row, head)
    const float r = rsqrtf(ss / (float)D + eps);
    const f32x4 w0 = *(const f32x4*)w, w1 = *(const f32x4*)(w + 4);
#if defined(GDF_EXP_ROPE_FULLWAIT)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // EXPERIMENT: every load of this iteration (x, cos, sin, gains) has landed before the math
#endif
#pragma unroll
    for (int e = 0; e < 4; ++e) { v[e] *= r * w0[e]; v[4 + e] *= r * w1[e]; }
    f16x8 o;
#pragma unroll
    for (int e = 0; e < 8; e += 2) {       // x * cos + stack([-x_imag, x_real]) * sin
      o[e] = f32_to_e16(v[e] * cs[e] - v[e + 1] * sn[e], BF ? 1 : 0);
      o[e + 1] = f32_to_e16(v[e + 1] * cs[e + 1] + v[e] * sn[e + 1], BF ? 1 : 0);
    }
    *(f16x8*)px = o;
  }
}
template <bool BF>
__global__ __launch_bounds__(256) void qk_norm_rope_kernel(half_t* x, int ld, long R, int heads, int q_col, int k_col,
                                                           const float* wq, const float* wk, float eps,
                                                           const float* cos_t, const float* sin_t, int pos0, int rps) {
  qk_norm_rope_body<BF>(x, ld, R, heads, q_col, k_col, wq, wk, eps, cos_t, sin_t, pos0, rps);
}

hipError_t launch_qk_norm_rope(half_t* x, int ld, int R, int heads, int D, int q_col, int k_col, const float* wq,
                               const float* wk, float eps, const float* cos_t, const float* sin_t, int pos0, int rps,
                               hipStream_t s, int bf16) {
  if (D != 128 || (ld & 7) || (q_col & 7) || (k_col & 7) || rps <= 0) return hipErrorInvalidValue;
  if (R <= 0) return hipSuccess;
  const long groups = (long)R * heads;
  if (bf16)
    hipLaunchKernelGGL(qk_norm_rope_kernel<true>, dim3((unsigned)((groups + 15) / 16)), dim3(256), 0, s, x, ld, (long)R, heads, q_col,
                       k_col, wq, wk, eps, cos_t, sin_t, pos0, rps);
  else
    hipLaunchKernelGGL(qk_norm_rope_kernel<false>, dim3((unsigned)((groups + 15) / 16)), dim3(256), 0, s, x, ld, (long)R, heads, q_col,
                       k_col, wq, wk, eps, cos_t, sin_t, pos0, rps);
  return hipGetLastError();
}

struct RopeAxes { int n; int dim[4]; int off[4]; int D; };

__global__ void rope_table_kernel(const float* ids, int S, RopeAxes ax, double theta, float* cos_t, float* sin_t, int row0) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int half = ax.D / 2;
  if (i >= S * half) return;
  const int r = i / half, pj = i - r * half;        // row, rotary pair index inside the row
  int a = 0;
  while (a + 1 < ax.n && 2 * pj >= ax.off[a + 1]) ++a;
  const int k = (2 * pj - ax.off[a]) / 2;           // pair index inside axis a
  const double freq = 1.0 / pow(theta, (double)(2 * k) / (double)ax.dim[a]);
  const double ang = (double)ids[(size_t)r * ax.n + a] * freq;
  const float c = (float)cos(ang), sn = (float)sin(ang);
  const size_t o = (size_t)(row0 + r) * ax.D + 2 * pj;
  cos_t[o] = c; cos_t[o + 1] = c;
  sin_t[o] = sn; sin_t[o + 1] = sn;
}

hipError_t launch_rope_table(const float* ids, int S, int n_axes, const int* axes_dim, double theta, float* cos_t,
                             float* sin_t, int row0, hipStream_t s) {
  if (n_axes < 1 || n_axes > 4) return hipErrorInvalidValue;
  RopeAxes ax{};
  ax.n = n_axes;
  int off = 0;
  for (int i = 0; i < n_axes; ++i) {
    if (axes_dim[i] % 2) return hipErrorInvalidValue;
    ax.dim[i] = axes_dim[i]; ax.off[i] = off; off += axes_dim[i];
  }
  ax.D = off;
  if (S <= 0) return hipSuccess;
  const int total = S * (off / 2);
  hipLaunchKernelGGL(rope_table_kernel, dim3((total + 255) / 256), dim3(256), 0, s, ids, S, ax, theta, cos_t, sin_t, row0);
  return hipGetLastError();
}

// one workgroup per row; the row is held in registers as packed halves (n <= 256 * 8 * 8 = 16384 per pass, looped beyond)
__global__ __launch_bounds__(256) void softmax_rows_kernel(half_t* x, int ld, int n, float scale) {
  __shared__ float red[8];
  half_t* row = x + (size_t)blockIdx.x * ld;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float sl2 = scale * 1.44269504088896340736f;
  constexpr int MAXV = 8;                                // f16x8 vectors per thread kept in registers
  f16x8 v[MAXV];
  const int nvec = n / 8;                                // host guarantees n % 8 == 0 and n <= 256 * 8 * MAXV
  float mx = -INFINITY;
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int c = tid + i * 256;
    if (c < nvec) {
      v[i] = *(const f16x8*)(row + c * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) mx = fmaxf(mx, (float)v[i][e]);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
  if (lane == 0) red[wave] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])) * sl2;
  float sum = 0.f;
  float ev[MAXV][8];
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int c = tid + i * 256;
    if (c < nvec) {
#pragma unroll
      for (int e = 0; e < 8; ++e) { ev[i][e] = __builtin_amdgcn_exp2f((float)v[i][e] * sl2 - mx); sum += ev[i][e]; }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
  if (lane == 0) red[4 + wave] = sum;
  __syncthreads();
  const float inv = 1.0f / (red[4] + red[5] + red[6] + red[7]);
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int c = tid + i * 256;
    if (c < nvec) {
      f16x8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = (_Float16)(ev[i][e] * inv);
      *(f16x8*)(row + c * 8) = o;
    }
  }
}

hipError_t launch_softmax_rows(half_t* x, int ld, int R, int n, float scale, hipStream_t s) {
  if ((n & 7) || (ld & 7) || n > 256 * 8 * 8) return hipErrorInvalidValue;
  if (R <= 0) return hipSuccess;
  hipLaunchKernelGGL(softmax_rows_kernel, dim3(R), dim3(256), 0, s, x, ld, n, scale);
  return hipGetLastError();
}

// quant_conv of one pixel's 2L moments (1x1: wq fp16 [2L][2L], bq fp32 or NULL = 0; wq == NULL: identity): m[0..L) = mean, m[L..2L) = logvar
__device__ __forceinline__ void vae_moments(const float* h, size_t pixel, int L2, const half_t* wq, const float* bq, float* m) {
  float hv[32];
  for (int c = 0; c < L2; ++c) hv[c] = h[pixel * L2 + c];
  for (int o = 0; o < L2; ++o) {
    if (wq) {
      float a = bq ? bq[o] : 0.f;
      for (int c = 0; c < L2; ++c) a += (float)wq[o * L2 + c] * hv[c];
      m[o] = a;
    } else {
      m[o] = hv[o];
    }
  }
}

// One latent element of the VAE tail — the ONE place its arithmetic is written: vae_finish_kernel and vae_finish_multi_kernel both call it, so
// the same operands give the same bits in either (tests/test_gpu_vae_multi.py compares them bit for bit)
// (vae_finish_f32 is that value before its one rounding, on operands already in registers: the packed tail reads eps / noise as pairs and
// rounds to bf16 as well)
__device__ __forceinline__ float vae_finish_f32(float mean, float logvar, bool has_eps, float eps, bool has_noise, float noise, float scaling,
                                                 float na, float nb, float in_scale) {
  float z = mean;
  if (has_eps) z += expf(0.5f * fminf(fmaxf(logvar, -30.0f), 20.0f)) * eps;
  float lat = scaling * z;
  if (has_noise) lat = na * lat + nb * noise;
  return in_scale * lat;
}
__device__ __forceinline__ _Float16 vae_finish_value(float mean, float logvar, const half_t* eps, const half_t* noise, size_t oi,
                                                      float scaling, float na, float nb, float in_scale) {
  return (_Float16)vae_finish_f32(mean, logvar, eps != nullptr, eps ? (float)eps[oi] : 0.f, noise != nullptr, noise ? (float)noise[oi] : 0.f,
                                  scaling, na, nb, in_scale);
}

__global__ void vae_finish_kernel(const float* h, int HW, int L, const half_t* wq, const float* bq, const half_t* eps,
                                  const half_t* noise, float scaling, float na, float nb, float in_scale, half_t* out, long total) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;      // (b, pixel)
  if (i >= total) return;
  const long b = i / HW;
  const int pix = (int)(i - b * HW);
  float m[16];
  vae_moments(h, (size_t)i, 2 * L, wq, bq, m);
  for (int c = 0; c < L; ++c) {
    const size_t oi = ((size_t)b * L + c) * HW + pix;
    out[oi] = vae_finish_value(m[c], m[L + c], eps, noise, oi, scaling, na, nb, in_scale);
  }
}

hipError_t launch_vae_finish(const float* h, int B, int HW, int L, const half_t* wq, const float* bq, const half_t* eps,
                             const half_t* noise, float scaling, float noise_a, float noise_b, float in_scale, half_t* out,
                             hipStream_t s) {
  if (L < 1 || L > 8) return hipErrorInvalidValue;
  const long total = (long)B * HW;
  if (total <= 0) return hipSuccess;
  hipLaunchKernelGGL(vae_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, h, HW, L, wq, bq, eps, noise,
                     scaling, noise_a, noise_b, in_scale, out, total);
  return hipGetLastError();
}

// The tail for K timesteps of the same B images: the moments are read and quant_conv applied ONCE per (image, pixel); row r = k * B + b of
// eps / noise / out (timestep-major) gets timestep k's scalars.  The K triples are kernel ARGUMENTS (uniform loads from the kernarg segment
// indexed by k): no device table, so no host -> device copy in front of the launch.  t_stride = elements between two timesteps' row blocks.
static_assert(GDF_MAX_TIMESTEPS == 8, "VaeTimesteps holds 8 triples");
__global__ void vae_finish_multi_kernel(const float* h, int HW, int L, const half_t* wq, const float* bq, const half_t* eps,
                                        const half_t* noise, float scaling, int K, VaeTimesteps ts, half_t* out, long total,
                                        long t_stride) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;      // (b, pixel): consecutive lanes = consecutive pixels
  if (i >= total) return;
  const long b = i / HW;
  const int pix = (int)(i - b * HW);
  float m[16];
  vae_moments(h, (size_t)i, 2 * L, wq, bq, m);
  for (int k = 0; k < K; ++k) {
    const float na = ts.noise_a[k], nb = ts.noise_b[k], is = ts.in_scale[k];
    for (int c = 0; c < L; ++c) {
      const size_t oi = (size_t)k * (size_t)t_stride + ((size_t)b * L + c) * HW + pix;
      out[oi] = vae_finish_value(m[c], m[L + c], eps, noise, oi, scaling, na, nb, is);
    }
  }
}

hipError_t launch_vae_finish_multi(const float* h, int B, int HW, int L, const half_t* wq, const float* bq, const half_t* eps,
                                   const half_t* noise, float scaling, int K, const float* noise_a, const float* noise_b,
                                   const float* in_scale, half_t* out, long t_stride, hipStream_t s) {
  if (L < 1 || L > 8 || K < 1 || K > GDF_MAX_TIMESTEPS || !noise_a || !noise_b || !in_scale) return hipErrorInvalidValue;
  const long total = (long)B * HW;
  if (total <= 0) return hipSuccess;
  if (t_stride < total * L) return hipErrorInvalidValue;           // the K row blocks must not overlap
  VaeTimesteps ts{};
  for (int k = 0; k < K; ++k) { ts.noise_a[k] = noise_a[k]; ts.noise_b[k] = noise_b[k]; ts.in_scale[k] = in_scale[k]; }
  hipLaunchKernelGGL(vae_finish_multi_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, h, HW, L, wq, bq, eps, noise,
                     scaling, K, ts, out, total, t_stride);
  return hipGetLastError();
}

// The tail of the Flux latent preparation (FluxImg2ImgPipeline.prepare_latents: retrieve_latents(vae.encode(image)), (z - shift_factor) *
// scaling_factor, scheduler.scale_noise, _pack_latents) in one pass over the moments:
//     out[b][gy * (w/2) + gx][c * 4 + dy * 2 + dx] = na * scaling * ((mean - shift) + std * eps) + nb * noise     at latent (b, c, 2gy + dy, 2gx + dx)
// i.e. vae_finish_value's arithmetic (vae_finish_f32) on (mean - shift) with in_scale = 1, written as the (B, (h/2)(w/2), 4L) token rows the MMDiT reads, fp16 or bf16 (BF).
// One lane per token, consecutive lanes = consecutive tokens of a row: a lane reads its four pixels' moment rows (2L fp32 each, 16-byte loads),
// per channel and dy ONE 4-byte eps / noise pair (the two dx; contiguous across the wave), builds the token's 4L values in registers and writes
// them with 16-byte stores.  LT = L at compile time (4, 16: everything stays in registers) or 0 (any L <= 16); QC: quant_conv through
// vae_moments (LT = 0 only).  vec = 0: the operands are not aligned for the wide accesses (or L is odd): element-wise loads and stores.
template <bool BF, int LT, bool QC>
__global__ __launch_bounds__(256) void vae_finish_packed_kernel(const float* h, int hh, int ww, int L, const half_t* wq, const float* bq,
                                                                const half_t* eps, const half_t* noise, float scaling, float shift, float na,
                                                                float nb, unsigned short* out, long total, int vec) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;      // (b, gy, gx)
  if (i >= total) return;
  const int Lr = LT ? LT : L, L2 = 2 * Lr;
  constexpr int UF = LT ? 64 : 1;                                  // channel loops: unrolled completely for a compile-time L, left alone otherwise
  const int gw = ww >> 1, gh = hh >> 1;
  const long r = i / gw;
  const int gx = (int)(i - r * gw);
  const long b = r / gh;
  const int gy = (int)(r - b * gh);
  const size_t HW = (size_t)hh * ww;
  unsigned short tok[64];
#pragma unroll
  for (int dy = 0; dy < 2; ++dy) {
    const size_t pix = (size_t)(2 * gy + dy) * ww + 2 * gx;         // dx = 0; dx = 1 is the next pixel
    float m[2][32];
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
      const size_t p = (size_t)b * HW + pix + dx;
      if (QC) {
        vae_moments(h, p, L2, wq, bq, m[dx]);
      } else if (vec) {
        const float4* hp = (const float4*)(h + p * L2);
#pragma unroll UF
        for (int j = 0; j < L2 / 4; ++j) { const float4 v = hp[j]; m[dx][4 * j] = v.x; m[dx][4 * j + 1] = v.y; m[dx][4 * j + 2] = v.z; m[dx][4 * j + 3] = v.w; }
      } else {
#pragma unroll UF
        for (int c = 0; c < L2; ++c) m[dx][c] = h[p * L2 + c];
      }
    }
#pragma unroll UF
    for (int c = 0; c < Lr; ++c) {
      const size_t e = ((size_t)b * Lr + c) * HW + pix;
      float ev[2] = {0.f, 0.f}, nv[2] = {0.f, 0.f};
      if (vec) {
        if (eps) { const uint32_t u = *(const uint32_t*)(eps + e); ev[0] = (float)__builtin_bit_cast(half_t, (unsigned short)(u & 0xffffu)); ev[1] = (float)__builtin_bit_cast(half_t, (unsigned short)(u >> 16)); }
        if (noise) { const uint32_t u = *(const uint32_t*)(noise + e); nv[0] = (float)__builtin_bit_cast(half_t, (unsigned short)(u & 0xffffu)); nv[1] = (float)__builtin_bit_cast(half_t, (unsigned short)(u >> 16)); }
      } else {
        if (eps) { ev[0] = (float)eps[e]; ev[1] = (float)eps[e + 1]; }
        if (noise) { nv[0] = (float)noise[e]; nv[1] = (float)noise[e + 1]; }
      }
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        const float v = vae_finish_f32(m[dx][c] - shift, m[dx][Lr + c], eps != nullptr, ev[dx], noise != nullptr, nv[dx], scaling, na, nb, 1.0f);
        tok[c * 4 + dy * 2 + dx] = BF ? __builtin_bit_cast(unsigned short, (__bf16)v) : __builtin_bit_cast(unsigned short, (_Float16)v);
      }
    }
  }
  unsigned short* row = out + (size_t)i * 4 * Lr;
  if (vec) {
#pragma unroll UF
    for (int j = 0; j < Lr / 2; ++j) {
      uint4 q;
      q.x = (uint32_t)tok[8 * j] | ((uint32_t)tok[8 * j + 1] << 16);
      q.y = (uint32_t)tok[8 * j + 2] | ((uint32_t)tok[8 * j + 3] << 16);
      q.z = (uint32_t)tok[8 * j + 4] | ((uint32_t)tok[8 * j + 5] << 16);
      q.w = (uint32_t)tok[8 * j + 6] | ((uint32_t)tok[8 * j + 7] << 16);
      *(uint4*)(row + 8 * j) = q;
    }
  } else {
    for (int k = 0; k < 4 * Lr; ++k) row[k] = tok[k];
  }
}

hipError_t launch_vae_finish_packed(const float* h, int B, int H, int W, int L, const half_t* wq, const float* bq, const half_t* eps,
                                    const half_t* noise, float scaling, float shift, float noise_a, float noise_b, int out_bf16, void* out,
                                    hipStream_t s) {
  if (L < 1 || L > 16 || H < 2 || W < 2 || (H & 1) || (W & 1) || !out || !h) return hipErrorInvalidValue;   // refused before anything is written
  const long total = (long)B * (H / 2) * (W / 2);
  if (total <= 0) return hipSuccess;
  const auto al = [](const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; };
  // L even: a moment row is a multiple of 16 bytes and so is a token row; H * W is even, so every eps / noise pair starts on 4 bytes
  const int vec = (L % 2 == 0) && al(h, 16) && al(out, 16) && al(eps, 4) && al(noise, 4);
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  unsigned short* o = (unsigned short*)out;
#define GDF_VFP(BF, LT, QC) hipLaunchKernelGGL((vae_finish_packed_kernel<BF, LT, QC>), grid, block, 0, s, h, H, W, L, wq, bq, eps, noise, \
                                               scaling, shift, noise_a, noise_b, o, total, vec)
  if (wq) { if (out_bf16) GDF_VFP(true, 0, true); else GDF_VFP(false, 0, true); }
  else if (L == 16) { if (out_bf16) GDF_VFP(true, 16, false); else GDF_VFP(false, 16, false); }
  else if (L == 4) { if (out_bf16) GDF_VFP(true, 4, false); else GDF_VFP(false, 4, false); }
  else { if (out_bf16) GDF_VFP(true, 0, false); else GDF_VFP(false, 0, false); }
#undef GDF_VFP
  return hipGetLastError();
}

__global__ void sincos_pos_embed_kernel(float* out, int C, int gh, int gw, float sh, float sw) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int S = gh * gw;
  if (i >= S * C) return;
  const int tok = i / C, c = i - tok * C;
  // diffusers: grid = np.meshgrid(grid_w, grid_h) reshaped [2,1,gw,gh] and flattened; grid[0] (x coordinates) feeds the
  // first half of the channels.  Flat index m of the (gw, gh)-shaped view == m of the (gh, gw) meshgrid array.
  const int y = tok / gw, x = tok - y * gw;
  const int half = C / 2, quarter = C / 4;
  const int cc = c < half ? c : c - half;
  const double pos = c < half ? (double)((float)x * sw) : (double)((float)y * sh);
  const int k = cc < quarter ? cc : cc - quarter;
  const double omega = 1.0 / pow(10000.0, (double)k / (double)quarter);
  const double a = pos * omega;
  out[i] = (float)(cc < quarter ? sin(a) : cos(a));
}

hipError_t launch_sincos_pos_embed(float* out, int C, int gh, int gw, int base_size, float interpolation_scale, hipStream_t s) {
  if (C % 4) return hipErrorInvalidValue;
  // grid_h = arange(gh) / (gh / base_size) / interpolation_scale (float32 arithmetic in numpy)
  const float sh = 1.0f / ((float)gh / (float)base_size) / interpolation_scale;
  const float sw = 1.0f / ((float)gw / (float)base_size) / interpolation_scale;
  const int total = gh * gw * C;
  hipLaunchKernelGGL(sincos_pos_embed_kernel, dim3((total + 255) / 256), dim3(256), 0, s, out, C, gh, gw, sh, sw);
  return hipGetLastError();
}

__global__ void add_table_kernel(const float* table, const float* vec, int ldvec, int period, long n, float* out, long ldo) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int b = blockIdx.y;
  out[(size_t)b * ldo + i] = table[i] + vec[(size_t)b * ldvec + (int)(i % period)];
}

hipError_t launch_add_table(const float* table, const float* vec, int ldvec, int period, int B, long n, float* out, long ldo,
                            hipStream_t s) {
  if (n <= 0 || B <= 0) return hipSuccess;
  hipLaunchKernelGGL(add_table_kernel, dim3((unsigned)((n + 255) / 256), B), dim3(256), 0, s, table, vec, ldvec, period, n, out, ldo);
  return hipGetLastError();
}

__global__ void patchify_kernel(const half_t* x, int Cin, int H, int W, int p, int kpad, half_t* out, long total) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;      // (row, col)
  if (i >= total) return;
  const long row = i / kpad;
  const int col = (int)(i - row * kpad);
  const int gh = H / p, gw = W / p;
  const long b = row / (gh * gw);
  const int t = (int)(row - b * gh * gw), ty = t / gw, tx = t - ty * gw;
  _Float16 v = (_Float16)0.f;
  if (col < Cin * p * p) {
    const int c = col / (p * p), r = col - c * p * p, py = r / p, px = r - py * p;
    v = x[(((size_t)b * Cin + c) * H + (ty * p + py)) * W + tx * p + px];
  }
  out[i] = v;
}

hipError_t launch_patchify(const half_t* x, int B, int Cin, int H, int W, int p, int kpad, half_t* out, hipStream_t s) {
  if (p < 1 || H % p || W % p || Cin * p * p > kpad) return hipErrorInvalidValue;
  const long total = (long)B * (H / p) * (W / p) * kpad;
  hipLaunchKernelGGL(patchify_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, x, Cin, H, W, p, kpad, out, total);
  return hipGetLastError();
}

__global__ void unpatchify_kernel(const half_t* x, int Cout, int gh, int gw, int p, half_t* out, long total) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;      // output element (b, c, y, x)
  if (i >= total) return;
  const int W = gw * p, H = gh * p;
  const int xx = (int)(i % W);
  const int yy = (int)((i / W) % H);
  const int c = (int)((i / ((long)W * H)) % Cout);
  const long b = i / ((long)W * H * Cout);
  const int ty = yy / p, py = yy - ty * p, tx = xx / p, px = xx - tx * p;
  out[i] = x[((size_t)b * gh * gw + (size_t)ty * gw + tx) * (p * p * Cout) + (py * p + px) * Cout + c];
}

hipError_t launch_unpatchify(const half_t* x, int B, int Cout, int gh, int gw, int p, half_t* out, hipStream_t s) {
  const long total = (long)B * Cout * gh * p * gw * p;
  if (total <= 0) return hipSuccess;
  hipLaunchKernelGGL(unpatchify_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, x, Cout, gh, gw, p, out, total);
  return hipGetLastError();
}

__global__ void relayout_rows_padk_kernel(const void* src, int f32, half_t* dst, int ksrc, int kdst, long total) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const long r = i / kdst;
  const int k = (int)(i - r * kdst);
  float v = 0.f;
  if (k < ksrc) v = f32 ? ((const float*)src)[r * ksrc + k] : (float)((const half_t*)src)[r * ksrc + k];
  dst[i] = (_Float16)v;
}

hipError_t launch_relayout_rows_padk(const void* src, int src_f32, half_t* dst, int R, int ksrc, int kdst, hipStream_t s) {
  const long total = (long)R * kdst;
  if (total <= 0) return hipSuccess;
  hipLaunchKernelGGL(relayout_rows_padk_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, src, src_f32, dst, ksrc,
                     kdst, total);
  return hipGetLastError();
}

__global__ void silu_vec_kernel(const float* x, float* out, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const float v = x[i];
    const float d = 1.0f + expf(-v);
    // v < -88.7: expf(-v) overflows and v / inf would flush a normal number (silu(-90) = -7.4e-38) to -0; v * e^v is the same quotient there
    out[i] = d < __builtin_inff() ? v / d : v * expf(v);
  }
}

hipError_t launch_silu_vec(const float* x, float* out, long n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(silu_vec_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, out, n);
  return hipGetLastError();
}

// ---- multi-step latent trajectory (gdf_trajectory, include/gdf.h): the scheduler update between two denoiser forwards ----
// Replaces the latent update of the reference's inversion loop (components/ddim_inversion.py:39-41) and, in general, any scheduler step of the
// form x' = c_sample x + c_eps eps followed by scale_model_input.  It lives in this file because this file is compiled without SLP vectorisation
// (no packed-fp32 forms: DESIGN.md 3.5) and the kernel runs between forwards while other queues may run GEMMs.
//   x     fp32 master latents (B, 4, H, W) NCHW, updated in place
//   eps   fp16 noise_pred (B, H, W, 4) channels-last, as the plan's conv_out writes it; read only
//   y     fp16 (B, 4, H, W): the next forward's input  c_in[next] * x'
//   tbuf  fp32 (B): the next forward's timestep
//   steps int32 {step, ticket, n_rows, 0} followed by float rows[n_rows][4] = {timestep, c_in, c_sample, c_eps}
// Launch k reads row `step` for the update and row min(step + 1, n_rows - 1) for c_in and the timestep, then step becomes step + 1: every step
// of a trajectory is the SAME launch with the SAME arguments, so one hipGraph serves them all.  `step` is advanced by the workgroup that
// finishes last (ticket counter), i.e. after every workgroup has read it.  prime = 1: no update (eps is not read, x is not written), row 0
// supplies c_in and the timestep and step becomes 0 — the launch in front of the first forward.  step outside [0, n_rows): nothing is written.
__global__ __launch_bounds__(256) void latent_step_kernel(float* x, const half_t* eps, half_t* y, float* tbuf, int* steps, int B, int HW,
                                                          int hw8, int prime) {
  const int k = steps[0], n = steps[2];
  if (n < 1) return;
  const bool live = prime || (k >= 0 && k < n);
  if (live) {
    const float* rows = (const float*)(steps + 4);
    const int nx = prime ? 0 : (k + 1 < n ? k + 1 : n - 1);
    const float cs = prime ? 1.f : rows[4 * k + 2], ce = prime ? 0.f : rows[4 * k + 3];
    const float tn = rows[4 * nx], cin = rows[4 * nx + 1];
    const long stride = (long)gridDim.x * blockDim.x, t0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    // 8 pixels of one sample per item: per channel two 16-byte loads / stores of x and one 16-byte store of y; eps: four 16-byte loads
    for (long i = t0; i < (long)B * hw8; i += stride) {
      const long b = i / hw8;
      const int p0 = (int)(i - b * hw8) * 8;
      f16x8 ev[4];
      if (!prime) {
        const f16x8* ep = (const f16x8*)(eps + ((size_t)b * HW + p0) * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) ev[j] = ep[j];
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float* xp = x + ((size_t)b * 4 + c) * HW + p0;
        f32x4 xa = *(const f32x4*)xp, xb = *(const f32x4*)(xp + 4);
        f16x8 yo;
#pragma unroll
        for (int p = 0; p < 8; ++p) {
          float v = p < 4 ? xa[p] : xb[p - 4];
          if (!prime) v = __fmaf_rn(cs, v, ce * (float)ev[p >> 1][(p & 1) * 4 + c]);
          if (p < 4) xa[p] = v; else xb[p - 4] = v;
          yo[p] = (_Float16)(cin * v);
        }
        if (!prime) { *(f32x4*)xp = xa; *(f32x4*)(xp + 4) = xb; }
        *(f16x8*)(y + ((size_t)b * 4 + c) * HW + p0) = yo;
      }
    }
    // scalar tail: the pixels of every sample past its last whole group (all of them when a plane is no multiple of 16 bytes)
    const int tail = HW - hw8 * 8;
    for (long i = t0; i < (long)B * tail; i += stride) {
      const long b = i / tail;
      const int p = hw8 * 8 + (int)(i - b * tail);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const size_t o = ((size_t)b * 4 + c) * HW + p;
        float v = x[o];
        if (!prime) { v = __fmaf_rn(cs, v, ce * (float)eps[((size_t)b * HW + p) * 4 + c]); x[o] = v; }
        y[o] = (_Float16)(cin * v);
      }
    }
    if (blockIdx.x == 0) for (int b = threadIdx.x; b < B; b += blockDim.x) tbuf[b] = tn;
  }
  __syncthreads();                               // every wave of this workgroup has read `step`
  if (threadIdx.x == 0) {
    const unsigned t = atomicAdd((unsigned*)&steps[1], 1u);
    if (t == gridDim.x - 1) { steps[1] = 0; if (live) steps[0] = prime ? 0 : k + 1; }
  }
}

hipError_t launch_latent_step(float* x, const half_t* eps, half_t* y, float* tbuf, int* steps, int B, int H, int W, int prime, hipStream_t s) {
  const long HW = (long)H * W;
  if (B < 1 || H < 1 || W < 1 || (size_t)B * HW * 4 >= (1ull << 31)) return hipErrorInvalidValue;
  if (!x || !y || !tbuf || !steps || (!prime && !eps)) return hipErrorInvalidValue;
  const bool al = (((uintptr_t)x | (uintptr_t)y | (uintptr_t)eps) & 15) == 0;
  const int hw8 = (al && HW % 8 == 0) ? (int)(HW / 8) : 0;
  const long items = (long)B * (hw8 ? hw8 : HW);
  const unsigned grid = (unsigned)std::min<long>((items + 255) / 256, 256);
  hipLaunchKernelGGL(latent_step_kernel, dim3(grid), dim3(256), 0, s, x, eps, y, tbuf, steps, B, (int)HW, hw8, prime);
  return hipGetLastError();
}

// ---- guided sampling (gdf_sample, include/gdf.h): classifier-free guidance + a scheduler step with history between two forwards ----
// Replaces, per UNet call of a text-to-image loop, `noise_pred_uncond + g (noise_pred_text - noise_pred_uncond)`, `scheduler.step` of any
// scheduler whose update is linear in the sample and the last five model outputs (DDIM, Euler, PLMS, LMS, DPM-Solver multistep:
// components/models.py sampling_table) and `scheduler.scale_model_input` + `torch.cat([latents] * 2)` for the next call.  Same file as
// latent_step_kernel for the same reason (no packed fp32), same ticket scheme: every step is the same launch with the same arguments.
//   x     fp32 master latents (B, 4, H, W) NCHW, updated in place
//   eps   fp16 noise_pred, channels-last as conv_out writes it, read only: guided (2B, H, W, 4), rows [0, B) unconditional and [B, 2B)
//         conditional (torch.cat([negative, positive])); unguided (B, H, W, 4)
//   hist  fp32 ring of the last five combined eps, (5, B, 4, H, W); slot k mod 5 is written by step k.  Five, not four: PNDM's warm-up
//         call at the repeated timestep is not kept in its history, so its first four-term step reaches back five calls
//   y     fp16 next forward input c_in[next] * x': guided (2B, 4, H, W), the same values in both halves; unguided (B, 4, H, W)
//   tbuf  fp32 next timestep, 2B or B entries
//   steps int32 {step, ticket, n_rows, guided}, float g, three unused words, then float rows[n_rows][8] =
//         {timestep, c_in, c_sample, w0, w1, w2, w3, w4}
// Step k:  e = e_u + g (e_c - e_u)  (unguided: e = eps);  hist[k mod 5] = e;  x' = c_sample x + sum_j w_j hist[(k - j) mod 5], all fp32; a term
// with w_j == 0 is skipped, so a ring slot that no step has written is never read.  prime = 1: no update (eps and hist untouched, x not
// written), row 0 supplies c_in and the timestep, step becomes 0.  step outside [0, n_rows): nothing is written.
__global__ __launch_bounds__(256) void guided_step_kernel(float* x, const half_t* eps, float* hist, half_t* y, float* tbuf, int* steps,
                                                          int B, int HW, int hw8, int prime) {
  const int k = steps[0], n = steps[2];
  if (n < 1) return;
  const bool guided = steps[3] != 0;
  const bool live = prime || (k >= 0 && k < n);
  if (live) {
    const float g = ((const float*)steps)[4];
    const float* rows = (const float*)(steps + 8);
    const int kr = prime ? 0 : k;
    const int nx = prime ? 0 : (k + 1 < n ? k + 1 : n - 1);
    const float cs = rows[8 * kr + 2];
    const float w0 = rows[8 * kr + 3], w1 = rows[8 * kr + 4], w2 = rows[8 * kr + 5], w3 = rows[8 * kr + 6], w4 = rows[8 * kr + 7];
    const float tn = rows[8 * nx], cin = rows[8 * nx + 1];
    const size_t slot = (size_t)B * 4 * HW;                       // elements of one ring slot = of the master
    const int s0 = kr % 5;                                        // (kr >= 0 here: live and not prime, or 0)
    float* hk = hist + (size_t)s0 * slot;
    const float* h1 = hist + (size_t)((s0 + 4) % 5) * slot;
    const float* h2 = hist + (size_t)((s0 + 3) % 5) * slot;
    const float* h3 = hist + (size_t)((s0 + 2) % 5) * slot;
    const float* h4 = hist + (size_t)((s0 + 1) % 5) * slot;
    const half_t* epc = eps + (guided ? (size_t)B * HW * 4 : 0);  // the conditional half
    half_t* y2 = y + slot;                                        // the second half of the guided input
    const long stride = (long)gridDim.x * blockDim.x, t0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    // 8 pixels of one sample per item.  eps: four 16-byte loads per half; per channel two 16-byte loads / stores of x, two stores of the
    // ring slot, two loads per history term in use and one 16-byte store of y per half
    for (long i = t0; i < (long)B * hw8; i += stride) {
      const long b = i / hw8;
      const int p0 = (int)(i - b * hw8) * 8;
      f16x8 eu[4], ec[4];
      if (!prime) {
        const f16x8* up = (const f16x8*)(eps + ((size_t)b * HW + p0) * 4);
        const f16x8* cp = (const f16x8*)(epc + ((size_t)b * HW + p0) * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) { eu[j] = up[j]; if (guided) ec[j] = cp[j]; }
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const size_t o = ((size_t)b * 4 + c) * HW + p0;
        f32x4 xa = *(const f32x4*)(x + o), xb = *(const f32x4*)(x + o + 4);
        if (!prime) {
          f32x4 ea, eb;
#pragma unroll
          for (int p = 0; p < 8; ++p) {
            const float u = (float)eu[p >> 1][(p & 1) * 4 + c];
            const float e = guided ? __fmaf_rn(g, (float)ec[p >> 1][(p & 1) * 4 + c] - u, u) : u;
            if (p < 4) ea[p] = e; else eb[p - 4] = e;
          }
          *(f32x4*)(hk + o) = ea; *(f32x4*)(hk + o + 4) = eb;
#pragma unroll
          for (int p = 0; p < 4; ++p) { xa[p] = cs * xa[p]; xb[p] = cs * xb[p]; }
          if (w0 != 0.f) {
#pragma unroll
            for (int p = 0; p < 4; ++p) { xa[p] = __fmaf_rn(w0, ea[p], xa[p]); xb[p] = __fmaf_rn(w0, eb[p], xb[p]); }
          }
          const float wj[4] = {w1, w2, w3, w4};
          const float* hj[4] = {h1, h2, h3, h4};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (wj[j] != 0.f) {
              const f32x4 ha = *(const f32x4*)(hj[j] + o), hb = *(const f32x4*)(hj[j] + o + 4);
#pragma unroll
              for (int p = 0; p < 4; ++p) { xa[p] = __fmaf_rn(wj[j], ha[p], xa[p]); xb[p] = __fmaf_rn(wj[j], hb[p], xb[p]); }
            }
          }
          *(f32x4*)(x + o) = xa; *(f32x4*)(x + o + 4) = xb;
        }
        f16x8 yo;
#pragma unroll
        for (int p = 0; p < 8; ++p) yo[p] = (_Float16)(cin * (p < 4 ? xa[p] : xb[p - 4]));
        *(f16x8*)(y + o) = yo;
        if (guided) *(f16x8*)(y2 + o) = yo;
      }
    }
    // scalar tail: the pixels of every sample past its last whole group (all of them when a plane is no multiple of 16 bytes)
    const int tail = HW - hw8 * 8;
    for (long i = t0; i < (long)B * tail; i += stride) {
      const long b = i / tail;
      const int p = hw8 * 8 + (int)(i - b * tail);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const size_t o = ((size_t)b * 4 + c) * HW + p;
        float v = x[o];
        if (!prime) {
          const size_t oe = ((size_t)b * HW + p) * 4 + c;
          const float u = (float)eps[oe];
          const float e = guided ? __fmaf_rn(g, (float)epc[oe] - u, u) : u;
          hk[o] = e;
          v = cs * v;
          if (w0 != 0.f) v = __fmaf_rn(w0, e, v);
          if (w1 != 0.f) v = __fmaf_rn(w1, h1[o], v);
          if (w2 != 0.f) v = __fmaf_rn(w2, h2[o], v);
          if (w3 != 0.f) v = __fmaf_rn(w3, h3[o], v);
          if (w4 != 0.f) v = __fmaf_rn(w4, h4[o], v);
          x[o] = v;
        }
        const half_t yv = (_Float16)(cin * v);
        y[o] = yv;
        if (guided) y2[o] = yv;
      }
    }
    const int nt = guided ? 2 * B : B;
    if (blockIdx.x == 0) for (int b = threadIdx.x; b < nt; b += blockDim.x) tbuf[b] = tn;
  }
  __syncthreads();                               // every wave of this workgroup has read `step`
  if (threadIdx.x == 0) {
    const unsigned t = atomicAdd((unsigned*)&steps[1], 1u);
    if (t == gridDim.x - 1) { steps[1] = 0; if (live) steps[0] = prime ? 0 : k + 1; }
  }
}

// B: samples of the master (the plans of a guided run have batch 2B).  The guided flag lives in the steps block on the device, so the size
// check covers the larger (guided) case.
hipError_t launch_guided_step(float* x, const half_t* eps, float* hist, half_t* y, float* tbuf, int* steps, int B, int H, int W, int prime,
                              hipStream_t s) {
  const long HW = (long)H * W;
  if (B < 1 || H < 1 || W < 1 || (size_t)B * HW * 4 * 5 >= (1ull << 31)) return hipErrorInvalidValue;
  if (!x || !hist || !y || !tbuf || !steps || (!prime && !eps)) return hipErrorInvalidValue;
  // (the halves of a guided eps / y are B * HW * 4 elements apart: with HW % 8 == 0 they share the base's 16-byte alignment)
  const bool al = (((uintptr_t)x | (uintptr_t)y | (uintptr_t)eps | (uintptr_t)hist) & 15) == 0;
  const int hw8 = (al && HW % 8 == 0) ? (int)(HW / 8) : 0;
  const long items = (long)B * (hw8 ? hw8 : HW);
  const unsigned grid = (unsigned)std::min<long>((items + 255) / 256, 256);
  hipLaunchKernelGGL(guided_step_kernel, dim3(grid), dim3(256), 0, s, x, eps, hist, y, tbuf, steps, B, (int)HW, hw8, prime);
  return hipGetLastError();
}

}  // namespace gdf
