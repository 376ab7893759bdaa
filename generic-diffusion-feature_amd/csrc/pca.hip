// PCA of feature maps on the device and the PCA picture the reference draws of a hooked layer or of the cross-attention maps, gfx950.
//
// Reference op replaced (paths in the reference project):
//   feature_visualization.py:84-101   plot_pca: sklearn PCA(n_components=3).fit(f).transform(f) on the (H W, C) samples of one map, per-component
//   (p - min) / (max - min), (. * 255).astype(uint8), a nearest resize of the short side to 512
//
// One call = G PCAs: one per image (G = B), or one over the B H W pixels of the batch (joint, G = 1).  Stages:
//   pca_mean_kernel      one workgroup = 32 channels of one PCA: the channel means (per-thread compensated fp32 sums of 8-pixel groups, a fixed
//                        tree), then max |x - mean| of each channel
//   pca_scale_kernel     the power of two that brings the largest centred magnitude into [2^13, 2^14): the fp16 low halves stay clear of the
//                        fp16 subnormals; the covariance is descaled by the exact inverse
//   pca_cov_kernel       one workgroup = one 128 x 128 tile of the upper triangle x one range of the samples: (x - mean) * scale split into an fp16
//                        (hi, lo) pair as it is staged, channel-major images in LDS, v_mfma_f32_32x32x16_f16 with fp32 accumulation, the products
//                        lo lo + lo hi + hi lo + hi hi.  Channels past C are staged as zeros.
//   pca_cov_reduce_kernel   the ranges' partial tiles added in range order, divided by n - 1, written with their mirror image (a diagonal tile
//                        from its upper half only: the matrix is exactly symmetric)
//   pca_init_kernel      the fixed starting block of min(8, C) hashed vectors, the flags
//   pca_matvec_kernel    Z = cov Q, one wave per row, 16-byte loads
//   pca_ritz_kernel      one workgroup per PCA: H = Q^T Z (8 x 8), cyclic Jacobi on 64 lanes, the Ritz pairs, the residuals ||cov v - lambda v||, the
//                        converged flag and, i / 2 + 2 iterations after it, the flag that stops the launches; then the next block: Z W
//                        orthonormalised by two passes of classical Gram-Schmidt
//   pca_finalize_kernel  the eigenvalues as Rayleigh quotients of the final vectors in double, the sign rule, components, variance, total variance
//   pca_project_kernel   (x - mean) . v_j in fp32 FMAs from the same source strides
//   pca_rgb_kernel       per-component min / max, (p - min) / (max - min) * 255 truncated, Pillow's nearest resize
// No atomics, no grid-wide wait: the iterations are ordinary launches, all enqueued; once a PCA's flag is set its later launches return at
// their first instruction.  Every reduction has a fixed order and a workgroup sees one PCA only, so the bits do not depend on the stream, on B or
// on the place in the batch.
#include <math.h>

#include <algorithm>

#include "feat_common.h"

namespace gdf {

namespace {

enum { PCA_T = 128, PCA_TP = 32, PCA_PS = 40, PCA_M = 8, PCA_LD = 65 };

// vec: 16-byte loads along C are legal (sc == 1, C a multiple of the vector, every pixel 16-byte aligned)
struct PcaSrc { const void* ptr; long sb, sc, sy, sx; int C, H, W, vec; };

// A tile of TC channels from c0 x TP samples from p0 of the PCA whose first image is b0 (sample p = image p / (H W), pixel p % (H W)), handed to
// put(channel in tile, sample in tile, value, inside): outside C or at pe and beyond the value is 0.  NT threads; TP divides NT, so a thread of the
// lanes-along-pixels path keeps its pixel.
template <typename T, int TC, int TP, int NT, typename F>
__device__ __forceinline__ void pca_tile(const PcaSrc& s, int b0, int c0, long p0, long pe, F put) {
  const T* f = (const T*)s.ptr;
  const int HW = s.H * s.W;
  if (s.vec) {
    constexpr int V = 16 / (int)sizeof(T), VP = TC / V;
    typedef T vt __attribute__((ext_vector_type(V)));
    for (int it = threadIdx.x; it < TP * VP; it += NT) {
      const int px = it / VP, cv = (it % VP) * V;
      const long p = p0 + px;
      const bool in = p < pe && c0 + cv < s.C;
      vt v;
#pragma unroll
      for (int e = 0; e < V; ++e) v[e] = (T)0.f;
      if (in) {
        const int b = b0 + (int)(p / HW), q = (int)(p % HW);
        v = *(const vt*)(f + (long)b * s.sb + (long)(q / s.W) * s.sy + (long)(q % s.W) * s.sx + c0 + cv);
      }
#pragma unroll
      for (int e = 0; e < V; ++e) put(cv + e, px, (float)v[e], in);
    }
  } else {
    const int px = threadIdx.x % TP;
    const long p = p0 + px;
    const bool pin = p < pe;
    long o = 0;
    if (pin) {
      const int b = b0 + (int)(p / HW), q = (int)(p % HW);
      o = (long)b * s.sb + (long)(q / s.W) * s.sy + (long)(q % s.W) * s.sx;
    }
    for (int cl = threadIdx.x / TP; cl < TC; cl += NT / TP) {
      const bool in = pin && c0 + cl < s.C;
      put(cl, px, in ? (float)f[o + (long)(c0 + cl) * s.sc] : 0.f, in);
    }
  }
}

// One workgroup = 32 channels of PCA g.  Thread t: channel t / 8 of the tile, pixels t % 8 + 8 i of every 64-pixel tile: their plain sum is added
// to a compensated (Kahan) fp32 sum; the eight threads of a channel are folded by a butterfly.  Then max |x - mean| the same way.
template <typename T>
__global__ __launch_bounds__(256) void pca_mean_kernel(PcaSrc s, int joint, long n, float* mean, float* chmax) {
  __shared__ float tile[32 * PCA_LD];
  const int g = blockIdx.y, c0 = blockIdx.x * 32, b0 = joint ? 0 : g;
  const int cl = threadIdx.x >> 3, sub = threadIdx.x & 7;
  float sum = 0.f, comp = 0.f;
  for (long p0 = 0; p0 < n; p0 += 64) {
    pca_tile<T, 32, 64, 256>(s, b0, c0, p0, n, [&](int c, int p, float v, bool) { tile[c * PCA_LD + p] = v; });
    __syncthreads();
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) t += tile[cl * PCA_LD + sub + 8 * i];
    const float y = t - comp, u = sum + y;
    comp = (u - sum) - y;
    sum = u;
    __syncthreads();
  }
#pragma unroll
  for (int off = 4; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
  const float mu = sum / (float)n;
  float mx = 0.f;
  for (long p0 = 0; p0 < n; p0 += 64) {
    pca_tile<T, 32, 64, 256>(s, b0, c0, p0, n, [&](int c, int p, float v, bool in) { tile[c * PCA_LD + p] = in ? v : NAN; });
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; ++i) mx = fmaxf(mx, fabsf(tile[cl * PCA_LD + sub + 8 * i] - mu));   // (fmaxf drops the NaN of a sample outside)
    __syncthreads();
  }
#pragma unroll
  for (int off = 4; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
  if (sub == 0 && c0 + cl < s.C) {
    mean[(long)g * s.C + c0 + cl] = mu;
    chmax[(long)g * s.C + c0 + cl] = mx;
  }
}

// scale[g] = 2^e with max |x - mean| * 2^e in [2^13, 2^14); 1 where that maximum is zero or not finite
__global__ __launch_bounds__(256) void pca_scale_kernel(const float* chmax, int C, float* scale) {
  __shared__ float red[256];
  const int g = blockIdx.x;
  float m = 0.f;
  for (int c = threadIdx.x; c < C; c += 256) m = fmaxf(m, chmax[(long)g * C + c]);
  red[threadIdx.x] = m;
  __syncthreads();
#pragma unroll
  for (int half = 128; half >= 1; half >>= 1) {
    if ((int)threadIdx.x < half) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + half]);
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    m = red[0];
    int e = 0;                                          // split_shift's rule, clamped (written out: through the helper the branch became a select)
    if (m > 0.f && m < INFINITY) e = min(40, max(-40, 13 - ilogbf(m)));
    scale[g] = ldexpf(1.f, e);
  }
}

// tile number t of the upper triangle of an nt x nt grid, row by row -> (ti, tj), ti <= tj
__device__ __forceinline__ void pca_tile_ij(int t, int nt, int& ti, int& tj) {
  ti = 0;
  while (t >= nt - ti) { t -= nt - ti; ++ti; }
  tj = ti + t;
}

// One workgroup (four waves) = tile (ti, tj) x sample range blockIdx.y of PCA g.  Per step of 32 samples the two 128-channel panels are staged as
// fp16 (hi, lo) images [channel][sample] (a diagonal tile stages one); wave w owns the 64 x 64 quarter (w & 1, w >> 1) as 2 x 2 MFMA tiles.  Lane
// (r = lane % 32, h = lane / 32) reads samples 8 h .. 8 h + 7 of channel r of a 32-channel block as the A operand (rows) and as the B operand
// (columns): the sum over the samples is the same whatever their order inside a step.  part: (G, S, tiles, 128, 128).
template <typename T>
__global__ __launch_bounds__(256) void pca_cov_kernel(PcaSrc s, int joint, long n, long per, const float* mean, const float* scale, float* part,
                                                      int nt) {
  __shared__ __attribute__((aligned(16))) _Float16 img[2][2][PCA_T * PCA_PS];
  __shared__ float mu[2][PCA_T];
  const int t = blockIdx.x, sp = blockIdx.y, g = blockIdx.z, b0 = joint ? 0 : g;
  int ti, tj;
  pca_tile_ij(t, nt, ti, tj);
  const bool diag = ti == tj;
  for (int i = threadIdx.x; i < 2 * PCA_T; i += 256) {
    const int c = (i < PCA_T ? ti : tj) * PCA_T + (i % PCA_T);
    mu[i / PCA_T][i % PCA_T] = c < s.C ? mean[(long)g * s.C + c] : 0.f;
  }
  const float sc = scale[g];
  __syncthreads();
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 31, h = lane >> 5, wi = w & 1, wj = w >> 1;
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
  const _Float16* A = img[0][0];
  const _Float16* Bm = diag ? img[0][0] : img[1][0];
  constexpr int LO = PCA_T * PCA_PS;                 // elements from a panel's hi image to its lo image
  const long pe = min(n, ((long)sp + 1) * per);
  for (long p0 = (long)sp * per; p0 < pe; p0 += PCA_TP) {
    for (int pn = 0; pn < (diag ? 1 : 2); ++pn) {
      _Float16* im = img[pn][0];
      const float* m = mu[pn];
      pca_tile<T, PCA_T, PCA_TP, 256>(s, b0, (pn ? tj : ti) * PCA_T, p0, pe, [&](int c, int p, float v, bool in) {
        const float d = in ? (v - m[c]) * sc : 0.f;
        const _Float16 hi = f32_to_f16_sat(d);
        im[c * PCA_PS + p] = hi;
        im[LO + c * PCA_PS + p] = f32_to_f16_sat(d - (float)hi);
      });
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < PCA_TP / 16; ++kk) {
      f16x8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int oa = (64 * wi + 32 * i + r) * PCA_PS + 16 * kk + 8 * h, ob = (64 * wj + 32 * i + r) * PCA_PS + 16 * kk + 8 * h;
        ah[i] = *(const f16x8*)(A + oa);
        al[i] = *(const f16x8*)(A + LO + oa);
        bh[i] = *(const f16x8*)(Bm + ob);
        bl[i] = *(const f16x8*)(Bm + LO + ob);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[i], bl[j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[i], bh[j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bl[j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bh[j], acc[i][j], 0, 0, 0);
        }
    }
    __syncthreads();
  }
  // accumulator register e of lane (r, h): row 8 (e / 4) + 4 h + e % 4, column r of its 32 x 32 tile
  float* out = part + (((long)g * gridDim.y + sp) * gridDim.x + t) * (PCA_T * PCA_T);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e)
        out[(64 * wi + 32 * i + 8 * (e >> 2) + 4 * h + (e & 3)) * PCA_T + 64 * wj + 32 * j + r] = acc[i][j][e];
}

// cov (G, Cpad, Cpad) = the S partial tiles in range order / scale^2 / (n - 1), each element written with its mirror image
__global__ __launch_bounds__(256) void pca_cov_reduce_kernel(const float* part, int S, int ntiles, int nt, const float* scale, long n, float* cov) {
  const int g = blockIdx.y, t = blockIdx.x / 64, e = (blockIdx.x % 64) * 256 + threadIdx.x;
  const int i = e / PCA_T, j = e % PCA_T;
  int ti, tj;
  pca_tile_ij(t, nt, ti, tj);
  if (ti == tj && i > j) return;
  float v = 0.f;
  for (int sp = 0; sp < S; ++sp) v += part[(((long)g * S + sp) * ntiles + t) * (PCA_T * PCA_T) + e];
  const float is = 1.f / scale[g];
  v = v * is * is / (float)(n - 1);
  const long Cpad = (long)nt * PCA_T;
  float* cg = cov + (long)g * Cpad * Cpad;
  const long a = (long)ti * PCA_T + i, b = (long)tj * PCA_T + j;
  cg[a * Cpad + b] = v;
  cg[b * Cpad + a] = v;
}

__device__ __forceinline__ float pca_hash(unsigned x) {          // a fixed value in [-1, 1) per (channel, vector)
  x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
  return (float)(int)x * 4.656612873077393e-10f;
}

// Q (G, 8, Cpad): vectors j < m hashed on channels c < C, zero elsewhere; done and info cleared
__global__ __launch_bounds__(256) void pca_init_kernel(float* Q, int* done, int* polish, int* info, int C, int Cpad, int m) {
  const int g = blockIdx.y, j = blockIdx.x;
  for (int c = threadIdx.x; c < Cpad; c += 256)
    Q[((long)g * PCA_M + j) * Cpad + c] = (j < m && c < C) ? pca_hash((unsigned)(c * PCA_M + j) + 0x9e3779b9U) : 0.f;
  if (j == 0 && threadIdx.x == 0) { done[g] = 0; polish[g] = -1; info[2 * g] = 0; info[2 * g + 1] = 0; }
}

// Z[j][c] = sum_c' cov[c][c'] Q[j][c']: one wave per row c, lanes along c' with 16 bytes each, a butterfly over the lanes
__global__ __launch_bounds__(256) void pca_matvec_kernel(const float* cov, const float* Q, float* Z, const int* done, int Cpad) {
  const int g = blockIdx.y;
  if (done && done[g]) return;
  const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  const float* row = cov + ((long)g * Cpad + c) * Cpad;
  const float* q = Q + (long)g * PCA_M * Cpad;
  float acc[PCA_M];
#pragma unroll
  for (int j = 0; j < PCA_M; ++j) acc[j] = 0.f;
  for (int x = lane * 4; x < Cpad; x += 256) {
    const float4 a = *(const float4*)(row + x);
#pragma unroll
    for (int j = 0; j < PCA_M; ++j) {
      const float4 v = *(const float4*)(q + (long)j * Cpad + x);
      acc[j] = fmaf(a.x, v.x, acc[j]);
      acc[j] = fmaf(a.y, v.y, acc[j]);
      acc[j] = fmaf(a.z, v.z, acc[j]);
      acc[j] = fmaf(a.w, v.w, acc[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < PCA_M; ++j)
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc[j] += __shfl_xor(acc[j], off);
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < PCA_M; ++j) Z[((long)g * PCA_M + j) * Cpad + c] = acc[j];
  }
}

// the sums of N values over the 1024 threads of a workgroup, every thread receives them: a butterfly inside each wave, then the sixteen waves in
// order.  red: 16 N floats
template <int N>
__device__ __forceinline__ void pca_block_sum(float (&v)[N], float* red) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v[i] += __shfl_xor(v[i], off);
  __syncthreads();
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < N; ++i) red[w * N + i] = v[i];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < N; ++i) {
    float a = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) a += red[k * N + i];
    v[i] = a;
  }
}

// One workgroup (1024 threads, thread t on rows t + 1024 i, i < R) per PCA.  first: the starting block is orthonormalised.  Otherwise, with Q orthonormal
// and Z = cov Q: H = Q^T Z, symmetrised; its eigenpairs by cyclic Jacobi on wave 0 (lane 8 r + c holds H[r][c] and W[r][c], a rotation is three
// broadcasts and three exchanges), the first m = min(8, C) sorted descending (the unused ones behind them); the Ritz vectors V = Q W -> Vr, values -> lam, and cov V = Z W; the PCA has converged when
// ||cov v_j - lambda_j v_j|| <= tol lambda_1 for the k wanted pairs.  If not, the next block is Z W orthonormalised by classical Gram-Schmidt, two
// passes per vector; a vector whose remainder falls below 2^-20 of the first vector's length (a direction the covariance does not have) becomes
// zero and stays zero.
template <int R>
__global__ __launch_bounds__(1024) void pca_ritz_kernel(float* Q, const float* Z, float* Vr, float* lam, int* info, int* done, int* polish, int Cpad,
                                                        int k, int m, float tol, int first) {
  __shared__ float red[16 * 16];
  __shared__ float Hs[64], Ws[64], th[PCA_M];
  const int g = blockIdx.x;
  if (done[g]) return;
  const int pol0 = polish[g], count = info[2 * g] + 1;  // (read before the first barrier, written after it)
  float* Qg = Q + (long)g * PCA_M * Cpad;
  const float* Zg = Z + (long)g * PCA_M * Cpad;
  float q[R][PCA_M], y[R][PCA_M];
#pragma unroll
  for (int i = 0; i < R; ++i) {
    const int c = threadIdx.x + 1024 * i;
#pragma unroll
    for (int j = 0; j < PCA_M; ++j) {
      q[i][j] = c < Cpad ? Qg[(long)j * Cpad + c] : 0.f;
      y[i][j] = (c < Cpad && !first) ? Zg[(long)j * Cpad + c] : 0.f;
    }
  }
  if (first) {
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int j = 0; j < PCA_M; ++j) y[i][j] = q[i][j];
  } else {
#pragma unroll
    for (int a0 = 0; a0 < PCA_M; a0 += 2) {
      float hh[16];
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        float a = 0.f;
#pragma unroll
        for (int i = 0; i < R; ++i) a = fmaf(q[i][a0 + (e >> 3)], y[i][e & 7], a);
        hh[e] = a;
      }
      pca_block_sum<16>(hh, red);
      if (threadIdx.x == 0) {
#pragma unroll
        for (int e = 0; e < 16; ++e) Hs[a0 * 8 + e] = hh[e];
      }
    }
    __syncthreads();
    if (threadIdx.x < 64) {
      const int l = threadIdx.x, r = l >> 3, cc = l & 7;
      float hv = 0.5f * (Hs[l] + Hs[cc * 8 + r]), wv = r == cc ? 1.f : 0.f;
      for (int sweep = 0; sweep < 16; ++sweep) {
        float od = r != cc ? hv * hv : 0.f, dg = r == cc ? hv * hv : 0.f;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) { od += __shfl_xor(od, off); dg += __shfl_xor(dg, off); }
        if (!(od > 1e-14f * dg)) break;
        for (int p = 0; p < PCA_M - 1; ++p)
          for (int qq = p + 1; qq < PCA_M; ++qq) {
            const float hpp = __shfl(hv, p * 9), hqq = __shfl(hv, qq * 9), hpq = __shfl(hv, p * 8 + qq);
            if (!(fabsf(hpq) > 1e-37f)) continue;
            const float theta = (hqq - hpp) / (2.f * hpq);
            const float tt = copysignf(1.f, theta) / (fabsf(theta) + sqrtf(theta * theta + 1.f));
            const float cs = 1.f / sqrtf(tt * tt + 1.f), sn = tt * cs;
            float o = __shfl(hv, r * 8 + (cc == p ? qq : p));               // H <- H J: columns p and q
            if (cc == p) hv = cs * hv - sn * o; else if (cc == qq) hv = sn * o + cs * hv;
            o = __shfl(hv, (r == p ? qq : p) * 8 + cc);                    // H <- J^T H: rows p and q
            if (r == p) hv = cs * hv - sn * o; else if (r == qq) hv = sn * o + cs * hv;
            if ((r == p && cc == qq) || (r == qq && cc == p)) hv = 0.f;    // the element the rotation annihilates
            o = __shfl(wv, r * 8 + (cc == p ? qq : p));                     // W <- W J
            if (cc == p) wv = cs * wv - sn * o; else if (cc == qq) wv = sn * o + cs * wv;
          }
      }
      const float mine = __shfl(hv, cc * 9);
      int rank = 0;
      for (int b = 0; b < PCA_M; ++b) {
        const float tb = __shfl(hv, b * 9);
        // the unused vectors j >= m (zero columns, Ritz value exactly 0) stay behind the m of the block, whatever the sign of a tiny Ritz value
        const bool bin = b < m, cin = cc < m;
        rank += ((bin && !cin) || (bin == cin && (tb > mine || (tb == mine && b < cc)))) ? 1 : 0;
      }
      Ws[r * 8 + rank] = wv;
      if (r == cc) th[rank] = hv;
    }
    __syncthreads();
    // V = Q W into q, cov V = Z W into y
#pragma unroll
    for (int i = 0; i < R; ++i) {
      float v[PCA_M], u[PCA_M];
#pragma unroll
      for (int j = 0; j < PCA_M; ++j) {
        float a = 0.f, b = 0.f;
#pragma unroll
        for (int e = 0; e < PCA_M; ++e) { a = fmaf(q[i][e], Ws[e * 8 + j], a); b = fmaf(y[i][e], Ws[e * 8 + j], b); }
        v[j] = a; u[j] = b;
      }
#pragma unroll
      for (int j = 0; j < PCA_M; ++j) { q[i][j] = v[j]; y[i][j] = u[j]; }
    }
    float rs[PCA_M];
#pragma unroll
    for (int j = 0; j < PCA_M; ++j) {
      float a = 0.f;
#pragma unroll
      for (int i = 0; i < R; ++i) { const float d = y[i][j] - th[j] * q[i][j]; a = fmaf(d, d, a); }
      rs[j] = a;
    }
    pca_block_sum<PCA_M>(rs, red);
    bool conv = true;
#pragma unroll
    for (int j = 0; j < PCA_M; ++j)
      if (j < k && !(sqrtf(rs[j]) <= tol * th[0])) conv = false;
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const int c = threadIdx.x + 1024 * i;
      if (c < Cpad) {
#pragma unroll
        for (int j = 0; j < PCA_M; ++j) Vr[((long)g * PCA_M + j) * Cpad + c] = q[i][j];
      }
    }
    if (threadIdx.x < PCA_M) lam[g * PCA_M + threadIdx.x] = th[threadIdx.x];
    // the criterion bounds an eigenvector's error by tol lambda_1 / gap only; count / 2 + 2 further iterations take the residual to its fp32 floor
    const int rem = pol0 < 0 ? (conv ? count / 2 + 2 : -1) : pol0 - 1;
    if (threadIdx.x == 0) {
      info[2 * g] = count;
      if (pol0 < 0 && conv) info[2 * g + 1] = 1;
      polish[g] = rem;
      if (rem == 0) done[g] = 1;
    }
    if (rem == 0) return;                              // (every thread holds the same sums: uniform)
  }
  // the next block: y orthonormalised into q
  float ref0 = 0.f;
#pragma unroll
  for (int j = 0; j < PCA_M; ++j) {
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
      float d[PCA_M + 1];
#pragma unroll
      for (int a = 0; a < PCA_M + 1; ++a) d[a] = 0.f;
#pragma unroll
      for (int i = 0; i < R; ++i) {
#pragma unroll
        for (int a = 0; a < j; ++a) d[a] = fmaf(q[i][a], y[i][j], d[a]);
        d[PCA_M] = fmaf(y[i][j], y[i][j], d[PCA_M]);
      }
      pca_block_sum<PCA_M + 1>(d, red);
      if (j == 0 && pass == 0) ref0 = d[PCA_M];
#pragma unroll
      for (int i = 0; i < R; ++i)
#pragma unroll
        for (int a = 0; a < j; ++a) y[i][j] = fmaf(-d[a], q[i][a], y[i][j]);
    }
    float na[1] = {0.f};
#pragma unroll
    for (int i = 0; i < R; ++i) na[0] = fmaf(y[i][j], y[i][j], na[0]);
    pca_block_sum<1>(na, red);
    const float inv = (na[0] > 0.f && na[0] > 9.094947017729282e-13f * ref0) ? 1.f / sqrtf(na[0]) : 0.f;   // (2^-20)^2
#pragma unroll
    for (int i = 0; i < R; ++i) q[i][j] = y[i][j] * inv;
  }
#pragma unroll
  for (int i = 0; i < R; ++i) {
    const int c = threadIdx.x + 1024 * i;
    if (c < Cpad) {
#pragma unroll
      for (int j = 0; j < PCA_M; ++j) Qg[(long)j * Cpad + c] = q[i][j];
    }
  }
}

// One workgroup = component j of PCA g.  Z = cov Vr (one more pca_matvec_kernel): the eigenvalue is the Rayleigh quotient <v, cov v> / <v, v> accumulated
// in double, rounded once.  An eigenvalue that is not above 2^-20 of the first cannot be told from rounding in fp32: the component is written as the
// zero vector with variance 0.  Otherwise the entry of largest magnitude (the lowest channel among equals) becomes positive.  For j == 0 the trace
// of cov in a fixed tree.
__global__ __launch_bounds__(256) void pca_finalize_kernel(const float* Vr, const float* Z, const float* cov, int C, int Cpad, int k,
                                                           float* components, float* variance, float* total) {
  __shared__ float rv[256];
  __shared__ int ri[256];
  __shared__ double rd[256], rd2[256];
  __shared__ float lam_s[2];
  const int j = blockIdx.x, g = blockIdx.y;
  for (int which = 0; which < 2; ++which) {            // the first eigenvalue, then this one
    const int jj = which ? j : 0;
    const float* v = Vr + ((long)g * PCA_M + jj) * Cpad;
    const float* z = Z + ((long)g * PCA_M + jj) * Cpad;
    double a = 0.0, b = 0.0;                          // <v, cov v> and <v, v>: v has unit length only to fp32 rounding
    for (int c = threadIdx.x; c < C; c += 256) { a += (double)v[c] * (double)z[c]; b += (double)v[c] * (double)v[c]; }
    rd[threadIdx.x] = a;
    rd2[threadIdx.x] = b;
    __syncthreads();
#pragma unroll
    for (int half = 128; half >= 1; half >>= 1) {
      if ((int)threadIdx.x < half) { rd[threadIdx.x] += rd[threadIdx.x + half]; rd2[threadIdx.x] += rd2[threadIdx.x + half]; }
      __syncthreads();
    }
    if (threadIdx.x == 0) lam_s[which] = rd2[0] > 0.0 ? (float)(rd[0] / rd2[0]) : 0.f;
    __syncthreads();
  }
  const bool keep = lam_s[1] > 9.5367431640625e-07f * lam_s[0] && lam_s[1] > 0.f;
  const float* v = Vr + ((long)g * PCA_M + j) * Cpad;
  float best = -1.f;
  int bi = 0;
  for (int c = threadIdx.x; c < C; c += 256) {
    const float a = fabsf(v[c]);
    if (a > best) { best = a; bi = c; }
  }
  rv[threadIdx.x] = best;
  ri[threadIdx.x] = bi;
  __syncthreads();
#pragma unroll
  for (int half = 128; half >= 1; half >>= 1) {
    if ((int)threadIdx.x < half) {
      const float a = rv[threadIdx.x + half];
      const int ia = ri[threadIdx.x + half];
      if (a > rv[threadIdx.x] || (a == rv[threadIdx.x] && ia < ri[threadIdx.x])) { rv[threadIdx.x] = a; ri[threadIdx.x] = ia; }
    }
    __syncthreads();
  }
  const float sg = !keep ? 0.f : v[ri[0]] < 0.f ? -1.f : 1.f;
  for (int c = threadIdx.x; c < C; c += 256) components[((long)g * k + j) * C + c] = keep ? sg * v[c] : 0.f;
  if (threadIdx.x == 0) variance[g * k + j] = keep ? lam_s[1] : 0.f;
  if (j == 0) {
    __syncthreads();
    float t = 0.f;
    for (int c = threadIdx.x; c < C; c += 256) t += cov[((long)g * Cpad + c) * Cpad + c];
    rv[threadIdx.x] = t;
    __syncthreads();
#pragma unroll
    for (int half = 128; half >= 1; half >>= 1) {
      if ((int)threadIdx.x < half) rv[threadIdx.x] += rv[threadIdx.x + half];
      __syncthreads();
    }
    if (threadIdx.x == 0) total[g] = rv[0];
  }
}

// One workgroup = 64 pixels of image b: per tile of 32 channels the values go through LDS; thread t: pixel t % 64, channels 8 (t / 64) .. + 7 of
// the tile (its wave's channels: mean and components come through uniform loads); the four slices are added in order.
template <typename T>
__global__ __launch_bounds__(256) void pca_project_kernel(PcaSrc s, int joint, const float* mean, const float* components, int k, float* proj) {
  __shared__ float tile[32 * PCA_LD];
  __shared__ float red[4 * PCA_M * 64];
  const int b = blockIdx.y, g = joint ? 0 : b, HW = s.H * s.W;
  const int px = threadIdx.x & 63, sl = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long p0 = (long)blockIdx.x * 64;
  const float* mu = mean + (long)g * s.C;
  const float* cp = components + (long)g * k * s.C;
  float acc[PCA_M];
#pragma unroll
  for (int j = 0; j < PCA_M; ++j) acc[j] = 0.f;
  for (int c0 = 0; c0 < s.C; c0 += 32) {
    pca_tile<T, 32, 64, 256>(s, b, c0, p0, HW, [&](int c, int p, float v, bool) { tile[c * PCA_LD + p] = v; });
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int c = c0 + sl * 8 + e;
      if (c < s.C) {                                    // (wave-uniform)
        const float d = tile[(sl * 8 + e) * PCA_LD + px] - mu[c];
#pragma unroll
        for (int j = 0; j < PCA_M; ++j)
          if (j < k) acc[j] = fmaf(d, cp[(long)j * s.C + c], acc[j]);
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < PCA_M; ++j) red[(sl * PCA_M + j) * 64 + px] = acc[j];
  __syncthreads();
  if (sl == 0 && p0 + px < HW) {
#pragma unroll
    for (int j = 0; j < PCA_M; ++j)
      if (j < k) {
        const float v = ((red[j * 64 + px] + red[(PCA_M + j) * 64 + px]) + red[(2 * PCA_M + j) * 64 + px]) + red[(3 * PCA_M + j) * 64 + px];
        proj[((long)b * k + j) * HW + p0 + px] = v;
      }
  }
}

// One workgroup = a stripe of output pixels of image b.  It first takes min and max of the three components over the image (the batch when joint):
// exact whatever the order; then n = (p - min) / (max - min), n * 255 truncated; the source pixel of output (oy, ox) is
// floor((o + 0.5) in / out) per axis, in integers.
__global__ __launch_bounds__(1024) void pca_rgb_kernel(const float* proj, int B, int H, int W, int joint, unsigned char* out, int OH, int OW) {
  __shared__ float rmin[16 * 3], rmax[16 * 3];
  const int b = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long HW = (long)H * W, n = joint ? (long)B * HW : HW;
  float mn[3], mx[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    float lo = INFINITY, hi = -INFINITY;
    for (long i = threadIdx.x; i < n; i += 1024) {
      const long bb = joint ? i / HW : b, q = joint ? i % HW : i;
      const float v = proj[(bb * 3 + j) * HW + q];
      lo = fminf(lo, v);
      hi = fmaxf(hi, v);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) { lo = fminf(lo, __shfl_xor(lo, off)); hi = fmaxf(hi, __shfl_xor(hi, off)); }
    if (lane == 0) { rmin[w * 3 + j] = lo; rmax[w * 3 + j] = hi; }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    float lo = rmin[j], hi = rmax[j];
#pragma unroll
    for (int i = 1; i < 16; ++i) { lo = fminf(lo, rmin[i * 3 + j]); hi = fmaxf(hi, rmax[i * 3 + j]); }
    mn[j] = lo;
    mx[j] = hi - lo;
  }
  const long total = (long)OH * OW;
  for (long o = (long)blockIdx.x * 1024 + threadIdx.x; o < total; o += (long)gridDim.x * 1024) {
    const long oy = o / OW, ox = o % OW;
    const long iy = min((long)H - 1, (2 * oy + 1) * H / (2l * OH)), ix = min((long)W - 1, (2 * ox + 1) * W / (2l * OW));
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const float nv = (proj[((long)b * 3 + j) * HW + iy * W + ix] - mn[j]) / mx[j];
      const float c = nv * 255.f;
      out[((long)b * total + o) * 3 + j] = mx[j] > 0.f ? (unsigned char)(int)c : (unsigned char)0;
    }
  }
}

// the sample ranges of the covariance: enough workgroups to fill the device, whole staging steps, and at most 8192 samples in one fp32
// accumulation chain while n <= 64 * 8192 (S is capped at 64: beyond that the chain, and its rounding error, grow with n / 64)
void pca_splits(int ntiles, long n, int& S, long& per) {
  long s = std::max<long>((512 + ntiles - 1) / ntiles, (n + 8191) / 8192);
  s = std::max<long>(1, std::min<long>(std::min<long>(s, 64), (n + PCA_TP - 1) / PCA_TP));
  per = ((n + s - 1) / s + PCA_TP - 1) / PCA_TP * PCA_TP;
  S = (int)((n + per - 1) / per);
}

struct PcaWs { float *chmax, *scale, *part, *cov, *Q, *Z, *Vr, *lam; int *done, *polish; size_t bytes; };
PcaWs pca_carve(void* base, int G, int C, long n) {
  const size_t nt = (size_t)(C + PCA_T - 1) / PCA_T, Cpad = nt * PCA_T, ntiles = nt * (nt + 1) / 2;
  int S;
  long per;
  pca_splits((int)ntiles, n, S, per);
  Carver c(base);
  PcaWs ws;
  ws.chmax = c.take<float>((size_t)G * C * 4);
  ws.scale = c.take<float>((size_t)G * 4);
  ws.part = c.take<float>((size_t)G * S * ntiles * PCA_T * PCA_T * 4);
  ws.cov = c.take<float>((size_t)G * Cpad * Cpad * 4);
  ws.Q = c.take<float>((size_t)G * PCA_M * Cpad * 4);
  ws.Z = c.take<float>((size_t)G * PCA_M * Cpad * 4);
  ws.Vr = c.take<float>((size_t)G * PCA_M * Cpad * 4);
  ws.lam = c.take<float>((size_t)G * PCA_M * 4);
  ws.done = c.take<int>((size_t)G * 4);
  ws.polish = c.take<int>((size_t)G * 4);
  ws.bytes = c.bytes();
  return ws;
}

PcaSrc pca_src(const AggSrc& f) { return PcaSrc{f.ptr, f.sb, f.sc, f.sy, f.sx, f.C, f.H, f.W, map_lanes_c(f) ? 1 : 0}; }

void pca_ritz(const PcaWs& ws, int G, int Cpad, int k, int m, float tol, int first, int* info, hipStream_t s) {
  const dim3 g((unsigned)G), b(1024);
  switch ((Cpad + 1023) / 1024) {                      // rows per thread
    case 1: hipLaunchKernelGGL(pca_ritz_kernel<1>, g, b, 0, s, ws.Q, ws.Z, ws.Vr, ws.lam, info, ws.done, ws.polish, Cpad, k, m, tol, first); break;
    case 2: hipLaunchKernelGGL(pca_ritz_kernel<2>, g, b, 0, s, ws.Q, ws.Z, ws.Vr, ws.lam, info, ws.done, ws.polish, Cpad, k, m, tol, first); break;
    case 3: hipLaunchKernelGGL(pca_ritz_kernel<3>, g, b, 0, s, ws.Q, ws.Z, ws.Vr, ws.lam, info, ws.done, ws.polish, Cpad, k, m, tol, first); break;
    default: hipLaunchKernelGGL(pca_ritz_kernel<4>, g, b, 0, s, ws.Q, ws.Z, ws.Vr, ws.lam, info, ws.done, ws.polish, Cpad, k, m, tol, first); break;
  }
}

}  // namespace

size_t pca_workspace(int B, int C, int H, int W, int joint) {
  return pca_carve(nullptr, joint ? 1 : B, C, (joint ? (long)B : 1l) * H * W).bytes;
}

hipError_t launch_pca(const AggSrc& f, int B, int k, int joint, int max_iter, float tol, float* mean, float* components, float* variance,
                      float* total_variance, float* projection, int* info, void* workspace, hipStream_t s) {
  const long HW = (long)f.H * f.W, n = (joint ? (long)B : 1l) * HW;
  if (!f.ptr || !mean || !components || !variance || !total_variance || !info || !workspace || ((uintptr_t)workspace & 15))
    return hipErrorInvalidValue;
  if (B < 0 || B > 65535 || f.C < 1 || f.C > PCA_MAXC || f.H < 1 || f.W < 1 || (long)std::max(B, 1) * HW >= (1l << 31)) return hipErrorInvalidValue;
  if (B == 0) return hipSuccess;
  if (k < 1 || k > PCA_M || k > f.C || k > n - 1 || max_iter < 1 || max_iter > PCA_MAXITER || !(tol >= 0.f && tol < INFINITY))
    return hipErrorInvalidValue;
  const int G = joint ? 1 : B, C = f.C, nt = (C + PCA_T - 1) / PCA_T, Cpad = nt * PCA_T, ntiles = nt * (nt + 1) / 2, m = std::min<int>(PCA_M, C);
  int S;
  long per;
  pca_splits(ntiles, n, S, per);
  const PcaWs ws = pca_carve(workspace, G, C, n);
  const PcaSrc src = pca_src(f);
  const dim3 gm((unsigned)((C + 31) / 32), (unsigned)G), gc((unsigned)ntiles, (unsigned)S, (unsigned)G);
  if (f.f32) {
    hipLaunchKernelGGL(pca_mean_kernel<float>, gm, dim3(256), 0, s, src, joint, n, mean, ws.chmax);
  } else {
    hipLaunchKernelGGL(pca_mean_kernel<_Float16>, gm, dim3(256), 0, s, src, joint, n, mean, ws.chmax);
  }
  hipLaunchKernelGGL(pca_scale_kernel, dim3((unsigned)G), dim3(256), 0, s, ws.chmax, C, ws.scale);
  if (f.f32) {
    hipLaunchKernelGGL(pca_cov_kernel<float>, gc, dim3(256), 0, s, src, joint, n, per, mean, ws.scale, ws.part, nt);
  } else {
    hipLaunchKernelGGL(pca_cov_kernel<_Float16>, gc, dim3(256), 0, s, src, joint, n, per, mean, ws.scale, ws.part, nt);
  }
  hipLaunchKernelGGL(pca_cov_reduce_kernel, dim3((unsigned)ntiles * 64, (unsigned)G), dim3(256), 0, s, ws.part, S, ntiles, nt, ws.scale, n, ws.cov);
  hipLaunchKernelGGL(pca_init_kernel, dim3(PCA_M, (unsigned)G), dim3(256), 0, s, ws.Q, ws.done, ws.polish, info, C, Cpad, m);
  pca_ritz(ws, G, Cpad, k, m, tol, 1, info, s);
  for (int it = 0; it < max_iter; ++it) {
    hipLaunchKernelGGL(pca_matvec_kernel, dim3((unsigned)Cpad / 4, (unsigned)G), dim3(256), 0, s, ws.cov, ws.Q, ws.Z, ws.done, Cpad);
    pca_ritz(ws, G, Cpad, k, m, tol, 0, info, s);
  }
  hipLaunchKernelGGL(pca_matvec_kernel, dim3((unsigned)Cpad / 4, (unsigned)G), dim3(256), 0, s, ws.cov, ws.Vr, ws.Z, (const int*)nullptr, Cpad);
  hipLaunchKernelGGL(pca_finalize_kernel, dim3((unsigned)k, (unsigned)G), dim3(256), 0, s, ws.Vr, ws.Z, ws.cov, C, Cpad, k, components, variance,
                     total_variance);
  if (projection) {
    const dim3 gp((unsigned)((HW + 63) / 64), (unsigned)B);
    if (f.f32) {
      hipLaunchKernelGGL(pca_project_kernel<float>, gp, dim3(256), 0, s, src, joint, mean, components, k, projection);
    } else {
      hipLaunchKernelGGL(pca_project_kernel<_Float16>, gp, dim3(256), 0, s, src, joint, mean, components, k, projection);
    }
  }
  return hipGetLastError();
}

hipError_t launch_pca_rgb(const float* projection, int B, int H, int W, int joint, unsigned char* out, int OH, int OW, hipStream_t s) {
  if (!projection || !out || B < 0 || B > 65535 || H < 1 || W < 1 || OH < 1 || OW < 1) return hipErrorInvalidValue;
  if (B == 0) return hipSuccess;
  const long total = (long)OH * OW;
  // every workgroup takes the min / max itself (the op has no workspace): at most 64 stripes per image, and with joint, where a workgroup reads
  // the whole batch, at most 64 workgroups in all while B <= 64 (beyond that one per image: B^2 H W reads)
  const long cap = joint ? std::max<long>(1, 64 / B) : 64;
  const unsigned stripes = (unsigned)std::max<long>(1, std::min<long>(cap, (total + 1023) / 1024));
  hipLaunchKernelGGL(pca_rgb_kernel, dim3(stripes, (unsigned)B), dim3(1024), 0, s, projection, B, H, W, joint, out, OH, OW);
  return hipGetLastError();
}

}  // namespace gdf
