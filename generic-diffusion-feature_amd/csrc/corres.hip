// Nearest-neighbour correspondence of annotated source points on two aggregated feature maps, gfx950.
//
// Reference op replaced (paths under /root/reference):
//   correspondence/correspondence/correspondence_utils.py:113-138   find_nn_source_correspondences: F.interpolate of both (B, C, h, w) maps to
//   the load size (bilinear), gather of the N source points, L2 normalisation of both sides, sims = q @ k^T, argmax over the LH * LW pixels
//
// Neither load-size map is materialised.  Bilinear interpolation is linear, so for a fine target pixel p with coarse taps T_i and weights w_i
//   <q, v_p> = sum_i w_i <q, T_i>            ||v_p||^2 = sum_ij w_i w_j <T_i, T_j>
// and one pass over the COARSE target yields everything the fine grid needs:
//   nn_query_kernel     B * NQ workgroups: the four taps of every source point blended in fp32 -> q (B, C, NQ) fp32 and 1 / ||q|| (B, NQ); the
//                       coarse kernels apply that factor once per product, so D holds <q_n / ||q_n||, T>
//   nn_coarse_x_kernel  lanes along x (NCHW, and any other strides): per coarse pixel D[n] = <q_n, T> and the five neighbour products
//   nn_coarse_c_kernel  lanes along C (channels-last, 16-byte loads): the same numbers
//   nn_fine_kernel      over LH x LW, one wave per 64 pixels x 4 queries: blend, scale by 1 / the Gram-form norm, per-lane best, wave fold -> partials
//   nn_final_kernel     B * N workgroups: the partials of one query -> (y, x) int64 and the fp32 score
// Every reduction has a fixed order and the comparison is a total order (score, then lowest index): the same inputs give the same bits.
// Queries are processed in chunks of at most NN_MAXQ; everything accumulates in fp32.
#include <math.h>

#include <algorithm>

#include "feat_common.h"

namespace gdf {

namespace {

enum { NN_NG = 5 };                                   // <T,T> <T,T_right> <T,T_down> <T,T_diag> <T_right,T_down>; neighbours clamp at the border

// bilinear_src, except that where the second tap clamps onto the first the weight is irrelevant and is returned as 0: every fine row (column)
// of such a run computes the same bits.
__device__ __forceinline__ void nn_src(int dst, float scale, int in, int& i0, int& i1, float& l1) {
  bilinear_src(dst, scale, in, i0, i1, l1);
  if (i1 == i0) l1 = 0.f;
}

// One workgroup = one (sample b, query slot n of the chunk).  points: (B, N, 2) fp32 (y, x) in load-size coordinates; the source index is
// round_half_even(clip(.)) as np.round does.  q: (B, C, NQ) fp32, not normalised; qi: (B, NQ) = 1 / ||q||; slots n >= nc are zero-filled.
__global__ __launch_bounds__(1024) void nn_query_kernel(const void* f, int f32, long sb, long sc, long sy, long sx, int C, int h, int w,
                                                        const float* points, int N, int n0, int nc, int NQ, int LH, int LW, float* q, float* qi) {
  __shared__ float part[16];
  const int n = blockIdx.x % NQ, b = blockIdx.x / NQ;
  float* qn = q + (long)b * C * NQ + n;
  if (n >= nc) {
    for (int c = threadIdx.x; c < C; c += 1024) qn[(long)c * NQ] = 0.f;
    if (threadIdx.x == 0) qi[b * NQ + n] = 0.f;
    return;
  }
  const float* pt = points + ((long)b * N + n0 + n) * 2;
  const int py = (int)rintf(fminf(fmaxf(pt[0], 0.f), (float)(LH - 1))), px = (int)rintf(fminf(fmaxf(pt[1], 0.f), (float)(LW - 1)));
  int y0, y1, x0, x1;
  float ly1, lx1;
  nn_src(py, (float)h / (float)LH, h, y0, y1, ly1);
  nn_src(px, (float)w / (float)LW, w, x0, x1, lx1);
  const float ly0 = 1.f - ly1, lx0 = 1.f - lx1;
  const long o00 = (long)b * sb + (long)y0 * sy + (long)x0 * sx, o01 = (long)b * sb + (long)y0 * sy + (long)x1 * sx;
  const long o10 = (long)b * sb + (long)y1 * sy + (long)x0 * sx, o11 = (long)b * sb + (long)y1 * sy + (long)x1 * sx;
  float ss = 0.f;
  for (int c = threadIdx.x; c < C; c += 1024) {
    const long oc = (long)c * sc;
    float t00, t01, t10, t11;
    if (f32) { t00 = ld<float>(f, o00 + oc); t01 = ld<float>(f, o01 + oc); t10 = ld<float>(f, o10 + oc); t11 = ld<float>(f, o11 + oc); }
    else { t00 = ld<_Float16>(f, o00 + oc); t01 = ld<_Float16>(f, o01 + oc); t10 = ld<_Float16>(f, o10 + oc); t11 = ld<_Float16>(f, o11 + oc); }
    const float v = ly0 * (lx0 * t00 + lx1 * t01) + ly1 * (lx0 * t10 + lx1 * t11);
    qn[(long)c * NQ] = v;
    ss += v * v;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) ss += __shfl_xor(ss, off);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = ss;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int k = 0; k < 16; ++k) t += part[k];
    qi[b * NQ + n] = 1.f / sqrtf(t);                  // (a zero norm gives inf, every product 0 * inf = NaN: no pixel wins)
  }
}

// One workgroup = 64 consecutive coarse pixels of one sample (flattened y * w + x: lanes along x) x 16 channel slices, one wave each.  Every
// lane reads its pixel and the right / down / diagonal neighbours (clamped at the border) channel by channel with the tensor's own strides:
// coalesced where sx == 1.  The wave's channel is uniform, so q comes through scalar loads.  The slices are summed through LDS in a fixed tree.
//   D: (B, h * w, NQ)   G: (B, h * w, 8) with the NN_NG products in slots 0..4
template <typename T, int NQ>
__global__ __launch_bounds__(1024) void nn_coarse_x_kernel(const T* f, long sb, long sc, long sy, long sx, int C, int h, int w, const float* q,
                                                           const float* qi, float* D, float* G) {
  constexpr int NV = NQ + NN_NG;
  __shared__ float red[8 * NV * 64];
  const int lane = threadIdx.x & 63, s = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = blockIdx.y, hw = h * w;
  const int p = blockIdx.x * 64 + lane;
  const int pp = min(p, hw - 1);                      // lanes past the plane compute a valid pixel and store nothing
  const int y = pp / w, x = pp - y * w;
  const int x1 = min(x + 1, w - 1), y1 = min(y + 1, h - 1);
  const T* fb = f + (long)b * sb;
  const long o00 = (long)y * sy + (long)x * sx, o01 = (long)y * sy + (long)x1 * sx;
  const long o10 = (long)y1 * sy + (long)x * sx, o11 = (long)y1 * sy + (long)x1 * sx;
  const int per = (C + 15) / 16, cb = s * per, ce = min(C, cb + per);
  const float* qb = q + (long)b * C * NQ;
  float acc[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) acc[v] = 0.f;
#pragma unroll 2
  for (int c = cb; c < ce; ++c) {
    const T* fc = fb + (long)c * sc;
    const float t = (float)fc[o00], r = (float)fc[o01], d = (float)fc[o10], g = (float)fc[o11];
    const float* qc = qb + (long)c * NQ;
#pragma unroll
    for (int n = 0; n < NQ; ++n) acc[n] = fmaf(t, qc[n], acc[n]);
    acc[NQ] = fmaf(t, t, acc[NQ]);
    acc[NQ + 1] = fmaf(t, r, acc[NQ + 1]);
    acc[NQ + 2] = fmaf(t, d, acc[NQ + 2]);
    acc[NQ + 3] = fmaf(t, g, acc[NQ + 3]);
    acc[NQ + 4] = fmaf(r, d, acc[NQ + 4]);
  }
#pragma unroll
  for (int half = 8; half >= 1; half >>= 1) {         // slices [half, 2 half) hand their sums to slices [0, half)
    if (s >= half && s < 2 * half) {
#pragma unroll
      for (int v = 0; v < NV; ++v) red[((s - half) * NV + v) * 64 + lane] = acc[v];
    }
    __syncthreads();
    if (s < half) {
#pragma unroll
      for (int v = 0; v < NV; ++v) acc[v] += red[(s * NV + v) * 64 + lane];
    }
    __syncthreads();
  }
  if (s == 0 && p < hw) {
    float* d = D + ((long)b * hw + p) * NQ;
    const float* s_ = qi + b * NQ;
#pragma unroll
    for (int n = 0; n < NQ; n += 4)
      *(float4*)(d + n) = make_float4(acc[n] * s_[n], acc[n + 1] * s_[n + 1], acc[n + 2] * s_[n + 2], acc[n + 3] * s_[n + 3]);
    float* g = G + ((long)b * hw + p) * 8;
    *(float4*)g = make_float4(acc[NQ], acc[NQ + 1], acc[NQ + 2], acc[NQ + 3]);
    g[4] = acc[NQ + 4];
  }
}

// Channels-last (sc == 1, C a multiple of the 16-byte vector, every pixel 16-byte aligned): one wave = NN_P consecutive pixels of one row, lanes
// along C with 16 bytes each.  The NN_P + 1 pixels of rows y and y + 1 are loaded once per 64-lane channel block and shared by the NN_P pixels,
// as is the lane's V x NQ block of q; the per-lane sums are folded across the wave by a butterfly at the end.
enum { NN_P = 4 };
template <typename T, int NQ>
__global__ __launch_bounds__(256) void nn_coarse_c_kernel(const T* f, long sb, long sy, long sx, int C, int h, int w, long runs, const float* q,
                                                          const float* qi, float* D, float* G) {
  constexpr int V = 16 / (int)sizeof(T), NV = NQ + NN_NG;
  typedef T vt __attribute__((ext_vector_type(V)));
  const int lane = threadIdx.x & 63;
  const long run = (long)blockIdx.x * 4 + (threadIdx.x >> 6);      // (b, y, group of NN_P pixels)
  if (run >= runs) return;                                         // (whole waves; no barrier below)
  const int nxg = (w + NN_P - 1) / NN_P;
  const int xg = (int)(run % nxg), y = (int)((run / nxg) % h), b = (int)(run / ((long)nxg * h));
  const int xa = xg * NN_P, y1 = min(y + 1, h - 1);
  const T* r0 = f + (long)b * sb + (long)y * sy;
  const T* r1 = f + (long)b * sb + (long)y1 * sy;
  const float* qb = q + (long)b * C * NQ;
  float acc[NN_P][NV];
#pragma unroll
  for (int j = 0; j < NN_P; ++j)
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[j][v] = 0.f;
  for (int c = lane * V; c < C; c += 64 * V) {
    vt t0[NN_P + 1], t1[NN_P + 1];
#pragma unroll
    for (int j = 0; j <= NN_P; ++j) {
      const long o = (long)min(xa + j, w - 1) * sx + c;
      t0[j] = *(const vt*)(r0 + o);
      t1[j] = *(const vt*)(r1 + o);
    }
    const float* qc = qb + (long)c * NQ;
#pragma unroll
    for (int e = 0; e < V; ++e) {
      float qv[NQ];
#pragma unroll
      for (int n = 0; n < NQ; n += 4) {
        const float4 u = *(const float4*)(qc + e * NQ + n);
        qv[n] = u.x; qv[n + 1] = u.y; qv[n + 2] = u.z; qv[n + 3] = u.w;
      }
#pragma unroll
      for (int j = 0; j < NN_P; ++j) {
        const float t = (float)t0[j][e], r = (float)t0[j + 1][e], d = (float)t1[j][e], g = (float)t1[j + 1][e];
#pragma unroll
        for (int n = 0; n < NQ; ++n) acc[j][n] = fmaf(t, qv[n], acc[j][n]);
        acc[j][NQ] = fmaf(t, t, acc[j][NQ]);
        acc[j][NQ + 1] = fmaf(t, r, acc[j][NQ + 1]);
        acc[j][NQ + 2] = fmaf(t, d, acc[j][NQ + 2]);
        acc[j][NQ + 3] = fmaf(t, g, acc[j][NQ + 3]);
        acc[j][NQ + 4] = fmaf(r, d, acc[j][NQ + 4]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NN_P; ++j)
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) acc[j][v] += __shfl_xor(acc[j][v], off);
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < NN_P; ++j) {
      if (xa + j >= w) break;
      const long pix = (long)b * h * w + (long)y * w + xa + j;
      float* d = D + pix * NQ;
      const float* s_ = qi + b * NQ;
#pragma unroll
      for (int n = 0; n < NQ; n += 4)
        *(float4*)(d + n) = make_float4(acc[j][n] * s_[n], acc[j][n + 1] * s_[n + 1], acc[j][n + 2] * s_[n + 2], acc[j][n + 3] * s_[n + 3]);
      float* g = G + pix * 8;
      *(float4*)g = make_float4(acc[j][NQ], acc[j][NQ + 1], acc[j][NQ + 2], acc[j][NQ + 3]);
      g[4] = acc[j][NQ + 4];
    }
  }
}

// The fine grid: gridDim.x workgroups per sample walk the LH * LW pixels in tiles of 64, ascending.  One wave = the tile x four queries (so a
// block has NQ / 4 waves and no barrier).  Per pixel: ATen's taps and weights, the squared norm from the Gram planes (a pixel whose norm is not
// positive never wins), then the blended dot products times 1 / norm.  Each lane keeps (best score, its lowest index) per query; the wave folds
// them in a fixed order into ps / pi (B, NQ, gridDim.x).
template <int NQ>
__global__ __launch_bounds__(16 * NQ) void nn_fine_kernel(const float* D, const float* G, int h, int w, int LH, int LW, int nc, float* ps, unsigned* pi) {
  const int lane = threadIdx.x & 63, n4 = (threadIdx.x >> 6) * 4;
  if (n4 >= nc) return;                               // (whole waves)
  const int b = blockIdx.y, npix = LH * LW;
  const float fy = (float)h / (float)LH, fx = (float)w / (float)LW;
  const long pb = (long)b * h * w;
  float bs[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  unsigned bi[4] = {0u, 0u, 0u, 0u};
  for (int p = blockIdx.x * 64 + lane; p < npix; p += gridDim.x * 64) {
    const int y = p / LW, x = p - y * LW;
    int y0, y1, x0, x1;
    float ly1, lx1;
    nn_src(y, fy, h, y0, y1, ly1);
    nn_src(x, fx, w, x0, x1, lx1);
    const float ly0 = 1.f - ly1, lx0 = 1.f - lx1;
    const float wa = ly0 * lx0, wb = ly0 * lx1, wc = ly1 * lx0, wd = ly1 * lx1;
    const long p00 = pb + (long)y0 * w + x0, p01 = pb + (long)y0 * w + x1, p10 = pb + (long)y1 * w + x0, p11 = pb + (long)y1 * w + x1;
    const float4 g00 = *(const float4*)(G + p00 * 8), g01 = *(const float4*)(G + p01 * 8);      // x self, y right, z down, w diagonal
    const float4 g10 = *(const float4*)(G + p10 * 8), g11 = *(const float4*)(G + p11 * 8);
    const float anti = G[p00 * 8 + 4];                                                          // <T01, T10>
    const float4 a = *(const float4*)(D + p00 * NQ + n4), bq = *(const float4*)(D + p01 * NQ + n4);
    const float4 c = *(const float4*)(D + p10 * NQ + n4), d = *(const float4*)(D + p11 * NQ + n4);
    const float nsq = (wa * wa * g00.x + wb * wb * g01.x + wc * wc * g10.x + wd * wd * g11.x) +
                      2.f * (wa * wb * g00.y + wc * wd * g10.y + wa * wc * g00.z + wb * wd * g01.z + wa * wd * g00.w + wb * wc * anti);
    if (!(nsq > 0.f)) continue;
    const float inv = 1.f / sqrtf(nsq);
    const float s0 = (wa * a.x + wb * bq.x + wc * c.x + wd * d.x) * inv, s1 = (wa * a.y + wb * bq.y + wc * c.y + wd * d.y) * inv;
    const float s2 = (wa * a.z + wb * bq.z + wc * c.z + wd * d.z) * inv, s3 = (wa * a.w + wb * bq.w + wc * c.w + wd * d.w) * inv;
    if (s0 > bs[0]) { bs[0] = s0; bi[0] = (unsigned)p; }
    if (s1 > bs[1]) { bs[1] = s1; bi[1] = (unsigned)p; }
    if (s2 > bs[2]) { bs[2] = s2; bi[2] = (unsigned)p; }
    if (s3 > bs[3]) { bs[3] = s3; bi[3] = (unsigned)p; }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    wave_best(bs[k], bi[k]);
    if (lane == 0 && n4 + k < nc) {
      const long o = ((long)b * NQ + n4 + k) * gridDim.x + blockIdx.x;
      ps[o] = bs[k];
      pi[o] = bi[k];
    }
  }
}

// One wave = one (sample, query of the chunk): folds the nblk partials and writes (y, x) and the score.  A query no pixel answered (its own norm
// is zero, or every target norm is) gets index 0 and a NaN score.
__global__ __launch_bounds__(64) void nn_final_kernel(const float* ps, const unsigned* pi, int nblk, int NQ, int nc, int N, int n0, int LW,
                                                      long long* out_yx, float* out_score) {
  const int n = blockIdx.x % nc, b = blockIdx.x / nc;
  const long o = ((long)b * NQ + n) * nblk;
  float s = -INFINITY;
  unsigned i = 0u;
  for (int k = threadIdx.x; k < nblk; k += 64) best_take(s, i, ps[o + k], pi[o + k]);
  wave_best(s, i);
  if (threadIdx.x == 0) {
    const long r = (long)b * N + n0 + n;
    out_yx[r * 2] = (long long)(i / (unsigned)LW);
    out_yx[r * 2 + 1] = (long long)(i % (unsigned)LW);
    out_score[r] = s == -INFINITY ? NAN : s;
  }
}

int nq_of(int n) { return std::min((n + 3) / 4 * 4, (int)NN_MAXQ); }     // the instantiation of a chunk of n queries: 4, 8, .. NN_MAXQ

struct NnWs { float *q, *qi, *D, *G, *ps; unsigned* pi; size_t bytes; };
NnWs nn_carve(void* base, int B, int N, int C, int h2, int w2) {
  const size_t nq = (size_t)nq_of(N), hw = (size_t)h2 * w2;
  Carver c(base);
  NnWs ws;
  ws.q = c.take<float>((size_t)B * C * nq * 4);
  ws.qi = c.take<float>((size_t)B * nq * 4);
  ws.D = c.take<float>((size_t)B * hw * nq * 4);
  ws.G = c.take<float>((size_t)B * hw * 8 * 4);
  ws.ps = c.take<float>((size_t)B * nq * NN_FINE_BLOCKS * 4);
  ws.pi = c.take<unsigned>((size_t)B * nq * NN_FINE_BLOCKS * 4);
  ws.bytes = c.bytes();
  return ws;
}

template <typename T, int NQ>
void nn_coarse(const AggSrc& f2, bool lanes_c, int B, const NnWs& ws, hipStream_t s) {
  const int h = f2.H, w = f2.W;
  if (lanes_c) {
    const long runs = (long)B * h * ((w + NN_P - 1) / NN_P);
    hipLaunchKernelGGL((nn_coarse_c_kernel<T, NQ>), dim3((unsigned)((runs + 3) / 4)), dim3(256), 0, s, (const T*)f2.ptr, f2.sb, f2.sy, f2.sx, f2.C, h,
                       w, runs, ws.q, ws.qi, ws.D, ws.G);
  } else {
    hipLaunchKernelGGL((nn_coarse_x_kernel<T, NQ>), dim3((unsigned)((h * w + 63) / 64), (unsigned)B), dim3(1024), 0, s, (const T*)f2.ptr, f2.sb,
                       f2.sc, f2.sy, f2.sx, f2.C, h, w, ws.q, ws.qi, ws.D, ws.G);
  }
}

template <int NQ>
void nn_chunk(const AggSrc& f2, bool lanes_c, int B, int nc, int LH, int LW, int nblk, const NnWs& ws, hipStream_t s) {
  if (f2.f32) nn_coarse<float, NQ>(f2, lanes_c, B, ws, s);
  else nn_coarse<_Float16, NQ>(f2, lanes_c, B, ws, s);
  hipLaunchKernelGGL(nn_fine_kernel<NQ>, dim3((unsigned)nblk, (unsigned)B), dim3(16 * NQ), 0, s, ws.D, ws.G, f2.H, f2.W, LH, LW, nc, ws.ps, ws.pi);
}

}  // namespace

size_t nn_match_workspace(int B, int N, int C, int h2, int w2) { return nn_carve(nullptr, B, N, C, h2, w2).bytes; }

hipError_t launch_nn_match(const AggSrc& f1, const AggSrc& f2, int B, const float* points, int N, int LH, int LW, long long* out_yx,
                           float* out_score, void* workspace, hipStream_t s) {
  if (!f1.ptr || !f2.ptr || !points || !out_yx || !out_score || !workspace || ((uintptr_t)workspace & 15)) return hipErrorInvalidValue;
  if (B < 0 || B > 65535 || N < 1 || LH < 1 || LW < 1 || f1.C < 1 || f1.C != f2.C || f1.H < 1 || f1.W < 1 || f2.H < 1 || f2.W < 1)
    return hipErrorInvalidValue;
  if ((long)LH * LW >= (1l << 30) || (long)B * f2.H * f2.W >= (1l << 31)) return hipErrorInvalidValue;
  if (B == 0) return hipSuccess;
  const NnWs ws = nn_carve(workspace, B, N, f2.C, f2.H, f2.W);
  const bool lanes_c = map_lanes_c(f2);
  const int nblk = (int)std::min<long>(((long)LH * LW + 63) / 64, (long)NN_FINE_BLOCKS);
  for (int n0 = 0; n0 < N; n0 += NN_MAXQ) {
    const int nc = std::min(N - n0, (int)NN_MAXQ), NQ = nq_of(nc);
    hipLaunchKernelGGL(nn_query_kernel, dim3((unsigned)(B * NQ)), dim3(1024), 0, s, f1.ptr, f1.f32, f1.sb, f1.sc, f1.sy, f1.sx, f1.C, f1.H, f1.W,
                       points, N, n0, nc, NQ, LH, LW, ws.q, ws.qi);
    by_nq<NN_MAXQ>(NQ, [&](auto nq) { nn_chunk<decltype(nq)::value>(f2, lanes_c, B, nc, LH, LW, nblk, ws, s); });
    hipLaunchKernelGGL(nn_final_kernel, dim3((unsigned)(B * nc)), dim3(64), 0, s, ws.ps, ws.pi, nblk, NQ, nc, N, n0, LW, out_yx, out_score);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace gdf
