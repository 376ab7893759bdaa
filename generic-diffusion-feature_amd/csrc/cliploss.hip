// The correspondence evaluator's CLIP-style loss on two hyperfeature maps, forward and backward, gfx950.
//
// Reference op replaced (paths under /root/reference):
//   correspondence/task-corres.py:70-80   compute_clip_loss: scale * batch_cosine_sim of the two maps in both directions (two P x P matrices),
//   N rows of each kept, cross_entropy against the other image's indices, the mean of the two; autograd for the backward
//
// Neither similarity matrix exists here.  Direction 0 has the queries in f1 (src), the keys in f2 and the labels tgt; direction 1 the roles
// swapped.  Per direction:
//   cl_gather_kernel      one workgroup per query: its pixel's C values normalised in fp32 -> q^ (C, NQ) per chunk, 1 / ||q||, a flag
//   cl_fwd_x_kernel       lanes along the pixels (NCHW, and any other strides): per key pixel <k, q^_n> and ||k||^2 over C -> cos, 1 / ||k||
//   cl_fwd_c_kernel       lanes along C (channels-last, 16-byte loads): the same numbers
//   cl_lse_kernel         one workgroup per query: max and sum of exp over the pixels of its cos column -> log-sum-exp, the term, a flag
//   cl_loss_kernel        one workgroup per pair: the 2 N terms in order -> loss, terms, the pair's validity flag
//   cl_bwd_kernel         one workgroup = a range of key pixels x 64 channels: G rebuilt from cos and the log-sum-exp, the dense gradient of the
//                         key map written, the partial sums  sum_p G[n, p] k^_p  of its range emitted
//   cl_rowsum_kernel      one workgroup per query: sum_p G[n, p] cos[n, p]
//   cl_rows_kernel        the partials reduced in range order, the query-side correction, the N rows added into the query map's gradient: per
//                         pixel in n order, the pixels in parallel
// No atomics; every reduction has a fixed order; a workgroup sees one pair only, so a pair's bits do not depend on B or its place in the batch.
// Queries are processed in chunks of at most CL_MAXQ; everything accumulates in fp32 with plain FMAs (compiled without SLP vectorisation).
#include <math.h>

#include <algorithm>

#include "feat_common.h"

namespace gdf {

namespace {

enum { CL_P = 4, CL_TILE = 64, CL_KS = CL_TILE + 1 };

__host__ __device__ inline int cl_nq(int n) { return n >= (int)CL_MAXQ ? (int)CL_MAXQ : (n + 3) / 4 * 4; }   // the instantiation of a chunk of n queries
__host__ __device__ inline int cl_npad(int N) { return N / CL_MAXQ * CL_MAXQ + (N % CL_MAXQ ? cl_nq(N % CL_MAXQ) : 0); }
// q^ of query n, channel c inside a pair's (C * Npad) block: full chunks first, each chunk (C, NQ)
__device__ __forceinline__ long cl_qoff(int n, int c, int C, int N) {
  const int n0 = n / CL_MAXQ * CL_MAXQ;
  return (long)C * n0 + (long)c * cl_nq(N - n0) + (n - n0);
}
__device__ __forceinline__ int cl_clamp(long long i, int P) { return i < 0 ? 0 : i >= (long long)P ? P - 1 : (int)i; }

// z = scale * cos, rounded ONCE and never fused into the subtraction that follows: where a label is the maximum of its row, z - lse is then exactly 0
// and G there exactly 0, as in the reference's softmax - onehot (a fused multiply-subtract would leave the product's rounding error, ~1e-6, in G)
__device__ __forceinline__ float cl_z(float scale, float c) {
#pragma clang fp contract(off)
  return scale * c;
}

// One workgroup = one (pair b, query slot n < Npad).  idx: (B, N) flat pixel indices of this map.  An index outside the map is clamped for the read
// and flagged; so is a norm that is not positive and finite.  Slots n >= N are zero-filled.
__global__ __launch_bounds__(256) void cl_gather_kernel(const void* f, int f32, long sb, long sc, long sy, long sx, int C, int W, int P,
                                                        const long long* idx, int N, int Npad, float* q, float* qinv, int* qbad) {
  __shared__ float red[256];
  const int n = blockIdx.x, b = blockIdx.y;
  float* qb = q + (long)b * C * Npad;
  if (n >= N) {
    for (int c = threadIdx.x; c < C; c += 256) qb[cl_qoff(n, c, C, N)] = 0.f;
    if (threadIdx.x == 0) { qinv[(long)b * Npad + n] = 0.f; qbad[(long)b * Npad + n] = 0; }
    return;
  }
  const long long i = idx[(long)b * N + n];
  const int p = cl_clamp(i, P);
  const long o = (long)b * sb + (long)(p / W) * sy + (long)(p % W) * sx;
  float ss = 0.f;
  for (int c = threadIdx.x; c < C; c += 256) {
    const float v = f32 ? ld<float>(f, o + (long)c * sc) : ld<_Float16>(f, o + (long)c * sc);
    ss = fmaf(v, v, ss);
  }
  const float inv = 1.f / sqrtf(block_sum256(ss, red));
  for (int c = threadIdx.x; c < C; c += 256) {
    const float v = f32 ? ld<float>(f, o + (long)c * sc) : ld<_Float16>(f, o + (long)c * sc);
    qb[cl_qoff(n, c, C, N)] = v * inv;
  }
  if (threadIdx.x == 0) {
    qinv[(long)b * Npad + n] = inv;
    qbad[(long)b * Npad + n] = (i != (long long)p || !(inv > 0.f && inv < INFINITY)) ? 1 : 0;
  }
}

// One workgroup = 64 consecutive key pixels of one pair (flat y * W + x: lanes along x) x 16 channel slices, one wave each.  The wave's channel is
// uniform, so q^ comes through scalar loads.  The slices are summed through LDS in a fixed tree.
//   q: the chunk's (C, NQ) block of this pair's set   cos: (B, P, Npad), this chunk at column n0   kinv: (B, P)
template <typename T, int NQ>
__global__ __launch_bounds__(1024) void cl_fwd_x_kernel(const T* f, long sb, long sc, long sy, long sx, int C, int W, int P, const float* q,
                                                        long qstride, int Npad, int n0, float* cos_, float* kinv) {
  constexpr int NV = NQ + 1;
  __shared__ float red[8 * NV * 64];
  const int lane = threadIdx.x & 63, s = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = blockIdx.y;
  const int p = blockIdx.x * 64 + lane;
  const int pp = min(p, P - 1);                       // lanes past the plane compute a valid pixel and store nothing
  const T* fb = f + (long)b * sb + (long)(pp / W) * sy + (long)(pp % W) * sx;
  const int per = (C + 15) / 16, cb = s * per, ce = min(C, cb + per);
  const float* qb = q + (long)b * qstride;
  float acc[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) acc[v] = 0.f;
#pragma unroll 2
  for (int c = cb; c < ce; ++c) {
    const float t = (float)fb[(long)c * sc];
    const float* qc = qb + (long)c * NQ;
#pragma unroll
    for (int n = 0; n < NQ; ++n) acc[n] = fmaf(t, qc[n], acc[n]);
    acc[NQ] = fmaf(t, t, acc[NQ]);
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
  if (s == 0 && p < P) {
    const float inv = 1.f / sqrtf(acc[NQ]);
    float* d = cos_ + ((long)b * P + p) * Npad + n0;
#pragma unroll
    for (int n = 0; n < NQ; n += 4) *(float4*)(d + n) = make_float4(acc[n] * inv, acc[n + 1] * inv, acc[n + 2] * inv, acc[n + 3] * inv);
    kinv[(long)b * P + p] = inv;
  }
}

// Channels-last (sc == 1, C a multiple of the 16-byte vector, every pixel 16-byte aligned): one wave = CL_P consecutive pixels, lanes along C with
// 16 bytes each; the lane's V x NQ block of q^ is shared by the CL_P pixels; the per-lane sums are folded across the wave by a butterfly.
template <typename T, int NQ>
__global__ __launch_bounds__(256) void cl_fwd_c_kernel(const T* f, long sb, long sy, long sx, int C, int W, int P, const float* q, long qstride,
                                                       int Npad, int n0, float* cos_, float* kinv) {
  constexpr int V = 16 / (int)sizeof(T), NV = NQ + 1;
  typedef T vt __attribute__((ext_vector_type(V)));
  const int lane = threadIdx.x & 63, b = blockIdx.y;
  const int pa = (blockIdx.x * 4 + (int)(threadIdx.x >> 6)) * CL_P;
  if (pa >= P) return;                                // (whole waves; no barrier below)
  const T* fb = f + (long)b * sb;
  long o[CL_P];
#pragma unroll
  for (int j = 0; j < CL_P; ++j) {
    const int pj = min(pa + j, P - 1);
    o[j] = (long)(pj / W) * sy + (long)(pj % W) * sx;
  }
  const float* qb = q + (long)b * qstride;
  float acc[CL_P][NV];
#pragma unroll
  for (int j = 0; j < CL_P; ++j)
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[j][v] = 0.f;
  for (int c = lane * V; c < C; c += 64 * V) {
    vt t[CL_P];
#pragma unroll
    for (int j = 0; j < CL_P; ++j) t[j] = *(const vt*)(fb + o[j] + c);
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
      for (int j = 0; j < CL_P; ++j) {
        const float v = (float)t[j][e];
#pragma unroll
        for (int n = 0; n < NQ; ++n) acc[j][n] = fmaf(v, qv[n], acc[j][n]);
        acc[j][NQ] = fmaf(v, v, acc[j][NQ]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < CL_P; ++j)
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) acc[j][v] += __shfl_xor(acc[j][v], off);
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < CL_P; ++j) {
      if (pa + j >= P) break;
      const float inv = 1.f / sqrtf(acc[j][NQ]);
      float* d = cos_ + ((long)b * P + pa + j) * Npad + n0;
#pragma unroll
      for (int n = 0; n < NQ; n += 4)
        *(float4*)(d + n) = make_float4(acc[j][n] * inv, acc[j][n + 1] * inv, acc[j][n + 2] * inv, acc[j][n + 3] * inv);
      kinv[(long)b * P + pa + j] = inv;
    }
  }
}

// One workgroup = one (pair, query n < N) of one direction: the exact maximum of z = scale * cos over the P key pixels, then the sum of
// exp(z - max), each thread over its pixels in ascending order and the 256 threads in a fixed tree.  A key pixel whose inverse norm is not positive
// and finite, a flagged query or a label outside the key map flags the term.
__global__ __launch_bounds__(256) void cl_lse_kernel(const float* cos_, const float* kinv, const int* qbad, const long long* label, int P, int N,
                                                     int Npad, float scale, float* lse, float* term, int* bad) {
  __shared__ float red[256];
  const int n = blockIdx.x, b = blockIdx.y;
  const float* cb = cos_ + (long)b * P * Npad + n;
  const float* kb = kinv + (long)b * P;
  float m = -INFINITY, nb = 0.f;
#pragma unroll 4
  for (int p = threadIdx.x; p < P; p += 256) {
    const float ki = kb[p];
    if (!(ki > 0.f && ki < INFINITY)) nb = 1.f;
    m = fmaxf(m, cl_z(scale, cb[(long)p * Npad]));
  }
  m = block_max256(m, red);
  nb = block_max256(nb, red);
  float se = 0.f;
#pragma unroll 4
  for (int p = threadIdx.x; p < P; p += 256) se += expf(cl_z(scale, cb[(long)p * Npad]) - m);
  se = block_sum256(se, red);
  if (threadIdx.x == 0) {
    const long long l = label[(long)b * N + n];
    const int lp = cl_clamp(l, P);
    const float ls = m + logf(se);
    const long o = (long)b * Npad + n;
    lse[o] = ls;
    term[o] = ls - cl_z(scale, cb[(long)lp * Npad]);
    bad[o] = (nb != 0.f || l != (long long)lp || qbad[o]) ? 1 : 0;
  }
}

// One workgroup = one pair: any flag of either direction makes the pair invalid (loss and terms NaN); otherwise the terms are summed in n order.
__global__ __launch_bounds__(64) void cl_loss_kernel(const float* term0, const float* term1, const int* bad0, const int* bad1, int N, int Npad,
                                                     float* loss, float* terms, int* valid) {
  const int b = blockIdx.x;
  const long o = (long)b * Npad;
  int any = 0;
  for (int n = threadIdx.x; n < N; n += 64) any |= bad0[o + n] | bad1[o + n];
  any = __syncthreads_or(any);
  if (terms) {
    for (int n = threadIdx.x; n < N; n += 64) {
      terms[((long)b * 2) * N + n] = any ? NAN : term0[o + n];
      terms[((long)b * 2 + 1) * N + n] = any ? NAN : term1[o + n];
    }
  }
  if (threadIdx.x == 0) {
    float s0 = 0.f, s1 = 0.f;
    for (int n = 0; n < N; ++n) { s0 += term0[o + n]; s1 += term1[o + n]; }
    loss[b] = any ? NAN : (s0 / (float)N + s1 / (float)N) * 0.5f;
    valid[b] = any ? 0 : 1;
  }
}

// G[n, p] = coef * (exp(scale * cos[n, p] - lse_n) - [p == label_n]); coef = grad_loss * scale / (2 N), NaN for an invalid pair
__device__ __forceinline__ float cl_coef(const float* grad_loss, const int* valid, int b, float scale, int N) {
  return valid[b] ? grad_loss[b] * scale / (2.f * (float)N) : NAN;
}

// One workgroup (256 threads) = PR consecutive key pixels x 64 channels of one pair, walked in tiles of 64 pixels.  Per tile:
//   G of the tile's pixels and this chunk's queries -> LDS (the exps are shared by the four waves), S_p = sum_n G[n, p] cos[n, p];
//   k^ = k / ||k|| of the tile -> LDS, staged with lanes along the pixels or, for a channels-last map, with 16-byte loads along C;
//   phase 1, lanes along the pixels, wave w on channels 16 w .. 16 w + 15:  dk = (sum_n G[n, p] q^_n[c] - k^_p[c] S_p) / ||k_p||, written or (for
//   the second chunk on) added to grad (B, C, P) fp32;
//   phase 2, lanes along the channels, wave w on a quarter of the queries:  part[n][c] += sum_p G[n, p] k^_p[c] over the tile, p ascending.
// part: (B, R, Npad, C).  grad or part may be null.
template <typename T, int NQ>
__global__ __launch_bounds__(256) void cl_bwd_kernel(const T* f, long sb, long sc, long sy, long sx, int lanes_c, int C, int W, int P, const float* q,
                                                     long qstride, int Npad, int n0, int N, const float* cos_, const float* kinv, const float* lse,
                                                     const long long* label, float scale, const float* grad_loss, const int* valid, float* grad,
                                                     int accumulate, float* part, int PR) {
  constexpr int QW = NQ / 4, V = 16 / (int)sizeof(T);
  typedef T vt __attribute__((ext_vector_type(V)));
  __shared__ float ks[CL_TILE * CL_KS];
  __shared__ __attribute__((aligned(16))) float Gs[CL_TILE * NQ];
  __shared__ float Ss[4 * CL_TILE];
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = blockIdx.x, c0 = blockIdx.y * CL_TILE, b = blockIdx.z;
  const float coef = cl_coef(grad_loss, valid, b, scale, N);
  const T* fb = f + (long)b * sb;
  const float* qb = q + (long)b * qstride;
  const float* cb = cos_ + (long)b * P * Npad + n0;
  const float* kb = kinv + (long)b * P;
  float* gb = grad ? grad + (long)b * C * P : nullptr;
  float ls[QW];
  int lab[QW];
#pragma unroll
  for (int j = 0; j < QW; ++j) {                      // this wave's share of the exps: queries w, w + 4, ..
    const int n = n0 + w + 4 * j;
    ls[j] = n < N ? lse[(long)b * Npad + n] : 0.f;
    lab[j] = n < N ? cl_clamp(label[(long)b * N + n], P) : -1;
  }
  float pacc[QW];
#pragma unroll
  for (int j = 0; j < QW; ++j) pacc[j] = 0.f;
  const int pe = (int)min((long)P, ((long)r + 1) * PR);
  for (int pt = r * PR; pt < pe; pt += CL_TILE) {
    const int p = pt + lane;
    const bool in = p < pe;
    const float ki = in ? kb[p] : 0.f;
    {
      float sp = 0.f;
#pragma unroll
      for (int j = 0; j < QW; ++j) {
        float g = 0.f;
        if (in && lab[j] >= 0) {
          const float cv = cb[(long)p * Npad + w + 4 * j];
          g = coef * (expf(cl_z(scale, cv) - ls[j]) - (p == lab[j] ? 1.f : 0.f));
          sp = fmaf(g, cv, sp);
        }
        Gs[lane * NQ + w + 4 * j] = g;
      }
      Ss[w * CL_TILE + lane] = sp;
    }
    if (lanes_c) {
      constexpr int VP = CL_TILE / V;                 // vectors per pixel of the tile
      for (int it = threadIdx.x; it < CL_TILE * VP; it += 256) {
        const int px = it / VP, cv = (it % VP) * V;
        const int pg = pt + px;
        vt v;
#pragma unroll
        for (int e = 0; e < V; ++e) v[e] = (T)0.f;
        float kp = 0.f;
        if (pg < pe && c0 + cv < C) {
          v = *(const vt*)(fb + (long)(pg / W) * sy + (long)(pg % W) * sx + c0 + cv);
          kp = kb[pg];
        }
#pragma unroll
        for (int e = 0; e < V; ++e) ks[(cv + e) * CL_KS + px] = (float)v[e] * kp;
      }
    } else {
      const long o = in ? (long)(p / W) * sy + (long)(p % W) * sx : 0;
#pragma unroll 4
      for (int i = 0; i < 16; ++i) {
        const int c = c0 + w * 16 + i;
        ks[(w * 16 + i) * CL_KS + lane] = (in && c < C) ? (float)fb[o + (long)c * sc] * ki : 0.f;
      }
    }
    __syncthreads();
    if (gb) {
      float G[NQ];
#pragma unroll
      for (int n = 0; n < NQ; n += 4) {
        const float4 u = *(const float4*)(Gs + lane * NQ + n);
        G[n] = u.x; G[n + 1] = u.y; G[n + 2] = u.z; G[n + 3] = u.w;
      }
      const float S = ((Ss[lane] + Ss[CL_TILE + lane]) + Ss[2 * CL_TILE + lane]) + Ss[3 * CL_TILE + lane];
#pragma unroll 2
      for (int i = 0; i < 16; ++i) {
        const int c = c0 + w * 16 + i;
        if (c >= C) break;                            // (wave-uniform)
        const float* qc = qb + (long)c * NQ;
        float a = 0.f;
#pragma unroll
        for (int n = 0; n < NQ; ++n) a = fmaf(G[n], qc[n], a);
        const float dk = (a - ks[(w * 16 + i) * CL_KS + lane] * S) * ki;
        if (in) {
          float* d = gb + (long)c * P + p;
          *d = accumulate ? *d + dk : dk;
        }
      }
    }
    if (part) {
      const float* kr = ks + lane * CL_KS;
      const int npx = min(CL_TILE, pe - pt);
      for (int px = 0; px < npx; ++px) {
        const float kv = kr[px];
#pragma unroll
        for (int j = 0; j < QW; ++j) pacc[j] = fmaf(Gs[px * NQ + w * QW + j], kv, pacc[j]);
      }
    }
    __syncthreads();
  }
  if (part && c0 + lane < C) {
#pragma unroll
    for (int j = 0; j < QW; ++j)
      part[(((long)b * gridDim.x + r) * Npad + n0 + w * QW + j) * C + c0 + lane] = pacc[j];
  }
}

// One workgroup = one (pair, query n < N) of one direction: T_n = sum_p G[n, p] cos[n, p], threads strided over p, a fixed tree.
__global__ __launch_bounds__(256) void cl_rowsum_kernel(const float* cos_, const float* lse, const long long* label, int P, int N, int Npad,
                                                        float scale, const float* grad_loss, const int* valid, float* T) {
  __shared__ float red[256];
  const int n = blockIdx.x, b = blockIdx.y;
  const float coef = cl_coef(grad_loss, valid, b, scale, N);
  const float* cb = cos_ + (long)b * P * Npad + n;
  const float ls = lse[(long)b * Npad + n];
  const long long lab = label[(long)b * N + n];
  float t = 0.f;
#pragma unroll 4
  for (int p = threadIdx.x; p < P; p += 256) {
    const float cv = cb[(long)p * Npad];
    t = fmaf(coef * (expf(cl_z(scale, cv) - ls) - ((long long)p == lab ? 1.f : 0.f)), cv, t);
  }
  t = block_sum256(t, red);
  if (threadIdx.x == 0) T[(long)b * Npad + n] = t;
}

// One workgroup = 256 channels of one (pair, query n).  Rows that name the same pixel must accumulate in n order, so the workgroup of the FIRST
// query of a pixel adds every row of that pixel, m ascending, on top of the dense gradient, and the workgroups of its later duplicates do nothing:
// per pixel the same chain of additions as a loop over n, with the pixels in parallel.  Row m: the R partials summed in range order,
// dq = (sum - q^_m[c] T_m) / ||q_m||.  Nothing is added for an invalid pair (its gradient is NaN already).
__global__ __launch_bounds__(256) void cl_rows_kernel(const float* part, int R, const float* q, const float* qinv, const float* T,
                                                      const long long* idx, const int* valid, int C, int P, int N, int Npad, float* grad) {
  const int n = blockIdx.x, c = blockIdx.y * 256 + threadIdx.x, b = blockIdx.z;
  if (!valid[b]) return;
  const long long* ib = idx + (long)b * N;
  const long long pix = ib[n];
  for (int m = 0; m < n; ++m)
    if (ib[m] == pix) return;                         // (uniform: a later duplicate)
  if (c >= C) return;
  const float* qb = q + (long)b * C * Npad;
  float* g = grad + ((long)b * C + c) * P + pix;
  float v = *g;
  for (int m = n; m < N; ++m) {
    if (ib[m] != pix) continue;
    float s = 0.f;
    for (int r = 0; r < R; ++r) s += part[(((long)b * R + r) * Npad + m) * C + c];
    v += (s - qb[cl_qoff(m, c, C, N)] * T[(long)b * Npad + m]) * qinv[(long)b * Npad + m];
  }
  *g = v;
}

// pixels per backward workgroup: at most CL_RANGES ranges per map, whole tiles
int cl_pr(int P) { return (int)std::max<long>(CL_TILE, (((long)P + CL_RANGES - 1) / CL_RANGES + CL_TILE - 1) / CL_TILE * CL_TILE); }

// direction d: queries in map d, keys in map 1 - d (P[1 - d] pixels)
struct ClDir { float *q, *qinv, *cos_, *kinv, *lse, *term, *T, *part; int *qbad, *bad; };
struct ClWs { ClDir d[2]; int* valid; size_t bytes; };
ClWs cl_carve(void* base, int B, int N, int C, int P1, int P2) {
  const size_t npad = (size_t)cl_npad(N);
  const int P[2] = {P1, P2};
  Carver c(base);
  ClWs ws;
  for (int d = 0; d < 2; ++d) {
    const size_t pk = (size_t)P[1 - d], R = (size_t)((pk + cl_pr((int)pk) - 1) / cl_pr((int)pk));
    ClDir& e = ws.d[d];
    e.q = c.take<float>((size_t)B * C * npad * 4);
    e.qinv = c.take<float>((size_t)B * npad * 4);
    e.qbad = c.take<int>((size_t)B * npad * 4);
    e.cos_ = c.take<float>((size_t)B * pk * npad * 4);
    e.kinv = c.take<float>((size_t)B * pk * 4);
    e.lse = c.take<float>((size_t)B * npad * 4);
    e.term = c.take<float>((size_t)B * npad * 4);
    e.bad = c.take<int>((size_t)B * npad * 4);
    e.T = c.take<float>((size_t)B * npad * 4);
    e.part = c.take<float>((size_t)B * R * npad * C * 4);
  }
  ws.valid = c.take<int>((size_t)B * 4);
  ws.bytes = c.bytes();
  return ws;
}

template <typename T, int NQ>
void cl_fwd(const AggSrc& k, int B, int P, const float* q, long qstride, int Npad, int n0, float* cos_, float* kinv, hipStream_t s) {
  if (map_lanes_c(k)) {
    hipLaunchKernelGGL((cl_fwd_c_kernel<T, NQ>), dim3((unsigned)((P + 4 * CL_P - 1) / (4 * CL_P)), (unsigned)B), dim3(256), 0, s, (const T*)k.ptr,
                       k.sb, k.sy, k.sx, k.C, k.W, P, q, qstride, Npad, n0, cos_, kinv);
  } else {
    hipLaunchKernelGGL((cl_fwd_x_kernel<T, NQ>), dim3((unsigned)((P + 63) / 64), (unsigned)B), dim3(1024), 0, s, (const T*)k.ptr, k.sb, k.sc, k.sy,
                       k.sx, k.C, k.W, P, q, qstride, Npad, n0, cos_, kinv);
  }
}

struct ClBwd { const float *cos_, *kinv, *lse, *grad_loss; const long long* label; const int* valid; float *grad, *part; float scale; int N, Npad; };

template <typename T, int NQ>
void cl_bwd(const AggSrc& k, int B, int P, const float* q, long qstride, int n0, const ClBwd& a, hipStream_t s) {
  const int PR = cl_pr(P), R = (P + PR - 1) / PR;
  hipLaunchKernelGGL((cl_bwd_kernel<T, NQ>), dim3((unsigned)R, (unsigned)((k.C + CL_TILE - 1) / CL_TILE), (unsigned)B), dim3(256), 0, s,
                     (const T*)k.ptr, k.sb, k.sc, k.sy, k.sx, map_lanes_c(k) ? 1 : 0, k.C, k.W, P, q, qstride, a.Npad, n0, a.N, a.cos_, a.kinv, a.lse,
                     a.label, a.scale, a.grad_loss, a.valid, a.grad, n0 > 0 ? 1 : 0, a.part, PR);
}

bool cl_args_ok(const AggSrc& f1, const AggSrc& f2, int B, int N, const void* workspace) {
  if (!f1.ptr || !f2.ptr || !workspace || ((uintptr_t)workspace & 15)) return false;
  if (B < 0 || B > 65535 || N < 1 || f1.C < 1 || f1.C != f2.C || f1.H < 1 || f1.W < 1 || f2.H < 1 || f2.W < 1) return false;
  return (long)f1.H * f1.W < (1l << 30) && (long)f2.H * f2.W < (1l << 30);
}

}  // namespace

size_t clip_loss_workspace(int B, int N, int C, int P1, int P2) { return cl_carve(nullptr, B, N, C, P1, P2).bytes; }

hipError_t launch_clip_loss(const AggSrc& f1, const AggSrc& f2, int B, const long long* src_idx, const long long* tgt_idx, int N, float scale,
                            float* loss, float* terms, void* workspace, hipStream_t s) {
  if (!cl_args_ok(f1, f2, B, N, workspace) || !src_idx || !tgt_idx || !loss || !(scale > 0.f && scale < INFINITY)) return hipErrorInvalidValue;
  if (B == 0) return hipSuccess;
  const AggSrc* maps[2] = {&f1, &f2};
  const long long* idx[2] = {src_idx, tgt_idx};
  const int C = f1.C, Npad = cl_npad(N), P[2] = {f1.H * f1.W, f2.H * f2.W};
  const ClWs ws = cl_carve(workspace, B, N, C, P[0], P[1]);
  for (int d = 0; d < 2; ++d) {
    const AggSrc& qm = *maps[d];
    const AggSrc& k = *maps[1 - d];
    const ClDir& e = ws.d[d];
    const int Pk = P[1 - d];
    hipLaunchKernelGGL(cl_gather_kernel, dim3((unsigned)Npad, (unsigned)B), dim3(256), 0, s, qm.ptr, qm.f32, qm.sb, qm.sc, qm.sy, qm.sx, C, qm.W,
                       P[d], idx[d], N, Npad, e.q, e.qinv, e.qbad);
    for (int n0 = 0; n0 < N; n0 += CL_MAXQ) {
      by_nq<CL_MAXQ>(cl_nq(N - n0), [&](auto nq) {
        constexpr int NQ = decltype(nq)::value;
        if (k.f32) cl_fwd<float, NQ>(k, B, Pk, e.q + (long)C * n0, (long)C * Npad, Npad, n0, e.cos_, e.kinv, s);
        else cl_fwd<_Float16, NQ>(k, B, Pk, e.q + (long)C * n0, (long)C * Npad, Npad, n0, e.cos_, e.kinv, s);
      });
    }
    hipLaunchKernelGGL(cl_lse_kernel, dim3((unsigned)N, (unsigned)B), dim3(256), 0, s, e.cos_, e.kinv, e.qbad, idx[1 - d], Pk, N, Npad, scale, e.lse,
                       e.term, e.bad);
  }
  hipLaunchKernelGGL(cl_loss_kernel, dim3((unsigned)B), dim3(64), 0, s, ws.d[0].term, ws.d[1].term, ws.d[0].bad, ws.d[1].bad, N, Npad, loss, terms,
                     ws.valid);
  return hipGetLastError();
}

hipError_t launch_clip_loss_backward(const AggSrc& f1, const AggSrc& f2, int B, const long long* src_idx, const long long* tgt_idx, int N,
                                     float scale, const float* grad_loss, float* grad_f1, float* grad_f2, void* workspace, hipStream_t s) {
  if (!cl_args_ok(f1, f2, B, N, workspace) || !src_idx || !tgt_idx || !grad_loss || !(scale > 0.f && scale < INFINITY)) return hipErrorInvalidValue;
  if (B == 0) return hipSuccess;
  const AggSrc* maps[2] = {&f1, &f2};
  const long long* idx[2] = {src_idx, tgt_idx};
  float* grads[2] = {grad_f1, grad_f2};
  const int C = f1.C, Npad = cl_npad(N), P[2] = {f1.H * f1.W, f2.H * f2.W};
  const ClWs ws = cl_carve(workspace, B, N, C, P[0], P[1]);
  // the dense passes first: direction d writes every element of the key map's gradient (map 1 - d) and the partials of the query map's rows
  for (int d = 0; d < 2; ++d) {
    const AggSrc& k = *maps[1 - d];
    const ClDir& e = ws.d[d];
    const int Pk = P[1 - d];
    if (!grads[1 - d] && !grads[d]) continue;
    const ClBwd a{e.cos_, e.kinv, e.lse, grad_loss, idx[1 - d], ws.valid, grads[1 - d], grads[d] ? e.part : nullptr, scale, N, Npad};
    for (int n0 = 0; n0 < N; n0 += CL_MAXQ) {
      by_nq<CL_MAXQ>(cl_nq(N - n0), [&](auto nq) {
        constexpr int NQ = decltype(nq)::value;
        if (k.f32) cl_bwd<float, NQ>(k, B, Pk, e.q + (long)C * n0, (long)C * Npad, n0, a, s);
        else cl_bwd<_Float16, NQ>(k, B, Pk, e.q + (long)C * n0, (long)C * Npad, n0, a, s);
      });
    }
  }
  // then the N rows of each query map, in n order, on top of its dense gradient
  for (int d = 0; d < 2; ++d) {
    if (!grads[d]) continue;
    const ClDir& e = ws.d[d];
    const int Pk = P[1 - d], PR = cl_pr(Pk), R = (Pk + PR - 1) / PR;
    hipLaunchKernelGGL(cl_rowsum_kernel, dim3((unsigned)N, (unsigned)B), dim3(256), 0, s, e.cos_, e.lse, idx[1 - d], Pk, N, Npad, scale, grad_loss,
                       ws.valid, e.T);
    hipLaunchKernelGGL(cl_rows_kernel, dim3((unsigned)N, (unsigned)((C + 255) / 256), (unsigned)B), dim3(256), 0, s, e.part, R, e.q, e.qinv, e.T, idx[d],
                       ws.valid, C, P[d], N, Npad, grads[d]);
  }
  return hipGetLastError();
}

}  // namespace gdf
