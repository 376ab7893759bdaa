// Post-processing kernels of the output stages that sit right after the hot path, gfx950.
// All of them are HBM-bound byte movers over hook tensors: 16-byte lanes where the layout allows, LDS only to turn the
// channels-last hook layout into the NCHW rows the consumers store.
//
// Reference ops replaced (paths under /root/reference):
//   extract_feature.py:113-125   `--aggregate_output`: F.interpolate(v, max_hw) (nearest) of every layer + torch.cat(dim=1)
//                                                                                                   -> resize_concat_kernel
//   feature/components/feature_extractor.py:51-53   `feature_resize`: F.adaptive_avg_pool2d(feat, (H/r, W/r))
//                                                                                                   -> avg_pool_kernel
//   feature/components/attention.py:238-244, 141-161 + feature/diffusion_feature.py:492-500   aggregated `attn` feature:
//   head mean, mean over the layers of one (category, size) group ('b (h w) c -> b c h w'), nearest resize to img/8, concat
//                                                                            -> maps_mean_kernel + resize_concat_kernel
//   correspondence/correspondence/aggregation_network.py:62-66, 79-83 + scarce_segmentation/task-pixel.py:50-55, 90-95   the evaluators' first
//   step on a feature dict: F.interpolate(v, (128, 128), mode='bilinear') of every layer + torch.cat(dim=1)  -> aggregate_kernel
#include <algorithm>

#include "feat_common.h"

namespace gdf {

// PyTorch `nearest`: src = min(floor(dst * (in / out)), in - 1) with the scale held in fp32
__device__ __forceinline__ int nearest_src(int dst, float scale, int in) {
  const int s = (int)floorf((float)dst * scale);
  return s < in - 1 ? s : in - 1;
}

// One workgroup = one (sample b, output row y, 64-channel chunk of one source layer).  The source row is read once,
// channel-fastest (128 B per pixel when sc == 1: the hook layout), transposed through LDS, and written x-fastest.
//   src: logical (B, C, H, W) with element strides (sb, sc, sy, sx), fp16 or fp32;  out: (B, Ctot, S, S) fp16 contiguous,
//   this layer occupying channels [coff, coff + C)
__global__ __launch_bounds__(256) void resize_concat_kernel(const half_t* s16, const float* s32, long sb, long sc, long sy, long sx,
                                                            int C, int H, int W, half_t* out, int Ctot, int coff, int S) {
  __shared__ _Float16 tile[128 * 66];                 // [xs][64 ch + 2 pad]: conflict-free x-fastest reads
  const int y = blockIdx.x % S, b = blockIdx.x / S;
  const int c0 = blockIdx.y * 64;
  const int nc = min(64, C - c0);
  const float fy = (float)H / (float)S, fx = (float)W / (float)S;
  const int ys = nearest_src(y, fy, H);
  for (int x0 = 0; x0 < W; x0 += 128) {               // source rows wider than 128 pixels: in slabs
    const int nw = min(128, W - x0);
    for (int i = threadIdx.x; i < nw * 64; i += 256) {
      const int xs = i >> 6, c = i & 63;
      float v = 0.f;
      if (c < nc) {
        const long o = (long)b * sb + (long)(c0 + c) * sc + (long)ys * sy + (long)(x0 + xs) * sx;
        v = s32 ? s32[o] : (float)s16[o];
      }
      tile[xs * 66 + c] = (_Float16)v;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nc * S; i += 256) {
      const int c = i / S, x = i - c * S;
      const int xs = nearest_src(x, fx, W) - x0;
      if (xs >= 0 && xs < nw) out[(((size_t)b * Ctot + coff + c0 + c) * S + y) * S + x] = tile[xs * 66 + c];
    }
    __syncthreads();
  }
}

hipError_t launch_resize_concat(const half_t* s16, const float* s32, long sb, long sc, long sy, long sx, int B, int C, int H, int W,
                                half_t* out, int Ctot, int coff, int S, hipStream_t s) {
  if (B <= 0 || C <= 0 || S <= 0) return hipSuccess;
  if (H <= 0 || W <= 0 || coff < 0 || coff + C > Ctot) return hipErrorInvalidValue;
  hipLaunchKernelGGL(resize_concat_kernel, dim3((unsigned)(B * S), (unsigned)((C + 63) / 64)), dim3(256), 0, s, s16, s32, sb, sc, sy, sx, C,
                     H, W, out, Ctot, coff, S);
  return hipGetLastError();
}

// ---- bilinear aggregation: F.interpolate(v, (OH, OW), mode='bilinear') of up to AGG_MAX layers + torch.cat(dim=1), one launch ----

// LDS tile [source pixel][64 ch + 1 pad] fp32 (x-fastest reads hit distinct banks) of `slab` <= AGG_SLAB pixels: the launch's widest source row,
// so that the narrow rows of the usual hooks leave room for more workgroups per CU
enum { AGG_SLAB = 128, AGG_LD = 65 };

// one source of the launch; `end` = running total of workgroups up to and including this source
struct AggItem { const void* ptr; long sb, sc, sy, sx; int C, H, W, coff, f32, vec; unsigned end; };
struct AggTable { AggItem it[AGG_MAX]; };

// Stage nw pixels x nc <= 64 channels of the two source rows r0 / r1 (each pointing at its (b, c0, y, x0) element), blended vertically in fp32,
// into tile[pixel][channel].  vec: sc == 1 and every pixel 16-byte aligned -> 16 bytes per lane, channel-fastest (the hook layout).
template <typename T, int V>
__device__ __forceinline__ void agg_stage(const T* r0, const T* r1, float l0, float l1, long sc, long sx, bool vec, int nw, int nc, float* tile) {
  typedef T vt __attribute__((ext_vector_type(V)));
  if (vec) {
    constexpr int G = 64 / V;
    for (int i = threadIdx.x; i < nw * G; i += 256) {
      const int xs = i / G, c = (i % G) * V;
      float* t = tile + xs * AGG_LD + c;
      const long o = (long)xs * sx + c;
      if (c + V <= nc) {
        const vt a = *(const vt*)(r0 + o);
        if (l1 != 0.f) {
          const vt b = *(const vt*)(r1 + o);
#pragma unroll
          for (int j = 0; j < V; ++j) t[j] = l0 * (float)a[j] + l1 * (float)b[j];
        } else {
#pragma unroll
          for (int j = 0; j < V; ++j) t[j] = (float)a[j];
        }
      } else {                                         // the partial group at the end of C: element by element, nothing past C is read
        for (int j = 0; c + j < nc; ++j) t[j] = l1 != 0.f ? l0 * (float)r0[o + j] + l1 * (float)r1[o + j] : (float)r0[o + j];
      }
    }
  } else {
    const bool xfast = sx < sc;                        // NCHW: consecutive lanes walk x
    for (int i = threadIdx.x; i < nw * nc; i += 256) {
      const int c = xfast ? i / nw : i % nc, xs = xfast ? i - c * nw : i / nc;
      const long o = (long)c * sc + (long)xs * sx;
      tile[xs * AGG_LD + c] = l1 != 0.f ? l0 * (float)r0[o] + l1 * (float)r1[o] : (float)r0[o];
    }
  }
}

// One workgroup = one (source, sample b, output row y, 64-channel chunk).  The two source rows of y are read once, blended in fp32 into LDS
// (slabs of `slab` pixels that overlap by one, so both horizontal taps of an output lie in the slab that owns it), then every thread blends
// V = 16 / sizeof(OT) consecutive outputs of one channel row and stores them as one 16-byte vector where the row start allows.
template <typename OT>
__global__ __launch_bounds__(256) void aggregate_kernel(AggTable t, OT* out, int Ctot, int OH, int OW, int slab) {
  constexpr int V = 16 / (int)sizeof(OT);
  typedef OT ovt __attribute__((ext_vector_type(V)));
  extern __shared__ float tile[];                     // slab * AGG_LD floats
  int k = 0;
  unsigned beg = 0;
  while (blockIdx.x >= t.it[k].end) beg = t.it[k++].end;    // (the grid == the last end: k stays inside the table)
  const AggItem& e = t.it[k];
  unsigned r = blockIdx.x - beg;
  const int y = (int)(r % (unsigned)OH);
  r /= (unsigned)OH;
  const int nch = (e.C + 63) / 64;
  const int c0 = (int)(r % (unsigned)nch) * 64, b = (int)(r / (unsigned)nch);
  const int nc = min(64, e.C - c0), W = e.W;
  const float fy = (float)e.H / (float)OH, fx = (float)W / (float)OW;
  int ys0, ys1;
  float ly1;
  bilinear_src(y, fy, e.H, ys0, ys1, ly1);
  const float ly0 = 1.f - ly1;
  const long base = (long)b * e.sb + (long)c0 * e.sc;

  // threads: gx lanes along x (a power of two covering the row's vectors, at most 64), 256 / gx channel rows per pass
  const int NG = (OW + V - 1) / V;
  int gsh = 0;
  while ((1 << gsh) < NG && gsh < 6) ++gsh;
  const int tx = threadIdx.x & ((1 << gsh) - 1), ty = threadIdx.x >> gsh, ry = 256 >> gsh;

  for (int x0 = 0;; x0 += slab - 1) {
    const bool last = x0 + slab >= W;
    const int nw = min(slab, W - x0);
    const long o0 = base + (long)ys0 * e.sy + (long)x0 * e.sx, o1 = base + (long)ys1 * e.sy + (long)x0 * e.sx;
    if (e.f32) agg_stage<float, 4>((const float*)e.ptr + o0, (const float*)e.ptr + o1, ly0, ly1, e.sc, e.sx, e.vec, nw, nc, tile);
    else agg_stage<_Float16, 8>((const _Float16*)e.ptr + o0, (const _Float16*)e.ptr + o1, ly0, ly1, e.sc, e.sx, e.vec, nw, nc, tile);
    __syncthreads();
    for (int xg = tx; xg < NG; xg += 1 << gsh) {
      const int x = xg * V;
      int a0[V], a1[V];
      float w1[V];
      unsigned own = 0;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        int i0, i1;
        bilinear_src(min(x + j, OW - 1), fx, W, i0, i1, w1[j]);
        const bool mine = x + j < OW && i0 >= x0 && (last || i0 < x0 + slab - 1);   // then x0 <= i0 <= i1 < x0 + nw
        own |= mine ? 1u << j : 0u;
        a0[j] = mine ? (i0 - x0) * AGG_LD : 0;
        a1[j] = mine ? (i1 - x0) * AGG_LD : 0;
      }
      if (!own) continue;
      for (int c = ty; c < nc; c += ry) {
        OT* row = out + (((size_t)b * Ctot + e.coff + c0 + c) * OH + y) * OW + x;
        ovt v;
#pragma unroll
        for (int j = 0; j < V; ++j) {                 // (a zero weight takes the other tap as it is: the identity resize keeps -0.0)
          const float t0 = tile[a0[j] + c], t1 = tile[a1[j] + c];
          v[j] = (OT)(w1[j] != 0.f ? (1.f - w1[j]) * t0 + w1[j] * t1 : t0);
        }
        if (own == (1u << V) - 1u && ((uintptr_t)row & 15) == 0) {
          *(ovt*)row = v;
        } else {                                       // odd OW, a coff that misaligns the row, the vector cut by a slab: element by element
#pragma unroll
          for (int j = 0; j < V; ++j)
            if (own >> j & 1) row[j] = v[j];
        }
      }
    }
    if (last) break;
    __syncthreads();
  }
}

hipError_t launch_aggregate(const AggSrc* srcs, int n, int B, void* out, int out_f32, int Ctot, int OH, int OW, hipStream_t s) {
  if (n < 1 || n > AGG_MAX || !srcs || !out || OH < 1 || OW < 1 || B < 0) return hipErrorInvalidValue;
  AggTable t{};
  size_t total = 0;
  int slab = 2;                                       // (two pixels at least: a slab advances by slab - 1)
  for (int k = 0; k < n; ++k) {
    const AggSrc& e = srcs[k];
    if (!e.ptr || e.C < 1 || e.H < 1 || e.W < 1 || e.coff < 0 || (long)e.coff + e.C > Ctot) return hipErrorInvalidValue;
    total += (size_t)B * OH * ((e.C + 63) / 64);
    if (total >= (1ull << 31)) return hipErrorInvalidValue;
    slab = std::max(slab, std::min(e.W, (int)AGG_SLAB));
    const int vec = map_pixels_aligned(e);            // (not map_lanes_c: agg_stage takes the partial group at the end of C element by element)
    t.it[k] = AggItem{e.ptr, e.sb, e.sc, e.sy, e.sx, e.C, e.H, e.W, e.coff, e.f32 ? 1 : 0, vec, (unsigned)total};
  }
  if (total == 0) return hipSuccess;
  for (int k = n; k < AGG_MAX; ++k) t.it[k].end = (unsigned)total;
  const unsigned lds = (unsigned)(slab * AGG_LD * sizeof(float));
  if (out_f32) hipLaunchKernelGGL(aggregate_kernel<float>, dim3((unsigned)total), dim3(256), lds, s, t, (float*)out, Ctot, OH, OW, slab);
  else hipLaunchKernelGGL(aggregate_kernel<_Float16>, dim3((unsigned)total), dim3(256), lds, s, t, (_Float16*)out, Ctot, OH, OW, slab);
  return hipGetLastError();
}

// `feature_resize`: F.adaptive_avg_pool2d to (OH, OW) = (H / r, W / r) of a channels-last hook: src (B, C, H, W) fp16 with strides
// (sb, 1, sy, sx) -> out (B, OH, OW, C) fp16 (returned to the caller as the (B, C, OH, OW) channels-last view, like every hook); fp32
// accumulation, 16 B per lane.  ATen's windows: output row o averages source rows [floor(o H / OH), ceil((o + 1) H / OH)) — exactly
// r rows where r divides H, otherwise longer windows that may overlap and together cover every row; columns likewise.
__global__ __launch_bounds__(256) void avg_pool_kernel(const half_t* src, long sb, long sy, long sx, int C, int H, int W, int OH, int OW,
                                                       half_t* out, long total) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;      // (b, oy, ox, c8)
  if (i >= total) return;
  const int C8 = C / 8;
  const int c = (int)(i % C8) * 8;
  const int ox = (int)((i / C8) % OW), oy = (int)((i / ((long)C8 * OW)) % OH);
  const long b = i / ((long)C8 * OW * OH);
  const int y0 = (int)((long)oy * H / OH), y1 = (int)((((long)oy + 1) * H + OH - 1) / OH);     // y1 <= H, x1 <= W
  const int x0 = (int)((long)ox * W / OW), x1 = (int)((((long)ox + 1) * W + OW - 1) / OW);
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int y = y0; y < y1; ++y)
    for (int x = x0; x < x1; ++x) {
      const f16x8 v = *(const f16x8*)(src + b * sb + (long)y * sy + (long)x * sx + c);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += (float)v[e];
    }
  const float inv = 1.0f / (float)((y1 - y0) * (x1 - x0));
  f16x8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = (_Float16)(acc[e] * inv);
  *(f16x8*)(out + (((size_t)b * OH + oy) * OW + ox) * C + c) = o;
}

hipError_t launch_avg_pool(const half_t* src, long sb, long sy, long sx, int B, int C, int H, int W, int r, half_t* out, hipStream_t s) {
  if (r < 1 || (C & 7) || (sb & 7) || (sy & 7) || (sx & 7) || H < r || W < r) return hipErrorInvalidValue;
  const int OH = H / r, OW = W / r;
  const long total = (long)B * OH * OW * (C / 8);
  if (total <= 0) return hipSuccess;
  hipLaunchKernelGGL(avg_pool_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, src, sb, sy, sx, C, H, W, OH, OW, out, total);
  return hipGetLastError();
}

// mean over heads and over `n` <= 32 maps of one (category, size) group: maps[l] (B, heads, Q, K) fp16 contiguous ->
// out (B, Q, K) fp32 (= the channels-last image of the (B, K, sqrt Q, sqrt Q) tensor resize_concat_kernel then consumes)
struct MapPtrs { const half_t* p[32]; };
__global__ __launch_bounds__(256) void maps_mean_kernel(MapPtrs m, int n, int heads, long QK, float* out, long total) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;      // (b, q*K + k)
  if (i >= total) return;
  const long b = i / QK, r = i - b * QK;
  float acc = 0.f;
  for (int l = 0; l < n; ++l) {
    const half_t* p = m.p[l] + (size_t)b * heads * QK + r;
    float a = 0.f;
    for (int h = 0; h < heads; ++h) a += (float)p[(size_t)h * QK];
    // the reference rounds the head mean to fp16 (`attention_probs.mean(1)` on an fp16 tensor) before averaging the layers
    acc += (float)(_Float16)(a / (float)heads);
  }
  out[i] = acc / (float)n;
}

hipError_t launch_maps_mean(const half_t* const* maps, int n, int B, int heads, int Q, int K, float* out, hipStream_t s) {
  if (n < 1 || n > 32 || heads < 1) return hipErrorInvalidValue;
  MapPtrs m{};
  for (int l = 0; l < n; ++l) m.p[l] = maps[l];
  const long QK = (long)Q * K, total = (long)B * QK;
  if (total <= 0) return hipSuccess;
  hipLaunchKernelGGL(maps_mean_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, m, n, heads, QK, out, total);
  return hipGetLastError();
}

}  // namespace gdf
