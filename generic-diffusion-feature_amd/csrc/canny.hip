// Canny edge detector on the device (gfx950): the preprocessor in front of the 'canny' / 'canny-xl' ControlNets.
//
// Reference op replaced: cv2.Canny(np.array(image), 100, 200) of feature/components/controlnet.py:30-36, restated from the published algorithm of
// OpenCV 4.x cv::Canny(src8u, low, high, apertureSize = 3, L2gradient = false): integer 3x3 Sobel per channel on a REPLICATED pixel
// border, mag = |dx| + |dy|, per pixel the channel of the largest mag (the first one on a tie), non-maximum suppression along the quantised gradient
// direction against a magnitude map whose border is ZERO, two thresholds, and hysteresis: a kept pixel above `high` is an edge, a kept pixel in
// (low, high] is an edge iff it is 8-connected through kept pixels to one above `high`.  That set is unique, so a parallel labelling is exact.
//
// Five launches, whatever the image holds (no device -> host read anywhere):
//   canny_classify_kernel   image -> class map uint8 [B][H][W]: 2 strong, 0 candidate, 1 neither (OpenCV's map values)
//   canny_label_tile_kernel class map -> parent[i] = index of the smallest pixel of i's component INSIDE its 32 x 32 tile (-1 for class 1), flag[i] = 0
//   canny_seam_kernel       unions across tile seams (agent-scope atomics on parent only; nobody waits for anybody)
//   canny_flag_kernel       every strong pixel marks its root
//   canny_emit_kernel       every candidate looks its root's mark up; writes uint8 0 / 255 or fp16 (B, 3, H, W) 0.0 / 1.0
// Pixel indices are global over the batch, i = b H W + y W + x < 2^31; neighbours never leave their image.
// parent[i] <= i holds from the label kernel on (a tile's row-major order agrees with the global order, and every union hangs the LARGER root
// under the smaller index), so every walk towards a root strictly decreases and ends.
#include <algorithm>

#include "kernels.h"

namespace gdf {

namespace {

enum { CL_TW = 64, CL_TH = 16, CL_PW = CL_TW + 4, CL_PH = CL_TH + 4, CL_PS = 72, CL_MW = CL_TW + 2, CL_MH = CL_TH + 2, CL_MS = 68, CL_RAW = 56 };
enum { LT = CANNY_LINK_TILE, LP = LT + 2 };

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// restore_from_tensor_to_image's quantisation of a [-1, 1] value: rint(clamp(x / 2 + 0.5, 0, 1) * 255), every step rounded to fp32, half to even
__device__ __forceinline__ uint8_t quantise(float x) {
  float v = __fadd_rn(__fmul_rn(x, 0.5f), 0.5f);
  v = fminf(fmaxf(v, 0.0f), 1.0f);
  return (uint8_t)(int)rintf(__fmul_rn(v, 255.0f));
}

}  // namespace

// One workgroup: a CL_TH x CL_TW pixel tile.  LDS: the bytes of tile + 2 (planar per channel), then (mag, dx, dy) of tile + 1, then NMS.
// Pixels outside the image are read through clamped coordinates (rows when they are loaded, columns when they are read); magnitudes outside the
// image are zero.
template <int SRC>   // GDF_CANNY_U8_HWC3, _U8_HW, _F32_NCHW, _F16_NCHW
__global__ __launch_bounds__(256) void canny_classify_kernel(const void* __restrict__ src, int B, int H, int W, int tiles_x, int tiles_y, int low,
                                                             int high, uint8_t* __restrict__ cls) {
  constexpr int NCH = SRC == 1 ? 1 : 3;
  __shared__ __attribute__((aligned(16))) uint8_t P[NCH][CL_PH][CL_PS];
  __shared__ __attribute__((aligned(16))) short M[CL_MH][CL_MS], DX[CL_MH][CL_MS], DY[CL_MH][CL_MS];
  const int tid = threadIdx.x;
  int blk = blockIdx.x;
  const int tx = blk % tiles_x; blk /= tiles_x;
  const int ty = blk % tiles_y;
  const int b = blk / tiles_y;
  const int x0 = tx * CL_TW, y0 = ty * CL_TH;
  const int xs = max(x0 - 2, 0), xe = min(x0 + CL_TW + 2, W);          // the columns of the image this tile reads: [xs, xe), never empty

  if constexpr (SRC <= 1) {
    // a row's bytes [xs * NCH, xe * NCH) are contiguous: aligned 4-byte loads over them, the bytes scattered to their channel planes
    const uint8_t* s8 = (const uint8_t*)src;
    const size_t total = (size_t)B * H * W * NCH;                    // bytes of the whole batch: nothing is read past them
    for (int it = tid; it < CL_PH * CL_RAW; it += 256) {
      const int r = it / CL_RAW, j = it - r * CL_RAW;
      const int yc = clampi(y0 - 2 + r, 0, H - 1);
      const size_t rb = ((size_t)b * H + yc) * W * NCH;
      const size_t lo_b = rb + (size_t)xs * NCH, hi_b = rb + (size_t)xe * NCH;
      const size_t a = (lo_b & ~(size_t)3) + 4 * (size_t)j;
      if (a >= hi_b) continue;
      uint32_t v = 0;
      if (a + 4 <= total) v = *(const uint32_t*)(s8 + a);
      else for (int k = 0; k < 4; ++k) if (a + k < total) v |= (uint32_t)s8[a + k] << (8 * k);
      for (int k = 0; k < 4; ++k) {
        const size_t o = a + k;
        if (o < lo_b || o >= hi_b) continue;
        const int rel = (int)(o - lo_b);                               // < CL_PW * NCH
        const int px = rel / NCH, ch = rel - px * NCH;
        P[ch][r][xs - (x0 - 2) + px] = (uint8_t)(v >> (8 * k));
      }
    }
  } else {
    for (int it = tid; it < NCH * CL_PH * CL_PW; it += 256) {
      const int c = it / (CL_PH * CL_PW), rem = it - c * (CL_PH * CL_PW);
      const int r = rem / CL_PW, j = rem - r * CL_PW;
      const int x = x0 - 2 + j;
      if (x < xs || x >= xe) continue;
      const int yc = clampi(y0 - 2 + r, 0, H - 1);
      const size_t idx = (((size_t)b * NCH + c) * H + yc) * W + x;
      float v;
      if constexpr (SRC == 2) v = ((const float*)src)[idx];
      else v = (float)((const _Float16*)src)[idx];
      P[c][r][j] = quantise(v);
    }
  }
  __syncthreads();

  // (mag, dx, dy) of tile + 1; position (i, j) is pixel (y0 - 1 + i, x0 - 1 + j), its 3 x 3 window rows i .. i + 2 of P
  for (int it = tid; it < CL_MH * CL_MW; it += 256) {
    const int i = it / CL_MW, j = it - i * CL_MW;
    const int gy = y0 - 1 + i, gx = x0 - 1 + j;
    int m = 0, dxs = 0, dys = 0;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
      const int xm = clampi(gx - 1, 0, W - 1) - (x0 - 2), xc = gx - (x0 - 2), xp = clampi(gx + 1, 0, W - 1) - (x0 - 2);
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int a0 = P[c][i][xm], a1 = P[c][i][xc], a2 = P[c][i][xp];
        const int b0 = P[c][i + 1][xm], b2 = P[c][i + 1][xp];
        const int c0 = P[c][i + 2][xm], c1 = P[c][i + 2][xc], c2 = P[c][i + 2][xp];
        const int dx = (a2 + 2 * b2 + c2) - (a0 + 2 * b0 + c0);
        const int dy = (c0 + 2 * c1 + c2) - (a0 + 2 * a1 + a2);
        const int mg = abs(dx) + abs(dy);
        if (c == 0 || mg > m) { m = mg; dxs = dx; dys = dy; }          // strict >: the first channel wins a tie
      }
    }
    M[i][j] = (short)m; DX[i][j] = (short)dxs; DY[i][j] = (short)dys;
  }
  __syncthreads();

  // non-maximum suppression and the two thresholds: 4 consecutive pixels of one row per thread
  const int ly = tid >> 4, lx = (tid & 15) * 4;
  const int y = y0 + ly;
  if (y >= H) return;
  uint32_t packed = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = ly + 1, j = lx + k + 1;
    const int m = M[i][j];
    int c = 1;
    if (m > low) {
      const int dx = DX[i][j], dy = DY[i][j];
      const int ax = abs(dx), ay = abs(dy) << 15;
      const int tg22 = ax * 13573, tg67 = tg22 + (ax << 16);
      bool keep;
      if (ay < tg22) keep = m > M[i][j - 1] && m >= M[i][j + 1];
      else if (ay > tg67) keep = m > M[i - 1][j] && m >= M[i + 1][j];
      else {
        const int s = (dx ^ dy) < 0 ? -1 : 1;
        keep = m > M[i - 1][j - s] && m > M[i + 1][j + s];
      }
      if (keep) c = m > high ? 2 : 0;
    }
    packed |= (uint32_t)c << (8 * k);
  }
  const int x = x0 + lx;
  const size_t o = ((size_t)b * H + y) * W + x;
  if (x + 3 < W && (o & 3) == 0) *(uint32_t*)(cls + o) = packed;
  else for (int k = 0; k < 4; ++k) if (x + k < W) cls[o + k] = (uint8_t)(packed >> (8 * k));
}

// One workgroup: a LT x LT tile of the class map, 4 consecutive pixels per thread.  Labels are LOCAL row-major indices (-1: class 1 or outside).
// Every pass takes the minimum over the pixel and its 8 neighbours, then jumps once through that label's own label.  Passes race on the LDS words;
// labels only ever decrease and always name a pixel of the same component, which is all the argument needs.
__global__ __launch_bounds__(256) void canny_label_tile_kernel(const uint8_t* __restrict__ cls, int H, int W, int tiles_x, int tiles_y,
                                                               int* __restrict__ parent, uint8_t* __restrict__ flag) {
  __shared__ int lab[LP][LP];
  const int tid = threadIdx.x;
  int blk = blockIdx.x;
  const int tx = blk % tiles_x; blk /= tiles_x;
  const int ty = blk % tiles_y;
  const int b = blk / tiles_y;
  const int x0 = tx * LT, y0 = ty * LT;
  for (int it = tid; it < LP * LP; it += 256) (&lab[0][0])[it] = -1;
  __syncthreads();
  const int ly = tid >> 3, lx = (tid & 7) * 4;
  const int y = y0 + ly, x = x0 + lx;
  const long base = ((long)b * H + y) * W + x;                           // < 2^31 wherever it is used (y < H, x < W)
  if (y < H && x < W) {
    uint32_t v;
    if (x + 3 < W && (base & 3) == 0) v = *(const uint32_t*)(cls + base);
    else { v = 0x01010101u; for (int k = 0; k < 4; ++k) if (x + k < W) v = (v & ~(0xffu << (8 * k))) | ((uint32_t)cls[base + k] << (8 * k)); }
    for (int k = 0; k < 4; ++k)
      if (x + k < W && ((v >> (8 * k)) & 0xff) != 1) lab[ly + 1][lx + k + 1] = ly * LT + lx + k;
  }
  __syncthreads();
  // Bound: after pass k every pixel within k steps (inside the tile) of its component's smallest pixel holds that pixel's index -- the barrier makes
  // pass k - 1's writes visible to pass k -- and no path is longer than LT * LT - 1 steps; one more pass sees no change.  The jump only speeds it up.
  for (int pass = 0; pass <= LT * LT; ++pass) {
    bool changed = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = ly + 1, j = lx + k + 1;
      const int l = lab[i][j];
      if (l < 0) continue;
      int m = l;
#pragma unroll
      for (int d = 0; d < 9; ++d) {
        const int n = lab[i + d / 3 - 1][j + d % 3 - 1];
        if (n >= 0 && n < m) m = n;
      }
      const int jump = lab[m / LT + 1][m % LT + 1];                      // m names a pixel of this component, so jump >= 0
      if (jump >= 0 && jump < m) m = jump;
      if (m < l) { lab[i][j] = m; changed = true; }
    }
    if (!__syncthreads_or(changed)) break;                               // workgroup-uniform
  }
  if (y < H && x < W) {
    int p[4];
    for (int k = 0; k < 4; ++k) {
      const int l = lab[ly + 1][lx + k + 1];
      p[k] = l < 0 ? -1 : (b * H + y0 + l / LT) * W + x0 + l % LT;
    }
    if (x + 3 < W && (base & 3) == 0) {
      *(int4*)(parent + base) = make_int4(p[0], p[1], p[2], p[3]);
      *(uint32_t*)(flag + base) = 0;
    } else {
      for (int k = 0; k < 4; ++k) if (x + k < W) { parent[base + k] = p[k]; flag[base + k] = 0; }
    }
  }
}

namespace {

// Root of i while other workgroups may be uniting: every read an agent-scope atomic load (a plain load may return a stale line of another XCD's
// write).  Bound: parent[j] <= j for every j at all times and the walk stops where parent[j] == j, so it visits strictly decreasing indices: at most
// i + 1 of them.  A stale or superseded ancestor is still a member of i's set with a smaller index, so the result is a member that WAS a root.
__device__ __forceinline__ int find_atomic(int* parent, int i) {
  for (;;) {
    const int p = __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p >= i || p < 0) return i;                                       // p == i: a root.  (p > i, p < 0 cannot happen; they would end the walk too)
    i = p;
  }
}

// Join the sets of a and b.  The larger root is hung under the smaller with an atomic min; the value the atomic RETURNS says whether that node was
// still a root.  If it was not (another union got there first) its former parent `old` has to be joined with b as well, whichever of the two the min
// kept.  Bound: a + b strictly decreases from one pass to the next (a is replaced by something <= old < a, b never grows) and both stay >= 0.
// Nothing here waits for another workgroup: a pass either finishes or makes progress by itself.
__device__ __forceinline__ void unite(int* parent, int a, int b) {
  a = find_atomic(parent, a);
  b = find_atomic(parent, b);
  while (a != b) {
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = __hip_atomic_fetch_min(parent + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == a) break;
    a = find_atomic(parent, old);
    b = find_atomic(parent, b);
  }
}

// Root of i between launches (nobody writes parent): plain loads.  Same bound as find_atomic.
__device__ __forceinline__ int find_plain(const int* __restrict__ parent, int i) {
  for (;;) {
    const int p = parent[i];
    if (p >= i || p < 0) return i;
    i = p;
  }
}

}  // namespace

// One thread per pixel; only pixels on a tile's first row, first column or last column have a neighbour among (W, NW, N, NE) in another tile.
// Every 8-adjacent pair has one member that sees the other in one of those four directions, the corner diagonals included.
__global__ __launch_bounds__(256) void canny_seam_kernel(const uint8_t* __restrict__ cls, int H, int W, int n, int* parent) {
  const unsigned u = blockIdx.x * 256u + threadIdx.x;                    // (n < 2^31: no wrap)
  if (u >= (unsigned)n) return;
  const int i = (int)u;
  const int hw = H * W;
  const int p = i % hw, y = p / W, x = p - y * W;
  const int tx = x % LT, ty = y % LT;
  const bool top = ty == 0 && y > 0, left = tx == 0 && x > 0, right = tx == LT - 1 && x + 1 < W && y > 0;
  if (!(top || left || right)) return;
  if (cls[i] == 1) return;
  if (left && cls[i - 1] != 1) unite(parent, i, i - 1);
  if (y > 0 && x > 0 && (top || left) && cls[i - W - 1] != 1) unite(parent, i, i - W - 1);
  if (top && cls[i - W] != 1) unite(parent, i, i - W);
  if (y > 0 && x + 1 < W && (top || right) && cls[i - W + 1] != 1) unite(parent, i, i - W + 1);
}

// 4 consecutive pixels per thread; every strong pixel marks its root (many writers, one value)
__global__ __launch_bounds__(256) void canny_flag_kernel(const uint8_t* __restrict__ cls, int n, const int* __restrict__ parent,
                                                         uint8_t* __restrict__ flag) {
  const unsigned u = (blockIdx.x * 256u + threadIdx.x) * 4u;             // (n < 2^31: no wrap)
  if (u >= (unsigned)n) return;
  const int i = (int)u;
  uint32_t v;
  if (i + 3 < n) v = *(const uint32_t*)(cls + i);
  else { v = 0x01010101u; for (int k = 0; k < 4; ++k) if (i + k < n) v = (v & ~(0xffu << (8 * k))) | ((uint32_t)cls[i + k] << (8 * k)); }
  for (int k = 0; k < 4; ++k)
    if (((v >> (8 * k)) & 0xff) == 2) flag[find_plain(parent, i + k)] = 1;
}

template <int DST>   // GDF_CANNY_DST_U8: uint8 [B][H][W] 0 / 255; GDF_CANNY_DST_F16_NCHW3: fp16 [B][3][H][W] 0.0 / 1.0
__global__ __launch_bounds__(256) void canny_emit_kernel(const uint8_t* __restrict__ cls, int hw, int n, const int* __restrict__ parent,
                                                         const uint8_t* __restrict__ flag, void* __restrict__ dst) {
  const unsigned u = (blockIdx.x * 256u + threadIdx.x) * 4u;             // (n < 2^31: no wrap)
  if (u >= (unsigned)n) return;
  const int i = (int)u;
  uint32_t v;
  if (i + 3 < n) v = *(const uint32_t*)(cls + i);
  else { v = 0x01010101u; for (int k = 0; k < 4; ++k) if (i + k < n) v = (v & ~(0xffu << (8 * k))) | ((uint32_t)cls[i + k] << (8 * k)); }
  bool e[4];
  for (int k = 0; k < 4; ++k) {
    const int c = (v >> (8 * k)) & 0xff;
    e[k] = c == 2 || (c == 0 && flag[find_plain(parent, i + k)] != 0);
  }
  if constexpr (DST == 0) {
    uint8_t* o = (uint8_t*)dst;
    if (i + 3 < n) *(uint32_t*)(o + i) = (e[0] ? 0xffu : 0u) | (e[1] ? 0xff00u : 0u) | (e[2] ? 0xff0000u : 0u) | (e[3] ? 0xff000000u : 0u);
    else for (int k = 0; k < 4; ++k) if (i + k < n) o[i + k] = e[k] ? 255 : 0;
  } else {
    uint16_t* o = (uint16_t*)dst;                                        // fp16 1.0 = 0x3c00
    if ((hw & 3) == 0) {                                                 // i % 4 == 0 and hw % 4 == 0: the four pixels share an image, 8-byte aligned
      const int b = i / hw, p = i - b * hw;
      const uint2 w = make_uint2((e[0] ? 0x3c00u : 0u) | (e[1] ? 0x3c000000u : 0u), (e[2] ? 0x3c00u : 0u) | (e[3] ? 0x3c000000u : 0u));
      for (int c = 0; c < 3; ++c) *(uint2*)(o + ((size_t)b * 3 + c) * hw + p) = w;
    } else {
      for (int k = 0; k < 4; ++k) {
        if (i + k >= n) break;
        const int b = (i + k) / hw, p = (i + k) - b * hw;
        for (int c = 0; c < 3; ++c) o[((size_t)b * 3 + c) * hw + p] = e[k] ? 0x3c00 : 0;
      }
    }
  }
}

size_t canny_workspace_bytes(int B, int H, int W) {
  const size_t n = (size_t)B * H * W;
  auto r16 = [](size_t v) { return (v + 15) / 16 * 16; };
  return r16(4 * n) + 2 * r16(n);                                        // parent int32 [n], flag uint8 [n], class map uint8 [n] (the fused entry's)
}

hipError_t launch_canny_classify(const void* src, int src_kind, int B, int H, int W, int low, int high, uint8_t* cls, hipStream_t s) {
  const int tx = (W + CL_TW - 1) / CL_TW, ty = (H + CL_TH - 1) / CL_TH;
  const dim3 grid((unsigned)((size_t)tx * ty * B)), block(256);
  switch (src_kind) {
    case 0: hipLaunchKernelGGL(canny_classify_kernel<0>, grid, block, 0, s, src, B, H, W, tx, ty, low, high, cls); break;
    case 1: hipLaunchKernelGGL(canny_classify_kernel<1>, grid, block, 0, s, src, B, H, W, tx, ty, low, high, cls); break;
    case 2: hipLaunchKernelGGL(canny_classify_kernel<2>, grid, block, 0, s, src, B, H, W, tx, ty, low, high, cls); break;
    case 3: hipLaunchKernelGGL(canny_classify_kernel<3>, grid, block, 0, s, src, B, H, W, tx, ty, low, high, cls); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_canny_link(const uint8_t* cls, int B, int H, int W, void* dst, int dst_kind, void* workspace, hipStream_t s) {
  const size_t n = (size_t)B * H * W;
  int* parent = (int*)workspace;
  uint8_t* flag = (uint8_t*)workspace + (4 * n + 15) / 16 * 16;
  const int tx = (W + LT - 1) / LT, ty = (H + LT - 1) / LT;
  const unsigned per_px = (unsigned)((n + 255) / 256), per_4 = (unsigned)((n + 1023) / 1024);
  hipLaunchKernelGGL(canny_label_tile_kernel, dim3((unsigned)((size_t)tx * ty * B)), dim3(256), 0, s, cls, H, W, tx, ty, parent, flag);
  hipLaunchKernelGGL(canny_seam_kernel, dim3(per_px), dim3(256), 0, s, cls, H, W, (int)n, parent);
  hipLaunchKernelGGL(canny_flag_kernel, dim3(per_4), dim3(256), 0, s, cls, (int)n, (const int*)parent, flag);
  if (dst_kind == 0)
    hipLaunchKernelGGL(canny_emit_kernel<0>, dim3(per_4), dim3(256), 0, s, cls, H * W, (int)n, (const int*)parent, (const uint8_t*)flag, dst);
  else if (dst_kind == 1)
    hipLaunchKernelGGL(canny_emit_kernel<1>, dim3(per_4), dim3(256), 0, s, cls, H * W, (int)n, (const int*)parent, (const uint8_t*)flag, dst);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

uint8_t* canny_workspace_cls(void* workspace, int B, int H, int W) {
  const size_t n = (size_t)B * H * W;
  auto r16 = [](size_t v) { return (v + 15) / 16 * 16; };
  return (uint8_t*)workspace + r16(4 * n) + r16(n);
}

}  // namespace gdf
