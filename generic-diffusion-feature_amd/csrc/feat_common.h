// What the feature-map ops share (post, corres, densematch, cliploss, pca, pixcls, agghead, aggwgrad): vector types, the rule
// for 16-byte loads along C, workspace carving, the row-scale rule of the fp16 (hi, lo) split, XCD numbering, (score, index) candidates, the
// fixed-order reductions and ATen's bilinear source index.  Every device helper is force-inlined into the including file's kernels and compiled
// under that file's flags; a helper that fixes a summation order says so, and the bits of the ops depend on it.
#pragma once
#include <math.h>
#include <string.h>

#include <type_traits>

#include "kernels.h"

#define GDF_LDS __attribute__((address_space(3)))

namespace gdf {

typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// the 16-byte vector of a map's element type and its length
template <typename T> struct MapVec;
template <> struct MapVec<_Float16> { typedef f16x8 type; enum { V = 8 }; };
template <> struct MapVec<float> { typedef f32x4 type; enum { V = 4 }; };

// ---- host: maps, workspaces, scales, grids ----

// sc == 1 and every pixel 16-byte aligned: a 16-byte vector may be loaded at any multiple of the vector length along C
inline bool map_pixels_aligned(const AggSrc& f) {
  const long vl = f.f32 ? 4 : 8;
  return f.sc == 1 && !((uintptr_t)f.ptr & 15) && !(f.sb % vl) && !(f.sy % vl) && !(f.sx % vl);
}
// lanes along C: a channels-last map whose C is whole vectors as well, so that no lane needs a partial vector
inline bool map_lanes_c(const AggSrc& f) { return map_pixels_aligned(f) && !(f.C % (f.f32 ? 4 : 8)); }

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// consecutive 256-byte aligned pieces of one allocation; a null base gives the byte count alone
struct Carver {
  char* base;
  size_t off = 0;
  explicit Carver(void* b) : base((char*)b) {}
  template <typename T> T* take(size_t bytes) {
    T* r = (T*)(base + off);
    off += up256(bytes);
    return r;
  }
  size_t bytes() const { return off; }
};

// the shift of a row of an fp16 (hi, lo) split: 2^shift brings the row's largest magnitude into [2^13, 2^14), so the low halves stay clear of the
// fp16 subnormals; 0 for a zero or non-finite maximum
__host__ __device__ __forceinline__ int split_shift(float m) { return (m > 0.f && m < INFINITY) ? 13 - ilogbf(m) : 0; }

// fp32 -> fp16 bits on the host, round to nearest even, subnormals included
inline uint16_t half_bits(float v) {
  const _Float16 h = (_Float16)v;
  uint16_t u;
  memcpy(&u, &h, 2);
  return u;
}

// Workgroups go round-robin over the XCDS dies, so `total` consecutive work items are dealt in chunks: die d runs items [d chunk, (d + 1) chunk)
// and neighbours share its L2.  The grid is xcd_chunk(total) * XCDS workgroups; a slot >= total returns at once.
enum { XCDS = 8 };
inline long xcd_chunk(long total) { return (total + XCDS - 1) / XCDS; }

// the instantiation of a chunk of nq queries, nq one of 4, 8, .. 20 or MAXQ: f(std::integral_constant<int, NQ>())
template <int MAXQ, typename F>
inline void by_nq(int nq, F&& f) {
  switch (nq) {
    case 4: f(std::integral_constant<int, 4>()); break;
    case 8: f(std::integral_constant<int, 8>()); break;
    case 12: f(std::integral_constant<int, 12>()); break;
    case 16: f(std::integral_constant<int, 16>()); break;
    case 20: f(std::integral_constant<int, 20>()); break;
    default: f(std::integral_constant<int, MAXQ>()); break;
  }
}

// ---- device ----
#if defined(__HIPCC__)

__device__ __forceinline__ long xcd_slot(unsigned block, unsigned chunk) { return (long)(block % XCDS) * chunk + block / XCDS; }

// every wave's LDS writes have landed and every wave's LDS reads have returned; global loads stay in flight (a __syncthreads() would drain them)
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

template <typename T>
__device__ __forceinline__ float ld(const void* p, long o) { return (float)((const T*)p)[o]; }

// ATen's area_pixel_compute_source_index (align_corners = false) in separately rounded fp32 operations, and the taps of upsample_bilinear2d
__device__ __forceinline__ void bilinear_src(int dst, float scale, int in, int& i0, int& i1, float& l1) {
#pragma clang fp contract(off)
  const float s = fmaxf(scale * ((float)dst + 0.5f) - 0.5f, 0.f);
  i0 = min((int)s, in - 1);
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = s - (float)i0;
}

// (score, index) candidates: the higher score wins, then the lower index: a total order.  A NaN never wins (scores enter only through `>`).
template <typename I>
__device__ __forceinline__ void best_take(float& s, I& i, float os, I oi) {
  if (os > s || (os == s && oi < i)) { s = os; i = oi; }
}
template <typename I>
__device__ __forceinline__ void wave_best(float& s, I& i) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float os = __shfl_xor(s, off);
    const I oi = (I)__shfl_xor((int)i, off);
    best_take(s, i, os, oi);
  }
}

// the sum (maximum) of 256 threads' values in a fixed tree, halves 128 .. 1; every thread receives it.  red: 256 floats
__device__ __forceinline__ float block_sum256(float v, float* red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int half = 128; half >= 1; half >>= 1) {
    if ((int)threadIdx.x < half) red[threadIdx.x] += red[threadIdx.x + half];
    __syncthreads();
  }
  return red[0];
}
__device__ __forceinline__ float block_max256(float v, float* red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int half = 128; half >= 1; half >>= 1) {
    if ((int)threadIdx.x < half) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + half]);
    __syncthreads();
  }
  return red[0];
}

#endif  // __HIPCC__

}  // namespace gdf
