// ControlNet conditioning kernels, gfx950.
//
// Reference op replaced (paths under the reference's feature/ directory):
//   diffusers/models/unet/unet_2d_condition.py:1236-1245, 1269-1270   `down_block_res_sample + down_block_additional_residual` for every
//   skip tensor and `sample + mid_block_additional_residual`          -> residual_add_kernel
//
// The UNet plan keeps no copies of its skip tensors: each one lives in the skip slice of the up-path concat buffer that consumes it, and the
// mid block's output in the h slice of the first of those buffers (model.cpp build()).  So the adds run in place on strided row slices, all
// of them in ONE launch that walks a small table: HBM-bound (read slice + read residual + write slice), 16 bytes per lane.
#include <algorithm>

#include "kernels.h"

namespace gdf {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// one tensor of the launch: rows of c8 16-byte vectors; `end` = running total of vectors up to and including this tensor
struct ResAddItem { half_t* dst; const half_t* res; unsigned end; int c8; int ld; int lo; };
struct ResAddTable { ResAddItem it[RES_ADD_MAX]; };

// dst[r][c] += res[r][c] for every tensor of the table.  Plain image: one fp32 add, one rounding to fp16.  Split image (lo > 0: the row holds
// hi at column c and lo = fp16(v - hi) `lo` elements further): v = hi + lo + res in fp32, stored as a new pair.
__global__ __launch_bounds__(256) void residual_add_kernel(ResAddTable t, unsigned total) {
  for (unsigned v = blockIdx.x * 256u + threadIdx.x; v < total; v += gridDim.x * 256u) {
    int k = 0;
    unsigned beg = 0;
    while (v >= t.it[k].end) beg = t.it[k++].end;          // (total == the last end: k stays inside the table)
    const ResAddItem& e = t.it[k];
    const unsigned i = v - beg, r = i / (unsigned)e.c8, c = (i - r * (unsigned)e.c8) * 8u;
    half_t* d = e.dst + (size_t)r * e.ld + c;
    const f16x8 a = *(const f16x8*)d;
    const f16x8 x = *(const f16x8*)(e.res + (size_t)i * 8);
    f16x8 hi;
    if (e.lo > 0) {
      const f16x8 al = *(const f16x8*)(d + e.lo);
      f16x8 lo;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float s = ((float)a[j] + (float)al[j]) + (float)x[j];
        hi[j] = (_Float16)s;
        lo[j] = (_Float16)(s - (float)hi[j]);
      }
      *(f16x8*)(d + e.lo) = lo;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) hi[j] = (_Float16)((float)a[j] + (float)x[j]);
    }
    *(f16x8*)d = hi;
  }
}

hipError_t launch_residual_add(const ResAddDesc* d, int n, hipStream_t s) {
  if (n < 0 || n > RES_ADD_MAX || (n > 0 && !d)) return hipErrorInvalidValue;
  ResAddTable t{};
  size_t total = 0;
  int m = 0;
  for (int k = 0; k < n; ++k) {
    const ResAddDesc& e = d[k];
    if (e.rows < 0 || e.C < 0 || (e.C & 7) || (e.ld & 7) || (e.lo & 7) || e.lo < 0 || e.ld < e.C) return hipErrorInvalidValue;
    if (e.rows == 0 || e.C == 0) continue;
    if (!e.dst || !e.res || ((uintptr_t)e.dst & 15) || ((uintptr_t)e.res & 15)) return hipErrorInvalidValue;
    if (e.lo > 0 && e.lo < e.C) return hipErrorInvalidValue;                 // the halves of a pair do not overlap
    total += (size_t)e.rows * (e.C / 8);
    if (total >= (1ull << 32)) return hipErrorInvalidValue;
    t.it[m++] = ResAddItem{e.dst, e.res, (unsigned)total, e.C / 8, e.ld, e.lo};
  }
  if (total == 0) return hipSuccess;
  for (int k = m; k < RES_ADD_MAX; ++k) t.it[k].end = (unsigned)total;
  // grid-stride from 2048 workgroups (8 of 4 waves on each of the chip's 256 CUs) up
  const unsigned grid = (unsigned)std::min<size_t>((total + 255) / 256, 2048);
  hipLaunchKernelGGL(residual_add_kernel, dim3(grid), dim3(256), 0, s, t, (unsigned)total);
  return hipGetLastError();
}

}  // namespace gdf
