// Output convolution of the correspondence evaluator's aggregation network on an aggregated feature map, gfx950.
//
// Reference op replaced (paths in the reference repository):
//   correspondence/correspondence/aggregation_network.py:20-22   self.out = nn.Conv2d(dim, out_dim, kernel_size=3, stride=1, padding=1, bias=False)
//   correspondence/correspondence/aggregation_network.py:97-100  x = x.type(torch.float32); x = self.out(x), on the 128 x 128 aggregated map,
//                                                                once per image of every pair (task-corres.py:60-67)
//
// out[b, co, y, x] = bias[co] + sum_{ci, dy, dx} W[co, ci, dy, dx] in[b, ci, y + dy - 1, x + dx - 1], zeros outside the image: an implicit GEMM with
// Cout as the MFMA rows, pixels as the columns and K = 9 Cin, fp32-exact in the sense of pixcls.hip:
//   weights   an fp16 (hi, lo) pair per element, every output channel's 9 Cin row scaled by a power of two that the fp32 epilogue undoes, packed at
//             creation in fragment order [32-row block][channel tile][tap][16-channel step][hi, lo][lane][8]: a wave streams its block with one
//             16-byte load per lane and fragment, straight into registers (no other wave of the workgroup wants those rows).
//   map       an fp16 map is multiplied as given (lo x, hi x: two passes on one x fragment); an fp32 map is split into (hi, lo) as it is staged
//             (three passes, lo lo dropped).
//   staging   a workgroup = 256 output channels x a 32 x 4 pixel patch of one image.  Per tile of 32 input channels the patch and its one-pixel halo
//             (34 x 6 pixels) go to LDS as [pixel][channel], 80 bytes per pixel; the B operand of a tap is a 16-byte read along the channels at the
//             pixel shifted by (dy, dx): any shift is a multiple of 80 bytes, so every read keeps its 16-byte alignment (the transposed LDS read
//             on a [channel][pixel] image would not: a shift of one pixel is 2 bytes).  All nine taps are served from the one image; the halo
//             outside the map and the channels from Cin up are ZEROS WRITTEN BY THE STAGING CODE, nothing beside the map is ever read.
//   sums      a wave's accumulators take one channel tile (18 MFMA steps); after each tile they are folded into a second fp32 total, so no
//             accumulator sees more than 36 (fp32 map: 54) accumulations however deep Cin is.
// Workgroups are numbered so that the pixel tiles of one 256-row block follow one another ON ONE XCD (they share the block's packed rows through
// that XCD's L2).  Every tile lies inside one image.  No atomics, no split-K, fixed summation order, stream-ordered, no allocation in a launch.
#include <math.h>

#include <algorithm>
#include <vector>

#include "feat_common.h"

namespace gdf {

namespace {

enum {
  AH_PW = 32, AH_PH = 4,             // pixel patch of a workgroup: one MFMA column block per patch row
  AH_LW = AH_PW + 2, AH_LH = AH_PH + 2,
  AH_NPX = AH_LW * AH_LH,            // staged pixels: the patch and its halo (204)
  AH_KT = 32,                        // channels per staged tile (two MFMA k-steps)
  AH_PST = 80,                       // bytes per staged pixel: 32 halves + 16 bytes; 20 dwords: the 16 lanes of a ds_read_b128 group hit 64 banks once
  AH_IMG = AH_NPX * AH_PST,          // bytes of one x image
  AH_NT = 512,                       // threads: eight waves, wave w = rows 32 w .. 32 w + 31 of the block, all 128 pixels
  AH_ROWS = 256,                     // output channels per workgroup
  AH_STEPS = 9 * AH_KT / 16,         // MFMA k-steps per tile: [tap][16-channel step]
  AH_NW = 3,                         // weight fragments in registers (the one in use and two ahead); divides AH_STEPS
};

struct AhArgs {
  const void* x; long sb, sc, sy, sx; int C, H, W;
  const u32x4* w; const float *inv_s, *bias; float* out;
  int Cout, nkt, nrb, tx, ty; long ntile; unsigned chunk; long total;
};

// T: the map's element type.  CL: channels-last map (sc == 1, C a multiple of the 16-byte vector, aligned pixels): 16-byte loads along C; otherwise
// two elements per thread and load with the map's own strides, lanes along the patch row (coalesced where sx == 1).
template <typename T, bool CL>
__global__ __launch_bounds__(AH_NT) void ah_conv_kernel(const AhArgs a) {
  constexpr bool F32 = sizeof(T) == 4;
  constexpr int NIMG = F32 ? 2 : 1;              // x images of a tile: hi (and lo)
  constexpr int BUF = NIMG * AH_IMG;             // bytes of one of the two staging buffers
  constexpr int V = MapVec<T>::V;
  constexpr int NCHP = AH_KT / V;                // CL: 16-byte chunks per pixel and tile
  constexpr int NIT = CL ? (AH_NPX * NCHP + AH_NT - 1) / AH_NT : AH_KT / 4;   // staging items per thread
  typedef typename MapVec<T>::type vt;
  extern __shared__ __attribute__((aligned(16))) char ah_smem[];

  // (row block, pixel tile) of this workgroup: consecutive numbers on one XCD
  const long L = xcd_slot(blockIdx.x, a.chunk);
  if (L >= a.total) return;                      // (whole workgroups, before any barrier)
  const int cb = (int)(L / a.ntile);
  const long tile = L % a.ntile;
  const int tpi = a.tx * a.ty;
  const int b = (int)(tile / tpi), tr = (int)(tile % tpi);
  const int y0 = (tr / a.tx) * AH_PH, x0 = (tr % a.tx) * AH_PW;

  const int t = threadIdx.x, lane = t & 63, w = __builtin_amdgcn_readfirstlane(t >> 6), lh = lane >> 5, q = lane & 31;
  const int rb = cb * (AH_ROWS / 32) + w;
  const bool active = rb < a.nrb;                // (wave-uniform) a block past Cout: the wave stages and waits, nothing else

  // ---- staging.  CL: item i of a thread is 16-byte chunk (t + 512 i) % NCHP of pixel (t + 512 i) / NCHP.  Otherwise threads 0-407 are (pixel
  // t % 204, half t / 204) and item i is the channel pair t / 204 + 2 i of that pixel: one offset and one test per thread ----
  constexpr int NOFF = CL ? NIT : 1;
  long xoff[NOFF];                               // element offset of the item's pixel and first channel in tile 0
  int loff[NOFF];                                // byte offset in an x image; < 0: no such item
  unsigned inside = 0;                           // bit i: the item's pixel lies in the map (otherwise zeros are staged and nothing is loaded)
  const int hf = t / AH_NPX;                     // (not CL)
#pragma unroll
  for (int i = 0; i < NOFF; ++i) {
    const int idx = t + AH_NT * i;
    const int pp = CL ? idx / NCHP : t - hf * AH_NPX, ch = CL ? idx % NCHP : hf;
    const bool item = CL ? pp < AH_NPX : hf < 2;
    const int ly = pp / AH_LW, lx = pp - ly * AH_LW;
    const int gy = y0 + ly - 1, gx = x0 + lx - 1;
    const bool in = item && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
    xoff[i] = in ? (long)b * a.sb + (long)gy * a.sy + (long)gx * a.sx + (long)(ch * (CL ? V : 2)) * a.sc : 0;
    inside |= in ? 1u << i : 0u;
    loff[i] = item ? pp * AH_PST + ch * (CL ? (F32 ? 8 : 16) : 4) : -1;
  }
  T xe[CL ? 1 : NIT][2];
  vt xv[CL ? NIT : 1];
  auto load_x = [&](int kt) {
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      if constexpr (CL) {
        const int c0 = kt * AH_KT + ((t + AH_NT * i) % NCHP) * V;
        xv[i] = (((inside >> i) & 1) && c0 < a.C) ? *(const vt*)((const T*)a.x + xoff[i] + kt * AH_KT) : (vt)(T)0;
      } else {
        const int c0 = kt * AH_KT + 2 * hf + 4 * i;
        const T* p = (const T*)a.x + xoff[0] + (long)(kt * AH_KT + 4 * i) * a.sc;
        xe[i][0] = (inside && c0 < a.C) ? p[0] : (T)0;
        xe[i][1] = (inside && c0 + 1 < a.C) ? p[a.sc] : (T)0;
      }
    }
  };
  auto store_x = [&](char* buf) {
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      if (loff[CL ? i : 0] < 0) continue;
      char* d = buf + loff[CL ? i : 0] + (CL ? 0 : 8 * i);
      if constexpr (CL && !F32) {
        *(f16x8*)d = xv[i];
      } else if constexpr (CL) {
        f16x4 hi, lo;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          hi[j] = f32_to_f16_sat(xv[i][j]);
          lo[j] = f32_to_f16_sat(xv[i][j] - (float)hi[j]);
        }
        *(f16x4*)d = hi;
        *(f16x4*)(d + AH_IMG) = lo;
      } else if constexpr (F32) {
        f16x2 hi, lo;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          hi[j] = f32_to_f16_sat(xe[i][j]);
          lo[j] = f32_to_f16_sat(xe[i][j] - (float)hi[j]);
        }
        *(f16x2*)d = hi;
        *(f16x2*)(d + AH_IMG) = lo;
      } else {
        f16x2 v;
        v[0] = xe[i][0];
        v[1] = xe[i][1];
        *(f16x2*)d = v;
      }
    }
  };

  // ---- weights: fragment g of this wave's row block is step g % 18 of tile g / 18; [hi, lo] x 64 lanes x 16 bytes each ----
  const long gend = (long)a.nkt * AH_STEPS;
  const u32x4* wp = a.w + (size_t)(active ? rb : 0) * (size_t)gend * 2 * 64 + lane;
  u32x4 whi[AH_NW], wlo[AH_NW];
  auto load_w = [&](int slot, long g) {
    if (!active) return;
    const u32x4* p = wp + (size_t)(g < gend ? g : gend - 1) * 2 * 64;   // (past the end: the last fragment again, unused)
    whi[slot] = p[0];
    wlo[slot] = p[64];
  };

  f32x16 acc[AH_PH], tot[AH_PH];
#pragma unroll
  for (int j = 0; j < AH_PH; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = tot[j][r] = 0.f;

  // B operand of lane (q, lh): pixel q of a patch row, channels 8 lh .. 8 lh + 7 of a 16-channel step (the A fragments are packed to match)
  const int xl = q * AH_PST + lh * 16;

  load_x(0);
  load_w(0, 0);
  load_w(1, 1);
  store_x(ah_smem);
  if (a.nkt > 1) load_x(1);
  lds_barrier();
  for (int kt = 0; kt < a.nkt; ++kt) {
    GDF_LDS const char* cur = (GDF_LDS const char*)(ah_smem + (kt & 1) * BUF) + xl;
    // the other buffer was last read in tile kt - 1, which every wave has left: tile kt + 1 goes there now, and tile kt + 2 sets out
    if (kt + 1 < a.nkt) store_x(ah_smem + ((kt + 1) & 1) * BUF);
    if (kt + 2 < a.nkt) load_x(kt + 2);
    if (active) {
#pragma unroll
      for (int st = 0; st < AH_STEPS; ++st) {
        constexpr int NS = AH_KT / 16;
        const int tap = st / NS, s = st % NS, dy = tap / 3, dx = tap % 3;
        load_w((st + 2) % AH_NW, (long)kt * AH_STEPS + st + 2);
        const f16x8 ahi = __builtin_bit_cast(f16x8, whi[st % AH_NW]), alo = __builtin_bit_cast(f16x8, wlo[st % AH_NW]);
        f16x8 xf[NIMG][AH_PH];
#pragma unroll
        for (int im = 0; im < NIMG; ++im)
#pragma unroll
          for (int j = 0; j < AH_PH; ++j)
            xf[im][j] = *(GDF_LDS const f16x8*)(cur + im * AH_IMG + ((j + dy) * AH_LW + dx) * AH_PST + s * 32);
#pragma unroll
        for (int j = 0; j < AH_PH; ++j) {
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(alo, xf[0][j], acc[j], 0, 0, 0);
          if constexpr (F32) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi, xf[NIMG - 1][j], acc[j], 0, 0, 0);
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi, xf[0][j], acc[j], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);       // (a step's LDS reads stay in the step: hoisted further they cost more registers than there are)
      }
#pragma unroll
      for (int j = 0; j < AH_PH; ++j) {
        tot[j] += acc[j];
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
      }
    }
    lds_barrier();
  }

  // accumulator register r of lane (q, lh) is row 8 (r / 4) + 4 lh + r % 4 (the output channel), column q (the pixel of patch row j): the lanes
  // of a store run along x
  if (!active) return;
  const int gx = x0 + q;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int co = rb * 32 + (r >> 2) * 8 + lh * 4 + (r & 3);
    if (co >= a.Cout || gx >= a.W) continue;
    const float is = a.inv_s[co], bb = a.bias[co];
    float* o = a.out + (((long)b * a.Cout + co) * a.H + y0) * a.W + gx;
#pragma unroll
    for (int j = 0; j < AH_PH; ++j)
      if (y0 + j < a.H) o[(long)j * a.W] = tot[j][r] * is + bb;
  }
}

template <typename T, bool CL>
hipError_t ah_launch(const AhArgs& a, unsigned grid, hipStream_t s) {
  constexpr int smem = 2 * (sizeof(T) == 4 ? 2 : 1) * AH_IMG;               // (under the 64 KiB a kernel may ask for without an attribute)
  hipLaunchKernelGGL((ah_conv_kernel<T, CL>), dim3(grid), dim3(AH_NT), smem, s, a);
  return hipGetLastError();
}

// the device image of a head at `base` (null: the sizes alone): [packed fragments][1 / scale][bias]
struct AhLayout { int nkt, nrb; size_t blk; char* w; float *inv_s, *bias; size_t bytes; };
AhLayout ah_layout(int Cin, int Cout, void* base) {
  AhLayout l;
  l.nkt = (Cin + AH_KT - 1) / AH_KT;
  l.nrb = (Cout + 31) / 32;
  l.blk = (size_t)l.nkt * AH_STEPS * 2 * 64 * 8;                            // halves of one 32-row block
  Carver c(base);
  l.w = c.take<char>((size_t)l.nrb * l.blk * 2);
  l.inv_s = c.take<float>((size_t)l.nrb * 32 * 4);
  l.bias = c.take<float>((size_t)l.nrb * 32 * 4);
  l.bytes = c.bytes();
  return l;
}

// agghead_create's rule for one row on the device: the row's largest magnitude, sh = split_shift(max) and 1 / scale = 2^-sh; rows from Cout up
// to the end of the last 32-row block get 1
__global__ __launch_bounds__(256) void ah_rowscale_kernel(const float* __restrict__ W, int Cout, long rowlen, float* inv_s) {
  __shared__ float red[256];
  const int co = blockIdx.x, t = threadIdx.x;
  float m = 0.f;
  if (co < Cout)
    for (long i = t; i < rowlen; i += 256) m = fmaxf(m, fabsf(W[(long)co * rowlen + i]));
  red[t] = m;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) red[t] = fmaxf(red[t], red[t + s]);
    __syncthreads();
  }
  if (t == 0) inv_s[co] = ldexpf(1.f, -split_shift(red[0]));
}

// One thread = one lane entry (32-row block, channel tile, 16-channel step, lane) of the fragment image: 8 channels x 9 taps of one row, 72
// consecutive floats of W, become the lane's 16 bytes of the 18 (tap, hi / lo) fragments; the 64 lanes of a fragment store 1 KB in a row.  The
// row's shift is read back from 1 / scale = 2^-sh (an exact power of two, subnormals included), so the handle needs no scratch; only where 2^-sh
// has underflowed to 0 (a row whose largest magnitude is below 2^-136) the thread finds the row's maximum again.
__global__ __launch_bounds__(256) void ah_pack_kernel(const float* __restrict__ W, const float* __restrict__ inv_s, int Cin, int Cout, int nkt,
                                                      long n, u32x4* img) {
  const long id = (long)blockIdx.x * 256 + threadIdx.x;
  if (id >= n) return;
  const int lane = (int)(id & 63), s = (int)((id >> 6) & 1), kt = (int)((id >> 7) % nkt);
  const long rb = (id >> 7) / nkt;
  const int co = (int)rb * 32 + (lane & 31), ci0 = kt * AH_KT + s * 16 + (lane >> 5) * 8;
  int shv = 0;
  if (co < Cout) {
    const float inv = inv_s[co];
    if (inv > 0.f) {
      shv = -ilogbf(inv);
    } else {
      float m = 0.f;
      for (long i = 0; i < (long)Cin * 9; ++i) m = fmaxf(m, fabsf(W[(long)co * Cin * 9 + i]));
      shv = split_shift(m);
    }
  }
  u32x4* o = img + ((rb * nkt + kt) * 9 * (AH_KT / 16) + s) * 2 * 64 + lane;
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    f16x8 hi, lo;
#pragma unroll
    for (int el = 0; el < 8; ++el) {
      const float v = (co < Cout && ci0 + el < Cin) ? ldexpf(W[((long)co * Cin + ci0 + el) * 9 + tap], shv) : 0.f;
      hi[el] = (_Float16)v;
      lo[el] = (_Float16)(v - (float)hi[el]);
    }
    o[(long)tap * (AH_KT / 16) * 2 * 64] = __builtin_bit_cast(u32x4, hi);
    o[(long)tap * (AH_KT / 16) * 2 * 64 + 64] = __builtin_bit_cast(u32x4, lo);
  }
}

}  // namespace

hipError_t agghead_create(int Cin, int Cout, const float* W, const float* bias, AggHead** out) {
  void* dev = nullptr;
  hipError_t e = hipMalloc(&dev, ah_layout(Cin, Cout, nullptr).bytes);
  if (e != hipSuccess) return e;
  const AhLayout l = ah_layout(Cin, Cout, dev);
  const int nkt = l.nkt, nrb = l.nrb;
  const size_t blk = l.blk;
  // one 32-row block at a time (the packed image of the largest head is close to 1 GB: it is never held on the host as a whole)
  std::vector<uint16_t> img(blk);
  std::vector<float> inv((size_t)nrb * 32, 1.f), bs((size_t)nrb * 32, 0.f);
  const size_t rowlen = (size_t)Cin * 9;
  for (int rb = 0; rb < nrb && e == hipSuccess; ++rb) {
    std::fill(img.begin(), img.end(), 0);
    for (int n = 0; n < 32; ++n) {
      const int co = rb * 32 + n;
      if (co >= Cout) break;
      const float* row = W + (size_t)co * rowlen;
      float mx = 0.f;
      for (size_t i = 0; i < rowlen; ++i) mx = std::max(mx, fabsf(row[i]));
      const int sh = split_shift(mx);
      inv[co] = ldexpf(1.f, -sh);
      if (bias) bs[co] = bias[co];
      for (int ci = 0; ci < Cin; ++ci) {
        const int kt = ci / AH_KT, s = (ci % AH_KT) / 16, lh = (ci % 16) / 8, el = ci % 8;
        for (int tap = 0; tap < 9; ++tap) {
          const float v = ldexpf(row[(size_t)ci * 9 + tap], sh);
          const _Float16 hi = (_Float16)v;
          uint16_t* dh = img.data() + (((((size_t)kt * 9 + tap) * (AH_KT / 16) + s) * 2 + 0) * 64 + lh * 32 + n) * 8 + el;
          dh[0] = half_bits((float)hi);
          dh[64 * 8] = half_bits(v - (float)hi);
        }
      }
    }
    e = hipMemcpy(l.w + (size_t)rb * blk * 2, img.data(), blk * 2, hipMemcpyHostToDevice);
  }
  if (e == hipSuccess) e = hipMemcpy(l.inv_s, inv.data(), inv.size() * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(l.bias, bs.data(), bs.size() * 4, hipMemcpyHostToDevice);
  if (e != hipSuccess) { (void)hipFree(dev); return e; }
  *out = new AggHead{Cin, Cout, nkt, nrb, dev, l.w, l.inv_s, l.bias};
  return hipSuccess;
}

// the packed image and 1 / scale of `h` from fp32 OIHW weights on the device: two launches, stream-ordered, nothing else
hipError_t agghead_update(AggHead* h, const float* W_dev, hipStream_t s) {
  if (!h || !W_dev) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ah_rowscale_kernel, dim3(h->nrb * 32), dim3(256), 0, s, W_dev, h->Cout, (long)h->Cin * 9, (float*)h->inv_s);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const long n = (long)h->nrb * h->nkt * 2 * 64;
  hipLaunchKernelGGL(ah_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, W_dev, h->inv_s, h->Cin, h->Cout, h->nkt, n,
                     (u32x4*)h->w);
  return hipGetLastError();
}

hipError_t agghead_create_device(int Cin, int Cout, const float* W_dev, const float* bias_dev, hipStream_t s, AggHead** out) {
  void* dev = nullptr;
  hipError_t e = hipMalloc(&dev, ah_layout(Cin, Cout, nullptr).bytes);
  if (e != hipSuccess) return e;
  const AhLayout l = ah_layout(Cin, Cout, dev);
  AggHead* h = new AggHead{Cin, Cout, l.nkt, l.nrb, dev, l.w, l.inv_s, l.bias};
  e = hipMemsetAsync(l.bias, 0, (size_t)l.nrb * 32 * 4, s);
  if (e == hipSuccess && bias_dev) e = hipMemcpyAsync(l.bias, bias_dev, (size_t)Cout * 4, hipMemcpyDeviceToDevice, s);
  if (e == hipSuccess) e = agghead_update(h, W_dev, s);
  if (e != hipSuccess) { agghead_destroy(h); return e; }
  *out = h;
  return hipSuccess;
}

void agghead_destroy(AggHead* h) {
  if (!h) return;
  (void)hipFree(h->dev);
  delete h;
}

hipError_t launch_agghead(const AggHead* h, const AggSrc& x, int B, float* out, hipStream_t s) {
  if (!h || !x.ptr || !out || x.C != h->Cin || x.H < 1 || x.W < 1 || B < 0) return hipErrorInvalidValue;
  if ((long)B * x.H * x.W >= (1l << 31)) return hipErrorInvalidValue;
  if (B == 0) return hipSuccess;
  const int tx = (x.W + AH_PW - 1) / AH_PW, ty = (x.H + AH_PH - 1) / AH_PH;
  const long ntile = (long)B * tx * ty, total = ntile * ((h->Cout + AH_ROWS - 1) / AH_ROWS);
  const long chunk = xcd_chunk(total);
  if (chunk * XCDS >= (1l << 31)) return hipErrorInvalidValue;
  const AhArgs a{x.ptr, x.sb, x.sc, x.sy, x.sx, x.C, x.H, x.W, (const u32x4*)h->w, h->inv_s, h->bias, out,
                 h->Cout, h->nkt, h->nrb, tx, ty, ntile, (unsigned)chunk, total};
  const bool cl = map_lanes_c(x);
  const unsigned grid = (unsigned)(chunk * XCDS);
  if (x.f32) return cl ? ah_launch<float, true>(a, grid, s) : ah_launch<float, false>(a, grid, s);
  return cl ? ah_launch<_Float16, true>(a, grid, s) : ah_launch<_Float16, false>(a, grid, s);
}

}  // namespace gdf
