// Weight gradient of the aggregation network's 3 x 3 output convolution (agghead.hip is its forward), gfx950.
//
// Reference op replaced (paths in the reference repository):
//   correspondence/task-corres.py train(): loss.backward() through aggregation_network.out (nn.Conv2d(dim, out_dim, 3, padding=1, bias=False),
//   correspondence/correspondence/aggregation_network.py:20-22), the only trained tensor of `--algorithm conv`
//
// dW[co, ci, dy, dx] = sum_{b, y, x} G[b, co, y, x] X[b, ci, y + dy - 1, x + dx - 1], zeros outside the image: a GEMM with Cout as the MFMA rows,
// (ci, tap) as the columns and K = B H W pixels, fp32-exact in the sense of agghead.hip:
//   G         an fp16 (hi, lo) pair per element after a power-of-two scale per output channel.  Two pre-passes: the first leaves max |G| and the
//             shift of every channel in the workspace (the epilogue undoes the shift exactly with ldexp), the second writes the pairs to the
//             workspace in MFMA fragment order [32-row block][k-step][hi, lo][lane][8], zeros where a patch leaves the image or the rows pass
//             Cout.  A wave streams its block with one 16-byte load per lane and fragment, straight into registers (no other wave of the
//             workgroup wants those rows), three k-steps ahead of their use.
//   X         an fp16 map is multiplied as given (lo x, hi x: two passes); an fp32 map is split into (hi, lo) as it is staged (three passes).
//   staging   a workgroup = 128 output channels x 32 input channels x all 9 taps, and walks over K in 32 x 4 pixel patches.  A patch and its
//             one-pixel halo go to LDS as [channel][row][x] with 8 halves of margin on either side of a row: row pitch 96 bytes, channel pitch 592.
//             K runs along x, so the B operand of the CENTRE column of taps is a 16-byte read at a multiple of 16 bytes.  The left and right
//             columns are one pixel = 2 bytes away, where no 16-byte LDS read (transposed or not) is aligned: they are NOT read.  The lane reads
//             the dword before and the dword after its aligned chunk and builds both shifted fragments in registers with five 16-bit funnel shifts
//             (three of them shared).  A vertical shift is one row pitch, a multiple of 16 bytes.  The halo outside the map, the pixels past the
//             end of a row or image and the channels from Cin up are ZEROS WRITTEN BY THE STAGING CODE, nothing beside the map is ever read, and a
//             patch lies inside one image: a tap never reaches from image b into image b + 1.
//   sums      nine 32 x 32 accumulators per wave take one patch (8 k-steps: 16 accumulations, fp32 map 24) and are then folded into a second fp32
//             total, so no accumulator sees a deeper chain however large B H W is.
// Workgroups are numbered so that the channel tiles of one 128-row block follow one another ON ONE XCD (they share the block's rows of G through
// that XCD's L2).  No atomics, no split-K, fixed summation order, stream-ordered, no allocation in a launch.
#include <math.h>

#include "feat_common.h"

namespace gdf {

namespace {

enum {
  WG_PW = 32, WG_PH = 4,             // pixel patch of one staging round: two k-steps per patch row
  WG_LH = WG_PH + 2,                 // staged rows: the patch and its halo
  WG_MARGIN = 8,                     // halves before and after a staged row's 32 pixels (one is used on either side)
  WG_PITCH = (WG_PW + 2 * WG_MARGIN) * 2,   // bytes per staged row (96: a multiple of 16)
  WG_CST = WG_LH * WG_PITCH + 16,    // bytes per staged channel: 148 dwords = 4 x 37: the 16 lanes of a ds_read_b128 group hit 64 banks once
  WG_CT = 32,                        // input channels per workgroup: one MFMA column block
  WG_IMG = WG_CT * WG_CST,           // bytes of one x image
  WG_NT = 256,                       // threads: four waves, wave w = rows 32 w .. 32 w + 31 of the block; one wave per SIMD (288 accumulators)
  WG_ROWS = 128,                     // output channels per workgroup
  WG_KS = WG_PH * WG_PW / 16,        // k-steps per patch
  WG_NG = 4,                         // G fragment pairs in registers (the one in use and three ahead); divides WG_KS
  WG_NPAIR = WG_CT * (WG_PW + 2),    // (channel, staged column) pairs of a patch
  WG_NSLOT = (WG_NPAIR + WG_NT - 1) / WG_NT,   // pairs per thread; each pair is WG_LH elements, one per staged row
};

struct WgArgs {
  const void* x; long sb, sc, sy, sx; int C, H, W;
  const u32x4* gs; const int* sh; float* dw;
  int Cout, nct, nrb, accumulate; long ntile; unsigned chunk; long total;
};

// max |G| over (b, y, x) of one output channel -> mx[co], and its split_shift -> sh[co]
__global__ __launch_bounds__(256) void wg_rowmax_kernel(const float* __restrict__ g, int B, int Cout, long P, float* mx, int* sh) {
  __shared__ float red[256];
  const int co = blockIdx.x, t = threadIdx.x;
  float m = 0.f;
  for (int b = 0; b < B; ++b) {
    const float* p = g + ((long)b * Cout + co) * P;
    for (long i = t; i < P; i += 256) m = fmaxf(m, fabsf(p[i]));
  }
  red[t] = m;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) red[t] = fmaxf(red[t], red[t + s]);
    __syncthreads();
  }
  if (t == 0) {
    m = red[0];
    mx[co] = m;
    sh[co] = split_shift(m);
  }
}

// One thread = one lane entry of G's fragment image: (32-row block, k-step, lane (q, lh)) holds row 32 block + q, pixels 8 lh .. 8 lh + 7 of the
// k-step; k-step 8 patch + st is patch row st / 2, pixels 16 (st % 2) .. + 15 of it; patches run along x, then y, then the images.
__global__ __launch_bounds__(256) void wg_split_kernel(const float* __restrict__ g, const int* __restrict__ sh, int Cout, int H, int W, int tx,
                                                       int ty, long nks, long n, u32x4* gs) {
  const long id = (long)blockIdx.x * 256 + threadIdx.x;
  if (id >= n) return;
  const int lane = (int)(id & 63), q = lane & 31, lh = lane >> 5;
  const long ks = (id >> 6) % nks, rb = (id >> 6) / nks;
  const int st = (int)(ks % WG_KS);
  const long patch = ks / WG_KS;
  const int b = (int)(patch / ((long)tx * ty)), tr = (int)(patch % ((long)tx * ty));
  const int y = (tr / tx) * WG_PH + (st >> 1), xs = (tr % tx) * WG_PW + 16 * (st & 1) + 8 * lh, co = (int)rb * 32 + q;
  const bool ok = co < Cout && y < H;
  const long off = ok ? (((long)b * Cout + co) * H + y) * W + xs : 0;
  const int shv = ok ? sh[co] : 0;
  f16x8 hi, lo;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float v = (ok && xs + j < W) ? ldexpf(g[off + j], shv) : 0.f;
    hi[j] = f32_to_f16_sat(v);
    lo[j] = f32_to_f16_sat(v - (float)hi[j]);
  }
  u32x4* o = gs + (size_t)(id >> 6) * 128 + lane;
  o[0] = __builtin_bit_cast(u32x4, hi);
  o[64] = __builtin_bit_cast(u32x4, lo);
}

// T: the map's element type.  The map is read with its own strides, lanes along the staged row (coalesced where sx == 1).
template <typename T>
__global__ __launch_bounds__(WG_NT) void wg_kernel(const WgArgs a) {
  constexpr bool F32 = sizeof(T) == 4;
  constexpr int NIMG = F32 ? 2 : 1;              // x images: hi (and lo)
  __shared__ __attribute__((aligned(16))) char wg_smem[NIMG * WG_IMG];

  // (row block, channel tile) of this workgroup: consecutive numbers on one XCD
  const long L = xcd_slot(blockIdx.x, a.chunk);
  if (L >= a.total) return;                      // (whole workgroups, before any barrier)
  const int cb = (int)(L / a.nct), ct = (int)(L % a.nct);

  const int t = threadIdx.x, lane = t & 63, w = __builtin_amdgcn_readfirstlane(t >> 6), lh = lane >> 5, q = lane & 31;
  const int rb = cb * (WG_ROWS / 32) + w;
  const bool active = rb < a.nrb;                // (wave-uniform) a block past Cout: the wave stages and waits, nothing else

  // the margins and the pad are never staged: give them a value once (the halves beside the staged columns are read and shifted out)
  for (int i = t * 16; i < NIMG * WG_IMG; i += WG_NT * 16) *(u32x4*)(wg_smem + i) = (u32x4)0u;
  __syncthreads();

  // ---- staging.  Pair t + 256 j of a thread is channel pair / 34, staged column pair % 34 (global x = x0 + column - 1); its six elements are
  // the six staged rows ----
  int sinfo[WG_NSLOT];                           // channel << 8 | column; < 0: no such pair
#pragma unroll
  for (int j = 0; j < WG_NSLOT; ++j) {
    const int pair = t + WG_NT * j, ch = pair / (WG_PW + 2);
    sinfo[j] = pair < WG_NPAIR ? (ch << 8) | (pair - ch * (WG_PW + 2)) : -1;
  }
  T xe[WG_NSLOT][WG_LH];
  auto load_x = [&](int b, int y0, int x0) {
#pragma unroll
    for (int j = 0; j < WG_NSLOT; ++j) {
      const int c = ct * WG_CT + (sinfo[j] >> 8), gx = x0 + (sinfo[j] & 255) - 1;
      const bool okc = sinfo[j] >= 0 && c < a.C && gx >= 0 && gx < a.W;
      const long off = okc ? (long)b * a.sb + (long)c * a.sc + (long)gx * a.sx : 0;
#pragma unroll
      for (int ly = 0; ly < WG_LH; ++ly) {
        const int gy = y0 + ly - 1;
        xe[j][ly] = (okc && gy >= 0 && gy < a.H) ? ((const T*)a.x)[off + (long)gy * a.sy] : (T)0;
      }
    }
  };
  auto store_x = [&]() {
#pragma unroll
    for (int j = 0; j < WG_NSLOT; ++j) {
      if (sinfo[j] < 0) continue;
      char* d = wg_smem + (sinfo[j] >> 8) * WG_CST + (WG_MARGIN - 1 + (sinfo[j] & 255)) * 2;
#pragma unroll
      for (int ly = 0; ly < WG_LH; ++ly) {
        if constexpr (F32) {
          const _Float16 hi = f32_to_f16_sat(xe[j][ly]);
          *(_Float16*)(d + ly * WG_PITCH) = hi;
          *(_Float16*)(d + ly * WG_PITCH + WG_IMG) = f32_to_f16_sat(xe[j][ly] - (float)hi);
        } else {
          *(_Float16*)(d + ly * WG_PITCH) = xe[j][ly];
        }
      }
    }
  };

  // ---- G: fragment pair g of this wave's row block is k-step g % 8 of patch g / 8; [hi, lo] x 64 lanes x 16 bytes each ----
  const long gend = a.ntile * WG_KS;
  const u32x4* gp = a.gs + (size_t)(active ? rb : 0) * (size_t)gend * 2 * 64 + lane;
  u32x4 ghi[WG_NG], glo[WG_NG];
  auto load_g = [&](int slot, long g) {
    if (!active) return;
    const u32x4* p = gp + (size_t)(g < gend ? g : gend - 1) * 2 * 64;     // (past the end: the last pair again, unused)
    ghi[slot] = p[0];
    glo[slot] = p[64];
  };

  f32x16 acc[9], tot[9];
#pragma unroll
  for (int j = 0; j < 9; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = tot[j][r] = 0.f;

  // B operand of lane (q, lh): channel q of the tile, pixels 8 lh .. 8 lh + 7 of a k-step (the A fragment holds the same pixels of row q)
  GDF_LDS const char* xb = (GDF_LDS const char*)wg_smem + q * WG_CST + (WG_MARGIN + 8 * lh) * 2;

  int b = 0, y0 = 0, x0 = 0;
  load_x(0, 0, 0);
#pragma unroll
  for (int st = 0; st < WG_NG - 1; ++st) load_g(st, st);
  for (long k = 0; k < a.ntile; ++k) {
    store_x();
    lds_barrier();
    int bn = b, yn = y0, xn = x0 + WG_PW;                  // the next patch: along x, then y, then the image
    if (xn >= a.W) { xn = 0; yn += WG_PH; }
    if (yn >= a.H) { yn = 0; ++bn; }
    if (k + 1 < a.ntile) load_x(bn, yn, xn);
    if (active) {
#pragma unroll
      for (int st = 0; st < WG_KS; ++st) {
        load_g((st + WG_NG - 1) % WG_NG, k * WG_KS + st + WG_NG - 1);
        const f16x8 ahi = __builtin_bit_cast(f16x8, ghi[st % WG_NG]), alo = __builtin_bit_cast(f16x8, glo[st % WG_NG]);
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
          GDF_LDS const char* p = xb + ((st >> 1) + dy) * WG_PITCH + (st & 1) * 32;
          f16x8 xf[NIMG][3];
#pragma unroll
          for (int im = 0; im < NIMG; ++im) {
            const u32x4 c = *(GDF_LDS const u32x4*)(p + im * WG_IMG);
            const unsigned pv = *(GDF_LDS const unsigned*)(p + im * WG_IMG - 4), nx = *(GDF_LDS const unsigned*)(p + im * WG_IMG + 16);
            // pixel i - 1 / i + 1 in the place of pixel i: the 16-bit funnel shifts of neighbouring dwords
            const unsigned s0 = (pv >> 16) | (c[0] << 16), s1 = (c[0] >> 16) | (c[1] << 16), s2 = (c[1] >> 16) | (c[2] << 16),
                           s3 = (c[2] >> 16) | (c[3] << 16), s4 = (c[3] >> 16) | (nx << 16);
            const u32x4 lft = {s0, s1, s2, s3}, rgt = {s1, s2, s3, s4};
            xf[im][0] = __builtin_bit_cast(f16x8, lft);
            xf[im][1] = __builtin_bit_cast(f16x8, c);
            xf[im][2] = __builtin_bit_cast(f16x8, rgt);
          }
#pragma unroll
          for (int dx = 0; dx < 3; ++dx) acc[dy * 3 + dx] = __builtin_amdgcn_mfma_f32_32x32x16_f16(alo, xf[0][dx], acc[dy * 3 + dx], 0, 0, 0);
          if constexpr (F32) {
#pragma unroll
            for (int dx = 0; dx < 3; ++dx)
              acc[dy * 3 + dx] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi, xf[NIMG - 1][dx], acc[dy * 3 + dx], 0, 0, 0);
          }
#pragma unroll
          for (int dx = 0; dx < 3; ++dx) acc[dy * 3 + dx] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi, xf[0][dx], acc[dy * 3 + dx], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);                 // (a step's loads and conversions stay in the step)
      }
      // (unconditional: a fold every second patch keeps both sets of accumulators live across a branch and costs the registers that are left)
#pragma unroll
      for (int j = 0; j < 9; ++j) {
        tot[j] += acc[j];
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
      }
    }
    b = bn; y0 = yn; x0 = xn;
    lds_barrier();                                          // every wave has left the patch: the next one may be stored
  }

  // accumulator register r of lane (q, lh) is row 8 (r / 4) + 4 lh + r % 4 (the output channel), column q (the input channel); a lane's nine
  // taps are nine consecutive floats of dW
  if (!active) return;
  const int ci = ct * WG_CT + q;
  if (ci >= a.C) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = cb * WG_ROWS + w * 32 + (r >> 2) * 8 + lh * 4 + (r & 3);
    if (row >= a.Cout) continue;
    const int s = a.sh[row];
    float* o = a.dw + ((long)row * a.C + ci) * 9;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const float v = ldexpf(tot[tap][r], -s);
      o[tap] = a.accumulate ? o[tap] + v : v;
    }
  }
}

// [max |G| per output channel][shift per output channel][G's fragment image: 2 KB per 32-row block and k-step]
struct WgWs { float* mx; int* sh; u32x4* gs; size_t bytes; };
WgWs wg_carve(void* base, int B, int Cout, int H, int W) {
  const size_t nks = (size_t)B * ((W + WG_PW - 1) / WG_PW) * ((H + WG_PH - 1) / WG_PH) * WG_KS;
  Carver c(base);
  WgWs ws;
  ws.mx = c.take<float>((size_t)Cout * 4);
  ws.sh = c.take<int>((size_t)Cout * 4);
  ws.gs = c.take<u32x4>((size_t)((Cout + 31) / 32) * nks * 2 * 64 * 16);
  ws.bytes = c.bytes();
  return ws;
}

}  // namespace

size_t agghead_wgrad_workspace(int B, int Cout, int H, int W) { return wg_carve(nullptr, B, Cout, H, W).bytes; }

hipError_t launch_agghead_wgrad(const AggSrc& x, int B, const float* g, int Cout, float* dw, int accumulate, void* workspace, hipStream_t s) {
  if (!x.ptr || !g || !dw || !workspace || x.C < 1 || x.H < 1 || x.W < 1 || Cout < 1 || B < 0) return hipErrorInvalidValue;
  if ((long)B * x.H * x.W >= (1l << 31)) return hipErrorInvalidValue;
  if (B == 0) return hipSuccess;
  const WgWs ws = wg_carve(workspace, B, Cout, x.H, x.W);
  const int nct = (x.C + WG_CT - 1) / WG_CT, ncb = (Cout + WG_ROWS - 1) / WG_ROWS, nrb = (Cout + 31) / 32;
  const int tx = (x.W + WG_PW - 1) / WG_PW, ty = (x.H + WG_PH - 1) / WG_PH;
  const long ntile = (long)B * tx * ty, nks = ntile * WG_KS, nsplit = (long)nrb * nks * 64;
  if ((nsplit + 255) / 256 >= (1l << 31)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(wg_rowmax_kernel, dim3(Cout), dim3(256), 0, s, g, B, Cout, (long)x.H * x.W, ws.mx, ws.sh);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(wg_split_kernel, dim3((unsigned)((nsplit + 255) / 256)), dim3(256), 0, s, g, (const int*)ws.sh, Cout, x.H, x.W, tx, ty, nks,
                     nsplit, ws.gs);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  const long total = (long)ncb * nct, chunk = xcd_chunk(total);
  const WgArgs a{x.ptr, x.sb, x.sc, x.sy, x.sx, x.C, x.H, x.W, ws.gs, ws.sh, dw, Cout, nct, nrb, accumulate ? 1 : 0, ntile, (unsigned)chunk, total};
  const unsigned grid = (unsigned)(chunk * XCDS);
  if (x.f32) hipLaunchKernelGGL(wg_kernel<float>, dim3(grid), dim3(WG_NT), 0, s, a);
  else hipLaunchKernelGGL(wg_kernel<_Float16>, dim3(grid), dim3(WG_NT), 0, s, a);
  return hipGetLastError();
}

}  // namespace gdf
