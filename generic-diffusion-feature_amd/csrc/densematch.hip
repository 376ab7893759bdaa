// Dense matching of two feature maps, gfx950: for every pixel of map 1 its best pixel of map 2 by cosine similarity, and the reverse, from ONE
// pass over the P1 x P2 similarity matrix that never leaves the registers.
//
// Reference ops replaced (paths in the reference project):
//   correspondence/correspondence/correspondence_utils.py:73-111    batch_cosine_sim + find_nn_correspondences: both maps flattened and L2-normalised,
//   sims = f1 @ f2^T (B, P1, P2) fp32, argmax over the last axis
//   correspondence/correspondence/correspondence_utils.py:264-274   find_best_buddies_correspondences: the same matrix row by row in a Python loop
//   (chunk_cosine_sim), torch.max over both axes
//
//   dm_pack_kernel    one read of a map (any strides, fp16 or fp32) -> K-contiguous fp16 operand panels [pixel][channel], C zero-padded to DM_KPAD, the
//                     pixels zero-padded to DM_TILE, and r[p] fp32.  An fp16 map is copied raw, r = 1 / ||v||.  An fp32 map is normalised in fp32,
//                     scaled by DM_SCALE and split into an fp16 (hi, lo) pair of panels, r = 1 / DM_SCALE.  A pixel whose computed norm is not
//                     positive and finite gets r = 0: the flag.
//   dm_match_kernel   one workgroup = one 256 x 256 tile of the matrix, four waves of 128 x 128 (4 x 4 v_mfma_f32_32x32x16_f16 blocks, 256
//                     accumulator registers), fp32 accumulation over K in the one fixed order.  fp16 x fp16 is one product per K step; a (hi, lo)
//                     operand adds lo x hi (lo x lo is dropped).  Operands are staged through one 64 KB LDS image (K step 64, or 32 where a
//                     pair is staged); the next K step's 16-byte global loads are issued before the MFMAs of this one and wait in registers.
//                     The image is XOR-swizzled by row so that the 16-byte fragment reads of 16 consecutive lanes and the 16-byte staging
//                     writes both cover 256 distinct bytes of banks.  A wave reads 8 fragments per 16 MFMAs.
//                     Epilogue: s = (dot * r1[p1]) * r2[p2] once, in fp32; the row reduction and the column reduction both see these bits.
//                     Each wave reduces its 128 x 128 block to (score, lowest index) per row and per column and writes them as partials.
//   dm_fold_kernel    the partials of one row (column) folded in ascending order under the total order (higher score, then lower index).
// No atomics; every reduction has a fixed order or is a fold under a total order: the same inputs give the same bits.
#include <math.h>

#include <algorithm>
#include <type_traits>

#include "feat_common.h"

namespace gdf {

namespace {

enum { DM_PACK_P = 64 };                               // pixels of one pack workgroup
#define DM_SCALE 4096.f                                // an fp32 map's unit vectors are stored as fp16 pairs of DM_SCALE * v: lo stays clear of
                                                       // the fp16 subnormals down to |v| ~ 2^-25, hi <= 4096

// (best_take's scores are never NaN here: the epilogue replaces them by -inf)

// One workgroup = DM_PACK_P consecutive pixels (flattened y * W + x) of one sample, all channels in chunks of 64 through an LDS tile.  The tile is
// loaded with lanes along the channels where sc == 1 and along the pixels otherwise, and written out with lanes along the channels, 16 bytes each.
// Pixels in [P, Pp) and channels in [C, Kp) are written as zeros.  F32: a first sweep takes the norms, the second writes (hi, lo).
template <typename T, bool F32>
__global__ __launch_bounds__(256) void dm_pack_kernel(const T* __restrict__ f, long sb, long sc, long sy, long sx, int C, int W, int P, int Pp, int Kp,
                                                      _Float16* __restrict__ panel, float* __restrict__ r) {
  __shared__ float tile[64 * 65];
  const int t = threadIdx.x, b = blockIdx.y, p0 = blockIdx.x * DM_PACK_P;
  const T* fb = f + (long)b * sb;
  const bool lanes_c = sc == 1;
  // the store phase: pixel sp + 32 i, channels sc8 .. sc8 + 7 of the chunk
  const int sp = t >> 3, sc8 = (t & 7) * 8;
  float ss[2] = {0.f, 0.f}, rn[2] = {0.f, 0.f};
  _Float16* hi = panel + (long)b * (F32 ? 2 : 1) * Pp * Kp;
  _Float16* lo = hi + (long)Pp * Kp;
  // the load phase: element i of a thread is (channel c, pixel pl) of the chunk; the pixel's offset is taken once (-1: past the map)
  long poff[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int p = p0 + (lanes_c ? (t >> 6) + 4 * i : (t & 63));
    const int y = p / W, x = p - y * W;
    poff[i] = p < P ? (long)y * sy + (long)x * sx : -1;
  }
  for (int sweep = 0; sweep < (F32 ? 2 : 1); ++sweep) {
    const bool write = !F32 || sweep == 1;
    for (int c0 = 0; c0 < Kp; c0 += 64) {
      __syncthreads();
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int a = t & 63, g = (t >> 6) + 4 * i;
        const int c = lanes_c ? a : g, pl = lanes_c ? g : a;
        float v = 0.f;
        if (poff[i] >= 0 && c0 + c < C) v = (float)fb[poff[i] + (long)(c0 + c) * sc];
        tile[c * 65 + pl] = v;
      }
      __syncthreads();
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int pl = sp + 32 * i;
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = tile[(sc8 + e) * 65 + pl];
        if (!F32 || sweep == 0) {
#pragma unroll
          for (int e = 0; e < 8; ++e) ss[i] = fmaf(v[e], v[e], ss[i]);
        }
        if (write) {
          const long o = (long)(p0 + pl) * Kp + c0 + sc8;
          f16x8 h, l;
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            if (F32) {
              const float w = (v[e] * rn[i]) * DM_SCALE;
              h[e] = (_Float16)w;
              l[e] = (_Float16)(w - (float)h[e]);
            } else {
              h[e] = (_Float16)v[e];
            }
          }
          *(f16x8*)(hi + o) = h;
          if (F32) *(f16x8*)(lo + o) = l;
        }
      }
    }
    if (!F32 || sweep == 0) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int off = 1; off <= 4; off <<= 1) ss[i] += __shfl_xor(ss[i], off);
        const float q = 1.f / sqrtf(ss[i]);
        rn[i] = (ss[i] > 0.f && q > 0.f && q < INFINITY) ? q : 0.f;
      }
    }
  }
  if ((t & 7) == 0) {
#pragma unroll
    for (int i = 0; i < 2; ++i) r[(long)b * Pp + p0 + sp + 32 * i] = F32 ? (rn[i] > 0.f ? 1.f / DM_SCALE : 0.f) : rn[i];
  }
}

// One workgroup = tile (ty, tx) of sample blockIdx.y, four waves of 128 x 128 each.  Panels: A (B, N1, P1p, Kp), Bm (B, N2, P2p, Kp) fp16;
// r1 (B, P1p), r2 (B, P2p).  Row partials prs / pri (B, 2 ntx, P1p): best column of the 128 columns a wave saw; column partials pcs / pci
// (B, 2 nty, P2p) likewise.  Workgroup ids are dealt round-robin to the eight XCDs; where the tile count is a multiple of 8 every XCD gets a
// contiguous eighth of the tiles, and in any case consecutive tiles walk 8 tile rows of one tile column first: the workgroups in flight on an
// XCD share operand panels in its L2.
template <int N1, int N2, int BK>
__global__ __launch_bounds__(256) void dm_match_kernel(const _Float16* __restrict__ A, const _Float16* __restrict__ Bm, const float* __restrict__ r1,
                                                       const float* __restrict__ r2, int P1p, int P2p, int Kp, int ntx, int nty, float* prs, int* pri,
                                                       float* pcs, int* pci, int do_rows, int do_cols) {
  constexpr int CH = BK / 8;                          // 16-byte chunks of a staged row
  constexpr int RP = 16 / CH;                         // rows per 256 bytes of LDS
  constexpr int NP = N1 + N2;                         // staged panels: [A hi, A lo][B hi, B lo]
  constexpr int PT = DM_TILE * CH;                    // chunks of one staged panel tile
  constexpr int LD = PT / 256;                        // chunks a thread moves per panel
  __shared__ u32x4 lds[NP * PT];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, wm = wv >> 1, wn = wv & 1;
  const int r = lane & 31, h = lane >> 5, b = blockIdx.y;
  const int nt = ntx * nty;
  const int id = (nt & 7) ? (int)blockIdx.x : (int)(blockIdx.x & 7) * (nt >> 3) + (int)(blockIdx.x >> 3);
  const int band = id / (DM_GROUP * ntx), first = band * DM_GROUP, gsz = min((int)DM_GROUP, nty - first), rem = id - band * DM_GROUP * ntx;
  const int ty = first + rem % gsz, tx = rem / gsz;
  const long row0 = (long)ty * DM_TILE, col0 = (long)tx * DM_TILE;
  const _Float16* pa = A + ((long)b * N1 * P1p + row0) * Kp;
  const _Float16* pb = Bm + ((long)b * N2 * P2p + col0) * Kp;

  u32x4 stage[NP][LD];
  auto load_global = [&](int k0) {
#pragma unroll
    for (int n = 0; n < NP; ++n) {
      const _Float16* src = n < N1 ? pa + (long)n * P1p * Kp : pb + (long)(n - N1) * P2p * Kp;
#pragma unroll
      for (int i = 0; i < LD; ++i) {
        const int q = t + 256 * i, row = q / CH, ch = q % CH;
        stage[n][i] = *(const u32x4*)(src + (long)row * Kp + k0 + ch * 8);
      }
    }
  };
  auto store_lds = [&]() {
#pragma unroll
    for (int n = 0; n < NP; ++n)
#pragma unroll
      for (int i = 0; i < LD; ++i) {
        const int q = t + 256 * i, row = q / CH, ch = q % CH;
        lds[n * PT + row * CH + (ch ^ ((row / RP) & (CH - 1)))] = stage[n][i];
      }
  };

  f32x16 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  // One LDS image, the next K step in registers: its global loads are issued as soon as this step's image is complete and fly under the MFMAs.
  const int nk = Kp / BK;
  load_global(0);
  store_lds();
  __syncthreads();
  for (int ks = 0; ks < nk; ++ks) {
    load_global(min(ks + 1, nk - 1) * BK);            // (unconditional: the last step loads its own slice again, and nothing reads that image)
#pragma unroll
    for (int kk = 0; kk < BK / 16; ++kk) {
      const int ch = kk * 2 + h;
      f16x8 fa[N1][4], fb[N2][4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = wm * 128 + i * 32 + r;
        const int o = row * CH + (ch ^ ((row / RP) & (CH - 1)));
#pragma unroll
        for (int n = 0; n < N1; ++n) fa[n][i] = __builtin_bit_cast(f16x8, lds[n * PT + o]);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = wn * 128 + j * 32 + r;
        const int o = row * CH + (ch ^ ((row / RP) & (CH - 1)));
#pragma unroll
        for (int n = 0; n < N2; ++n) fb[n][j] = __builtin_bit_cast(f16x8, lds[(N1 + n) * PT + o]);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if constexpr (N1 == 2) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[N1 - 1][i], fb[0][j], acc[i][j], 0, 0, 0);
          if constexpr (N2 == 2) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[0][i], fb[N2 - 1][j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[0][i], fb[0][j], acc[i][j], 0, 0, 0);
        }
    }
    __syncthreads();                                  // every wave has read this image
    store_lds();
    __syncthreads();
  }

  // ---- epilogue: acc[i][j][reg] is row wm 128 + 32 i + (reg & 3) + 8 (reg >> 2) + 4 h, column wn 128 + 32 j + r of the tile ----
  const float* r1b = r1 + (long)b * P1p + row0 + wm * 128;
  const float* r2b = r2 + (long)b * P2p + col0 + wn * 128;
  float c2[4], cs[4];
  int gc[4], ci[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    c2[j] = r2b[j * 32 + r];
    gc[j] = (int)col0 + wn * 128 + j * 32 + r;
    cs[j] = -INFINITY;
    ci[j] = 0;
  }
  float os[2] = {-INFINITY, -INFINITY};               // the row results this lane stores: slot s is i = 2 s + (r >> 4), reg = r & 15
  int oi[2] = {0, 0};
  auto row_block = [&](auto ic) {                     // (one call per i: the compiler's unroll budget does not cover all 64 rows as one nest)
    constexpr int i = decltype(ic)::value;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int row = i * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
      const float ra = r1b[row];
      const int gr = (int)row0 + wm * 128 + row;
      float s = -INFINITY;
      int ix = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float v = (acc[i][j][reg] * ra) * c2[j];
        v = (ra > 0.f && c2[j] > 0.f && v == v) ? v : -INFINITY;
        if (do_cols) best_take(cs[j], ci[j], v, gr);
        if (j == 0) { s = v; ix = gc[0]; }
        else best_take(s, ix, v, gc[j]);
      }
      if (do_rows) {
#pragma unroll
        for (int off = 16; off >= 1; off >>= 1) {
          const float ts = __shfl_xor(s, off);
          const int ti = __shfl_xor(ix, off);
          best_take(s, ix, ts, ti);
        }
        if (r == (i & 1) * 16 + reg) { os[i >> 1] = s; oi[i >> 1] = ix; }
      }
    }
  };
  row_block(std::integral_constant<int, 0>());
  row_block(std::integral_constant<int, 1>());
  row_block(std::integral_constant<int, 2>());
  row_block(std::integral_constant<int, 3>());
  if (do_rows) {
#pragma unroll
    for (int sl = 0; sl < 2; ++sl) {
      const int reg = r & 15, row = (2 * sl + (r >> 4)) * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
      const long o = ((long)b * 2 * ntx + 2 * tx + wn) * P1p + row0 + wm * 128 + row;
      prs[o] = os[sl];
      pri[o] = oi[sl];
    }
  }
  if (do_cols) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float ts = __shfl_xor(cs[j], 32);
      const int ti = __shfl_xor(ci[j], 32);
      best_take(cs[j], ci[j], ts, ti);
    }
    const long o = ((long)b * 2 * nty + 2 * ty + wm) * P2p + col0 + wn * 128;
    if (h == 0) {                                     // (both halves hold the same four results; static indices keep them in registers)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        pcs[o + j * 32 + r] = cs[j];
        pci[o + j * 32 + r] = ci[j];
      }
    }
  }
}

// One thread = one row (column) of one sample: its nparts partials, ascending.  A row no pixel answered gets index 0 and a NaN score.
__global__ __launch_bounds__(256) void dm_fold_kernel(const float* __restrict__ ps, const int* __restrict__ pi, int nparts, int P, int Pp, int* nn,
                                                      float* sim) {
  const int p = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (p >= P) return;
  float s = -INFINITY;
  int i = 0;
  for (int k = 0; k < nparts; ++k) {
    const long o = ((long)b * nparts + k) * Pp + p;
    best_take(s, i, ps[o], pi[o]);
  }
  const bool none = s == -INFINITY;
  nn[(long)b * P + p] = none ? 0 : i;
  sim[(long)b * P + p] = none ? NAN : s;
}

long dm_pad(long v, long m) { return (v + m - 1) / m * m; }

struct DmWs { _Float16 *a, *b; float *r1, *r2, *prs; int* pri; float* pcs; int* pci; size_t bytes; };
DmWs dm_carve(void* base, int B, int C, long P1, long P2, int f32_1, int f32_2) {
  const size_t P1p = (size_t)dm_pad(P1, DM_TILE), P2p = (size_t)dm_pad(P2, DM_TILE), Kp = (size_t)dm_pad(C, DM_KPAD), nb = (size_t)B;
  const size_t ntx = P2p / DM_TILE, nty = P1p / DM_TILE;
  Carver c(base);
  DmWs w;
  w.a = c.take<_Float16>(nb * (f32_1 ? 2 : 1) * P1p * Kp * 2);
  w.b = c.take<_Float16>(nb * (f32_2 ? 2 : 1) * P2p * Kp * 2);
  w.r1 = c.take<float>(nb * P1p * 4);
  w.r2 = c.take<float>(nb * P2p * 4);
  w.prs = c.take<float>(nb * 2 * ntx * P1p * 4);
  w.pri = c.take<int>(nb * 2 * ntx * P1p * 4);
  w.pcs = c.take<float>(nb * 2 * nty * P2p * 4);
  w.pci = c.take<int>(nb * 2 * nty * P2p * 4);
  w.bytes = c.bytes();
  return w;
}

void dm_pack(const AggSrc& f, int B, int P, int Pp, int Kp, _Float16* panel, float* r, hipStream_t s) {
  const dim3 grid((unsigned)(Pp / DM_PACK_P), (unsigned)B);
  if (f.f32)
    hipLaunchKernelGGL((dm_pack_kernel<float, true>), grid, dim3(256), 0, s, (const float*)f.ptr, f.sb, f.sc, f.sy, f.sx, f.C, f.W, P, Pp, Kp, panel, r);
  else
    hipLaunchKernelGGL((dm_pack_kernel<_Float16, false>), grid, dim3(256), 0, s, (const _Float16*)f.ptr, f.sb, f.sc, f.sy, f.sx, f.C, f.W, P, Pp, Kp,
                       panel, r);
}

template <int N1, int N2, int BK>
void dm_match(const DmWs& ws, int B, int P1p, int P2p, int Kp, bool rows, bool cols, hipStream_t s) {
  const int ntx = P2p / DM_TILE, nty = P1p / DM_TILE;
  hipLaunchKernelGGL((dm_match_kernel<N1, N2, BK>), dim3((unsigned)(ntx * nty), (unsigned)B), dim3(256), 0, s, ws.a, ws.b, ws.r1, ws.r2, P1p, P2p, Kp,
                     ntx, nty, ws.prs, ws.pri, ws.pcs, ws.pci, (int)rows, (int)cols);
}

}  // namespace

size_t dense_match_workspace(int B, int C, long P1, long P2, int f32_1, int f32_2) { return dm_carve(nullptr, B, C, P1, P2, f32_1, f32_2).bytes; }

hipError_t launch_dense_match(const AggSrc& f1, const AggSrc& f2, int B, int* nn12, float* sim12, int* nn21, float* sim21, void* workspace,
                              hipStream_t s) {
  if (!f1.ptr || !f2.ptr || !workspace || ((uintptr_t)workspace & 15)) return hipErrorInvalidValue;
  if (B < 0 || B > 65535 || f1.C < 1 || f1.C != f2.C || f1.H < 1 || f1.W < 1 || f2.H < 1 || f2.W < 1) return hipErrorInvalidValue;
  const bool rows = nn12 && sim12, cols = nn21 && sim21;
  if ((!nn12) != (!sim12) || (!nn21) != (!sim21) || (!rows && !cols)) return hipErrorInvalidValue;
  const long P1 = (long)f1.H * f1.W, P2 = (long)f2.H * f2.W;
  if (P1 > DM_MAXP || P2 > DM_MAXP) return hipErrorInvalidValue;
  const long P1p = dm_pad(P1, DM_TILE), P2p = dm_pad(P2, DM_TILE), Kp = dm_pad(f1.C, DM_KPAD);
  if ((P1p / DM_TILE) * (P2p / DM_TILE) >= (1l << 31)) return hipErrorInvalidValue;
  if (B == 0) return hipSuccess;
  const DmWs ws = dm_carve(workspace, B, f1.C, P1, P2, f1.f32, f2.f32);
  dm_pack(f1, B, (int)P1, (int)P1p, (int)Kp, ws.a, ws.r1, s);
  dm_pack(f2, B, (int)P2, (int)P2p, (int)Kp, ws.b, ws.r2, s);
  if (!f1.f32 && !f2.f32) dm_match<1, 1, 64>(ws, B, (int)P1p, (int)P2p, (int)Kp, rows, cols, s);
  else if (f1.f32 && !f2.f32) dm_match<2, 1, 32>(ws, B, (int)P1p, (int)P2p, (int)Kp, rows, cols, s);
  else if (!f1.f32 && f2.f32) dm_match<1, 2, 32>(ws, B, (int)P1p, (int)P2p, (int)Kp, rows, cols, s);
  else dm_match<2, 2, 32>(ws, B, (int)P1p, (int)P2p, (int)Kp, rows, cols, s);
  if (rows)
    hipLaunchKernelGGL(dm_fold_kernel, dim3((unsigned)((P1 + 255) / 256), (unsigned)B), dim3(256), 0, s, ws.prs, ws.pri, (int)(2 * (P2p / DM_TILE)),
                       (int)P1, (int)P1p, nn12, sim12);
  if (cols)
    hipLaunchKernelGGL(dm_fold_kernel, dim3((unsigned)((P2 + 255) / 256), (unsigned)B), dim3(256), 0, s, ws.pcs, ws.pci, (int)(2 * (P1p / DM_TILE)),
                       (int)P2, (int)P2p, nn21, sim21);
  return hipGetLastError();
}

}  // namespace gdf
