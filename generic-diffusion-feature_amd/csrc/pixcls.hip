// Pixel-classifier ensemble of the label-scarce segmentation evaluator on an aggregated feature map, gfx950.
//
// Reference op replaced (paths under /root/reference):
//   scarce_segmentation/segmentation/pixel_classifier.py:14-36    pixel_classifier: Linear(dim, h1) ReLU BatchNorm1d Linear(h1, h2) ReLU BatchNorm1d
//                                                                 Linear(h2, classes), (h1, h2) = (128, 32), from 30 classes up (256, 128)
//   scarce_segmentation/segmentation/pixel_classifier.py:70-107   predict_labels: every model of the ensemble over every pixel, per-model argmax,
//                                                                 Categorical entropies, mean softmax, Jensen-Shannon uncertainty, torch.mode
//
// The networks arrive BatchNorm-folded (eval-mode BatchNorm1d after ReLU is affine and folds into the next Linear; components/postproc.py does
// it in fp64), so a model is W3 relu(W2 relu(W1 x + b1) + b2) + b3.  Two kernels:
//   pc_mlp_kernel   one workgroup = 128 pixels x one model.  Layer 1 on v_mfma_f32_32x32x16_f16 with fp32 accumulation: W1 is an fp16 (hi, lo)
//                   pair per element, rows scaled by a power of two that the fp32 epilogue undoes; an fp16 map is multiplied as given (x hi, x lo:
//                   two passes on one x fragment), an fp32 map is split into (hi, lo) as it is staged (three passes, lo lo dropped).  x tiles are
//                   staged [channel][pixel] in LDS and read as the B operand with the transposed LDS read; W1 tiles are packed in fragment order at
//                   creation and copied as they are.  Layer 2 runs on the MFMA units too, on the workgroup's own hidden tile: hidden 1 as an fp16 (hi, lo)
//                   pair in LDS, W2 as a scaled (hi, lo) pair, three products; layer 3 is fp32 FMAs on hidden 2 (fp32 in LDS).  No hidden value
//                   is ever a single 16-bit number and the hidden tensors never reach memory.  Output: fp32 logits (M, P, K).
//   pc_vote_kernel  one thread per pixel: per model log-softmax, lowest-index argmax and entropy; the renormalised mean softmax, its entropy as
//                   Categorical(probs) computes it, js = H(mean) - mean H_m, and the most frequent label (the smallest among equally frequent).
// Workgroups are numbered so that the M models of one pixel tile follow one another ON ONE XCD (they share the tile's x through that XCD's L2).
// No atomics, fixed summation orders, stream-ordered, nothing read back, no allocation in a launch.
#include <math.h>

#include <algorithm>
#include <vector>

#include "feat_common.h"

namespace gdf {

namespace {

typedef __fp16 pc_fp16x4 __attribute__((__vector_size__(4 * sizeof(__fp16))));

enum {
  PC_BP = 128,           // pixels per workgroup
  PC_KT = 32,            // channels per staged tile (two MFMA k-steps)
  PC_LDX = 160,          // halves per [channel] row of the x image: 128 pixels + 64 bytes, an odd multiple of 64 bytes (conflict-free transposed reads)
  PC_NT = 256,           // threads: four waves, wave w = pixel half (w & 1) x hidden half (w >> 1)
  PC_XIMG = PC_KT * PC_LDX * 2,      // bytes of one x image
};

// k of element e of the fragment of lane half lh within a 16-channel step: what ds_read_b64_tr_b16 hands out (rows 4 lh + e, then 8 + 4 lh + e - 4)
constexpr int pc_perm(int lh, int e) { return e < 4 ? 4 * lh + e : 8 + 4 * lh + (e - 4); }

struct PcArgs {
  const void* x; long sb, sc, sy, sx; int C, H, W; long P;
  const u32x4* w1; const float *inv_s, *b1; const u32x4* w2; const float *inv_s2, *b2, *w3, *b3;
  float* logits; int M, K, nkt; unsigned chunk; long total;
};

// T: the map's element type.  H1P / H2P: the hidden widths padded to (128, 32) or (256, 128) with zero weights.  CL: channels-last map (sc == 1,
// C a multiple of the 16-byte vector, aligned pixels): 16-byte loads along C; otherwise one element per load with the map's own strides, lanes
// along the flattened pixel index (coalesced where sx == 1).
template <typename T, int H1P, int H2P, bool CL>
__global__ __launch_bounds__(PC_NT) void pc_mlp_kernel(const PcArgs a) {
  constexpr bool F32 = sizeof(T) == 4;
  constexpr int NIMG = F32 ? 2 : 1;              // x images in LDS: hi (and lo)
  constexpr int NRB = H1P / 32;                  // 32-row blocks of W1 per model
  constexpr int NBW = NRB / 2;                   // ... per wave
  constexpr int WT16 = NRB * 2 * 2 * 64;         // 16-byte chunks of one W1 tile: [k-step 2][row block][hi, lo][lane]
  constexpr int NWR = WT16 / PC_NT;              // ... per thread
  constexpr int V = MapVec<T>::V;
  constexpr int NCH = PC_KT / V / 2;             // CL: 16-byte chunks per thread and tile
  typedef typename MapVec<T>::type vt;
  extern __shared__ __attribute__((aligned(16))) char pc_smem[];
  char* sW = pc_smem;
  char* sX = pc_smem + WT16 * 16;

  // (tile, model) of this workgroup: consecutive numbers on one XCD
  const long L = xcd_slot(blockIdx.x, a.chunk);
  if (L >= a.total) return;                      // (whole workgroups, before any barrier)
  const int m = (int)(L % a.M);
  const long tile = L / a.M;

  const int t = threadIdx.x, lane = t & 63, w = __builtin_amdgcn_readfirstlane(t >> 6), lh = lane >> 5, i16 = lane & 15;
  const int px = t & 127, kr = __builtin_amdgcn_readfirstlane(t >> 7);
  const long gp = tile * PC_BP + px;
  long xoff;
  {
    const long pp = gp < a.P ? gp : a.P - 1;     // pixels past the map load a valid pixel and store nothing
    const long hw = (long)a.H * a.W;
    const long b = pp / hw, r = pp - b * hw;
    const long y = r / a.W, xx = r - y * a.W;
    xoff = b * a.sb + y * a.sy + xx * a.sx;
  }
  const T* xp = (const T*)a.x + xoff;
  const u32x4* wp = a.w1 + (long)m * a.nkt * WT16;

  T xe[CL ? 1 : 16];
  vt xv[CL ? NCH : 1];
  u32x4 wr[NWR];
  auto load_tile = [&](int kt) {
    if constexpr (CL) {
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        const int c0 = kt * PC_KT + (kr + 2 * i) * V;
        xv[i] = c0 < a.C ? *(const vt*)(xp + c0) : (vt)(T)0;
      }
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int c = kt * PC_KT + kr + 2 * i;
        xe[i] = c < a.C ? xp[(long)c * a.sc] : (T)0;
      }
    }
#pragma unroll
    for (int i = 0; i < NWR; ++i) wr[i] = wp[(long)kt * WT16 + t + PC_NT * i];
  };
  auto put = [&](int k, T v) {                   // channel k of the tile, this thread's pixel
    _Float16* hi = (_Float16*)sX + k * PC_LDX + px;
    if constexpr (F32) {
      const _Float16 h = f32_to_f16_sat(v);
      *hi = h;
      *(_Float16*)((char*)hi + PC_XIMG) = f32_to_f16_sat(v - (float)h);
    } else {
      *hi = v;
    }
  };
  auto store_tile = [&]() {
    if constexpr (CL) {
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
#pragma unroll
        for (int j = 0; j < V; ++j) put((kr + 2 * i) * V + j, xv[i][j]);
      }
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i) put(kr + 2 * i, xe[i]);
    }
#pragma unroll
    for (int i = 0; i < NWR; ++i) *(u32x4*)(sW + (t + PC_NT * i) * 16) = wr[i];
  };

  f32x16 acc[2][NBW];
#pragma unroll
  for (int pb = 0; pb < 2; ++pb)
#pragma unroll
    for (int cb = 0; cb < NBW; ++cb)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[pb][cb][r] = 0.f;

  // transposed read: lane 4 q + p of a 16-lane group names row q, columns 4 p .. 4 p + 3 of a 4 x 16 block; the lane's two groups of a half
  // take pixel columns 0-15 and 16-31 of the 32-pixel block
  GDF_LDS const char* xl = (GDF_LDS const char*)sX + ((4 * lh + (i16 >> 2)) * PC_LDX + (w & 1) * 64 + 16 * ((lane >> 4) & 1) + (i16 & 3) * 4) * 2;
  const char* wl = sW + ((w >> 1) * NBW * 2 * 64 + lane) * 16;

  load_tile(0);
  for (int kt = 0; kt < a.nkt; ++kt) {
    __syncthreads();
    store_tile();
    __syncthreads();
    if (kt + 1 < a.nkt) load_tile(kt + 1);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      f16x8 xf[NIMG][2];
#pragma unroll
      for (int im = 0; im < NIMG; ++im)
#pragma unroll
        for (int pb = 0; pb < 2; ++pb) {
          GDF_LDS const char* p = xl + im * PC_XIMG + (16 * s * PC_LDX + pb * 32) * 2;
          union { pc_fp16x4 q[2]; f16x8 h; } u;
          u.q[0] = __builtin_amdgcn_ds_read_tr16_b64_v4f16((GDF_LDS pc_fp16x4*)p);
          u.q[1] = __builtin_amdgcn_ds_read_tr16_b64_v4f16((GDF_LDS pc_fp16x4*)(p + 8 * PC_LDX * 2));
          xf[im][pb] = u.h;
        }
#pragma unroll
      for (int cb = 0; cb < NBW; ++cb) {
        const char* q = wl + (s * NRB + cb) * 2 * 64 * 16;
        const f16x8 whi = *(const f16x8*)q, wlo = *(const f16x8*)(q + 64 * 16);
#pragma unroll
        for (int pb = 0; pb < 2; ++pb) {
          acc[pb][cb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wlo, xf[0][pb], acc[pb][cb], 0, 0, 0);
          if constexpr (F32) acc[pb][cb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(whi, xf[NIMG - 1][pb], acc[pb][cb], 0, 0, 0);
          acc[pb][cb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(whi, xf[0][pb], acc[pb][cb], 0, 0, 0);
        }
      }
    }
  }

  // Layer 2 on the MFMA units as well, fp32-exact in the sense of layer 1: hidden 1 = relu(acc / scale + b1) goes to LDS as an fp16 (hi, lo) pair
  // of images [hidden unit][pixel] (the layout of the x tiles, read transposed as the B operand), 128 hidden units at a time; W2 is a scaled
  // (hi, lo) pair in fragment order, read from memory; three products (lo lo dropped).  Accumulator register r of lane (q = lane % 32, lh) is
  // row 8 (r / 4) + 4 lh + r % 4 (the hidden unit), column q (the pixel).
  constexpr int NCHK = H1P / 128;                // chunks of 128 hidden units
  constexpr int T2 = H2P == 32 ? 1 : 2;          // layer-2 tile of a wave: T2 pixel blocks x T2 row blocks of 32
  constexpr int NJB = H2P / 32;
  const int pb2 = H2P == 32 ? w : (w & 1) * 2, jb2 = H2P == 32 ? 0 : (w >> 1) * 2;
  f32x16 acc2[T2][T2];
#pragma unroll
  for (int i = 0; i < T2; ++i)
#pragma unroll
    for (int j = 0; j < T2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc2[i][j][r] = 0.f;
  constexpr int HIMG = 128 * PC_LDX * 2;         // bytes of one hidden image
  GDF_LDS const char* hl = (GDF_LDS const char*)pc_smem + ((4 * lh + (i16 >> 2)) * PC_LDX + pb2 * 32 + 16 * ((lane >> 4) & 1) + (i16 & 3) * 4) * 2;
  const u32x4* w2p = a.w2 + (long)m * (H1P / 16) * NJB * 2 * 64 + lane;
#pragma unroll
  for (int ch = 0; ch < NCHK; ++ch) {
    __syncthreads();                             // the staging tiles (the previous chunk) have been read
    if (NCHK == 1 || (w >> 1) == ch) {           // (wave-uniform)
#pragma unroll
      for (int cb = 0; cb < NBW; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = (NCHK == 1 ? (w >> 1) * 64 : 0) + cb * 32 + (r >> 2) * 8 + lh * 4 + (r & 3);
          const int n = ch * 128 + row;
          const float is = a.inv_s[m * H1P + n], bb = a.b1[m * H1P + n];
#pragma unroll
          for (int pb = 0; pb < 2; ++pb) {
            const float h = fmaxf(acc[pb][cb][r] * is + bb, 0.f);
            const _Float16 hh = f32_to_f16_sat(h);   // (saturating: a hidden value beyond twice the fp16 range loses accuracy, not finiteness)
            _Float16* d = (_Float16*)pc_smem + row * PC_LDX + (w & 1) * 64 + pb * 32 + (lane & 31);
            *d = hh;
            *(_Float16*)((char*)d + HIMG) = f32_to_f16_sat(h - (float)hh);
          }
        }
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      f16x8 hf[2][T2];
#pragma unroll
      for (int im = 0; im < 2; ++im)
#pragma unroll
        for (int i = 0; i < T2; ++i) {
          GDF_LDS const char* p = hl + im * HIMG + (16 * s * PC_LDX + i * 32) * 2;
          union { pc_fp16x4 q[2]; f16x8 h; } u;
          u.q[0] = __builtin_amdgcn_ds_read_tr16_b64_v4f16((GDF_LDS pc_fp16x4*)p);
          u.q[1] = __builtin_amdgcn_ds_read_tr16_b64_v4f16((GDF_LDS pc_fp16x4*)(p + 8 * PC_LDX * 2));
          hf[im][i] = u.h;
        }
#pragma unroll
      for (int j = 0; j < T2; ++j) {
        const u32x4* q = w2p + (((long)(ch * 8 + s) * NJB + jb2 + j) * 2) * 64;
        const f16x8 whi = __builtin_bit_cast(f16x8, q[0]), wlo = __builtin_bit_cast(f16x8, q[64]);
#pragma unroll
        for (int i = 0; i < T2; ++i) {
          acc2[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wlo, hf[0][i], acc2[i][j], 0, 0, 0);
          acc2[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(whi, hf[1][i], acc2[i][j], 0, 0, 0);
          acc2[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(whi, hf[0][i], acc2[i][j], 0, 0, 0);
        }
      }
    }
  }
  // hidden 2 = relu(acc2 / scale + b2) -> LDS [unit][pixel] fp32
  __syncthreads();
  float* Hs = (float*)pc_smem;
#pragma unroll
  for (int j = 0; j < T2; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int u = (jb2 + j) * 32 + (r >> 2) * 8 + lh * 4 + (r & 3);
      const float is = a.inv_s2[m * H2P + u], bb = a.b2[m * H2P + u];
#pragma unroll
      for (int i = 0; i < T2; ++i) Hs[u * PC_BP + (pb2 + i) * 32 + (lane & 31)] = fmaxf(acc2[i][j][r] * is + bb, 0.f);
    }
  __syncthreads();

  // layer 3: the classes in two halves
  const int kh = (a.K + 1) / 2, c0 = kr * kh, c1 = min(a.K, c0 + kh);
  for (int c = c0; c < c1; ++c) {
    const float* wq = a.w3 + ((long)m * a.K + c) * H2P;
    float v = a.b3[m * a.K + c];
#pragma unroll 8
    for (int j = 0; j < H2P; ++j) v = fmaf(Hs[j * PC_BP + px], wq[j], v);
    if (gp < a.P) a.logits[((long)m * a.P + gp) * a.K + c] = v;
  }
}

// One thread per pixel over the logits (M, P, K); mean softmax and per-model labels of the block's 128 pixels live in LDS.
__global__ __launch_bounds__(128) void pc_vote_kernel(const float* logits, int M, int K, long P, long long* labels, float* js, unsigned char* mlab) {
  __shared__ float mean[PC_MAXK][128];
  __shared__ int lab[PC_MAXM][128];
  const int t = threadIdx.x;
  const long p = (long)blockIdx.x * 128 + t, pp = p < P ? p : P - 1;
  for (int c = 0; c < K; ++c) mean[c][t] = 0.f;
  float hsum = 0.f;
  for (int m = 0; m < M; ++m) {
    const float* l = logits + ((long)m * P + pp) * K;
    float mx = l[0];
    int am = 0;
    for (int c = 1; c < K; ++c) {
      const float v = l[c];
      if (v > mx) { mx = v; am = c; }            // strict: the lowest index among equal maxima
    }
    float s = 0.f;
    for (int c = 0; c < K; ++c) s += expf(l[c] - mx);
    const float ls = logf(s);
    float h = 0.f;
    for (int c = 0; c < K; ++c) {
      const float lp = fmaxf((l[c] - mx) - ls, -3.402823466e38f);          // Categorical clamps its logits at the lowest finite number
      const float pr = expf(lp);
      h -= pr * lp;
      mean[c][t] += pr;
    }
    hsum += h;
    lab[m][t] = am;
    if (mlab && p < P) mlab[(long)m * P + p] = (unsigned char)am;
  }
  float tot = 0.f;
  for (int c = 0; c < K; ++c) {
    const float q = mean[c][t] / (float)M;
    mean[c][t] = q;
    tot += q;
  }
  const float eps = 1.1920928955078125e-07f;
  float H = 0.f;
  for (int c = 0; c < K; ++c) {
    const float q = mean[c][t] / tot;
    H -= q * logf(fminf(fmaxf(q, eps), 1.f - eps));
  }
  int bl = 0, bc = 0;
  for (int m = 0; m < M; ++m) {
    const int v = lab[m][t];
    int cnt = 0;
    for (int k = 0; k < M; ++k) cnt += lab[k][t] == v ? 1 : 0;
    if (cnt > bc || (cnt == bc && v < bl)) { bc = cnt; bl = v; }
  }
  if (p < P) {
    labels[p] = bl;
    if (js) js[p] = H - hsum / (float)M;
  }
}

float pc_half_value(uint16_t h) {
  const int e = (h >> 10) & 31, f = h & 1023;
  const float v = e ? ldexpf((float)(f | 1024), e - 25) : ldexpf((float)f, -24);
  return (h & 0x8000) ? -v : v;
}

template <typename T, int H1P, int H2P, bool CL>
hipError_t pc_launch(const PcArgs& a, unsigned grid, hipStream_t s) {
  constexpr int stage = (H1P / 32) * 4096 + (sizeof(T) == 4 ? 2 : 1) * PC_XIMG, hid = 2 * 128 * PC_LDX * 2;   // (hid >= H2P * PC_BP * 4 too)
  constexpr int smem = stage > hid ? stage : hid;
  static std::atomic<uint64_t> raised{0};
  const hipError_t e = ensure_dyn_smem(raised, (const void*)pc_mlp_kernel<T, H1P, H2P, CL>, smem);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((pc_mlp_kernel<T, H1P, H2P, CL>), dim3(grid), dim3(PC_NT), smem, s, a);
  return hipGetLastError();
}

template <typename T, bool CL>
hipError_t pc_launch_nets(const PixCls* pc, const PcArgs& a, unsigned grid, hipStream_t s) {
  return pc->H1P == 128 ? pc_launch<T, 128, 32, CL>(a, grid, s) : pc_launch<T, 256, 128, CL>(a, grid, s);
}

// One model's weight matrix src (rows x cols, row-major) as MFMA A-operand fragments: each row scaled by the power of two that puts its largest
// magnitude into [2^13, 2^14) (so the low half stays clear of the fp16 subnormals), split into fp16 hi = fp16(v), lo = fp16(v - hi), and laid out
// [16-column step][32-row block of RB][hi, lo][lane][8] with a lane's eight columns in the transposed LDS read's order (pc_perm).  dst holds
// `steps` steps (columns from `cols` up and rows from `rows` up are zero); inv[r] = 1 / scale of row r.
void pc_pack_pairs(const float* src, int rows, int cols, int RB, int steps, uint16_t* dst, float* inv) {
  std::vector<uint16_t> hi((size_t)steps * 16), lo((size_t)steps * 16);
  for (int n = 0; n < RB * 32; ++n) {
    inv[n] = 1.f;
    if (n >= rows) continue;
    const float* row = src + (size_t)n * cols;
    float mx = 0.f;
    for (int c = 0; c < cols; ++c) mx = std::max(mx, fabsf(row[c]));
    const int sh = split_shift(mx);
    inv[n] = ldexpf(1.f, -sh);
    std::fill(hi.begin(), hi.end(), 0);
    std::fill(lo.begin(), lo.end(), 0);
    for (int c = 0; c < cols; ++c) {
      const float v = ldexpf(row[c], sh);
      hi[c] = half_bits(v);
      lo[c] = half_bits(v - pc_half_value(hi[c]));
    }
    const int rb = n / 32, q = n % 32;
    for (int s = 0; s < steps; ++s)
      for (int lh = 0; lh < 2; ++lh) {
        uint16_t* dh = dst + ((((size_t)s * RB + rb) * 2 + 0) * 64 + lh * 32 + q) * 8;
        uint16_t* dl = dh + 64 * 8;
        for (int e = 0; e < 8; ++e) {
          dh[e] = hi[16 * s + pc_perm(lh, e)];
          dl[e] = lo[16 * s + pc_perm(lh, e)];
        }
      }
  }
}

// the image of an ensemble, on the host and on the device: [W1 pairs][1 / scale][b1][W2 pairs][1 / scale][b2][W3][b3]
struct PcImage { uint16_t* w1; float *is, *b1; uint16_t* w2; float *is2, *b2, *w3, *b3; size_t bytes; };
PcImage pc_image(void* base, size_t M, size_t w1n, size_t w2n, int H1P, int H2P, int K) {
  Carver c(base);
  PcImage i;
  i.w1 = c.take<uint16_t>(M * w1n * 2);
  i.is = c.take<float>(M * H1P * 4);
  i.b1 = c.take<float>(M * H1P * 4);
  i.w2 = c.take<uint16_t>(M * w2n * 2);
  i.is2 = c.take<float>(M * H2P * 4);
  i.b2 = c.take<float>(M * H2P * 4);
  i.w3 = c.take<float>(M * K * H2P * 4);
  i.b3 = c.take<float>(M * K * 4);
  i.bytes = c.bytes();
  return i;
}

}  // namespace

hipError_t pixcls_create(int C, int M, int h1, int h2, int K, const float* W1, const float* b1, const float* W2, const float* b2,
                         const float* W3, const float* b3, PixCls** out) {
  const bool large = h1 > 128 || h2 > 32;
  const int H1P = large ? 256 : 128, H2P = large ? 128 : 32;
  const int nkt = (C + PC_KT - 1) / PC_KT, NRB = H1P / 32, NJB = H2P / 32;
  const size_t w1n = (size_t)nkt * 2 * NRB * 2 * 64 * 8, w2n = (size_t)(H1P / 16) * NJB * 2 * 64 * 8;          // halves per model
  const size_t bytes = pc_image(nullptr, M, w1n, w2n, H1P, H2P, K).bytes;
  std::vector<char> host(bytes, 0);
  const PcImage hi = pc_image(host.data(), M, w1n, w2n, H1P, H2P, K);
  uint16_t *pw = hi.w1, *pw2 = hi.w2;
  float *is = hi.is, *pb1 = hi.b1, *is2 = hi.is2, *pb2 = hi.b2, *pw3 = hi.w3, *pb3 = hi.b3;
  for (int m = 0; m < M; ++m) {
    pc_pack_pairs(W1 + (size_t)m * h1 * C, h1, C, NRB, nkt * 2, pw + m * w1n, is + m * H1P);
    pc_pack_pairs(W2 + (size_t)m * h2 * h1, h2, h1, NJB, H1P / 16, pw2 + m * w2n, is2 + m * H2P);
    for (int n = 0; n < h1; ++n) pb1[m * H1P + n] = b1[(size_t)m * h1 + n];                                   // (padding: zero weights, zero bias)
    for (int j = 0; j < h2; ++j) pb2[m * H2P + j] = b2[(size_t)m * h2 + j];
    for (int c = 0; c < K; ++c) {
      pb3[m * K + c] = b3[(size_t)m * K + c];
      for (int j = 0; j < h2; ++j) pw3[((size_t)m * K + c) * H2P + j] = W3[((size_t)m * K + c) * h2 + j];
    }
  }
  void* dev = nullptr;
  hipError_t e = hipMalloc(&dev, bytes);
  if (e != hipSuccess) return e;
  e = hipMemcpy(dev, host.data(), bytes, hipMemcpyHostToDevice);
  if (e != hipSuccess) { (void)hipFree(dev); return e; }
  const PcImage di = pc_image(dev, M, w1n, w2n, H1P, H2P, K);
  *out = new PixCls{C, M, h1, h2, K, H1P, H2P, nkt, dev, di.w1, di.is, di.b1, di.w2, di.is2, di.b2, di.w3, di.b3};
  return hipSuccess;
}

void pixcls_destroy(PixCls* pc) {
  if (!pc) return;
  (void)hipFree(pc->dev);
  delete pc;
}

size_t pixcls_workspace(const PixCls* pc, long P) { return up256((size_t)pc->M * (size_t)P * pc->K * 4); }

hipError_t launch_pixcls(const PixCls* pc, const AggSrc& x, int B, long long* labels, float* js, unsigned char* model_labels, float* logits,
                         void* workspace, hipStream_t s) {
  if (!pc || !x.ptr || !labels || !workspace || ((uintptr_t)workspace & 15) || x.C != pc->C || x.H < 1 || x.W < 1 || B < 0)
    return hipErrorInvalidValue;
  const long P = (long)B * x.H * x.W;
  if (P >= (1l << 31)) return hipErrorInvalidValue;
  if (B == 0) return hipSuccess;
  float* lg = logits ? logits : (float*)workspace;
  const long tiles = (P + PC_BP - 1) / PC_BP, total = tiles * pc->M;
  const unsigned chunk = (unsigned)xcd_chunk(total);
  const PcArgs a{x.ptr, x.sb, x.sc, x.sy, x.sx, x.C, x.H, x.W, P, (const u32x4*)pc->w1, pc->inv_s, pc->b1, (const u32x4*)pc->w2, pc->inv_s2, pc->b2, pc->w3, pc->b3,
                 lg, pc->M, pc->K, pc->nkt, chunk, total};
  const bool cl = map_lanes_c(x);
  hipError_t e;
  if (x.f32) e = cl ? pc_launch_nets<float, true>(pc, a, chunk * XCDS, s) : pc_launch_nets<float, false>(pc, a, chunk * XCDS, s);
  else e = cl ? pc_launch_nets<_Float16, true>(pc, a, chunk * XCDS, s) : pc_launch_nets<_Float16, false>(pc, a, chunk * XCDS, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(pc_vote_kernel, dim3((unsigned)((P + 127) / 128)), dim3(128), 0, s, lg, pc->M, pc->K, P, labels, js, model_labels);
  return hipGetLastError();
}

}  // namespace gdf
