// MFMA GEMM + implicit-GEMM 3x3 convolution for gfx950 (MI355X), fp16 operands, fp32 accumulate: kernels, tile selection, launchers, split-K.
//
//   D[M,N] = A[M,K] * Wt[N,K]^T  with a fused epilogue (bias, per-sample row vector, residual add,
//   GEGLU gate, fp16/fp32 dual store, pre-residual aux store).
//
// Reference ops this one kernel family replaces (paths under /root/reference/feature/diffusers/models):
//   nn.Linear in Attention.to_q/to_k/to_v/to_out (attention_processor.py:241-267), FeedForward.net
//   (attention.py:1238-1258, GEGLU), Transformer2DModel.proj_in/proj_out (transformers/transformer_2d.py:178-209),
//   nn.Conv2d 3x3 in ResnetBlock2D.conv1/conv2 (resnet.py:269,285), conv_shortcut 1x1 (resnet.py:311-318),
//   Downsample2D.conv stride 2 (downsampling.py:115-118), Upsample2D nearest x2 + conv (upsampling.py:176-193),
//   UNet conv_in / conv_out (unet/unet_2d_condition.py:260-262,480-482).
//
// Structure: BM x BN x 64 block tile, mfma_f32_16x16x32_f16, template <MODE, BM, BN, STAGES, GEGLU, DIT>:
//   * STAGES = 9 / 8: the 8-phase main loops of the large tiles (256x320 with 2x4 waves of 128x80 and B resident in registers;
//     256x256 with 4x2 waves of 64x128 and A resident): the two waves of a SIMD run one workgroup barrier apart, so one multiplies
//     while the other reads fragments and issues DMA; half-tile / quarter-tile DMA runs 1.5 K-tiles ahead with ONE counted
//     `s_waitcnt vmcnt(N)` per K-tile.  These carry 65 % of an SDXL step and 70 % of a Flux step (see the blocks below).
//   * STAGES = 3: 256x128, 8 waves, 3-stage LDS ring (144 KiB), counted waits, raw `s_barrier`, one per K-tile.
//   * STAGES = 2: 128x128 / 128x160 / 128x16 (4 waves, 2 workgroups per CU: narrow N, few tiles, epilogue-heavy GEMMs) and
//     the 2-stage ring form of the 256-row tiles (kept as the bit-exact reference of the 8-phase loops, tools/stress_gemm8.py).
//   * Both operands are streamed HBM -> LDS with `buffer_load_dwordx4 ... lds` (no VGPR round trip).
//     The LDS image is lane-linear, so the bank-conflict XOR swizzle is applied on the SOURCE address
//     (chunk ^= row&7) and mirrored on the ds_read_b128 side.
//   * Convolution zero padding, M/N tails and the nearest-x2 upsample are all done in the address
//     generator: out-of-image taps get an out-of-range buffer offset, which the hardware returns as 0.
//   * Epilogue is staged per wave through LDS so every global store / residual load is a full
//     16-byte-per-lane, 128-byte-per-row access.
//
// Source layout (round 6): gemm_common.h (types, LDS-DMA, MFMA wrappers, GELU, tile order), gemm_tile.h (GemmTile: tile geometry, tile origin,
// operand address generators), gemm_mainloop_ring.h (2- / 3-stage LDS rings), gemm_mainloop_8phase.h (the two-group 256x256 / 256x320 loops),
// gemm_epilogue.h (the staged epilogue), this file (gemm_body = locate -> main loop -> epilogue, the kernel wrappers, dispatch: gemm_select -> GemmSel
// descriptor -> instantiation table -> launch_gemm / gemm_kernel_name, split-K).
#include "gemm_mainloop_ring.h"
#include "gemm_mainloop_8phase.h"
#include "gemm_epilogue.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <mutex>
#include <string>

namespace gdf {

template <int MODE, int BM, int BN, int STAGES, bool GEGLU, bool DIT, bool BF = false, bool QKN = false, bool SPLIT = false, bool MX = false,
          bool GNS = false>
__device__ __forceinline__ void gemm_body(const GemmParams& p) {
  using T = GemmTile<MODE, BM, BN, STAGES, GEGLU, DIT, BF, QKN, SPLIT, MX, GNS>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T t(p, smem);
  const int tiles_n = (p.N + BN - 1) / BN;
  const int nblk = ((p.M + BM - 1) / BM) * tiles_n;
  // Persistent form: the launcher may start fewer workgroups than tiles (one per CU for the two-group 256x256 kernels); workgroup b
  // then walks the tiles b, b + gridDim.x, ... — with gridDim.x a multiple of 8 these are the tiles the hardware would have given the
  // same XCD round after round, so the super-block order below is unchanged.  Saves the workgroup relaunch between rounds
  // (profiles/r02_gemm_tile_trace.txt: 2.6 us from a tile's last instruction to the first of the next tile on that CU, of ~37 us per tile at
  // K = 1280) and the kernel-argument / descriptor setup.  A plain launch has gridDim.x == nblk: one trip.
  // Compiled as a loop only where the register budget has room for the loop-carried lane constants (256x320: 9-11 VGPRs spilled).
  constexpr bool PERSIST = (STAGES == 8);
  int vb = blockIdx.x;
  do {
  t.locate(vb, tiles_n, nblk);
  f32x4 acc[T::FM][T::FN];
#pragma unroll
  for (int i = 0; i < T::FM; ++i)
#pragma unroll
    for (int j = 0; j < T::FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  if constexpr (STAGES == 8) gemm_mainloop_8phase_256(t, acc);
  else if constexpr (STAGES == 9) gemm_mainloop_8phase_320(t, acc);
  else gemm_mainloop_ring(t, acc);
  __syncthreads();   // all waves finished reading the last tile: LDS is free for epilogue staging
  gemm_epilogue(t, acc);
  if constexpr (!PERSIST) break;
  vb += gridDim.x;
  if (vb >= nblk) break;
  // every wave is done with the staging area before the next tile's DMA lands.  Raw barrier + lgkmcnt only: __syncthreads() would
  // also wait (vmcnt) for this tile's global stores, which may drain under the next tile's prologue
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  } while (true);
}

template <int MODE, int BM, int BN, int STAGES, bool GEGLU>
__global__ __launch_bounds__(BM * 2, 2) void gemm_kernel(const GemmParams p) {
  gemm_body<MODE, BM, BN, STAGES, GEGLU, false>(p);
}
// 3x3 conv whose epilogue also writes GroupNorm partial sums (GemmParams::gn_partial; the VAE and UNet op programs: PlanBuilder::gn_epi)
template <int MODE, int BM, int BN, int STAGES>
__global__ __launch_bounds__(BM * 2, 2) void gemm_gn_kernel(const GemmParams p) {
  gemm_body<MODE, BM, BN, STAGES, false, false, false, false, false, false, true>(p);
}
// the same tiles with split fp16 hi + lo operands ("precise" plans)
template <int MODE, int BM, int BN, int STAGES, bool GEGLU>
__global__ __launch_bounds__(BM * 2, 2) void gemm_split_kernel(const GemmParams p) {
  gemm_body<MODE, BM, BN, STAGES, GEGLU, false, false, false, true>(p);
}
// dense GEMM with the MMDiT epilogue (tanh-GELU / per-sample gate / two-region sample map); BF: bf16 operands and activations
template <int BM, int BN, int STAGES, bool BF, bool QKN>
__global__ __launch_bounds__(BM * 2, 2) void gemm_dit_kernel(const GemmParams p) {
  gemm_body<A_DENSE, BM, BN, STAGES, false, true, BF, QKN>(p);
}

// the MMDiT kernels with split bf16 hi + lo A operands / outputs ('bfloat16x2' plans, gdf_flux.h)
template <int BM, int BN, int STAGES, bool BF, bool QKN>
__global__ __launch_bounds__(BM * 2, 2) void gemm_dit_split_kernel(const GemmParams p) {
  gemm_body<A_DENSE, BM, BN, STAGES, false, true, BF, QKN, true>(p);
}

// MMDiT GEMM on fp8 (e4m3) operands, bf16 output ('fp8-mx' plans, gdf_flux.h): MX-scaled MFMA, K = 128 per instruction
template <int BM, int BN, int STAGES>
__global__ __launch_bounds__(BM * 2, 2) void gemm_mx_kernel(const GemmParams p) {
  gemm_body<A_DENSE, BM, BN, STAGES, false, true, true, false, false, true>(p);
}

// workgroups of a persistent launch of a 1-workgroup-per-CU kernel: the CU count of the current device (a multiple of 8 XCDs);
// GDF_PERSIST=0 (diagnostics) launches one workgroup per tile instead
static int persist_wgs() {
  static const int off = [] { const char* e = getenv("GDF_PERSIST"); return e && atoi(e) == 0; }();
  if (off) return 1 << 30;
  static std::atomic<int> cus[16];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return 1 << 30;
  int n = cus[dev].load(std::memory_order_relaxed);
  if (n == 0) {
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 8 || (n & 7)) n = 1 << 30;
    cus[dev].store(n, std::memory_order_relaxed);
  }
  return n;
}

// the __global__ wrapper that runs gemm_body with these template arguments: the one map from an instantiation to its kernel symbol
template <int MODE, int BM, int BN, int STAGES, bool GEGLU, bool DIT, bool BF, bool QKN, bool SPLIT, bool MX, bool GNS>
static constexpr auto gemm_wrapper() -> void (*)(const GemmParams) {
  if constexpr (MX) return gemm_mx_kernel<BM, BN, STAGES>;
  else if constexpr (GNS) return gemm_gn_kernel<MODE, BM, BN, STAGES>;
  else if constexpr (DIT && SPLIT) return gemm_dit_split_kernel<BM, BN, STAGES, BF, QKN>;
  else if constexpr (DIT) return gemm_dit_kernel<BM, BN, STAGES, BF, QKN>;
  else if constexpr (SPLIT) return gemm_split_kernel<MODE, BM, BN, STAGES, GEGLU>;
  else return gemm_kernel<MODE, BM, BN, STAGES, GEGLU>;
}

template <int MODE, int BM, int BN, int STAGES, bool GEGLU, bool DIT, bool BF, bool QKN, bool SPLIT, bool MX, bool GNS>
static hipError_t launch_t(const GemmParams& p, hipStream_t s) {
  const int tiles_m = (p.M + BM - 1) / BM, tiles_n = (p.N + BN - 1) / BN;
  const int smem = (STAGES >= 8 ? 2 : STAGES) * (BM * 128 + BN * 128);
  constexpr auto fn = gemm_wrapper<MODE, BM, BN, STAGES, GEGLU, DIT, BF, QKN, SPLIT, MX, GNS>();
  static std::atomic<uint64_t> attr_mask{0};             // per template instantiation, one bit per device
  if (const hipError_t e = ensure_dyn_smem(attr_mask, (const void*)fn, smem); e != hipSuccess) return e;
  GemmParams q = p;
  q.sb_gm = q.sb_gn = 0;
  if (!p.no_superblock) {
    const int conc = (p.cus > 0 ? p.cus / 8 : 32) * ((BM == 256) ? 1 : 2);   // workgroups one XCD keeps resident (32 CUs x 1 or 2; a CU partition: cus / 8)
    for (int gn = 4; gn >= 2; gn >>= 1) {                                     // widest super-block: 4 tiles
      const int gm = conc / gn;
      if (tiles_n % gn == 0 && tiles_m % gm == 0 && (tiles_m / gm) * (tiles_n / gn) >= 8 && tiles_n > gn) {
        q.sb_gm = gm; q.sb_gn = gn;
        break;
      }
    }
  }
  int gx = tiles_m * tiles_n;
  const int pw = (p.cus > 0 && p.cus < persist_wgs()) ? p.cus : persist_wgs();
  if (STAGES == 8 && gx > pw && !(p.batch > 1)) gx = pw;   // persistent: one workgroup per CU walks the tiles
  const dim3 grid(gx, (STAGES == 2 && p.splitk > 1) ? p.splitk : p.batch > 1 ? p.batch : 1);
  hipLaunchKernelGGL(fn, grid, dim3(BM * 2), smem, s, q);
  return hipGetLastError();
}

// ---- dispatch: select (host arithmetic only, no device call) -> descriptor -> instantiation table -> launch / name ----
// The descriptor (GemmSel, kernels.h) spells one instantiation: the template arguments of gemm_body.  launch_gemm() launches the table
// entry the descriptor names and gemm_kernel_name() prints the same descriptor, so what a test or a profile reads is what runs.
// a table entry: key, launcher, rows of a wave tile (the GroupNorm statistics slab of the GNS forms), all from the same template arguments
struct GemmInst { GemmSel k; hipError_t (*launch)(const GemmParams&, hipStream_t); int wtm; };
template <int MODE, int BM, int BN, int STAGES, bool GEGLU = false, bool DIT = false, bool BF = false, bool QKN = false, bool SPLIT = false,
          bool MX = false, bool GNS = false>
static constexpr GemmInst inst() {
  return {{true, MODE, BM, BN, STAGES, GEGLU, DIT, BF, QKN, SPLIT, MX, GNS, false}, launch_t<MODE, BM, BN, STAGES, GEGLU, DIT, BF, QKN, SPLIT, MX, GNS>,
          GemmTile<MODE, BM, BN, STAGES, GEGLU, DIT, BF, QKN, SPLIT, MX, GNS>::WTM};
}
// every instantiation of the library; a descriptor none of them matches is an error, never another kernel
static const GemmInst kGemmInst[] = {
    inst<A_DENSE, 128, 16, 2>(),                             // gemm_kernel: dense
    inst<A_DENSE, 128, 128, 2>(),
    inst<A_DENSE, 128, 160, 2>(),
    inst<A_DENSE, 256, 128, 3>(),
    inst<A_DENSE, 256, 320, 2>(),
    inst<A_DENSE, 256, 320, 9>(),
    inst<A_DENSE, 128, 128, 2, true>(),                      // GEGLU: weight rows / bias interleaved [16 h | 16 gate] (launch_relayout_rows geglu = 16)
    inst<A_DENSE, 256, 128, 3, true>(),
    inst<A_DENSE, 256, 320, 2, true>(),
    inst<A_DENSE, 256, 256, 8, true>(),
    inst<A_CONV3, 128, 16, 2>(),                             // 3x3 conv (128x16: conv_out)
    inst<A_CONV3, 128, 128, 2>(),
    inst<A_CONV3, 128, 160, 2>(),
    inst<A_CONV3, 256, 128, 3>(),
    inst<A_CONV3, 256, 320, 2>(),
    inst<A_CONV3, 256, 256, 8>(),
    inst<A_CONV3, 256, 320, 9>(),
    inst<A_CONV_SMALLC, 128, 128, 2>(),                      // conv_in
    inst<A_CONV_SMALLC, 128, 160, 2>(),
    inst<A_DENSE, 128, 128, 2, false, false, false, false, true>(),  // gemm_split_kernel ("precise" plans), a reduced set of tiles: dense / conv 256x320 two-group, 128x160, 128x128
    inst<A_DENSE, 128, 160, 2, false, false, false, false, true>(),
    inst<A_DENSE, 256, 320, 9, false, false, false, false, true>(),
    inst<A_DENSE, 128, 128, 2, true, false, false, false, true>(),   // (GEGLU: 256x256 two-group and 128x128)
    inst<A_DENSE, 256, 256, 8, true, false, false, false, true>(),
    inst<A_CONV3, 128, 16, 2, false, false, false, false, true>(),   // (the narrow-N tile: conv_out)
    inst<A_CONV3, 128, 128, 2, false, false, false, false, true>(),
    inst<A_CONV3, 128, 160, 2, false, false, false, false, true>(),
    inst<A_CONV3, 256, 320, 9, false, false, false, false, true>(),
    inst<A_CONV_SMALLC, 128, 128, 2, false, false, false, false, true>(),
    inst<A_CONV_SMALLC, 128, 160, 2, false, false, false, false, true>(),
    inst<A_DENSE, 128, 128, 2, false, true>(),               // gemm_dit_kernel: fp16, then bf16; QKN on the 256x256 tile only
    inst<A_DENSE, 256, 128, 3, false, true>(),
    inst<A_DENSE, 256, 256, 2, false, true>(),
    inst<A_DENSE, 256, 256, 2, false, true, false, true>(),
    inst<A_DENSE, 256, 256, 8, false, true>(),
    inst<A_DENSE, 256, 256, 8, false, true, false, true>(),
    inst<A_DENSE, 128, 128, 2, false, true, true>(),
    inst<A_DENSE, 256, 128, 3, false, true, true>(),
    inst<A_DENSE, 256, 256, 2, false, true, true>(),
    inst<A_DENSE, 256, 256, 2, false, true, true, true>(),
    inst<A_DENSE, 256, 256, 8, false, true, true>(),
    inst<A_DENSE, 256, 256, 8, false, true, true, true>(),
    inst<A_DENSE, 128, 128, 2, false, true, true, false, true>(),    // gemm_dit_split_kernel: bf16 hi + lo operands ('bfloat16x2' plans)
    inst<A_DENSE, 256, 256, 8, false, true, true, false, true>(),
    inst<A_DENSE, 256, 256, 8, false, true, true, true, true>(),
    inst<A_DENSE, 256, 256, 8, false, true, true, false, false, true>(),   // gemm_mx_kernel: fp8 (e4m3) operands ('fp8-mx' plans), the 256x256 two-group tile only
    inst<A_CONV3, 128, 128, 2, false, false, false, false, false, false, true>(),   // gemm_gn_kernel: GroupNorm partial sums from the epilogue of a plain 3x3 conv / conv_in
    inst<A_CONV3, 128, 160, 2, false, false, false, false, false, false, true>(),
    inst<A_CONV3, 256, 128, 3, false, false, false, false, false, false, true>(),
    inst<A_CONV3, 256, 256, 8, false, false, false, false, false, false, true>(),
    inst<A_CONV3, 256, 320, 9, false, false, false, false, false, false, true>(),
    inst<A_CONV_SMALLC, 128, 128, 2, false, false, false, false, false, false, true>(),
};

static const GemmInst* find_inst(const GemmSel& k) {
  for (const GemmInst& e : kGemmInst)
    if (e.k.MODE == k.MODE && e.k.BM == k.BM && e.k.BN == k.BN && e.k.STAGES == k.STAGES && e.k.GEGLU == k.GEGLU && e.k.DIT == k.DIT &&
        e.k.BF == k.BF && e.k.QKN == k.QKN && e.k.SPLIT == k.SPLIT && e.k.MX == k.MX && e.k.GNS == k.GNS) return &e;
  return nullptr;
}
struct Tile { int bm, bn, st; };                       // BM, BN, STAGES
static constexpr Tile T128x16{128, 16, 2}, T128x128{128, 128, 2}, T128x160{128, 160, 2}, T256x128{256, 128, 3}, T256x320R{256, 320, 2},
    T256x256R{256, 256, 2}, T256x256{256, 256, 8}, T256x320{256, 320, 9}, NO_TILE{0, 0, 0};
static bool operator==(const Tile& a, const Tile& b) { return a.bm == b.bm && a.bn == b.bn && a.st == b.st; }

// The public `variant` codes (include/gdf_ops.h), decoded here and nowhere else.  UNet / VAE forms: false = not a code, which means the
// 128x128 tile.  825 / 826 are the 256x256 two-group tile of the GEGLU / of the conv form; on the other form they name no tile it has.
static bool unet_tile(int code, bool geglu, Tile& t) {
  t = code == 16 ? T128x16 : code == 160 ? T128x160 : code == 256 ? T256x128 : code == 320 ? T256x320R : code == 932 ? T256x320
      : code == 825 ? (geglu ? T256x256 : NO_TILE) : code == 826 ? (geglu ? NO_TILE : T256x256) : T128x128;
  return code == 128 || !(t == T128x128);
}
// MMDiT forms: false = not one of their four codes, which means the automatic choice
static bool dit_tile(int code, Tile& t) {
  if (code != 128 && code != 1256 && code != 2128 && code != 8256) return false;
  t = code == 128 ? T128x128 : code == 1256 ? T256x256R : code == 2128 ? T256x128 : T256x256;
  return true;
}
// Tile selection.  Every channel count of the SD / SDXL UNets is a multiple of 160 (320 k), so the 128x160 tile
// (2 workgroups per CU, 72 KiB LDS each) covers N without a ragged last column tile and makes M/128 * N/160 a
// multiple of the 512 workgroup slots for the SDXL batch-16 shapes (no tail round).  128x128 serves other N;
// 256x128 (8 waves, 3-stage ring) wins for very large problems.
// fraction of the workgroup slots that do useful work when `tiles` equal tiles run on `slots` concurrent slots (whole rounds)
static double round_fill(long tiles, int slots) {
  if (tiles <= 0) return 0.0;
  const long rounds = (tiles + slots - 1) / slots;
  return (double)tiles / (double)(rounds * slots);
}
static Tile splitk_tile(int N) {                       // split-K lives in the 2-stage ring tiles
  static const int force = [] { const char* e = getenv("GDF_SPLITK_TILE"); return e ? atoi(e) : 0; }();   // diagnostics: 128 | 160
  if (force == 160 && N % 160 == 0) return T128x160;
  if (force == 128 && N % 128 == 0) return T128x128;
  // round 5: the 128x160 tile whenever it divides N (SD1.5's 8x8 level, N = 1280: 750 / 891 vs 715 / 824 TFLOP/s at K = 11520 / 23040,
  // tools/bench_conv_small_m.py)
  return (N % 160 == 0) ? T128x160 : T128x128;
}
static Tile dit_auto_tile(const GemmParams& p) {   // MMDiT widths are multiples of 256 (3072 = 24 x 128): 256x256 tiles (128 KiB ring, 1 workgroup / CU)
  const long t256 = (long)((p.M + 255) / 256) * ((p.N + 255) / 256);
  // 8-phase schedule: 1177-1362 vs 1002-1188 TFLOP/s (2-stage ring) at the Flux shapes.  A ragged last column tile is fine up to
  // 1/8 of padding (PixArt C = 1152 = 4.5 x 256: 1017-1187 vs 873-1020 on the 256x128 ring)
  if (t256 >= 128 && (long)((p.N + 255) / 256) * 256 <= (long)p.N + p.N / 8) return T256x256;
  return (p.N % 128 == 0 && (long)((p.M + 255) / 256) * (p.N / 128) >= 256) ? T256x128 : T128x128;   // PixArt: C = 1152 = 9 x 128
}

static Tile unet_auto_tile(const GemmParams& p) {
  const int S1 = p.cus > 0 ? p.cus : 256, S2 = 2 * S1;   // workgroup slots at 1 / 2 workgroups per CU (whole chip or a CU partition)
  const long tiles320 = (long)((p.M + 255) / 256) * ((p.N + 319) / 320);
  auto rank320 = [&](double r160, double r128) {         // N % 320 == 0: 256x320 two-group against the two small tiles, rate x fill of the rounds
    const double s320 = 1.00 * round_fill(tiles320, S1), s160 = r160 * round_fill((long)((p.M + 127) / 128) * (p.N / 160), S2);
    const double s128 = r128 * round_fill((long)((p.M + 127) / 128) * ((p.N + 127) / 128), S2);
    return (s320 >= s160 && s320 >= s128) ? T256x320 : (s160 >= s128 ? T128x160 : T128x128);
  };
  if (p.geglu) {
    // 8-phase 256x256: 1130 vs 1073 TFLOP/s (256x320 ring) at 16384 x 10240 x 1280, 899 vs 869 at 65536 x 5120 x 640
    // The batch-16 shapes fill whole rounds of every tile; other batch sizes may leave a mostly idle last round, so the
    // candidates are ranked by (measured rate at full rounds) x (fill of the rounds they need)
    const long tm256 = (p.M + 255) / 256, tm128 = (p.M + 127) / 128;
    double best = 0.0; Tile bt = T128x128;
    auto cand = [&](Tile t, double rate, long tiles, int slots) { const double sc = rate * round_fill(tiles, slots); if (sc > best) { best = sc; bt = t; } };
    if (p.N % 256 == 0) cand(T256x256, 1.00, tm256 * (p.N / 256), S1);
    if (p.N % 320 == 0) cand(T256x320R, 0.95, tm256 * (p.N / 320), S1);
    cand(T256x128, 0.80, tm256 * ((p.N + 127) / 128), S1);
    cand(T128x128, 0.70, tm128 * ((p.N + 127) / 128), S2);
    return bt;
  }
  if (p.mode != A_DENSE) {                                                 // convs (K = 9 Cin is long)
    if (p.N % 320 == 0) return rank320(0.85, 0.70);                        // 8-phase 256x320: 1150-1350 TFLOP/s (ring 1090-1310, 128x160 950-1140)
    if (p.N % 160 == 0) return T128x160;
    if (p.N % 256 == 0 && (long)((p.M + 255) / 256) * (p.N / 256) >= 256) return T256x256;   // VAE widths 256 / 512: 989-1146 vs 830-965 (256x128 ring)
    return (p.N <= 128 && p.M >= (1 << 20)) ? T256x128 : T128x128;         // VAE level-0 convs (N = 128, 4 M pixels): 797 vs 697
  }
  // short-K GEMMs with the fp32 residual epilogue (attention out-projections: 10 B/element of epilogue traffic against
  // 20 K-tiles of MFMA work) fill the chip in ONE round of 256x320 tiles, so main loop and epilogue traffic never overlap;
  // 128x160 tiles run 2 workgroups per CU and 2+ rounds (80 vs 89 us at 16384 x 1280 x 1280)
  // (round 2: with the two-phase main loop the 256x320 tile wins again where its tiles fill whole rounds — 16384 x 1280 x 1280
  // 64.7 vs 77.7 us, 32768 x 640 x 640 47.0 vs 49.8, 65536 x 640 x 640 equal; it still loses at half-filled rounds, 8192 x 1280 x 1280
  // 47.3 vs 37.3, and at N = 320, tools/bench_res32.py)
  if (p.res32 && p.K <= 1536 && p.N % 160 == 0 && tiles320 <= S2 &&
      !(p.N % 320 == 0 && p.N >= 640 && p.K >= 640 && tiles320 % S1 == 0)) return T128x160;
  if (p.N % 320 == 0) return rank320(0.87, 0.72);                          // 8-phase: qkv 1113, ff_out 1088, attn2_q 1045, shortcut 1086 (ring: 1051 / 983 / 980 / 1002)
  if (p.N % 160 == 0 && p.K >= 1024) return T128x160;
  if ((long)p.M * p.N >= (1L << 26) && (long)((p.M + 255) / 256) * ((p.N + 127) / 128) >= S2) return T256x128;    // short-K, large MxN (qkv @ C=640): 712 vs 642
  return T128x128;
}

// every reason launch_gemm refuses a launch and every tile it chooses: the queries answer "none" exactly where the launch returns an error
GemmSel gemm_select(const GemmParams& p) {
  GemmSel k{};                                                                              // ok = false
  if ((p.mode != A_CONV_SMALLC && (p.K % BK) != 0) || (p.mode == A_CONV3 && (p.Cin % BK) != 0)) return k;
  if (p.k_w > 0 && (p.K != 2 * p.k_w || (p.k_w % BK) != 0 || p.mode == A_CONV_SMALLC || (p.dit && !p.bf16) || (p.mode == A_CONV3 && (p.k_w % (9 * BK)) != 0)))
    return k;                                                                               // split operands: K = [hi | lo] over one weight matrix
  if (p.o16_lo > 0 && ((p.dit && !p.bf16) || p.bn == 16 || (p.o16_lo % 8) != 0)) return k;   // (MMDiT: the bf16 pair form only)
  if ((p.out_f16 && !(p.dit && p.bf16)) || (p.bf16 && !p.dit)) return k;                    // bf16 exists on the MMDiT path only
  // split hi + lo operands or outputs ("precise" UNet plans, 'bfloat16x2' MMDiT plans): their own instantiations
  const bool split = p.k_w > 0 || p.o16_lo > 0;
  Tile t; bool forced = false, known = true;                                                // (the tile is GemmParams::variant's; that was a code)
  if (p.dit) {
    if (p.mx) t = T256x256;                                                                 // fp8 operands: the one tile
    else if (!dit_tile(p.variant, t)) t = dit_auto_tile(p);
    if (split) t = (t.bm == 256 && t.bn == 256) ? T256x256 : T128x128;                      // 'bfloat16x2' plans: 256x256 two-group or 128x128
  } else if (p.bn == 16) t = T128x16;
  else if (p.splitk > 1) t = splitk_tile(p.N);
  else if (p.variant) { known = unet_tile(p.variant, p.geglu != 0, t); forced = true; }
  else t = unet_auto_tile(p);
  if (t.bn != 16 && ((p.geglu ? p.N / 2 : p.N) % 8) != 0) return k;                         // ragged N only in the BN = 16 variant
  k.MODE = p.mode; k.GEGLU = p.geglu != 0; k.DIT = p.dit != 0; k.BF = p.dit && p.bf16; k.QKN = p.dit && p.qkn_nq; k.SPLIT = split; k.MX = p.dit && p.mx; k.GNS = p.gn_partial != nullptr;
  auto found = [&](const Tile& x) { k.BM = x.bm; k.BN = x.bn; k.STAGES = x.st; return find_inst(k); };
  if (p.gn_partial) {
    // GroupNorm partial sums from the epilogue: plain 3x3 convs, one slab per wave tile; a forced tile without this epilogue (or a number that is no code) is refused
    if ((p.mode != A_CONV3 && p.mode != A_CONV_SMALLC) || p.dit || p.geglu || p.splitk > 1 || p.batch > 1 || split || p.bn == 16) return k;
    if ((p.M % 64) != 0 || (p.N % 8) != 0) return k;
    if (p.mode == A_CONV_SMALLC ? t == T128x160 : !known) return k;
    if (p.mode == A_CONV_SMALLC) t = T128x128;                                              // conv_in: the 128x128 tile
    if (const GemmInst* e = found(t)) k.ok = (p.M % e->wtm) == 0;
    return k;
  }
  if (p.dit) {
    if (p.mode != A_DENSE || p.geglu || p.batch > 1) return k;
    if (p.qkn_nq && (t.bm != 256 || t.bn != 256 || (p.qkn_nq % 128) != 0)) return k;       // one head per 128-column wave tile
    if (p.qkn_nq && (p.res32 || p.res16 || p.rowvec || p.aux16 || p.out32)) return k;       // the QKN instantiation: bias -> norm + RoPE -> out16 only
    if (p.mx && (!p.bf16 || p.qkn_nq || split || (p.N % 8))) return k;                      // fp8 (e4m3) operands ('fp8-mx' plans)
  } else {
    if (p.geglu && (p.mode != A_DENSE || (p.N % 32) != 0)) return k;                        // weight rows / bias interleaved [16 h | 16 gate]
    if (t.bn == 16 && (p.mode == A_CONV_SMALLC || (split && !p.geglu && p.mode != A_CONV3))) return k;   // narrow N: conv_out, plain dense
    if (p.mode == A_CONV_SMALLC && !(t == T128x160)) t = T128x128;                          // conv_in has two tiles: any other choice means 128x128
  }
  if (!found(t)) {
    // the fall-backs, all to the form's 128x128 tile: the reduced tile set of the split forms (silent: it is their selection rule), and a
    // forced tile this form has no instantiation of (flagged: the C ABI refuses it).  Anything else without an entry is an error
    const bool reduced = split && t.bn != 16;
    if ((!reduced && !forced) || !found(T128x128)) return k;
    k.forced_missing = !reduced;
  }
  k.ok = true;
  return k;
}

// true when an MMDiT GEMM of this shape runs on the 256x256 tile, i.e. may carry the fused RMSNorm + RoPE epilogue (qkn_*)
bool gemm_qkn_ok(int M, int N, int K) {
  GemmParams g{}; g.M = M; g.N = N; g.K = K; g.dit = 1; g.mode = A_DENSE;
  const GemmSel k = gemm_select(g);
  return k.ok && k.BM == 256 && k.BN == 256;
}

// kernel symbol (as rocprofv3 prints it) of the instantiation the descriptor spells; nullptr where launch_gemm refuses
const char* gemm_kernel_name(const GemmSel& k) {
  if (!k.ok) return nullptr;
  auto tf = [](bool v) { return v ? "true" : "false"; };
  char tmp[64];
  if (k.MX) snprintf(tmp, sizeof tmp, "gemm_mx_kernel<%d, %d, %d>", k.BM, k.BN, k.STAGES);
  else if (k.GNS) snprintf(tmp, sizeof tmp, "gemm_gn_kernel<%d, %d, %d, %d>", k.MODE, k.BM, k.BN, k.STAGES);
  else if (k.DIT) snprintf(tmp, sizeof tmp, "%s<%d, %d, %d, %s, %s>", k.SPLIT ? "gemm_dit_split_kernel" : "gemm_dit_kernel", k.BM, k.BN, k.STAGES, tf(k.BF), tf(k.QKN));
  else snprintf(tmp, sizeof tmp, "%s<%d, %d, %d, %d, %s>", k.SPLIT ? "gemm_split_kernel" : "gemm_kernel", k.MODE, k.BM, k.BN, k.STAGES, tf(k.GEGLU));
  // interned: the returned pointer stays valid for the life of the library (plan build time only, mutex-protected)
  static std::mutex mu;
  static std::deque<std::string> names;
  std::lock_guard<std::mutex> lk(mu);
  for (const std::string& n : names) if (n == tmp) return n.c_str();
  names.emplace_back(tmp);
  return names.back().c_str();
}
// rows per GroupNorm statistics slab when `p` runs with gn_partial set: the wave-tile height of the selected instantiation, 0 = it cannot
int gemm_gn_slab_rows(const GemmParams& p) {
  GemmParams q = p; q.gn_partial = (float*)1;                                               // selects the form only: never followed
  const GemmSel k = gemm_select(q);
  return k.ok ? find_inst(k)->wtm : 0;
}

hipError_t launch_gemm(const GemmParams& p, hipStream_t s) {
  if (p.M <= 0 || p.N <= 0) return hipSuccess;
  const GemmSel k = gemm_select(p);
  const GemmInst* e = k.ok ? find_inst(k) : nullptr;
  return e && (p.out16 || !k.GNS) ? e->launch(p, s) : hipErrorInvalidValue;                 // (the statistics are those of the stored fp16 image)
}

// ---- split-K: sum the partial slabs in a fixed order (deterministic) and apply the GEMM epilogue of kernels.h ----
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const GemmParams p, const float* ws, int splitk) {
  const int CH = p.N / 8;
  const long total = (long)p.M * CH;
  const float a_sc = p.acc_scale != 0.f ? p.acc_scale : 1.0f, o_sc = p.out16_scale != 0.f ? p.out16_scale : 1.0f;
  const size_t slab = (size_t)p.M * p.N;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int row = (int)(i / CH), col = (int)(i - (long)row * CH) * 8;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = 0.f;
    for (int sp = 0; sp < splitk; ++sp) {
      const f32x4* q = (const f32x4*)(ws + sp * slab + (size_t)row * p.N + col);
      const f32x4 a = q[0], b = q[1];
#pragma unroll
      for (int e = 0; e < 4; ++e) { v[e] += a[e]; v[4 + e] += b[e]; }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      v[e] *= a_sc;
      if (p.bias) v[e] += p.bias[col + e];
      if (p.rowvec) v[e] += p.rowvec[(size_t)(row / p.rows_per_sample) * p.ldrv + col + e];
    }
    if (p.aux16) {
      f16x8 h;
#pragma unroll
      for (int e = 0; e < 8; ++e) h[e] = (_Float16)v[e];
      *(f16x8*)(p.aux16 + (size_t)row * p.ldaux + col) = h;
    }
    if (p.res32) {
      const f32x4* q = (const f32x4*)(p.res32 + (size_t)row * p.ldres + col);
      const f32x4 a = q[0], b = q[1];
#pragma unroll
      for (int e = 0; e < 4; ++e) { v[e] += a[e]; v[4 + e] += b[e]; }
    } else if (p.res16) {
      const f16x8 r = *(const f16x8*)(p.res16 + (size_t)row * p.ldres + col);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] += (float)r[e];
    }
    if (p.out16) {
      f16x8 h;
#pragma unroll
      for (int e = 0; e < 8; ++e) h[e] = (_Float16)(v[e] * o_sc);
      *(f16x8*)(p.out16 + (size_t)row * p.ldo16 + col) = h;
      if (p.o16_lo > 0) {
        f16x8 l;
#pragma unroll
        for (int e = 0; e < 8; ++e) l[e] = (_Float16)(v[e] * o_sc - (float)h[e]);
        *(f16x8*)(p.out16 + (size_t)row * p.ldo16 + col + p.o16_lo) = l;
      }
    }
    if (p.out32) {
      f32x4* q = (f32x4*)(p.out32 + (size_t)row * p.ldo32 + col);
      q[0] = f32x4{v[0], v[1], v[2], v[3]};
      q[1] = f32x4{v[4], v[5], v[6], v[7]};
    }
  }
}

// > 1 when splitting K pays: a plain (UNet) GEMM / conv whose 128-row tiles fill less than half of the chip's 512 workgroup slots
// while every tile walks a long K.  The factor keeps >= 16 K-tiles per range and aims at ~2 workgroups per CU.
int gemm_splitk_factor(const GemmParams& p) {
  static const int off = [] { const char* e = getenv("GDF_SPLITK"); return e && atoi(e) == 0; }();     // diagnostics: GDF_SPLITK=0
  if (off || p.dit || p.geglu || p.bn == 16 || p.batch > 1 || p.mode == A_CONV_SMALLC || p.variant || (p.N % 128) || (p.K % BK)) return 1;
  const long tiles = (long)((p.M + 127) / 128) * (p.N / splitk_tile(p.N).bn);
  const int nk = p.K / BK;
  const int S1 = p.cus > 0 ? p.cus : 256;
  if (tiles >= S1 || nk < 64) return 1;
  int s = (int)(2 * S1 / tiles);
  if (s > nk / 16) s = nk / 16;
  if (s > 8) s = 8;
  return s < 2 ? 1 : s;
}

// pass 1 of launch_gemm_splitk (raw partial sums, one slab per K range) as parameters of launch_gemm: false where the split launch is refused;
// `splitk` comes back clamped to the K-tile count, <= 1 meaning the plain launch of `p`
bool gemm_splitk_pass1(const GemmParams& p, int& splitk, float* ws, GemmParams& g) {
  g = p;
  if (splitk <= 1) return true;
  if (p.dit || p.geglu || p.batch > 1 || (p.N % 8) || p.mode == A_CONV_SMALLC || (p.K % BK)) return false;
  if (splitk > p.K / BK) splitk = p.K / BK;
  if (splitk <= 1) return true;
  g.bias = nullptr; g.rowvec = nullptr; g.res32 = nullptr; g.res16 = nullptr; g.aux16 = nullptr; g.out16 = nullptr;
  g.acc_scale = 0.f; g.out16_scale = 0.f;
  g.out32 = ws; g.ldo32 = p.N; g.splitk = splitk; g.o32_sstride = (long)p.M * p.N; g.variant = 0;
  return true;
}

hipError_t launch_gemm_splitk(const GemmParams& p, int splitk, float* ws, hipStream_t s) {
  GemmParams g;
  if (!gemm_splitk_pass1(p, splitk, ws, g)) return hipErrorInvalidValue;
  if (splitk <= 1) return launch_gemm(p, s);
  hipError_t e = launch_gemm(g, s);
  if (e != hipSuccess) return e;
  long blocks = ((long)p.M * (p.N / 8) + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, s, p, (const float*)ws, splitk);
  return hipGetLastError();
}

}  // namespace gdf
