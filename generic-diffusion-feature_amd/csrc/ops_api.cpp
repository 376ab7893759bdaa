// extern "C" kernel-level entry points (include/gdf_ops.h): one launch each, used by tests and micro-benchmarks.
#include "../../include/gdf_ops.h"
#include "model.h"

using namespace gdf;

// the GEMM / conv kernels address both operands with 32-bit buffer offsets whose top bit marks "out of range"
static bool span_ok(size_t a_bytes, size_t w_bytes, const char* what) {
  if (a_bytes < (1ull << 31) && w_bytes < (1ull << 31)) return true;
  set_error(std::string(what) + ": operand larger than 2 GiB (32-bit buffer offsets); split the rows");
  return false;
}

static int fin(hipError_t e, const char* what) {
  if (e == hipSuccess) return GDF_OK;
  set_error(std::string(what) + ": " + hipGetErrorString(e));
  return GDF_ERR_HIP;
}

static AttnParams attn_params(const gdf_attn_args& g) {
  AttnParams a{};
  a.q = (const half_t*)g.q; a.ldq = g.ldq; a.k = (const half_t*)g.k; a.ldk = g.ldk; a.v = (const half_t*)g.v; a.ldv = g.ldv;
  a.o = (half_t*)g.o; a.ldo = g.ldo; a.B = g.B; a.heads = g.heads; a.Sq = g.Sq; a.Sk = g.Sk; a.D = g.D; a.kv_bstride = g.kv_bstride;
  a.scale = g.scale != 0.f ? g.scale : 1.0f / sqrtf((float)g.D);
  a.map = (half_t*)g.map; a.map2 = (half_t*)g.map2; a.kv_len = g.kv_len; a.seg_T = g.seg_T; a.bf16 = g.bf16; a.o_lo = g.o_lo;
  a.o_pair_bf16 = g.o_pair_bf16; a.q_lo = g.q_lo; a.kv_lo = g.kv_lo; a.o_scale = g.o_scale;
  return a;
}

// GemmParams of gdf_op_gemm_ex / gdf_op_gemm_kernel: M, K, OH, OW and the byte extents are derived as gdf_op_gemm_split / gdf_op_conv3x3_split / conv_in_run /
// gdf_op_gemm_mx derive them.  what == nullptr: the host-only query (no error text)
static int gemm_params(const gdf_gemm_args& a, GemmParams& g, const char* what) {
  auto bad = [&](const char* msg) { if (what) set_error(std::string(what) + ": " + msg); return GDF_ERR_ARG; };
  if (a.mode != 0 && a.mode != 1) return bad("mode is 0 (dense) or 1 (conv3)");
  if (a.N < 0 || a.a_lo < 0 || a.lda < 0) return bad("negative size");
  size_t a_bytes, w_bytes;
  if (a.mode == 1 && a.Cin <= 8) {                                               // the conv_in form: packed 8-channel pixels, 16 taps x 8 channels of weights, K = 128
    if (a.B < 0 || a.H < 0 || a.Wd < 0) return bad("negative size");
    if (a.stride != 1 || a.ups || a.pad0 || a.a_lo > 0) return bad("conv_in form (Cin <= 8): stride 1, no ups / pad0 / a_lo");
    const size_t M = (size_t)a.B * a.H * a.Wd;
    a_bytes = M * 16; w_bytes = (size_t)a.N * 256;
    g.lda = 8; g.M = (int)M; g.K = 128; g.mode = A_CONV_SMALLC; g.H = a.H; g.W = a.Wd; g.OH = a.H; g.OW = a.Wd; g.stride = 1; g.Cin = 8;
    g.rows_per_sample = a.rows_per_sample > 0 ? a.rows_per_sample : a.H * a.Wd;
  } else if (a.mode == 1) {
    if (a.B < 0 || a.H < 0 || a.Wd < 0 || (a.stride != 1 && a.stride != 2)) return bad("conv3: sizes >= 0, stride 1 or 2");
    const int IH = a.ups ? 2 * a.H : a.H, IW = a.ups ? 2 * a.Wd : a.Wd;
    const int OH = (IH - 1) / a.stride + 1, OW = (IW - 1) / a.stride + 1;
    a_bytes = ((size_t)a.B * a.H * a.Wd - 1) * a.lda * 2 + (size_t)(a.a_lo + a.Cin) * 2;
    w_bytes = (size_t)a.N * 9 * a.Cin * 2;
    g.lda = a.lda; g.M = a.B * OH * OW; g.K = 9 * a.Cin * (a.a_lo > 0 ? 2 : 1); g.mode = A_CONV3; g.H = a.H; g.W = a.Wd; g.OH = OH; g.OW = OW;
    if (a.a_lo > 0) { g.k_w = 9 * a.Cin; g.a_lo_bytes = (uint32_t)a.a_lo * 2u; }
    g.stride = a.stride; g.ups = a.ups ? 1 : 0; g.pad0 = a.pad0 ? 1 : 0; g.Cin = a.Cin;
    g.rows_per_sample = a.rows_per_sample > 0 ? a.rows_per_sample : OH * OW;
  } else if (a.mx) {                                                             // fp8 rows in 2-byte units (kernels.h GemmParams::mx), query only
    if ((a.K % 128) || (a.lda % 2)) return bad("fp8: K must be a multiple of 128, lda even");
    a_bytes = ((size_t)a.M - 1) * a.lda + (size_t)a.K; w_bytes = (size_t)a.N * a.K;
    g.lda = a.lda / 2; g.M = a.M; g.K = a.K / 2; g.mode = A_DENSE; g.mx = 1;
    g.rows_per_sample = 1;
  } else {
    a_bytes = ((size_t)a.M - 1) * a.lda * 2 + (size_t)(a.a_lo + a.K) * 2;
    w_bytes = (size_t)a.N * a.K * 2;
    g.lda = a.lda; g.M = a.M; g.K = a.a_lo > 0 ? 2 * a.K : a.K; g.mode = A_DENSE;
    if (a.a_lo > 0) { g.k_w = a.K; g.a_lo_bytes = (uint32_t)a.a_lo * 2u; }
    g.rows_per_sample = a.rows_per_sample > 0 ? a.rows_per_sample : 1;
  }
  if (g.M <= 0 || a.N == 0) { g.N = a.N; return GDF_OK; }                        // empty problem: nothing is launched
  if (!(a_bytes < (1ull << 31) && w_bytes < (1ull << 31))) {
    if (what) span_ok(a_bytes, w_bytes, what);
    return GDF_ERR_UNSUPPORTED;
  }
  g.A = (const half_t*)a.A; g.a_bytes = (uint32_t)a_bytes; g.N = a.N;
  g.Wt = (const half_t*)a.W; g.w_bytes = (uint32_t)w_bytes;
  const int Nout = a.geglu ? a.N / 2 : a.N;
  g.bias = a.bias; g.rowvec = a.rowvec; g.ldrv = a.ldrv > 0 ? a.ldrv : a.N;
  g.res32 = a.res32; g.res16 = (const half_t*)a.res16; g.ldres = a.ldres > 0 ? a.ldres : Nout;
  g.out16 = (half_t*)a.out16; g.ldo16 = a.ldo16 > 0 ? a.ldo16 : Nout; g.out32 = a.out32; g.ldo32 = a.ldo32 > 0 ? a.ldo32 : Nout;
  g.aux16 = (half_t*)a.aux16; g.ldaux = a.ldaux > 0 ? a.ldaux : Nout;
  g.geglu = a.geglu ? 16 : 0; g.bn = a.bn == 16 ? 16 : 128; g.variant = a.variant; g.no_superblock = a.no_superblock ? 1 : 0;
  g.batch = a.batch; g.w_bstride = a.w_bstride; g.o_bstride = a.o_bstride;
  g.dit = a.dit || a.mx ? 1 : 0; g.act = a.act; g.rv_mul = a.rv_mul; g.rv_seg_rows = a.rv_seg_rows; g.rv_rps2 = a.rv_rps2 > 0 ? a.rv_rps2 : 1; g.rv_tok = a.rv_tok;
  g.qkn_nq = a.qkn_nq; g.qkn_wq = a.qkn_wq; g.qkn_wk = a.qkn_wk; g.qkn_eps = a.qkn_eps; g.rope_cos = a.rope_cos; g.rope_sin = a.rope_sin;
  g.qkn_pos0 = a.qkn_pos0; g.qkn_rps = a.qkn_rps > 0 ? a.qkn_rps : 1; g.qkn_seg_rows = a.qkn_seg_rows; g.qkn_pos1 = a.qkn_pos1; g.qkn_rps2 = a.qkn_rps2 > 0 ? a.qkn_rps2 : 1;
  g.bf16 = a.bf16 || a.mx ? 1 : 0; g.out_f16 = a.out_f16;
  g.acc_scale = a.acc_scale; g.out16_scale = a.out16_scale; g.o16_lo = a.o16_lo; g.cus = a.cus;
  return GDF_OK;
}

extern "C" {

int gdf_op_attention_ex(const gdf_attn_args* args, void* stream) {
  if (!args) { set_error("gdf_op_attention_ex: args is NULL"); return GDF_ERR_ARG; }
  return fin(launch_attention(attn_params(*args), (hipStream_t)stream), "attention_ex");
}

const char* gdf_op_attention_kernel(const gdf_attn_args* args) {
  return args ? attention_kernel_name(attn_params(*args)) : nullptr;
}

int gdf_op_gemm_ex(const gdf_gemm_args* args, void* stream) {
  if (!args) { set_error("gdf_op_gemm_ex: args is NULL"); return GDF_ERR_ARG; }
  if (args->mx) { set_error("gdf_op_gemm_ex: the fp8 form is launched by gdf_op_gemm_mx (it needs the operands' scales)"); return GDF_ERR_ARG; }
  GemmParams g{};
  const int rc = gemm_params(*args, g, "gemm_ex");
  if (rc != GDF_OK) return rc;
  if (gemm_select(g).forced_missing) { set_error("gemm_ex: this form has no instantiation of the forced tile variant"); return GDF_ERR_ARG; }
  if (args->splitk > 1) return fin(launch_gemm_splitk(g, args->splitk, args->splitk_ws, (hipStream_t)stream), "gemm_ex");
  return fin(launch_gemm(g, (hipStream_t)stream), "gemm_ex");
}

const char* gdf_op_gemm_kernel(const gdf_gemm_args* args) {
  if (!args) return nullptr;
  GemmParams p{}, g{};
  if (gemm_params(*args, p, nullptr) != GDF_OK || p.M <= 0 || p.N <= 0) return nullptr;
  int splitk = args->splitk;
  if (!gemm_splitk_pass1(p, splitk, nullptr, g)) return nullptr;      // (splitk <= 1: g = p)
  const GemmSel k = gemm_select(g);
  return k.forced_missing ? nullptr : gemm_kernel_name(k);
}

int gdf_op_gemm(const void* A, int lda, const void* W, const float* bias, const float* res32, const void* res16,
                int ldres, void* out16, int ldo16, float* out32, int ldo32, int M, int N, int K, int flags,
                void* stream) {
  GemmParams g{};
  if (!span_ok(((size_t)M - 1) * lda * 2 + (size_t)K * 2, (size_t)N * K * 2, "gemm")) return GDF_ERR_UNSUPPORTED;
  g.A = (const half_t*)A; g.lda = lda; g.a_bytes = (uint32_t)(((size_t)M - 1) * lda * 2 + (size_t)K * 2);
  g.M = M; g.N = N; g.K = K; g.mode = A_DENSE;
  g.Wt = (const half_t*)W; g.w_bytes = (uint32_t)((size_t)N * K * 2);
  g.bias = bias; g.res32 = res32; g.res16 = (const half_t*)res16; g.ldres = ldres;
  g.out16 = (half_t*)out16; g.ldo16 = ldo16; g.out32 = out32; g.ldo32 = ldo32;
  g.geglu = (flags & 1) ? 16 : 0; g.bn = (flags & 2) ? 16 : 128; g.variant = (flags >> 8) & 0xfff; g.no_early_mma = (flags >> 20) & 1; g.no_superblock = (flags >> 21) & 1; g.rows_per_sample = 1;
  return fin(launch_gemm(g, (hipStream_t)stream), "gemm");
}

// GemmParams of gdf_op_conv3x3 / gdf_op_conv3x3_gn / gdf_op_conv3x3_gn_info (pointers may be null for the host-only query)
static GemmParams conv3x3_params(const void* x, int ld, int B, int H, int W, int Cin, const void* Wt, int Cout, const float* bias,
                                 const float* rowvec, int stride, int ups, const float* res32, void* aux16, void* out16,
                                 float* out32, int narrow) {
  const int IH = ups ? 2 * H : H, IW = ups ? 2 * W : W;
  const int OH = (IH - 1) / stride + 1, OW = (IW - 1) / stride + 1;
  GemmParams g{};
  g.A = (const half_t*)x; g.lda = ld; g.a_bytes = (uint32_t)(((size_t)B * H * W - 1) * ld * 2 + (size_t)Cin * 2);
  g.M = B * OH * OW; g.N = Cout; g.K = 9 * Cin; g.mode = A_CONV3; g.H = H; g.W = W; g.OH = OH; g.OW = OW;
  g.stride = stride; g.ups = ups; g.Cin = Cin;
  g.Wt = (const half_t*)Wt; g.w_bytes = (uint32_t)((size_t)Cout * 9 * Cin * 2);
  g.bias = bias; g.rowvec = rowvec; g.rows_per_sample = OH * OW; g.ldrv = Cout;
  g.res32 = res32; g.ldres = Cout;
  g.aux16 = (half_t*)aux16; g.ldaux = Cout;
  g.out16 = (half_t*)out16; g.ldo16 = Cout; g.out32 = out32; g.ldo32 = Cout;
  g.bn = (narrow & 1) ? 16 : 128; g.variant = (narrow >> 8) & 0xfff; g.no_early_mma = (narrow >> 20) & 1;
  return g;
}

int gdf_op_conv3x3(const void* x, int ld, int B, int H, int W, int Cin, const void* Wt, int Cout, const float* bias,
                   const float* rowvec, int stride, int ups, const float* res32, void* aux16, void* out16,
                   float* out32, int narrow, void* stream) {
  if (!span_ok(((size_t)B * H * W - 1) * ld * 2 + (size_t)Cin * 2, (size_t)Cout * 9 * Cin * 2, "conv3x3")) return GDF_ERR_UNSUPPORTED;
  const GemmParams g = conv3x3_params(x, ld, B, H, W, Cin, Wt, Cout, bias, rowvec, stride, ups, res32, aux16, out16, out32, narrow);
  return fin(launch_gemm(g, (hipStream_t)stream), "conv3x3");
}

int gdf_op_conv3x3_gn(const void* x, int ld, int B, int H, int W, int Cin, const void* Wt, int Cout, const float* bias,
                      const float* rowvec, int stride, int ups, const float* res32, void* aux16, void* out16,
                      float* out32, int narrow, float out16_scale, float* gn_partial, void* stream) {
  if (!gn_partial) { set_error("gdf_op_conv3x3_gn: gn_partial is NULL"); return GDF_ERR_ARG; }
  if (!span_ok(((size_t)B * H * W - 1) * ld * 2 + (size_t)Cin * 2, (size_t)Cout * 9 * Cin * 2, "conv3x3_gn")) return GDF_ERR_UNSUPPORTED;
  GemmParams g = conv3x3_params(x, ld, B, H, W, Cin, Wt, Cout, bias, rowvec, stride, ups, res32, aux16, out16, out32, narrow);
  g.out16_scale = out16_scale; g.gn_partial = gn_partial;
  return fin(launch_gemm(g, (hipStream_t)stream), "conv3x3_gn");
}

const char* gdf_op_conv3x3_gn_info(int B, int H, int W, int Cin, int Cout, int stride, int ups, int flags, int* slab_rows) {
  GemmParams g = conv3x3_params(nullptr, Cin, B, H, W, Cin, nullptr, Cout, nullptr, nullptr, stride, ups, nullptr, nullptr, nullptr, nullptr, flags);
  if (Cin <= 8) { g.mode = A_CONV_SMALLC; g.K = 128; g.Cin = 8; }                     // the conv_in form (gdf_op_conv_in_gn)
  g.gn_partial = (float*)1;                                                             // label only: never followed
  const int sr = gemm_gn_slab_rows(g);
  if (slab_rows) *slab_rows = sr;
  return sr > 0 ? gemm_kernel_name(g) : nullptr;
}

// ---- split-operand forms of the "precise" plans (kernels.h GemmParams::k_w / a_lo_bytes / o16_lo) ----
int gdf_op_gemm_split(const void* A, int lda, int a_lo, const void* W, const float* bias, const float* res32, int ldres, void* out16,
                      int ldo16, int o16_lo, float* out32, int ldo32, int M, int N, int Kw, int flags, void* stream) {
  GemmParams g{};
  const size_t a_bytes = ((size_t)M - 1) * lda * 2 + (size_t)(a_lo + Kw) * 2;
  if (!span_ok(a_bytes, (size_t)N * Kw * 2, "gemm_split")) return GDF_ERR_UNSUPPORTED;
  g.A = (const half_t*)A; g.lda = lda; g.a_bytes = (uint32_t)a_bytes;
  g.M = M; g.N = N; g.K = a_lo > 0 ? 2 * Kw : Kw; g.mode = A_DENSE;
  if (a_lo > 0) { g.k_w = Kw; g.a_lo_bytes = (uint32_t)a_lo * 2u; }
  g.Wt = (const half_t*)W; g.w_bytes = (uint32_t)((size_t)N * Kw * 2);
  g.bias = bias; g.res32 = res32; g.ldres = ldres;
  g.out16 = (half_t*)out16; g.ldo16 = ldo16; g.o16_lo = o16_lo; g.out32 = out32; g.ldo32 = ldo32;
  g.geglu = (flags & 1) ? 16 : 0; g.bn = 128; g.rows_per_sample = 1;
  return fin(launch_gemm(g, (hipStream_t)stream), "gemm_split");
}

int gdf_op_conv3x3_split(const void* x, int ld, int a_lo, int B, int H, int W, int Cin, const void* Wt, int Cout, const float* bias,
                         int stride, int ups, const float* res32, void* out16, int ldo16, int o16_lo, float* out32, void* stream) {
  const int IH = ups ? 2 * H : H, IW = ups ? 2 * W : W;
  const int OH = (IH - 1) / stride + 1, OW = (IW - 1) / stride + 1;
  GemmParams g{};
  const size_t a_bytes = ((size_t)B * H * W - 1) * ld * 2 + (size_t)(a_lo + Cin) * 2;
  if (!span_ok(a_bytes, (size_t)Cout * 9 * Cin * 2, "conv3x3_split")) return GDF_ERR_UNSUPPORTED;
  g.A = (const half_t*)x; g.lda = ld; g.a_bytes = (uint32_t)a_bytes;
  g.M = B * OH * OW; g.N = Cout; g.K = 9 * Cin * (a_lo > 0 ? 2 : 1); g.mode = A_CONV3; g.H = H; g.W = W; g.OH = OH; g.OW = OW;
  if (a_lo > 0) { g.k_w = 9 * Cin; g.a_lo_bytes = (uint32_t)a_lo * 2u; }
  g.stride = stride; g.ups = ups; g.Cin = Cin;
  g.Wt = (const half_t*)Wt; g.w_bytes = (uint32_t)((size_t)Cout * 9 * Cin * 2);
  g.bias = bias; g.rows_per_sample = OH * OW; g.res32 = res32; g.ldres = Cout;
  g.out16 = (half_t*)out16; g.ldo16 = ldo16; g.o16_lo = o16_lo; g.out32 = out32; g.ldo32 = Cout; g.bn = 128;
  return fin(launch_gemm(g, (hipStream_t)stream), "conv3x3_split");
}

int gdf_op_layernorm_split(const float* x32, int ld, int R, int C, float eps, const float* gamma, const float* beta, void* y, int ldy,
                           int y_lo, void* stream) {
  return fin(launch_layernorm(nullptr, x32, ld, R, C, eps, gamma, beta, (half_t*)y, (hipStream_t)stream, ldy, y_lo), "layernorm_split");
}

int gdf_op_groupnorm_split(const void* x16, int x_lo, const float* x32, int ld, int B, int HW, int C, int G, float eps, const float* gamma,
                           const float* beta, int silu, void* y, int ldy, int y_lo, void* scratch, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (gn_fused_slab(B, HW, C, G))
    return fin(launch_gn_fused((const half_t*)x16, x32, ld, B, HW, C, G, eps, gamma, beta, silu, (half_t*)y, s, x_lo, ldy, y_lo), "gn_fused_split");
  float* partial = (float*)scratch;
  float* ab = partial + (gn_partial_floats(B, HW, C) + 63) / 64 * 64;
  hipError_t e = launch_gn_stats((const half_t*)x16, x32, ld, B, HW, C, G, eps, gamma, beta, partial, ab, s, x_lo);
  if (e != hipSuccess) return fin(e, "gn_stats_split");
  return fin(launch_gn_apply((const half_t*)x16, x32, ld, B, HW, C, ab, silu, (half_t*)y, s, x_lo, ldy, y_lo), "gn_apply_split");
}

int gdf_op_attention_split(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* o, int ldo, int o_lo, int B,
                           int heads, int Sq, int Sk, int D, void* map, void* stream) {
  AttnParams a{};
  a.q = (const half_t*)q; a.ldq = ldq; a.k = (const half_t*)k; a.ldk = ldk; a.v = (const half_t*)v; a.ldv = ldv;
  a.o = (half_t*)o; a.ldo = ldo; a.o_lo = o_lo; a.B = B; a.heads = heads; a.Sq = Sq; a.Sk = Sk; a.D = D; a.kv_bstride = Sk;
  a.scale = 1.0f / sqrtf((float)D); a.map = (half_t*)map;
  return fin(launch_attention(a, (hipStream_t)stream), "attention_split");
}

int gdf_op_attention_pair(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, int qkv_lo, void* o, int ldo, int o_lo, int B,
                          int heads, int Sq, int Sk, int D, void* stream) {
  if (qkv_lo <= 0 || (qkv_lo & 7)) return fin(hipErrorInvalidValue, "attention_pair");
  AttnParams a{};
  a.q = (const half_t*)q; a.ldq = ldq; a.k = (const half_t*)k; a.ldk = ldk; a.v = (const half_t*)v; a.ldv = ldv; a.q_lo = a.kv_lo = qkv_lo;
  a.o = (half_t*)o; a.ldo = ldo; a.o_lo = o_lo; a.B = B; a.heads = heads; a.Sq = Sq; a.Sk = Sk; a.D = D; a.kv_bstride = Sk;
  a.scale = 1.0f / sqrtf((float)D);
  return fin(launch_attention(a, (hipStream_t)stream), "attention_pair");
}

int gdf_op_conv3x3_splitk(const void* x, int ld, int B, int H, int W, int Cin, const void* Wt, int Cout, const float* bias,
                          const float* rowvec, int stride, int ups, const float* res32, void* aux16, void* out16,
                          float* out32, int splitk, float* ws, void* stream) {
  const int IH = ups ? 2 * H : H, IW = ups ? 2 * W : W;
  const int OH = (IH - 1) / stride + 1, OW = (IW - 1) / stride + 1;
  GemmParams g{};
  if (!span_ok(((size_t)B * H * W - 1) * ld * 2 + (size_t)Cin * 2, (size_t)Cout * 9 * Cin * 2, "conv3x3_splitk")) return GDF_ERR_UNSUPPORTED;
  g.A = (const half_t*)x; g.lda = ld; g.a_bytes = (uint32_t)(((size_t)B * H * W - 1) * ld * 2 + (size_t)Cin * 2);
  g.M = B * OH * OW; g.N = Cout; g.K = 9 * Cin; g.mode = A_CONV3; g.H = H; g.W = W; g.OH = OH; g.OW = OW;
  g.stride = stride; g.ups = ups; g.Cin = Cin;
  g.Wt = (const half_t*)Wt; g.w_bytes = (uint32_t)((size_t)Cout * 9 * Cin * 2);
  g.bias = bias; g.rowvec = rowvec; g.rows_per_sample = OH * OW; g.ldrv = Cout;
  g.res32 = res32; g.ldres = Cout;
  g.aux16 = (half_t*)aux16; g.ldaux = Cout;
  g.out16 = (half_t*)out16; g.ldo16 = Cout; g.out32 = out32; g.ldo32 = Cout; g.bn = 128;
  if (splitk == 0) splitk = gemm_splitk_factor(g);          // 0: the plan builder's own choice (returned through *ws[0]? no: see gdf_op_splitk_factor)
  return fin(launch_gemm_splitk(g, splitk, ws, (hipStream_t)stream), "conv3x3_splitk");
}

int gdf_op_splitk_factor(int M, int N, int K, int conv) {
  GemmParams g{}; g.M = M; g.N = N; g.K = K; g.mode = conv ? A_CONV3 : A_DENSE; g.bn = 128;
  return gemm_splitk_factor(g);
}

static int conv_in_run(const void* x_nchw, int B, int Cin, int H, int W, const void* w_oihw, const float* bias, int Cout,
                       void* out16, void* scratch, float out16_scale, float* gn_partial, hipStream_t s, const char* what) {
  half_t* lat8 = (half_t*)scratch;
  half_t* w = (half_t*)((char*)scratch + (size_t)B * H * W * 16);
  hipError_t e = launch_pack_latents((const half_t*)x_nchw, B, Cin, H, W, lat8, nullptr, s);
  if (e != hipSuccess) return fin(e, "pack_latents");
  e = launch_relayout_conv(w_oihw, 0, w, Cout, Cin, 9, 8, 16, s);
  if (e != hipSuccess) return fin(e, "relayout");
  GemmParams g{};
  const size_t M = (size_t)B * H * W;
  g.A = lat8; g.lda = 8; g.a_bytes = (uint32_t)(M * 16);
  g.M = (int)M; g.N = Cout; g.K = 128; g.mode = A_CONV_SMALLC; g.H = H; g.W = W; g.OH = H; g.OW = W; g.stride = 1; g.Cin = 8;
  g.Wt = w; g.w_bytes = (uint32_t)((size_t)Cout * 256);
  g.bias = bias; g.out16 = (half_t*)out16; g.ldo16 = Cout; g.bn = 128; g.rows_per_sample = 1;
  g.out16_scale = out16_scale; g.gn_partial = gn_partial;
  return fin(launch_gemm(g, s), what);
}

int gdf_op_conv_in(const void* x_nchw, int B, int Cin, int H, int W, const void* w_oihw, const float* bias, int Cout,
                   void* out16, void* scratch, void* stream) {
  return conv_in_run(x_nchw, B, Cin, H, W, w_oihw, bias, Cout, out16, scratch, 0.f, nullptr, (hipStream_t)stream, "conv_in");
}

int gdf_op_conv_in_gn(const void* x_nchw, int B, int Cin, int H, int W, const void* w_oihw, const float* bias, int Cout,
                      void* out16, void* scratch, float out16_scale, float* gn_partial, void* stream) {
  if (!gn_partial) { set_error("gdf_op_conv_in_gn: gn_partial is NULL"); return GDF_ERR_ARG; }
  return conv_in_run(x_nchw, B, Cin, H, W, w_oihw, bias, Cout, out16, scratch, out16_scale, gn_partial, (hipStream_t)stream, "conv_in_gn");
}

int gdf_op_attention(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* o, int ldo,
                     int B, int heads, int Sq, int Sk, int D, void* map, void* stream) {
  AttnParams a{};
  a.q = (const half_t*)q; a.ldq = ldq; a.k = (const half_t*)k; a.ldk = ldk; a.v = (const half_t*)v; a.ldv = ldv;
  a.o = (half_t*)o; a.ldo = ldo; a.B = B; a.heads = heads; a.Sq = Sq; a.Sk = Sk; a.D = D; a.kv_bstride = Sk;
  a.scale = 1.0f / sqrtf((float)D); a.map = (half_t*)map;
  return fin(launch_attention(a, (hipStream_t)stream), "attention");
}

size_t gdf_op_groupnorm_scratch_bytes(int B, int HW, int C) { return gn_partial_floats(B, HW, C) * 4 + (size_t)B * C * 8 + 256; }

int gdf_op_groupnorm(const void* x16, const float* x32, int ld, int B, int HW, int C, int G, float eps,
                     const float* gamma, const float* beta, int silu, void* y, void* scratch, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (gn_fused_slab(B, HW, C, G))
    return fin(launch_gn_fused((const half_t*)x16, x32, ld, B, HW, C, G, eps, gamma, beta, silu, (half_t*)y, s), "gn_fused");
  float* partial = (float*)scratch;
  float* ab = partial + (gn_partial_floats(B, HW, C) + 63) / 64 * 64;
  hipError_t e = launch_gn_stats((const half_t*)x16, x32, ld, B, HW, C, G, eps, gamma, beta, partial, ab, s);
  if (e != hipSuccess) return fin(e, "gn_stats");
  return fin(launch_gn_apply((const half_t*)x16, x32, ld, B, HW, C, ab, silu, (half_t*)y, s), "gn_apply");
}

// ---- the GroupNorm producers one at a time (tests/test_gpu_groupnorm.py) ----
int gdf_op_gn_path(int B, int HW, int C, int G, int* fused_sc, int* slab_rows, int* nslab) {
  if (B < 1 || HW < 1 || C < 1 || G < 1) { set_error("gdf_op_gn_path: sizes must be positive"); return GDF_ERR_ARG; }
  const int slab = gn_stats_slab(B, HW);
  if (fused_sc) *fused_sc = gn_fused_slab(B, HW, C, G);
  if (slab_rows) *slab_rows = slab;
  if (nslab) *nslab = (HW + slab - 1) / slab;
  return GDF_OK;
}

int gdf_op_gn_stats(const void* x16, int x_lo, const float* x32, int ld, int B, int HW, int C, int G, float eps, const float* gamma,
                    const float* beta, float* partial, float* ab, void* stream) {
  return fin(launch_gn_stats((const half_t*)x16, x32, ld, B, HW, C, G, eps, gamma, beta, partial, ab, (hipStream_t)stream, x_lo), "gn_stats");
}

int gdf_op_gn_apply(const void* x16, int x_lo, const float* x32, int ld, int B, int HW, int C, const float* ab, int silu, void* y,
                    int ldy, int y_lo, void* stream) {
  return fin(launch_gn_apply((const half_t*)x16, x32, ld, B, HW, C, ab, silu, (half_t*)y, (hipStream_t)stream, x_lo, ldy, y_lo), "gn_apply");
}

int gdf_op_gn_finalize(const float* partial, int nslab, int B, int HW, int C, int G, float eps, const float* gamma, const float* beta,
                       float* ab, float* fold, void* stream) {
  return fin(launch_gn_finalize(partial, nslab, B, HW, C, G, eps, gamma, beta, ab, fold, (hipStream_t)stream), "gn_finalize");
}

size_t gdf_op_gn_fold_floats(int B, int nslab, int C) { return gn_fold_floats(B, nslab, C); }

int gdf_op_layernorm(const void* x16, const float* x32, int ld, int R, int C, float eps, const float* gamma,
                     const float* beta, void* y, void* stream) {
  return fin(launch_layernorm((const half_t*)x16, x32, ld, R, C, eps, gamma, beta, (half_t*)y, (hipStream_t)stream), "layernorm");
}

int gdf_op_copy2d(const void* s16, const float* s32, int lds, void* dst, int ldd, int R, int C, void* stream) {
  return fin(launch_copy2d((const half_t*)s16, s32, lds, (half_t*)dst, ldd, R, C, (hipStream_t)stream), "copy2d");
}

int gdf_op_copy2d_ex(const void* s16, const float* s32, int lds, void* dst, int ldd, int R, int C, int src_bf16, int sat, int s_lo, float scale,
                     void* stream) {
  return fin(launch_copy2d((const half_t*)s16, s32, lds, (half_t*)dst, ldd, R, C, (hipStream_t)stream, src_bf16, sat, s_lo, scale), "copy2d_ex");
}

// ---- the glue kernels one at a time (tests/test_gpu_glue.py) ----
int gdf_op_sinusoid(const float* t, int B, int n_per_row, int dim, float* out, int ldo, int col_off, int round_f16, float tscale, void* stream) {
  return fin(launch_sinusoid(t, B, n_per_row, dim, out, ldo, col_off, round_f16, (hipStream_t)stream, tscale), "sinusoid");
}
int gdf_op_widen(const void* x, int src_bf16, int B, int n, float* out, int ldo, int col_off, void* stream) {
  return fin(launch_widen((const half_t*)x, B, n, out, ldo, col_off, (hipStream_t)stream, src_bf16), "widen");
}
int gdf_op_silu_vec(const float* x, float* out, long n, void* stream) {
  return fin(launch_silu_vec(x, out, n, (hipStream_t)stream), "silu_vec");
}
int gdf_op_add_table(const float* table, const float* vec, int ldvec, int period, int B, long n, float* out, long ldo, void* stream) {
  return fin(launch_add_table(table, vec, ldvec, period, B, n, out, ldo, (hipStream_t)stream), "add_table");
}
int gdf_op_pack_latents(const void* x_nchw, int B, int Cin, int H, int W, void* nhwc8, void* hook_nhwc, void* stream) {
  return fin(launch_pack_latents((const half_t*)x_nchw, B, Cin, H, W, (half_t*)nhwc8, (half_t*)hook_nhwc, (hipStream_t)stream), "pack_latents");
}
int gdf_op_patchify(const void* x_nchw, int B, int Cin, int H, int W, int p, int kpad, void* out, void* stream) {
  return fin(launch_patchify((const half_t*)x_nchw, B, Cin, H, W, p, kpad, (half_t*)out, (hipStream_t)stream), "patchify");
}
int gdf_op_unpatchify(const void* x, int B, int Cout, int gh, int gw, int p, void* out_nchw, void* stream) {
  return fin(launch_unpatchify((const half_t*)x, B, Cout, gh, gw, p, (half_t*)out_nchw, (hipStream_t)stream), "unpatchify");
}
int gdf_op_vae_finish(const float* h, int B, int HW, int L, const void* wq, const float* bq, const void* eps, const void* noise, float scaling,
                      float noise_a, float noise_b, float in_scale, void* out, void* stream) {
  return fin(launch_vae_finish(h, B, HW, L, (const half_t*)wq, bq, (const half_t*)eps, (const half_t*)noise, scaling, noise_a, noise_b, in_scale,
                               (half_t*)out, (hipStream_t)stream), "vae_finish");
}
int gdf_op_vae_finish_multi(const float* h, int B, int HW, int L, const void* wq, const float* bq, const void* eps, const void* noise,
                            float scaling, int n_t, const float* noise_a, const float* noise_b, const float* in_scale, void* out, void* stream) {
  if (n_t < 1 || n_t > GDF_MAX_TIMESTEPS) { set_error("vae_finish_multi: n_t must be 1.." + std::to_string(GDF_MAX_TIMESTEPS)); return GDF_ERR_ARG; }
  if (!noise_a || !noise_b || !in_scale) { set_error("vae_finish_multi: null coefficient array"); return GDF_ERR_ARG; }
  return fin(launch_vae_finish_multi(h, B, HW, L, (const half_t*)wq, bq, (const half_t*)eps, (const half_t*)noise, scaling, n_t, noise_a,
                                     noise_b, in_scale, (half_t*)out, (long)B * L * HW, (hipStream_t)stream), "vae_finish_multi");
}
int gdf_op_vae_finish_packed(const float* h, int B, int H, int W, int L, const void* wq, const float* bq, const void* eps, const void* noise,
                             float scaling, float shift, float noise_a, float noise_b, int out_bf16, void* out, void* stream) {
  return fin(launch_vae_finish_packed(h, B, H, W, L, (const half_t*)wq, bq, (const half_t*)eps, (const half_t*)noise, scaling, shift, noise_a,
                                      noise_b, out_bf16, out, (hipStream_t)stream), "vae_finish_packed");
}
int gdf_op_vae_dec_prepare(const void* latents, const void* noise_pred, int B, int HW, int L, float c_sample, float c_eps, float inv_scaling,
                           const void* wq, const float* bq, void* nhwc8, void* stream) {
  return fin(launch_vae_dec_prepare((const half_t*)latents, (const half_t*)noise_pred, B, HW, L, c_sample, c_eps, inv_scaling, (const half_t*)wq, bq,
                                    (half_t*)nhwc8, (hipStream_t)stream), "vae_dec_prepare");
}
int gdf_op_relayout_rows_padk(const void* src, int src_f32, void* dst, int R, int ksrc, int kdst, void* stream) {
  return fin(launch_relayout_rows_padk(src, src_f32, (half_t*)dst, R, ksrc, kdst, (hipStream_t)stream), "relayout_rows_padk");
}
int gdf_op_relayout_conv(const void* src, int src_dtype, void* dst, int O, int I, int T, int ipad, int tpad, int cblk, void* stream) {
  return fin(launch_relayout_conv(src, src_dtype, (half_t*)dst, O, I, T, ipad, tpad, (hipStream_t)stream, cblk), "relayout_conv");
}
int gdf_op_relayout_rows(const void* src, int src_dtype, void* dst, int R, int K, int row_off, int geglu, int dst_bf16, void* stream) {
  return fin(launch_relayout_rows(src, src_dtype, (half_t*)dst, R, K, row_off, geglu, (hipStream_t)stream, dst_bf16), "relayout_rows");
}
int gdf_op_relayout_vec(const void* src, int src_dtype, float* dst, int R, int row_off, int geglu, void* stream) {
  return fin(launch_relayout_vec(src, src_dtype, dst, R, row_off, geglu, (hipStream_t)stream), "relayout_vec");
}

int gdf_op_relayout_conv3(const void* w, void* dst, int O, int I, void* stream) {
  return fin(launch_relayout_conv(w, 0, (half_t*)dst, O, I, 9, I, 9, (hipStream_t)stream, 64), "relayout_conv3");
}
int gdf_op_relayout_geglu(const void* w, const float* bias, void* w_dst, float* bias_dst, int R, int K, int group, void* stream) {
  hipError_t e = launch_relayout_rows(w, 0, (half_t*)w_dst, R, K, 0, group, (hipStream_t)stream);
  if (e != hipSuccess) return fin(e, "relayout_geglu");
  if (bias) e = launch_relayout_vec(bias, 1, bias_dst, R, 0, group, (hipStream_t)stream);
  return fin(e, "relayout_geglu_bias");
}

int gdf_op_small_linear(const float* x, int ldx, int M, int K, const void* W, const float* bias, int N, int silu_in,
                        int accumulate, float* out, int ldo, void* stream) {
  return fin(launch_small_linear(x, ldx, M, K, (const half_t*)W, bias, N, silu_in, accumulate, out, ldo, (hipStream_t)stream), "small_linear");
}

int gdf_op_small_linear_ex(const float* x, int ldx, int M, int K, const void* W, int w_bf16, const float* bias, int N, int silu_in,
                           int accumulate, float* out, int ldo, void* stream) {
  return fin(launch_small_linear(x, ldx, M, K, (const half_t*)W, bias, N, silu_in, accumulate, out, ldo, (hipStream_t)stream, w_bf16), "small_linear_ex");
}

int gdf_op_softmax_rows(void* x, int ld, int R, int n, float scale, void* stream) {
  return fin(launch_softmax_rows((half_t*)x, ld, R, n, scale, (hipStream_t)stream), "softmax_rows");
}

int gdf_op_sincos_pos_embed(float* out, int C, int gh, int gw, int base_size, float interpolation_scale, void* stream) {
  return fin(launch_sincos_pos_embed(out, C, gh, gw, base_size, interpolation_scale, (hipStream_t)stream), "sincos_pos_embed");
}

int gdf_op_resize_concat(const void* src, int src_f32, long sb, long sc, long sy, long sx, int B, int C, int H, int W, void* out,
                         int Ctot, int coff, int S, void* stream) {
  return fin(launch_resize_concat(src_f32 ? nullptr : (const half_t*)src, src_f32 ? (const float*)src : nullptr, sb, sc, sy, sx, B, C, H, W,
                                  (half_t*)out, Ctot, coff, S, (hipStream_t)stream), "resize_concat");
}
// ---- the feature-map ops: one map descriptor conversion and one checker per entry point ----
static AggSrc to_src(const gdf_agg_src& e) { return AggSrc{e.ptr, e.f32, e.sb, e.sc, e.sy, e.sx, e.C, e.H, e.W, e.coff}; }

// The refusals of entry point `op`.  Every check returns 0 where it passes and otherwise the code to return, with the error text set; the entry
// points call them in the order in which their refusals are documented to fire.
struct OpCheck {
  const char* op;
  int fail(int rc, const std::string& msg) const { set_error(std::string(op) + ": " + msg); return rc; }
  int bad(const std::string& msg) const { return fail(GDF_ERR_ARG, msg); }
  int big(const std::string& msg) const { return fail(GDF_ERR_UNSUPPORTED, msg); }
  int feat(const gdf_agg_src* a, const gdf_agg_src* b = nullptr) const { return (!a->ptr || (b && !b->ptr)) ? bad("null feature pointer") : 0; }
  int dims(const gdf_agg_src* a, const gdf_agg_src* b = nullptr) const {
    if (a->C < 1 || a->H < 1 || a->W < 1 || (b && (b->C < 1 || b->H < 1 || b->W < 1))) return bad("C, H and W >= 1");
    return (b && a->C != b->C) ? bad("the two maps differ in C") : 0;
  }
  int aligned(const void* ws) const { return ((uintptr_t)ws & 15) ? bad("the workspace must be 16-byte aligned") : 0; }
  int batch(int B) const { return B > 65535 ? big("B > 65535; split the batch") : 0; }
  int room(size_t have, size_t need, const char* fn) const { return have < need ? bad(std::string("workspace smaller than ") + fn + " says") : 0; }
};

int gdf_op_aggregate(const gdf_agg_src* srcs, int n, int B, void* out, int out_f32, int Ctot, int OH, int OW, int mode, void* stream) {
  const OpCheck ck{"gdf_op_aggregate"};
  if (n < 1 || n > AGG_MAX) return ck.bad("1 <= n <= 16 sources");
  if (!srcs || !out) return ck.bad("null pointer");
  if (mode != 0 && mode != 1) return ck.bad("mode is 0 (nearest) or 1 (bilinear)");
  if (B < 0 || OH < 1 || OW < 1) return ck.bad("B >= 0, OH and OW >= 1");
  if (mode == 0 && (out_f32 || OH != OW)) return ck.bad("nearest writes fp16 and a square grid (gdf_op_resize_concat's kernel)");
  size_t blocks = 0;
  AggSrc a[AGG_MAX];
  for (int k = 0; k < n; ++k) {
    const gdf_agg_src& e = srcs[k];
    if (!e.ptr) return ck.bad("null source pointer");
    if (e.C < 1 || e.H < 1 || e.W < 1) return ck.bad("C, H and W >= 1");
    if (e.coff < 0 || (long)e.coff + e.C > Ctot) return ck.bad("coff < 0 or coff + C > Ctot");
    blocks += (size_t)B * OH * ((e.C + 63) / 64);
    a[k] = to_src(e);
  }
  if (blocks >= (1ull << 31)) return ck.big("2^31 workgroups or more; split the batch");
  if (B == 0) return GDF_OK;
  if (mode == 1) return fin(launch_aggregate(a, n, B, out, out_f32, Ctot, OH, OW, (hipStream_t)stream), "gdf_op_aggregate");
  for (int k = 0; k < n; ++k) {
    const AggSrc& e = a[k];
    const hipError_t rc = launch_resize_concat(e.f32 ? nullptr : (const half_t*)e.ptr, e.f32 ? (const float*)e.ptr : nullptr, e.sb, e.sc, e.sy, e.sx,
                                               B, e.C, e.H, e.W, (half_t*)out, Ctot, e.coff, OH, (hipStream_t)stream);
    if (rc != hipSuccess) return fin(rc, "gdf_op_aggregate");
  }
  return GDF_OK;
}
size_t gdf_op_nn_match_workspace(int B, int N, int C, int h2, int w2) {
  return nn_match_workspace(std::max(B, 1), std::max(N, 1), std::max(C, 1), std::max(h2, 1), std::max(w2, 1));
}
int gdf_op_nn_match(const gdf_agg_src* f1, const gdf_agg_src* f2, int B, const float* points, int N, int LH, int LW, long long* out_yx,
                    float* out_score, void* workspace, size_t workspace_bytes, void* stream) {
  const OpCheck ck{"gdf_op_nn_match"};
  int rc;
  if (!f1 || !f2 || !points || !out_yx || !out_score || !workspace) return ck.bad("null pointer");
  if ((rc = ck.feat(f1, f2))) return rc;
  if (B < 0 || N < 1 || LH < 1 || LW < 1) return ck.bad("B >= 0, N, LH and LW >= 1");
  if ((rc = ck.dims(f1, f2)) || (rc = ck.aligned(workspace)) || (rc = ck.batch(B))) return rc;
  if ((long long)LH * LW >= (1ll << 30)) return ck.big("LH * LW >= 2^30 pixels (32-bit flat indices)");
  if ((long long)std::max(B, 1) * f2->H * f2->W >= (1ll << 31)) return ck.big("B * h2 * w2 >= 2^31; split the batch");
  if ((rc = ck.room(workspace_bytes, gdf_op_nn_match_workspace(B, N, f2->C, f2->H, f2->W), "gdf_op_nn_match_workspace"))) return rc;
  if (B == 0) return GDF_OK;
  return fin(launch_nn_match(to_src(*f1), to_src(*f2), B, points, N, LH, LW, out_yx, out_score, workspace, (hipStream_t)stream), "gdf_op_nn_match");
}
size_t gdf_op_dense_match_workspace(int B, int C, int P1, int P2, int f32_1, int f32_2) {
  return dense_match_workspace(std::max(B, 1), std::max(C, 1), std::min(std::max(P1, 1), (int)DM_MAXP), std::min(std::max(P2, 1), (int)DM_MAXP),
                               f32_1 != 0, f32_2 != 0);
}
int gdf_op_dense_match(const gdf_agg_src* f1, const gdf_agg_src* f2, int B, int* nn12, float* sim12, int* nn21, float* sim21, void* workspace,
                       size_t workspace_bytes, void* stream) {
  const OpCheck ck{"gdf_op_dense_match"};
  int rc;
  if (!f1 || !f2 || !workspace) return ck.bad("null pointer");
  if ((rc = ck.feat(f1, f2))) return rc;
  if ((!nn12) != (!sim12) || (!nn21) != (!sim21)) return ck.bad("an output pair is given whole or not at all");
  if (!nn12 && !nn21) return ck.bad("both output pairs are null");
  if (B < 0) return ck.bad("B >= 0");
  if ((rc = ck.dims(f1, f2)) || (rc = ck.aligned(workspace)) || (rc = ck.batch(B))) return rc;
  const long long P1 = (long long)f1->H * f1->W, P2 = (long long)f2->H * f2->W;
  if (P1 > DM_MAXP || P2 > DM_MAXP) return ck.big("more than 2^30 pixels in a map (32-bit indices)");
  if (((P1 + DM_TILE - 1) / DM_TILE) * ((P2 + DM_TILE - 1) / DM_TILE) >= (1ll << 31)) return ck.big("2^31 tiles or more; split a map");
  if ((rc = ck.room(workspace_bytes, gdf_op_dense_match_workspace(B, f1->C, (int)P1, (int)P2, f1->f32, f2->f32), "gdf_op_dense_match_workspace")))
    return rc;
  if (B == 0) return GDF_OK;
  return fin(launch_dense_match(to_src(*f1), to_src(*f2), B, nn12, sim12, nn21, sim21, workspace, (hipStream_t)stream), "gdf_op_dense_match");
}
size_t gdf_op_clip_loss_workspace(int B, int N, int C, int P1, int P2) {
  return clip_loss_workspace(std::max(B, 1), std::max(N, 1), std::max(C, 1), std::max(P1, 1), std::max(P2, 1));
}
// the checks the forward and the backward share; 0 = go on, -1 = B == 0 (a successful no-op)
static int clip_loss_args(const char* what, const gdf_agg_src* f1, const gdf_agg_src* f2, int B, const void* src_idx, const void* tgt_idx, int N,
                          float scale, const void* workspace, size_t workspace_bytes) {
  const OpCheck ck{what};
  int rc;
  if (!f1 || !f2 || !src_idx || !tgt_idx || !workspace) return ck.bad("null pointer");
  if ((rc = ck.feat(f1, f2))) return rc;
  if (B < 0 || N < 1) return ck.bad("B >= 0 and N >= 1");
  if ((rc = ck.dims(f1, f2))) return rc;
  if (!(scale > 0.f) || !std::isfinite(scale)) return ck.bad("the scale must be positive and finite");
  if ((rc = ck.aligned(workspace)) || (rc = ck.batch(B))) return rc;
  if ((long long)f1->H * f1->W >= (1ll << 30) || (long long)f2->H * f2->W >= (1ll << 30)) return ck.big("H * W >= 2^30 pixels (32-bit flat indices)");
  if ((rc = ck.room(workspace_bytes, gdf_op_clip_loss_workspace(B, N, f1->C, f1->H * f1->W, f2->H * f2->W), "gdf_op_clip_loss_workspace"))) return rc;
  return B == 0 ? -1 : 0;
}
int gdf_op_clip_loss(const gdf_agg_src* f1, const gdf_agg_src* f2, int B, const long long* src_idx, const long long* tgt_idx, int N, float scale,
                     float* loss, float* terms, void* workspace, size_t workspace_bytes, void* stream) {
  if (!loss) return OpCheck{"gdf_op_clip_loss"}.bad("null pointer");
  const int rc = clip_loss_args("gdf_op_clip_loss", f1, f2, B, src_idx, tgt_idx, N, scale, workspace, workspace_bytes);
  if (rc) return rc < 0 ? GDF_OK : rc;
  return fin(launch_clip_loss(to_src(*f1), to_src(*f2), B, src_idx, tgt_idx, N, scale, loss, terms, workspace, (hipStream_t)stream), "gdf_op_clip_loss");
}
int gdf_op_clip_loss_backward(const gdf_agg_src* f1, const gdf_agg_src* f2, int B, const long long* src_idx, const long long* tgt_idx, int N,
                              float scale, const float* grad_loss, float* grad_f1, float* grad_f2, void* workspace, size_t workspace_bytes,
                              void* stream) {
  if (!grad_loss) return OpCheck{"gdf_op_clip_loss_backward"}.bad("null pointer");
  const int rc = clip_loss_args("gdf_op_clip_loss_backward", f1, f2, B, src_idx, tgt_idx, N, scale, workspace, workspace_bytes);
  if (rc) return rc < 0 ? GDF_OK : rc;
  return fin(launch_clip_loss_backward(to_src(*f1), to_src(*f2), B, src_idx, tgt_idx, N, scale, grad_loss, grad_f1, grad_f2, workspace, (hipStream_t)stream),
             "gdf_op_clip_loss_backward");
}
size_t gdf_op_pca_workspace(int B, int C, int H, int W, int k, int joint) {
  (void)k;                                             // (the block always has 8 vectors)
  return pca_workspace(std::max(B, 1), std::min(std::max(C, 1), (int)PCA_MAXC), std::max(H, 1), std::max(W, 1), joint ? 1 : 0);
}
int gdf_op_pca(const gdf_agg_src* src, int B, int k, int joint, int max_iter, float tol, float* mean, float* components, float* variance,
               float* total_variance, float* projection, int* info, void* workspace, size_t workspace_bytes, void* stream) {
  const OpCheck ck{"gdf_op_pca"};
  int rc;
  if (!src || !mean || !components || !variance || !total_variance || !info || !workspace) return ck.bad("null pointer");
  if ((rc = ck.feat(src))) return rc;
  if (B < 0) return ck.bad("B >= 0");
  if ((rc = ck.dims(src))) return rc;
  if (joint != 0 && joint != 1) return ck.bad("joint is 0 or 1");
  if (k < 1 || k > 8) return ck.bad("1 <= k <= 8");
  if (max_iter < 1 || max_iter > PCA_MAXITER) return ck.bad("1 <= max_iter <= 1024");
  if (!(tol >= 0.f) || !std::isfinite(tol)) return ck.bad("tol is finite and not negative");
  if ((rc = ck.aligned(workspace))) return rc;
  const long long samples = (long long)(joint ? std::max(B, 1) : 1) * src->H * src->W;
  if (k > src->C || k > samples - 1) return ck.bad("k <= min(C, samples - 1)");
  if (src->C > PCA_MAXC) return ck.big("C > 4096");
  if ((rc = ck.batch(B))) return rc;
  if ((long long)std::max(B, 1) * src->H * src->W >= (1ll << 31)) return ck.big("B * H * W >= 2^31; split the batch");
  if ((rc = ck.room(workspace_bytes, gdf_op_pca_workspace(B, src->C, src->H, src->W, k, joint), "gdf_op_pca_workspace"))) return rc;
  if (B == 0) return GDF_OK;
  return fin(launch_pca(to_src(*src), B, k, joint, max_iter, tol, mean, components, variance, total_variance, projection, info, workspace,
                        (hipStream_t)stream), "gdf_op_pca");
}
int gdf_op_pca_rgb(const float* projection, int B, int H, int W, int joint, unsigned char* out, int OH, int OW, void* stream) {
  const OpCheck ck{"gdf_op_pca_rgb"};
  if (!projection || !out) return ck.bad("null pointer");
  if (B < 0 || H < 1 || W < 1 || OH < 1 || OW < 1) return ck.bad("B >= 0, H, W, OH and OW >= 1");
  if (joint != 0 && joint != 1) return ck.bad("joint is 0 or 1");
  if (B > 65535 || (long long)std::max(B, 1) * H * W >= (1ll << 31) || (long long)std::max(B, 1) * OH * OW >= (1ll << 31))
    return ck.big("B > 65535, B * H * W or B * OH * OW >= 2^31; split the batch");
  if (B == 0) return GDF_OK;
  return fin(launch_pca_rgb(projection, B, H, W, joint, out, OH, OW, (hipStream_t)stream), "gdf_op_pca_rgb");
}
int gdf_pixcls_create(int C, int M, int h1, int h2, int K, const float* W1, const float* b1, const float* W2, const float* b2, const float* W3,
                      const float* b3, gdf_pixcls* out) {
  const OpCheck ck{"gdf_pixcls_create"};
  if (out) *out = nullptr;
  if (!W1 || !b1 || !W2 || !b2 || !W3 || !b3 || !out) return ck.bad("null pointer");
  if (C < 1 || M < 1 || h1 < 1 || h2 < 1 || K < 1) return ck.bad("C, M, h1, h2 and K >= 1");
  if (M > PC_MAXM || K > PC_MAXK || h1 > PC_MAXH || h2 > PC_MAXH || h1 % 32 || h2 % 32)
    return ck.big("M <= 16, K <= 64, h1 and h2 multiples of 32 up to 256");
  PixCls* pc = nullptr;
  const int rc = fin(pixcls_create(C, M, h1, h2, K, W1, b1, W2, b2, W3, b3, &pc), "gdf_pixcls_create");
  if (rc == GDF_OK) *out = (gdf_pixcls)pc;
  return rc;
}
void gdf_pixcls_destroy(gdf_pixcls h) { pixcls_destroy((PixCls*)h); }
size_t gdf_pixcls_workspace(gdf_pixcls h, int B, int H, int W) {
  if (!h) return 0;
  return pixcls_workspace((const PixCls*)h, (long)std::max(B, 1) * std::max(H, 1) * std::max(W, 1));
}
int gdf_pixcls_predict(gdf_pixcls h, const gdf_agg_src* x, int B, long long* labels, float* js, uint8_t* model_labels, float* logits,
                       void* workspace, size_t workspace_bytes, void* stream) {
  const OpCheck ck{"gdf_pixcls_predict"};
  int rc;
  if (!h || !x || !labels || !workspace) return ck.bad("null pointer");
  if ((rc = ck.feat(x))) return rc;
  const PixCls* pc = (const PixCls*)h;
  if (B < 0 || x->H < 1 || x->W < 1) return ck.bad("B >= 0, H and W >= 1");
  if (x->C != pc->C) return ck.bad("the map's C differs from the ensemble's");
  if ((uintptr_t)workspace & 15) return ck.bad("workspace not 16-byte aligned");      // (this entry point's own wording)
  if ((long long)std::max(B, 1) * x->H * x->W >= (1ll << 31)) return ck.big("B * H * W >= 2^31; split the batch");
  if ((rc = ck.room(workspace_bytes, gdf_pixcls_workspace(h, B, x->H, x->W), "gdf_pixcls_workspace"))) return rc;
  if (B == 0) return GDF_OK;
  return fin(launch_pixcls(pc, to_src(*x), B, labels, js, model_labels, logits, workspace, (hipStream_t)stream), "gdf_pixcls_predict");
}
int gdf_agghead_create(int Cin, int Cout, const float* W, const float* bias, gdf_agghead* out) {
  const OpCheck ck{"gdf_agghead_create"};
  if (out) *out = nullptr;
  if (!W || !out) return ck.bad("null pointer");
  if (Cin < 1 || Cout < 1) return ck.bad("Cin and Cout >= 1");
  const size_t n = (size_t)Cout * Cin * 9;
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(W[i])) return ck.bad("a weight is not finite");
  for (int i = 0; bias && i < Cout; ++i)
    if (!std::isfinite(bias[i])) return ck.bad("a bias is not finite");
  AggHead* h = nullptr;
  const int rc = fin(agghead_create(Cin, Cout, W, bias, &h), "gdf_agghead_create");
  if (rc == GDF_OK) *out = (gdf_agghead)h;
  return rc;
}
void gdf_agghead_destroy(gdf_agghead h) { agghead_destroy((AggHead*)h); }
int gdf_agghead_forward(gdf_agghead h, const gdf_agg_src* x, int B, float* out, void* stream) {
  const OpCheck ck{"gdf_agghead_forward"};
  int rc;
  if (!h || !x || !out) return ck.bad("null pointer");
  if ((rc = ck.feat(x))) return rc;
  const AggHead* ah = (const AggHead*)h;
  if (B < 0 || x->H < 1 || x->W < 1) return ck.bad("B >= 0, H and W >= 1");
  if (x->C != ah->Cin) return ck.bad("the map's C differs from the head's Cin");
  if ((long long)std::max(B, 1) * x->H * x->W >= (1ll << 31)) return ck.bad("B * H * W >= 2^31; split the batch");
  if (B == 0) return GDF_OK;
  return fin(launch_agghead(ah, to_src(*x), B, out, (hipStream_t)stream), "gdf_agghead_forward");
}
int gdf_agghead_create_device(int Cin, int Cout, const float* W_dev, const float* bias_dev, void* stream, gdf_agghead* out) {
  const OpCheck ck{"gdf_agghead_create_device"};
  if (out) *out = nullptr;
  if (!W_dev || !out) return ck.bad("null pointer");
  if (Cin < 1 || Cout < 1) return ck.bad("Cin and Cout >= 1");
  AggHead* h = nullptr;
  const int rc = fin(agghead_create_device(Cin, Cout, W_dev, bias_dev, (hipStream_t)stream, &h), "gdf_agghead_create_device");
  if (rc == GDF_OK) *out = (gdf_agghead)h;
  return rc;
}
int gdf_agghead_update(gdf_agghead h, const float* W_dev, void* stream) {
  if (!h || !W_dev) return OpCheck{"gdf_agghead_update"}.bad("null pointer");
  return fin(agghead_update((AggHead*)h, W_dev, (hipStream_t)stream), "gdf_agghead_update");
}
size_t gdf_agghead_wgrad_workspace(int B, int Cin, int Cout, int H, int W) {
  (void)Cin;
  return agghead_wgrad_workspace(std::max(B, 1), std::max(Cout, 1), std::max(H, 1), std::max(W, 1));
}
int gdf_agghead_wgrad(const gdf_agg_src* x, int B, const float* grad_out, int Cout, float* dW, int accumulate, void* ws, size_t ws_bytes,
                      void* stream) {
  const OpCheck ck{"gdf_agghead_wgrad"};
  int rc;
  if (!x || !grad_out || !dW || !ws) return ck.bad("null pointer");
  if ((rc = ck.feat(x))) return rc;
  if (B < 0 || Cout < 1 || x->C < 1 || x->H < 1 || x->W < 1) return ck.bad("B >= 0, Cout, C, H and W >= 1");
  if ((long long)std::max(B, 1) * x->H * x->W >= (1ll << 31)) return ck.bad("B * H * W >= 2^31; split the batch");
  if ((rc = ck.aligned(ws))) return rc;
  if ((rc = ck.room(ws_bytes, gdf_agghead_wgrad_workspace(B, x->C, Cout, x->H, x->W), "gdf_agghead_wgrad_workspace"))) return rc;
  if (B == 0) return GDF_OK;
  return fin(launch_agghead_wgrad(to_src(*x), B, grad_out, Cout, dW, accumulate, ws, (hipStream_t)stream), "gdf_agghead_wgrad");
}
int gdf_op_avg_pool(const void* src, long sb, long sy, long sx, int B, int C, int H, int W, int r, void* out, void* stream) {
  return fin(launch_avg_pool((const half_t*)src, sb, sy, sx, B, C, H, W, r, (half_t*)out, (hipStream_t)stream), "avg_pool");
}
int gdf_op_maps_mean(const void* const* maps, int n, int B, int heads, int Q, int K, float* out, void* stream) {
  return fin(launch_maps_mean((const half_t* const*)maps, n, B, heads, Q, K, out, (hipStream_t)stream), "maps_mean");
}

int gdf_op_residual_add(const gdf_residual_add_item* items, int n, void* stream) {
  if (n < 0 || n > RES_ADD_MAX || (n > 0 && !items)) { set_error("gdf_op_residual_add: 0 <= n <= 16 items"); return GDF_ERR_ARG; }
  ResAddDesc d[RES_ADD_MAX];
  for (int k = 0; k < n; ++k)
    d[k] = ResAddDesc{(half_t*)items[k].dst, items[k].ld, items[k].lo, (const half_t*)items[k].res, items[k].rows, items[k].C};
  return fin(launch_residual_add(d, n, (hipStream_t)stream), "residual_add");
}

int gdf_op_cond_conv3x3(const void* x, int B, int H, int W, int Cin, int ldx, const void* w_packed, const float* bias, int Cout, int stride,
                        int silu, void* out, int ldo, int add_into, void* stream) {
  auto bad = [](const char* msg) { set_error(std::string("gdf_op_cond_conv3x3: ") + msg); return GDF_ERR_ARG; };
  if (!cond_conv_ok(Cin, Cout)) return bad("(Cin, Cout) is none of 8->16, 16->16, 16->32, 32->32, 32->96, 96->96, 96->256, 256->64n");
  if (B < 1 || H < 1 || W < 1) return bad("empty image");
  if (stride != 1 && stride != 2) return bad("stride is 1 or 2");
  if (stride == 2 && ((H | W) & 1)) return bad("stride 2 needs even H and W");
  if (ldx < Cin || ldo < Cout) return bad("leading dimension smaller than the channel count");
  if ((ldx & 7) || (ldo & 7)) return bad("leading dimensions must be multiples of 8");
  if (!x || !w_packed || !out || (((uintptr_t)x | (uintptr_t)w_packed | (uintptr_t)out | (uintptr_t)bias) & 15)) return bad("null or misaligned pointer (16 bytes)");
  if ((size_t)B * ((H - 1) / stride + 1) * ((W - 1) / stride + 1) >= (1ull << 31)) return bad("2^31 output pixels or more");
  CondConvParams p{};
  p.x = (const half_t*)x; p.w = (const half_t*)w_packed; p.bias = bias; p.out = (half_t*)out;
  p.B = B; p.H = H; p.W = W; p.Cin = Cin; p.ldx = ldx; p.Cout = Cout; p.ldo = ldo; p.stride = stride; p.silu = silu ? 1 : 0; p.add = add_into ? 1 : 0;
  return fin(launch_cond_conv3x3(p, (hipStream_t)stream), "cond_conv3x3");
}
size_t gdf_op_cond_weight_bytes(int Cin, int Cout) { return cond_conv_ok(Cin, Cout) ? cond_conv_weight_bytes(Cin, Cout) : 0; }
int gdf_op_cond_pack_weights(const void* w_oihw, int src_dtype, void* dst, int Cout, int Cin_src, int Cin, void* stream) {
  if (!w_oihw || !dst || !cond_conv_ok(Cin, Cout) || Cin_src < 1 || Cin_src > Cin || src_dtype < 0 || src_dtype > 2) {
    set_error("gdf_op_cond_pack_weights: bad arguments"); return GDF_ERR_ARG;
  }
  return fin(launch_cond_pack_weights(w_oihw, src_dtype, (half_t*)dst, Cout, Cin_src, Cin, (hipStream_t)stream), "cond_pack_weights");
}
int gdf_op_cond_pack_image(const void* x_nchw, int src_dtype, int B, int C, int H, int W, void* nhwc8, void* stream) {
  if (!x_nchw || !nhwc8 || B < 1 || H < 1 || W < 1 || C < 1 || C > 8 || (src_dtype != GDF_F16 && src_dtype != GDF_F32) || ((uintptr_t)nhwc8 & 15)) {
    set_error("gdf_op_cond_pack_image: bad arguments"); return GDF_ERR_ARG;
  }
  return fin(launch_cond_pack_image(x_nchw, src_dtype, B, C, H, W, (half_t*)nhwc8, (hipStream_t)stream), "cond_pack_image");
}

// shared argument check of the gdf_op_canny_* entries: sizes, the 32-bit label range, kinds and alignment
static int canny_check(const char* what, int B, int H, int W, const void* src, int src_kind, const void* cls, const void* dst, int dst_kind,
                       const void* workspace) {
  auto bad = [&](const char* msg) { set_error(std::string(what) + ": " + msg); return GDF_ERR_ARG; };
  if (B < 1 || H < 1 || W < 1) return bad("B, H, W >= 1");
  if ((size_t)B * H * W >= (1ull << 31)) {
    set_error(std::string(what) + ": B * H * W >= 2^31 pixels (32-bit component labels); split the batch");
    return GDF_ERR_UNSUPPORTED;
  }
  if (src_kind < GDF_CANNY_U8_HWC3 || src_kind > GDF_CANNY_F16_NCHW) return bad("src_kind is GDF_CANNY_U8_HWC3, _U8_HW, _F32_NCHW or _F16_NCHW");
  if (dst_kind != GDF_CANNY_DST_U8 && dst_kind != GDF_CANNY_DST_F16_NCHW3) return bad("dst_kind is GDF_CANNY_DST_U8 or GDF_CANNY_DST_F16_NCHW3");
  if (!src || !cls || !dst || !workspace) return bad("null pointer");
  if ((uintptr_t)src & 3) return bad("src must be 4-byte aligned");
  if (((uintptr_t)cls | (uintptr_t)dst | (uintptr_t)workspace) & 15) return bad("cls, dst and workspace must be 16-byte aligned");
  return GDF_OK;
}
static const char canny_ok_ptr[16] __attribute__((aligned(16))) = {0};   // stands in for the pointers an entry does not take

size_t gdf_op_canny_workspace_bytes(int B, int H, int W) {
  if (B < 1 || H < 1 || W < 1 || (size_t)B * H * W >= (1ull << 31)) return 0;
  return canny_workspace_bytes(B, H, W);
}
int gdf_op_canny_classify(const void* src, int src_kind, int B, int H, int W, int low, int high, void* cls, void* stream) {
  if (int rc = canny_check("gdf_op_canny_classify", B, H, W, src, src_kind, cls, canny_ok_ptr, GDF_CANNY_DST_U8, canny_ok_ptr)) return rc;
  if (low > high) std::swap(low, high);
  return fin(launch_canny_classify(src, src_kind, B, H, W, low, high, (uint8_t*)cls, (hipStream_t)stream), "canny_classify");
}
int gdf_op_canny_link(const void* cls, int B, int H, int W, void* dst, int dst_kind, void* workspace, void* stream) {
  if (int rc = canny_check("gdf_op_canny_link", B, H, W, canny_ok_ptr, GDF_CANNY_U8_HW, cls, dst, dst_kind, workspace)) return rc;
  return fin(launch_canny_link((const uint8_t*)cls, B, H, W, dst, dst_kind, workspace, (hipStream_t)stream), "canny_link");
}
int gdf_op_canny(const void* src, int src_kind, int B, int H, int W, int low, int high, void* dst, int dst_kind, void* workspace, void* stream) {
  if (int rc = canny_check("gdf_op_canny", B, H, W, src, src_kind, canny_ok_ptr, dst, dst_kind, workspace)) return rc;
  if (low > high) std::swap(low, high);
  uint8_t* cls = canny_workspace_cls(workspace, B, H, W);
  if (int rc = fin(launch_canny_classify(src, src_kind, B, H, W, low, high, cls, (hipStream_t)stream), "canny_classify")) return rc;
  return fin(launch_canny_link(cls, B, H, W, dst, dst_kind, workspace, (hipStream_t)stream), "canny_link");
}

// shared argument check of the gdf_op_pil_* entries for one axis pair: sizes, then the largest ratio the kernels' tables are sized for
static int pil_axis_check(const char* what, int in, int out) {
  if (in < 1 || out < 1) { set_error(std::string(what) + ": sizes >= 1"); return GDF_ERR_ARG; }
  if ((long long)in > 32ll * out) {
    set_error(std::string(what) + ": " + std::to_string(in) + " -> " + std::to_string(out) + " samples: in / out > 32 (ksize > 129) is not built; "
              "reduce the source on the host first");
    return GDF_ERR_UNSUPPORTED;
  }
  return GDF_OK;
}
int gdf_op_pil_coeffs(int in, int out, void* bounds, void* kk, int* ksize, void* stream) {
  if (!bounds || !kk || !ksize) { set_error("gdf_op_pil_coeffs: null pointer"); return GDF_ERR_ARG; }
  if (((uintptr_t)bounds | (uintptr_t)kk) & 3) { set_error("gdf_op_pil_coeffs: bounds and kk must be 4-byte aligned"); return GDF_ERR_ARG; }
  if (int rc = pil_axis_check("gdf_op_pil_coeffs", in, out)) return rc;
  *ksize = pil_ksize(in, out);
  return fin(launch_pil_coeffs(in, out, (int*)bounds, (int*)kk, (hipStream_t)stream), "pil_coeffs");
}
static int pil_resize_check(const char* what, int src_h, int src_w, int channels, int out_h, int out_w) {
  if (channels != 1 && channels != 3) { set_error(std::string(what) + ": channels is 1 (mode L) or 3 (mode RGB)"); return GDF_ERR_ARG; }
  if (int rc = pil_axis_check(what, src_w, out_w)) return rc;
  if (int rc = pil_axis_check(what, src_h, out_h)) return rc;
  const size_t lim = 1ull << 31;
  if ((size_t)src_h * src_w * channels >= lim || (size_t)src_h * out_w * channels >= lim || (size_t)out_h * out_w * 3 >= lim) {
    set_error(std::string(what) + ": 2^31 bytes or more in the source, the intermediate or the output (32-bit lane indices)");
    return GDF_ERR_UNSUPPORTED;
  }
  return GDF_OK;
}
size_t gdf_op_pil_resize_workspace_bytes(int src_h, int src_w, int channels, int out_h, int out_w) {
  if (pil_resize_check("gdf_op_pil_resize_workspace_bytes", src_h, src_w, channels, out_h, out_w)) return 0;
  return pil_resize_workspace_bytes(src_h, src_w, channels, out_h, out_w);
}
int gdf_op_pil_resize_u8(const void* src, int src_h, int src_w, int channels, int out_h, int out_w, void* dst_u8_hwc3, void* dst_f32_chw,
                         void* workspace, void* stream) {
  auto bad = [](const char* msg) { set_error(std::string("gdf_op_pil_resize_u8: ") + msg); return GDF_ERR_ARG; };
  if (!src || !workspace) return bad("null pointer");
  if (!dst_u8_hwc3 && !dst_f32_chw) return bad("null pointer: one of dst_u8_hwc3, dst_f32_chw is needed");
  if ((uintptr_t)dst_f32_chw & 3) return bad("dst_f32_chw must be 4-byte aligned");
  if ((uintptr_t)workspace & 15) return bad("workspace must be 16-byte aligned");
  if (int rc = pil_resize_check("gdf_op_pil_resize_u8", src_h, src_w, channels, out_h, out_w)) return rc;
  return fin(launch_pil_resize_u8((const uint8_t*)src, src_h, src_w, channels, out_h, out_w, (uint8_t*)dst_u8_hwc3, (float*)dst_f32_chw, workspace,
                                  (hipStream_t)stream), "pil_resize_u8");
}

// element type of the 16-bit operands of the MMDiT entry points below, per calling thread (GDF_F16 default)
static thread_local int g_e16_bf = 0;
int gdf_op_set_e16(int dtype) {
  if (dtype != GDF_F16 && dtype != GDF_BF16) { set_error("gdf_op_set_e16: GDF_F16 or GDF_BF16"); return GDF_ERR_ARG; }
  g_e16_bf = dtype == GDF_BF16;
  return GDF_OK;
}

int gdf_op_gemm_dit(const void* A, int lda, const void* W, const float* bias, int act, const float* vec, int ldvec, int vec_mul,
                    int rps, int seg_rows, int rps2, const float* res32, int ldres, void* aux16, int ldaux, void* out16,
                    int ldo16, float* out32, int ldo32, int M, int N, int K, int variant, void* stream) {
  GemmParams g{};
  if (!span_ok(((size_t)M - 1) * lda * 2 + (size_t)K * 2, (size_t)N * K * 2, "gemm_dit")) return GDF_ERR_UNSUPPORTED;
  g.A = (const half_t*)A; g.lda = lda; g.a_bytes = (uint32_t)(((size_t)M - 1) * lda * 2 + (size_t)K * 2);
  g.M = M; g.N = N; g.K = K; g.mode = A_DENSE;
  g.Wt = (const half_t*)W; g.w_bytes = (uint32_t)((size_t)N * K * 2);
  g.bias = bias; g.dit = 1; g.act = act; g.rowvec = vec; g.ldrv = ldvec; g.rv_mul = vec_mul; g.rows_per_sample = rps > 0 ? rps : 1;
  g.rv_seg_rows = seg_rows; g.rv_rps2 = rps2 > 0 ? rps2 : 1;
  g.res32 = res32; g.ldres = ldres; g.aux16 = (half_t*)aux16; g.ldaux = ldaux;
  g.out16 = (half_t*)out16; g.ldo16 = ldo16; g.out32 = out32; g.ldo32 = ldo32; g.bn = 128; g.variant = variant; g.bf16 = g_e16_bf;
  return fin(launch_gemm(g, (hipStream_t)stream), "gemm_dit");
}

int gdf_op_quant_rows_fp8(const void* x16, int ld, int R, int K, int src_bf16, void* q8, int ldq, float* scale, void* stream) {
  return fin(launch_quant_rows_fp8((const half_t*)x16, ld, R, K, src_bf16, (unsigned char*)q8, ldq, scale, (hipStream_t)stream), "quant_rows_fp8");
}

int gdf_op_gemm_mx(const void* A8, int lda, const float* a_scale, const void* W8, const float* w_scale, const float* bias, int act,
                   const float* res32, int ldres, void* out16, int ldo16, float* out32, int ldo32, int M, int N, int K, void* stream) {
  if ((K % 128) || (lda % 2)) { gdf::set_error("gemm_mx: K must be a multiple of 128, lda even"); return GDF_ERR_ARG; }
  GemmParams g{};
  if (!span_ok(((size_t)M - 1) * lda + (size_t)K, (size_t)N * K, "gemm_mx")) return GDF_ERR_UNSUPPORTED;
  // fp8 rows in 2-byte units (kernels.h GemmParams::mx)
  g.A = (const half_t*)A8; g.lda = lda / 2; g.a_bytes = (uint32_t)(((size_t)M - 1) * lda + (size_t)K);
  g.M = M; g.N = N; g.K = K / 2; g.mode = A_DENSE;
  g.Wt = (const half_t*)W8; g.w_bytes = (uint32_t)((size_t)N * K);
  g.bias = bias; g.dit = 1; g.act = act; g.rows_per_sample = 1; g.rv_rps2 = 1;
  g.res32 = res32; g.ldres = ldres; g.out16 = (half_t*)out16; g.ldo16 = ldo16; g.out32 = out32; g.ldo32 = ldo32; g.bn = 128; g.bf16 = 1;
  g.mx = 1; g.mx_rowscale = a_scale; g.mx_colscale = w_scale;
  return fin(launch_gemm(g, (hipStream_t)stream), "gemm_mx");
}

int gdf_op_layernorm_mod(const float* x32, int ld, int R, int C, float eps, const float* scale, const float* shift, int ldm,
                         int rps, int seg_rows, int rps2, void* y, void* stream) {
  return fin(launch_layernorm_mod(nullptr, x32, ld, R, C, eps, scale, shift, ldm, rps, seg_rows, rps2, (half_t*)y, (hipStream_t)stream,
                                  g_e16_bf), "layernorm_mod");
}

int gdf_op_layernorm_mod_ex(const void* x16, const float* x32, int ld, int R, int C, float eps, const float* scale, const float* shift,
                            int ldm, int rps, int seg_rows, int rps2, void* y, int bf16, int ldy, int y_lo, void* q8, int ldq8,
                            float* q8_scale, void* stream) {
  return fin(launch_layernorm_mod((const half_t*)x16, x32, ld, R, C, eps, scale, shift, ldm, rps, seg_rows, rps2, (half_t*)y,
                                  (hipStream_t)stream, bf16, ldy, y_lo, (unsigned char*)q8, ldq8, q8_scale), "layernorm_mod_ex");
}

int gdf_op_layernorm_mod_path(int C) { return layernorm_mod_maxc(C); }

int gdf_op_qk_norm_rope(void* x, int ld, int R, int heads, int q_col, int k_col, const float* wq, const float* wk, float eps,
                        const float* cos_t, const float* sin_t, int pos0, int rps, void* stream) {
  return fin(launch_qk_norm_rope((half_t*)x, ld, R, heads, 128, q_col, k_col, wq, wk, eps, cos_t, sin_t, pos0, rps, (hipStream_t)stream,
                                 g_e16_bf), "qk_norm_rope");
}

int gdf_op_rope_table(const float* ids, int S, int a0, int a1, int a2, float* cos_t, float* sin_t, int row0, void* stream) {
  const int ax[3] = {a0, a1, a2};
  return fin(launch_rope_table(ids, S, 3, ax, 10000.0, cos_t, sin_t, row0, (hipStream_t)stream), "rope_table");
}

int gdf_op_attention_joint(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* o, int ldo, int B,
                           int heads, int T, int S, int D, void* stream) {
  AttnParams a{};
  a.q = (const half_t*)q; a.ldq = ldq; a.k = (const half_t*)k; a.ldk = ldk; a.v = (const half_t*)v; a.ldv = ldv;
  a.o = (half_t*)o; a.ldo = ldo; a.B = B; a.heads = heads; a.Sq = T + S; a.Sk = T + S; a.D = D; a.kv_bstride = T + S;
  a.scale = 1.0f / sqrtf((float)D); a.map = nullptr; a.seg_T = T; a.bf16 = g_e16_bf;
  return fin(launch_attention(a, (hipStream_t)stream), "attention_joint");
}

int gdf_op_latent_step(float* latents_f32, const void* noise_pred, void* latents_f16, float* timesteps, void* steps, int B, int H, int W,
                       int prime, void* stream) {
  return fin(launch_latent_step(latents_f32, (const half_t*)noise_pred, (half_t*)latents_f16, timesteps, (int*)steps, B, H, W, prime,
                                (hipStream_t)stream), "latent_step");
}

int gdf_op_guided_step(float* latents_f32, const void* noise_pred, float* history, void* latents_f16, float* timesteps, void* steps, int B,
                       int H, int W, int prime, void* stream) {
  return fin(launch_guided_step(latents_f32, (const half_t*)noise_pred, history, (half_t*)latents_f16, timesteps, (int*)steps, B, H, W, prime,
                                (hipStream_t)stream), "guided_step");
}

}  // extern "C"
