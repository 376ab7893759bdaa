"""The GEMM coverage contract, checked without a GPU: every GEMM / conv kernel instantiation that a sweep of legal arguments makes launch_gemm
choose has a kernel-level case in tests/test_gpu_gemm.py (CASES) — or, for the gemm_gn_kernel forms (GroupNorm sums from the conv epilogue), in
the table of tests/test_gpu_groupnorm.py.  Uses gdf_op_gemm_kernel / gdf_op_conv3x3_gn_info only (host arithmetic, no device)."""
import ctypes
import itertools

from ops_binding import GemmArgs, lib
from test_gpu_gemm import CASES, DK, DSK, GK, MX, SK, check_case, gemm_args, kernel_name
from test_gpu_groupnorm import CONV_CASES

from components import native

ONE = ctypes.c_void_p(1)                                   # never followed: only "set or not" is read
IMG = {64: (8, 8), 200: (10, 20), 1024: (32, 32), 4096: (64, 64), 16384: (128, 128), 65536: (256, 256)}


# instantiations launch_gemm has that the sweep below does not reach, each with the reason it keeps a row
OFF_SWEEP = {
    # the 2-stage ring forms of the 256-row tiles: only a forced `variant` (320 / 1256) selects them; they are the bit-exact references
    # of the 8-phase main loops (tools and the order rows of CASES launch them)
    GK(0, 256, 320, 2), GK(1, 256, 320, 2), DK(256, 256, 2), DK(256, 256, 2, False, True), DK(256, 256, 2, True), DK(256, 256, 2, True, True),
    GK(1, 256, 128, 3),        # N <= 128 convs from 2^20 pixels up (the VAE's level-0 convs at 1024 x 1024): M is beyond the sweep
    GK(0, 128, 128, 2, True),  # GEGLU where the 256-row tiles would leave a mostly idle last round (row counts off the sweep's grid)
}


def widths():
    base = {128, 256, 512}                                 # VAE
    for cfg in native.ARCH_CONFIGS.values():
        base |= set(cfg["block_out_channels"])
    for cfg in list(native.PIXART_CONFIGS.values()) + list(native.FLUX_CONFIGS.values()):
        base.add(cfg["num_attention_heads"] * cfg["attention_head_dim"])
    return sorted({w * m for w in base for m in (1, 3, 4, 8)} | {4})


def name(L, M, N, K, conv=False, res32=False, geglu=0, bn=0, split=False, splitk=0, dit=0, bf16=0, qkn=0, cus=0, mx=0, variant=0, **kw):
    a = GemmArgs()
    a.N, a.geglu, a.bn, a.splitk, a.dit, a.bf16, a.cus, a.mx, a.variant = N, geglu, bn, splitk, dit, bf16, cus, mx, variant
    if conv:
        a.mode, a.B, (a.H, a.Wd), a.Cin, a.stride, a.lda = 1, 1, IMG[M], K, 1, 2 * K if split else K
    else:
        a.mode, a.M, a.K, a.lda = 0, M, K, 2 * K if split else K
    if res32:
        a.res32 = ONE
    if split:
        a.a_lo, a.o16_lo = K, 0 if bn == 16 else (N // 2 if geglu else N)
    a.qkn_nq = qkn
    for k, v in kw.items():
        setattr(a, k, v)
    return kernel_name(L, a)


def reachable_names(L):
    names = set()
    W = widths()
    for M, N, K, cus in itertools.product(IMG, W, W, (0, 64)):
        if K % 64:
            continue
        for conv, res32, split, splitk in itertools.product((False, True), (False, True), (False, True), (0, 4)):
            names.add(name(L, M, N, K, conv=conv, res32=res32, split=split, splitk=splitk, cus=cus))
            if not splitk and not res32:
                names.add(name(L, M, N, K, conv=conv, split=split, bn=16, cus=cus))
            if not conv and not splitk and not res32 and N % 32 == 0:
                names.add(name(L, M, N, K, geglu=1, split=split, cus=cus))
        for bf16, qkn, split in itertools.product((0, 1), (0, 128), (False, True)):
            if split and not bf16:
                continue
            names.add(name(L, M, N, K, dit=1, bf16=bf16, qkn=qkn if N >= 384 else 0, split=split, cus=cus))
        if K % 128 == 0:
            names.add(name(L, M, N, K, mx=1, cus=cus))
        if N > 4:
            names.add(name(L, M, N, 4, conv=True, cus=cus))                  # conv_in
            names.add(name(L, M, N, 4, conv=True, cus=cus, o16_lo=N))        # conv_in of a "precise" plan: plain operand, pair output
    names.discard(None)                                                      # (operands beyond 2 GiB, N = 4 on a wide tile, QKN off the 256x256 tile)
    return names


def reachable_gn_names(L):
    names = set()
    for M, N, K, ups in itertools.product(IMG, widths(), (4, 64, 128, 320, 512), (0, 1)):
        n = L.gdf_op_conv3x3_gn_info(1, IMG[M][0], IMG[M][1], K, N, 1, ups, 0, None)
        if n is not None:
            names.add(n.decode())
    return names


def test_every_case_names_the_kernel_the_query_returns():
    L = lib()
    wrong = [(c["id"], c["kernel"], kernel_name(L, gemm_args(c))) for c in CASES if kernel_name(L, gemm_args(c)) != c["kernel"]]
    assert not wrong, wrong
    assert len({c["id"] for c in CASES}) == len(CASES)


def test_reachable_kernels_are_all_kernel_tested():
    L = lib()
    tested, reachable, gn = {c["kernel"] for c in CASES}, reachable_names(L), reachable_gn_names(L)
    assert len(reachable) > 20 and gn
    report = "\ntested:\n  %s\nreachable:\n  %s\n" % tuple("\n  ".join(sorted(s)) for s in (tested, reachable))
    assert reachable <= tested, "reachable kernels without a kernel test: %s%s" % (sorted(reachable - tested), report)
    gn_tested = {c["kernel"] for c in CONV_CASES}
    assert gn <= gn_tested, "reachable gemm_gn_kernel forms without a row in the GroupNorm suite: %s" % sorted(gn - gn_tested)
    # and no row claims a kernel that nothing reaches: what the sweep does not reach is exactly the short list above
    assert tested - reachable == OFF_SWEEP, sorted((tested - reachable) ^ OFF_SWEEP)
    print("GEMM_REACHABLE\n" + "\n".join(sorted(reachable)))


VARIANT_CODES = (16, 128, 160, 256, 320, 825, 826, 932, 1256, 2128, 8256, 832)   # the eleven public codes and 832, a number that is no code


def test_forced_variants_name_only_kernel_tested_instantiations():
    """every form x every forced `variant` code: the query answers None or a kernel with a kernel-level row — nothing nameable lies outside the
    tested instantiation list (a name printed for an instantiation that does not exist would be outside it)"""
    L = lib()
    tested = {c["kernel"] for c in CASES} | {c["kernel"] for c in CONV_CASES}
    outside = []
    for v in VARIANT_CODES:
        got = {}
        for M, N, K in itertools.product((200, 4096, 16384), (128, 320, 1280, 3072), (64, 1280)):
            for split in (False, True):
                got["dense", split, M, N, K] = name(L, M, N, K, split=split, variant=v)
                got["conv3", split, M, N, K] = name(L, M, N, K, conv=True, split=split, variant=v)
                got["conv_in", split, M, N] = name(L, M, N, 4, conv=True, variant=v, **(dict(o16_lo=N) if split else {}))
                got["geglu", split, M, N, K] = name(L, M, N, K, geglu=1, split=split, variant=v)
                got["narrow", split, M, N, K] = name(L, M, N, K, conv=True, bn=16, split=split, variant=v)
            got["narrow dense", M, N, K] = name(L, M, N, K, bn=16, variant=v)
            for bf16, split, qkn in ((0, False, 0), (0, False, 128), (1, False, 0), (1, False, 128), (1, True, 0), (1, True, 128)):
                got["dit", bf16, split, qkn, M, N, K] = name(L, M, N, K, dit=1, bf16=bf16, split=split, qkn=qkn, variant=v)
            got["mx", M, N, K] = name(L, M, N, K, mx=1, variant=v)
            for cin in (4, K):
                n = L.gdf_op_conv3x3_gn_info(1, IMG[M][0], IMG[M][1], cin, N, 1, 0, v << 8, None)
                got["gn", M, N, cin] = n.decode() if n is not None else None
        assert any(n is not None for n in got.values()), v
        outside += [(v, k, n) for k, n in got.items() if n is not None and n not in tested]
    assert not outside, outside[:20]


def test_case_inputs_leave_the_bounds_their_headroom():
    """the CPU half of the small cases: the emulated contract (fp32 accumulation, one rounding) stays under a third of every per-block bound"""
    L = lib()
    bad = []
    for c in CASES:
        if c["form"] in ("conv", "conv_in_ex", "dense") and layout_elems(c) <= 1 << 18:
            try:
                check_case(c, L, gpu=False)
            except AssertionError as e:
                bad.append((c["id"], str(e)[:160]))
    assert not bad, bad


def layout_elems(c):
    from test_gpu_gemm import layout
    y = layout(c)
    return y["M"] * y["N"] * y["batch"]


def test_documented_selection_rules():
    L = lib()
    assert name(L, 16384, 640, 640, res32=True) == GK(0, 128, 160, 2)             # SDXL attention out-projection: fp32 residual, short K
    assert name(L, 16384, 1280, 1280, conv=True) == GK(1, 256, 320, 9)            # the N = 1280 conv: 8-phase 256x320
    assert name(L, 16384, 1152, 1152, dit=1) == DK(256, 256, 8)                   # PixArt: N = 1152 = 4.5 x 256, a ragged last column tile within 1/8 of padding
    assert name(L, 65536, 384, 1152, dit=1) == DK(256, 128, 3)                    # N = 3 x 128 (a third of padding on 256 columns): 256x128
    assert name(L, 4608, 3072, 3072, dit=1, bf16=1) == DK(256, 256, 8, True)      # Flux: 8-phase 256x256
    assert name(L, 4608, 9216, 3072, dit=1, bf16=1, qkn=3072) == DK(256, 256, 8, True, True)
    assert name(L, 4608, 9216, 3072, dit=1, bf16=1, qkn=3072, split=True) == DSK(256, 256, 8, True)
    assert name(L, 16384, 10240, 1280, geglu=1) == GK(0, 256, 256, 8, True)       # GEGLU 16384 x 10240 x 1280
    assert name(L, 64, 1280, 1280 * 9, splitk=4) == GK(0, 128, 160, 2)            # split-K lives on the 2-stage ring tiles
    assert name(L, 64, 256, 1280 * 9, splitk=4) == GK(0, 128, 128, 2)
    assert name(L, 16384, 4, 320, conv=True, bn=16) == GK(1, 128, 16, 2)          # conv_out
    assert name(L, 16384, 320, 4, conv=True) == GK(2, 128, 128, 2)                # conv_in (Cout = 320 scores the 256x320 tile, which conv_in does not have)
    assert name(L, 16384, 160, 4, conv=True) == GK(2, 128, 160, 2)
    assert name(L, 4608, 3072, 3072, mx=1) == MX
    assert name(L, 16384, 1280, 1280, split=True) == SK(0, 256, 320, 9)
    assert name(L, 16384, 1280, 1280, cus=64) is not None


def test_rejected_arguments_have_no_kernel():
    L = lib()
    assert name(L, 200, 128, 128) is not None
    assert name(L, 200, 128, 96) is None                                          # K % 64
    assert name(L, 200, 128, 128, bf16=1) is None                                 # bf16 without dit
    assert name(L, 4608, 9216, 3072, dit=1, qkn=3072) is not None
    assert name(L, 4608, 9216, 3072, dit=1, qkn=3000) is None                     # qkn_nq % 128
    assert name(L, 200, 128, 128, o16_lo=128) is not None
    assert name(L, 200, 128, 128, o16_lo=132) is None                             # o16_lo % 8
    assert name(L, 200, 128, 128, dit=1, out_f16=1) is None                       # out_f16 without bf16
    assert name(L, 200, 128, 128, dit=1, bf16=1, out_f16=1) is not None
    assert name(L, 200, 132, 128) is None                                         # ragged N off the BN = 16 tile
    assert name(L, 200, 128, 128, geglu=1, splitk=2) is None                      # split-K: plain epilogues only
    assert name(L, 200, 128, 128, variant=826) is None                            # a forced tile the form has no instantiation of
    assert name(L, 200, 128, 128, variant=825) is None
    assert name(L, 200, 128, 128, geglu=1, variant=160) is None
    assert name(L, 200, 128, 128, geglu=1, variant=825) is not None
    assert name(L, 200, 128, 128, conv=True, variant=825) is None
    assert name(L, 200, 128, 128, conv=True, variant=826) == GK(1, 256, 256, 8)
    assert name(L, 200, 128, 4, conv=True, a_lo=8) is None                        # conv_in: plain operand only
    assert name(L, 0, 128, 128) is None                                           # empty problem: nothing is launched
    assert name(L, 65536, 128, 24576) is None                                     # A beyond 2 GiB
    assert L.gdf_op_gemm_kernel(None) is None
