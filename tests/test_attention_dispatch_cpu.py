"""The attention coverage contract, checked without a GPU: every attention kernel instantiation that a shipped model at its
benchmark sizes, or a sweep of legal arguments, makes the dispatcher choose has a kernel-level case in
tests/test_gpu_attention.py (CASES).  Uses gdf_op_attention_kernel only (host arithmetic, no device)."""
import ctypes
import itertools

from ops_binding import AttnArgs, lib
from test_gpu_attention import AK, CASES, MK, attn_args, kernel_name

from components import native


def name(L, D, heads, B, Sq, Sk, maps=False, kv_len=False, seg_T=0, bf16=0, pair=False, **kw):
    a = AttnArgs()
    C = heads * D
    a.ldq = a.ldk = a.ldv = kw.get("ldq", 2 * C if pair else C)
    a.ldo = kw.get("ldo", C)
    a.B, a.heads, a.Sq, a.Sk, a.D, a.kv_bstride = B, heads, Sq, Sk, D, Sk
    a.seg_T, a.bf16 = seg_T, bf16
    a.q_lo = a.kv_lo = C if pair else 0
    if maps:
        a.map = ctypes.c_void_p(1)                  # never followed: only "set or not" is read
        if seg_T:
            a.map2 = ctypes.c_void_p(1)
    if kv_len:
        a.kv_len = ctypes.c_void_p(1)
    return kernel_name(L, a)


def names_tested():
    return {c["kernel"] for c in CASES}


def production_names(L):
    names = set()
    A = native.ARCH_CONFIGS
    # UNets: level i has (latent side / 2^i)^2 tokens and block_out_channels[i] / heads[i] wide heads; the mid block sits at the last level's size
    unets = [("1-5", 64, (1, 8, 32)), ("2-1", 64, (1, 8, 32)), ("xl", 128, (1, 16))]
    for key, side, batches in unets:
        cfg = A[key]
        levels = [(i, (side >> i) ** 2) for i, on in enumerate(cfg["has_attn"]) if on]
        last = len(cfg["block_out_channels"]) - 1
        levels.append((last, (side >> last) ** 2))                                     # mid block
        for (i, Sq), B, maps, pair in itertools.product(levels, batches, (False, True), (False, True)):
            heads = cfg["heads"][i]
            D = cfg["block_out_channels"][i] // heads
            for Sk in (Sq, 77):
                names.add(name(L, D, heads, B, Sq, Sk, maps=maps, pair=pair))
    for key in ("pixart-sigma",):
        cfg = native.PIXART_CONFIGS[key]
        heads, D = cfg["num_attention_heads"], cfg["attention_head_dim"]
        for B, maps in itertools.product((1, 4), (False, True)):
            names.add(name(L, D, heads, B, 4096, 4096, maps=maps))
            names.add(name(L, D, heads, B, 4096, 300, maps=maps, kv_len=True))
    cfg = native.FLUX_CONFIGS["flux"]
    heads, D = cfg["num_attention_heads"], cfg["attention_head_dim"]
    for B, maps, bf in itertools.product((1, 8), (False, True), (0, 1)):
        names.add(name(L, D, heads, B, 512 + 4096, 512 + 4096, maps=maps, seg_T=512, bf16=bf))
    return names


def reachable_names(L):
    names = set()
    sizes = (64, 100, 128, 300, 512, 1000, 1024, 4096)
    for D, Sq, Sk, BH, maps in itertools.product((32, 40, 64, 72, 80, 128, 160), sizes, sizes, (1, 8, 80, 160), (False, True)):
        forms = [dict(), dict(kv_len=True)]
        if Sq == Sk and Sq > 64:
            forms.append(dict(seg_T=64))
        if D == 128:
            forms += [dict(bf16=1), dict(bf16=1, kv_len=True)] + ([dict(bf16=1, seg_T=64)] if Sq == Sk and Sq > 64 else [])
        if 40 <= D <= 80:
            forms.append(dict(pair=True))
        for f in forms:
            names.add(name(L, D, BH if BH < 80 else BH // 16, 1 if BH < 80 else 16, Sq, Sk, maps=maps, **f))
    return names


def test_every_case_names_the_kernel_the_dispatcher_picks():
    L = lib()
    wrong = [(c["id"], c["kernel"], kernel_name(L, attn_args(c))) for c in CASES if kernel_name(L, attn_args(c)) != c["kernel"]]
    assert not wrong, wrong
    assert len({c["id"] for c in CASES}) == len(CASES)


def test_production_and_reachable_kernels_are_all_kernel_tested():
    L = lib()
    tested, production, reachable = names_tested(), production_names(L), reachable_names(L)
    assert None not in production and None not in reachable
    report = "\ntested:\n  %s\nproduction:\n  %s\nreachable:\n  %s\n" % tuple("\n  ".join(sorted(s)) for s in (tested, production, reachable))
    assert production <= tested, "production kernels without a kernel test: %s%s" % (sorted(production - tested), report)
    assert reachable <= tested, "reachable kernels without a kernel test: %s%s" % (sorted(reachable - tested), report)
    # and no row claims a kernel that nothing reaches (a stale name would make the table look wider than it is)
    assert tested <= reachable | production, "rows naming unreachable kernels: %s%s" % (sorted(tested - (reachable | production)), report)


def test_headline_shapes_take_the_kernels_the_table_says():
    """spot checks of the selection itself, from the dispatcher's documented rules"""
    L = lib()
    assert name(L, 64, 10, 16, 4096, 4096) == AK(64, 2)                       # SDXL 1024^2 self attention: 64 query rows per wave
    assert name(L, 64, 2, 1, 1024, 1024) == AK(64)                            # 16 workgroups: half-filled slots, 32 rows per wave
    assert name(L, 40, 8, 8, 4096, 77) == AK(40, 2, PV16=True)
    assert name(L, 72, 16, 4, 4096, 300, kv_len=True) == AK(72, PV16=True)
    assert name(L, 128, 24, 1, 4608, 4608, seg_T=512, bf16=1) == AK(128, 1, 8, BF=True)
    assert name(L, 128, 24, 1, 512, 512, bf16=1) == AK(128, BF=True)
    assert name(L, 40, 8, 8, 4096, 4096, maps=True) == MK(40, True, 3, True)
    assert name(L, 40, 8, 8, 4096, 77, maps=True) == MK(40, False)
    assert name(L, 64, 10, 1, 4096, 4096, pair=True) == AK(64, 1, 8, OCC=1, QKP=True)


def test_rejected_arguments_have_no_kernel():
    L = lib()
    assert name(L, 64, 2, 1, 128, 128) is not None
    assert name(L, 64, 2, 1, 128, 128, ldq=132) is None                       # ldq % 8
    assert name(L, 64, 2, 1, 128, 128, ldo=130) is None                       # ldo % 4
    assert name(L, 48, 2, 1, 128, 128) is None                                # no such head dim
    assert name(L, 64, 2, 1, 128, 128, bf16=1) is None                        # bf16: D = 128 only
    assert name(L, 128, 2, 1, 140, 140, seg_T=12, maps=True) is None          # an 8-key chunk would straddle the text / image boundary
    assert name(L, 128, 2, 1, 140, 140, seg_T=12) == AK(128)
    assert L.gdf_op_attention_kernel(None) is None
