"""Host side of the feature-map ops (no GPU): the workspace byte counts and every refusal of the C entry points of
csrc/ops_api.cpp return before any launch, so they can be pinned without a device.  WORKSPACE and REFUSALS below were recorded from the
library as it was before the helpers moved into csrc/feat_common.h and the wrappers onto one checker; a layout that shifts by a byte, a check
that fires in another order or a message that changes by a character fails here.

gdf_pixcls_workspace and the later refusals of gdf_pixcls_predict / gdf_agghead_forward need a handle, and a handle needs device memory:
they stay with tests/test_gpu_pixel_classifier.py and tests/test_gpu_agg_head.py."""
import ctypes as C

import pytest

vp, ci, sz, fp = C.c_void_p, C.c_int, C.c_size_t, C.c_float


class AggSrc(C.Structure):
    """gdf_agg_src of include/gdf_ops.h (same field order)"""
    _fields_ = [("ptr", vp), ("f32", ci), ("sb", C.c_long), ("sc", C.c_long), ("sy", C.c_long), ("sx", C.c_long),
                ("C", ci), ("H", ci), ("W", ci), ("coff", ci)]


SIGS = {
    "gdf_op_aggregate": (ci, [vp, ci, ci, vp, ci, ci, ci, ci, ci, vp]),
    "gdf_op_nn_match_workspace": (sz, [ci] * 5),
    "gdf_op_nn_match": (ci, [vp, vp, ci, vp, ci, ci, ci, vp, vp, vp, sz, vp]),
    "gdf_op_dense_match_workspace": (sz, [ci] * 6),
    "gdf_op_dense_match": (ci, [vp, vp, ci, vp, vp, vp, vp, vp, sz, vp]),
    "gdf_op_clip_loss_workspace": (sz, [ci] * 5),
    "gdf_op_clip_loss": (ci, [vp, vp, ci, vp, vp, ci, fp, vp, vp, vp, sz, vp]),
    "gdf_op_clip_loss_backward": (ci, [vp, vp, ci, vp, vp, ci, fp, vp, vp, vp, vp, sz, vp]),
    "gdf_op_pca_workspace": (sz, [ci] * 6),
    "gdf_op_pca": (ci, [vp, ci, ci, ci, ci, fp, vp, vp, vp, vp, vp, vp, vp, sz, vp]),
    "gdf_op_pca_rgb": (ci, [vp, ci, ci, ci, ci, vp, ci, ci, vp]),
    "gdf_pixcls_create": (ci, [ci] * 5 + [vp] * 7),
    "gdf_pixcls_workspace": (sz, [vp, ci, ci, ci]),
    "gdf_pixcls_predict": (ci, [vp, vp, ci, vp, vp, vp, vp, vp, sz, vp]),
    "gdf_agghead_create": (ci, [ci, ci, vp, vp, vp]),
    "gdf_agghead_forward": (ci, [vp, vp, ci, vp, vp]),
    "gdf_agghead_create_device": (ci, [ci, ci, vp, vp, vp, vp]),
    "gdf_agghead_update": (ci, [vp, vp, vp]),
    "gdf_agghead_wgrad_workspace": (sz, [ci] * 5),
    "gdf_agghead_wgrad": (ci, [vp, ci, vp, ci, vp, ci, vp, sz, vp]),
}


def bind(path):
    L = C.CDLL(path)
    for n, (r, a) in SIGS.items():
        f = getattr(L, n)
        f.restype, f.argtypes = r, a
    L.gdf_last_error.restype = C.c_char_p
    return L


# ---- workspace byte counts: (function, arguments).  N at 1, 4, 24, 25 and 49 (a full and a partial chunk of 24 queries), C off the multiples
# of 8, B = 0 (the wrappers clamp to 1) and the largest sizes DESIGN.md 3.24-3.30 quote ----
WS_CASES = (
    [("gdf_op_nn_match_workspace", (B, N, Cc, h, w)) for B, N, Cc, h, w in
     [(1, 1, 8, 4, 4), (2, 4, 40, 12, 12), (2, 24, 77, 16, 16), (2, 25, 77, 16, 16), (1, 49, 1283, 9, 7), (0, 5, 8, 4, 4), (0, 0, 0, 0, 0),
      (3, 17, 384, 32, 32), (2, 12, 1280, 64, 64), (65535, 1, 1, 1, 1), (2, 49, 3680, 128, 128), (1, 24, 7360, 128, 128)]] +
    [("gdf_op_dense_match_workspace", a) for a in
     [(1, 8, 16, 16, 0, 0), (2, 8, 16, 16, 0, 0), (2, 40, 144, 144, 0, 1), (2, 77, 256, 257, 1, 0), (1, 65, 255, 1, 1, 1), (0, 8, 16, 16, 0, 0),
      (0, 0, 0, 0, 0, 0), (3, 64, 1024, 4096, 0, 0), (1, 1283, 63, 513, 1, 1), (2, 3680, 16384, 16384, 1, 1), (1, 7360, 16384, 16384, 0, 0),
      (1, 8, 1 << 30, 1 << 30, 0, 0), (1, 8, 2147483647, 5, 0, 0)]] +
    [("gdf_op_clip_loss_workspace", (B, N, Cc, P1, P2)) for B, N, Cc, P1, P2 in
     [(1, 1, 8, 16, 16), (2, 4, 40, 144, 100), (2, 24, 77, 256, 256), (2, 25, 77, 256, 255), (1, 49, 1283, 63, 1025), (0, 5, 8, 16, 16),
      (0, 0, 0, 0, 0), (3, 48, 384, 1024, 1024), (2, 72, 64, 4096, 64), (2, 73, 3, 1, 1), (2, 49, 3680, 16384, 16384), (16, 24, 3680, 4096, 4096)]] +
    [("gdf_op_pca_workspace", a) for a in
     [(1, 8, 4, 4, 3, 0), (2, 77, 64, 64, 3, 0), (2, 77, 64, 64, 3, 1), (3, 129, 7, 9, 8, 0), (0, 8, 4, 4, 3, 0), (0, 0, 0, 0, 0, 0), (1, 320, 32, 32, 3, 0),
      (4, 1280, 16, 16, 3, 1), (1, 1280, 32, 32, 3, 0), (1, 1280, 64, 64, 3, 0), (1, 1280, 128, 128, 3, 0), (1, 3520, 128, 128, 3, 0),
      (1, 4096, 128, 128, 3, 0), (1, 5000, 8, 8, 3, 0), (64, 96, 128, 128, 1, 1)]] +
    [("gdf_agghead_wgrad_workspace", (B, Cin, Cout, H, W)) for B, Cin, Cout, H, W in
     [(1, 8, 1, 1, 1), (2, 40, 33, 5, 33), (2, 77, 128, 32, 32), (1, 8, 129, 4, 32), (3, 64, 31, 7, 65), (0, 8, 8, 4, 4), (0, 0, 0, 0, 0),
      (2, 384, 384, 64, 64), (1, 3520, 3520, 128, 128), (1, 3840, 3840, 128, 128), (2, 7360, 3680, 128, 128), (4, 7360, 3680, 128, 128)]] +
    [("gdf_pixcls_workspace", (None, 2, 4, 4))]                                 # (a null handle: 0)
)

FEAT, WS, ODD, BIG = 0x10000, 0x20000, 0x20008, 1 << 60                         # pointers no refusal dereferences; ODD: not 16-byte aligned


def src(ptr=FEAT, Cc=8, H=4, W=4, f32=0):
    s = AggSrc()
    s.ptr, s.f32, s.sb, s.sc, s.sy, s.sx, s.C, s.H, s.W, s.coff = ptr, f32, Cc * H * W, H * W, W, 1, Cc, H, W, 0
    return s


def refusal_cases(L):
    """name -> a call that is refused (or, for B = 0, succeeds) before any launch; the order of the names is the order of the checks"""
    a, b, nul = src(), src(), src(ptr=None)
    A, Bp = C.addressof(a), C.addressof(b)
    keep = [a, b, nul]
    cases = {}

    def two(key, call, ws_bytes):
        """the checks the two-map ops share; call(f1, f2, B, ws, bytes)"""
        def with_b(**kw):
            t = src(**kw)
            keep.append(t)
            return C.addressof(t)
        cases[key + ":null"] = lambda: call(None, Bp, 2, WS, BIG)
        cases[key + ":null-ws"] = lambda: call(A, Bp, 2, None, BIG)
        cases[key + ":null-feature"] = lambda: call(A, C.addressof(nul), 2, WS, BIG)
        cases[key + ":B<0"] = lambda: call(A, Bp, -1, WS, BIG)
        cases[key + ":H<1"] = lambda: call(A, with_b(H=0), 2, WS, BIG)
        cases[key + ":C-differs"] = lambda: call(A, with_b(Cc=9), 2, WS, BIG)
        cases[key + ":misaligned"] = lambda: call(A, Bp, 2, ODD, BIG)
        cases[key + ":B>65535"] = lambda: call(A, Bp, 65536, WS, BIG)
        cases[key + ":B>65535-before-small-ws"] = lambda: call(A, Bp, 65536, WS, 0)
        cases[key + ":small-ws"] = lambda: call(A, Bp, 2, WS, ws_bytes - 1)
        cases[key + ":C-differs-before-misaligned"] = lambda: call(A, with_b(Cc=9), 2, ODD, 0)
        cases[key + ":B=0"] = lambda: call(A, Bp, 0, WS, BIG)

    # gdf_op_aggregate
    def agg(n=1, B=2, out=WS, f32=0, Ctot=8, OH=8, OW=8, mode=1, s=a):
        return L.gdf_op_aggregate(C.addressof(s) if s is not None else None, n, B, out, f32, Ctot, OH, OW, mode, None)
    cases["aggregate:n=0"] = lambda: agg(n=0)
    cases["aggregate:n=17"] = lambda: agg(n=17)
    cases["aggregate:null"] = lambda: agg(out=None)
    cases["aggregate:mode"] = lambda: agg(mode=2)
    cases["aggregate:OH<1"] = lambda: agg(OH=0)
    cases["aggregate:nearest-f32"] = lambda: agg(mode=0, f32=1)
    cases["aggregate:null-source"] = lambda: agg(s=nul)
    cases["aggregate:C<1"] = lambda: agg(s=keep.append(src(Cc=0)) or keep[-1])
    cases["aggregate:coff"] = lambda: agg(Ctot=7)
    cases["aggregate:2^31-workgroups"] = lambda: agg(B=1 << 20, OH=1 << 12)
    cases["aggregate:B=0"] = lambda: agg(B=0)

    # gdf_op_nn_match
    def nn(f1, f2, B, ws, nb, pts=WS, N=5, LH=16, LW=16):
        return L.gdf_op_nn_match(f1, f2, B, pts, N, LH, LW, WS, WS, ws, nb, None)
    two("nn_match", nn, L.gdf_op_nn_match_workspace(2, 5, 8, 4, 4))
    cases["nn_match:null-points"] = lambda: nn(A, Bp, 2, WS, BIG, pts=None)
    cases["nn_match:N<1"] = lambda: nn(A, Bp, 2, WS, BIG, N=0)
    cases["nn_match:LH*LW"] = lambda: nn(A, Bp, 2, WS, BIG, LH=1 << 15, LW=1 << 15)

    # gdf_op_dense_match
    def dm(f1, f2, B, ws, nb, nn12=WS, sim12=WS, nn21=WS, sim21=WS):
        return L.gdf_op_dense_match(f1, f2, B, nn12, sim12, nn21, sim21, ws, nb, None)
    two("dense_match", dm, L.gdf_op_dense_match_workspace(2, 8, 16, 16, 0, 0))
    cases["dense_match:half-pair"] = lambda: dm(A, Bp, 2, WS, BIG, nn12=None)
    cases["dense_match:no-output"] = lambda: dm(A, Bp, 2, WS, BIG, nn12=None, sim12=None, nn21=None, sim21=None)
    cases["dense_match:half-pair-before-B<0"] = lambda: dm(A, Bp, -1, WS, BIG, sim21=None)

    # gdf_op_clip_loss / gdf_op_clip_loss_backward
    def cl(f1, f2, B, ws, nb, idx=WS, N=5, scale=14.0, loss=WS):
        return L.gdf_op_clip_loss(f1, f2, B, idx, WS, N, scale, loss, None, ws, nb, None)

    def clb(f1, f2, B, ws, nb, idx=WS, N=5, scale=14.0, gl=WS):
        return L.gdf_op_clip_loss_backward(f1, f2, B, idx, WS, N, scale, gl, WS, WS, ws, nb, None)
    nb_cl = L.gdf_op_clip_loss_workspace(2, 5, 8, 16, 16)
    two("clip_loss", cl, nb_cl)
    two("clip_loss_backward", clb, nb_cl)
    for key, f, out in (("clip_loss", cl, "loss"), ("clip_loss_backward", clb, "gl")):
        cases[key + ":null-" + out] = lambda f=f, out=out: f(None, None, 2, None, 0, **{out: None})
        cases[key + ":null-idx"] = lambda f=f: f(A, Bp, 2, WS, BIG, idx=None)
        cases[key + ":N<1"] = lambda f=f: f(A, Bp, 2, WS, BIG, N=0)
        cases[key + ":scale=0"] = lambda f=f: f(A, Bp, 2, WS, BIG, scale=0.0)
        cases[key + ":scale=inf"] = lambda f=f: f(A, Bp, 2, WS, BIG, scale=float("inf"))
        cases[key + ":scale-before-misaligned"] = lambda f=f: f(A, Bp, 2, ODD, BIG, scale=-1.0)

    # gdf_op_pca / gdf_op_pca_rgb
    def pca(s=a, B=2, k=3, joint=0, it=64, tol=1e-6, mean=WS, ws=WS, nb=BIG):
        return L.gdf_op_pca(C.addressof(s) if s is not None else None, B, k, joint, it, tol, mean, WS, WS, WS, None, WS, ws, nb, None)
    big_c, one_px = src(Cc=5000), src(H=1, W=1)
    keep.extend([big_c, one_px])
    cases["pca:null"] = lambda: pca(mean=None)
    cases["pca:null-src"] = lambda: pca(s=None)
    cases["pca:null-feature"] = lambda: pca(s=nul)
    cases["pca:B<0"] = lambda: pca(B=-1)
    cases["pca:W<1"] = lambda: pca(s=keep.append(src(W=0)) or keep[-1])
    cases["pca:joint"] = lambda: pca(joint=2)
    cases["pca:k=0"] = lambda: pca(k=0)
    cases["pca:k=9"] = lambda: pca(k=9)
    cases["pca:max_iter"] = lambda: pca(it=1025)
    cases["pca:tol"] = lambda: pca(tol=-1.0)
    cases["pca:misaligned"] = lambda: pca(ws=ODD)
    cases["pca:k>samples-1"] = lambda: pca(s=one_px, k=1)
    cases["pca:C>4096"] = lambda: pca(s=big_c)
    cases["pca:B>65535"] = lambda: pca(B=65536)
    cases["pca:small-ws"] = lambda: pca(nb=L.gdf_op_pca_workspace(2, 8, 4, 4, 3, 0) - 1)
    cases["pca:joint-before-k"] = lambda: pca(joint=-1, k=0)
    cases["pca:B=0"] = lambda: pca(B=0)

    def rgb(proj=WS, B=2, H=4, W=4, joint=0, out=WS, OH=8, OW=8):
        return L.gdf_op_pca_rgb(proj, B, H, W, joint, out, OH, OW, None)
    cases["pca_rgb:null"] = lambda: rgb(out=None)
    cases["pca_rgb:OW<1"] = lambda: rgb(OW=0)
    cases["pca_rgb:joint"] = lambda: rgb(joint=3)
    cases["pca_rgb:B>65535"] = lambda: rgb(B=65536)
    cases["pca_rgb:2^31"] = lambda: rgb(B=2, OH=1 << 15, OW=1 << 15)
    cases["pca_rgb:B=0"] = lambda: rgb(B=0)

    # gdf_pixcls_create / gdf_pixcls_predict (the refusals that need no handle)
    hout = vp()
    keep.append(hout)

    def pcc(Cc=8, M=2, h1=128, h2=32, K=4, W1=WS, out=C.addressof(hout)):
        return L.gdf_pixcls_create(Cc, M, h1, h2, K, W1, WS, WS, WS, WS, WS, out)
    cases["pixcls_create:null"] = lambda: pcc(W1=None)
    cases["pixcls_create:null-out"] = lambda: pcc(out=None)
    cases["pixcls_create:M<1"] = lambda: pcc(M=0)
    cases["pixcls_create:M>16"] = lambda: pcc(M=17)
    cases["pixcls_create:K>64"] = lambda: pcc(K=65)
    cases["pixcls_create:h1%32"] = lambda: pcc(h1=100)
    cases["pixcls_create:h2>256"] = lambda: pcc(h2=288)
    cases["pixcls_predict:null"] = lambda: L.gdf_pixcls_predict(None, A, 2, WS, None, None, None, WS, BIG, None)

    # gdf_agghead_*
    import array
    wts = array.array("f", [0.5] * (2 * 3 * 9))
    nan = array.array("f", [0.5] * (2 * 3 * 9 - 1) + [float("nan")])
    bias_inf = array.array("f", [0.0, float("inf")])
    keep.extend([wts, nan, bias_inf])
    adr = lambda arr: arr.buffer_info()[0]
    cases["agghead_create:null"] = lambda: L.gdf_agghead_create(3, 2, None, None, C.addressof(hout))
    cases["agghead_create:null-out"] = lambda: L.gdf_agghead_create(3, 2, adr(wts), None, None)
    cases["agghead_create:Cin<1"] = lambda: L.gdf_agghead_create(0, 2, adr(wts), None, C.addressof(hout))
    cases["agghead_create:nan-weight"] = lambda: L.gdf_agghead_create(3, 2, adr(nan), None, C.addressof(hout))
    cases["agghead_create:inf-bias"] = lambda: L.gdf_agghead_create(3, 2, adr(wts), adr(bias_inf), C.addressof(hout))
    cases["agghead_forward:null"] = lambda: L.gdf_agghead_forward(None, A, 2, WS, None)
    cases["agghead_create_device:null"] = lambda: L.gdf_agghead_create_device(3, 2, None, None, None, C.addressof(hout))
    cases["agghead_create_device:Cout<1"] = lambda: L.gdf_agghead_create_device(3, 0, WS, None, None, C.addressof(hout))
    cases["agghead_update:null"] = lambda: L.gdf_agghead_update(None, WS, None)

    def wg(s=a, B=2, g=WS, Cout=4, ws=WS, nb=BIG):
        return L.gdf_agghead_wgrad(C.addressof(s) if s is not None else None, B, g, Cout, WS, 0, ws, nb, None)
    cases["agghead_wgrad:null"] = lambda: wg(g=None)
    cases["agghead_wgrad:null-x"] = lambda: wg(s=None)
    cases["agghead_wgrad:null-feature"] = lambda: wg(s=nul)
    cases["agghead_wgrad:B<0"] = lambda: wg(B=-1)
    cases["agghead_wgrad:Cout<1"] = lambda: wg(Cout=0)
    cases["agghead_wgrad:2^31"] = lambda: wg(s=keep.append(src(H=1 << 15, W=1 << 15)) or keep[-1])
    cases["agghead_wgrad:misaligned"] = lambda: wg(ws=ODD)
    cases["agghead_wgrad:small-ws"] = lambda: wg(nb=L.gdf_agghead_wgrad_workspace(2, 8, 4, 4, 4) - 1)
    cases["agghead_wgrad:2^31-before-misaligned"] = lambda: wg(s=keep.append(src(H=1 << 15, W=1 << 15)) or keep[-1], ws=ODD)
    cases["agghead_wgrad:B=0"] = lambda: wg(B=0)
    return cases


def collect(L):
    """(workspace byte counts, refusals) of library L in the form of WORKSPACE and REFUSALS"""
    ws = [int(getattr(L, fn)(*args)) for fn, args in WS_CASES]
    ref = {}
    for name, call in refusal_cases(L).items():
        rc = int(call())
        ref[name] = (rc, L.gdf_last_error().decode() if rc else "")
    return ws, ref


# ---- recorded from the parent commit's build (collect() above on that library) ----
WORKSPACE = [34048, 80896, 473856, 473856, 328448, 67072, 33792, 928000, 975104, 2152693760, 5294336, 3000576, 75776, 151552, 217088, 563200, 272384, 75776,
 75776, 3600384, 5533696, 1040449536, 516030464, 144115471543697408, 176093692928, 5376, 22528, 253696, 295168, 3437312, 5888, 5376, 8733952, 3139328,
 19712, 65949952, 205310208, 144640, 8546048, 4273664, 2042624, 144640, 144640, 13211904, 35518464, 35518464, 42727424, 42727424, 104954624,
 136725504, 102122496, 4273664, 16896, 262656, 1049600, 83456, 295424, 16896, 16896, 12585984, 230714880, 251688960, 482374656, 964719616, 0]
REFUSALS = {'aggregate:n=0': (1, 'gdf_op_aggregate: 1 <= n <= 16 sources'),
 'aggregate:n=17': (1, 'gdf_op_aggregate: 1 <= n <= 16 sources'),
 'aggregate:null': (1, 'gdf_op_aggregate: null pointer'),
 'aggregate:mode': (1, 'gdf_op_aggregate: mode is 0 (nearest) or 1 (bilinear)'),
 'aggregate:OH<1': (1, 'gdf_op_aggregate: B >= 0, OH and OW >= 1'),
 'aggregate:nearest-f32': (1, "gdf_op_aggregate: nearest writes fp16 and a square grid (gdf_op_resize_concat's kernel)"),
 'aggregate:null-source': (1, 'gdf_op_aggregate: null source pointer'),
 'aggregate:C<1': (1, 'gdf_op_aggregate: C, H and W >= 1'),
 'aggregate:coff': (1, 'gdf_op_aggregate: coff < 0 or coff + C > Ctot'),
 'aggregate:2^31-workgroups': (4, 'gdf_op_aggregate: 2^31 workgroups or more; split the batch'),
 'aggregate:B=0': (0, ''),
 'nn_match:null': (1, 'gdf_op_nn_match: null pointer'),
 'nn_match:null-ws': (1, 'gdf_op_nn_match: null pointer'),
 'nn_match:null-feature': (1, 'gdf_op_nn_match: null feature pointer'),
 'nn_match:B<0': (1, 'gdf_op_nn_match: B >= 0, N, LH and LW >= 1'),
 'nn_match:H<1': (1, 'gdf_op_nn_match: C, H and W >= 1'),
 'nn_match:C-differs': (1, 'gdf_op_nn_match: the two maps differ in C'),
 'nn_match:misaligned': (1, 'gdf_op_nn_match: the workspace must be 16-byte aligned'),
 'nn_match:B>65535': (4, 'gdf_op_nn_match: B > 65535; split the batch'),
 'nn_match:B>65535-before-small-ws': (4, 'gdf_op_nn_match: B > 65535; split the batch'),
 'nn_match:small-ws': (1, 'gdf_op_nn_match: workspace smaller than gdf_op_nn_match_workspace says'),
 'nn_match:C-differs-before-misaligned': (1, 'gdf_op_nn_match: the two maps differ in C'),
 'nn_match:B=0': (0, ''),
 'nn_match:null-points': (1, 'gdf_op_nn_match: null pointer'),
 'nn_match:N<1': (1, 'gdf_op_nn_match: B >= 0, N, LH and LW >= 1'),
 'nn_match:LH*LW': (4, 'gdf_op_nn_match: LH * LW >= 2^30 pixels (32-bit flat indices)'),
 'dense_match:null': (1, 'gdf_op_dense_match: null pointer'),
 'dense_match:null-ws': (1, 'gdf_op_dense_match: null pointer'),
 'dense_match:null-feature': (1, 'gdf_op_dense_match: null feature pointer'),
 'dense_match:B<0': (1, 'gdf_op_dense_match: B >= 0'),
 'dense_match:H<1': (1, 'gdf_op_dense_match: C, H and W >= 1'),
 'dense_match:C-differs': (1, 'gdf_op_dense_match: the two maps differ in C'),
 'dense_match:misaligned': (1, 'gdf_op_dense_match: the workspace must be 16-byte aligned'),
 'dense_match:B>65535': (4, 'gdf_op_dense_match: B > 65535; split the batch'),
 'dense_match:B>65535-before-small-ws': (4, 'gdf_op_dense_match: B > 65535; split the batch'),
 'dense_match:small-ws': (1, 'gdf_op_dense_match: workspace smaller than gdf_op_dense_match_workspace says'),
 'dense_match:C-differs-before-misaligned': (1, 'gdf_op_dense_match: the two maps differ in C'),
 'dense_match:B=0': (0, ''),
 'dense_match:half-pair': (1, 'gdf_op_dense_match: an output pair is given whole or not at all'),
 'dense_match:no-output': (1, 'gdf_op_dense_match: both output pairs are null'),
 'dense_match:half-pair-before-B<0': (1, 'gdf_op_dense_match: an output pair is given whole or not at all'),
 'clip_loss:null': (1, 'gdf_op_clip_loss: null pointer'),
 'clip_loss:null-ws': (1, 'gdf_op_clip_loss: null pointer'),
 'clip_loss:null-feature': (1, 'gdf_op_clip_loss: null feature pointer'),
 'clip_loss:B<0': (1, 'gdf_op_clip_loss: B >= 0 and N >= 1'),
 'clip_loss:H<1': (1, 'gdf_op_clip_loss: C, H and W >= 1'),
 'clip_loss:C-differs': (1, 'gdf_op_clip_loss: the two maps differ in C'),
 'clip_loss:misaligned': (1, 'gdf_op_clip_loss: the workspace must be 16-byte aligned'),
 'clip_loss:B>65535': (4, 'gdf_op_clip_loss: B > 65535; split the batch'),
 'clip_loss:B>65535-before-small-ws': (4, 'gdf_op_clip_loss: B > 65535; split the batch'),
 'clip_loss:small-ws': (1, 'gdf_op_clip_loss: workspace smaller than gdf_op_clip_loss_workspace says'),
 'clip_loss:C-differs-before-misaligned': (1, 'gdf_op_clip_loss: the two maps differ in C'),
 'clip_loss:B=0': (0, ''),
 'clip_loss_backward:null': (1, 'gdf_op_clip_loss_backward: null pointer'),
 'clip_loss_backward:null-ws': (1, 'gdf_op_clip_loss_backward: null pointer'),
 'clip_loss_backward:null-feature': (1, 'gdf_op_clip_loss_backward: null feature pointer'),
 'clip_loss_backward:B<0': (1, 'gdf_op_clip_loss_backward: B >= 0 and N >= 1'),
 'clip_loss_backward:H<1': (1, 'gdf_op_clip_loss_backward: C, H and W >= 1'),
 'clip_loss_backward:C-differs': (1, 'gdf_op_clip_loss_backward: the two maps differ in C'),
 'clip_loss_backward:misaligned': (1, 'gdf_op_clip_loss_backward: the workspace must be 16-byte aligned'),
 'clip_loss_backward:B>65535': (4, 'gdf_op_clip_loss_backward: B > 65535; split the batch'),
 'clip_loss_backward:B>65535-before-small-ws': (4, 'gdf_op_clip_loss_backward: B > 65535; split the batch'),
 'clip_loss_backward:small-ws': (1, 'gdf_op_clip_loss_backward: workspace smaller than gdf_op_clip_loss_workspace says'),
 'clip_loss_backward:C-differs-before-misaligned': (1, 'gdf_op_clip_loss_backward: the two maps differ in C'),
 'clip_loss_backward:B=0': (0, ''),
 'clip_loss:null-loss': (1, 'gdf_op_clip_loss: null pointer'),
 'clip_loss:null-idx': (1, 'gdf_op_clip_loss: null pointer'),
 'clip_loss:N<1': (1, 'gdf_op_clip_loss: B >= 0 and N >= 1'),
 'clip_loss:scale=0': (1, 'gdf_op_clip_loss: the scale must be positive and finite'),
 'clip_loss:scale=inf': (1, 'gdf_op_clip_loss: the scale must be positive and finite'),
 'clip_loss:scale-before-misaligned': (1, 'gdf_op_clip_loss: the scale must be positive and finite'),
 'clip_loss_backward:null-gl': (1, 'gdf_op_clip_loss_backward: null pointer'),
 'clip_loss_backward:null-idx': (1, 'gdf_op_clip_loss_backward: null pointer'),
 'clip_loss_backward:N<1': (1, 'gdf_op_clip_loss_backward: B >= 0 and N >= 1'),
 'clip_loss_backward:scale=0': (1, 'gdf_op_clip_loss_backward: the scale must be positive and finite'),
 'clip_loss_backward:scale=inf': (1, 'gdf_op_clip_loss_backward: the scale must be positive and finite'),
 'clip_loss_backward:scale-before-misaligned': (1, 'gdf_op_clip_loss_backward: the scale must be positive and finite'),
 'pca:null': (1, 'gdf_op_pca: null pointer'),
 'pca:null-src': (1, 'gdf_op_pca: null pointer'),
 'pca:null-feature': (1, 'gdf_op_pca: null feature pointer'),
 'pca:B<0': (1, 'gdf_op_pca: B >= 0'),
 'pca:W<1': (1, 'gdf_op_pca: C, H and W >= 1'),
 'pca:joint': (1, 'gdf_op_pca: joint is 0 or 1'),
 'pca:k=0': (1, 'gdf_op_pca: 1 <= k <= 8'),
 'pca:k=9': (1, 'gdf_op_pca: 1 <= k <= 8'),
 'pca:max_iter': (1, 'gdf_op_pca: 1 <= max_iter <= 1024'),
 'pca:tol': (1, 'gdf_op_pca: tol is finite and not negative'),
 'pca:misaligned': (1, 'gdf_op_pca: the workspace must be 16-byte aligned'),
 'pca:k>samples-1': (1, 'gdf_op_pca: k <= min(C, samples - 1)'),
 'pca:C>4096': (4, 'gdf_op_pca: C > 4096'),
 'pca:B>65535': (4, 'gdf_op_pca: B > 65535; split the batch'),
 'pca:small-ws': (1, 'gdf_op_pca: workspace smaller than gdf_op_pca_workspace says'),
 'pca:joint-before-k': (1, 'gdf_op_pca: joint is 0 or 1'),
 'pca:B=0': (0, ''),
 'pca_rgb:null': (1, 'gdf_op_pca_rgb: null pointer'),
 'pca_rgb:OW<1': (1, 'gdf_op_pca_rgb: B >= 0, H, W, OH and OW >= 1'),
 'pca_rgb:joint': (1, 'gdf_op_pca_rgb: joint is 0 or 1'),
 'pca_rgb:B>65535': (4, 'gdf_op_pca_rgb: B > 65535, B * H * W or B * OH * OW >= 2^31; split the batch'),
 'pca_rgb:2^31': (4, 'gdf_op_pca_rgb: B > 65535, B * H * W or B * OH * OW >= 2^31; split the batch'),
 'pca_rgb:B=0': (0, ''),
 'pixcls_create:null': (1, 'gdf_pixcls_create: null pointer'),
 'pixcls_create:null-out': (1, 'gdf_pixcls_create: null pointer'),
 'pixcls_create:M<1': (1, 'gdf_pixcls_create: C, M, h1, h2 and K >= 1'),
 'pixcls_create:M>16': (4, 'gdf_pixcls_create: M <= 16, K <= 64, h1 and h2 multiples of 32 up to 256'),
 'pixcls_create:K>64': (4, 'gdf_pixcls_create: M <= 16, K <= 64, h1 and h2 multiples of 32 up to 256'),
 'pixcls_create:h1%32': (4, 'gdf_pixcls_create: M <= 16, K <= 64, h1 and h2 multiples of 32 up to 256'),
 'pixcls_create:h2>256': (4, 'gdf_pixcls_create: M <= 16, K <= 64, h1 and h2 multiples of 32 up to 256'),
 'pixcls_predict:null': (1, 'gdf_pixcls_predict: null pointer'),
 'agghead_create:null': (1, 'gdf_agghead_create: null pointer'),
 'agghead_create:null-out': (1, 'gdf_agghead_create: null pointer'),
 'agghead_create:Cin<1': (1, 'gdf_agghead_create: Cin and Cout >= 1'),
 'agghead_create:nan-weight': (1, 'gdf_agghead_create: a weight is not finite'),
 'agghead_create:inf-bias': (1, 'gdf_agghead_create: a bias is not finite'),
 'agghead_forward:null': (1, 'gdf_agghead_forward: null pointer'),
 'agghead_create_device:null': (1, 'gdf_agghead_create_device: null pointer'),
 'agghead_create_device:Cout<1': (1, 'gdf_agghead_create_device: Cin and Cout >= 1'),
 'agghead_update:null': (1, 'gdf_agghead_update: null pointer'),
 'agghead_wgrad:null': (1, 'gdf_agghead_wgrad: null pointer'),
 'agghead_wgrad:null-x': (1, 'gdf_agghead_wgrad: null pointer'),
 'agghead_wgrad:null-feature': (1, 'gdf_agghead_wgrad: null feature pointer'),
 'agghead_wgrad:B<0': (1, 'gdf_agghead_wgrad: B >= 0, Cout, C, H and W >= 1'),
 'agghead_wgrad:Cout<1': (1, 'gdf_agghead_wgrad: B >= 0, Cout, C, H and W >= 1'),
 'agghead_wgrad:2^31': (1, 'gdf_agghead_wgrad: B * H * W >= 2^31; split the batch'),
 'agghead_wgrad:misaligned': (1, 'gdf_agghead_wgrad: the workspace must be 16-byte aligned'),
 'agghead_wgrad:small-ws': (1, 'gdf_agghead_wgrad: workspace smaller than gdf_agghead_wgrad_workspace says'),
 'agghead_wgrad:2^31-before-misaligned': (1, 'gdf_agghead_wgrad: B * H * W >= 2^31; split the batch'),
 'agghead_wgrad:B=0': (0, '')}


@pytest.fixture(scope="module")
def got():
    import __graft_entry__ as G
    G.build()
    return collect(bind(G.LIB))


def test_workspace_byte_counts_are_those_of_the_parent(got):
    assert len(WORKSPACE) == len(WS_CASES) >= 60
    for (fn, args), have, want in zip(WS_CASES, got[0], WORKSPACE):
        assert have == want, (fn, args, have, want)


def test_refusals_return_the_parents_codes_and_messages(got):
    assert sorted(got[1]) == sorted(REFUSALS) and len(REFUSALS) >= 120
    for name, want in REFUSALS.items():
        assert got[1][name] == want, (name, got[1][name], want)
    codes = {rc for rc, _ in REFUSALS.values()}
    assert codes == {0, 1, 4}                                                   # GDF_OK (B = 0), GDF_ERR_ARG, GDF_ERR_UNSUPPORTED
