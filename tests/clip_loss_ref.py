"""Float64 oracle, reference arithmetic, fp32 emulation, seeded generators, bounds and ctypes binding of the correspondence loss
(gdf_op_clip_loss / gdf_op_clip_loss_backward, components/postproc.py clip_loss / compute_clip_loss), shared by tests/test_clip_loss_cpu.py and
tests/test_gpu_clip_loss.py.

The op (reference correspondence/task-corres.py:70-80): both maps L2-normalised per pixel; direction 1 takes the rows src of map 1 against every pixel
of map 2, logits = scale * cosine, cross-entropy against tgt; direction 2 the same with the roles swapped; loss = (mean term1 + mean term2) / 2.

Oracle: that chain in float64 with torch's autograd, from the inputs as given (an fp16 map is exact in float64); per pair the loss, the 2 N terms and
the gradients of both maps for an upstream gradient g (default 1 per pair).
Reference arithmetic: the same chain in fp32 on the CPU with autograd, BOTH full P x P similarity matrices built as the reference builds them.

Bounds: no new constant.  MARGIN (= 8) and the 16-pixel block of block_rel are the project's, from tests/pixel_classifier_ref.py.
  gradients   relative L2 error per block of 16 consecutive pixels over all C against the oracle; a result passes when its worst block is within
              MARGIN x the worst block of the reference arithmetic on the same inputs.
  terms       worst absolute error over the 2 N terms within MARGIN x the reference arithmetic's worst term error, but the bound is never below
              8 * 2^-24 * (scale + ln P): a few fp32 roundings of the quantities that enter the final subtraction lse - z[label], both of which
              scale + ln P bounds in magnitude (derived, not measured; the reference's own error can be far smaller by chance).
  loss        the same rule on the scalar.
emulate() restates the device kernels' arithmetic in numpy fp32 — dot products of the raw key pixel with the normalised query in 16 channel
slices folded in the kernel's tree, times the inverse norm; the exact maximum, then exp sums per strided thread and a tree; G rebuilt from cos and
the log-sum-exp; partial sums per pixel range — so that the bounds can be checked against the kernel's summation order without a GPU."""
import ctypes as C
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from aggregate_ref import AggSrc
from pixel_classifier_ref import MARGIN, block_rel, gen_features

GDF_ERR_ARG, GDF_ERR_UNSUPPORTED = 1, 4
SCALE = 1 / 0.07
vp, ci = C.c_void_p, C.c_int
FWD_ARGTYPES = [vp, vp, ci, vp, vp, ci, C.c_float, vp, vp, vp, C.c_size_t, vp]
BWD_ARGTYPES = [vp, vp, ci, vp, vp, ci, C.c_float, vp, vp, vp, vp, C.c_size_t, vp]


def bind(L):
    L.gdf_op_clip_loss_workspace.restype, L.gdf_op_clip_loss_workspace.argtypes = C.c_size_t, [ci] * 5
    L.gdf_op_clip_loss.restype, L.gdf_op_clip_loss.argtypes = ci, FWD_ARGTYPES
    L.gdf_op_clip_loss_backward.restype, L.gdf_op_clip_loss_backward.argtypes = ci, BWD_ARGTYPES
    L.gdf_last_error.restype = C.c_char_p
    L.gdf_abi_version.restype = ci
    return L


def agg_src(ptr, f32, strides, shape):
    s = AggSrc()
    s.ptr, s.f32 = ptr, int(f32)
    s.sb, s.sc, s.sy, s.sx = strides
    _, s.C, s.H, s.W = shape
    return s


# ------------------------------------------------------------------------------------------------------------------------------
# generators
# ------------------------------------------------------------------------------------------------------------------------------
def smooth(v):
    """the 3 x 3 box filter with edge replication of tests/test_gpu_correspond.py: neighbouring pixels correlate, as real features do"""
    p = F.pad(v.float(), (1, 1, 1, 1), mode="replicate")
    return F.avg_pool2d(p, 3, stride=1).to(v.dtype)


def features(B, C_, h, w, f32=False, seed=0, smoothed=False):
    v = gen_features(B, C_, h, w, True, seed)
    v = smooth(v) if smoothed else v
    return v if f32 else v.half()


def indices(B, N, P, seed, distinct=False):
    g = torch.Generator().manual_seed(seed + 991)
    if distinct:
        return torch.stack([torch.randperm(P, generator=g)[:N] for _ in range(B)])
    return torch.randint(0, P, (B, N), generator=g)


# ------------------------------------------------------------------------------------------------------------------------------
# oracle and reference arithmetic
# ------------------------------------------------------------------------------------------------------------------------------
def _pair(a, b, src, tgt, scale, full):
    """one pair: maps a (C, h1, w1), b (C, h2, w2) of one dtype, indices (N,) -> (loss, terms (2, N)), differentiable"""
    k1 = a.reshape(1, a.shape[0], -1).permute(0, 2, 1)
    k2 = b.reshape(1, b.shape[0], -1).permute(0, 2, 1)
    k1 = k1 / torch.linalg.norm(k1, dim=-1)[:, :, None]
    k2 = k2 / torch.linalg.norm(k2, dim=-1)[:, :, None]
    if full:                                                             # both P x P matrices, then the rows: what the reference does
        l1 = (scale * torch.matmul(k1, k2.permute(0, 2, 1)))[0, src]
        l2 = (scale * torch.matmul(k2, k1.permute(0, 2, 1)))[0, tgt]
    else:
        l1 = scale * (k1[0, src] @ k2[0].T)
        l2 = scale * (k2[0, tgt] @ k1[0].T)
    terms = torch.stack([F.cross_entropy(l1, tgt, reduction="none"), F.cross_entropy(l2, src, reduction="none")])
    return (F.cross_entropy(l1, tgt) + F.cross_entropy(l2, src)) / 2, terms


def _chain_loss(a, b, src, tgt, scale, full):
    """the summed loss of a batch, differentiable with respect to a and b (whatever produced them)"""
    return sum(_pair(a[i], b[i], src[i], tgt[i], scale, full)[0] for i in range(src.shape[0]))


def _chain(f1, f2, src, tgt, scale, g, dtype, full):
    B = src.shape[0]
    a = f1.detach().to(dtype).clone().requires_grad_(True)
    b = f2.detach().to(dtype).clone().requires_grad_(True)
    g = torch.ones(B, dtype=dtype) if g is None else g.to(dtype)
    res = [_pair(a[i], b[i], src[i], tgt[i], scale, full) for i in range(B)]
    loss = torch.stack([r[0] for r in res])
    (loss * g).sum().backward()
    return loss.detach(), torch.stack([r[1] for r in res]).detach(), a.grad, b.grad


def oracle(f1, f2, src, tgt, scale=SCALE, g=None):
    """-> loss (B,), terms (B, 2, N), grad_f1, grad_f2, all float64"""
    return _chain(f1, f2, src, tgt, scale, g, torch.float64, False)


def reference(f1, f2, src, tgt, scale=SCALE, g=None):
    """the reference's arithmetic: fp32 on the CPU, both similarity matrices, autograd"""
    return _chain(f1, f2, src, tgt, scale, g, torch.float32, True)


# ------------------------------------------------------------------------------------------------------------------------------
# fp32 emulation of the kernels' summation order (numpy)
# ------------------------------------------------------------------------------------------------------------------------------
f32 = np.float32


def _tree(parts):
    """fold a list of arrays as the kernels' LDS trees do: the upper half onto the lower half, repeatedly (length a power of two)"""
    parts = list(parts)
    while len(parts) > 1:
        h = len(parts) // 2
        parts = [parts[i] + parts[i + h] for i in range(h)]
    return parts[0]


def _direction(q_map, k_map, qi, lab, scale, coef):
    """one direction of one pair.  q_map (C, Pq), k_map (C, Pk) fp32 -> terms (N,), dense gradient of the key map (C, Pk), rows (N, C)"""
    Cn, Pk = k_map.shape
    N = len(qi)
    per = (Cn + 15) // 16
    qraw = q_map[:, qi]                                                  # (C, N)
    qinv = np.array([f32(1) / np.sqrt(_tree([np.add.reduce((qraw[t::256, n] * qraw[t::256, n]).astype(f32), dtype=f32) for t in range(256)]))
                     for n in range(N)], dtype=f32)
    qh = (qraw * qinv[None]).astype(f32)                                 # (C, N)
    slices = []
    nsl = []
    for s in range(16):
        blk = k_map[s * per:min(Cn, (s + 1) * per)]
        slices.append((blk.T @ qh[s * per:min(Cn, (s + 1) * per)]).astype(f32) if len(blk) else np.zeros((Pk, N), f32))
        nsl.append((blk * blk).sum(0, dtype=f32) if len(blk) else np.zeros(Pk, f32))
    dots, nsq = _tree(slices), _tree(nsl)
    kinv = (f32(1) / np.sqrt(nsq)).astype(f32)
    cos = (dots * kinv[:, None]).astype(f32)                             # (Pk, N)
    z = (f32(scale) * cos).astype(f32)
    m = z.max(0)
    e = np.exp((z - m[None]).astype(f32)).astype(f32)
    se = np.array([_tree([np.add.reduce(e[t::256, n], dtype=f32) for t in range(256)]) for n in range(N)], dtype=f32)
    lse = (m + np.log(se).astype(f32)).astype(f32)
    terms = (lse - z[lab, np.arange(N)]).astype(f32)
    G = np.exp((z - lse[None]).astype(f32)).astype(f32)
    G[lab, np.arange(N)] -= f32(1)
    G = (f32(coef) * G).astype(f32)                                      # (Pk, N)
    S = (G * cos).sum(1, dtype=f32)
    kh = (k_map * kinv[None]).astype(f32)                                # (C, Pk)
    dense = (((qh @ G.T).astype(f32) - kh * S[None]) * kinv[None]).astype(f32)
    PR = max(64, (((Pk + 15) // 16 + 63) // 64) * 64)                       # the pixel range of one backward workgroup
    part = np.zeros((N, Cn), f32)
    for r0 in range(0, Pk, PR):
        part = (part + (G[r0:r0 + PR].T @ kh[:, r0:r0 + PR].T).astype(f32)).astype(f32)
    T = np.array([_tree([np.add.reduce((G[t::256, n] * cos[t::256, n]).astype(f32), dtype=f32) for t in range(256)]) for n in range(N)], dtype=f32)
    rows = ((part - qh.T * T[:, None]) * qinv[:, None]).astype(f32)
    return terms, dense, rows


def emulate(f1, f2, src, tgt, scale=SCALE, g=None):
    """-> loss (B,), terms (B, 2, N), grad_f1, grad_f2 as fp32 torch tensors, in the kernels' arithmetic"""
    B, N = src.shape
    a, b = f1.float().numpy(), f2.float().numpy()
    loss, terms = np.zeros(B, f32), np.zeros((B, 2, N), f32)
    g1, g2 = np.zeros(a.shape, f32), np.zeros(b.shape, f32)
    for i in range(B):
        coef = f32(f32(1.0 if g is None else float(g[i])) * f32(scale)) / f32(2 * N)
        m1, m2 = a[i].reshape(a.shape[1], -1), b[i].reshape(b.shape[1], -1)
        s, t = src[i].numpy(), tgt[i].numpy()
        t1, d2, r1 = _direction(m1, m2, s, t, scale, coef)
        t2, d1, r2 = _direction(m2, m1, t, s, scale, coef)
        for n in range(N):
            d1[:, s[n]] += r1[n]
            d2[:, t[n]] += r2[n]
        terms[i, 0], terms[i, 1] = t1, t2
        s0, s1 = f32(0), f32(0)
        for n in range(N):
            s0, s1 = f32(s0 + t1[n]), f32(s1 + t2[n])
        loss[i] = (s0 / f32(N) + s1 / f32(N)) * f32(0.5)
        g1[i], g2[i] = d1.reshape(a.shape[1:]), d2.reshape(b.shape[1:])
    return torch.from_numpy(loss), torch.from_numpy(terms), torch.from_numpy(g1), torch.from_numpy(g2)


# ------------------------------------------------------------------------------------------------------------------------------
# bounds
# ------------------------------------------------------------------------------------------------------------------------------
def _blocks(t):
    """(B, C, H, W) -> (B, P, C) for block_rel"""
    return t.reshape(t.shape[0], t.shape[1], -1).permute(0, 2, 1)


class Bounds:
    """oracle, reference arithmetic and the bounds of one set of inputs"""

    def __init__(self, f1, f2, src, tgt, scale=SCALE, g=None):
        self.args = (f1, f2, src, tgt, scale, g)
        self.loss, self.terms, self.g1, self.g2 = oracle(f1, f2, src, tgt, scale, g)
        rl, rt, r1, r2 = reference(f1, f2, src, tgt, scale, g)
        P = max(f1.shape[2] * f1.shape[3], f2.shape[2] * f2.shape[3])
        floor = 8 * 2.0 ** -24 * (scale + math.log(P))
        self.ref_terms = float((rt.double() - self.terms).abs().max())
        self.ref_loss = float((rl.double() - self.loss).abs().max())
        self.ref_g1 = float(block_rel(_blocks(r1), _blocks(self.g1)).max())
        self.ref_g2 = float(block_rel(_blocks(r2), _blocks(self.g2)).max())
        self.b_terms, self.b_loss = max(MARGIN * self.ref_terms, floor), max(MARGIN * self.ref_loss, floor)
        self.b_g1, self.b_g2 = MARGIN * self.ref_g1, MARGIN * self.ref_g2

    def check(self, loss, terms, g1, g2, what=""):
        """any of the four may be None.  Prints error, bound and reference error, then asserts."""
        rows = []
        if loss is not None:
            rows.append(("loss", float((loss.double() - self.loss).abs().max()), self.b_loss, self.ref_loss))
        if terms is not None:
            rows.append(("terms", float((terms.double() - self.terms).abs().max()), self.b_terms, self.ref_terms))
        if g1 is not None:
            rows.append(("grad_f1", float(block_rel(_blocks(g1), _blocks(self.g1)).max()), self.b_g1, self.ref_g1))
        if g2 is not None:
            rows.append(("grad_f2", float(block_rel(_blocks(g2), _blocks(self.g2)).max()), self.b_g2, self.ref_g2))
        for name, err, bound, ref in rows:
            print("clip loss %s: %s error %.3e, bound %.3e (reference fp32: %.3e)" % (what, name, err, bound, ref))
        for name, err, bound, ref in rows:
            assert math.isfinite(err) and err <= bound, (what, name, err, bound, ref)


# ------------------------------------------------------------------------------------------------------------------------------
# the cases of one forward + backward against the oracle (tests/test_gpu_clip_loss.py; tests/test_clip_loss_cpu.py runs emulate() on them)
# ------------------------------------------------------------------------------------------------------------------------------
# C, (h1, w1), fp32 map 1, channels-last 1, (h2, w2), fp32 map 2, channels-last 2, N, B, smoothed, kind of indices
CASES = {
    "C 40 on 6 x 6": (40, (6, 6), 0, 0, (6, 6), 0, 0, 20, 1, 0, "random"),                     # less than one pixel block
    "C 72 channels-last B 2 N 64": (72, (5, 7), 0, 1, (5, 7), 0, 1, 64, 2, 0, "random"),        # C no multiple of 64, chunks 24 + 24 + 16
    "smoothed C 16 on 9 x 9 N 70": (16, (9, 9), 0, 0, (9, 9), 0, 0, 70, 1, 1, "random"),        # 81 pixels: a partial block; 70 = 24 + 24 + 22
    "two grids two types": (24, (9, 9), 1, 0, (12, 12), 0, 1, 20, 2, 0, "random"),
    "fp32 channels-last": (20, (7, 5), 1, 1, (7, 5), 1, 1, 12, 2, 0, "random"),
    "one row": (40, (1, 9), 0, 0, (1, 9), 0, 0, 8, 2, 0, "random"),
    "one column": (40, (9, 1), 0, 1, (9, 1), 0, 1, 8, 2, 0, "random"),
    "N 1": (8, (16, 16), 1, 0, (16, 16), 1, 0, 1, 1, 0, "random"),                              # four pixel blocks, the 4-query instantiation
    "C 3520 on 8 x 8": (3520, (8, 8), 0, 0, (8, 8), 0, 0, 20, 1, 0, "random"),                  # the reference's depth
    "duplicate indices": (40, (6, 6), 0, 0, (6, 6), 0, 0, 20, 1, 0, "duplicates"),             # src[n] repeated under different labels, tgt too
}


def _cl(t):
    return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (f1, f2, src, tgt, Bounds) of a case; computed once and shared"""
    C_, g1, a32, acl, g2, b32, bcl, N, B, sm, kind = CASES[name]
    seed = sum(map(ord, name))
    f1 = features(B, C_, *g1, f32=bool(a32), seed=seed, smoothed=bool(sm))
    f2 = features(B, C_, *g2, f32=bool(b32), seed=seed + 1, smoothed=bool(sm))
    f1, f2 = (_cl(f1) if acl else f1.contiguous()), (_cl(f2) if bcl else f2.contiguous())
    P1, P2 = g1[0] * g1[1], g2[0] * g2[1]
    src, tgt = indices(B, N, P1, seed), indices(B, N, P2, seed + 1)
    if kind == "duplicates":
        src[:, 1], src[:, 2], src[:, 7] = src[:, 0], src[:, 0], src[:, 5]                       # one source pixel under three labels
        tgt[:, 9], tgt[:, 5] = tgt[:, 8], tgt[:, 7]                                             # and labels that repeat
        assert len(set(tgt[0, :3].tolist())) == 3
    return f1, f2, src, tgt, Bounds(f1, f2, src, tgt)
