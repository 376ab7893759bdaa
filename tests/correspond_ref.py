"""Float64 oracle and acceptance rule of the nearest-neighbour correspondence (gdf_op_nn_match, components/postproc.py nn_match /
find_nn_source_correspondences), shared by tests/test_correspond_cpu.py and tests/test_gpu_correspond.py.

The op: both maps upsampled to (LH, LW) as ATen's upsample_bilinear2d (align_corners = False) does, the source pixels gathered from the first,
s[n, p] = <q_n / ||q_n||, v_p> / ||v_p||, argmax over p (lowest index), the score there.  Coordinates come from coords() of aggregate_ref.py
(numpy float32, separately rounded, as ATen defines them); the blend, the norms and the score matrix S are float64.

Per-pixel tolerance, from the number formats alone.  With the four taps T_i of pixel p, a_i = ||T_i|| and weights w_i,
  rho_p = (sum_i w_i a_i) / ||v_p||  >= 1       the cancellation factor of the blend
  eps   = (C + 16) * 2^-24                      a C-term fp32 dot product plus the few roundings of blend and normalisation
  tol_p = eps * (2 rho_p + rho_p^2)
2 rho covers the numerator sum_i w_i <q, T_i> (each term bounded by eps w_i a_i, relative to ||v_p|| that is eps rho) and the query's own
normalisation; rho^2 covers the Gram-form norm ||v||^2 = sum_ij w_i w_j <T_i, T_j>, whose terms are bounded by eps w_i w_j a_i a_j, i.e.
eps rho^2 relative to ||v||^2, with slack for the square root.  None of this is a measured figure.

Acceptance of a returned pixel p* for query n:   S[n, p*] + tol[p*] >= max_p (S[n, p] - tol[p])   and   |score - S[n, p*]| <= tol[p*] + 2^-23.

Duplicate classes: fine rows with the same (i0, i1, lambda) — where i0 == i1, any lambda — carry the same source row; columns likewise; pixels of
one (row class, column class) pair carry the same vector, and the device computes the same bits for them, so it must return the lowest index of
the class of its answer.  A query is ambiguous when pixels of more than one class are acceptable; every test case requires that at most 10 % of
its queries are (a condition on the inputs: the check cannot pass vacuously)."""
import ctypes as C

import numpy as np

from aggregate_ref import AggSrc, coords

NN_ARGTYPES = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
GDF_ERR_ARG = 1


def bind(L):
    L.gdf_op_nn_match.restype, L.gdf_op_nn_match.argtypes = C.c_int, NN_ARGTYPES
    L.gdf_op_nn_match_workspace.restype, L.gdf_op_nn_match_workspace.argtypes = C.c_size_t, [C.c_int] * 5
    L.gdf_last_error.restype = C.c_char_p
    L.gdf_abi_version.restype = C.c_int
    return L


def agg_src(ptr, f32, strides, shape):
    s = AggSrc()
    s.ptr, s.f32 = ptr, int(f32)
    s.sb, s.sc, s.sy, s.sx = strides
    _, s.C, s.H, s.W = shape
    return s


def source_index(points, LH, LW):
    """points (N, 2) (y, x) -> integer (y, x): round_half_even(clip(.)), the reference's points_to_idxs"""
    p = np.asarray(points, dtype=np.float64)
    return np.stack([np.round(np.clip(p[:, 0], 0, LH - 1)), np.round(np.clip(p[:, 1], 0, LW - 1))], -1).astype(np.int64)


def _upsample(v, LH, LW):
    """v (C, h, w) float64 -> (C, LH, LW) float64 and the per-pixel sum_i w_i ||T_i||"""
    _, y0, y1, ly0, ly1 = coords(LH, v.shape[1])
    _, x0, x1, lx0, lx1 = coords(LW, v.shape[2])

    def blend(t):
        top, bot = t[..., y0, :], t[..., y1, :]
        return ly0[:, None] * (lx0 * top[..., x0] + lx1 * top[..., x1]) + ly1[:, None] * (lx0 * bot[..., x0] + lx1 * bot[..., x1])
    return blend(v), blend(np.sqrt((v * v).sum(0)))


def _axis_classes(out, inn, twins=False):
    _, i0, i1, _, l1 = coords(out, inn)
    keys = [(int(a), int(b), 0.0 if a == b and not twins else float(l)) for a, b, l in zip(i0, i1, l1)]
    ids = {}
    return np.array([ids.setdefault(k, len(ids)) for k in keys])


def classes(LH, LW, h, w, twins=False):
    """-> (LH * LW,) class id of every fine pixel.  twins: the narrower classes of identical taps AND weights (lambda counts where i0 == i1 too),
    whose members any implementation of the chain computes with the same bits"""
    r, c = _axis_classes(LH, h, twins), _axis_classes(LW, w, twins)
    return (r[:, None] * (int(c.max()) + 1) + c[None, :]).reshape(-1)


def same_answer(got_yx, want_yx, cls, twin, LW, rows):
    """Two implementations on the queries `rows` (a mask; the non-ambiguous ones): the same class everywhere, and the same pixel wherever the
    class of the answer is one twin class (then both compute equal bits for all its members and argmax names the lowest).  In a class whose members
    differ in lambda (the clamped last rows / columns) an fp32 chain that blends l0 T + l1 T rounds member by member, and which member it names is
    its rounding noise: there only the class can be compared."""
    p, w = np.asarray(got_yx)[:, 0] * LW + np.asarray(got_yx)[:, 1], np.asarray(want_yx)[:, 0] * LW + np.asarray(want_yx)[:, 1]
    assert np.array_equal(cls[p][rows], cls[w][rows]), np.nonzero((cls[p] != cls[w]) & rows)[0][:8]
    one_twin = np.array([len(np.unique(twin[cls == cls[k]])) == 1 for k in w])
    assert np.array_equal(p[rows & one_twin], w[rows & one_twin]), np.nonzero((p != w) & rows & one_twin)[0][:8]
    return int((rows & one_twin).sum())


def oracle(f1, f2, points, LH, LW):
    """f1 (C, h1, w1), f2 (C, h2, w2) arrays (one sample), points (N, 2) -> S (N, LH LW) float64, tol (LH LW,), class ids (LH LW,)"""
    f1, f2 = np.asarray(f1, dtype=np.float64), np.asarray(f2, dtype=np.float64)
    Cn = f1.shape[0]
    idx = source_index(points, LH, LW)
    u1, _ = _upsample(f1, LH, LW)
    q = u1[:, idx[:, 0], idx[:, 1]].T                                       # (N, C)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    v, wa = _upsample(f2, LH, LW)
    nrm = np.sqrt((v * v).sum(0))
    S = (q @ v.reshape(Cn, -1)) / nrm.reshape(-1)
    rho = (wa / nrm).reshape(-1)
    eps = (Cn + 16) * 2.0 ** -24
    return S, eps * (2 * rho + rho * rho), classes(LH, LW, f2.shape[1], f2.shape[2])


def accepted(S, tol):
    """-> bool (N, LH LW): the pixels a correct implementation may return"""
    return S + tol[None] >= (S - tol[None]).max(1, keepdims=True)


def ambiguous(S, tol, cls):
    """-> bool (N,): pixels of more than one class are acceptable"""
    acc = accepted(S, tol)
    return np.array([len(np.unique(cls[a])) > 1 for a in acc])


def check(yx, score, f1, f2, points, LH, LW, lowest_in_class=True, what=""):
    """assert the acceptance rule (and, for the device, the duplicate-class rule) for one sample: yx (N, 2) integers, score (N,) or None;
    asserts the 10 % ambiguity condition; returns the ambiguity mask.  Prints the figures first."""
    S, tol, cls = oracle(f1, f2, points, LH, LW)
    yx = np.asarray(yx)
    N = S.shape[0]
    assert yx.shape == (N, 2) and (yx >= 0).all() and (yx[:, 0] < LH).all() and (yx[:, 1] < LW).all(), (what, yx.shape)
    p = yx[:, 0] * LW + yx[:, 1]
    acc = accepted(S, tol)
    amb = ambiguous(S, tol, cls)
    rows = np.arange(N)
    gap = (S - tol[None]).max(1) - (S[rows, p] + tol[p])                    # <= 0 when accepted
    serr = np.abs(np.asarray(score, dtype=np.float64) - S[rows, p]) / (tol[p] + 2.0 ** -23) if score is not None else np.zeros(N)
    print("nn_match %s: %d queries, %d ambiguous, %d not accepted (worst gap %.3e), %d off the oracle's argmax, worst score error %.3f of its bound"
          % (what, N, int(amb.sum()), int((~acc[rows, p]).sum()), float(gap.max()), int((p != S.argmax(1)).sum()), float(serr.max())))
    assert acc[rows, p].all(), (what, "not accepted", np.nonzero(~acc[rows, p])[0][:8])
    assert np.isfinite(serr).all() and (serr <= 1.0).all(), (what, "score", float(serr.max()))
    if lowest_in_class:
        first = np.array([np.nonzero(cls == cls[k])[0][0] for k in p])
        assert (p == first).all(), (what, "not the lowest index of its class", np.nonzero(p != first)[0][:8])
    assert amb.sum() <= 0.1 * N, (what, "more than 10 % of the queries are ambiguous", int(amb.sum()), N)
    return amb
