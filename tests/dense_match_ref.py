"""Float64 oracle and acceptance rule of dense matching (gdf_op_dense_match, components/postproc.py dense_match / mutual_nn /
dense_nn_correspondences), shared by tests/test_dense_match_cpu.py and tests/test_gpu_dense_match.py.

The op: both maps flattened to (P, C) and L2-normalised, S = A^ B^T, for every row its best column (lowest index) and the score there, and
the same for every column.  The oracle computes S in float64 from the inputs as given (an fp16 map's values are exact in float64).

Tolerance on the cosine, from the number formats alone (none of it measured).

fp16 x fp16.  The products of two fp16 values are exact in fp32 (22 significant bits).  An fp32 accumulation of C terms errs by at most
C 2^-24 sum |a_c b_c| <= C 2^-24 ||a|| ||b||.  Each norm is the square root of an fp32 sum of C exact squares, accumulated in a tree: the sum
errs by at most C 2^-24 relative, the root halves that and adds a rounding, the reciprocal another: (C / 2 + 2) 2^-24 per norm.  The epilogue
multiplies twice: 2 roundings.  With slack:
    tol = (C + 2 (C / 2 + 2) + 2 + ..) 2^-24 <= (2 C + 16) 2^-24.

An fp32 map is normalised in fp32, v = x * (1 / ||x||), scaled by a power of two (exact) and stored as fp16 hi + lo with hi = fp16(w),
lo = fp16(w - hi).  Its own terms, each relative to ||a|| ||b|| = 1:
    the norm                      (C / 2 + 2) 2^-24, as above (already counted in 2 C + 16), plus one rounding of x * (1 / ||x||) per element: 2^-24
    the residual w - hi - lo      w - hi is exact in fp32 and at most 2^-11 |w|; lo keeps 11 bits of it: 2^-22 |w| per element, i.e. 2^-22 on
                                  the dot product — unless lo is an fp16 subnormal (quantum 2^-24 in the scaled units, 2^-36 after the 2^12
                                  scale is undone): at most 2^-37 per element, 2^-37 sum_c |b_c| <= 2^-37 sqrt(C) on the dot product
    the dropped lo x lo           only where both maps are pairs: |lo| <= 2^-11 |w| on both sides, 2^-22
    the extra accumulation        every extra MFMA pass adds C terms to the fp32 sum, whose absolute values sum to at most
                                  (1 + 2^-10) ||a|| ||b||: C 2^-24 per pass (one pass per pair operand)
so, with n = the number of fp32 maps (0, 1 or 2):
    tol = (2 C + 16) 2^-24 + n (C 2^-24 + 2^-24 + 2^-22 + sqrt(C) 2^-37) + (n == 2) 2^-22.

Acceptance of a returned index j for row p:   S[p, j] + tol >= max S[p, :] - tol   and   |score - S[p, j]| <= tol + 2^-23; where several
columns carry identical vectors (`classes`), the lowest index of the class of j must be named.  The same rules hold for columns.
A row (column) is ambiguous when its two best oracle scores, taken over distinct classes, differ by <= 2 tol; every test case requires that at
most 10 % of its rows and of its columns are (a condition on the inputs: the check cannot pass vacuously)."""
import ctypes as C

import numpy as np

from aggregate_ref import AggSrc

DM_ARGTYPES = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
GDF_ERR_ARG, GDF_ERR_UNSUPPORTED = 1, 4
MAX_AMBIGUOUS = 0.10


def bind(L):
    L.gdf_op_dense_match.restype, L.gdf_op_dense_match.argtypes = C.c_int, DM_ARGTYPES
    L.gdf_op_dense_match_workspace.restype, L.gdf_op_dense_match_workspace.argtypes = C.c_size_t, [C.c_int] * 6
    L.gdf_last_error.restype = C.c_char_p
    L.gdf_abi_version.restype = C.c_int
    return L


def agg_src(ptr, f32, strides, shape):
    s = AggSrc()
    s.ptr, s.f32 = ptr, int(f32)
    s.sb, s.sc, s.sy, s.sx = strides
    _, s.C, s.H, s.W = shape
    return s


def tolerance(Cn, n_f32=0):
    t = (2 * Cn + 16) * 2.0 ** -24
    t += n_f32 * (Cn * 2.0 ** -24 + 2.0 ** -24 + 2.0 ** -22 + np.sqrt(Cn) * 2.0 ** -37)
    return t + (2.0 ** -22 if n_f32 == 2 else 0.0)


def oracle(f1, f2):
    """f1 (C, h1, w1), f2 (C, h2, w2) numpy -> S (P1, P2) float64; a pixel of zero norm gives NaN rows / columns"""
    a = f1.reshape(f1.shape[0], -1).T.astype(np.float64)
    b = f2.reshape(f2.shape[0], -1).T.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        a = a / np.linalg.norm(a, axis=1)[:, None]
        b = b / np.linalg.norm(b, axis=1)[:, None]
    return a @ b.T


def classes(f):
    """f (C, h, w) -> (P,) the lowest pixel index carrying the same vector"""
    v = np.ascontiguousarray(f.reshape(f.shape[0], -1).T)
    _, first, inv = np.unique(v, axis=0, return_index=True, return_inverse=True)
    return first[inv.reshape(-1)]


def ambiguous(S, tol, cls):
    """rows of S whose best two scores over DISTINCT column classes differ by <= 2 tol"""
    rep = np.unique(cls)
    T = np.where(np.isnan(S[:, rep]), -np.inf, S[:, rep])
    if T.shape[1] < 2:
        return np.zeros(S.shape[0], dtype=bool)
    top = np.partition(T, T.shape[1] - 2, axis=1)[:, -2:]
    with np.errstate(invalid="ignore"):                  # (-inf) - (-inf): a row nobody answers is not ambiguous
        return np.isfinite(top[:, 0]) & (top[:, 1] - top[:, 0] <= 2 * tol)


def check_direction(nn, sim, S, tol, cls, what="", lowest_in_class=True, skip=None):
    """nn (P,), sim (P,) or None against the rows of S (P, Q); cls (Q,) the duplicate classes of the columns; rows in `skip` are not judged.
    Returns the ambiguity mask after asserting the cap."""
    nn = np.asarray(nn).astype(np.int64)
    P, Q = S.shape
    assert nn.shape == (P,) and (nn >= 0).all() and (nn < Q).all(), what
    keep = np.ones(P, dtype=bool) if skip is None else ~skip
    rows = np.arange(P)
    got = S[rows, nn]
    best = np.nanmax(np.where(np.isnan(S), -np.inf, S), axis=1)
    bad = keep & ~(got + tol >= best - tol)
    amb = ambiguous(S, tol, cls)
    err = 0.0
    if sim is not None:
        d = np.abs(np.asarray(sim, dtype=np.float64) - got)
        err = float(d[keep].max()) if keep.any() else 0.0
    print("dense_match %s: %d rows, %d ambiguous, %d not accepted, %d off the oracle's argmax, worst score error %.3f of its bound %.3e"
          % (what, P, int(amb.sum()), int(bad.sum()), int((keep & (got < best)).sum()), err / (tol + 2.0 ** -23), tol + 2.0 ** -23))
    assert amb.mean() <= MAX_AMBIGUOUS, "%s: %.1f %% ambiguous rows: the inputs do not test the op" % (what, 100 * amb.mean())
    assert not bad.any(), "%s: %d rows outside the tolerance, first %d" % (what, int(bad.sum()), int(np.argmax(bad)))
    if sim is not None:
        assert err <= tol + 2.0 ** -23, "%s: score error %.3e > %.3e" % (what, err, tol + 2.0 ** -23)
    if lowest_in_class:
        off = keep & (cls[nn] != nn)
        assert not off.any(), "%s: %d rows name a later member of a duplicate class" % (what, int(off.sum()))
    return amb


def check(nn12, sim12, nn21, sim21, f1, f2, what="", lowest_in_class=True):
    """one sample: f1 (C, h1, w1), f2 (C, h2, w2) numpy in their own dtype; both directions against the oracle"""
    n32 = int(f1.dtype == np.float32) + int(f2.dtype == np.float32)
    tol = tolerance(f1.shape[0], n32)
    S = oracle(f1, f2)
    amb12 = check_direction(nn12, sim12, S, tol, classes(f2), what + " rows", lowest_in_class) if nn12 is not None else None
    amb21 = check_direction(nn21, sim21, S.T, tol, classes(f1), what + " columns", lowest_in_class) if nn21 is not None else None
    return amb12, amb21
