"""Dense matching on the GPU (-m gpu): the kernels of csrc/densematch.hip through gdf_op_dense_match (include/gdf_ops.h), components/postproc.py
dense_match / mutual_nn / dense_nn_correspondences / find_best_buddies_correspondences and FeatureExtractor.match.

Kernel level: ONE gdf_op_dense_match call against the float64 oracle of tests/dense_match_ref.py — the acceptance rule with its tolerance derived
from the number formats, the duplicate-class rule and the <= 10 % ambiguity condition (checked for these inputs on the CPU as well, in
tests/test_dense_match_cpu.py); no measured figure.  Outputs and the workspace are guard-filled as in tests/test_gpu_glue.py: the (B, P) elements
written, everything behind them and behind the reported workspace size untouched."""
import ctypes
import os

import numpy as np
import pytest
import torch

import dense_match_ref as R
from ops_binding import P, lib, ok, stream, vp
from test_dense_match_cpu import planted
from test_gpu_glue import _cl, gen, guard, is_guard

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAT32I, PAT8, TAIL = 0x7FDA7FDA, 0xA5, 4096


def _lib():
    return R.bind(lib())


def feats(B, C_, h, w, f32=False, chlast=False, seed=0):
    v = torch.randn(B, C_, h, w, generator=gen(seed))
    v = v if f32 else v.half()
    return _cl(v) if chlast else v.contiguous()


def launch(L, d1, d2, st=None, rows=True, cols=True):
    """d1, d2: device tensors -> (nn12 (B, P1) int32, sim12, nn21 (B, P2), sim21) on the CPU after the guard checks; a direction not asked for is
    passed as null pointers and returned as None"""
    B, C_ = d1.shape[:2]
    P1, P2 = d1.shape[2] * d1.shape[3], d2.shape[2] * d2.shape[3]
    nn12, nn21 = (torch.full((B * n + 64,), PAT32I, dtype=torch.int32, device="cuda") for n in (P1, P2))
    sim12, sim21 = guard((B * P1 + 64,), torch.float32), guard((B * P2 + 64,), torch.float32)
    nbytes = L.gdf_op_dense_match_workspace(B, C_, P1, P2, int(d1.dtype == torch.float32), int(d2.dtype == torch.float32))
    ws = torch.full((nbytes + TAIL,), PAT8, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 16 == 0
    s1 = R.agg_src(d1.data_ptr(), d1.dtype == torch.float32, d1.stride(), d1.shape)
    s2 = R.agg_src(d2.data_ptr(), d2.dtype == torch.float32, d2.stride(), d2.shape)
    ok(L.gdf_op_dense_match(ctypes.addressof(s1), ctypes.addressof(s2), B, P(nn12) if rows else None, P(sim12) if rows else None,
                            P(nn21) if cols else None, P(sim21) if cols else None, P(ws), nbytes, st if st is not None else stream()), L)
    torch.cuda.synchronize()
    nn12, sim12, nn21, sim21, ws = nn12.cpu(), sim12.cpu(), nn21.cpu(), sim21.cpu(), ws.cpu()
    assert bool((ws[nbytes:] == PAT8).all()), "written behind the reported workspace size"
    out = []
    for nn, sim, n, asked in ((nn12, sim12, P1, rows), (nn21, sim21, P2, cols)):
        assert bool((nn[B * n:] == PAT32I).all()) and bool(is_guard(sim[B * n:]).all()), "written behind the outputs"
        if asked:
            assert not bool((nn[:B * n] == PAT32I).any()) and not bool(is_guard(sim[:B * n]).any()), "owned outputs not written"
            out += [nn[:B * n].view(B, n), sim[:B * n].view(B, n)]
        else:
            assert bool((nn == PAT32I).all()) and bool(is_guard(sim).all()), "a direction not asked for was written"
            out += [None, None]
    return tuple(out)


def run(f1, f2, what="", st=None):
    """host tensors (their strides are kept on the device) -> one call, every sample checked against the oracle"""
    d1, d2 = f1.cuda(), f2.cuda()
    assert d1.stride() == f1.stride() and d2.stride() == f2.stride()
    got = launch(_lib(), d1, d2, st)
    for b in range(f1.shape[0]):
        R.check(got[0][b].numpy(), got[1][b].numpy(), got[2][b].numpy(), got[3][b].numpy(), f1[b].numpy(), f2[b].numpy(), "%s, sample %d" % (what, b))
    return got


def same_bits(a, b):
    return all(torch.equal(x, y) if x.dtype == torch.int32 else torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


# C, (h1, w1), fp32 1, channels-last 1, (h2, w2), fp32 2, channels-last 2, B
CASES = {
    "fp16 NCHW several tiles": (200, (40, 36), 0, 0, (33, 31), 0, 0, 1),          # 1440 x 1023: 6 x 4 tiles of 256, a partial tile on both axes, 4 K steps
    "fp16 channels-last": (72, (40, 36), 0, 1, (33, 31), 0, 1, 1),                # C no multiple of 64: two K steps, the second zero-padded
    "fp32 odd C": (37, (17, 19), 1, 0, (24, 20), 1, 0, 1),                        # 323 x 480: every product of two (hi, lo) pairs, two K steps of 32
    "fp16 against fp32": (40, (9, 15), 0, 0, (12, 11), 1, 1, 2),                  # a pair on the column side only
    "fp32 against fp16": (40, (12, 11), 1, 1, (9, 15), 0, 0, 2),                  # a pair on the row side only
    "one small tile": (24, (5, 7), 0, 0, (3, 4), 0, 0, 2),                        # 35 x 12 inside one tile
    "one pixel against many": (24, (1, 1), 0, 0, (13, 11), 0, 0, 2),
    "many against one pixel": (24, (13, 11), 1, 0, (1, 1), 0, 1, 2),
}


@pytest.mark.parametrize("name", list(CASES))
def test_one_call_against_the_oracle(name):
    C_, g1, a32, acl, g2, b32, bcl, B = CASES[name]
    if B == 1:                                                                    # the inputs whose ambiguity share the CPU suite asserts
        from test_dense_match_cpu import _white
        a, b = _white(C_, g1, g2, bool(a32), 7)
        f1, f2 = torch.from_numpy(a)[None], torch.from_numpy(b)[None]
        f1, f2 = (_cl(f1) if acl else f1), (_cl(f2) if bcl else f2)
    else:
        seed = sum(map(ord, name))
        f1, f2 = feats(B, C_, *g1, f32=bool(a32), chlast=bool(acl), seed=seed), feats(B, C_, *g2, f32=bool(b32), chlast=bool(bcl), seed=seed + 1)
    run(f1, f2, name)


def test_planted_permutation_is_found_exactly_at_both_batch_positions():
    """C = 3520, 512 pixels a side, b = a[perm] + 0.5 noise: best score >= 0.88 against <= 0.084, so every row recovers the permutation and every
    pixel is mutual.  B = 2 with the samples swapped: a sample's bits do not depend on its batch position."""
    from components.postproc import mutual_nn
    a, b, perm = planted()
    fa, fb = torch.from_numpy(a)[None], torch.from_numpy(b)[None]
    f1, f2 = torch.cat([fa, fb]), torch.cat([fb, fa])                             # sample 0: a against b; sample 1: b against a
    nn12, sim12, nn21, sim21 = run(f1, f2, "planted")
    inv = np.argsort(perm)
    assert np.array_equal(nn12[0].numpy(), inv) and np.array_equal(nn21[0].numpy(), perm)
    assert float(sim12.min()) >= 0.88 - R.tolerance(3520) and float(sim21.min()) >= 0.88 - R.tolerance(3520)
    assert torch.equal(nn12[0], nn21[1]) and torch.equal(nn21[0], nn12[1])        # the transposed problem names the same pairs
    d1, d2 = f1.cuda(), f2.cuda()
    swapped = launch(_lib(), torch.cat([d1[1:], d1[:1]]), torch.cat([d2[1:], d2[:1]]))
    assert same_bits([t[[1, 0]] for t in swapped], (nn12, sim12, nn21, sim21))
    mask, m12, _ = mutual_nn(d1, d2)
    assert bool(mask.all()) and torch.equal(m12.cpu().int(), nn12)


def test_duplicated_pixels_name_the_lowest_index_in_both_directions():
    B, C_ = 2, 48
    f1, f2 = feats(B, C_, 12, 13, seed=71), feats(B, C_, 15, 18, seed=72)
    p1, p2 = f1.flatten(2), f2.flatten(2)
    p2[:, :, 140] = p2[:, :, 3]                                                   # two waves of one tile (128 columns each)
    p2[:, :, 260] = p2[:, :, 17]                                                  # across the 256-pixel tile boundary; three of a kind
    p2[:, :, 77] = p2[:, :, 17]
    p1[:, :, 150] = p1[:, :, 9]                                                   # across the 128-row boundary between two waves
    p1[:, :, 64] = p1[:, :, 31]                                                   # two 32-row MFMA blocks of one wave
    # every pixel of f1 that prefers a duplicated pixel of f2 must name the first of its class, and the reverse: check() asserts it; make sure
    # the duplicated classes are in fact chosen by someone
    p1[:, :, 5] = p2[:, :, 140] * 1.5
    p1[:, :, 6] = p2[:, :, 260] * 0.5
    p2[:, :, 8] = p1[:, :, 150] * 2
    p2[:, :, 9] = p1[:, :, 64]
    nn12, _, nn21, _ = run(f1, f2, "duplicates")
    assert nn12[:, 5].tolist() == [3, 3] and nn12[:, 6].tolist() == [17, 17] and nn21[:, 8].tolist() == [9, 9] and nn21[:, 9].tolist() == [31, 31]


def test_zero_pixels_never_win_and_return_nan():
    B, C_ = 2, 40
    for f32 in (False, True):
        f1, f2 = feats(B, C_, 14, 11, f32=f32, seed=81), feats(B, C_, 10, 13, f32=f32, seed=82)
        z1, z2 = 70, 129                                                         # the second MFMA block of a wave; the second wave
        f1.flatten(2)[:, :, z1] = 0
        f2.flatten(2)[:, :, z2] = 0
        ref = launch(_lib(), *(feats(B, C_, 14, 11, f32=f32, seed=81).cuda(), feats(B, C_, 10, 13, f32=f32, seed=82).cuda()))
        nn12, sim12, nn21, sim21 = launch(_lib(), f1.cuda(), f2.cuda())
        tol = R.tolerance(C_, 2 * int(f32))
        for b in range(B):
            S = R.oracle(f1[b].numpy(), f2[b].numpy())
            skip1, skip2 = np.arange(154) == z1, np.arange(130) == z2
            R.check_direction(nn12[b].numpy(), sim12[b].numpy(), S, tol, R.classes(f2[b].numpy()), "zero pixel rows", skip=skip1)
            R.check_direction(nn21[b].numpy(), sim21[b].numpy(), S.T, tol, R.classes(f1[b].numpy()), "zero pixel columns", skip=skip2)
        assert not bool((nn12 == z2).any()) and not bool((nn21 == z1).any())      # never wins
        assert nn12[:, z1].tolist() == [0, 0] and bool(torch.isnan(sim12[:, z1]).all())
        assert nn21[:, z2].tolist() == [0, 0] and bool(torch.isnan(sim21[:, z2]).all())
        keep1, keep2 = torch.arange(154) != z1, torch.arange(130) != z2
        assert bool(torch.isfinite(sim12[:, keep1]).all()) and bool(torch.isfinite(sim21[:, keep2]).all())
        # no other row is disturbed: rows that did not choose the zeroed pixel before keep their bits
        same1, same2 = keep1[None] & (ref[0] != z2), keep2[None] & (ref[2] != z1)
        assert torch.equal(nn12[same1], ref[0][same1]) and torch.equal(sim12[same1].view(torch.int32), ref[1][same1].view(torch.int32))
        assert torch.equal(nn21[same2], ref[2][same2]) and torch.equal(sim21[same2].view(torch.int32), ref[3][same2].view(torch.int32))
    # every pixel of one map zero: no row is answered
    f1, f2 = feats(1, 16, 3, 3, seed=83), torch.zeros(1, 16, 2, 2, dtype=torch.float16)
    nn12, sim12, nn21, sim21 = launch(_lib(), f1.cuda(), f2.cuda())
    assert not bool(nn12.any()) and not bool(nn21.any()) and bool(torch.isnan(sim12).all()) and bool(torch.isnan(sim21).all())


def test_strided_views_keep_the_nan_padding_out():
    """both maps are views into larger NaN-filled buffers: x stride 2 inside an NCHW buffer (the any-stride path), and a channels-last buffer
    whose pixels are 8 channels longer than C (the K padding must come from zeros, not from the neighbouring memory)"""
    B, C_, h, w = 2, 24, 9, 8
    L = _lib()

    def nchw_view(v):
        buf = torch.full((B, C_ + 3, h + 2, 2 * w + 1), float("nan"), dtype=v.dtype, device="cuda")
        view = buf[:, 1:C_ + 1, 1:h + 1, 1:2 * w:2]
        view.copy_(v)
        return buf, view

    def cl_view(v):
        buf = torch.full((B, h + 1, w + 2, C_ + 8), float("nan"), dtype=v.dtype, device="cuda")
        view = buf[:, :h, 1:w + 1, :C_].permute(0, 3, 1, 2)
        view.copy_(v)
        return buf, view

    for f32 in (False, True):
        v1, v2 = feats(B, C_, h, w, f32=f32, seed=31), feats(B, C_, h, w, f32=f32, seed=32)
        for what, mk in (("x stride 2", nchw_view), ("padded channels-last pixels", cl_view)):
            b1, d1 = mk(v1)
            b2, d2 = mk(v2)
            assert tuple(d2.shape) == (B, C_, h, w) and not d2.is_contiguous() and bool(torch.isnan(b2).any())
            got = launch(L, d1, d2)
            assert bool(torch.isfinite(got[1]).all()) and bool(torch.isfinite(got[3]).all())
            for b in range(B):
                R.check(got[0][b].numpy(), got[1][b].numpy(), got[2][b].numpy(), got[3][b].numpy(), v1[b].numpy(), v2[b].numpy(),
                        "%s, sample %d" % (what, b))


def test_one_direction_only_leaves_the_other_outputs_untouched():
    f1, f2 = feats(2, 72, 13, 12, seed=91).cuda(), feats(2, 72, 11, 14, f32=True, seed=92).cuda()
    L = _lib()
    both = launch(L, f1, f2)
    rows = launch(L, f1, f2, cols=False)                                          # launch() asserts that the null direction's buffers keep the guard
    cols = launch(L, f1, f2, rows=False)
    assert rows[2] is None and cols[0] is None
    assert same_bits(rows[:2], both[:2]) and same_bits(cols[2:], both[2:])


def test_streams_repeats_and_a_running_gemm_keep_the_bits():
    """the same inputs: the same bits on a second stream, on a repeated call, and while a GEMM runs on another stream.  Once each, no loop."""
    L = _lib()
    pairs = [(feats(2, 200, 20, 19, seed=41).cuda(), feats(2, 200, 17, 21, seed=42).cuda()),
             (feats(1, 72, 20, 19, f32=True, seed=43).cuda(), _cl(feats(1, 72, 17, 21, seed=44)).cuda())]
    solo = [launch(L, d1, d2) for d1, d2 in pairs]
    again = [launch(L, d1, d2) for d1, d2 in pairs]
    s0, s1 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    other = [launch(L, d1, d2, st=vp(s0.cuda_stream)) for d1, d2 in pairs]
    M = K = 4096
    g = torch.Generator().manual_seed(0)
    A = (torch.randn(M, K, generator=g) * 0.1).half().cuda()
    Wt = (torch.randn(M, K, generator=g) * 0.1).half().cuda()
    o16 = torch.zeros(M, M, dtype=torch.half, device="cuda")
    torch.cuda.synchronize()
    for _ in range(6):                                                            # a few milliseconds of GEMM queued on s1, then the calls on s0
        ok(L.gdf_op_gemm(P(A), K, P(Wt), None, None, None, 0, P(o16), M, None, 0, M, M, K, 0, vp(s1.cuda_stream)), L)
    beside = [launch(L, d1, d2, st=vp(s0.cuda_stream)) for d1, d2 in pairs]
    for got in (again, other, beside):
        for g_, w_ in zip(got, solo):
            assert same_bits(g_, w_)
    assert bool(torch.isfinite(o16.float()).all())


def test_refusals_and_the_empty_batch_launch_nothing():
    L = _lib()
    d = feats(2, 8, 4, 4).cuda()
    nn, sim = torch.full((32,), PAT32I, dtype=torch.int32, device="cuda"), guard((32,), torch.float32)
    nbytes = L.gdf_op_dense_match_workspace(2, 8, 16, 16, 0, 0)
    ws = torch.full((nbytes,), PAT8, dtype=torch.uint8, device="cuda")
    s1, s2 = R.agg_src(d.data_ptr(), 0, d.stride(), d.shape), R.agg_src(d.data_ptr(), 0, d.stride(), d.shape)

    def call(B=2, nb=nbytes, n=nn):
        return L.gdf_op_dense_match(ctypes.addressof(s1), ctypes.addressof(s2), B, P(n) if n is not None else None, P(sim), P(nn), P(sim), P(ws), nb,
                                    stream())
    assert call(nb=nbytes - 1) == R.GDF_ERR_ARG and call(B=-1) == R.GDF_ERR_ARG and call(n=None) == R.GDF_ERR_ARG
    assert b"gdf_op_dense_match" in L.gdf_last_error()
    s2.C = 9
    assert call() == R.GDF_ERR_ARG
    s2.C = 8
    assert call(B=65536) == R.GDF_ERR_UNSUPPORTED
    assert call(B=0) == 0
    torch.cuda.synchronize()
    assert bool((nn.cpu() == PAT32I).all()) and bool(is_guard(sim.cpu()).all()) and bool((ws.cpu() == PAT8).all())


# ------------------------------------------------------------------------------------------------------------------------------
# Python level
# ------------------------------------------------------------------------------------------------------------------------------
def test_python_wrappers_agree_with_the_c_call():
    import diffusion_feature
    from components.postproc import cycle_index, dense_match, dense_nn_correspondences, mutual_nn
    f1, f2 = feats(2, 40, 12, 12, seed=51), feats(2, 40, 12, 12, f32=True, chlast=True, seed=52)
    d1, d2 = f1.cuda(), f2.cuda()
    want = launch(_lib(), d1, d2)
    got = dense_match(d1, d2)
    assert all(t.is_cuda for t in got) and got[0].dtype == torch.int64 and got[2].dtype == torch.int64 and got[1].dtype == torch.float32
    assert same_bits([got[0].cpu().int(), got[1].cpu(), got[2].cpu().int(), got[3].cpu()], want)
    one = dense_match(d1, d2, "21")
    assert one[0] is None and one[1] is None and torch.equal(one[2], got[2])
    fe = diffusion_feature.FeatureExtractor.__new__(diffusion_feature.FeatureExtractor)
    assert all(torch.equal(x, y) for x, y in zip(fe.match(d1, d2), got))
    # mutual_nn's mask, recomputed from the op's own outputs
    mask, nn12, sim12 = mutual_nn(d1, d2)
    nn12_w, nn21_w = want[0].long(), want[2].long()
    assert torch.equal(mask.cpu(), nn21_w.gather(1, nn12_w) == torch.arange(144)[None]) and torch.equal(nn12.cpu(), nn12_w)
    assert torch.equal(cycle_index(got[0], got[2]).cpu(), nn21_w.gather(1, nn12_w)) and 0 < int(mask.sum()) < mask.numel()
    m2 = fe.match(d1, d2, mutual=True)
    assert torch.equal(m2[0], mask) and torch.equal(m2[1], nn12) and torch.equal(m2[2].view(torch.int32), sim12.view(torch.int32))
    sal1, sal2 = torch.rand(2, 144, generator=gen(5)), torch.rand(2, 12, 12, generator=gen(6))
    masked = mutual_nn(d1, d2, sal1, sal2.cuda(), thresh=0.4)[0].cpu()
    reached = torch.zeros(2, 144, dtype=torch.bool)
    for b in range(2):
        reached[b, nn21_w[b][sal2[b].reshape(-1) > 0.4]] = True
    assert torch.equal(masked, mask.cpu() & (sal1 > 0.4) & reached)
    p1, p2 = dense_nn_correspondences(d1, d2)
    assert p1.dtype == torch.float32 and p2.dtype == torch.float32 and tuple(p1.shape) == tuple(p2.shape) == (2, 144, 2)
    assert torch.equal(p2.cpu(), torch.stack([nn12_w // 12, nn12_w % 12], -1).float())
    assert p1[0, 13].tolist() == [1.0, 1.0] and p1[1, 25].tolist() == [2.0, 1.0]


@pytest.mark.parametrize("name", ["nn_fp16", "nn_fp32"])
def test_reference_results_on_the_device(name):
    from components.postproc import dense_match, dense_nn_correspondences
    z = np.load(os.path.join(ROOT, "tests", "golden", "dense_match.npz"))
    f1, f2 = torch.from_numpy(z[name + ":f1"]), torch.from_numpy(z[name + ":f2"])
    nn12, sim12, nn21, sim21 = (t.cpu() for t in dense_match(f1.cuda(), f2.cuda()))
    amb12, amb21 = R.check(nn12[0].numpy(), sim12[0].numpy(), nn21[0].numpy(), sim21[0].numpy(), f1[0].numpy(), f2[0].numpy(), "golden " + name)
    assert np.array_equal(nn12[0].numpy()[~amb12], z[name + ":nn12"][0][~amb12]) and np.array_equal(nn21[0].numpy()[~amb21], z[name + ":nn21"][0][~amb21])
    p1, p2 = dense_nn_correspondences(f1.cuda(), f2.cuda())
    assert np.array_equal(p1.cpu().numpy(), z[name + ":points1"]) and np.array_equal(p2.cpu().numpy()[0][~amb12], z[name + ":points2"][0][~amb12])


def test_best_buddies_on_the_device_equal_the_reference():
    pytest.importorskip("sklearn")
    from components.postproc import find_best_buddies_correspondences, mutual_nn
    z = np.load(os.path.join(ROOT, "tests", "golden", "dense_match.npz"))
    d1, d2, s1, s2 = (torch.from_numpy(z["bb:" + k]).cuda() for k in ("d1", "d2", "s1", "s2"))
    k, thresh = int(z["bb:args"][0]), float(z["bb:args"][1])
    f1, f2 = (d[:, 0].permute(0, 2, 1)[..., None] for d in (d1, d2))
    mask, nn12, _ = mutual_nn(f1, f2, s1, s2, thresh)
    S = R.oracle(z["bb:d1"][0, 0].T[:, :, None], z["bb:d2"][0, 0].T[:, :, None])
    tol = R.tolerance(d1.shape[-1], 2)
    assert not R.ambiguous(S, tol, np.arange(S.shape[1])).any() and not R.ambiguous(S.T, tol, np.arange(S.shape[0])).any()
    assert np.array_equal(nn12[0].cpu().numpy(), z["bb:nn12"]) and np.array_equal(mask[0].cpu().numpy(), z["bb:mask"])
    p1, p2 = find_best_buddies_correspondences(d1, d2, s1, s2, num_pairs=k, thresh=thresh)
    # x = idx % n is an integer and exact; y = idx / n is a float32 quotient, which the device's division rounds within one ulp of the host's
    for got, want in ((p1.cpu().numpy(), z["bb:points1"]), (p2.cpu().numpy(), z["bb:points2"])):
        assert got.shape == want.shape and np.array_equal(got[:, 1], want[:, 1]) and np.array_equal(np.rint(got[:, 0] * 12), np.rint(want[:, 0] * 12))
        assert np.allclose(got[:, 0], want[:, 0], rtol=2.0 ** -22, atol=0)
