"""Output-stage post-processing on the GPU through libgdf.so (include/gdf_ops.h, csrc/post.hip) — the steps right after
the hot path:

  resize_concat      extract_feature.py:113-125   `--aggregate_output`: nearest-resize every layer to the largest H, W, concat
  aggregate          correspondence/aggregation_network.py:62-66, scarce_segmentation/task-pixel.py:50-55   the evaluators' form of it:
                     F.interpolate(v, size, mode='bilinear') of every layer + torch.cat(dim=1), one launch per 16 layers
  nn_match / find_nn_source_correspondences   correspondence/correspondence/correspondence_utils.py:113-138   the evaluators' second step:
                     nearest neighbours of N source points among the load-size target pixels, without either load-size map (csrc/corres.hip)
  dense_match / mutual_nn / dense_nn_correspondences / find_best_buddies_correspondences   correspondence/correspondence/correspondence_utils.py:
                     73-111, 230-323   dense matching of two maps: best pixel and cosine in both directions from one MFMA pass, the P1 x P2
                     matrix never built (csrc/densematch.hip)
  clip_loss / compute_clip_loss   correspondence/task-corres.py:70-80   the evaluator's loss on two hyperfeature maps, forward and backward,
                     without either P x P similarity matrix (csrc/cliploss.hip); a torch.autograd.Function on device tensors
  PixelClassifierEnsemble / predict_labels    scarce_segmentation/segmentation/pixel_classifier.py:14-36, 70-107   the label-scarce evaluator's
                     second step: an ensemble of per-pixel MLPs, majority vote and Jensen-Shannon uncertainty (csrc/pixcls.hip)
  AggregationHead    correspondence/correspondence/aggregation_network.py:20-22, 97-100   the correspondence evaluator's trained head: the fp32
                     3 x 3 output convolution on the aggregated map (csrc/agghead.hip)
  TrainableAggregationHead   correspondence/task-corres.py:144-162 train() on aggregation_network.out   the same head as a torch.nn.Module whose
                     forward is that device convolution and whose backward is the device weight gradient (csrc/aggwgrad.hip); updated weights
                     are repacked on the device
  pca / pca_rgb      feature_visualization.py:84-101   plot_pca: the PCA of a feature map and its picture (csrc/pca.hip)
  rescale_points / compute_pck   correspondence/correspondence/correspondence_utils.py:53-59, 160-167   validate()'s two host helpers (numpy)
  avg_pool           components/feature_extractor.py:51-53   `feature_resize` (adaptive_avg_pool2d to (H/r, W/r))
  aggregate_maps     components/attention.py:238-244, 141-161 + diffusion_feature.py:492-500   aggregated `attn` feature

Device tensors go through the HIP kernels (and fail loudly if the library is missing); host tensors (accept-all mode hands
out `.cpu()` copies, feature_extractor.py:65-66) are plain data already off the GPU path and use torch on the CPU.
"""
import collections
import ctypes as C
import math
import warnings

import numpy as np
import torch
import torch.nn.functional as F

from . import native

_SIG = {
    "gdf_op_resize_concat": (C.c_int, [C.c_void_p, C.c_int, C.c_long, C.c_long, C.c_long, C.c_long, C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "gdf_op_avg_pool": (C.c_int, [C.c_void_p, C.c_long, C.c_long, C.c_long, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                  C.c_void_p]),
    "gdf_op_maps_mean": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
}


class AggSrc(C.Structure):
    """gdf_agg_src (include/gdf_ops.h)"""
    _fields_ = [("ptr", C.c_void_p), ("f32", C.c_int), ("sb", C.c_long), ("sc", C.c_long), ("sy", C.c_long), ("sx", C.c_long),
                ("C", C.c_int), ("H", C.c_int), ("W", C.c_int), ("coff", C.c_int)]


_SIG["gdf_op_aggregate"] = (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p])
AGG_MAX = 16                                             # sources of one gdf_op_aggregate launch
_SIG["gdf_op_nn_match_workspace"] = (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int])
_SIG["gdf_op_nn_match"] = (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_size_t, C.c_void_p])
_SIG["gdf_op_dense_match_workspace"] = (C.c_size_t, [C.c_int] * 6)
_SIG["gdf_op_dense_match"] = (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                        C.c_void_p])
_SIG["gdf_op_clip_loss_workspace"] = (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int])
_SIG["gdf_op_clip_loss"] = (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_size_t, C.c_void_p])
_SIG["gdf_op_clip_loss_backward"] = (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p])
_SIG["gdf_pixcls_create"] = (C.c_int, [C.c_int] * 5 + [C.c_void_p] * 6 + [C.POINTER(C.c_void_p)])
_SIG["gdf_pixcls_destroy"] = (None, [C.c_void_p])
_SIG["gdf_pixcls_workspace"] = (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int])
_SIG["gdf_pixcls_predict"] = (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                        C.c_void_p])
_SIG["gdf_agghead_create"] = (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)])
_SIG["gdf_agghead_destroy"] = (None, [C.c_void_p])
_SIG["gdf_agghead_forward"] = (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p])
_SIG["gdf_agghead_create_device"] = (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)])
_SIG["gdf_agghead_update"] = (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p])
_SIG["gdf_agghead_wgrad_workspace"] = (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int])
_SIG["gdf_agghead_wgrad"] = (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p])
_SIG["gdf_op_pca_workspace"] = (C.c_size_t, [C.c_int] * 6)
_SIG["gdf_op_pca"] = (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p])
_SIG["gdf_op_pca_rgb"] = (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p])
_lib = None


def _L():
    global _lib
    if _lib is None:
        lib = native.load_library()
        for n, (r, a) in _SIG.items():
            f = getattr(lib, n)
            f.restype, f.argtypes = r, a
        _lib = lib
    return _lib


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def resize_concat(feats, size=None):
    """[(B, C_l, H_l, W_l) fp16 / fp32 tensors, any strides] -> (B, sum C_l, S, S) fp16, S = max W_l unless given:
    F.interpolate(v, S) (nearest) of every tensor + torch.cat(dim=1)."""
    feats = list(feats)
    S = int(size or max(v.shape[-1] for v in feats))
    if not feats[0].is_cuda:
        return torch.cat([F.interpolate(v, S) for v in feats], dim=1)
    dev = feats[0].device
    B = feats[0].shape[0]
    ctot = sum(v.shape[1] for v in feats)
    with torch.cuda.device(dev):
        out = torch.empty(B, ctot, S, S, dtype=torch.float16, device=dev)
        off = 0
        for v in feats:
            if v.dtype not in (torch.float16, torch.float32):
                v = v.float()
            b, c, h, w = v.shape
            sb, sc, sy, sx = v.stride()
            native._check(_L().gdf_op_resize_concat(C.c_void_p(v.data_ptr()), int(v.dtype == torch.float32), sb, sc, sy, sx, b, c, h, w,
                                                    C.c_void_p(out.data_ptr()), ctot, off, S, _stream(dev)), "resize_concat")
            off += c
    return out


def aggregate(feats, size=None, mode='bilinear', dtype=torch.float16):
    """[(B, C_l, H_l, W_l) tensors, any strides] -> (B, sum C_l, OH, OW) `dtype` (fp16 or fp32):
    torch.cat([F.interpolate(v, size, mode=mode) for v in feats], 1), mode 'bilinear' (align_corners=False) or 'nearest'.
    size: an int, (OH, OW), or None = the largest W (as resize_concat).  Device tensors: aggregate_kernel, one launch per 16 tensors."""
    feats = list(feats)
    if mode not in ('nearest', 'bilinear'):
        raise ValueError(f"mode is 'nearest' or 'bilinear', not {mode!r}")
    if dtype not in (torch.float16, torch.float32):
        raise ValueError(f"dtype is torch.float16 or torch.float32, not {dtype}")
    if not feats or any(v.dim() != 4 for v in feats):
        raise ValueError("feats is a non-empty list of 4-D tensors")
    if size is None:
        size = max(v.shape[-1] for v in feats)
    OH, OW = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
    if not feats[0].is_cuda:
        return torch.cat([F.interpolate(v.float(), (OH, OW), mode=mode) for v in feats], 1).to(dtype)
    dev = feats[0].device
    B = feats[0].shape[0]
    if any(v.shape[0] != B or v.device != dev for v in feats):
        raise ValueError("every tensor has the same batch size and device")
    feats = [v if v.dtype in (torch.float16, torch.float32) else v.float() for v in feats]
    ctot = sum(v.shape[1] for v in feats)
    with torch.cuda.device(dev):
        out = torch.empty(B, ctot, OH, OW, dtype=dtype, device=dev)
        off = 0
        for i in range(0, len(feats), AGG_MAX):
            part = feats[i:i + AGG_MAX]
            srcs = (AggSrc * len(part))()
            for s, v in zip(srcs, part):
                s.ptr, s.f32 = v.data_ptr(), int(v.dtype == torch.float32)
                s.sb, s.sc, s.sy, s.sx = v.stride()
                _, s.C, s.H, s.W = v.shape
                s.coff = off
                off += v.shape[1]
            native._check(_L().gdf_op_aggregate(srcs, len(part), B, C.c_void_p(out.data_ptr()), int(dtype == torch.float32), ctot, OH, OW,
                                                int(mode == 'bilinear'), _stream(dev)), "aggregate")
    return out


def _agg_src(v):
    s = AggSrc()
    s.ptr, s.f32 = v.data_ptr(), int(v.dtype == torch.float32)
    s.sb, s.sc, s.sy, s.sx = v.stride()
    _, s.C, s.H, s.W = v.shape
    return s


def nn_match(feats1, feats2, source_points, load_size=(512, 512)):
    """feats1 (B, C, h1, w1), feats2 (B, C, h2, w2), fp16 or fp32 with any strides; source_points (B, N, 2) or, for B = 1, (N, 2): (y, x) in
    load-size coordinates -> (points2 int64 (B, N, 2) (y, x), scores fp32 (B, N)).
    The reference's find_nn_source_correspondences for a load size (LH, LW): both maps F.interpolate'd to it (bilinear), the source pixels
    idx = LW * round(clip(y, 0, LH - 1)) + round(clip(x, 0, LW - 1)) (np.round: half to even) gathered, both sides L2-normalised, argmax of q @ k^T
    (lowest index of the maximum) and the cosine there.  Device tensors: gdf_op_nn_match, which builds neither load-size map; host tensors: that
    torch chain in fp32."""
    LH, LW = (int(load_size), int(load_size)) if isinstance(load_size, int) else (int(load_size[0]), int(load_size[1]))
    if feats1.dim() != 4 or feats2.dim() != 4 or feats1.shape[0] != feats2.shape[0] or feats1.shape[1] != feats2.shape[1]:
        raise ValueError("feats1 and feats2 are (B, C, h, w) tensors with the same B and C")
    if LH < 1 or LW < 1:
        raise ValueError("load_size >= 1")
    B = feats1.shape[0]
    pts = torch.as_tensor(source_points)
    if pts.dim() == 2 and B == 1:
        pts = pts[None]
    if pts.dim() != 3 or pts.shape[0] != B or pts.shape[2] != 2 or pts.shape[1] < 1:
        raise ValueError("source_points is (B, N, 2), or (N, 2) for B = 1, with N >= 1")
    N = pts.shape[1]
    if not feats2.is_cuda:
        f1 = F.interpolate(feats1.float(), (LH, LW), mode="bilinear")
        f2 = F.interpolate(feats2.float(), (LH, LW), mode="bilinear")
        p = pts.detach().cpu().double().numpy()
        idx = torch.from_numpy((LW * np.round(np.clip(p[..., 0], 0, LH - 1)) + np.round(np.clip(p[..., 1], 0, LW - 1))).astype(np.int64))
        f1 = f1.flatten(2).permute(0, 2, 1)
        f2 = f2.flatten(2).permute(0, 2, 1)
        q = torch.gather(f1, 1, idx[..., None].expand(B, N, f1.shape[2]))
        q = q / torch.linalg.norm(q, dim=-1)[:, :, None]
        f2 = f2 / torch.linalg.norm(f2, dim=-1)[:, :, None]
        score, best = torch.matmul(q, f2.permute(0, 2, 1)).max(dim=-1)
        return torch.stack([best // LW, best % LW], dim=-1), score
    dev = feats2.device
    if feats1.device != dev:
        raise ValueError("feats1 and feats2 are on the same device")
    feats1, feats2 = (v if v.dtype in (torch.float16, torch.float32) else v.float() for v in (feats1, feats2))
    with torch.cuda.device(dev):
        pts = pts.to(device=dev, dtype=torch.float32).contiguous()
        out = torch.empty(B, N, 2, dtype=torch.int64, device=dev)
        score = torch.empty(B, N, dtype=torch.float32, device=dev)
        if B == 0:
            return out, score
        L = _L()
        nbytes = L.gdf_op_nn_match_workspace(B, N, feats2.shape[1], feats2.shape[2], feats2.shape[3])
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        s1, s2 = _agg_src(feats1), _agg_src(feats2)
        native._check(L.gdf_op_nn_match(C.addressof(s1), C.addressof(s2), B, C.c_void_p(pts.data_ptr()), N, LH, LW, C.c_void_p(out.data_ptr()),
                                        C.c_void_p(score.data_ptr()), C.c_void_p(ws.data_ptr()), nbytes, _stream(dev)), "nn_match")
    return out, score


def find_nn_source_correspondences(img1_feats, img2_feats, source_points, output_size, load_size):
    """The reference's function (correspondence/correspondence/correspondence_utils.py:113-138), same signature and return value:
    source_points a numpy (N, 2) array of (y, x) in load-size coordinates -> (points1 = torch.from_numpy(source_points), points2 (N, 2) int64
    (y, x) of batch element 0).  output_size is unused, as in the reference.  The points are clipped and rounded on the host in their own
    precision (np.round), so a float64 annotation rounds as the reference rounds it."""
    LH, LW = (int(load_size), int(load_size)) if isinstance(load_size, int) else (int(load_size[0]), int(load_size[1]))
    p = np.asarray(source_points)
    idx = np.stack([np.round(np.clip(p[:, 0], 0, LH - 1)), np.round(np.clip(p[:, 1], 0, LW - 1))], -1).astype(np.float32)
    B = img1_feats.shape[0]
    points2, _ = nn_match(img1_feats, img2_feats, torch.from_numpy(idx)[None].expand(B, -1, -1), (LH, LW))
    return torch.from_numpy(source_points), points2[0]


def dense_match(feats1, feats2, directions="both"):
    """feats1 (B, C, h1, w1), feats2 (B, C, h2, w2), fp16 or fp32 with any strides -> (nn12 int64 (B, P1), sim12 fp32 (B, P1), nn21 int64 (B, P2),
    sim21 fp32 (B, P2)), P = h * w, pixel p = y * w + x: for every pixel of feats1 its pixel of feats2 with the highest cosine similarity (lowest
    index of the maximum) and that cosine, and the same for every pixel of feats2 among those of feats1.
    The reference's batch_cosine_sim followed by max over both axes of the (B, P1, P2) matrix.  Device tensors: gdf_op_dense_match, which never
    builds the matrix; host tensors: that torch chain in fp32.  directions: "both", "12" or "21"; the pair not asked for is returned as None.
    A pixel of zero norm never wins; its own entry is index 0 with a NaN score on the device (the host chain propagates NaN as the reference)."""
    if feats1.dim() != 4 or feats2.dim() != 4 or feats1.shape[0] != feats2.shape[0] or feats1.shape[1] != feats2.shape[1]:
        raise ValueError("feats1 and feats2 are (B, C, h, w) tensors with the same B and C")
    if directions not in ("both", "12", "21"):
        raise ValueError(f"directions is 'both', '12' or '21', not {directions!r}")
    if min(feats1.shape[1:]) < 1 or min(feats2.shape[1:]) < 1:
        raise ValueError("C, h and w >= 1")
    B, Cn = feats1.shape[:2]
    P1, P2 = feats1.shape[2] * feats1.shape[3], feats2.shape[2] * feats2.shape[3]
    d12, d21 = directions != "21", directions != "12"
    if not feats2.is_cuda:
        a = feats1.float().flatten(2).permute(0, 2, 1)
        b = feats2.float().flatten(2).permute(0, 2, 1)
        a = a / torch.linalg.norm(a, dim=-1)[:, :, None]
        b = b / torch.linalg.norm(b, dim=-1)[:, :, None]
        sims = torch.matmul(a, b.permute(0, 2, 1))
        sim12, nn12 = sims.max(dim=-1) if d12 else (None, None)
        sim21, nn21 = sims.max(dim=-2) if d21 else (None, None)
        return nn12, sim12, nn21, sim21
    dev = feats2.device
    if feats1.device != dev:
        raise ValueError("feats1 and feats2 are on the same device")
    feats1, feats2 = (v if v.dtype in (torch.float16, torch.float32) else v.float() for v in (feats1, feats2))
    with torch.cuda.device(dev):
        nn12 = torch.empty(B, P1, dtype=torch.int32, device=dev) if d12 else None
        sim12 = torch.empty(B, P1, dtype=torch.float32, device=dev) if d12 else None
        nn21 = torch.empty(B, P2, dtype=torch.int32, device=dev) if d21 else None
        sim21 = torch.empty(B, P2, dtype=torch.float32, device=dev) if d21 else None
        if B > 0:
            L = _L()
            f32 = [int(v.dtype == torch.float32) for v in (feats1, feats2)]
            nbytes = L.gdf_op_dense_match_workspace(B, Cn, P1, P2, f32[0], f32[1])
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            s1, s2 = _agg_src(feats1), _agg_src(feats2)
            ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None       # noqa: E731
            native._check(L.gdf_op_dense_match(C.addressof(s1), C.addressof(s2), B, ptr(nn12), ptr(sim12), ptr(nn21), ptr(sim21),
                                               C.c_void_p(ws.data_ptr()), nbytes, _stream(dev)), "dense_match")
    return (nn12.long() if d12 else None), sim12, (nn21.long() if d21 else None), sim21


def cycle_index(nn12, nn21):
    """nn21.gather(1, nn12) (B, P1): where the cycle image 1 -> image 2 -> image 1 ends for every pixel of image 1; the input of cycle-consistency
    masks and distances (the reference's find_cyclical_correspondences computes it as torch.gather(nn_2, dim=-1, index=nn_1))."""
    return nn21.gather(1, nn12)


def _mutual_mask(nn12, nn21, saliency1, saliency2, thresh):
    B, P1 = nn12.shape
    mask = cycle_index(nn12, nn21) == torch.arange(P1, device=nn12.device)[None]
    if saliency1 is not None:
        mask = mask & (torch.as_tensor(saliency1).to(nn12.device).reshape(B, P1) > thresh)
    if saliency2 is not None:
        fg2 = torch.as_tensor(saliency2).to(nn12.device).reshape(B, nn21.shape[1]) > thresh
        hit = torch.zeros(B, P1, dtype=torch.int32, device=nn12.device)
        hit.scatter_add_(1, nn21, fg2.to(torch.int32))
        mask = mask & (hit > 0)
    return mask


def mutual_nn(feats1, feats2, saliency1=None, saliency2=None, thresh=0.05):
    """Mutual nearest neighbours ("best buddies") of two maps -> (mask (B, P1) bool, nn12 int64 (B, P1), sim12 fp32 (B, P1)):
    mask[b, p] = nn21[b, nn12[b, p]] == p, i.e. pixel p of feats1 and its best pixel of feats2 choose each other.  Both directions come from
    ONE dense_match call, so they reduce the same similarity bits.
    With saliencies ((B, P1) and (B, P2), or (B, h, w) maps) the mask is combined with the two foreground conditions of the reference's
    find_best_buddies_correspondences: saliency1[p] > thresh, and p is the nearest neighbour of at least one pixel q of feats2 with
    saliency2[q] > thresh.  Either saliency may be given alone.  O(P) torch ops on the vectors of dense_match; cycle_index(nn12, nn21) is
    the gather this mask compares with arange."""
    nn12, sim12, nn21, _ = dense_match(feats1, feats2)
    return _mutual_mask(nn12, nn21, saliency1, saliency2, thresh), nn12, sim12


def dense_nn_correspondences(feats1, feats2):
    """(points1, points2) in the layout of the reference's find_nn_correspondences (correspondence_utils.py:90-111): float32 (b, P, 2), points1 its
    meshgrid of the (h, w) grid of feats2 (it derives the grid from the matrix's last axis and assumes a square one; here w and h are taken
    from feats2, so square grids give the reference's values), points2 = (nn12 // h, nn12 % h).  Deliberate deviation: this function takes the two
    maps, not the (b, P, P) matrix, which is never built (dense_match); the two maps must have the same number of pixels, as the reference's
    expand() requires."""
    w, h = feats2.shape[2], feats2.shape[3]
    if feats1.shape[2] * feats1.shape[3] != w * h:
        raise ValueError("find_nn_correspondences' layout needs maps of the same number of pixels")
    nn12 = dense_match(feats1, feats2, "12")[0]
    b = nn12.shape[0]
    points1 = torch.stack(torch.meshgrid(torch.arange(w, device=nn12.device), torch.arange(h, device=nn12.device), indexing="ij"), dim=-1).expand((b, w, h, 2)).reshape((b, -1, 2))
    points2 = torch.stack([nn12 // h, nn12 % h], dim=-1)
    return points1.to(torch.float32), points2.to(torch.float32)


def find_best_buddies_correspondences(descriptors1, descriptors2, saliency_map1, saliency_map2, num_pairs=10, thresh=0.05):
    """The reference's function (correspondence_utils.py:230-323), same signature and return value: descriptors B x 1 x T x D of a square token
    grid, saliency maps B x T -> (points1, points2), (k, 2) (y, x) in token coordinates of batch element 0 (y is the true quotient idx / n, a
    float, as in the reference), k <= num_pairs; ([], []) if no pair survives.  The similarity matrix and its two max go through dense_match
    (mutual_nn); the selection — k-means on the normalised concatenated descriptors of the surviving pairs, the most salient pair per
    cluster — uses scikit-learn's KMeans(random_state=0) as the reference does."""
    try:
        from sklearn.cluster import KMeans
    except ImportError as e:
        raise ImportError("find_best_buddies_correspondences selects its pairs with scikit-learn's KMeans, which is not importable here; "
                          "mutual_nn gives the best-buddies mask without it") from e
    B, _, T, D = descriptors1.shape
    n = int(np.sqrt(T))
    f1 = descriptors1[:1, 0].permute(0, 2, 1)[..., None]                  # (1, D, T, 1): a logical (B, C, h, w) map, any strides
    f2 = descriptors2[:1, 0].permute(0, 2, 1)[..., None]
    sal1, sal2 = saliency_map1[0], saliency_map2[0]
    mask, nn1, _ = mutual_nn(f1, f2, sal1[None], sal2[None], thresh)
    mask, nn1 = mask[0], nn1[0]
    d1 = descriptors1[0, 0, mask, :].float().cpu().numpy()
    d2 = descriptors2[0, 0, nn1[mask], :].float().cpu().numpy()
    both = np.concatenate((d1, d2), axis=1)
    if len(both) == 0:
        return [], []
    both = both / np.sqrt((both ** 2).sum(axis=1))[:, None]
    k = min(num_pairs, len(both))
    labels = KMeans(n_clusters=k, random_state=0).fit(both).labels_
    rank = ((sal1[mask] + sal2[nn1[mask]]) / 2).cpu().numpy()
    best, pick = np.full(k, -np.inf), np.zeros(k, dtype=np.int64)
    for i, (lab, rk) in enumerate(zip(labels, rank)):                     # the first pair of the highest mean saliency in every cluster
        if rk > best[lab]:
            best[lab], pick[lab] = rk, i
    idx1 = torch.nonzero(mask, as_tuple=False).squeeze(1)[pick]
    idx2 = nn1[idx1]
    return torch.stack([idx1 / n, idx1 % n], dim=-1), torch.stack([idx2 / n, idx2 % n], dim=-1)


CLIP_SCALE = 1 / 0.07                                 # exp(logit_scale) of the reference's AggregationNetwork (aggregation_network.py:25)


class _ClipLoss(torch.autograd.Function):
    """gdf_op_clip_loss / gdf_op_clip_loss_backward on device maps: the forward leaves the backward's state in a workspace tensor that the graph
    keeps; grad_output goes down as the device (B,) tensor, nothing is read back."""

    @staticmethod
    def forward(ctx, feats1, feats2, src, tgt, scale):
        dev = feats1.device
        B, N = src.shape
        with torch.cuda.device(dev):
            L = _L()
            loss = torch.empty(B, dtype=torch.float32, device=dev)
            P1, P2 = feats1.shape[2] * feats1.shape[3], feats2.shape[2] * feats2.shape[3]
            nbytes = L.gdf_op_clip_loss_workspace(B, N, feats1.shape[1], P1, P2)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            s1, s2 = _agg_src(feats1), _agg_src(feats2)
            native._check(L.gdf_op_clip_loss(C.addressof(s1), C.addressof(s2), B, C.c_void_p(src.data_ptr()), C.c_void_p(tgt.data_ptr()), N, scale,
                                             C.c_void_p(loss.data_ptr()), None, C.c_void_p(ws.data_ptr()), nbytes, _stream(dev)), "clip_loss")
        ctx.save_for_backward(feats1, feats2, src, tgt, ws)
        ctx.scale = scale
        return loss

    @staticmethod
    def backward(ctx, grad):
        feats1, feats2, src, tgt, ws = ctx.saved_tensors
        dev = feats1.device
        B, N = src.shape
        need = ctx.needs_input_grad[:2]
        with torch.cuda.device(dev):
            grad = grad.to(torch.float32).contiguous()
            g = [torch.empty(v.shape, dtype=torch.float32, device=dev) if n else None for v, n in zip((feats1, feats2), need)]
            if any(need):
                s1, s2 = _agg_src(feats1), _agg_src(feats2)
                L = _L()
                native._check(L.gdf_op_clip_loss_backward(
                    C.addressof(s1), C.addressof(s2), B, C.c_void_p(src.data_ptr()), C.c_void_p(tgt.data_ptr()), N, ctx.scale,
                    C.c_void_p(grad.data_ptr()), *(C.c_void_p(t.data_ptr()) if t is not None else None for t in g), C.c_void_p(ws.data_ptr()),
                    ws.numel(), _stream(dev)), "clip_loss_backward")
        g = [t if t is None or t.dtype == v.dtype else t.to(v.dtype) for t, v in zip(g, (feats1, feats2))]
        return g[0], g[1], None, None, None


def clip_loss(feats1, feats2, src_idx, tgt_idx, scale=CLIP_SCALE):
    """feats1 (B, C, h1, w1), feats2 (B, C, h2, w2), fp16 or fp32 with any strides; src_idx, tgt_idx int64 (B, N) or, for B = 1, (N,): flat pixel
    indices y w + x into feats1 and feats2 -> the loss of every pair, (B,) fp32.
    The reference's compute_clip_loss per pair: with both maps L2-normalised per pixel, scale * (rows src_idx of feats1) @ feats2^T against the labels
    tgt_idx and the same with the roles swapped, cross_entropy of each, the mean of the two.  Device tensors: gdf_op_clip_loss as an autograd
    Function (neither P x P matrix is built; gradients come back as fp32 computed, cast to the map's dtype); host tensors: that torch chain in fp32
    on the needed rows, differentiable by torch."""
    if feats1.dim() != 4 or feats2.dim() != 4 or feats1.shape[0] != feats2.shape[0] or feats1.shape[1] != feats2.shape[1]:
        raise ValueError("feats1 and feats2 are (B, C, h, w) tensors with the same B and C")
    if min(feats1.shape[1:]) < 1 or min(feats2.shape[1:]) < 1:
        raise ValueError("C, h and w >= 1")
    scale = float(scale)
    if not (scale > 0 and math.isfinite(scale)):
        raise ValueError("scale is positive and finite")
    B = feats1.shape[0]
    idx = []
    for v in (src_idx, tgt_idx):
        v = torch.as_tensor(v)
        if v.is_floating_point() or v.dtype == torch.bool:
            raise ValueError("src_idx and tgt_idx are integer tensors")
        if v.dim() == 1 and B == 1:
            v = v[None]
        idx.append(v)
    if idx[0].dim() != 2 or idx[0].shape != idx[1].shape or idx[0].shape[0] != B or idx[0].shape[1] < 1:
        raise ValueError("src_idx and tgt_idx are (B, N), or (N,) for B = 1, with N >= 1")
    dev = feats1.device
    if feats2.device != dev:
        raise ValueError("feats1 and feats2 are on the same device")
    src, tgt = (v.to(device=dev, dtype=torch.int64).contiguous() for v in idx)
    if not feats1.is_cuda:
        k1, k2 = (v.float().flatten(2).permute(0, 2, 1) for v in (feats1, feats2))
        k1 = k1 / torch.linalg.norm(k1, dim=-1)[:, :, None]
        k2 = k2 / torch.linalg.norm(k2, dim=-1)[:, :, None]
        out = []
        for b in range(B):
            l1 = F.cross_entropy(scale * (k1[b, src[b]] @ k2[b].T), tgt[b])
            l2 = F.cross_entropy(scale * (k2[b, tgt[b]] @ k1[b].T), src[b])
            out.append((l1 + l2) / 2)
        return torch.stack(out) if out else torch.zeros(0)
    feats1, feats2 = (v if v.dtype in (torch.float16, torch.float32) else v.float() for v in (feats1, feats2))
    if B == 0:
        return torch.zeros(0, dtype=torch.float32, device=dev)
    return _ClipLoss.apply(feats1, feats2, src, tgt, scale)


def points_to_idxs(points, output_size):
    """The reference's formula (correspondence/correspondence/correspondence_utils.py:140-146) verbatim, in the points' own precision: (N, 2) (y, x)
    -> output_size[1] * round(clip(y, 0, output_size[1] - 1)) + round(clip(x, 0, output_size[0] - 1)); np.round rounds half to even."""
    points = np.asarray(points)
    if points.ndim != 2 or points.shape[1] != 2 or points.shape[0] < 1:
        raise ValueError("points is a numpy (N, 2) array of (y, x) with N >= 1")
    points_y = np.clip(points[:, 0], 0, output_size[1] - 1)
    points_x = np.clip(points[:, 1], 0, output_size[0] - 1)
    return output_size[1] * np.round(points_y) + np.round(points_x)


def compute_clip_loss(aggregation_network, img1_hyperfeats, img2_hyperfeats, source_points, target_points, output_size):
    """The reference's function (correspondence/task-corres.py:70-80), same signature and return value: a 0-dim tensor.  B must be 1, as there.
    aggregation_network: anything with a `logit_scale` (a tensor or a number), or None for log(1 / 0.07).  The points are numpy (N, 2) (y, x)
    arrays in output-size coordinates; an index that leaves its map is a ValueError (the reference fails inside its gather)."""
    if img1_hyperfeats.dim() != 4 or img2_hyperfeats.dim() != 4 or img1_hyperfeats.shape[0] != 1 or img2_hyperfeats.shape[0] != 1:
        raise ValueError("compute_clip_loss takes (1, C, h, w) hyperfeatures")
    output_size = (int(output_size), int(output_size)) if isinstance(output_size, int) else (int(output_size[0]), int(output_size[1]))
    if aggregation_network is None:
        scale = CLIP_SCALE
    else:
        ls = aggregation_network.logit_scale
        scale = math.exp(float(ls.detach()) if isinstance(ls, torch.Tensor) else float(ls))
    idx = []
    for pts, v in ((source_points, img1_hyperfeats), (target_points, img2_hyperfeats)):
        i = points_to_idxs(pts, output_size)
        if not np.isfinite(i).all() or (i < 0).any() or (i >= v.shape[2] * v.shape[3]).any():
            raise ValueError("a point's index leaves its %d x %d map (output_size %r)" % (v.shape[2], v.shape[3], output_size))
        idx.append(torch.from_numpy(i.astype(np.int64)))
    if idx[0].shape != idx[1].shape:
        raise ValueError("source_points and target_points have the same length")
    return clip_loss(img1_hyperfeats, img2_hyperfeats, idx[0], idx[1], scale)[0]


_PC_KEYS = ("0.weight", "0.bias", "2.weight", "2.bias", "2.running_mean", "2.running_var", "3.weight", "3.bias", "5.weight", "5.bias",
            "5.running_mean", "5.running_var", "6.weight", "6.bias")
PC_BN_EPS = 1e-5                                         # nn.BatchNorm1d's default, what pixel_classifier builds


def pixel_classifier_params(model):
    """One member of the ensemble -> {"0.weight": fp32 CPU tensor, ...} for the keys of layers.{0,2,3,5,6}: `model` is a reference pixel_classifier
    module (in eval mode: training-mode BatchNorm uses batch statistics, which no folded network reproduces) or its state dict, with or without
    the `module.` prefix nn.DataParallel saves."""
    if isinstance(model, torch.nn.Module):
        if model.training:
            raise ValueError("pixel classifier in training mode: call .eval() (BatchNorm must use its running statistics)")
        model = model.state_dict()
    sd = {}
    for k, v in model.items():
        k = k[len("module."):] if k.startswith("module.") else k
        if k.startswith("layers."):
            sd[k[len("layers."):]] = v.detach().to("cpu", torch.float32)
    missing = [k for k in _PC_KEYS if k not in sd]
    if missing:
        raise ValueError("not a pixel_classifier state dict: no layers.%s" % missing[0])
    w1, w2, w3 = sd["0.weight"], sd["3.weight"], sd["6.weight"]
    if w1.dim() != 2 or w2.dim() != 2 or w3.dim() != 2 or w2.shape[1] != w1.shape[0] or w3.shape[1] != w2.shape[0]:
        raise ValueError("not a pixel_classifier state dict: the three Linear layers do not chain")
    return {k: sd[k] for k in _PC_KEYS}


def fold_pixel_classifier(sd):
    """BatchNorm-folded fp32 parameters (W1, b1, W2, b2, W3, b3) of one pixel_classifier_params dict.  Eval-mode BatchNorm1d after ReLU is
    y = a h + d with a = gamma / sqrt(var + eps), d = beta - mean a, so the next Linear becomes (W diag(a)) h + (W d + b): computed in fp64 and
    rounded once to fp32."""
    d = {k: v.double() for k, v in sd.items()}
    out = [d["0.weight"], d["0.bias"]]
    for bn, lin in (("2", "3"), ("5", "6")):
        a = d[bn + ".weight"] / torch.sqrt(d[bn + ".running_var"] + PC_BN_EPS)
        sh = d[bn + ".bias"] - d[bn + ".running_mean"] * a
        out += [d[lin + ".weight"] * a[None, :], d[lin + ".weight"] @ sh + d[lin + ".bias"]]
    return tuple(v.float().contiguous() for v in out)


class PixelClassifierEnsemble:
    """The reference's list of pixel_classifier models (load_ensemble) as one device op.  models: a list of modules or of state dicts, all of one
    architecture, recognised from the shapes: dim -> 128 -> 32 -> classes, or dim -> 256 -> 128 -> classes from 30 classes up."""

    def __init__(self, models):
        models = list(models)
        if not models:
            raise ValueError("an ensemble has at least one model")
        self.params = [pixel_classifier_params(m) for m in models]
        shapes = [tuple(tuple(v.shape) for v in p.values()) for p in self.params]
        if any(s != shapes[0] for s in shapes):
            raise ValueError("the models of an ensemble have the same shapes")
        w1, w2, w3 = (self.params[0][k] for k in ("0.weight", "3.weight", "6.weight"))
        self.M, self.C, self.h1, self.h2, self.K = len(models), w1.shape[1], w1.shape[0], w2.shape[0], w3.shape[0]
        folded = [fold_pixel_classifier(p) for p in self.params]
        self.folded = tuple(torch.stack([f[i] for f in folded]).contiguous() for i in range(6))     # W1 (M, h1, C), b1, W2, b2, W3, b3
        self._handles = {}

    def _handle(self, dev):
        """gdf_pixcls of this ensemble on `dev` (created on first use there; the library refuses sizes it has no kernel for)"""
        key = torch.device(dev).index or 0
        if key not in self._handles:
            h = C.c_void_p()
            with torch.cuda.device(dev):
                native._check(_L().gdf_pixcls_create(self.C, self.M, self.h1, self.h2, self.K, *[C.c_void_p(t.data_ptr()) for t in self.folded],
                                                     C.byref(h)), "pixcls_create")
            self._handles[key] = h
        return self._handles[key]

    def __del__(self):
        for h in getattr(self, "_handles", {}).values():
            try:
                _lib.gdf_pixcls_destroy(h)
            except Exception:
                pass

    def _map(self, features, size):
        """-> (the logical (B, C, H, W) view, the shape of the label tensor)"""
        if features.dim() == 4:
            v, shape = features, (features.shape[0], features.shape[2], features.shape[3])
        elif features.dim() == 2:
            if size is None:
                raise ValueError("a (P, dim) matrix needs size=(H, W)")
            size = tuple(int(s) for s in size)
            if len(size) != 2 or size[0] * size[1] != features.shape[0]:
                raise ValueError("size is (H, W) with H * W = P")
            v, shape = features.t().unflatten(1, size).unsqueeze(0), size
        else:
            raise ValueError("features is a (B, C, H, W) map or a (P, dim) matrix")
        if v.shape[1] != self.C:
            raise ValueError(f"the features have {v.shape[1]} channels, the ensemble takes {self.C}")
        if v.shape[2] < 1 or v.shape[3] < 1:
            raise ValueError("H and W >= 1")
        return v, shape

    def _host(self, v):
        """the reference's torch chain in fp32 on a host map -> (labels, js, model labels, logits)"""
        from torch.distributions import Categorical
        B, _, H, W = v.shape
        x = v.permute(0, 2, 3, 1).reshape(-1, self.C).float()
        logits, ent, labs, mean = [], [], [], None
        for p in self.params:
            h = x
            for lin, bn in (("0", "2"), ("3", "5")):
                h = F.batch_norm(F.relu(F.linear(h, p[lin + ".weight"], p[lin + ".bias"])), p[bn + ".running_mean"], p[bn + ".running_var"],
                                 p[bn + ".weight"], p[bn + ".bias"], False, 0.0, PC_BN_EPS)
            preds = F.linear(h, p["6.weight"], p["6.bias"])
            logits.append(preds)
            ent.append(Categorical(logits=preds).entropy())
            sm = torch.softmax(preds, 1)
            mean = sm if mean is None else mean + sm
            labs.append(torch.max(torch.log_softmax(preds, 1), 1)[1])
        mean = mean / self.M
        js = Categorical(mean).entropy() - torch.mean(torch.stack(ent), 0)
        labs = torch.stack(labs)
        return (torch.mode(labs, 0)[0].reshape(B, H, W), js.reshape(B, H, W), labs.to(torch.uint8).reshape(self.M, B, H, W), torch.stack(logits))

    def predict_full(self, features, size=None):
        """-> (labels int64, top_k, js fp32, model_labels uint8 (M, ...), logits fp32 (M, P, K)), on the device of `features`.
        features: a (B, C, H, W) map, fp16 or fp32 with any strides -> labels and js (B, H, W), top_k (B,); or the reference's (P, dim) matrix with
        size = (H, W) -> labels and js of that size, top_k 0-d.  top_k is the reference's js.sort()[0][-int(P / 10):].mean() per image."""
        v, shape = self._map(features, size)
        B, _, H, W = v.shape
        if not v.is_cuda:
            labels, js, mlab, logits = self._host(v)
        else:
            dev = v.device
            v = v if v.dtype in (torch.float16, torch.float32) else v.float()
            with torch.cuda.device(dev):
                labels = torch.empty(B, H, W, dtype=torch.int64, device=dev)
                js = torch.empty(B, H, W, dtype=torch.float32, device=dev)
                mlab = torch.empty(self.M, B, H, W, dtype=torch.uint8, device=dev)
                logits = torch.empty(self.M, B * H * W, self.K, dtype=torch.float32, device=dev)
                if B > 0:
                    L, h = _L(), self._handle(dev)
                    nbytes = L.gdf_pixcls_workspace(h, B, H, W)
                    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
                    src = _agg_src(v)
                    native._check(L.gdf_pixcls_predict(h, C.addressof(src), B, C.c_void_p(labels.data_ptr()), C.c_void_p(js.data_ptr()),
                                                       C.c_void_p(mlab.data_ptr()), C.c_void_p(logits.data_ptr()), C.c_void_p(ws.data_ptr()), nbytes,
                                                       _stream(dev)), "pixcls_predict")
        P = H * W
        top_k = torch.stack([row.sort()[0][-int(P / 10):].mean() for row in js.reshape(B, P)]) if B > 0 else js.new_zeros(0)
        if features.dim() == 2:
            return labels.reshape(shape), top_k[0], js.reshape(shape), mlab.reshape(self.M, *shape), logits
        return labels, top_k, js, mlab, logits

    def predict(self, features, size=None):
        """-> (labels int64, top_k): see predict_full"""
        return self.predict_full(features, size)[:2]


_pc_cache = {}


def predict_labels(models, features, size):
    """The reference's function (scarce_segmentation/segmentation/pixel_classifier.py:70-107), same signature and return value: features a
    (P, dim) matrix (tensor or numpy array), size = (H, W) -> (labels int64 of that size on the CPU, 0-d top_k).  models: a
    PixelClassifierEnsemble, or the reference's list of modules; the ensemble built from a list is kept, with the list, under the list's identity
    (and rebuilt when its length changes).  Host features are moved to the GPU as the reference moves them, when there is one."""
    if isinstance(features, np.ndarray):
        features = torch.from_numpy(features)
    if isinstance(models, PixelClassifierEnsemble):
        ens = models
    else:
        hit = _pc_cache.get(id(models))
        if hit is None or hit[0] is not models or hit[1] != len(models):
            hit = (models, len(models), PixelClassifierEnsemble(models))
            _pc_cache[id(models)] = hit
        ens = hit[2]
    if not features.is_cuda and torch.cuda.is_available():
        features = features.cuda()
    labels, top_k = ens.predict(features, size)
    return labels.cpu(), top_k


def _head_conv(conv):
    """an nn.Conv2d -> (weight, bias); anything but the reference's 3 x 3, stride 1, padding 1 convolution is refused"""
    want = dict(kernel_size=(3, 3), stride=(1, 1), padding=(1, 1), dilation=(1, 1), groups=1)
    for k, v in want.items():
        got = getattr(conv, k)
        if (tuple(got) if isinstance(got, (tuple, list)) else got) != v:
            raise ValueError(f"AggregationHead: the convolution has {k} = {got}, the head is a 3 x 3 convolution with stride 1, padding 1, "
                             "no dilation and no groups")
    if getattr(conv, "padding_mode", "zeros") != "zeros":
        raise ValueError(f"AggregationHead: padding_mode = {conv.padding_mode!r}, the head pads with zeros")
    return conv.weight, conv.bias


def aggregation_head_params(source):
    """-> (weight (Cout, Cin, 3, 3), bias (Cout) or None) as fp32 CPU tensors.  source: the reference's AggregationNetwork (its `.out`), an
    nn.Conv2d, a weight tensor, a state dict holding `out.weight` (and `out.bias`), with or without the `module.` prefix, or the checkpoint
    task-corres.py saves ({"aggregation_network": state dict, ...})."""
    bias = None
    if isinstance(source, torch.nn.Conv2d):
        weight, bias = _head_conv(source)
    elif isinstance(source, torch.nn.Module):
        if not isinstance(getattr(source, "out", None), torch.nn.Conv2d):
            raise ValueError("AggregationHead: the module has no `out` convolution")
        weight, bias = _head_conv(source.out)
    elif isinstance(source, dict):
        sd = source.get("aggregation_network", source)
        if not isinstance(sd, dict):
            raise ValueError("AggregationHead: `aggregation_network` is not a state dict")
        sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}
        if "out.weight" not in sd:
            raise ValueError("AggregationHead: not an aggregation-network state dict: no out.weight")
        weight, bias = sd["out.weight"], sd.get("out.bias")
    elif torch.is_tensor(source):
        weight = source
    else:
        raise ValueError("AggregationHead: source is an aggregation network, an nn.Conv2d, a weight tensor, a state dict or a checkpoint")
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3) or weight.shape[0] < 1 or weight.shape[1] < 1:
        raise ValueError(f"AggregationHead: the weight is (Cout, Cin, 3, 3), not {tuple(weight.shape)}")
    weight = weight.detach().to("cpu", torch.float32).contiguous()
    if bias is not None:
        bias = bias.detach().to("cpu", torch.float32).contiguous()
        if tuple(bias.shape) != (weight.shape[0],):
            raise ValueError("AggregationHead: the bias is (Cout,)")
    return weight, bias


class AggregationHead:
    """The reference AggregationNetwork's output convolution (x.type(torch.float32); self.out(x)) as one device op: (B, Cin, H, W) or the
    reference's unbatched (Cin, H, W), fp16 or fp32 with any strides -> (B, Cout, H, W) / (Cout, H, W) fp32.  source: see aggregation_head_params."""

    def __init__(self, source):
        self.weight, self.bias = aggregation_head_params(source)
        self.Cout, self.Cin = int(self.weight.shape[0]), int(self.weight.shape[1])
        self._handles = {}

    def _handle(self, dev):
        """gdf_agghead of this head on `dev` (packed and uploaded on first use there)"""
        key = torch.device(dev).index or 0
        if key not in self._handles:
            h = C.c_void_p()
            with torch.cuda.device(dev):
                native._check(_L().gdf_agghead_create(self.Cin, self.Cout, C.c_void_p(self.weight.data_ptr()),
                                                      C.c_void_p(self.bias.data_ptr()) if self.bias is not None else None, C.byref(h)),
                              "agghead_create")
            self._handles[key] = h
        return self._handles[key]

    def __del__(self):
        for h in getattr(self, "_handles", {}).values():
            try:
                _lib.gdf_agghead_destroy(h)
            except Exception:
                pass

    def __call__(self, x):
        if x.dim() == 3:
            return self(x[None])[0]
        if x.dim() != 4 or x.shape[1] != self.Cin:
            raise ValueError(f"AggregationHead: x is (B, {self.Cin}, H, W) or ({self.Cin}, H, W), not {tuple(x.shape)}")
        if x.shape[2] < 1 or x.shape[3] < 1:
            raise ValueError("AggregationHead: H and W >= 1")
        if not x.is_cuda:
            return F.conv2d(x.float(), self.weight, self.bias, padding=1)
        dev = x.device
        x = x if x.dtype in (torch.float16, torch.float32) else x.float()
        B, _, H, W = x.shape
        with torch.cuda.device(dev):
            out = torch.empty(B, self.Cout, H, W, dtype=torch.float32, device=dev)
            if B > 0:
                src = _agg_src(x)
                native._check(_L().gdf_agghead_forward(self._handle(dev), C.addressof(src), B, C.c_void_p(out.data_ptr()), _stream(dev)),
                              "agghead_forward")
        return out


class _HeadConv(torch.autograd.Function):
    """gdf_agghead_forward on a TrainableAggregationHead's handle; the backward is gdf_agghead_wgrad and returns the gradient of the weight.  The map
    gets no gradient."""

    @staticmethod
    def forward(ctx, weight, x, handle):
        dev = x.device
        B, _, H, W = x.shape
        with torch.cuda.device(dev):
            out = torch.empty(B, weight.shape[0], H, W, dtype=torch.float32, device=dev)
            if B > 0:
                src = _agg_src(x)
                native._check(_L().gdf_agghead_forward(handle, C.addressof(src), B, C.c_void_p(out.data_ptr()), _stream(dev)), "agghead_forward")
        ctx.save_for_backward(x)
        ctx.wshape = tuple(weight.shape)
        return out

    @staticmethod
    def backward(ctx, grad):
        x, = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None
        dev = x.device
        B, Cin, H, W = x.shape
        Cout = ctx.wshape[0]
        with torch.cuda.device(dev):
            if B == 0:
                return torch.zeros(ctx.wshape, dtype=torch.float32, device=dev), None, None
            grad = grad.to(torch.float32).contiguous()
            dw = torch.empty(ctx.wshape, dtype=torch.float32, device=dev)
            L = _L()
            nbytes = L.gdf_agghead_wgrad_workspace(B, Cin, Cout, H, W)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            src = _agg_src(x)
            native._check(L.gdf_agghead_wgrad(C.addressof(src), B, C.c_void_p(grad.data_ptr()), Cout, C.c_void_p(dw.data_ptr()), 0,
                                              C.c_void_p(ws.data_ptr()), nbytes, _stream(dev)), "agghead_wgrad")
        return dw, None, None


class TrainableAggregationHead(torch.nn.Module):
    """The reference AggregationNetwork's trained part as a torch.nn.Module: `self.out = nn.Conv2d(Cin, Cout, 3, padding=1, bias=False)` holds the
    only parameter, so state_dict() has the reference's key `out.weight`, a task-corres.py checkpoint loads into it, and what it saves loads into
    the reference and into AggregationHead.  `logit_scale` is the reference's constant log(1 / 0.07), a plain tensor that is not trained.

    source: anything aggregation_head_params accepts (a source with a bias is a ValueError: the reference's head has none), or Cin with Cout for
    nn.Conv2d's own initialisation.

    head(x) on a device map ((B, Cin, H, W) or (Cin, H, W), fp16 or fp32, any strides; the module must be on that device) runs
    gdf_agghead_forward; its backward runs gdf_agghead_wgrad and gives out.weight its gradient.  x gets none: extraction is not differentiable on
    the native path, and a device x that requires a gradient is a ValueError.  The packed weights are refreshed lazily: when out.weight's
    version counter or storage differs from what was packed (an optimiser step, load_state_dict, copy_, .to(device)), the next forward runs
    gdf_agghead_update first; refresh() forces that.  Writes that bypass the version counter (through `.data`) need refresh().  One handle per
    device.  .eval() and .train() change nothing.  Host tensors take F.conv2d through self.out with torch's own autograd."""

    def __init__(self, source, Cout=None):
        super().__init__()
        if isinstance(source, int) and not isinstance(source, bool):
            if Cout is None or int(Cout) < 1 or source < 1:
                raise ValueError("TrainableAggregationHead(Cin, Cout): Cin and Cout >= 1")
            self.out = torch.nn.Conv2d(source, int(Cout), kernel_size=3, stride=1, padding=1, bias=False)
        else:
            if Cout is not None:
                raise ValueError("TrainableAggregationHead: Cout goes with Cin, not with a source of weights")
            weight, bias = aggregation_head_params(source)
            if bias is not None:
                raise ValueError("TrainableAggregationHead: the source has a bias; the reference's head has none")
            self.out = torch.nn.Conv2d(weight.shape[1], weight.shape[0], kernel_size=3, stride=1, padding=1, bias=False)
            with torch.no_grad():
                self.out.weight.copy_(weight)
        self.Cout, self.Cin = int(self.out.weight.shape[0]), int(self.out.weight.shape[1])
        self.logit_scale = torch.ones([]) * math.log(1 / 0.07)
        self._handles = {}                               # device index -> [gdf_agghead, packed version, packed data_ptr]

    def _handle(self, dev, force=False):
        """gdf_agghead of this head on `dev`, holding the weights as they are now"""
        w = self.out.weight
        if w.device != dev:
            raise ValueError(f"TrainableAggregationHead: the map is on {dev}, the module on {w.device}; move the module with .to(device)")
        if w.dtype != torch.float32 or not w.is_contiguous():
            raise ValueError("TrainableAggregationHead: out.weight is a contiguous fp32 tensor")
        key = dev.index or 0
        state = (w._version, w.data_ptr())
        with torch.cuda.device(dev):
            if key not in self._handles:
                h = C.c_void_p()
                native._check(_L().gdf_agghead_create_device(self.Cin, self.Cout, C.c_void_p(w.data_ptr()), None, _stream(dev), C.byref(h)),
                              "agghead_create_device")
                self._handles[key] = [h, state]
            elif force or self._handles[key][1] != state:
                native._check(_L().gdf_agghead_update(self._handles[key][0], C.c_void_p(w.data_ptr()), _stream(dev)), "agghead_update")
                self._handles[key][1] = state
        return self._handles[key][0]

    def refresh(self):
        """repack out.weight now (on the device the module is on), whatever the version counter says"""
        if self.out.weight.is_cuda:
            self._handle(self.out.weight.device, force=True)

    def __del__(self):
        for h in getattr(self, "_handles", {}).values():
            try:
                _lib.gdf_agghead_destroy(h[0])
            except Exception:
                pass

    def forward(self, x):
        if x.dim() == 3:
            return self(x[None])[0]
        if x.dim() != 4 or x.shape[1] != self.Cin:
            raise ValueError(f"TrainableAggregationHead: x is (B, {self.Cin}, H, W) or ({self.Cin}, H, W), not {tuple(x.shape)}")
        if x.shape[2] < 1 or x.shape[3] < 1:
            raise ValueError("TrainableAggregationHead: H and W >= 1")
        if not x.is_cuda:
            return self.out(x.float())
        if x.requires_grad:
            raise ValueError("TrainableAggregationHead: a device map that requires a gradient: the native head has no input gradient (extraction "
                             "is not differentiable on the native path); detach the map")
        x = x if x.dtype in (torch.float16, torch.float32) else x.float()
        return _HeadConv.apply(self.out.weight, x, self._handle(x.device))


PCAResult = collections.namedtuple("PCAResult", "mean components explained_variance explained_variance_ratio projection n_iter converged")
PCA_MAX_COMPONENTS, PCA_MAX_C = 8, 4096


def _pca_args(features, n_components, joint):
    if not torch.is_tensor(features) or features.dim() != 4:
        raise ValueError("features is a (B, C, H, W) tensor")
    B, C_, H, W = features.shape
    if min(C_, H, W) < 1:
        raise ValueError("C, H and W >= 1")
    k = int(n_components)
    n = (B if joint else 1) * H * W
    if not 1 <= k <= PCA_MAX_COMPONENTS:
        raise ValueError(f"1 <= n_components <= {PCA_MAX_COMPONENTS}")
    if k > min(C_, n - 1):
        raise ValueError(f"n_components = {k} exceeds min(C, samples - 1) = {min(C_, n - 1)}")
    return B, C_, H, W, k


def _pca_host(features, k, joint):
    """the reference's arithmetic in float64 on a host tensor: eigh of the centred covariance, the sign rule -> float64 tensors"""
    B, C_, H, W = features.shape
    x = features.double().permute(0, 2, 3, 1).reshape(B, H * W, C_)
    x = x.reshape(1, B * H * W, C_) if joint else x
    mean = x.mean(1, keepdim=True)
    xc = x - mean
    cov = xc.transpose(1, 2) @ xc / (x.shape[1] - 1)
    w, v = torch.linalg.eigh(cov)
    w, v = w.flip(-1)[:, :k], v.flip(-1)[:, :, :k].transpose(1, 2)                        # (G, k), (G, k, C), descending
    big = v.abs().argmax(-1, keepdim=True)
    sign = torch.sign(torch.gather(v, 2, big))
    v = v * torch.where(sign == 0, torch.ones_like(sign), sign)
    keep = (w > 2.0 ** -20 * w[:, :1]) & (w > 0)                                          # as the device op: such a direction is rounding, not data
    w, v = torch.where(keep, w, torch.zeros_like(w)), v * keep[:, :, None]
    proj = (xc @ v.transpose(1, 2)).reshape(B, H * W, k).permute(0, 2, 1).reshape(B, k, H, W)
    return mean[:, 0], v, w, cov.diagonal(dim1=1, dim2=2).sum(-1), proj


def pca(features, n_components=3, joint=False, max_iter=256, tol=2.0 ** -20):
    """features (B, C, H, W), fp16 or fp32 with any strides -> PCAResult(mean (G, C), components (G, k, C), explained_variance (G, k),
    explained_variance_ratio (G, k), projection (B, k, H, W), n_iter (G,) int32, converged (G,) bool), fp32 on the device of `features`.
    The reference's PCA(n_components).fit(f).transform(f) (feature_visualization.py:84-88) of every image's H W samples (G = B) or, joint, of the
    B H W samples of the batch (G = 1): per-channel mean, the leading eigenvectors of the sample covariance (divisor n - 1), each signed so that
    its entry of largest magnitude is positive.  Device tensors: gdf_op_pca (block subspace iteration, at most max_iter iterations, converged when
    every residual is at most tol x the largest eigenvalue; a run that does not converge warns once and returns its last estimate).  Host
    tensors: torch.linalg.eigh in float64 (n_iter 0, converged).  On either path a component whose eigenvalue is not above 2^-20 of the first is
    the zero vector with variance 0."""
    B, C_, H, W, k = _pca_args(features, n_components, joint)
    max_iter, tol = int(max_iter), float(tol)
    if not 1 <= max_iter <= 1024:
        raise ValueError("1 <= max_iter <= 1024")
    if not (tol >= 0 and math.isfinite(tol)):
        raise ValueError("tol is finite and not negative")
    G = 1 if joint else B
    if not features.is_cuda:
        mean, comp, var, total, proj = _pca_host(features, k, joint)
        return PCAResult(mean.float(), comp.float(), var.float(), (var / total[:, None]).float(), proj.float(),
                         torch.zeros(G, dtype=torch.int32), torch.ones(G, dtype=torch.bool))
    if C_ > PCA_MAX_C:
        raise ValueError(f"C = {C_}: the device PCA takes at most {PCA_MAX_C} channels")
    dev = features.device
    features = features if features.dtype in (torch.float16, torch.float32) else features.float()
    with torch.cuda.device(dev):
        f32 = dict(dtype=torch.float32, device=dev)
        mean, comp, var, total = torch.empty(G, C_, **f32), torch.empty(G, k, C_, **f32), torch.empty(G, k, **f32), torch.empty(G, **f32)
        proj = torch.empty(B, k, H, W, **f32)
        info = torch.zeros(G, 2, dtype=torch.int32, device=dev)
        if B > 0:
            L = _L()
            nbytes = L.gdf_op_pca_workspace(B, C_, H, W, k, int(bool(joint)))
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            src = _agg_src(features)
            native._check(L.gdf_op_pca(C.addressof(src), B, k, int(bool(joint)), max_iter, tol, C.c_void_p(mean.data_ptr()), C.c_void_p(comp.data_ptr()),
                                       C.c_void_p(var.data_ptr()), C.c_void_p(total.data_ptr()), C.c_void_p(proj.data_ptr()),
                                       C.c_void_p(info.data_ptr()), C.c_void_p(ws.data_ptr()), nbytes, _stream(dev)), "pca")
        converged = info[:, 1] != 0
        if B > 0 and not bool(converged.all()):
            warnings.warn("pca: the subspace iteration did not converge in %d iterations (tol %.3g); the last estimate is returned" % (max_iter, tol))
    return PCAResult(mean, comp, var, var / total[:, None], proj, info[:, 0].contiguous(), converged)


def pca_rgb(features, size=512, joint=False):
    """features (B, C, H, W) -> (B, OH, OW, 3) uint8 on the device of `features`: the reference's plot_pca picture (feature_visualization.py:84-94)
    of every image: the projection onto the three leading principal components, (p - min) / (max - min) per component over the image (over the
    batch when joint, which also shares one PCA), (. * 255) truncated, and Pillow's nearest resize of the short side to `size` (the long side to
    int(size * long / short)); size=None keeps the grid.  A component of zero range is 0.  Device tensors: gdf_op_pca and gdf_op_pca_rgb;
    host tensors: float64 torch."""
    B, C_, H, W, _ = _pca_args(features, 3, joint)
    if size is None:
        OH, OW = H, W
    else:
        size = int(size)
        if size < 1:
            raise ValueError("size >= 1")
        OH, OW = (size, int(size * W / H)) if H <= W else (int(size * H / W), size)
    if not features.is_cuda:
        proj = _pca_host(features, 3, joint)[4]
        dims = (0, 2, 3) if joint else (2, 3)
        lo, hi = proj.amin(dims, keepdim=True), proj.amax(dims, keepdim=True)
        n = torch.where(hi > lo, (proj - lo) / (hi - lo), torch.zeros_like(proj))
        u8 = (n * 255).to(torch.uint8)
        iy = torch.clamp(((2 * torch.arange(OH) + 1) * H) // (2 * OH), max=H - 1)
        ix = torch.clamp(((2 * torch.arange(OW) + 1) * W) // (2 * OW), max=W - 1)
        return u8[:, :, iy][:, :, :, ix].permute(0, 2, 3, 1).contiguous()
    proj = pca(features, 3, joint).projection
    dev = features.device
    with torch.cuda.device(dev):
        out = torch.empty(B, OH, OW, 3, dtype=torch.uint8, device=dev)
        if B > 0:
            native._check(_L().gdf_op_pca_rgb(C.c_void_p(proj.data_ptr()), B, H, W, int(bool(joint)), C.c_void_p(out.data_ptr()), OH, OW,
                                              _stream(dev)), "pca_rgb")
    return out


def rescale_points(points, old_shape, new_shape):
    """The reference's helper (correspondence/correspondence/correspondence_utils.py:53-59), same signature: points (N, 2) in (y, x) order, the
    shapes in (w, h) order -> the points scaled by (new h / old h, new w / old w)."""
    return np.multiply(points, np.array([new_shape[1] / old_shape[1], new_shape[0] / old_shape[0]]))


def compute_pck(predicted_points, target_points, load_size, pck_threshold=0.1, target_bounding_box=None):
    """The reference's helper (correspondence_utils.py:160-167), same signature -> (distances (N,), correct (N,) bool, their fraction): a point is
    correct when its Euclidean distance to the target is at most pck_threshold times the longer side of the image (load_size) or, when given, of
    the target's bounding box (left, top, right, bottom)."""
    distances = np.linalg.norm(predicted_points - target_points, axis=-1)
    if target_bounding_box is None:
        side = max(load_size)
    else:
        left, top, right, bottom = target_bounding_box
        side = max(right - left, bottom - top)
    pck = distances <= pck_threshold * side
    return distances, pck, pck.sum() / len(pck)


def avg_pool(feat, r):
    """(B, C, H, W) fp16 -> (B, C, H // r, W // r) fp16 (channels-last storage for device tensors): F.adaptive_avg_pool2d to that size.
    Where r divides H and W that is the mean over r x r windows; otherwise output row o averages the source rows
    [floor(o H / OH), ceil((o + 1) H / OH)) (columns likewise), on the device and on the host alike."""
    if r <= 1:
        return feat
    tgt = (feat.shape[2] // r, feat.shape[3] // r)
    b, c, h, w = feat.shape
    if not feat.is_cuda or feat.dtype != torch.float16 or feat.stride(1) != 1 or c % 8 or any(s % 8 for s in feat.stride()[0:1] + feat.stride()[2:]):
        if feat.is_cuda and feat.dtype == torch.float16 and c % 8 == 0:
            return avg_pool(feat.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2), r)   # make it channels-last, then the kernel
        return F.adaptive_avg_pool2d(feat.float(), tgt).to(torch.float16)
    dev = feat.device
    with torch.cuda.device(dev):
        out = torch.empty(b, tgt[0], tgt[1], c, dtype=torch.float16, device=dev)
        native._check(_L().gdf_op_avg_pool(C.c_void_p(feat.data_ptr()), feat.stride(0), feat.stride(2), feat.stride(3), b, c, h, w, r,
                                           C.c_void_p(out.data_ptr()), _stream(dev)), "avg_pool")
    return out.permute(0, 3, 1, 2)


def aggregate_maps(maps_by_category, out_size):
    """{category: [(B, heads, Q, K) fp16 maps in execution order]} -> (B, sum K, out_size, out_size) fp16: head mean, mean over
    the maps of one (category, query-grid size) group, nearest resize, concat in category then first-seen-size order."""
    groups = []
    for cat, maps in maps_by_category.items():
        by_size = {}
        for m in maps:
            by_size.setdefault(int(math.sqrt(m.shape[2])), []).append(m)
        groups.extend(by_size.items())
    first = groups[0][1][0]
    if not first.is_cuda:
        outs = []
        for size, lst in groups:
            acc = [m.float().mean(1).to(torch.float16).float() for m in lst]
            b, q, k = acc[0].shape
            avg = torch.stack(acc).mean(0).reshape(b, size, q // size, k).permute(0, 3, 1, 2)
            outs.append(F.interpolate(avg, size=(out_size, out_size)).to(torch.float16))
        return torch.cat(outs, dim=-3)
    dev = first.device
    B = first.shape[0]
    ktot = sum(lst[0].shape[3] for _, lst in groups)
    with torch.cuda.device(dev):
        out = torch.empty(B, ktot, out_size, out_size, dtype=torch.float16, device=dev)
        off = 0
        for size, lst in groups:
            assert len(lst) <= 32, "more than 32 maps in one (category, size) group"     # SDXL up_* @ 32x32: 3 x 10 blocks = 30; PixArt: 28
            lst = [m.contiguous() for m in lst]
            _, heads, Q, K = lst[0].shape
            mean = torch.empty(B, Q, K, dtype=torch.float32, device=dev)
            ptrs = (C.c_void_p * len(lst))(*[m.data_ptr() for m in lst])
            native._check(_L().gdf_op_maps_mean(ptrs, len(lst), B, heads, Q, K, C.c_void_p(mean.data_ptr()), _stream(dev)), "maps_mean")
            # (B, Q, K) == channels-last image of the logical (B, C = K, size, Q / size) tensor
            wq = Q // size
            native._check(_L().gdf_op_resize_concat(C.c_void_p(mean.data_ptr()), 1, Q * K, 1, wq * K, K, B, K, size, wq,
                                                    C.c_void_p(out.data_ptr()), ktot, off, out_size, _stream(dev)), "resize_concat")
            off += K
            del mean
    return out
