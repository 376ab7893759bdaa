#!/usr/bin/env python3
"""The PCA picture of a feature map on the device (feature_visualization.py:84-101, plot_pca) for the shapes a user draws: an SDXL hook (C = 1280
on 32^2, 64^2, 128^2, channels-last fp16), the attention maps (C = 77 on 64^2, NCHW fp16) and an aggregated map (C = 3520 on 128^2, NCHW fp16), on
the same seeded device tensors (a planted spectrum 1, 0.5, 0.25, then 0.03 through random mixing, per-channel offsets: the fastest-converging
kind of input), and the C = 1280, 64^2 hook once more with a slow spectrum (1, 0.8, 0.6, then 0.55 * 0.97^i: a flat tail):

  a_pca_rgb     postproc.pca_rgb(x, 512): gdf_op_pca + gdf_op_pca_rgb and torch's allocations
  a_op          gdf_op_pca + gdf_op_pca_rgb, outputs and workspace allocated once
  a_cov_1it     gdf_op_pca with max_iter = 1 and no projection: mean, covariance, one iteration, the final Rayleigh quotient
  a_no_proj     gdf_op_pca with the default tol and max_iter, no projection  (a_no_proj - a_cov_1it: the remaining iterations)
  a_pca         gdf_op_pca with the projection                                (a_pca - a_no_proj: the projection)
  a_pca_exact   gdf_op_pca with max_iter = the iterations the default call used: the same work without the enqueued launches that return at
                once  (a_pca - a_pca_exact: those 2 * (256 - iterations) launches)
  a_rgb         gdf_op_pca_rgb alone (min / max, colour, nearest resize to 512)
  b_torch       the torch device chain: centre in fp32, x.T @ x / (n - 1), torch.linalg.eigh, the sign rule, project, colour, index-resize
  c_sklearn     the reference's chain on the host (sklearn PCA(3).fit().transform(), numpy colouring, Pillow's nearest resize), where sklearn
                imports: one call, wall clock, the host copy of the map not counted

    python tools/bench_pca.py [--out profiles/pca_visualize.txt] [--rounds 5] [--calls 5] [--calls-b 2]

Time: device events around windows of back-to-back calls; the variants alternate inside every one of `--rounds` rounds, after a warm-up of every
variant on every shape.  Per variant the median window and the spread = (slowest - fastest window) / median are reported per call.  The iteration
count and the largest difference of the two pictures are printed.  Nothing is asserted.  Without a GPU the tool fails."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "generic-diffusion-feature_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402

SHAPES = [(1280, 32, "cl", "planted"), (1280, 64, "cl", "planted"), (1280, 128, "cl", "planted"), (77, 64, "nchw", "planted"),
          (3520, 128, "nchw", "planted"), (1280, 64, "cl", "slow")]
SIZE = 512


def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def make_map(C_, S, layout, kind):
    gd = torch.Generator(device="cuda").manual_seed(C_ * 1000 + S)
    if kind == "slow":
        spec = 0.55 * 0.97 ** (torch.arange(C_, device="cuda", dtype=torch.float32) - 3)
        spec[:3] = torch.tensor([1.0, 0.8, 0.6], device="cuda")
    else:
        spec = torch.full((C_,), 0.03, device="cuda")
        spec[:3] = torch.tensor([1.0, 0.5, 0.25], device="cuda")
    mix, _ = torch.linalg.qr(torch.randn(C_, C_, generator=gd, device="cuda"))
    z = torch.randn(S * S, C_, generator=gd, device="cuda") * spec.sqrt()
    x = z @ mix.T + torch.randn(C_, generator=gd, device="cuda")
    x = x.T.reshape(1, C_, S, S).half().contiguous()
    return x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2) if layout == "cl" else x


def torch_chain(x, size):
    B, C_, H, W = x.shape
    f = x[0].float().reshape(C_, -1).T
    fc = f - f.mean(0, keepdim=True)
    cov = fc.T @ fc / (f.shape[0] - 1)
    w, v = torch.linalg.eigh(cov)
    v = v[:, -3:].flip(1).T
    big = v.abs().argmax(1, keepdim=True)
    v = v * torch.sign(torch.gather(v, 1, big))
    p = (fc @ v.T).T.reshape(3, H, W)
    lo, hi = p.amin((1, 2), keepdim=True), p.amax((1, 2), keepdim=True)
    u8 = ((p - lo) / (hi - lo) * 255).to(torch.uint8)
    iy = torch.clamp(((2 * torch.arange(size, device=x.device) + 1) * H) // (2 * size), max=H - 1)
    ix = torch.clamp(((2 * torch.arange(size, device=x.device) + 1) * W) // (2 * size), max=W - 1)
    return u8[:, iy][:, :, ix].permute(1, 2, 0).contiguous()


def sklearn_chain(f, S):
    from PIL import Image
    from sklearn.decomposition import PCA
    import numpy as np
    t0 = time.perf_counter()
    p = PCA(n_components=3)
    img = p.fit(f).transform(f).reshape(S, S, 3)
    img = (img - img.min(axis=(0, 1))) / (img.max(axis=(0, 1)) - img.min(axis=(0, 1)))
    Image.fromarray((img * 255).astype(np.uint8)).resize((SIZE, SIZE), Image.NEAREST)
    return (time.perf_counter() - t0) * 1e3


def bench(C_, S, layout, kind, rounds, calls, calls_b):
    from components import native, postproc
    x = make_map(C_, S, layout, kind)
    L, vp = postproc._L(), ctypes.c_void_p
    nbytes = L.gdf_op_pca_workspace(1, C_, S, S, 3, 0)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    f32 = dict(dtype=torch.float32, device="cuda")
    mean, comp, var, tot, proj = torch.empty(C_, **f32), torch.empty(3, C_, **f32), torch.empty(3, **f32), torch.empty(1, **f32), torch.empty(3, S, S, **f32)
    info = torch.zeros(2, dtype=torch.int32, device="cuda")
    out = torch.empty(SIZE, SIZE, 3, dtype=torch.uint8, device="cuda")
    src = postproc._agg_src(x)

    def op(max_iter=256, projection=True):
        native._check(L.gdf_op_pca(ctypes.addressof(src), 1, 3, 0, max_iter, 2.0 ** -20, vp(mean.data_ptr()), vp(comp.data_ptr()), vp(var.data_ptr()),
                                   vp(tot.data_ptr()), vp(proj.data_ptr()) if projection else None, vp(info.data_ptr()), vp(ws.data_ptr()), nbytes,
                                   vp(torch.cuda.current_stream().cuda_stream)), "pca")

    def rgb():
        native._check(L.gdf_op_pca_rgb(vp(proj.data_ptr()), 1, S, S, 0, vp(out.data_ptr()), SIZE, SIZE, vp(torch.cuda.current_stream().cuda_stream)),
                      "pca_rgb")

    def both():
        op()
        rgb()

    variants = {"a_pca_rgb_postproc": (lambda: postproc.pca_rgb(x, SIZE), calls), "a_op_pca_and_rgb": (both, calls),
                "a_cov_1it_no_projection": (lambda: op(1, False), calls), "a_no_proj": (lambda: op(256, False), calls), "a_pca": (op, calls),
                "a_rgb": (rgb, calls), "b_torch_chain": (lambda: torch_chain(x, SIZE), calls_b)}
    both()
    torch.cuda.synchronize()
    n_iter, converged = int(info[0]), int(info[1])
    variants["a_pca_exact_iterations"] = (lambda: op(max(n_iter, 1)), calls)
    diff = (out.int() - torch_chain(x, SIZE).int()).abs()
    for fn, _ in variants.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(rounds):
        for k, (fn, n) in variants.items():
            ms[k].append(window(fn, n))
    res = dict(C=C_, grid=[S, S], spectrum=kind, layout="fp16 channels-last" if layout == "cl" else "fp16 NCHW", size=SIZE, workspace_mb=round(nbytes / 1e6, 2),
               map_mb=round(x.numel() * 2 / 1e6, 2), iterations=n_iter, converged=converged, rounds=rounds, calls_per_window_a=calls,
               calls_per_window_b=calls_b, picture_values_differing_from_torch_chain=int((diff > 0).sum()), picture_max_difference=int(diff.max()))
    for k, t in ms.items():
        t = sorted(t)
        med = t[len(t) // 2]
        res[k] = dict(ms_median=round(med, 4), ms_fastest=round(t[0], 4), ms_slowest=round(t[-1], 4), spread=round((t[-1] - t[0]) / med, 4))
    a, b = res["a_pca_rgb_postproc"], res["b_torch_chain"]
    res["speedup_a_pca_rgb_over_b_torch_chain"] = round(b["ms_median"] / a["ms_median"], 2)
    res["a_faster_than_b_beyond_spread"] = bool(a["ms_slowest"] < b["ms_fastest"])
    res["derived_ms"] = dict(iterations_after_the_first=round(res["a_no_proj"]["ms_median"] - res["a_cov_1it_no_projection"]["ms_median"], 4),
                             projection=round(res["a_pca"]["ms_median"] - res["a_no_proj"]["ms_median"], 4),
                             launches_that_return_at_once=round(res["a_pca"]["ms_median"] - res["a_pca_exact_iterations"]["ms_median"], 4),
                             per_iteration_run=round((res["a_pca_exact_iterations"]["ms_median"] - res["a_pca"]["ms_median"]
                                                      + res["a_no_proj"]["ms_median"] - res["a_cov_1it_no_projection"]["ms_median"])
                                                     / max(n_iter - 1, 1), 4))
    try:
        f = x[0].float().reshape(C_, -1).T.cpu().numpy()
        res["c_sklearn_host_ms_one_call"] = round(sklearn_chain(f, S), 1)
        res["speedup_a_pca_rgb_over_c_sklearn"] = round(res["c_sklearn_host_ms_one_call"] / a["ms_median"], 1)
    except ImportError:
        res["c_sklearn_host_ms_one_call"] = None
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pca_visualize.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--calls-b", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_pca.py measures on the GPU; none is visible")
    lines = ["# tools/bench_pca.py on %s: the PCA picture of one (1, C, S, S) map at size %d; ms per call (median of %d windows, device events)"
             % (torch.cuda.get_device_name(0), SIZE, args.rounds),
             "# a = gdf_op_pca + gdf_op_pca_rgb (a_pca_rgb_postproc: through postproc.pca_rgb), b = the torch device chain (centre, x.T @ x, "
             "torch.linalg.eigh, project, colour), c = scikit-learn on the host (one call, wall clock)"]
    for C_, S, layout, kind in SHAPES:
        r = bench(C_, S, layout, kind, args.rounds, args.calls, args.calls_b)
        print(json.dumps(r), flush=True)
        lines.append(json.dumps(r))
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
