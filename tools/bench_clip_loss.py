#!/usr/bin/env python3
"""The correspondence evaluator's loss on the device: compute_clip_loss (correspondence/task-corres.py:70-80) on two (1, C, 128, 128) hyperfeature
maps with N = 20 annotated points, forward and forward + backward, for the reference's three widths (C = 3520, 3840, 3680), as fp32 NCHW maps
(what the head writes) and as fp16 NCHW maps (what aggregate writes), on the same seeded device tensors:

  a_fwd     gdf_op_clip_loss, workspace allocated once: the forward kernels of csrc/cliploss.hip alone
  a_fb      gdf_op_clip_loss + gdf_op_clip_loss_backward, gradients allocated once
  a_py_fwd  postproc.clip_loss under no_grad (a_fwd + the workspace and result tensors from torch's allocator)
  a_py_fb   postproc.clip_loss(...).sum().backward() on leaf maps: the call a training step makes
  b_fwd     the reference's chain under no_grad: batch_cosine_sim twice (two P x P matrices), the N rows, cross_entropy; an fp16 map is cast first
  b_fb      the same with torch's autograd backward to both maps

    python tools/bench_clip_loss.py [--out profiles/clip_loss.txt] [--rounds 5] [--calls 10] [--calls-b 2]

Time: device events around windows of back-to-back calls (`--calls` for a, `--calls-b` for b); the variants alternate inside every one of
`--rounds` rounds, after a warm-up of every variant on every shape.  Per variant the median window and the spread = (slowest - fastest window) /
median are reported per call.  GB/s of a: the floor traffic — one read of each map in the forward, one more read and one fp32 write per map in the
backward — over the median time.  Both losses are printed.  Nothing is asserted.  Without a GPU the tool fails."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "generic-diffusion-feature_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

WIDTHS = [3520, 3840, 3680]
HW, N, SCALE = 128, 20, 1 / 0.07


def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def reference_chain(f1, f2, src, tgt):
    """the reference's arithmetic on device tensors: flatten, normalise, both similarity matrices, the rows, cross_entropy"""
    k1, k2 = (v.float().view(1, v.shape[1], -1).permute(0, 2, 1) for v in (f1, f2))
    k1 = k1 / torch.linalg.norm(k1, dim=-1)[:, :, None]
    k2 = k2 / torch.linalg.norm(k2, dim=-1)[:, :, None]
    l1 = SCALE * torch.matmul(k1, k2.permute(0, 2, 1))
    l2 = SCALE * torch.matmul(k2, k1.permute(0, 2, 1))
    return (F.cross_entropy(l1[0, src], tgt) + F.cross_entropy(l2[0, tgt], src)) / 2


def bench(C_, f32, rounds, calls, calls_b):
    from components import native, postproc
    gd = torch.Generator(device="cuda").manual_seed(C_ + int(f32))
    cs = 0.25 * 16.0 ** torch.rand(C_, generator=gd, device="cuda")
    f1, f2 = ((torch.randn(1, C_, HW, HW, generator=gd, device="cuda") * cs[None, :, None, None]) for _ in range(2))
    if not f32:
        f1, f2 = f1.half(), f2.half()
    g = torch.Generator().manual_seed(C_)
    src, tgt = (torch.randint(0, HW * HW, (1, N), generator=g).cuda() for _ in range(2))
    L, vp = postproc._L(), ctypes.c_void_p
    nbytes = L.gdf_op_clip_loss_workspace(1, N, C_, HW * HW, HW * HW)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    loss, ones = torch.empty(1, device="cuda"), torch.ones(1, device="cuda")
    g1, g2 = torch.empty(1, C_, HW, HW, device="cuda"), torch.empty(1, C_, HW, HW, device="cuda")
    s1, s2 = postproc._agg_src(f1), postproc._agg_src(f2)

    def fwd():
        native._check(L.gdf_op_clip_loss(ctypes.addressof(s1), ctypes.addressof(s2), 1, vp(src.data_ptr()), vp(tgt.data_ptr()), N, SCALE,
                                         vp(loss.data_ptr()), None, vp(ws.data_ptr()), nbytes, vp(torch.cuda.current_stream().cuda_stream)), "clip_loss")

    def fb():
        fwd()
        native._check(L.gdf_op_clip_loss_backward(ctypes.addressof(s1), ctypes.addressof(s2), 1, vp(src.data_ptr()), vp(tgt.data_ptr()), N, SCALE,
                                                  vp(ones.data_ptr()), vp(g1.data_ptr()), vp(g2.data_ptr()), vp(ws.data_ptr()), nbytes,
                                                  vp(torch.cuda.current_stream().cuda_stream)), "clip_loss_backward")

    def py_fwd():
        with torch.no_grad():
            return postproc.clip_loss(f1, f2, src, tgt)

    def py_fb():
        a, b = f1.detach().requires_grad_(True), f2.detach().requires_grad_(True)
        postproc.clip_loss(a, b, src, tgt).sum().backward()
        return a.grad

    def b_fwd():
        with torch.no_grad():
            return reference_chain(f1, f2, src[0], tgt[0])

    def b_fb():
        a, b = f1.detach().requires_grad_(True), f2.detach().requires_grad_(True)
        reference_chain(a, b, src[0], tgt[0]).backward()
        return a.grad

    variants = {"a_fwd_clip_loss_op": (fwd, calls), "a_fb_clip_loss_op_forward_backward": (fb, calls), "a_py_fwd_postproc_clip_loss": (py_fwd, calls),
                "a_py_fb_postproc_clip_loss_backward": (py_fb, calls), "b_fwd_torch_chain": (b_fwd, calls_b), "b_fb_torch_chain_autograd": (b_fb, calls_b)}
    fb()
    ga = g1.clone()
    a32 = f1.float().requires_grad_(True)                             # (an fp16 leaf would get an fp16 gradient, most of it below fp16's range)
    reference_chain(a32, f2, src[0], tgt[0]).backward()
    gb = a32.grad
    losses = dict(a=float(loss), b=float(b_fwd()))
    grad_rel = float((ga.double() - gb.double()).norm() / gb.double().norm())
    del ga, gb
    for fn, _ in variants.values():                                   # warm-up of every variant on this shape
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(rounds):
        for k, (fn, n) in variants.items():
            ms[k].append(window(fn, n))
    elt = 4 if f32 else 2
    fwd_bytes = 2.0 * C_ * HW * HW * elt
    fb_bytes = 2 * fwd_bytes + 2.0 * C_ * HW * HW * 4
    res = dict(C=C_, grid=[HW, HW], N=N, maps="fp32 NCHW" if f32 else "fp16 NCHW", workspace_mb=round(nbytes / 1e6, 2),
               floor_mb_forward=round(fwd_bytes / 1e6, 1), floor_mb_forward_backward=round(fb_bytes / 1e6, 1), rounds=rounds, calls_per_window_a=calls,
               calls_per_window_b=calls_b, loss_a=losses["a"], loss_b=losses["b"], grad_f1_rel_l2_a_against_b=float("%.3e" % grad_rel))
    for k, t in ms.items():
        t = sorted(t)
        med = t[len(t) // 2]
        res[k] = dict(ms_median=round(med, 4), ms_fastest=round(t[0], 4), ms_slowest=round(t[-1], 4), spread=round((t[-1] - t[0]) / med, 4))
        if k.startswith("a_"):
            res[k]["floor_gb_per_s"] = round((fb_bytes if "_fb_" in k else fwd_bytes) / (med * 1e-3) / 1e9, 1)
    for kind in ("fwd", "fb"):
        a = next(v for k, v in res.items() if k.startswith("a_py_%s_" % kind))
        b = next(v for k, v in res.items() if k.startswith("b_%s_" % kind))
        res["speedup_a_py_%s_over_b" % kind] = round(b["ms_median"] / a["ms_median"], 1)
        res["a_py_%s_faster_than_b_beyond_spread" % kind] = bool(a["ms_slowest"] < b["ms_fastest"])
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_loss.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--calls-b", type=int, default=2)
    ap.add_argument("--widths", default=",".join(map(str, WIDTHS)))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_clip_loss.py measures on the GPU; none is visible")
    lines = ["# tools/bench_clip_loss.py on %s: compute_clip_loss on two (1, C, %d, %d) maps, N = %d; ms per call (median of %d windows, device events)"
             % (torch.cuda.get_device_name(0), HW, HW, N, args.rounds),
             "# a = gdf_op_clip_loss (+ _backward), a_py = postproc.clip_loss (+ autograd), b = the reference's torch chain (two P x P matrices, "
             "cross_entropy, autograd) on the same device tensors; a's GB/s = floor traffic / median time"]
    for C_ in (int(v) for v in args.widths.split(",")):
        for f32 in (True, False):
            r = bench(C_, f32, args.rounds, args.calls, args.calls_b)
            print(json.dumps(r), flush=True)
            lines.append(json.dumps(r))
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
