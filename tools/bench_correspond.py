#!/usr/bin/env python3
"""The evaluators' second step on the device: nearest neighbours of N = 20 source points between two aggregated (1, C, 128, 128) fp16 maps at
the load size 512 x 512, one image pair per call, for C = 3520 (SD1.5 practical set) and C = 3840 (SDXL practical set), on the same seeded
device tensors:

  a     gdf_op_nn_match on an NCHW target (what aggregate returns), workspace allocated once: the five kernels of csrc/corres.hip alone
  a_cl  the same on a channels-last target (lanes along C)
  a_py  postproc.nn_match (a + the workspace and result tensors from torch's allocator, the call a user makes)
  b     the reference's torch chain (correspondence_utils.py find_nn_source_correspondences) on the same tensors: two F.interpolate to 512^2,
        gather, two normalisations, matmul, argmax

    python tools/bench_correspond.py [--out profiles/correspond.txt] [--rounds 9] [--calls 20]

Time: device events around windows of `--calls` back-to-back calls; the variants alternate inside every one of `--rounds` rounds, after a warm-up
of every variant on every shape.  Per variant the median window and the spread = (slowest - fastest window) / median are reported per call.
Rates of a / a_cl: GB/s = ONE read of the target (C * 128 * 128 * 2 bytes) over the median time; GFLOP/s = the algorithm's fp32 operations,
(2 N + 10) per target element in the coarse pass + (8 N + 40) per fine pixel, over the same time: whole-call rates of five dependent launches.
Nothing is asserted; the number of points on which a and b agree is reported (b rounds its maps to fp16).  Without a GPU the tool fails."""
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

CONFIGS = [("SD1.5 practical, C=3520", 3520), ("SDXL practical, C=3840", 3840)]
HW, LOAD, N = 128, 512, 20
RESIDUAL_ADD_TBPS = 5.1


def torch_chain(f1, f2, idx):
    """the reference's find_nn_source_correspondences on device tensors (idx: the flat source indices, on the device)"""
    a = F.interpolate(f1, (LOAD, LOAD), mode="bilinear").flatten(2).permute(0, 2, 1)
    b = F.interpolate(f2, (LOAD, LOAD), mode="bilinear").flatten(2).permute(0, 2, 1)
    a = a[:, idx, :]
    a = a / torch.linalg.norm(a, dim=-1)[:, :, None]
    b = b / torch.linalg.norm(b, dim=-1)[:, :, None]
    best = torch.matmul(a, b.permute(0, 2, 1)).argmax(dim=-1)
    return torch.stack([best // LOAD, best % LOAD], dim=-1)


def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def bench(name, C_, rounds, calls):
    from components import native, postproc
    g = torch.Generator(device="cuda").manual_seed(C_)
    f1 = torch.randn(1, C_, HW, HW, generator=g, device="cuda", dtype=torch.float16)
    f2 = torch.randn(1, C_, HW, HW, generator=g, device="cuda", dtype=torch.float16)
    f2cl = f2.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    pts = torch.rand(1, N, 2, generator=g, device="cuda") * (LOAD - 1)
    idx = (LOAD * torch.round(pts[0, :, 0]) + torch.round(pts[0, :, 1])).long()
    L = postproc._L()
    nbytes = L.gdf_op_nn_match_workspace(1, N, C_, HW, HW)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    yx = torch.empty(1, N, 2, dtype=torch.int64, device="cuda")
    sc = torch.empty(1, N, dtype=torch.float32, device="cuda")
    s1 = postproc._agg_src(f1)
    vp = ctypes.c_void_p

    def op(target):
        s2 = postproc._agg_src(target)
        st = vp(torch.cuda.current_stream().cuda_stream)
        native._check(L.gdf_op_nn_match(ctypes.addressof(s1), ctypes.addressof(s2), 1, vp(pts.data_ptr()), N, LOAD, LOAD, vp(yx.data_ptr()),
                                        vp(sc.data_ptr()), vp(ws.data_ptr()), nbytes, st), "nn_match")

    variants = {"a_nn_match_op_nchw": lambda: op(f2), "a_cl_nn_match_op_channels_last": lambda: op(f2cl),
                "a_py_postproc_nn_match": lambda: postproc.nn_match(f1, f2, pts, (LOAD, LOAD)), "b_torch_chain": lambda: torch_chain(f1, f2, idx)}
    op(f2)
    got = yx.clone()
    want = torch_chain(f1, f2, idx)
    torch.cuda.synchronize()
    agree = int((got == want).all(-1).sum())
    del want
    for fn in variants.values():                                 # warm-up of every variant on this shape
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            ms[k].append(window(fn, calls))
    target_bytes = C_ * HW * HW * 2
    flop = (2 * N + 10) * C_ * HW * HW + (8 * N + 40) * LOAD * LOAD
    res = dict(config=name, C=C_, grid=[HW, HW], load_size=[LOAD, LOAD], N=N, target_mb=round(target_bytes / 1e6, 2), gflop=round(flop / 1e9, 3),
               workspace_mb=round(nbytes / 1e6, 2), rounds=rounds, calls_per_window=calls, points_equal_a_vs_b=agree)
    for k, t in ms.items():
        t = sorted(t)
        med = t[len(t) // 2]
        res[k] = dict(ms_median=round(med, 4), ms_fastest=round(t[0], 4), ms_slowest=round(t[-1], 4), spread=round((t[-1] - t[0]) / med, 4))
        if k.startswith("a_") and "py" not in k:
            res[k].update(target_gb_per_s=round(target_bytes / (med * 1e-3) / 1e9, 1), fp32_gflop_per_s=round(flop / (med * 1e-3) / 1e9, 1),
                          share_of_residual_add_rate=round(target_bytes / (med * 1e-3) / 1e12 / RESIDUAL_ADD_TBPS, 3))
    A, Bv = res["a_py_postproc_nn_match"], res["b_torch_chain"]
    res["a_py_faster_than_b_beyond_spread"] = bool(A["ms_slowest"] < Bv["ms_fastest"])
    res["speedup_a_py_over_b"] = round(Bv["ms_median"] / A["ms_median"], 2)
    res["speedup_a_op_over_b"] = round(Bv["ms_median"] / res["a_nn_match_op_nchw"]["ms_median"], 2)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "correspond.txt"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_correspond.py measures on the GPU; none is visible")
    lines = ["# tools/bench_correspond.py on %s: N = %d source points, two (1, C, %d, %d) fp16 maps, load size %d^2; ms per call (median of %d windows "
             "of %d calls, device events)" % (torch.cuda.get_device_name(0), N, HW, HW, LOAD, args.rounds, args.calls),
             "# a = gdf_op_nn_match (NCHW target), a_cl = channels-last target, a_py = postproc.nn_match, b = the reference's torch chain; GB/s = one "
             "read of the target / median time; residual_add_kernel reaches %.1f TB/s" % RESIDUAL_ADD_TBPS]
    for name, C_ in CONFIGS:
        r = bench(name, C_, args.rounds, args.calls)
        print(json.dumps(r), flush=True)
        lines.append(json.dumps(r))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
