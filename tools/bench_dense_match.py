#!/usr/bin/env python3
"""Dense matching on the device: best pixel and cosine in both directions between two seeded (1, C, 128, 128) maps (P = 16384 pixels a side),
one image pair per call, for C = 3520 (SD1.5 practical set) and C = 3840 (SDXL practical set), fp16 and fp32 maps, NCHW and channels-last, on the
same device tensors:

  a     gdf_op_dense_match, workspace and outputs allocated once: the five launches of csrc/densematch.hip alone (two packs, match, two folds)
  a_py  postproc.dense_match (a + the workspace and result tensors from torch's allocator and the int64 casts, the call a user makes)
  b     the reference's torch chain (correspondence_utils.py batch_cosine_sim, then max over both axes) on the same tensors: flatten, two
        normalisations, ONE matmul to the (1, P, P) fp32 matrix, two max; an fp16 map is cast to fp32 first, as the reference's head output is fp32

    python tools/bench_dense_match.py [--out profiles/dense_match.txt] [--rounds 7] [--calls 5]

Time: device events around windows of `--calls` back-to-back calls; the variants alternate inside every one of `--rounds` rounds, after a warm-up
of every variant on every shape.  Per variant the median window and the spread = (slowest - fastest window) / median are reported per call.
Rates of a: TFLOP/s = 2 P^2 C (the useful multiply-adds of the cosine matrix, whatever the number of MFMA passes) over the median time of the
WHOLE call; share_of_f16_mfma_peak = that over the 2.5 PFLOP/s dense fp16 peak.  Nothing is asserted; the number of rows and columns on which a and
b name the same index is reported (white noise at these C has many near-ties, and b's fp32 matmul rounds differently).  Without a GPU the tool
fails."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "generic-diffusion-feature_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402

CONFIGS = [("SD1.5 practical, C=3520", 3520), ("SDXL practical, C=3840", 3840)]
HW = 128
F16_MFMA_PEAK_TFLOPS = 2500.0


def torch_chain(f1, f2):
    """the reference's batch_cosine_sim and the two max of find_best_buddies_correspondences on device tensors"""
    a = f1.float().flatten(2).permute(0, 2, 1)
    b = f2.float().flatten(2).permute(0, 2, 1)
    a = a / torch.linalg.norm(a, dim=-1)[:, :, None]
    b = b / torch.linalg.norm(b, dim=-1)[:, :, None]
    sims = torch.matmul(a, b.permute(0, 2, 1))
    s1, n1 = sims.max(dim=-1)
    s2, n2 = sims.max(dim=-2)
    return n1, s1, n2, s2


def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def bench(name, C_, f32, chlast, rounds, calls):
    from components import native, postproc
    g = torch.Generator(device="cuda").manual_seed(C_)
    dt = torch.float32 if f32 else torch.float16
    f1 = torch.randn(1, C_, HW, HW, generator=g, device="cuda", dtype=torch.float32).to(dt)
    f2 = torch.randn(1, C_, HW, HW, generator=g, device="cuda", dtype=torch.float32).to(dt)
    if chlast:
        f1, f2 = (v.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2) for v in (f1, f2))
    P = HW * HW
    L = postproc._L()
    nbytes = L.gdf_op_dense_match_workspace(1, C_, P, P, int(f32), int(f32))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    nn12, nn21 = torch.empty(1, P, dtype=torch.int32, device="cuda"), torch.empty(1, P, dtype=torch.int32, device="cuda")
    sim12, sim21 = torch.empty(1, P, device="cuda"), torch.empty(1, P, device="cuda")
    s1, s2 = postproc._agg_src(f1), postproc._agg_src(f2)
    vp = ctypes.c_void_p

    def op():
        st = vp(torch.cuda.current_stream().cuda_stream)
        native._check(L.gdf_op_dense_match(ctypes.addressof(s1), ctypes.addressof(s2), 1, vp(nn12.data_ptr()), vp(sim12.data_ptr()),
                                           vp(nn21.data_ptr()), vp(sim21.data_ptr()), vp(ws.data_ptr()), nbytes, st), "dense_match")

    variants = {"a_dense_match_op": op, "a_py_postproc_dense_match": lambda: postproc.dense_match(f1, f2), "b_torch_chain": lambda: torch_chain(f1, f2)}
    op()
    want = torch_chain(f1, f2)
    torch.cuda.synchronize()
    agree = [int((nn12.long() == want[0]).sum()), int((nn21.long() == want[2]).sum())]
    worst = max(float((sim12 - want[1]).abs().max()), float((sim21 - want[3]).abs().max()))
    del want
    for fn in variants.values():                                 # warm-up of every variant on this shape
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            ms[k].append(window(fn, calls))
    flop = 2.0 * P * P * C_
    res = dict(config=name, C=C_, dtype="fp32" if f32 else "fp16", layout="channels_last" if chlast else "nchw", pixels=[P, P], tflop=round(flop / 1e12, 3),
               workspace_mb=round(nbytes / 1e6, 1), rounds=rounds, calls_per_window=calls, rows_cols_equal_a_vs_b=agree,
               worst_score_difference_a_vs_b=worst)
    for k, t in ms.items():
        t = sorted(t)
        med = t[len(t) // 2]
        res[k] = dict(ms_median=round(med, 4), ms_fastest=round(t[0], 4), ms_slowest=round(t[-1], 4), spread=round((t[-1] - t[0]) / med, 4))
        if k == "a_dense_match_op":
            tf = flop / (med * 1e-3) / 1e12
            res[k].update(tflop_per_s=round(tf, 1), share_of_f16_mfma_peak=round(tf / F16_MFMA_PEAK_TFLOPS, 4))
    A, Bv = res["a_py_postproc_dense_match"], res["b_torch_chain"]
    res["a_py_faster_than_b_beyond_spread"] = bool(A["ms_slowest"] < Bv["ms_fastest"])
    res["speedup_a_py_over_b"] = round(Bv["ms_median"] / A["ms_median"], 2)
    res["speedup_a_op_over_b"] = round(Bv["ms_median"] / res["a_dense_match_op"]["ms_median"], 2)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_match.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_dense_match.py measures on the GPU; none is visible")
    lines = ["# tools/bench_dense_match.py on %s: two (1, C, %d, %d) maps, both directions; ms per call (median of %d windows of %d calls, device "
             "events)" % (torch.cuda.get_device_name(0), HW, HW, args.rounds, args.calls),
             "# a = gdf_op_dense_match, a_py = postproc.dense_match, b = the reference's torch chain (fp32 matmul to the P x P matrix, two max); "
             "TFLOP/s = 2 P^2 C / median time of the whole call; fp16 MFMA peak taken as %.0f TFLOP/s" % F16_MFMA_PEAK_TFLOPS]
    for name, C_ in CONFIGS:
        for f32 in (False, True):
            for chlast in (False, True):
                r = bench(name, C_, f32, chlast, args.rounds, args.calls)
                print(json.dumps(r), flush=True)
                lines.append(json.dumps(r))
                torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
