#!/usr/bin/env python3
"""The correspondence evaluator's trained head on the device: the fp32 3 x 3 output convolution of the reference's AggregationNetwork
(correspondence/correspondence/aggregation_network.py:20-22, 97-100) on one (1, Cin, 128, 128) fp16 aggregated map, for the reference's three
heads (SD1.5 alone 3520 -> 3520, SDXL alone 3840 -> 3840, both models 7360 -> 3680), on the same seeded device tensors:

  a_nchw  gdf_agghead_forward on the NCHW map (what aggregate returns), output allocated once: the kernel of csrc/agghead.hip alone
  a_cl    the same on a channels-last map (16-byte loads along C)
  a_py    AggregationHead.__call__ on the NCHW map (a_nchw + the output tensor from torch's allocator, the call a user makes)
  b_nchw  F.conv2d(x.float(), w, padding=1) on the NCHW map: the reference's arithmetic (the cast is part of it, as in the reference)
  b_cl    the same on the channels-last map

    python tools/bench_agg_head.py [--out profiles/agg_head.txt] [--rounds 5] [--calls 3] [--heads 0,1,2]

Time: device events around windows of `--calls` back-to-back calls; the variants alternate inside every one of `--rounds` rounds, after a warm-up
of every variant on every shape.  Per variant the median window and the spread = (slowest - fastest window) / median are reported per call.
TFLOP/s of a: both fp16 MFMA passes (x W_hi, x W_lo), 2 x 2 x 9 Cin Cout H W operations, over the median time of the call; TFLOP/s of b: the
fp32 convolution's 2 x 9 Cin Cout H W over its median.  Error: the worst relative L2 error per block of 16 consecutive pixels against a float64
CPU oracle on a slice (16 output channels, the 8 x 32 pixels of the top-left corner, padding included), for a_nchw and for b_nchw.
Nothing is asserted.  Without a GPU the tool fails."""
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

HEADS = [("SD1.5 alone 3520 -> 3520", 3520, 3520), ("SDXL alone 3840 -> 3840", 3840, 3840), ("both models 7360 -> 3680", 7360, 3680)]
HW = 128
SY, SX = 8, 32                                                       # the slice the oracle covers


def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def setup(Cin, Cout):
    from components import native, postproc
    g = torch.Generator().manual_seed(Cin + Cout)
    scale = 0.25 * 16.0 ** torch.rand(Cout, generator=g)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5 * scale[:, None, None, None]).contiguous()
    head = postproc.AggregationHead(w)
    gd = torch.Generator(device="cuda").manual_seed(Cin)
    cs = 0.25 * 16.0 ** torch.rand(Cin, generator=gd, device="cuda")
    f = (torch.randn(1, Cin, HW, HW, generator=gd, device="cuda") * cs[None, :, None, None]).half()
    L, h = postproc._L(), head._handle(f.device)
    out = torch.empty(1, Cout, HW, HW, dtype=torch.float32, device="cuda")
    vp = ctypes.c_void_p

    def op(x):                                                       # (holds `head`: the handle lives as long as its head)
        assert head._handle(f.device) is h
        src = postproc._agg_src(x)
        native._check(L.gdf_agghead_forward(h, ctypes.addressof(src), 1, vp(out.data_ptr()), vp(torch.cuda.current_stream().cuda_stream)),
                      "agghead_forward")
        return out
    return w, head, f, op


def block_error(got, want):
    """(Cs, SY, SX) against float64: worst relative L2 error per block of 16 consecutive pixels over the Cs channels"""
    d = (got.double() - want).permute(1, 2, 0).reshape(-1, 16 * got.shape[0]).norm(dim=1)
    n = want.permute(1, 2, 0).reshape(-1, 16 * got.shape[0]).norm(dim=1)
    return float((d / n).max())


def bench(name, Cin, Cout, rounds, calls):
    w, head, f, op = setup(Cin, Cout)
    fcl = f.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    wd = w.cuda()
    variants = {"a_nchw_agghead_op": lambda: op(f), "a_cl_agghead_op_channels_last": lambda: op(fcl), "a_py_aggregation_head_call": lambda: head(f),
                "b_nchw_torch_conv2d_fp32": lambda: F.conv2d(f.float(), wd, padding=1), "b_cl_torch_conv2d_fp32_channels_last": lambda: F.conv2d(fcl.float(), wd, padding=1)}
    rows = list(range(8)) + list(range(Cout - 8, Cout))
    want = F.conv2d(f[:, :, :SY + 1, :SX + 1].cpu().double(), w[rows].double(), padding=1)[0, :, :SY, :SX]
    err = {"a_nchw_agghead_op": block_error(op(f)[0, rows, :SY, :SX].cpu(), want),
           "b_nchw_torch_conv2d_fp32": block_error(variants["b_nchw_torch_conv2d_fp32"]()[0, rows, :SY, :SX].cpu(), want)}
    for fn in variants.values():                                      # warm-up of every variant on this shape
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            ms[k].append(window(fn, calls))
    flop32 = 2.0 * 9 * Cin * Cout * HW * HW
    res = dict(head=name, Cin=Cin, Cout=Cout, grid=[HW, HW], map_mb=round(Cin * HW * HW * 2 / 1e6, 1), packed_weights_mb=round(
        ((Cout + 31) // 32) * ((Cin + 31) // 32) * 36864 / 1e6, 1), fp32_tflop=round(flop32 / 1e12, 3), mfma_tflop_both_passes=round(2 * flop32 / 1e12, 3),
        rounds=rounds, calls_per_window=calls)
    for k, t in ms.items():
        t = sorted(t)
        med = t[len(t) // 2]
        res[k] = dict(ms_median=round(med, 3), ms_fastest=round(t[0], 3), ms_slowest=round(t[-1], 3), spread=round((t[-1] - t[0]) / med, 4))
        if k.startswith("a_"):
            res[k]["mfma_tflop_per_s_both_passes"] = round(2 * flop32 / (med * 1e-3) / 1e12, 1)
        else:
            res[k]["fp32_tflop_per_s"] = round(flop32 / (med * 1e-3) / 1e12, 1)
        if k in err:
            res[k]["worst_block_error_vs_fp64_on_slice"] = float("%.3e" % err[k])
    best_b = min(res["b_nchw_torch_conv2d_fp32"]["ms_fastest"], res["b_cl_torch_conv2d_fp32_channels_last"]["ms_fastest"])
    res["a_py_faster_than_b_beyond_spread"] = bool(res["a_py_aggregation_head_call"]["ms_slowest"] < best_b)
    res["speedup_a_py_over_b_nchw"] = round(res["b_nchw_torch_conv2d_fp32"]["ms_median"] / res["a_py_aggregation_head_call"]["ms_median"], 2)
    res["speedup_a_op_over_b_nchw"] = round(res["b_nchw_torch_conv2d_fp32"]["ms_median"] / res["a_nchw_agghead_op"]["ms_median"], 2)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "agg_head.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--heads", default="0,1,2", help="indices into the three heads")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_agg_head.py measures on the GPU; none is visible")
    heads = [HEADS[int(i)] for i in args.heads.split(",")]
    lines = ["# tools/bench_agg_head.py on %s: the aggregation network's fp32 3 x 3 output convolution on one (1, Cin, %d, %d) fp16 map; ms per call "
             "(median of %d windows of %d calls, device events)" % (torch.cuda.get_device_name(0), HW, HW, args.rounds, args.calls),
             "# a = gdf_agghead_forward (NCHW / channels-last map), a_py = AggregationHead.__call__, b = F.conv2d(x.float(), w, padding=1) on the same "
             "device tensors; a's TFLOP/s = both fp16 MFMA passes / median time, b's = the fp32 convolution's operations / median time"]
    for name, Cin, Cout in heads:
        r = bench(name, Cin, Cout, args.rounds, args.calls)
        print(json.dumps(r), flush=True)
        lines.append(json.dumps(r))
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
