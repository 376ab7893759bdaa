#!/usr/bin/env python3
"""Training the correspondence evaluator's head on the device (correspondence/task-corres.py train(), `--algorithm conv`): the weight gradient of
the fp32 3 x 3 output convolution, the device repack of updated weights and a whole training step, on (1, Cin, 128, 128) fp16 aggregated maps for
the reference's three heads (SD1.5 alone 3520 -> 3520, SDXL alone 3840 -> 3840, both models 7360 -> 3680), on the same seeded device tensors:

  a_wgrad        gdf_agghead_wgrad alone (pre-passes and kernel of csrc/aggwgrad.hip), dW and workspace allocated once
  b_update       gdf_agghead_update alone (csrc/agghead.hip), with GB/s against its byte floor: 36 Cin Cout bytes read, the packed image written
  c_native_step  a full native step: TrainableAggregationHead on both maps, clip_loss, backward, AdamW.step(), the refresh of the packed weights
  d_torch_wgrad  torch's fp32 device weight gradient of the same tensors: torch.nn.grad.conv2d_weight(x.float(), ..., padding=1)
  e_torch_step   the step without this kernel: nn.Conv2d in fp32 on both maps -> the device clip_loss -> backward -> AdamW.step()

    python tools/bench_agg_head_train.py [--out profiles/agg_head_train.txt] [--rounds 5] [--calls 2] [--heads 0,1,2]

Time: device events around windows of `--calls` back-to-back calls; the variants alternate inside every one of `--rounds` rounds, after a warm-up
of every variant on every shape.  Per variant the median window with the fastest and the slowest is reported per call.  TFLOP/s of a: both fp16 MFMA
passes, 2 x 2 x 9 Cin Cout H W operations, over the median time of the call; TFLOP/s of d: the fp32 gradient's 2 x 9 Cin Cout H W over its median.
Error: the worst relative L2 error per input channel against a float64 CPU oracle on a slice (16 output channels x 8 input channels, all
pixels), for a and for d.  Nothing is asserted.  Without a GPU the tool fails."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "generic-diffusion-feature_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402

HEADS = [("SD1.5 alone 3520 -> 3520", 3520, 3520), ("SDXL alone 3840 -> 3840", 3840, 3840), ("both models 7360 -> 3680", 7360, 3680)]
HW, NPTS = 128, 64
vp = ctypes.c_void_p


def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def channel_error(got, want):
    d = (got.double() - want).pow(2).sum((0, 2, 3)).sqrt()
    return float((d / want.pow(2).sum((0, 2, 3)).sqrt()).max())


def bench(name, Cin, Cout, rounds, calls):
    from components import native, postproc
    dev = torch.device("cuda", 0)
    gd = torch.Generator(device="cuda").manual_seed(Cin + Cout)
    cs = 0.25 * 16.0 ** torch.rand(Cin, generator=gd, device="cuda")
    f1 = (torch.randn(1, Cin, HW, HW, generator=gd, device="cuda") * cs[None, :, None, None]).half()
    f2 = (torch.randn(1, Cin, HW, HW, generator=gd, device="cuda") * cs[None, :, None, None]).half()
    g = torch.randn(1, Cout, HW, HW, generator=gd, device="cuda") * 1e-5
    src = torch.randperm(HW * HW, generator=gd, device="cuda")[:NPTS][None]
    tgt = torch.randperm(HW * HW, generator=gd, device="cuda")[:NPTS][None]
    head = postproc.TrainableAggregationHead(Cin, Cout).to(dev)
    conv = torch.nn.Conv2d(Cin, Cout, 3, padding=1, bias=False).to(dev)
    with torch.no_grad():
        conv.weight.copy_(head.out.weight)
    opt_c = torch.optim.AdamW(head.parameters(), lr=5e-4, weight_decay=0.01)
    opt_e = torch.optim.AdamW(conv.parameters(), lr=5e-4, weight_decay=0.01)
    L = postproc._L()
    h = head._handle(dev)
    dw = torch.empty(Cout, Cin, 3, 3, dtype=torch.float32, device=dev)
    nbytes = L.gdf_agghead_wgrad_workspace(1, Cin, Cout, HW, HW)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    stream = lambda: vp(torch.cuda.current_stream().cuda_stream)     # noqa: E731

    def a():
        s = postproc._agg_src(f1)
        native._check(L.gdf_agghead_wgrad(ctypes.addressof(s), 1, vp(g.data_ptr()), Cout, vp(dw.data_ptr()), 0, vp(ws.data_ptr()), nbytes, stream()),
                      "agghead_wgrad")
        return dw

    def b():
        native._check(L.gdf_agghead_update(h, vp(head.out.weight.data_ptr()), stream()), "agghead_update")

    def c():
        opt_c.zero_grad()
        postproc.clip_loss(head(f1), head(f2), src, tgt)[0].backward()
        opt_c.step()
        head._handle(dev)                                            # the refresh the next forward would run

    def d():
        return torch.nn.grad.conv2d_weight(f1.float(), (Cout, Cin, 3, 3), g, padding=1)

    def e():
        opt_e.zero_grad()
        postproc.clip_loss(conv(f1.float()), conv(f2.float()), src, tgt)[0].backward()
        opt_e.step()

    variants = {"a_wgrad": a, "b_update": b, "c_native_step": c, "d_torch_wgrad": d, "e_torch_step": e}
    rows, cols = list(range(8)) + list(range(Cout - 8, Cout)), list(range(4)) + list(range(Cin - 4, Cin))
    want = torch.nn.grad.conv2d_weight(f1[:, cols].cpu().double(), (16, 8, 3, 3), g[:, rows].cpu().double(), padding=1)
    err = {"a_wgrad": channel_error(a()[rows][:, cols].cpu(), want), "d_torch_wgrad": channel_error(d()[rows][:, cols].cpu(), want)}
    for fn in variants.values():                                     # warm-up of every variant on this shape
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            ms[k].append(window(fn, calls))
    flop32 = 2.0 * 9 * Cin * Cout * HW * HW
    packed = ((Cout + 31) // 32) * ((Cin + 31) // 32) * 36864
    res = dict(head=name, Cin=Cin, Cout=Cout, grid=[HW, HW], points=NPTS, dW_mb=round(36 * Cin * Cout / 1e6, 1), packed_weights_mb=round(packed / 1e6, 1),
               wgrad_workspace_mb=round(nbytes / 1e6, 1), fp32_tflop=round(flop32 / 1e12, 3), mfma_tflop_both_passes=round(2 * flop32 / 1e12, 3),
               rounds=rounds, calls_per_window=calls)
    for k, t in ms.items():
        t = sorted(t)
        med = t[len(t) // 2]
        res[k] = dict(ms_median=round(med, 3), ms_fastest=round(t[0], 3), ms_slowest=round(t[-1], 3))
        if k == "a_wgrad":
            res[k]["mfma_tflop_per_s_both_passes"] = round(2 * flop32 / (med * 1e-3) / 1e12, 1)
        if k == "d_torch_wgrad":
            res[k]["fp32_tflop_per_s"] = round(flop32 / (med * 1e-3) / 1e12, 1)
        if k == "b_update":
            res[k]["gb_per_s_against_byte_floor"] = round((36.0 * Cin * Cout + packed) / (med * 1e-3) / 1e9, 1)
        if k in err:
            res[k]["worst_channel_error_vs_fp64_on_slice"] = float("%.3e" % err[k])
    res["speedup_a_over_d"] = round(res["d_torch_wgrad"]["ms_median"] / res["a_wgrad"]["ms_median"], 2)
    res["speedup_c_over_e"] = round(res["e_torch_step"]["ms_median"] / res["c_native_step"]["ms_median"], 2)
    res["a_faster_than_d_beyond_spread"] = bool(res["a_wgrad"]["ms_slowest"] < res["d_torch_wgrad"]["ms_fastest"])
    res["c_faster_than_e_beyond_spread"] = bool(res["c_native_step"]["ms_slowest"] < res["e_torch_step"]["ms_fastest"])
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "agg_head_train.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--heads", default="0,1,2", help="indices into the three heads")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_agg_head_train.py measures on the GPU; none is visible")
    heads = [HEADS[int(i)] for i in args.heads.split(",")]
    lines = ["# tools/bench_agg_head_train.py on %s: training the aggregation network's 3 x 3 head on (1, Cin, %d, %d) fp16 maps; ms per call (median of "
             "%d windows of %d calls, device events)" % (torch.cuda.get_device_name(0), HW, HW, args.rounds, args.calls),
             "# a = gdf_agghead_wgrad, b = gdf_agghead_update, c = a native step (2 forwards, clip_loss, backward, AdamW, refresh), d = torch's fp32 "
             "weight gradient, e = the step through nn.Conv2d in fp32; a's TFLOP/s = both fp16 MFMA passes / median time, d's = the fp32 operations / "
             "median time"]
    for name, Cin, Cout in heads:
        r = bench(name, Cin, Cout, args.rounds, args.calls)
        print(json.dumps(r), flush=True)
        lines.append(json.dumps(r))
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
