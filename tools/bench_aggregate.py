#!/usr/bin/env python3
"""The evaluators' output stage on the device: bilinear resize of every hooked layer to 128 x 128 + channel concat, three ways on the same
device tensors (seeded, in the hooks' own channels-last layout), for the SDXL practical set at B = 16 and the SD1.5 practical set at B = 32.

  a  postproc.aggregate(feats, 128, 'bilinear')            aggregate_kernel (csrc/post.hip), one launch
  b  torch.cat([F.interpolate(f, (128, 128), mode='bilinear') for f in feats], 1)      the reference's formulation in torch
  c  postproc.resize_concat(feats, 128)                    the nearest-neighbour kernel of --aggregate_output, which writes the same bytes

    python tools/bench_aggregate.py [--out profiles/aggregate_bilinear.txt] [--rounds 9] [--calls 50]

Time: device events around windows of `--calls` back-to-back calls; the three variants alternate inside every one of `--rounds` rounds, after a
warm-up of every variant on every shape.  Per variant the median window, and the spread = (slowest - fastest window) / median, are reported per
call.  Bytes are computed from the shapes, each counted once: a and c read every source and write the result; b also writes and re-reads one
resized temporary per layer.  GB/s = those bytes over the median time — a whole-call rate, set beside the 5.1 TB/s residual_add_kernel reaches.
Nothing is asserted except that a and b agree to fp16 rounding; without a GPU the tool fails."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "generic-diffusion-feature_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

RESIDUAL_ADD_TBPS = 5.1
# (C, H = W) of the practical layer sets (configs/config_xl_practical.json at 1024^2, configs/config_15_practical.json at 512^2), hook order
CONFIGS = [("SDXL practical, 1024^2, B=16", 16, [(1280, 32), (1280, 32), (640, 64), (640, 64)]),
           ("SD1.5 practical, 512^2, B=32", 32, [(1280, 16), (1280, 16), (640, 32), (320, 64)])]
SIZE = 128


def hooks(B, layers, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return [torch.randn(B, hw, hw, c, generator=g, device="cuda", dtype=torch.float16).permute(0, 3, 1, 2) for c, hw in layers]


def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def bench(name, B, layers, rounds, calls):
    from components.postproc import aggregate, resize_concat
    feats = hooks(B, layers, seed=B)
    variants = {"a_aggregate_kernel_bilinear": lambda: aggregate(feats, SIZE, "bilinear"),
                "b_torch_interpolate_cat_bilinear": lambda: torch.cat([F.interpolate(f, (SIZE, SIZE), mode="bilinear") for f in feats], 1),
                "c_resize_concat_kernel_nearest": lambda: resize_concat(feats, SIZE)}
    src = sum(f.numel() * 2 for f in feats)
    out = B * sum(c for c, _ in layers) * SIZE * SIZE * 2
    nbytes = {"a_aggregate_kernel_bilinear": src + out, "b_torch_interpolate_cat_bilinear": src + 3 * out, "c_resize_concat_kernel_nearest": src + out}
    a, b = variants["a_aggregate_kernel_bilinear"](), variants["b_torch_interpolate_cat_bilinear"]()
    torch.cuda.synchronize()
    worst = max(float((a[:, i:i + 64].float() - b[:, i:i + 64].float()).abs().max()) for i in range(0, a.shape[1], 64))
    assert a.shape == b.shape and worst < 2e-2, worst            # |randn| < 6: an fp16 ulp or two between two fp32 blends in different operation order
    del a, b
    for fn in variants.values():                                 # warm-up of every variant on this shape
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            ms[k].append(window(fn, calls))
    res = dict(config=name, batch=B, layers=[dict(C=c, H=hw, W=hw) for c, hw in layers], out_shape=[B, sum(c for c, _ in layers), SIZE, SIZE],
               source_gb=round(src / 1e9, 4), result_gb=round(out / 1e9, 4), rounds=rounds, calls_per_window=calls, max_abs_diff_a_vs_b=worst)
    for k, t in ms.items():
        t = sorted(t)
        med = t[len(t) // 2]
        res[k] = dict(ms_median=round(med, 4), ms_fastest=round(t[0], 4), ms_slowest=round(t[-1], 4), spread=round((t[-1] - t[0]) / med, 4),
                      gb_moved=round(nbytes[k] / 1e9, 4), gb_per_s=round(nbytes[k] / (med * 1e-3) / 1e9, 1))
    A, Bv, Cv = (res[k] for k in variants)
    res["a_faster_than_b_beyond_spread"] = bool(A["ms_slowest"] < Bv["ms_fastest"])
    res["speedup_a_over_b"] = round(Bv["ms_median"] / A["ms_median"], 3)
    res["time_a_over_c"] = round(A["ms_median"] / Cv["ms_median"], 3)
    res["a_share_of_residual_add_rate"] = round(A["gb_per_s"] / (RESIDUAL_ADD_TBPS * 1e3), 3)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aggregate_bilinear.txt"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_aggregate.py measures on the GPU; none is visible")
    lines = ["# tools/bench_aggregate.py on %s: bilinear resize to 128^2 + concat; ms per call (median of %d windows of %d calls, device events)"
             % (torch.cuda.get_device_name(0), args.rounds, args.calls),
             "# a = aggregate_kernel, b = torch F.interpolate + cat, c = resize_concat_kernel (nearest); GB/s = bytes from the shapes / median time; "
             "residual_add_kernel reaches %.1f TB/s" % RESIDUAL_ADD_TBPS]
    for name, B, layers in CONFIGS:
        r = bench(name, B, layers, args.rounds, args.calls)
        print(json.dumps(r), flush=True)
        lines.append(json.dumps(r))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
