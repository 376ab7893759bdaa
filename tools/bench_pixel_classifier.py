#!/usr/bin/env python3
"""The label-scarce segmentation evaluator's second step on the device: an ensemble of M = 10 pixel classifiers over one aggregated
(1, C, 256, 256) fp16 map, for C = 3520 (the SDXL practical set) and C = 8448 (the reference's `dim`), with K = 19 classes (the small nets,
dim -> 128 -> 32 -> K) and K = 34 (the large nets, dim -> 256 -> 128 -> K), on the same seeded device tensors:

  a     gdf_pixcls_predict on the NCHW map (what aggregate returns), workspace allocated once: the two kernels of csrc/pixcls.hip alone
  a_cl  the same on a channels-last map (16-byte loads along C)
  a_py  PixelClassifierEnsemble.predict (a + the result and workspace tensors from torch's allocator and top_k, the call a user makes)
  b     the reference's predict_labels chain (scarce_segmentation/segmentation/pixel_classifier.py:70-107) on the same device tensors: the
        (P, dim) view of the map turned to fp32, every model's nn.Sequential in fp32, Categorical, softmax, a `.cpu()` per model, torch.mode

    python tools/bench_pixel_classifier.py [--out profiles/pixel_classifier.txt] [--rounds 5] [--calls 4]
    python tools/bench_pixel_classifier.py --launches 2 --config 1      # two launches of `a` of one configuration, for a counter run

Time: device events around windows of `--calls` back-to-back calls (b ends in its own host copies); the variants alternate inside every one of
`--rounds` rounds, after a warm-up of every variant on every shape.  Per variant the median window and the spread = (slowest - fastest window) /
median are reported per call.  TFLOP/s of a / a_cl: the MFMA passes of layer 1 alone, 2 passes x 2 P C M h1 operations for an fp16 map, over the
median time of the whole call (both kernels, layers 2 and 3 and the vote included): a whole-call rate, not the main loop's.
Nothing is asserted; the share of pixels on which a and b give the same label is reported.  Without a GPU the tool fails."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "generic-diffusion-feature_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
from torch.distributions import Categorical  # noqa: E402

CONFIGS = [("SDXL practical C=3520, K=19 small nets", 3520, 19), ("SDXL practical C=3520, K=34 large nets", 3520, 34),
           ("reference dim C=8448, K=19 small nets", 8448, 19), ("reference dim C=8448, K=34 large nets", 8448, 34)]
HW, M = 256, 10


def make_models(C_, K, seed):
    """M seeded networks of the reference's two shapes, eval mode, with BatchNorm statistics away from their initial values"""
    torch.manual_seed(seed)
    h1, h2 = (128, 32) if K < 30 else (256, 128)
    out = []
    for _ in range(M):
        net = nn.Sequential(nn.Linear(C_, h1), nn.ReLU(), nn.BatchNorm1d(h1), nn.Linear(h1, h2), nn.ReLU(), nn.BatchNorm1d(h2), nn.Linear(h2, K))
        with torch.no_grad():
            for m in net:
                if isinstance(m, nn.Linear):
                    m.weight.copy_(1.5 * torch.randn_like(m.weight) / m.in_features ** 0.5)
                    m.bias.copy_(0.3 * torch.randn_like(m.bias))
                if isinstance(m, nn.BatchNorm1d):
                    m.weight.copy_(1 + 0.2 * torch.randn_like(m.weight))
                    m.bias.copy_(0.2 * torch.randn_like(m.bias))
                    m.running_mean.copy_(0.4 + 0.1 * torch.randn_like(m.running_mean))
                    m.running_var.copy_(0.3 + 0.2 * torch.rand_like(m.running_var))
        holder = nn.Module()
        holder.layers = net
        out.append(holder.eval())
    return out


def torch_chain(models, features, size):
    """the reference's predict_labels on device modules and a device (P, dim) matrix"""
    mean_seg, all_entropy, seg_mode_ensemble = None, [], []
    with torch.no_grad():
        x = features.float()                                          # the reference's X is torch.float
        for net in models:
            preds = net.layers(x)
            all_entropy.append(Categorical(logits=preds).entropy())
            sm = torch.softmax(preds, 1)
            mean_seg = sm if mean_seg is None else mean_seg + sm
            seg_mode_ensemble.append(torch.max(torch.log_softmax(preds, 1), 1)[1].reshape(*size).cpu().detach())
        mean_seg = mean_seg / len(models)
        js = Categorical(mean_seg).entropy() - torch.mean(torch.stack(all_entropy), 0)
        top_k = js.sort()[0][-int(js.shape[0] / 10):].mean()
        return torch.mode(torch.stack(seg_mode_ensemble, dim=-1), 2)[0], top_k


def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def setup(C_, K):
    from components import native, postproc
    models = make_models(C_, K, C_ + K)
    ens = postproc.PixelClassifierEnsemble(models)
    g = torch.Generator(device="cuda").manual_seed(C_)
    scale = 0.25 * 16.0 ** torch.rand(C_, generator=g, device="cuda")
    f = (torch.randn(1, C_, HW, HW, generator=g, device="cuda") * scale[None, :, None, None]).half()
    L, h = postproc._L(), ens._handle(f.device)
    nbytes = L.gdf_pixcls_workspace(h, 1, HW, HW)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    labels = torch.empty(1, HW, HW, dtype=torch.int64, device="cuda")
    js = torch.empty(1, HW, HW, dtype=torch.float32, device="cuda")
    vp = ctypes.c_void_p

    def op(x):                                                       # (holds `ens`: the handle lives as long as its ensemble)
        assert ens._handle(f.device) is h
        src = postproc._agg_src(x)
        st = vp(torch.cuda.current_stream().cuda_stream)
        native._check(L.gdf_pixcls_predict(h, ctypes.addressof(src), 1, vp(labels.data_ptr()), vp(js.data_ptr()), None, None, vp(ws.data_ptr()),
                                           nbytes, st), "pixcls_predict")
    return models, ens, f, op, labels, nbytes


def bench(name, C_, K, rounds, calls):
    models, ens, f, op, labels, nbytes = setup(C_, K)
    fcl = f.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    dev_models = [m.cuda() for m in models]
    x = f[0].view(C_, -1).permute(1, 0)                               # the (P, dim) view of task-pixel.py:100
    variants = {"a_pixcls_op_nchw": lambda: op(f), "a_cl_pixcls_op_channels_last": lambda: op(fcl),
                "a_py_ensemble_predict": lambda: ens.predict(f), "b_torch_chain": lambda: torch_chain(dev_models, x, (HW, HW))}
    op(f)
    got = labels[0].cpu()
    want, _ = torch_chain(dev_models, x, (HW, HW))
    torch.cuda.synchronize()
    same = float((got == want).float().mean())
    for fn in variants.values():                                      # warm-up of every variant on this shape
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            ms[k].append(window(fn, calls))
    h1 = ens.h1
    flop = 2 * 2.0 * HW * HW * C_ * M * h1                            # two MFMA passes (x W1_hi, x W1_lo) of layer 1
    res = dict(config=name, C=C_, K=K, M=M, grid=[HW, HW], nets=[ens.h1, ens.h2], map_mb=round(C_ * HW * HW * 2 / 1e6, 1),
               mfma_tflop=round(flop / 1e12, 3), workspace_mb=round(nbytes / 1e6, 2), rounds=rounds, calls_per_window=calls,
               share_of_pixels_with_equal_labels_a_vs_b=round(same, 5))
    for k, t in ms.items():
        t = sorted(t)
        med = t[len(t) // 2]
        res[k] = dict(ms_median=round(med, 3), ms_fastest=round(t[0], 3), ms_slowest=round(t[-1], 3), spread=round((t[-1] - t[0]) / med, 4))
        if k.startswith("a_") and "py" not in k:
            res[k]["mfma_tflop_per_s_whole_call"] = round(flop / (med * 1e-3) / 1e12, 1)
    A, Bv = res["a_py_ensemble_predict"], res["b_torch_chain"]
    res["a_py_faster_than_b_beyond_spread"] = bool(A["ms_slowest"] < Bv["ms_fastest"])
    res["speedup_a_py_over_b"] = round(Bv["ms_median"] / A["ms_median"], 2)
    res["speedup_a_op_over_b"] = round(Bv["ms_median"] / res["a_pixcls_op_nchw"]["ms_median"], 2)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pixel_classifier.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--launches", type=int, default=0, help="only this many launches of variant a of --config (for a counter run); writes nothing")
    ap.add_argument("--config", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_pixel_classifier.py measures on the GPU; none is visible")
    if args.launches:
        name, C_, K = CONFIGS[args.config]
        _, _, f, op, _, _ = setup(C_, K)
        for _ in range(args.launches):
            op(f)
        torch.cuda.synchronize()
        print("launched", args.launches, "x", name)
        sys.exit(0)
    lines = ["# tools/bench_pixel_classifier.py on %s: M = %d pixel classifiers over one (1, C, %d, %d) fp16 map; ms per call (median of %d windows of "
             "%d calls, device events)" % (torch.cuda.get_device_name(0), M, HW, HW, args.rounds, args.calls),
             "# a = gdf_pixcls_predict (NCHW map), a_cl = channels-last map, a_py = PixelClassifierEnsemble.predict, b = the reference's predict_labels "
             "chain in fp32 on the same device tensors; TFLOP/s = the two fp16 MFMA passes of layer 1 / median time of the whole call"]
    for name, C_, K in CONFIGS:
        r = bench(name, C_, K, args.rounds, args.calls)
        print(json.dumps(r), flush=True)
        lines.append(json.dumps(r))
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
