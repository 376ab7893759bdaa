#!/usr/bin/env python3
"""DDIM-inversion extraction against plain extraction: SD1.5, 512x512, batch 32, one MI355X, synthetic weights.

    python tools/bench_inversion.py [--batch 32] [--img 512] [--t 50 200] [--steps 3] [--warmup 2] [--version 1-5]

For every t: `FeatureExtractor.extract(...)` and `extract(..., use_ddim_inversion=True)` on the same image batch resident on the
device, `--steps` timed calls each after `--warmup` untimed ones (plan creation, eager warm-up forward, graph construction), wall
clock around a device synchronisation.  The inversion runs K = the number of DDIM timesteps (100-step schedule) up to t hook-less
UNet forwards before the extraction forward (reference feature/components/ddim_inversion.py), so about (K + 1) UNet steps plus the
VAE encoder are expected.  Prints one JSON line.  Not run by any test."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "generic-diffusion-feature_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
os.environ.setdefault("GDF_SYNTHETIC_WEIGHTS", "1")

import torch  # noqa: E402


def timed(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--version", default="1-5")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--img", type=int, default=512)
    ap.add_argument("--t", type=int, nargs="+", default=[50, 200])
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import diffusion_feature
    from components.models import ddim_inversion_table
    layer = {"up-level1-repeat1-vit-block0-cross-q": True, "up-level2-repeat2-res-out": True}
    df = diffusion_feature.FeatureExtractor(layer=layer, version=a.version, img_size=a.img, device="cuda:0")
    prompt = df.encode_prompt("a photo of a cat")
    img = (torch.rand(a.batch, 3, a.img, a.img, generator=torch.Generator().manual_seed(0)) * 2 - 1).cuda()
    out = dict(metric="ms per extract() call", version=a.version, img=a.img, batch=a.batch, steps=a.steps, warmup=a.warmup, runs=[])
    for t in a.t:
        plain = timed(lambda: df.extract(prompt, a.batch, img, image_type="tensors", t=t), a.warmup, a.steps)
        inv = timed(lambda: df.extract(prompt, a.batch, img, image_type="tensors", t=t, use_ddim_inversion=True), a.warmup, a.steps)
        df.pipe.scheduler.set_timesteps(1000, device="cpu")
        k = len(ddim_inversion_table(df.pipe.scheduler, 100, df.pipe.get_timesteps(1000, t / 1000, "cpu")[0][:1]))
        traj = next(p for key, p in df.pipe.unet._plans.items() if key[4] == ())
        cap, lau, fail = traj.graph_stats()
        out["runs"].append(dict(t=t, inversion_steps=k, plain_ms=round(plain, 2), inverted_ms=round(inv, 2), ratio=round(inv / plain, 2),
                                per_inversion_step_ms=round((inv - plain) / k, 2), graphs_built=cap, graph_launches=lau, eager_fallbacks=fail))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
