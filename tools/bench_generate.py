#!/usr/bin/env python3
"""Guided generation with background feature extraction: the device-resident run against the host-driven loop, one MI355X, synthetic weights.

    python tools/bench_generate.py [--batch 16] [--img 512] [--steps 50] [--guidance 7.5] [--reps 3] [--version 1-5]

SD1.5, 512x512, B = 16 (the forwards have batch 32), 50 steps, the practical layer set kept at 5 encounters.  Three figures, ms per
UNET CALL, measured alternately `--reps` times on the same box after one untimed pass of each (plan creation, eager warm-up forwards,
graph construction), wall clock around a device synchronisation:
  generate    `FeatureExtractor.generate` (NativeUNet.sample: fp32 master, guidance + scheduler step in one kernel, one replayed graph for
              the hook-less calls)
  host loop   the loop it replaces over the same `pipe.unet`: fp32 latents kept by the host side, guidance and table arithmetic in torch,
              a hooked forward on every call (the store keeps the 5 encounters and drops the rest)
  plain step  one hook-less batch-32 UNet forward (graph replay), for reference
Prints one JSON line (medians and every repetition).  Not run by any test."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "generic-diffusion-feature_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
os.environ.setdefault("GDF_SYNTHETIC_WEIGHTS", "1")

import torch  # noqa: E402


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--version", default="1-5")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--img", type=int, default=512)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--guidance", type=float, default=7.5)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import diffusion_feature
    from components.models import sampling_table
    layer = os.path.join(ROOT, "generic-diffusion-feature_amd", "configs", "config_15_practical.json")
    df = diffusion_feature.FeatureExtractor(layer=layer, version=a.version, img_size=a.img, device="cuda:0")
    prompts = df.encode_prompt("a photo of a cat")
    B, g = a.batch, a.guidance
    rows, sigma0 = sampling_table(df.scheduler_backup, a.steps)
    n = len(rows)
    enc = sorted({1, max(1, n // 5), max(1, 2 * n // 5), max(1, 3 * n // 5), n})
    df.set_background_extraction(enc)
    lat = torch.randn(B, 4, a.img // 8, a.img // 8, generator=torch.Generator().manual_seed(0)).cuda()
    unet = df.pipe.unet
    ctx = torch.cat([prompts[1].repeat(B, 1, 1), prompts[0].repeat(B, 1, 1)], 0).cuda()

    def generate():
        df.generate(prompts, B, num_inference_steps=a.steps, guidance_scale=g, latents=lat)

    def host_loop():
        df.feature_store.reset()
        unet.shared_ctx = False
        x, hist = lat * sigma0, []
        for k, (t, c_in, c_s, *w) in enumerate(rows):
            inp = (x * c_in).half()
            eps = unet(torch.cat([inp, inp], 0), timestep=torch.tensor([t]), encoder_hidden_states=ctx, added_cond_kwargs={})[0].float()
            hist = (hist + [eps[:B] + g * (eps[B:] - eps[:B])])[-5:]
            x = c_s * x
            for j in range(min(5, k + 1)):
                if w[j] != 0.0:
                    x = x + w[j] * hist[-1 - j]
        return x

    x32 = torch.cat([lat, lat], 0).half()
    tt = torch.full((2 * B,), rows[0][0], device="cuda")

    def plain_steps():
        for _ in range(10):
            unet.forward_raw(x32, tt, ctx, hook_ids=[])

    for fn in (generate, host_loop, plain_steps, plain_steps):
        fn()
    torch.cuda.synchronize()
    gen, host, plain = [], [], []
    for _ in range(a.reps):
        gen.append(wall(generate) / n)
        host.append(wall(host_loop) / n)
        plain.append(wall(plain_steps) / 10)
    sampler = next(p for key, p in unet._plans.items() if key[4] == () and key[0] == 2 * B)
    cap, lau, fail = sampler.graph_stats()
    med = statistics.median
    r = lambda v: [round(x, 2) for x in v]
    print(json.dumps(dict(metric="ms per UNet call", version=a.version, img=a.img, batch=B, plan_batch=2 * B, unet_calls=n, encounters=enc,
                          hooks=len(unet.requested_ids()), guidance=g, generate_ms=round(med(gen), 2), host_loop_ms=round(med(host), 2),
                          plain_step_ms=round(med(plain), 2), generate_all=r(gen), host_loop_all=r(host), plain_step_all=r(plain),
                          hookless_plan_graphs_built=cap, graph_launches=lau, eager_fallbacks=fail)))


if __name__ == "__main__":
    main()
