#!/usr/bin/env python3
"""VAE encode + sample + noise-add (include/gdf_vae.h) at the headline shape: 16 images of 1024x1024, per-op profile.
    python tools/bench_vae.py [--batch 16] [--img 1024] [--steps 3]
--config flux: the native Flux latent preparation (profiles/flux_native_vae.txt) in ONE process —
    the Flux VAE's encode_packed and the SD VAE's encode at the same batch, alternating rounds; the packed tail kernel alone; and the Flux product
    call (extract on SyntheticFluxPipe) with the native VAE and with the average-pool stand-in.
    python tools/bench_vae.py --config flux [--batch 8] [--img 1024] [--steps 5] [--rounds 5] [--flux-layers 19,38] [--no-extract]"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "generic-diffusion-feature_amd")):
    sys.path.insert(0, p)
import torch
from components.native import NativeVAEEncoder, VAE_CONFIGS
from oracle.vae_ref import ARCH_SD_VAE, flops_per_image     # FLOP model only

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=16); ap.add_argument("--img", type=int, default=1024)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--config", choices=("sd", "flux"), default="sd")
ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--flux-layers", default=""); ap.add_argument("--no-extract", action="store_true")
a = ap.parse_args()


def spread(v):
    v = sorted(v)
    return "median %.3f ms (min %.3f, max %.3f, n=%d)" % (v[len(v) // 2], v[0], v[-1], len(v))


def timed(fn, steps):
    """ms per call of `steps` back-to-back calls, host clock around a device synchronise"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def bench_flux(a):
    import ctypes as C
    from components import native
    B = a.batch if a.batch != 16 else 8
    lat = a.img // 8
    g = torch.Generator(device="cuda").manual_seed(0)
    x = (torch.rand(B, 3, a.img, a.img, device="cuda", generator=g) * 2 - 1).half()
    sd = NativeVAEEncoder(VAE_CONFIGS["sd"], device="cuda:0").init_synthetic(0)
    fx = NativeVAEEncoder(VAE_CONFIGS["flux"], device="cuda:0").init_synthetic(1)
    e4 = torch.randn(B, 4, lat, lat, device="cuda", generator=g).half(); n4 = torch.randn_like(e4)
    e16 = torch.randn(B, 16, lat, lat, device="cuda", generator=g).half(); n16 = torch.randn_like(e16)
    run_sd = lambda: sd.encode(x, eps=e4, noise=n4, scaling_factor=0.13025, noise_a=1.0, noise_b=0.6, input_scale=0.86)
    run_fx = lambda: fx.encode_packed(x, eps=e16, noise=n16, scaling_factor=0.3611, shift_factor=0.1159, sigma=0.35, out_dtype=torch.float16)
    for f in (run_sd, run_fx):                                      # warm-up: eager first call, then the graph build, then a replay
        for _ in range(3):
            f()
    t_sd, t_fx = [], []
    for _ in range(a.rounds):                                       # alternating rounds of `steps` calls each
        t_sd.append(timed(run_sd, a.steps)); t_fx.append(timed(run_fx, a.steps))
    print(f"# batch {B} x {a.img}^2, {a.rounds} alternating rounds of {a.steps} calls, host clock around a device synchronise")
    print(f"SD   VAE encode        (L =  4, NCHW fp16 out):   {spread(t_sd)}")
    print(f"Flux VAE encode_packed (L = 16, packed fp16 out): {spread(t_fx)}")
    m_sd, m_fx = sorted(t_sd)[len(t_sd) // 2], sorted(t_fx)[len(t_fx) // 2]
    print(f"Flux / SD medians: {m_fx / m_sd:.4f}; SD's own spread (max - min) / median: {(max(t_sd) - min(t_sd)) / m_sd:.4f}")
    # ---- the packed tail alone: 16 rotating operand sets (16 x 29 MB at batch 8 > the 256 MB last-level cache), device events ----
    L = native.load_library()
    vp, ci, fp = C.c_void_p, C.c_int, C.c_float
    L.gdf_op_vae_finish_packed.restype = ci
    L.gdf_op_vae_finish_packed.argtypes = [vp, ci, ci, ci, ci, vp, vp, vp, vp, fp, fp, fp, fp, ci, vp, vp]
    sets = [(torch.randn(B * lat * lat, 32, device="cuda"), torch.randn(B, 16, lat, lat, device="cuda").half(),
             torch.randn(B, 16, lat, lat, device="cuda").half(), torch.empty(B, lat * lat // 4, 64, device="cuda", dtype=torch.float16)) for _ in range(16)]
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: C.c_void_p(t.data_ptr())

    def tail(k):
        h, e, n, o = sets[k % 16]
        rc = L.gdf_op_vae_finish_packed(P(h), B, lat, lat, 16, None, None, P(e), P(n), 0.3611, 0.1159, 0.65, 0.35, 0, P(o), st)
        assert rc == 0, L.gdf_last_error()
    for k in range(32):
        tail(k)
    nl, t_tail = 160, []
    for _ in range(a.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(nl):
            tail(k)
        e1.record(); torch.cuda.synchronize()
        t_tail.append(e0.elapsed_time(e1) / nl)
    byt = B * lat * lat * (32 * 4 + 16 * 2 * 3)                      # moments fp32 + eps + noise + tokens: 224 B per latent pixel
    m = sorted(t_tail)[len(t_tail) // 2]
    print(f"vae_finish_packed_kernel (L = 16, fp16, {byt / 1e6:.1f} MB per launch, {nl} launches per round over 16 operand sets, device events): "
          f"{spread(t_tail)} = {byt / m / 1e6:.0f} GB/s at the median")
    if a.no_extract:
        return
    # ---- the product call: extract on SyntheticFluxPipe, one pipe, the native VAE switched per round ----
    os.environ["GDF_FLUX_NATIVE_VAE"] = "1"
    import numpy as np
    from PIL import Image
    import diffusion_feature
    from components.models import SyntheticFluxPipe
    from components.native import FLUX_CONFIGS
    cfg = dict(FLUX_CONFIGS["flux"])
    if a.flux_layers:
        cfg["num_layers"], cfg["num_single_layers"] = [int(v) for v in a.flux_layers.split(",")]
    nblk = cfg["num_layers"] + cfg["num_single_layers"]
    del sd, fx, sets
    torch.cuda.empty_cache()
    pipe = SyntheticFluxPipe("cuda:0", seed=0, cfg=cfg)
    layer = {f"vit-block{nblk // 2}-out": True, f"vit-block{nblk - 1}-out": True}
    df = diffusion_feature.FeatureExtractor(layer=layer, version="flux", img_size=a.img, device="cuda:0", external_model=pipe)
    rs = np.random.RandomState(0)
    imgs = [Image.fromarray((rs.rand(a.img, a.img, 3) * 255).astype(np.uint8)) for _ in range(B)]
    nat = pipe.native_vae

    def extract(native_on):
        pipe.native_vae = nat if native_on else None
        df.extract("a photo of a cat", batch_size=B, image=imgs, t=300)
    for on in (True, False, True, False):
        extract(on)
    t_on, t_off = [], []
    for _ in range(a.rounds):
        t_on.append(timed(lambda: extract(True), 2)); t_off.append(timed(lambda: extract(False), 2))
    print(f"# extract on SyntheticFluxPipe ({cfg['num_layers']} + {cfg['num_single_layers']} blocks), batch {B} x {a.img}^2, 2 hooks, {a.rounds} alternating rounds of 2 calls")
    print(f"extract, GDF_FLUX_NATIVE_VAE=1 (native 16-channel VAE): {spread(t_on)}")
    print(f"extract, switch off (average-pool stand-in, torch):     {spread(t_off)}")


if a.config == "flux":
    bench_flux(a)
    sys.exit(0)
enc = NativeVAEEncoder(VAE_CONFIGS["sd"], device="cuda:0").init_synthetic(0)
g = torch.Generator(device="cuda").manual_seed(0)
x = (torch.rand(a.batch, 3, a.img, a.img, device="cuda", generator=g) * 2 - 1).half()
eps = torch.randn(a.batch, 4, a.img // 8, a.img // 8, device="cuda", generator=g).half(); noise = torch.randn_like(eps)
kw = dict(eps=eps, noise=noise, scaling_factor=0.13025, noise_a=1.0, noise_b=0.6, input_scale=0.86)
enc.encode(x, **kw); torch.cuda.synchronize()
_, prof = enc.encode(x, profile=True, **kw)
t0 = time.perf_counter()
for _ in range(a.steps):
    out = enc.encode(x, **kw)
torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / a.steps
fl = flops_per_image(ARCH_SD_VAE, a.img)
plan = enc._plan(a.batch, a.img, a.img)
print(f"VAE encode+sample+noise: batch {a.batch} x {a.img}^2: {dt * 1e3:.1f} ms/batch = {a.batch / dt:.1f} img/s, "
      f"{fl / 1e12:.2f} TFLOP/img -> {a.batch * fl / dt / 1e12:.0f} TFLOP/s; workspace {plan.ws_bytes / 1e9:.2f} GB; finite={bool(torch.isfinite(out.float()).all())}")
rows = {}
for name, ms, f_, k in prof:
    r = rows.setdefault(name, [0.0, 0.0, 0]); r[0] += ms; r[1] += f_; r[2] += 1
print("# per-op profile of ONE sub-batch pass:")
for name, r in sorted(rows.items(), key=lambda kv: -kv[1][0]):
    print(f"# {name:18s} n={r[2]:4d} {r[0]:9.3f} ms  {r[1] / 1e9 / max(r[0], 1e-9):8.1f} TFLOP/s")

# ---- `vae-out`: scheduler step + decoder (include/gdf_vae.h decoder half) at the same shape ----
from components.native import NativeVAEDecoder
from oracle.vae_ref import dec_flops_per_image
dec = NativeVAEDecoder(VAE_CONFIGS["sd"], device="cuda:0").init_synthetic(1)
lat = torch.randn(a.batch, 4, a.img // 8, a.img // 8, device="cuda", generator=g).half(); npred = torch.randn_like(lat)
dkw = dict(c_sample=1.0, c_eps=-0.4, scaling_factor=0.13025)
dec.decode(lat, npred, **dkw); torch.cuda.synchronize()
_, dprof = dec.decode(lat, npred, profile=True, **dkw)
t0 = time.perf_counter()
for _ in range(a.steps):
    img = dec.decode(lat, npred, **dkw)
torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / a.steps
fl = dec_flops_per_image(ARCH_SD_VAE, a.img)
dplan = dec._plan(a.batch, a.img // 8, a.img // 8)
print(f"VAE step+decode (vae-out): batch {a.batch} x {a.img}^2: {dt * 1e3:.1f} ms/batch = {a.batch / dt:.1f} img/s, "
      f"{fl / 1e12:.2f} TFLOP/img -> {a.batch * fl / dt / 1e12:.0f} TFLOP/s; workspace {dplan.ws_bytes / 1e9:.2f} GB; finite={bool(torch.isfinite(img.float()).all())}")
rows = {}
for name, ms, f_, k in dprof:
    r = rows.setdefault(name, [0.0, 0.0, 0]); r[0] += ms; r[1] += f_; r[2] += 1
print("# per-op profile of ONE sub-batch pass (decoder):")
for name, r in sorted(rows.items(), key=lambda kv: -kv[1][0]):
    print(f"# {name:18s} n={r[2]:4d} {r[0]:9.3f} ms  {r[1] / 1e9 / max(r[0], 1e-9):8.1f} TFLOP/s")
