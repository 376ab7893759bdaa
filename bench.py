#!/usr/bin/env python3
"""Benchmark of the hot path: SDXL 1024^2 single-timestep feature extraction (BASELINE.json configs[2]).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--batch 16] [--version xl]      (N > 1: starts its N ranks itself)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W
    python bench.py ... --full                   # also the per-kernel / roofline figures, power, the other plans and configs, the CPU baseline
    python bench.py ... --dump-outputs DIR       # after the timed steps: what the last step returned, as DIR/<name>.npy (float32)

A step = one UNet forward over one batch of `--batch` synthetic 1024x1024 images' pre-noised latents
(already resident in HBM) with the `config_xl_practical` hooks written to HBM.  One process per GPU, the
image batch is sharded (weak scaling: every rank runs its own `--batch`), weights are generated on rank 0
and broadcast once over RCCL, no collective in the hot loop.  Prints ONE JSON line on rank 0.

A plain run sets up, warms up, times the K steps (hipGraph replay, the product path) and prints the line; everything
else it can measure (the synchronising per-op pass, event nodes around the dominant kernel, hook-write rate, power,
the hipgraph / eager legs, other operand plans and configurations, the CPU baseline) runs only under --full.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(ROOT, "generic-diffusion-feature_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

PRACTICAL = {
    "xl": ["up-level0-repeat0-vit-block7-out", "up-level0-repeat0-vit-block5-out",
           "up-level1-repeat0-vit-block0-cross-q", "up-level1-repeat0-vit-block0-out"],
    "1-5": ["up-level1-repeat1-vit-block0-cross-q", "up-level1-repeat2-res-out",
            "up-level2-repeat1-vit-block0-cross-q", "up-level3-repeat0-vit-block0-self-k"],
}
MFMA_PEAK_TFLOPS = 2500.0      # dense fp16/bf16 MFMA peak, /opt/skills/guides/MI355X_MICROARCH.md
# what a loop of nothing but independent mfma_f32_16x16x32_f16 sustains on uniform-random operands (2 waves per SIMD, 128 accumulators):
# the chip is power-limited under MFMA load, zero operands reach 2440-2460 (tools/micro/mfma_shape.hip, profiles/r03_mfma_shape_ceiling.txt)
MFMA_RANDOM_DATA_CEILING_TFLOPS = 1930.0
HBM_PEAK_GBS = 8000.0


def unet_flops_per_image(cfg, lat):
    """Algorithmic FLOPs (2*MACs of convs, linears, QK^T, PV) per image — SURVEY.md §8(d)."""
    boc = cfg["block_out_channels"]; L = len(boc); nl = cfg["layers_per_block"]; cd = cfg["cross_attention_dim"]
    f = dict(conv=0.0, attn_linear=0.0, ff=0.0, self_attn=0.0, cross_attn=0.0)

    def conv(ci, co, hw, k=9):
        f["conv"] += 2.0 * hw * ci * co * k

    def resnet(ci, co, hw):
        conv(ci, co, hw); conv(co, co, hw)
        f["attn_linear"] += 2.0 * 1280 * co            # time_emb_proj (per image)
        if ci != co:
            conv(ci, co, hw, 1)

    def vit(c, hw, depth):
        f["attn_linear"] += 2 * 2.0 * hw * c * c       # proj_in / proj_out
        for _ in range(depth):
            f["attn_linear"] += 2.0 * hw * c * c * 4   # self q,k,v,out
            f["attn_linear"] += 2.0 * hw * c * c * 2   # cross q,out
            f["attn_linear"] += 2.0 * 77 * cd * c * 2  # cross k,v
            f["ff"] += 2.0 * hw * c * 8 * c + 2.0 * hw * 4 * c * c
            f["self_attn"] += 4.0 * hw * hw * c
            f["cross_attn"] += 4.0 * hw * 77 * c

    hw = lat * lat
    conv(cfg["in_channels"], boc[0], hw)
    ci = boc[0]
    for lv in range(L):
        for _ in range(nl):
            resnet(ci, boc[lv], hw)
            if cfg["has_attn"][lv]:
                vit(boc[lv], hw, cfg["transformer_layers"][lv])
            ci = boc[lv]
        if lv != L - 1:
            conv(boc[lv], boc[lv], hw // 4); hw //= 4
    resnet(boc[-1], boc[-1], hw); vit(boc[-1], hw, cfg["transformer_layers"][-1]); resnet(boc[-1], boc[-1], hw)
    prev = boc[-1]
    for i in range(L):
        lv = L - 1 - i
        co = boc[lv]; cskip = boc[max(lv - 1, 0)]
        for r in range(nl + 1):
            resnet((prev if r == 0 else co) + (cskip if r == nl else co), co, hw)
            if cfg["has_attn"][lv]:
                vit(co, hw, cfg["transformer_layers"][lv])
        if i != L - 1:
            hw *= 4; conv(co, co, hw)
        prev = co
    conv(boc[0], cfg["out_channels"], hw)
    return f


def cpu_baseline(version, lat_full, budget_s=100.0):
    """Time the CPU oracle (oracle/unet_ref.py, fp32) on a BOUNDED sample of the same workload: thread count
    calibrated on one ResnetBlock2D + one BasicTransformerBlock (best of 16/32/64/128), then the largest resolution whose
    predicted time fits `budget_s` (scaled by the algorithmic FLOP ratio when that is not the full resolution)."""
    from oracle import unet_ref as R
    arch = R.ARCHS[version]
    # the host CPUs THIS process may run on: under an N-rank launch every rank is pinned to its share of the host (components/dist.py
    # pin_rank_cores), and os.cpu_count() would report the whole machine
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    # 1. calibrate the thread count on the two block types that carry the forward: one ResnetBlock2D at level 0
    #    (320 -> 320 @ lat x lat) + one BasicTransformerBlock at the deepest attention level (C = 1280), both through the
    #    oracle's own block functions; candidates 16 / 32 / 64 / 128 threads (capped by the host)
    g = torch.Generator().manual_seed(0)
    c0, cd = arch["block_out_channels"][0], arch["cross_dim"]
    lv = max(i for i, a_ in enumerate(arch["down_attn"]) if a_)
    c2, tok = arch["block_out_channels"][lv], (lat_full >> lv) ** 2
    heads = arch["heads"][lv]
    rp = {"r.norm1.weight": torch.ones(c0), "r.norm1.bias": torch.zeros(c0), "r.norm2.weight": torch.ones(c0), "r.norm2.bias": torch.zeros(c0),
          "r.conv1.weight": torch.randn(c0, c0, 3, 3, generator=g) * 0.02, "r.conv1.bias": torch.zeros(c0),
          "r.conv2.weight": torch.randn(c0, c0, 3, 3, generator=g) * 0.02, "r.conv2.bias": torch.zeros(c0),
          "r.time_emb_proj.weight": torch.randn(c0, 1280, generator=g) * 0.02, "r.time_emb_proj.bias": torch.zeros(c0)}
    bp = {}
    for n_ in ("norm1", "norm2", "norm3"):
        bp[f"b.{n_}.weight"] = torch.ones(c2); bp[f"b.{n_}.bias"] = torch.zeros(c2)
    for n_, (o_, i_) in {"attn1.to_q": (c2, c2), "attn1.to_k": (c2, c2), "attn1.to_v": (c2, c2), "attn1.to_out.0": (c2, c2),
                         "attn2.to_q": (c2, c2), "attn2.to_k": (c2, cd), "attn2.to_v": (c2, cd), "attn2.to_out.0": (c2, c2),
                         "ff.net.0.proj": (8 * c2, c2), "ff.net.2": (c2, 4 * c2)}.items():
        bp[f"b.{n_}.weight"] = torch.randn(o_, i_, generator=g) * i_ ** -0.5
        if n_.endswith("to_out.0") or n_.startswith("ff"):
            bp[f"b.{n_}.bias"] = torch.zeros(o_)
    xr, emb = torch.randn(1, c0, lat_full, lat_full, generator=g), torch.randn(1, 1280, generator=g)
    xb, ctxb = torch.randn(1, tok, c2, generator=g), torch.randn(1, 77, cd, generator=g)
    cal_flops = 2.0 * lat_full * lat_full * c0 * c0 * 18 + 2.0 * tok * c2 * c2 * (6 + 12) + 4.0 * tok * tok * c2
    nostore = R.Store({"none": True})

    def cal_once():
        with torch.no_grad():
            R.resnet_block(rp, "r", xr, emb, nostore, "x")
            R.basic_transformer_block(bp, "b", xb, ctxb, heads, nostore, "x", False)

    best = (0.0, 1)
    all_rate = None
    for nt in sorted({min(cores, c) for c in (16, 32, 64, 128)} | {cores}):
        torch.set_num_threads(nt)
        cal_once()
        t = time.time(); n = 0
        while time.time() - t < 1.0:
            cal_once(); n += 1
        rate = n * cal_flops / (time.time() - t)
        if nt == cores:
            all_rate = rate                            # every host CPU (BASELINE.md §3's nominal setting): reported, not selected —
        if rate > best[0] and (nt < cores or cores <= 128):  # only the oversubscribed case is excluded: a full forward on 256 OpenMP threads ran 0.003 img/s (330 s / image)
            best = (rate, nt)
    rate, threads = best
    torch.set_num_threads(threads)
    # 2. constant-filled weights, one shared buffer per distinct fan-in (CPU timing is data independent and the
    #    buffers are read-only, so aliasing is harmless; the parity tests use the seeded random weights)
    shapes = R.param_shapes(arch)
    need = {}
    for name, shape in shapes.items():
        n = 1
        for s_ in shape:
            n *= s_
        is_norm = ".norm" in name or name.startswith("conv_norm_out")
        fan = 1
        for s_ in shape[1:]:
            fan *= s_
        key = fan if (name.endswith(".weight") and not is_norm) else (-1 if name.endswith(".weight") else -2)
        need[key] = max(need.get(key, 0), n)
    bufs = {k: torch.empty(n).fill_(k ** -0.5 if k > 0 else (1.0 if k == -1 else 0.01)) for k, n in need.items()}
    P = {}
    for name, shape in shapes.items():
        n = 1
        for s_ in shape:
            n *= s_
        is_norm = ".norm" in name or name.startswith("conv_norm_out")
        fan = 1
        for s_ in shape[1:]:
            fan *= s_
        key = fan if (name.endswith(".weight") and not is_norm) else (-1 if name.endswith(".weight") else -2)
        P[name] = bufs[key][:n].view(shape)
    ids = PRACTICAL[version]
    cfg = _cfg(version)
    fl = {lat: sum(unet_flops_per_image(cfg, lat).values()) for lat in (lat_full, lat_full // 2, lat_full // 4)}

    def run(lat):
        I = R.synth_inputs(arch, 1, lat, seed=1)
        st = R.Store({k: True for k in ids})
        t = time.time()
        with torch.no_grad():
            R.unet_forward(P, arch, I["sample"], I["timestep"], I["ctx"], I.get("text_embeds"), I.get("time_ids"), store=st)
        return time.time() - t

    eff = 0.8 * rate                                   # whole-UNet efficiency relative to the two calibration blocks
    lat = lat_full
    for cand in (lat_full, lat_full // 2, lat_full // 4):
        lat = cand
        if 9.0 * fl[cand] / eff <= budget_s:           # (1 warm-up + 2 reps) x (batch 1 + batch 2) = 9 image-forwards
            break

    def run_b(batch, reps):
        """>= 1 warm-up + `reps` timed repetitions of a batch-`batch` forward; returns the best time / image"""
        I = R.synth_inputs(arch, batch, lat, seed=1)
        ts = []
        for r in range(1 + reps):
            st = R.Store({k: True for k in ids})
            t = time.time()
            with torch.no_grad():
                R.unet_forward(P, arch, I["sample"], I["timestep"], I["ctx"], I.get("text_embeds"), I.get("time_ids"), store=st)
            if r > 0:
                ts.append((time.time() - t) / batch)
        return min(ts), ts

    scale = fl[lat_full] / fl[lat]
    t1, reps1 = run_b(1, 2)
    t2, reps2 = run_b(2, 2)
    best_t, best_b = min((t1, 1), (t2, 2))
    per_img = best_t * scale
    # all host CPUs: projected from the calibration blocks' rate on `cores` threads relative to the chosen thread count (a full
    # forward on 256 oversubscribed OpenMP threads would take minutes per image — measured once: 0.003 img/s)
    all_ips = (1.0 / per_img) * (all_rate / rate) if all_rate else None
    how = (f"full {lat * 8}x{lat * 8} resolution" if lat == lat_full else
           f"{lat * 8}x{lat * 8} scaled by the algorithmic FLOP ratio {scale:.1f}x to {lat_full * 8}x{lat_full * 8}")
    spent = sum(reps1) * 1.5 + sum(r * 2 for r in reps2) * 1.5
    return dict(value=round(1.0 / per_img, 5), unit="images/s", cores=threads, kind="port",
                batch1_images_per_s=round(1.0 / (t1 * scale), 5), batch2_images_per_s=round(1.0 / (t2 * scale), 5),
                all_cores={"cores": cores, "images_per_s_projected": round(all_ips, 5),
                           "calibration_gflops": round(all_rate / 1e9, 1)} if all_ips else None,
                sample=f"oracle/unet_ref.py fp32 at {how}; 1 warm-up + 2 timed repetitions each at batch 1 ({t1:.1f} s/img) and "
                       f"batch 2 ({t2:.1f} s/img), best = batch {best_b} on {threads} threads; ~{spent:.0f} s of CPU work "
                       f"(of {cores} host CPUs; thread count = best of 16/32/64/128 (and the host CPU count up to 128) on one level-0 ResnetBlock2D + one C=1280 "
                       f"BasicTransformerBlock of the oracle, {rate / 1e9:.0f} GFLOP/s there; on all {cores} CPUs the same two blocks run "
                       f"{(all_rate or 0) / 1e9:.0f} GFLOP/s)")


def _cfg(version):
    from components.native import ARCH_CONFIGS
    return ARCH_CONFIGS[version]


def csrc_sha():
    """sha256[:16] over the kernel / executor sources (sorted by name): stamps PMC results to the code they were taken on"""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(PKG, "csrc")
    for f in sorted(os.listdir(d)):
        if f.endswith((".hip", ".cpp", ".h")):
            h.update(f.encode()); h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()[:16]


DUMP_LIMIT_BYTES = 64_000_000


def dump_outputs(outdir, arrays, limit_bytes=DUMP_LIMIT_BYTES):
    """Write every tensor of `arrays` ({name: tensor}) as <outdir>/<name>.npy in float32, at most `limit_bytes` in all.  A tensor of
    more elements than its even share of the limit is written as a fixed sample of its flattened (row-major) elements: sorted indices
    drawn from a generator seeded with the name, so every run and every build writes the same positions.  Returns {name: (shape, kept)}."""
    import zlib
    import numpy as np
    os.makedirs(outdir, exist_ok=True)
    share = limit_bytes // 4 // max(1, len(arrays))
    info = {}
    for name, t in arrays.items():
        flat = t.detach().reshape(-1)
        n = flat.numel()
        if n > share:
            idx = np.sort(np.random.default_rng(zlib.crc32(name.encode())).choice(n, size=share, replace=False))
            flat = flat[torch.from_numpy(idx).to(flat.device)]
        a = flat.float().cpu().numpy()
        np.save(os.path.join(outdir, name + ".npy"), a if n > share else a.reshape(tuple(t.shape)))
        info[name] = (tuple(t.shape), min(n, share))
    return info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=16, help="images per GPU per step")
    ap.add_argument("--version", default="xl", choices=("xl", "1-5", "flux"),
                    help="xl = BASELINE headline (configs[2]); 1-5 = configs[1]; flux = configs[4] (single GPU, tools/bench_flux.py)")
    ap.add_argument("--img", type=int, default=0, help="image size (default 1024 for xl, 512 for 1-5)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--flux-dtype", default="bfloat16", choices=("bfloat16", "float16", "bfloat16x2", "fp8-mx", "float16s", "auto"), help="--version flux only")
    ap.add_argument("--fp16-stream", action="store_true", help="disable the fp32 master of the residual stream")
    ap.add_argument("--early-exit", action="store_true", help="opt-in: stop after the last requested hook")
    ap.add_argument("--precise", nargs="?", const="precise", default=None,
                    help="operand plan of the measured step: absent = 'auto' (chosen from the requested hooks: plain fp16 operands for the headline's "
                         "four); --precise = every operand class split (fp16 hi + lo, K doubled); --precise selective | plain | stream,attn_out ...")
    ap.add_argument("--full", action="store_true",
                    help="beyond the headline: per-op pass, live roofline of the dominant kernel (event nodes in the timed graphs), hook-write "
                         "rate, power, hipgraph / eager legs, plans / e2e / other_configs (N = 1, unless --no-extras), CPU baseline (unless "
                         "--no-cpu-baseline)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what the last step returned (noise_pred and every hook) as DIR/<name>.npy, float32, "
                         "at most 64 MB in all (larger tensors: a fixed seeded sample of their elements)")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip the plans / other_configs / e2e legs (N = 1 only run them)")
    ap.add_argument("--profile-ops", action="store_true", help="print a per-op time table (extra synchronising pass)")
    ap.add_argument("--e2e", action="store_true",
                    help="N = 1: time FeatureExtractor.extract(image_type='tensors') instead of the UNet step — VAE encode + sample + noise-add + "
                         "UNet + hooks on synthetic 1024^2 images resident in HBM, --steps batches; prints its own JSON line (the default line "
                         "carries the same measurement as its `e2e` block)")
    args = ap.parse_args()
    if args.dump_outputs and (args.e2e or args.version == "flux"):
        sys.exit("--dump-outputs covers the UNet step (--version xl / 1-5)")

    if args.e2e:                                   # the product call end to end; not BASELINE.json's metric: a separate line
        if int(os.environ.get("WORLD_SIZE", "1")) != 1 or args.gpus != 1 or args.version != "xl":
            sys.exit("--e2e is a single-GPU SDXL measurement")
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import bench_extra as BX_e2e                 # (a function-level `import torch` / `import ... as BX` here would shadow the names used below)
        dev = torch.device("cuda:0"); torch.cuda.set_device(dev)
        img = args.img or 1024
        blk = BX_e2e.e2e_block(dev, "xl", args.batch, img, PRACTICAL["xl"], steps=max(2, args.steps))
        print(json.dumps({"metric": "images/sec FeatureExtractor.extract end to end (VAE encode + noise-add + UNet + hooks), SDXL %d^2 single-timestep" % img,
                          "value": blk["extract_images_per_s"], "unit": "images/s", "n_gpus": 1, "steps": max(2, args.steps), "warmup": 3,
                          "ms_per_step": blk["extract_ms_per_batch"], "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f16",
                          "data": "synthetic", "config": {"workload": "FeatureExtractor.extract(image_type='tensors'), batch %d, t=100, hooks=config_xl_practical, "
                                                           "images resident in HBM" % args.batch, "global_batch": args.batch}, "e2e": blk}))
        return

    if args.version == "flux":                    # BASELINE configs[4]: same JSON schema, single GPU (tools/bench_flux.py)
        sys.argv = [sys.argv[0], "--steps", str(args.steps), "--warmup", str(args.warmup)] + (["--dtype", args.flux_dtype]) + \
                   (["--batch", str(args.batch)] if args.batch != 16 else []) + (["--no-cpu-baseline"] if args.no_cpu_baseline or not args.full else [])
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import bench_flux
        return bench_flux.main()
    rank = int(os.environ.get("RANK", "0")); world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # test hook: exercise the multi-rank code path on a 1-GPU box (all ranks on cuda:0, gloo instead of RCCL)
    share_gpu = os.environ.get("GDF_BENCH_SHARE_GPU", "0") == "1"
    if share_gpu:
        local = 0
    from components import dist as D
    pinned = None
    if not D.needs_self_launch(args.gpus) and world > 1:
        pinned = D.pin_rank_cores()        # this rank's share of the host cores, before anything touches the GPU or starts a thread pool
    if D.needs_self_launch(args.gpus):
        # The front door for N ranks (BASELINE configs[3]): `python3 bench.py --gpus N ...` started as ONE plain process starts its N
        # ranks itself — ordinary child processes with RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set, rendezvous on 127.0.0.1 — and
        # exits with their code; rank 0 inherits stdout, so its single JSON line is this command's output.  Nothing above this line
        # touches the GPU (device_count() does not initialise it), nothing is exec'd over a process that did.
        if not share_gpu and torch.cuda.device_count() < args.gpus:
            sys.exit(f"--gpus {args.gpus} needs {args.gpus} visible GPUs, torch.cuda.device_count() = {torch.cuda.device_count()}")
        sys.exit(D.self_launch(os.path.abspath(__file__), sys.argv[1:], args.gpus))
    if world != args.gpus:
        sys.exit(f"--gpus {args.gpus} does not match WORLD_SIZE={world}: one rank per GPU")
    # fail fast, before anything initialises a GPU (device_count() does not): N ranks need N visible GPUs
    if not share_gpu and torch.cuda.device_count() < max(1, args.gpus):
        sys.exit(f"--gpus {args.gpus} needs {args.gpus} visible GPUs, torch.cuda.device_count() = {torch.cuda.device_count()}")
    if not torch.cuda.is_available():
        sys.exit("bench.py needs an MI355X (no CPU fallback for the measured path)")
    torch.cuda.set_device(local)
    dev = torch.device(f"cuda:{local}")
    import torch.distributed as dist
    # test hook (GDF_RCCL_ONE_RANK=1 with WORLD_SIZE=1): the N-rank code path — RCCL group, weight broadcast, rank evidence, barriers, MAX over
    # ranks — in a ONE-rank RCCL group: the only RCCL configuration a 1-GPU box can run (two ranks cannot share a device under RCCL)
    multi = world > 1 or D.one_rank_group()
    json_fd = 1
    if multi:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        # RCCL prints a version banner ("RCCL version : ...", "Librccl path : ...") through C stdio on STDOUT, flushed at exit — i.e. AFTER the
        # JSON line (seen on hardware with the one-rank group).  The contract is ONE JSON line on stdout: keep the real stdout aside for that
        # line and point fd 1 at stderr for everything else this process (and the libraries in it) ever prints.
        sys.stdout.flush()
        json_fd = os.dup(1)
        os.dup2(2, 1)
        try:
            if share_gpu:
                dist.init_process_group("gloo", rank=rank, world_size=world)
            else:
                dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        except RuntimeError as e:
            if rank == 0 and ("EADDRINUSE" in str(e) or "address already in use" in str(e).lower()):
                print(f"[bench] rendezvous port {os.environ['MASTER_PORT']} is taken: {str(e)[:200]}", file=sys.stderr)
                sys.exit(D.RENDEZVOUS_BIND_FAILED)     # self_launch retries once on another port
            raise
        if dist.get_world_size() != args.gpus:
            sys.exit(f"process group reports {dist.get_world_size()} ranks, --gpus {args.gpus}")

    if os.environ.get("GDF_TEST_HOOKS") == "1" and os.environ.get("GDF_TEST_FAIL_RANK") == str(rank) and world > 1:
        sys.exit(3)                        # tests/test_gpu_dist.py only: a rank dying AFTER the rendezvous (the others sit in a collective) must fail the whole job
    group = D.group_evidence(dev)          # backend, ranks that answered one all_reduce, the PCI bus id of every rank's device
    from components.native import NativeUNet
    import ctypes as C
    cfg = _cfg(args.version)
    img = args.img or (1024 if args.version == "xl" else 512)
    lat = img // 8
    B = args.batch

    # ---- weights: generated on rank 0 in HBM (already in the kernels' layout), the arena broadcast once over RCCL ----
    unet = NativeUNet(cfg, device=dev, stream_fp32=not args.fp16_stream, early_exit=args.early_exit,
                      precise=None if args.precise is None else (False if args.precise == "plain" else args.precise))
    t0 = time.time()
    if rank == 0:
        unet.init_synthetic(seed=0)
    torch.cuda.synchronize()
    t_init = time.time() - t0
    if multi:
        dist.barrier()
    t0 = time.time()
    D.broadcast_model_weights(unet)        # flat device arena, 512 MiB pieces, rank 0 -> all (no-op for one process)
    assert unet.ready()
    torch.cuda.synchronize()
    t_bcast = time.time() - t0

    # ---- synthetic inputs, resident in HBM: one prompt repeated, t = 100 (random data, never zeros) ----
    g = torch.Generator(device=dev).manual_seed(1 + rank)
    x = torch.randn(B, 4, lat, lat, generator=g, device=dev).half()
    ctx = torch.randn(1, 77, cfg["cross_attention_dim"], generator=g, device=dev).half().expand(B, -1, -1).contiguous()
    t = torch.full((B,), 100.0, device=dev)
    txt = tid = None
    if cfg["addition_embed_text_time"]:
        pooled = cfg["add_in_dim"] - 6 * cfg["addition_time_embed_dim"]
        txt = torch.randn(1, pooled, generator=g, device=dev).half().expand(B, -1).contiguous()
        tid = torch.tensor([[img, img, 0, 0, img, img]], dtype=torch.float32, device=dev).repeat(B, 1)
    ids = PRACTICAL[args.version]

    def step():
        return unet.forward_raw(x, t, ctx, txt, tid, hook_ids=ids, shared_ctx=True)   # one prompt repeated

    prof = None
    # (a plan's first forward runs eagerly and its second builds the hipGraph: a plain run warms up with at least two, so that no graph is
    # built inside the timed region; under --full the timing graphs below are built before the clock as well)
    for w in range(max(1 if args.full else 2, args.warmup)):
        step()
    torch.cuda.synchronize()
    lib = unet.lib
    plan = unet._plan(B, lat, lat, 77, ids, True)
    if args.full or args.profile_ops:
        # a synchronising per-op pass (untimed): the per-kernel figures, and under --full the dominant kernel, timed live below with HIP events
        _, _, prof = unet.forward_raw(x, t, ctx, txt, tid, hook_ids=ids, profile=True, shared_ctx=True)
    out = None
    if args.full:
        by_label = {}
        for name, ms, fl, lab in prof:
            d = by_label.setdefault(lab, [0.0, 0.0, 0])
            d[0] += ms; d[1] += fl; d[2] += 1
        # the kernel that carries the most time AMONG those that carry algorithmic FLOPs (the roofline below is an MFMA roofline; on a tiny workload under
        # contention — the share-GPU tests — a bandwidth-bound norm kernel can top the list by a hair, and 0 FLOP / time is not a rate)
        flop_labels = [k for k in by_label if by_label[k][1] > 0]
        dominant = max(flop_labels or by_label, key=lambda k: by_label[k][0])
        TIMING_STRIDE = 8        # every 8th launch of the dominant kernel carries an event pair (an event node costs ~3.5 us inside a graph)
        rc = lib.gdf_plan_set_timing_stride(plan.handle, TIMING_STRIDE)
        assert rc == 0, lib.gdf_last_error()
        rc = lib.gdf_plan_set_timing(plan.handle, dominant.encode())
        assert rc == 0, lib.gdf_last_error()
        # The timed region below is the PRODUCT path: one hipGraphLaunch per step.  With timing switched on the library replays graphs
        # that carry event-record nodes around every launch of the dominant kernel (gdf.h gdf_plan_set_timing; one graph per timing
        # event set), so `roofline.achieved` is measured live inside the same K steps that give `value`.  Those graphs are built
        # here, before the clock starts; then the accumulators are reset.  (Results are dropped before each step so that the plan
        # reuses one hook-buffer set: a stable binding, no graph construction inside the timed region — asserted below.)
        for _ in range(4):
            out = None
            out = step()
        torch.cuda.synchronize()
        rc = lib.gdf_plan_set_timing(plan.handle, dominant.encode())
        assert rc == 0, lib.gdf_last_error()
    st_before = plan.graph_stats()

    def barrier():
        if multi:
            dist.barrier()
    sampler = None
    if args.full:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import bench_extra as BX
        sampler = BX.PowerSampler(local) if rank == 0 else None
    if sampler is not None:
        sampler.start()
    barrier(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = None
        out = step()
    torch.cuda.synchronize(); barrier()
    dt = time.perf_counter() - t0
    power = sampler.finish(t0, t0 + dt, images=B * args.steps) if sampler is not None else None
    st_after = plan.graph_stats()
    cap_in_region = st_after[0] - st_before[0]
    launches_in_region = st_after[1] - st_before[1]
    fails_in_region = st_after[2] - st_before[2]
    per_rank_ms = [1e3 * dt / args.steps]
    if multi:
        tt = torch.tensor([dt, -dt], device="cpu" if share_gpu else dev, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)                    # MAX over ranks of (dt, -dt): slowest and fastest rank
        per_rank_ms = [1e3 * float(-tt[1]) / args.steps, 1e3 * float(tt[0]) / args.steps]
        dt = float(tt[0])
        # That was the job's LAST collective.  The group is taken down here, on every rank, so that the ranks > 0 can finish and exit while
        # rank 0 runs its untimed legs (the per-op rooflines and the CPU baseline): no peer is ever left parked inside an RCCL call.
        torch.cuda.synchronize()
        dist.barrier()
        dist.destroy_process_group()
    if args.full:
        ms_tot = C.c_double(); launches = C.c_long(); fl_tot = C.c_double()
        lib.gdf_plan_read_timing(plan.handle, C.byref(ms_tot), C.byref(launches), C.byref(fl_tot))
        lib.gdf_plan_set_timing(plan.handle, None)
    hook_bytes = sum(v.numel() * 2 for v in out[1].values())
    for v in out[1].values():
        assert torch.isfinite(v.float()).all()
    if args.dump_outputs and rank == 0:
        # what a caller of the timed path receives from its last step: noise_pred (B, 4, H, W) and every requested hook
        dumped = dump_outputs(args.dump_outputs, {"noise_pred": out[0], **out[1]})
        print("[bench] wrote %d arrays to %s: %s" % (len(dumped), args.dump_outputs, ", ".join(
            f"{k} {s} ({n} values)" for k, (s, n) in dumped.items())), file=sys.stderr)

    if rank == 0:
        fl = unet_flops_per_image(cfg, lat)
        fl_img = sum(fl.values())
        if args.full:
            kv_img = 0.0
            for name, ms, f_, lab in prof:
                if name == "attn2_kv":
                    kv_img += f_                                       # (shared_ctx: the op's FLOPs are those of ONE prompt)
        ips = world * B * args.steps / dt
        if args.full:
            # HBM bytes/launch of the dominant kernel from the rocprofv3 --pmc passes of THIS command (tools/final_profile.sh ->
            # profiles/pmc_traffic_current.json).  The file is stamped with a hash of the kernel sources it was measured on: a
            # stamp that does not match the sources being benchmarked means the number is stale, and `traffic` is null.
            traffic, traffic_stale = None, None
            try:
                tj = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic_current.json")))
                if args.version == "xl" and B == 16 and dominant in tj:
                    if tj.get("_meta", {}).get("csrc_sha") == csrc_sha():
                        traffic, traffic_stale = tj[dominant]["hbm_bytes_per_launch"], False
                    else:                                              # measured on other kernel sources than the ones benchmarked: say so
                        traffic_stale = True
            except Exception:
                traffic = None
            achieved = (fl_tot.value / 1e12) / (ms_tot.value / 1e3) if ms_tot.value > 0 else 0.0
            dom_ops = {}
            for name, ms, f_, lab in prof:
                if lab == dominant:
                    d_ = dom_ops.setdefault(name, [0.0, 0.0]); d_[0] += ms; d_[1] += f_
        res = {
            "metric": "images/sec feature-extract, SDXL 1024^2 single-timestep" if args.version == "xl"
                      else "images/sec feature-extract, SD1.5 512^2 single-timestep",
            "value": round(ips, 3), "unit": "images/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(1e3 * dt / args.steps, 3), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f16", "data": "synthetic", "rccl": group,
            "timed_region": {"path": ("hipGraph replay (product default)" + (", event-record nodes around the dominant kernel" if args.full else "")
                                      if (plan.graph and launches_in_region == args.steps and fails_in_region == 0) else
                                      "eager launches (GDF_HIP_GRAPH=0)" if not plan.graph else
                                      f"MIXED: {launches_in_region} graph launches, {fails_in_region} eager fallbacks in {args.steps} steps"),
                             "graph_captures_inside": int(cap_in_region), "graph_launches_inside": int(launches_in_region),
                             "eager_fallbacks_inside": int(fails_in_region)},
            "config": {"workload": f"{'SDXL' if args.version == 'xl' else 'SD1.5'} UNet {img}x{img} (latent {lat}x{lat}), "
                                   f"batch {B}/GPU, t=100, hooks=config_{'xl' if args.version == 'xl' else '15'}_practical "
                                   f"({len(ids)} ids, {hook_bytes / B / 1e6:.2f} MB/img), full forward"
                                   + (" with early exit" if args.early_exit else ""),
                       "global_batch": world * B, "parallelism": f"dp{world} (batch sharded, weights broadcast once)",
                       "residual_stream": "fp16" if args.fp16_stream else "fp32 master + fp16 shadow",
                       "operands": (f"split-operand plan, class mask {unet.last_split} (fp16 hi + lo pairs for those operand classes, contraction over "
                                    "[hi | lo] x [W | W]; TFLOP/s figures count algorithmic FLOPs)" if unet.last_split else
                                    "fp16 activations x fp16 weights (the plan level 'auto' selects for these hooks: every one within 1e-3)"),
                       "tflop_per_image": round(fl_img / 1e12, 3),
                       # EXECUTED FLOPs: with one prompt repeated over the batch (reference diffusion_feature.py:272) the text K/V
                       # projections run once per batch (shared_ctx), not once per image
                       **({"model_tflops_per_s": round(ips * (fl_img - kv_img * (B - 1) / B) / 1e12, 1),
                           "shared_ctx_kv_gflop_per_image_not_executed": round(kv_img * (B - 1) / B / 1e9, 1)} if args.full else {}),
                       "weights_init_s": round(t_init, 1), "weights_broadcast_s": round(t_bcast, 3),
                       "weights_broadcast_gb_per_s": round(unet.weight_blob().numel() / 1e9 / t_bcast, 1) if multi and t_bcast > 0 else None,
                       "launched_by": ("bench.py itself (components/dist.py self_launch)" if os.environ.get("GDF_SELF_LAUNCHED") == "1" else
                                       "torch.distributed.run" if world > 1 else "single process"),
                       "max_inflight_forwards": int(os.environ.get("GDF_MAX_INFLIGHT", "4" if world > 1 else "0")),
                       "per_rank_ms_per_step": {"min": round(per_rank_ms[0], 3), "max": round(per_rank_ms[-1], 3)},
                       "rank_cpu_affinity": {"rank0_cpus": len(pinned), "first": pinned[0], "last": pinned[-1]} if pinned else None},
        }
        if args.full:
            res.update({
                "roofline": {"bound": "mfma", "kernel": dominant, "achieved": round(achieved, 1), "peak": MFMA_PEAK_TFLOPS,
                             "unit": "TFLOP/s", "frac": round(achieved / MFMA_PEAK_TFLOPS, 4), "traffic": traffic, "traffic_stale": traffic_stale,
                             "frac_of_random_operand_mfma_ceiling": round(achieved / MFMA_RANDOM_DATA_CEILING_TFLOPS, 4),
                             "random_operand_mfma_ceiling": MFMA_RANDOM_DATA_CEILING_TFLOPS,
                             "launches": int(launches.value), "avg_launch_ms": round(ms_tot.value / max(1, launches.value), 4),
                             "sampling": f"HIP events around every {TIMING_STRIDE}th launch of the kernel in program order, all K steps "
                                         f"({int(launches.value)} of {TIMING_STRIDE * int(launches.value)} launches)",
                             "flops_per_launch_g": round(fl_tot.value / max(1, launches.value) / 1e9, 2),
                             "share_of_step_time": round(by_label[dominant][0] / sum(v[0] for v in by_label.values()), 3),
                             # the same kernel symbol serves several op classes of the plan: TFLOP/s and ms per class (synchronising
                             # per-op pass).  Since round 2 the fp32-residual attention out-projections (HBM-bound epilogue, 0.27 of
                             # the peak on the 128x160 ring in round 1) run on this kernel too, which lowers its AVERAGE rate while
                             # every class and the step got faster.
                             "by_op": {n: {"tflops": round(v[1] / 1e9 / max(v[0], 1e-9), 1), "ms": round(v[0], 3)}
                                       for n, v in sorted(dom_ops.items(), key=lambda kv: -kv[1][0])}},
                "kernel_time_share": {k: round(v[0] / sum(x[0] for x in by_label.values()), 3)
                                      for k, v in sorted(by_label.items(), key=lambda kv: -kv[1][0])[:8]},
                "kernel_tflops": {k: round(v[1] / 1e9 / v[0], 1) for k, v in by_label.items() if v[1] > 0 and v[0] > 0},
            })
            # ---- the rooflines BASELINE.json's north_star names, from the synchronising per-op pass (one forward) ----
            # attention-MFMA: self-attention QK^T + PV FLOPs / time of those launches; conv: 3x3 conv FLOPs / time (MFMA) and the
            # ResBlock activation bytes of SURVEY.md §8d (2 Cin + 3 Cout per pixel, fp16) / time of all ResBlock ops (HBM);
            # hook writes: bytes of the hooks stored by copy2d_kernel / its time.
            grp = {}
            for name, ms, f_, _k in prof:
                g_ = grp.setdefault(name, [0.0, 0.0]); g_[0] += ms; g_[1] += f_
            def tsum(names):
                return sum(grp[n][0] for n in names if n in grp), sum(grp[n][1] for n in names if n in grp)
            a_ms, a_fl = tsum(["attn1"])
            c_ms, c_fl = tsum(["res_conv1", "res_conv2", "upsample", "downsample"])
            r_ms, _ = tsum(["res_conv1", "res_conv2", "res_shortcut", "gn_stats", "gn_apply_silu"])
            res_bytes = B * (610.8e6 if args.version == "xl" and lat == 128 else 152.9e6 if args.version == "1-5" and lat == 64 else 0.0)
            h_ms, _ = tsum(["hook_store"])
            # only the hooks the plan routes through hook_store (copy2d_kernel); the others are written by their producer's epilogue
            copied = sum(nbytes for i, (_hid, _shp, _str, nbytes) in enumerate(plan.hooks) if lib.gdf_plan_hook_copied(plan.handle, i))
            res["rooflines"] = {
                "attention_mfma": {"kernel": "attn_kernel", "achieved": round(a_fl / 1e9 / max(a_ms, 1e-9), 1), "peak": MFMA_PEAK_TFLOPS,
                                   "unit": "TFLOP/s", "frac": round(a_fl / 1e9 / max(a_ms, 1e-9) / MFMA_PEAK_TFLOPS, 4),
                                   "ms_per_step": round(a_ms, 3)},
                "conv_mfma": {"achieved": round(c_fl / 1e9 / max(c_ms, 1e-9), 1), "peak": MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                              "frac": round(c_fl / 1e9 / max(c_ms, 1e-9) / MFMA_PEAK_TFLOPS, 4), "ms_per_step": round(c_ms, 3)},
                "conv_hbm": {"achieved": round(res_bytes / 1e6 / max(r_ms, 1e-9), 1) if res_bytes else None, "peak": HBM_PEAK_GBS,
                             "unit": "GB/s", "frac": round(res_bytes / 1e6 / max(r_ms, 1e-9) / HBM_PEAK_GBS, 4) if res_bytes else None,
                             "note": "ResBlock activation bytes (2 Cin + 3 Cout per pixel, fp16) / time of conv + GroupNorm + shortcut ops: "
                                     "the fused block is MFMA-bound, so this fraction is far below 1 by construction",
                             "ms_per_step": round(r_ms, 3)},
                "hook_writes": {"kernel": "copy2d_kernel", "achieved": round(2 * copied / 1e6 / max(h_ms, 1e-9), 1) if h_ms > 0 else None,
                                "peak": HBM_PEAK_GBS, "unit": "GB/s (read + write)",
                                "frac": round(2 * copied / 1e6 / max(h_ms, 1e-9) / HBM_PEAK_GBS, 4) if h_ms > 0 else None,
                                "bytes_per_step": copied, "ms_per_step": round(h_ms, 4)},
            }
            # hook writes as rocprofv3 sees them: HIP events around every copy2d_kernel launch inside the replayed graph (the
            # synchronising per-op pass above includes ~5 us of launch + sync latency per 20-us kernel)
            if h_ms > 0 and copied:
                lib.gdf_plan_set_timing_stride(plan.handle, 1)
                if lib.gdf_plan_set_timing(plan.handle, b"copy2d_kernel") == 0:
                    o2 = None
                    for _ in range(6):
                        o2 = None
                        o2 = step()
                    torch.cuda.synchronize()
                    hm = C.c_double(); hl = C.c_long(); hf = C.c_double()
                    lib.gdf_plan_read_timing(plan.handle, C.byref(hm), C.byref(hl), C.byref(hf))
                    lib.gdf_plan_set_timing(plan.handle, None)
                    o2 = None
                    n_copy = sum(1 for name, *_r in prof if name == "hook_store")
                    if hl.value >= n_copy > 0 and hm.value > 0:
                        steps_t = hl.value / n_copy
                        ev_ms = hm.value / steps_t
                        hw = res["rooflines"]["hook_writes"]
                        hw.update({"achieved": round(2 * copied / 1e6 / ev_ms, 1), "frac": round(2 * copied / 1e6 / ev_ms / HBM_PEAK_GBS, 4),
                                   "ms_per_step": round(ev_ms, 4), "timing": "HIP events around every copy2d_kernel launch inside the graph replay",
                                   "sync_pass_gbs": hw["achieved"]})
            # ---- extra legs (N = 1): the same steps WITHOUT the timing nodes (`hipgraph.value`: what FeatureExtractor.extract runs) and
            # eagerly launched (`eager_host_cpu_ms_per_step`: the host cost the graph removes)
            if world == 1:
                def leg():
                    for _ in range(3):
                        step()
                    torch.cuda.synchronize()
                    capw = plan.graph_stats()[0]
                    c0 = time.process_time(); t1 = time.perf_counter()
                    for _ in range(args.steps):
                        step()
                    c1 = time.process_time()
                    torch.cuda.synchronize()
                    return time.perf_counter() - t1, (c1 - c0) / args.steps * 1e3, capw
                dt2, cpu_graph, cap0 = leg()
                cap1, lau1, _f1 = plan.graph_stats()
                lib.gdf_plan_set_graph(plan.handle, 0); plan.graph = False
                _, cpu_eager, _ = leg()
                lib.gdf_plan_set_graph(plan.handle, 1); plan.graph = True
                res["hipgraph"] = {"value": round(B * args.steps / dt2, 3), "unit": "images/s",
                                   "host_cpu_ms_per_step": round(cpu_graph, 2), "eager_host_cpu_ms_per_step": round(cpu_eager, 2),
                                   "captures_total": cap1, "captures_in_timed_steps": cap1 - cap0,
                                   "graph_launches": lau1, "ops_per_step": lib.gdf_plan_num_ops(plan.handle)}
            if power:
                res["power"] = power
            if world == 1 and not args.no_extras and args.precise is None and not args.early_exit and not args.fp16_stream:
                try:
                    res["plans"] = BX.plans_block(unet, step, B, res["hipgraph"]["value"])
                except Exception as e:
                    res["plans"] = {"error": repr(e)[:300]}
                unet._plans.clear(); torch.cuda.empty_cache()
                if args.version == "xl" and B == 16 and not args.img:
                    try:
                        res["e2e"] = BX.e2e_block(dev, args.version, B, img, ids)
                    except Exception as e:
                        res["e2e"] = {"error": repr(e)[:300]}
                    res["other_configs"] = BX.other_configs_block(dev, unet_flops_per_image, PRACTICAL)
        if args.profile_ops:
            rows = {}
            for name, ms, f_, _k in prof:
                r = rows.setdefault(name, [0.0, 0.0, 0]); r[0] += ms; r[1] += f_; r[2] += 1
            for name, r in sorted(rows.items(), key=lambda kv: -kv[1][0]):
                print(f"# {name:16s} n={r[2]:4d} {r[0]:9.3f} ms  {r[1] / 1e9 / max(r[0], 1e-9):8.1f} TFLOP/s", file=sys.stderr)
        if args.full and not args.no_cpu_baseline:
            # (any N: rank 0 times it after the process group is gone, on its own share of the host cores)
            res["cpu_baseline"] = cpu_baseline(args.version, lat)
            res["cpu_baseline"]["host"] = {"cpus": os.cpu_count(), "rank0_affinity_cpus": len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else None,
                                           "pinned_by": "components/dist.py pin_rank_cores" if pinned else None,
                                           "when": "after the timed region" + (", after destroy_process_group (the other ranks have left)" if multi else "")}
            res["config"]["gpu_over_cpu"] = round(ips / res["cpu_baseline"]["value"], 1)
        if json_fd == 1:
            print(json.dumps(res))
        else:
            sys.stdout.flush()
            os.write(json_fd, (json.dumps(res) + "\n").encode())


if __name__ == "__main__":
    main()
