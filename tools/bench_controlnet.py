#!/usr/bin/env python3
"""UNet forward with and without ControlNet residuals (gdf_forward_res, include/gdf.h): step time of both and the time of the one
residual_add_kernel launch (HIP events inside the replayed graph, gdf_plan_set_timing) against its HBM traffic.

    python tools/bench_controlnet.py [xl|1-5] [batch]        # SDXL 1024^2 B=16 / SD1.5 512^2 B=32, practical hooks, synthetic weights
    python tools/bench_controlnet.py --model [xl|1-5 batch]  # the ControlNet as a native model: its forward, the UNet step with its block, both,
                                                             # and the conditioning embedding's convs against their HBM traffic
    python tools/bench_controlnet.py --ops [xl|1-5 batch]    # fingerprint of the uncontrolled bench plan's op program (to compare two commits)

Bytes of the add: read skip + read residual + write skip per element (split STREAM images: two reads and two writes of the pair).  The
achievable HBM rate it is set against is DESIGN.md's 6.29 TB/s.  Prints one JSON line per configuration."""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "generic-diffusion-feature_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402
import bench  # noqa: E402
from components.native import NativeUNet  # noqa: E402

HBM_ACHIEVABLE = 6.29e12


def measure(version, B, steps=10):
    cfg = bench._cfg(version)
    lat = 128 if version == "xl" else 64
    unet = NativeUNet(cfg, device="cuda:0").init_synthetic(0)
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(B, 4, lat, lat, generator=g, device="cuda").half()
    ctx = torch.randn(1, 77, cfg["cross_attention_dim"], generator=g, device="cuda").half().expand(B, -1, -1).contiguous()
    t = torch.full((B,), 100.0, device="cuda")
    txt = tid = None
    if cfg["addition_embed_text_time"]:
        txt = torch.randn(1, 1280, generator=g, device="cuda").half().expand(B, -1).contiguous()
        tid = torch.tensor([[1024, 1024, 0, 0, 1024, 1024]], dtype=torch.float32, device="cuda").repeat(B, 1)
    ids = bench.PRACTICAL[version]
    lay, nbytes = unet.residual_layout(B, lat, lat)
    block = (0.1 * torch.randn(nbytes // 2, generator=g, device="cuda")).half()
    elems = sum(b * c * h * w for _, (b, c, h, w) in lay)

    def timed(residuals):
        step = lambda: unet.forward_raw(x, t, ctx, txt, tid, hook_ids=ids, shared_ctx=True, residuals=residuals)
        o = None
        for _ in range(3):
            o = None
            o = step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            o = None
            o = step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3, step

    ms_plain, _ = timed(None)
    ms_res, step = timed(block)
    split = unet.last_split
    plan = unet._plan(B, lat, lat, 77, ids, True, split, residuals=True)
    lib = unet.lib
    lib.gdf_plan_set_timing_stride(plan.handle, 1)
    assert lib.gdf_plan_set_timing(plan.handle, b"residual_add_kernel") == 0, lib.gdf_last_error()
    o = None
    for _ in range(steps + 2):                       # (the first timed replays build the graphs that carry the event nodes)
        o = None
        o = step()
    torch.cuda.synchronize()
    ms, n, fl = C.c_double(), C.c_long(), C.c_double()
    lib.gdf_plan_read_timing(plan.handle, C.byref(ms), C.byref(n), C.byref(fl))
    lib.gdf_plan_set_timing(plan.handle, None)
    add_ms = ms.value / max(n.value, 1)
    stream_split = bool(split & 1)                   # SP_STREAM: the concat buffers hold (hi, lo) pairs
    add_bytes = elems * 2 * (5 if stream_split else 3)
    cap, lau, fail = plan.graph_stats()
    return dict(version=version, batch=B, latent=lat, hooks=len(ids), split_mask=split, tensors=len(lay), residual_block_mb=round(nbytes / 1e6, 1),
                unet_ms=round(ms_plain, 2), unet_with_residuals_ms=round(ms_res, 2), residual_add_ms=round(add_ms, 4),
                residual_add_launches_timed=n.value, residual_add_gb=round(add_bytes / 1e9, 3),
                residual_add_gbps=round(add_bytes / (add_ms * 1e-3) / 1e9, 1) if add_ms > 0 else None,
                fraction_of_achievable_hbm=round(add_bytes / (add_ms * 1e-3) / HBM_ACHIEVABLE, 3) if add_ms > 0 else None,
                share_of_step=round(add_ms / ms_res, 5), graph_failures=fail)


def embed_traffic_bytes(B, lat, c0, cond=(16, 32, 96, 256)):
    """HBM bytes of the conditioning embedding as shipped (unfused): the pack kernel (read the fp16 NCHW image, write 8-channel pixels), then
    per conv its input read once and its output written once, and the read of conv_out's image by conv_in's epilogue"""
    px = B * (8 * lat) ** 2
    total = px * 3 * 2 + px * 8 * 2
    layers = [(8, cond[0], 1), (cond[0], cond[0], 1), (cond[0], cond[1], 2), (cond[1], cond[1], 1), (cond[1], cond[2], 2), (cond[2], cond[2], 1),
              (cond[2], cond[3], 2), (cond[3], c0, 1)]
    conv = 0
    for ci, co, st in layers:
        conv += px * ci * 2
        px //= st * st
        conv += px * co * 2
    return total + conv + px * c0 * 2, conv


def measure_model(version, B, steps=10):
    """the ControlNet as a native model: its forward (writing straight into the UNet plan's staged residual block), the UNet step with that
    block, both together, and the embedding's convs by HIP events inside the replayed graph against the traffic of embed_traffic_bytes"""
    from components.native import NativeControlNet
    cfg = bench._cfg(version)
    lat = 128 if version == "xl" else 64
    unet = NativeUNet(cfg, device="cuda:0").init_synthetic(0)
    cn = NativeControlNet(cfg, device="cuda:0").init_synthetic(1000)
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(B, 4, lat, lat, generator=g, device="cuda").half()
    ctx = torch.randn(1, 77, cfg["cross_attention_dim"], generator=g, device="cuda").half().expand(B, -1, -1).contiguous()
    t = torch.full((B,), 100.0, device="cuda")
    txt = tid = None
    if cfg["addition_embed_text_time"]:
        txt = torch.randn(1, 1280, generator=g, device="cuda").half().expand(B, -1).contiguous()
        tid = torch.tensor([[1024, 1024, 0, 0, 1024, 1024]], dtype=torch.float32, device="cuda").repeat(B, 1)
    cond = (torch.randint(0, 256, (B, 3, 8 * lat, 8 * lat), generator=g, device="cuda").float() / 255).half()
    ids = bench.PRACTICAL[version]
    split = unet.split_for(ids, lat=lat)
    dst = unet.residual_buffer(B, lat, lat, 77, ids, True)
    control = lambda: cn.forward_raw(x, t, ctx, txt, tid, cond, shared_ctx=True, split=split, out=dst)
    step = lambda: unet.forward_raw(x, t, ctx, txt, tid, hook_ids=ids, shared_ctx=True, residuals=dst)

    def timed(fn):
        o = None
        for _ in range(3):
            o = None
            o = fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            o = None
            o = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3
    ms_cn = timed(control)
    ms_unet = timed(step)
    ms_both = timed(lambda: (control(), step())[1])
    ms_plain = timed(lambda: unet.forward_raw(x, t, ctx, txt, tid, hook_ids=ids, shared_ctx=True))
    plan = cn._plan(B, lat, lat, 77, True, split, direct=True)
    lib = cn.lib
    lib.gdf_plan_set_timing_stride(plan.handle, 1)
    assert lib.gdf_plan_set_timing(plan.handle, b"cond_conv3x3_kernel") == 0, lib.gdf_last_error()
    for _ in range(steps + 2):
        control()
    torch.cuda.synchronize()
    ms, n, fl = C.c_double(), C.c_long(), C.c_double()
    lib.gdf_plan_read_timing(plan.handle, C.byref(ms), C.byref(n), C.byref(fl))
    lib.gdf_plan_set_timing(plan.handle, None)
    chain_ms = ms.value / max(n.value, 1) * 8                  # eight conv launches per forward
    total_b, conv_b = embed_traffic_bytes(B, lat, cfg["block_out_channels"][0])
    cap, lau, fail = plan.graph_stats()
    return dict(model="controlnet", version=version, batch=B, latent=lat, split_mask=split, controlnet_ops=lib.gdf_plan_num_ops(plan.handle),
                controlnet_ms=round(ms_cn, 2), unet_with_residuals_ms=round(ms_unet, 2), both_ms=round(ms_both, 2), unet_plain_ms=round(ms_plain, 2),
                embed_convs_ms=round(chain_ms, 3), embed_conv_launches_timed=n.value, embed_convs_gb=round(conv_b / 1e9, 3),
                embed_total_gb=round(total_b / 1e9, 3), embed_convs_tflop=round(fl.value / max(n.value, 1) * 8 / 1e12, 3),
                embed_convs_tbps=round(conv_b / (chain_ms * 1e-3) / 1e12, 3) if chain_ms > 0 else None,
                fraction_of_achievable_hbm=round(conv_b / (chain_ms * 1e-3) / HBM_ACHIEVABLE, 3) if chain_ms > 0 else None,
                embed_share_of_controlnet=round(chain_ms / ms_cn, 4), graph_failures=fail)


def op_program(version, B):
    """the uncontrolled bench plan's op program (kernel symbol per op) and workspace size: compared between two commits"""
    cfg = bench._cfg(version)
    lat = 128 if version == "xl" else 64
    unet = NativeUNet(cfg, device="cuda:0")
    ids = bench.PRACTICAL[version]
    plan = unet._plan(B, lat, lat, 77, ids, True, unet.split_for(ids, lat=lat))
    n = unet.lib.gdf_plan_num_ops(plan.handle)
    import hashlib
    ops = [unet.lib.gdf_plan_op_kernel(plan.handle, i).decode() for i in range(n)]
    return dict(op_program=version, batch=B, ops=n, workspace_bytes=plan.ws_bytes, sha256=hashlib.sha256("\n".join(ops).encode()).hexdigest())


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] in ("--model", "--ops"):
        fn = measure_model if sys.argv[1] == "--model" else op_program
        for v, b in ([(sys.argv[2], int(sys.argv[3]))] if len(sys.argv) > 3 else [("xl", 16), ("1-5", 32)]):
            print(json.dumps(fn(v, b)), flush=True)
        sys.exit(0)
    which = [(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else (16 if sys.argv[1] == "xl" else 32))] if len(sys.argv) > 1 else [("xl", 16), ("1-5", 32)]
    for v, b in which:
        print(json.dumps(measure(v, b)), flush=True)
