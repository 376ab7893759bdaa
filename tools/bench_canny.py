#!/usr/bin/env python3
"""The device Canny (csrc/canny.hip, gdf_op_canny*): time per stage by HIP events against the bytes each stage moves once, and the CLI with
`--control canny` on its two input paths.

    python tools/bench_canny.py                 # the kernels: SDXL 1024^2 B=16 and SD1.5 512^2 B=32, fp32 / fp16 NCHW and uint8 HWC sources
    python tools/bench_canny.py --cli [N]       # extract_feature.py --control canny-xl, SDXL 1024^2 B=16, N images (default 64): loader threads against
                                                # --loader_threads 0; and, where cv2 is installed, the host cv2.Canny loop over the same images

Bytes per pixel, each counted once: classify reads the source (12 fp32 / 6 fp16 / 3 uint8) and writes 1; the linking stage reads the class map in
each of its four launches (4), writes parent + flag (5) and the edges (6 as the fp16 control tensor, 1 as uint8).  The walks towards a root
(flag and emit launches, candidates and strong pixels only) come on top and are data dependent: they are in the time, not in the bytes.  The rate is
set against the 6.29 TB/s DESIGN.md uses as achievable.  Prints one JSON line per measurement; nothing is asserted."""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "generic-diffusion-feature_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

HBM_ACHIEVABLE = 6.29e12
SRC_BYTES = {"f32_nchw": 12, "f16_nchw": 6, "u8_hwc3": 3}
KIND = {"u8_hwc3": 0, "f32_nchw": 2, "f16_nchw": 3}
vp = C.c_void_p


def images(B, S, seed=0):
    """(B, 3, S, S) fp32 in [-1, 1] on the byte lattice: blurred noise (sigma about 2 pixels), stretched per image"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(B * 3, 1, S, S, generator=g, device="cuda")
    k = torch.exp(-0.5 * (torch.arange(-6, 7, device="cuda", dtype=torch.float32) / 2.0) ** 2)
    k = k / k.sum()
    x = F.conv2d(F.conv2d(x, k.view(1, 1, -1, 1), padding=(6, 0)), k.view(1, 1, 1, -1), padding=(0, 6)).view(B, 3, S, S)
    lo, hi = x.amin((1, 2, 3), keepdim=True), x.amax((1, 2, 3), keepdim=True)
    u = ((x - lo) / (hi - lo) * 255).round()
    return u / 255 * 2 - 1


def timed(fn, reps=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    ev[0].record()
    for i in range(reps):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    ts = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(reps))
    return ts[len(ts) // 2], ts[0]


def kernels(B, S, kind, name):
    from components import native
    L = native.load_library()
    x = images(B, S)
    src = x if kind == "f32_nchw" else x.half() if kind == "f16_nchw" else ((x / 2 + 0.5) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    n = B * S * S
    ws = torch.empty(L.gdf_op_canny_workspace_bytes(B, S, S), dtype=torch.uint8, device="cuda")
    cls = torch.empty(n, dtype=torch.uint8, device="cuda")
    ctl = torch.empty((B, 3, S, S), dtype=torch.float16, device="cuda")
    u8 = torch.empty((B, S, S), dtype=torch.uint8, device="cuda")
    st = vp(torch.cuda.current_stream().cuda_stream)
    ok = lambda rc: rc == 0 or sys.exit(L.gdf_last_error().decode())
    classify = lambda: ok(L.gdf_op_canny_classify(vp(src.data_ptr()), KIND[kind], B, S, S, 100, 200, vp(cls.data_ptr()), st))
    link16 = lambda: ok(L.gdf_op_canny_link(vp(cls.data_ptr()), B, S, S, vp(ctl.data_ptr()), 1, vp(ws.data_ptr()), st))
    link8 = lambda: ok(L.gdf_op_canny_link(vp(cls.data_ptr()), B, S, S, vp(u8.data_ptr()), 0, vp(ws.data_ptr()), st))
    fused = lambda: ok(L.gdf_op_canny(vp(src.data_ptr()), KIND[kind], B, S, S, 100, 200, vp(ctl.data_ptr()), 1, vp(ws.data_ptr()), st))
    out = dict(config=name, batch=B, size=S, source=kind, pixels=n)
    classify()
    torch.cuda.synchronize()
    c = cls.view(B, S, S)
    out.update(strong_fraction=round(float((c == 2).float().mean()), 4), candidate_fraction=round(float((c == 0).float().mean()), 4))
    for label, fn, bpp in (("classify", classify, SRC_BYTES[kind] + 1), ("link_to_fp16_control", link16, 4 + 5 + 6), ("link_to_u8", link8, 4 + 5 + 1),
                           ("fused_to_fp16_control", fused, SRC_BYTES[kind] + 1 + 4 + 5 + 6)):
        med, best = timed(fn)
        out[label] = dict(ms_median=round(med, 4), ms_best=round(best, 4), bytes_per_pixel=bpp, gb=round(n * bpp / 1e9, 4),
                          tbps=round(n * bpp / (med * 1e-3) / 1e12, 3), fraction_of_achievable_hbm=round(n * bpp / (med * 1e-3) / HBM_ACHIEVABLE, 3))
    out["edge_fraction"] = round(float((ctl[:, 0] > 0).float().mean()), 4)
    # the host's share of one call (queueing five launches): the call returns before the device has finished
    t0 = time.perf_counter()
    for _ in range(50):
        native.canny(src, 100, 200)
    out["host_ms_per_native_canny_call"] = round((time.perf_counter() - t0) / 50 * 1e3, 4)
    torch.cuda.synchronize()
    return out


def cli_paths(n_images):
    import shutil
    import tempfile
    import numpy as np
    from PIL import Image
    os.environ.setdefault("GDF_SYNTHETIC_WEIGHTS", "1")
    import bench as BB
    import extract_feature as cli
    tmp = tempfile.mkdtemp(prefix="gdf_canny_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        rs = np.random.RandomState(0)
        base = (rs.rand(160, 160, 3) * 255).astype(np.uint8)
        os.makedirs(os.path.join(tmp, "imgs"))
        for i in range(n_images):
            Image.fromarray(np.roll(base, i, 0)).resize((1280, 960), Image.BICUBIC).save(os.path.join(tmp, "imgs", f"img{i:04d}.jpg"), quality=92)
        with open(os.path.join(tmp, "prompt.txt"), "w") as f:
            f.write("a photo of a cat")
        with open(os.path.join(tmp, "layers.json"), "w") as f:
            json.dump({k: True for k in BB.PRACTICAL["xl"]}, f)
        base_args = ["--layer", os.path.join(tmp, "layers.json"), "--version", "xl", "--img_size", "1024", "--t", "100", "-b", "16", "--control", "canny-xl",
                     "--input_dir", os.path.join(tmp, "imgs", "*.jpg"), "--prompt_file", os.path.join(tmp, "prompt.txt")]
        out = dict(config="extract_feature.py --control canny-xl, SDXL 1024^2 B=16, synthetic weights", images=n_images, source="1280x960 JPEG q92",
                   host_cpus_used=min(16, os.cpu_count() or 1), note="each figure includes building the extractor and its first (plan-building) batch")
        for label, extra in (("loader_threads_0", ["--loader_threads", "0"]), ("loader_threads_8", ["--loader_threads", "8"])):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cli.main(base_args + ["--output_dir", os.path.join(tmp, label)] + extra)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            out[label] = dict(seconds=round(dt, 2), img_per_s=round(n_images / dt, 2))
            shutil.rmtree(os.path.join(tmp, label), ignore_errors=True)
        try:
            import cv2
            ims = [np.array(Image.open(p).resize((1024, 1024)).convert("RGB")) for p in sorted(os.listdir(os.path.join(tmp, "imgs")))[:16]]
            t0 = time.perf_counter()
            for im in ims:
                cv2.Canny(im, 100, 200)
            out["host_cv2_ms_per_batch_of_16"] = round((time.perf_counter() - t0) * 1e3, 2)
        except ImportError:
            out["host_cv2_ms_per_batch_of_16"] = "cv2 is not installed on this box"
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--cli":
        print(json.dumps(cli_paths(int(sys.argv[2]) if len(sys.argv) > 2 else 64)), flush=True)
        sys.exit(0)
    for B, S, name in ((16, 1024, "SDXL 1024^2 B=16"), (32, 512, "SD1.5 512^2 B=32")):
        for kind in ("f32_nchw", "f16_nchw", "u8_hwc3"):
            print(json.dumps(kernels(B, S, kind, name)), flush=True)
