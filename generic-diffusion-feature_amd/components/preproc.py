"""The PIL-to-tensor step of FeatureExtractor.extract on the device (csrc/preproc.hip): the bytes of every image are uploaded as
uint8 and gdf_op_pil_resize_u8 does Pillow's bicubic resize, .convert("RGB") and the image processor's normalisation, equal bit for bit to
`preprocess_image` on the host.  Opt-in: FeatureExtractor(device_preprocess=True) or GDF_DEVICE_PREPROCESS=1.

Images of mode RGB or L whose sides are at most 32 x `size` go through the kernels; anything else (P, 1, RGBA / LA — Pillow resizes those
premultiplied —, 16-bit, CMYK, a larger source) goes through the host function for that image alone and its fp32 row travels in the same
upload.  One pinned staging buffer per call holds everything at 16-byte offsets and is sent with ONE asynchronous copy; the buffers form a
ring, each guarded by an event recorded behind its copy, so the host never waits for the kernels and never rewrites bytes a copy still reads."""
import ctypes as C
import os
import threading

import numpy as np
import torch

DEVICE_MODES = ("RGB", "L")
MAX_RATIO = 32                        # gdf_op_pil_resize_u8 refuses in / out > 32 on an axis (ksize > 129)
RING = 3                              # staging buffers per device: the host may be this many calls ahead of the copies before it waits for one
ALIGN = 16

_rings = {}
_ring_lock = threading.Lock()      # a slot is picked, filled, sent and its event recorded as one step


def env_enabled():
    return os.environ.get("GDF_DEVICE_PREPROCESS", "").strip().lower() not in ("", "0", "false", "off", "no")


def is_hip_device(device):
    try:
        return torch.device(device).type == "cuda"
    except (RuntimeError, TypeError):
        return False


def resolve_flag(flag, device):
    """FeatureExtractor's `device_preprocess` keyword -> bool.  None reads GDF_DEVICE_PREPROCESS (the default is off; the variable is a
    preference and is ignored on a device that is not a HIP one); True on such a device raises: there is no CPU form of the kernels."""
    if flag is None:
        return env_enabled() and is_hip_device(device)
    if flag and not is_hip_device(device):
        raise RuntimeError(f"device_preprocess=True needs a HIP device, got {device!r}: the resize runs in libgdf.so's kernels and there is no "
                           "CPU fallback (leave it off to preprocess on the host)")
    return bool(flag)


def route(img, size):
    """'device' for an image the kernels take, 'host' for one that goes through the host function"""
    mode = getattr(img, "mode", None)
    if mode not in DEVICE_MODES:
        return "host"
    w, h = img.size
    if w < 1 or h < 1 or w > MAX_RATIO * size or h > MAX_RATIO * size:
        return "host"
    return "device"


def _up(n):
    return (n + ALIGN - 1) // ALIGN * ALIGN


def plan_batch(images, size, host_fn):
    """-> (items, total bytes): per image ('device', offset, array uint8 (h, w[, 3])) or ('host', offset, array fp32 (3, size, size)), the offsets
    multiples of 16 into one staging buffer"""
    items, off = [], 0
    for img in images:
        if route(img, size) == "device":
            a = np.ascontiguousarray(np.asarray(img))
            if a.dtype != np.uint8 or a.shape[:2] != (img.size[1], img.size[0]) or a.shape[2:] not in ((), (3,)):
                raise RuntimeError(f"device_preprocess: mode {img.mode} gave {a.dtype} {a.shape}")
            items.append(("device", off, a))
        else:
            row = host_fn(img)
            a = np.ascontiguousarray(row.detach().to(torch.float32).cpu().numpy().reshape(3, size, size))
            items.append(("host", off, a))
        off += _up(a.nbytes)
    return items, off


def default_host_fn(size):
    """preprocess_image of a pipeline whose image processor is the plain one: resize, convert, (u / 255) * 2 - 1"""
    def fn(img):
        a = np.asarray(img.resize((size, size)).convert("RGB"), dtype=np.float32) / 255.0
        return torch.from_numpy(a).permute(2, 0, 1)[None] * 2.0 - 1.0
    return fn


class _Slot:
    def __init__(self):
        self.buf, self.event = None, None


def _next_slot(dev, nbytes):
    """the ring's next staging buffer, at least nbytes long, once the copy that last read it has finished"""
    ring = _rings.setdefault(str(dev), {"slots": [_Slot() for _ in range(RING)], "next": 0})
    slot = ring["slots"][ring["next"]]
    ring["next"] = (ring["next"] + 1) % RING
    if slot.event is not None:
        slot.event.synchronize()           # RING calls back: only a host that far ahead of its own uploads waits here
    if slot.buf is None or slot.buf.numel() < nbytes:
        slot.buf = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, pin_memory=True)
    return slot


def device_preprocess(images, size, device, host_fn=None):
    """[PIL images] -> (B, 3, size, size) fp32 on `device`, equal to torch.concat([preprocess_image(i) for i in images]) bit for bit; queued on
    the CURRENT stream, nothing is read back and the host waits for no kernel.  host_fn(img) -> (1, 3, size, size) is the host path of the
    images the kernels do not take (FeatureExtractor passes its preprocess_image)."""
    from components import native
    if not is_hip_device(device):
        raise RuntimeError(f"device_preprocess needs a HIP device, got {device!r}; there is no CPU fallback")
    images = list(images)
    if not images:
        raise ValueError("device_preprocess: no images")
    size = int(size)
    lib = native.load_library()
    items, total = plan_batch(images, size, host_fn or default_host_fn(size))
    dev = torch.device(device)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    ws_bytes = 0
    for kind, _off, a in items:
        if kind == "device":
            n = lib.gdf_op_pil_resize_workspace_bytes(a.shape[0], a.shape[1], 1 if a.ndim == 2 else 3, size, size)
            if n == 0:
                raise RuntimeError(f"device_preprocess: {a.shape} -> {size}: {lib.gdf_last_error().decode()}")
            ws_bytes = max(ws_bytes, n)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        with _ring_lock:
            slot = _next_slot(dev, total)
            stage = slot.buf.numpy()
            for _kind, off, a in items:
                stage[off:off + a.nbytes] = a.reshape(-1).view(np.uint8)
            staged = torch.empty(total, dtype=torch.uint8, device=dev)
            staged.copy_(slot.buf[:total], non_blocking=True)
            if slot.event is None:
                slot.event = torch.cuda.Event()
            slot.event.record(stream)
        out = torch.empty((len(items), 3, size, size), dtype=torch.float32, device=dev)
        ws = torch.empty(max(ws_bytes, ALIGN), dtype=torch.uint8, device=dev)          # one workspace: the launches of a stream run in order
        sp = C.c_void_p(stream.cuda_stream)
        for b, (kind, off, a) in enumerate(items):
            if kind == "device":
                native._check(lib.gdf_op_pil_resize_u8(C.c_void_p(staged.data_ptr() + off), a.shape[0], a.shape[1], 1 if a.ndim == 2 else 3,
                                                       size, size, None, C.c_void_p(out[b].data_ptr()), C.c_void_p(ws.data_ptr()), sp),
                              "op_pil_resize_u8")
            else:
                out[b].copy_(staged[off:off + a.nbytes].view(torch.float32).view(3, size, size))
    return out
