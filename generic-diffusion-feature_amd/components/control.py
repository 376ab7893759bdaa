"""ControlNet conditioning on the native path: the reference's ControlNetPipeline (/root/reference/feature/components/controlnet.py:87-136)
with every model a NativeControlNet (components/native.py, include/gdf_control.h).

The preprocessors turn an ordinary image into a control image.  On a HIP device 'canny' / 'canny-xl' run there (device_canny: components/native.py
canny, csrc/canny.hip — cv2.Canny(image, 100, 200) restated) on the image batch the VAE encoder is about to read; that is the
product path, with no CPU fallback and whether or not cv2 is installed.  What stays on the host, and optional: controlnet_aux's MidasDetector
('depth') and, on any other device, cv2.Canny — imported at first use; `control_image=` hands over already-processed control images and needs none.
What the reference does per call and this does too: preprocess every image, VaeImageProcessor(do_convert_rgb=True, do_normalize=False)
-> (B, 3, h, w) in [0, 1] `.half()`, run every ControlNet on the UNet's own inputs (conditioning_scale 1, guess_mode off), add the
residuals of several ControlNets elementwise in fp16.  Here the residuals are ONE flat fp16 block (gdf_forward_res's layout), so the merge is
one torch add on the blocks — the reference's fp16 add, bit for bit."""
import numpy as np
import torch
import torch.nn.functional as F

REPOS = {"canny": "lllyasviel/sd-controlnet-canny", "depth": "lllyasviel/sd-controlnet-depth", "canny-xl": "diffusers/controlnet-canny-sdxl-1.0"}


def _missing(module, choice):
    return NotImplementedError(f"the '{choice}' preprocessor needs the Python module {module}, which is not installed: pass already-processed "
                               f"control images with control_image= instead")


def canny_preprocessor():
    """reference controlnet.py:30-36: cv2.Canny(image, 100, 200) replicated to three channels"""
    try:
        import cv2
    except ImportError:
        raise _missing("cv2", "canny") from None
    from PIL import Image

    def f(image):
        e = cv2.Canny(np.array(image), 100, 200)[:, :, None]
        return Image.fromarray(np.concatenate([e, e, e], axis=2))
    return f


def depth_preprocessor():
    """reference controlnet.py:69-72"""
    try:
        from controlnet_aux import MidasDetector
    except ImportError:
        raise _missing("controlnet_aux", "depth") from None
    return MidasDetector.from_pretrained("lllyasviel/Annotators")


PREPROCESSORS = {"canny": canny_preprocessor, "canny-xl": canny_preprocessor, "depth": depth_preprocessor}


def device_canny(source):
    """The device form of canny_preprocessor + control_tensor: `source` — the (B, 3, S, S) tensor in [-1, 1] preprocess_image made (it quantises
    to the very bytes of the RGB image it came from) or uint8 (B, S, S, 3) image bytes, on the HIP device — -> (B, 3, S, S) fp16 of 0.0 / 1.0,
    the three-channel edge image divided by 255.  Queued on the current stream."""
    from components import native
    return native.canny(source, 100, 200, out='control')


DEVICE_PREPROCESSORS = {"canny": device_canny, "canny-xl": device_canny}       # the choices whose preprocessor runs on a HIP device


def is_hip_device(device):
    return torch.device(device).type == "cuda"


def device_preprocessed(choices, device="cuda"):
    """True when every choice's preprocessor runs on `device`: nobody needs the PIL images (the CLI's loader-thread path stays on)"""
    return bool(choices) and is_hip_device(device) and all(c in DEVICE_PREPROCESSORS for c in choices)


def control_tensor(images, height, width):
    """Control images -> (B, 3, height, width) fp16 in [0, 1], as VaeImageProcessor(do_convert_rgb=True, do_normalize=False).preprocess
    followed by `.half()` gives it: PIL images are converted to RGB, resized (lanczos, the processor's default) where their size differs and
    divided by 255; a (B, 3, h, w) tensor in [0, 1] is resized with F.interpolate (the processor's torch branch) where its size differs."""
    if torch.is_tensor(images):
        t = images
        if t.dim() == 3:
            t = t[None]
        if t.dim() != 4 or t.shape[1] != 3:
            raise ValueError(f"control_image must be (B, 3, h, w), got {tuple(images.shape)}")
        t = t.float()
        if tuple(t.shape[-2:]) != (height, width):
            t = F.interpolate(t, size=(height, width))
        return t.half()
    from PIL import Image
    out = []
    for im in (images if isinstance(images, (list, tuple)) else [images]):
        im = im.convert("RGB")
        if im.size != (width, height):
            im = im.resize((width, height), resample=Image.LANCZOS)
        out.append(torch.from_numpy(np.array(im).astype(np.float32) / 255.0).permute(2, 0, 1))
    return torch.stack(out).half()


class ControlNetPipeline:
    def __init__(self, pipe, choices, device, models=None):
        """choices: names from {'canny', 'depth', 'canny-xl'}; anything else raises NotImplementedError as the reference does.
        models (native extension): ready models, one per choice, instead of the checkpoints / synthetic weights."""
        self.choices = list(choices)
        for c in self.choices:
            if c not in REPOS:
                raise NotImplementedError
        self.device = device
        self.vae_scale_factor = int(getattr(pipe, "vae_scale_factor", 8))
        self.control = list(models) if models is not None else [self._load(pipe, c, i) for i, c in enumerate(self.choices)]
        if len(self.control) != len(self.choices):
            raise ValueError("one model per choice")
        self._pre = {}
        self.on_device = is_hip_device(device)

    def device_route(self, choice):
        return self.on_device and choice in DEVICE_PREPROCESSORS

    def needs_pil(self):
        """some choice's preprocessor runs on the host and wants the PIL images"""
        return not all(self.device_route(c) for c in self.choices)

    def needs_source(self):
        """some choice's preprocessor runs on the device and wants the image batch there"""
        return any(self.device_route(c) for c in self.choices)

    def _load(self, pipe, choice, index):
        from components.native import NativeControlNet, native_controlnet_from
        cfg = pipe.unet.cfg
        if getattr(pipe, "synthetic_weights", False):           # GDF_SYNTHETIC_WEIGHTS=1: no checkpoints offline
            return NativeControlNet(cfg, self.device).init_synthetic(seed=1000 + index)
        from diffusers import ControlNetModel
        m = ControlNetModel.from_pretrained(REPOS[choice], torch_dtype=torch.float16, use_safetensors=True)
        cn = native_controlnet_from(m, self.device)
        diff = [k for k in cfg if k != "out_channels" and tuple(np.atleast_1d(cfg[k])) != tuple(np.atleast_1d(cn.cfg[k]))]
        if diff:
            raise ValueError(f"ControlNet '{choice}' ({REPOS[choice]}) does not match this pipeline's UNet: {diff} differ")
        return cn

    def preprocessor(self, choice):
        if choice not in self._pre:
            self._pre[choice] = PREPROCESSORS[choice]()
        return self._pre[choice]

    def control_images(self, choice, images, height, width, control_image=None, source=None, shared=None):
        """the control image batch of one ControlNet: `control_image` (already processed), the device preprocessor's output for `source` (on
        the device already; `shared`: a dict that keeps one result per preprocessor for the ControlNets of one call), or the host
        preprocessor's output for the PIL `images`"""
        if control_image is None and self.device_route(choice):
            if source is None:
                raise ValueError("ControlNet conditioning needs the image batch on the device (image_type='image' or 'tensors') or control_image=")
            pre = DEVICE_PREPROCESSORS[choice]
            cond = shared.get(pre) if shared is not None else None
            if cond is None:
                cond = pre(source)
                if shared is not None:
                    shared[pre] = cond
            return cond if tuple(cond.shape[-2:]) == (height, width) else control_tensor(cond, height, width)
        if control_image is None:
            if images is None:
                raise ValueError("ControlNet conditioning needs the PIL images (image_type='image') or control_image=")
            pre = self.preprocessor(choice)
            control_image = [pre(im) for im in images]
        return control_tensor(control_image, height, width)

    def generate_control_info(self, images, latents, t, prompt_embeds, added_cond_kwargs, control_image=None, shared_ctx=False, split=0,
                              out=None, source=None):
        """-> the residual block (flat fp16, NativeUNet.forward_raw(residuals=...)) of all ControlNets for the UNet inputs `latents`, `t`,
        `prompt_embeds`, `added_cond_kwargs`.  out: a flat fp16 tensor the (first) model writes straight into.
        images: the PIL images of the host preprocessors; source: the image batch on the device for the device preprocessors (device_canny)."""
        akw = added_cond_kwargs or {}
        B, _, H, W = latents.shape
        block = None
        shared = {}
        for choice, model in zip(self.choices, self.control):
            cond = self.control_images(choice, images, H * self.vae_scale_factor, W * self.vae_scale_factor, control_image, source, shared)
            if control_image is not None or not self.device_route(choice):
                cond = cond.to(self.device)
            if cond.shape[0] == 1 and B > 1:
                cond = cond.expand(B, -1, -1, -1)
            b = model.forward_raw(latents, t, prompt_embeds, akw.get("text_embeds"), akw.get("time_ids"), cond, shared_ctx=shared_ctx, split=split,
                                  out=out if block is None else None)
            block = b if block is None else block.add_(b) if block is out else block + b        # `samples_prev + samples_curr` in fp16 (:131-135)
        return block
