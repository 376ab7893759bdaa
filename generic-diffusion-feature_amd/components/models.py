"""Model registry of the native path — same entry point and version/dtype strings as the reference's
feature/components/models.py::get_diffusion_model (:10-175).

What is native here is the DENOISER (`pipe.unet` -> components.native.NativeUNet, libgdf.so).  Everything
upstream of the hot path (text encoders, VAE encoder, scheduler) is, as in the reference, whatever the
diffusers pipeline provides.  Offline (no diffusers, no checkpoints — the situation of the build and
benchmark boxes) `GDF_SYNTHETIC_WEIGHTS=1` selects a SyntheticPipe: seeded random UNet weights of the true
architecture plus deterministic stand-ins for prompt encoding / latent preparation, so the hot path can be
exercised and measured end to end.
"""
import hashlib
import math
import os
import types

import torch

from .native import (ARCH_CONFIGS, FLUX_CONFIGS, PIXART_CONFIGS, VAE_CONFIGS, NativeFluxTransformer, NativePixArtTransformer,
                     NativeUNet, NativeVAEDecoder, NativeVAEEncoder, config_from_diffusers)

# version -> (HF repo id, pipeline class name) exactly as the reference selects them (models.py:18-70)
_HF = {
    "1-5": ("stable-diffusion-v1-5/stable-diffusion-v1-5", "StableDiffusionImg2ImgPipeline"),
    "2-1": ("stabilityai/stable-diffusion-2-1-base", "StableDiffusionImg2ImgPipeline"),      # + EulerDiscreteScheduler (:38-39)
    "xl": ("stabilityai/stable-diffusion-xl-base-1.0", "StableDiffusionXLImg2ImgPipeline"),
    "pgv2": ("playgroundai/playground-v2-1024px-aesthetic", "StableDiffusionXLImg2ImgPipeline"),
}
_LATER = ("if", "hunyuan")                       # no BASELINE config (pixel-space UNet / untested DiT)


def _fill(model, loader):
    """Weights of a native model.  Single process — or a process group the launch did not opt in with (components/dist.py
    enable_weight_broadcast: extract_feature.py / bench.py under torchrun do) —: just `loader(model)` (checkpoint re-layout or
    synthetic init).  Data-parallel launch: rank 0 runs the loader, every other rank receives the flat device arena over RCCL
    (broadcast_model_weights; the arena sizes are checked to agree first)."""
    from . import dist as D
    if not D.weight_broadcast_enabled():
        loader(model)
        return model
    rank, _world = D.rank_world()
    if rank == 0:
        loader(model)
    return D.broadcast_model_weights(model)


def _parse_dtype(dtype):
    if dtype == 'float32':
        return torch.float32
    if dtype == 'float16':
        return torch.float16
    raise NotImplementedError                                    # reference models.py:11-16


class _Scheduler:
    """Minimal noise schedule (scaled-linear betas 0.00085..0.012, 1000 steps) for the synthetic pipe:
    DDPM-style variance-preserving add_noise for '1-5' (PNDM family, identity scale_model_input) and the
    sigma parameterisation for 'xl' (EulerDiscrete: x + sigma*noise, x/sqrt(sigma^2+1))."""

    def __init__(self, euler):
        betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float64) ** 2
        self.alphas_cumprod = torch.cumprod(1.0 - betas, 0).float()
        self.euler = euler
        self.timesteps = None

    def set_timesteps(self, n, device=None):
        self.timesteps = torch.arange(n - 1, -1, -1, device=device) * (1000 // n)

    def _sigma(self, t):
        ac = self.alphas_cumprod[int(t.flatten()[0])]
        return float(((1 - ac) / ac) ** 0.5)

    def scale_model_input(self, x, t):
        if not self.euler:
            return x
        return x / (self._sigma(t) ** 2 + 1) ** 0.5

    def add_noise(self, x, noise, t):
        a, b = self.noise_scalars(t)
        return a * x + b * noise

    def step_scalars(self, t):
        """(c_sample, c_eps) with step(eps, t, x).prev_sample = c_sample x + c_eps eps for the FIRST step after set_timesteps:
        PNDM's first step_plms call (eq. 9 of the PNDM paper with the model output as is) for '1-5', the Euler step
        x + (sigma_next - sigma) eps otherwise (epsilon prediction; un-vendored diffusers schedulers, oracle/vae_ref.py)."""
        ti = int(t.flatten()[0])
        if self.euler:
            idx = int((self.timesteps == ti).nonzero()[0]) if self.timesteps is not None else None
            nxt = int(self.timesteps[idx + 1]) if idx is not None and idx + 1 < len(self.timesteps) else -1
            acn = float(self.alphas_cumprod[nxt]) if nxt >= 0 else 1.0
            sig_next = ((1 - acn) / acn) ** 0.5 if nxt >= 0 else 0.0
            return 1.0, sig_next - self._sigma(t)
        step = 1000 // len(self.timesteps) if self.timesteps is not None else 1
        a_t = float(self.alphas_cumprod[ti])
        a_p = float(self.alphas_cumprod[ti - step]) if ti - step >= 0 else float(self.alphas_cumprod[0])
        den = a_t * (1 - a_p) ** 0.5 + (a_t * (1 - a_t) * a_p) ** 0.5
        return (a_p / a_t) ** 0.5, -(a_p - a_t) / den

    def step(self, model_output, t, sample, return_dict=False):
        a, b = self.step_scalars(t)
        return (a * sample + b * model_output,)

    def noise_scalars(self, t):
        """(noise_a, noise_b) with add_noise(x, n, t) = a x + b n."""
        ac = float(self.alphas_cumprod[int(t.flatten()[0])])
        if self.euler:
            return 1.0, self._sigma(t)
        return ac ** 0.5, (1 - ac) ** 0.5


def scheduler_noise_scalars(scheduler, timestep):
    """(a, b) such that scheduler.add_noise(x, noise, timestep) == a * x + b * noise for the call `prepare_latents` of the img2img pipelines makes
    (reference feature/diffusion_feature.py:371-380 -> diffusers prepare_latents -> scheduler.add_noise).  Schedulers that say so themselves
    (`noise_scalars`: the synthetic pipe's) are asked; a diffusers scheduler is PROBED on a deep copy with one-element CPU tensors — (x, noise) =
    (1, 0) and (0, 1), linearity verified on a third point — so every family the reference configures gives its own coefficients: PNDM / DDPM
    (sqrt(ac), sqrt(1 - ac); '1-5'), EulerDiscrete (1, sigma; '2-1', 'xl', 'pgv2': models.py:26,38,51), DPMSolverMultistep
    (alpha_t, sigma_t; the PixArt pipelines).  (Until round 6 this read `scheduler.sigmas` directly, which is the Euler rule — wrong for
    DPMSolverMultistep, which also has `sigmas` and `index_for_timestep`.)"""
    if hasattr(scheduler, "noise_scalars"):
        return scheduler.noise_scalars(timestep)
    import copy
    t1 = timestep.flatten()[:1] if torch.is_tensor(timestep) else torch.as_tensor([timestep])

    def probe(x, n):
        sch = copy.deepcopy(scheduler)
        one = lambda v: torch.full((1, 1, 1, 1), float(v), dtype=torch.float64)
        return float(sch.add_noise(one(x), one(n), t1.cpu()).flatten()[0])
    a, b = probe(1.0, 0.0), probe(0.0, 1.0)
    chk = probe(0.5, -2.0)
    if abs(chk - (0.5 * a - 2.0 * b)) > 1e-6 * (1.0 + abs(chk)):
        raise NotImplementedError("scheduler.add_noise is not linear in (sample, noise) for this scheduler configuration")
    return a, b


def scheduler_step_scalars(scheduler, timestep):
    """(c_sample, c_eps) such that `scheduler.step(noise_pred, timestep, latents)[0] == c_sample * latents + c_eps * noise_pred` for the
    call the reference makes at feature/diffusion_feature.py:478-480 (the first step after set_timesteps).  Schedulers that say so
    themselves (`step_scalars`) are asked; for a diffusers scheduler the two coefficients are PROBED on a deep copy with two
    one-element CPU tensors — (x, eps) = (1, 0) and (0, 1) — because the first PNDM / Euler step is linear in both (epsilon / v
    prediction without thresholding or clipping), which the probe verifies on a third point."""
    if hasattr(scheduler, "step_scalars"):
        return scheduler.step_scalars(timestep)
    import copy
    t0 = timestep.flatten()[0] if torch.is_tensor(timestep) else timestep

    def probe_on(dev, x, e):
        sch = copy.deepcopy(scheduler)
        t = t0.to(dev) if torch.is_tensor(t0) else t0
        out = sch.step(torch.full((1, 1, 1, 1), float(e), dtype=torch.float64, device=dev), t,
                       torch.full((1, 1, 1, 1), float(x), dtype=torch.float64, device=dev), return_dict=False)[0]
        return float(out.flatten()[0])

    def probe(x, e):
        try:
            return probe_on("cpu", x, e)                 # diffusers keeps sigmas / alphas_cumprod on the CPU
        except (RuntimeError, TypeError):
            if torch.is_tensor(t0) and t0.device.type != "cpu":
                return probe_on(t0.device, x, e)         # a scheduler whose tables live on the timestep's device
            raise
    a, b = probe(1.0, 0.0), probe(0.0, 1.0)
    chk = probe(0.5, -2.0)
    if abs(chk - (0.5 * a - 2.0 * b)) > 1e-6 * (1.0 + abs(chk)):
        raise NotImplementedError("scheduler.step is not linear in (sample, model_output) for this scheduler configuration; "
                                  "'vae-out' needs a linear first step (PNDM / EulerDiscrete as the reference configures them)")
    return a, b


def sampling_table(scheduler, num_inference_steps):
    """A scheduler's whole `set_timesteps(n)` ... `step` run as rows (timestep, c_in, c_sample, w0, w1, w2, w3, w4) for NativeUNet.sample, plus
    its init_noise_sigma (1.0 when it has none): forward k sees c_in[k] x_k at timestep[k], then
        x_{k+1} = c_sample[k] x_k + sum_{j<5} w_j[k] e_{k-j}                                   (e_i: the model output of call i).
    Works for every scheduler whose run is LINEAR in (x_0, e_0, ..., e_{K-1}) reaching back at most five UNet calls — DDIM, EulerDiscrete,
    PNDM / PLMS (four outputs, but its warm-up call at the repeated timestep is not among them, so call 4 reaches call 0), LMS,
    DPMSolverMultistep without thresholding — and needs none of their formulas: like scheduler_step_scalars it PROBES.
    On deep copies, after set_timesteps(n), the whole step chain runs in float64 on one-element tensors for the basis inputs x_0 = 1 with
    every e = 0 and e_i = 1 alone for each i, which gives x_k = A_k x_0 + sum_i B_{k,i} e_i; then
        c_sample[k] = A_{k+1} / A_k,      w_j[k] = B_{k+1,k-j} - c_sample[k] B_{k,k-j}.
    Every coefficient older than j = 4 must vanish (1e-9 of the row's largest) and one more chain on random inputs must follow the table;
    a scheduler that fails either check (ancestral and other stochastic ones, thresholding, more history) raises NotImplementedError.
    c_in[k] is `scale_model_input(1, t_k)`.  The timesteps are `scheduler.timesteps` as they stand: PNDM with skip_prk_steps lists its
    second timestep twice, which is two rows and two UNet calls.  K + 2 chains of K steps: milliseconds for the usual 20-50 steps."""
    import copy
    name = type(scheduler).__name__
    base = copy.deepcopy(scheduler)
    base.set_timesteps(int(num_inference_steps))
    ts = [t for t in base.timesteps]
    K = len(ts)
    if K < 1:
        raise ValueError("the scheduler has no timesteps")
    one = lambda v: torch.full((1, 1, 1, 1), float(v), dtype=torch.float64)

    def chain(x0, es):
        sch = copy.deepcopy(base)
        x, xs, cin = one(x0), [float(x0)], []
        for k, t in enumerate(ts):
            cin.append(float(sch.scale_model_input(one(1.0), t).flatten()[0]))
            x = sch.step(one(es[k]), t, x, return_dict=False)[0].double()
            xs.append(float(x.flatten()[0]))
        return xs, cin

    zeros = [0.0] * K
    A, c_in = chain(1.0, zeros)
    Bm = [chain(0.0, [1.0 if i == j else 0.0 for j in range(K)])[0] for i in range(K)]          # Bm[i][k] = B_{k,i}
    rows = []
    for k in range(K):
        if A[k] == 0.0:
            raise NotImplementedError(f"{name}: the sample's own coefficient vanishes at step {k}; no per-step table exists")
        cs = A[k + 1] / A[k]
        w = [Bm[k - j][k + 1] - cs * Bm[k - j][k] for j in range(k + 1)]
        top = max([abs(cs)] + [abs(v) for v in w])
        future = max([abs(Bm[i][k + 1]) for i in range(k + 1, K)] + [0.0])
        if any(abs(v) > 1e-9 * top for v in w[5:]) or future > 1e-9 * top:
            raise NotImplementedError(f"{name}: step {k} reaches back more than five UNet calls; NativeUNet.sample keeps five model outputs")
        w = (w + [0.0] * 5)[:5]
        rows.append((float(ts[k]), c_in[k], cs) + tuple(w))
    # the linearity check: one chain on random inputs against the table's recurrence, at every step
    g = torch.Generator().manual_seed(1234)
    x0 = float(torch.randn(1, generator=g, dtype=torch.float64))
    es = torch.randn(K, generator=g, dtype=torch.float64).tolist()
    xs, _ = chain(x0, es)
    x = x0
    for k in range(K):
        x = rows[k][2] * x + sum(rows[k][3 + j] * es[k - j] for j in range(min(5, k + 1)))
        if not abs(x - xs[k + 1]) <= 1e-6 * (1.0 + abs(xs[k + 1])):
            raise NotImplementedError(f"{name}: scheduler.step is not a fixed linear function of the sample and the model outputs (step {k}: "
                                      f"{xs[k + 1]!r} against {x!r} from the probed coefficients) — stochastic or thresholding schedulers cannot "
                                      "run as a device-resident table")
        x = xs[k + 1]
    return rows, float(getattr(base, "init_noise_sigma", 1.0))


def ddim_timesteps(config, num_inference_steps, num_train_timesteps=1000):
    """DDIMScheduler.set_timesteps(num_inference_steps).timesteps (descending ints) from the scheduler config alone — the published rule of
    diffusers' DDIMScheduler per `timestep_spacing` (Table 2 of arXiv 2305.08891), restated so that no diffusers install is needed; the class
    itself is used when it can be imported.  `config`: anything with attributes or keys (a missing entry takes DDIMScheduler's default)."""
    def cfg(name, default):
        if config is None:
            return default
        if isinstance(config, dict):
            return config.get(name, default)
        return getattr(config, name, default)
    T = int(cfg("num_train_timesteps", num_train_timesteps))
    offset = int(cfg("steps_offset", 0))
    spacing = cfg("timestep_spacing", "leading")
    n = int(num_inference_steps)
    if n < 1 or n > T:
        raise ValueError(f"num_inference_steps must be in [1, {T}]")
    try:
        from diffusers import DDIMScheduler
        sch = DDIMScheduler.from_config(config)
        sch.set_timesteps(n)
        return [int(v) for v in sch.timesteps]
    except Exception:                                                # not importable here, or a config the class does not take: the rule itself
        pass
    import numpy as np
    if spacing == "linspace":
        ts = np.linspace(0, T - 1, n).round()[::-1].astype(np.int64)
    elif spacing == "leading":
        ts = (np.arange(0, n) * (T // n)).round()[::-1].astype(np.int64) + offset
    elif spacing == "trailing":
        ts = np.round(np.arange(T, 0, -T / n)).astype(np.int64) - 1
    else:
        raise ValueError(f"unknown timestep_spacing {spacing!r}: 'leading', 'trailing' or 'linspace'")
    return [int(v) for v in ts]


def ddim_inversion_table(scheduler, num_inference_steps, stop_at_t):
    """The reference's DDIM inversion loop (feature/components/ddim_inversion.py:19-43) as rows (timestep, c_in, c_sample, c_eps) for
    NativeUNet.trajectory: the DDIM timesteps of `scheduler.config` reversed (ascending) and walked from index 1; at timestep t the UNet sees
    the latents as they are (c_in = 1: DDIM's scale_model_input is the identity, and the loop does not call it, :28-31) and
        current_t = max(0, t - 1000 // n), a_cur = alphas_cumprod[current_t], a_next = alphas_cumprod[t]
        latents = (latents - sqrt(1 - a_cur) eps) sqrt(a_next / a_cur) + sqrt(1 - a_next) eps                                  (:39-41)
                = c_sample latents + c_eps eps,   c_sample = sqrt(a_next / a_cur),  c_eps = sqrt(1 - a_next) - sqrt(1 - a_cur) c_sample;
    the loop ends after the first step with t >= stop_at_t (:42-43).  alphas_cumprod is the PIPELINE scheduler's (:35-36); a scheduler without a
    config (the synthetic pipes') takes DDIMScheduler's defaults over its own number of training steps.  Coefficients are computed in float64."""
    ac = scheduler.alphas_cumprod
    ac = ac.double().cpu().tolist() if torch.is_tensor(ac) else [float(v) for v in ac]
    n = int(num_inference_steps)
    stop = float(stop_at_t.flatten()[0]) if torch.is_tensor(stop_at_t) else float(stop_at_t)
    ts = ddim_timesteps(getattr(scheduler, "config", None), n, num_train_timesteps=len(ac))[::-1]
    rows = []
    for i in range(1, n):
        t = ts[i]
        a_cur, a_next = ac[max(0, t - 1000 // n)], ac[t]
        c_sample = (a_next / a_cur) ** 0.5
        rows.append((t, 1.0, c_sample, (1.0 - a_next) ** 0.5 - (1.0 - a_cur) ** 0.5 * c_sample))
        if t >= stop:
            break
    return rows


def native_vae_decoder(pipe, device):
    """The pipe's native AutoencoderKL decoder, created on first use (only a config that asks for 'vae-out' needs it)."""
    dec = getattr(pipe, "_native_vae_decoder", None)
    if dec is None:
        if getattr(pipe, "native_vae", None) is not None and not hasattr(pipe.vae, "state_dict"):      # synthetic pipe
            dec = _fill(NativeVAEDecoder(VAE_CONFIGS["sd"], device=device), lambda m: m.init_synthetic(getattr(pipe, "_seed", 0) + 2))
        else:
            vc = pipe.vae.config
            dec = NativeVAEDecoder(dict(in_channels=vc.in_channels, latent_channels=vc.latent_channels,
                                        block_out_channels=tuple(vc.block_out_channels), layers_per_block=vc.layers_per_block,
                                        use_quant_conv=int(getattr(vc, "use_post_quant_conv", getattr(vc, "use_quant_conv", True)))),
                                   device=device)
            _fill(dec, lambda m: m.load_vae_state_dict(pipe.vae.state_dict()))
        pipe._native_vae_decoder = dec
    return dec


def native_prepare_latents(pipe, image, timestep, batch_size, num_images_per_prompt, dtype, device, generator=None):
    """Drop-in for `StableDiffusion(XL)Img2ImgPipeline.prepare_latents` as the reference calls it
    (feature/diffusion_feature.py:371-380): VAE encode -> latent_dist.sample -> * scaling_factor -> scheduler.add_noise,
    executed by libgdf.so (include/gdf_vae.h); the random tensors come from torch exactly where the pipeline draws them."""
    enc = pipe.native_vae
    f = 1 << (len(enc.cfg["block_out_channels"]) - 1)
    B, _, H, W = image.shape
    shape = (B, enc.cfg["latent_channels"], H // f, W // f)
    eps = torch.randn(shape, generator=generator, device=device, dtype=torch.float32)
    noise = torch.randn(shape, generator=generator, device=device, dtype=torch.float32)
    a, b = scheduler_noise_scalars(pipe.scheduler, timestep)
    lat = enc.encode(image, eps=eps, noise=noise, scaling_factor=float(pipe.vae.config.scaling_factor), noise_a=a, noise_b=b)
    return lat.to(dtype)


def flux_native_vae_enabled():
    """GDF_FLUX_NATIVE_VAE=1: the Flux pipelines encode through the native 16-channel VAE (NativeVAEEncoder.encode_packed).  Off by default:
    the synthetic pipe's average-pool stand-in (and every figure recorded with it) stays what it was until a real checkpoint's full-size
    parity is on record."""
    return os.environ.get("GDF_FLUX_NATIVE_VAE", "0") not in ("", "0")


def flux_pack_index(L, h, w):
    """(L, h, w) long tensor: the flat position of latent (c, y, x) inside one image's packed (S, 4L) token block,
    (y//2 * (w//2) + x//2) * 4L + c*4 + (y%2)*2 + (x%2) — `FluxImg2ImgPipeline._pack_latents` as an index expression (the layout
    csrc/dit.hip vae_finish_packed_kernel writes)."""
    c = torch.arange(L).view(L, 1, 1)
    y = torch.arange(h).view(1, h, 1)
    x = torch.arange(w).view(1, 1, w)
    return ((y // 2) * (w // 2) + x // 2) * (4 * L) + c * 4 + (y % 2) * 2 + (x % 2)


def flux_scale_noise_sigma(scheduler, timestep):
    """The sigma `FlowMatchEulerDiscreteScheduler.scale_noise(sample, timestep, noise)` would use — it returns sigma * noise +
    (1 - sigma) * sample — as a host float, from the scheduler's own table.  The table INDEX is found the way scale_noise finds it, on the
    host: the begin index the pipeline's get_timesteps set (or the step index once stepping has begun); only a scheduler without one is
    searched for `timestep`.  The VALUE is the fp32 table entry, not its rounding to the latents' dtype.  A table the pipeline left on the
    CPU costs no device read; one it moved to the device (set_timesteps(device=...)) costs the 4-byte read of that one entry."""
    sig = scheduler.sigmas
    begin = getattr(scheduler, "begin_index", getattr(scheduler, "_begin_index", None))
    step = getattr(scheduler, "step_index", getattr(scheduler, "_step_index", None))
    if begin is None:
        t0 = timestep.flatten()[0] if torch.is_tensor(timestep) else timestep
        st = scheduler.timesteps
        idx = scheduler.index_for_timestep(t0.to(st.device) if torch.is_tensor(t0) else t0, st)
    else:
        idx = step if step is not None else begin
    return float(sig[int(idx)])


def native_flux_prepare_latents(pipe, image, timestep, batch_size, num_channels_latents, height, width, dtype, device, generator, latents=None):
    """Drop-in for `FluxImg2ImgPipeline.prepare_latents` (diffusers pipeline_flux_img2img.py: `_encode_vae_image` = (vae.encode(image)
    .sample() - shift_factor) * scaling_factor, `scheduler.scale_noise`, `_pack_latents`): one libgdf call (NativeVAEEncoder.encode_packed,
    include/gdf_vae.h gdf_vae_encode_packed).  Returns (packed latents (B, S, 4L), latent_image_ids).
    Random draws, in the pipeline's order: eps (the posterior sample of vae.encode, one row per IMAGE), then noise (randn_tensor, one row per
    batch entry); both fp32 on the device in the latent NCHW shape, from `generator`.  sigma: flux_scale_noise_sigma; noise_a = 1 - sigma,
    noise_b = sigma; shift_factor and scaling_factor from pipe.vae.config.  batch_size an integer multiple of the image count repeats the
    images (and their eps) as the pipeline's torch.cat does.
    dtype: the latents come out in the native transformer's 16-bit OPERAND type (fp16 under the default 'auto' mode) when that and `dtype`
    differ only by fp16 versus bf16.  Nothing between prepare_latents and the transformer does arithmetic on the latents — the pipeline hands
    them over as they are and NativeFluxTransformer casts them to its operand type first thing — so bf16 latents would only put a second,
    coarser rounding (8 bits, then 11) in front of the same operand; written in the operand type they are the fp32 value rounded once.  (The
    pipeline also casts the timestep to latents.dtype: fp16 holds sigma * 1000 more exactly than bf16.)  Any other `dtype` gets a plain cast.
    One exception: while the transformer's first-forward activation range check is still armed (a real checkpoint's first call,
    NativeFluxTransformer.arm_range_check) the operand type is not settled — that forward may re-load the model in 'bfloat16x2' — so that one
    call hands the latents over in `dtype`, the pipeline's bf16, which either outcome takes as it is (bf16 -> fp16 is exact from 2^-17 up):
    a model that falls back computes what one loaded in 'bfloat16x2' from the start computes, bit for bit."""
    if latents is not None:
        raise NotImplementedError("native_flux_prepare_latents: caller-supplied latents are not supported (the pipeline returns them unchanged; "
                                  "unset GDF_FLUX_NATIVE_VAE for that path)")
    if isinstance(generator, (list, tuple)):
        raise NotImplementedError("native_flux_prepare_latents: one generator for the whole batch")
    enc = pipe.native_vae
    L = enc.cfg["latent_channels"]
    if int(num_channels_latents) != L:
        raise ValueError(f"the transformer expects {num_channels_latents} latent channels, the VAE has {L}")
    f = 1 << (len(enc.cfg["block_out_channels"]) - 1)
    image = image.to(device)
    n_img, _, H, W = image.shape
    h, w = H // f, W // f
    if h % 2 or w % 2 or h * f != H or w * f != W:
        raise ValueError(f"image size {H}x{W} does not give an even latent grid")
    rep = 1
    if batch_size > n_img:
        if batch_size % n_img:
            raise ValueError(f"Cannot duplicate `image` of batch size {n_img} to {batch_size} text prompts.")
        rep = batch_size // n_img
    eps = torch.randn((n_img, L, h, w), generator=generator, device=device, dtype=torch.float32)
    noise = torch.randn((n_img * rep, L, h, w), generator=generator, device=device, dtype=torch.float32)
    if rep > 1:
        image, eps = image.repeat(rep, 1, 1, 1), eps.repeat(rep, 1, 1, 1)
    vc = pipe.vae.config
    sigma = flux_scale_noise_sigma(pipe.scheduler, timestep)
    tr = getattr(pipe, "transformer", None)
    io = getattr(tr, "io_dtype", None)
    sixteen = (torch.float16, torch.bfloat16)
    settled = io in sixteen and getattr(tr, "_range_check_sd", None) is None
    out_dtype = io if settled else (dtype if dtype in sixteen else torch.float16)
    tok = enc.encode_packed(image, eps=eps, noise=noise, scaling_factor=float(vc.scaling_factor),
                            shift_factor=float(getattr(vc, "shift_factor", None) or 0.0), sigma=sigma, out_dtype=out_dtype)
    if dtype not in sixteen:
        tok = tok.to(dtype)
    ids = pipe._prepare_latent_image_ids(n_img * rep, h // 2, w // 2, device, dtype)
    return tok, ids


def native_prepare_latents_multi(pipe, image, timesteps, batch_size, dtype, device, generator=None, schedulers=None):
    """`native_prepare_latents` for K timesteps of the same B images from ONE VAE encode (NativeVAEEncoder.encode_multi): returns
    (K*B, L, h, w) TIMESTEP-MAJOR — rows k*B:(k+1)*B are the B images noised for timesteps[k] (each entry what the single call takes: a
    one-element or (B,) tensor).
    The random draws are DEFINED as those of native_prepare_latents at batch K*B: eps = randn((K*B, L, h, w)), then noise = randn(...), both
    fp32 on the device, so every (image, timestep) row has its own posterior sample and its own noise, and the single call on the images
    tiled K times draws the same numbers.  (a, b) per timestep come from scheduler_noise_scalars: PNDM, Euler and DPM-Solver alike.
    schedulers: the scheduler object that PICKED timesteps[k], one per timestep (None: pipe.scheduler for all).  It matters: diffusers'
    img2img `get_timesteps` leaves `begin_index` on the scheduler it ran on, and Euler / DPM-Solver `add_noise` then reads the sigma AT
    that index whatever timestep it is given — asking one scheduler for all K timesteps would noise every row for the last one picked."""
    enc = pipe.native_vae
    f = 1 << (len(enc.cfg["block_out_channels"]) - 1)
    B, _, H, W = image.shape
    K = len(timesteps)
    shape = (K * B, enc.cfg["latent_channels"], H // f, W // f)
    eps = torch.randn(shape, generator=generator, device=device, dtype=torch.float32)
    noise = torch.randn(shape, generator=generator, device=device, dtype=torch.float32)
    if schedulers is not None and len(schedulers) != K:
        raise ValueError("schedulers must hold one scheduler per timestep")
    ab = [scheduler_noise_scalars(schedulers[k] if schedulers is not None else pipe.scheduler, t) for k, t in enumerate(timesteps)]
    lat = enc.encode_multi(image, eps=eps, noise=noise, scaling_factor=float(pipe.vae.config.scaling_factor),
                           noise_a=[a for a, _ in ab], noise_b=[b for _, b in ab], input_scale=[1.0] * K)
    return lat.to(dtype)


class SyntheticPipe:
    """Offline stand-in for the diffusers img2img pipeline object (`pipe`) used by FeatureExtractor."""
    synthetic_weights = True                      # seeded N(0, 1/fan_in) weights: the statistics the operand-plan table was made on

    def __init__(self, version, device, seed=0, stream_fp32=True):
        cfg = ARCH_CONFIGS[version]
        self.version = version
        self.device = device
        self._seed = seed
        self.unet = _fill(NativeUNet(cfg, device=device, stream_fp32=stream_fp32), lambda m: m.init_synthetic(seed))
        empty = types.SimpleNamespace(parameters=lambda: iter(()), to=lambda *a, **k: None)
        self.vae = types.SimpleNamespace(parameters=lambda: iter(()), config=types.SimpleNamespace(
            scaling_factor=0.13025 if cfg["addition_embed_text_time"] else 0.18215))
        # true-architecture AutoencoderKL encoder (seeded random weights) in libgdf.so: the step before the hot path
        self.native_vae = _fill(NativeVAEEncoder(VAE_CONFIGS["sd"], device=device), lambda m: m.init_synthetic(seed + 1))
        self.text_encoder = empty
        if cfg["addition_embed_text_time"]:
            pooled = cfg["add_in_dim"] - 6 * cfg["addition_time_embed_dim"]
            self.text_encoder_2 = types.SimpleNamespace(parameters=lambda: iter(()), to=lambda *a, **k: None,
                                                        config=types.SimpleNamespace(projection_dim=pooled))
        self.scheduler = _Scheduler(euler=bool(cfg["addition_embed_text_time"]) or version == "2-1")   # reference models.py:26,38,51
        self.config = types.SimpleNamespace(requires_aesthetics_score=False)
        self.image_processor = types.SimpleNamespace(preprocess=self._preprocess)
        self._cfg = cfg

    # -- upstream stand-ins (deterministic, NOT the real encoders) -------------------------------
    def _preprocess(self, img):
        import numpy as np
        imgs = img if isinstance(img, (list, tuple)) else [img]
        out = []
        for im in imgs:
            if torch.is_tensor(im):
                out.append(im.float()[None] if im.dim() == 3 else im.float())
            else:
                a = torch.from_numpy(np.asarray(im, dtype=np.float32) / 255.0).permute(2, 0, 1)[None]
                out.append(a * 2.0 - 1.0)
        return torch.cat(out, 0)

    def _embeds(self, text, shape):
        seed = int.from_bytes(hashlib.sha256(text.encode()).digest()[:4], "little")
        g = torch.Generator().manual_seed(seed)
        return torch.randn(shape, generator=g).to(self.device, torch.float16)

    def encode_prompt(self, prompt, device=None, num_images_per_prompt=1, negative_prompt='',
                      do_classifier_free_guidance=True):
        cd = self._cfg["cross_attention_dim"]
        pe, ne = self._embeds(prompt, (1, 77, cd)), self._embeds("neg:" + (negative_prompt or ''), (1, 77, cd))
        if self._cfg["addition_embed_text_time"]:
            pd = self._cfg["add_in_dim"] - 6 * self._cfg["addition_time_embed_dim"]
            return pe, ne, self._embeds("pool:" + prompt, (1, pd)), self._embeds("npool:", (1, pd))
        return pe, ne

    def get_timesteps(self, num_inference_steps, strength, device):
        init = min(int(num_inference_steps * strength), num_inference_steps)
        t_start = max(num_inference_steps - init, 0)
        ts = self.scheduler.timesteps[t_start:]
        return ts, num_inference_steps - t_start

    def prepare_latents(self, image, timestep, batch_size, num_images_per_prompt, dtype, device, generator=None):
        """prepare_latents of the img2img pipelines on the native VAE encoder (random-weight AutoencoderKL offline)."""
        g = generator or torch.Generator(device=device).manual_seed(1234)
        return native_prepare_latents(self, image.to(device), timestep, batch_size, num_images_per_prompt, dtype, device, g)

    def prepare_latents_multi(self, image, timesteps, batch_size, dtype, device, generator=None, schedulers=None):
        """prepare_latents for several timesteps of the same images (native_prepare_latents_multi); the same default generator."""
        g = generator or torch.Generator(device=device).manual_seed(1234)
        return native_prepare_latents_multi(self, image.to(device), timesteps, batch_size, dtype, device, g, schedulers)


class SyntheticPixartPipe(SyntheticPipe):
    """Offline stand-in for diffusers' PixArtSigmaPipeline as FeatureExtractor uses it: true-architecture DiT
    (NativePixArtTransformer, seeded random weights), native VAE encoder, stand-in T5 embeddings with a ragged mask."""

    def __init__(self, version, device, seed=0, cfg=None, n_txt=None):
        cfg = dict(cfg or PIXART_CONFIGS[version])
        alpha = version == "pixart-alpha"                         # PixArtAlphaPipeline: max_sequence_length 120, sd-vae-ft-ema
        n_txt = n_txt or (120 if alpha else 300)
        self.version = version
        self.device = device
        self._pcfg = cfg
        self.n_txt = n_txt
        self.transformer = _fill(NativePixArtTransformer(cfg, device=device), lambda m: m.init_synthetic(seed))
        self.unet = self.transformer               # reference models.py:91 `pipe.unet = pipe.transformer`
        empty = types.SimpleNamespace(parameters=lambda: iter(()), to=lambda *a, **k: None)
        self.vae = types.SimpleNamespace(parameters=lambda: iter(()), config=types.SimpleNamespace(scaling_factor=0.18215 if alpha else 0.13025))
        self.native_vae = _fill(NativeVAEEncoder(VAE_CONFIGS["sd"], device=device), lambda m: m.init_synthetic(seed + 1))
        self.text_encoder = empty
        self.scheduler = _Scheduler(euler=False)
        self.config = types.SimpleNamespace(requires_aesthetics_score=False)
        self.image_processor = types.SimpleNamespace(preprocess=self._preprocess)

    def encode_prompt(self, prompt, device=None, num_images_per_prompt=1, negative_prompt='',
                      do_classifier_free_guidance=True, **kw):
        """(prompt_embeds, prompt_attention_mask, negative_prompt_embeds, negative_prompt_attention_mask) — PixArt order."""
        cc = self._pcfg["caption_channels"]
        n_valid = max(1, min(self.n_txt, len(prompt.split()) + 2))
        mask = (torch.arange(self.n_txt, device=self.device)[None] < n_valid).to(torch.int64)
        return self._embeds(prompt, (1, self.n_txt, cc)), mask, self._embeds("neg:", (1, self.n_txt, cc)), torch.ones_like(mask)


class SyntheticFluxPipe:
    """Offline stand-in for the reference's PATCHED FluxImg2ImgPipeline as `FeatureExtractor.extract` drives it
    (`pipe(image=..., prompt=..., strength=t/1000, guidance_scale=1)`, diffusion_feature.py:246-254): true-architecture
    MMDiT (NativeFluxTransformer, seeded random weights) + deterministic stand-ins for the T5/CLIP encoders and the
    16-channel VAE, flow-matching sigmas with the resolution-dependent shift, 2x2 latent packing and the img2img
    strength -> timestep rule.  Like the reference's pipeline (feature/diffusers/pipelines/flux/pipeline_flux_img2img.py:
    804-841: `return` at the end of the FIRST loop iteration) one call runs EXACTLY ONE transformer forward, at
    sigmas[t_start], and returns None."""
    synthetic_weights = True

    num_inference_steps = 28                      # FluxImg2ImgPipeline.__call__ default
    returns_after_first_forward = True            # like the reference's patched pipeline (:841)
    # FlowMatchEulerDiscreteScheduler config of black-forest-labs/FLUX.1-dev (scheduler/scheduler_config.json) [memory]
    sched_cfg = dict(base_image_seq_len=256, max_image_seq_len=4096, base_shift=0.5, max_shift=1.15)

    def __init__(self, device, seed=0, cfg=None, n_txt=512):
        self.device = device
        self._cfg = dict(cfg or FLUX_CONFIGS["flux"])
        self.n_txt = n_txt
        self.transformer = _fill(NativeFluxTransformer(self._cfg, device=device, compute_dtype=flux_compute_dtype()), lambda m: m.init_synthetic(seed))
        self.unet = self.transformer               # reference models.py:169 `pipe.unet = pipe.transformer`
        empty = types.SimpleNamespace(parameters=lambda: iter(()), to=lambda *a, **k: None)
        self.vae = types.SimpleNamespace(parameters=lambda: iter(()), config=types.SimpleNamespace(scaling_factor=0.3611, shift_factor=0.1159))
        self.text_encoder = empty
        self.text_encoder_2 = empty
        self.scheduler = types.SimpleNamespace()
        self.image_processor = types.SimpleNamespace(preprocess=SyntheticPipe._preprocess.__get__(self))
        self.last_call = None                      # (sigma, packed latents, prompt embeds, ...) of the last call: test / debugging aid
        # GDF_FLUX_NATIVE_VAE=1: the true-architecture 16-channel encoder (seeded random weights) in place of the average-pool stand-in
        self.native_vae = None
        if flux_native_vae_enabled():
            self.native_vae = _fill(NativeVAEEncoder(VAE_CONFIGS["flux"], device=device), lambda m: m.init_synthetic(seed + 1))

    def _embeds(self, text, shape):
        seed = int.from_bytes(hashlib.sha256(text.encode()).digest()[:4], "little")
        return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(self.device, torch.float16)

    def sigmas(self, n_steps, image_seq_len):
        """pipeline_flux_img2img.py:744-760: sigmas = linspace(1, 1/N, N), shifted by mu = calculate_shift(image_seq_len, ...)
        (`time_shift`: exp(mu) / (exp(mu) + (1/sigma - 1)), FlowMatchEulerDiscreteScheduler with dynamic shifting), + final 0."""
        c = self.sched_cfg
        m = (c["max_shift"] - c["base_shift"]) / (c["max_image_seq_len"] - c["base_image_seq_len"])
        mu = image_seq_len * m + (c["base_shift"] - m * c["base_image_seq_len"])
        s = torch.linspace(1.0, 1.0 / n_steps, n_steps, dtype=torch.float64)
        s = math.exp(mu) / (math.exp(mu) + (1.0 / s - 1.0))
        return s.tolist() + [0.0]

    def __call__(self, image=None, prompt=None, strength=0.6, guidance_scale=7.0, num_inference_steps=None, **kw):
        dev = self.device
        imgs = image if isinstance(image, (list, tuple)) else [image]
        x = torch.cat([self.image_processor.preprocess(i) for i in imgs], 0).to(dev, torch.float32)
        B = x.shape[0]
        prompts = prompt if isinstance(prompt, (list, tuple)) else [prompt] * B
        enc = torch.cat([self._embeds(p, (1, self.n_txt, self._cfg["joint_attention_dim"])) for p in prompts], 0)
        pooled = torch.cat([self._embeds("pool:" + p, (1, self._cfg["pooled_projection_dim"])) for p in prompts], 0)
        native = self.native_vae is not None
        Bc, Cc, H, W = B, 16, x.shape[2] // 8, x.shape[3] // 8
        if not native:
            # synthetic 16-channel 'VAE encode' (8x8 average pooling + fixed channel mix), then 2x2 packing -> (B, S, 64)
            lat = torch.nn.functional.avg_pool2d(x, 8)
            mix = torch.linspace(-1.0, 1.0, 48, device=dev).reshape(16, 3)
            lat = torch.einsum("oc,bchw->bohw", mix, lat) * 2.0
            Bc, Cc, H, W = lat.shape
        gh, gw = H // 2, W // 2
        pack = lambda z: z.view(Bc, Cc, gh, 2, gw, 2).permute(0, 2, 4, 1, 3, 5).reshape(Bc, gh * gw, Cc * 4)
        # img2img schedule (get_timesteps, :606-616): the last int(N * strength) steps remain; only the FIRST of them is run
        N = num_inference_steps or self.num_inference_steps
        sigmas = self.sigmas(N, gh * gw)
        init = min(N * strength, N)
        t_start = int(max(N - init, 0))
        if N - t_start < 1:
            raise ValueError(f"After adjusting the num_inference_steps by strength parameter: {strength}, the number of "
                             f"pipeline steps is {N - t_start} which is < 1 and not appropriate for this pipeline.")
        s0 = sigmas[t_start]
        if native:
            # encode + posterior sample + (z - shift) * scaling + scale_noise + packing in ONE libgdf call, written in the transformer's
            # operand type; draws: eps, then noise (native_flux_prepare_latents), from the stand-in path's fixed seed
            g = torch.Generator(device=dev).manual_seed(1234)
            eps = torch.randn((Bc, Cc, H, W), generator=g, device=dev)
            noise = torch.randn((Bc, Cc, H, W), generator=g, device=dev)
            z = self.native_vae.encode_packed(x, eps=eps, noise=noise, scaling_factor=self.vae.config.scaling_factor,
                                              shift_factor=self.vae.config.shift_factor, sigma=s0, out_dtype=self.transformer.io_dtype)
        else:
            noise = torch.randn(lat.shape, generator=torch.Generator(device=dev).manual_seed(1234), device=dev)
            z = pack((1.0 - s0) * lat + s0 * noise)                  # FlowMatchEulerDiscreteScheduler.scale_noise
        img_ids = torch.zeros(gh, gw, 3, device=dev)
        img_ids[..., 1] = torch.arange(gh, device=dev)[:, None]; img_ids[..., 2] = torch.arange(gw, device=dev)[None, :]
        img_ids = img_ids.reshape(gh * gw, 3)
        txt_ids = torch.zeros(self.n_txt, 3, device=dev)
        guidance = torch.full((B,), float(guidance_scale), device=dev) if self._cfg["guidance_embeds"] else None
        t = torch.full((B,), s0, device=dev)                          # the pipeline passes timestep / 1000 = sigma (:816)
        self.last_call = dict(sigma=s0, t_start=t_start, hidden_states=z, encoder_hidden_states=enc, pooled_projections=pooled,
                              img_ids=img_ids, txt_ids=txt_ids, guidance=guidance, grid=(gh, gw))
        # ONE denoiser forward through the model's __call__ (it delivers the hooks to the FeatureStore), then return like the
        # reference's patched loop does (:841) — no scheduler.step, no further steps, no VAE decode
        self.transformer(hidden_states=z, timestep=t, guidance=guidance, pooled_projections=pooled, encoder_hidden_states=enc,
                         txt_ids=txt_ids, img_ids=img_ids, joint_attention_kwargs=None, return_dict=False, grid=(gh, gw))
        return None


def flux_compute_dtype():
    """Arithmetic of the Flux transformer behind FeatureExtractor: 'auto' (round 5 default: fp16 operands with range scaling, every hook within
    1e-3 of the fp32 reference at the bf16 mode's speed; NativeFluxTransformer) unless GDF_FLUX_DTYPE names another mode ('bfloat16' = the
    reference's own dtype, 'bfloat16x2', 'float16', 'fp8-mx')."""
    return os.environ.get("GDF_FLUX_DTYPE", "") or "auto"


def flux_config_from_diffusers(c):
    """FluxTransformer2DModel `.config` -> the fields of FLUX_CONFIGS"""
    return dict(in_channels=c.in_channels, num_layers=c.num_layers, num_single_layers=c.num_single_layers,
                attention_head_dim=c.attention_head_dim, num_attention_heads=c.num_attention_heads,
                joint_attention_dim=c.joint_attention_dim, pooled_projection_dim=c.pooled_projection_dim,
                guidance_embeds=int(bool(c.guidance_embeds)), axes_dims_rope=tuple(c.axes_dims_rope), mlp_ratio=4)


def _native_flux_from_diffusers(pipe, device):
    """Swap pipe.transformer (diffusers FluxTransformer2DModel, bf16) for the native MMDiT with the same weights."""
    cfg = flux_config_from_diffusers(pipe.transformer.config)
    net = NativeFluxTransformer(cfg, device=device, compute_dtype=flux_compute_dtype())
    sd = pipe.transformer.state_dict()
    _fill(net, lambda m: m.load_state_dict(sd))
    # the fp16 modes ('auto' -> 'float16s') were validated on seeded synthetic weights; the load-time guard only looks at WEIGHT
    # cast error.  A real checkpoint additionally gets an ACTIVATION range check on its first forward (NativeFluxTransformer.arm_range_check):
    # a saturated / non-finite 16-bit tensor anywhere in the model re-loads these weights in 'bfloat16x2' (bf16's range, the reference's dtype
    # as operand pairs) with one warning.  The state dict is held until that forward has run.
    net.arm_range_check(sd)
    pipe.transformer = net
    pipe.unet = net
    if flux_native_vae_enabled():
        _native_flux_vae_from_diffusers(pipe, device)
    return pipe


def _native_flux_vae_from_diffusers(pipe, device):
    """GDF_FLUX_NATIVE_VAE=1: pipe.native_vae = the 16-channel AutoencoderKL encoder half in libgdf.so with pipe.vae's weights (filled like the
    UNet versions' VAE: _fill, i.e. rank 0 loads and broadcasts under a data-parallel launch); pipe.prepare_latents =
    native_flux_prepare_latents, bound to a weak proxy for the reason given in _native_vae_from_diffusers."""
    vc = pipe.vae.config
    enc = NativeVAEEncoder(dict(in_channels=vc.in_channels, latent_channels=vc.latent_channels,
                                block_out_channels=tuple(vc.block_out_channels), layers_per_block=vc.layers_per_block,
                                use_quant_conv=int(getattr(vc, "use_quant_conv", True))), device=device)
    _fill(enc, lambda m: m.load_vae_state_dict(pipe.vae.state_dict()))
    pipe.native_vae = enc
    import weakref
    pipe.prepare_latents = types.MethodType(native_flux_prepare_latents, weakref.proxy(pipe))
    return pipe


def pixart_config_from_diffusers(c):
    """PixArtTransformer2DModel / Transformer2DModel `.config` -> the fields of PIXART_CONFIGS (interpolation_scale None = diffusers' default
    max(sample_size // 64, 1))"""
    ss = int(c.sample_size)
    isc = getattr(c, "interpolation_scale", None)
    if getattr(c, "use_additional_conditions", None):
        raise NotImplementedError("PixArt-alpha micro-conditioning (use_additional_conditions) is not native")
    return dict(num_attention_heads=int(c.num_attention_heads), attention_head_dim=int(c.attention_head_dim), in_channels=int(c.in_channels),
                out_channels=int(c.out_channels), num_layers=int(c.num_layers), patch_size=int(c.patch_size), sample_size=ss,
                caption_channels=int(c.caption_channels), interpolation_scale=int(isc) if isc is not None else max(ss // 64, 1))


def _img2img_get_timesteps(self, num_inference_steps, strength, device, denoising_start=None):
    """`get_timesteps` of the img2img pipelines, for pipelines that do not have one: the STOCK PixArt pipelines are text-to-image (the reference
    carries patched copies that add this method and an image-taking prepare_latents: feature/diffusers/pipelines/pixart_alpha/
    pipeline_pixart_sigma.py:598-700).  Same rule: the last int(N * strength) steps remain."""
    init_timestep = min(int(num_inference_steps * strength), num_inference_steps)
    t_start = max(num_inference_steps - init_timestep, 0)
    order = getattr(self.scheduler, "order", 1)
    timesteps = self.scheduler.timesteps[t_start * order:]
    if hasattr(self.scheduler, "set_begin_index"):
        self.scheduler.set_begin_index(t_start * order)
    return timesteps, num_inference_steps - t_start


def _native_vae_from_diffusers(pipe, device):
    """pipe.native_vae = the AutoencoderKL encoder half in libgdf.so with pipe.vae's weights; pipe.prepare_latents = native_prepare_latents,
    pipe.prepare_latents_multi = native_prepare_latents_multi"""
    vc = pipe.vae.config
    enc = NativeVAEEncoder(dict(in_channels=vc.in_channels, latent_channels=vc.latent_channels,
                                block_out_channels=tuple(vc.block_out_channels), layers_per_block=vc.layers_per_block,
                                use_quant_conv=int(getattr(vc, "use_quant_conv", True))), device=device)
    _fill(enc, lambda m: m.load_vae_state_dict(pipe.vae.state_dict()))
    pipe.native_vae = enc
    # (bound to a weak proxy: `pipe.prepare_latents = MethodType(f, pipe)` would make the pipeline a reference cycle, and a cycle is freed by the
    #  cyclic collector at an arbitrary later allocation — in whatever thread that happens to run — together with its multi-GB device arenas)
    import weakref
    pipe.prepare_latents = types.MethodType(native_prepare_latents, weakref.proxy(pipe))
    pipe.prepare_latents_multi = types.MethodType(native_prepare_latents_multi, weakref.proxy(pipe))
    return pipe


def _native_from_diffusers(pipe, device):
    """Swap pipe.unet (diffusers UNet2DConditionModel) for the native implementation with the same weights."""
    cfg = getattr(pipe, "_gdf_unet_config", None) or config_from_diffusers(pipe.unet.config)   # ranks > 0 may have no UNet module
    unet = NativeUNet(cfg, device=device)
    _fill(unet, lambda m: m.load_state_dict(pipe.unet.state_dict()))
    pipe.unet = unet
    # the step before the hot path: VAE encode + sample + noise-add in libgdf.so as well.
    # GDF_NATIVE_VAE=0 keeps diffusers' prepare_latents (e.g. the original SDXL VAE, whose activations need fp32).
    if os.environ.get("GDF_NATIVE_VAE", "1") not in ("", "0"):
        _native_vae_from_diffusers(pipe, device)
    return pipe


def _model_id(repo, offline_lora, offline_lora_filename):
    """The reference's rule for every version (feature/components/models.py:21-22, 33-34, 46-47, 60-61, 74-75, 90-91, 106-107, 153-154):
    `offline_lora` WITHOUT a file name is a local model directory that replaces the hub id; with a file name it is a LoRA that
    diffusion_feature.py:50-52 loads on top of the hub model."""
    return offline_lora if (offline_lora and not offline_lora_filename) else repo


def get_diffusion_model(version, dtype, offline_lora=None, offline_lora_filename=None, device="cuda"):
    dt = _parse_dtype(dtype)
    if version in _LATER:
        raise NotImplementedError(f"version '{version}' is not on the native hot path yet (SURVEY.md §8f / Appendix D)")
    synthetic = os.environ.get("GDF_SYNTHETIC_WEIGHTS", "0") not in ("", "0")
    if version == "flux":                                         # reference models.py:150-170 (bf16 pipeline, fp16 hooks)
        if synthetic:
            return SyntheticFluxPipe(device, seed=int(os.environ.get("GDF_SYNTHETIC_SEED", "0")))
        try:
            import diffusers
        except ImportError as e:
            raise RuntimeError("diffusers is not installed and GDF_SYNTHETIC_WEIGHTS is not set (see INTEGRATION.md)") from e
        pipe = diffusers.FluxImg2ImgPipeline.from_pretrained(_model_id('black-forest-labs/FLUX.1-dev', offline_lora, offline_lora_filename),
                                                             torch_dtype=torch.bfloat16, use_safetensors=True)
        if offline_lora and offline_lora_filename:
            pipe.load_lora_weights(offline_lora, weight_name=offline_lora_filename)
            pipe.fuse_lora()
        return _native_flux_from_diffusers(pipe.to(device), device)
    if version in PIXART_CONFIGS:                                 # reference models.py:72-111 (PixArtSigmaPipeline)
        if synthetic:
            return SyntheticPixartPipe(version, device, seed=int(os.environ.get("GDF_SYNTHETIC_SEED", "0")))
        try:
            import diffusers
        except ImportError as e:
            raise RuntimeError("diffusers is not installed and GDF_SYNTHETIC_WEIGHTS is not set (see INTEGRATION.md)") from e
        if version == "pixart-alpha":                             # reference models.py:103-115 (120-token T5 captions, SD VAE)
            pipe = diffusers.PixArtAlphaPipeline.from_pretrained(_model_id("PixArt-alpha/PixArt-XL-2-512x512", offline_lora, offline_lora_filename),
                                                                 torch_dtype=dt, variant="fp16", use_safetensors=True).to(device)
        else:
            repo = "PixArt-alpha/PixArt-Sigma-XL-2-1024-MS" if version == "pixart-sigma" else "PixArt-alpha/PixArt-Sigma-XL-2-512-MS"
            pipe = diffusers.PixArtSigmaPipeline.from_pretrained(_model_id(repo, offline_lora, offline_lora_filename), torch_dtype=dt,
                                                                 use_safetensors=True).to(device)
        if offline_lora and offline_lora_filename:                # reference diffusion_feature.py:50-52 (every version); fused: the weights are read next
            pipe.load_lora_weights(offline_lora, weight_name=offline_lora_filename)
            pipe.fuse_lora()
        # the architecture comes from the LOADED module (PIXART_CONFIGS holds the same numbers for the synthetic pipes)
        net = NativePixArtTransformer(pixart_config_from_diffusers(pipe.transformer.config), device=device)
        _fill(net, lambda m: m.load_state_dict({k: v for k, v in pipe.transformer.state_dict().items() if k != "pos_embed.pos_embed"}))
        pipe.transformer = pipe.unet = net
        # a STOCK diffusers PixArt pipeline is text-to-image: no `get_timesteps`, no image-taking `prepare_latents` (the reference patches both
        # in).  Round 6: the img2img front half is supplied here — the native VAE encoder + scheduler.add_noise for prepare_latents (unless
        # GDF_NATIVE_VAE=0 and the installed pipeline is the reference's patched one), the img2img rule for get_timesteps
        if os.environ.get("GDF_NATIVE_VAE", "1") not in ("", "0"):
            _native_vae_from_diffusers(pipe, device)
        if not hasattr(pipe, "get_timesteps"):
            import weakref
            pipe.get_timesteps = types.MethodType(_img2img_get_timesteps, weakref.proxy(pipe))
        return pipe
    if version not in _HF:
        raise NotImplementedError                                 # reference models.py:173-174
    if synthetic:
        return SyntheticPipe(version, device, seed=int(os.environ.get("GDF_SYNTHETIC_SEED", "0")))
    try:
        import diffusers
    except ImportError as e:
        raise RuntimeError("diffusers is not installed and GDF_SYNTHETIC_WEIGHTS is not set: the text encoders / VAE / "
                           "checkpoint loading upstream of the native UNet come from diffusers (see INTEGRATION.md)") from e
    repo, cls = _HF[version]
    # reference models.py:51-53, 65-67: 'xl' / 'pgv2' load the fp16 VARIANT whatever `dtype` says (dtype='float32' upcasts those fp16 weights: the
    # native arena then holds them exactly, and the float32 mode's full-split plan is 2-3e-4 from the reference's fp32 evaluation)
    kw = dict(variant="fp16") if version in ("xl", "pgv2") else {}
    from . import dist as D
    rank, world = D.rank_world()
    # data-parallel launch (opt-in, see _fill): only rank 0 reads the 5 GB UNet checkpoint, the other ranks receive the re-laid-out
    # arena.  With an offline LoRA every rank loads its own UNet instead: load_lora_weights / fuse_lora need the module, and each
    # rank fuses the same weights (the broadcast then only overwrites them with rank 0's identical arena).
    lora = bool(offline_lora and offline_lora_filename)
    skip_unet = D.weight_broadcast_enabled() and rank != 0 and not lora
    if skip_unet:
        kw["unet"] = None
    model_id = _model_id(repo, offline_lora, offline_lora_filename)
    if version == "2-1":
        # reference models.py:38-39: ONLY '2-1' swaps the scheduler (Euler made from the checkpoint's own scheduler config); 'xl' / 'pgv2' / '1-5'
        # keep whatever scheduler their checkpoint names — the probes (scheduler_noise_scalars / scheduler_step_scalars) ask the OBJECT
        kw["scheduler"] = diffusers.EulerDiscreteScheduler.from_pretrained(model_id, subfolder="scheduler")
    pipe = getattr(diffusers, cls).from_pretrained(model_id, torch_dtype=dt, use_safetensors=True, **kw)
    if lora:                                                      # reference diffusion_feature.py:50-52
        pipe.load_lora_weights(offline_lora, weight_name=offline_lora_filename)
        pipe.fuse_lora()
    # the architecture descriptor comes from rank 0's LOADED module (constructor defaults filled in: the raw config.json of SD1.5 /
    # SD2.1 lacks `transformer_layers_per_block`, SD1.5's also `use_linear_projection`) and is sent to the ranks without a UNet
    cfg = config_from_diffusers(pipe.unet.config) if pipe.unet is not None else None
    if D.weight_broadcast_enabled():
        cfg = D.broadcast_object(cfg, src=0)
    pipe._gdf_unet_config = cfg
    pipe = pipe.to(device)
    return _native_from_diffusers(pipe, device)
