"""`diffusion_feature.FeatureExtractor` — drop-in for the reference's public API
(/root/reference/feature/diffusion_feature.py:26-527) with the denoiser forward executed by
hand-written HIP kernels for MI355X (libgdf.so) instead of patched diffusers modules.

Kept verbatim: constructor keywords (:27-40), `encode_prompt` (:149-206) 4-tuple contract,
`extract` signature and return contract (:222-235, :517) — dict[layer_id -> (B,C,H,W) fp16 tensor] in hook
execution order —, `preprocess_image`, `offload_prompt_encoder`, background-extraction accessors,
the layer-selection config surface (JSON path | dict | None) and the version / dtype strings.
In scope are the single-timestep path and, for the UNet versions, `use_ddim_inversion` (the inversion steps run as one device-resident
trajectory, NativeUNet.trajectory) and `generate`: a classifier-free-guided text-to-image run with background extraction — the hooked
layers keep the features of the UNet calls named by `set_background_extraction` (reference generate_with_extraction.py) — as one
device-resident run (NativeUNet.sample), and `control=` / `use_control`: ControlNet conditioning of the extraction forward with the
ControlNet itself a native model (components/control.py, NativeControlNet) and the Canny preprocessor in front of it a device kernel
(csrc/canny.hip), and `t=[t1, ..., tK]`: K timesteps of the same images from one VAE encode and one UNet forward of K*B rows
(_extract_multi, split_timesteps), and `device_preprocess=`: the PIL-to-tensor step in front of all of it as device kernels
(components/preproc.py, csrc/preproc.hip).  `denoising_from` is not.
"""
import copy
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from components.models import get_diffusion_model
from components.feature_extractor import (ATTENTION_CATEGORIES, aggregate_attention, attention_map_ids,
                                          dit_attention_map_ids, prepare_feature_extractor)


_PRE_POOL = None


def _map_threads(fn, items):
    """[fn(x) for x in items] on a small thread pool: preprocess_image is a PIL resize + a float conversion per image (20-45 ms at 1024^2, both release the GIL);
    the reference's serial list comprehension (:358-364) leaves the GPU idle for 0.3-0.7 s per batch of 16.  Same results, same order.
    GDF_PREPROCESS_THREADS=0 restores the serial loop."""
    global _PRE_POOL
    n = int(os.environ.get("GDF_PREPROCESS_THREADS", "-1"))
    n = min(8, os.cpu_count() or 1) if n < 0 else n
    if n <= 1 or len(items) <= 1:
        return [fn(x) for x in items]
    if _PRE_POOL is None:
        from concurrent.futures import ThreadPoolExecutor
        _PRE_POOL = ThreadPoolExecutor(max_workers=n, thread_name_prefix="gdf-pre")
    return list(_PRE_POOL.map(fn, items))


class FeatureExtractor(nn.Module):
    def __init__(self,
                 layer,            # filename of the layer json, a pre-loaded dict, or None (= all layers)
                 version,          # '1-5', '2-1', 'xl', 'pgv2', 'flux', 'pixart-sigma', 'pixart-sigma-512', 'pixart-alpha'
                 device,
                 dtype='float16',  # 'float32': the front-end modules in fp32 and the UNet on the full-split operand plan (see `precise`)
                 img_size=1024,    # 512 for 1-5, 1024 otherwise
                 offline_lora=None,
                 offline_lora_filename=None,
                 feature_resize=1,
                 control=None,
                 attention=None,
                 train_unet=False,
                 external_model=None,
                 precise=None,     # native extension: operand plan of the UNet versions — None = 'auto' (the cheapest plan level that keeps
                                   # every REQUESTED layer within 1e-3 of the fp32 reference: plain fp16 operands / the selective split /
                                   # the full split), False = plain, True = full split, 'selective', or a class list ('stream,attn_out')
                 verify=None,      # native extension (None = ON for real checkpoints, OFF for GDF_SYNTHETIC_WEIGHTS pipelines; GDF_VERIFY=0/1 overrides):
                                   # True = runtime self-check of the automatic operand plan on the first batch of
                                   # every layer set: the chosen level and the full split are both run, the requested layers compared, and the level
                                   # escalated (with one warning) when any differs by more than the family's acceptance bound (d^2 + e_full^2 <= (0.97e-3)^2) — the plan chooser's error table comes from
                                   # synthetic weight statistics, real checkpoints may be heavier-tailed (components/native.py _verify_level)
                 early_exit=False, # native extension, OPT-IN: stop the denoiser forward after the last requested layer (the reference always runs the
                                   # whole forward and discards `noise_pred`; the returned features are bit-identical either way).  Ignored when
                                   # 'vae-out' (which needs the model output) is requested
                 device_preprocess=None,  # native extension, OPT-IN (UNet and PixArt versions): the PIL-to-tensor step of image_type='image' on the
                                   # device — the images' bytes are uploaded as uint8 and Pillow's bicubic resize, convert("RGB") and the normalisation run
                                   # as kernels (components/preproc.py, csrc/preproc.hip), bit for bit what preprocess_image gives.  None reads
                                   # GDF_DEVICE_PREPROCESS (default off); True needs a HIP device
                 ):
        super().__init__()
        from components.preproc import resolve_flag
        self.device_preprocess = resolve_flag(device_preprocess, device)                  # (True on a device that is not a HIP one raises, before anything loads)
        if control and (version == 'flux' or version.startswith('pixart')):
            raise NotImplementedError("control= exists for the UNet versions ('1-5', '2-1', 'xl', 'pgv2') only: the native ControlNet is the "
                                      "encoder half of a UNet (include/gdf_control.h)")
        if attention:
            bad = [a for a in attention if a not in ATTENTION_CATEGORIES]
            if bad:
                raise ValueError(f"unknown attention categories {bad}; choose from {ATTENTION_CATEGORIES}")
        if train_unet:
            raise NotImplementedError("the native denoiser is inference-only (no backward kernels)")
        if external_model:
            pipe = external_model
        else:
            pipe = get_diffusion_model(version, dtype, offline_lora, offline_lora_filename, device=device)

        self.feature_store = prepare_feature_extractor(version, pipe, layer, feature_resize, train_unet)
        self.store_vae_output = bool(self.feature_store.to_store.get('vae-out', False))          # reference :60
        if self.store_vae_output and (version == 'flux' or version.startswith('pixart')):
            # reference: the flux branch returns before the decode (:246-254); for PixArt `scheduler.step` would receive the
            # transformer's 8-channel output (learned sigma) against 4-channel latents (:466-480) — there is no working behaviour to match
            raise NotImplementedError("'vae-out' exists for the UNet versions ('1-5', '2-1', 'xl', 'pgv2') only")

        if self.store_vae_output:
            # built HERE, on every rank: under a data-parallel launch its weight fill is a collective (components/dist.py), and a rank
            # whose image shard is empty never reaches extract()
            from components.models import native_vae_decoder
            native_vae_decoder(pipe, device)
        if early_exit and not self.store_vae_output and hasattr(pipe.unet, "early_exit"):
            pipe.unet.early_exit = True
        if hasattr(pipe.unet, "_verify_level"):
            # verify=None: ON for real checkpoints (their weight statistics are not the synthetic ones the plan chooser's table was made on:
            # heavy-tailed weights put the plain plan at 1.8e-3 where the table says 9e-4, profiles/r05_heavy_tailed_plan_levels.txt), OFF for
            # the seeded synthetic pipelines (the table's own statistics, asserted per hook in tests/test_gpu_fullsize.py); GDF_VERIFY=0 / 1 overrides
            env = os.environ.get("GDF_VERIFY", "")
            if verify is None:
                verify = (env not in ("", "0")) if env != "" else not getattr(pipe, "synthetic_weights", False)
            pipe.unet.verify = bool(verify)
        if precise is None and dtype == 'float32' and not external_model and hasattr(pipe.unet, "set_precise"):
            # dtype='float32' asks the reference for fp32 arithmetic (feature/components/models.py:11-12: the whole pipeline in torch.float32).  The
            # native UNet's MFMA operands are 16-bit either way; the plan that is closest to fp32 arithmetic is the full split (every operand an
            # fp16 hi + lo pair: 1.9-2.7e-4 from fp32 against 7-9e-4 for the automatic level), at 0.55x the throughput — the reference's own
            # float32 mode costs more than that.  An explicit `precise=` still wins.
            precise = True
        if precise is not None:
            if hasattr(pipe.unet, "set_precise"):
                pipe.unet.set_precise(precise)
            elif precise not in (False, 0, "auto"):
                raise NotImplementedError("split-operand plans exist for the UNet versions ('1-5', '2-1', 'xl', 'pgv2') only")
        self.pipe = pipe
        self.control_pipe = None
        if control:                                                                      # reference :62-65
            if not hasattr(pipe.unet, "residual_buffer"):
                raise NotImplementedError("control= needs the native UNet (libgdf.so); this pipeline has none")
            from components.control import ControlNetPipeline
            self.control_pipe = ControlNetPipeline(pipe, control, device)
        self.attention_store = None
        # (version == 'flux' with attention=[...]: the reference registers an AttentionStore but its flux branch of extract()
        #  returns before the aggregation step (diffusion_feature.py:246-254 vs :492-500), so no 'attn' entry is ever produced —
        #  accepted and ignored here as well)
        self.scheduler_backup = copy.deepcopy(self.pipe.scheduler)
        self.version = version
        self.img_size = img_size
        self.device = device
        self.control = control
        self.attention = attention

        # freeze whatever torch modules the front-end carries (reference :98-111)
        to_disable = [self.pipe.vae, self.pipe.text_encoder, self.pipe.unet]
        if version in ['xl', 'pgv2', 'flux']:
            to_disable.append(self.pipe.text_encoder_2)
        for m in to_disable:
            for p in m.parameters():
                p.requires_grad = False

    # ------------------------------------------------------------------------------------------
    def _preprocess_basic(self, x):
        return x.resize((self.img_size, self.img_size)).convert("RGB")

    def preprocess_image(self, x, is_tensor=False):
        if not is_tensor:
            return self.pipe.image_processor.preprocess(self._preprocess_basic(x))
        return self.pipe.image_processor.preprocess([x[i] for i in range(x.shape[0])])

    def preprocess_images_device(self, images):
        """torch.concat([preprocess_image(i) for i in images]) made on the device: (B, 3, img_size, img_size) fp32 there, the same bits
        (components/preproc.py device_preprocess; modes other than RGB / L take preprocess_image itself, image by image)"""
        from components.preproc import device_preprocess
        return device_preprocess(images, self.img_size, self.device, host_fn=self.preprocess_image)

    def _preprocess_images(self, images):
        """the batch of image_type='image' (reference :358-364): on the device when the extractor was built with device_preprocess, else on the
        host's thread pool"""
        if getattr(self, 'device_preprocess', False):
            return self.preprocess_images_device(images)
        return torch.concat(_map_threads(self.preprocess_image, list(images)), dim=0)

    def restore_from_tensor_to_image(self, x):
        """(B, 3, h, w) in [-1, 1] -> list of RGB PIL images (reference :143-144, VaeImageProcessor.postprocess with do_denormalize): to fp32,
        (x / 2 + 0.5).clamp(0, 1) * 255 rounded half to even — the quantisation the device Canny applies when it reads such a tensor itself"""
        from PIL import Image
        u = ((x.detach().float().cpu() / 2 + 0.5).clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous().numpy()
        return [Image.fromarray(a) for a in u]

    def encode_prompt(self, prompt_str=None, prompt_file=None):
        assert prompt_str != None and prompt_file == None or prompt_str == None and prompt_file != None
        if prompt_file:
            with open(prompt_file, 'r') as f:
                prompts = f.read()
                print('prompt:', prompts)
        else:
            prompts = prompt_str
        if len(prompts.split(' ')) > 70 and hasattr(self.pipe, 'tokenizer'):
            # reference :165-171: prompts of more than 70 words bypass the pipeline's 77-token truncation (components/encode_long_prompt.py);
            # the UNet then sees (1, n_tokens, C) embeddings — the text length is a plan parameter of the native UNet — and no pooled embeddings
            prompt_embeds, negative_prompt_embeds = _chunked_prompt_embeds(self.pipe, prompts, '', self.device)
            return prompt_embeds, negative_prompt_embeds, None, None
        ret = self.pipe.encode_prompt(prompt=prompts, device=self.device, num_images_per_prompt=1,
                                      negative_prompt='', do_classifier_free_guidance=True)
        if self.version in ('xl', 'pgv2') or self.version.startswith('pixart'):
            # SDXL: (embeds, negative, pooled, negative_pooled); PixArt: (embeds, mask, negative, negative_mask) — the
            # reference returns the pipeline's 4-tuple as is (diffusion_feature.py:182-206)
            prompt_embeds, negative_prompt_embeds, pooled, negative_pooled = ret
        else:
            prompt_embeds, negative_prompt_embeds = ret
            pooled, negative_pooled = None, None
        return prompt_embeds, negative_prompt_embeds, pooled, negative_pooled

    def offload_prompt_encoder(self, persistent=False):
        to_offload = [self.pipe.text_encoder]
        if hasattr(self.pipe, 'text_encoder_2'):
            to_offload.append(self.pipe.text_encoder_2)
        for t in to_offload:
            if not persistent and hasattr(t, 'to'):
                t.to('cpu')

    # ------------------------------------------------------------------------------------------
    def extract(self, prompts, batch_size, image, image_type='image', t=50, denoising_from=None,
                use_control=False, use_ddim_inversion=False, control_image=None):
        """One single-timestep denoiser forward; returns {layer_id: (B,C,H,W) fp16}.
        image_type: 'image' (list of PIL), 'tensors' ((B,3,h,w) in [-1,1]) or — native extension —
        'latents' (pre-noised latents (B,4,H/8,W/8), skipping the VAE stage).
        use_ddim_inversion (UNet versions): the latents are the image's DDIM inversion up to timestep t instead of its noised encoding
        (reference :381-386), see _ddim_inverted_latents.
        use_control (UNet versions, an extractor built with control=[...]): the ControlNets see exactly the UNet's inputs and their residuals
        enter the extraction forward (reference :408-465); the inversion forwards of use_ddim_inversion run without them, as in the reference.
        The control images come from `image`, PIL or tensors (reference :259-263): on a HIP device the 'canny' choices read the (B, 3, S, S)
        batch this call makes for the VAE encoder anyway (components/control.py device_canny); the host preprocessors ('depth') get the PIL
        images, restored from a tensor as the reference restores them.
        control_image — native extension — hands over already-processed control images ((B, 3, h, w) in [0, 1] or PIL) instead of running
        any preprocessor.
        t = [t1, ..., tK] — native extension, UNet versions, 1 <= K <= 8 — extracts the B images at K timesteps in one call: every feature is
        (K*B, C, H, W), timestep-major (split_timesteps(feats, K) gives the K per-timestep dicts); see _extract_multi."""
        if isinstance(t, (list, tuple)):                 # several timesteps of the same images: one VAE encode, one UNet forward of K*B rows
            return self._extract_multi(prompts, batch_size, image, image_type, list(t), denoising_from, use_control, use_ddim_inversion)
        control_pipe = getattr(self, "control_pipe", None) if use_control else None
        if use_control and control_pipe is None:
            raise NotImplementedError("use_control: this extractor was built without control=[...], it has no ControlNet to run")
        if use_control and control_image is None and (image_type == 'latents' or (image_type != 'image' and not hasattr(control_pipe, 'needs_source'))):
            # (latents carry no image; and a control pipeline that is not components/control.py's cannot say which form of the images it wants)
            raise ValueError("use_control derives the control images from the images (image_type='image' or 'tensors'); with latents pass "
                             "control_image=")
        if denoising_from:
            raise NotImplementedError("denoising_from is deprecated upstream and runs there only together with ControlNet (its denoising call "
                                      "reads the ControlNet branch's raw image, reference diffusion_feature.py:394); not native")
        if use_ddim_inversion:
            if self.version == 'flux' or self.version.startswith('pixart'):
                raise NotImplementedError("use_ddim_inversion exists for the UNet versions ('1-5', '2-1', 'xl', 'pgv2') only: the reference's "
                                          "inversion loop calls pipe.unet (components/ddim_inversion.py:31)")
            if image_type == 'latents':
                raise ValueError("use_ddim_inversion inverts an image: image_type must be 'image' or 'tensors'")
        # the preprocessors' input (reference :259-263, :433): the PIL images for the host ones, restored from a tensor where tensors came in; the
        # device ones read `control_source`, set below once the batch for the VAE exists
        derive = control_pipe is not None and control_image is None
        raw_image, control_source = None, None
        if derive and control_pipe.needs_pil():
            raw_image = list(image) if image_type == 'image' else self.restore_from_tensor_to_image(image)
        self.feature_store.reset()
        device = self.device
        if self.version == 'flux':                                                       # reference :246-254
            # ONE denoiser forward per call, at sigmas[t_start]: the reference's patched pipeline returns after its first
            # transformer call (feature/diffusers/pipelines/flux/pipeline_flux_img2img.py:804-841).  The synthetic pipe does
            # the same by construction; a stock diffusers pipeline is stopped by the native transformer (SingleForwardDone).
            from components.native import SingleForwardDone
            tr = getattr(self.pipe, 'transformer', None)
            stock = tr is not None and hasattr(tr, 'single_forward') and not getattr(self.pipe, 'returns_after_first_forward', False)
            if stock:
                tr.single_forward = True
            imgs = _map_threads(lambda i: i.resize((self.img_size, self.img_size)).convert("RGB"), list(image))
            if stock and isinstance(prompts, str) and len(imgs) > 1:
                # a stock FluxImg2ImgPipeline takes its batch size from the PROMPT (a str = 1) and then fails to pack B > 1 image latents;
                # the CLI hands the raw prompt text over (reference extract_feature.py:81-82): one copy per image
                prompts = [prompts] * len(imgs)
            try:
                self.pipe(image=imgs, prompt=prompts, strength=t / 1000, guidance_scale=1)
            except SingleForwardDone:
                pass
            finally:
                if stock:
                    tr.single_forward = False
            return self.feature_store.stored_feats

        is_dit = self.version.startswith('pixart')
        if is_dit:                                                                       # reference :277-283
            prompt_embeds, prompt_attention_mask, _neg, _negm = prompts
            if prompt_embeds.shape[0] == 1 and batch_size > 1:
                prompt_embeds = prompt_embeds.repeat(batch_size, 1, 1)
                prompt_attention_mask = prompt_attention_mask.repeat(batch_size, 1)
            pooled = None
        else:
            prompt_embeds, _neg, pooled, _negp = prompts
            prompt_embeds = prompt_embeds.repeat(batch_size, 1, 1)                       # reference :272
            if pooled is not None:
                pooled = pooled.repeat(batch_size, 1, 1).squeeze(1)                      # :275

        # timestep selection through the scheduler, as the reference does (:288-295) — but the scheduler's bookkeeping stays on the HOST
        # (round 5).  With the timestep table on the device (the reference passes device=device) every `int(t)` / `index_for_timestep` /
        # `sigmas[i]` of the scheduler is a device -> host read that waits for the GPU work queued before it: extract() spent 214 of its
        # 225 ms blocked (tools/profile_extract_host.py) and could not queue the UNet behind the VAE.  The values are the same integers.
        self.pipe.scheduler = copy.deepcopy(self.scheduler_backup)
        self.pipe.scheduler.set_timesteps(1000, device='cpu')
        timesteps, _ = self.pipe.get_timesteps(1000, t / 1000, 'cpu')
        latent_timestep = timesteps[:1].repeat(batch_size)
        t = timesteps[:1]

        added_cond_kwargs = {}
        if self.version in ('xl', 'pgv2'):                                               # :324-354
            # (cached on the device per batch size: a pageable host -> device copy is stream ordered, i.e. it blocks the host until the
            #  previous forward has finished)
            key = (self.img_size, batch_size, str(prompt_embeds.dtype), str(device))
            cache = self.__dict__.setdefault('_time_ids_cache', {})
            if key not in cache:
                add_time_ids = _get_add_time_ids(self.pipe, (self.img_size, self.img_size), (0, 0),
                                                 (self.img_size, self.img_size), dtype=prompt_embeds.dtype)
                cache[key] = add_time_ids.to(device).repeat(batch_size, 1)
            added_cond_kwargs = {"text_embeds": pooled.to(device), "time_ids": cache[key]}

        if image_type == 'latents':
            latents = image.to(device)
        else:
            if image_type == 'image':                                                    # :358-364
                image = self._preprocess_images(list(image))
            elif tuple(image.shape[-2:]) != (self.img_size, self.img_size):
                if derive and control_pipe.needs_source():
                    # the reference, literally (:259-263, :433): restore to PIL, _preprocess_basic (PIL's resize, not the bilinear one below), and
                    # those bytes go to the device
                    import numpy as np
                    basic = [self._preprocess_basic(r) for r in (raw_image if raw_image is not None else self.restore_from_tensor_to_image(image))]
                    control_source = torch.from_numpy(np.stack([np.array(b) for b in basic])).to(device)
                # (bilinear resampling at scale 1 samples exactly the pixel centres: the identity, so tensors that already have the target
                #  size — e.g. the CLI's loader threads, which ran preprocess_image themselves — skip the launch)
                image = F.interpolate(image, (self.img_size, self.img_size), mode='bilinear')
            if derive and control_source is None and control_pipe.needs_source():
                # the batch the VAE encoder reads, moved to the device once and shared: preprocess_image's 2 (u / 255) - 1 quantises back to the
                # bytes u of _preprocess_basic(image), so the PIL images are not resized a second time for Canny
                image = control_source = image.to(device, non_blocking=True)
            if use_ddim_inversion:                                                       # :381-386 (the feature store has nothing to pause:
                latents = self._ddim_inverted_latents(image, prompts, prompt_embeds, added_cond_kwargs, t)    # the trajectory's plan has no hooks)
            else:
                latents = self.pipe.prepare_latents(image, latent_timestep, 1, batch_size, prompt_embeds.dtype, device)

        latent_model_input = self.pipe.scheduler.scale_model_input(latents, t)          # :405-406

        # aggregated `attention=[...]` feature (reference :67-68, :492-500): the needed '*-map' hooks are requested
        # internally; AttentionStore keeps query grids in [img/32, img/16] (components/attention.py:541)
        attn_ids = None
        if self.attention and hasattr(self.pipe.unet, 'extra_hook_ids'):
            lat = latents.shape[-1]
            attn_ids = attention_map_ids(self.pipe.unet.cfg, self.pipe.unet.hook_names(), self.attention, lat,
                                         self.img_size // 32, self.img_size // 16)
            self.pipe.unet.extra_hook_ids = [i for ids in attn_ids.values() for i in ids]

        if is_dit:                                                                       # reference :466-474
            tr = self.pipe.transformer
            dit_ids = None
            if self.attention and hasattr(tr, 'extra_hook_ids'):                         # AttentionStore(img/32, img/8), all 'up'
                grid = latents.shape[-1] // int(tr.cfg.get("patch_size", 2))
                dit_ids = dit_attention_map_ids(tr.hook_names(), self.attention, grid, self.img_size // 32, self.img_size // 8)
                tr.extra_hook_ids = [i for ids in dit_ids.values() for i in ids]
            tr(latent_model_input, encoder_hidden_states=prompt_embeds.to(device),
               encoder_attention_mask=prompt_attention_mask.to(device), timestep=t, return_dict=False,
               added_cond_kwargs={'resolution': None, 'aspect_ratio': None})
            if dit_ids is not None and any(dit_ids.values()):
                extra = tr.last_extra
                maps = {c: [extra[i] for i in ids if i in extra] for c, ids in dit_ids.items() if ids}
                self.feature_store.stored_feats['attn'] = aggregate_attention(maps, self.img_size // 8)      # reference :492-500
                tr.last_extra = {}
            return self.feature_store.stored_feats
        # ---- the hot path: native UNet forward, hooks written by the kernels (:445-465) ----
        if hasattr(self.pipe.unet, 'shared_ctx'):
            # prompt_embeds.repeat(batch_size, 1, 1) above: ONE prompt for the whole batch -> the text K/V are computed once per call.  (Embeddings
            # that already carried several rows are not that case: the promise is only made for a (1, n, C) prompt.)
            self.pipe.unet.shared_ctx = prompts[0].shape[0] == 1
        if control_pipe is not None:                                                     # reference :408-439 (no classifier-free guidance here)
            noise_pred = self._controlled_forward(control_pipe, raw_image, control_image, latent_model_input, t, prompt_embeds.to(device),
                                                  added_cond_kwargs, control_source)
        else:
            noise_pred = self.pipe.unet(latent_model_input, timestep=t, encoder_hidden_states=prompt_embeds.to(device),
                                        added_cond_kwargs=added_cond_kwargs, down_block_additional_residuals=None,
                                        mid_block_additional_residual=None, return_dict=False)[0]
        if self.store_vae_output:                                                        # reference :477-485
            from components.models import native_vae_decoder, scheduler_step_scalars
            a, b = scheduler_step_scalars(self.pipe.scheduler, t)                         # scheduler.step(noise_pred, t, latents)[0]
            self.feature_store.stored_feats['vae-out'] = native_vae_decoder(self.pipe, device).decode(
                latents, noise_pred, c_sample=a, c_eps=b, scaling_factor=float(self.pipe.vae.config.scaling_factor))
        if attn_ids is not None:
            extra = self.pipe.unet.last_extra
            maps = {c: [extra[i] for i in ids if i in extra] for c, ids in attn_ids.items()}
            self.feature_store.stored_feats['attn'] = aggregate_attention(maps, self.img_size // 8)
            self.pipe.unet.last_extra = {}
        return self.feature_store.stored_feats                                           # :517

    def _extract_multi(self, prompts, batch_size, image, image_type, ts, denoising_from, use_control, use_ddim_inversion):
        """extract() for K timesteps of the same B images: the images are preprocessed and VAE-encoded ONCE (prepare_latents_multi: only the
        encoder's last kernel fans out), then ONE UNet forward of batch K*B runs with a per-row timestep.  Rows k*B:(k+1)*B of every feature
        belong to ts[k] (the [negative, positive] convention of generate()); duplicates in `ts` are allowed — each row has its own posterior
        sample and noise.  The random draws are those of the single-timestep call at batch K*B (native_prepare_latents_multi).  Those rows have
        the bits of the single-timestep pieces on the same draws: the VAE encode of the B images (plan batch B) with slice k of eps / noise
        and timestep k's scalars, then extract(t=ts[k], image_type='latents') on the K*B stacked rows.  (NOT necessarily the bits of
        extract(t=ts[k]) on the images tiled K times: that call encodes at plan batch K*B, and at small sizes the encoder's GEMMs split K
        by M, i.e. sum in another order)
        What a K*B-row batch of one timestep supports works here as well: feature_resize, '*-map' hooks, attention=[...], early_exit,
        precise=, verify.  Each of the following is ONE trajectory or ONE scheduler step and is refused: use_ddim_inversion, use_control,
        'vae-out', image_type='latents'; so are the flux / PixArt versions and a pipeline without the native VAE encoder."""
        from components.native import MAX_TIMESTEPS
        self.feature_store.reset()
        K = len(ts)
        if self.version == 'flux' or self.version.startswith('pixart'):
            raise NotImplementedError("t=[...] exists for the UNet versions ('1-5', '2-1', 'xl', 'pgv2') only: the flux pipeline takes one "
                                      "strength per call and the PixArt transformer's plan one timestep per batch")
        if not 1 <= K <= MAX_TIMESTEPS:
            raise ValueError(f"t=[...] takes 1..{MAX_TIMESTEPS} timesteps per call (the VAE tail kernel carries that many coefficient "
                             f"triples in its arguments), got {K}")
        if denoising_from:
            raise NotImplementedError("denoising_from is not native (see extract)")
        if use_ddim_inversion:
            raise NotImplementedError("t=[...] with use_ddim_inversion: every timestep is the end of its own inversion trajectory, there is "
                                      "no encode to share; call extract once per timestep")
        if use_control:
            raise NotImplementedError("t=[...] with use_control: the ControlNets run on one timestep's UNet inputs; call extract once per "
                                      "timestep")
        if self.store_vae_output:
            raise NotImplementedError("t=[...] with 'vae-out' requested: the decoder takes ONE scheduler step's scalars; call extract once "
                                      "per timestep")
        if image_type == 'latents':
            raise ValueError("t=[...] noises the images' encoding once per timestep: image_type must be 'image' or 'tensors' (latents are "
                             "already noised for one timestep)")
        if getattr(self.pipe, 'native_vae', None) is None or not hasattr(self.pipe, 'prepare_latents_multi'):
            raise NotImplementedError("t=[...] shares one NATIVE VAE encode between the timesteps; this pipeline has no native VAE encoder "
                                      "(GDF_NATIVE_VAE=0)")
        device = self.device
        n = K * batch_size
        prompt_embeds, _neg, pooled, _negp = prompts
        prompt_embeds = prompt_embeds.repeat(n, 1, 1)
        if pooled is not None:
            pooled = pooled.repeat(n, 1, 1).squeeze(1)

        # every timestep through a fresh copy of the scheduler, as the single path picks its one (host-side bookkeeping: see extract)
        schedulers, t_rows = [], []
        for tk in ts:
            sch = self.pipe.scheduler = copy.deepcopy(self.scheduler_backup)
            sch.set_timesteps(1000, device='cpu')
            timesteps, _ = self.pipe.get_timesteps(1000, tk / 1000, 'cpu')
            schedulers.append(sch)
            t_rows.append(timesteps[:1])

        added_cond_kwargs = {}
        if self.version in ('xl', 'pgv2'):
            key = (self.img_size, n, str(prompt_embeds.dtype), str(device))
            cache = self.__dict__.setdefault('_time_ids_cache', {})
            if key not in cache:
                add_time_ids = _get_add_time_ids(self.pipe, (self.img_size, self.img_size), (0, 0),
                                                 (self.img_size, self.img_size), dtype=prompt_embeds.dtype)
                cache[key] = add_time_ids.to(device).repeat(n, 1)
            added_cond_kwargs = {"text_embeds": pooled.to(device), "time_ids": cache[key]}

        if image_type == 'image':
            image = self._preprocess_images(list(image))
        elif tuple(image.shape[-2:]) != (self.img_size, self.img_size):
            image = F.interpolate(image, (self.img_size, self.img_size), mode='bilinear')
        # (a, b) of timestep k from the scheduler copy that picked it, as the single path's prepare_latents asks ITS copy: get_timesteps left
        # begin_index on each, and diffusers' Euler / DPM-Solver add_noise reads the sigma at that index
        latents = self.pipe.prepare_latents_multi(image, [tr.repeat(batch_size) for tr in t_rows], batch_size, prompt_embeds.dtype, device,
                                                  schedulers=schedulers)
        # scale_model_input per timestep, each on the scheduler copy that picked it: the torch ops of the single path on the same values
        latent_model_input = torch.cat([sch.scale_model_input(latents[k * batch_size:(k + 1) * batch_size], t_rows[k])
                                        for k, sch in enumerate(schedulers)], dim=0)
        t_vec = torch.cat([tr.repeat(batch_size) for tr in t_rows])                     # host vector, one timestep per row

        attn_ids = None
        if self.attention and hasattr(self.pipe.unet, 'extra_hook_ids'):
            attn_ids = attention_map_ids(self.pipe.unet.cfg, self.pipe.unet.hook_names(), self.attention, latents.shape[-1],
                                         self.img_size // 32, self.img_size // 16)
            self.pipe.unet.extra_hook_ids = [i for ids in attn_ids.values() for i in ids]
        if hasattr(self.pipe.unet, 'shared_ctx'):
            self.pipe.unet.shared_ctx = prompts[0].shape[0] == 1
        self.pipe.unet(latent_model_input, timestep=t_vec, encoder_hidden_states=prompt_embeds.to(device),
                       added_cond_kwargs=added_cond_kwargs, down_block_additional_residuals=None,
                       mid_block_additional_residual=None, return_dict=False)
        if attn_ids is not None:
            extra = self.pipe.unet.last_extra
            maps = {c: [extra[i] for i in ids if i in extra] for c, ids in attn_ids.items()}
            self.feature_store.stored_feats['attn'] = aggregate_attention(maps, self.img_size // 8)
            self.pipe.unet.last_extra = {}
        return self.feature_store.stored_feats

    def _controlled_forward(self, control_pipe, raw_image, control_image, latent_model_input, t, prompt_embeds, added_cond_kwargs, source=None):
        """The extraction forward with ControlNet residuals: the ControlNets run on the UNet's own inputs with the UNet plan's shared-ctx
        promise and operand split, write their block straight into that plan's staged residual buffer (no staging copy), and the UNet runs
        with it; hooks reach the feature store as in NativeUNet.__call__.
        raw_image: the PIL images of the host preprocessors (None when no choice has one); source: the device preprocessors' image batch."""
        unet = self.pipe.unet
        ids = unet.requested_ids()
        have = set(ids)
        ids = ids + [i for i in unet.extra_hook_ids if i not in have]
        B, _, H, W = latent_model_input.shape
        split = unet.split_for(ids, lat=min(H, W))
        basic = [self._preprocess_basic(r) for r in raw_image] if raw_image is not None else None
        out = unet.residual_buffer(B, H, W, prompt_embeds.shape[1], ids, unet.shared_ctx)
        block = control_pipe.generate_control_info(basic, latent_model_input, t, prompt_embeds, added_cond_kwargs, control_image=control_image,
                                                   shared_ctx=unet.shared_ctx, split=split, out=out, source=source)
        noise, hooks = unet.forward_raw(latent_model_input, t, prompt_embeds, added_cond_kwargs.get("text_embeds"),
                                        added_cond_kwargs.get("time_ids"), hook_ids=ids, shared_ctx=unet.shared_ctx, residuals=block)
        unet.last_extra = {k: v for k, v in hooks.items() if k in set(unet.extra_hook_ids)}
        if unet.feature_store is not None:
            for hid, tns in hooks.items():
                if hid in have:
                    unet.feature_store.store(tns, hid)
        return noise

    def _ddim_inverted_latents(self, image, prompts, prompt_embeds, added_cond_kwargs, t):
        """The reference's `ddim_inversion(self.pipe, image, device, prompts, 100, t)` (:385, components/ddim_inversion.py:7-45) on the native path:
        VAE encode without noise -> fp32 latents -> the inversion steps as ONE device-resident trajectory (no fp16 rounding of the latents and no
        host round trip between steps) -> fp32 latents, which the caller hands to scale_model_input as it does the noised ones.
        Kept as the reference has it, odd or not: the inversion forwards see the UN-scaled latents (:28-31: no scale_model_input, whatever the
        pipeline's scheduler is) while the extraction forward that follows applies the pipeline scheduler's scale_model_input to the result;
        '1-5' / '2-1' scale the VAE sample by the constant 0.18215 (:15) and condition on prompts[0] (:31).
        Native extension: the reference cannot run this for 'xl' / 'pgv2' (its UNet call passes no added_cond_kwargs, :31); here they use
        vae.config.scaling_factor and the text_embeds / time_ids of the extraction forward."""
        from components.models import ddim_inversion_table
        unet, enc = self.pipe.unet, getattr(self.pipe, 'native_vae', None)
        if enc is None or not hasattr(unet, 'trajectory'):
            raise NotImplementedError("use_ddim_inversion needs the native VAE encoder and UNet (libgdf.so); this pipeline has neither")
        device = self.device
        xl = self.version in ('xl', 'pgv2')
        image = image.to(device)
        f = 1 << (len(enc.cfg["block_out_channels"]) - 1)
        B, _, H, W = image.shape
        eps = torch.randn((B, enc.cfg["latent_channels"], H // f, W // f), device=device, dtype=torch.float32)    # latent_dist.sample() (:15)
        sf = float(self.pipe.vae.config.scaling_factor) if xl else 0.18215
        lat = enc.encode(image, eps=eps, noise=None, noise_a=1.0, noise_b=0.0, scaling_factor=sf)
        table = ddim_inversion_table(self.pipe.scheduler, 100, t)
        return unet.trajectory(lat.float(), table, prompt_embeds.to(device), added_cond_kwargs.get("text_embeds"),
                               added_cond_kwargs.get("time_ids"), shared_ctx=prompts[0].shape[0] == 1)

    def generate(self, prompts, batch_size, num_inference_steps=50, guidance_scale=7.5, latents=None, generator=None, output_type='latent'):
        """A text-to-image run with background feature extraction (UNet versions): what the reference's generate_with_extraction.py gets from
        a stock pipeline call after `set_background_extraction([1, 10, 20, ...])` — every requested layer keeps the features of the N-th,
        M-th, ... UNet call — as ONE device-resident run: fp32 master latents, guidance and the scheduler step in one kernel between
        forwards, a hook-less plan replayed from one graph for the calls nobody keeps (NativeUNet.sample).
        prompts: encode_prompt()'s 4-tuple, repeated over the batch as extract() does.  guidance_scale > 1: the forwards have batch
        2 * batch_size, [negative, positive]; <= 1: the unguided batch, as diffusers does.  latents: (B,4,h,w) standard-normal noise (drawn
        with `generator` when None); it is scaled by the scheduler's init_noise_sigma.
        Afterwards `get_background_extraction()` gives {id: {encounter: (2B|B, C, H, W)}} (encounters count UNet calls from 1; indices past
        the last call never fire) and feature_store.feats[id]['count'] is the number of calls; with store_idx None the store holds
        {id: tensor} of the last call, as the reference's overwrite per call leaves it.
        Returns the final fp32 latents, or with output_type='pt' (latents, image (B,3,H,W) fp16 from the native VAE decoder)."""
        if self.version == 'flux' or self.version.startswith('pixart'):
            raise NotImplementedError("generate exists for the UNet versions ('1-5', '2-1', 'xl', 'pgv2') only: the device-resident sampler "
                                      "drives pipe.unet")
        if getattr(self, "control_pipe", None) is not None:
            raise NotImplementedError("generate with a ControlNet is not native: the device-resident sampler runs the UNet without residuals; "
                                      "build the extractor without control= to generate")
        if self.attention:
            raise NotImplementedError("generate does not produce the aggregated attention=[...] feature: the reference aggregates its "
                                      "AttentionStore once per extract() call, there is no per-encounter form to match")
        if output_type not in ('latent', 'pt'):
            raise ValueError("output_type must be 'latent' or 'pt'")
        from components.feature_extractor import background_capture_rows
        from components.models import sampling_table
        unet = self.pipe.unet
        if not hasattr(unet, 'sample'):
            raise NotImplementedError("generate needs the native UNet (libgdf.so); this pipeline has none")
        fs = self.feature_store
        fs.reset()
        device = self.device
        guided = float(guidance_scale) > 1.0
        xl = self.version in ('xl', 'pgv2')
        prompt_embeds, negative, pooled, negative_pooled = prompts
        ctx_pos = prompt_embeds.repeat(batch_size, 1, 1).to(device)                     # as extract() (:272)
        ctx_neg = negative.repeat(batch_size, 1, 1).to(device) if guided else None
        text_embeds = time_ids = None
        if xl:
            pos_p = pooled.repeat(batch_size, 1, 1).squeeze(1)
            text_embeds = (torch.cat([negative_pooled.repeat(batch_size, 1, 1).squeeze(1), pos_p], 0) if guided else pos_p).to(device)
            add_time_ids = _get_add_time_ids(self.pipe, (self.img_size, self.img_size), (0, 0), (self.img_size, self.img_size),
                                             dtype=torch.float32)
            time_ids = add_time_ids.to(device).repeat(text_embeds.shape[0], 1)

        self.pipe.scheduler = copy.deepcopy(self.scheduler_backup)
        rows, init_sigma = sampling_table(self.pipe.scheduler, num_inference_steps)
        f = int(getattr(self.pipe, 'vae_scale_factor', 8))
        shape = (batch_size, unet.cfg["in_channels"], self.img_size // f, self.img_size // f)
        if latents is None:
            gdev = generator.device if generator is not None else device
            latents = torch.randn(shape, generator=generator, device=gdev, dtype=torch.float32)
        elif tuple(latents.shape) != shape:
            raise ValueError(f"latents must have shape {shape}")
        x0 = latents.to(device, torch.float32) * init_sigma

        known = set(unet.hook_names())
        ids = [i for i in unet.requested_ids() if i in known]
        active = fs.status != 'pause' and bool(ids)
        caps = background_capture_rows(fs.store_idx, len(rows)) if active else []
        x, captured = unet.sample(x0, rows, guidance_scale, ctx_pos, ctx_neg, text_embeds, time_ids, hook_ids=ids if caps else (),
                                  capture_rows=caps)
        # delivery through the store, so that feature_resize, the cross-k / cross-v drop and accept_all -> cpu apply as in extract()
        dropped = lambda hid: 'cross-k' in hid or 'cross-v' in hid
        for k in caps:
            for hid, t in captured[k].items():
                if fs.store_idx is not None and not dropped(hid):
                    # the calls between two captures ran without hooks: the store's own counter catches up before it counts this one
                    fs.feats.setdefault(hid, {'feat': {}, 'count': 0})['count'] = k
                fs.store(t, hid)
        if active and fs.store_idx is not None:
            for hid in ids:
                if not dropped(hid):
                    fs.feats.setdefault(hid, {'feat': {}, 'count': 0})['count'] = len(rows)
        if output_type == 'pt':
            from components.models import native_vae_decoder
            image = native_vae_decoder(self.pipe, device).decode(x, None, c_sample=1.0, c_eps=0.0,
                                                                 scaling_factor=float(self.pipe.vae.config.scaling_factor))
            return x, image
        return x

    def aggregate(self, feats=None, size=128, mode='bilinear', dtype=torch.float16):
        """The evaluators' first step on a feature dict (reference correspondence/aggregation_network.py:62-66, scarce_segmentation/
        task-pixel.py:50-55): torch.cat([F.interpolate(f, size, mode=mode) for f in feats.values()], 1) -> (B, sum C, OH, OW) `dtype`.
        feats defaults to the dict of the last extract(); the values are taken in dict order (hook execution order, `attn` last).
        Device tensors: one aggregate_kernel launch per 16 layers (components/postproc.py aggregate)."""
        from components.postproc import aggregate
        if feats is None:
            feats = self.feature_store.stored_feats
        if not feats:
            raise ValueError("aggregate: no features (call extract() first or pass feats=)")
        return aggregate(list(feats.values()) if isinstance(feats, dict) else list(feats), size, mode, dtype)

    def correspond(self, feats1, feats2, source_points, load_size=(512, 512)):
        """The evaluators' second step (reference correspondence/correspondence/correspondence_utils.py:113-138) on two aggregated maps, e.g. two
        results of aggregate(): the nearest neighbour of every source point among the load-size target pixels -> (points2 int64 (B, N, 2) (y, x),
        cosine scores fp32 (B, N)).  Device tensors: gdf_op_nn_match, neither load-size map is built (components/postproc.py nn_match)."""
        from components.postproc import nn_match
        return nn_match(feats1, feats2, source_points, load_size)

    def match(self, feats1, feats2, mutual=False):
        """Dense matching of two maps (reference correspondence/correspondence/correspondence_utils.py:73-111, batch_cosine_sim +
        find_nn_correspondences, and the two torch.max of find_best_buddies_correspondences): for every pixel of feats1 its best pixel of feats2 by
        cosine similarity and the reverse -> (nn12 int64 (B, P1), sim12 fp32, nn21 int64 (B, P2), sim21 fp32); mutual=True: the mutual
        nearest-neighbour mask instead -> (mask (B, P1) bool, nn12, sim12).  Device tensors: gdf_op_dense_match, the P1 x P2 matrix is never
        built (components/postproc.py dense_match, mutual_nn)."""
        from components.postproc import dense_match, mutual_nn
        return mutual_nn(feats1, feats2) if mutual else dense_match(feats1, feats2)

    def correspondence_loss(self, feats1, feats2, source_points, target_points, scale=None):
        """The correspondence evaluator's loss (reference correspondence/task-corres.py:70-80, compute_clip_loss) on two maps from hyperfeature()
        or aggregate(): the symmetric cross-entropy of scale * cosine similarity between the N source pixels of feats1 and the N target pixels of
        feats2 -> (B,) fp32, differentiable with respect to both maps.  source_points / target_points: (B, N, 2) or, for B = 1, (N, 2) (y, x) in
        the maps' own pixel coordinates, clipped and rounded half to even as the reference's points_to_idxs does; scale: exp(logit_scale),
        None = 1 / 0.07.  Device tensors: gdf_op_clip_loss, neither similarity matrix is built (components/postproc.py clip_loss)."""
        import numpy as np
        from components.postproc import CLIP_SCALE, clip_loss
        idx = []
        for pts, v in ((source_points, feats1), (target_points, feats2)):
            p = np.asarray(pts.detach().cpu() if isinstance(pts, torch.Tensor) else pts)
            if p.ndim < 2 or p.shape[-1] != 2:
                raise ValueError("points are (B, N, 2) or (N, 2) arrays of (y, x)")
            h, w = v.shape[2], v.shape[3]
            idx.append(torch.from_numpy((w * np.round(np.clip(p[..., 0], 0, h - 1)) + np.round(np.clip(p[..., 1], 0, w - 1))).astype(np.int64)))
        return clip_loss(feats1, feats2, idx[0], idx[1], CLIP_SCALE if scale is None else scale)

    def segment(self, ensemble, feats=None, size=256):
        """The label-scarce segmentation evaluator on a feature dict (reference scarce_segmentation/task-pixel.py:85-103): aggregate(feats, size)
        (bilinear) and the pixel-classifier ensemble's vote on the result -> (labels int64 (B, OH, OW), top_k (B,)), on the device.
        ensemble: a components.postproc.PixelClassifierEnsemble, or the reference's list of pixel_classifier modules."""
        from components.postproc import PixelClassifierEnsemble
        if not isinstance(ensemble, PixelClassifierEnsemble):
            ensemble = PixelClassifierEnsemble(ensemble)
        return ensemble.predict(self.aggregate(feats, size))

    def hyperfeature(self, head=None, feats=None, size=128):
        """The correspondence evaluator's descriptor map from a feature dict (reference correspondence/correspondence/aggregation_network.py:62-66,
        97-100, AggregationNetwork.forward(x, do_conv) from the extraction onward): aggregate(feats, size) (bilinear, fp16) and, when a head is
        given, its fp32 3 x 3 output convolution -> (B, Cout, OH, OW) fp32; head=None is do_conv=False and returns the aggregated map.  Either
        result feeds correspond() as it is.  head: a components.postproc.AggregationHead, a TrainableAggregationHead (passed through as it is: the
        result then carries the graph for out.weight), or anything an AggregationHead is built from (the reference's
        AggregationNetwork, an nn.Conv2d, a weight, a state dict, a task-corres.py checkpoint)."""
        from components.postproc import AggregationHead, TrainableAggregationHead
        agg = self.aggregate(feats, size)
        if head is None:
            return agg
        if not isinstance(head, (AggregationHead, TrainableAggregationHead)):
            head = AggregationHead(head)
        return head(agg)

    def visualize(self, feats=None, layers=None, size=512, joint=False):
        """The reference's PCA pictures (feature_visualization.py:84-101, plot_pca) of a feature dict -> {layer id: (B, OH, OW, 3) uint8 tensor}:
        every map projected onto its three leading principal components, each component scaled to 0 .. 255 over the image, resized (nearest) so
        that the short side is `size` (None keeps the grid).  feats defaults to the dict of the last extract(); layers: the ids to draw (None =
        all, in dict order; `attn` included, its C is the token count).  joint: one PCA and one colour scale for the whole batch of a layer.
        Device tensors: gdf_op_pca and gdf_op_pca_rgb (components/postproc.py pca_rgb)."""
        from components.postproc import pca_rgb
        if feats is None:
            feats = self.feature_store.stored_feats
        if not feats:
            raise ValueError("visualize: no features (call extract() first or pass feats=)")
        ids = list(feats) if layers is None else list(layers)
        missing = [i for i in ids if i not in feats]
        if missing:
            raise ValueError("visualize: no layer %r among the features" % (missing[0],))
        return {i: pca_rgb(feats[i], size, joint) for i in ids}

    def set_background_extraction(self, idxs):
        self.feature_store.store_idx = idxs

    def get_background_extraction(self):
        return {k: v['feat'] for k, v in self.feature_store.feats.items()}


def split_timesteps(feats, K):
    """The K per-timestep dicts of an `extract(..., t=[t1, ..., tK])` result: entry k holds, for every id, rows k*B:(k+1)*B of the stored
    (K*B, ...) tensor — VIEWS, no copies."""
    K = int(K)
    if K < 1:
        raise ValueError("K must be >= 1")
    out = [{} for _ in range(K)]
    for hid, v in feats.items():
        if v.shape[0] % K:
            raise ValueError(f"'{hid}' has {v.shape[0]} rows: not a multiple of K = {K}")
        B = v.shape[0] // K
        for k in range(K):
            out[k][hid] = v[k * B:(k + 1) * B]
    return out


DiffusionFeature = FeatureExtractor      # name used by BASELINE.json's north_star


def _chunked_prompt_embeds(pipe, prompt, negative_prompt, device):
    """Text embeddings of a prompt longer than the tokenizer window, as the reference produces them (feature/components/encode_long_prompt.py:5-40):
    the text with the larger WORD count is tokenised without truncation, the other one padded to that token count; both id rows are cut into windows of
    `tokenizer.model_max_length` ids, every window goes through `pipe.text_encoder` on its own (the last window as short as it happens to be) and the
    windows' hidden states are concatenated along the token axis.  Returns (prompt_embeds, negative_prompt_embeds), both (1, n_tokens, C)."""
    tok = pipe.tokenizer
    window = tok.model_max_length

    def free(text):
        return tok(text, return_tensors="pt", truncation=False).input_ids.to(device)

    def padded(text, n):
        return tok(text, return_tensors="pt", truncation=False, padding="max_length", max_length=n).input_ids.to(device)

    if len(prompt.split(" ")) >= len(negative_prompt.split(" ")):
        ids = free(prompt)
        neg_ids = padded(negative_prompt, ids.shape[-1])
    else:
        neg_ids = free(negative_prompt)
        ids = padded(prompt, neg_ids.shape[-1])
    n = ids.shape[-1]
    encode = lambda rows: torch.cat([pipe.text_encoder(rows[:, a:a + window])[0] for a in range(0, n, window)], dim=1)
    return encode(ids), encode(neg_ids)


def _get_add_time_ids(pipe, original_size, crops_coords_top_left, target_size, dtype,
                      aesthetic_score=6.0, negative_aesthetic_score=2.5):
    """SDXL micro-conditioning vector and its consistency check (reference :534-571)."""
    if pipe.config.requires_aesthetics_score:
        ids = list(original_size + crops_coords_top_left + (aesthetic_score,))
    else:
        ids = list(original_size + crops_coords_top_left + target_size)
    passed = pipe.unet.config.addition_time_embed_dim * len(ids) + pipe.text_encoder_2.config.projection_dim
    expected = pipe.unet.add_embedding.linear_1.in_features
    if expected != passed:
        raise ValueError(f"Model expects an added time embedding vector of length {expected}, but a vector of "
                         f"{passed} was created. Check `requires_aesthetics_score` / `projection_dim`.")
    return torch.tensor([ids], dtype=dtype)
