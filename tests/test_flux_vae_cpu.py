"""The host side of the native Flux latent preparation, without a GPU: the packing index expression, the sigma lookup, the VAE config, the
GEMM instantiation conv_out selects with 32 output channels, and the new symbols."""
import ctypes
import os
import re
import sys

import pytest
import torch

from ops_binding import GemmArgs, lib
from test_gemm_dispatch_cpu import kernel_name
from test_gpu_gemm import CASES

from components import models as M
from components import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = os.path.join(ROOT, "tests", "fake_diffusers")


@pytest.fixture()
def D(monkeypatch):
    monkeypatch.syspath_prepend(FAKE)
    sys.modules.pop("diffusers", None)
    import diffusers
    assert diffusers.__version__.endswith("+fake")
    yield diffusers
    sys.modules.pop("diffusers", None)


def test_pack_index_is_pack_latents(D):
    B, L, h, w = 2, 16, 6, 10
    lat = torch.arange(B * L * h * w, dtype=torch.float32).view(B, L, h, w)
    want = D.FluxImg2ImgPipeline._pack_latents(lat, B, L, h, w)
    idx = M.flux_pack_index(L, h, w)
    assert idx.shape == (L, h, w) and sorted(idx.reshape(-1).tolist()) == list(range(L * h * w))
    got = torch.empty(B, L * h * w)
    got[:, idx.reshape(-1)] = lat.reshape(B, -1)
    assert torch.equal(got.view(B, (h // 2) * (w // 2), 4 * L), want)


@pytest.mark.parametrize("strength", [0.1, 0.3, 0.85])
def test_sigma_lookup_is_scale_noises(D, strength):
    """what the stock pipeline does up to prepare_latents: shifted sigmas, get_timesteps (which sets the begin index), then
    scale_noise(0, t, 1) = sigma * 1 + (1 - sigma) * 0"""
    import numpy as np
    sch = D.FlowMatchEulerDiscreteScheduler(shift=3.0, use_dynamic_shifting=True, base_shift=0.5, max_shift=1.15, base_image_seq_len=256,
                                            max_image_seq_len=4096)
    pipe = D.FluxImg2ImgPipeline.__new__(D.FluxImg2ImgPipeline)
    pipe.scheduler = sch
    n = 28
    mu = D.calculate_shift(4096, 256, 4096, 0.5, 1.15)
    sch.set_timesteps(sigmas=np.linspace(1.0, 1 / n, n), mu=mu)
    for with_begin_index in (True, False):
        ts, _ = pipe.get_timesteps(n, strength, "cpu")
        if not with_begin_index:
            sch._begin_index = None                             # a scheduler that was never given one: the table is searched for the timestep
        t = ts[:1].repeat(2)
        want = sch.scale_noise(torch.zeros(2, 1, 1, 1), t, torch.ones(2, 1, 1, 1)).flatten()
        got = M.flux_scale_noise_sigma(sch, t)
        assert isinstance(got, float) and got == float(want[0]) == float(want[1])
        assert got == float(sch.sigmas[int(max(n - min(n * strength, n), 0))])


def test_flux_vae_config_is_the_checkpoints(D):
    """against the AutoencoderKL config the stub's FluxImg2ImgPipeline builds its VAE with (FluxImg2ImgPipeline._build)"""
    vc = D._vae_shell(torch.float32, 0, 0.3611, latent_channels=16, shift_factor=0.1159, quant=False, sample_size=1024).config
    cfg = native.VAE_CONFIGS["flux"]
    assert cfg == dict(in_channels=vc.in_channels, latent_channels=vc.latent_channels, block_out_channels=tuple(vc.block_out_channels),
                       layers_per_block=vc.layers_per_block, use_quant_conv=int(vc.use_quant_conv))
    assert cfg["latent_channels"] == 16 and cfg["use_quant_conv"] == 0
    sd = native.VAE_CONFIGS["sd"]
    assert {k: v for k, v in cfg.items() if k not in ("latent_channels", "use_quant_conv")} == \
           {k: v for k, v in sd.items() if k not in ("latent_channels", "use_quant_conv")}           # the SD trunk


@pytest.mark.parametrize("B,hw", [(1, 8), (2, 8), (1, 128), (4, 128)])
def test_flux_conv_out_selects_a_kernel_tested_gemm(B, hw):
    """encoder.conv_out of the Flux VAE: conv3x3, Cin = 512, N = 32 (2 * 16 moments), the bn = 16 fp32-output epilogue — 64 latent pixels (a
    64^2 image) and 16384 (1024^2), one image and a sub-batch: an instantiation launch_gemm already has, i.e. one with a kernel-level case"""
    L = lib()
    a = GemmArgs()
    a.mode, a.B, a.H, a.Wd, a.Cin, a.N, a.stride, a.lda = 1, B, hw, hw, 512, 32, 1, 512
    a.bias, a.out32, a.ldo32, a.bn = ctypes.c_void_p(1), ctypes.c_void_p(1), 32, 16
    name = kernel_name(L, a)
    assert name is not None and name in {c["kernel"] for c in CASES}, name
    a.N, a.ldo32 = 8, 8                                           # the SD VAE's conv_out: the same instantiation
    assert kernel_name(L, a) == name


def test_new_symbols_are_declared_and_exported():
    inc = os.path.join(ROOT, "include")
    vae_h, ops_h = open(os.path.join(inc, "gdf_vae.h")).read(), open(os.path.join(inc, "gdf_ops.h")).read()
    assert re.search(r"\bint\s+gdf_vae_encode_packed\s*\(", vae_h) and re.search(r"\bint\s+gdf_op_vae_finish_packed\s*\(", ops_h)
    L = native.load_library()
    for n in ("gdf_vae_encode_packed", "gdf_op_vae_finish_packed", "gdf_vae_encode", "gdf_op_vae_finish"):
        assert hasattr(L, n), n
    assert "gdf_vae_encode_packed" in native.SIGNATURES
    # argument checks that need no device: a null plan, and the kernel entry's refusals
    assert L.gdf_vae_encode_packed(None, None, None, None, 1.0, 0.0, 1.0, 0.0, 0, None, None, None) != 0
    f = L.gdf_op_vae_finish_packed
    f.restype = ctypes.c_int
    vp, ci, fp = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    f.argtypes = [vp, ci, ci, ci, ci, vp, vp, vp, vp, fp, fp, fp, fp, ci, vp, vp]
    one = ctypes.c_void_p(16)
    for (Lc, H, W, out) in ((17, 4, 4, one), (4, 3, 4, one), (4, 4, 5, one), (4, 4, 4, None)):
        assert f(one, 1, H, W, Lc, None, None, None, None, 1.0, 0.0, 1.0, 0.0, 0, out, None) != 0
        assert b"vae_finish_packed" in L.gdf_last_error()


def test_switch_is_off_by_default(monkeypatch):
    monkeypatch.delenv("GDF_FLUX_NATIVE_VAE", raising=False)
    assert not M.flux_native_vae_enabled()
    monkeypatch.setenv("GDF_FLUX_NATIVE_VAE", "1")
    assert M.flux_native_vae_enabled()
    monkeypatch.setenv("GDF_FLUX_NATIVE_VAE", "0")
    assert not M.flux_native_vae_enabled()
