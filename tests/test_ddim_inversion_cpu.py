"""CPU-side checks of DDIM-inversion extraction (no GPU): the coefficient table NativeUNet.trajectory runs
(components/models.py ddim_inversion_table, restating the loop of the reference's components/ddim_inversion.py:19-43),
and the two new entry points of the library."""
import ctypes
import math
import types

import numpy as np
import pytest
import torch


def _alphas(n=1000):
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, n, dtype=torch.float64) ** 2       # SD's scaled-linear schedule
    return torch.cumprod(1.0 - betas, 0)


def _sched(**cfg):
    return types.SimpleNamespace(alphas_cumprod=_alphas(cfg.get("num_train_timesteps", 1000)), config=types.SimpleNamespace(**cfg))


SD = dict(num_train_timesteps=1000, steps_offset=1, timestep_spacing="leading")


def test_table_rows_stop_rule_and_closed_form():
    from components.models import ddim_inversion_table
    s = _sched(**SD)
    rows = ddim_inversion_table(s, 100, 50)
    assert [r[0] for r in rows] == [11, 21, 31, 41, 51]
    assert [r[0] for r in ddim_inversion_table(s, 100, 1)] == [11]
    full = ddim_inversion_table(s, 100, 2000)
    assert len(full) == 99 and full[-1][0] == 991 and [r[0] for r in full] == list(range(11, 992, 10))
    # the scheduler timestep reaches the table as the one-element tensor extract() holds
    assert ddim_inversion_table(s, 100, torch.tensor([50])) == rows
    ac = s.alphas_cumprod.tolist()
    for t, c_in, c_s, c_e in full:
        a_cur, a_next = ac[max(0, t - 10)], ac[t]
        assert c_in == 1.0
        assert abs(c_s - math.sqrt(a_next / a_cur)) <= 1e-12
        assert abs(c_e - (math.sqrt(1 - a_next) - math.sqrt(1 - a_cur) * math.sqrt(a_next / a_cur))) <= 1e-12


def test_timestep_spacings_are_the_published_sequences():
    from components.models import ddim_timesteps, ddim_inversion_table
    ns = types.SimpleNamespace
    assert ddim_timesteps(ns(**SD), 100) == list(range(991, 0, -10))
    assert ddim_timesteps(ns(num_train_timesteps=1000, steps_offset=0, timestep_spacing="leading"), 4) == [750, 500, 250, 0]
    assert ddim_timesteps(ns(num_train_timesteps=1000, steps_offset=1, timestep_spacing="trailing"), 4) == [999, 749, 499, 249]
    assert ddim_timesteps(ns(num_train_timesteps=1000, steps_offset=0, timestep_spacing="trailing"), 100) == list(range(999, 0, -10))
    assert ddim_timesteps(ns(num_train_timesteps=1000, steps_offset=0, timestep_spacing="linspace"), 4) == [999, 666, 333, 0]
    assert ddim_timesteps(ns(num_train_timesteps=1000, steps_offset=0, timestep_spacing="linspace"), 7) == \
        [int(v) for v in np.linspace(0, 999, 7).round()[::-1]]
    assert ddim_timesteps(dict(SD), 100) == list(range(991, 0, -10))                          # a plain dict config
    with pytest.raises(ValueError):
        ddim_timesteps(ns(num_train_timesteps=1000, timestep_spacing="karras"), 10)
    # reversed and walked from index 1: trailing 9, 19, 29, ... -> rows 19, 29, ...; linspace n = 100: 0, 10.09 -> 10, ...
    tr = _sched(num_train_timesteps=1000, steps_offset=0, timestep_spacing="trailing")
    assert [r[0] for r in ddim_inversion_table(tr, 100, 40)] == [19, 29, 39, 49]
    li = _sched(num_train_timesteps=1000, steps_offset=0, timestep_spacing="linspace")
    assert [r[0] for r in ddim_inversion_table(li, 100, 30)] == [10, 20, 30]


def test_table_works_for_a_scheduler_without_a_config():
    """the synthetic pipes' scheduler: alphas_cumprod and nothing else -> DDIMScheduler's defaults (leading, offset 0)"""
    from components.models import _Scheduler, ddim_inversion_table
    for euler in (False, True):
        rows = ddim_inversion_table(_Scheduler(euler), 100, 50)
        assert [r[0] for r in rows] == [10, 20, 30, 40, 50]
        assert all(r[1] == 1.0 and 1.0 > r[2] > 0.9 and r[3] > 0 for r in rows)


def test_table_reproduces_the_reference_recurrence():
    """A stub "UNet" (a fixed function of (x, t)) run through the table against the reference's loop, both in float64; the loop body is
    the formula of components/ddim_inversion.py:33-43 written out."""
    from components.models import ddim_inversion_table
    s = _sched(**SD)
    alphas_cumprod = s.alphas_cumprod
    g = torch.Generator().manual_seed(3)
    x0 = torch.randn(2, 4, 8, 8, generator=g, dtype=torch.float64)
    unet = lambda x, t: torch.tanh(0.7 * x + 0.001 * t) - 0.3 * x.flip(1)
    num_inference_steps, stop_at_t = 100, 200

    timesteps = list(range(1, 1000, 10))                 # reversed(DDIMScheduler(leading, offset 1).timesteps)
    latents = x0.clone()
    steps = 0
    for i in range(1, num_inference_steps):
        t = timesteps[i]
        noise_pred = unet(latents, t)
        current_t = max(0, t - (1000 // num_inference_steps))
        next_t = t
        alpha_t = alphas_cumprod[current_t]
        alpha_t_next = alphas_cumprod[next_t]
        latents = (latents - (1 - alpha_t).sqrt() * noise_pred) * (alpha_t_next.sqrt() / alpha_t.sqrt()) + (
            1 - alpha_t_next
        ).sqrt() * noise_pred
        steps += 1
        if t >= stop_at_t:
            break

    rows = ddim_inversion_table(s, num_inference_steps, stop_at_t)
    assert len(rows) == steps == 20
    x = x0.clone()
    for t, c_in, c_s, c_e in rows:
        x = c_s * x + c_e * unet(c_in * x, t)
    assert float((x - latents).abs().max()) <= 1e-12 * float(latents.abs().max())


def test_trajectory_entry_points_are_exported_and_bound():
    import __graft_entry__ as G
    G.build()
    from components import native
    lib = ctypes.CDLL(G.LIB)
    assert hasattr(lib, "gdf_trajectory") and hasattr(lib, "gdf_op_latent_step")
    assert "gdf_trajectory" in native.SIGNATURES
    bound = native.load_library().gdf_trajectory
    assert bound.restype is ctypes.c_int and len(bound.argtypes) == 10
    assert lib.gdf_abi_version() == 1                                                        # additive: the ABI version stays
    assert hasattr(native.NativeUNet, "trajectory")
    # a null plan is refused with a message, not a crash
    assert bound(None, None, 1, None, None, None, None, None, None, None) != 0
    assert b"null plan" in native.load_library().gdf_last_error()


def test_extract_flags_raise_with_their_own_messages():
    """denoising_from / use_control stay unsupported, each saying why; the inversion flag is refused for the DiT versions by name.
    (The checks come before anything touches the pipeline, so a bare object stands in for the extractor.)"""
    import diffusion_feature as D
    fx = types.SimpleNamespace(version="1-5")
    with pytest.raises(NotImplementedError, match="ControlNet"):
        D.FeatureExtractor.extract(fx, None, 1, None, use_control=True)
    with pytest.raises(NotImplementedError, match="denoising_from"):
        D.FeatureExtractor.extract(fx, None, 1, None, denoising_from=100)
    for v in ("pixart-sigma", "flux"):
        with pytest.raises(NotImplementedError, match="use_ddim_inversion"):
            D.FeatureExtractor.extract(types.SimpleNamespace(version=v), None, 1, None, use_ddim_inversion=True)
    with pytest.raises(ValueError, match="image_type"):
        D.FeatureExtractor.extract(fx, None, 1, None, image_type="latents", use_ddim_inversion=True)
