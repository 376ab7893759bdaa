"""Multi-timestep extraction, the parts that need no GPU: the CLI's --t parsing, split_timesteps on CPU tensors, the two new C symbols
(declared in the headers, exported by the built library, bound by components/native.py) and HostWriter's sub-directory."""
import ctypes
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "generic-diffusion-feature_amd"))


def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(gdf_[a-z0-9_]+)\s*\(", src)))


def test_cli_t_parsing(capsys):
    import extract_feature as cli
    assert cli.parse_args(["--t", "50"]).t == 50                        # one value stays an int: today's path and output tree
    assert cli.parse_args(["--t", "50", "100"]).t == [50, 100]
    assert cli.parse_args(["--t", "300", "100", "-b", "4"]).t == [300, 100]          # order kept: it is the row order of the features
    assert cli.parse_args([]).t is None
    with pytest.raises(SystemExit) as e:
        cli.parse_args(["--t", "100", "100"])
    assert e.value.code not in (0, None)
    assert "repeated" in capsys.readouterr().err


def test_split_timesteps_on_cpu_tensors():
    from diffusion_feature import split_timesteps
    K, B = 3, 2
    feats = {"a": torch.arange(K * B * 4 * 5 * 5, dtype=torch.float32).reshape(K * B, 4, 5, 5).half(),
             "b": torch.randn(K * B, 7, 3, 3).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)}        # channels-last strides
    parts = split_timesteps(feats, K)
    assert len(parts) == K and all(list(p.keys()) == ["a", "b"] for p in parts)
    for k, p in enumerate(parts):
        for hid, v in p.items():
            assert v.shape[0] == B and torch.equal(v, feats[hid][k * B:(k + 1) * B])
            assert v.untyped_storage().data_ptr() == feats[hid].untyped_storage().data_ptr()              # a view, not a copy
            assert v.data_ptr() == feats[hid][k * B].data_ptr()
    parts[1]["a"].zero_()                                               # writing through the view reaches the stored tensor
    assert float(feats["a"][B:2 * B].abs().sum()) == 0.0 and float(feats["a"][:B].abs().sum()) > 0.0
    assert split_timesteps(feats, 1)[0]["a"].shape == feats["a"].shape
    assert split_timesteps({}, 4) == [{}, {}, {}, {}]
    with pytest.raises(ValueError):
        split_timesteps(feats, 4)                                       # 6 rows are not 4 groups
    with pytest.raises(ValueError):
        split_timesteps(feats, 0)


def test_new_symbols_declared_exported_and_bound():
    import __graft_entry__ as G
    G.build()
    assert "gdf_vae_encode_multi" in _declared("gdf_vae.h")
    assert "gdf_op_vae_finish_multi" in _declared("gdf_ops.h")
    # ONE definition of the limit (include/gdf.h, which both headers include); the Python constant repeats it and is held to it here
    defs = {h: re.findall(r"#define\s+GDF_MAX_TIMESTEPS\s+(\d+)", open(os.path.join(ROOT, "include", h)).read())
            for h in ("gdf.h", "gdf_vae.h", "gdf_ops.h")}
    assert defs == {"gdf.h": ["8"], "gdf_vae.h": [], "gdf_ops.h": []}, defs
    for h in ("gdf_vae.h", "gdf_ops.h"):
        assert re.search(r'#include\s+"gdf.h"', open(os.path.join(ROOT, "include", h)).read()), h
    assert "#define GDF_MAX_TIMESTEPS" not in open(os.path.join(ROOT, "generic-diffusion-feature_amd", "csrc", "kernels.h")).read()
    lib = ctypes.CDLL(G.LIB)
    for n in ("gdf_vae_encode_multi", "gdf_op_vae_finish_multi", "gdf_vae_encode", "gdf_op_vae_finish"):
        assert hasattr(lib, n), n
    from components import native
    assert "gdf_vae_encode_multi" in native.SIGNATURES and native.MAX_TIMESTEPS == int(defs["gdf.h"][0])
    res, args = native.SIGNATURES["gdf_vae_encode_multi"]
    assert res is ctypes.c_int and len(args) == 12 and args[5] is ctypes.c_int
    assert args[6] is args[7] is args[8] is ctypes.POINTER(ctypes.c_float)      # the coefficient arrays are host pointers
    from components import models
    assert callable(models.native_prepare_latents_multi)
    # refusals that need no device: n_t outside 1..8 and null coefficient arrays never reach a launch
    lib.gdf_op_vae_finish_multi.restype = ctypes.c_int
    lib.gdf_last_error.restype = ctypes.c_char_p
    lib.gdf_op_vae_finish_multi.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 4 + [
        ctypes.c_float, ctypes.c_int] + [ctypes.POINTER(ctypes.c_float)] * 3 + [ctypes.c_void_p, ctypes.c_void_p]
    c = (ctypes.c_float * 9)(*([1.0] * 9))
    for n_t in (0, 9, -1):
        assert lib.gdf_op_vae_finish_multi(None, 1, 16, 4, None, None, None, None, 1.0, n_t, c, c, c, None, None) != 0
        assert b"vae_finish_multi" in lib.gdf_last_error()
    assert lib.gdf_op_vae_finish_multi(None, 1, 16, 4, None, None, None, None, 1.0, 2, c, None, c, None, None) != 0


def test_host_writer_subdirectory(tmp_path):
    """HostWriter.submit(..., subdir=) puts the SAME layouts one level down; without it the paths are the parent layout's"""
    import extract_feature as cli
    feats = {"layer-x": torch.arange(2 * 3 * 2 * 2, dtype=torch.float32).reshape(2, 3, 2, 2).half(),
             "layer-y": torch.ones(2, 5, 4, 4).half()}
    tree = lambda root: sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)
    for mode, want in (({}, ["layer-x/n0.npy", "layer-x/n1.npy", "layer-y/n0.npy", "layer-y/n1.npy"]),
                       ({"sample_name_first": True}, ["n0/layer-x.npy", "n0/layer-y.npy", "n1/layer-x.npy", "n1/layer-y.npy"]),
                       ({"aggregate_output": True}, ["n0.npy", "n1.npy"])):
        out = tmp_path / ("o_" + "_".join(mode) if mode else "o_plain")
        args = types.SimpleNamespace(output_dir=str(out), aggregate_output=False, sample_name_first=False)
        args.__dict__.update(mode)
        w = cli.HostWriter(args)
        w.submit(dict(feats), ["n0", "n1"])
        w.submit(dict(feats), ["n0", "n1"], subdir="t100")
        w.close()
        assert tree(out) == sorted(want + ["t100/" + p for p in want])
        for p in want:
            assert np.array_equal(np.load(out / p), np.load(out / "t100" / p))
        if not mode:
            assert np.array_equal(np.load(out / "layer-x" / "n1.npy"), feats["layer-x"][1].numpy())


# ---- the host logic of extract(t=[...]) on a diffusers scheduler, without a GPU ---------------------------------------------------------
class _RecordingEncoder:
    """stands where NativeVAEEncoder stands: records the scalars it is asked to apply and returns latents of ones"""
    cfg = dict(block_out_channels=(1, 1, 1, 1), latent_channels=4)

    def __init__(self):
        self.single, self.multi = [], []

    def encode(self, image, eps=None, noise=None, scaling_factor=1.0, noise_a=1.0, noise_b=0.0, input_scale=1.0):
        self.single.append((float(noise_a), float(noise_b)))
        return torch.ones(eps.shape, dtype=torch.float16)

    def encode_multi(self, image, eps=None, noise=None, scaling_factor=1.0, noise_a=(1.0,), noise_b=(0.0,), input_scale=(1.0,)):
        self.multi.append([(float(a), float(b)) for a, b in zip(noise_a, noise_b)])
        return torch.ones(eps.shape, dtype=torch.float16)


class _Pipe:
    """a bare pipeline object (weak-referenceable, as the diffusers pipelines are)"""


class _RecordingUNet:
    shared_ctx = False

    def __init__(self):
        self.calls = []

    def parameters(self):
        return iter(())

    def __call__(self, sample, timestep=None, **kw):
        self.calls.append((sample.clone(), torch.as_tensor(timestep).clone()))
        return (None,)


@pytest.mark.parametrize("family", ["euler", "dpm", "pndm"])
def test_every_timestep_gets_its_own_noise_scalars_on_diffusers_schedulers(family, monkeypatch):
    """extract(t=[50, 400, 800]) on the restated diffusers schedulers of tests/fake_diffusers: timestep k's (noise_a, noise_b) and its
    scale_model_input factor equal those of extract(t=t_k).  The img2img get_timesteps leaves begin_index on the scheduler it ran on and
    Euler / DPM-Solver add_noise then reads the sigma AT that index: the scalars must be asked of the scheduler copy that picked the timestep
    (asking the last copy for all of them gives every row the last timestep's sigma)."""
    import types
    import weakref
    monkeypatch.syspath_prepend(os.path.join(ROOT, "tests", "fake_diffusers"))
    sys.modules.pop("diffusers", None)
    import diffusers
    try:
        import diffusion_feature
        from components import models as M
        from components.feature_extractor import FeatureStore
        sch = {"euler": diffusers.EulerDiscreteScheduler, "dpm": diffusers.DPMSolverMultistepScheduler, "pndm": diffusers.PNDMScheduler}[family](
            beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", **({"skip_prk_steps": True} if family == "pndm" else {}))
        enc, unet = _RecordingEncoder(), _RecordingUNet()
        pipe = _Pipe()
        pipe.scheduler, pipe.native_vae, pipe.unet = sch, enc, unet
        pipe.vae = types.SimpleNamespace(config=types.SimpleNamespace(scaling_factor=0.18215))
        proxy = weakref.proxy(pipe)
        pipe.get_timesteps = types.MethodType(M._img2img_get_timesteps, proxy)
        pipe.prepare_latents = types.MethodType(M.native_prepare_latents, proxy)                  # bound as _native_vae_from_diffusers binds them
        pipe.prepare_latents_multi = types.MethodType(M.native_prepare_latents_multi, proxy)
        fe = diffusion_feature.FeatureExtractor.__new__(diffusion_feature.FeatureExtractor)
        torch.nn.Module.__init__(fe)
        fe.pipe, fe.version, fe.device, fe.img_size, fe.attention, fe.store_vae_output = pipe, "2-1", "cpu", 64, None, False
        fe.feature_store = FeatureStore({"x": True}, 1, False)
        import copy
        fe.scheduler_backup = copy.deepcopy(sch)
        B, ts = 2, [50, 400, 800]
        prompts = (torch.zeros(1, 77, 8, dtype=torch.float16), None, None, None)
        img = torch.zeros(B, 3, 64, 64)
        fe.extract(prompts, B, img, image_type="tensors", t=ts)
        assert len(enc.multi) == 1 and len(enc.multi[0]) == len(ts) and not enc.single
        multi_in, multi_t = unet.calls[-1]
        assert tuple(multi_in.shape) == (len(ts) * B, 4, 8, 8) and multi_t.numel() == len(ts) * B
        for k, t in enumerate(ts):
            fe.extract(prompts, B, img, image_type="tensors", t=t)
            a, b = enc.single[-1]
            single_in, single_t = unet.calls[-1]
            assert enc.multi[0][k] == (a, b), (family, t, enc.multi[0][k], (a, b))
            rows = slice(k * B, (k + 1) * B)
            assert torch.equal(multi_in[rows], single_in), (family, t)                           # latents of ones: the scale_model_input factor
            assert torch.equal(multi_t[rows].float(), single_t.float().reshape(-1)[:1].expand(B)), (family, t)
        bs = [b for _, b in enc.multi[0]]
        assert bs[0] < bs[1] < bs[2]                                                           # more noise at later timesteps
    finally:
        sys.modules.pop("diffusers", None)
