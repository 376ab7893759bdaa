"""Bilinear aggregation of hooked features, the parts that need no GPU: the C symbol (declared, exported, bound, refusals on the host), the
host-tensor path of components/postproc.py aggregate, FeatureExtractor.aggregate's dict order and the CLI's --aggregate_mode / --aggregate_size."""
import ctypes
import os
import re
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "generic-diffusion-feature_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from aggregate_ref import AggSrc, bind, reference  # noqa: E402


def _cl(t):
    return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def _feats(seed=0):
    g = torch.Generator().manual_seed(seed)
    return {"up-a": _cl(torch.randn(2, 12, 4, 4, generator=g).half()), "up-b": _cl(torch.randn(2, 5, 16, 16, generator=g).half()),
            "attn": torch.randn(2, 7, 8, 8, generator=g).half()}


def _torch_form(feats, size, mode="bilinear"):
    return torch.cat([F.interpolate(v.float(), size, mode=mode) for v in feats], 1).to(torch.float16)


def test_symbol_declared_exported_and_bound():
    import __graft_entry__ as G
    G.build()
    src = open(os.path.join(ROOT, "include", "gdf_ops.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+gdf_op_aggregate\s*\(\s*const\s+gdf_agg_src\s*\*", code)
    m = re.search(r"typedef\s+struct\s+gdf_agg_src\s*\{(.*?)\}\s*gdf_agg_src\s*;", code, flags=re.S)
    assert m, "gdf_agg_src is not declared"
    fields = re.findall(r"\b(ptr|f32|sb|sc|sy|sx|C|H|W|coff)\b", m.group(1))
    assert fields == [n for n, _ in AggSrc._fields_], fields
    lib = bind(ctypes.CDLL(G.LIB))
    assert hasattr(lib, "gdf_op_aggregate") and lib.gdf_abi_version() == 1
    from components import postproc
    res, args = postproc._SIG["gdf_op_aggregate"]
    assert res is ctypes.c_int and len(args) == 10 and ctypes.sizeof(postproc.AggSrc) == ctypes.sizeof(AggSrc) == 64
    assert [n for n, _ in postproc.AggSrc._fields_] == [n for n, _ in AggSrc._fields_]
    assert callable(postproc.aggregate) and callable(postproc.resize_concat)


def test_argument_errors_are_refused_on_the_host():
    """every refusal happens before any launch: the pointers are host memory that no kernel could touch, and there may be no device at all"""
    import __graft_entry__ as G
    G.build()
    lib = bind(ctypes.CDLL(G.LIB))
    mem = (ctypes.c_char * 4096)()
    ptr = ctypes.addressof(mem)

    def call(n=1, B=1, out=ptr, out_f32=0, Ctot=8, OH=4, OW=4, mode=1, srcs="one", **over):
        s = (AggSrc * 2)()
        for e in s:
            e.ptr, e.f32, e.sb, e.sc, e.sy, e.sx, e.C, e.H, e.W, e.coff = ptr, 0, 128, 1, 32, 8, 4, 4, 4, 0
        s[1].coff = 4
        for k, v in over.items():
            setattr(s[1] if k.endswith("1") else s[0], k.rstrip("1"), v)
        return lib.gdf_op_aggregate(None if srcs is None else s, n, B, out, out_f32, Ctot, OH, OW, mode, None)

    cases = [dict(n=0), dict(n=-1), dict(n=17), dict(srcs=None), dict(out=None), dict(ptr=None), dict(n=2, ptr1=None),
             dict(C=0), dict(H=0), dict(W=0), dict(n=2, W1=-3), dict(OH=0), dict(OW=0), dict(OW=-2),
             dict(coff=-1), dict(coff=5), dict(n=2, coff1=5), dict(C=9),
             dict(mode=2), dict(mode=-1),
             dict(mode=0, out_f32=1), dict(mode=0, OH=4, OW=6)]
    for kw in cases:
        assert call(**kw) != 0, kw
        assert b"gdf_op_aggregate" in lib.gdf_last_error(), (kw, lib.gdf_last_error())
    # B == 0 is a successful no-op in both modes, checked after the arguments
    assert call(B=0) == 0 and call(B=0, n=2, mode=0) == 0
    assert call(B=0, mode=7) != 0


def test_host_tensors_equal_the_torch_expression():
    from components.postproc import aggregate, resize_concat
    feats = list(_feats().values())
    for size, hw in ((24, (24, 24)), ((10, 36), (10, 36)), (None, (16, 16)), (16, (16, 16))):
        got = aggregate(feats, size)
        assert got.dtype == torch.float16 and tuple(got.shape) == (2, 24) + hw
        assert torch.equal(got, _torch_form(feats, hw))
    got32 = aggregate(feats, 24, dtype=torch.float32)
    assert got32.dtype == torch.float32
    assert torch.equal(got32, torch.cat([F.interpolate(v.float(), (24, 24), mode="bilinear") for v in feats], 1))
    # ATen's fp32 CPU kernel lies within the tests' bound of the float64 reference (aggregate_ref.py)
    for v in feats:
        ref, bound = reference(v.float().numpy(), 24, 24, out_f32=True)
        err = np.abs(F.interpolate(v.float(), (24, 24), mode="bilinear").double().numpy() - ref)
        assert (err <= bound).all()
    # nearest: resize_concat's host result, with and without a size
    assert torch.equal(aggregate(feats, None, mode="nearest"), resize_concat(feats))
    assert torch.equal(aggregate(feats, 24, mode="nearest"), resize_concat(feats, 24))
    with pytest.raises(ValueError):
        aggregate(feats, 24, mode="bicubic")
    with pytest.raises(ValueError):
        aggregate([], 24)


def test_feature_extractor_aggregate_keeps_dict_order():
    import diffusion_feature
    fe = diffusion_feature.FeatureExtractor.__new__(diffusion_feature.FeatureExtractor)
    torch.nn.Module.__init__(fe)
    feats = _feats(1)
    fe.feature_store = types.SimpleNamespace(stored_feats=feats)
    got = fe.aggregate(size=24)                                           # the dict of the last extract()
    assert tuple(got.shape) == (2, 24, 24, 24) and torch.equal(got, _torch_form(list(feats.values()), (24, 24)))
    assert torch.equal(got[:, :12], _torch_form([feats["up-a"]], (24, 24))) and torch.equal(got[:, 17:], _torch_form([feats["attn"]], (24, 24)))
    swapped = {k: feats[k] for k in ("attn", "up-a", "up-b")}
    got = fe.aggregate(swapped, size=(8, 12), dtype=torch.float32)         # an explicit dict: ITS order
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, 24, 8, 12)
    assert torch.equal(got.half(), _torch_form(list(swapped.values()), (8, 12)))
    assert tuple(fe.aggregate().shape) == (2, 24, 128, 128)                # the evaluators' default grid
    fe.feature_store = types.SimpleNamespace(stored_feats={})
    with pytest.raises(ValueError):
        fe.aggregate()


def test_cli_flags(capsys):
    import extract_feature as cli
    a = cli.parse_args(["--aggregate_output"])
    assert a.aggregate_mode == "nearest" and a.aggregate_size is None
    a = cli.parse_args([])
    assert a.aggregate_mode == "nearest" and a.aggregate_size is None and not a.aggregate_output
    a = cli.parse_args(["--aggregate_output", "--aggregate_mode", "bilinear", "--aggregate_size", "24"])
    assert a.aggregate_mode == "bilinear" and a.aggregate_size == 24
    assert cli.parse_args(["--aggregate_output", "--aggregate_size", "24", "40"]).aggregate_size == (24, 40)
    for bad in (["--aggregate_mode", "bilinear"], ["--aggregate_size", "24"], ["--aggregate_mode", "nearest"],
                ["--aggregate_output", "--aggregate_size", "1", "2", "3"], ["--aggregate_output", "--aggregate_size", "0"],
                ["--aggregate_output", "--aggregate_mode", "bicubic"]):
        with pytest.raises(SystemExit) as e:
            cli.parse_args(bad)
        assert e.value.code not in (0, None), bad
    with pytest.raises(SystemExit):
        cli.parse_args(["--aggregate_mode", "bilinear"])
    assert "--aggregate_output" in capsys.readouterr().err


def test_cli_writer_on_cpu_tensors(tmp_path, monkeypatch):
    import extract_feature as cli
    from components import postproc
    feats = _feats(2)
    calls = []
    real_rc, real_agg = postproc.resize_concat, postproc.aggregate
    monkeypatch.setattr(postproc, "resize_concat", lambda *a, **k: (calls.append("resize_concat"), real_rc(*a, **k))[1])
    monkeypatch.setattr(postproc, "aggregate", lambda *a, **k: (calls.append("aggregate"), real_agg(*a, **k))[1])

    def run(name, argv):
        a = cli.parse_args(["--output_dir", str(tmp_path / name)] + argv)
        w = cli.HostWriter(a)
        w.submit(dict(feats), ["n0", "n1"])
        w.close()
        return [np.load(tmp_path / name / f"n{j}.npy") for j in range(2)]

    got = run("default", ["--aggregate_output"])                          # the defaults take today's call and write today's files
    assert calls == ["resize_concat"]
    want = real_rc(list(feats.values()))
    for j in range(2):
        assert got[j].shape == (24, 16, 16) and np.array_equal(got[j], want[j].numpy())
    del calls[:]
    got = run("bilinear", ["--aggregate_output", "--aggregate_mode", "bilinear", "--aggregate_size", "24"])
    assert calls == ["aggregate"]
    want = _torch_form(list(feats.values()), (24, 24))
    for j in range(2):
        assert got[j].shape == (24, 24, 24) and got[j].dtype == np.float16 and np.array_equal(got[j], want[j].numpy())
    got = run("rect", ["--aggregate_output", "--aggregate_mode", "bilinear", "--aggregate_size", "8", "12"])
    assert got[1].shape == (24, 8, 12) and np.array_equal(got[1], _torch_form(list(feats.values()), (8, 12))[1].numpy())
    got = run("bilinear_default_size", ["--aggregate_output", "--aggregate_mode", "bilinear"])
    assert got[0].shape == (24, 16, 16) and np.array_equal(got[0], _torch_form(list(feats.values()), (16, 16))[0].numpy())
