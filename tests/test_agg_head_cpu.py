"""Aggregation-network head without a GPU: the source forms components/postproc.py AggregationHead accepts, its host-tensor path against F.conv2d,
the refusals, FeatureExtractor.hyperfeature on host tensors, and the header."""
import os
import re
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "generic-diffusion-feature_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import agg_head_ref as R  # noqa: E402
from components import postproc  # noqa: E402


@pytest.mark.parametrize("bias", [False, True])
def test_every_source_form_gives_the_same_parameters(bias):
    w, b = R.gen_weight(7, 12, seed=1, bias=bias)
    forms = R.sources(w, b)
    assert len(forms) == (5 if bias else 6)
    for name, src in forms.items():
        head = postproc.AggregationHead(src)
        assert (head.Cin, head.Cout) == (12, 7), name
        assert head.weight.dtype == torch.float32 and not head.weight.is_cuda and torch.equal(head.weight, w), name
        assert (head.bias is None) == (b is None) and (b is None or torch.equal(head.bias, b)), name
    half = postproc.AggregationHead(w.half())                                              # any floating type: converted to fp32 once
    assert half.weight.dtype == torch.float32 and torch.equal(half.weight, w.half().float())


def test_host_path_is_the_reference_arithmetic():
    w, b = R.gen_weight(9, 20, seed=2, bias=True)
    for f32 in (False, True):
        v = R.gen_features(2, 20, 7, 5, f32, seed=3)
        for bias in (None, b):
            head = postproc.AggregationHead(R.Network(w, bias))
            got = head(v)
            assert got.dtype == torch.float32 and tuple(got.shape) == (2, 9, 7, 5)
            assert torch.equal(got, F.conv2d(v.float(), w, bias, padding=1))
            assert torch.equal(got, R.Network(w, bias)(v).detach())                        # the stand-in module's forward: the reference's two lines
            R.Bounds(w, bias, v).check(got, "host path")
            one = head(v[1])                                                               # the reference's unbatched (Cin, H, W)
            assert tuple(one.shape) == (9, 7, 5) and torch.equal(one, head(v[1:2])[0])
    cl = v.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)                            # any strides
    R.Bounds(w, b, v).check(head(cl), "host path, channels-last")                          # (torch picks another algorithm there: not the same bits)


def test_other_convolutions_and_shapes_are_refused():
    conv = torch.nn.Conv2d
    for bad in (conv(4, 4, 1), conv(4, 4, 3, stride=2, padding=1), conv(4, 4, 3, padding=0), conv(4, 4, 3, padding=2, dilation=2),
                conv(4, 4, 3, padding=1, groups=2), conv(4, 4, 3, padding=1, padding_mode="reflect"), conv(4, 4, (3, 5), padding=1)):
        with pytest.raises(ValueError):
            postproc.AggregationHead(bad)
    for bad in (torch.zeros(4, 4, 1, 1), torch.zeros(4, 4, 3), {"in.weight": torch.zeros(4, 4, 3, 3)}, {"aggregation_network": 3},
                torch.nn.Linear(4, 4), 3, {"out.weight": torch.zeros(4, 4, 3, 3), "out.bias": torch.zeros(5)}):
        with pytest.raises(ValueError):
            postproc.AggregationHead(bad)
    head = postproc.AggregationHead(torch.zeros(4, 6, 3, 3))
    for bad in (torch.zeros(1, 5, 3, 3), torch.zeros(6, 3), torch.zeros(1, 1, 6, 3, 3), torch.zeros(1, 6, 0, 3)):
        with pytest.raises(ValueError):
            head(bad)


def test_hyperfeature_on_host_tensors():
    import diffusion_feature
    fe = diffusion_feature.FeatureExtractor.__new__(diffusion_feature.FeatureExtractor)
    v = R.gen_features(2, 20, 8, 6, False, seed=5)
    feats = {"a": v[:, :12], "b": F.avg_pool2d(v[:, 12:].float(), 2).half()}
    w, _ = R.gen_weight(5, 20, seed=6)
    agg = postproc.aggregate(list(feats.values()), (10, 9))
    none = fe.hyperfeature(None, feats, (10, 9))
    assert none.dtype == torch.float16 and torch.equal(none, agg)                          # do_conv=False
    head = postproc.AggregationHead(w)
    got = fe.hyperfeature(head, feats, (10, 9))
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, 5, 10, 9) and torch.equal(got, head(agg))
    assert torch.equal(fe.hyperfeature(R.Network(w), feats, (10, 9)), got)                 # anything a head is built from


def test_header_declares_the_handle_and_the_three_functions():
    src = open(os.path.join(ROOT, "include", "gdf_ops.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert "typedef struct gdf_agghead_s* gdf_agghead;" in code
    assert re.search(r"\bint\s+gdf_agghead_create\s*\(\s*int\s+Cin\s*,\s*int\s+Cout\s*,\s*const\s+float\s*\*\s*W\s*,\s*const\s+float\s*\*\s*bias\s*,"
                     r"\s*gdf_agghead\s*\*\s*out\s*\)", code)
    assert re.search(r"\bvoid\s+gdf_agghead_destroy\s*\(\s*gdf_agghead\s+h\s*\)", code)
    assert re.search(r"\bint\s+gdf_agghead_forward\s*\(\s*gdf_agghead\s+h\s*,\s*const\s+gdf_agg_src\s*\*\s*x\s*,\s*int\s+B\s*,\s*float\s*\*\s*out\s*,"
                     r"\s*void\s*\*\s*stream\s*\)", code)
    assert len(postproc._SIG["gdf_agghead_create"][1]) == 5 and len(postproc._SIG["gdf_agghead_forward"][1]) == 5
