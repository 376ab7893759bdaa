"""Trainable aggregation head without a GPU: the float64 oracle of tests/agg_head_train_ref.py against hand-computed cases, the emulation of the
kernel's split arithmetic within the bound on every GPU case's inputs, components/postproc.py TrainableAggregationHead on the host (autograd, state
dict, checkpoints, refusals), rescale_points / compute_pck, and the declarations of include/gdf_ops.h."""
import io
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import agg_head_train_ref as R
import clip_loss_ref as CR
from ops_binding import ROOT
from components import postproc


def test_oracle_on_hand_computed_cases():
    # one pixel: only the centre tap sees the map
    x = torch.tensor([[[[3.0]], [[-2.0]]]])                                   # (1, 2, 1, 1)
    g = torch.tensor([[[[5.0]]]])                                             # (1, 1, 1, 1)
    want = torch.zeros(1, 2, 3, 3, dtype=torch.float64)
    want[0, 0, 1, 1], want[0, 1, 1, 1] = 15.0, -10.0
    assert torch.equal(R.oracle(x, g), want)
    # a 2 x 2 map and one gradient element at (0, 1): dW[dy, dx] = 2 X[0 + dy - 1, 1 + dx - 1], zeros outside
    x = torch.tensor([[[[1.0, 2.0], [3.0, 4.0]]]])
    g = torch.zeros(1, 1, 2, 2)
    g[0, 0, 0, 1] = 2.0
    want = torch.tensor([[[[0.0, 0.0, 0.0], [2.0, 4.0, 0.0], [6.0, 8.0, 0.0]]]], dtype=torch.float64)
    assert torch.equal(R.oracle(x, g), want)
    # two images add, and an image's taps never see the other image
    x2 = torch.cat([x, 10 * x])
    g2 = torch.cat([g, g])
    assert torch.equal(R.oracle(x2, g2), 11 * want)
    # the same thing through autograd
    w = torch.zeros(1, 1, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(x2.double(), w, padding=1).backward(g2.double())
    assert torch.equal(w.grad, 11 * want)


def test_channel_error_is_per_input_channel():
    want = torch.zeros(2, 3, 3, 3, dtype=torch.float64)
    want[:, 0] = 1.0
    want[:, 1] = 100.0
    got = want.clone().float()
    got[0, 0, 0, 0] += 0.5                                                   # a large error of the small channel is not hidden by the large one
    rel = R.channel_rel(got, want)
    assert abs(float(rel[0]) - 0.5 / 18 ** 0.5) < 1e-12 and float(rel[1]) == 0 and float(rel[2]) == 0   # all-zero channel, all-zero result
    got[1, 2, 1, 1] = 1e-30
    assert R.channel_error(got, want) == float("inf")                        # something where the oracle has exactly nothing


@pytest.mark.parametrize("name", list(R.CASES))
def test_emulated_split_arithmetic_is_within_the_bound(name):
    x, g, bd = R.case(name)
    if x.shape[2] * x.shape[3] >= 128 * 128:                                 # the full-K cases, thinned to Cout 4 to stay quick
        g = g[:, :4].contiguous()
        bd = R.Bounds(x, g)
    bd.check(R.emulate(x, g), "emulation, " + name)


def test_emulated_zero_channel_and_impulse_are_exact():
    x = (1 + (torch.arange(2 * 3 * 4 * 5) * 37) % 509).view(2, 3, 4, 5).half()
    g = torch.zeros(2, 4, 4, 5)
    g[1, 2, 3, 4] = 3.0
    got = R.emulate(x, g)
    assert torch.equal(got.double(), R.oracle(x, g)) and float(got[0].abs().max()) == 0 and float(got[2, 1, 0, 0]) == 3 * float(x[1, 1, 2, 3])


def _head(w):
    return postproc.TrainableAggregationHead(w)


def test_host_path_is_conv2d_with_autograd():
    w, x1, x2, src, tgt = R.step_inputs()
    head = _head(w)
    assert [k for k, _ in head.named_parameters()] == ["out.weight"] and isinstance(head.out, torch.nn.Conv2d) and head.out.bias is None
    out = head(x1)
    assert out.dtype == torch.float32 and out.requires_grad and torch.equal(out.detach(), F.conv2d(x1.float(), w, padding=1))
    assert tuple(head(x1[0]).shape) == (8, 12, 12)                           # the reference's unbatched map
    loss = postproc.clip_loss(head(x1), head(x2), src, tgt)[0]
    loss.backward()
    want, bound, ref_err = R.step_bounds()
    err = R.channel_error(head.out.weight.grad, want)
    print("host training step: worst channel error %.3e, bound %.3e (reference fp32 chain: %.3e)" % (err, bound, ref_err))
    assert err <= bound
    head.eval()
    assert torch.equal(head(x1).detach(), out.detach())
    head.train()
    assert float(head.logit_scale.exp()) == pytest.approx(1 / 0.07) and not isinstance(head.logit_scale, torch.nn.Parameter)
    assert "logit_scale" not in head.state_dict()


def test_cin_cout_constructor_uses_conv2d_initialisation():
    torch.manual_seed(5)
    head = postproc.TrainableAggregationHead(6, 4)
    torch.manual_seed(5)
    conv = torch.nn.Conv2d(6, 4, 3, padding=1, bias=False)
    assert torch.equal(head.out.weight, conv.weight) and (head.Cin, head.Cout) == (6, 4)


def test_state_dict_and_checkpoint_round_trips():
    w, _ = R.gen_weight(5, 8, 31)
    w2, _ = R.gen_weight(5, 8, 32)
    head = _head(w)
    assert list(head.state_dict().keys()) == ["out.weight"]
    # what the reference saves loads into the module ...
    net = R.Network(w2)
    buf = io.BytesIO()
    torch.save({"step": 7, "config": {}, "aggregation_network": net.state_dict(), "optimizer_state_dict": {}}, buf)
    buf.seek(0)
    ckpt = torch.load(buf, map_location="cpu")
    head.load_state_dict(ckpt["aggregation_network"])
    assert torch.equal(head.out.weight, w2)
    assert torch.equal(postproc.TrainableAggregationHead(ckpt).out.weight, w2)
    # ... and what the module saves loads into the reference and into AggregationHead
    net1 = R.Network(w)
    net1.load_state_dict(head.state_dict())
    assert torch.equal(net1.out.weight, w2)
    frozen = postproc.AggregationHead({"aggregation_network": head.state_dict()})
    assert torch.equal(frozen.weight, w2) and frozen.bias is None
    assert torch.equal(postproc.AggregationHead(head).weight, w2)            # the module itself is a source
    x = R.gen_features(1, 8, 5, 6, False, 33)
    assert torch.equal(frozen(x), head(x).detach())
    for name, src in __import__("agg_head_ref").sources(w).items():         # every form AggregationHead accepts
        assert torch.equal(postproc.TrainableAggregationHead(src).out.weight, w), name


def test_twenty_steps_lower_the_loss_on_the_cpu():
    x1, x2, src, tgt = R.run_inputs()
    head = _head(R.run_head())
    losses = R.training_run(head, lambda a, b, s, t: postproc.clip_loss(a, b, s, t)[0], x1, x2, src, tgt)
    print("CPU fp32 run: loss %.6f -> %.6f" % (losses[0], losses[-1]))
    assert len(losses) == R.RUN["steps"] + 1 and losses[-1] < losses[0]
    # the same through a plain nn.Conv2d: the fp32 CPU chain of the reference
    net = R.Network(R.run_head())
    ref = R.training_run(net, lambda a, b, s, t: CR._chain_loss(a, b, s, t, CR.SCALE, True), x1.float(), x2.float(), src, tgt)
    assert ref[-1] < ref[0]


def test_value_errors():
    w, b = R.gen_weight(5, 8, 41, bias=True)
    with pytest.raises(ValueError, match="bias"):
        postproc.TrainableAggregationHead(R.Network(w, b))
    with pytest.raises(ValueError, match="bias"):
        postproc.TrainableAggregationHead({"out.weight": w, "out.bias": b})
    with pytest.raises(ValueError):
        postproc.TrainableAggregationHead(8)                                 # Cin without Cout
    with pytest.raises(ValueError):
        postproc.TrainableAggregationHead(8, 0)
    with pytest.raises(ValueError):
        postproc.TrainableAggregationHead(w, 5)                              # Cout beside a source
    with pytest.raises(ValueError):
        postproc.TrainableAggregationHead(torch.zeros(5, 8, 1, 1))
    with pytest.raises(ValueError):
        postproc.TrainableAggregationHead("head.pt")
    head = _head(w)
    with pytest.raises(ValueError):
        head(torch.zeros(1, 9, 4, 4))                                        # the wrong C
    with pytest.raises(ValueError):
        head(torch.zeros(8, 4))


def test_hyperfeature_passes_the_module_through():
    import diffusion_feature
    fe = diffusion_feature.FeatureExtractor.__new__(diffusion_feature.FeatureExtractor)
    w, _ = R.gen_weight(5, 12, 51)
    head = _head(w)
    feats = {"a": R.gen_features(2, 8, 10, 9, False, 52), "b": R.gen_features(2, 4, 5, 5, False, 53)}
    got = fe.hyperfeature(head, feats, (10, 9))
    assert got.requires_grad and torch.equal(got.detach(), head(postproc.aggregate(list(feats.values()), (10, 9))).detach())
    got.sum().backward()
    assert head.out.weight.grad is not None                                  # not frozen into a new AggregationHead on the way


def test_rescale_points_and_compute_pck():
    pts = np.array([[10.0, 20.0], [0.0, 5.0]])                               # (y, x); shapes are (w, h)
    got = postproc.rescale_points(pts, (100, 50), (200, 25))
    assert np.array_equal(got, np.array([[5.0, 40.0], [0.0, 10.0]]))         # y by 25 / 50, x by 200 / 100
    pred = np.array([[0.0, 0.0], [3.0, 4.0], [0.0, 6.0], [30.0, 40.0]])
    tgt = np.zeros((4, 2))
    d, ok, frac = postproc.compute_pck(pred, tgt, (40, 50))                   # threshold 0.1 x 50 = 5: the second point is exactly on it
    assert np.array_equal(d, np.array([0.0, 5.0, 6.0, 50.0])) and ok.tolist() == [True, True, False, False] and frac == 0.5
    d, ok, frac = postproc.compute_pck(pred, tgt, (40, 50), pck_threshold=0.1, target_bounding_box=(10, 20, 70, 50))   # 0.1 x max(60, 30) = 6
    assert ok.tolist() == [True, True, True, False] and frac == 0.75
    d, ok, frac = postproc.compute_pck(pred, tgt, (40, 50), 0.2, (0, 0, 10, 20))                                    # 0.2 x 20 = 4
    assert ok.tolist() == [True, False, False, False] and frac == 0.25


def test_header_declares_the_training_functions():
    src = open(os.path.join(ROOT, "include", "gdf_ops.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bsize_t\s+gdf_agghead_wgrad_workspace\s*\(\s*int\s+B\s*,\s*int\s+Cin\s*,\s*int\s+Cout\s*,\s*int\s+H\s*,\s*int\s+W\s*\)", code)
    assert re.search(r"\bint\s+gdf_agghead_wgrad\s*\(\s*const\s+gdf_agg_src\s*\*\s*x\s*,\s*int\s+B\s*,\s*const\s+float\s*\*\s*grad_out\s*,\s*int\s+Cout"
                     r"\s*,\s*float\s*\*\s*dW\s*,\s*int\s+accumulate\s*,\s*void\s*\*\s*ws\s*,\s*size_t\s+ws_bytes\s*,\s*void\s*\*\s*stream\s*\)", code)
    assert re.search(r"\bint\s+gdf_agghead_create_device\s*\(\s*int\s+Cin\s*,\s*int\s+Cout\s*,\s*const\s+float\s*\*\s*W_dev\s*,\s*const\s+float\s*\*"
                     r"\s*bias_dev\s*,\s*void\s*\*\s*stream\s*,\s*gdf_agghead\s*\*\s*out\s*\)", code)
    assert re.search(r"\bint\s+gdf_agghead_update\s*\(\s*gdf_agghead\s+h\s*,\s*const\s+float\s*\*\s*W_dev\s*,\s*void\s*\*\s*stream\s*\)", code)
    assert len(postproc._SIG["gdf_agghead_wgrad"][1]) == 9 and len(postproc._SIG["gdf_agghead_update"][1]) == 3
    assert len(postproc._SIG["gdf_agghead_create_device"][1]) == 6 and len(postproc._SIG["gdf_agghead_wgrad_workspace"][1]) == 5
