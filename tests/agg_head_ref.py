"""Float64 oracle, seeded generators, acceptance rule and ctypes binding of the aggregation-network head (gdf_agghead_*, components/postproc.py
AggregationHead, FeatureExtractor.hyperfeature), shared by tests/test_agg_head_cpu.py and tests/test_gpu_agg_head.py.

The op (reference correspondence/correspondence/aggregation_network.py:20-22, 97-100): x.type(torch.float32) and nn.Conv2d(dim, out_dim,
kernel_size=3, stride=1, padding=1, bias=False) on the aggregated map.

Oracle: F.conv2d in float64 from the inputs as given (an fp16 map is exact in float64).
Reference arithmetic: F.conv2d in fp32 on the CPU, what the reference's head computes.
Bound: no fixed constant.  The error is the relative L2 error per block of 16 consecutive pixels (p = (b H + y) W + x) over all Cout against the
oracle; a result passes when its worst block is within MARGIN = 8 x the worst block of the reference arithmetic on the same inputs: the rule and
the margin of pixel_classifier_ref.Bounds (the project's margin for a different fp32 summation order).
Generators (seeded): weights randn / sqrt(9 Cin) times a per-output-channel scale in [0.25, 4] (log-uniform), fp32; features as
pixel_classifier_ref.gen_features (randn times a per-channel scale in [0.25, 4])."""
import ctypes as C

import torch
import torch.nn.functional as F

from pixel_classifier_ref import BLOCK, MARGIN, agg_src, block_rel, gen_features  # noqa: F401

GDF_ERR_ARG = 1
vp, ci = C.c_void_p, C.c_int


def bind(L):
    L.gdf_agghead_create.restype, L.gdf_agghead_create.argtypes = ci, [ci, ci, vp, vp, C.POINTER(vp)]
    L.gdf_agghead_destroy.restype, L.gdf_agghead_destroy.argtypes = None, [vp]
    L.gdf_agghead_forward.restype, L.gdf_agghead_forward.argtypes = ci, [vp, vp, ci, vp, vp]
    L.gdf_last_error.restype = C.c_char_p
    return L


def gen_weight(Cout, Cin, seed, bias=False):
    """-> (weight (Cout, Cin, 3, 3) fp32, bias (Cout) fp32 or None)"""
    g = torch.Generator().manual_seed(seed)
    scale = 0.25 * 16.0 ** torch.rand(Cout, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5 * scale[:, None, None, None]
    return w.float().contiguous(), (0.3 * torch.randn(Cout, generator=g)).float() if bias else None


def oracle(w, bias, v):
    """-> (B, Cout, H, W) float64"""
    return F.conv2d(v.double(), w.double(), bias.double() if bias is not None else None, padding=1)


def reference(w, bias, v):
    """the reference's arithmetic: x.type(torch.float32), nn.Conv2d on the CPU -> (B, Cout, H, W) fp32"""
    return F.conv2d(v.float(), w, bias, padding=1)


def pixels(t):
    """(B, Cout, H, W) -> (1, P, Cout), pixel p = (b H + y) W + x: the layout pixel_classifier_ref.block_rel takes"""
    return t.permute(0, 2, 3, 1).reshape(1, -1, t.shape[1])


def block_error(got, want):
    """worst relative L2 error over the blocks of 16 consecutive pixels, all Cout, against the float64 oracle"""
    rel = block_rel(pixels(got), pixels(want))
    return float(rel.max()) if bool(torch.isfinite(rel).all()) else float("inf")


class Bounds:
    """the bound of one case, taken from the reference's fp32 arithmetic on that case's inputs"""

    def __init__(self, w, bias, v):
        self.oracle = oracle(w, bias, v)
        self.ref_err = block_error(reference(w, bias, v), self.oracle)
        self.bound = MARGIN * self.ref_err

    def check(self, got, what=""):
        assert tuple(got.shape) == tuple(self.oracle.shape), (what, tuple(got.shape), tuple(self.oracle.shape))
        err = block_error(got, self.oracle)
        print("aggregation head %s: worst block error %.3e, bound %.3e (reference fp32: %.3e)" % (what, err, self.bound, self.ref_err))
        assert err <= self.bound, (what, err, self.bound)
        return err


class Network(torch.nn.Module):
    """stand-in of the reference's AggregationNetwork: the same `out` convolution and state-dict key (its __init__ loads diffusion pipelines)"""

    def __init__(self, w, bias=None):
        super().__init__()
        self.out = torch.nn.Conv2d(w.shape[1], w.shape[0], kernel_size=3, stride=1, padding=1, bias=bias is not None)
        with torch.no_grad():
            self.out.weight.copy_(w)
            if bias is not None:
                self.out.bias.copy_(bias)
        self.logit_scale = torch.ones([])

    def forward(self, x):
        return self.out(x.type(torch.float32))


def sources(w, bias=None):
    """every form AggregationHead accepts, by name"""
    net = Network(w, bias)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    out = {"network": net, "conv2d": net.out, "state dict": sd, "module. state dict": {"module." + k: v for k, v in sd.items()},
           "checkpoint": {"aggregation_network": sd, "optimizer": {}, "epoch": 3}}
    if bias is None:
        out["weight"] = w.clone()
    return out
