"""Golden file of the correspondence loss from the REFERENCE's own code (build container only).

    python tests/golden/gen_golden_clip_loss.py        # needs /root/reference; writes tests/golden/clip_loss.npz

Runs the reference's compute_clip_loss (correspondence/task-corres.py:70-80), loaded at run time from the file by path, on the CPU in fp32 on three
small seeded cases, with torch's autograd for the gradients of both maps.  The script imports diffusion_feature (through its aggregation network)
and torchvision, which none of the functions used here touch: stand-in modules take their places (empty but for the name FeatureExtractor).
The fixture is pure data: per case the two maps, the points (float64, (y, x) in output-size coordinates, some out of range, some on .5), the
output size, the loss and the two gradients."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/correspondence"

# name: (C, output size = the maps' grid, fp32 maps?, N, smoothed?)
CASES = {"c40_6x6": (40, 6, False, 20, False),
         "smoothed_9x9": (16, 9, False, 70, True),
         "f32_8x8": (72, 8, True, 24, False)}


def smooth(v):
    """3 x 3 box filter with edge replication: neighbouring pixels correlate, as real features do"""
    p = torch.nn.functional.pad(v, (1, 1, 1, 1), mode="replicate")
    return torch.nn.functional.avg_pool2d(p, 3, stride=1)


def inputs(name):
    C, L, f32, N, sm = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    f1, f2 = torch.randn(1, C, L, L, generator=g), torch.randn(1, C, L, L, generator=g)
    if sm:
        f1, f2 = smooth(f1), smooth(f2)
    if not f32:
        f1, f2 = f1.half(), f2.half()
    pts = (torch.rand(2, N, 2, generator=g, dtype=torch.float64) * 1.2 - 0.1) * L       # uniform over [-0.1 L, 1.1 L): some out of range
    pts[:, :6] = torch.floor(pts[:, :6]) + 0.5                                          # .5: half to even
    return f1, f2, pts[0].numpy(), pts[1].numpy(), L


def load_reference():
    for name in ("torchvision", "diffusion_feature"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["diffusion_feature"].FeatureExtractor = None                            # the one name aggregation_network.py imports from it
    sys.path.insert(0, REF)
    spec = importlib.util.spec_from_file_location("task_corres", os.path.join(REF, "task-corres.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    R = load_reference()
    net = types.SimpleNamespace(logit_scale=torch.ones([]) * np.log(1 / 0.07))          # aggregation_network.py:25
    arrs = {}
    for name in CASES:
        f1, f2, sp, tp, L = inputs(name)
        a, b = f1.float().clone().requires_grad_(True), f2.float().clone().requires_grad_(True)
        loss = R.compute_clip_loss(net, a, b, sp, tp, (L, L))
        assert loss.dim() == 0 and loss.dtype == torch.float32
        loss.backward()
        arrs[name + ":f1"], arrs[name + ":f2"] = f1.numpy(), f2.numpy()
        arrs[name + ":source_points"], arrs[name + ":target_points"], arrs[name + ":output_size"] = sp, tp, np.array([L, L])
        arrs[name + ":loss"], arrs[name + ":grad_f1"], arrs[name + ":grad_f2"] = loss.detach().numpy(), a.grad.numpy(), b.grad.numpy()
    out = os.path.join(HERE, "clip_loss.npz")
    np.savez_compressed(out, **arrs)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
