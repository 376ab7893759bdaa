"""Golden file of the correspondence step from the REFERENCE's own code (build container only).

    python tests/golden/gen_golden_corres.py        # needs /root/reference; writes tests/golden/corres_nn.npz

Runs the reference's find_nn_source_correspondences (correspondence/correspondence/correspondence_utils.py:113-138), imported at run time, on the
CPU in fp32 on three small seeded cases of tests/test_gpu_correspond.py and records inputs and outputs.  The module imports torchvision, which only
its process_image uses: an empty stand-in module takes its place.  The fixture is pure data: per case the two feature maps, the points (float64,
(y, x), some out of range, some on .5), the load size and the reference's points2."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/correspondence/correspondence"

# name: (C, (h1, w1), fp32 source?, (h2, w2), load size, N, smoothed?)
CASES = {"x4": (40, (6, 6), False, (6, 6), 24, 64, False),
         "ratio_10_3": (16, (9, 9), False, (9, 9), 30, 64, True),
         "two_grids": (136, (9, 9), True, (12, 12), 48, 70, False)}


def smooth(v):
    """3 x 3 box filter with edge replication: neighbouring pixels correlate, as real features do"""
    p = torch.nn.functional.pad(v, (1, 1, 1, 1), mode="replicate")
    return torch.nn.functional.avg_pool2d(p, 3, stride=1)


def inputs(name):
    C, g1, f32, g2, L, N, sm = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    f1, f2 = torch.randn(1, C, *g1, generator=g), torch.randn(1, C, *g2, generator=g)
    if sm:
        f1, f2 = smooth(f1), smooth(f2)
    f1 = f1 if f32 else f1.half()
    f2 = f2.half()
    pts = (torch.rand(N, 2, generator=g, dtype=torch.float64) * 1.2 - 0.1) * L          # uniform over [-0.1 L, 1.1 L): some out of range
    pts[:8] = torch.floor(pts[:8]) + 0.5                                                # .5: half to even
    return f1, f2, pts.numpy(), L


def main():
    sys.modules.setdefault("torchvision", types.ModuleType("torchvision"))
    sys.path.insert(0, REF)
    import correspondence_utils as R
    arrs = {}
    for name in CASES:
        f1, f2, pts, L = inputs(name)
        p1, p2 = R.find_nn_source_correspondences(f1.float(), f2.float(), pts, None, (L, L))
        assert p2.dtype == torch.int64 and tuple(p2.shape) == (pts.shape[0], 2) and p1.dtype == torch.float64
        arrs[name + ":f1"], arrs[name + ":f2"], arrs[name + ":points"] = f1.numpy(), f2.numpy(), pts
        arrs[name + ":load_size"], arrs[name + ":points2"] = np.array([L, L]), p2.numpy()
    out = os.path.join(HERE, "corres_nn.npz")
    np.savez_compressed(out, **arrs)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
