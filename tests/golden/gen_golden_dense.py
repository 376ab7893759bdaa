"""Golden file of dense matching from the REFERENCE's own code (build container only).

    python tests/golden/gen_golden_dense.py        # needs /root/reference and scikit-learn; writes tests/golden/dense_match.npz

Runs, on the CPU in fp32 and imported at run time, the reference's
  batch_cosine_sim + find_nn_correspondences   (correspondence/correspondence/correspondence_utils.py:73-111) on two pairs of small seeded maps, and
  find_best_buddies_correspondences            (:230-323) on B x 1 x T x D descriptors with saliencies,
and records inputs and outputs.  The module imports torchvision and matplotlib, which the functions run here do not use: empty stand-in modules
take their place where they are missing.  The fixture is pure data.

The intermediate results recorded beside the best-buddies points (the mutual mask with the saliency conditions, nn_1, nn_2) are recomputed
here with the reference's own chunk_cosine_sim, line for line as the function does."""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/correspondence/correspondence"

# name: (C, (h, w) of both maps, fp32?)
NN_CASES = {"nn_fp16": (24, (12, 12), False), "nn_fp32": (20, (11, 11), True)}
# name: (T = n * n tokens, D, num_pairs, thresh)
BB_CASES = {"bb": (144, 24, 6, 0.05)}


def smooth(v):
    p = torch.nn.functional.pad(v, (1, 1, 1, 1), mode="replicate")
    return torch.nn.functional.avg_pool2d(p, 3, stride=1)


def nn_inputs(name):
    C, g, f32 = NN_CASES[name]
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    f1 = torch.randn(1, C, *g, generator=gen)
    f2 = torch.roll(f1, (3, -2), (2, 3)) + 0.7 * torch.randn(1, C, *g, generator=gen)     # related maps: a shifted copy plus noise
    return (f1, f2) if f32 else (f1.half(), f2.half())


def bb_inputs(name):
    T, D, _, _ = BB_CASES[name]
    n = int(np.sqrt(T))
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    d1 = smooth(torch.randn(1, D, n, n, generator=gen)) * 3
    d2 = d1 + 0.35 * torch.randn(1, D, n, n, generator=gen)
    d1, d2 = (v.flatten(2).permute(0, 2, 1)[:, None].contiguous() for v in (d1, d2))      # B x 1 x T x D
    s1, s2 = torch.rand(1, T, generator=gen) * 0.2, torch.rand(1, T, generator=gen) * 0.2  # about a quarter below thresh = 0.05
    return d1, d2, s1, s2


def main():
    for mod in ("torchvision", "matplotlib", "matplotlib.pyplot", "matplotlib.colors"):
        try:
            importlib.import_module(mod)
        except ImportError:
            m = types.ModuleType(mod)
            m.ListedColormap = None
            sys.modules[mod] = m
    sys.path.insert(0, REF)
    import correspondence_utils as R
    arrs = {}
    for name in NN_CASES:
        f1, f2 = nn_inputs(name)
        sims = R.batch_cosine_sim(f1.float(), f2.float())
        p1, p2 = R.find_nn_correspondences(sims)
        assert p1.dtype == torch.float32 and p2.dtype == torch.float32 and p1.shape == p2.shape == (1, sims.shape[-1], 2)
        arrs[name + ":f1"], arrs[name + ":f2"] = f1.numpy(), f2.numpy()
        arrs[name + ":points1"], arrs[name + ":points2"] = p1.numpy(), p2.numpy()
        arrs[name + ":nn12"], arrs[name + ":nn21"] = sims.argmax(-1).numpy(), sims.argmax(-2).numpy()
        arrs[name + ":sim12"], arrs[name + ":sim21"] = sims.max(-1)[0].numpy(), sims.max(-2)[0].numpy()
    for name in BB_CASES:
        d1, d2, s1, s2 = bb_inputs(name)
        T, D, k, thresh = BB_CASES[name]
        p1, p2 = R.find_best_buddies_correspondences(d1, d2, s1, s2, num_pairs=k, thresh=thresh)
        sims = R.chunk_cosine_sim(d1, d2)
        sim_1, nn_1 = torch.max(sims, dim=-1)
        sim_2, nn_2 = torch.max(sims, dim=-2)
        nn_1, nn_2 = nn_1[0, 0], nn_2[0, 0]
        mask = nn_2[nn_1] == torch.arange(T)
        fg = torch.zeros(T, dtype=torch.bool)
        fg[nn_2[s2[0] > thresh]] = True
        mask = mask & (s1[0] > thresh) & fg
        assert len(p1) == k and int(mask.sum()) > k, (len(p1), int(mask.sum()))
        arrs[name + ":d1"], arrs[name + ":d2"], arrs[name + ":s1"], arrs[name + ":s2"] = d1.numpy(), d2.numpy(), s1.numpy(), s2.numpy()
        arrs[name + ":args"] = np.array([k, thresh])
        arrs[name + ":mask"], arrs[name + ":nn12"], arrs[name + ":nn21"] = mask.numpy(), nn_1.numpy(), nn_2.numpy()
        arrs[name + ":sim12"] = sim_1[0, 0].numpy()
        arrs[name + ":points1"], arrs[name + ":points2"] = torch.as_tensor(p1).numpy(), torch.as_tensor(p2).numpy()
    out = os.path.join(HERE, "dense_match.npz")
    np.savez_compressed(out, **arrs)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
