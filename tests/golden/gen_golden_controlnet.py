"""Golden vectors of the UNet forward WITH ControlNet residuals, from the REFERENCE's own UNet2DConditionModel.forward (build container only).

    python tests/golden/gen_golden_controlnet.py      # needs the reference tree; writes tests/golden/unet_tiny_residuals_{xl,15}.npz

As gen_golden_unet.py: oracle/ref_unet.py drives the reference's unet_2d_condition.py (here its `down_block_additional_residuals` /
`mid_block_additional_residual` branch, :1194, 1236-1245, 1269-1270) over the reference's own blocks on a shrunken architecture, with the
reference's accept-all feature store.  A fixture holds pure data: the seeded inputs, the ordered hook ids the reference stored and per hook its
shape, L2 norm and 1024 seeded sample positions with their fp32 values.  The weights and the residuals are regenerated from their seeds
(oracle.unet_ref.synth_params, tests/controlnet_oracle.py synth_residuals); the fixture pins the residuals by per-tensor checksums."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import controlnet_oracle as CO  # noqa: E402
from oracle import ref_unet as RU, unet_ref as R  # noqa: E402

NS = 1024
RES_SEED, RES_SCALE = 7, 0.5


def sample_idx(numel, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, numel, (min(NS, numel),), generator=g)


def main():
    for tag, base, lat, batch in (("xl", "xl", 16, 2), ("15", "1-5", 16, 1)):
        c0 = 320 if base == "1-5" else 64
        arch = R.tiny_arch(base, time_embed_dim=4 * c0)           # the reference derives time_embed_dim = 4 * block_out_channels[0]
        net = RU.build_reference_unet(arch).eval()
        P = R.synth_params(arch, seed=0)
        net.load_state_dict(P)
        _, prep, _ = RU.reference_unet_class()
        store = prep(base, types.SimpleNamespace(unet=net), None, 1, True)    # accept-all; train_unet=True keeps tensors on the CPU
        I = R.synth_inputs(arch, batch, lat, seed=1, same_prompt=False)
        down, mid = CO.synth_residuals(arch, batch, lat, seed=RES_SEED, scale=RES_SCALE)
        akw = {"text_embeds": I["text_embeds"], "time_ids": I["time_ids"]} if "text_embeds" in I else None
        with torch.no_grad():
            y = net(I["sample"], I["timestep"][0], I["ctx"], added_cond_kwargs=akw, down_block_additional_residuals=tuple(down),
                    mid_block_additional_residual=mid, return_dict=False)[0]
        arrs = {"in:" + k: v.numpy() for k, v in I.items()}
        arrs["res_sum"] = np.array([float(t.double().sum()) for t in down + [mid]])
        arrs["res_abs"] = np.array([float(t.double().abs().sum()) for t in down + [mid]])
        order = list(store.stored_feats.keys())
        for n, (k, v) in enumerate(store.stored_feats.items()):
            v = v.float().contiguous()
            idx = sample_idx(v.numel(), n)
            arrs["hook:" + k] = v.flatten()[idx].numpy()
            arrs["norm:" + k] = np.float64(v.double().norm().item())
            arrs["shape:" + k] = np.array(v.shape)
        arrs["out"] = y.numpy()
        arrs["meta"] = np.array(repr(dict(base=base, arch=arch, lat=lat, batch=batch, wseed=0, res_seed=RES_SEED, res_scale=RES_SCALE,
                                          order=order, ns=NS)))
        path = os.path.join(HERE, f"unet_tiny_residuals_{tag}.npz")
        np.savez_compressed(path, **arrs)
        print(tag, len(order), "hooks ->", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
