"""PCA pictures of a saved feature file: the counterpart of the reference's feature_visualization.py, whose settings are arguments here.

    python feature_visualization.py --input up-level0-repeat0-vit-block5-out.npy --block_divide 1280 --output ./vis --task_name block5
    python feature_visualization.py --input agg.npy --block_divide 1280 640 --have_attn --attn_type up_cross down_cross --attn_len 77 ...

--input is one (C, H, W) array as extract_feature.py writes it: first the hooked layers (--block_divide: the channels of each, in order), then,
with --have_attn, the aggregated attention maps: for every --attn_type in order, one group of --attn_len token maps per query-grid size.  Written
under <output>/<task_name>/:

    base/{i}.png                 the PCA picture of layer i (components/postproc.py pca_rgb: gdf_op_pca + gdf_op_pca_rgb on --device cuda)
    attn/<type>/{i}.png          the PCA picture of the i-th group of token maps of that type
    attn/<type>/<i>/<j>.png      token j of that group in grey: 255 a / max(a), 256 x 256 (Pillow, on the host)
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "generic-diffusion-feature_amd"))


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="PCA pictures of a saved feature file")
    p.add_argument("--input", required=True, help="a (C, H, W) .npy file")
    p.add_argument("--block_divide", type=int, nargs="*", default=[], help="channels of every hooked layer in the file, in order")
    p.add_argument("--no_base", action="store_true", help="the file holds attention maps only")
    p.add_argument("--have_attn", action="store_true", help="attention maps follow the hooked layers")
    p.add_argument("--attn_type", nargs="*", default=["up_cross"], help="the attention categories in the file, in order")
    p.add_argument("--attn_len", type=int, default=77, help="token maps per group")
    p.add_argument("--size", type=int, default=512, help="short side of the PCA pictures")
    p.add_argument("--output", default="./vis")
    p.add_argument("--task_name", default=None, help="sub-directory of --output (default: the input's file name)")
    p.add_argument("--device", default=None, help="cuda (default when there is one) or cpu")
    return p.parse_args(argv)


def split_channels(feat, sizes, what):
    out, at = [], 0
    for c in sizes:
        if c < 1 or at + c > feat.shape[0]:
            raise SystemExit(f"{what}: {list(sizes)} does not fit {feat.shape[0]} channels")
        out.append(feat[at:at + c])
        at += c
    return out, feat[at:]


def save_pca(maps, paths, size, device):
    """one picture per (C, H, W) array; maps of one shape go through the op as one batch of independent PCAs"""
    import torch
    from PIL import Image
    from components.postproc import pca_rgb
    by_shape = {}
    for m, path in zip(maps, paths):
        by_shape.setdefault(m.shape, []).append((m, path))
    for group in by_shape.values():
        x = torch.from_numpy(np.stack([m for m, _ in group]))
        x = x if x.dtype in (torch.float16, torch.float32, torch.float64) else x.float()
        pics = pca_rgb(x.to(device), size).cpu().numpy()
        for pic, (_, path) in zip(pics, group):
            Image.fromarray(pic).save(path)


def main(argv=None):
    args = parse_args(argv)
    import torch
    from PIL import Image
    device = args.device or ("cuda" if torch.cuda.is_available() else "cpu")
    feat = np.load(args.input)
    if feat.ndim != 3:
        raise SystemExit(f"--input holds a {feat.ndim}-D array; a (C, H, W) feature file is expected")
    out_dir = os.path.join(args.output, args.task_name or os.path.splitext(os.path.basename(args.input))[0])
    os.makedirs(out_dir, exist_ok=True)
    rest = feat
    if not args.no_base:
        if not args.block_divide:
            args.block_divide = [feat.shape[0]]
        layers, rest = split_channels(feat, args.block_divide, "--block_divide")
        os.makedirs(os.path.join(out_dir, "base"), exist_ok=True)
        save_pca(layers, [os.path.join(out_dir, "base", f"{i}.png") for i in range(len(layers))], args.size, device)
    if args.have_attn:
        n_type = len(args.attn_type)
        if n_type < 1 or args.attn_len < 1 or rest.shape[0] == 0 or rest.shape[0] % (n_type * args.attn_len):
            raise SystemExit(f"{rest.shape[0]} attention channels are not {n_type} type(s) x groups of {args.attn_len} tokens")
        per_type = rest.shape[0] // n_type
        for t, name in enumerate(args.attn_type):
            block = rest[t * per_type:(t + 1) * per_type]
            groups = [block[i:i + args.attn_len] for i in range(0, per_type, args.attn_len)]
            for i in range(len(groups)):
                os.makedirs(os.path.join(out_dir, "attn", name, str(i)), exist_ok=True)
            save_pca(groups, [os.path.join(out_dir, "attn", name, f"{i}.png") for i in range(len(groups))], args.size, device)
            for i, maps in enumerate(groups):
                for j, a in enumerate(maps):
                    grey = (255 * a / a.max()).astype(np.uint8)
                    Image.fromarray(np.repeat(grey[:, :, None], 3, axis=2)).resize((256, 256)).save(
                        os.path.join(out_dir, "attn", name, str(i), f"{j}.png"))
    return out_dir


if __name__ == "__main__":
    main()
