"""Makes tests/golden/pca_vis.npz: two small fp16 feature maps and the pixels of the PNG the reference's own plot_pca writes for each.

    python tests/golden/gen_golden_pca.py --reference <reference checkout>/feature_visualization.py

The reference file is a script whose settings run at import, so it is not imported: its `plot_pca` function is located with `ast`, compiled from
the file at run time and executed with the names it uses (PCA, Image, sqrt, np) and a stand-in for torchvision's `Resize(512, NEAREST)`, which
calls Pillow's nearest resize as torchvision does for a PIL image.  Nothing of the reference is stored but the pixels it produced.  Needs
scikit-learn and Pillow; run once, no test needs it.  The seeds are searched so that no value of either input lies where a float32 computation
could round to the other integer (tests/pca_ref.py Bounds.excluded): the tests assert equality outright."""
import argparse
import ast
import os
import sys
import tempfile
from math import sqrt

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "generic-diffusion-feature_amd"))
import pca_ref as R  # noqa: E402

INPUTS = (("c24_10x10", "planted", 24, 10), ("c77_12x12", "planted", 77, 12))


class _Transforms:
    """what plot_pca uses of torchvision.transforms"""

    class InterpolationMode:
        NEAREST = "nearest"

    class Resize:
        def __init__(self, size, interpolation=None):
            self.size = size

        def __call__(self, img):
            from PIL import Image
            w, h = img.size
            ow, oh = (self.size, int(self.size * h / w)) if w <= h else (int(self.size * w / h), self.size)
            return img.resize((ow, oh), Image.NEAREST)


def load_plot_pca(path):
    from PIL import Image
    from sklearn.decomposition import PCA
    tree = ast.parse(open(path).read(), path)
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "plot_pca"]
    assert len(fn) == 1, "no plot_pca in " + path
    ns = dict(PCA=PCA, Image=Image, sqrt=sqrt, np=np, T=_Transforms)
    exec(compile(ast.Module(body=fn, type_ignores=[]), path, "exec"), ns)
    return ns["plot_pca"]


def main():
    from PIL import Image
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference's feature_visualization.py")
    ap.add_argument("--out", default=os.path.join(HERE, "pca_vis.npz"))
    args = ap.parse_args()
    plot_pca = load_plot_pca(args.reference)
    data = {}
    for name, kind, C_, S in INPUTS:
        for seed in range(1000):
            x = R.features(kind, 1, C_, S, S, seed)
            bd = R.Bounds(x, 3, False, 512)
            if not bd.excluded().any():
                break
        else:
            raise SystemExit("no seed without a value in the excluded zone for " + name)
        with tempfile.TemporaryDirectory() as tmp:
            png = os.path.join(tmp, "0.png")
            plot_pca(x[0].reshape(C_, -1).transpose(), png)                  # d x h x w -> n x d, as the reference's caller does
            pix = np.array(Image.open(png))
        assert pix.shape == (512, 512, 3) and pix.dtype == np.uint8
        print(name, "seed", seed, "pixels equal to the oracle:", bool(np.array_equal(pix, bd.want["u8"][0])))
        data[name + ":x"], data[name + ":png"], data[name + ":seed"] = x, pix, np.int64(seed)
    np.savez_compressed(args.out, **data)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
