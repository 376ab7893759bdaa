"""Golden file of the label-scarce segmentation step from the REFERENCE's own code (build container only).

    python tests/golden/gen_golden_pixel.py        # needs /root/reference; writes tests/golden/pixel_classifier.npz

Runs the reference's pixel_classifier modules and predict_labels (scarce_segmentation/segmentation/pixel_classifier.py:14-107), imported at run
time, on the CPU in fp32 on two small seeded ensembles, one per architecture, and records inputs and outputs.  predict_labels moves its input with
`.cuda()`; inside this script only, that method is the identity.  The fixture is pure data: per case the state dicts (the keys nn.DataParallel
saves for the first case, plain keys for the second), the (P, dim) feature matrix, the size, and the reference's labels and top_k."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/scarce_segmentation"
sys.path.insert(0, os.path.dirname(HERE))
import pixel_classifier_ref as R  # noqa: E402

# name: (dim, classes, M, (H, W), fp32 features?, state-dict key prefix)
CASES = {"small": (24, 5, 3, (16, 16), False, "module."),
         "large": (16, 34, 3, (16, 16), True, "")}


def main():
    sys.path.insert(0, REF)
    from segmentation import pixel_classifier as PC
    torch.Tensor.cuda = lambda self, *a, **k: self
    arrs = {}
    for name, (dim, K, M, size, f32, prefix) in CASES.items():
        seed = sum(map(ord, name))
        sds = R.gen_models(dim, M, K, seed)
        models = []
        for sd in sds:
            net = PC.pixel_classifier(K, dim)
            net.load_state_dict(sd)
            models.append(net.eval())
        feats = R.gen_features(1, dim, *size, f32, seed + 1)
        x = feats[0].reshape(dim, -1).permute(1, 0)                                      # the (P, dim) view of task-pixel.py:100
        labels, top_k = PC.predict_labels(models, x.float(), size=size)
        assert labels.dtype == torch.int64 and tuple(labels.shape) == size and top_k.dim() == 0
        for m, sd in enumerate(sds):
            for k, v in sd.items():
                arrs["%s:model%d:%s%s" % (name, m, prefix, k)] = v.numpy()
        arrs[name + ":features"], arrs[name + ":size"] = x.contiguous().numpy(), np.array(size)
        arrs[name + ":labels"], arrs[name + ":top_k"] = labels.numpy(), top_k.numpy()
    out = os.path.join(HERE, "pixel_classifier.npz")
    np.savez_compressed(out, **arrs)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
