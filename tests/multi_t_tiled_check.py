"""Child process of tests/test_gpu_multi_t.py::test_tiled_single_timestep_calls_without_split_k (run with GDF_SPLITK=0 and
GDF_SYNTHETIC_WEIGHTS=1): rows k*B:(k+1)*B of every feature of extract(t=[50, 400, 50]) on B = 2 images equal, bit for bit, the same rows of
extract(t=t_k) on the images tiled K times — '1-5' (PNDM family, with a '*-map' hook and attention=['up_cross']) and 'xl' (Euler family, added
conditioning), 128 x 128.  Exit status 0 and a last line "tiled check ok" when every row agrees."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "generic-diffusion-feature_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402
import diffusion_feature  # noqa: E402

B, TS, IMG = 2, [50, 400, 50], 128
K = len(TS)
LAYERS = {
    "1-5": {"up-level1-repeat1-vit-block0-cross-q": True, "up-level2-repeat2-res-out": True, "up-level2-repeat0-vit-block0-cross-map": True},
    "xl": {"up-level1-repeat1-vit-block0-out": True, "up-level2-repeat2-res-out": True, "up-level1-repeat0-vit-block0-cross-map": True},
}
assert os.environ.get("GDF_SPLITK") == "0" and os.environ.get("GDF_SYNTHETIC_WEIGHTS") == "1"
bad = 0
for version, layer in LAYERS.items():
    df = diffusion_feature.FeatureExtractor(layer=dict(layer), version=version, img_size=IMG, device="cuda:0",
                                            attention=["up_cross"] if version == "1-5" else None)
    prompt = df.encode_prompt("a photo of a cat")
    img = torch.rand(B, 3, IMG, IMG, generator=torch.Generator().manual_seed(5)) * 2 - 1
    torch.manual_seed(0)
    multi = {k: v.clone() for k, v in df.extract(prompt, batch_size=B, image=img, image_type="tensors", t=TS).items()}
    tiled = img.repeat(K, 1, 1, 1)
    for k, t in enumerate(TS):
        torch.manual_seed(0)
        single = df.extract(prompt, batch_size=K * B, image=tiled, image_type="tensors", t=t)
        assert list(single.keys()) == list(multi.keys())
        rows = slice(k * B, (k + 1) * B)
        for hid in multi:
            n = int((multi[hid][rows] != single[hid][rows]).sum())
            print("%s %s t=%d rows %d:%d: %d of %d elements differ" % (version, hid, t, rows.start, rows.stop, n, multi[hid][rows].numel()))
            bad += n > 0
        del single
    del df, multi
torch.cuda.synchronize()
if bad:
    print("tiled check FAILED: %d (hook, timestep) groups differ" % bad)
    sys.exit(1)
print("tiled check ok")
