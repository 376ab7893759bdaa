#!/usr/bin/env python3
"""(image, timestep) pairs per second of ONE extract(t=[t1..tK]) against K single-timestep extract() calls, same process, same extractor:
SDXL 1024^2 batch 16 and SD1.5 512^2 batch 32, practical layer sets, synthetic weights, K in {1, 2, 4}.

Method: every (configuration, K) warms both forms up (plans, graphs, hook-buffer pools), then runs `--rounds` rounds that ALTERNATE a window of
the K single calls and a window of the multi call; a window is `--iters` repetitions ended by a device synchronise (host clock around it).
Reported per form: the median window and the min..max spread over the rounds, as pairs/s = K * B * iters / window.  The single-timestep
path is the one every earlier version of the project has, so "single" is the baseline.  K = 1 compares t=[T] with t=T.

    python tools/bench_multi_t.py [--configs xl,1-5] [--ks 1,2,4] [--rounds 5] [--iters 3] [--out profiles/multi_t_extract.txt]
"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "generic-diffusion-feature_amd")):
    sys.path.insert(0, p)
import torch
os.environ.setdefault("GDF_SYNTHETIC_WEIGHTS", "1")
import diffusion_feature
import bench as BB

CONFIGS = {"xl": dict(version="xl", img=1024, batch=16), "1-5": dict(version="1-5", img=512, batch=32)}
TIMESTEPS = [100, 300, 500, 700]

ap = argparse.ArgumentParser()
ap.add_argument("--configs", default="xl,1-5"); ap.add_argument("--ks", default="1,2,4")
ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--iters", type=int, default=3)
ap.add_argument("--out", default=None, help="also write the report to this file")
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_multi_t.py measures on the GPU; there is none")

lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


say("# extract(t=[t1..tK]) vs K x extract(t=tk): (image, timestep) pairs per second; median [min .. max] over %d alternating rounds of %d "
    "repetitions" % (a.rounds, a.iters))
say("# device: %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
results = []
for name in a.configs.split(","):
    c = CONFIGS[name]
    B, S = c["batch"], c["img"]
    df = diffusion_feature.FeatureExtractor({k: True for k in BB.PRACTICAL[c["version"]]}, c["version"], device="cuda:0", img_size=S)
    prompts = df.encode_prompt("a photo of a cat")
    img = (torch.rand(B, 3, S, S, generator=torch.Generator().manual_seed(0)) * 2 - 1).half().cuda()

    def single(ts):
        for t in ts:
            f = df.extract(prompts, B, img, image_type="tensors", t=t)
            del f

    def multi(ts):
        f = df.extract(prompts, B, img, image_type="tensors", t=list(ts))
        del f

    def window(fn, ts):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        with torch.no_grad():
            for _ in range(a.iters):
                fn(ts)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    say()
    say("## %s %dx%d, batch %d, %d practical layers" % (c["version"], S, S, B, len(BB.PRACTICAL[c["version"]])))
    for K in [int(k) for k in a.ks.split(",")]:
        ts = TIMESTEPS[:K]
        with torch.no_grad():
            for _ in range(3):                       # warm-up of every shape both forms use
                single(ts); multi(ts)
        w = {"single": [], "multi": []}
        for _ in range(a.rounds):
            w["single"].append(window(single, ts))
            w["multi"].append(window(multi, ts))
        rate = lambda dt: K * B * a.iters / dt
        row = {"config": name, "K": K, "batch": B}
        for form in ("single", "multi"):
            r = sorted(rate(dt) for dt in w[form])
            row[form] = {"median": statistics.median(r), "min": r[0], "max": r[-1], "ms_per_call_set": 1e3 * statistics.median(w[form]) / a.iters}
        row["speedup_median"] = row["multi"]["median"] / row["single"]["median"]
        results.append(row)
        say("K=%d  %-28s %8.1f pairs/s  [%7.1f .. %7.1f]   %7.1f ms per K timesteps" % (
            K, "%d x extract(t=int)" % K, row["single"]["median"], row["single"]["min"], row["single"]["max"], row["single"]["ms_per_call_set"]))
        say("K=%d  %-28s %8.1f pairs/s  [%7.1f .. %7.1f]   %7.1f ms per K timesteps   x%.3f" % (
            K, "1 x extract(t=[%d values])" % K, row["multi"]["median"], row["multi"]["min"], row["multi"]["max"], row["multi"]["ms_per_call_set"],
            row["speedup_median"]))
    del df, img
    torch.cuda.empty_cache()
say()
say(json.dumps({"multi_t_extract": results}))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
