#!/usr/bin/env python3
"""extract(image_type='image') with the PIL-to-tensor step on the host (the thread pool of diffusion_feature._map_threads) against the same step
on the device (FeatureExtractor(device_preprocess=True), components/preproc.py), same process, same extractor — the flag is the only thing
that differs: SDXL 1024^2 batch 16 and SD1.5 512^2 batch 32, practical layer sets, synthetic weights, PIL sources of 2048 x 1024 and of
exactly img_size.

The caller modelled is one that READS a feature after every call (an aggregation network, a notebook): it cannot queue the next call's host
work under the GPU, so it pays the host time inside extract() in full.  Method: both forms are warmed up (plans, graphs, staging buffers), then
`--rounds` rounds ALTERNATE a window of `--iters` calls per form; every call is timed on the host (time inside extract(), GPU work still
queued, as tools/profile_extract_host.py measures it) and followed by a read of one feature element, and the window ends with a synchronise.
Reported per form: the median and min..max over the rounds of the host time per call and of images/s = B * iters / window.

    python tools/bench_preprocess.py [--configs xl,1-5] [--sources 2048x1024,native] [--rounds 5] [--iters 3] [--out profiles/device_preprocess.txt]
"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "generic-diffusion-feature_amd")):
    sys.path.insert(0, p)
import numpy as np
import torch
from PIL import Image
os.environ.setdefault("GDF_SYNTHETIC_WEIGHTS", "1")
import diffusion_feature
import bench as BB

CONFIGS = {"xl": dict(version="xl", img=1024, batch=16), "1-5": dict(version="1-5", img=512, batch=32)}

ap = argparse.ArgumentParser()
ap.add_argument("--configs", default="xl,1-5"); ap.add_argument("--sources", default="2048x1024,native")
ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--iters", type=int, default=3)
ap.add_argument("--out", default=None, help="also write the report to this file")
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_preprocess.py measures on the GPU; there is none")

lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


say("# extract(image_type='image'): PIL-to-tensor step on the host thread pool vs on the device; a caller that reads one feature after every call")
say("# median [min .. max] over %d alternating rounds of %d calls; host ms = wall time inside extract() per call" % (a.rounds, a.iters))
say("# device: %s, torch %s, Pillow %s, host threads for the host form: %s" % (
    torch.cuda.get_device_name(0), torch.__version__, Image.__version__, os.environ.get("GDF_PREPROCESS_THREADS", "min(8, cpus)")))
results = []
for name in a.configs.split(","):
    c = CONFIGS[name]
    B, S = c["batch"], c["img"]
    df = diffusion_feature.FeatureExtractor({k: True for k in BB.PRACTICAL[c["version"]]}, c["version"], device="cuda:0", img_size=S)
    prompts = df.encode_prompt("a photo of a cat")
    last = BB.PRACTICAL[c["version"]][-1]
    for source in a.sources.split(","):
        w, h = (S, S) if source == "native" else [int(v) for v in source.split("x")]
        g = np.random.default_rng(0)
        pil = [Image.fromarray(g.integers(0, 256, (h, w, 3), dtype=np.uint8)) for _ in range(B)]

        def window(on_device):
            df.device_preprocess = on_device
            host = []
            torch.cuda.synchronize(); t0 = time.perf_counter()
            with torch.no_grad():
                for _ in range(a.iters):
                    h0 = time.perf_counter()
                    f = df.extract(prompts, B, pil, t=100)
                    host.append(time.perf_counter() - h0)
                    f[last][0, 0, 0, 0].item()                # the caller reads a feature: the host waits for this call's GPU work here
                    del f
            torch.cuda.synchronize()
            return time.perf_counter() - t0, statistics.median(host)

        for _ in range(3):                                   # warm-up of both forms
            window(False); window(True)
        w_ = {"host": [], "device": []}
        for _ in range(a.rounds):
            w_["host"].append(window(False))
            w_["device"].append(window(True))
        row = {"config": name, "batch": B, "img_size": S, "source": "%dx%d" % (w, h)}
        say()
        say("## %s %dx%d, batch %d, PIL sources %d x %d" % (c["version"], S, S, B, w, h))
        for form in ("host", "device"):
            rate = sorted(B * a.iters / dt for dt, _ in w_[form])
            hms = sorted(1e3 * hm for _, hm in w_[form])
            row[form] = {"img_per_s": {"median": statistics.median(rate), "min": rate[0], "max": rate[-1]},
                         "host_ms_per_call": {"median": statistics.median(hms), "min": hms[0], "max": hms[-1]}}
            say("%-7s host time in extract() %7.1f ms [%7.1f .. %7.1f]   %7.1f img/s [%7.1f .. %7.1f]" % (
                form, row[form]["host_ms_per_call"]["median"], hms[0], hms[-1], row[form]["img_per_s"]["median"], rate[0], rate[-1]))
        row["speedup_median"] = row["device"]["img_per_s"]["median"] / row["host"]["img_per_s"]["median"]
        say("device / host: x%.3f images/s" % row["speedup_median"])
        results.append(row)
    df.device_preprocess = False
    del df
    torch.cuda.empty_cache()
say()
say(json.dumps({"device_preprocess": results}))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
