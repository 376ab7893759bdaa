"""CPU-side checks (no GPU): the C-ABI library loads and exports every symbol include/*.h declares, and the
host-side mirror of the reference interface (FeatureStore filtering, id scheme, config surface, error behaviour)."""
import ctypes
import json
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(gdf_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    import __graft_entry__ as G
    G.build()                                              # hipcc cross-compiles gfx950 without a GPU
    lib = ctypes.CDLL(G.LIB)
    names = _declared("gdf.h") + _declared("gdf_ops.h") + _declared("gdf_flux.h") + _declared("gdf_vae.h") + _declared("gdf_pixart.h")
    assert len(names) >= 40
    for n in names:
        assert hasattr(lib, n), n
    assert lib.gdf_abi_version() == 1


def test_binding_covers_header():
    from components import native
    assert sorted(native.SIGNATURES) == sorted(set(_declared("gdf.h") + _declared("gdf_flux.h") + _declared("gdf_vae.h") + _declared("gdf_pixart.h")))


def test_native_path_fails_loudly_without_gpu():
    from components import native
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError):
        native.NativeUNet(native.ARCH_CONFIGS["1-5"])
    # the C ABI itself also refuses (no CPU fallback inside the library)
    lib = native.load_library()
    h = ctypes.c_void_p()
    a = native.arch_desc(native.ARCH_CONFIGS["1-5"])
    assert lib.gdf_model_create(ctypes.byref(a), ctypes.byref(h)) != 0
    assert b"no HIP device" in lib.gdf_last_error()


def test_layer_ids_match_reference_dumps():
    from components.feature_extractor import unet_layer_ids
    from components.native import ARCH_CONFIGS
    for ver, fn in (("1-5", "ids_15_full.txt"), ("xl", "ids_xl_full.txt")):
        assert unet_layer_ids(ARCH_CONFIGS[ver]) == open(os.path.join(GOLD, fn)).read().split()


def test_shipped_configs_are_subsets_of_the_id_space():
    """(the product's own id generator; the oracle-side check of every reference config is
    test_every_layer_config_of_the_reference_is_served)"""
    from components.feature_extractor import unet_layer_ids
    from components.native import ARCH_CONFIGS
    cdir = os.path.join(ROOT, "generic-diffusion-feature_amd", "configs")
    for f in sorted(os.listdir(cdir)):
        if not f.endswith(".json"):
            continue
        ver = "1-5" if "_15_" in f else "xl"
        ids = set(unet_layer_ids(ARCH_CONFIGS[ver]))
        cfg = json.load(open(os.path.join(cdir, f)))
        assert cfg and all(isinstance(v, bool) for v in cfg.values())
        # `cross-k` / `cross-v` ids (config_15_analysis) are produced and dropped by the reference's FeatureStore; config_figure mixes
        # in one SD1.5-only id: unknown ids are silently ignored on both sides (feature_extractor.py:36)
        extra = sorted(k for k in set(cfg) - ids if not k.endswith(("cross-k", "cross-v")))
        assert len(extra) <= (1 if f == "config_figure.json" else 0), (f, extra[:3])


def test_feature_store_semantics():
    from components.feature_extractor import FeatureGatherer, FeatureStore
    st = FeatureStore({"a-out": True, "a-cross-k": True, "b-out": False}, 1, False)
    g = FeatureGatherer("a", st)
    tok = torch.randn(2, 16, 8).half()
    g.gather(tok, "out"); g.gather(tok, "cross-k"); FeatureGatherer("b", st).gather(tok, "out")
    assert list(st.stored_feats) == ["a-out"]                       # filtered: cross-k dropped, b-out not requested
    v = st.stored_feats["a-out"]
    assert v.shape == (2, 8, 4, 4) and torch.equal(v.permute(0, 2, 3, 1).reshape(2, 16, 8), tok)
    old = st.stored_feats
    st.reset()
    assert st.stored_feats == {} and list(old) == ["a-out"]         # previously returned dict stays valid
    st.pause(); g.gather(tok, "out"); assert st.stored_feats == {}
    st.resume()
    pooled = FeatureStore({"a-out": True}, 2, False)
    FeatureGatherer("a", pooled).gather(tok, "out")
    assert pooled.stored_feats["a-out"].shape == (2, 8, 2, 2)
    allst = FeatureStore(None, 1, False)
    assert allst.accept_all and allst.to_store == {}
    bg = FeatureStore({"a-out": True}, 1, False); bg.store_idx = [2]
    for _ in range(3):
        FeatureGatherer("a", bg).gather(tok, "out")
    assert bg.stored_feats["a-out"]["count"] == 3 and list(bg.stored_feats["a-out"]["feat"]) == [2]


def test_model_registry_error_behaviour(monkeypatch):
    from components import models
    with pytest.raises(NotImplementedError):
        models.get_diffusion_model("xl", "bfloat16")                 # reference models.py:11-16
    with pytest.raises(NotImplementedError):
        models.get_diffusion_model("no-such-version", "float16")     # reference models.py:173-174
    with pytest.raises(NotImplementedError):
        models.get_diffusion_model("hunyuan", "float16")             # out of scope, says so
    from components.native import PIXART_CONFIGS, ARCH_CONFIGS
    assert PIXART_CONFIGS["pixart-alpha"] == PIXART_CONFIGS["pixart-sigma-512"]      # same DiT at sample_size 64 (models.py:103-115)
    assert {"1-5", "2-1", "xl", "pgv2"} <= set(ARCH_CONFIGS)
    monkeypatch.delenv("GDF_SYNTHETIC_WEIGHTS", raising=False)
    with pytest.raises(RuntimeError):
        models.get_diffusion_model("1-5", "float16")                 # no diffusers, no synthetic opt-in: loud failure
    with pytest.raises(RuntimeError):
        models.get_diffusion_model("pixart-alpha", "float16")


def test_bench_dump_outputs_fixed_sample_within_limit(tmp_path):
    """bench.py --dump-outputs: float32 .npy per output, the whole tensor when it fits its share of the limit, else the same seeded
    sample of its flattened elements on every run (whatever else is dumped beside it)."""
    import zlib
    import numpy as np
    import bench
    g = torch.Generator().manual_seed(0)
    big, small = torch.randn(3, 1000, generator=g).half(), torch.randn(2, 5, generator=g)
    info = bench.dump_outputs(str(tmp_path / "a"), {"big": big, "small": small}, limit_bytes=8000)
    assert info == {"big": ((3, 1000), 1000), "small": ((2, 5), 10)}
    a, s = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "a" / "small.npy")
    assert a.dtype == s.dtype == np.float32 and a.nbytes + s.nbytes <= 8000
    assert np.array_equal(s, small.numpy())
    idx = np.sort(np.random.default_rng(zlib.crc32(b"big")).choice(3000, size=1000, replace=False))
    assert np.array_equal(a, big.float().numpy().reshape(-1)[idx])
    bench.dump_outputs(str(tmp_path / "b"), {"small": small.t(), "big": big}, limit_bytes=8000)
    assert np.array_equal(np.load(tmp_path / "b" / "big.npy"), a) and np.load(tmp_path / "b" / "small.npy").shape == (5, 2)


def test_bench_flop_model_matches_survey_totals():
    import bench
    from components.native import ARCH_CONFIGS
    xl = bench.unet_flops_per_image(ARCH_CONFIGS["xl"], 128)
    sd = bench.unet_flops_per_image(ARCH_CONFIGS["1-5"], 64)
    assert abs(sum(xl.values()) / 1e12 - 6.761) < 2e-3 and abs(sum(sd.values()) / 1e12 - 0.803) < 1e-3
    assert abs(xl["self_attn"] / 1e12 - 0.752) < 1e-3 and abs(xl["ff"] / 1e12 - 2.819) < 1e-3


def test_aggregate_attention_matches_reference_attention_store():
    """components.feature_extractor.aggregate_attention vs the reference's AttentionStore (components/attention.py:102-161)
    + the interpolate/cat of diffusion_feature.py:492-500, fed with the same random probability maps (the reference's result for
    them: tests/golden/attn_store_cat.npz, tests/golden/gen_golden_attn.py main_store_cat)."""
    import numpy as np
    from components.feature_extractor import aggregate_attention
    z = np.load(os.path.join(GOLD, "attn_store_cat.npz"))
    g = torch.Generator().manual_seed(0)
    maps = {"up_cross": [], "down_self": []}
    for place, cross, q, k in (("up", True, 16, 77), ("up", True, 64, 77), ("up", True, 16, 77), ("down", False, 64, 64)):
        probs = torch.softmax(torch.randn(2, 4, q, k, generator=g), -1)
        maps[f"{place}_{'cross' if cross else 'self'}"].append(probs)  # the reference stored probs.mean(1) (attention.py:241)
    sel = ["up_cross", "down_self"]
    assert str(z["sel"]) == repr(sel)
    ref = torch.from_numpy(z["out"])
    got = aggregate_attention({c: maps[c] for c in sel}, 16)
    assert got.shape == ref.shape == (2, 77 + 77 + 64, 16, 16)
    assert torch.allclose(got.float(), ref, atol=1e-3)


def test_attention_map_id_selection():
    from components.feature_extractor import attention_map_ids, unet_layer_ids
    from components.native import ARCH_CONFIGS
    cfg = ARCH_CONFIGS["1-5"]
    ids = attention_map_ids(cfg, unet_layer_ids(cfg), ["up_cross", "mid_self"], 64, 512 // 32, 512 // 16)
    # AttentionStore(img/32, img/16) keeps 16x16 and 32x32 grids: up-level1 (16^2) and up-level2 (32^2); mid is 8x8 -> dropped
    assert ids["mid_self"] == []
    assert ids["up_cross"] == [f"up-level{l}-repeat{r}-vit-block0-cross-map" for l in (1, 2) for r in range(3)]


def test_flux_layer_ids_match_oracle_and_reference_golden():
    """flux id scheme (reference components/feature_extractor.py:98-123): host list == oracle == order recorded from the
    reference's own run in tests/golden/flux_tiny.npz."""
    import ast
    import numpy as np
    from components.feature_extractor import flux_layer_ids
    from components.native import FLUX_CONFIGS
    from oracle import flux_ref as FR
    z = np.load(os.path.join(GOLD, "flux_tiny.npz"))
    meta = ast.literal_eval(str(z["meta"]))
    assert [i for i in flux_layer_ids(meta["arch"]) if not i.endswith("-map")] == meta["order"] == FR.hook_ids(meta["arch"])
    zm = np.load(os.path.join(GOLD, "flux_tiny_maps.npz"))          # the reference on its FluxAttnStoreProcessor
    assert flux_layer_ids(meta["arch"]) == ast.literal_eval(str(zm["meta"]))["order"] == FR.hook_ids(meta["arch"], maps=True)
    ids = flux_layer_ids(FLUX_CONFIGS["flux"])
    assert len(ids) == 19 * 9 + 38 * 7 and ids[0] == "vit-block0-q" and ids[-1] == "vit-block56-out"


def _run_output_stage(tmp_path, device):
    """extract_feature.HostWriter on the fixture's feature tensors (as channels-last strided views, the layout the native
    path hands out) -> {mode: {relative path: array}}"""
    import ast
    import types
    import numpy as np
    sys.path.insert(0, ROOT)
    import extract_feature as cli
    z = np.load(os.path.join(GOLD, "cli_output_stage.npz"))
    meta = ast.literal_eval(str(z["meta"]))
    feats = {}
    for k in meta["order"]:
        t = torch.from_numpy(z["feat:" + k]).to(device)
        feats[k] = t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)          # (B,C,H,W) view of NHWC storage
    got = {}
    for mode, kw in meta["modes"].items():
        d = tmp_path / mode
        args = types.SimpleNamespace(output_dir=str(d), aggregate_output=kw["aggregate_output"], sample_name_first=kw["sample_name_first"])
        names = meta["names"][kw["nested_input_dir"]] if kw["use_original_filename"] else [f"{kw['split']}{j}" for j in range(3)]
        w = cli.HostWriter(args)
        w.submit(feats, names)
        w.flush()
        got[mode] = {}
        for root, _, files in os.walk(d):
            for f in files:
                got[mode][os.path.relpath(os.path.join(root, f), d)] = np.load(os.path.join(root, f))
    want = {}
    for k in z.files:
        if k.startswith("file:"):
            _, mode, rel = k.split(":", 2)
            want.setdefault(mode, {})[rel] = z[k]
    return got, want


def check_output_stage(got, want):
    import numpy as np
    assert got.keys() == want.keys()
    for mode in want:
        assert sorted(got[mode]) == sorted(want[mode]), mode                   # same directory tree, same file names
        for rel, arr in want[mode].items():
            g = got[mode][rel]
            assert g.dtype == arr.dtype and g.shape == arr.shape, (mode, rel)
            assert np.array_equal(g.view(np.uint16), arr.view(np.uint16)), (mode, rel)   # byte-exact


def test_output_stage_matches_reference_files(tmp_path):
    """(f)2: `--aggregate_output` / per-layer / --sample_name_first files are byte-identical to what the reference's own
    output stage (/root/reference/extract_feature.py:112-148, executed by tests/golden/gen_golden_cli.py) wrote for the same
    feature tensors — incl. a non-integer nearest-resize ratio (6 -> 8)."""
    got, want = _run_output_stage(tmp_path, "cpu")
    check_output_stage(got, want)


def _attn_golden():
    import ast
    import numpy as np
    z = np.load(os.path.join(GOLD, "attn_aggregate.npz"))
    meta = ast.literal_eval(str(z["meta"]))
    maps = [(h, torch.from_numpy(z["map:" + h])) for h in meta["order"]]
    cases = [(ast.literal_eval(str(z["sel:" + n])), torch.from_numpy(z["out:" + n])) for n in ("a", "b")]
    return meta, maps, cases


def test_aggregated_attention_matches_reference_golden():
    """(f)3: oracle/attn_agg_ref.py AND the product's aggregate_attention / attention_map_ids-style selection against
    tests/golden/attn_aggregate.npz = the reference's own AttentionStore (gen_golden_attn.py)."""
    from components.feature_extractor import aggregate_attention
    from oracle import attn_agg_ref as AR
    meta, maps, cases = _attn_golden()
    for sel, want in cases:
        got = AR.aggregate(maps, sel, meta["min_size"], meta["max_size"], meta["out_size"])
        assert got.shape == want.shape and torch.allclose(got, want, atol=1e-6), float((got - want).abs().max())
        by_cat = {c: [m for h, m in maps if AR.category_of(h) == c and meta["min_size"] ** 2 <= m.shape[2] <= meta["max_size"] ** 2]
                  for c in sel}
        prod = aggregate_attention(by_cat, meta["out_size"])
        assert prod.dtype == torch.float16 and torch.allclose(prod.float(), want, atol=1e-3)


def test_scheduler_step_scalars_probe_and_formulas():
    """`vae-out` (reference diffusion_feature.py:478-480): scheduler.step(noise_pred, t, latents)[0] travels to libgdf as two scalars.
    A diffusers-style scheduler is probed on a deep copy (state untouched, linearity verified); the synthetic pipe's scheduler states
    its own coefficients, which are the oracle's PNDM-first-step / Euler formulas."""
    import torch
    from components.models import _Scheduler, scheduler_step_scalars
    from oracle import vae_ref as VR

    class Lin:                                   # a stateful, linear scheduler: what PNDM's first step_plms call / Euler's step are
        def __init__(self):
            self.calls = 0

        def step(self, model_output, timestep, sample, return_dict=True):
            self.calls += 1
            return (0.97 * sample - 0.125 * float(timestep) * model_output,)

    sch = Lin()
    a, b = scheduler_step_scalars(sch, torch.tensor([4.0]))
    assert abs(a - 0.97) < 1e-12 and abs(b + 0.5) < 1e-12 and sch.calls == 0

    class Clipped(Lin):
        def step(self, model_output, timestep, sample, return_dict=True):
            return ((sample - model_output).clamp(-1, 1),)
    with pytest.raises(NotImplementedError):
        scheduler_step_scalars(Clipped(), torch.tensor([4.0]))

    for euler in (False, True):
        s = _Scheduler(euler=euler)
        s.set_timesteps(1000)
        for ti in (999, 100, 1, 0):
            a, b = scheduler_step_scalars(s, torch.tensor([ti]))
            if euler:
                ac = s.alphas_cumprod
                sig = lambda i: float(((1 - ac[i]) / ac[i]) ** 0.5) if i >= 0 else 0.0
                ra, rb = VR.euler_step_scalars(sig(ti), sig(ti - 1))
            else:
                ra, rb = VR.pndm_first_step_scalars(s.alphas_cumprod, ti, ti - 1)
            assert abs(a - ra) < 1e-6 and abs(b - rb) < 1e-6, (euler, ti, a, b, ra, rb)
        x, e = torch.randn(2, 4, 8, 8), torch.randn(2, 4, 8, 8)
        assert torch.allclose(s.step(e, torch.tensor([100]), x)[0], a * 0 + scheduler_step_scalars(s, torch.tensor([100]))[0] * x
                              + scheduler_step_scalars(s, torch.tensor([100]))[1] * e)


def test_vae_decoder_oracle_structure():
    """Structural pins of the decoder restatement (the wiring is un-vendored diffusers): parameter count of the published SD VAE
    (83,653,863 = 34,163,664 encoder + quant_conv, 49,490,199 decoder + post_quant_conv) and the output geometry."""
    import torch
    from oracle import vae_ref as VR
    assert sum(math_prod(s) for s in VR.dec_param_shapes(VR.ARCH_SD_VAE).values()) == 49490199
    assert sum(math_prod(s) for s in VR.param_shapes(VR.ARCH_SD_VAE).values()) == 34163664
    a = VR.tiny_arch()
    P = VR.synth_dec_params(a)
    with torch.no_grad():
        y = VR.decode(P, a, torch.randn(2, 4, 8, 8))
    assert tuple(y.shape) == (2, 3, 32, 32) and torch.isfinite(y).all()
    # decode is what vae_out applies after the linear scheduler step
    z, e = torch.randn(1, 4, 8, 8), torch.randn(1, 4, 8, 8)
    with torch.no_grad():
        assert torch.allclose(VR.vae_out(P, a, z, e, 1.0, -0.3, 0.5), VR.decode(P, a, (z - 0.3 * e) / 0.5))


def math_prod(shape):
    n = 1
    for s in shape:
        n *= s
    return n


def test_every_layer_config_of_the_reference_is_served():
    """The layer-selection surface (north star: `feature/configs`): every config file the reference ships exists here with the same
    {id: bool} content, and every id it switches on is one the native model of its version can emit — except `cross-k` / `cross-v`,
    which the reference produces and its FeatureStore drops (feature_extractor.py:38-39): requesting them yields nothing on both sides."""
    import glob
    import json
    from oracle import unet_ref as R
    cdir = os.path.join(ROOT, "generic-diffusion-feature_amd", "configs")
    names = sorted(os.path.basename(f) for f in glob.glob(os.path.join(cdir, "*.json")))
    assert names == ["config_15_amalgamation.json", "config_15_amalgamation_small.json", "config_15_analysis.json", "config_15_full.json",
                     "config_15_legacy.json", "config_15_practical.json", "config_figure.json", "config_pg_amalgamation.json",
                     "config_xl_analysis.json", "config_xl_analysis2.json", "config_xl_full.json", "config_xl_legacy.json",
                     "config_xl_practical.json"]
    ids = {"15": set(R.stored_hook_ids(R.ARCHS["1-5"])), "xl": set(R.stored_hook_ids(R.ARCHS["xl"]))}
    for n in names:
        cfg = json.load(open(os.path.join(cdir, n)))
        assert cfg and all(isinstance(v, bool) for v in cfg.values()), n
        arch = "15" if "_15_" in n else "xl"                      # config_figure / config_pg_* are SDXL-family (Playground v2) selections
        on = [k for k, v in cfg.items() if v and not k.endswith(("cross-k", "cross-v"))]
        missing = [k for k in on if k not in ids[arch]]
        if n == "config_figure.json":
            assert len(missing) <= 1, missing                     # one id of that file exists only in the SD1.5 topology
        else:
            assert not missing, (n, missing[:5])
    # identical content, key order too: the reference's own files as fingerprinted by tests/golden/gen_reference_configs.py
    import hashlib
    ref = json.load(open(os.path.join(GOLD, "reference_configs.json")))
    assert sorted(ref) == names
    for n in names:
        cfg = json.load(open(os.path.join(cdir, n)))
        assert {"sha256": hashlib.sha256(json.dumps(cfg).encode()).hexdigest(), "ids": len(cfg)} == ref[n], n


def test_operand_plan_selection_table_and_masks():
    """Round 4: the operand plan is chosen per hook set (components/native.py choose_split) from the committed CPU-emulation table
    (components/operand_error_table.json, tools/operand_subsets.py): plain fp16 operands when every requested hook's emulated error is
    <= AUTO_BOUND (9.3e-4 since round 5), else the light level (only `gnv` split), else the architecture's selective preset, else the full split.  Every shipped layer config lands on a level whose emulated
    worst hook is within the bound; the BASELINE headline hooks stay on the plain plan."""
    import glob
    import json
    from components import native as N
    assert N.split_mask(None) == 0 and N.split_mask(False) == 0 and N.split_mask(True) == N.SPLIT_ALL == N.split_mask("precise") == 8191
    assert N.split_mask("selective") == N.SPLIT_SELECTIVE == N.split_mask("stream,gnv,attn_out,out,sampler,xqkv") == N.split_mask(395 | 4096)
    with pytest.raises(ValueError):
        N.split_mask("stream,bogus")
    tab = json.load(open(os.path.join(os.path.dirname(N.__file__), "operand_error_table.json")))
    import bench
    for ver, fam in (("xl", "xl"), ("pgv2", "xl"), ("1-5", "1-5"), ("2-1", "1-5")):
        assert N.arch_family(N.ARCH_CONFIGS[ver]) == fam
    assert N.choose_split(N.ARCH_CONFIGS["xl"], bench.PRACTICAL["xl"]) == 0               # the headline runs plain fp16 operands
    # SD1.5's practical `self-k` measures 9.70e-4 on the plain plan (3.0 % under the contract): it is handed to the LIGHT level (9.1e-4)
    assert N.choose_split(N.ARCH_CONFIGS["1-5"], bench.PRACTICAL["1-5"]) == N.SPLIT_LIGHT == N.SPLIT_CLASSES["gnv"] | N.SPLIT_CLASSES["xqkv"]
    assert N.choose_split(N.ARCH_CONFIGS["1-5"], bench.PRACTICAL["1-5"][:3]) == 0
    assert N.AUTO_BOUND <= 9.3e-4
    # the table is emulated at the BASELINE resolution; smaller latent grids average the rounding over fewer elements (measured x 1.11 from 1024^2 to
    # 448^2): the chooser scales the table by (table lat / lat)^0.13 there, so a hook near the bound climbs a level at low resolution and never drops one
    bx = N.auto_bound(N.ARCH_CONFIGS["xl"])
    assert bx == N.AUTO_BOUND_BY_FAMILY["xl"] <= 8.5e-4 and N.auto_bound(N.ARCH_CONFIGS["1-5"]) <= 9.1e-4     # per family: input variation (tools/input_variation.py)
    near = [h for h, r in tab["xl"]["hooks"].items() if 0.96 * bx <= r[0] <= bx]
    assert near and all(N.choose_split(N.ARCH_CONFIGS["xl"], [h], lat=128) == 0 for h in near)
    assert all(N.choose_split(N.ARCH_CONFIGS["xl"], [h], lat=32) != 0 for h in near)
    assert N.choose_split(N.ARCH_CONFIGS["xl"], bench.PRACTICAL["xl"], lat=256) == N.choose_split(N.ARCH_CONFIGS["xl"], bench.PRACTICAL["xl"], lat=128) == 0
    for ids in (bench.PRACTICAL["xl"], near[:3], ["unet-out"]):
        lv = [N.choose_split(N.ARCH_CONFIGS["xl"], ids, lat=l) for l in (128, 96, 64, 32, 16)]
        order = {0: 0, N.SPLIT_LIGHT: 1, N.SELECTIVE_BY_ARCH["xl"]: 2, N.SPLIT_ALL: 3}
        assert [order[x] for x in lv] == sorted(order[x] for x in lv), lv               # monotone: never a cheaper level at a smaller grid
    worst_xl = max(tab["xl"]["hooks"], key=lambda h: tab["xl"]["hooks"][h][0])
    assert worst_xl.endswith("ffn-inner") and tab["xl"]["hooks"][worst_xl][0] > 1e-3 > tab["xl"]["hooks"][worst_xl][1]
    assert N.choose_split(N.ARCH_CONFIGS["xl"], [worst_xl]) == N.SELECTIVE_BY_ARCH["xl"]
    assert N.choose_split(N.ARCH_CONFIGS["xl"], bench.PRACTICAL["xl"] + [worst_xl]) == N.SELECTIVE_BY_ARCH["xl"]
    assert N.choose_split(N.ARCH_CONFIGS["xl"], ["unet-out"]) == N.SELECTIVE_BY_ARCH["xl"]
    assert N.choose_split(N.ARCH_CONFIGS["1-5"], ["down-level0-repeat0-vit-block0-self-map"]) == N.SELECTIVE_BY_ARCH["1-5"]
    assert N.choose_split(N.ARCH_CONFIGS["xl"], []) == 0
    tiny = dict(N.ARCH_CONFIGS["xl"], block_out_channels=(64, 128, 256))                   # unknown architecture: kind rules
    assert N.arch_family(tiny) is None and N.choose_split(tiny, ["mid-vit-block0-ffn-inner"]) == N.SPLIT_SELECTIVE
    assert N.choose_split(tiny, ["unet-in", "unet-after-conv-in"]) == 0
    cfg_dir = os.path.join(os.path.dirname(os.path.dirname(N.__file__)), "configs")
    for f in sorted(glob.glob(os.path.join(cfg_dir, "*.json"))):
        ids = [k for k, v in json.load(open(f)).items() if v]
        ver = "xl" if ("_xl_" in f or "_pg_" in f) else "1-5"
        m = N.choose_split(N.ARCH_CONFIGS[ver], ids)
        assert m in (0, N.SPLIT_LIGHT, N.SELECTIVE_BY_ARCH[ver]), f                        # no shipped config needs the full split
        col = 0 if m == 0 else (2 if m == N.SPLIT_LIGHT else 1)                            # columns: plain, selective, light
        worst = max((tab[ver]["hooks"][i][col] for i in ids if i in tab[ver]["hooks"]), default=0.0)
        assert worst <= N.auto_bound(N.ARCH_CONFIGS[ver]), (f, worst)
        if any(i.endswith("-map") or i == "unet-out" for i in ids):
            assert m != 0, f


def test_bench_main_has_no_function_level_import_shadowing_module_names():
    """A function-level `import torch` anywhere inside bench.main() makes `torch` a local of the WHOLE function: every use before that
    statement raises UnboundLocalError — on the default path, which the CPU suite cannot run (round 4: the --e2e branch did exactly that)."""
    import ast
    import os
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py")).read()
    tree = ast.parse(src)
    top = set()
    for n in tree.body:
        if isinstance(n, (ast.Import, ast.ImportFrom)):
            top.update((a.asname or a.name).split(".")[0] for a in n.names)
    assert "torch" in top
    for fn in (n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef)):
        inner = set()
        for n in ast.walk(fn):
            if isinstance(n, (ast.Import, ast.ImportFrom)):
                inner.update((a.asname or a.name).split(".")[0] for a in n.names if not (isinstance(n, ast.Import) and "." in a.name and not a.asname and a.name.split(".")[0] in top and False))
        # `import torch.distributed as dist` binds only `dist`; a bare `import torch.x` would bind `torch`
        bad = {m for m in inner if m in top and m in ("torch", "os", "sys", "json", "time", "argparse")}
        assert not bad, (fn.name, bad)
