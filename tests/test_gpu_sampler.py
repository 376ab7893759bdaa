"""Guided sampling with background feature extraction (-m gpu): guided_step_kernel against float64 numpy, NativeUNet.sample against the
CPU oracle chained with the same table, captured hooks against single forwards, the hipGraph replay of the plain rows, and
`FeatureExtractor.generate` against the host-driven loop over the same `pipe.unet`."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import cfg_from_oracle_arch, oracle_run, rel_l2
from oracle import unet_ref as R
from oracle.operand_floor import fp16_operands

pytestmark = pytest.mark.gpu
vp, ci = C.c_void_p, C.c_int
GUARD = 64                       # sentinel elements in front of and behind every buffer (keeps the payload 16-byte aligned)
NH = 5                           # depth of the history ring


def _lib():
    from components import native
    return native.load_library()


def _guarded(n, dtype, sentinel):
    buf = torch.full((n + 2 * GUARD,), sentinel, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, n, sentinel):
    g = torch.cat([buf[:GUARD], buf[GUARD + n:]])
    return bool((g == sentinel).all())


def _steps_block(rows, guided, g):
    """int32 {step, ticket, n_rows, guided}, float g, three unused words, float rows[n][8] (include/gdf_ops.h) in a guarded int32 buffer"""
    n = 8 + 8 * len(rows)
    buf, pay = _guarded(n, torch.int32, 0x5A5A5A5A)
    pay[:4] = torch.tensor([0, 0, len(rows), int(guided)], dtype=torch.int32)
    pay[4:8] = torch.tensor([g, 0.0, 0.0, 0.0], dtype=torch.float32).view(torch.int32)
    pay[8:] = torch.tensor(rows, dtype=torch.float32).reshape(-1).view(torch.int32)
    return buf, pay, n


# seven rows with the history pattern of a PLMS run — 1, 2, 2, 3, 4, 4, 4 terms; row 4 reaches back five calls (w4), rows 5 and 6 wrap the
# ring — and a different c_in != 1 per row.  (timestep, c_in, c_sample, w0 .. w4)
KROWS = [(901.0, 0.50, 1.0625, -0.1210, 0.0, 0.0, 0.0, 0.0),
         (751.0, 0.75, 1.0000, -0.0605, -0.0605, 0.0, 0.0, 0.0),
         (751.0, 0.625, 1.0391, -0.1544, 0.0, 0.0515, 0.0, 0.0),
         (601.0, 0.875, 1.0273, -0.1711, 0.1190, 0.0, -0.0372, 0.0),
         (451.0, 1.25, 1.0195, -0.1835, 0.1968, -0.1234, 0.0, 0.0300),
         (301.0, 0.9375, 1.0117, -0.1432, 0.1536, -0.0963, 0.0234, 0.0),
         (151.0, 1.125, 1.0059, -0.0917, 0.0983, -0.0617, 0.0150, 0.0)]


# (B, H, W): whole 16-byte groups for the first three; 6 x 6 and 5 x 7 have planes that are no multiple of 16 bytes and take the scalar path
@pytest.mark.parametrize("guided", [True, False])
@pytest.mark.parametrize("B,H,W", [(1, 8, 8), (2, 16, 16), (3, 24, 24), (1, 6, 6), (2, 5, 7)])
def test_guided_step_kernel_against_float64(B, H, W, guided):
    L = _lib()
    s = vp(torch.cuda.current_stream().cuda_stream)
    gs = 7.5
    K = len(KROWS)
    r32 = np.asarray(KROWS, dtype=np.float32).astype(np.float64)
    PB = 2 * B if guided else B
    n, ny = B * 4 * H * W, PB * 4 * H * W
    g = torch.Generator().manual_seed(B * 1000 + H + int(guided))
    xbuf, x = _guarded(n, torch.float32, 12345.0)
    ybuf, y = _guarded(ny, torch.float16, 77.0)
    tbuf, t = _guarded(PB, torch.float32, -5.0)
    hbuf, h = _guarded(NH * n, torch.float32, -777.0)
    sbuf, st, ns = _steps_block(KROWS, guided, gs)
    x.copy_(torch.randn(n, generator=g))
    h.fill_(float("nan"))                                    # a ring slot read before it was written would poison x

    def check_guards():
        assert _guards_intact(xbuf, n, 12345.0) and _guards_intact(ybuf, ny, 77.0) and _guards_intact(tbuf, PB, -5.0)
        assert _guards_intact(hbuf, NH * n, -777.0) and _guards_intact(sbuf, ns, 0x5A5A5A5A)

    def check_y(y_ref, slack):
        yy = y.double().cpu().numpy().reshape(-1, n)
        assert np.array_equal(yy[0], yy[-1])                 # both halves of a guided input carry the same bits
        bound = 2.0 ** -11 * np.abs(y_ref) + slack + 2.0 ** -25
        assert np.all(np.abs(yy[0] - y_ref) <= bound), float(np.max(np.abs(yy[0] - y_ref) - bound))

    def launch(e, prime):
        rc = L.gdf_op_guided_step(vp(x.data_ptr()), vp(e.data_ptr()) if e is not None else None, vp(h.data_ptr()), vp(y.data_ptr()),
                                  vp(t.data_ptr()), vp(st.data_ptr()), B, H, W, prime, s)
        assert rc == 0, L.gdf_last_error()
        torch.cuda.synchronize()

    hdr = lambda k: [k, 0, K, int(guided)]
    # prime: the master and the ring are not touched, row 0 scales the input and gives the timestep
    x0 = x.clone()
    launch(None, 1)
    assert torch.equal(x, x0) and st[:4].tolist() == hdr(0) and bool(torch.isnan(h).all())
    assert t.tolist() == [901.0] * PB
    check_y(r32[0, 1] * x0.double().cpu().numpy(), 0.0)
    check_guards()

    es, ms = [], []                                          # per step: the combined eps and its magnitude, float64, (B, 4, H, W)
    for k in range(K):
        e = (torch.randn(PB, H, W, 4, generator=g) * 1.3).half().cuda()       # channels-last noise_pred, [uncond, cond]
        e0 = e.clone()
        xin = x.double().cpu().numpy().reshape(B, 4, H, W)
        launch(e, 0)
        ee = e0.double().cpu().numpy().transpose(0, 3, 1, 2)
        if guided:
            eu, ec = ee[:B], ee[B:]
            es.append(eu + gs * (ec - eu)); ms.append(np.abs(eu) + gs * (np.abs(ec) + np.abs(eu)))
        else:
            es.append(ee); ms.append(np.abs(ee))
        cs, w = r32[k, 2], r32[k, 3:8]
        ref, mag = cs * xin, np.abs(cs * xin)
        for j in range(min(NH, k + 1)):
            ref = ref + w[j] * es[k - j]
            mag = mag + np.abs(w[j]) * ms[k - j]
        got = x.double().cpu().numpy().reshape(B, 4, H, W)
        # at most 8 fp32 roundings (2 in e, 1 in c_sample x, 5 fused multiply-adds), each relative to a partial sum <= mag
        assert np.all(np.abs(got - ref) <= 2.0 ** -21 * mag), (k, float(np.max(np.abs(got - ref) / mag)))
        nxt = min(k + 1, K - 1)
        cin, tn = r32[nxt, 1], r32[nxt, 0]
        check_y((cin * ref).reshape(-1), (2.0 ** -21 * cin * mag).reshape(-1))
        assert t.tolist() == [float(tn)] * PB, (k, t.tolist())
        assert st[:4].tolist() == hdr(k + 1)
        assert torch.equal(e, e0)                                            # the noise input is read only
        ring = h.double().cpu().numpy().reshape(NH, B, 4, H, W)
        assert np.all(np.abs(ring[k % NH] - es[k]) <= 2.0 ** -23 * ms[k])    # the slot this step wrote: two roundings
        assert bool(np.isnan(ring[k + 1:]).all())                            # slots no step has reached stay unwritten
        check_guards()

    # a launch past the table writes nothing and does not advance
    xa, ya, ha = x.clone(), y.clone(), h.clone()
    launch(e, 0)
    assert torch.equal(x, xa) and torch.equal(y, ya) and torch.equal(h, ha) and st[:4].tolist() == hdr(K) and t.tolist() == [151.0] * PB
    check_guards()


# ---- NativeUNet.sample against the oracle chain -----------------------------------------------------------------------------------------
def _table(base):
    from components.models import sampling_table
    from test_sampling_table_cpu import EulerSched, PLMSSched
    rows, _ = sampling_table(EulerSched() if base == "xl" else PLMSSched(), 6)
    assert len(rows) == (6 if base == "xl" else 7)
    return rows


def _inputs(base):
    """distinct samples, distinct positive / negative conditioning ([negative, positive] where a tensor holds both halves)"""
    arch = R.tiny_arch(base)
    P = R.synth_params(arch, seed=0)
    I, N = R.synth_inputs(arch, 2, 16, seed=1), R.synth_inputs(arch, 2, 16, seed=2)
    assert not torch.equal(I["sample"][0], I["sample"][1]) and not torch.equal(I["ctx"], N["ctx"])
    cat = {"ctx": torch.cat([N["ctx"], I["ctx"]], 0)}
    for k in ("text_embeds", "time_ids"):
        if k in I and I[k] is not None:
            cat[k] = torch.cat([N[k], I[k]], 0)
    return arch, P, I, N, cat


def _oracle_chain(arch, P, x0, cat, rows, g):
    x, hist = x0.float().clone(), []
    B = x.shape[0]
    for k, (t, c_in, c_s, *w) in enumerate(rows):
        J = dict(cat, sample=torch.cat([c_in * x] * 2, 0), timestep=torch.tensor([float(t)]))
        eps = oracle_run(arch, P, J, ids=["unet-out"])["unet-out"].float()
        hist.append(eps[:B] + g * (eps[B:] - eps[:B]))
        x = float(np.float32(c_s)) * x                                          # the fp32 coefficients the device table holds
        for j in range(min(NH, k + 1)):
            if w[j] != 0.0:
                x = x + float(np.float32(w[j])) * hist[k - j]
    return x


def _native_unet(arch, P):
    from components.native import NativeUNet
    u = NativeUNet(cfg_from_oracle_arch(arch), device="cuda:0")
    u.load_state_dict({k: v.half() for k, v in P.items()})
    return u


def _sample(u, I, N, cat, rows, g, **kw):
    c = lambda k: cat[k].cuda() if k in cat and k != "ctx" else None
    x, caps = u.sample(I["sample"].float().cuda(), rows, g, I["ctx"].cuda(), N["ctx"].cuda(), c("text_embeds"), c("time_ids"), **kw)
    torch.cuda.synchronize()
    return x, caps


@pytest.mark.parametrize("base", ["1-5", "xl"])
def test_sample_matches_oracle_chain(base):
    """A guided run (g = 2: both halves weighted non-trivially) of 7 PLMS / 6 Euler rows, fp32 oracle chain vs libgdf.so, per sample against
    the same chain on fp16 operands.  Measured figures: DESIGN.md, the sampler section."""
    arch, P, I, N, cat = _inputs(base)
    rows, g = _table(base), 2.0
    ref = _oracle_chain(arch, P, I["sample"], cat, rows, g)
    with fp16_operands():
        flo = _oracle_chain(arch, P, I["sample"], cat, rows, g)
    got, caps = _sample(_native_unet(arch, P), I, N, cat, rows, g)
    assert caps == {} and got.dtype == torch.float32 and tuple(got.shape) == tuple(ref.shape)
    for b in range(2):
        e, f = rel_l2(got[b], ref[b]), rel_l2(flo[b], ref[b])
        print(f"[sample {base} lat16 K={len(rows)} g=2 sample {b}] native {e:.3e}  floor chain {f:.3e}  ratio {e / f:.2f}  bound {1.3 * f + 5e-5:.3e}")
        assert e <= 1.3 * f + 5e-5, (base, b, e, f)
    assert rel_l2(ref, I["sample"]) > 1e-2


# ---- captured hooks are the forward's own bits --------------------------------------------------------------------------------------------
WANT_IDS = ["down-level1-repeat0-vit-block0-cross-q", "up-level1-upsampler-out", "mid-vit-block0-self-map"]


def _existing(u, want):
    """the ids of `want` this architecture has; a missing one is replaced by the nearest id (in execution order) with the same last two words"""
    names = u.hook_names()
    out = []
    for w in want:
        if w not in names:
            tail = "-".join(w.split("-")[-2:])
            w = next(n for n in names if n.endswith(tail) and n not in out)
        out.append(w)
    return [n for n in names if n in out]                                       # execution order


def test_captured_hooks_are_the_forwards_own_bits():
    arch, P, I, N, cat = _inputs("1-5")
    rows, g = _table("1-5"), 2.0
    u = _native_unet(arch, P)
    ids = _existing(u, WANT_IDS)
    assert len(ids) == 3
    last = len(rows) - 1
    x_caps, caps = _sample(u, I, N, cat, rows, g, hook_ids=ids, capture_rows=[0, 2, last])
    x_plain, none = _sample(u, I, N, cat, rows, g, hook_ids=ids)                # (the same ids promised: the same operand-split level)
    assert none == {} and sorted(caps) == [0, 2, last]
    assert torch.equal(x_caps, x_plain)                                         # a capture row computes what the plain row computes
    for k in (0, 2, last):
        xk = I["sample"].float().cuda() if k == 0 else _sample(u, I, N, cat, rows[:k], g, hook_ids=ids)[0]
        inp = (xk * float(np.float32(rows[k][1]))).half()
        _, hooks = u.forward_raw(torch.cat([inp, inp], 0), torch.full((4,), rows[k][0], device="cuda"), cat["ctx"].cuda(), hook_ids=ids)
        torch.cuda.synchronize()
        assert list(caps[k].keys()) == list(hooks.keys()) == ids
        for i in ids:
            assert caps[k][i].shape[0] == 4 and caps[k][i].dtype == torch.float16
            assert torch.equal(caps[k][i], hooks[i]), (k, i)
    assert not torch.equal(caps[0][ids[0]], caps[2][ids[0]])


# ---- graph replay ---------------------------------------------------------------------------------------------------------------------------
def test_plain_rows_replay_one_graph(monkeypatch):
    monkeypatch.setenv("GDF_HIP_GRAPH", "1")
    arch, P, I, N, cat = _inputs("xl")
    rows, g = _table("xl"), 2.0
    u = _native_unet(arch, P)
    ids = _existing(u, WANT_IDS[:1])
    last = len(rows) - 1
    # captures at rows 0, 2, last: the plain plan runs rows 1 (eager warm-up), 3 (builds the graph), 4 (replays it)
    first, _ = _sample(u, I, N, cat, rows, g, hook_ids=ids, capture_rows=[0, 2, last])
    plain = next(p for k, p in u._plans.items() if k[4] == ())
    assert plain.graph
    n_plain = len(rows) - 3
    c0, l0, f0 = plain.graph_stats()
    assert c0 == 1 and l0 == n_plain - 1 and f0 == 0, (c0, l0, f0)
    second, _ = _sample(u, I, N, cat, rows, g, hook_ids=ids)                    # no captures: every row replays the same graph
    c1, l1, f1 = plain.graph_stats()
    assert (c1 - c0, l1 - l0, f1 - f0) == (0, len(rows), 0), (c1 - c0, l1 - l0, f1 - f0)
    eager, _ = _sample(u, I, N, cat, rows, g, hook_ids=ids, eager=True)
    assert plain.graph_stats() == (c1, l1, f1)
    assert torch.equal(first, second) and torch.equal(first, eager)
    assert not torch.equal(first, I["sample"].float().cuda())
    # a `plain` plan built with hooks is refused, and says so
    hooked = u._plan(4, 16, 16, 77, ["unet-out"], False, 0, early_exit=False)
    buf = torch.zeros(1 << 16, device="cuda")
    p = vp(buf.data_ptr())
    rc = u.lib.gdf_sample(hooked.handle, None, p, 1, (C.c_float * 8)(1, 1, 1, 0, 0, 0, 0, 0), 2.0, p, None, None, None, 0, None, p, p, p, None, None)
    assert rc != 0 and b"zero hooks" in u.lib.gdf_last_error()


# ---- the product call -----------------------------------------------------------------------------------------------------------------------
LAYERS = {"up-level1-repeat1-vit-block0-cross-q": True, "up-level2-repeat2-res-out": True}
IMG = 128                                                                       # a 16 x 16 latent


def _host_loop(df, prompts, x0, rows, g, order=0):
    """the loop generate replaces: pipe.unet once per row on fp16(c_in x) of fp32 latents kept by the host, the table arithmetic in torch,
    the store counting for itself.  order 1 / 2: the same formulas rounded another, equally valid way — the update (1) or the guidance
    combine (2) evaluated in float64 and rounded to fp32 once instead of after every operation — which is how far the loop's own result is
    defined"""
    pipe, B = df.pipe, x0.shape[0]
    pipe.unet.shared_ctx = False
    ctx = torch.cat([prompts[1].repeat(B, 1, 1), prompts[0].repeat(B, 1, 1)], 0).cuda()
    x, hist = x0.clone(), []
    for k, (t, c_in, c_s, *w) in enumerate(rows):
        inp = (x * float(np.float32(c_in))).half()
        eps = pipe.unet(torch.cat([inp, inp], 0), timestep=torch.tensor([t]), encoder_hidden_states=ctx, added_cond_kwargs={})[0].float()
        if order == 2:
            hist.append((eps[:B].double() + g * (eps[B:].double() - eps[:B].double())).float())
        else:
            hist.append(eps[:B] + g * (eps[B:] - eps[:B]))
        used = [j for j in range(min(NH, k + 1)) if w[j] != 0.0]
        if order == 1:
            x = (float(np.float32(c_s)) * x.double() + sum(float(np.float32(w[j])) * hist[k - j].double() for j in used)).float()
        else:
            x = float(np.float32(c_s)) * x
            for j in used:
                x = x + float(np.float32(w[j])) * hist[k - j]
    return x


def test_generate_with_background_extraction(monkeypatch):
    monkeypatch.setenv("GDF_SYNTHETIC_WEIGHTS", "1")
    import diffusion_feature
    from components.feature_extractor import layer_grid
    from components.models import sampling_table
    df = diffusion_feature.FeatureExtractor(layer=dict(LAYERS), version="1-5", img_size=IMG, device="cuda:0")
    prompts = df.encode_prompt("a photo of a cat")
    lat = torch.randn(2, 4, IMG // 8, IMG // 8, generator=torch.Generator().manual_seed(9))
    g = 2.0
    rows, sigma0 = sampling_table(df.scheduler_backup, 6)
    n_rows = len(rows)

    df.set_background_extraction([1, 3, 99])
    x = df.generate(prompts, batch_size=2, num_inference_steps=6, guidance_scale=g, latents=lat)
    got = df.get_background_extraction()
    assert x.dtype == torch.float32 and tuple(x.shape) == (2, 4, IMG // 8, IMG // 8) and torch.isfinite(x).all()
    assert list(got) == list(LAYERS)
    for i in LAYERS:
        assert sorted(got[i]) == [1, 3]
        assert df.feature_store.feats[i]["count"] == n_rows
        s = layer_grid(df.pipe.unet.cfg, i, IMG // 8)
        for f in got[i].values():
            assert f.dtype == torch.float16 and f.shape[0] == 4 and tuple(f.shape[2:]) == (s, s)
    got = {i: {k: v.clone() for k, v in d.items()} for i, d in got.items()}

    # the host-driven loop over the same pipe.unet, the store counting the calls itself
    df.feature_store.reset()
    xh = _host_loop(df, prompts, lat.cuda() * sigma0, rows, g)
    torch.cuda.synchronize()
    host = {i: dict(d) for i, d in df.get_background_extraction().items()}
    counts = {i: df.feature_store.feats[i]["count"] for i in LAYERS}
    # The loop's own error: its table arithmetic rounded two other ways (float64, one rounding).  A difference in the last bit of the
    # latents flips fp16 roundings of the next forward's input and from there of its operands, so two runs of the same chain differ like
    # two draws of the operand-rounding error — the floor of the chain bound (test_sample_matches_oracle_chain: 1.3 floor + 5e-5), taken here from the
    # reference itself, the larger of the two.
    floor = {i: 0.0 for i in LAYERS}
    floor_x = 0.0
    for order in (1, 2):
        df.feature_store.reset()
        xo = _host_loop(df, prompts, lat.cuda() * sigma0, rows, g, order=order)
        torch.cuda.synchronize()
        alt = df.get_background_extraction()
        for i in LAYERS:
            assert torch.equal(alt[i][1], host[i][1])
            floor[i] = max(floor[i], rel_l2(alt[i][3], host[i][3]))
        floor_x = max(floor_x, rel_l2(xo, xh))
    for i in LAYERS:
        assert sorted(host[i]) == [1, 3] and counts[i] == n_rows
        assert host[i][1].shape == got[i][1].shape
        assert torch.equal(got[i][1], host[i][1]), i                             # encounter 1: both paths feed the same first input
        e = rel_l2(got[i][3], host[i][3])
        print(f"[generate 1-5 encounter 3 {i}] device-resident vs host loop {e:.3e}  the loop against itself {floor[i]:.3e}  "
              f"bound {1.3 * floor[i] + 5e-5:.3e}")
        assert e <= 1.3 * floor[i] + 5e-5, (i, e, floor[i])
    e = rel_l2(x, xh)
    print(f"[generate 1-5 final latents] device-resident vs host loop {e:.3e}  the loop against itself {floor_x:.3e}  bound {1.3 * floor_x + 5e-5:.3e}")
    assert e <= 1.3 * floor_x + 5e-5, (e, floor_x)

    # store_idx None: a plain {id: tensor} of the last call
    df.set_background_extraction(None)
    df.generate(prompts, batch_size=2, num_inference_steps=6, guidance_scale=g, latents=lat)
    plain = {k: v.clone() for k, v in df.feature_store.stored_feats.items()}
    df.set_background_extraction([n_rows])
    df.generate(prompts, batch_size=2, num_inference_steps=6, guidance_scale=g, latents=lat)
    lastc = df.get_background_extraction()
    assert list(plain) == list(LAYERS)
    for i in LAYERS:
        assert torch.is_tensor(plain[i]) and torch.equal(plain[i], lastc[i][n_rows]), i

    # the unguided batch, and the decoded image
    df.set_background_extraction([2])
    x1, img = df.generate(prompts, batch_size=2, num_inference_steps=6, guidance_scale=1.0, latents=lat, output_type="pt")
    assert tuple(img.shape) == (2, 3, IMG, IMG) and torch.isfinite(img.float()).all()
    assert df.get_background_extraction()[list(LAYERS)[0]][2].shape[0] == 2
    assert not torch.equal(x1, x)


def test_generate_is_refused_where_it_does_not_apply():
    import types
    import diffusion_feature as D
    with pytest.raises(NotImplementedError, match="UNet versions"):
        D.FeatureExtractor.generate(types.SimpleNamespace(version="flux", attention=None), None, 2)
    with pytest.raises(NotImplementedError, match="attention"):
        D.FeatureExtractor.generate(types.SimpleNamespace(version="1-5", attention=["up_cross"]), None, 2)
