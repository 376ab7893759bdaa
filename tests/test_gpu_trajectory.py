"""Device-resident multi-step latent trajectories (-m gpu): latent_step_kernel against float64 numpy, gdf_trajectory against the
CPU oracle chained with the same coefficient table, its hipGraph replay, `FeatureExtractor.extract(use_ddim_inversion=True)`
(reference feature/diffusion_feature.py:381-386, components/ddim_inversion.py) and the kernel's bits beside another queue's GEMM."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from helpers import cfg_from_oracle_arch, oracle_run, rel_l2
from oracle import unet_ref as R
from oracle.operand_floor import fp16_operands

pytestmark = pytest.mark.gpu
vp, ci = C.c_void_p, C.c_int
GUARD = 64                       # sentinel elements in front of and behind every buffer (keeps the payload 16-byte aligned)


def _lib():
    from components import native
    L = native.load_library()
    L.gdf_op_latent_step.restype, L.gdf_op_latent_step.argtypes = ci, [vp, vp, vp, vp, vp, ci, ci, ci, ci, vp]
    return L


def _guarded(n, dtype, sentinel):
    """(whole buffer, payload view of n elements) with GUARD sentinel elements on both sides"""
    buf = torch.full((n + 2 * GUARD,), sentinel, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, n, sentinel):
    g = torch.cat([buf[:GUARD], buf[GUARD + n:]])
    return bool((g == sentinel).all())


def _steps_block(rows):
    """int32 {step, ticket, n_rows, 0} + float rows (include/gdf_ops.h) inside a guarded int32 buffer"""
    n = 4 + 4 * len(rows)
    buf, pay = _guarded(n, torch.int32, 0x5A5A5A5A)
    pay[:4] = torch.tensor([0, 0, len(rows), 0], dtype=torch.int32)
    pay[4:] = torch.tensor(rows, dtype=torch.float32).reshape(-1).view(torch.int32)
    return buf, pay, n


# (B, H, W): the first three are the UNet-like shapes (whole 16-byte groups; 3 x 24 x 24 x 4 = 6912 elements = 864 groups of 8, not a
# multiple of any power-of-two span >= 512); 6 x 6 and 5 x 7 have planes that are no multiple of 16 bytes and take the scalar path
@pytest.mark.parametrize("B,H,W", [(1, 8, 8), (2, 16, 16), (3, 24, 24), (1, 6, 6), (2, 5, 7)])
def test_latent_step_kernel_against_float64(B, H, W):
    L = _lib()
    s = vp(torch.cuda.current_stream().cuda_stream)
    rows = [(11.0, 0.5, 0.9921875, 0.046875), (21.0, 0.75, 1.0117, -0.0313), (31.0, 1.0, 0.9873, 0.0721)]      # one c_in != 1 per use
    r32 = np.asarray(rows, dtype=np.float32).astype(np.float64)
    n = B * 4 * H * W
    g = torch.Generator().manual_seed(B * 1000 + H)
    xbuf, x = _guarded(n, torch.float32, 12345.0)
    ybuf, y = _guarded(n, torch.float16, 77.0)
    tbuf, t = _guarded(B, torch.float32, -5.0)
    sbuf, st, ns = _steps_block(rows)
    x.copy_(torch.randn(n, generator=g))

    def check_guards():
        assert _guards_intact(xbuf, n, 12345.0) and _guards_intact(ybuf, n, 77.0) and _guards_intact(tbuf, B, -5.0)
        assert _guards_intact(sbuf, ns, 0x5A5A5A5A)

    def check_y(y_ref, slack):
        yy = y.double().cpu().numpy()
        bound = 2.0 ** -11 * np.abs(y_ref) + slack + 2.0 ** -25
        assert np.all(np.abs(yy - y_ref) <= bound), float(np.max(np.abs(yy - y_ref) - bound))

    # prime: the launch in front of the first forward — the master is not touched, row 0 scales the input and gives the timestep
    x0 = x.clone()
    assert L.gdf_op_latent_step(vp(x.data_ptr()), None, vp(y.data_ptr()), vp(t.data_ptr()), vp(st.data_ptr()), B, H, W, 1, s) == 0, L.gdf_last_error()
    torch.cuda.synchronize()
    assert torch.equal(x, x0) and st[:4].tolist() == [0, 0, 3, 0]
    assert t.tolist() == [11.0] * B
    check_y(r32[0, 1] * x0.double().cpu().numpy(), 0.0)
    check_guards()

    for k in range(3):
        e = (torch.randn(B, H, W, 4, generator=g) * 1.3).half().cuda()       # channels-last noise_pred
        e0 = e.clone()
        xin = x.double().cpu().numpy().reshape(B, 4, H, W)
        assert L.gdf_op_latent_step(vp(x.data_ptr()), vp(e.data_ptr()), vp(y.data_ptr()), vp(t.data_ptr()), vp(st.data_ptr()), B, H, W, 0, s) == 0, \
            L.gdf_last_error()
        torch.cuda.synchronize()
        ee = e0.double().cpu().numpy().transpose(0, 3, 1, 2)
        cs, ce = r32[k, 2], r32[k, 3]
        nxt = min(k + 1, 2)
        cin, tn = r32[nxt, 1], r32[nxt, 0]
        ref = cs * xin + ce * ee
        mag = np.abs(cs * xin) + np.abs(ce * ee)
        got = x.double().cpu().numpy().reshape(B, 4, H, W)
        assert np.all(np.abs(got - ref) <= 2.0 ** -22 * mag), (k, float(np.max(np.abs(got - ref) / mag)))
        check_y((cin * ref).reshape(-1), (2.0 ** -22 * cin * mag).reshape(-1))
        assert t.tolist() == [float(tn)] * B, (k, t.tolist())
        assert st[:4].tolist() == [k + 1, 0, 3, 0]
        assert torch.equal(e, e0)                                            # the noise input is read only
        check_guards()

    # a step past the table writes nothing and does not advance
    xa, ya = x.clone(), y.clone()
    assert L.gdf_op_latent_step(vp(x.data_ptr()), vp(e.data_ptr()), vp(y.data_ptr()), vp(t.data_ptr()), vp(st.data_ptr()), B, H, W, 0, s) == 0
    torch.cuda.synchronize()
    assert torch.equal(x, xa) and torch.equal(y, ya) and st[:4].tolist() == [3, 0, 3, 0] and t.tolist() == [31.0] * B
    check_guards()


# ---- gdf_trajectory against the oracle chain ---------------------------------------------------------------------------------------
def _real_table(k=5):
    """the first k rows of the inversion table of an SD scheduler config (leading, offset 1, 100 steps): timesteps 11 .. 51"""
    from components.models import ddim_inversion_table
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float64) ** 2
    sch = types.SimpleNamespace(alphas_cumprod=torch.cumprod(1.0 - betas, 0),
                                config=types.SimpleNamespace(num_train_timesteps=1000, steps_offset=1, timestep_spacing="leading"))
    rows = ddim_inversion_table(sch, 100, 50)
    assert len(rows) == k
    return rows


def _oracle_chain(arch, P, I, rows):
    x = I["sample"].float().clone()
    for t, c_in, c_s, c_e in rows:
        J = dict(I, sample=(c_in * x), timestep=torch.tensor([float(t)]))
        eps = oracle_run(arch, P, J, ids=["unet-out"])["unet-out"].float()
        x = float(np.float32(c_s)) * x + float(np.float32(c_e)) * eps          # the fp32 coefficients the device table holds
    return x


def _native_unet(arch, P):
    from components.native import NativeUNet
    u = NativeUNet(cfg_from_oracle_arch(arch), device="cuda:0")
    u.load_state_dict({k: v.half() for k, v in P.items()})
    return u


def _run_trajectory(u, I, rows, **kw):
    g = lambda k: I[k].cuda() if k in I else None
    out = u.trajectory(I["sample"].float().cuda(), rows, g("ctx"), g("text_embeds"), g("time_ids"), **kw)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("base", ["1-5", "2-1", "xl"])
def test_trajectory_matches_oracle_chain(base):
    """Five inversion steps, fp32 oracle chain vs libgdf.so.  Measured (MI355X; native / fp16-operand floor chain, worse sample): see DESIGN.md
    "DDIM inversion"."""
    arch = R.tiny_arch(base)
    P = R.synth_params(arch, seed=0)
    I = R.synth_inputs(arch, 2, 16, seed=1)
    assert not torch.equal(I["sample"][0], I["sample"][1])
    rows = _real_table()
    ref = _oracle_chain(arch, P, I, rows)
    with fp16_operands():
        flo = _oracle_chain(arch, P, I, rows)
    got = _run_trajectory(_native_unet(arch, P), I, rows)
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(ref.shape)
    for b in range(2):
        e, f = rel_l2(got[b], ref[b]), rel_l2(flo[b], ref[b])
        print(f"[trajectory {base} lat16 K=5 sample {b}] native {e:.3e}  floor chain {f:.3e}  bound {1.3 * f + 5e-5:.3e}")
        assert e <= 1.3 * f + 5e-5, (base, b, e, f)
    # and the chain moved the latents by far more than that
    assert rel_l2(ref, I["sample"]) > 1e-2


def test_trajectory_replays_one_graph(monkeypatch):
    monkeypatch.setenv("GDF_HIP_GRAPH", "1")
    arch = R.tiny_arch("xl")
    P = R.synth_params(arch, seed=0)
    I = R.synth_inputs(arch, 2, 16, seed=1)
    rows = _real_table()
    u = _native_unet(arch, P)
    first = _run_trajectory(u, I, rows)                    # step 0 eager (warm-up), step 1 builds the graph, steps 2-4 replay it
    plan = next(p for k, p in u._plans.items() if k[4] == ())
    assert plan.graph
    assert u.lib.gdf_plan_num_ops(plan.handle) > 0
    c0, l0, f0 = plan.graph_stats()
    assert c0 == 1 and l0 == 4 and f0 == 0, (c0, l0, f0)
    second = _run_trajectory(u, I, rows)
    c1, l1, f1 = plan.graph_stats()
    assert (c1 - c0, l1 - l0, f1 - f0) == (0, 5, 0), (c1 - c0, l1 - l0, f1 - f0)
    eager = _run_trajectory(u, I, rows, eager=True)
    assert plan.graph_stats() == (c1, l1, f1)
    assert torch.equal(first, second) and torch.equal(first, eager)
    assert not torch.equal(first, I["sample"].float().cuda())
    # a plan built with hooks cannot run a trajectory, and says so
    hooked = u._plan(2, 16, 16, 77, ["unet-out"], False, 0, early_exit=False)
    buf = torch.zeros(1 << 16, device="cuda")
    rc = u.lib.gdf_trajectory(hooked.handle, vp(buf.data_ptr()), 1, (C.c_float * 4)(1, 1, 1, 0), vp(buf.data_ptr()), None, None,
                              vp(buf.data_ptr()), vp(buf.data_ptr()), None)
    assert rc != 0 and b"zero hooks" in u.lib.gdf_last_error()


# ---- the product path -------------------------------------------------------------------------------------------------------------------
LAYERS = {"up-level1-repeat1-vit-block0-cross-q": True, "up-level2-repeat2-res-out": True}


def test_extract_with_ddim_inversion(monkeypatch):
    monkeypatch.setenv("GDF_SYNTHETIC_WEIGHTS", "1")
    import diffusion_feature
    from components.models import ddim_inversion_table
    df = diffusion_feature.FeatureExtractor(layer=dict(LAYERS), version="1-5", img_size=128, device="cuda:0")
    prompt = df.encode_prompt("a photo of a cat")
    img = torch.rand(2, 3, 128, 128, generator=torch.Generator().manual_seed(5)) * 2 - 1
    keep = lambda f: {k: v.clone() for k, v in f.items()}

    torch.manual_seed(0)
    plain = keep(df.extract(prompt, batch_size=2, image=img, image_type="tensors", t=50))
    torch.manual_seed(0)
    inv = keep(df.extract(prompt, batch_size=2, image=img, image_type="tensors", t=50, use_ddim_inversion=True))
    assert list(inv.keys()) == list(plain.keys()) == list(LAYERS)
    for k in LAYERS:
        assert inv[k].shape == plain[k].shape and inv[k].dtype == torch.float16
        assert torch.isfinite(inv[k].float()).all()
        assert not torch.equal(inv[k], plain[k]), k

    # the same by hand: VAE encode without noise -> trajectory -> extract on the latents
    pipe = df.pipe
    torch.manual_seed(0)
    eps = torch.randn((2, 4, 16, 16), device="cuda:0", dtype=torch.float32)
    lat = pipe.native_vae.encode(img.cuda(), eps=eps, noise=None, noise_a=1.0, noise_b=0.0, scaling_factor=0.18215)
    sch = pipe.scheduler
    sch.set_timesteps(1000, device="cpu")
    t_sched = pipe.get_timesteps(1000, 50 / 1000, "cpu")[0][:1]
    table = ddim_inversion_table(sch, 100, t_sched)
    assert [r[0] for r in table] == [10, 20, 30, 40, 50]
    ctx = prompt[0].repeat(2, 1, 1).cuda()
    x = pipe.unet.trajectory(lat.float(), table, ctx, shared_ctx=True)
    assert x.dtype == torch.float32 and not torch.equal(x, lat.float())
    hand = keep(df.extract(prompt, batch_size=2, image=x, image_type="latents", t=50))
    for k in LAYERS:
        assert torch.equal(hand[k], inv[k]), k


def test_extract_with_ddim_inversion_xl(monkeypatch):
    monkeypatch.setenv("GDF_SYNTHETIC_WEIGHTS", "1")
    import diffusion_feature
    layer = {"up-level1-repeat1-vit-block0-out": True, "up-level2-repeat2-res-out": True}
    df = diffusion_feature.FeatureExtractor(layer=layer, version="xl", img_size=128, device="cuda:0")
    prompt = df.encode_prompt("a photo of a cat")
    img = torch.rand(2, 3, 128, 128, generator=torch.Generator().manual_seed(6)) * 2 - 1
    torch.manual_seed(0)
    f = df.extract(prompt, batch_size=2, image=img, image_type="tensors", t=50, use_ddim_inversion=True)
    assert list(f.keys()) == list(layer)
    assert tuple(f["up-level1-repeat1-vit-block0-out"].shape) == (2, 640, 8, 8)
    assert tuple(f["up-level2-repeat2-res-out"].shape) == (2, 320, 16, 16)
    for v in f.values():
        assert v.dtype == torch.float16 and torch.isfinite(v.float()).all()


def test_extract_with_ddim_inversion_refused_for_pixart(monkeypatch):
    monkeypatch.setenv("GDF_SYNTHETIC_WEIGHTS", "1")
    import diffusion_feature
    from components.models import SyntheticPixartPipe
    from oracle import pixart_ref as PR
    pipe = SyntheticPixartPipe("pixart-sigma", "cuda:0", seed=0, cfg=PR.tiny_arch(heads=8, num_layers=2, sample_size=16), n_txt=20)
    df = diffusion_feature.FeatureExtractor(layer={"vit-block1-out": True}, version="pixart-sigma", img_size=128, device="cuda:0", external_model=pipe)
    with pytest.raises(NotImplementedError, match="use_ddim_inversion"):
        df.extract(df.encode_prompt("a photo of a cat"), batch_size=1, image=torch.zeros(1, 3, 128, 128), image_type="tensors", t=50,
                   use_ddim_inversion=True)


def test_cli_flag_writes_the_same_layout(tmp_path, monkeypatch):
    """`extract_feature.py --use_ddim_inversion`: the same files as without the flag (names, shapes, dtype), different values."""
    import json
    import os
    import sys
    from PIL import Image
    monkeypatch.setenv("GDF_SYNTHETIC_WEIGHTS", "1")
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import extract_feature as cli
    rs = np.random.RandomState(0)
    (tmp_path / "imgs").mkdir()
    for n in ("a", "b", "c"):
        Image.fromarray((rs.rand(100, 120, 3) * 255).astype(np.uint8)).save(tmp_path / "imgs" / f"{n}.png")
    (tmp_path / "prompt.txt").write_text("a photo of a cat")
    (tmp_path / "layers.json").write_text(json.dumps(LAYERS))
    base = ["--layer", str(tmp_path / "layers.json"), "--version", "1-5", "--img_size", "128", "--t", "50", "-b", "2", "--seed", "0",
            "--input_dir", str(tmp_path / "imgs" / "*.png"), "--prompt_file", str(tmp_path / "prompt.txt"), "--use_original_filename"]
    cli.main(base + ["--output_dir", str(tmp_path / "plain")])
    cli.main(base + ["--output_dir", str(tmp_path / "inv"), "--use_ddim_inversion"])
    files = lambda d: sorted(os.path.relpath(os.path.join(r, f), tmp_path / d) for r, _, fs in os.walk(tmp_path / d) for f in fs)
    assert files("plain") == files("inv") and len(files("inv")) == 6
    for f in files("inv"):
        a, b = np.load(tmp_path / "plain" / f), np.load(tmp_path / "inv" / f)
        assert a.shape == b.shape and b.dtype == np.float16 and np.isfinite(b.astype(np.float32)).all()
        assert not np.array_equal(a, b), f


# ---- the update kernel beside another queue's GEMM ---------------------------------------------------------------------------------------
def test_latent_step_beside_matmul_on_a_second_stream_keeps_its_bits():
    """fp32 FMA chains in PACKED form gave wrong low halves beside another queue's GEMM on this device; latent_step_kernel is
    built without them.  200 consecutive steps of one trajectory (in place: an error in any step reaches every later one) on one stream, alone
    and while torch.matmul keeps a second stream busy; every step's latents and fp16 output must have the same bits.  One run, no retry."""
    L = _lib()
    B, H, W, K = 2, 64, 64, 200
    n = B * 4 * H * W
    g = torch.Generator().manual_seed(11)
    rows = [(float(k), 1.0 if k % 3 else 0.75, 1.01 if k % 2 else 0.99, 0.05 * (-1) ** k * (1 + k % 7)) for k in range(K)]
    x0 = torch.randn(n, generator=g).cuda()
    e = torch.randn(B, H, W, 4, generator=g).half().cuda()
    x, y, t = torch.empty_like(x0), torch.empty(n, dtype=torch.half, device="cuda"), torch.empty(B, device="cuda")
    _, st, _ = _steps_block(rows)
    hdr = st[:4].clone()
    s0, s1 = torch.cuda.Stream(), torch.cuda.Stream()
    a = torch.randn(4096, 4096, generator=g).half().cuda()
    b = torch.randn(4096, 4096, generator=g).half().cuda()
    c = torch.empty_like(a)
    torch.matmul(a, b, out=c)                                                # (library initialisation outside the measured part)
    torch.cuda.synchronize()

    def run():
        xs, ys = [], []
        with torch.cuda.stream(s0):
            x.copy_(x0); st[:4] = hdr
            for _ in range(K):
                rc = L.gdf_op_latent_step(vp(x.data_ptr()), vp(e.data_ptr()), vp(y.data_ptr()), vp(t.data_ptr()), vp(st.data_ptr()), B, H, W, 0,
                                          vp(s0.cuda_stream))
                assert rc == 0, L.gdf_last_error()
                xs.append(x.clone()); ys.append(y.clone())
                s0.synchronize()                                             # step by step, so that every launch meets the other stream's work
        return xs, ys

    solo_x, solo_y = run()
    torch.cuda.synchronize()
    assert st[:4].tolist() == [K, 0, K, 0]
    import threading
    stop, done, errs = threading.Event(), [0], []

    def matmuls():                                                           # a second host thread keeps the second stream busy until the steps are done
        try:
            torch.cuda.set_device(0)
            with torch.cuda.stream(s1):
                while not stop.is_set():
                    torch.matmul(a, b, out=c); s1.synchronize(); done[0] += 1
        except Exception as ex:
            errs.append(ex)
    th = threading.Thread(target=matmuls)
    th.start()
    try:
        while done[0] < 2 and not errs and th.is_alive():                    # (the partner is up and running)
            s1.synchronize()
        before = done[0]
        beside_x, beside_y = run()
    finally:
        stop.set(); th.join()
    torch.cuda.synchronize()
    assert not errs, errs
    assert done[0] - before >= 2, "no matmul ran while the 200 steps did"
    bad = [k for k in range(K) if not (torch.equal(solo_x[k], beside_x[k]) and torch.equal(solo_y[k], beside_y[k]))]
    assert not bad, bad[:10]
    assert not torch.equal(solo_x[0], solo_x[-1])
