"""ControlNet residuals on the GPU (-m gpu): residual_add_kernel through the C ABI (include/gdf_ops.h gdf_op_residual_add) against float64,
and NativeUNet with residuals (gdf_forward_res, include/gdf.h) against the CPU oracle (tests/controlnet_oracle.py) and the golden vectors of
the reference's own forward (tests/golden/unet_tiny_residuals_*.npz)."""
import ctypes as C
import functools
import types

import pytest
import torch

import controlnet_oracle as CO
from helpers import cfg_from_oracle_arch, rel_l2
from oracle import unet_ref as R
from oracle.operand_floor import fp16_operands
from test_controlnet_cpu import residual_golden

pytestmark = pytest.mark.gpu
vp, ci = C.c_void_p, C.c_int
GUARD = 64                       # sentinel elements in front of and behind every buffer (keeps the payload 16-byte aligned)
TOL, TOL_SPLIT = 2e-3, 6e-4      # tests/test_gpu_unet.py: shrunken widths (with 1.3 x the fp16-operand floor + 5e-5), split plans
TOL_PAIR = 3e-6                  # tests/test_gpu_gemm.py: a (hi, lo) pair per 16 x 16 block


class Item(C.Structure):
    """gdf_residual_add_item of include/gdf_ops.h (same field order)"""
    _fields_ = [("dst", vp), ("ld", ci), ("lo", ci), ("res", vp), ("rows", ci), ("C", ci)]


def _lib():
    from components import native
    L = native.load_library()
    L.gdf_op_residual_add.restype, L.gdf_op_residual_add.argtypes = ci, [C.POINTER(Item), ci, vp]
    return L


def _guarded(vals, sentinel):
    """(whole buffer, payload view) of a flat fp16 device copy of `vals` with GUARD sentinel elements on both sides"""
    n = vals.numel()
    buf = torch.full((n + 2 * GUARD,), sentinel, dtype=torch.float16, device="cuda")
    buf[GUARD:GUARD + n] = vals.reshape(-1).to("cuda", torch.float16)
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, sentinel):
    return bool((torch.cat([buf[:GUARD], buf[-GUARD:]]) == sentinel).all())


# ---- test 1: the kernel -------------------------------------------------------------------------------------------------------------------
CH = 72                                                   # h-slice columns in front of the skip slice (sentinels): ld > C, offset slice
SHAPES = [(c, b * h * w) for c in (64, 320) for (b, h, w) in ((1, 8, 8), (2, 5, 7), (3, 16, 16))]
SENT = 777.0


def _case(pair, seed):
    """host tensors of one launch over all SHAPES: per tensor the concat rows [h | skip] (pair: [h_hi | skip_hi | h_lo | skip_lo]) with
    sentinels in the h columns, the residual, and the float64 reference of the skip slice"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for c, rows in SHAPES:
        v = torch.randn(rows, c, generator=g)
        res = (0.5 * torch.randn(rows, c, generator=g)).half()
        hi = v.half()
        lo = (v - hi.float()).half()
        w = CH + c
        row = torch.full((rows, 2 * w if pair else w), SENT, dtype=torch.float16)
        row[:, CH:w] = hi
        if pair:
            row[:, w + CH:] = lo
        ref = hi.double() + res.double() + (lo.double() if pair else 0)
        out.append((row, res, ref))
    return out


def _launch(L, case, pair):
    bufs, items = [], (Item * len(case))()
    for k, ((row, res, _), (c, rows)) in enumerate(zip(case, SHAPES)):
        db, d = _guarded(row, -3.0)
        rb, r = _guarded(res, -5.0)
        bufs.append((db, d.view(rows, -1), rb, r.view(rows, c)))
        items[k] = Item(d.data_ptr() + CH * 2, row.shape[1], (CH + c) if pair else 0, r.data_ptr(), rows, c)
    assert L.gdf_op_residual_add(items, len(case), None) == 0, L.gdf_last_error()
    torch.cuda.synchronize()
    return bufs


@pytest.mark.parametrize("pair", [False, True], ids=["plain", "pair"])
def test_residual_add_kernel(pair):
    """One launch over six tensors (C in {64, 320} x rows in {64, 70, 768}), each a slice of a wider row.  Plain fp16 images:
    |got - ref| <= 2^-11 |ref| + 2^-24 (one fp16 rounding plus the subnormal spacing); (hi, lo) pairs: relative L2 <= 3e-6 per 16 x 16 block.
    Sentinel columns of the h slice, guards around every buffer and the residual itself are untouched; a second launch gives the same bits."""
    L = _lib()
    case = _case(pair, seed=11 + pair)
    bufs = _launch(L, case, pair)
    again = _launch(L, case, pair)
    for (row, res, ref), (c, rows), (db, d, rb, r), (_, d2, _, _) in zip(case, SHAPES, bufs, again):
        w = CH + c
        assert _guards_intact(db, -3.0) and _guards_intact(rb, -5.0), (c, rows)
        assert torch.equal(r.cpu(), res), (c, rows)                                      # the residual is read only
        assert bool((d[:, :CH] == SENT).all()), (c, rows)                                # neighbouring h columns survive
        assert torch.equal(d, d2), (c, rows)
        got = d[:, CH:w].cpu().double()
        if not pair:
            err = (got - ref).abs()
            bound = 2.0 ** -11 * ref.abs() + 2.0 ** -24
            assert bool((err <= bound).all()), (c, rows, float((err - bound).max()))
        else:
            assert bool((d[:, w:w + CH] == SENT).all()), (c, rows)
            got = got + d[:, w + CH:].cpu().double()
            pr, pc = -rows % 16, -c % 16
            e = torch.nn.functional.pad(got - ref, (0, pc, 0, pr)).reshape((rows + pr) // 16, 16, (c + pc) // 16, 16)
            f = torch.nn.functional.pad(ref, (0, pc, 0, pr)).reshape((rows + pr) // 16, 16, (c + pc) // 16, 16)
            rel = e.pow(2).sum((1, 3)).sqrt() / f.pow(2).sum((1, 3)).sqrt()
            print(f"pair C={c} rows={rows}: worst 16x16 block {float(rel.max()):.2e}")
            assert float(rel.max()) <= TOL_PAIR, (c, rows, float(rel.max()))
            # the pair is a split: hi alone is the value to one fp16 rounding
            assert bool(((d[:, CH:w].cpu().double() - ref).abs() <= 2.0 ** -11 * ref.abs() + 2.0 ** -24).all()), (c, rows)


def test_residual_add_rejects_bad_arguments():
    """misaligned pointers, widths that are no multiple of 8, a pair whose halves overlap, more than 16 tensors: an error, nothing launched"""
    L = _lib()
    db, d = _guarded(torch.zeros(8, 64), -3.0)
    rb, r = _guarded(torch.ones(8, 32), -5.0)
    ok = dict(dst=d.data_ptr(), ld=64, lo=0, res=r.data_ptr(), rows=8, C=32)
    for bad in (dict(dst=d.data_ptr() + 2), dict(res=r.data_ptr() + 8), dict(C=28), dict(ld=60), dict(lo=16), dict(lo=36), dict(ld=24), dict(rows=-1)):
        it = (Item * 1)(Item(**dict(ok, **bad)))
        assert L.gdf_op_residual_add(it, 1, None) != 0, bad
    assert L.gdf_op_residual_add((Item * 17)(*[Item(**ok)] * 17), 17, None) != 0
    torch.cuda.synchronize()
    assert bool((d == 0).all()) and _guards_intact(db, -3.0) and _guards_intact(rb, -5.0)
    assert L.gdf_op_residual_add((Item * 1)(Item(**ok)), 1, None) == 0
    torch.cuda.synchronize()
    assert bool((d.view(8, 64)[:, :32] == 1).all()) and bool((d.view(8, 64)[:, 32:] == 0).all())


# ---- test 4: NativeUNet with residuals ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference(tag):
    """the golden's architecture, weights, inputs and residuals; the oracle's hooks (accept-all, maps included) with and without the fp16-operand
    rounding — computed once per architecture and shared, never modified"""
    meta, I, down, mid, gold, _ = residual_golden(tag)
    arch = meta["arch"]
    P = R.synth_params(arch, seed=meta["wseed"])

    def run():
        st = R.Store(None)
        with torch.no_grad():
            CO.unet_forward_res(P, arch, I["sample"], I["timestep"], I["ctx"], I.get("text_embeds"), I.get("time_ids"), down, mid, store=st)
        return st.feats
    ref = run()
    with fp16_operands():
        flo = run()
    return arch, P, I, down, mid, gold, ref, flo


def _native(arch, P, **kw):
    from components.native import NativeUNet
    u = NativeUNet(cfg_from_oracle_arch(arch), device="cuda:0", **kw)
    u.load_state_dict({k: v.half() for k, v in P.items()})
    return u


def _run(u, I, ids, residuals=None):
    g = lambda k: I[k].cuda() if k in I else None
    noise, hooks = u.forward_raw(g("sample"), g("timestep"), g("ctx"), g("text_embeds"), g("time_ids"), hook_ids=ids, residuals=residuals)
    torch.cuda.synchronize()
    return noise, hooks


def _block(u, down, mid):
    return u.pack_residuals([t.cuda() for t in down], mid.cuda())


def _untouched(k):
    return k.startswith(("down-", "mid-")) or k in ("unet-in", "unet-after-conv-in")


@pytest.mark.parametrize("tag", ["xl", "15"])
def test_unet_with_residuals_matches_oracle_and_golden(tag):
    arch, P, I, down, mid, gold, ref, flo = _reference(tag)
    u = _native(arch, P, precise=False)
    ids = list(ref.keys())
    block = _block(u, down, mid)
    # the plan reports the layout the architecture-level function computes
    from components import native as N
    plan = u._plan(I["sample"].shape[0], 16, 16, I["ctx"].shape[1], ids, False, 0, residuals=True)
    lay, nbytes = u.residual_layout(I["sample"].shape[0], 16, 16)
    assert u.lib.gdf_plan_residual_count(plan.handle) == len(lay) == len(down) + 1 and u.lib.gdf_plan_residual_bytes(plan.handle) == nbytes
    for i, (off, shape) in enumerate(lay):
        o, s = C.c_size_t(), (C.c_int64 * 4)()
        assert u.lib.gdf_plan_residual_info(plan.handle, i, C.byref(o), C.byref(s)) == 0 and (o.value, tuple(s)) == (off, shape)
    assert u.lib.gdf_plan_residual_count(u._plan(I["sample"].shape[0], 16, 16, I["ctx"].shape[1], ids, False, 0).handle) == 0
    assert N.residual_layout(u.cfg, I["sample"].shape[0], 16, 16) == (lay, nbytes)

    noise, hooks = _run(u, I, ids, block)
    assert list(hooks.keys()) == ids
    errs = {k: rel_l2(hooks[k], ref[k]) for k in ids}
    worst = max(errs, key=errs.get)
    print(f"[{tag} residuals] hooks={len(ids)} worst {worst} = {errs[worst]:.2e}; median {sorted(errs.values())[len(errs) // 2]:.2e}")
    bad = {k: v for k, v in errs.items() if not v < TOL}
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1])[:8]
    assert rel_l2(noise, ref["unet-out"]) < TOL
    over = {k: (errs[k], rel_l2(flo[k], ref[k])) for k in ids if not errs[k] <= 1.3 * rel_l2(flo[k], ref[k]) + 5e-5}
    assert not over, sorted(over.items(), key=lambda kv: -kv[1][0])[:8]
    # the reference's own forward: the sampled positions of every hook it stored (fp32 values: the floor, the fp16-operand oracle's fp16
    # hooks, is taken against the same values, so both sides carry the rounding of the hook's own fp16 storage)
    gerr = {}
    for k, (idx, vals, _, shape) in gold.items():
        assert tuple(hooks[k].shape) == shape, k
        s = lambda t: t.float().cpu().contiguous().flatten()[idx]
        gerr[k] = (rel_l2(s(hooks[k]), vals), rel_l2(s(flo[k]), vals))
    worst = max(gerr, key=lambda k: gerr[k][0])
    print(f"[{tag} residuals, golden] hooks={len(gerr)} worst {worst} = {gerr[worst][0]:.2e}")
    bad = {k: v for k, v in gerr.items() if not (v[0] < TOL and v[0] <= 1.3 * v[1] + 5e-5)}
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1][0])[:8]

    # the down path, the mid block and their hooks are those of the plain forward, bit for bit; the up path is not
    noise0, plain = _run(u, I, ids)
    for k in ids:
        assert torch.equal(plain[k], hooks[k]) == _untouched(k), k
    assert not torch.equal(noise0, noise)
    # deterministic, and replayed from the plan's graph (keyed on the buffer addresses, the staged residual block among them): the second
    # call builds the graph of its hook-buffer set, the third — on the same set, handed back by dropping h2 — builds nothing new
    n2, h2 = _run(u, I, ids, block)
    for k in ids:
        assert torch.equal(h2[k], hooks[k]), k
    del n2, h2                                            # (every view of the set, the noise prediction among them)
    cap = plan.graph_stats()
    n3, h3 = _run(u, I, ids, block)
    assert cap[0] >= 1 and plan.graph_stats() == (cap[0], cap[1] + 1, 0), (cap, plan.graph_stats())
    for k in ids:
        assert torch.equal(h3[k], hooks[k]), k
    assert torch.equal(n3, noise)


@pytest.mark.parametrize("tag", ["xl", "15"])
def test_unet_with_residuals_split_plan(tag):
    """precise=True: split STREAM images, the add is hi + lo + residual in fp32 and re-split; the file's bound for split plans"""
    arch, P, I, down, mid, _, ref, _ = _reference(tag)
    u = _native(arch, P, precise=True)
    ids = list(ref.keys())
    noise, hooks = _run(u, I, ids, _block(u, down, mid))
    errs = {k: rel_l2(hooks[k], ref[k]) for k in ids}
    worst = max(errs, key=errs.get)
    print(f"[{tag} residuals, precise] hooks={len(ids)} worst {worst} = {errs[worst]:.2e}")
    bad = {k: v for k, v in errs.items() if not v < TOL_SPLIT}
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1])[:8]
    assert rel_l2(noise, ref["unet-out"]) < TOL_SPLIT
    _, plain = _run(u, I, ids)
    for k in ids:
        assert torch.equal(plain[k], hooks[k]) == _untouched(k), k


def test_unet_call_packs_torch_residuals():
    """NativeUNet.__call__ with NCHW tensors (the reference's call, diffusion_feature.py:446-465) gives the bits of the packed block; a wrong
    count or shape is a ValueError; down residuals without the mid residual are the T2I-Adapter route and are refused"""
    arch, P, I, down, mid, _, ref, _ = _reference("xl")
    u = _native(arch, P, precise=False)
    ids = ["down-level1-repeat1-vit-out", "mid-repeat1-res-out", "up-level0-repeat0-res-out", "up-level2-repeat2-res-out"]
    noise, hooks = _run(u, I, ids, _block(u, down, mid))
    got = {}
    u.feature_store = types.SimpleNamespace(accept_all=False, to_store={k: True for k in ids}, store=lambda t, hid: got.__setitem__(hid, t))
    akw = {"text_embeds": I["text_embeds"].cuda(), "time_ids": I["time_ids"].cuda()}
    call = lambda d, m: u(I["sample"].cuda(), I["timestep"].cuda(), I["ctx"].cuda(), added_cond_kwargs=akw,
                          down_block_additional_residuals=d, mid_block_additional_residual=m, return_dict=False)[0]
    dn, md = [t.cuda().half() for t in down], mid.cuda().half()
    out = call(dn, md)
    torch.cuda.synchronize()
    assert torch.equal(out, noise) and list(got.keys()) == ids
    for k in ids:
        assert torch.equal(got[k], hooks[k]), k
    with pytest.raises(ValueError):
        call(dn[:-1], md)
    with pytest.raises(ValueError):
        call(dn[:3] + [dn[3][:, :, :4]] + dn[4:], md)
    with pytest.raises(ValueError):
        call(dn, md[:, :64])
    with pytest.raises(ValueError):
        call(dn, md[:1])
    with pytest.raises(NotImplementedError):
        call(dn, None)
    with pytest.raises(ValueError):
        _run(u, I, ids, _block(u, down, mid)[:-128])
    # a plan created for residuals does not run without them, and the other way round
    plan = u._plan(2, 16, 16, I["ctx"].shape[1], ids, False, 0, residuals=True)
    with pytest.raises(RuntimeError, match="gdf_forward_res"):
        plan.run(u.device, [("sample", I["sample"].cuda(), torch.float16), ("t", I["timestep"].cuda(), torch.float32), ("ctx", I["ctx"].cuda(), torch.float16),
                            ("txt", akw["text_embeds"], torch.float16), ("tid", akw["time_ids"], torch.float32)], (2, 16, 16, 4),
                 u._launch(plan, u.lib.gdf_forward, u.lib.gdf_plan_profile, "forward", False))
    torch.cuda.synchronize()


def test_early_exit_in_front_of_the_up_path_reads_no_residuals():
    """early_exit with down / mid hooks only: the op program ends before the adds; the call runs and returns the plain forward's hooks"""
    arch, P, I, down, mid, _, ref, _ = _reference("15")
    ids = ["down-level0-repeat1-vit-out", "down-level2-downsampler-out", "mid-vit-block0-ffn-inner", "mid-repeat1-res-out"]
    u = _native(arch, P, precise=False)
    _, full = _run(u, I, ids, _block(u, down, mid))
    ue = _native(arch, P, precise=False, early_exit=True)
    _, ee = _run(ue, I, ids, _block(ue, down, mid))
    _, plain = _run(ue, I, ids)
    n_full = u.lib.gdf_plan_num_ops(u._plan(1, 16, 16, I["ctx"].shape[1], ids, False, 0, residuals=True).handle)
    n_ee = ue.lib.gdf_plan_num_ops(ue._plan(1, 16, 16, I["ctx"].shape[1], ids, False, 0, residuals=True).handle)
    assert n_ee < n_full
    for k in ids:
        assert torch.equal(full[k], ee[k]) and torch.equal(plain[k], ee[k]), k
    # one more hook, behind the adds: the early-exit plan now runs them
    ids2 = ids + ["up-level0-repeat0-res-out"]
    _, a = _run(u, I, ids2, _block(u, down, mid))
    _, b = _run(ue, I, ids2, _block(ue, down, mid))
    _, c = _run(ue, I, ids2)
    assert torch.equal(a[ids2[-1]], b[ids2[-1]]) and not torch.equal(c[ids2[-1]], b[ids2[-1]])


def test_verify_ladder_passes_the_residuals_to_every_level(monkeypatch):
    """verify=True with residuals: the table's level (stubbed to plain, as tests/test_gpu_unet.py does for these shrunken widths) and the full
    split both run WITH the block — a full split without it would differ from the plain plan on every up hook by far more than the bound and
    escalate.  One check, no escalation, and the result handed out is the plain plan's own."""
    import warnings
    import components.plan_levels as PL
    monkeypatch.setattr(PL, "choose_split", lambda cfg, hook_ids, lat=None: 0)
    arch, P, I, down, mid, _, ref, _ = _reference("xl")
    ids = ["down-level1-repeat0-vit-block0-out", "mid-vit-block0-self-q", "up-level1-repeat0-vit-block0-out", "up-level2-repeat2-res-out"]
    u = _native(arch, P, precise="auto", verify=True)
    u.verify_bound = 3e-3
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        _, hv = _run(u, I, ids, _block(u, down, mid))
    assert not [x for x in w if "gdf verify" in str(x.message)]
    assert len(u.verify_log) == 1 and u.verify_log[0][2] == 0 and u.last_split == 0 and tuple(ids) in u._verified
    up = _native(arch, P, precise=False)
    _, plain = _run(up, I, ids, _block(up, down, mid))
    _, bare = _run(up, I, ids)
    for k in ids:
        assert torch.equal(hv[k], plain[k]), k
        assert rel_l2(hv[k], ref[k]) < TOL, k
    assert rel_l2(bare[ids[-1]], ref[ids[-1]]) > 10 * 3e-3           # what a level WITHOUT the block would have shown the ladder
