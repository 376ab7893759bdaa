"""The plan executor every model family runs through (csrc/plan_exec.cpp), pinned on the tiny SDXL topology: the live kernel timing of
gdf_plan_set_timing / _set_timing_stride / _read_timing inside graph replays (event-record nodes, one graph per event set) and in eager
execution, their argument errors, and the per-op profile."""
import ctypes as C
import math

import pytest
import torch

from helpers import cfg_from_oracle_arch
from oracle import unet_ref as R

pytestmark = pytest.mark.gpu
IDS = ["down-level1-repeat0-vit-block0-cross-q", "mid-vit-block1-out", "up-level2-repeat2-res-out", "unet-out"]
EV_RING = 4          # Plan::EV_RING: timing event sets, one graph each
N_FWD = 6            # more forwards than event sets, so the ring wraps


def _unet():
    from components.native import NativeUNet
    arch = R.tiny_arch("xl")
    P = R.synth_params(arch, seed=0)
    I = R.synth_inputs(arch, 2, 16, seed=1)
    unet = NativeUNet(cfg_from_oracle_arch(arch), device="cuda:0")
    unet.load_state_dict({k: v.half() for k, v in P.items()})
    args = [I[k].cuda() for k in ("sample", "timestep", "ctx", "text_embeds", "time_ids")]
    return unet, args


def _hooks(unet, args):
    """one forward; clones of its hooks, the result itself dropped (so that the plan hands the same hook-buffer set out again)"""
    out = unet.forward_raw(*args, hook_ids=IDS)[1]
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in out.items()}


def _read(lib, plan):
    ms, n, fl = C.c_double(), C.c_long(), C.c_double()
    assert lib.gdf_plan_read_timing(plan.handle, C.byref(ms), C.byref(n), C.byref(fl)) == 0
    return ms.value, n.value, fl.value


def _timed_forwards(graph):
    assert N_FWD > EV_RING
    unet, args = _unet()
    lib = unet.lib
    ref = _hooks(unet, args)                                        # the plan's first forward: eager, untimed
    plan = unet._plan(2, 16, 16, 77, IDS, False)
    assert plan.graph == graph and plan.graph_stats() == (0, 0, 0)
    prof = unet.forward_raw(*args, hook_ids=IDS, profile=True)[2]   # [(name, ms, flops, kernel label)] in program order
    torch.cuda.synchronize()
    by_label = {}
    for _, _, fl, lab in prof:
        by_label.setdefault(lab, []).append(fl)
    L = max(by_label, key=lambda k: len(by_label[k]))
    n_L = len(by_label[L])
    assert n_L >= 4                                                 # a stride of 3 skips ops and leaves a remainder
    if graph:                                                       # the untimed graph of this binding exists before timing starts
        assert all(torch.equal(v, ref[k]) for k, v in _hooks(unet, args).items())
        assert plan.graph_stats() == (1, 1, 0)
    for stride in (1, 3):
        assert lib.gdf_plan_set_timing_stride(plan.handle, stride) == 0, lib.gdf_last_error()
        assert lib.gdf_plan_set_timing(plan.handle, L.encode()) == 0, lib.gdf_last_error()
        for _ in range(N_FWD):
            got = _hooks(unet, args)
            for k in IDS:
                assert torch.equal(got[k], ref[k]), (stride, k)
        ms, launches, flops = _read(lib, plan)
        want = N_FWD * sum(by_label[L][::stride])
        print("stride %d: label %s, %d ops, %d launches, %.4f ms, %.6g flop (expected %.6g)" % (stride, L, n_L, launches, ms, flops, want))
        assert launches == N_FWD * math.ceil(n_L / stride)
        assert math.isfinite(ms) and ms > 0
        assert abs(flops - want) <= 1e-9 * max(want, 1.0)
        assert plan.graph_stats()[2] == 0
        assert lib.gdf_plan_set_timing(plan.handle, None) == 0      # (the stride may only change while no label is timed)
    before = plan.graph_stats()
    got = _hooks(unet, args)
    assert all(torch.equal(got[k], ref[k]) for k in IDS)
    after = plan.graph_stats()
    if graph:
        assert after == (before[0], before[1] + 1, 0), (before, after)   # a replay of the untimed graph: nothing new is built
    else:
        assert before == after == (0, 0, 0)
    assert _read(lib, plan) == (0.0, 0, 0.0)                        # switched off: nothing accumulates


def test_timed_graph_replay(monkeypatch):
    monkeypatch.setenv("GDF_HIP_GRAPH", "1")
    _timed_forwards(True)


def test_timed_eager_execution(monkeypatch):
    monkeypatch.setenv("GDF_HIP_GRAPH", "0")                        # read by _Plan.__init__
    _timed_forwards(False)


def test_timing_argument_errors():
    unet, args = _unet()
    lib = unet.lib
    _hooks(unet, args)
    plan = unet._plan(2, 16, 16, 77, IDS, False)
    assert lib.gdf_plan_set_timing(plan.handle, b"no_such_kernel") != 0
    assert b"no op with kernel label" in lib.gdf_last_error()
    assert lib.gdf_plan_set_timing_stride(plan.handle, 0) != 0
    assert b"timing stride must be >= 1" in lib.gdf_last_error()
    label = lib.gdf_plan_op_kernel(plan.handle, 0)
    assert lib.gdf_plan_set_timing(plan.handle, label) == 0, lib.gdf_last_error()
    assert lib.gdf_plan_set_timing_stride(plan.handle, 2) == 3      # GDF_ERR_STATE
    assert b"set the stride before gdf_plan_set_timing" in lib.gdf_last_error()
    assert lib.gdf_plan_set_timing(plan.handle, None) == 0
    assert lib.gdf_plan_set_timing_stride(plan.handle, 2) == 0


def test_profile_rows_match_the_op_program(monkeypatch):
    monkeypatch.setenv("GDF_HIP_GRAPH", "1")
    unet, args = _unet()
    lib = unet.lib
    ref = _hooks(unet, args)
    plan = unet._plan(2, 16, 16, 77, IDS, False)
    assert all(torch.equal(v, ref[k]) for k, v in _hooks(unet, args).items())
    before = plan.graph_stats()
    assert before == (1, 1, 0)
    _, hooks, prof = unet.forward_raw(*args, hook_ids=IDS, profile=True)
    torch.cuda.synchronize()
    assert len(prof) == lib.gdf_plan_num_ops(plan.handle) > 0
    for i, (name, ms, flops, label) in enumerate(prof):
        assert name and label == lib.gdf_plan_op_kernel(plan.handle, i).decode(), i
        assert ms >= 0 and flops >= 0, (i, name, ms, flops)
    assert plan.graph_stats() == before
    for k in IDS:
        assert torch.equal(hooks[k], ref[k]), k
