"""CPU-side checks of guided sampling with background extraction (no GPU): the probed scheduler table NativeUNet.sample runs
(components/models.py sampling_table) against three small schedulers written here from the published algorithms — an Euler step in the
sigma parameterisation (Karras et al. 2022, alg. 1 without churn), PLMS (Liu et al. 2022, eq. 9 + the Adams-Bashforth weights of eq. 12,
with the warm-up that visits the second timestep twice) and an ancestral Euler step (noise added in `step`) —, the encounter -> row
mapping, and the new entry points."""
import ctypes
import math

import pytest
import torch


def _alphas(n=1000):
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, n, dtype=torch.float64) ** 2       # SD's scaled-linear schedule
    return torch.cumprod(1.0 - betas, 0)


class EulerSched:
    """x_{k+1} = x_k + (sigma_{k+1} - sigma_k) eps on the sigma scale; the model sees x / sqrt(sigma^2 + 1).  Order 1, c_in != 1."""

    def __init__(self):
        self.alphas_cumprod = _alphas()
        self.timesteps = None

    def set_timesteps(self, n, device=None):
        self.timesteps = torch.linspace(999, 0, n).round().long()
        ac = self.alphas_cumprod[self.timesteps]
        self.sigmas = torch.cat([((1 - ac) / ac) ** 0.5, torch.zeros(1, dtype=torch.float64)])
        self.init_noise_sigma = float(self.sigmas[0])             # (diffusers' 'linspace' spacing: the largest sigma)
        self.i = 0

    def scale_model_input(self, x, t):
        return x / (self.sigmas[self.i] ** 2 + 1) ** 0.5

    def step(self, eps, t, x, return_dict=False):
        out = x + (self.sigmas[self.i + 1] - self.sigmas[self.i]) * eps
        self.i += 1
        return (out,)


class AncestralSched(EulerSched):
    """Euler ancestral: step down to sigma_down, then add sigma_up * randn."""

    def step(self, eps, t, x, return_dict=False):
        s, sn = self.sigmas[self.i], self.sigmas[self.i + 1]
        up = (sn ** 2 * (s ** 2 - sn ** 2) / s ** 2) ** 0.5
        down = (sn ** 2 - up ** 2) ** 0.5
        out = x + (down - s) * eps + up * torch.randn(x.shape, dtype=x.dtype)
        self.i += 1
        return (out,)


class PLMSSched:
    """Pseudo linear multistep with the one-step warm-up that needs no Runge-Kutta calls: call 0 takes e_0 as it is, call 1 — at the SAME
    timestep as call 2's predecessor, i.e. the second timestep is listed twice — redoes the first transfer with (e_0 + e_1) / 2, then
    (3 e_1 - e_0) / 2, (23, -16, 5) / 12 and (55, -59, 37, -9) / 24 from there on.  The output of call 1 is not kept: the history holds one output per DISTINCT
    timestep, so the first four-term step (call 4) reaches back to call 0 — five calls, the depth of the sampler's ring."""

    def __init__(self):
        self.alphas_cumprod = _alphas()
        self.timesteps = None

    def set_timesteps(self, n, device=None):
        self.gap = 1000 // n
        ts = (torch.arange(0, n) * self.gap).long() + 1
        self.timesteps = torch.cat([ts[:-1], ts[-2:-1], ts[-1:]]).flip(0)            # e.g. 6 steps: 7 entries, the second one twice
        self.ets, self.counter, self.cur = [], 0, None

    def scale_model_input(self, x, t):
        return x

    def _transfer(self, x, t, prev, e):
        a_t = self.alphas_cumprod[t]
        a_p = self.alphas_cumprod[prev] if prev >= 0 else torch.tensor(1.0, dtype=torch.float64)
        den = a_t * (1 - a_p) ** 0.5 + (a_t * (1 - a_t) * a_p) ** 0.5
        return (a_p / a_t) ** 0.5 * x - (a_p - a_t) * e / den

    def step(self, eps, t, x, return_dict=False):
        t = int(t)
        prev = t - self.gap
        if self.counter != 1:
            self.ets = self.ets[-3:]
            self.ets.append(eps)
        else:
            prev, t = t, t + self.gap
        if len(self.ets) == 1 and self.counter == 0:
            e = eps
            self.cur = x
        elif len(self.ets) == 1 and self.counter == 1:
            e = (eps + self.ets[-1]) / 2
            x, self.cur = self.cur, None
        elif len(self.ets) == 2:
            e = (3 * self.ets[-1] - self.ets[-2]) / 2
        elif len(self.ets) == 3:
            e = (23 * self.ets[-1] - 16 * self.ets[-2] + 5 * self.ets[-3]) / 12
        else:
            e = (55 * self.ets[-1] - 59 * self.ets[-2] + 37 * self.ets[-3] - 9 * self.ets[-4]) / 24
        self.counter += 1
        return (self._transfer(x, t, prev, e),)


def _own_chain(sch, n, x0, es):
    sch.set_timesteps(n)
    x, xs = x0.clone(), []
    for k, t in enumerate(sch.timesteps):
        sch.scale_model_input(x, t)
        x = sch.step(es[k], t, x)[0]
        xs.append(x)
    return xs


@pytest.mark.parametrize("cls,n_rows", [(EulerSched, 6), (PLMSSched, 7)])
def test_table_reproduces_the_schedulers_own_chain(cls, n_rows):
    """float64 on both sides, coefficient ratios <= 1e3: 1e-9 relative at every step."""
    from components.models import sampling_table
    rows, sigma0 = sampling_table(cls(), 6)
    assert len(rows) == n_rows
    g = torch.Generator().manual_seed(7)
    x0 = torch.randn(2, 4, 8, 8, generator=g, dtype=torch.float64)
    es = [torch.randn(2, 4, 8, 8, generator=g, dtype=torch.float64) for _ in rows]
    want = _own_chain(cls(), 6, x0, es)
    x = x0.clone()
    for k, (t, c_in, c_s, *w) in enumerate(rows):
        x = c_s * x + sum(w[j] * es[k - j] for j in range(min(5, k + 1)))
        err = float((x - want[k]).abs().max()) / float(want[k].abs().max())
        assert err <= 1e-9, (k, err)
    sch = cls()
    sch.set_timesteps(6)
    assert [r[0] for r in rows] == [float(t) for t in sch.timesteps]
    if cls is EulerSched:
        assert all(r[2] == 1.0 for r in rows)                                   # the Euler step keeps the sample's coefficient at 1
        assert all(r[1] != 1.0 and abs(r[1] - 1 / math.sqrt(float(sch.sigmas[k]) ** 2 + 1)) <= 1e-12 for k, r in enumerate(rows))
        assert all(r[3] != 0.0 and r[4:] == (0.0, 0.0, 0.0, 0.0) for r in rows)
        assert sigma0 == sch.init_noise_sigma and sigma0 > 10
    else:
        assert [sum(1 for v in r[3:] if v != 0.0) for r in rows] == [1, 2, 2, 3, 4, 4, 4]
        assert rows[4][7] != 0.0 and rows[4][6] == 0.0                          # call 4: outputs 4, 3, 2 and 0
        assert rows[1][0] == rows[2][0]                                         # the second timestep twice: two rows, two UNet calls
        assert all(r[1] == 1.0 for r in rows) and sigma0 == 1.0                  # no init_noise_sigma attribute -> 1.0


def test_stochastic_scheduler_is_refused_by_name():
    from components.models import sampling_table
    torch.manual_seed(0)
    with pytest.raises(NotImplementedError, match="AncestralSched"):
        sampling_table(AncestralSched(), 6)


def test_synthetic_scheduler_goes_through_the_same_probe():
    from components.models import _Scheduler, sampling_table
    for euler in (False, True):
        s = _Scheduler(euler)
        rows, sigma0 = sampling_table(s, 6)
        assert s.timesteps is None                                              # probed on copies
        s.set_timesteps(6)
        assert len(rows) == 6 and [r[0] for r in rows] == [float(t) for t in s.timesteps] and sigma0 == 1.0
        c_s, c_e = s.step_scalars(s.timesteps[0])
        assert abs(rows[0][2] - c_s) <= 1e-12 * abs(c_s) and abs(rows[0][3] - c_e) <= 1e-12 * abs(c_e)
        assert rows[0][4:] == (0.0, 0.0, 0.0, 0.0)
        assert abs(rows[0][1] - float(s.scale_model_input(torch.ones(1, dtype=torch.float64), s.timesteps[0]))) <= 1e-12


def test_encounters_map_to_rows():
    from components.feature_extractor import background_capture_rows
    assert background_capture_rows([1, 3, 99], 7) == [0, 2]
    assert background_capture_rows(None, 7) == [6]
    assert background_capture_rows([7, 1, 1], 7) == [0, 6]
    assert background_capture_rows([0, 8], 7) == []


def test_sampler_entry_points_are_exported_and_bound():
    import __graft_entry__ as G
    G.build()
    from components import native
    import diffusion_feature
    lib = ctypes.CDLL(G.LIB)
    for name in ("gdf_sample", "gdf_sample_state_bytes", "gdf_op_guided_step"):
        assert hasattr(lib, name), name
        assert name in native.SIGNATURES, name
    L = native.load_library()
    assert L.gdf_sample.restype is ctypes.c_int and len(L.gdf_sample.argtypes) == 17
    assert lib.gdf_abi_version() == 1                                                        # additive: the ABI version stays
    assert hasattr(native.NativeUNet, "sample") and hasattr(diffusion_feature.FeatureExtractor, "generate")
    # the state block: fp16 input + timesteps + five fp32 history slots + the steps block, and nothing for a bad request
    n = L.gdf_sample_state_bytes(4, 16, 16, 7)
    assert n >= 4 * 4 * 256 * (2 + 20) + 4 * 4 + 32 + 7 * 32 and n % 256 == 0
    assert L.gdf_sample_state_bytes(4, 16, 16, 0) == 0 and L.gdf_sample_state_bytes(4, 16, 16, 1025) == 0
    # a null plan is refused with a message, not a crash
    assert L.gdf_sample(None, None, None, 1, None, 1.0, None, None, None, None, 0, None, None, None, None, None, None) != 0
    assert b"null plan" in L.gdf_last_error()


def test_generate_refuses_what_it_does_not_cover():
    """(the checks come before anything touches the pipeline, so a bare object stands in for the extractor)"""
    import types
    import diffusion_feature as D
    for v in ("flux", "pixart-sigma"):
        with pytest.raises(NotImplementedError, match="UNet versions"):
            D.FeatureExtractor.generate(types.SimpleNamespace(version=v, attention=None), None, 1)
    with pytest.raises(NotImplementedError, match="attention"):
        D.FeatureExtractor.generate(types.SimpleNamespace(version="1-5", attention=["up_cross"]), None, 1)
