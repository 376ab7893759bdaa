"""csrc/preproc.hip on the device (-m gpu): the coefficient tables against the NumPy oracle (tests/pil_resample_oracle.py) int for int, the uint8
output against Pillow itself byte for byte, the fp32 output against FeatureExtractor.preprocess_image bit for bit, for every shape of the oracle's
CASES as RGB noise, RGB of bytes 0 / 255 and L.  Every destination and the workspace sit between guard bytes that must survive, and the sources
start at odd byte offsets as they do in a staging buffer."""
import ctypes as C
import functools
import importlib.util
import os
import types

import numpy as np
import pytest
import torch
from PIL import Image

import pil_resample_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
GUARD = 64                                   # bytes (a multiple of 16: the workspace behind its guard stays 16-byte aligned)
FILL = 0xA5
IDS = ["%dx%d-%d" % (h, w, s) for (h, w), s in O.CASES]


@pytest.fixture(scope="module")
def lib():
    from components import native
    return native.load_library()


def _stream():
    return C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _guarded(nbytes):
    """a device buffer of nbytes between two guards -> (whole buffer, address of the payload)"""
    buf = torch.full((GUARD + nbytes + GUARD,), FILL, dtype=torch.uint8, device=DEV)
    return buf, buf.data_ptr() + GUARD


def _payload(buf, nbytes):
    g = buf.cpu().numpy()
    assert (g[:GUARD] == FILL).all() and (g[GUARD + nbytes:] == FILL).all(), "guard bytes were written"
    return g[GUARD:GUARD + nbytes]


@functools.lru_cache(maxsize=None)
def _reference(case, kind):
    """(source array, Pillow's bytes (S, S, 3)) — made once per case and kind, shared by the tests below, never modified"""
    (h, w), s = O.CASES[case]
    a = O.source(kind, h, w)
    want = np.array(Image.fromarray(a).resize((s, s)).convert("RGB"))
    a.setflags(write=False)
    want.setflags(write=False)
    return a, want


def _resize(lib, a, size, offset, want_u8, want_f32):
    """gdf_op_pil_resize_u8 of the array a, its bytes at `offset` into a device buffer -> (uint8 (S, S, 3) | None, fp32 (3, S, S) | None)"""
    h, w = a.shape[:2]
    c = 1 if a.ndim == 2 else 3
    src = torch.full((offset + a.size + 16,), FILL, dtype=torch.uint8, device=DEV)
    src[offset:offset + a.size] = torch.from_numpy(a.reshape(-1).copy()).to(DEV)
    n_ws = lib.gdf_op_pil_resize_workspace_bytes(h, w, c, size, size)
    assert n_ws >= 16 and n_ws % 16 == 0
    ws, ws_p = _guarded(n_ws)
    u8, u8_p = _guarded(size * size * 3) if want_u8 else (None, None)
    f32, f32_p = _guarded(size * size * 3 * 4) if want_f32 else (None, None)
    rc = lib.gdf_op_pil_resize_u8(C.c_void_p(src.data_ptr() + offset), h, w, c, size, size, C.c_void_p(u8_p), C.c_void_p(f32_p), C.c_void_p(ws_p),
                                  _stream())
    assert rc == 0, lib.gdf_last_error()
    torch.cuda.synchronize()
    _payload(ws, n_ws)
    got_u8 = _payload(u8, size * size * 3).reshape(size, size, 3) if want_u8 else None
    got_f32 = _payload(f32, size * size * 12).view(np.float32).reshape(3, size, size) if want_f32 else None
    return got_u8, got_f32


@pytest.mark.parametrize("n_in,n_out", O.axis_pairs(), ids=lambda v: str(v))
def test_tables_equal_the_oracle(lib, n_in, n_out):
    want_b, want_k, ksize = O.coeffs(n_in, n_out)
    bounds, bounds_p = _guarded(n_out * 8)
    kk, kk_p = _guarded(n_out * ksize * 4)
    ks = C.c_int(0)
    rc = lib.gdf_op_pil_coeffs(n_in, n_out, C.c_void_p(bounds_p), C.c_void_p(kk_p), C.byref(ks), _stream())
    assert rc == 0, lib.gdf_last_error()
    torch.cuda.synchronize()
    assert ks.value == ksize
    assert np.array_equal(_payload(bounds, n_out * 8).view(np.int32).reshape(n_out, 2), want_b)
    assert np.array_equal(_payload(kk, n_out * ksize * 4).view(np.int32).reshape(n_out, ksize), want_k)


@pytest.mark.parametrize("case", range(len(O.CASES)), ids=IDS)
def test_bytes_equal_pillow(lib, case):
    size = O.CASES[case][1]
    for j, kind in enumerate(O.KINDS):
        a, want = _reference(case, kind)
        got, _ = _resize(lib, a, size, (case + 2 * j) % 4, True, False)       # offsets 0 .. 3: odd ones for every case
        assert np.array_equal(got, want), kind


def _extractor(processor, size):
    """FeatureExtractor.preprocess_image over the given image processor, nothing else of the extractor"""
    import diffusion_feature as D
    fe = D.FeatureExtractor.__new__(D.FeatureExtractor)
    torch.nn.Module.__init__(fe)
    fe.img_size, fe.pipe = size, types.SimpleNamespace(image_processor=processor)
    return fe


@functools.lru_cache(maxsize=None)
def _processors():
    from components.models import SyntheticPipe
    spec = importlib.util.spec_from_file_location("_fake_diffusers_pil_gpu", os.path.join(ROOT, "tests", "fake_diffusers", "diffusers", "__init__.py"))
    fake = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fake)
    return (types.SimpleNamespace(preprocess=lambda im: SyntheticPipe._preprocess(None, im)), fake.VaeImageProcessor(vae_scale_factor=8))


@pytest.mark.parametrize("case", range(len(O.CASES)), ids=IDS)
def test_floats_equal_preprocess_image(lib, case):
    size = O.CASES[case][1]
    for j, kind in enumerate(O.KINDS):
        a, _ = _reference(case, kind)
        _, got = _resize(lib, a, size, (case + 2 * j + 1) % 4, False, True)
        got = torch.from_numpy(got.copy())[None]
        for proc in _processors():
            want = _extractor(proc, size).preprocess_image(Image.fromarray(a))
            assert want.dtype == torch.float32 and tuple(want.shape) == (1, 3, size, size) and torch.equal(got, want), (kind, type(proc).__name__)


def test_both_destinations_in_one_call_and_every_offset(lib):
    case = 0
    size = O.CASES[case][1]
    for off in range(16):
        kind = O.KINDS[off % 3]
        a, want = _reference(case, kind)
        u8, f32 = _resize(lib, a, size, off, True, True)
        assert np.array_equal(u8, want) and np.array_equal(f32, O.normalise(want)), (off, kind)


def test_device_preprocess_mixed_batch_equals_the_host_path(lib):
    """components/preproc.py: RGB of two sizes, L, a source of the target size, and RGBA / P, which fall back to the host image by image"""
    from components import preproc as P
    size = 64
    g = np.random.default_rng(11)
    rgb = [Image.fromarray(g.integers(0, 256, s + (3,), dtype=np.uint8)) for s in ((90, 70), (41, 133), (size, size))]
    imgs = [rgb[0], Image.fromarray(g.integers(0, 256, (50, 77), dtype=np.uint8)), rgb[1].convert("RGBA"), rgb[2], rgb[0].convert("P")]
    fe = _extractor(_processors()[0], size)
    want = torch.cat([fe.preprocess_image(im) for im in imgs], 0)
    for _ in range(P.RING + 2):                                               # more calls than staging buffers: the ring wraps
        got = P.device_preprocess(imgs, size, DEV, host_fn=fe.preprocess_image)
        assert got.is_cuda and got.dtype == torch.float32 and torch.equal(got.cpu(), want)
