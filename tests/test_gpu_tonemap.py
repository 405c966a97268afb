"""The tone-mapping stage on the device (include/amvpt_tonemap.h): k_tonemap_hist, k_exposure and k_tonemap against the
host entries, which tests/test_tonemap.py pins on the header's definition.  Everything is compared bit for bit: the
whole state struct as bytes (the histogram is integer adds, the exposure float64 +, -, *, one correctly rounded
division and a power of two from its bits), float outputs as bit patterns, sRGB bytes as bytes.  Every output,
the state among them, lies between guard bytes, and the source is checked unchanged.

The shapes follow the kernels' constants (csrc/amvpt_tonemap.hip): 256 threads of four pixels, and a histogram grid
capped at 1024 blocks, so one round of it covers 1024 * 256 * 4 = 1 048 576 pixels."""
import ctypes
import os

import numpy as np
import pytest

from conftest import SCENES
from test_tonemap import SKIPPED, bin_gray, bins_ref, gray, hist_ref, lum32

pytestmark = pytest.mark.gpu

CBOX = os.path.join(SCENES, "cbox_grid.xml")
GUARD = 64
ONE_ROUND = 1024 * 256 * 4
OPS = ("linear", "reinhard", "aces")


@pytest.fixture(scope="module")
def A(amvpt_mod, gpu_ready):
    return amvpt_mod


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


class Guarded:
    """`nbytes` payload bytes on the device `offset` bytes behind GUARD bytes of 0xA5, with as many behind them."""

    def __init__(self, nbytes, offset=0, fill=None):
        torch = _torch()
        self.n, self.off = nbytes, GUARD + offset
        self.buf = torch.full((self.off + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        if fill is not None:
            self.buf[self.off:self.off + nbytes] = torch.from_numpy(np.frombuffer(fill, dtype=np.uint8).copy()).cuda()
        self.ptr = self.buf.data_ptr() + self.off

    def payload(self):
        host = self.buf.cpu().numpy()
        assert (host[:self.off] == 0xA5).all() and (host[self.off + self.n:] == 0xA5).all(), "guard bytes were written"
        return host[self.off:self.off + self.n].copy()


class Source:
    """A float32 image on the device, `offset` floats off the 16-byte alignment of its allocation."""

    def __init__(self, img, offset=0):
        torch = _torch()
        self.img = np.ascontiguousarray(img, dtype=np.float32)
        self.flat = torch.zeros(self.img.size + offset, dtype=torch.float32, device="cuda")
        self.flat[offset:] = torch.from_numpy(self.img.ravel()).cuda()
        self.ptr = self.flat.data_ptr() + 4 * offset
        assert self.ptr % 16 == 4 * offset
        self.h, self.w, self.c = self.img.shape

    def unchanged(self):
        got = self.flat.cpu().numpy()[self.flat.numel() - self.img.size:]
        assert np.array_equal(got.view(np.uint32), self.img.ravel().view(np.uint32)), "the source was written"


def device_meter(A, src, q, state=None, rect=None, stream=None):
    """amvpt_tonemap_meter into a guarded state that starts as `state` (None: fresh) -> (TonemapState, Guarded)."""
    g = state if isinstance(state, Guarded) else Guarded(ctypes.sizeof(A.TonemapState), fill=bytes(state or A.TonemapState()))
    A.tonemap_meter_device(src.ptr, src.c, src.w, src.h, g.ptr, q, rect=rect, stream=stream)
    _torch().cuda.synchronize()
    src.unchanged()
    return A.TonemapState.from_buffer_copy(g.payload().tobytes()), g


def device_map(A, src, q, state_ptr=None, as_bytes=True, offset=0, stream=None, sync=True):
    g = Guarded(src.h * src.w * (3 if as_bytes else 4 * src.c), offset=offset)
    (A.tonemap_srgb8_device if as_bytes else A.tonemap_device)(src.ptr, src.c, src.w, src.h, g.ptr, q, state_ptr=state_ptr,
                                                               stream=stream)
    _torch().cuda.synchronize()
    src.unchanged()
    out = g.payload()
    return out.reshape(src.h, src.w, 3) if as_bytes else out.view(np.float32).reshape(src.h, src.w, src.c)


def same_state(A, dev, host):
    assert bytes(dev) == bytes(host), ((dev.counted, dev.skipped, dev.frames, dev.exposure, dev.log2_exposure),
                                       (host.counted, host.skipped, host.frames, host.exposure, host.log2_exposure),
                                       np.nonzero(dev.histogram() != host.histogram())[0][:8])


def check_all(A, img, q, src_offset=0, dst_offset=0, rect=None):
    """meter, tonemap_srgb8 and tonemap_apply of one image on the device against the host, with the state's exposure
    (q.auto_exposure) or the manual one."""
    src = Source(img, src_offset)
    host = state_ptr = None
    if q.auto_exposure:
        host = A.tonemap_meter_host(img, q, rect=rect)
        dev, g = device_meter(A, src, q, rect=rect)
        same_state(A, dev, host)
        state_ptr = g.ptr
    got8 = device_map(A, src, q, state_ptr, True, dst_offset)
    want8 = A.tonemap_srgb8_host(img, q, state=host)
    assert np.array_equal(got8, want8), np.argwhere(got8 != want8)[:8]
    gotf = device_map(A, src, q, state_ptr, False, 4 * dst_offset)
    wantf = A.tonemap_host(img, q, state=host)
    assert np.array_equal(gotf.view(np.uint32), wantf.view(np.uint32)), np.argwhere(gotf.view(np.uint32) != wantf.view(np.uint32))[:8]
    return got8


def noise(shape, seed, spread=6.0):
    rng = np.random.default_rng(seed)
    img = np.exp2(rng.uniform(-spread, spread, shape)).astype(np.float32)
    if shape[2] == 4:
        img[..., 3] = rng.random(shape[:2], dtype=np.float32)
    return img


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("shape", [(1, 1, 3), (5, 37, 3), (5, 37, 4)], ids=["1x1", "37x5x3", "37x5x4"])
def test_smallest_shapes(A, shape, offset):
    """One pixel, and 185 pixels (46 threads of four and one pixel in the last); with the source 4 bytes off its
    alignment and the byte output 1 byte (the float output 4 bytes) off, the scalar-load and byte-store instances."""
    img = noise(shape, 31)
    if shape[1] > 1:
        img[2, 3, :3] = (np.nan, np.inf, -1.0)
        img[4, 36, :3] = 0.0
    for op in OPS:
        for auto in (False, True):
            q = A.TonemapParams(op=op, auto_exposure=auto, ev=0.5, white=3.0)
            out = check_all(A, img, q, offset, offset)
    assert shape[1] == 1 or len(np.unique(out)) > 20


def test_grid_stride_frame(A):
    """1025 x 1025 = 1 050 625 pixels: 2049 more than one round of the capped histogram grid covers, so the stride loop
    runs a second, ragged round of 512 threads of four and one thread with one pixel."""
    assert 1025 * 1025 - ONE_ROUND == 2049
    img = noise((1025, 1025, 3), 37)
    img[1024, 1024] = 3e4          # the pixel of the last thread: alone in its bin
    img[::7, ::5, 1] = 0.0
    q = A.TonemapParams(op="reinhard", auto_exposure=True)
    src = Source(img)
    host = A.tonemap_meter_host(img, q)
    dev, g = device_meter(A, src, q)
    same_state(A, dev, host)
    last = int(bins_ref(lum32(img[1024:, 1024:]))[0])
    assert dev.counted + dev.skipped == 1025 * 1025 and last > 480 and dev.hist[last] == 1
    got = device_map(A, src, q, g.ptr)
    assert np.array_equal(got, A.tonemap_srgb8_host(img, q, state=host))


def test_contention_frames(A):
    """Every pixel in one bin: the worst same-address contention, and the count is the pixel count exactly.  Then one
    pixel in each of the 512 bins beside the skipped values: every flush path once."""
    q = A.TonemapParams(auto_exposure=True)
    one = np.full((511, 513, 3), 0.5, dtype=np.float32)
    dev, _ = device_meter(A, Source(one), q)
    same_state(A, dev, A.tonemap_meter_host(one, q))
    assert dev.counted == 511 * 513 and dev.skipped == 0 and int(dev.histogram().max()) == 511 * 513
    black = np.zeros((300, 301, 4), dtype=np.float32)
    dev, _ = device_meter(A, Source(black), q)
    same_state(A, dev, A.tonemap_meter_host(black, q))
    assert (dev.counted, dev.skipped, dev.frames) == (0, 300 * 301, 0)
    each = np.concatenate([bin_gray({b: 1 for b in range(512)}), gray(SKIPPED)], axis=1)
    dev, _ = device_meter(A, Source(each), q)
    same_state(A, dev, A.tonemap_meter_host(each, q))
    assert (dev.histogram() == 1).all() and dev.skipped == len(SKIPPED)


@pytest.mark.parametrize("channels", [3, 4])
def test_metering_rectangle(A, channels):
    """A rectangle with an odd origin and an odd width inside a larger frame, rows of the full width from an odd row (one
    flat run of pixels, off 16-byte alignment with 3 channels), and the last pixel alone."""
    img = noise((45, 67, channels), 41)
    q = A.TonemapParams(auto_exposure=True)
    src = Source(img)
    for rect in ((3, 5, 31, 17), (0, 3, 67, 9), (66, 44, 1, 1), (1, 0, 65, 45)):
        host = A.tonemap_meter_host(img, q, rect=rect)
        dev, _ = device_meter(A, src, q, rect=rect)
        same_state(A, dev, host)
        assert np.array_equal(dev.histogram(), hist_ref(img, rect)[0]) and dev.counted == rect[2] * rect[3]


def test_state_reuse_and_adaptation(A):
    q = A.TonemapParams(auto_exposure=True, adapt=0.25)
    first, second = noise((33, 47, 3), 43, 3.0), noise((33, 47, 3), 47, 3.0) * np.float32(37.0)
    host = A.tonemap_meter_host(first, q)
    dev, g = device_meter(A, Source(first), q)
    same_state(A, dev, host)
    A.tonemap_meter_host(second, q, state=host)
    dev, g = device_meter(A, Source(second), q, state=g)
    same_state(A, dev, host)
    assert dev.frames == 2 and np.array_equal(dev.histogram(), hist_ref(second)[0])
    assert abs(dev.log2_exposure - host.log2_exposure) == 0 and dev.counted == 33 * 47


def test_stream_ordering(A):
    """meter and tonemap_srgb8 back to back on a stream of the caller's, nothing between them."""
    torch = _torch()
    img = noise((129, 257, 4), 53)
    q = A.TonemapParams(op="aces", auto_exposure=True, ev=-0.5)
    src = Source(img)
    state = Guarded(ctypes.sizeof(A.TonemapState), fill=bytes(A.TonemapState()))
    out = Guarded(129 * 257 * 3)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    A.tonemap_meter_device(src.ptr, 4, 257, 129, state.ptr, q, stream=st.cuda_stream)
    A.tonemap_srgb8_device(src.ptr, 4, 257, 129, out.ptr, q, state_ptr=state.ptr, stream=st.cuda_stream)
    st.synchronize()
    host = A.tonemap_meter_host(img, q)
    assert state.payload().tobytes() == bytes(host)
    assert np.array_equal(out.payload().reshape(129, 257, 3), A.tonemap_srgb8_host(img, q, state=host))
    src.unchanged()


@pytest.fixture(scope="module")
def rendered(A):
    s = A.load_file(CBOX, res=32, gx=4, gy=2, spp=4)
    return s, A.render(s, seed=1)


@pytest.mark.parametrize("auto", [False, True], ids=["manual", "auto"])
@pytest.mark.parametrize("op", OPS)
def test_operators_on_a_rendered_frame(A, rendered, op, auto):
    _, image = rendered
    assert image.max() > 1.0
    q = A.TonemapParams(op=op, auto_exposure=auto, ev=-1.0)
    out = check_all(A, image, q)
    assert len(np.unique(out)) > 50


def test_tone_mapper_object(A, rendered):
    torch = _torch()
    _, image = rendered
    q = A.TonemapParams(op="reinhard", auto_exposure=True, adapt=0.5)
    tm = A.ToneMapper(q)
    frame = torch.from_numpy(image).cuda()
    host = A.TonemapState()
    for scale, rect in ((1.0, None), (8.0, (32, 0, 64, 64))):
        f = (frame * scale).contiguous()
        A.tonemap_meter_host(f.cpu().numpy(), q, state=host, rect=rect)
        got = tm.run(f, rect=rect)
        torch.cuda.synchronize()
        assert bytes(tm.state()) == bytes(host)
        assert np.array_equal(got.cpu().numpy(), A.tonemap_srgb8_host(f.cpu().numpy(), q, state=host))
    assert host.frames == 2
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    gotf = tm.run_float(frame, stream=st.cuda_stream)
    st.synchronize()
    A.tonemap_meter_host(image, q, state=host)
    assert np.array_equal(gotf.cpu().numpy().view(np.uint32), A.tonemap_host(image, q, state=host).view(np.uint32))
    tm.reset()
    assert bytes(tm.state()) == bytes(A.TonemapState())
    manual = A.ToneMapper(A.TonemapParams(op="aces", ev=1.0))
    assert np.array_equal(manual.run(frame).cpu().numpy(), A.tonemap_srgb8_host(image, manual.params))
    with pytest.raises(ValueError, match="contiguous float32"):
        tm.run(image)


def test_display_with_a_tone_mapper(A):
    """display(..., tonemap=) returns the bytes of the same stages called one by one on the frame it showed, with an
    accumulator and without; tonemap=None returns the bytes the call returned before."""
    import amvpt.display as D
    s = A.load_file(CBOX, res=16, gx=4, gy=2, spp=1)
    size = (96, 54)
    p = D.preset_for_scene(s)
    D.display(s, size=size)
    plain = D.display(s, size=size, rerender=False)
    assert np.array_equal(plain, D.display(s, size=size, rerender=False, tonemap=None))
    q = A.TonemapParams(op="aces", auto_exposure=True)
    # without an accumulator: the plain torch path
    tm = A.ToneMapper(q)
    shown = D.display(s, size=size, seed=1, tonemap=tm)
    frame = tm.frame.cpu().numpy()
    host = A.tonemap_meter_host(frame, q)
    assert bytes(tm.state()) == bytes(host) and host.frames == 1
    assert shown.shape == (54, 96, 3) and np.array_equal(shown, D.interlace(A.tonemap_srgb8_host(frame, q, state=host), p, size))
    assert not np.array_equal(shown, D.interlace(D.srgb8(frame), p, size))
    # with one: the accumulated frame is what is metered and shown, and the state adapts over the calls
    acc, tm = A.TemporalAccumulator(), A.ToneMapper(A.TonemapParams(op="reinhard", auto_exposure=True, adapt=0.5))
    host = A.TonemapState()
    for seed in (1, 2):
        shown = D.display(s, size=size, seed=seed, temporal=acc, tonemap=tm)
        frame = acc.image.cpu().numpy()
        A.tonemap_meter_host(frame, tm.params, state=host)
        assert bytes(tm.state()) == bytes(host)
        assert np.array_equal(shown, D.interlace(A.tonemap_srgb8_host(frame, tm.params, state=host), p, size))
    assert host.frames == 2 and acc.frames == 2
    # a manual exposure through the denoiser's path, and the refusal of a cached frame
    manual = A.ToneMapper(A.TonemapParams(op="linear", ev=-2.0))
    dq = A.DenoiseParams(iterations=1)
    shown = D.display(s, size=size, seed=3, tonemap=manual, denoise=dq)
    assert np.array_equal(shown, D.interlace(A.tonemap_srgb8_host(manual.frame.cpu().numpy(), manual.params), p, size))
    with pytest.raises(ValueError, match="needs a fresh frame"):
        D.display(s, size=size, tonemap=tm, rerender=False)
