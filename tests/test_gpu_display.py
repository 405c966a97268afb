"""The display stage on the device: k_interlace and k_srgb8 against the host entries (amvpt_display.h).

k_interlace is integer and unfused float32 arithmetic, so the device image must equal amvpt_interlace_host's byte for
byte (tests/test_display.py pins the host entry on the restated reference); k_srgb8 forms its power from float64 +, -, *
alone, so it equals the host entry byte for byte too, and is held to the float64 curve under the same half-integer
band.  The many-block case has a row pitch of 3003
bytes (no multiple of 4), a last thread with one pixel, a 4-channel source and a preset whose view scale is not 1; the
2 x 2 and 5 x 2 outputs fit one thread and one thread plus a tail.  Every destination lies between guard bytes."""
import os

import numpy as np
import pytest

from conftest import SCENES
from test_display import (KATS, check_srgb8_ramp, kat_preset, pattern, ramp_image, special_values)

pytestmark = pytest.mark.gpu

CBOX = os.path.join(SCENES, "cbox_grid.xml")
GUARD = 64


@pytest.fixture(scope="module")
def D(amvpt_mod, gpu_ready):
    import amvpt.display as display
    return display


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _guarded(nbytes):
    """A device byte buffer with GUARD bytes of 0xA5 on each side of `nbytes` payload bytes."""
    torch = _torch()
    return torch.full((GUARD + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")


def _payload(buf, shape):
    host = buf.cpu().numpy()
    n = int(np.prod(shape))
    assert (host[:GUARD] == 0xA5).all() and (host[GUARD + n:] == 0xA5).all(), "guard bytes were written"
    return host[GUARD:GUARD + n].reshape(shape).copy()


def device_interlace(D, src, preset, size, quilt=False, nearest=False, stream=None, offset=0):
    """amvpt_interlace on the device over a guarded destination (`offset` shifts it off dword alignment)."""
    torch = _torch()
    dw, dh = size
    d_src = torch.from_numpy(np.ascontiguousarray(src)).cuda()
    buf = _guarded(dw * dh * 3 + offset)
    D.interlace_device(d_src.data_ptr(), src.shape[1], src.shape[0], src.shape[2], buf.data_ptr() + GUARD + offset,
                       (dw, dh), preset, quilt=quilt, nearest=nearest, stream=stream)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    n = dw * dh * 3
    assert (host[:GUARD + offset] == 0xA5).all() and (host[GUARD + offset + n:] == 0xA5).all(), "guard bytes were written"
    assert np.array_equal(d_src.cpu().numpy(), src), "the source was written"
    return host[GUARD + offset:GUARD + offset + n].reshape(dh, dw, 3).copy()


def device_srgb8(D, image, stream=None):
    torch = _torch()
    h, w, c = image.shape
    d_img = torch.from_numpy(np.ascontiguousarray(image, dtype=np.float32)).cuda()
    buf = _guarded(h * w * 3)
    D.srgb8_device(d_img.data_ptr(), c, w, h, buf.data_ptr() + GUARD, stream=stream)
    torch.cuda.synchronize()
    return _payload(buf, (h, w, 3))


def _case_id(k):
    return "%dx%d-%dx%d-%s-%s-%s" % (k["src"][0], k["src"][1], k["dst"][0], k["dst"][1], k["preset"],
                                     "quilt" if k["quilt"] else "lenticular", "nearest" if k["nearest"] else "bilinear")


@pytest.mark.parametrize("k", KATS["interlace"], ids=_case_id)
def test_interlace_equals_the_host_on_the_known_answers(D, k):
    src = pattern(*k["src"])
    p = kat_preset(D, k["preset"])
    want = D.interlace(src, p, tuple(k["dst"]), quilt=k["quilt"], nearest=k["nearest"])
    got = device_interlace(D, src, p, tuple(k["dst"]), quilt=k["quilt"], nearest=k["nearest"])
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]


@pytest.mark.parametrize("nearest", [False, True], ids=["bilinear", "nearest"])
def test_interlace_many_blocks_and_every_tail(D, nearest):
    """509 x 517 x 4 -> 1001 x 563: 550 blocks, rows of 3003 bytes, 563563 pixels = 140890 threads of four + three."""
    src = pattern(509, 517, 4)
    p = kat_preset(D, "second")
    want = D.interlace(src, p, (1001, 563), nearest=nearest)
    got = device_interlace(D, src, p, (1001, 563), nearest=nearest)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]


@pytest.mark.parametrize("size", [(2, 2), (5, 2)], ids=["2x2", "5x2"])
@pytest.mark.parametrize("offset", [0, 1], ids=["dword", "unaligned"])
def test_interlace_smallest_outputs(D, size, offset):
    """One thread, and one thread plus a two-pixel tail; at a destination off dword alignment the byte-store instance."""
    src = pattern(64, 96)
    p = kat_preset(D, "LKG4x8")
    for quilt in (False, True):
        want = D.interlace(src, p, size, quilt=quilt)
        got = device_interlace(D, src, p, size, quilt=quilt, offset=offset)
        assert np.array_equal(got, want), (quilt, got.tolist(), want.tolist())


def test_interlace_unaligned_destination_many_blocks(D):
    src = pattern(90, 45)
    p = kat_preset(D, "second")
    want = D.interlace(src, p, (333, 77))
    for offset in (1, 2, 3):
        got = device_interlace(D, src, p, (333, 77), offset=offset)
        assert np.array_equal(got, want), offset


def test_srgb8_ramp_on_the_device(D):
    out = device_srgb8(D, ramp_image())
    assert np.array_equal(out[..., 0], out[..., 1]) and np.array_equal(out[..., 0], out[..., 2])
    check_srgb8_ramp(out[..., 0].ravel())


@pytest.mark.parametrize("channels", [3, 4])
def test_srgb8_special_values_and_37x23(D, channels):
    """The special values, and a 37 x 23 image (851 pixels: 212 threads of four and a tail of three) with values
    from -0.125 to 1.125, equal the host entry byte for byte: the curve is float64 +, -, * on both sides."""
    x, want = special_values()
    img = np.zeros((1, len(x), channels), dtype=np.float32)
    img[..., :3] = x.reshape(1, -1, 1)
    img[..., 3:] = 0.5
    got = device_srgb8(D, img)
    assert np.array_equal(got, D.srgb8(img))
    assert np.array_equal(got[0, :, 0], want)
    rng = np.random.default_rng(11)
    img = (rng.random((23, 37, channels), dtype=np.float32) * np.float32(1.25) - np.float32(0.125))
    img[3, 5, :3] = (np.nan, np.inf, -np.inf)
    host, dev = D.srgb8(img), device_srgb8(D, img)
    assert np.array_equal(host, dev), np.argwhere(host != dev)[:8]
    assert dev[3, 5].tolist() == [0, 255, 0]
    assert len(np.unique(dev)) > 200


def test_srgb8_unaligned_buffers(D):
    """A source off 16-byte or a destination off 4-byte alignment takes the scalar instance: the same bytes."""
    torch = _torch()
    rng = np.random.default_rng(5)
    img = rng.random((23, 37, 3), dtype=np.float32)
    want = D.srgb8(img)
    flat = torch.zeros(img.size + 1, dtype=torch.float32, device="cuda")
    flat[1:] = torch.from_numpy(img.ravel()).cuda()
    for src_off, dst_off in ((1, 0), (0, 3), (1, 1)):
        buf = _guarded(want.size + dst_off)
        src = flat[1:] if src_off else flat[1:].clone()
        assert src.data_ptr() % 16 == (4 if src_off else 0)
        D.srgb8_device(src.data_ptr(), 3, 37, 23, buf.data_ptr() + GUARD + dst_off)
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        assert (host[:GUARD + dst_off] == 0xA5).all() and (host[GUARD + dst_off + want.size:] == 0xA5).all()
        assert np.array_equal(host[GUARD + dst_off:GUARD + dst_off + want.size], want.ravel()), (src_off, dst_off)


def _scene(amvpt_mod):
    return amvpt_mod.load_file(CBOX, res=32, gx=4, gy=2, spp=4)


def test_display_end_to_end_equals_the_host_entries(D, amvpt_mod):
    """display(scene) against the host entries applied to render(scene, seed=1), with the scene's preset.

    Two renders of one seed are not bit-identical: the splat sums floats with atomics in an order that varies
    (tests/test_gpu_parity.py holds two films to 1e-5 of the largest value; only AMVPT_OPT_DETERMINISTIC films are
    compared bit for bit).  So nothing here compares one render's bytes with another's.  The chain is exact instead,
    link by link, each on ONE frame: the stage alone (rerender=False) on the frame render() left on the device equals
    interlace(srgb8(image)) of that frame's download byte for byte, in every mode; and display() -- render and stage
    in one call -- equals the stage alone on the frame it rendered.  Both calls render the same lanes."""
    s = _scene(amvpt_mod)
    c_render, c_display = amvpt_mod.Counters(), amvpt_mod.Counters()
    image = amvpt_mod.render(s, seed=1, counters=c_render)
    p = D.preset_for_scene(s)
    assert tuple(p.grid) == (4, 2)
    quilt8 = D.srgb8(image)
    for quilt in (False, True):
        for nearest in (False, True):
            want = D.interlace(quilt8, p, (96, 54), quilt=quilt, nearest=nearest)
            same_frame = D.display(s, size=(96, 54), quilt=quilt, nearest=nearest, rerender=False)
            assert np.array_equal(same_frame, want), (quilt, nearest, np.argwhere(same_frame != want)[:8])
    want = D.interlace(quilt8, p, (96, 54))
    assert want.std() > 0 and len(np.unique(want)) > 50
    # an explicit preset, other than the scene's, on the same frame
    q = kat_preset(D, "second")
    assert np.array_equal(D.display(s, q, size=(41, 29), rerender=False), D.interlace(quilt8, q, (41, 29)))

    for quilt in (False, True):
        for nearest in (False, True):
            got = D.display(s, size=(96, 54), seed=1, quilt=quilt, nearest=nearest, counters=c_display)
            assert got.shape == (54, 96, 3) and got.dtype == np.uint8
            assert c_display.lanes == c_render.lanes and c_display.lanes > 0
            again = D.display(s, size=(96, 54), quilt=quilt, nearest=nearest, rerender=False)
            assert np.array_equal(got, again), (quilt, nearest)
    assert got.std() > 0


def test_display_refuses_before_rendering(D, amvpt_mod):
    s = _scene(amvpt_mod)
    with pytest.raises(RuntimeError, match="no developed frame"):
        D.display(s, size=(96, 54), rerender=False)
    before = amvpt_mod.render_stats(s)["renders"]
    with pytest.raises(RuntimeError, match="dst_w"):
        D.display(s, size=(1, 54))
    bad = D.preset_for_scene(s)
    bad.grid[1] = 0
    with pytest.raises(RuntimeError, match=r"grid\[1\]"):
        D.display(s, bad, size=(96, 54))
    assert amvpt_mod.render_stats(s)["renders"] == before


def test_display_on_a_caller_stream(D, amvpt_mod):
    """Render and stage on a caller stream: display(stream=st) equals the stage alone, on the same stream, on the frame
    it rendered; and the stage on the frame render(stream=st) left equals the host entries on that frame's download."""
    torch = _torch()
    s = _scene(amvpt_mod)
    st = torch.cuda.Stream()
    p = D.preset_for_scene(s)
    with torch.cuda.stream(st):
        got = D.display(s, size=(96, 54), seed=1, stream=st.cuda_stream)
        assert np.array_equal(got, D.display(s, size=(96, 54), rerender=False, stream=st.cuda_stream))
        image = amvpt_mod.render(s, seed=1, stream=st.cuda_stream)
        same_frame = D.display(s, size=(96, 54), rerender=False, stream=st.cuda_stream)
    assert np.array_equal(same_frame, D.interlace(D.srgb8(image), p, (96, 54)))
    assert got.std() > 0
    src = pattern(64, 96)
    p = kat_preset(D, "LKG4x8")
    assert np.array_equal(device_interlace(D, src, p, (96, 54), stream=st.cuda_stream), D.interlace(src, p, (96, 54)))
    ramp = ramp_image()
    check_srgb8_ramp(device_srgb8(D, ramp, stream=st.cuda_stream)[..., 0].ravel())


def test_stage_twice_reads_and_never_writes(D, amvpt_mod):
    """The stage reads the developed frame and never writes it or the film.

    On the scene's cache: after one render, the stage run twice (rerender=False) gives the host entries' bytes of that
    frame's download both times -- a stage that wrote the cached image would change its second result.
    On caller buffers, where the film itself can be read back: render into a film, develop, run both kernels twice;
    film, developed image and sRGB quilt are bit-identical afterwards, developing the film again gives the same
    image, and both display images equal the host entries'."""
    import ctypes
    torch = _torch()
    s = _scene(amvpt_mod)
    p = D.preset_for_scene(s)
    image = amvpt_mod.render(s, seed=1)
    want = D.interlace(D.srgb8(image), p, (96, 54))
    for _ in range(2):
        assert np.array_equal(D.display(s, size=(96, 54), rerender=False), want)

    L = amvpt_mod.hip_lib()
    sd, vd, prm = s.describe(0, 1, 0)
    dev = amvpt_mod.DeviceScene(sd)
    h, w = prm.film_height, prm.film_width
    C, T = (5, 4) if prm.film_alpha else (4, 3)
    film = torch.zeros((h, w, C), dtype=torch.float32, device="cuda")
    dev.render(vd, prm, film.data_ptr())
    img = torch.zeros((h, w, T), dtype=torch.float32, device="cuda")
    assert L.amvpt_develop(ctypes.c_void_p(film.data_ptr()), ctypes.c_void_p(img.data_ptr()), w, h, prm.film_alpha,
                           None) == 0
    torch.cuda.synchronize()
    film_keep, img_keep = film.clone(), img.clone()
    assert float(img.abs().max()) > 0
    q = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    out = torch.zeros((2, 54, 96, 3), dtype=torch.uint8, device="cuda")
    for i in range(2):
        D.srgb8_device(img.data_ptr(), T, w, h, q.data_ptr())
        torch.cuda.synchronize()
        qkeep = q.clone()
        D.interlace_device(q.data_ptr(), w, h, 3, out[i].data_ptr(), (96, 54), p)
        torch.cuda.synchronize()
        assert torch.equal(film, film_keep) and torch.equal(img, img_keep) and torch.equal(q, qkeep)
    img2 = torch.zeros_like(img)
    assert L.amvpt_develop(ctypes.c_void_p(film.data_ptr()), ctypes.c_void_p(img2.data_ptr()), w, h, prm.film_alpha,
                           None) == 0
    torch.cuda.synchronize()
    assert torch.equal(img2, img_keep)
    host = D.interlace(D.srgb8(img_keep.cpu().numpy()), p, (96, 54))
    assert np.array_equal(out[0].cpu().numpy(), host) and np.array_equal(out[1].cpu().numpy(), host)
