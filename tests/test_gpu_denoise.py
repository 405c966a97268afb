"""The a-trous denoiser on the device (include/amvpt_denoise.h) against its host entry, bit for bit.

amvpt_denoise_host is pinned to a numpy restatement of the definition by tests/test_denoise.py; here amvpt_denoise
must equal it on every float of the same cases and of sizes around the 32 x 8 tile, with iterations 1 .. 5 so that
both step classes run (the LDS-staged kernel at steps 1 and 2, the direct one from step 4), with guard floats behind
out and scratch and with the inputs compared before and after.  Then the layers above: amvpt.denoise and the host
library's entry on the device scene and frame a render cached.
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import SCENES
from test_denoise import (CASE_NAMES, SENTINEL, build_cases, params_of, random_image, refusal_rows, synthetic_guides)
from test_gpu_bvh_walks import _torch
from test_guides import bits, open_scene_xml

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 256   # floats behind out and scratch that must stay as they were
SIZES = {"one_tile_32x8": (32, 8), "tile_plus_one_33x9": (33, 9), "two_tiles_less_one_63x15": (63, 15),
         "wide_257x3": (257, 3)}


@pytest.fixture(scope="module", autouse=True)
def _device_started(gpu_ready, amvpt_mod):
    """The process's one-time costs (torch, the HIP context, the code objects) are paid here when this module is the
    first to use the device."""
    torch = _torch()
    g = torch.zeros((8, 8, 8), dtype=torch.float32, device="cuda")
    img = torch.ones((8, 8, 3), dtype=torch.float32, device="cuda")
    out = torch.zeros_like(img)
    amvpt_mod.denoise_device(img.data_ptr(), 3, 8, 8, g.data_ptr(), out.data_ptr(), None, params_of(amvpt_mod, 1))
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def cases(oracle, amvpt_mod):
    hits = []
    for s in (amvpt_mod.load_file(os.path.join(SCENES, "cbox_grid.xml"), res=16, gx=4, gy=2),
              amvpt_mod.load_string(open_scene_xml(), res=16, gx=4, gy=2)):
        sd, vd, p = s.describe(0, 0, 0)
        hits.append(oracle.primary_hits(sd, vd, p))
    all_ = build_cases(*hits)
    for name, (w, h) in SIZES.items():
        all_[name] = (synthetic_guides(w, h, 40 + w), None)
    return all_


def _device_denoise(amvpt_mod, img, g, q, with_scratch=True):
    """amvpt_denoise on uploads of img and g -> the result; asserts the guards and that the inputs are as uploaded."""
    torch = _torch()
    h, w, c = img.shape
    n = img.size
    d_img, d_g = torch.from_numpy(img).cuda(), torch.from_numpy(np.ascontiguousarray(g)).cuda()
    out = torch.full((n + GUARD,), float(SENTINEL), dtype=torch.float32, device="cuda")
    scratch = torch.full((n + GUARD,), float(SENTINEL), dtype=torch.float32, device="cuda") if with_scratch else None
    amvpt_mod.denoise_device(d_img.data_ptr(), c, w, h, d_g.data_ptr(), out.data_ptr(),
                             scratch.data_ptr() if scratch is not None else None, q)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[n:] == SENTINEL).all(), "the guard behind out was written"
    if scratch is not None:
        s = scratch.cpu().numpy()
        assert (s[n:] == SENTINEL).all(), "the guard behind scratch was written"
        assert (s[:n] == SENTINEL).all() == (q.iterations == 1)
    assert np.array_equal(bits(d_img.cpu().numpy()), bits(img)), "the image was modified on the device"
    assert np.array_equal(bits(d_g.cpu().numpy()), bits(g)), "the guides were modified on the device"
    return o[:n].reshape(h, w, c)


def _assert_same(got, want):
    same = bits(got) == bits(want)
    assert same.all(), "%d of %d floats differ from the host entry, first at %s" % (
        (~same).sum(), same.size, np.argwhere(~same)[:3].tolist())


# ---- 1. device against host, bit for bit ---------------------------------------------------------------------------

@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("name", CASE_NAMES + list(SIZES))
def test_device_equals_host(gpu_ready, amvpt_mod, cases, name, channels):
    g, tile = cases[name]
    img = random_image(g, channels, 100 + channels, tile=tile)
    assert not np.isfinite(img).all()
    for iterations in (1, 2, 3, 4, 5):
        q = params_of(amvpt_mod, iterations)
        _assert_same(_device_denoise(amvpt_mod, img, g, q), amvpt_mod.denoise_host(img, g, q))
    q1 = params_of(amvpt_mod, 1)
    _assert_same(_device_denoise(amvpt_mod, img, g, q1, with_scratch=False), amvpt_mod.denoise_host(img, g, q1))


def test_other_parameters(gpu_ready, amvpt_mod, cases):
    g, _ = cases["synthetic_37x29"]
    img = random_image(g, 3, 21)
    for q in (amvpt_mod.DenoiseParams(8, 0.3, 0.5, 0.011, 0), amvpt_mod.DenoiseParams(2, 7.0, 1e-4, 3.0, 7)):
        _assert_same(_device_denoise(amvpt_mod, img, g, q), amvpt_mod.denoise_host(img, g, q))


# ---- 2. end to end ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def rendered(amvpt_mod):
    """cbox_grid.xml res=32, 4 spp: a device render developed on the device, and DeviceScene.guides, downloaded."""
    torch = _torch()
    s = amvpt_mod.load_file(os.path.join(SCENES, "cbox_grid.xml"), res=32, spp=4, gx=4, gy=2)
    sd, vd, p = s.describe(0, 0, 0)
    w, h = p.film_width, p.film_height
    dev = amvpt_mod.DeviceScene(sd)
    film = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    img = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    g = torch.zeros((h, w, 8), dtype=torch.float32, device="cuda")
    dev.render(vd, p, film.data_ptr())
    L = amvpt_mod.hip_lib()
    assert L.amvpt_develop(ctypes.c_void_p(film.data_ptr()), ctypes.c_void_p(img.data_ptr()), w, h, p.film_alpha, None) == 0
    dev.guides(vd, p, g.data_ptr())
    torch.cuda.synchronize()
    return s, img.cpu().numpy(), g.cpu().numpy()


def test_end_to_end(gpu_ready, amvpt_mod, rendered):
    s, img, g = rendered
    assert img.shape == (64, 128, 3) and np.isfinite(img).all() and img.max() > 0
    sp = amvpt_mod.denoise_sigma_plane(g)
    assert 0.04 < sp < 0.06
    got = amvpt_mod.denoise(s, image=img)
    want = amvpt_mod.denoise_host(img, g, amvpt_mod.DenoiseParams(sigma_plane=sp))
    _assert_same(got, want)
    assert not np.array_equal(got, img)
    # fields as keywords, and a whole DenoiseParams
    q = amvpt_mod.DenoiseParams(iterations=5, sigma_color=0.5, sigma_plane=0.1, normal_squarings=2)
    _assert_same(amvpt_mod.denoise(s, image=img, iterations=5, sigma_color=0.5, sigma_plane=0.1, normal_squarings=2),
                 amvpt_mod.denoise_host(img, g, q))
    _assert_same(amvpt_mod.denoise(s, image=img, params=q), amvpt_mod.denoise_host(img, g, q))
    # views do not mix: filtering one view's tile alone gives that tile of the whole result
    tile = (slice(32, 64), slice(64, 96))
    _assert_same(amvpt_mod.denoise_host(img[tile], g[tile], q), amvpt_mod.denoise_host(img, g, q)[tile])


# ---- 3. refusals -----------------------------------------------------------------------------------------------------

def test_refusals(gpu_ready, amvpt_mod):
    torch = _torch()
    L = amvpt_mod.hip_lib()
    w, h, c = 6, 5, 3
    g = synthetic_guides(w, h, 3)
    img = random_image(g, c, 4, specials=False)
    d_img, d_g = torch.from_numpy(img).cuda(), torch.from_numpy(g).cuda()
    out = torch.full((img.size,), float(SENTINEL), dtype=torch.float32, device="cuda")
    scratch = torch.full((img.size,), float(SENTINEL), dtype=torch.float32, device="cuda")
    base = dict(image=d_img.data_ptr(), channels=c, width=w, height=h, guides=d_g.data_ptr(), params=amvpt_mod.DenoiseParams(),
                out=out.data_ptr(), scratch=scratch.data_ptr())
    for rid, change, names in refusal_rows(amvpt_mod, base, img.size):
        a = dict(base, **change)
        rc = L.amvpt_denoise(a["image"], a["channels"], a["width"], a["height"], a["guides"],
                             ctypes.byref(a["params"]) if a["params"] is not None else None, a["out"], a["scratch"], None)
        msg = L.amvpt_last_error().decode()
        assert rc == 1, (rid, rc)
        assert msg.startswith("amvpt_denoise: ") and names in msg, (rid, msg)
    torch.cuda.synchronize()
    assert (out == float(SENTINEL)).all() and (scratch == float(SENTINEL)).all(), "a refused call wrote"


# ---- 4. the host library's entry and the display stage ---------------------------------------------------------------

def test_host_entry(gpu_ready, amvpt_mod, rendered):
    """amvpt_host_denoise_stream filters the frame the render cached, with the guides of the cached device scene: the
    Python path's result, and no second scene."""
    import amvpt.display as D
    torch = _torch()
    _, _, g = rendered
    s = amvpt_mod.load_file(os.path.join(SCENES, "cbox_grid.xml"), res=32, spp=4, gx=4, gy=2)
    q = amvpt_mod.DenoiseParams(sigma_plane=amvpt_mod.denoise_sigma_plane(g))
    with pytest.raises(RuntimeError, match="no developed frame of this sensor is cached"):
        amvpt_mod.host_denoise(s, q)
    img = amvpt_mod.render(s)
    before = amvpt_mod.render_stats(s)
    assert (before["scene_creates"], before["renders"]) == (1, 1)
    want = amvpt_mod.denoise_host(img, g, q)
    _assert_same(amvpt_mod.host_denoise(s, q), want)
    stream = torch.cuda.Stream()
    _assert_same(amvpt_mod.host_denoise(s, q, stream=stream.cuda_stream), want)   # the cached frame is still the noisy one
    _assert_same(amvpt_mod.denoise(s, image=img), want)
    assert amvpt_mod.render_stats(s) == before, "the denoiser created a scene, a buffer or a render"
    # the display stage: the unfiltered frame's bytes, then the filtered frame's after denoise=
    size = (96, 54)
    plain = D.display(s, size=size, rerender=False)
    assert np.array_equal(plain, D.interlace(D.srgb8(img), D.preset_for_scene(s), size))
    shown = D.display(s, size=size, rerender=False, denoise=q)
    assert np.array_equal(shown, D.interlace(D.srgb8(want), D.preset_for_scene(s), size))
    assert not np.array_equal(shown, plain)
    assert np.array_equal(D.display(s, size=size, rerender=False), shown)   # the filtered frame is the cached one now
    after = amvpt_mod.render_stats(s)
    assert (after["scene_creates"], after["renders"]) == (1, 1)
    # denoise=True renders and filters with the scene's default parameters
    fresh = D.display(s, size=size, denoise=True)
    assert fresh.shape == (54, 96, 3) and amvpt_mod.render_stats(s)["renders"] == 2
    assert np.array_equal(fresh, D.display(s, size=size, rerender=False))
