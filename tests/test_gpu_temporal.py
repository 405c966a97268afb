"""Temporal accumulation on the device (include/amvpt_temporal.h) against its host entry, bit for bit.

amvpt_temporal_host is pinned to a numpy restatement of the definition by tests/test_temporal.py; here amvpt_temporal
must equal it on every float of the same cases and of sizes around the 32 x 8 block, with guard floats behind both
outputs and with the inputs compared before and after.  Then the projection pin (a hit point projected into the view it
was traced from lands in its own pixel, for the render's own guide records) and the layers above:
amvpt.TemporalAccumulator over real renders and the display stage.
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import SCENES
from test_gpu_bvh_walks import _torch
from test_guides import bits, xml_of
from test_temporal import (CASE_NAMES, SENTINEL, SHIFT, build_cases, call_with, moved, refusal_base, refusal_rows,
                           synthetic_case)

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 256   # floats behind both outputs that must stay as they were
SIZES = {"one_block_32x8": (32, 8), "block_plus_one_33x9": (33, 9), "two_blocks_less_one_63x15": (63, 15),
         "wide_257x3": (257, 3)}


@pytest.fixture(scope="module", autouse=True)
def _device_started(gpu_ready, amvpt_mod):
    """The process's one-time costs (torch, the HIP context, the code objects) are paid here when this module is the
    first to use the device."""
    torch = _torch()
    s, vd, p, planes = refusal_base(amvpt_mod)
    dev = [torch.from_numpy(planes[k]).cuda() for k in ("image", "guides", "hist_image", "hist_guides", "hist_count")]
    out, cnt = torch.zeros_like(dev[0]), torch.zeros_like(dev[4])
    amvpt_mod.temporal_device(dev[0].data_ptr(), 3, dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), dev[4].data_ptr(),
                              vd, p, out.data_ptr(), cnt.data_ptr())
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def cases(gpu_ready, oracle, amvpt_mod):
    all_ = build_cases(oracle, amvpt_mod)
    for i, (name, (w, h)) in enumerate(SIZES.items()):
        all_[name] = synthetic_case(amvpt_mod, w, h, 70 + i)
    return all_


def _device_temporal(amvpt_mod, k, img, hi, hc, tp, rect=None, cut=None):
    """amvpt_temporal on uploads of the planes (`cut`: the slices of `rect`) -> (image, count); asserts the guards and
    that the inputs are as uploaded."""
    torch = _torch()
    host = [np.ascontiguousarray(a[cut] if cut is not None else a) for a in (img, k.g, hi, k.hg, hc)]
    dev = [torch.from_numpy(a).cuda() for a in host]
    n, m = host[0].size, host[4].size
    out = torch.full((n + GUARD,), float(SENTINEL), dtype=torch.float32, device="cuda")
    cnt = torch.full((m + GUARD,), float(SENTINEL), dtype=torch.float32, device="cuda")
    amvpt_mod.temporal_device(dev[0].data_ptr(), host[0].shape[2], dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(),
                              dev[4].data_ptr(), k.prev_views, k.p, out.data_ptr(), cnt.data_ptr(), tp=tp, rect=rect)
    torch.cuda.synchronize()
    o, c = out.cpu().numpy(), cnt.cpu().numpy()
    assert (o[n:] == SENTINEL).all(), "the guard behind out_image was written"
    assert (c[m:] == SENTINEL).all(), "the guard behind out_count was written"
    for d, a in zip(dev, host):
        assert np.array_equal(bits(d.cpu().numpy()), bits(a)), "an input was modified on the device"
    return o[:n].reshape(host[0].shape), c[:m].reshape(host[4].shape)


def _assert_same(got, want, what=""):
    for a, b, plane in zip(got, want, ("image", "count")):
        same = bits(a) == bits(b)
        assert same.all(), "%s %s: %d of %d floats differ from the host entry, first at %s" % (
            what, plane, (~same).sum(), same.size, np.argwhere(~same)[:3].tolist())


# ---- 1. device against host, bit for bit ---------------------------------------------------------------------------

@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("name", CASE_NAMES + list(SIZES))
def test_device_equals_host(amvpt_mod, cases, name, channels):
    k = cases[name]
    img, hi, hc = k.planes(channels, 100 + channels)
    assert not np.isfinite(img).all() and not np.isfinite(hi).all()
    for tp in (amvpt_mod.TemporalParams(), amvpt_mod.TemporalParams(4, 0.005, 0.99), amvpt_mod.TemporalParams(65535, 0.3, -1.0)):
        want = amvpt_mod.temporal_host(img, k.g, hi, k.hg, hc, k.prev_views, k.p, tp)
        _assert_same(_device_temporal(amvpt_mod, k, img, hi, hc, tp), want, "%s %r" % (name, tp))
    assert (want[1] > 1).any() or min(img.shape[:2]) == 1


def test_view_tables_of_changing_size(amvpt_mod, cases):
    """The upload of the previous views is reused from call to call: tables of 1, 8, 4, 8, 1 and 8 views in turn, each with
    its own values, must each be the one its launch reads."""
    tp = amvpt_mod.TemporalParams()
    for name in ("synthetic_37x29", "cbox_moved", "batch_turned", "cone_reversed_moved", "one_block_32x8", "thinlens_moved"):
        k = cases[name]
        img, hi, hc = k.planes(3, 3, specials=False)
        _assert_same(_device_temporal(amvpt_mod, k, img, hi, hc, tp), amvpt_mod.temporal_host(img, k.g, hi, k.hg, hc, k.prev_views, k.p, tp), name)


def test_an_empty_history_gives_the_current_image(amvpt_mod, cases):
    k = cases["cbox_moved"]
    img, hi, _ = k.planes(4, 7, specials=False)
    out, cnt = _device_temporal(amvpt_mod, k, img, hi, np.zeros(k.g.shape[:2], dtype=F), amvpt_mod.TemporalParams())
    assert np.array_equal(bits(out), bits(img)) and (cnt == 1).all()


def test_a_rectangle_of_whole_tiles(amvpt_mod, cases):
    for name, rect in (("cbox_moved", (16, 16, 32, 16)), ("cone_reversed_moved", (48, 0, 16, 32)), ("batch_turned", (16, 0, 32, 32))):
        k = cases[name]
        img, hi, hc = k.planes(3, 9)
        whole = amvpt_mod.temporal_host(img, k.g, hi, k.hg, hc, k.prev_views, k.p)
        x0, y0, w, h = rect
        cut = (slice(y0, y0 + h), slice(x0, x0 + w))
        part = _device_temporal(amvpt_mod, k, img, hi, hc, amvpt_mod.TemporalParams(), rect=rect, cut=cut)
        _assert_same(part, (whole[0][cut], whole[1][cut]), name)


# ---- 2. refusals -----------------------------------------------------------------------------------------------------

def test_refusals(gpu_ready, amvpt_mod):
    torch = _torch()
    L = amvpt_mod.hip_lib()
    s, vd, p, planes = refusal_base(amvpt_mod)
    dev = {k: torch.from_numpy(v).cuda() for k, v in planes.items()}
    n_img = planes["image"].size
    out = torch.full((n_img,), float(SENTINEL), dtype=torch.float32, device="cuda")
    cnt = torch.full((128,), float(SENTINEL), dtype=torch.float32, device="cuda")
    base = dict({k: v.data_ptr() for k, v in dev.items()}, channels=3, prev_views=vd, params=p, rect=None,
                tp=amvpt_mod.TemporalParams(), out_image=out.data_ptr(), out_count=cnt.data_ptr())
    rows = refusal_rows(amvpt_mod, base, n_img, 128)
    assert len(rows) == 47
    for rid, change, status, names in rows:
        rc = call_with(L.amvpt_temporal, dict(base, **change), stream=True)
        msg = L.amvpt_last_error().decode()
        assert rc == status, (rid, rc, msg)
        assert msg.startswith("amvpt_temporal: ") and names in msg, (rid, msg)
    torch.cuda.synchronize()
    assert (out == float(SENTINEL)).all() and (cnt == float(SENTINEL)).all(), "a refused call wrote"
    assert call_with(L.amvpt_temporal, base, stream=True) == 0
    torch.cuda.synchronize()
    want = amvpt_mod.temporal_host(planes["image"], planes["guides"], planes["hist_image"], planes["hist_guides"],
                                   planes["hist_count"], vd, p)
    _assert_same((out.cpu().numpy().reshape(8, 16, 3), cnt.cpu().numpy().reshape(8, 16)), want)


# ---- 3. the projection pin -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("defines", [dict(), dict(cam="thinlens")], ids=["perspective", "thinlens"])
def test_a_hit_point_reprojects_into_its_own_pixel(gpu_ready, amvpt_mod, defines):
    """Previous views = current views, guide records from DeviceScene.guides: dtemporal.h's restatement of camera_uv
    against the render's own raygen.  The history image holds each pixel's coordinates (small integers, exact in the
    weighted mean), its count is 1 and the current image is 0, so out = h / 2 exactly with h the weighted mean of the
    accepted taps' coordinates, the reprojected position less the half pixel: floor(h + .5) is floor(fx), floor(fy)
    wherever the pixel's own tap carries the weight -- and it does: |h - (x, y)| stays below 0.05 pixel (the guide ray
    leaves the pixel centre; what remains is float rounding, about 1e-5)."""
    torch = _torch()
    s = amvpt_mod.load_file(os.path.join(SCENES, "cbox_grid.xml"), res=16, gx=4, gy=2, **defines)
    sd, vd, p = s.describe(0, 0, 0)
    w, h = p.film_width, p.film_height
    assert (w, h) == (64, 32) and vd[0].type == (1 if defines else 0)
    dev = amvpt_mod.DeviceScene(sd)
    g = torch.zeros((h, w, 8), dtype=torch.float32, device="cuda")
    dev.guides(vd, p, g.data_ptr())
    ys, xs = np.mgrid[0:h, 0:w]
    hi = torch.from_numpy(np.stack([xs, ys, np.ones_like(xs)], axis=-1).astype(F)).cuda()
    hc = torch.ones((h, w), dtype=torch.float32, device="cuda")
    img, out, cnt = torch.zeros_like(hi), torch.zeros_like(hi), torch.zeros_like(hc)
    amvpt_mod.temporal_device(img.data_ptr(), 3, g.data_ptr(), hi.data_ptr(), g.data_ptr(), hc.data_ptr(), vd, p,
                              out.data_ptr(), cnt.data_ptr())
    torch.cuda.synchronize()
    rec, o, c = g.cpu().numpy(), out.cpu().numpy(), cnt.cpu().numpy()
    hit = rec[..., 0] >= 0
    assert hit.mean() > 0.8
    assert (c[hit] == 2).all() and (o[hit][:, 2] == 0.5).all(), "a hit pixel found no history in its own view"
    hx, hy = 2 * o[..., 0], 2 * o[..., 1]
    off = max(np.abs(hx - xs)[hit].max(), np.abs(hy - ys)[hit].max())
    print("projection pin (%s): the reprojected position is within %.2e pixel of the pixel centre" % (
        "thinlens" if defines else "perspective", off))
    assert (np.floor(hx + F(.5)) == xs)[hit].all() and (np.floor(hy + F(.5)) == ys)[hit].all()
    assert off < 0.05
    assert (c[~hit] == 2).all()   # a miss takes the same pixel of the same view


# ---- 4. end to end ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def three_frames(gpu_ready, amvpt_mod):
    """cbox_grid.xml as 4 x 2 views of 16 x 16: three 1-spp frames with the camera moved between them, each rendered and
    developed on the device and pushed through one TemporalAccumulator -> per frame (image, guides, accumulated image,
    count) downloaded, with the views and parameters."""
    torch = _torch()
    L = amvpt_mod.hip_lib()
    box = xml_of("cbox_grid.xml")
    acc = amvpt_mod.TemporalAccumulator()
    dev, frames = None, []
    for i in range(3):
        xml = moved(box, SHIFT[0] * i, SHIFT[1] * i) if i else box
        s = amvpt_mod.load_string(xml, res=16, gx=4, gy=2, spp=1)
        sd, vd, p = s.describe(0, 10 + i, 1)
        dev = dev or amvpt_mod.DeviceScene(sd)   # the scene is static: only the views change
        w, h = p.film_width, p.film_height
        film = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
        img = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        dev.render(vd, p, film.data_ptr())
        assert L.amvpt_develop(ctypes.c_void_p(film.data_ptr()), ctypes.c_void_p(img.data_ptr()), w, h, p.film_alpha, None) == 0
        out = acc.push(dev, vd, p, img)
        torch.cuda.synchronize()
        frames.append(dict(image=img.cpu().numpy(), guides=acc.guides.cpu().numpy(), out=out.cpu().numpy(),
                           count=acc.count.cpu().numpy(), views=vd, params=p, scene=s))
    return acc, dev, frames


def test_accumulator_equals_the_host_entry(amvpt_mod, three_frames):
    acc, _, frames = three_frames
    assert acc.frames == 3 and frames[0]["image"].shape == (32, 64, 3)
    hi, hg, hc = np.zeros_like(frames[0]["image"]), np.zeros_like(frames[0]["guides"]), np.zeros((32, 64), dtype=F)
    prev = frames[0]["views"]
    for i, f in enumerate(frames):
        assert np.isfinite(f["image"]).all() and f["image"].max() > 0
        want = amvpt_mod.temporal_host(f["image"], f["guides"], hi, hg, hc, prev, f["params"])
        _assert_same((f["out"], f["count"]), want, "frame %d" % i)
        hi, hc, hg, prev = want[0], want[1], f["guides"], f["views"]
    assert np.array_equal(frames[0]["out"], frames[0]["image"]) and (frames[0]["count"] == 1).all()
    assert frames[2]["count"].max() == 3 and 0.2 < (frames[2]["count"] > 1).mean() < 1
    assert not np.array_equal(frames[2]["out"], frames[2]["image"])
    # views do not mix: one tile's rectangle, processed alone on the device, is that tile of the whole-quilt result
    f, g1 = frames[2], frames[1]

    class K:
        g, hg, p, prev_views = f["guides"], g1["guides"], f["params"], g1["views"]
    rect = (32, 16, 16, 16)
    cut = (slice(16, 32), slice(32, 48))
    part = _device_temporal(amvpt_mod, K, f["image"], g1["out"], g1["count"], amvpt_mod.TemporalParams(), rect=rect, cut=cut)
    _assert_same(part, (f["out"][cut], f["count"][cut]), "tile")
    acc2 = amvpt_mod.TemporalAccumulator(amvpt_mod.TemporalParams(max_history=2))
    assert acc2.params.max_history == 2 and acc2.image is None


def test_accumulator_resets(amvpt_mod, three_frames):
    torch = _torch()
    acc, dev, frames = three_frames
    f = frames[2]
    a = amvpt_mod.TemporalAccumulator()
    img = torch.from_numpy(f["image"]).cuda()
    first = a.push(dev, f["views"], f["params"], img).cpu().numpy()
    second = a.push(dev, f["views"], f["params"], img.data_ptr())   # a device pointer: 3 channels without film_alpha
    torch.cuda.synchronize()
    assert np.array_equal(first, f["image"]) and a.count.max() == 2
    # the same frame pushed twice on a static camera: the taps beside the pixel itself weigh a rounding of its position
    # (below 2^-15 of a pixel at coordinates below 64), so no value moves by more than that share of the largest one
    assert (np.abs(second.cpu().numpy() - f["image"]) <= 1e-4 * f["image"].max()).all()
    a.reset()
    assert a.frames == 0 and a.image is None
    again = a.push(dev, f["views"], f["params"], img)
    torch.cuda.synchronize()
    assert np.array_equal(again.cpu().numpy(), f["image"]) and (a.count == 1).all()
    # another channel count starts over
    img4 = torch.cat([img, torch.ones_like(img[..., :1])], dim=-1).contiguous()
    out4 = a.push(dev, f["views"], f["params"], img4)
    torch.cuda.synchronize()
    assert out4.shape == (32, 64, 4) and (a.count == 1).all() and np.array_equal(out4.cpu().numpy(), img4.cpu().numpy())
    a.push(dev, f["views"], f["params"], img4)
    torch.cuda.synchronize()
    assert a.count.max() == 2
    # another film size starts over, and so does another number of views on the same film size
    gen = torch.Generator(device="cuda").manual_seed(3)
    small = torch.rand((16, 32, 4), dtype=torch.float32, device="cuda", generator=gen) + 0.01
    for defines, n_views in ((dict(res=8, gx=4, gy=2), 8), (dict(res=16, gx=2, gy=1), 2)):
        s = amvpt_mod.load_file(os.path.join(SCENES, "cbox_grid.xml"), spp=1, **defines)
        _, vd, p = s.describe(0, 0, 1)
        assert (p.film_width, p.film_height, p.n_views) == (32, 16, n_views)
        first = a.push(dev, vd, p, small)
        torch.cuda.synchronize()
        assert a.frames == 1 and (a.count == 1).all() and torch.equal(first, small)
        a.push(dev, vd, p, small)
        torch.cuda.synchronize()
        assert a.frames == 2 and a.count.max() == 2


def test_display_stage(amvpt_mod, three_frames):
    """temporal=None returns the bytes the call returned before; an accumulator shows the accumulated frame."""
    import amvpt.display as D
    s = amvpt_mod.load_file(os.path.join(SCENES, "cbox_grid.xml"), res=16, gx=4, gy=2, spp=1)
    size = (96, 54)
    D.display(s, size=size)
    plain = D.display(s, size=size, rerender=False)
    assert np.array_equal(plain, D.display(s, size=size, rerender=False, temporal=None))
    acc = amvpt_mod.TemporalAccumulator()
    shown = None
    for seed in (1, 2, 3):
        shown = D.display(s, size=size, seed=seed, temporal=acc)
    assert acc.frames == 3 and (acc.count.cpu().numpy()[acc.guides.cpu().numpy()[..., 0] >= 0] == 3).all()
    want = D.interlace(D.srgb8(acc.image.cpu().numpy()), D.preset_for_scene(s), size)
    assert shown.shape == (54, 96, 3) and np.array_equal(shown, want)
    q = amvpt_mod.DenoiseParams(iterations=2)
    filtered = D.display(s, size=size, seed=4, temporal=acc, denoise=q)
    want = D.interlace(D.srgb8(amvpt_mod.denoise_host(acc.image.cpu().numpy(), acc.guides.cpu().numpy(), q)), D.preset_for_scene(s), size)
    assert np.array_equal(filtered, want) and acc.frames == 4
    with pytest.raises(ValueError, match="needs a fresh frame"):
        D.display(s, size=size, temporal=acc, rerender=False)
