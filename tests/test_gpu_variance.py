"""The variance-guided denoiser on the device (include/amvpt_variance.h) against its host entries, bit for bit.

The three host entries are pinned to numpy restatements of the definition by tests/test_variance.py; here
amvpt_temporal_moments, amvpt_variance and amvpt_denoise_variance must equal them on every float of the same cases and
of sizes around the 32 x 8 block, at iterations 1 to 5 (the LDS tile kernels of steps 1 and 2 and the plain one from
step 4; step 16 leaves the 16 x 16 tiles of the 64 x 32 quilts), with values that are not finite in every plane, with
guard floats behind every output and with the inputs compared before and after.  Then the layers above:
amvpt.TemporalAccumulator(moments=True) over real renders and the display stage.
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import SCENES
from test_gpu_bvh_walks import _torch
from test_guides import bits, xml_of
from test_temporal import CASE_NAMES, SENTINEL, SHIFT, build_cases, moved, refusal_base, refusal_rows, synthetic_case
from test_variance import (call_filter, call_moments, call_variance, filter_refusal_rows, history_moments, moments_refusal_rows,
                           refusal_planes, ringed_variance, seeded_stage2, stage_inputs, variance_refusal_rows)

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 256   # floats behind every output that must stay as they were
SIZES = {"one_block_32x8": (32, 8), "block_plus_one_33x9": (33, 9), "two_blocks_less_one_63x15": (63, 15),
         "wide_257x3": (257, 3)}


@pytest.fixture(scope="module", autouse=True)
def _device_started(gpu_ready, amvpt_mod):
    """The process's one-time costs (torch, the HIP context, the code objects) are paid here when this module is the
    first to use the device."""
    torch = _torch()
    pl = refusal_planes()
    dev = {k: torch.from_numpy(np.ascontiguousarray(pl[k])).cuda() for k in ("moments", "count", "guides")}
    out = torch.zeros((pl["h"], pl["w"]), dtype=torch.float32, device="cuda")
    amvpt_mod.variance_device(dev["moments"].data_ptr(), dev["count"].data_ptr(), dev["guides"].data_ptr(), pl["w"], pl["h"], out.data_ptr())
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def cases(gpu_ready, oracle, amvpt_mod):
    all_ = build_cases(oracle, amvpt_mod)
    for i, (name, (w, h)) in enumerate(SIZES.items()):
        all_[name] = synthetic_case(amvpt_mod, w, h, 70 + i)
    return all_


def _run(host_inputs, out_sizes, launch):
    """Uploads the inputs, hands `launch` their tensors and guarded output tensors, and returns the outputs; asserts the
    guards and that the inputs are as uploaded.  An output size of None is a buffer the call does without."""
    torch = _torch()
    host = [np.ascontiguousarray(a) for a in host_inputs]
    dev = [torch.from_numpy(a).cuda() for a in host]
    outs = [torch.full((n + GUARD,), float(SENTINEL), dtype=torch.float32, device="cuda") if n is not None else None for n in out_sizes]
    launch(dev, outs)
    torch.cuda.synchronize()
    res = []
    for o, n in zip(outs, out_sizes):
        if o is None:
            res.append(None)
            continue
        a = o.cpu().numpy()
        assert (a[n:] == SENTINEL).all(), "the guard behind an output was written"
        res.append(a[:n])
    for d, a in zip(dev, host):
        assert np.array_equal(bits(d.cpu().numpy()), bits(a)), "an input was modified on the device"
    return res


def _device_moments(amvpt_mod, k, img, hi, hc, hm, tp, rect=None, cut=None):
    ins = [a[cut] if cut is not None else a for a in (img, k.g, hi, k.hg, hc, hm)]
    h, w, c = ins[0].shape

    def launch(d, o):
        amvpt_mod.temporal_moments_device(d[0].data_ptr(), c, d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(),
                                          d[5].data_ptr(), k.prev_views, k.p, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(),
                                          tp=tp, rect=rect)
    o = _run(ins, (h * w * c, h * w, 2 * h * w), launch)
    return o[0].reshape(h, w, c), o[1].reshape(h, w), o[2].reshape(h, w, 2)


def _device_temporal(amvpt_mod, k, img, hi, hc, tp):
    h, w, c = img.shape

    def launch(d, o):
        amvpt_mod.temporal_device(d[0].data_ptr(), c, d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(),
                                  k.prev_views, k.p, o[0].data_ptr(), o[1].data_ptr(), tp=tp)
    o = _run((img, k.g, hi, k.hg, hc), (h * w * c, h * w), launch)
    return o[0].reshape(h, w, c), o[1].reshape(h, w)


def _device_variance(amvpt_mod, mom, cnt, g, q):
    h, w = cnt.shape

    def launch(d, o):
        amvpt_mod.variance_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), w, h, o[0].data_ptr(), params=q)
    return _run((mom, cnt, g), (h * w,), launch)[0].reshape(h, w)


def _device_filter(amvpt_mod, img, var, g, q, scratch=True, var_out=True):
    h, w, c = img.shape

    def launch(d, o):
        ptr = [t.data_ptr() if t is not None else None for t in o]
        amvpt_mod.denoise_variance_device(d[0].data_ptr(), c, w, h, d[1].data_ptr(), d[2].data_ptr(), ptr[0], ptr[1], ptr[2], ptr[3],
                                          params=q)
    o = _run((img, var, g), (h * w * c, h * w * c if scratch else None, h * w if var_out else None, h * w if scratch else None), launch)
    return o[0].reshape(h, w, c), (o[2].reshape(h, w) if var_out else None)


def _assert_same(got, want, what=""):
    for i, (a, b) in enumerate(zip(got, want)):
        same = bits(a) == bits(b)
        assert same.all(), "%s output %d: %d of %d floats differ from the host entry, first at %s" % (
            what, i, (~same).sum(), same.size, np.argwhere(~same)[:3].tolist())


# ---- 1. device against host, bit for bit ---------------------------------------------------------------------------

@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("name", CASE_NAMES + list(SIZES))
def test_device_equals_host(amvpt_mod, cases, name, channels):
    k = cases[name]
    img, hi, hc = k.planes(channels, 100 + channels)
    hm = history_moments(k, 107)
    assert not np.isfinite(img).all() and not np.isfinite(hi).all() and not np.isfinite(hm).all()
    for tp in (amvpt_mod.TemporalParams(), amvpt_mod.TemporalParams(4, 0.005, 0.99)):
        want = amvpt_mod.temporal_moments_host(img, k.g, hi, k.hg, hc, hm, k.prev_views, k.p, tp)
        got = _device_moments(amvpt_mod, k, img, hi, hc, hm, tp)
        _assert_same(got, want, "%s stage 1 %r" % (name, tp))
    # the moments entry and amvpt_temporal give the same image and count on the device
    _assert_same(_device_temporal(amvpt_mod, k, img, hi, hc, tp), got[:2], name + " amvpt_temporal")
    s = stage_inputs(amvpt_mod, k, channels)
    for mh in (1, 4, 9):
        q = amvpt_mod.VarianceParams(min_history=mh)
        want_v = amvpt_mod.variance_host(s["mom"], s["cnt"], k.g, q)
        _assert_same([_device_variance(amvpt_mod, s["mom"], s["cnt"], k.g, q)], [want_v], "%s stage 2 min_history %d" % (name, mh))
    # a count and moments stage 1 never writes: NaN, infinities, 0 and 0.5, beside short histories too
    mom2, cnt2 = seeded_stage2(k, s)
    assert np.isnan(cnt2).any() and np.isinf(cnt2).any() and not np.isfinite(mom2).all()
    for mh in (1, 4, 9):
        q = amvpt_mod.VarianceParams(min_history=mh)
        got_v = _device_variance(amvpt_mod, mom2, cnt2, k.g, q)
        _assert_same([got_v], [amvpt_mod.variance_host(mom2, cnt2, k.g, q)], "%s stage 2, seeded count, min_history %d" % (name, mh))
        assert np.isfinite(got_v).all() and (got_v >= 0).all()
    var = ringed_variance(amvpt_mod.variance_host(s["mom"], s["cnt"], k.g), k.g)
    assert not np.isfinite(var).all() and not np.isfinite(s["out"]).all()
    for it in range(1, 6):
        q = amvpt_mod.VarianceParams(iterations=it)
        want_f = amvpt_mod.denoise_variance_host(s["out"], var, k.g, q)
        _assert_same(_device_filter(amvpt_mod, s["out"], var, k.g, q), want_f, "%s stage 3, %d iterations" % (name, it))
    assert not np.array_equal(want_f[0][..., :3], s["out"][..., :3])


def test_buffers_that_may_be_absent(amvpt_mod, cases):
    k = cases["block_plus_one_33x9"]
    s = stage_inputs(amvpt_mod, k, 3)
    var = amvpt_mod.variance_host(s["mom"], s["cnt"], k.g)
    for it, kw in ((1, dict(scratch=False, var_out=False)), (1, dict(scratch=False)), (2, dict(var_out=False))):
        q = amvpt_mod.VarianceParams(iterations=it)
        got = _device_filter(amvpt_mod, s["out"], var, k.g, q, **kw)
        want = amvpt_mod.denoise_variance_host(s["out"], var, k.g, q)
        _assert_same(got[:1] if got[1] is None else got, want, "iterations %d %r" % (it, kw))


def test_view_tables_of_changing_size(amvpt_mod, cases):
    """The upload of the previous views is shared with amvpt_temporal and reused from call to call: tables of 1, 8, 4, 8
    and 1 views in turn through the moments entry, each with its own values, must each be the one its launch reads."""
    tp = amvpt_mod.TemporalParams()
    for name in ("synthetic_37x29", "cbox_moved", "batch_turned", "cone_reversed_moved", "one_block_32x8"):
        k = cases[name]
        img, hi, hc = k.planes(3, 3, specials=False)
        hm = history_moments(k, 4, specials=False)
        want = amvpt_mod.temporal_moments_host(img, k.g, hi, k.hg, hc, hm, k.prev_views, k.p, tp)
        _assert_same(_device_moments(amvpt_mod, k, img, hi, hc, hm, tp), want, name)


def test_a_rectangle_of_whole_tiles(amvpt_mod, cases):
    for name, rect in (("cbox_moved", (16, 16, 32, 16)), ("batch_turned", (16, 0, 32, 32))):
        k = cases[name]
        s = stage_inputs(amvpt_mod, k, 3, seed=9)
        x0, y0, w, h = rect
        cut = (slice(y0, y0 + h), slice(x0, x0 + w))
        part = _device_moments(amvpt_mod, k, s["img"], s["hi"], s["hc"], s["hm"], amvpt_mod.TemporalParams(), rect=rect, cut=cut)
        _assert_same(part, (s["out"][cut], s["cnt"][cut], s["mom"][cut]), name)


# ---- 2. refusals -----------------------------------------------------------------------------------------------------

def test_refusals_of_the_temporal_stage(gpu_ready, amvpt_mod):
    torch = _torch()
    L = amvpt_mod.hip_lib()
    s, vd, p, planes = refusal_base(amvpt_mod)
    planes["hist_moments"] = np.ones((8, 16, 2), dtype=F)
    dev = {k: torch.from_numpy(v).cuda() for k, v in planes.items()}
    n_img = planes["image"].size
    outs = [torch.full((n,), float(SENTINEL), dtype=torch.float32, device="cuda") for n in (n_img, 128, 256)]
    base = dict({k: v.data_ptr() for k, v in dev.items()}, channels=3, prev_views=vd, params=p, rect=None,
                tp=amvpt_mod.TemporalParams(), out_image=outs[0].data_ptr(), out_count=outs[1].data_ptr(), out_moments=outs[2].data_ptr())
    rows = refusal_rows(amvpt_mod, base, n_img, 128) + moments_refusal_rows(amvpt_mod, base, n_img, 128)
    assert len(rows) == 47 + 12
    for rid, change, status, names in rows:
        rc = call_moments(L.amvpt_temporal_moments, dict(base, **change), stream=True)
        msg = L.amvpt_last_error().decode()
        assert rc == status, (rid, rc, msg)
        assert msg.startswith("amvpt_temporal_moments: ") and names in msg, (rid, msg)
    torch.cuda.synchronize()
    assert all((o == float(SENTINEL)).all() for o in outs), "a refused call wrote"
    assert call_moments(L.amvpt_temporal_moments, base, stream=True) == 0
    torch.cuda.synchronize()
    want = amvpt_mod.temporal_moments_host(planes["image"], planes["guides"], planes["hist_image"], planes["hist_guides"],
                                           planes["hist_count"], planes["hist_moments"], vd, p)
    _assert_same((outs[0].cpu().numpy().reshape(8, 16, 3), outs[1].cpu().numpy().reshape(8, 16), outs[2].cpu().numpy().reshape(8, 16, 2)), want)


def test_refusals_of_the_variance_and_the_filter(gpu_ready, amvpt_mod):
    """The rows of the host entries' test over device pointers: the planes lie in one device buffer as they do in the
    host one, so every row's overlap is the only one."""
    torch = _torch()
    L = amvpt_mod.hip_lib()
    pl = refusal_planes()
    w, h, n_px, n_img = pl["w"], pl["h"], pl["w"] * pl["h"], pl["image"].size
    arena = torch.from_numpy(pl["arena"]).cuda()
    at = {k: arena.data_ptr() + (pl[k].ctypes.data - pl["arena"].ctypes.data) for k in pl if k not in ("w", "h", "arena")}
    base = dict(moments=at["moments"], count=at["count"], guides=at["guides"], width=w, height=h, params=amvpt_mod.VarianceParams(),
                out=at["variance_out"])
    for rid, change, names in variance_refusal_rows(amvpt_mod, base, n_px):
        rc = call_variance(L.amvpt_variance, dict(base, **change), stream=True)
        msg = L.amvpt_last_error().decode()
        assert rc == 1 and msg.startswith("amvpt_variance: ") and names in msg, (rid, rc, msg)
    base3 = dict({k: at[k] for k in ("out", "scratch", "var_out", "var_scratch", "image", "variance", "guides")}, channels=3, width=w,
                 height=h, params=amvpt_mod.VarianceParams())
    for rid, change, names in filter_refusal_rows(amvpt_mod, base3, n_img, n_px):
        rc = call_filter(L.amvpt_denoise_variance, dict(base3, **change), stream=True)
        msg = L.amvpt_last_error().decode()
        assert rc == 1 and msg.startswith("amvpt_denoise_variance: ") and names in msg, (rid, rc, msg)
    torch.cuda.synchronize()
    assert np.array_equal(bits(arena.cpu().numpy()), bits(pl["arena"])), "a refused call wrote"
    assert call_variance(L.amvpt_variance, base, stream=True) == 0 and call_filter(L.amvpt_denoise_variance, base3, stream=True) == 0
    torch.cuda.synchronize()
    after = arena.cpu().numpy()
    off = lambda k: (pl[k].ctypes.data - pl["arena"].ctypes.data) // 4   # noqa: E731
    want_v = amvpt_mod.variance_host(pl["moments"], pl["count"], pl["guides"])
    want_f = amvpt_mod.denoise_variance_host(pl["image"], pl["variance"], pl["guides"])
    assert np.array_equal(bits(after[off("variance_out"):off("variance_out") + n_px]), bits(want_v.ravel()))
    assert np.array_equal(bits(after[off("out"):off("out") + n_img]), bits(want_f[0].ravel()))
    assert np.array_equal(bits(after[off("var_out"):off("var_out") + n_px]), bits(want_f[1].ravel()))


# ---- 3. end to end ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def three_frames(gpu_ready, amvpt_mod):
    """cbox_grid.xml as 4 x 2 views of 16 x 16: three 1-spp frames with the camera moved between them, each rendered and
    developed on the device and pushed through one TemporalAccumulator(moments=True) -> per frame the downloaded
    planes, with the views and parameters."""
    torch = _torch()
    L = amvpt_mod.hip_lib()
    box = xml_of("cbox_grid.xml")
    acc = amvpt_mod.TemporalAccumulator(moments=True)
    dev, frames = None, []
    for i in range(3):
        xml = moved(box, SHIFT[0] * i, SHIFT[1] * i) if i else box
        s = amvpt_mod.load_string(xml, res=16, gx=4, gy=2, spp=1)
        sd, vd, p = s.describe(0, 10 + i, 1)
        dev = dev or amvpt_mod.DeviceScene(sd)
        w, h = p.film_width, p.film_height
        film = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
        img = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        dev.render(vd, p, film.data_ptr())
        assert L.amvpt_develop(ctypes.c_void_p(film.data_ptr()), ctypes.c_void_p(img.data_ptr()), w, h, p.film_alpha, None) == 0
        out = acc.push(dev, vd, p, img)
        torch.cuda.synchronize()
        frames.append(dict(image=img.cpu().numpy(), guides=acc.guides.cpu().numpy(), out=out.cpu().numpy(),
                           count=acc.count.cpu().numpy(), moments=acc.moments.cpu().numpy(), views=vd, params=p, scene=s))
    return acc, dev, frames


def test_accumulator_equals_the_host_entries(amvpt_mod, three_frames):
    torch = _torch()
    acc, _, frames = three_frames
    assert acc.frames == 3 and acc.with_moments and frames[0]["image"].shape == (32, 64, 3)
    hi, hg, hc = np.zeros_like(frames[0]["image"]), np.zeros_like(frames[0]["guides"]), np.zeros((32, 64), dtype=F)
    hm = np.zeros((32, 64, 2), dtype=F)
    prev = frames[0]["views"]
    for i, f in enumerate(frames):
        want = amvpt_mod.temporal_moments_host(f["image"], f["guides"], hi, hg, hc, hm, prev, f["params"])
        _assert_same((f["out"], f["count"], f["moments"]), want, "frame %d" % i)
        hi, hc, hm, hg, prev = want[0], want[1], want[2], f["guides"], f["views"]
    assert frames[2]["count"].max() == 3 and 0.2 < (frames[2]["count"] > 1).mean() < 1 and (frames[2]["count"] < 3).any()
    q = amvpt_mod.VarianceParams(min_history=3)
    var = acc.variance(q)
    out, vout = acc.denoise(q)
    torch.cuda.synchronize()
    f = frames[2]
    want_v = amvpt_mod.variance_host(f["moments"], f["count"], f["guides"], q)
    want_f = amvpt_mod.denoise_variance_host(f["out"], want_v, f["guides"], q)
    _assert_same((var.cpu().numpy(), out.cpu().numpy(), vout.cpu().numpy()), (want_v, want_f[0], want_f[1]), "accumulator")
    assert want_v.max() > 0 and not np.array_equal(want_f[0], f["out"])
    assert np.array_equal(bits(acc.image.cpu().numpy()), bits(f["out"])), "denoise touched the history"
    # the plain accumulator over the same frames keeps the same image and count
    plain = amvpt_mod.TemporalAccumulator()
    dev = three_frames[1]
    for fr in frames:
        plain.push(dev, fr["views"], fr["params"], torch.from_numpy(fr["image"]).cuda())
    torch.cuda.synchronize()
    assert plain.moments is None
    _assert_same((plain.image.cpu().numpy(), plain.count.cpu().numpy()), (f["out"], f["count"]), "moments=False")


def test_display_stage(amvpt_mod, three_frames):
    """display(..., temporal=acc, denoise=VarianceParams) shows the host pipeline's bytes; the defaults are untouched."""
    import amvpt.display as D
    s = amvpt_mod.load_file(os.path.join(SCENES, "cbox_grid.xml"), res=16, gx=4, gy=2, spp=1)
    size = (96, 54)
    acc = amvpt_mod.TemporalAccumulator(moments=True)
    q = amvpt_mod.VarianceParams(iterations=3)
    shown = None
    for seed in (1, 2, 3):
        shown = D.display(s, size=size, seed=seed, temporal=acc, denoise=q)
    assert acc.frames == 3 and shown.shape == (54, 96, 3)
    g = acc.guides.cpu().numpy()
    var = amvpt_mod.variance_host(acc.moments.cpu().numpy(), acc.count.cpu().numpy(), g, q)
    filtered = amvpt_mod.denoise_variance_host(acc.image.cpu().numpy(), var, g, q)[0]
    assert np.array_equal(shown, D.interlace(D.srgb8(filtered), D.preset_for_scene(s), size))
    assert not np.array_equal(shown, D.interlace(D.srgb8(acc.image.cpu().numpy()), D.preset_for_scene(s), size))
    # the accumulator without the new object shows the accumulated frame, as before
    plain = D.display(s, size=size, seed=4, temporal=acc)
    assert np.array_equal(plain, D.interlace(D.srgb8(acc.image.cpu().numpy()), D.preset_for_scene(s), size))
    with pytest.raises(ValueError, match="moments=True"):
        D.display(s, size=size, temporal=amvpt_mod.TemporalAccumulator(), denoise=q)
