"""View synthesis on the device (include/amvpt_synth.h) against its host entries, bit for bit.

amvpt_synth_host and amvpt_synth_fill_host are pinned to a numpy restatement of the definition by tests/test_synth.py;
here amvpt_synth and amvpt_synth_fill must equal them on every float of the same cases and of target sizes around the
32 x 8 block, with guard floats behind every output and with the inputs compared before and after.  Then the layers
above: amvpt.ViewSynthesizer over a real render and the display stage.
"""
import ctypes

import numpy as np
import pytest

from test_gpu_bvh_walks import _torch
from test_guides import bits, xml_of
from test_synth import (CASE_NAMES, N_ROWS, SENTINEL, Arena, build_cases, call_fill, call_with, check_rows, fill_planes,
                        fill_refusal_rows, from_temporal, param_sets, refusal_planes, refusal_rows)
from test_temporal import synthetic_case

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 256   # floats behind every output that must stay as they were
SIZES = {"one_block_32x8": (32, 8), "block_plus_one_33x9": (33, 9), "two_blocks_less_one_63x15": (63, 15),
         "wide_257x3": (257, 3)}


@pytest.fixture(scope="module")
def cases(gpu_ready, oracle, amvpt_mod):
    all_ = build_cases(oracle, amvpt_mod)
    for i, (name, (w, h)) in enumerate(SIZES.items()):
        all_[name] = from_temporal(synthetic_case(amvpt_mod, w, h, 70 + i))
        all_[name].name = name
    return all_


def _guarded(torch, n):
    return torch.full((n + GUARD,), float(SENTINEL), dtype=torch.float32, device="cuda")


def _device_synth(amvpt_mod, k, img, q, rect=None, cut=None):
    """amvpt_synth and amvpt_synth_fill on uploads of the planes (`cut`: the slices of `rect` of the target records)
    -> ((image, cover) of stage 1, (image, cover) after the fill); asserts the guards and that the inputs are as
    uploaded."""
    torch = _torch()
    dg = np.ascontiguousarray(k.dg[cut] if cut is not None else k.dg)
    host = [np.ascontiguousarray(img), k.sg, dg]
    dev = [torch.from_numpy(a).cuda() for a in host]
    h, w = dg.shape[:2]
    c = img.shape[2]
    n, m = h * w * c, h * w
    out, cov = _guarded(torch, n), _guarded(torch, m)
    amvpt_mod.synth_device(dev[0].data_ptr(), c, dev[1].data_ptr(), k.sv, k.sp, dev[2].data_ptr(), k.dv, k.dp, out.data_ptr(),
                           cov.data_ptr(), sp=q, rect=rect)
    fout, fscr, fcov, fcscr = _guarded(torch, n), _guarded(torch, n), _guarded(torch, m), _guarded(torch, m)
    before = (out.clone(), cov.clone())
    amvpt_mod.synth_fill_device(out.data_ptr(), c, w, h, cov.data_ptr(), dev[2].data_ptr(), fout.data_ptr(), fcov.data_ptr(),
                                fscr.data_ptr(), fcscr.data_ptr(), sp=q)
    torch.cuda.synchronize()
    for t, size in ((out, n), (cov, m), (fout, n), (fscr, n), (fcov, m), (fcscr, m)):
        assert (t[size:] == float(SENTINEL)).all(), "a guard behind an output was written"
    for d, a in zip(dev, host):
        assert np.array_equal(bits(d.cpu().numpy()), bits(a)), "an input was modified on the device"
    assert torch.equal(out.view(torch.int32), before[0].view(torch.int32)) and torch.equal(cov.view(torch.int32), before[1].view(torch.int32))
    one = (out.cpu().numpy()[:n].reshape(h, w, c), cov.cpu().numpy()[:m].reshape(h, w))
    return one, (fout.cpu().numpy()[:n].reshape(h, w, c), fcov.cpu().numpy()[:m].reshape(h, w))


def _assert_same(got, want, what=""):
    for a, b, plane in zip(got, want, ("image", "cover")):
        same = bits(a) == bits(b)
        assert same.all(), "%s %s: %d of %d floats differ from the host entry, first at %s" % (
            what, plane, (~same).sum(), same.size, np.argwhere(~same)[:3].tolist())


def _host(amvpt_mod, k, img, q, rect=None, cut=None):
    dg = k.dg[cut] if cut is not None else k.dg
    one = amvpt_mod.synth_host(img, k.sg, k.sv, k.sp, dg, k.dv, k.dp, q, rect=rect)
    return one, amvpt_mod.synth_fill_host(one[0], one[1], dg, q)


# ---- 1. device against host, bit for bit ---------------------------------------------------------------------------

@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("name", CASE_NAMES + list(SIZES))
def test_device_equals_host(amvpt_mod, cases, name, channels):
    k = cases[name]
    img = k.image(channels, 100 + channels)
    assert not np.isfinite(img).all()
    for q in param_sets(amvpt_mod):
        want = _host(amvpt_mod, k, img, q)
        got = _device_synth(amvpt_mod, k, img, q)
        _assert_same(got[0], want[0], "%s stage 1 %r" % (name, q))
        _assert_same(got[1], want[1], "%s fill %r" % (name, q))
    assert (want[0][1] > 0).any()


def test_view_tables_of_changing_size(amvpt_mod, cases):
    """The upload of the view tables is reused from call to call: source tables of 1, 8, 4, 8 and 1 views in turn (and
    target tables of 1, 15, 4, 15 and 1), each with its own values, must each be the one its launch reads."""
    q = amvpt_mod.SynthParams()
    for name in ("synthetic_37x29", "cbox", "batch", "cone_reversed", "one_block_32x8"):
        k = cases[name]
        img = k.image(3, 3, specials=False)
        got, want = _device_synth(amvpt_mod, k, img, q), _host(amvpt_mod, k, img, q)
        _assert_same(got[0], want[0], name)
        _assert_same(got[1], want[1], name + " fill")


def test_a_rectangle_of_whole_tiles(amvpt_mod, cases):
    for name, rect in (("cbox", (16, 16, 48, 32)), ("cbox_tiles_12x8", (24, 8, 12, 16)), ("cone_reversed", (64, 0, 16, 48)),
                       ("batch", (12, 0, 24, 8))):
        k = cases[name]
        img = k.image(3, 9)
        x0, y0, w, h = rect
        cut = (slice(y0, y0 + h), slice(x0, x0 + w))
        whole = amvpt_mod.synth_host(img, k.sg, k.sv, k.sp, k.dg, k.dv, k.dp)
        part, _ = _device_synth(amvpt_mod, k, img, amvpt_mod.SynthParams(), rect=rect, cut=cut)
        _assert_same(part, (whole[0][cut], whole[1][cut]), name)


# ---- 2. refusals -----------------------------------------------------------------------------------------------------

def test_refusals(gpu_ready, amvpt_mod):
    """Every plane lives in one device buffer with gaps between them (test_synth.Arena): a refused call leaves all of it
    as it was, and a good call afterwards is correct."""
    torch = _torch()
    L = amvpt_mod.hip_lib()
    s, vd, p, planes = refusal_planes(amvpt_mod)
    n_img = planes["src_image"].size
    A = Arena(planes, dict(dst_image=n_img, dst_cover=128))
    buf = torch.from_numpy(A.buf).cuda()
    base = dict(A.addresses(buf.data_ptr()), channels=3, src_views=vd, src_params=p, dst_views=vd, dst_params=p, rect=None,
                sp=amvpt_mod.SynthParams())
    rows = refusal_rows(amvpt_mod, base, n_img, 128)
    assert len(rows) == N_ROWS
    check_rows(L, L.amvpt_synth, "amvpt_synth", rows, base)
    torch.cuda.synchronize()
    assert np.array_equal(bits(buf.cpu().numpy()), bits(A.buf)), "a refused call wrote"
    assert call_with(L.amvpt_synth, base, stream=True) == 0
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    want = amvpt_mod.synth_host(planes["src_image"], planes["src_guides"], vd, p, planes["dst_guides"], vd, p)
    _assert_same((A.plane(got, "dst_image", (8, 16, 3)), A.plane(got, "dst_cover", (8, 16))), want)
    # stage 2
    fplanes = fill_planes(amvpt_mod)
    B = Arena(fplanes, dict(out=n_img, scratch=n_img, cover_out=128, cover_scratch=128))
    fbuf = torch.from_numpy(B.buf).cuda()
    q = amvpt_mod.SynthParams(fill_iterations=2)
    fbase = dict(B.addresses(fbuf.data_ptr()), channels=3, width=16, height=8, sp=q)
    for rid, change, names in fill_refusal_rows(amvpt_mod, fbase, n_img, 128):
        rc = call_fill(L.amvpt_synth_fill, dict(fbase, **change), stream=True)
        msg = L.amvpt_last_error().decode()
        assert rc == 1 and msg.startswith("amvpt_synth_fill: ") and names in msg, (rid, rc, msg)
    torch.cuda.synchronize()
    assert np.array_equal(bits(fbuf.cpu().numpy()), bits(B.buf)), "a refused call wrote"
    assert call_fill(L.amvpt_synth_fill, fbase, stream=True) == 0
    torch.cuda.synchronize()
    got = fbuf.cpu().numpy()
    want = amvpt_mod.synth_fill_host(fplanes["image"], fplanes["cover"], fplanes["guides"], q)
    _assert_same((B.plane(got, "out", (8, 16, 3)), B.plane(got, "cover_out", (8, 16))), want)
    assert (want[1] == -1).any()
    # no iteration: copies on the stream, no scratch needed
    q0 = amvpt_mod.SynthParams(fill_iterations=0)
    assert call_fill(L.amvpt_synth_fill, dict(fbase, sp=q0, scratch=None, cover_scratch=None), stream=True) == 0
    torch.cuda.synchronize()
    got = fbuf.cpu().numpy()
    assert np.array_equal(bits(B.plane(got, "out", (8, 16, 3))), bits(fplanes["image"]))
    assert np.array_equal(bits(B.plane(got, "cover_out", (8, 16))), bits(fplanes["cover"]))


# ---- 3. end to end ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def rendered(gpu_ready, amvpt_mod):
    """cbox_grid.xml as 4 x 2 views of 16 x 16 at 1 spp, rendered and developed on the device; the same XML with a 5 x 3
    grid is the target."""
    torch = _torch()
    L = amvpt_mod.hip_lib()
    box = xml_of("cbox_grid.xml")
    s = amvpt_mod.load_string(box, res=16, gx=4, gy=2, spp=1)
    d = amvpt_mod.load_string(box, res=16, gx=5, gy=3)
    sd, vd, p = s.describe(0, 10, 1)
    dev = amvpt_mod.DeviceScene(sd)
    w, h = p.film_width, p.film_height
    film = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    img = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    dev.render(vd, p, film.data_ptr())
    assert L.amvpt_develop(ctypes.c_void_p(film.data_ptr()), ctypes.c_void_p(img.data_ptr()), w, h, p.film_alpha, None) == 0
    torch.cuda.synchronize()
    return dict(src=s, dst=d, dev=dev, views=vd, params=p, image=img)


def _host_pipeline(amvpt_mod, vs, views, params):
    """The host entries on the downloaded planes of the synthesizer's last run."""
    si, sg, dg = vs.source_image.cpu().numpy(), vs.source_guides.cpu().numpy(), vs.guides.cpu().numpy()
    one = amvpt_mod.synth_host(si, sg, views, params, dg, vs.dst_views, vs.dst_params, vs.params)
    return amvpt_mod.synth_fill_host(one[0], one[1], dg, vs.params) if vs.params.fill_iterations else one


def test_synthesizer_equals_the_host_entries(amvpt_mod, rendered):
    torch = _torch()
    r = rendered
    vs = amvpt_mod.ViewSynthesizer(r["dst"])
    out, cover = vs.run(r["dev"], r["views"], r["params"], r["image"])
    torch.cuda.synchronize()
    assert out.shape == (48, 80, 3) and cover.shape == (48, 80) and vs.guide_runs == 1
    si = r["image"].cpu().numpy()
    assert np.isfinite(si).all() and si.max() > 0
    want = _host_pipeline(amvpt_mod, vs, r["views"], r["params"])
    _assert_same((out.cpu().numpy(), cover.cpu().numpy()), want, "first run")
    assert vs.holes == int((want[1] == 0).sum()) and (want[1] > 0).mean() > 0.9
    first = (out.cpu().numpy().copy(), cover.cpu().numpy().copy())
    # unchanged target views: the guide records are not computed again, and the bytes are the same
    out2, cover2 = vs.run(r["dev"], r["views"], r["params"], r["image"])
    torch.cuda.synchronize()
    assert vs.guide_runs == 1 and out2.data_ptr() != out.data_ptr()
    _assert_same((out2.cpu().numpy(), cover2.cpu().numpy()), first, "second run")
    # the source's records given by the caller: the same bytes, and no fill where fill_iterations is 0
    vs0 = amvpt_mod.ViewSynthesizer(r["dst"], amvpt_mod.SynthParams(fill_iterations=0))
    out0, cover0 = vs0.run(r["dev"], r["views"], r["params"], r["image"], src_guides=vs.source_guides)
    torch.cuda.synchronize()
    _assert_same((out0.cpu().numpy(), cover0.cpu().numpy()), _host_pipeline(amvpt_mod, vs0, r["views"], r["params"]), "no fill")
    assert not (cover0 < 0).any()
    # changed target views compute them again
    moved = amvpt_mod.load_string(xml_of("cbox_grid.xml").replace('origin="0, 0, 3.9" target="0, 0, 0"', 'origin="0.1, 0, 3.9" target="0.1, 0, 0"'),
                                  res=16, gx=5, gy=3)
    _, vd2, p2 = moved.describe(0, 0, 0)
    vs.set_views(vd2, p2)
    out3, cover3 = vs.run(r["dev"], r["views"], r["params"], r["image"])
    torch.cuda.synchronize()
    assert vs.guide_runs == 2
    _assert_same((out3.cpu().numpy(), cover3.cpu().numpy()), _host_pipeline(amvpt_mod, vs, r["views"], r["params"]), "moved targets")
    assert not np.array_equal(out3.cpu().numpy(), first[0])
    with pytest.raises(ValueError, match="contiguous float32"):
        vs.run(r["dev"], r["views"], r["params"], r["image"][:16])


def test_display_stage(amvpt_mod, rendered):
    """synth=None returns the bytes the call returned before; a ViewSynthesizer shows its dense quilt, alone and behind
    an accumulator and a denoiser."""
    import amvpt.display as D
    s, d = rendered["src"], rendered["dst"]
    size = (96, 54)
    D.display(s, size=size)
    plain = D.display(s, size=size, rerender=False)
    assert np.array_equal(plain, D.display(s, size=size, rerender=False, synth=None))
    assert np.array_equal(plain, D.display(s, size=size, rerender=False, temporal=None, synth=None))
    vs = amvpt_mod.ViewSynthesizer(d)
    _, vd, p = s.describe(0, 1, 0)
    shown = D.display(s, size=size, seed=1, synth=vs)
    want = D.interlace(D.srgb8(_host_pipeline(amvpt_mod, vs, vd, p)[0]), D.preset_for_scene(d), size)
    assert shown.shape == (54, 96, 3) and np.array_equal(shown, want)
    assert D.preset_for_scene(d).grid[:] == [5, 3] and vs.image.shape == (48, 80, 3) and vs.guide_runs == 1
    assert not np.array_equal(shown, D.display(s, size=size, seed=1))
    # behind the accumulator and the denoiser: the synthesizer's source is the filtered accumulated frame
    acc = amvpt_mod.TemporalAccumulator()
    q = amvpt_mod.DenoiseParams(iterations=2)
    for seed in (1, 2):
        shown = D.display(s, size=size, seed=seed, temporal=acc, denoise=q, synth=vs)
    assert acc.frames == 2 and vs.guide_runs == 1
    filtered = amvpt_mod.denoise_host(acc.image.cpu().numpy(), acc.guides.cpu().numpy(), q)
    assert np.array_equal(bits(vs.source_image.cpu().numpy()), bits(filtered))
    want = D.interlace(D.srgb8(_host_pipeline(amvpt_mod, vs, vd, p)[0]), D.preset_for_scene(d), size)
    assert np.array_equal(shown, want)
    with pytest.raises(ValueError, match="needs a fresh frame"):
        D.display(s, size=size, synth=vs, rerender=False)
