"""The row splat's fixed-pitch wave windows and their static flush against the run-time geometry and the generic flush.

A wave window of at most 16 columns takes the fixed-pitch layout (rows 16 cells apart, planes 100 apart) and, when it
lies inside the film window, the unrolled flush (wave_flush_fixed); AMVPT_OPT_GENERIC_FLUSH keeps the run-time
geometry and wave_flush's loop everywhere, so one build renders the same frame both ways.  Every case holds both
renders to the bar of test_gpu_parity.py: records bit-identical to the CPU oracle's, the float film within 1e-5 of
the oracle film's scale (float-atomic reordering) -- against the oracle and against each other -- and the splat
counters equal.  The shapes are the smallest that reach each path: the bench's kernel instance, windows clipped at
the borders of the quilt and of the tiles, a partial film window with its overflow list, windows wider than 16
columns (asserted from the oracle's records), a 5-channel film and a second filter's row instance.
"""
import os

import numpy as np
import pytest

from conftest import SCENES
from test_rfilters import elem

pytestmark = pytest.mark.gpu

CBOX = os.path.join(SCENES, "cbox_grid.xml")
CONE = os.path.join(SCENES, "cbox_cone.xml")
TOL = 1e-5
F32 = np.float32
COUNTERS = ("view_splats", "splat_fallback", "nonfinite_samples", "negative_samples")


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _bit_equal(a, b):
    return (a == b) | (np.isnan(a) & np.isnan(b))


def _close(got, want, scale, what):
    err = np.abs(got - want).max() / scale
    print("%s: max |diff| / max |oracle film| = %.3e" % (what, err))
    assert err < TOL, "%s: film max relative difference %.3e" % (what, err)


class Shot:
    """One single-pass scene with its device scene and the oracle's film and records (computed once per key)."""
    _oracle = {}

    def __init__(self, amvpt_mod, oracle, key, scene_file, rgba=False, view=None, **defines):
        xml = open(scene_file).read()
        if rgba:
            assert xml.count('name="pixel_format" value="rgb"') == 1
            xml = xml.replace('name="pixel_format" value="rgb"', 'name="pixel_format" value="rgba"')
        if view is not None:   # per-view width x height instead of res x res
            for axis, v in zip(("width", "height"), view):
                old = '<integer name="%s" value="$res"/>' % axis
                assert xml.count(old) == 1
                xml = xml.replace(old, '<integer name="%s" value="%d"/>' % (axis, v))
        self.mod = amvpt_mod
        self.scene = amvpt_mod.load_string(xml, **defines)
        self.sd, self.vd, self.p = self.scene.describe(0, 0, 0)
        self.plan = oracle.plan(self.p)
        assert self.plan["passes"] == 1 and self.plan["spp_per_pass"] == 16
        self.C = 5 if self.p.film_alpha else 4
        assert self.C == (5 if rgba else 4)
        self.dev = amvpt_mod.DeviceScene(self.sd)
        if key not in Shot._oracle:
            ofilm, orec, _ = oracle.render(self.sd, self.vd, self.p, threads=16, record_pass=0)
            Shot._oracle[key] = (ofilm, orec)
        self.ofilm, self.orec = Shot._oracle[key]
        self.scale = np.abs(self.ofilm).max()

    def render(self, flags=0, records=False, **kw):
        """(film, records or None, counters) of one amvpt_render_ex; kw: lanes / window / overflow arguments."""
        torch = _torch()
        shape = (self.p.film_height, self.p.film_width) if "window" not in kw else (kw["window"][3], kw["window"][2])
        film = torch.zeros(shape + (self.C,), dtype=torch.float32, device="cuda")
        rec = None
        if records:
            rec = torch.zeros((self.plan["lanes"], self.plan["group"], 8), dtype=torch.float32, device="cuda")
        cnt = self.mod.Counters()
        self.dev.render_ex(self.vd, self.p, film.data_ptr(), flags=flags, counters=cnt,
                           records_ptr=rec.data_ptr() if records else None, **kw)
        torch.cuda.synchronize()
        return film.cpu().numpy(), (rec.cpu().numpy() if records else None), cnt

    def parity(self):
        """Both flushes: plain renders (the instance without the record path) and record renders."""
        films = {}
        for name, flags in (("static", 0), ("generic", self.mod.OPT_GENERIC_FLUSH)):
            film, _, cnt = self.render(flags)
            _close(film, self.ofilm, self.scale, name + " flush vs oracle")
            rfilm, rec, rcnt = self.render(flags, records=True)
            eq = _bit_equal(rec, self.orec)
            assert eq.all(), "%s flush: %d of %d lane records differ" % (name, (~eq.all(axis=(1, 2))).sum(), len(rec))
            _close(rfilm, self.ofilm, self.scale, name + " flush, record render, vs oracle")
            films[name] = (film, cnt)
        _close(films["static"][0], films["generic"][0], self.scale, "static vs generic flush")
        for c in COUNTERS:
            a, b = getattr(films["static"][1], c), getattr(films["generic"][1], c)
            print("%s: %d / %d" % (c, a, b))
            assert a == b, "%s differs between the two flushes: %d / %d" % (c, a, b)
        assert films["static"][1].view_splats > 0
        return films


def wave_widths(rec, film_width, radius=2.0):
    """Columns of the wave window of every (wave, reprojected view slot) from the oracle's records: the union of the
    valid lanes' footprints as ImageBlock::put's non-coalesced method cuts them (imageblock.cpp:265-427; the default
    Gaussian's radius 2: 4 cells), a wave being 64 consecutive lanes (4 pixels x 16 samples).  0: no valid lane."""
    n, G, _ = rec.shape
    assert n % 64 == 0
    valid = rec[:, 1:, 7] != 0
    pfx = rec[:, 1:, 0].astype(F32) - F32(0.5)
    p0 = np.maximum(np.ceil(pfx - F32(radius)), 0).astype(np.int64)
    p1 = np.minimum(np.floor(pfx + F32(radius)), film_width - 1).astype(np.int64)
    ok = valid & (p0 <= p1)
    nx = np.minimum(p1 - p0 + 1, int(np.ceil(2 * radius)))
    lo = np.where(ok, p0, 1 << 30).reshape(n // 64, 64, G - 1).min(axis=1)
    hi = np.where(ok, p0 + nx, -(1 << 30)).reshape(n // 64, 64, G - 1).max(axis=1)
    has = ok.reshape(n // 64, 64, G - 1).any(axis=1)
    return np.where(has, hi - lo, 0), has


def test_bench_instance(gpu_ready, amvpt_mod, oracle):
    """Config M's kernel instance (G = 8, all-diffuse, whole-quilt film) at 4 x 2 views of 32 x 32."""
    s = Shot(amvpt_mod, oracle, "m", CBOX, res=32, spp=16, gx=4, gy=2, reuse=8, sa_mis="true")
    assert s.plan["group"] == 8 and (s.p.film_width, s.p.film_height) == (128, 64)
    ww, has = wave_widths(s.orec, s.p.film_width)
    assert (ww[has] <= 16).mean() > 0.9   # the fixed-pitch window is this frame's common case
    s.parity()


def test_windows_at_the_film_edges(gpu_ready, amvpt_mod, oracle):
    """Views of 20 x 12 px on a 2 x 2 grid, G = 4: the width is no multiple of 16 and every tile border is at most
    12 px from a pixel, so windows are clipped at all four borders of the quilt and of each tile."""
    s = Shot(amvpt_mod, oracle, "edges", CBOX, view=(20, 12), spp=16, gx=2, gy=2, reuse=4)
    assert s.plan["group"] == 4 and (s.p.film_width, s.p.film_height) == (40, 24)
    s.parity()


@pytest.mark.parametrize("border", [True, False], ids=["tiles_plus_border", "tiles_only"])
def test_partial_film_window(gpu_ready, amvpt_mod, oracle, border):
    """The view-group partition of two ranks on one device: each rank renders its tile rectangle's lanes into the film
    window of that rectangle plus the 4-px filter border, with an overflow list; the windows and lists, summed, equal
    the whole-frame render and the oracle's film.  tiles_only drops the border, so the footprints at the rectangle's
    edge leave the window: those wave windows take the generic flush and fill the overflow list."""
    import amvpt.dist as adist
    torch = _torch()
    s = Shot(amvpt_mod, oracle, "groups", CBOX, res=24, spp=16, gx=4, gy=2, reuse=4)
    groups = adist.view_group_partition(s.p, s.plan["group"], 2)
    assert groups is not None and len(groups) == 2
    whole = s.render()[0]
    _close(whole, s.ofilm, s.scale, "whole frame vs oracle")
    cap = 1 << 18
    sums = {}
    for name, flags in (("static", 0), ("generic", amvpt_mod.OPT_GENERIC_FLUSH)):
        quilt = torch.zeros((s.p.film_height, s.p.film_width, 4), dtype=torch.float32, device="cuda")
        spilled, tot = 0, dict.fromkeys(COUNTERS, 0)
        for rect, win in groups:
            if not border:
                win = rect
            assert (win[2], win[3]) != (s.p.film_width, s.p.film_height)   # a partial window
            ov = torch.zeros(4 * (cap + 1), dtype=torch.int32, device="cuda")
            film, _, cnt = s.render(flags, lanes=amvpt_mod.LaneSet(0, 0, *rect), window=win, overflow_ptr=ov.data_ptr(),
                                    overflow_capacity=cap)
            idx, val = adist.overflow_entries(ov)
            assert cnt.film_overflow == idx.numel()
            spilled += idx.numel()
            x0, y0, w, h = win
            quilt[y0:y0 + h, x0:x0 + w] += torch.from_numpy(film).cuda()
            quilt.view(-1).index_add_(0, idx, val)
            for c in COUNTERS:
                tot[c] += getattr(cnt, c)
        print("%s flush: %d overflow entries" % (name, spilled))
        assert border or spilled > 0
        sums[name] = (quilt.cpu().numpy(), tot, spilled)
        _close(sums[name][0], s.ofilm, s.scale, name + " flush, gathered windows vs oracle")
        _close(sums[name][0], whole, s.scale, name + " flush, gathered windows vs whole frame")
    _close(sums["static"][0], sums["generic"][0], s.scale, "static vs generic flush")
    assert sums["static"][1] == sums["generic"][1] and sums["static"][2] == sums["generic"][2]


WIDE = dict(res=48, spp=16, cone=100)


def test_windows_wider_than_16_columns(gpu_ready, amvpt_mod, oracle):
    """Strong parallax (the cone layout opened to WIDE's angle): the four pixels of a wave straddle depth edges and
    reproject far apart, so their window is wider than the fixed-pitch layout's 16 columns and keeps the run-time
    geometry.  Asserted from the oracle's records, so the case cannot pass vacuously."""
    s = Shot(amvpt_mod, oracle, "wide", CONE, **WIDE)
    assert s.plan["group"] == 8
    ww, has = wave_widths(s.orec, s.p.film_width)
    frac = (ww > 16).mean()   # of every (wave, reprojected view) pair, those without a valid lane included
    print("(wave, view) pairs wider than 16 columns: %.4f of %d (%d with a valid lane)" % (frac, ww.size, has.sum()))
    assert frac >= 0.01
    s.parity()


def test_rgba_film(gpu_ready, amvpt_mod, oracle):
    """A 5-channel (RGBAW) film, 2 x 2 views of 16 x 16: no row splat, the block window with its own flush."""
    s = Shot(amvpt_mod, oracle, "rgba", CBOX, rgba=True, res=16, spp=16, gx=2, gy=2, reuse=4)
    s.parity()


def test_tent_row_instance(gpu_ready, amvpt_mod, oracle):
    """The tent filter's row instance (a second kF).  The oracle knows the Gaussian and the box only: the records
    are its own (they do not depend on the filter) and the film is test_rfilters.put_film's restatement of
    ImageBlock::put over them, as in test_gpu_rfilters.py."""
    from test_gpu_rfilters import BASE, Frame
    f = Frame(amvpt_mod, oracle, elem("tent"), **BASE)
    want, _ = f.restatement()
    scale = np.abs(want).max()
    _close(f.check_records(), want, scale, "record render vs restatement")
    films, cnts = [], []
    for flags in (0, amvpt_mod.OPT_GENERIC_FLUSH):
        cnt = amvpt_mod.Counters()
        films.append(f.render(flags=flags, counters=cnt)[0])
        cnts.append([getattr(cnt, c) for c in COUNTERS])
        _close(films[-1], want, scale, "flags %d vs restatement" % flags)
    _close(films[0], films[1], scale, "static vs generic flush")
    assert cnts[0] == cnts[1] and cnts[0][0] > 0
