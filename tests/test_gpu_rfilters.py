"""The tent, Mitchell-Netravali, Catmull-Rom and Lanczos reconstruction filters on the device.

The oracle knows the Gaussian and the box filter only, but the per-lane records (ImageBlock::put's arguments) do
not depend on the filter: every render's records must equal the oracle's bit for bit (the oracle is given the same
params with the default Gaussian), and every film must equal the numpy restatement of ImageBlock::put over those
records (tests/test_rfilters.py: put_film, anchored there on the oracle's own film) with the filter's weights from
amvpt.rfilter_eval.  Tolerance: 1e-5 of the film's largest magnitude, test_gpu_parity.py's bar against float-atomic
reordering; the deterministic film is compared bit for bit (within the tolerance for Lanczos, whose sine is the
platform's)."""
import ctypes
import os

import numpy as np
import pytest

from conftest import SCENES
from test_rfilters import CBOX, CBOX_PATH, elem, filter_xml, gaussian_params, put_film, weight_fn_of

pytestmark = pytest.mark.gpu

CBOX_BATCH = os.path.join(SCENES, "cbox_batch.xml")
BASE = dict(res=24, spp=32, gx=4, gy=2, reuse=8)
TOL = 1e-5


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _bit_equal(a, b):
    return (a == b) | (np.isnan(a) & np.isnan(b))


class Frame:
    """One loaded scene with its device scene, plan and the oracle's records of every pass."""
    _records = {}   # (scene file, rgba, defines) -> records per pass: they do not depend on the filter

    def __init__(self, amvpt_mod, oracle, filt, scene=CBOX, rgba=False, **defines):
        xml = filter_xml(filt, scene)
        if rgba:
            assert xml.count('name="pixel_format" value="rgb"') == 1
            xml = xml.replace('name="pixel_format" value="rgb"', 'name="pixel_format" value="rgba"')
        self.mod = amvpt_mod
        self.scene = amvpt_mod.load_string(xml, **defines)
        self.sd, self.vd, self.p = self.scene.describe(0, 0, 0)
        self.plan = oracle.plan(self.p)
        self.dev = amvpt_mod.DeviceScene(self.sd)
        self.C = 5 if self.p.film_alpha else 4
        assert self.C == (5 if rgba else 4)
        self.radius = amvpt_mod.rfilter_eval(self.p, np.zeros(1, dtype=np.float32))[1]
        key = (scene, rgba, tuple(sorted(defines.items())))
        if key not in Frame._records and not self.p.adaptive:
            q = gaussian_params(self.p)
            Frame._records[key] = [oracle.render(self.sd, self.vd, q, threads=16, record_pass=k)[1]
                                   for k in range(self.plan["passes"])]
        self.orecs = Frame._records.get(key)

    def render(self, flags=0, record_pass=None, counters=None):
        torch = _torch()
        film = torch.zeros((self.p.film_height, self.p.film_width, self.C), dtype=torch.float32, device="cuda")
        rec = None
        if record_pass is not None:
            rec = torch.zeros((self.plan["lanes"], self.plan["group"], 8), dtype=torch.float32, device="cuda")
        self.dev.render_ex(self.vd, self.p, film.data_ptr(), flags=flags, counters=counters,
                           records_ptr=rec.data_ptr() if rec is not None else None, record_pass=record_pass or 0)
        torch.cuda.synchronize()
        return film.cpu().numpy(), (rec.cpu().numpy() if rec is not None else None)

    def restatement(self):
        """(float64-summed film, fixed-point film) of ImageBlock::put over the oracle's records."""
        coalesce_single = self.plan["spp_per_pass"] >= 4
        return put_film(self.orecs, self.plan["group"], self.p, weight_fn_of(self.mod, self.p), self.radius,
                        coalesce_single, fixed="both")

    def check_records(self):
        """Records of every pass equal the oracle's bit for bit, all lanes; returns the last record render's film."""
        film = None
        for k in range(self.plan["passes"]):
            film, rec = self.render(record_pass=k)
            eq = _bit_equal(rec, self.orecs[k])
            assert eq.all(), "pass %d: %d of %d lanes differ" % (k, (~eq.all(axis=(1, 2))).sum(), len(rec))
        return film


def _close(got, want, what):
    scale = np.abs(want).max()
    err = np.abs(got - want).max() / scale
    print("%s: max |diff| / max |film| = %.3e" % (what, err))
    assert err < TOL, "%s: film max relative difference %.3e" % (what, err)


FILM_CASES = [
    ("tent", elem("tent")),
    ("tent_r1.7", elem("tent", radius=1.7)),
    ("mitchell", elem("mitchell")),
    ("mitchell_b0_c.5", elem("mitchell", B=0.0, C=0.5)),
    ("catmullrom", elem("catmullrom")),
    ("lanczos", elem("lanczos")),
]


@pytest.mark.parametrize("filt", [c[1] for c in FILM_CASES], ids=[c[0] for c in FILM_CASES])
def test_filter_film(gpu_ready, amvpt_mod, oracle, filt):
    """Base shape (96 x 48 film, 2 passes of 16, G = 8: the smallest at which the row splat is eligible): records,
    the plain render (the row splat where the filter has one), the block-window render and the deterministic film."""
    f = Frame(amvpt_mod, oracle, filt, **BASE)
    assert (f.plan["passes"], f.plan["spp_per_pass"], f.plan["group"]) == (2, 16, 8)
    assert (f.p.film_width, f.p.film_height, f.plan["lanes"]) == (96, 48, 73728)
    want, want_fx = f.restatement()
    rec_film = f.check_records()
    _close(rec_film, want, "record render")
    _close(f.render()[0], want, "plain render")
    _close(f.render(flags=amvpt_mod.OPT_BLOCK_SPLAT)[0], want, "block splat")
    det = f.render(flags=amvpt_mod.OPT_DETERMINISTIC)[0]
    if "lanczos" in filt:
        _close(det, want_fx, "deterministic film")
    else:
        eq = _bit_equal(det, want_fx)
        assert eq.all(), "deterministic film: %d floats differ" % (~eq).sum()


PATH_CASES = [
    # k_splat_single (G = 1)
    ("mitchell_reuse1", elem("mitchell"), dict(BASE, reuse=1), dict()),
    # the stock path integrator
    ("tent_stock_path", elem("tent"), dict(res=32, spp=16), dict(scene=CBOX_PATH)),
    # spp per pass not a power of two: the block window
    ("catmullrom_spp24", elem("catmullrom"), dict(BASE, spp=24), dict()),
    # RGBAW film (C = 5)
    ("mitchell_rgba", elem("mitchell"), BASE, dict(rgba=True)),
    # crop window: offset and edge clipping (test_gpu_parity.py test_crop_window's batch case)
    ("tent_crop", elem("tent"), dict(res=32, width=128, spp=16, crop_w=64, crop_h=16, crop_x=32, crop_y=8),
     dict(scene=CBOX_BATCH)),
    # footprints of 7 and 6 cells, wider than the window path's 5: direct atomics
    ("tent_r2.6", elem("tent", radius=2.6), BASE, dict()),
    ("lanczos_3", elem("lanczos", lobes=3), BASE, dict()),
    # 3- and 2-cell footprints
    ("tent_r0.75", elem("tent", radius=0.75), BASE, dict()),
]


@pytest.mark.parametrize("filt,defines,kw", [c[1:] for c in PATH_CASES], ids=[c[0] for c in PATH_CASES])
def test_filter_paths(gpu_ready, amvpt_mod, oracle, filt, defines, kw):
    """The smallest variations that reach the other splat kernels and the clipping code: bit-identical records and
    the film against the restatement."""
    f = Frame(amvpt_mod, oracle, filt, **kw, **defines)
    want, _ = f.restatement()
    _close(f.check_records(), want, "record render")
    _close(f.render()[0], want, "plain render")


def test_filter_paths_adaptive_fill(gpu_ready, amvpt_mod, oracle):
    """Mitchell with adaptive = 2 (k_splat_adapt).  The fill's puts are not in the records, so the plain film is
    compared with the block-splat film and the deterministic film; all three re-trace the same lanes."""
    f = Frame(amvpt_mod, oracle, elem("mitchell"), **dict(BASE, adaptive=2))
    films, lanes = [], []
    for flags in (0, amvpt_mod.OPT_BLOCK_SPLAT, amvpt_mod.OPT_DETERMINISTIC):
        cnt = amvpt_mod.Counters()
        films.append(f.render(flags=flags, counters=cnt)[0])
        lanes.append(cnt.adaptive_lanes)
    assert lanes[0] > 0 and lanes[0] == lanes[1] == lanes[2]
    _close(films[0], films[2], "plain vs deterministic")
    _close(films[1], films[2], "block splat vs deterministic")
    _close(films[0], films[1], "plain vs block splat")


def test_filter_film_window(gpu_ready, amvpt_mod, oracle):
    """Mitchell through amvpt_render_ex into the left half of the quilt with an overflow list.  Every lane of a group
    of 8 splats into all eight tiles, so the lanes are those of the first tile only (a rectangle lane set), which
    keeps the overflow list small: window plus overflow, summed by amvpt_film_accumulate, equals the whole-quilt
    render of the same lanes (its left half plus what spills to the right)."""
    torch = _torch()
    f = Frame(amvpt_mod, oracle, elem("mitchell"), **BASE)
    W, H = f.p.film_width, f.p.film_height
    lanes = amvpt_mod.LaneSet(0, 0, 0, 0, BASE["res"], BASE["res"])
    whole = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    f.dev.render_ex(f.vd, f.p, whole.data_ptr(), lanes=lanes)
    cap = 1 << 21
    win = torch.zeros((H, W // 2, 4), dtype=torch.float32, device="cuda")
    ov = torch.zeros(4 * (cap + 1), dtype=torch.int32, device="cuda")
    cnt = amvpt_mod.Counters()
    f.dev.render_ex(f.vd, f.p, win.data_ptr(), lanes=lanes, window=(0, 0, W // 2, H), overflow_ptr=ov.data_ptr(),
                    overflow_capacity=cap, counters=cnt)
    torch.cuda.synchronize()
    n = int(ov[:2].view(torch.int64)[0].item())
    print("overflow cells:", n)
    assert 0 < n <= cap and cnt.film_overflow == n
    quilt = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    L = amvpt_mod.hip_lib()
    rc = L.amvpt_film_accumulate(ctypes.c_void_p(quilt.data_ptr()), W, H, 4, ctypes.c_void_p(win.data_ptr()), 0, 0,
                                 W // 2, H, ctypes.c_void_p(ov.data_ptr() + 16), ctypes.c_uint64(n), None)
    assert rc == 0, L.amvpt_last_error()
    torch.cuda.synchronize()
    whole = whole.cpu().numpy()
    assert np.abs(whole[:, W // 2:]).max() > 0   # the right half is reached: the spill is not empty
    _close(quilt.cpu().numpy(), whole, "window + overflow")


def test_block_splat_flag_default_gaussian(gpu_ready, amvpt_mod, oracle):
    """AMVPT_OPT_BLOCK_SPLAT on the path that existed before the flag: the default Gaussian's row splat against
    its block window; records bit-identical to the oracle."""
    f = Frame(amvpt_mod, oracle, '<rfilter type="gaussian"/>', **BASE)
    assert f.p.rfilter == 1
    plain = f.render()[0]
    block = f.render(flags=amvpt_mod.OPT_BLOCK_SPLAT)[0]
    _close(block, plain, "block splat vs row splat")
    for k in range(f.plan["passes"]):
        _, rec = f.render(flags=amvpt_mod.OPT_BLOCK_SPLAT, record_pass=k)
        assert _bit_equal(rec, f.orecs[k]).all()
    want, _ = f.restatement()
    _close(block, want, "block splat vs restatement")
    _close(plain, want, "row splat vs restatement")
